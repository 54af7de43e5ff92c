"""Per-point labels (pwpp_set_labels) and the cloud-order lists (PWPP_ORDER_CLOUD) on a real MI355X, against the
fixed-point oracle and the golden masks of the reference: every path that writes index lists labels its frames, cloud
order returns both lists in ascending cloud index and is byte-identical from run to run, and neither disturbs the
other output orders."""
import ctypes

import numpy as np
import pytest

import oracle_lib as ol
import pwpp_hip
import pwpp_synth
from test_gpu_inputs import Placed, encode, expected_array, submit
from test_gpu_parity import apply_variant, assert_frame_equal, to_oracle_params

pytestmark = pytest.mark.gpu

G, NG, UN = pwpp_hip.LABEL_GROUND, pwpp_hip.LABEL_NONGROUND, pwpp_hip.LABEL_UNCLASSIFIED
TINY = np.finfo(np.float32).tiny


@pytest.fixture(scope="module")
def oracle(oracle_built):
    return oracle_built.restatement()


def expected_labels(n, ground, nonground):
    lab = np.full(n, UN, np.uint8)
    lab[np.asarray(nonground, np.int64)] = NG
    lab[np.asarray(ground, np.int64)] = G
    return lab


def check_labels(h, frame, n, ref=None, cloud=False):
    """The frame's labels against the handle's own lists, the oracle's sets and the count identities; cloud order: sorted lists."""
    lab = h.labels(frame)
    assert lab.dtype == np.uint8 and lab.shape == (n,)
    g, ng = h.ground_indices(frame), h.nonground_indices(frame)
    assert np.array_equal(lab, expected_labels(n, g, ng)), "labels disagree with the handle's own lists"
    c = h.all_counts()[frame]
    assert (int((lab == G).sum()), int((lab == NG).sum()), int((lab == UN).sum())) == (c[0], c[1], c[5])
    if ref is not None:
        assert np.array_equal(lab, expected_labels(n, ref.ground_idx, ref.nonground_idx)), "labels disagree with the oracle"
    if cloud:
        assert np.all(np.diff(g) > 0) and np.all(np.diff(ng) > 0), "cloud order: lists not ascending"
        if ref is not None:
            assert np.array_equal(g, np.sort(ref.ground_idx)) and np.array_equal(ng, np.sort(ref.nonground_idx))
    return lab


def check_batch(h, frames, refs, cloud=False):
    for i, c in enumerate(frames):
        check_labels(h, i, c.shape[0], refs[i] if refs is not None else None, cloud)


def lists_of(h, frames):
    return [(h.ground_indices(i).tobytes(), h.nonground_indices(i).tobytes()) for i in range(frames)]


def test_kitti_labels_fresh_and_stateful(kitti, oracle, golden):
    h = pwpp_hip.Handle()
    h.set_labels(True)
    h.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    for k, pts in enumerate(kitti):
        lab = check_labels(h, k, pts.shape[0], ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts))
        assert np.array_equal(np.packbits(lab == G), golden["f32/fresh/%d/ground_mask" % k])
        assert_frame_equal(h, k, ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts), pts.shape[0])
    s = pwpp_hip.Handle()
    s.set_labels(True)
    est = ol.Estimator(oracle, arith=ol.ARITH_FXP)
    for k, pts in enumerate(kitti):
        s.estimate_ground(pts)
        lab = check_labels(s, 0, pts.shape[0], est.run(pts))
        assert np.array_equal(np.packbits(lab == G), golden["f32/seq/%d/ground_mask" % k])


def test_labels_getters_need_a_call_with_labels(kitti):
    h = pwpp_hip.Handle()
    with pytest.raises(pwpp_hip.PwppError):
        h.labels(0)  # no call yet
    h.estimate_ground_batch(kitti[:2], mode=pwpp_hip.MODE_FRESH)
    for get in (lambda: h.labels(0), lambda: h.all_labels(), lambda: h.device_labels()):
        with pytest.raises(pwpp_hip.PwppError, match="without labels"):
            get()
    h.set_labels(True)
    h.estimate_ground_batch(kitti[:2], mode=pwpp_hip.MODE_FRESH)
    assert h.labels(1).shape == (kitti[1].shape[0],)
    with pytest.raises(pwpp_hip.PwppError):
        h.labels(2)  # out of range


def test_cloud_order_lists_getters_and_views(kitti, oracle):
    h = pwpp_hip.Handle()
    h.set_order(pwpp_hip.ORDER_CLOUD)
    h.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(p) for p in kitti]
    check_batch(h, kitti, refs, cloud=True)
    allidx, base, counts = h.all_indices()
    labs, lbase = h.all_labels()
    assert np.array_equal(base, lbase)
    for k, pts in enumerate(kitti):
        g, ng = h.ground_indices(k), h.nonground_indices(k)
        assert np.array_equal(h.ground(k), pts[g, :3]) and np.array_equal(h.nonground(k), pts[ng, :3])
        seg = allidx[base[k]:base[k + 1]]
        assert np.array_equal(seg[:counts[k, 0]], g) and np.array_equal(seg[counts[k, 0]:counts[k, 0] + counts[k, 1]], ng)
        assert np.array_equal(labs[base[k]:base[k + 1]], h.labels(k))
    dev = hip_copy(h.device_view().indices, allidx.nbytes)
    assert np.array_equal(dev.view(np.int32), allidx)
    first = lists_of(h, 6)
    h.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    assert lists_of(h, 6) == first, "cloud order is not byte-identical from run to run"


def _hip():
    """The HIP runtime this process already uses (the one libpwpp_hip.so is bound to), for raw device-to-host copies."""
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64.so" in ln})
    assert paths, "no HIP runtime mapped"
    lib = ctypes.CDLL(paths[0])
    lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    lib.hipDeviceSynchronize.argtypes = []
    return lib


def hip_copy(ptr, nbytes):
    out = np.empty(max(nbytes, 1), np.uint8)
    hip = _hip()
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemcpy(out.ctypes.data, ptr, nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out[:nbytes]


def test_device_labels_pointer(kitti):
    h = pwpp_hip.Handle()
    h.set_labels(True)
    h.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    labs, base = h.all_labels()
    ptr = h.device_labels()
    assert ptr != 0
    assert np.array_equal(hip_copy(ptr, int(base[-1])), labs)
    out = np.zeros(int(base[-1]) + 5, np.uint8)
    labs2, _ = h.all_labels(out)
    assert np.array_equal(labs2, labs) and not out[int(base[-1]):].any()


def test_cloud_order_is_deterministic_on_the_overlap_schedule_and_through_a_pipe(kitti, oracle):
    """128+ frames take the overlap schedule (cloud order does not force the single-stream one): two runs are byte-identical
    without sorting; a pipe of depth 2 too."""
    F = 132
    frames = [kitti[i % 6] for i in range(F)]
    refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(p) for p in kitti]
    h = pwpp_hip.Handle()
    h.set_order(pwpp_hip.ORDER_CLOUD)
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    first = lists_of(h, F)
    for i in (0, 1, 63, 64, 65, 66, 67, 127, 128, F - 1):
        check_labels(h, i, frames[i].shape[0], refs[i % 6], cloud=True)
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert lists_of(h, F) == first
    import torch
    dev = torch.device("cuda", 0)
    tens = [torch.from_numpy(f).to(dev) for f in kitti]
    torch.cuda.synchronize()
    ptrs = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in tens])
    ns = (ctypes.c_int32 * 6)(*[f.shape[0] for f in kitti])
    pipe = pwpp_hip.Pipe(depth=2)
    try:
        for i in range(2):
            pipe.handle(i).set_order(pwpp_hip.ORDER_CLOUD)
        seen = []
        for rep in range(4):
            hv = pipe.submit_device_batch((ptrs, ns, 6))
            hv.synchronize()
            seen.append(lists_of(hv, 6))
            check_batch(hv, kitti, refs, cloud=True)
        assert seen[0] == seen[1] == seen[2] == seen[3]
        pipe.drain()
    finally:
        pipe.close()


def _wedge(src, rng, lo):
    w = src.copy()
    sel = rng.random(w.shape[0]) < 0.7
    r = np.hypot(w[sel, 0], w[sel, 1])
    a = rng.uniform(lo, lo + 0.17, sel.sum())
    w[sel, 0] = (r * np.cos(a)).astype(np.float32)
    w[sel, 1] = (r * np.sin(a)).astype(np.float32)
    return w


@pytest.mark.parametrize("order", [pwpp_hip.ORDER_SCATTER, pwpp_hip.ORDER_CLOUD])
def test_every_path_labels_its_frames(kitti, oracle, order):
    """Labels on (and cloud order) down every path that writes lists: a single frame, fresh batches, forced two-pass binning, the
    in-place and the no-arena redo after a segment overflow, the whole-batch redo, the overflow arena, stateful streams with and
    without K5 split, profiling, and the serial fix-up of frames whose patches start from the plane fitted before them."""
    cloud = order == pwpp_hip.ORDER_CLOUD
    est = lambda p, op=None: ol.Estimator(oracle, op, arith=ol.ARITH_FXP).run(p)
    refs = [est(p) for p in kitti]

    def handle(**opts):
        h = pwpp_hip.Handle(opts.pop("params", None))
        h.set_labels(True)
        h.set_order(order)
        for k, v in opts.items():
            h.set_option(k, v)
        return h

    # single frame; fresh batch; two-pass; profiling
    h = handle()
    h.estimate_ground(kitti[3])
    check_labels(h, 0, kitti[3].shape[0], refs[3], cloud)
    for opts in (dict(), dict(one_pass=0)):
        h = handle(**opts)
        h.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
        check_batch(h, kitti, refs, cloud)
    h = handle()
    h.set_profiling(True)
    h.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    check_batch(h, kitti, refs, cloud)
    prof = h.kernel_profile()
    assert prof["k_emit"][1] == 1 and prof["k_emit"][0] > 0
    # overflow redo: the wedge cloud in a batch sized for KITTI (in place), without the arena, and the whole batch
    rng = np.random.default_rng(5)
    wedge = _wedge(kitti[0], rng, 0.1)
    odd = [wedge, kitti[1], kitti[2], wedge, kitti[3]]
    rodd = [est(p) for p in odd]
    for opts in (dict(), dict(debug_flags=2048), dict(redo_whole_batch=1)):
        h = handle(**opts)
        h.estimate_ground_batch([kitti[i % 6] for i in range(7)], mode=pwpp_hip.MODE_FRESH)
        h.estimate_ground_batch(odd, mode=pwpp_hip.MODE_FRESH)
        assert h.redo_stats()[1] >= 1
        check_batch(h, odd, rodd, cloud)
    # overflow arena: one sector of a frame of 72 40 % denser than the handle has seen -- its parts move into the arena on the
    # device (the case of test_overflow_arena_moves_parts_on_the_device)
    arng = np.random.default_rng(11)
    a = np.arctan2(kitti[0][:, 1], kitti[0][:, 0])
    sel = np.where((a > 0.3) & (a < 0.6))[0]
    extra = kitti[0][arng.choice(sel, int(len(sel) * 0.4), replace=True)].copy()
    extra[:, :3] += arng.normal(0.0, 0.004, (len(extra), 3)).astype(np.float32)
    dense = np.ascontiguousarray(np.concatenate([kitti[0], extra]).astype(np.float32))
    base = [kitti[i % 6] for i in range(72)]
    h = handle()
    h.estimate_ground_batch(base, mode=pwpp_hip.MODE_FRESH)
    odd2 = list(base)
    odd2[10] = dense
    h.estimate_ground_batch(odd2, mode=pwpp_hip.MODE_FRESH)
    assert h.arena_stats()[0] >= 1 and h.redo_stats()[1] == 0
    for i in (0, 9, 10, 11, 71):
        check_labels(h, i, odd2[i].shape[0], est(dense) if i == 10 else refs[i % 6], cloud)
    # stateful streams in lock step, K5 in one and in two launches
    for split in ("0", "1"):
        h = handle(split_k5=split)
        h.set_num_streams(3)
        ests = [ol.Estimator(oracle, arith=ol.ARITH_FXP) for _ in range(3)]
        for t in range(3):
            fr = [kitti[(s + t) % 6] for s in range(3)]
            h.estimate_ground_batch(fr, mode=pwpp_hip.MODE_STREAMS)
            check_batch(h, fr, [ests[s].run(fr[s]) for s in range(3)], cloud)
    # fix-up frames (k_fit_fixup, stages 2 | 4 | 8)
    frng = np.random.default_rng(5)

    def spoil(c, k):
        c = c.copy()
        c[frng.choice(c.shape[0], k, replace=False), 2] = -np.inf
        lone = np.array([[70.0, 30.0 + i, 1e30, 0.5] for i in range(3)] + [[3.5, -1.0, 3e38, 0.5]], np.float32)
        return np.ascontiguousarray(np.concatenate([c, lone]))

    spoiled = [spoil(kitti[0], 40), kitti[1], spoil(kitti[5], 3)]
    for variant in (dict(), dict(num_min_pts=0)):
        p = apply_variant(pwpp_hip.default_params(), variant)
        op = to_oracle_params(p)
        h = handle(params=p)
        h.estimate_ground_batch(spoiled, mode=pwpp_hip.MODE_FRESH)
        assert h.fixed_up_frames() >= 1
        check_batch(h, spoiled, [est(c, op) for c in spoiled], cloud)


@pytest.mark.parametrize("mem", ["host", "pinned_slab", "device"])
@pytest.mark.parametrize("layout", ["row4", "col3", "fields48", "fields_noi"])
def test_labels_for_every_layout_and_memory_kind(kitti, oracle, layout, mem):
    names = [kitti[0], kitti[4], pwpp_synth.add_edge_cases(pwpp_synth.make_cloud(23, beams=32, azimuth_steps=900), 23)]
    exps = [expected_array(p, layout) for p in names]
    refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(e) for e in exps]
    for order in (pwpp_hip.ORDER_SCATTER, pwpp_hip.ORDER_CLOUD):
        h = pwpp_hip.Handle()
        h.set_labels(True)
        h.set_order(order)
        placed = Placed([encode(e, layout, 7 + k) for k, e in enumerate(exps)], mem)
        try:
            submit(h, placed, layout, [len(e) for e in exps], pwpp_hip.MODE_FRESH)
            for k, e in enumerate(exps):
                check_labels(h, k, len(e), refs[k], order == pwpp_hip.ORDER_CLOUD)
                if order == pwpp_hip.ORDER_CLOUD:
                    assert np.array_equal(h.ground(k), e[h.ground_indices(k), :3])
        finally:
            placed.free()


def test_unclassified_rnr_and_out_of_range_points(kitti, oracle):
    """z == FLT_MIN: UNCLASSIFIED and in neither list; a second batch with such points elsewhere leaves nothing of the first;
    RNR hits and points beyond max_range / inside min_range are NONGROUND."""
    rng = np.random.default_rng(3)
    a, b = kitti[2].copy(), kitti[2].copy()
    pa = rng.choice(a.shape[0], 300, replace=False)
    pb = rng.choice(b.shape[0], 500, replace=False)
    a[pa, 2] = TINY
    b[pb, 2] = TINY
    for order in (pwpp_hip.ORDER_SCATTER, pwpp_hip.ORDER_CLOUD):
        h = pwpp_hip.Handle()
        h.set_labels(True)
        h.set_order(order)
        for batch in ([a, kitti[1]], [b, kitti[1]], [kitti[2], kitti[1]]):
            h.estimate_ground_batch(batch, mode=pwpp_hip.MODE_FRESH)
            refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(p) for p in batch]
            check_batch(h, batch, refs, order == pwpp_hip.ORDER_CLOUD)
            lab = h.labels(0)
            drop = np.flatnonzero(batch[0][:, 2] == TINY)
            assert np.array_equal(np.flatnonzero(lab == UN), drop)
            assert not np.isin(drop, h.ground_indices(0)).any() and not np.isin(drop, h.nonground_indices(0)).any()
            assert h.all_counts()[0, 5] == len(drop)
    # RNR and range: every such point is non-ground
    c = kitti[0].copy()
    far = rng.choice(c.shape[0], 200, replace=False)
    c[far, :2] *= 200.0
    near = rng.choice(np.setdiff1d(np.arange(c.shape[0]), far), 200, replace=False)
    c[near, :2] *= 0.01
    h = pwpp_hip.Handle()
    h.set_labels(True)
    h.estimate_ground(c)
    ref = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(c)
    lab = check_labels(h, 0, c.shape[0], ref)
    assert np.all(lab[far] == NG) and np.all(lab[near] == NG)
    assert h.all_counts()[0, 4] > 0  # out of range


def test_modes_do_not_disturb_each_other(kitti, oracle):
    refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(p) for p in kitti]
    # reference order: byte-equal lists with and without labels
    plain, lab = pwpp_hip.Handle(), pwpp_hip.Handle()
    for h in (plain, lab):
        h.set_output_order(True)
    lab.set_labels(True)
    for h in (plain, lab):
        h.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    assert lists_of(plain, 6) == lists_of(lab, 6)
    check_batch(lab, kitti, refs)
    # scatter order with labels: the same sets
    s = pwpp_hip.Handle()
    s.set_labels(True)
    s.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    for k in range(6):
        assert_frame_equal(s, k, refs[k], kitti[k].shape[0])
    # one handle through scatter -> cloud -> reference -> cloud
    h = pwpp_hip.Handle()
    for order in (pwpp_hip.ORDER_SCATTER, pwpp_hip.ORDER_CLOUD, pwpp_hip.ORDER_REFERENCE, pwpp_hip.ORDER_CLOUD):
        h.set_order(order)
        h.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
        if order == pwpp_hip.ORDER_REFERENCE:
            assert lists_of(h, 6) == lists_of(plain, 6)
            with pytest.raises(pwpp_hip.PwppError):
                h.labels(0)
        elif order == pwpp_hip.ORDER_CLOUD:
            check_batch(h, kitti, refs, cloud=True)
        else:
            for k in range(6):
                assert_frame_equal(h, k, refs[k], kitti[k].shape[0])
    with pytest.raises(pwpp_hip.PwppError):
        h.set_order(7)
    # the workspace grows only with labels, and trim gives it back
    w = pwpp_hip.Handle()
    w.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    off = w.workspace_bytes()
    w.set_labels(True)
    w.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    on = w.workspace_bytes()
    assert on > off
    w.set_order(pwpp_hip.ORDER_CLOUD)
    w.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    assert w.workspace_bytes() > on
    w.trim_workspace()
    assert w.workspace_bytes() < off


def test_pybind_module_labels_and_cloud_order(kitti, golden):
    import pypatchworkpp
    params = pypatchworkpp.Parameters()
    pp = pypatchworkpp.patchworkpp(params)
    pp.setLabels(True)
    for k, pts in enumerate(kitti):
        pp.estimateGround(pts)
        lab = pp.getLabels()
        assert lab.dtype == np.uint8 and lab.shape == (pts.shape[0],)
        assert np.array_equal(np.packbits(lab == G), golden["f32/seq/%d/ground_mask" % k])
    c = pypatchworkpp.patchworkpp(params)
    c.setCloudOrder(True)
    c.estimateGround(kitti[0])
    g, ng = c.getGroundIndices(), c.getNongroundIndices()
    assert np.all(np.diff(g) > 0) and np.all(np.diff(ng) > 0)
    lab = c.getLabels()
    assert np.array_equal(np.flatnonzero(lab == G), g) and np.array_equal(np.flatnonzero(lab == NG), ng)
    assert np.array_equal(c.getGround(), kitti[0][g, :3])
    d = pypatchworkpp.patchworkpp(params)  # (a first frame again: the object is stateful)
    d.setCloudOrder(True)
    d.setCloudOrder(False)
    d.estimateGround(kitti[0])
    assert np.array_equal(np.sort(d.getGroundIndices()), g)
    with pytest.raises(RuntimeError):
        d.getLabels()  # scatter order, labels off
