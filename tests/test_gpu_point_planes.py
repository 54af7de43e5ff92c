"""Per-point patch rows and plane distances (pwpp_set_point_planes) on a real MI355X, against the fixed-point oracle: a point's
row is the oracle record of the bin the reference's pc2czm puts it in (restated in numpy, with RNR and the FLT_MIN marker), its
distance is the reference's calc_point_to_plane_d against that record's plane, bit for bit.  Every path that writes index lists
writes them, the outputs are deterministic, and turning the feature on changes no other output."""
import ctypes

import numpy as np
import pytest

import oracle_lib as ol
import pwpp_hip
import pwpp_synth
from test_arith_flavours import steep_plane_cloud
from test_gpu_inputs import Placed, encode, expected_array, submit, to_hip_params
from test_gpu_labels import _wedge, hip_copy
from test_gpu_parity import apply_variant, assert_frame_equal, to_oracle_params
from test_ref_fidelity import boundary_case

pytestmark = pytest.mark.gpu

F32 = np.float32
TINY = np.finfo(F32).tiny
GROUND_DECISIONS = (2, 4, 6)  # far_ground, ground, tgr_revert (oracle_lib.DEC_NAMES)
EDGE_TOL = 1e-9               # relative distance to a ring / sector / range edge below which numpy's bin may be the other one
MAX_EDGE_POINTS = 8           # ... and how many such points a frame may have where numpy and the device disagree


@pytest.fixture(scope="module")
def oracle(oracle_built):
    return oracle_built.restatement()


def czm_bins(pts, p):
    """pc2czm (reference patchworkpp.cpp:578-622) in numpy doubles, as _numpy_bins of test_capi_cpu.py: the bin of every point
    (-1 outside (min_range, max_range]), and whether the point lies within EDGE_TOL of a range, zone, ring or sector edge."""
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        r = np.sqrt(x * x + y * y)
        th = np.arctan2(y, x)
        th = np.where(th > 0, th, th + 2 * np.pi)
        mn, mx = p.min_range, p.max_range
        mr = [mn, (7 * mn + mx) / 8, (3 * mn + mx) / 4, (mn + mx) / 2, mx]
        rings, sect = list(p.num_rings_each_zone), list(p.num_sectors_each_zone)
        base = np.cumsum([0] + [a * b for a, b in zip(rings, sect)])
        ok = (r > mn) & (r <= mx)
        k = np.digitize(r, mr[1:4])
        code = np.full(len(r), -1)
        near = np.zeros(len(r), bool)
        for e in mr:
            near |= np.abs(r - e) <= EDGE_TOL * max(abs(e), 1.0)
        for z in range(4):
            m = ok & (k == z)
            fr = (r[m] - mr[z]) / ((mr[z + 1] - mr[z]) / rings[z])
            fs = th[m] / (2 * np.pi / sect[z])
            ring = np.minimum(fr.astype(int), rings[z] - 1)
            sec = np.minimum(fs.astype(int), sect[z] - 1)
            code[m] = base[z] + ring * sect[z] + sec
            near[m] |= (np.abs(fr - np.round(fr)) <= EDGE_TOL * np.maximum(fr, 1.0)) | (np.abs(fs - np.round(fs)) <= EDGE_TOL * np.maximum(fs, 1.0))
    return code, near


def rnr_mask(pts, p, sensor_height):
    """Reflected noise removal (ref :385-396) with the sensor height the frame was binned with: r is a FLOAT there."""
    if not p.enable_RNR or pts.shape[1] < 4:
        return np.zeros(len(pts), bool)
    x, y, z, w = (pts[:, i].astype(F32) for i in range(4))
    with np.errstate(all="ignore"):
        rf = np.sqrt(x * x + y * y)
        ang = np.arctan2(z.astype(np.float64), rf.astype(np.float64)) * 180 / np.pi
        return (ang < p.RNR_ver_angle_thr) & (z.astype(np.float64) < -sensor_height - 0.8) & (w < p.RNR_intensity_thr)


def expected_patches(pts, ref, p, sensor_height):
    """The oracle's row of every point (-1: no patch), and the points whose numpy bin is uncertain (next to an edge)."""
    code, near = czm_bins(pts, p)
    code[(pts[:, 2] == TINY) | rnr_mask(pts, p, sensor_height)] = -1
    nb = sum(a * b for a, b in zip(p.num_rings_each_zone, p.num_sectors_each_zone))
    row_of = np.full(nb + 1, -1, np.int64)
    row_of[ref.records["bin"]] = np.arange(len(ref.records))
    return row_of[code].astype(np.int32), near


def expected_distances(pts, patch, recs):
    """calc_point_to_plane_d (ref :551-554) in its own operations: float32 products and sums left to right, + d in double, one
    rounding to float; NaN where there is no patch."""
    out = np.full(len(pts), np.nan, F32)
    m = patch >= 0
    nrm, d = recs["normal"][patch[m]].astype(F32), recs["d"][patch[m]]
    x, y, z = (np.ascontiguousarray(pts[m, i], F32) for i in range(3))
    with np.errstate(all="ignore"):
        s = (nrm[:, 0] * x + nrm[:, 1] * y) + nrm[:, 2] * z  # (float32 arrays: no promotion, no fused multiply-add)
        out[m] = (s.astype(np.float64) + d).astype(F32)
    return out


def check_point_planes(h, frame, pts, ref, p, sensor_height=None, planes=None):
    """The frame's rows and distances against the oracle (membership, counts per patch, ground counts, distances); the
    distances against `planes` (records with normal and d) where given, else against the oracle's records."""
    pts = np.ascontiguousarray(pts, F32)
    n = len(pts)
    sh = p.sensor_height if sensor_height is None else sensor_height
    pat, dist = h.point_patches(frame), h.point_distances(frame)
    assert pat.dtype == np.int32 and pat.shape == (n,) and dist.dtype == F32 and dist.shape == (n,)
    recs = ref.records
    want, near = expected_patches(pts, ref, p, sh)
    bad = pat != want
    assert not (bad & ~near).any(), "patch rows differ from the oracle at %s" % np.flatnonzero(bad & ~near)[:10]
    assert bad.sum() <= MAX_EDGE_POINTS, "%d points next to a bin edge disagree" % bad.sum()
    assert pat.min(initial=0) >= -1 and pat.max(initial=-1) < len(recs)
    assert np.array_equal(np.bincount(pat[pat >= 0], minlength=len(recs)), recs["n_points"])
    assert (pat == -1).sum() == n - recs["n_points"].sum()
    ground = np.zeros(n, bool)
    ground[ref.ground_idx] = True
    g_per_patch = np.bincount(pat[ground & (pat >= 0)], minlength=len(recs))
    assert np.array_equal(g_per_patch, np.where(np.isin(recs["decision"], GROUND_DECISIONS), recs["n_ground"], 0))
    exp = expected_distances(pts, pat, recs if planes is None else planes)
    odd = np.flatnonzero(np.isnan(dist) != np.isnan(exp))
    assert len(odd) == 0, "NaN where the restatement has none, or the other way round: points %s, z %s, rows %s, %s against %s" % (
        odd[:6], pts[odd[:6], 2], pat[odd[:6]], dist[odd[:6]], exp[odd[:6]])
    assert np.isnan(dist[pat == -1]).all()
    ok = ~np.isnan(exp)
    assert np.array_equal(dist[ok].view(np.uint32), exp[ok].view(np.uint32)), "distances differ from the reference's formula"
    return pat, dist


def handle(params=None, **opts):
    h = pwpp_hip.Handle(params)
    h.set_point_planes(True)
    for k, v in opts.items():
        h.set_option(k, v)
    return h


def test_kitti_fresh_and_stateful(kitti, oracle):
    op = oracle.default_params()
    h = handle()
    h.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    for k, pts in enumerate(kitti):
        ref = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts)
        pat, dist = check_point_planes(h, k, pts, ref, op)
        assert_frame_equal(h, k, ref, pts.shape[0])
        rec = h.patch_records(k)
        assert np.array_equal(rec["bin"], ref.records["bin"]) and np.array_equal(h.normals(k), rec["normal"])
        assert (pat >= 0).mean() > 0.5 and (dist[pat >= 0] > 0.3).any() and (np.abs(dist[pat >= 0]) < 0.2).mean() > 0.3
    s = handle()
    est = ol.Estimator(oracle, arith=ol.ARITH_FXP)
    sh = op.sensor_height
    for k, pts in enumerate(kitti):
        s.estimate_ground(pts)
        ref = est.run(pts)
        check_point_planes(s, 0, pts, ref, op, sh)
        sh = ref.sensor_height


def test_getters_need_a_call_with_point_planes(kitti):
    h = pwpp_hip.Handle()
    with pytest.raises(pwpp_hip.PwppError):
        h.point_patches(0)  # no call yet
    h.estimate_ground_batch(kitti[:2], mode=pwpp_hip.MODE_FRESH)
    for get in (lambda: h.point_patches(0), lambda: h.point_distances(1), lambda: h.all_point_patches(),
                lambda: h.all_point_distances(), lambda: h.device_point_planes()):
        with pytest.raises(pwpp_hip.PwppError, match="without point planes"):
            get()
    h.set_point_planes(True)
    h.estimate_ground_batch(kitti[:2], mode=pwpp_hip.MODE_FRESH)
    assert h.point_patches(1).shape == (kitti[1].shape[0],)
    with pytest.raises(pwpp_hip.PwppError):
        h.point_distances(2)  # out of range
    h.set_point_planes(False)
    h.estimate_ground_batch(kitti[:2], mode=pwpp_hip.MODE_FRESH)
    with pytest.raises(pwpp_hip.PwppError, match="without point planes"):
        h.point_patches(0)


def test_batch_getters_and_device_pointers(kitti):
    h = handle()
    h.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    pats, base = h.all_point_patches()
    dists, base2 = h.all_point_distances()
    assert np.array_equal(base, base2) and len(pats) == len(dists) == int(base[-1])
    for k in range(len(kitti)):
        assert np.array_equal(pats[base[k]:base[k + 1]], h.point_patches(k))
        assert np.array_equal(dists[base[k]:base[k + 1]].view(np.uint32), h.point_distances(k).view(np.uint32))
    pp, dp = h.device_point_planes()
    assert pp and dp
    assert np.array_equal(hip_copy(pp, pats.nbytes).view(np.int32), pats)
    assert np.array_equal(hip_copy(dp, dists.nbytes).view(np.uint32), dists.view(np.uint32))
    out = np.full(int(base[-1]) + 3, 7, np.int32)
    got, _ = h.all_point_patches(out)
    assert np.array_equal(got, pats) and (out[int(base[-1]):] == 7).all()
    with pytest.raises(ValueError):
        h.all_point_distances(np.zeros(4, F32))


def test_every_path_writes_its_frames(kitti, oracle):
    """Single frame, fresh batch, two-pass binning, profiling, the three overflow redos, the overflow arena, stateful streams with
    K5 in one and in two launches, and the serial fix-up of frames (num_min_pts default and 0)."""
    op = oracle.default_params()
    est = lambda pts, o=None: ol.Estimator(oracle, o, arith=ol.ARITH_FXP).run(pts)
    refs = [est(pts) for pts in kitti]

    def check_batch(h, frames, rs, p=op):
        for i, pts in enumerate(frames):
            check_point_planes(h, i, pts, rs[i], p)

    h = handle()
    h.estimate_ground(kitti[3])
    check_point_planes(h, 0, kitti[3], refs[3], op)
    for opts in (dict(), dict(one_pass=0)):
        h = handle(**opts)
        h.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
        check_batch(h, kitti, refs)
    h = handle()
    h.set_profiling(True)
    h.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    check_batch(h, kitti, refs)
    prof = h.kernel_profile()
    assert prof["k_emit"][1] == 1 and prof["k_emit"][0] > 0
    # overflow redo: in place, without the arena, the whole batch
    wedge = _wedge(kitti[0], np.random.default_rng(5), 0.1)
    odd = [wedge, kitti[1], kitti[2], wedge, kitti[3]]
    rodd = [est(pts) for pts in odd]
    for opts in (dict(), dict(debug_flags=2048), dict(redo_whole_batch=1)):
        h = handle(**opts)
        h.estimate_ground_batch([kitti[i % 6] for i in range(7)], mode=pwpp_hip.MODE_FRESH)
        h.estimate_ground_batch(odd, mode=pwpp_hip.MODE_FRESH)
        assert h.redo_stats()[1] >= 1
        check_batch(h, odd, rodd)
    # overflow arena: one sector of a frame of 72 denser than the handle has seen (test_gpu_labels.py)
    arng = np.random.default_rng(11)
    a = np.arctan2(kitti[0][:, 1], kitti[0][:, 0])
    sel = np.where((a > 0.3) & (a < 0.6))[0]
    extra = kitti[0][arng.choice(sel, int(len(sel) * 0.4), replace=True)].copy()
    extra[:, :3] += arng.normal(0.0, 0.004, (len(extra), 3)).astype(F32)
    dense = np.ascontiguousarray(np.concatenate([kitti[0], extra]).astype(F32))
    base = [kitti[i % 6] for i in range(72)]
    h = handle()
    h.estimate_ground_batch(base, mode=pwpp_hip.MODE_FRESH)
    odd2 = list(base)
    odd2[10] = dense
    h.estimate_ground_batch(odd2, mode=pwpp_hip.MODE_FRESH)
    assert h.arena_stats()[0] >= 1 and h.redo_stats()[1] == 0
    for i in (0, 9, 10, 11, 71):
        check_point_planes(h, i, odd2[i], est(dense) if i == 10 else refs[i % 6], op)
    # stateful streams in lock step: RNR of a frame uses the height its stream had before it
    for split in ("0", "1"):
        h = handle(split_k5=split)
        h.set_num_streams(3)
        ests = [ol.Estimator(oracle, arith=ol.ARITH_FXP) for _ in range(3)]
        sh = [op.sensor_height] * 3
        for t in range(3):
            fr = [kitti[(s + t) % 6] for s in range(3)]
            h.estimate_ground_batch(fr, mode=pwpp_hip.MODE_STREAMS)
            for s in range(3):
                ref = ests[s].run(fr[s])
                check_point_planes(h, s, fr[s], ref, op, sh[s])
                sh[s] = ref.sensor_height
    # fix-up frames (k_fit_fixup, stages 2 | 4 | 8)
    frng = np.random.default_rng(5)

    def spoil(c, k):
        c = c.copy()
        c[frng.choice(c.shape[0], k, replace=False), 2] = -np.inf
        lone = np.array([[70.0, 30.0 + i, 1e30, 0.5] for i in range(3)] + [[3.5, -1.0, 3e38, 0.5]], F32)
        return np.ascontiguousarray(np.concatenate([c, lone]))

    spoiled = [spoil(kitti[0], 40), kitti[1], spoil(kitti[5], 3)]
    for variant in (dict(), dict(num_min_pts=0)):
        p = apply_variant(pwpp_hip.default_params(), variant)
        o = to_oracle_params(p)
        h = handle(params=p)
        h.estimate_ground_batch(spoiled, mode=pwpp_hip.MODE_FRESH)
        assert h.fixed_up_frames() >= 1
        check_batch(h, spoiled, [est(c, o) for c in spoiled], o)


@pytest.mark.parametrize("mem", ["host", "pinned_slab", "pinned_scattered", "device"])
@pytest.mark.parametrize("layout", ["row4", "row3", "col4", "col3", "fields16", "fields48", "fields_noi", "fields12"])
def test_every_layout_and_memory_kind(kitti, oracle, layout, mem):
    op = oracle.default_params()
    names = [kitti[0], kitti[4], pwpp_synth.add_edge_cases(pwpp_synth.make_cloud(23, beams=32, azimuth_steps=900), 23)]
    exps = [expected_array(pts, layout) for pts in names]
    refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(e) for e in exps]
    h = handle()
    placed = Placed([encode(e, layout, 7 + k) for k, e in enumerate(exps)], mem)
    try:
        submit(h, placed, layout, [len(e) for e in exps], pwpp_hip.MODE_FRESH)
        for k, e in enumerate(exps):
            check_point_planes(h, k, e, refs[k], op)
        placed.assert_unchanged()
    finally:
        placed.free()


def _nonfinite_z(src, rng):
    """A KITTI frame with NaN / +-inf heights, +-0 and subnormal coordinates in its patches, the FLT_MIN marker, RNR hits and
    points beyond max_range."""
    c = src.copy()
    idx = rng.choice(c.shape[0], 600, replace=False)
    c[idx[:60], 2] = np.nan
    c[idx[60:90], 2] = np.inf
    c[idx[90:120], 2] = -np.inf
    c[idx[120:180], 2] = TINY
    c[idx[180:240], :2] *= 200.0                     # beyond max_range
    c[idx[240:300], 3] = 0.01                        # dark ...
    c[idx[240:300], 2] = -4.0                        # ... and low: RNR where the angle says so
    c[idx[300:330], 2] = 0.0
    c[idx[330:360], 2] = -0.0
    c[idx[360:390], 2] = np.float32(1e-40)
    c[idx[390:420], 2] = np.float32(-1e-40)
    lone = np.array([[5.0, 0.0, np.nan, 0.5], [0.0, 7.0, np.inf, 0.5], [-6.0, 0.0, -np.inf, 0.5], [9.0, -0.0, -1.7, 0.5],
                     [-0.0, 9.0, -1.7, 0.5], [1e-40, 11.0, -1.7, 0.5]], F32)
    return np.ascontiguousarray(np.concatenate([c, lone]))


def test_boundary_clouds(kitti, oracle):
    """NaN / +-inf x, y, z; +-0 and subnormal coordinates; RNR points; points beyond max_range; a facade taller than the z range
    of the fit sums (flag_clamped); a num_min_pts that leaves small bins."""
    rng = np.random.default_rng(17)
    for kind in ("default", "ties"):
        op, pts = boundary_case(oracle, kind)
        h = handle(params=to_hip_params(op))
        h.estimate_ground(pts)
        ref = ol.Estimator(oracle, op, arith=ol.ARITH_FXP).run(pts)
        pat, _ = check_point_planes(h, 0, pts, ref, op)
        assert (pat == -1).any()
    op = oracle.default_params()
    odd = _nonfinite_z(kitti[1], rng)
    h = handle()
    h.estimate_ground(odd)
    ref = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(odd)
    # (a NaN height is undefined in the reference -- it sorts a bin with a.z < b.z -- and the records of patches that hold one are not
    # part of the parity contract: the distances are checked against the planes the handle reports, the contract's own words)
    mine = h.patch_records(0)
    pat, dist = check_point_planes(h, 0, odd, ref, op, planes=mine)
    assert (pat[np.isnan(odd[:, 2])] >= 0).any() and np.isinf(dist).any()
    assert (pat[odd[:, 2] == TINY] == -1).all()
    steep = steep_plane_cloud(kitti[2])
    h = handle()
    h.estimate_ground_batch([kitti[0], steep], mode=pwpp_hip.MODE_FRESH)
    assert h.clamped_frames() == 1
    for i, pts in enumerate((kitti[0], steep)):
        check_point_planes(h, i, pts, ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts), op)
    p = apply_variant(pwpp_hip.default_params(), dict(num_min_pts=40))
    o = to_oracle_params(p)
    h = handle(params=p)
    h.estimate_ground_batch(kitti[:3], mode=pwpp_hip.MODE_FRESH)
    for i in range(3):
        ref = ol.Estimator(oracle, o, arith=ol.ARITH_FXP).run(kitti[i])
        pat, _ = check_point_planes(h, i, kitti[i], ref, o)
        code, _ = czm_bins(kitti[i], o)
        small = (code >= 0) & ~np.isin(code, ref.records["bin"])
        assert small.any() and (pat[small] == -1).all()


def _outputs(h, frames):
    return [(h.point_patches(i).tobytes(), h.point_distances(i).tobytes()) for i in range(frames)]


def test_deterministic_on_the_overlap_schedule_and_through_a_pipe(kitti, oracle):
    F = 132  # (128+ frames: the overlap schedule)
    frames = [kitti[i % 6] for i in range(F)]
    refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts) for pts in kitti]
    op = oracle.default_params()
    h = handle()
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    first = _outputs(h, F)
    for i in (0, 1, 63, 64, 65, 66, 67, 127, 128, F - 1):
        check_point_planes(h, i, frames[i], refs[i % 6], op)
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert _outputs(h, F) == first, "point planes differ from run to run"
    import torch
    dev = torch.device("cuda", 0)
    tens = [torch.from_numpy(f).to(dev) for f in frames]
    torch.cuda.synchronize()
    ptrs = (ctypes.c_void_p * F)(*[t.data_ptr() for t in tens])
    ns = (ctypes.c_int32 * F)(*[f.shape[0] for f in frames])
    pipe = pwpp_hip.Pipe(depth=2)
    try:
        for i in range(2):
            pipe.handle(i).set_point_planes(True)
        seen = []
        for rep in range(4):
            hv = pipe.submit_device_batch((ptrs, ns, F))
            hv.synchronize()
            seen.append(_outputs(hv, F))
            if rep == 0:
                for i in (0, 65, F - 1):
                    check_point_planes(hv, i, frames[i], refs[i % 6], op)
        assert seen[0] == seen[1] == seen[2] == seen[3] == first
        pipe.drain()
    finally:
        pipe.close()


def _everything(h, frames, streams):
    """Every output but the point planes, as bytes; index lists sorted where their order is the scatter's."""
    out = []
    for i in range(frames):
        g, ng = h.ground_indices(i), h.nonground_indices(i)
        out.append((np.sort(g).tobytes(), np.sort(ng).tobytes(), h.counts(i), h.patch_records(i).tobytes(),
                    h.centers(i).tobytes(), h.normals(i).tobytes()))
    if streams:
        for s in range(frames):
            out.append((bytes(h.state(s)), np.asarray(h.plane_state(s)).tobytes(),
                        b"".join(h.history(s, w, r).tobytes() for w in (0, 1) for r in range(4))))
    return out


@pytest.mark.parametrize("order", [pwpp_hip.ORDER_SCATTER, pwpp_hip.ORDER_REFERENCE, pwpp_hip.ORDER_CLOUD])
@pytest.mark.parametrize("labels", [False, True])
def test_turning_it_on_changes_nothing_else(kitti, order, labels):
    ordered = order != pwpp_hip.ORDER_SCATTER
    for mode, frames in ((pwpp_hip.MODE_FRESH, kitti), (pwpp_hip.MODE_STREAMS, kitti[:3])):
        hs = []
        for on in (False, True):
            h = pwpp_hip.Handle()
            h.set_order(order)
            h.set_labels(labels)
            h.set_point_planes(on)
            if mode == pwpp_hip.MODE_STREAMS:
                h.set_num_streams(3)
            for _ in range(2 if mode == pwpp_hip.MODE_STREAMS else 1):
                h.estimate_ground_batch(frames, mode=mode)
            hs.append(h)
        off, on = hs
        n = len(frames)
        assert _everything(off, n, mode == pwpp_hip.MODE_STREAMS) == _everything(on, n, mode == pwpp_hip.MODE_STREAMS)
        if ordered:
            for i in range(n):
                assert off.ground_indices(i).tobytes() == on.ground_indices(i).tobytes()
                assert off.nonground_indices(i).tobytes() == on.nonground_indices(i).tobytes()
        if labels or order == pwpp_hip.ORDER_CLOUD:
            assert off.all_labels()[0].tobytes() == on.all_labels()[0].tobytes()
        assert on.point_patches(0).shape == (frames[0].shape[0],)


def test_workspace_grows_only_with_the_feature_and_trim_gives_it_back(kitti):
    ref = pwpp_hip.Handle()  # (the same calls and the trim, without the feature)
    for _ in range(2):
        ref.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    ref.trim_workspace()
    ref.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    never = ref.workspace_bytes()
    w = pwpp_hip.Handle()
    w.set_point_planes(True)
    w.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    on = w.workspace_bytes()
    assert on >= never + 8 * sum(len(p) for p in kitti)
    w.set_point_planes(False)
    w.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    w.trim_workspace()
    w.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    assert w.workspace_bytes() == never


def test_pybind_module_and_ctypes_handle_agree_with_the_c_getters(kitti):
    import pypatchworkpp
    pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    pp.setPointPlanes(True)
    h = handle()
    L = pwpp_hip.load()
    for pts in kitti[:3]:
        pp.estimateGround(pts)
        h.estimate_ground(pts)
        a, d = pp.getPointPatches(), pp.getPointDistances()
        assert a.dtype == np.int32 and d.dtype == F32 and a.shape == d.shape == (pts.shape[0],)
        ca, cd = np.empty(len(pts), np.int32), np.empty(len(pts), F32)
        assert L.pwpp_get_point_patches(h._h, 0, ca.ctypes.data_as(ctypes.c_void_p)) == 0
        assert L.pwpp_get_point_distances(h._h, 0, cd.ctypes.data_as(ctypes.c_void_p)) == 0
        assert np.array_equal(a, ca) and np.array_equal(h.point_patches(0), ca)
        assert np.array_equal(d.view(np.uint32), cd.view(np.uint32)) and np.array_equal(h.point_distances(0).view(np.uint32), cd.view(np.uint32))
        assert np.array_equal(pp.getCenters(), h.centers(0)) and (a < len(pp.getCenters())).all()
    q = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    q.estimateGround(kitti[0])
    with pytest.raises(RuntimeError):
        q.getPointPatches()
