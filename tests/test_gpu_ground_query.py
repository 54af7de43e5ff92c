"""The ground queries (pwpp_query_ground, pwpp_rasterize_ground) on a real MI355X: the fitted ground model of the last call at
arbitrary positions and as a grid, against the point planes of the cloud's own points, against the oracle's records through the
numpy restatement (tests/ground_query_ref.py), after every kind of call, from host and device memory -- and that asking changes
nothing else.  Shapes are small on purpose: a KITTI frame or three, lists of a few thousand positions, grids of a few rows."""
import ctypes

import numpy as np
import pytest

import ground_query_ref as gq
import oracle_lib as ol
import pwpp_hip
import pwpp_synth
from test_gpu_parity import apply_variant, to_oracle_params
from test_gpu_point_planes import MAX_EDGE_POINTS, czm_bins, rnr_mask
from test_tiny_fits import ROS_LAUNCH

pytestmark = pytest.mark.gpu

F32 = np.float32
TINY = np.finfo(F32).tiny
E_ARG, E_STATE = -1, -4
DT = pwpp_hip.GROUND_SAMPLE_DTYPE
NAN, INF = np.nan, np.inf
# On the decision surfaces of pc2czm with the default CZM (min_range 2.7, max_range 80, zone radii 12.3625 / 22.025 / 41.35): the
# four axes, the diagonals, r exactly min_range and max_range, the zone radii, the origin; NaN and +-inf coordinates; the skip
# marker FLT_MIN and non-finite values as z (z plays no part in the bin).
FIXED_POSITIONS = np.array(
    [[5, 0, -1.7], [-5, 0, -1.7], [0, 5, -1.7], [0, -5, -1.7], [4, 4, -1.7], [-4, 4, -1.7], [-4, -4, -1.7], [4, -4, -1.7],
     [2.7, 0, -1.7], [0, 2.7, -1.7], [80, 0, -1.7], [0, -80, -1.7], [12.3625, 0, -1.7], [0, 22.025, -1.7], [-41.35, 0, -1.7],
     [0, 0, -1.7], [NAN, 3, -1.7], [3, NAN, -1.7], [INF, 3, -1.7], [3, -INF, -1.7], [-INF, INF, 0], [1e3, 1e3, 0], [1.0, 1.0, 0],
     [6, 2, TINY], [6, 2, NAN], [6, 2, INF], [-7, 3, -INF], [30, -30, 1.5]], F32)


def uniform_positions(n=4000, seed=20):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-90.0, 90.0, (n, 3)).astype(F32)
    xyz[:, 2] = rng.uniform(-3.0, 1.0, n).astype(F32)
    return xyz


def all_positions():
    return np.ascontiguousarray(np.concatenate([uniform_positions(), FIXED_POSITIONS]))


@pytest.fixture(scope="module")
def oracle(oracle_built):
    return oracle_built.restatement()


@pytest.fixture(scope="module")
def refs(kitti, oracle):
    """The oracle's results of the first three KITTI frames with default parameters, computed once."""
    return [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts) for pts in kitti[:3]]


def assert_samples(got, xyz, recs, p, what=""):
    """`got` against the restated query of `xyz` over the patch records `recs`: positions next to a bin edge may land in the
    neighbouring patch (at most MAX_EDGE_POINTS of them); everything else is bit-equal."""
    want, near = gq.restate_query(xyz, recs, p)
    assert got.dtype == DT and got.shape == want.shape
    bad = got["patch"] != want["patch"]
    assert not (bad & ~near).any(), "%s: rows differ from the restatement at %s" % (what, np.flatnonzero(bad & ~near)[:8])
    assert bad.sum() <= MAX_EDGE_POINTS, "%s: %d positions next to a bin edge disagree" % (what, bad.sum())
    # (a position that landed in the neighbouring patch is checked against THAT patch's plane)
    want = gq.samples_from_rows(xyz, got["patch"], recs) if bad.any() else want
    assert gq.same_samples(got, want), "%s: samples differ from the restated formulas" % what
    none = got["patch"] == -1
    assert (got["decision"][none] == 0).all() and np.isnan(got["ground_z"][none]).all() and np.isnan(got["distance"][none]).all()
    return want


def device_tensor(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def test_the_cloud_queried_against_itself(kitti):
    p = pwpp_hip.default_params()
    pts = kitti[2].copy()
    pts[100:4000:100, 2] = TINY  # (the skip marker on a few points of the scan)
    h = pwpp_hip.Handle()
    h.set_point_planes(True)
    h.estimate_ground_batch([pts], mode=pwpp_hip.MODE_FRESH)
    q = h.query_ground(pts[:, :3])
    pat, dist = h.point_patches(0), h.point_distances(0)
    own = pat >= 0
    assert own.mean() > 0.5
    assert np.array_equal(q["patch"][own], pat[own])  # (no edge allowance: both sides use the device's bin)
    assert np.array_equal(q["distance"][own].view(np.uint32), dist[own].view(np.uint32))
    rec = h.patch_records(0)
    assert np.array_equal(q["decision"][own], rec["decision"][pat[own]])
    # RNR and the FLT_MIN marker are tests on cloud points: a removed point's POSITION still queries into its bin's patch
    extra = ~own & (q["patch"] >= 0)
    removed = rnr_mask(pts, p, p.sensor_height) | (pts[:, 2] == TINY)
    assert extra.any() and removed[extra].all()
    # the ROS launch file's parameters (num_min_pts 0: every bin is a row, empty ones included) on half a synthetic scan
    rp = apply_variant(pwpp_hip.default_params(), ROS_LAUNCH)
    syn = pwpp_synth.make_cloud(7, beams=32, azimuth_steps=900)
    syn = np.ascontiguousarray(syn[syn[:, 1] > 0.5])
    h = pwpp_hip.Handle(rp)
    h.set_point_planes(True)
    h.estimate_ground_batch([syn], mode=pwpp_hip.MODE_FRESH)
    rec = h.patch_records(0)
    assert len(rec) == gq.num_bins(rp) and (rec["n_points"] == 0).sum() > 100
    q = h.query_ground(syn[:, :3])
    pat, dist = h.point_patches(0), h.point_distances(0)
    own = pat >= 0
    assert own.sum() > 0.5 * len(syn)
    assert np.array_equal(q["patch"][own], pat[own]) and np.array_equal(q["distance"][own].view(np.uint32), dist[own].view(np.uint32))
    assert (q["patch"][~own & (syn[:, 2] != TINY)] == -1).all()  # (no RNR here: only positions outside the range)
    mirror = syn[:2000, :3] * np.array([1, -1, 1], F32)  # positions in the empty half: rows that own no points
    got = h.query_ground(mirror)
    assert_samples(got, mirror, rec, to_oracle_params(rp), "empty bins")
    inside = got["patch"] >= 0
    assert inside.sum() > 1500 and (rec["n_points"][got["patch"][inside]] == 0).mean() > 0.9
    assert np.array_equal(got["patch"][inside], rec["bin"][got["patch"][inside]])


def test_against_the_oracle(kitti, oracle, refs):
    op = oracle.default_params()
    xyz = all_positions()
    h = pwpp_hip.Handle()
    h.estimate_ground_batch([kitti[0]], mode=pwpp_hip.MODE_FRESH)
    got = h.query_ground(xyz)
    want = assert_samples(got, xyz, refs[0].records, op, "oracle records")
    # both answers are well populated: 38 % of the draw lies outside the range; of the rest the restatement finds a patch for ~950
    assert (got["patch"] >= 0).sum() == (want["patch"] >= 0).sum() > 400 and (got["patch"] == -1).sum() > 1000
    fixed = got[-len(FIXED_POSITIONS):]
    assert (fixed["patch"][:15] >= 0).sum() >= 8                       # axes, diagonals, range and zone radii
    assert (fixed["patch"][15:23] == -1).all()                         # origin, NaN / inf, far outside, inside min_range
    assert fixed["patch"][23] >= 0 and fixed["patch"][23] == fixed["patch"][24] == fixed["patch"][25]   # z plays no part
    assert np.isnan(fixed["distance"][24]) and np.isinf(fixed["distance"][25]) and np.isfinite(fixed["ground_z"][24:26]).all()
    assert set(np.unique(want["decision"])) >= {0, 4}


def test_list_sizes_and_frame_selectors(kitti):
    op = to_oracle_params(pwpp_hip.default_params())
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(kitti[:3], mode=pwpp_hip.MODE_FRESH)
    L = pwpp_hip.load()
    pool = all_positions()[-257:]
    per_frame = [h.query_ground(pool, frames=f) for f in range(3)]
    for f in range(3):
        assert_samples(per_frame[f], pool, h.patch_records(f), op, "frame %d" % f)
    assert not gq.same_samples(per_frame[0], per_frame[1])
    sel_all = np.array([(2, 0, -1, 1, 3, 1, 2, 0)[i % 8] for i in range(257)], np.int32)
    for m in (0, 1, 63, 64, 65, 257):
        xyz, sel = np.ascontiguousarray(pool[:m]), np.ascontiguousarray(sel_all[:m])
        out = np.zeros(m + 1, DT)
        out.view(np.uint8)[:] = 0xA5
        rc = L.pwpp_query_ground(h._h, xyz.ctypes.data_as(ctypes.c_void_p), sel.ctypes.data_as(ctypes.c_void_p), m, pwpp_hip.MEM_HOST,
                                 out.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0
        assert (out[m:].view(np.uint8) == 0xA5).all(), "the sample behind the list was written"
        want = np.zeros(m, DT)
        want["patch"], want["ground_z"], want["distance"] = -1, np.nan, np.nan
        for f in range(3):
            want[sel == f] = per_frame[f][:m][sel == f]
        assert gq.same_samples(out[:m], want), "m = %d" % m
        if m:
            assert gq.same_samples(h.query_ground(xyz, frames=sel), want)
    assert gq.same_samples(h.query_ground(pool), per_frame[0])  # (no selector: frame 0)


GRIDS = [(5, 3, 4.0), (64, 1, 0.75), (67, 2, 1.25), (130, 9, 1.5)]  # nx, ny, cell in metres


def grid_origin(nx, ny, cell):
    """An origin that puts the centres of column nx // 2 on x == 0 and of row ny // 2 on y == 0, hence a diagonal on |x| == |y|."""
    return -(nx // 2 + 0.5) * cell, -(ny // 2 + 0.5) * cell


@pytest.mark.parametrize("debug_flags", [0, 16])
def test_raster_equals_query(kitti, debug_flags):
    import torch
    h = pwpp_hip.Handle()
    h.set_option("debug_flags", debug_flags)
    h.estimate_ground_batch(kitti[:3], mode=pwpp_hip.MODE_FRESH)
    for nx, ny, cell in GRIDS:
        x0, y0 = grid_origin(nx, ny, cell)
        centres = gq.cell_centres(x0, y0, cell, nx, ny)
        assert (centres[:, 0] == 0).sum() == ny and (centres[:, 1] == 0).sum() == nx
        assert (np.abs(centres[:, 0]) == np.abs(centres[:, 1])).sum() >= min(nx, ny)
        cells = [h.query_ground(centres, frames=f) for f in range(3)]
        for first, count in ((0, 3), (1, 2), (2, 1)):
            for ground_only in (False, True):
                want_h = np.stack([c["ground_z"].reshape(ny, nx) for c in cells[first:first + count]]).copy()
                want_p = np.stack([c["patch"].reshape(ny, nx) for c in cells[first:first + count]])
                if ground_only:
                    dec = np.stack([c["decision"].reshape(ny, nx) for c in cells[first:first + count]])
                    want_h[np.isin(dec, gq.HIDDEN_DECISIONS)] = np.nan
                hgt, pat = h.rasterize_ground(x0, y0, cell, nx, ny, first, count, ground_only=ground_only, with_patches=True)
                alone = h.rasterize_ground(x0, y0, cell, nx, ny, first, count, ground_only=ground_only)
                assert hgt.shape == pat.shape == alone.shape == (count, ny, nx) and hgt.dtype == F32 and pat.dtype == np.int32
                assert np.array_equal(pat, want_p)
                for img in (hgt, alone):
                    nan = np.isnan(want_h)
                    assert np.array_equal(np.isnan(img), nan) and np.array_equal(img[~nan].view(np.uint32), want_h[~nan].view(np.uint32))
                # device output, 4 bytes off a 16-byte boundary, with a poisoned word on either side
                n = count * ny * nx
                dh = torch.full((n + 3,), -7.0, dtype=torch.float32, device="cuda")
                dp = torch.full((n + 3,), -7, dtype=torch.int32, device="cuda")
                assert dh.data_ptr() % 16 == 0 and dp.data_ptr() % 16 == 0
                h.rasterize_ground_device(x0, y0, cell, nx, ny, dh.data_ptr() + 4, dp.data_ptr() + 4, first, count, ground_only)
                h.synchronize()
                gh, gp = dh.cpu().numpy(), dp.cpu().numpy()
                assert gh[0] == -7 and (gh[n + 1:] == -7).all() and gp[0] == -7 and (gp[n + 1:] == -7).all()
                assert np.array_equal(gh[1:n + 1].view(np.uint32), hgt.reshape(-1).view(np.uint32)) and np.array_equal(gp[1:n + 1], pat.reshape(-1))
    dec = np.concatenate([c["decision"] for c in cells])
    assert np.isin(dec, gq.HIDDEN_DECISIONS).any(), "no cell of the last grid exercises PWPP_GRID_GROUND_ONLY"


def test_after_every_kind_of_call(kitti):
    import torch
    xyz = all_positions()[::4]
    p = pwpp_hip.default_params()
    op = to_oracle_params(p)
    # a streams-mode step
    h = pwpp_hip.Handle()
    h.set_num_streams(2)
    for t in range(2):
        h.estimate_ground_batch([kitti[t], kitti[t + 2]], mode=pwpp_hip.MODE_STREAMS)
    for f in range(2):
        assert_samples(h.query_ground(xyz, frames=f), xyz, h.patch_records(f), op, "streams")
    # a frame that takes the serial fix-up
    lp = apply_variant(pwpp_hip.default_params(), dict(num_lpr=0))
    h = pwpp_hip.Handle(lp)
    before = h.fixed_up_frames()
    h.estimate_ground_batch(kitti[:2], mode=pwpp_hip.MODE_FRESH)
    got = h.query_ground(xyz, frames=1)  # (the query itself lands the call and finishes the frame)
    assert h.fixed_up_frames() > before
    assert_samples(got, xyz, h.patch_records(1), to_oracle_params(lp), "fix-up")
    # a batch whose one-pass segments are far too small: frames are binned again
    h = pwpp_hip.Handle()
    h.set_option("one_pass_scale", 0.02)
    tens = [device_tensor(f) for f in kitti[:3]]
    ptrs, ns = [t.data_ptr() for t in tens], [f.shape[0] for f in kitti[:3]]
    h.estimate_ground_batch_device(ptrs, ns)
    got = h.query_ground(xyz, frames=2)  # (asynchronous call: the query lands it and redoes the frames)
    assert h.redo_stats()[1] > 0, "the overflow redo did not run"
    assert_samples(got, xyz, h.patch_records(2), op, "redo")
    # a pipe's handle
    pipe = pwpp_hip.Pipe(depth=2)
    try:
        batch = h.make_device_batch(ptrs, ns)
        for rep in range(3):
            hv = pipe.submit_device_batch(batch)
            got = hv.query_ground(xyz, frames=rep)
            assert_samples(got, xyz, hv.patch_records(rep), op, "pipe")
        pipe.drain()
    finally:
        pipe.close()
    del tens
    torch.cuda.synchronize()


def test_memory_kinds_agree(kitti):
    import torch
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(kitti[:2], mode=pwpp_hip.MODE_FRESH)
    xyz = all_positions()
    sel = (np.arange(len(xyz)) % 2).astype(np.int32)
    host = h.query_ground(xyz, frames=sel)
    for shift in (0, 4):  # (a sample array 16-byte aligned, and 4 bytes off)
        dx, ds = device_tensor(xyz), device_tensor(sel)
        dout = torch.full((4 * len(xyz) + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        h.query_ground_device(dx.data_ptr(), ds.data_ptr(), len(xyz), dout.data_ptr() + shift)
        h.synchronize()  # (complete after pwpp_synchronize: the copy below is on another stream)
        raw = dout.cpu().numpy()
        k = shift // 4
        assert raw[k:k + 4 * len(xyz)].tobytes() == host.tobytes()
        assert (raw[:k] == 0x5A5A5A5A).all() and (raw[k + 4 * len(xyz):] == 0x5A5A5A5A).all()
    L = pwpp_hip.load()
    out = np.zeros(4, DT)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.pwpp_query_ground(h._h, vp(xyz), None, 4, pwpp_hip.MEM_HOST_PINNED, vp(out)) == E_ARG


def test_state_and_arguments(kitti):
    L = pwpp_hip.load()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    xyz = np.ascontiguousarray(all_positions()[:64])
    out = np.zeros(64, DT)
    img = np.zeros(3 * 16, F32)
    grid = lambda **kw: pwpp_hip.GroundGrid(**dict(dict(x0=-2.0, y0=-2.0, cell=1.0, nx=4, ny=4, flags=0, pad_=0), **kw))
    query = lambda h, m=64, x=xyz, o=out, mem=pwpp_hip.MEM_HOST: L.pwpp_query_ground(h._h, vp(x) if x is not None else None, None, m, mem,
                                                                                     vp(o) if o is not None else None)
    raster = lambda h, g, first=0, frames=1, mem=pwpp_hip.MEM_HOST, o=img: L.pwpp_rasterize_ground(
        h._h, ctypes.byref(g) if g is not None else None, first, frames, mem, vp(o) if o is not None else None, None)
    h = pwpp_hip.Handle()
    assert query(h) == E_STATE and raster(h, grid()) == E_STATE  # before any call
    h.estimate_ground_batch(kitti[:3], mode=pwpp_hip.MODE_FRESH)
    assert query(h) == 0 and raster(h, grid(), 0, 3) == 0
    assert query(h, m=0) == 0 and query(h, m=0, x=None, o=None) == 0
    assert query(h, o=None) == E_ARG and query(h, x=None) == E_ARG and query(h, m=-1) == E_ARG
    assert query(h, mem=pwpp_hip.MEM_HOST_PINNED) == E_ARG and query(h, mem=7) == E_ARG
    assert raster(h, None) == E_ARG and raster(h, grid(), o=None) == E_ARG
    for bad in (dict(nx=0), dict(ny=0), dict(nx=-3), dict(cell=0.0), dict(cell=-1.0), dict(cell=np.nan), dict(cell=np.inf)):
        assert raster(h, grid(**bad)) == E_ARG, bad
    for first, frames in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2), (0, -1)):
        assert raster(h, grid(), first, frames) == E_ARG, (first, frames)
    assert raster(h, grid(nx=1 << 16, ny=1 << 15), 0, 2) == E_ARG  # 2^32 cells; nothing is written before the check
    assert raster(h, grid(), mem=pwpp_hip.MEM_HOST_PINNED) == E_ARG
    assert raster(h, grid(), 2, 1) == 0
    # a second call followed by a query answers from the new call (the bin -> row table is ranked anew)
    op = to_oracle_params(pwpp_hip.default_params())
    pos = all_positions()
    first = h.query_ground(pos, frames=0)
    half = np.ascontiguousarray(kitti[4][kitti[4][:, 0] > 0])  # (half a scan: other bins are patches)
    h.estimate_ground_batch([half], mode=pwpp_hip.MODE_FRESH)
    second = h.query_ground(pos)
    assert_samples(second, pos, h.patch_records(0), op, "second call")
    assert not np.array_equal(first["patch"], second["patch"])
    assert (h.query_ground(pos, frames=1)["patch"] == -1).all()  # (the last call had one frame)
    h.trim_workspace()
    assert query(h) == E_STATE and raster(h, grid()) == E_STATE
    assert b"no frame" in L.pwpp_last_error()
    h.estimate_ground_batch(kitti[:1], mode=pwpp_hip.MODE_FRESH)
    assert query(h) == 0


def _everything(h, frames):
    out = []
    for i in range(frames):
        out.append((h.ground_indices(i).tobytes(), h.nonground_indices(i).tobytes(), h.counts(i), h.patch_records(i).tobytes(),
                    h.centers(i).tobytes(), h.normals(i).tobytes(), h.labels(i).tobytes()))
    for s in range(frames):
        out.append((bytes(h.state(s)), np.asarray(h.plane_state(s)).tobytes(),
                    b"".join(h.history(s, w, r).tobytes() for w in (0, 1) for r in range(4))))
    return out


def test_nothing_else_moves(kitti):
    pos = all_positions()
    res = []
    for ask in (False, True):
        h = pwpp_hip.Handle()
        h.set_order(pwpp_hip.ORDER_CLOUD)
        h.set_num_streams(3)
        h.estimate_ground_batch(kitti[:3], mode=pwpp_hip.MODE_STREAMS)
        if ask:
            h.query_ground(pos, frames=1)
            h.rasterize_ground(-20.0, -20.0, 0.5, 80, 80, with_patches=True)
        h.estimate_ground_batch(kitti[3:6], mode=pwpp_hip.MODE_STREAMS)
        res.append(_everything(h, 3))
    assert res[0] == res[1], "a ground query between two calls changed the second call's outputs"
    # the workspace: nothing is held for the queries before the first one; the trim gives everything back
    ref = pwpp_hip.Handle()
    ref.estimate_ground_batch(kitti[:3], mode=pwpp_hip.MODE_FRESH)
    w = pwpp_hip.Handle()
    w.estimate_ground_batch(kitti[:3], mode=pwpp_hip.MODE_FRESH)
    before = w.workspace_bytes()
    assert before == ref.workspace_bytes()
    w.query_ground(pos)
    asked = w.workspace_bytes()
    assert asked >= before + 4 * 3 * gq.num_bins(w.params) + 32 * len(pos)
    w.rasterize_ground(-20.0, -20.0, 0.5, 8, 8)
    assert w.workspace_bytes() == asked  # (the staging buffer is reused)
    ref.trim_workspace()
    w.trim_workspace()
    assert w.workspace_bytes() == ref.workspace_bytes() < before


def test_pybind_module_and_ctypes_handle_agree_with_the_c_calls(kitti):
    import pypatchworkpp
    pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    h = pwpp_hip.Handle()
    L = pwpp_hip.load()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pos = all_positions()
    with pytest.raises(RuntimeError):
        pp.queryGround(pos)  # no frame yet
    pp.estimateGround(kitti[1])
    h.estimate_ground(kitti[1])
    a = pp.queryGround(pos)
    c = np.zeros(len(pos), DT)
    assert L.pwpp_query_ground(h._h, vp(pos), None, len(pos), pwpp_hip.MEM_HOST, vp(c)) == 0
    assert a.dtype == DT and a.shape == c.shape and a.tobytes() == c.tobytes() and h.query_ground(pos).tobytes() == c.tobytes()
    assert (a["patch"] < len(pp.getCenters())).all() and (a["patch"] >= 0).any()
    for ground_only in (False, True):
        img = pp.getElevationMap(-30.0, -12.0, 0.5, 120, 48, ground_only)
        g = pwpp_hip.GroundGrid(-30.0, -12.0, 0.5, 120, 48, pwpp_hip.GRID_GROUND_ONLY if ground_only else 0, 0)
        ci = np.zeros((48, 120), F32)
        assert L.pwpp_rasterize_ground(h._h, ctypes.byref(g), 0, 1, pwpp_hip.MEM_HOST, vp(ci), None) == 0
        assert img.dtype == F32 and img.shape == (48, 120) and img.tobytes() == ci.tobytes()
        assert h.rasterize_ground(-30.0, -12.0, 0.5, 120, 48, ground_only=ground_only)[0].tobytes() == ci.tobytes()
    assert np.isfinite(ci).mean() > 0.5
    with pytest.raises(RuntimeError):
        pp.getElevationMap(0.0, 0.0, 0.0, 4, 4)
