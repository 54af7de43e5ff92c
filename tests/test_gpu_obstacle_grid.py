"""The obstacle grid (pwpp_rasterize_obstacles) on a real MI355X: the non-ground points of the last call counted per cell of a
pwpp_ground_grid -- against the numpy restatement (tests/obstacle_grid_ref.py) fed with the library's own non-ground rows and
ground queries (bit for bit), against the oracle's non-ground set and records, after every kind of call and in every output
order, from host and device memory, with an input transform -- and that asking changes nothing else.  Shapes are small on
purpose: synthetic scans of ~3 k points, a KITTI frame where the oracle or a redo is involved."""
import ctypes

import numpy as np
import pytest

import ground_query_ref as gq
import obstacle_grid_ref as og
import oracle_lib as ol
import pwpp_hip
import pwpp_synth
from test_gpu_inputs import Placed, encode, expected_array, submit
from test_gpu_parity import apply_variant
from test_gpu_point_planes import MAX_EDGE_POINTS
from test_tiny_fits import ROS_LAUNCH

pytestmark = pytest.mark.gpu

F32 = np.float32
E_ARG, E_STATE = -1, -4
INF = np.inf
SHAPES = [(1, 1), (7, 5), (64, 64), (257, 3)]  # nx, ny: one cell, a few, several blocks' worth, a row longer than a block


def small_cloud(seed):
    return pwpp_synth.make_cloud(seed, beams=16, azimuth_steps=200)


def inner_cloud(n=300, seed=3):
    """Every point inside min_range of both parameter sets (r < 0.9 m): all of it non-ground, none of it with a patch."""
    rng = np.random.default_rng(seed)
    a, r = rng.uniform(0, 2 * np.pi, n), rng.uniform(0.05, 0.9, n)
    return np.ascontiguousarray(np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-1.8, 0.5, n), rng.uniform(0, 1, n)], 1), F32)


def three_frames():
    """Three frames of different sizes: a scan, an empty frame, a frame that is all unref."""
    return [small_cloud(5), np.zeros((0, 4), F32), inner_cloud()]


def grids_of(nx, ny):
    """(x0, y0, cell) per shape: cells of 0.5 m around (6, 1); an offset grid that cuts the cloud (x > 2 only, cells that are no
    binary fraction); and for the single cell the whole range, so that every counted point meets in one word."""
    out = [(6.0 - 0.25 * nx, 1.0 - 0.25 * ny, 0.5), (2.0, -ny * 1.7 / 3, 1.7)]
    if nx * ny == 1:
        out.append((-150.0, -150.0, 300.0))
    return out


def restated(h, f, x0, y0, cell, nx, ny, h_min, h_max, ground_only):
    """The restatement fed with the library's own rows and samples of frame f."""
    xyz = h.nonground(f)
    return og.restate_obstacles(xyz, h.query_ground(xyz, frames=f), x0, y0, cell, nx, ny, h_min, h_max, ground_only)


def images(h, x0, y0, cell, nx, ny, h_min, h_max, **kw):
    return h.rasterize_obstacles(x0, y0, cell, nx, ny, h_min, h_max, want_top=True, want_unref=True, **kw)


def as_bytes(imgs):
    return tuple(np.ascontiguousarray(a).tobytes() for a in imgs)


def device_tensor(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


# ---- against the library's own query -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["default", "ros_launch"])
def test_against_the_librarys_own_query(variant):
    p = pwpp_hip.default_params() if variant == "default" else apply_variant(pwpp_hip.default_params(), ROS_LAUNCH)
    frames = three_frames()
    h = pwpp_hip.Handle(p)
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert h.counts(1)[:2] == (0, 0) and h.counts(2)[:2] == (0, len(frames[2]))
    xyz0 = h.nonground(0)
    q0 = h.query_ground(xyz0, frames=0)
    owned = np.flatnonzero((q0["patch"] >= 0) & np.isfinite(q0["distance"]) & (xyz0[:, 0] > 2.5))
    assert len(owned) > 200
    one = float(np.sort(q0["distance"][owned])[len(owned) // 2])  # one point's own height: h_min == h_max
    bands = [(0.2, 2.5), (-INF, INF), (one, one)]
    seen_count = seen_unref = 0
    for nx, ny in SHAPES:
        for x0, y0, cell in grids_of(nx, ny):
            for h_min, h_max in bands:
                for ground_only in (False, True):
                    got = images(h, x0, y0, cell, nx, ny, h_min, h_max, ground_only=ground_only)
                    assert all(a.shape == (3, ny, nx) for a in got)
                    assert got[0].dtype == np.int32 and got[1].dtype == F32 and got[2].dtype == np.int32
                    what = "%dx%d at (%g, %g) cell %g band [%g, %g] ground_only %s" % (nx, ny, x0, y0, cell, h_min, h_max, ground_only)
                    for f in range(3):
                        want = restated(h, f, x0, y0, cell, nx, ny, h_min, h_max, ground_only)
                        for g, w, name in zip(got, want, ("count", "top", "unref")):
                            assert og.same_images(g[f], w), "%s, frame %d: %s differs from the restatement" % (what, f, name)
                    nan = np.isnan(got[1])
                    assert np.array_equal(nan, got[0] == 0) and (got[1][nan].view(np.uint32) == og.QNAN_BITS).all()
                    assert got[0][1].sum() == 0 and got[2][1].sum() == 0 and got[0][2].sum() == 0  # the empty frame, the unref frame
                    if cell == 300.0:  # every point of a frame in one cell: the atomics under full contention
                        n0, n2 = h.counts(0)[1], h.counts(2)[1]
                        assert got[2][2, 0, 0] == n2 == len(frames[2])
                        if (h_min, h_max) == (-INF, INF):
                            # only a point WITH a reference and a NaN height is in neither image (a hidden patch's are unref)
                            ref0 = (q0["patch"] >= 0) & ~(ground_only & np.isin(q0["decision"], gq.HIDDEN_DECISIONS))
                            assert got[0][0, 0, 0] + got[2][0, 0, 0] == n0 - np.isnan(q0["distance"][ref0]).sum()
                        if h_min == h_max:
                            assert got[0][0, 0, 0] >= 1 and got[1][0, 0, 0] == F32(one)
                    seen_count += int(got[0].sum())
                    seen_unref += int(got[2].sum())
    assert seen_count > 2000 and seen_unref > 1000  # (every loop above compared populated images)


def test_exact_binning_only_gives_the_same_images():
    frames = three_frames()
    res = []
    for flags in (0, 16):
        h = pwpp_hip.Handle()
        h.set_option("debug_flags", flags)
        h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
        res.append(as_bytes(images(h, -32.0, -32.0, 1.0, 64, 64, 0.2, 2.5)))
    assert res[0] == res[1]


# ---- against the oracle ------------------------------------------------------------------------------------------------------
def test_against_the_oracle(kitti, oracle_built):
    oracle = oracle_built.restatement()
    op = oracle.default_params()
    pts = kitti[0]
    ref = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts)
    xyz = np.ascontiguousarray(pts[np.sort(ref.nonground_idx), :3], F32)
    s, near = gq.restate_query(xyz, ref.records, op)
    h = pwpp_hip.Handle()
    h.estimate_ground_batch([pts], mode=pwpp_hip.MODE_FRESH)
    x0, y0, cell, nx, ny = -64.0, -64.0, 2.0, 64, 64
    kx, ix = og.cells_of(xyz[:, 0], x0, cell, nx)
    ky, iy = og.cells_of(xyz[:, 1], y0, cell, ny)
    near_cells = set((iy * nx + ix)[near & kx & ky].tolist())
    plain = None
    for h_min, h_max, ground_only in ((0.2, 2.5, False), (-INF, INF, False), (0.2, 2.5, True)):
        got = tuple(a[0] for a in images(h, x0, y0, cell, nx, ny, h_min, h_max, ground_only=ground_only))
        want = og.restate_obstacles(xyz, s, x0, y0, cell, nx, ny, h_min, h_max, ground_only)
        dc, du = got[0] != want[0], got[2] != want[2]
        moved = int(np.abs(got[0] - want[0]).sum() + np.abs(got[2] - want[2]).sum())
        print("band [%g, %g] ground_only %s: counted %d, unref %d, |difference| %d, near points %d"
              % (h_min, h_max, ground_only, got[0].sum(), got[2].sum(), moved, near.sum()))
        assert moved <= 2 * MAX_EDGE_POINTS
        assert set(np.flatnonzero((dc | du).reshape(-1)).tolist()) <= near_cells, "a cell differs that holds no point next to a bin edge"
        same = ~dc
        assert og.same_images(got[1][same], want[1][same]), "top differs in a cell whose count agrees"
        assert got[0].sum() > 5000 and got[2].sum() > 0
        if (h_min, h_max) == (0.2, 2.5):
            if ground_only:  # (the frame has non-ground points in patches that PWPP_GRID_GROUND_ONLY hides)
                assert got[2].sum() > plain[2].sum() and np.array_equal(got[0] + got[2] >= plain[0] + plain[2], np.ones((ny, nx), bool))
            plain = got


# ---- independence of schedule ---------------------------------------------------------------------------------------------
GRID = (-40.0, -40.0, 1.25, 64, 64)
BAND = (0.2, 2.5)


def reference_images(frames, params=None):
    h = pwpp_hip.Handle(params)
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    first = as_bytes(images(h, *GRID, *BAND))
    assert first == as_bytes(images(h, *GRID, *BAND)), "two identical calls differ"
    return first


def test_orders_layouts_and_memory_kinds_give_the_same_images():
    frames = three_frames()
    want = reference_images(frames)
    assert np.frombuffer(want[0], np.int32).sum() > 300
    for order in (pwpp_hip.ORDER_SCATTER, pwpp_hip.ORDER_REFERENCE, pwpp_hip.ORDER_CLOUD):
        h = pwpp_hip.Handle()
        h.set_order(order)
        h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
        assert as_bytes(images(h, *GRID, *BAND)) == want, "output order %d" % order
    for layout in ("row4", "col4", "fields48"):
        exps = [expected_array(f, layout) for f in frames]
        for mem in ("host", "pinned_slab", "device"):
            placed = Placed([encode(e, layout, 3 + k) for k, e in enumerate(exps)], mem)
            try:
                h = pwpp_hip.Handle()
                submit(h, placed, layout, [len(e) for e in exps], pwpp_hip.MODE_FRESH)
                assert as_bytes(images(h, *GRID, *BAND)) == want, (layout, mem)  # (the input is alive: `placed`)
                placed.assert_unchanged()
            finally:
                placed.free()


def test_after_a_redo_arena_moves_streams_and_on_a_pipe(kitti):
    import torch
    frames = list(kitti[:3])
    want = reference_images(frames)
    # one-pass segments far too small: the frames are binned again when the raster lands the asynchronous call
    h = pwpp_hip.Handle()
    h.set_option("one_pass_scale", 0.02)
    tens = [device_tensor(f) for f in frames]
    ptrs, ns = [t.data_ptr() for t in tens], [f.shape[0] for f in frames]
    h.estimate_ground_batch_device(ptrs, ns)
    got = as_bytes(images(h, *GRID, *BAND))
    assert h.redo_stats()[1] > 0, "the overflow redo did not run"
    assert got == want
    # a pipe's handles
    pipe = pwpp_hip.Pipe(depth=2)
    try:
        batch = h.make_device_batch(ptrs, ns)
        for rep in range(3):
            hv = pipe.submit_device_batch(batch)
            assert as_bytes(images(hv, *GRID, *BAND)) == want, "pipe, submit %d" % rep
        pipe.drain()
    finally:
        pipe.close()
    del tens
    torch.cuda.synchronize()
    # the first step of three stateful streams = three fresh frames
    h = pwpp_hip.Handle()
    h.set_num_streams(3)
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_STREAMS)
    assert as_bytes(images(h, *GRID, *BAND)) == want
    # the overflow arena: one sector of a frame of 72 denser than the handle has seen (test_gpu_point_planes.py)
    rng = np.random.default_rng(11)
    a = np.arctan2(kitti[0][:, 1], kitti[0][:, 0])
    sel = np.where((a > 0.3) & (a < 0.6))[0]
    extra = kitti[0][rng.choice(sel, int(len(sel) * 0.4), replace=True)].copy()
    extra[:, :3] += rng.normal(0.0, 0.004, (len(extra), 3)).astype(F32)
    dense = np.ascontiguousarray(np.concatenate([kitti[0], extra]).astype(F32))
    base = [kitti[i % 6] for i in range(72)]
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(base, mode=pwpp_hip.MODE_FRESH)
    odd = list(base)
    odd[10] = dense
    h.estimate_ground_batch(odd, mode=pwpp_hip.MODE_FRESH)
    assert h.arena_stats()[0] >= 1 and h.redo_stats()[1] == 0
    got = as_bytes(images(h, *GRID, *BAND, frame_first=9, frames=3))
    assert got == reference_images(odd[9:12])


# ---- input transform ----------------------------------------------------------------------------------------------------------
def test_with_an_input_transform():
    import input_transform_ref as xf
    T = xf.rigid(np.radians(3.0), np.radians(-5.0), np.radians(20.0), t=(0.2, -0.1, 0.15))
    level = three_frames()
    sensor = [np.ascontiguousarray(xf.transform_cloud(xf.inverse(T), c), F32) if len(c) else c for c in level]
    pre = []
    for c in sensor:
        t = c.copy()
        if len(c):
            t[:, :3] = pwpp_hip.transform_points(T, c[:, :3])
        pre.append(t)
    on = pwpp_hip.Handle()
    on.set_input_transforms(T)
    on.estimate_ground_batch(sensor, mode=pwpp_hip.MODE_FRESH)
    want = reference_images(pre)
    assert as_bytes(images(on, *GRID, *BAND)) == want
    assert np.frombuffer(want[0], np.int32).sum() > 300
    assert want != reference_images(sensor)  # (the tilt matters: the untransformed cloud gives other images)


# ---- memory kinds -----------------------------------------------------------------------------------------------------------
def test_memory_kinds_agree():
    import torch
    frames = [small_cloud(5), small_cloud(6)[:1500], inner_cloud(), small_cloud(8)]
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    for nx, ny, cell in ((64, 64, 1.25), (7, 5, 3.0), (257, 3, 0.5), (1, 1, 300.0)):
        x0, y0 = -0.5 * nx * cell, -0.5 * ny * cell
        full = images(h, x0, y0, cell, nx, ny, *BAND)
        for first, count in ((0, 4), (1, 2), (3, 1)):
            host = images(h, x0, y0, cell, nx, ny, *BAND, frame_first=first, frames=count)
            for a, b in zip(host, full):
                assert a.tobytes() == b[first:first + count].tobytes(), "a sub-range differs from the full range's slice"
            # a NULL top or unref leaves the other images unchanged
            assert h.rasterize_obstacles(x0, y0, cell, nx, ny, *BAND, first, count, want_top=False).tobytes() == host[0].tobytes()
            c2, u2 = h.rasterize_obstacles(x0, y0, cell, nx, ny, *BAND, first, count, want_top=False, want_unref=True)
            c3, t3 = h.rasterize_obstacles(x0, y0, cell, nx, ny, *BAND, first, count)
            assert as_bytes((c2, u2)) == as_bytes((host[0], host[2])) and as_bytes((c3, t3)) == as_bytes(host[:2])
            # device outputs, 4 bytes off a 16-byte boundary, with poisoned words on either side
            n = count * ny * nx
            dev = [torch.full((n + 7,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
            assert all(d.data_ptr() % 16 == 0 for d in dev)
            for shift, with_top, with_unref in ((1, True, True), (0, True, False), (3, False, True), (2, False, False)):
                for d in dev:
                    d.fill_(-7)
                torch.cuda.synchronize()
                ptr = [d.data_ptr() + 4 * shift for d in dev]
                h.rasterize_obstacles_device(x0, y0, cell, nx, ny, *BAND, ptr[0], ptr[1] if with_top else 0, ptr[2] if with_unref else 0,
                                             first, count)
                h.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
                raw = [d.cpu().numpy() for d in dev]
                for k, used in enumerate((True, with_top, with_unref)):
                    body = raw[k][shift:shift + n]
                    if used:
                        assert body.tobytes() == host[k].tobytes(), "device image %d, shift %d" % (k, shift)
                        assert (raw[k][:shift] == -7).all() and (raw[k][shift + n:] == -7).all(), "a word outside the image was written"
                    else:
                        assert (raw[k] == -7).all()


# ---- state and arguments ----------------------------------------------------------------------------------------------------
def test_state_and_arguments():
    L = pwpp_hip.load()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    cnt, top = np.zeros(3 * 16, np.int32), np.zeros(3 * 16, F32)
    grid = lambda **kw: pwpp_hip.GroundGrid(**dict(dict(x0=-2.0, y0=-2.0, cell=1.0, nx=4, ny=4, flags=0, pad_=0), **kw))

    def raster(h, g, first=0, frames=1, mem=pwpp_hip.MEM_HOST, band=(0.2, 2.5), c=cnt, t=top):
        return L.pwpp_rasterize_obstacles(h._h, ctypes.byref(g) if g is not None else None, band[0], band[1], first, frames, mem, vp(c), vp(t), None)

    h = pwpp_hip.Handle()
    assert raster(h, grid()) == E_STATE  # before any call
    frames = three_frames()
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert raster(h, grid(), 0, 3) == 0 and raster(h, grid(), 2, 1) == 0 and raster(h, grid(), t=None) == 0
    assert raster(h, None) == E_ARG and raster(h, grid(), c=None) == E_ARG
    for bad in (dict(nx=0), dict(ny=0), dict(nx=-3), dict(cell=0.0), dict(cell=-1.0), dict(cell=np.nan), dict(cell=np.inf), dict(x0=np.nan),
                dict(flags=2), dict(flags=3), dict(flags=-1)):
        assert raster(h, grid(**bad)) == E_ARG, bad
    assert raster(h, grid(flags=pwpp_hip.GRID_GROUND_ONLY)) == 0
    for first, count in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2), (0, -1)):
        assert raster(h, grid(), first, count) == E_ARG, (first, count)
    assert raster(h, grid(nx=1 << 16, ny=1 << 15), 0, 2) == E_ARG  # 2^32 cells; nothing is written before the check
    assert raster(h, grid(), mem=pwpp_hip.MEM_HOST_PINNED) == E_ARG and raster(h, grid(), mem=7) == E_ARG
    for band in ((np.nan, 1.0), (0.0, np.nan), (np.nan, np.nan), (1.0, 0.5), (INF, -INF)):
        assert raster(h, grid(), band=band) == E_ARG, band
    for band in ((-INF, INF), (1.0, 1.0), (INF, INF), (-INF, -INF)):
        assert raster(h, grid(), band=band) == 0, band
    # the workspace: the staging buffer of the ground queries, nothing of its own
    a, b = pwpp_hip.Handle(), pwpp_hip.Handle()
    for w in (a, b):
        w.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert a.workspace_bytes() == b.workspace_bytes()
    a.rasterize_ground(-20.0, -20.0, 0.5, 80, 80, with_patches=True)
    b.rasterize_obstacles(-20.0, -20.0, 0.5, 80, 80, 0.2, 2.5, want_top=False, want_unref=True)
    assert a.workspace_bytes() == b.workspace_bytes()
    a.trim_workspace()
    b.trim_workspace()
    assert a.workspace_bytes() == b.workspace_bytes()
    h.trim_workspace()
    assert raster(h, grid()) == E_STATE and b"no frame" in L.pwpp_last_error()
    h.estimate_ground_batch(frames[:1], mode=pwpp_hip.MODE_FRESH)
    assert raster(h, grid()) == 0 and raster(h, grid(), 1, 1) == E_ARG  # (the last call had one frame)


# ---- nothing else moves ---------------------------------------------------------------------------------------------------
def _everything(h, frames):
    out = []
    for i in range(frames):
        out.append((h.ground_indices(i).tobytes(), h.nonground_indices(i).tobytes(), h.counts(i), h.patch_records(i).tobytes(),
                    h.centers(i).tobytes(), h.normals(i).tobytes(), h.labels(i).tobytes()))
    for s in range(frames):
        out.append((bytes(h.state(s)), np.asarray(h.plane_state(s)).tobytes(),
                    b"".join(h.history(s, w, r).tobytes() for w in (0, 1) for r in range(4))))
    return out


def test_nothing_else_moves():
    first, second = [small_cloud(s) for s in (5, 6, 7)], [small_cloud(s) for s in (8, 9, 10)]
    h = pwpp_hip.Handle()
    h.set_order(pwpp_hip.ORDER_CLOUD)
    h.set_num_streams(3)
    h.estimate_ground_batch(first, mode=pwpp_hip.MODE_STREAMS)
    before = _everything(h, 3)
    imgs = images(h, -20.0, -20.0, 0.5, 80, 80, 0.2, 2.5, ground_only=True)
    assert imgs[0].sum() > 100
    assert _everything(h, 3) == before, "a raster changed the results of the call it reads"
    h.estimate_ground_batch(second, mode=pwpp_hip.MODE_STREAMS)
    asked = _everything(h, 3)
    ref = pwpp_hip.Handle()
    ref.set_order(pwpp_hip.ORDER_CLOUD)
    ref.set_num_streams(3)
    ref.estimate_ground_batch(first, mode=pwpp_hip.MODE_STREAMS)
    ref.estimate_ground_batch(second, mode=pwpp_hip.MODE_STREAMS)
    assert _everything(ref, 3) == asked, "a raster between two calls changed the second call's outputs"


# ---- bindings -----------------------------------------------------------------------------------------------------------------
def test_pybind_module_and_ctypes_handle_agree_with_the_c_call():
    import pypatchworkpp
    pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    h = pwpp_hip.Handle()
    L = pwpp_hip.load()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    with pytest.raises(RuntimeError):
        pp.getObstacleMap(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5)  # no frame yet
    pts = small_cloud(5)
    pp.estimateGround(pts)
    h.estimate_ground(pts)
    for ground_only in (False, True):
        g = pwpp_hip.GroundGrid(-30.0, -12.0, 0.5, 120, 48, pwpp_hip.GRID_GROUND_ONLY if ground_only else 0, 0)
        cc, ct = np.zeros((48, 120), np.int32), np.zeros((48, 120), F32)
        assert L.pwpp_rasterize_obstacles(h._h, ctypes.byref(g), 0.2, 2.5, 0, 1, pwpp_hip.MEM_HOST, vp(cc), vp(ct), None) == 0
        count, top = pp.getObstacleMap(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5, ground_only)
        assert count.dtype == np.int32 and top.dtype == F32 and count.shape == top.shape == (48, 120)
        assert count.tobytes() == cc.tobytes() and top.tobytes() == ct.tobytes()
        hc, ht = h.rasterize_obstacles(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5, ground_only=ground_only)
        assert hc[0].tobytes() == cc.tobytes() and ht[0].tobytes() == ct.tobytes()
    assert cc.sum() > 100
    with pytest.raises(RuntimeError):
        pp.getObstacleMap(0.0, 0.0, 0.0, 4, 4, 0.2, 2.5)
    with pytest.raises(RuntimeError):
        pp.getObstacleMap(0.0, 0.0, 1.0, 4, 4, 2.5, 0.2)
