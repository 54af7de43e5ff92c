"""The terrain analysis (pwpp_terrain_grid, pwpp_terrain_ground) on a real MI355X, byte for byte against the restatement of
tests/terrain_ref.py -- the bits of step, slope and rough, count and cost of whole images compared, no tolerance, for every value of
the option "terrain_path".  The kernel's tile is 32 x 8 cells (PWPP_TERRAIN_TILE_X, _Y), and the shapes are written for it: 1 x 1,
1 x 9 and 9 x 1, one short of, equal to and one past the tile in each direction separately and together, two tiles plus one, and
70 x 67 x 3 (ragged last tiles; a halo that crosses rows and frames in memory and must not read across them).  Radii 1 to 4, cells of
0.5, 0.3 and 2^-3, min_known 1, 3 and (2r+1)^2, finite and infinite limits, holes of 0, 30 and 90 per cent, a frame that is all NaN,
limit heights, 1023.9 beside -1023.9, host memory and device memory with arrays misaligned to their minimum in poisoned
surroundings, every pattern of absent outputs that matters, the overlaps, pwpp_terrain_ground against rasterize-then-analyse,
fusedTerrain, two device calls back to back, the workspace, and that asking changes nothing else."""
import ctypes
import functools

import numpy as np
import pytest

import pwpp_hip
import terrain_ref as tr
from test_gpu_obstacle_grid import _everything, small_cloud, three_frames

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
TX, TY = 32, 8  # the kernel's tile
SHAPES = [(1, 1, 1), (1, 9, 1), (9, 1, 1), (TX - 1, TY, 1), (TX, TY, 1), (TX + 1, TY, 1), (TX, TY - 1, 1), (TX, TY + 1, 1), (TX - 1, TY - 1, 1),
          (TX + 1, TY + 1, 1), (2 * TX + 1, 2 * TY + 1, 1), (70, 67, 3)]  # (nx, ny, frames)
RADII = (1, 2, 3, 4)
CELLS = (0.5, 0.3, 0.125)
LIMITS = ((0.2, 0.3, 0.05), (tr.INF, tr.INF, tr.INF), (tr.INF, 0.5, tr.INF), (1.0, tr.INF, 0.01))
PATHS = (0, 1, 2)
DTYPES = (np.float32, np.float32, np.float32, np.uint8, np.int8)
shape_ids = lambda s: "%dx%dx%d" % s


def params_of(r, min_known, limits):
    return pwpp_hip.TerrainParams(int(r), int(min_known), float(limits[0]), float(limits[1]), float(limits[2]), 0)


@functools.lru_cache(maxsize=None)
def case(nx, ny, frames, r, k):
    """The image, the parameters and the expected outputs of one combination: computed once, shared, never written.  k rotates the
    cell size, min_known, the limits, the holes and whether limit heights are among the cells."""
    cell, limits = CELLS[k % 3], LIMITS[k % 4]
    min_known = (1, 3, (2 * r + 1) ** 2)[(k // 2) % 3]
    h = np.concatenate([tr.random_heights(1, ny, nx, 100 * k + f, holes=(0.3, 0.0, 0.9)[(k + f) % 3], limits=(k + f) % 2 == 1) for f in range(frames)])
    want = tr.terrain(h, cell, r, min_known, *limits)
    for a in (h,) + want:
        a.setflags(write=False)
    return h, cell, r, min_known, limits, want


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()  # (no estimate call: pwpp_terrain_grid needs the handle's stream and buffer only)


def all_paths(h, call):
    """call() at "terrain_path" 0, 1 and 2: identical bytes; returns them."""
    res = []
    for path in PATHS:
        h.set_option("terrain_path", path)
        res.append(call())
    h.set_option("terrain_path", 0)
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert (a is None and b is None) or a.tobytes() == b.tobytes(), "the values of terrain_path differ"
    return res[0]


def check(got, want, what, wanted=(True,) * 5):
    for name, g, w, dt, on in zip(tr.NAMES, got, want, DTYPES, wanted):
        if not on:
            assert g is None, what
            continue
        assert g.dtype == dt and g.shape == w.shape, "%s: %s" % (what, name)
        if g.tobytes() != w.tobytes():
            gb, wb = (g.view(np.uint32), w.view(np.uint32)) if dt == np.float32 else (g, w)
            bad = np.argwhere(gb != wb)
            assert False, "%s: %d cells of %s differ, the first %s: %r, expected %r" % (what, len(bad), name, bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


def on_host(h, hgt, cell, r, min_known, limits, wanted=(True,) * 5):
    return h.terrain_grid(hgt, cell, params_of(r, min_known, limits), *wanted)


def on_device(h, hgt, cell, r, min_known, limits, wanted=(True,) * 5, off=1):
    """terrain_grid on device arrays; every array starts `off` of its own elements behind a 256-byte boundary -- 4 bytes for the
    floats, 1 for the bytes: their minimum; what surrounds them is poisoned and must survive, the heights must not be written."""
    import torch
    frames, ny, nx = hgt.shape
    cells = hgt.size
    dh = torch.full((cells + 128,), -77.0, dtype=torch.float32, device="cuda")
    outs = [torch.full((cells + 128,), -7, dtype=torch.int32 if dt == np.float32 else torch.int8, device="cuda") for dt in DTYPES]
    assert all(b.data_ptr() % 256 == 0 for b in outs + [dh])
    dh[off:off + cells] = torch.from_numpy(hgt.reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    ptrs = [(b.data_ptr() + off * b.element_size()) if on else 0 for b, on in zip(outs, wanted)]
    h.terrain_grid_device(nx, ny, frames, cell, dh.data_ptr() + 4 * off, params_of(r, min_known, limits), *ptrs)
    h.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
    rh = dh.cpu().numpy()
    assert (rh[:off] == -77).all() and (rh[off + cells:] == -77).all() and rh[off:off + cells].tobytes() == hgt.tobytes(), "the heights were written"
    got = []
    for b, dt, on in zip(outs, DTYPES, wanted):
        raw = b.cpu().numpy()
        assert (raw[:off] == -7).all() and (raw[off + cells:] == -7).all(), "an element outside an image was written"
        if not on:
            assert (raw == -7).all(), "an output that was not asked for was written"
        got.append(raw[off:off + cells].view(dt).reshape(hgt.shape) if on else None)
    return tuple(got)


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_shapes_and_radii_against_the_reference(handle, shape, r):
    k = SHAPES.index(shape) + 5 * r
    args = case(*shape, r, k)
    what = "%s r %d k %d" % (shape_ids(shape), r, k)
    check(all_paths(handle, lambda: on_host(handle, *args[:-1])), args[-1], what + " (host)")
    if shape[0] * shape[1] >= TX * TY:
        check(all_paths(handle, lambda: on_device(handle, *args[:-1])), args[-1], what + " (device)")


@pytest.mark.parametrize("r", RADII)
def test_every_cell_size_min_known_and_limit(handle, r):
    """On one image of several tiles: the three cell sizes, the three values of min_known and the four sets of limits, crossed."""
    h = case(45, 19, 1, r, 1)[0]
    for cell in CELLS:
        for min_known in (1, 3, (2 * r + 1) ** 2):
            for limits in LIMITS:
                want = tr.terrain(h, cell, r, min_known, *limits)
                check(on_host(handle, h, cell, r, min_known, limits), want, "cell %g min_known %d limits %s" % (cell, min_known, limits))


@pytest.mark.parametrize("r", (1, 4))
def test_a_frame_that_is_all_nan_and_the_largest_moments(handle, r):
    ny, nx = 19, 37
    yy, xx = np.mgrid[0:ny, 0:nx]
    h = np.stack([tr.random_heights(1, ny, nx, 5)[0], np.full((ny, nx), np.nan, np.float32),
                  np.where((xx + yy) % 2 == 0, 1023.9, -1023.9).astype(np.float32),      # the largest N
                  np.where(xx < nx // 2, 1024.0, -1024.0).astype(np.float32),             # the largest |Cxz| at the edge
                  tr.random_heights(1, ny, nx, 6, holes=0.5, limits=True)[0]])
    want = tr.terrain(h, 0.5, r, 3, 500.0, 1e4, 900.0)
    assert (want[3][1] == 0).all() and (want[4][1] == -1).all() and want[2][2].max() > 1000.0
    check(all_paths(handle, lambda: on_host(handle, h, 0.5, r, 3, (500.0, 1e4, 900.0))), want, "extremes (host)")
    check(all_paths(handle, lambda: on_device(handle, h, 0.5, r, 3, (500.0, 1e4, 900.0))), want, "extremes (device)")


def test_every_pattern_of_absent_outputs(handle):
    args = case(70, 67, 3, 2, 3)
    patterns = [tuple(i == j for i in range(5)) for j in range(5)] + [(True, False, True, False, True), (False, True, False, True, False)]
    for wanted in patterns:
        what = "outputs %s" % (wanted,)
        check(all_paths(handle, lambda: on_host(handle, *args[:-1], wanted)), args[-1], what + " (host)", wanted)
        check(all_paths(handle, lambda: on_device(handle, *args[:-1], wanted)), args[-1], what + " (device)", wanted)
    with pytest.raises(pwpp_hip.PwppError):
        on_host(handle, *args[:-1], (False,) * 5)
    assert b"null outputs" in pwpp_hip.load().pwpp_last_error()


def test_overlaps_and_alignment_are_refused_with_a_live_handle(handle):
    L = pwpp_hip.load()
    vp = lambda a, n=0: ctypes.c_void_p(a.ctypes.data + n)
    h = np.zeros(64, np.float32)
    f = [np.zeros(64, np.float32) for _ in range(3)]
    b = [np.zeros(64, np.uint8) for _ in range(2)]
    p = params_of(1, 3, LIMITS[0])
    call = lambda height, step, slope, rough, count, cost, mem=pwpp_hip.MEM_HOST: L.pwpp_terrain_grid(handle._h, 8, 8, 1, 0.5, mem, height, ctypes.byref(p), step,
                                                                                                    slope, rough, count, cost)
    assert call(vp(h), vp(h), None, None, None, None) == E_ARG and b"height and step overlap" in L.pwpp_last_error()
    assert call(vp(h), vp(f[0]), vp(f[0], 252), None, None, None) == E_ARG and b"step and slope overlap" in L.pwpp_last_error()
    assert call(vp(h), None, None, vp(f[2]), vp(f[2], 255), None) == E_ARG and b"rough and count overlap" in L.pwpp_last_error()
    assert call(vp(h), None, None, None, vp(b[0]), vp(b[0], 63)) == E_ARG and b"count and cost overlap" in L.pwpp_last_error()
    assert call(vp(h), None, None, None, None, vp(h, 100)) == E_ARG and b"height and cost overlap" in L.pwpp_last_error()
    assert call(ctypes.c_void_p(4098), ctypes.c_void_p(8192), None, None, None, None, pwpp_hip.MEM_DEVICE) == E_ARG and b"4-byte aligned" in L.pwpp_last_error()
    assert call(vp(h), vp(f[0]), vp(f[1]), vp(f[2]), vp(b[0]), vp(b[1])) == 0   # and nothing of it is sticky
    with pytest.raises(pwpp_hip.PwppError):
        handle.set_option("terrain_path", 3)


# ---- pwpp_terrain_ground -------------------------------------------------------------------------------------------------------
def test_terrain_ground_is_rasterize_ground_plus_terrain_grid():
    import torch
    nx, ny, cell = 120, 96, 0.5
    x0, y0 = -30.0, -24.0
    limits = (0.3, 0.4, 0.05)
    p = params_of(2, 5, limits)
    L = pwpp_hip.load()
    h = pwpp_hip.Handle()
    g = pwpp_hip.GroundGrid(x0, y0, cell, nx, ny, 0, 0)
    cost = np.zeros(nx * ny, np.int8)
    assert L.pwpp_terrain_ground(h._h, ctypes.byref(g), 0, 1, pwpp_hip.MEM_HOST, ctypes.byref(p), None, None, None, None,
                                 cost.ctypes.data_as(ctypes.c_void_p), None) == E_STATE
    h.set_labels(True)  # (_everything reads them)
    h.estimate_ground(small_cloud(5))
    before = _everything(h, 1)
    for ground_only in (False, True):
        what = "ground_only %s" % ground_only
        img = h.rasterize_ground(x0, y0, cell, nx, ny, ground_only=ground_only)
        assert np.isfinite(img).sum() > 200 and np.isnan(img).any()
        steps = h.terrain_grid(img, cell, p)
        got = all_paths(h, lambda: h.terrain_ground(x0, y0, cell, nx, ny, p, ground_only=ground_only, want_frames=True))
        assert got[5].tobytes() == img.tobytes(), what + ": the per-frame images differ from pwpp_rasterize_ground's"
        check(got[:5], steps, what + ": differs from the two steps")
        check(h.terrain_ground(x0, y0, cell, nx, ny, p, ground_only=ground_only), steps, what + ": the images kept in the handle")
        check(got[:5], tr.terrain(img, cell, 2, 5, *limits), what)
        assert (got[4] >= 0).sum() > 100
    # into device memory at the minimum alignment, the frames' images kept and asked for
    cells = nx * ny
    outs = [torch.full((cells + 128,), -7, dtype=torch.int32 if dt == np.float32 else torch.int8, device="cuda") for dt in DTYPES]
    dh = torch.full((cells + 128,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for h_ptr in (0, dh.data_ptr() + 4):
        h.terrain_ground_device(x0, y0, cell, nx, ny, p, *([b.data_ptr() + b.element_size() for b in outs] + [h_ptr]), ground_only=True)
        h.synchronize()
        for b, w in zip(outs, got[:5]):
            raw = b.cpu().numpy()
            assert raw[1:1 + cells].tobytes() == w.tobytes() and raw[0] == -7 and (raw[1 + cells:] == -7).all()
    rh = dh.cpu().numpy()
    assert rh[1:1 + cells].tobytes() == img.tobytes() and rh[0] == -7 and (rh[1 + cells:] == -7).all()
    assert _everything(h, 1) == before, "the terrain analysis changed the results of the call it reads"


def test_three_frames_of_a_batch_and_a_sub_range():
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(three_frames(), mode=pwpp_hip.MODE_FRESH)  # a 16-beam scan, an empty frame, a frame that is all unref
    grid = (-16.0, -16.0, 0.5, 64, 64)
    p = params_of(1, 3, LIMITS[0])
    img = h.rasterize_ground(*grid)
    got = all_paths(h, lambda: h.terrain_ground(*grid, p))
    check(got, tr.terrain(img, 0.5, 1, 3, *LIMITS[0]), "three frames")
    assert (got[3][0] > 0).sum() > 100 and not got[3][1].any()  # the empty frame has no ground
    sub = h.terrain_ground(*grid, p, frame_first=1, frames=2)
    assert all(a.tobytes() == b[1:].tobytes() for a, b in zip(sub, got))


def test_two_device_calls_back_to_back_each_under_their_own_parameters():
    """The parameters travel in the launch: two calls with different ones on the same heights, one synchronize() after both."""
    import torch
    h = pwpp_hip.Handle()
    hgt = case(70, 67, 3, 2, 3)[0]
    calls = [(0.5, 1, 3, LIMITS[0]), (0.3, 4, 40, LIMITS[3])]
    want = [tr.terrain(hgt, cell, r, mk, *lim) for cell, r, mk, lim in calls]
    assert want[0][4].tobytes() != want[1][4].tobytes()
    dh = torch.from_numpy(hgt.copy()).cuda()
    out = [[torch.full((hgt.size,), -7, dtype=torch.int32 if dt == np.float32 else torch.int8, device="cuda") for dt in DTYPES] for _ in calls]
    torch.cuda.synchronize()
    for (cell, r, mk, lim), o in zip(calls, out):
        h.terrain_grid_device(70, 67, 3, cell, dh.data_ptr(), params_of(r, mk, lim), *[b.data_ptr() for b in o])
    h.synchronize()
    for i, o in enumerate(out):
        check(tuple(b.cpu().numpy().view(dt).reshape(hgt.shape) for b, dt in zip(o, DTYPES)), want[i], "call %d of two" % i)


# ---- workspace ------------------------------------------------------------------------------------------------------------------
def test_workspace_and_that_nothing_else_moves():
    h = pwpp_hip.Handle()
    empty = h.workspace_bytes()
    args = case(70, 67, 3, 2, 3)
    cells = args[0].size
    check(on_host(h, *args[:-1]), args[-1], "before any estimate call")
    grown = h.workspace_bytes()
    assert grown >= empty + 4 * cells * 4 + 2 * cells, "the cluster buffer is not counted"   # the staged heights, three float images, two byte images
    h.trim_workspace()
    assert h.workspace_bytes() == empty, "pwpp_trim_workspace did not free the cluster buffer"
    # with the feature unused nothing is allocated; with it used nothing of the estimate path moves
    a, b = pwpp_hip.Handle(), pwpp_hip.Handle()
    frames = three_frames()
    for w in (a, b):
        w.set_labels(True)
        w.set_order(pwpp_hip.ORDER_CLOUD)  # (a deterministic order of the index lists: two calls are compared below)
        w.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert a.workspace_bytes() == b.workspace_bytes()
    before, t_before = _everything(b, 3), b.time_us()
    b.terrain_ground(-20.0, -20.0, 0.5, 80, 80, params_of(2, 3, LIMITS[0]))
    assert b.workspace_bytes() >= a.workspace_bytes() + 4 * 3 * 80 * 80  # the kept height images
    assert _everything(b, 3) == before and b.time_us() == t_before, "the terrain analysis changed the results of the call it reads"
    for w in (a, b):
        w.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert _everything(b, 3) == _everything(a, 3), "an estimate call after a terrain call differs from one without"
    b.trim_workspace()
    a.trim_workspace()
    assert a.workspace_bytes() == b.workspace_bytes()


def test_pybind_module_agrees_with_the_ctypes_handle():
    import pypatchworkpp
    pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    h = pwpp_hip.Handle()
    tp = pypatchworkpp.TerrainParams()
    with pytest.raises(RuntimeError):
        pp.getTerrain(-30.0, -12.0, 0.5, 120, 48)  # no frame yet
    m = pypatchworkpp.FusedElevationMap()
    m.x0, m.y0, m.cell, m.nx, m.ny, m.n_max = -32.0, -14.0, 0.5, 130, 56, 4
    with pytest.raises(ValueError):
        pp.fusedTerrain(m)  # no mean yet
    pose = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    for seed in (5, 6, 7):   # a map fused from three frames
        pts = small_cloud(seed)
        pp.estimateGround(pts)
        h.estimate_ground(pts)   # (the same sequence: what ground_only blanks depends on the frames before)
        _, _, mean = pp.updateElevationMap(m, pose, 0.0, -30.0, -12.0, 0.5, 120, 48)
    names = ("step", "slope", "rough", "count", "cost")
    got = pp.getTerrain(-30.0, -12.0, 0.5, 120, 48)   # the defaults: radius 1, min_known 3, every limit infinite
    want = h.terrain_ground(-30.0, -12.0, 0.5, 120, 48, params_of(1, 3, LIMITS[1]))
    for n, g, w, dt in zip(names, got, want, DTYPES):
        assert g.dtype == dt and g.shape == (48, 120) and g.tobytes() == w[0].tobytes(), n
    assert set(np.unique(got[4]).tolist()) == {-1, 0}
    tp.radius, tp.min_known, tp.step_max, tp.slope_max, tp.rough_max = 2, 6, 0.3, 0.4, 0.05
    got = pp.fusedTerrain(m, tp)
    want = h.terrain_grid(mean, 0.5, params_of(2, 6, (0.3, 0.4, 0.05)))
    for n, g, w, dt in zip(names, got, want, DTYPES):
        assert g.dtype == dt and g.shape == (56, 130) and g.tobytes() == w.tobytes(), n
    check(want, tr.terrain(mean, 0.5, 2, 6, 0.3, 0.4, 0.05), "the fused mean")
    assert (got[4] >= 0).sum() > 100
    got = pp.getTerrain(-30.0, -12.0, 0.5, 120, 48, tp, True)
    want = h.terrain_ground(-30.0, -12.0, 0.5, 120, 48, params_of(2, 6, (0.3, 0.4, 0.05)), ground_only=True)
    assert all(g.tobytes() == w[0].tobytes() for g, w in zip(got, want))
