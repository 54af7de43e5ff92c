"""The cost-to-reach field (pwpp_reach_grid, pwpp_reach_ground) on a real MI355X, exactly equal -- reach and from -- to the heap
Dijkstra of tests/reach_ref.py, for host and device memory (the byte images at odd addresses, the int32 images at their minimum
alignment) and for every value of the option "reach_path".  The tiled kernel's tile is PWPP_REACH_TILE_X x _Y cells, read from
csrc/pwpp_reach.h, and the shapes are written for it: 1 x 1, 1 x N and N x 1, a tile exactly and one cell more or fewer each way, 2 x 2
and 3 x 3 tiles with ragged edges; 96 x 96 for the corridors, whose paths cross tile borders many times.  References are computed once
and shared.

This file stops at 9 tiles and 64 frames: the tiled kernel's dirty bits fit one word of 32 here and a call is one launch.  Frames of 34 to
257 tiles, whose bits fill 2 to 9 words, and a call of more than 2^22 frames, which is cut into several launches, are in
tests/test_gpu_reach_large.py."""
import ctypes
import functools

import numpy as np
import pytest

import pwpp_hip
import reach_ref as rr
from test_gpu_obstacle_grid import _everything, small_cloud, three_frames
from test_reach_cpu import TILE_X as TX, TILE_Y as TY

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
PATHS = (0, 1, 2)
SHAPES = [(1, 1), (1, 9), (9, 1), (1, 2 * TY + 3), (2 * TX + 3, 1), (TX, TY), (TX - 1, TY), (TX + 1, TY), (TX, TY - 1), (TX, TY + 1), (TX - 1, TY - 1),
          (TX + 1, TY + 1), (2 * TX - 5, 2 * TY - 7), (3 * TX - 3, 3 * TY - 11)]  # (nx, ny)
shape_ids = lambda s: "%dx%d" % s


def params_of(p):
    return pwpp_hip.ReachParams(p["base"], p["lethal"], p["unknown"], p["clearance2"], p["max_reach"], 0)


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()  # (no estimate call: pwpp_reach_grid needs the handle's stream and buffer only)


def on_host(h, cost, src, p, dist2=None):
    return h.reach_grid(cost, src, params_of(p), dist2=dist2)


def on_device(h, cost, src, p, dist2=None):
    """reach_grid on device arrays: the cost bytes start 1 byte, the int32 images 4 bytes behind a 256-byte boundary -- their minimum;
    what surrounds them is poisoned and must survive, and the inputs must not be written."""
    import torch
    c3 = cost.reshape((-1,) + cost.shape[-2:])
    frames, ny, nx = c3.shape
    cells = c3.size
    dc = torch.full((cells + 128,), -7, dtype=torch.int8, device="cuda")
    dd, dr, df = (torch.full((cells + 128,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    assert all(b.data_ptr() % 256 == 0 for b in (dc, dd, dr, df))
    dc[1:1 + cells] = torch.from_numpy(c3.reshape(-1).copy()).cuda()
    if dist2 is not None:
        dd[1:1 + cells] = torch.from_numpy(np.ascontiguousarray(dist2, np.int32).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    h.reach_grid_device(nx, ny, frames, dc.data_ptr() + 1, src, params_of(p), dr.data_ptr() + 4, df.data_ptr() + 4,
                        dd.data_ptr() + 4 if dist2 is not None else 0)
    h.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
    rc, rd = dc.cpu().numpy(), dd.cpu().numpy()
    assert rc[0] == -7 and (rc[1 + cells:] == -7).all() and rc[1:1 + cells].tobytes() == c3.tobytes(), "the cost bytes were written"
    if dist2 is None:
        assert (rd == -7).all(), "a dist2 image that was not given was written"
    else:
        assert rd[0] == -7 and (rd[1 + cells:] == -7).all() and rd[1:1 + cells].tobytes() == np.ascontiguousarray(dist2, np.int32).tobytes()
    out = []
    for b in (dr, df):
        raw = b.cpu().numpy()
        assert raw[0] == -7 and (raw[1 + cells:] == -7).all(), "an element outside an image was written"
        out.append(raw[1:1 + cells].reshape(cost.shape))
    return tuple(out)


def same(got, want, what):
    for name, g, w in zip(("reach", "from"), got, want):
        assert g.dtype == np.int32 and g.shape == w.shape, "%s: %s" % (what, name)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            assert False, "%s: %d cells of %s differ, the first %s: %r, expected %r" % (what, len(bad), name, bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


def everywhere(h, cost, src, p, want, what, dist2=None):
    """Every path, in host and in device memory, against `want`."""
    for path in PATHS:
        h.set_option("reach_path", path)
        try:
            same(on_host(h, cost, src, p, dist2), want, "%s (host, path %d)" % (what, path))
            same(on_device(h, cost, src, p, dist2), want, "%s (device, path %d)" % (what, path))
        finally:
            h.set_option("reach_path", 0)


@functools.lru_cache(maxsize=None)
def shape_case(nx, ny):
    """A random image of two frames with walls and unknown cells, its sources and the expected fields: computed once, never written."""
    k = SHAPES.index((nx, ny))
    cost = rr.random_cost(2, ny, nx, 40 + k, lethal=0.12, unknown=0.08)
    src = np.array([[(nx - 1) // 2, (ny - 1) // 2], [nx - 1, 0]], np.int32)
    p = rr.params(base=1 + 9 * k, lethal=(100, 101, 90)[k % 3], unknown=(-1, 0, 60)[k % 3])
    want = rr.reach(cost, src, p)
    for a in (cost, src) + want:
        a.setflags(write=False)
    return cost, src, p, want


@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_shapes_against_the_reference(handle, shape):
    cost, src, p, want = shape_case(*shape)
    everywhere(handle, cost, src, p, want, shape_ids(shape))
    if shape[0] * shape[1] > 100:
        assert (want[0] != rr.NONE).sum() > shape[0] * shape[1] // 2


def test_the_option_is_checked(handle):
    with pytest.raises(Exception):
        handle.set_option("reach_path", 3)
    with pytest.raises(Exception):
        handle.set_option("reach_path", -1)


# ---- 96 x 96: corridors, sources, rules -----------------------------------------------------------------------------------------
N = 96
FREE = rr.params(base=2, lethal=100, unknown=-1)


@functools.lru_cache(maxsize=None)
def corridor(kind):
    cost = rr.serpentine(N, N) if kind == "serpentine" else rr.spiral(N)
    want = rr.reach(cost, (0, 0), FREE)
    for a in (cost,) + want:
        a.setflags(write=False)
    return cost, want


@pytest.mark.parametrize("kind", ["serpentine", "spiral"])
def test_a_corridor_across_the_tiles(handle, kind):
    """A path of about nx * ny / 2 steps that crosses tile borders many times: the worst case of every sweep schedule."""
    cost, want = corridor(kind)
    free = int((cost == 0).sum())
    # every step an edge of two free cells, 5 * (2 + 2): the path is as long as the corridor (the spiral's last turn ends in a 2 x 2 block)
    assert free > N * N // 2 - N and 20 * (free - 3) <= want[0][cost == 0].max() <= 20 * (free - 1)
    everywhere(handle, cost, (0, 0), FREE, want, kind)


@functools.lru_cache(maxsize=None)
def field():
    """A 96 x 96 image with walls, unknown cells and dear ground, shared by the cases below."""
    cost = rr.random_cost(1, N, N, 77, lethal=0.18, unknown=0.1)[0]
    cost.setflags(write=False)
    return cost


def test_a_source_in_each_corner_on_a_tile_border_and_on_an_impassable_cell(handle):
    cost = field().copy()
    wall = (TX, TY + 3)
    cost[wall[1], wall[0]] = 100
    cost.setflags(write=False)
    p = rr.params(base=3, unknown=20)
    for src in ((0, 0), (N - 1, 0), (0, N - 1), (N - 1, N - 1), (TX - 1, TY), (TX, TY - 1), (2 * TX, 2 * TY), wall):
        want = rr.reach(cost, src, p)
        assert want[0][src[1], src[0]] == 0 and (want[0] != rr.NONE).sum() > N * N // 2
        everywhere(handle, cost, src, p, want, "source %r" % (src,))


def test_a_sealed_source_a_diagonal_gap_and_a_one_cell_corridor(handle):
    p = rr.params(base=1)
    cost = np.zeros((N, N), np.int8)
    sx, sy = TX, TY - 1   # on a tile's corner
    cost[sy - 1:sy + 2, sx - 1:sx + 2] = 100
    want = rr.reach(cost, (sx, sy), p)
    assert (want[0] != rr.NONE).sum() == 1 and (want[1] >= 0).sum() == 1   # sealed: only the source, itself lethal
    everywhere(handle, cost, (sx, sy), p, want, "sealed")
    cost[sy - 1, sx - 1] = 0   # a diagonal gap across the tiles' corner: closed
    want = rr.reach(cost, (sx, sy), p)
    assert (want[0] != rr.NONE).sum() == 1
    everywhere(handle, cost, (sx, sy), p, want, "diagonal gap")
    cost[sy - 1, sx] = 0       # an edge: open
    want = rr.reach(cost, (sx, sy), p)
    assert (want[0] != rr.NONE).sum() == N * N - 6
    everywhere(handle, cost, (sx, sy), p, want, "edge gap")
    cost = np.full((N, N), 100, np.int8)   # a corridor one cell wide along a tile border, round a corner and back
    cost[TY, 2:N - 2] = 7
    cost[TY:N - 3, N - 3] = 9
    cost[N - 4, 5:N - 2] = -1
    q = rr.params(base=4, unknown=11)
    want = rr.reach(cost, (2, TY), q)
    assert (want[0] != rr.NONE).sum() == (cost != 100).sum() > 2 * N
    everywhere(handle, cost, (2, TY), q, want, "corridor")


def test_unknown_lethal_dist2_and_max_reach(handle):
    cost = field()
    src = (N // 2, N // 2)
    fields = {}
    for unknown in (-1, 0, 55, 100):
        p = rr.params(base=5, unknown=unknown)
        want = fields[unknown] = rr.reach(cost, src, p)
        everywhere(handle, cost, src, p, want, "unknown %d" % unknown)
    assert len({w[0].tobytes() for w in fields.values()}) == 3   # 100 is lethal at lethal = 100: as -1
    assert fields[-1][0].tobytes() == fields[100][0].tobytes()
    present = int(cost[(cost > 30) & (cost < 60)][0])
    seen = set()
    for lethal in (1, present, 101):
        p = rr.params(base=5, lethal=lethal, unknown=0)
        want = rr.reach(cost, src, p)
        seen.add(want[0].tobytes())
        everywhere(handle, cost, src, p, want, "lethal %d" % lethal)
    assert len(seen) == 3
    # dist2: random squared distances, PWPP_DIST_BEYOND among them
    rng = np.random.default_rng(9)
    d2 = rng.integers(0, 30, cost.shape).astype(np.int32)
    d2[rng.random(cost.shape) < 0.1] = rr.DIST_BEYOND
    seen = set()
    for clearance2 in (0, 4, 12):
        p = rr.params(base=5, unknown=0, clearance2=clearance2)
        want = rr.reach(cost, src, p, d2)
        seen.add(want[0].tobytes())
        everywhere(handle, cost, src, p, want, "clearance2 %d" % clearance2, dist2=d2)
    assert len(seen) == 3
    beyond = np.full(cost.shape, rr.DIST_BEYOND, np.int32)
    p = rr.params(base=5, unknown=0, clearance2=2 ** 31 - 2)
    want = rr.reach(cost, src, rr.params(base=5, unknown=0))   # PWPP_DIST_BEYOND everywhere blocks nothing
    everywhere(handle, cost, src, p, want, "dist2 beyond everywhere", dist2=beyond)
    # max_reach at an exact value of a cell and one below it
    free = fields[55]
    values = np.unique(free[0][free[0] != rr.NONE])
    v = int(values[len(values) // 3])
    for limit in (v, v - 1):
        p = rr.params(base=5, unknown=55, max_reach=limit)
        want = (np.where(free[0] <= limit, free[0], rr.NONE).astype(np.int32), np.where(free[0] <= limit, free[1], -1).astype(np.int32))
        same(rr.reach(cost, src, p), want, "the reference under max_reach %d" % limit)
        everywhere(handle, cost, src, p, want, "max_reach %d" % limit)
    assert ((free[0] == v).sum() >= 1) and (want[0] == v).sum() == 0


def test_uniform_open_fields_where_nearly_every_cell_has_tied_predecessors(handle):
    for c, base, src in ((0, 1, (0, 0)), (100, 255, (N - 1, N // 2)), (33, 7, (TX, TY))):
        cost = np.full((N, N), c, np.int8)
        p = rr.params(base=base, lethal=101)
        want = rr.reach(cost, src, p)
        yy, xx = np.mgrid[0:N, 0:N]
        dx, dy = abs(xx - src[0]), abs(yy - src[1])
        assert np.array_equal(want[0], 2 * (base + c) * (5 * np.maximum(dx, dy) + 2 * np.minimum(dx, dy)))
        everywhere(handle, cost, src, p, want, "uniform %d" % c)


def test_sixty_four_frames_with_their_own_sources_each_as_on_its_own(handle):
    n, frames = 40, 64
    rng = np.random.default_rng(12)
    cost = rr.random_cost(frames, n, n, 90, lethal=0.1, unknown=0.05)
    for f in range(0, frames, 2):   # alternately walled: a wall with one gap across the frame
        cost[f, n // 2, :] = 100
        cost[f, n // 2, (7 * f) % n] = 0
    src = np.stack([rng.integers(0, n, frames), rng.integers(0, n, frames)], axis=1).astype(np.int32)
    p = rr.params(base=2, unknown=30)
    want = rr.reach(cost, src, p)
    everywhere(handle, cost, src, p, want, "64 frames")
    for f in (0, 1, 31, 63):   # each frame's result equals its single-frame result
        one = handle.reach_grid(cost[f], src[f], params_of(p))
        same(one, (want[0][f], want[1][f]), "frame %d on its own" % f)
    again = handle.reach_grid(cost, src, params_of(p))   # repeated calls give the same bytes
    same(again, want, "a second call")
    # one source for all the frames
    want = rr.reach(cost[:5], (3, 4), p)
    everywhere(handle, cost[:5], (3, 4), p, want, "one source for five frames")
    # without from
    reach, frm = handle.reach_grid(cost[:5], (3, 4), params_of(p), want_from=False)
    assert frm is None and reach.tobytes() == want[0].tobytes()


def test_arguments_that_need_a_device_and_overlaps(handle):
    L = pwpp_hip.load()
    cost = np.zeros((4, 4), np.int8)
    with pytest.raises(Exception, match="outside"):
        handle.reach_grid(cost, (4, 0), params_of(FREE))
    with pytest.raises(Exception, match="sources"):
        handle.reach_grid(np.zeros((3, 4, 4), np.int8), [(0, 0), (1, 1)], params_of(FREE))
    reach = np.zeros(16, np.int32)
    src = np.zeros(2, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.pwpp_reach_grid(handle._h, 4, 4, 1, pwpp_hip.MEM_HOST, vp(cost), None, ctypes.byref(params_of(FREE)), vp(src), 1, vp(reach), vp(reach)) == E_ARG
    assert b"overlap" in L.pwpp_last_error()
    assert L.pwpp_reach_grid(handle._h, 4, 4, 1, 2, vp(cost), None, ctypes.byref(params_of(FREE)), vp(src), 1, vp(reach), None) == E_ARG   # PWPP_MEM_HOST_PINNED


# ---- pwpp_reach_ground ----------------------------------------------------------------------------------------------------------
def tparams():
    return pwpp_hip.TerrainParams(1, 3, 0.3, 0.4, 0.05, 0)


def ground_on_device(h, grid, n_frames, tp, p, source_xy, keep, **kw):
    """reach_ground into device arrays at their minimum alignment -- reach and from 4 bytes, the cost bytes (keep: not asked for) 1 byte
    behind a 256-byte boundary; what surrounds them is poisoned and must survive.  Returns (reach, from, cost or None), (n_frames, ny, nx)."""
    import torch
    nx, ny = grid[3], grid[4]
    cells = n_frames * nx * ny
    dr, df = (torch.full((cells + 128,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    dc = torch.full((cells + 128,), -7, dtype=torch.int8, device="cuda")
    assert all(b.data_ptr() % 256 == 0 for b in (dr, df, dc))
    torch.cuda.synchronize()
    h.reach_ground_device(*grid, tp, params_of(p), source_xy, dr.data_ptr() + 4, df.data_ptr() + 4, 0 if keep else dc.data_ptr() + 1, **kw)
    h.synchronize()
    out = []
    for b in (dr, df, dc):
        raw = b.cpu().numpy()
        assert raw[0] == -7 and (raw[1 + cells:] == -7).all(), "an element outside an image was written"
        out.append(raw[1:1 + cells].reshape(n_frames, ny, nx))
    assert not keep or (out[2] == -7).all(), "cost images that were not asked for were written"
    return out[0], out[1], None if keep else out[2]


def test_reach_ground_is_terrain_ground_plus_reach_grid():
    nx, ny, cell = 120, 96, 0.5
    x0, y0 = -30.0, -24.0
    tp, p = tparams(), rr.params(base=3, lethal=100, unknown=40)
    L = pwpp_hip.load()
    h = pwpp_hip.Handle()
    g = pwpp_hip.GroundGrid(x0, y0, cell, nx, ny, 0, 0)
    reach = np.zeros(nx * ny, np.int32)
    xy = np.zeros(2, np.float64)
    assert L.pwpp_reach_ground(h._h, ctypes.byref(g), 0, 1, pwpp_hip.MEM_HOST, ctypes.byref(tp), ctypes.byref(params_of(p)), xy.ctypes.data_as(ctypes.c_void_p), 1,
                               reach.ctypes.data_as(ctypes.c_void_p), None, None) == E_STATE
    h.set_labels(True)  # (_everything reads them)
    h.estimate_ground(small_cloud(5))
    before = _everything(h, 1)
    source_xy = (1.3, -2.2)
    src = (int(np.floor((source_xy[0] - x0) / cell)), int(np.floor((source_xy[1] - y0) / cell)))
    for ground_only in (False, True):
        what = "ground_only %s" % ground_only
        cost = h.terrain_ground(x0, y0, cell, nx, ny, tp, ground_only=ground_only)[4]
        assert (cost >= 0).sum() > 200 and (cost < 0).any()
        steps = h.reach_grid(cost, src, params_of(p))
        want = rr.reach(cost, src, p)
        same(steps, want, what + ": the two steps")
        assert (want[0] != rr.NONE).sum() > 500
        for path in PATHS:
            h.set_option("reach_path", path)
            got = h.reach_ground(x0, y0, cell, nx, ny, tp, params_of(p), source_xy, ground_only=ground_only, want_cost=True)
            assert got[2].tobytes() == cost.tobytes(), what + ": the cost images differ from pwpp_terrain_ground's"
            same(got[:2], want, what + ", path %d" % path)
            same(h.reach_ground(x0, y0, cell, nx, ny, tp, params_of(p), source_xy, ground_only=ground_only), want, what + ": the cost kept in the handle")
            for keep in (True, False):   # into device memory: the cost images kept in the handle, and asked for
                got = ground_on_device(h, (x0, y0, cell, nx, ny), 1, tp, p, source_xy, keep, ground_only=ground_only)
                same(got[:2], want, what + ", path %d (device, cost %s)" % (path, "kept" if keep else "returned"))
                assert keep or got[2].tobytes() == cost.tobytes(), what + ": the device cost images differ"
        h.set_option("reach_path", 0)
    assert _everything(h, 1) == before, "the reach changed the results of the call it reads"


def test_three_frames_of_a_batch_per_frame_sources_and_a_sub_range():
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(three_frames(), mode=pwpp_hip.MODE_FRESH)  # a 16-beam scan, an empty frame, a frame that is all unref
    grid = (-16.0, -16.0, 0.5, 64, 64)
    tp, p = tparams(), rr.params(base=2, unknown=10)
    cost = h.terrain_ground(*grid, tp)[4]
    xy = np.array([[0.2, 0.3], [-15.9, 15.9], [4.0, -7.5]])
    src = np.floor((xy + 16.0) / 0.5).astype(np.int32)
    want, one = rr.reach(cost, src, p), rr.reach(cost, src[0], p)
    for path in PATHS:
        h.set_option("reach_path", path)
        same(h.reach_ground(*grid, tp, params_of(p), xy), want, "three frames, their own sources, path %d" % path)
        got = ground_on_device(h, grid, 3, tp, p, xy, False)
        same(got[:2], want, "three frames, their own sources, path %d (device)" % path)
        assert got[2].tobytes() == cost.tobytes()
        same(ground_on_device(h, grid, 3, tp, p, xy[0], True)[:2], one, "three frames, one source, path %d (device)" % path)
        sub = ground_on_device(h, grid, 2, tp, p, xy[1:], False, frame_first=1, frames=2)
        same(sub[:2], (want[0][1:], want[1][1:]), "a sub-range, path %d (device)" % path)
        assert sub[2].tobytes() == cost[1:].tobytes()
    h.set_option("reach_path", 0)
    assert (want[0][0] != rr.NONE).sum() > 100 and (want[0][1] != rr.NONE).sum() == 64 * 64   # the empty frame is all unknown: 10 everywhere
    same(h.reach_ground(*grid, tp, params_of(p), xy[0]), one, "three frames, one source")
    sub = h.reach_ground(*grid, tp, params_of(p), xy[1:], frame_first=1, frames=2, want_cost=True)
    same(sub[:2], (want[0][1:], want[1][1:]), "a sub-range")
    assert sub[2].tobytes() == cost[1:].tobytes()
    with pytest.raises(Exception, match="sources"):
        h.reach_ground(*grid, tp, params_of(p), xy[:2])
    with pytest.raises(Exception, match="outside the grid"):
        h.reach_ground(*grid, tp, params_of(p), (16.0, 0.0))


# ---- workspace ------------------------------------------------------------------------------------------------------------------
def test_workspace_and_that_nothing_else_moves():
    h = pwpp_hip.Handle()
    empty = h.workspace_bytes()
    cost, src, p, want = shape_case(*SHAPES[-1])
    cells = cost.size
    same(on_host(h, cost, src, p), want, "before any estimate call")
    grown = h.workspace_bytes()
    assert grown >= empty + 2 * cells * 4 + cells + 2 * cells, "the cluster buffer is not counted"   # reach, from, the staged bytes, the terms
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
    b.reach_ground(-20.0, -20.0, 0.5, 80, 80, tparams(), params_of(FREE))
    assert b.workspace_bytes() >= a.workspace_bytes() + 3 * 80 * 80 * (4 + 1 + 2)  # the kept heights, cost bytes and terms
    assert _everything(b, 3) == before and b.time_us() == t_before, "the reach changed the results of the call it reads"
    for w in (a, b):
        w.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert _everything(b, 3) == _everything(a, 3), "an estimate call after a reach call differs from one without"
    b.trim_workspace()
    a.trim_workspace()
    assert a.workspace_bytes() == b.workspace_bytes()


def test_pybind_module_agrees_with_the_ctypes_handle():
    import pypatchworkpp
    pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    h = pwpp_hip.Handle()
    with pytest.raises(RuntimeError):
        pp.getReach(-30.0, -12.0, 0.5, 120, 48)  # no frame yet
    m = pypatchworkpp.FusedElevationMap()
    m.x0, m.y0, m.cell, m.nx, m.ny, m.n_max = -32.0, -14.0, 0.5, 130, 56, 4
    with pytest.raises(ValueError):
        pp.fusedReach(m)  # no mean yet
    pose = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    for seed in (5, 6):   # a map fused from two frames
        pts = small_cloud(seed)
        pp.estimateGround(pts)
        h.estimate_ground(pts)
        _, _, mean = pp.updateElevationMap(m, pose, 0.0, -30.0, -12.0, 0.5, 120, 48)
    tp, rp = pypatchworkpp.TerrainParams(), pypatchworkpp.ReachParams()
    got = pp.getReach(-30.0, -12.0, 0.5, 120, 48)   # the defaults: the source at (0, 0) m, base 1, lethal 100, unknown impassable
    want = h.reach_ground(-30.0, -12.0, 0.5, 120, 48, pwpp_hip.TerrainParams(1, 3, np.inf, np.inf, np.inf, 0), params_of(rr.params()))
    for g, w in zip(got, want):
        assert g.dtype == np.int32 and g.shape == (48, 120) and g.tobytes() == w[0].tobytes()
    assert got[0][24, 60] == 0 and got[1][24, 60] == 24 * 120 + 60
    tp.radius, tp.min_known, tp.step_max, tp.slope_max, tp.rough_max = 2, 6, 0.3, 0.4, 0.05
    rp.base, rp.unknown, rp.max_reach = 4, 50, 30000
    got = pp.fusedReach(m, tp, rp, 2.25, -3.75)
    cost = h.terrain_grid(mean, 0.5, pwpp_hip.TerrainParams(2, 6, 0.3, 0.4, 0.05, 0))[4]
    src = (int((2.25 + 32.0) / 0.5), int((-3.75 + 14.0) / 0.5))
    want = rr.reach(cost, src, rr.params(base=4, unknown=50, max_reach=30000))
    for g, w in zip(got, want):
        assert g.dtype == np.int32 and g.shape == (56, 130) and g.tobytes() == w.tobytes()
    assert 100 < (want[0] != rr.NONE).sum() < 56 * 130
    with pytest.raises(RuntimeError):
        pp.fusedReach(m, tp, rp, 100.0, 0.0)   # the source lies outside the map
