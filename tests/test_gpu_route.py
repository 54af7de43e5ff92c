"""The routes on the reach field (pwpp_route_grid, pwpp_plan_grid) on a real MI355X, exactly equal -- rows, cells, waypoints -- to the
restatement of tests/route_ref.py, for host and device memory (the cost bytes at odd addresses, the int32 images, the rows and the lists
at their minimum alignment, poisoned surroundings intact, inputs unwritten) and for every value of the option "route_path".  The shapes
are the smallest that can go wrong: 1 x 1, 1 x 9 and 9 x 1, corridors with a waypoint at every bend, a comb, random images with walls
and unknown cells, a dist2 image with a clearance, a source whose bytes are impassable under a line; routes of look - 1 .. look + 2
cells at every look where the wave kernel's rounds of 64 candidates begin and end; the list limits one below, at and one above a route's
counts; 1, 63, 64 and 65 starts; routes of 700 to 900 cells that wrap the wave kernel's window of 512, a cycle among them; hand-made broken
from images.  References are computed once and shared."""
import functools

import numpy as np
import pytest

import pwpp_hip
import reach_ref as rr
import route_ref as rt

pytestmark = pytest.mark.gpu

PATHS = (0, 1, 2)


def params_of(p):
    return pwpp_hip.ReachParams(p["base"], p["lethal"], p["unknown"], p["clearance2"], p["max_reach"], 0)


def route_params_of(q):
    return pwpp_hip.RouteParams(q["max_cells"], q["max_waypoints"], q["look"], q["line_cost"])


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()  # (no estimate call: the routes need the handle's stream and buffer only)


def on_host(h, cost, src, p, frm, starts, q, dist2=None):
    return h.route_grid(cost, src, params_of(p), frm, starts, route_params_of(q), dist2=dist2)


def poisoned(torch, words, dtype):
    b = torch.full((words + 128,), -7, dtype=dtype, device="cuda")
    assert b.data_ptr() % 256 == 0
    return b


def on_device(h, cost, src, p, frm, starts, q, dist2=None, plan=False, field=False):
    """route_grid (plan: plan_grid, field: with its optional outputs) on device arrays: the cost bytes start 1 byte, every int32 array 4
    bytes behind a 256-byte boundary -- their minimum; what surrounds them is poisoned and must survive, and the inputs must not be written."""
    import torch
    c3 = cost.reshape((-1,) + cost.shape[-2:])
    frames, ny, nx = c3.shape
    cells = c3.size
    st = np.asarray(starts, np.int32)
    n = st.shape[-2]
    routes = frames * n
    dc = poisoned(torch, cells, torch.int8)
    dd, df, dre = (poisoned(torch, cells, torch.int32) for _ in range(3))
    drows, dcells, dwps = poisoned(torch, routes * 8, torch.int32), poisoned(torch, routes * q["max_cells"], torch.int32), poisoned(torch, routes * q["max_waypoints"], torch.int32)
    dc[1:1 + cells] = torch.from_numpy(c3.reshape(-1).copy()).cuda()
    if dist2 is not None:
        dd[1:1 + cells] = torch.from_numpy(np.ascontiguousarray(dist2, np.int32).reshape(-1).copy()).cuda()
    if not plan:
        df[1:1 + cells] = torch.from_numpy(np.ascontiguousarray(frm, np.int32).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    lists = dict(cells_ptr=dcells.data_ptr() + 4 if q["max_cells"] else 0, waypoints_ptr=dwps.data_ptr() + 4 if q["max_waypoints"] else 0,
                 dist2_ptr=dd.data_ptr() + 4 if dist2 is not None else 0)
    if plan:
        h.plan_grid_device(nx, ny, frames, dc.data_ptr() + 1, src, params_of(p), st, route_params_of(q), drows.data_ptr() + 4,
                           reach_ptr=dre.data_ptr() + 4 if field else 0, from_ptr=df.data_ptr() + 4 if field else 0, **lists)
    else:
        h.route_grid_device(nx, ny, frames, dc.data_ptr() + 1, src, params_of(p), df.data_ptr() + 4, st, route_params_of(q), drows.data_ptr() + 4, **lists)
    h.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
    rc, rd, rf = dc.cpu().numpy(), dd.cpu().numpy(), df.cpu().numpy()
    assert rc[0] == -7 and (rc[1 + cells:] == -7).all() and rc[1:1 + cells].tobytes() == c3.tobytes(), "the cost bytes were written"
    if dist2 is None:
        assert (rd == -7).all(), "a dist2 image that was not given was written"
    else:
        assert rd[0] == -7 and (rd[1 + cells:] == -7).all() and rd[1:1 + cells].tobytes() == np.ascontiguousarray(dist2, np.int32).tobytes()
    if not plan:
        assert rf[0] == -7 and (rf[1 + cells:] == -7).all() and rf[1:1 + cells].tobytes() == np.ascontiguousarray(frm, np.int32).tobytes(), "from was written"
    elif not field:
        assert (rf == -7).all() and (dre.cpu().numpy() == -7).all(), "a field image that was not given was written"
    out = []
    for b, words, dtype, shape in ((drows, routes * 8, rt.ROW, (frames, n)), (dcells, routes * q["max_cells"], np.int32, (frames, n, q["max_cells"])),
                                   (dwps, routes * q["max_waypoints"], np.int32, (frames, n, q["max_waypoints"]))):
        raw = b.cpu().numpy()
        assert raw[0] == -7 and (raw[1 + words:] == -7).all(), "an element outside an array was written"
        out.append(raw[1:1 + words].copy().view(dtype).reshape(shape))
    if plan and field:
        for b in (dre, df):
            raw = b.cpu().numpy()
            assert raw[0] == -7 and (raw[1 + cells:] == -7).all()
            out.append(raw[1:1 + cells].reshape(cost.shape))
    return tuple(out)


def same(got, want, what):
    for name, g, w in zip(("rows", "cells", "waypoints", "reach", "from"), got, want):
        if g is None:
            assert w.size == 0, "%s: no %s" % (what, name)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s %r %r" % (what, name, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            if name == "rows":
                bad = np.argwhere(g != w)
                assert False, "%s: %d rows differ, the first %s: %r, expected %r" % (what, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])])
            bad = np.argwhere(g != w)
            assert False, "%s: %d entries of %s differ, the first %s: %r, expected %r" % (what, len(bad), name, bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


def everywhere(h, cost, src, p, frm, starts, q, want, what, dist2=None):
    """Every path, in host and in device memory, against `want`."""
    for path in PATHS:
        h.set_option("route_path", path)
        try:
            same(on_host(h, cost, src, p, frm, starts, q, dist2), want, "%s (host, path %d)" % (what, path))
            same(on_device(h, cost, src, p, frm, starts, q, dist2), want, "%s (device, path %d)" % (what, path))
        finally:
            h.set_option("route_path", 0)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def all_cells(nx, ny, step=1):
    return np.array([(x, y) for y in range(0, ny, step) for x in range(0, nx, step)], np.int32)


def test_the_option_is_checked(handle):
    for v in (3, -1):
        with pytest.raises(Exception):
            handle.set_option("route_path", v)


# ---- the smallest images ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_case(nx, ny):
    cost = rr.random_cost(2, ny, nx, 3 * nx + ny, lethal=0.1, unknown=0.1)
    src = np.array([[0, 0], [nx - 1, ny - 1]], np.int32)
    p = rr.params(base=2, unknown=30)
    _, frm = rr.reach(cost, src, p)
    starts = all_cells(nx, ny)
    q = rt.route_params(max_cells=5, max_waypoints=3, look=4, line_cost=40)
    return frozen(cost, src, frm, starts) + (p, q, rt.routes(cost, src, p, frm, starts, q))


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1)], ids=lambda s: "%dx%d" % s)
def test_the_smallest_images(handle, shape):
    cost, src, frm, starts, p, q, want = small_case(*shape)
    assert want[0]["status"][0, 0] == rt.OK and want[0]["cells"][0, 0] == 1 and want[0]["waypoints"][0, 0] == 1   # the start on the source
    everywhere(handle, cost, src, p, frm, starts, q, want, "%dx%d" % shape)


# ---- corridors: a waypoint at every bend ------------------------------------------------------------------------------------------
FREE = rr.params(base=2, lethal=100, unknown=-1)


@functools.lru_cache(maxsize=None)
def corridor(kind):
    one = rr.serpentine(21, 17) if kind == "serpentine" else rr.spiral(29 if kind == "spiral29" else 17)
    cost = np.stack([one, one])
    _, frm = rr.reach(cost, (0, 0), FREE)
    far = int(np.argmax(np.where(frm[0] >= 0, rr.reach(one, (0, 0), FREE)[0], -1)))   # the corridor's other end
    ny, nx = one.shape
    starts = np.array([(far % nx, far // nx), (0, 0), (nx - 1, 0)], np.int32)
    q = rt.route_params(max_cells=nx * ny, max_waypoints=nx * ny, look=40, line_cost=0)
    return frozen(cost, frm, starts) + (q, rt.routes(cost, (0, 0), FREE, frm, starts, q))


@pytest.mark.parametrize("kind", ["serpentine", "spiral17", "spiral29"])
def test_a_corridor_has_a_waypoint_at_every_bend(handle, kind):
    cost, frm, starts, q, want = corridor(kind)
    row, cells, wps = want[0][0, 0], want[1][0, 0], want[2][0, 0]
    assert row["status"] == rt.OK and row["cells"] > cost[0].size // 3 and row["corner_steps"] == 0
    nx = cost.shape[2]
    route = cells[:row["cells"]].tolist()
    bends = [b for a, b, c in zip(route, route[1:], route[2:]) if b - a != c - b]
    assert len(bends) >= 10 and set(bends) <= set(wps[:row["waypoints"]].tolist()), "a line across a bend would cut its corner"
    assert row["waypoints"] == len(bends) + 2   # look reaches along every straight stretch
    everywhere(handle, cost, (0, 0), FREE, frm, starts, q, want, kind)


# ---- routes longer than the wave kernel's window of 512 cells ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_case(kind):
    if kind == "strip":   # 3 x 700: dear cells scattered, lines of up to 256 cells that straddle cell 512 of the route
        rng = np.random.default_rng(7)
        cost = np.zeros((2, 3, 700), np.int8)
        cost[:, 0, :] = np.where(rng.random((2, 700)) < 0.25, 60, 0)
        cost[:, 2, :] = np.where(rng.random((2, 700)) < 0.25, 60, 0)
        cost[0, 1, :] = np.where(rng.random(700) < 0.02, 60, 0)
        cost[:, 1, 0] = 0
        src, p = (0, 1), rr.params(base=2)
        starts = np.array([(699, 1), (699, 0), (640, 2), (511, 1), (512, 1), (513, 1)], np.int32)
    else:
        one = rr.serpentine(33, 41) if kind == "serpentine" else rr.spiral(41)
        cost = np.stack([one, one])
        src, p = (0, 0), FREE
        reach = rr.reach(one, src, p)[0]
        far = int(np.argmax(np.where(reach != rr.NONE, reach, -1)))
        starts = np.array([(far % 41, far // 41), (40, 0)], np.int32)
    _, frm = rr.reach(cost, src, p)
    return frozen(cost, frm, starts) + (src, p)


@pytest.mark.parametrize("look", [64, 255, 256])
@pytest.mark.parametrize("kind", ["serpentine", "spiral", "strip"])
def test_routes_that_wrap_the_window_of_the_wave_kernel(handle, kind, look):
    cost, frm, starts, src, p = long_case(kind)
    q = rt.route_params(max_cells=cost[0].size if look == 64 else 0, max_waypoints=120, look=look, line_cost=20)
    want = rt.routes(cost, src, p, frm, starts, q)
    row = want[0][0, 0]
    assert row["status"] == rt.OK and row["cells"] > 512 + 150 and 2 < row["waypoints"] < 120
    if kind == "strip":
        assert (want[0]["status"] == rt.OK).all() and want[0][1, 0]["waypoints"] == -(-699 // look) + 1   # the clear row: lines of `look` cells, one from cell 256 to 512
    everywhere(handle, cost, src, p, frm, starts, q, want, "%s, look %d" % (kind, look))


def test_a_cycle_walked_past_the_window_to_the_hop_bound(handle):
    """A 2-cycle on 30 x 30 free cells: 899 hops, the searches run all along and everything they stored is taken back."""
    cost = np.zeros((1, 30, 30), np.int8)
    p = rr.params(base=1)
    _, frm = rr.reach(cost, (0, 0), p)
    f = frm.copy()
    f[0, 15, 15], f[0, 15, 16] = 15 * 30 + 16, 15 * 30 + 15
    starts = np.array([(15, 15), (29, 0)], np.int32)
    for look in (3, 256):
        q = rt.route_params(max_cells=900, max_waypoints=900, look=look, line_cost=0)
        want = rt.routes(cost, (0, 0), p, f, starts, q)
        row = want[0][0, 0]
        assert row["status"] == rt.BROKEN and row["cells"] == 900 and row["cost"] == 899 * 10 and row["waypoints"] == 0 and (want[2][0, 0] == -1).all()
        assert want[1][0, 0].tolist() == [15 * 30 + 15, 15 * 30 + 16] * 450 and want[0][0, 1]["status"] == rt.OK
        everywhere(handle, cost, (0, 0), p, f, starts, q, want, "cycle, look %d" % look)


# ---- a comb, random images, a clearance, a source under a line -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def image_case(kind):
    d2 = None
    if kind == "comb":
        cost = np.stack([rr.comb(40, 56, 9, 3, 5), rr.comb(40, 56, 7, 2, 6)])
        src, p = np.array([[0, 20]], np.int32), rr.params(base=3)
        starts = np.array([(55, 0), (55, 39), (30, 20), (10, 39), (0, 20)], np.int32)
        q = rt.route_params(max_cells=600, max_waypoints=80, look=30, line_cost=45)
    elif kind == "random":
        cost = rr.random_cost(2, 47, 61, 12, lethal=0.2, unknown=0.1)
        src, p = np.array([[30, 23], [0, 46]], np.int32), rr.params(base=7, lethal=90, unknown=45)
        starts = all_cells(61, 47, 5)
        q = rt.route_params(max_cells=60, max_waypoints=20, look=12, line_cost=60)
    elif kind == "dist2":
        cost = rr.random_cost(2, 40, 40, 13, lethal=0.04, unknown=0.0)
        wall = cost >= 100
        yy, xx = np.mgrid[0:40, 0:40]
        d2 = np.full(cost.shape, rr.DIST_BEYOND, np.int32)
        for f in range(2):   # the squared distance to the nearest lethal cell, by hand
            for y, x in np.argwhere(wall[f]):
                d2[f] = np.minimum(d2[f], (yy - y) ** 2 + (xx - x) ** 2)
        src, p = np.array([[20, 20]], np.int32), rr.params(base=4, clearance2=2)
        starts = all_cells(40, 40, 4)
        q = rt.route_params(max_cells=70, max_waypoints=20, look=20, line_cost=100)
    else:  # the source's own bytes are impassable: every route's last line ends on it
        cost = np.zeros((2, 9, 13), np.int8)
        cost[:, 0:5, 6] = 100        # a wall, the source its last cell
        cost[1, 4, 6] = -1           # unknown in the second frame, impassable too
        src, p = np.array([[6, 4]], np.int32), rr.params(base=5)
        starts = np.array([(0, 4), (12, 4), (6, 8), (0, 0), (12, 0), (6, 4)], np.int32)
        q = rt.route_params(max_cells=20, max_waypoints=6, look=16, line_cost=0)
    _, frm = rr.reach(cost, src, p, d2)
    want = rt.routes(cost, src, p, frm, starts, q, d2)
    return frozen(cost, src, frm, starts) + (p, q, d2, want)


@pytest.mark.parametrize("kind", ["comb", "random", "dist2", "source"])
def test_images_against_the_reference(handle, kind):
    cost, src, frm, starts, p, q, d2, want = image_case(kind)
    rows = want[0]
    assert (rows["status"] == rt.OK).sum() >= rows.size // 2
    if kind in ("comb", "random"):
        assert ((rows["waypoints"] > 2) & (rows["waypoints"] < rows["cells"])).any() and (rows["corner_steps"] > 0).any()
    if kind == "random":
        assert (rows["status"] == rt.NONE).any() and (rows["cells"] > 60).any() and (rows["waypoints"] > 20).any()
    if kind == "dist2":
        ok = rows["status"] == rt.OK
        assert (rows["min_dist2"][ok] < rr.DIST_BEYOND).all() and (rows["min_dist2"][ok] > 2).any() and (rows["min_dist2"][~ok] == rr.DIST_BEYOND).all()
        assert (rows["status"] == rt.NONE).any()   # a start inside the clearance is impassable
    if kind == "source":
        assert (rows["status"] == rt.OK).all() and (rows["waypoints"][:, :3] == 2).all() and (rows["max_term"] == 5).all()   # one line each, ending on the lethal source
    everywhere(handle, cost, src, p, frm, starts, q, want, kind, d2)


def test_a_line_that_merely_passes_over_the_source(handle):
    """(4, 2) is lethal and the source.  A hand-made from leads from (5, 2) round it -- (5, 1), (4, 1), (3, 1), (3, 2) -- and into it from the
    west: every hop a step.  With look = 4 the source itself is out of the first search's reach, and the line (5, 2) -> (3, 2) passes over
    it: clear only because the source has its term wherever it is read."""
    cost = np.zeros((1, 5, 9), np.int8)
    cost[0, 2, 4] = 100
    src, p = (4, 2), rr.params(base=3)
    i = lambda x, y: y * 9 + x
    _, frm = rr.reach(cost, src, p)
    q = rt.route_params(max_cells=12, max_waypoints=4, look=4, line_cost=0)
    starts = np.array([(0, 2), (8, 2), (8, 0)], np.int32)
    want = rt.routes(cost, src, p, frm, starts, q)
    assert (want[0]["status"] == rt.OK).all() and (want[0]["max_term"] == 3).all()
    everywhere(handle, cost, src, p, frm, starts, q, want, "to the source")
    f = frm.copy().reshape(-1)
    for a, b in (((5, 2), (5, 1)), ((5, 1), (4, 1)), ((4, 1), (3, 1)), ((3, 1), (3, 2)), ((3, 2), (4, 2))):
        f[i(*a)] = i(*b)
    want = rt.routes(cost, src, p, f, [(5, 2)], q)
    assert want[0]["status"][0, 0] == rt.OK and want[0]["cells"][0, 0] == 6 and want[2][0, 0].tolist() == [i(5, 2), i(3, 2), i(4, 2), -1]
    everywhere(handle, cost, src, p, f.reshape(cost.shape), np.array([(5, 2)], np.int32), q, want, "over the source")
    # the same cell under a line where it is no source: a from along row 2 from (8, 2) to another source, (0, 2), breaks at the hop onto it
    f2 = np.full((1, 5, 9), -1, np.int32)
    f2[0, 2, 1:9] = 2 * 9 + np.arange(0, 8)
    f2[0, 2, 0] = 2 * 9
    want = rt.routes(cost, (0, 2), p, f2, [(8, 2)], q)
    assert want[0]["status"][0, 0] == rt.BROKEN and want[0]["cells"][0, 0] == 4
    everywhere(handle, cost, (0, 2), p, f2, np.array([(8, 2)], np.int32), q, want, "onto a lethal cell")


# ---- routes of look - 1 .. look + 2 cells ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def strip():
    """3 x 262 cells, dear cells scattered over the outer rows and a few over the middle one: routes towards (0, 1) weave, and lines fail by their cost."""
    rng = np.random.default_rng(61)
    cost = np.zeros((2, 3, 262), np.int8)
    cost[:, 0, :] = np.where(rng.random((2, 262)) < 0.3, 60, 0)
    cost[:, 2, :] = np.where(rng.random((2, 262)) < 0.3, 60, 0)
    cost[:, 1, :] = np.where(rng.random((2, 262)) < 0.06, 60, 0)
    cost[1, 1, :] = 0   # the second frame: a clear middle row
    cost[:, 1, 0] = 0
    p = rr.params(base=2)
    _, frm = rr.reach(cost, (0, 1), p)
    return frozen(cost, frm) + (p,)


@pytest.mark.parametrize("look", [1, 2, 63, 64, 65, 256])
def test_routes_as_long_as_look_and_one_or_two_cells_more(handle, look):
    cost, frm, p = strip()
    starts = np.array([(max(n - 1, 0), 1) for n in (look - 1, look, look + 1, look + 2)] + [(261, 0), (261, 2)], np.int32)   # on row 1 a route of n cells starts at x = n - 1 or a little less
    q = rt.route_params(max_cells=0, max_waypoints=40 if look > 2 else 262, look=look, line_cost=20)
    want = rt.routes(cost, (0, 1), p, frm, starts, q)
    rows = want[0]
    assert (rows["status"] == rt.OK).all()
    if look >= 63:
        assert (rows["waypoints"][1, :4] == np.array([2, 2, 2, 3])).all()           # the clear row: one line of look cells, then the rest
        assert (rows["waypoints"][0] > rows["waypoints"][1]).all()                  # the weaving frame needs more
    if look == 1:
        assert np.array_equal(rows["waypoints"], rows["cells"])
    everywhere(handle, cost, (0, 1), p, frm, starts, q, want, "look %d" % look)


# ---- the limits of the lists ------------------------------------------------------------------------------------------------------
def test_list_limits_below_at_and_above_the_counts_and_none(handle):
    cost, src, frm, grid, p, q0, _, seen = image_case("random")
    starts = np.array([grid[int(np.argmax(seen[0]["cells"][0]))], (5, 40)], np.int32)   # the longest route of the first frame
    full = rt.routes(cost, src, p, frm, starts, dict(q0, max_cells=400, max_waypoints=400))
    cells, wps = int(full[0]["cells"][0, 0]), int(full[0]["waypoints"][0, 0])
    assert cells > 20 and 3 < wps < cells
    for max_cells, max_wps in ((cells - 1, wps - 1), (cells, wps), (cells + 1, wps + 1), (0, wps), (cells, 0), (0, 0), (1, 1)):
        q = dict(q0, max_cells=max_cells, max_waypoints=max_wps)
        want = rt.routes(cost, src, p, frm, starts, q)
        for name in rt.ROW.names:
            if name != "waypoints" or max_wps > 0:
                assert np.array_equal(want[0][name], full[0][name]), "a limit changed %s" % name
        everywhere(handle, cost, src, p, frm, starts, q, want, "limits %d, %d" % (max_cells, max_wps))


# ---- many starts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_starts", [1, 63, 64, 65])
def test_many_starts_repeated_on_the_source_unreachable_and_beyond_max_reach(handle, n_starts):
    cost, src, _, _, p, q0, _, _ = image_case("random")
    p = dict(p, max_reach=2500)
    reach, frm = rr.reach(cost, src, p)
    free = rr.reach(cost, src, dict(p, max_reach=0))[0]
    beyond = np.argwhere((reach[0] == rr.NONE) & (free[0] != rr.NONE))
    walled = np.argwhere(free[0] == rr.NONE)
    assert len(beyond) > 50 and len(walled) > 50
    rng = np.random.default_rng(n_starts)
    starts = np.stack([rng.integers(0, 61, n_starts), rng.integers(0, 47, n_starts)], axis=-1).astype(np.int32)
    special = [(30, 23), (beyond[0][1], beyond[0][0]), (walled[0][1], walled[0][0]), tuple(starts[0])]   # the first frame's source, beyond the limit, walled in, a repeat
    for k, s in enumerate(special[:n_starts]):
        starts[-1 - k] = s
    q = dict(q0, max_cells=30, max_waypoints=8)
    want = rt.routes(cost, src, p, frm, starts, q)
    if n_starts > 4:
        assert (want[0]["status"][0, -3:-1] == rt.NONE).all() and want[0]["cells"][0, -1] == 1 and want[0][0, -4] == want[0][0, 0]
    assert (want[0]["cost"][want[0]["status"] == rt.OK] <= 2500).all()
    everywhere(handle, cost, src, p, frm, starts, q, want, "%d starts" % n_starts)


def test_one_start_set_for_all_frames_and_one_per_frame(handle):
    cost, src, frm, _, p, q, _, _ = image_case("random")
    one = all_cells(61, 47, 9)
    per_frame = np.stack([one, one[::-1]])
    a = rt.routes(cost, src, p, frm, one, q)
    b = rt.routes(cost, src, p, frm, per_frame, q)
    assert a[0][0].tobytes() == b[0][0].tobytes() and a[0][1].tobytes() == b[0][1][::-1].tobytes() and a[0][1].tobytes() != b[0][1].tobytes()
    everywhere(handle, cost, src, p, frm, one, q, a, "one set")
    everywhere(handle, cost, src, p, frm, per_frame, q, b, "a set per frame")


# ---- plan = reach + route --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "dist2", "comb"])
def test_plan_grid_is_reach_grid_then_route_grid(handle, kind):
    cost, src, frm, starts, p, q, d2, want = image_case(kind)
    field = rr.reach(cost, src, p, d2)
    for path in PATHS:
        handle.set_option("route_path", path)
        try:
            same(handle.plan_grid(cost, src, params_of(p), starts, route_params_of(q), dist2=d2), want, "plan (host, path %d)" % path)
            same(handle.plan_grid(cost, src, params_of(p), starts, route_params_of(q), dist2=d2, want_field=True), want + field, "plan with the field (host, path %d)" % path)
            same(on_device(handle, cost, src, p, None, starts, q, d2, plan=True), want, "plan (device, path %d)" % path)
            same(on_device(handle, cost, src, p, None, starts, q, d2, plan=True, field=True), want + field, "plan with the field (device, path %d)" % path)
        finally:
            handle.set_option("route_path", 0)
    # and the two calls one after the other on the device's own field
    reach, frm_gpu = handle.reach_grid(cost, src, params_of(p), dist2=d2)
    same(on_host(handle, cost, src, p, frm_gpu, starts, q, d2), want, "reach_grid then route_grid")


# ---- broken from images ----------------------------------------------------------------------------------------------------------------
def broken_cases():
    """8 x 8 of free ground but for a wall cell at (3, 2) and (2, 3), the source at (0, 0); from images made by hand.  The walk is bounded
    by its hops, so nothing is provoked: each ends PWPP_ROUTE_BROKEN with the prefix the valid hops gave."""
    cost = np.zeros((1, 8, 8), np.int8)
    cost[0, 2, 3] = cost[0, 3, 2] = 100
    p = rr.params(base=1)
    _, good = rr.reach(cost, (0, 0), p)
    i = lambda x, y: y * 8 + x
    out = {}
    f = good.copy()
    f[0, 5, 5], f[0, 5, 4] = i(4, 5), i(5, 5)                      # a 2-cycle: 63 hops, then the bound
    out["cycle"] = (f, (5, 5), 64, [i(5, 5), i(4, 5)] * 32)
    f = good.copy()
    f[0, 6, 6] = i(5, 6)
    f[0, 6, 5] = 64                                                # one past the image
    out["out of range"] = (f, (6, 6), 2, [i(6, 6), i(5, 6)])
    f = good.copy()
    f[0, 6, 5] = -2                                                # negative, not the -1 of an unreached START
    out["negative"] = (f, (5, 6), 1, [i(5, 6)])
    f = good.copy()
    f[0, 7, 7], f[0, 6, 6] = i(6, 6), i(4, 6)                      # two cells away
    out["non-neighbour"] = (f, (7, 7), 2, [i(7, 7), i(6, 6)])
    f = good.copy()
    f[0, 3, 3] = i(2, 2)                                           # between the two wall cells
    out["cut corner"] = (f, (3, 3), 1, [i(3, 3)])
    f = good.copy()
    f[0, 4, 4], f[0, 4, 3] = i(3, 4), i(3, 4)                      # names itself away from the source
    out["ends off the source"] = (f, (4, 4), 2, [i(4, 4), i(3, 4)])
    f = good.copy()
    f[0, 1, 3] = i(3, 2)                                           # onto a wall
    out["onto a wall"] = (f, (3, 1), 1, [i(3, 1)])
    return cost, p, out


@pytest.mark.parametrize("kind", ["cycle", "out of range", "negative", "non-neighbour", "cut corner", "ends off the source", "onto a wall"])
def test_a_broken_from_ends_broken_with_its_prefix(handle, kind):
    cost, p, cases = broken_cases()
    frm, start, cells, prefix = cases[kind]
    q = rt.route_params(max_cells=70, max_waypoints=70, look=3, line_cost=0)
    starts = np.array([start, (7, 0)], np.int32)   # (and a sound route beside it)
    want = rt.routes(cost, (0, 0), p, frm, starts, q)
    row = want[0][0, 0]
    assert row["status"] == rt.BROKEN and row["cells"] == cells and row["waypoints"] == 0 and (want[2][0, 0] == -1).all()
    assert want[1][0, 0, :cells].tolist() == prefix and (want[1][0, 0, cells:] == -1).all()
    if kind == "cycle":
        assert row["cost"] == 63 * 10 and row["edge_steps"] == 63
    assert want[0][0, 1]["status"] == rt.OK and want[0][0, 1]["cells"] == 8
    everywhere(handle, cost, (0, 0), p, frm, starts, q, want, kind)


# ---- the layers above --------------------------------------------------------------------------------------------------------------------
def test_workspace_is_counted_and_trimmed():
    h = pwpp_hip.Handle()
    empty = h.workspace_bytes()
    cost, src, frm, starts, p, q, d2, want = image_case("random")
    same(h.plan_grid(cost, src, params_of(p), starts, route_params_of(q)), want, "before any estimate call")
    assert h.workspace_bytes() >= empty + cost.size * (1 + 2 + 4 + 4) + want[1].size * 4, "the cluster buffer is not counted"   # bytes, terms, reach, from, the cell lists
    h.trim_workspace()
    assert h.workspace_bytes() == empty, "pwpp_trim_workspace did not free the cluster buffer"


def test_pybind_module_agrees_with_the_ctypes_handle():
    import pypatchworkpp
    from test_gpu_obstacle_grid import small_cloud
    pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    h = pwpp_hip.Handle()
    starts_xy = [(10.25, 3.0), (-20.0, -8.1), (0.1, 0.1), (29.9, 11.9)]
    with pytest.raises(RuntimeError):
        pp.getRoutes(-30.0, -12.0, 0.5, 120, 48, starts_xy)  # no frame yet
    pts = small_cloud(5)
    pp.estimateGround(pts)
    h.estimate_ground(pts)
    tp, rp, qp = pypatchworkpp.TerrainParams(), pypatchworkpp.ReachParams(), pypatchworkpp.RouteParams()
    rp.base, rp.unknown = 3, 40
    qp.max_cells, qp.max_waypoints, qp.look, qp.line_cost = 200, 30, 24, 50
    rows, cells, wps, xy = pp.getRoutes(-30.0, -12.0, 0.5, 120, 48, starts_xy, tp, rp, qp, 1.0, -1.0)
    p, q = rr.params(base=3, unknown=40), rt.route_params(200, 30, 24, 50)
    reach, frm, cost = h.reach_ground(-30.0, -12.0, 0.5, 120, 48, pwpp_hip.TerrainParams(1, 3, np.inf, np.inf, np.inf, 0), params_of(p), source_xy=(1.0, -1.0), want_cost=True)
    cell_of = lambda x, y: (int((x + 30.0) / 0.5), int((y + 12.0) / 0.5))
    want = rt.routes(cost[0], cell_of(1.0, -1.0), p, frm[0], [cell_of(*s) for s in starts_xy], q)
    assert rows.shape == (4, 8) and rows.astype("<i4").tobytes() == want[0].tobytes() and cells.tobytes() == want[1].tobytes() and wps.tobytes() == want[2].tobytes()
    assert (want[0]["status"] == rt.OK).any()
    known = wps >= 0
    assert np.isnan(xy[~known]).all() and np.array_equal(xy[known][:, 0], -30.0 + (wps[known] % 120 + 0.5) * 0.5) and np.array_equal(xy[known][:, 1], -12.0 + (wps[known] // 120 + 0.5) * 0.5)
    # planRoutes on any cost image: a costmap's
    c = rr.random_cost(1, 48, 120, 3, lethal=0.1)[0]
    got = pp.planRoutes(c, -30.0, -12.0, 0.5, 120, 48, starts_xy, rp, qp, 1.0, -1.0)
    want = rt.plan(c, cell_of(1.0, -1.0), p, [cell_of(*s) for s in starts_xy], q)
    assert got[0].astype("<i4").tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
    with pytest.raises(RuntimeError):
        pp.planRoutes(c, -30.0, -12.0, 0.5, 120, 48, [(100.0, 0.0)], rp, qp)   # a start outside the grid
