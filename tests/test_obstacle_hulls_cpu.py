"""No-GPU checks of the obstacle hulls (pwpp_hull_obstacles, pwpp_hull_points, pwpp_hull_vertex_xy): the exports, the feature macro,
the 64-byte row field by field, the bindings; every argument check that comes before the device is touched; pwpp_hull_points -- the
functions the kernels compile, on the host -- byte for byte against the restatement of tests/obstacle_hulls_ref.py (a monotone
chain and an all-edges rectangle in Python integers) on single points, duplicates, collinear runs, a square, an L of two walls, a
circle of hundreds of vertices with truncated lists, the ends of the coordinate range, skipped points and 2 000 random sets on a
16 x 16 sub-lattice; the header's invariants; and the stand-alone program that runs the same functions against a brute force of its
own (tools/hull_check.cpp), built with the address and undefined-behaviour sanitizers where the toolchain has them.

Points are given on the lattice: with the grid's origin at 0 a float32 x = q / 1024 is exact for q < 2^24 and quantises to q.  The
cell rule keeps dx < nx * cell <= 1024 m, so the largest q a call can produce is 2^20 (from the float32 below 1024); the header's
bound 2^20 + 1 is reached in tools/hull_check.cpp, which packs its points itself."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import obstacle_boxes_ref as ob
import obstacle_hulls_ref as oh
import pwpp_hip
from obstacle_grid_ref import F32, QNAN_BITS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")
E_ARG = -1
GRID = (0.0, 0.0, 1.0, 1024, 1024)  # x0, y0, cell, nx, ny: the whole extent the contract allows
QTOP = 1 << 20                      # the largest q a point inside the grid can have


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pwpp_hip.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "lib/libpwpp_hip.so"], check=True, stdout=subprocess.DEVNULL)
    return pwpp_hip.load()


def lattice(q, z=0.5):
    """(m, 3) float32 positions of (m, 2) lattice pairs; q = 2^20 becomes the float32 just below 1024, which quantises to it."""
    q = np.asarray(q, np.int64).reshape(-1, 2)
    xy = (q.astype(np.float64) / 1024.0).astype(F32)
    xy[q == QTOP] = np.nextafter(F32(1024.0), F32(0.0))
    assert np.array_equal(oh.quantise(0.0, 0.0, np.concatenate([xy, np.zeros((len(q), 1), F32)], 1)), q)
    return np.concatenate([xy, np.full((len(q), 1), z, F32)], 1)


def run(q, row, max_hulls, max_vertices, grid=GRID, what=""):
    """pwpp_hull_points with and without a list against the restatement; returns (rows, lists, the restatement's full lists)."""
    xyz = lattice(q) if not isinstance(q, np.ndarray) or q.dtype != F32 else q
    row = np.broadcast_to(np.asarray(row, np.int32), (len(xyz),)).copy()
    rows, lists = pwpp_hip.hull_points(*grid, xyz, row, max_hulls, max_vertices)
    bare, none = pwpp_hip.hull_points(*grid, xyz, row, max_hulls, max_vertices, with_vertices=False)
    ref_rows, ref_lists = oh.hull_rows(*grid, xyz, row, max_hulls, max_vertices)
    assert none is None and bare.tobytes() == rows.tobytes(), what + ": the rows depend on whether a list is asked for"
    oh.same(rows, lists, ref_rows, ref_lists, what)
    return rows, lists, ref_lists


def is_empty(r):
    w = np.frombuffer(r.tobytes(), np.uint32)
    return (w[[0, 1, 2, 4, 5, 6, 7, 8, 9]] == 0).all() and w[3] == 0xffffffff and (w[10:] == QNAN_BITS).all()


def test_symbols_macro_prototypes_and_layout(lib):
    hdr = open(os.path.join(ROOT, "include", "pwpp.h")).read()
    for name in ("pwpp_hull_obstacles", "pwpp_hull_points", "pwpp_hull_vertex_xy"):
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr
    assert "#define PWPP_HAS_OBSTACLE_HULLS 1" in hdr
    assert len(lib.pwpp_hull_obstacles.argtypes) == 12 and len(lib.pwpp_hull_points.argtypes) == 8 and len(lib.pwpp_hull_vertex_xy.argtypes) == 3
    assert pwpp_hip.OBSTACLE_HULL_DTYPE == oh.HULL_DTYPE and oh.HULL_DTYPE.itemsize == 64
    want = [("points", 0), ("n_vertices", 4), ("stored", 8), ("rect_edge", 12), ("area2", 16), ("qx_min", 24), ("qx_max", 28), ("qy_min", 32), ("qy_max", 36),
            ("cx", 40), ("cy", 44), ("ax", 48), ("ay", 52), ("length", 56), ("width", 60)]
    assert [(n, oh.HULL_DTYPE.fields[n][1]) for n in oh.HULL_DTYPE.names] == want
    for name in ("hull_obstacles", "hull_obstacles_device"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    import pypatchworkpp
    assert hasattr(pypatchworkpp.patchworkpp, "getObstacleHulls")


def test_every_argument_error_is_named_before_the_device_is_touched(lib):
    lab = np.zeros(16, np.int32)
    out = np.zeros(4, oh.HULL_DTYPE)
    ver = np.zeros((4, 8, 2), np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    g = pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 4, 4, 0, 0)

    def hulls(h=fake, gr=g, band=(0.2, 2.5), frames=1, mem=pwpp_hip.MEM_HOST, label=vp(lab), table=vp(out), max_hulls=4, vertices=vp(ver), max_vertices=8):
        return lib.pwpp_hull_obstacles(h, ctypes.byref(gr) if gr is not None else None, band[0], band[1], 0, frames, mem, label, table, max_hulls, vertices, max_vertices)

    assert hulls(h=None) == E_ARG and b"null handle" in lib.pwpp_last_error()
    assert hulls(gr=None) == E_ARG and b"null grid" in lib.pwpp_last_error()
    assert hulls(label=None) == E_ARG and b"null label" in lib.pwpp_last_error()
    assert hulls(table=None) == E_ARG and b"null hull table" in lib.pwpp_last_error()
    for m in (0, -1):
        assert hulls(max_hulls=m) == E_ARG and b"max_hulls" in lib.pwpp_last_error()
    for m in (0, -1, 1025):
        assert hulls(max_vertices=m) == E_ARG and b"max_vertices" in lib.pwpp_last_error()
        assert hulls(max_vertices=m, vertices=None) == E_ARG and b"max_vertices" in lib.pwpp_last_error()
    assert hulls(frames=(1 << 12) + 1, max_hulls=1 << 12, max_vertices=1) == E_ARG and b"2^24" in lib.pwpp_last_error()
    assert hulls(frames=2, max_hulls=(1 << 23) + 1, max_vertices=1) == E_ARG and b"2^24" in lib.pwpp_last_error()
    assert hulls(frames=1 << 10, max_hulls=1 << 10, max_vertices=257) == E_ARG and b"2^28" in lib.pwpp_last_error()
    assert hulls(frames=1, max_hulls=(1 << 18) + 1, max_vertices=1024) == E_ARG and b"2^28" in lib.pwpp_last_error()
    assert hulls(band=(2.5, 0.2)) == E_ARG and b"height band" in lib.pwpp_last_error()
    assert hulls(band=(np.nan, 1.0)) == E_ARG and b"height band" in lib.pwpp_last_error()
    assert hulls(gr=pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 4, 4, 2, 0)) == E_ARG and b"grid flags" in lib.pwpp_last_error()
    for nx, ny, cell in ((1025, 4, 1.0), (4, 1025, 1.0), (2049, 2048, 0.5), (4, 4, 256.5), (4, 4, np.nan)):
        assert hulls(gr=pwpp_hip.GroundGrid(0.0, 0.0, cell, nx, ny, 0, 0)) == E_ARG and b"1024 m" in lib.pwpp_last_error(), (nx, ny, cell)
    assert hulls(mem=pwpp_hip.MEM_HOST_PINNED) == E_ARG and b"PWPP_MEM_HOST or PWPP_MEM_DEVICE" in lib.pwpp_last_error()
    assert hulls(mem=pwpp_hip.MEM_DEVICE, table=ctypes.c_void_p(out.ctypes.data + 4)) == E_ARG and b"8-byte aligned" in lib.pwpp_last_error()

    xyz, row = np.zeros((2, 3), F32), np.zeros(2, np.int32)

    def points(gr=g, xyz=vp(xyz), row=vp(row), m=2, table=vp(out), max_hulls=4, vertices=vp(ver), max_vertices=8):
        return lib.pwpp_hull_points(ctypes.byref(gr) if gr is not None else None, xyz, row, m, table, max_hulls, vertices, max_vertices)

    assert points() == 0 and points(vertices=None) == 0
    assert points(gr=None) == E_ARG and points(table=None) == E_ARG and points(xyz=None) == E_ARG and points(row=None) == E_ARG
    assert points(max_hulls=0) == E_ARG and points(m=-1) == E_ARG and points(m=(1 << 22) + 1) == E_ARG
    assert points(max_vertices=0) == E_ARG and points(max_vertices=1025) == E_ARG and points(max_hulls=(1 << 24) + 1, max_vertices=1) == E_ARG
    assert points(max_hulls=(1 << 18) + 1, max_vertices=1024) == E_ARG and b"2^28" in lib.pwpp_last_error()
    assert points(m=0, xyz=None, row=None) == 0
    assert points(gr=pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 1025, 4, 0, 0)) == E_ARG and b"1024 m" in lib.pwpp_last_error()
    for bad in (dict(nx=0), dict(cell=0.0), dict(cell=np.inf), dict(x0=np.nan)):
        kw = dict(dict(x0=0.0, y0=0.0, cell=1.0, nx=4, ny=4, flags=0, pad_=0), **bad)
        assert points(gr=pwpp_hip.GroundGrid(**kw)) == E_ARG, bad
    q, xy = np.array([3, 5], np.int32), np.zeros(2, np.float64)
    assert lib.pwpp_hull_vertex_xy(ctypes.byref(g), vp(q), vp(xy)) == 0
    assert lib.pwpp_hull_vertex_xy(None, vp(q), vp(xy)) == E_ARG and lib.pwpp_hull_vertex_xy(ctypes.byref(g), None, vp(xy)) == E_ARG
    assert lib.pwpp_hull_vertex_xy(ctypes.byref(g), vp(q), None) == E_ARG


def test_one_point_two_points_and_duplicates(lib):
    rows, lists, _ = run([(7, 9)], 0, 2, 4, what="one point")
    r = rows[0]
    assert (r["points"], r["n_vertices"], r["stored"], r["rect_edge"], r["area2"]) == (1, 1, 1, 0, 0)
    assert (r["ax"], r["ay"], r["length"], r["width"]) == (1.0, 0.0, 0.0, 0.0) and r["cx"] == F32(7 / 1024) and r["cy"] == F32(9 / 1024)
    assert is_empty(rows[1]) and lists[0, 0].tolist() == [7, 9]
    rows, lists, _ = run([(7, 9)] * 5, 0, 1, 4, what="duplicates only")
    assert (rows[0]["points"], rows[0]["n_vertices"]) == (5, 1)
    rows, lists, _ = run([(700, 9), (7, 900), (700, 9)], 0, 1, 4, what="two points")
    assert (rows[0]["points"], rows[0]["n_vertices"], rows[0]["rect_edge"], rows[0]["area2"], rows[0]["width"]) == (3, 2, 0, 0, 0.0)
    assert lists[0, :2].tolist() == [[700, 9], [7, 900]]   # the smallest (qy, qx) first
    for mv in (1, 2):
        rows, _, _ = run([(700, 9), (7, 900)], 0, 1, mv, what="two points, max_vertices %d" % mv)
        assert rows[0]["stored"] == mv and (rows[0]["rect_edge"] == -1) == (mv == 1)


@pytest.mark.parametrize("d", [(1, 0), (0, 1), (1, 1), (1, -1), (7, 3)], ids=["x", "y", "diagonal", "antidiagonal", "skew"])
def test_a_collinear_run_has_two_vertices(lib, d):
    steps = [(k * 7) % 13 for k in range(13)] + [4, 4]
    q = [(5000 + d[0] * s, 5000 + d[1] * s) for s in steps]
    rows, lists, _ = run(q, 0, 1, 8, what="collinear %s" % (d,))
    ends = sorted([(5000, 5000), (5000 + 12 * d[0], 5000 + 12 * d[1])], key=lambda p: (p[1], p[0]))
    assert rows[0]["n_vertices"] == 2 and rows[0]["points"] == 15 and rows[0]["area2"] == 0 and rows[0]["width"] == 0.0
    assert lists[0, :2].tolist() == [list(p) for p in ends]
    assert rows[0]["length"] == F32(np.sqrt(np.float64(144 * (d[0] ** 2 + d[1] ** 2))) / 1024.0)


def test_a_square_ties_on_all_four_edges_and_edge_0_wins(lib):
    for s in (1, 512, QTOP):
        q = [(0, 0), (s, 0), (s, s), (0, s), (s // 2, s // 2), (s // 2, 0)]
        rows, lists, _ = run(q, 0, 1, 4, what="square of %d" % s)
        r = rows[0]
        assert (r["n_vertices"], r["rect_edge"], r["area2"]) == (4, 0, 2 * s * s) and lists[0].tolist() == [[0, 0], [s, 0], [s, s], [0, s]]
        assert (r["ax"], r["ay"]) == (1.0, 0.0) and r["length"] == r["width"] == F32(s / 1024.0)


def l_shape():
    """A car seen from a corner: a long wall along x and a short one along y, turned by atan2(3, 4) on the lattice."""
    q = [(200000 + 4 * 40 * k, 200000 + 3 * 40 * k) for k in range(0, 41)] + [(200000 - 3 * 40 * k, 200000 + 4 * 40 * k) for k in range(1, 19)]
    return q + q[:7]


def test_an_l_of_two_walls_gets_a_rectangle_below_the_box(lib):
    q = l_shape()
    rows, lists, ref_lists = run(q, 0, 1, 8, what="an L")
    r = rows[0]
    assert r["n_vertices"] == 3 and r["points"] == len(q)
    assert (r["ax"], r["ay"]) == (F32(0.8), F32(0.6)) or (r["ax"], r["ay"]) == (F32(0.6), F32(-0.8)) or (r["ax"], r["ay"]) == (F32(0.6), F32(0.8))
    assert {float(r["length"]), float(r["width"])} == {float(F32(8000 / 1024.0)), float(F32(3600 / 1024.0))}   # the two walls: 40 and 18 steps of 200
    xyz = lattice(q)
    box = pwpp_hip.box_points(*GRID, xyz, np.ones(len(q), F32), np.zeros(len(q), np.int32), 1)[0]
    assert float(r["length"]) * float(r["width"]) < float(box["length"]) * float(box["width"]), "the box of an L is not larger than its tightest rectangle"
    assert oh.box_area_not_below(oh.edge(ref_lists[0], int(r["rect_edge"])), box["ax"], box["ay"], ref_lists[0])


def test_a_circle_of_hundreds_of_vertices_full_and_truncated(lib):
    t = 2 * np.pi * np.arange(300) / 300
    q = np.stack([np.rint(524288 + 524288 * np.cos(t)), np.rint(524288 + 524288 * np.sin(t))], 1).astype(np.int64)
    q = np.minimum(q, QTOP)
    n = len(oh.hull(q.tolist()))
    assert n >= 200
    full, lists, ref_lists = run(q, 0, 1, 1024, what="circle, 1024")
    assert full[0]["n_vertices"] == full[0]["stored"] == n and full[0]["rect_edge"] >= 0
    exact, _, _ = run(q, 0, 1, n, what="circle, n")
    assert exact.tobytes() == full.tobytes()
    cut, cut_lists, _ = run(q, 0, 1, n - 1, what="circle, n - 1")
    assert cut[0]["n_vertices"] == n and cut[0]["stored"] == n - 1 and cut[0]["rect_edge"] == -1 and cut[0]["area2"] == full[0]["area2"]
    assert np.isnan(cut[0]["cx"]) and cut_lists[0].tolist() == lists[0, :n - 1].tolist()


def test_the_ends_of_the_coordinate_range(lib):
    top = QTOP
    for q in ([(0, 0), (top, 0), (top, top), (0, top), (top // 2, 1), (1, top // 3)], [(0, 1), (top, 0), (top - 1, top), (1, top - 1)], [(0, 0), (top, top)],
              [(top, 0), (0, top), (top, top)]):
        rows, _, ref_lists = run(q, 0, 1, 8, what="range ends %s" % (q,))
        e = oh.edge(ref_lists[0], int(rows[0]["rect_edge"]))
        assert e[0] * e[1] * e[2] < 1 << 124
    assert max(oh.edge([(0, 1), (top, 0), (top - 1, top), (1, top - 1)], 0)[:2]) > 1 << 40   # the extents need 64 bits, their product 128


def test_skipped_points(lib):
    q = [(100, 100), (900, 100), (900, 900), (100, 900)]
    xyz = np.concatenate([lattice(q), lattice(q)])
    xyz[4:, :2] += F32(3.0)
    xyz[7, 2] = np.nan                                    # a NaN z: never counted
    row = np.array([0, 0, 0, 0, -1, 5, 1, 1], np.int32)  # -1, a rank beyond a table of two rows
    rows, lists, _ = run(xyz, row, 2, 8, what="skipped points")
    assert rows[0]["n_vertices"] == 4 and rows[1]["points"] == 1 and rows[1]["n_vertices"] == 1
    out = xyz.copy()
    out[0, 0] = F32(-0.5)       # outside the grid
    out[1, 1] = F32(1024.0)
    out[2, 0] = np.nan
    rows, _, _ = run(out, row, 2, 8, what="points outside the grid")
    assert rows[0]["points"] == 1 and rows[0]["n_vertices"] == 1
    rows, _, _ = run(xyz, np.full(8, -1, np.int32), 3, 8, what="no point at all")
    assert all(is_empty(r) for r in rows)
    # off the lattice and off the origin: the quantisation is the boxes'
    rng = np.random.default_rng(3)
    far = (-1000.0, -1000.0, 4.0, 256, 256)
    pts = np.concatenate([rng.uniform(-1000.0, 24.0, (400, 2)), rng.uniform(0.0, 1.0, (400, 1))], 1).astype(F32)
    run(pts, rng.integers(-1, 4, 400), 3, 16, grid=far, what="far origin")


def test_random_sets_on_a_sub_lattice_and_the_invariants(lib):
    rng = np.random.default_rng(20261021)
    sets = 0
    for call in range(20):
        per_row, q, row = [], [], []
        for r in range(100):
            n = int(rng.integers(1, 201)) if r % 4 else int(rng.integers(1, 9))
            pitch, ox, oy = int(rng.integers(1, 60000)), int(rng.integers(0, 100000)), int(rng.integers(0, 100000))
            pts = np.stack([ox + pitch * rng.integers(0, 16, n), oy + pitch * rng.integers(0, 16, n)], 1)
            per_row.append(pts.tolist())
            q.append(pts)
            row.append(np.full(n, r))
        q, row = np.concatenate(q), np.concatenate(row)
        perm = rng.permutation(len(q))
        mv = 3 if call % 4 == 3 else 32
        rows, lists, ref_lists = run(q[perm], row[perm], 100, mv, what="random sets, call %d" % call)
        xyz = lattice(q)
        boxes = pwpp_hip.box_points(*GRID, xyz, np.ones(len(q), F32), row, 100)
        for r in range(100):
            v, n = ref_lists[r], len(ref_lists[r])
            assert rows[r]["points"] == len(per_row[r]) and rows[r]["n_vertices"] == n <= 32
            if n >= 2:
                pts = np.asarray(per_row[r], np.int64)   # (every cross below 2^43: exact in int64)
                for k in range(n):
                    a, b = v[k], v[(k + 1) % n]
                    assert ((b[0] - a[0]) * (pts[:, 1] - a[1]) - (b[1] - a[1]) * (pts[:, 0] - a[0]) >= 0).all(), "a point right of a hull edge"
                    assert n == 2 or oh.cross(a, b, v[(k + 2) % n]) > 0
            if rows[r]["rect_edge"] >= 0:
                assert oh.box_area_not_below(oh.edge(v, int(rows[r]["rect_edge"])), boxes[r]["ax"], boxes[r]["ay"], v), "the rectangle is larger than the box"
            else:
                assert n > mv
            sets += 1
    assert sets == 2000


def test_boxes_and_hulls_count_the_same_points(lib):
    """include/pwpp.h: pwpp_box_points and pwpp_hull_points count the same points (heights equal to z: both NaN rules agree).
    The cell rule written out: u = ((double)x - x0) / cell, kept iff 0 <= u < n."""
    x0, y0, cell, nx, ny, rows = 0.1, 0.0, 0.5, 8, 5, 6  # (x0 is no binary fraction: no float32 x makes dx zero)
    below, above = lambda v: np.nextafter(F32(v), F32(-np.inf)), lambda v: np.nextafter(F32(v), F32(np.inf))
    far = F32(x0 + nx * cell)
    edge = [(F32(x0), 1.0), (below(x0), 1.0),             # the float32 at x0 (just right of the double) and the one before it
            (far, 1.0), (below(far), 1.0), (above(far), 1.0),
            (1.0, -0.0), (1.0, below(0.0)), (1.0, F32(ny * cell)), (1.0, below(ny * cell)),
            (np.nan, 1.0), (1.0, np.inf), (-np.inf, 1.0)]
    rng = np.random.default_rng(17)
    xy = np.concatenate([np.array(edge, F32), (rng.random((40, 2)) * [nx * cell + 1.0, ny * cell + 1.0] + [x0 - 0.5, y0 - 0.5]).astype(F32)])
    xy = np.concatenate([xy, np.tile(np.array([[1.3, 0.8]], F32), (4, 1))])  # four points inside, for the rows at the table's ends
    z = rng.normal(0.0, 1.0, len(xy)).astype(F32)
    z[[14, 21, 30]] = np.nan
    row = rng.integers(-1, rows + 1, len(xy)).astype(np.int32)
    row[:len(edge)] = np.arange(len(edge)) % rows
    row[-4:] = [-1, 0, rows - 1, rows]
    xyz = np.concatenate([xy, z[:, None]], 1)
    with np.errstate(invalid="ignore"):
        u, v = (xy[:, 0].astype(np.float64) - x0) / cell, (xy[:, 1].astype(np.float64) - y0) / cell
        inside = (u >= 0.0) & (u < nx) & (v >= 0.0) & (v < ny)
    assert inside[:len(edge)].tolist() == [True, False, True, True, False, True, False, False, True, False, False, False]
    keep = inside & (row >= 0) & (row < rows) & ~np.isnan(z)
    want = np.bincount(row[keep], minlength=rows)
    assert 0 < keep.sum() < len(xy) and (want > 0).all() and (~keep[[14, 21, 30]]).all()
    boxes = pwpp_hip.box_points(x0, y0, cell, nx, ny, xyz, z, row, rows)
    hulls, _ = pwpp_hip.hull_points(x0, y0, cell, nx, ny, xyz, row, rows, 8)
    assert boxes["points"].tolist() == hulls["points"].tolist() == want.tolist()


def test_vertex_xy(lib):
    q = np.array([[0, 0], [1, 1024], [QTOP, 5]], np.int32)
    xy = pwpp_hip.hull_vertex_xy(-3.5, 2.25, 1.0, 8, 8, q)
    assert xy.dtype == np.float64 and xy.tolist() == [[-3.5, 2.25], [-3.5 + 1 / 1024.0, 3.25], [-3.5 + 1024.0, 2.25 + 5 / 1024.0]]


# ---- the same functions against a brute force, stand-alone ----------------------------------------------------------------------------
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def sanitizers_work(tmp_path):
    """The toolchain links the two runtimes into a program and that program starts in this environment."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        return False
    return subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0


def test_hull_check_program_builds_and_passes(tmp_path):
    exe = tmp_path / "hull_check"
    flags = SANITIZE if sanitizers_work(tmp_path) else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags +
                   ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "hull_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)  # (a stand-alone child process with its own main)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 mismatches" in r.stdout and "3349 cases" in r.stdout


CPP = r"""
#include "patchwork/patchworkpp.h"
#ifndef PWPP_HAS_OBSTACLE_HULLS
#error "include/pwpp.h does not announce the obstacle hulls"
#endif
static_assert(sizeof(pwpp_obstacle_hull) == 64 && alignof(pwpp_obstacle_hull) == 8, "64 bytes, 8-byte aligned");
double use(patchwork::PatchWorkpp &pw) {
    patchwork::PatchWorkpp::ObstacleHulls o = pw.getObstacleHulls(-40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f);
    patchwork::PatchWorkpp::ObstacleHulls d = pw.getObstacleHulls(-40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f, 16, 2, 4, true);
    double x = 0.0, y = 0.0;
    if (o.count) o.vertexXY(0, 0, x, y);
    return x + y + o.label[3 * 160 + 5] + o.count + (o.count ? o.hulls[0].length * o.hulls[0].ax + (double)o.hulls[0].area2 + o.vertices[0] : 0) + d.count;
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_method_compiles(tmp_path, flavour):
    src = tmp_path / "obstacle_hulls.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    cmd += ["-DPWPP_NO_EIGEN"] if flavour == "plain" else ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "hulls.c"
    src.write_text('#include "pwpp.h"\nint f(void) { pwpp_obstacle_hull r; r.points = 0; r.area2 = 0; r.width = 0.0f; return (int)sizeof(r) + r.points + (int)r.area2 + (int)r.width; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
