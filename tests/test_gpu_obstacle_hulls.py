"""The obstacle hulls (pwpp_hull_obstacles) on a real MI355X, byte for byte: against pwpp_hull_points (the same functions on the
host) and against the restatement of tests/obstacle_hulls_ref.py (a monotone chain, every edge tried in Python integers), both fed
from the library's own non-ground rows and ground queries by the recipe of the box tests -- on the labels of pwpp_label_obstacles
and on edited label images, with and without vertex lists, with lists too short for a row, at every value of the option
"hulls_path", on a frame sub-range, far from the grid's origin where q is largest, from host and from misaligned device memory --
and that asking changes nothing else.  No tolerance anywhere.  The clouds have ~3 k points (the far-origin one ~11 k) with planted
outlines: a square, an L of two walls, a circle of hundreds of vertices, a diagonal wall; grids of 64 x 64 cells of 0.5 m."""
import ctypes

import numpy as np
import pytest

import obstacle_hulls_ref as oh
import pwpp_hip
import pwpp_synth
from test_gpu_obstacle_boxes import counted_points
from test_gpu_obstacle_clusters import GRIDS
from test_gpu_obstacle_grid import _everything, inner_cloud, small_cloud

pytestmark = pytest.mark.gpu

F32 = np.float32
E_ARG, E_STATE = -1, -4
BAND = (0.2, 2.5)
PATHS = (0, 1, 2)
GRID = GRIDS[0]  # (-16, -16, 0.5, 64, 64)


def planted(seed):
    """small_cloud(seed) with outlines standing on the level ground around it, each at three heights (so every (x, y) comes thrice)."""
    base = small_cloud(seed)
    s = np.arange(0.0, 3.0, 0.25)
    square = [(8 + t, 8.0) for t in s] + [(11.0, 8 + t) for t in s] + [(11 - t, 11.0) for t in s] + [(8.0, 11 - t) for t in s]
    ell = [(-12 + t, -12.0) for t in np.arange(0.0, 6.01, 0.25)] + [(-12.0, -12 + t) for t in np.arange(0.25, 3.01, 0.25)]
    a = 2 * np.pi * np.arange(240) / 240
    circle = list(zip(-9 + 2.5 * np.cos(a), 9 + 2.5 * np.sin(a)))
    wall = [(6 + t, -12 + t) for t in np.arange(0.0, 6.01, 0.2)]
    xy = np.array(square + ell + circle + wall, np.float64)
    rows = [np.concatenate([xy, np.full((len(xy), 1), -1.723 + hgt), np.full((len(xy), 1), 0.5)], 1) for hgt in (0.5, 1.0, 1.5)]
    return np.ascontiguousarray(np.concatenate([base] + rows), F32)


def restated(h, label, grid, band, max_hulls, max_vertices, first=0):
    """Per frame (rows, lists) twice: through pwpp_hull_points and through the restatement."""
    host, ref = [], []
    for fr in range(label.shape[0]):
        xyz, hgt, iy, ix = counted_points(h, first + fr, grid, band)
        row = label[fr, iy, ix].astype(np.int32)
        host.append(pwpp_hip.hull_points(*grid, xyz, row, max_hulls, max_vertices))
        ref.append(oh.hull_rows(*grid, xyz, row, max_hulls, max_vertices))
    return host, ref


def on_every_path(h, grid, band, label, max_hulls, max_vertices, **kw):
    """hull_obstacles at every value of "hulls_path", with and without a list: identical rows, identical stored vertices."""
    runs = []
    for path in PATHS:
        h.set_option("hulls_path", path)
        rows, lists = h.hull_obstacles(*grid, *band, label, max_hulls, max_vertices, **kw)
        bare, none = h.hull_obstacles(*grid, *band, label, max_hulls, max_vertices, with_vertices=False, **kw)
        assert none is None and bare.tobytes() == rows.tobytes(), "hulls_path %d: the rows depend on whether a list is asked for" % path
        runs.append((rows, lists))
    h.set_option("hulls_path", 0)
    stored = runs[0][0]["stored"]
    for path, (rows, lists) in zip(PATHS[1:], runs[1:]):
        assert rows.tobytes() == runs[0][0].tobytes(), "hulls_path %d differs from hulls_path 0" % path
        for fr, r in zip(*np.nonzero(stored)):
            assert lists[fr, r, :stored[fr, r]].tobytes() == runs[0][1][fr, r, :stored[fr, r]].tobytes(), "hulls_path %d: the list of frame %d row %d" % (path, fr, r)
    return runs[0]


def check(h, grid, band, label, max_hulls, max_vertices, what, **kw):
    rows, lists = on_every_path(h, grid, band, label, max_hulls, max_vertices, **kw)
    host, ref = restated(h, label, grid, band, max_hulls, max_vertices, kw.get("frame_first", 0))
    assert rows.dtype == oh.HULL_DTYPE and rows.shape == (label.shape[0], max_hulls) and lists.shape == rows.shape + (max_vertices, 2), what
    for fr in range(label.shape[0]):
        oh.same(host[fr][0], host[fr][1], ref[fr][0], ref[fr][1], "%s, frame %d, pwpp_hull_points against the restatement" % (what, fr))
        oh.same(rows[fr], lists[fr], ref[fr][0], ref[fr][1], "%s, frame %d" % (what, fr))
    return rows, lists, [r[1] for r in ref]


def empty_rows(rows):
    w = np.frombuffer(np.ascontiguousarray(rows).tobytes(), np.uint32).reshape(-1, 16)
    return (w[:, [0, 1, 2, 4, 5, 6, 7, 8, 9]] == 0).all() and (w[:, 3] == 0xffffffff).all() and (w[:, 10:] == 0x7fc00000).all()


@pytest.fixture(scope="module")
def scan():
    """A handle after three frames: a scan with planted outlines (its list length is no multiple of 64), an empty frame, a frame
    that is all unref."""
    h = pwpp_hip.Handle()
    h.estimate_ground_batch([planted(5), np.zeros((0, 4), F32), inner_cloud()], mode=pwpp_hip.MODE_FRESH)
    return h


@pytest.fixture(scope="module")
def labels(scan):
    label, table, n = scan.label_obstacles(*GRID, *BAND, 1, 8, max_clusters=256)
    assert 4 <= n[0] <= 256 and n[1] == 0 and n[2] == 0
    return label, table, int(n[0])


# ---- the labels of pwpp_label_obstacles ---------------------------------------------------------------------------------------------
def test_cluster_labels_against_the_host_function_and_the_restatement(scan, labels):
    h = scan
    label, table, n0 = labels
    full, lists, ref_lists = check(h, GRID, BAND, label, n0, 1024, "max_vertices 1024")
    assert np.array_equal(full["points"][0], table["points"][0, :n0]), "points differ from the cluster rows'"
    assert (full["n_vertices"][0] >= 1).all() and (full["rect_edge"][0] >= 0).all() and empty_rows(full[1:])
    most = int(full["n_vertices"][0].max())
    print("clusters %d, vertices per row %s" % (n0, sorted(full["n_vertices"][0].tolist())))
    assert most > 32, "the planted circle is not among the clusters"
    # the invariants of the header: every counted point left of or on every edge; the rectangle no larger than the box of the row
    boxes = h.box_obstacles(*GRID, *BAND, label, n0)
    xyz, hgt, iy, ix = counted_points(h, 0, GRID, BAND)
    q, row = oh.quantise(GRID[0], GRID[1], xyz), label[0, iy, ix]
    for r in range(n0):
        v, pts = ref_lists[0][r], q[row == r]
        assert len(pts) == full["points"][0, r] == boxes["points"][0, r]
        for k in range(len(v) if len(v) >= 2 else 0):
            a, b = v[k], v[(k + 1) % len(v)]
            assert ((b[0] - a[0]) * (pts[:, 1] - a[1]) - (b[1] - a[1]) * (pts[:, 0] - a[0]) >= 0).all(), "row %d: a point right of edge %d" % (r, k)
        assert oh.box_area_not_below(oh.edge(v, int(full["rect_edge"][0, r])), boxes["ax"][0, r], boxes["ay"][0, r], v), "row %d: the rectangle is larger than the box" % r
    # lists too short for some rows: 32 (the circle), 3, 1
    for mv in (32, 3, 1):
        cut, cut_lists, _ = check(h, GRID, BAND, label, n0, mv, "max_vertices %d" % mv)
        over = full["n_vertices"][0] > mv
        assert over.any() and (cut["rect_edge"][0][over] == -1).all() and np.isnan(cut["cx"][0][over]).all()
        assert np.array_equal(cut["n_vertices"], full["n_vertices"]) and np.array_equal(cut["area2"], full["area2"]) and np.array_equal(cut["points"], full["points"])
        assert np.ascontiguousarray(cut[0][~over]).tobytes() == np.ascontiguousarray(full[0][~over]).tobytes()
    # a shorter table drops rows and nothing else; a longer one has empty rows behind
    few, _, _ = check(h, GRID, BAND, label, n0 - 1, 32, "one row less")
    both, _, _ = check(h, GRID, BAND, label, n0 + 3, 32, "three rows more")
    assert np.ascontiguousarray(both[:, :n0 - 1]).tobytes() == few.tobytes() and empty_rows(both[:, n0:])


# ---- edited label images ----------------------------------------------------------------------------------------------------------
def test_edited_label_images(scan, labels):
    h = scan
    label, _, n0 = labels
    x0, y0, cell, nx, ny = GRID
    counted = len(counted_points(h, 0, GRID, BAND)[0])
    # every cluster merged into row 0: one row holds all counted points of the labelled cells
    merged = np.where(label >= 0, 0, -1).astype(np.int32)
    one, _, _ = check(h, GRID, BAND, merged, 1, 64, "every cluster merged into row 0")
    assert one["points"][0, 0] == counted > 500 and one["n_vertices"][0, 0] >= 5 and empty_rows(one[1:])
    # every cell 0, the unlabelled ones too (min_count 1: the same points)
    zero, _, _ = check(h, GRID, BAND, np.zeros((3, ny, nx), np.int32), 2, 64, "every label 0")
    assert zero[0, 0].tobytes() == one[0, 0].tobytes() and empty_rows(zero[:, 1:])
    # rows dropped: every second cluster, and a checkerboard of -1 over up to 64 distinct rows inside a wave
    dropped = np.where(label % 2 == 1, -1, label).astype(np.int32)
    half, _, _ = check(h, GRID, BAND, dropped, n0, 32, "every second cluster dropped")
    assert empty_rows(half[0, 1::2]) and (half["points"][0, 0::2] > 0).all()
    cells = np.arange(nx * ny, dtype=np.int32).reshape(ny, nx)
    yy, xx = np.mgrid[0:ny, 0:nx]
    board = np.broadcast_to(np.where((xx + yy) % 2 == 0, -1, cells % 64), (3, ny, nx)).astype(np.int32)
    mixed, _, _ = check(h, GRID, BAND, board, 64, 16, "a checkerboard of -1")
    assert 0 < mixed["points"].sum() < counted
    # ranks beyond the table, and negative ones of every size
    wild = np.broadcast_to(cells % 7, (3, ny, nx)).copy()
    wild[:, ::3, :] = np.iinfo(np.int32).max
    wild[:, 1::3, ::2] = np.iinfo(np.int32).min
    few, _, _ = check(h, GRID, BAND, wild, 5, 16, "ranks beyond the table")
    assert 0 < few["points"].sum() < counted


# ---- a frame sub-range --------------------------------------------------------------------------------------------------------------
def test_three_frames_and_frame_first_above_zero():
    h = pwpp_hip.Handle()
    h.estimate_ground_batch([small_cloud(6), planted(7), small_cloud(8)], mode=pwpp_hip.MODE_FRESH)
    label, _, n = h.label_obstacles(*GRID, *BAND, 1, 8, max_clusters=256)
    rows = int(n.max())
    assert n.min() >= 3
    full, lists, _ = check(h, GRID, BAND, label, rows, 32, "three frames")
    assert (full["points"][:, 0] > 0).all()
    for first, frames in ((1, 2), (2, 1), (1, 1)):
        sub, sub_lists, _ = check(h, GRID, BAND, label[first:first + frames], rows, 32, "frames %d..%d" % (first, first + frames), frame_first=first, frames=frames)
        assert sub.tobytes() == np.ascontiguousarray(full[first:first + frames]).tobytes()


# ---- far from the origin ----------------------------------------------------------------------------------------------------------
def test_far_origin_has_the_largest_q():
    grid = (-1000.0, -1000.0, 4.0, 256, 256)
    band = (-np.inf, np.inf)
    h = pwpp_hip.Handle()
    h.estimate_ground_batch([pwpp_synth.make_cloud(21, beams=32, azimuth_steps=400)], mode=pwpp_hip.MODE_FRESH)
    rows, _, _ = check(h, grid, band, np.zeros((1, 256, 256), np.int32), 1, 64, "far origin")
    r = rows[0, 0]
    assert r["points"] >= 4096 and r["qx_max"] > 1000 * 1024 and r["qy_max"] > 1000 * 1024 and r["n_vertices"] >= 8
    assert r["area2"] > 1 << 31


# ---- device memory ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_device_memory_label_one_word_off_a_16_byte_boundary(scan, labels, path):
    import torch
    h = scan
    label, _, n0 = labels
    x0, y0, cell, nx, ny = GRID
    rows, mv = n0 + 2, 32
    want, want_lists = h.hull_obstacles(*GRID, *BAND, label, rows, mv)
    cells = 3 * nx * ny
    d_label = torch.full((cells + 8,), -7, dtype=torch.int32, device="cuda")
    d_hulls = torch.full((3 * rows * 16 + 8,), -7, dtype=torch.int32, device="cuda")
    d_lists = torch.full((3 * rows * mv * 2 + 8,), -7, dtype=torch.int32, device="cuda")
    assert d_label.data_ptr() % 16 == 0 and d_hulls.data_ptr() % 16 == 0 and d_lists.data_ptr() % 16 == 0
    d_label[1:1 + cells] = torch.from_numpy(label.reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    L = pwpp_hip.load()
    g = pwpp_hip.GroundGrid(x0, y0, cell, nx, ny, 0, 0)
    dp = ctypes.c_void_p
    for mem, at in ((pwpp_hip.MEM_HOST_PINNED, 8), (pwpp_hip.MEM_DEVICE, 4), (pwpp_hip.MEM_DEVICE, 12)):   # pinned memory; a table off its 8 bytes
        assert L.pwpp_hull_obstacles(h._h, ctypes.byref(g), BAND[0], BAND[1], 0, 3, mem, dp(d_label.data_ptr() + 4), dp(d_hulls.data_ptr() + at), rows,
                                     dp(d_lists.data_ptr() + 4), mv) == E_ARG, (mem, at)
    h.set_option("hulls_path", path)
    h.hull_obstacles_device(*GRID, *BAND, d_label.data_ptr() + 4, d_hulls.data_ptr() + 8, rows, d_lists.data_ptr() + 4, mv)
    h.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
    raw_l, raw_h, raw_v = d_label.cpu().numpy(), d_hulls.cpu().numpy(), d_lists.cpu().numpy()
    d_hulls.fill_(-7)
    torch.cuda.synchronize()
    h.hull_obstacles_device(*GRID, *BAND, d_label.data_ptr() + 4, d_hulls.data_ptr() + 8, rows, None, mv)   # no lists
    h.synchronize()
    h.set_option("hulls_path", 0)
    assert d_hulls.cpu().numpy().tobytes() == raw_h.tobytes(), "the rows depend on whether a list is asked for"
    assert raw_h[2:2 + 3 * rows * 16].tobytes() == want.tobytes()
    assert (raw_h[:2] == -7).all() and (raw_h[2 + 3 * rows * 16:] == -7).all(), "a word outside the hull table was written"
    got_lists = raw_v[1:1 + 3 * rows * mv * 2].reshape(3, rows, mv, 2)
    for fr, r in zip(*np.nonzero(want["stored"])):
        k = want["stored"][fr, r]
        assert got_lists[fr, r, :k].tobytes() == want_lists[fr, r, :k].tobytes()
    assert raw_v[0] == -7 and (raw_v[1 + 3 * rows * mv * 2:] == -7).all(), "a word outside the vertex lists was written"
    assert raw_l[0] == -7 and (raw_l[1 + cells:] == -7).all() and np.array_equal(raw_l[1:1 + cells], label.reshape(-1)), "the label image was written"


# ---- nothing else moves -----------------------------------------------------------------------------------------------------------
def test_estimate_hulls_estimate_and_the_workspace_after_trim():
    first, second = [small_cloud(s) for s in (5, 6, 7)], [small_cloud(s) for s in (8, 9, 10)]
    grid = (-20.0, -20.0, 0.5, 80, 80)
    h = pwpp_hip.Handle()
    h.set_order(pwpp_hip.ORDER_CLOUD)
    h.set_num_streams(3)
    ref = pwpp_hip.Handle()
    ref.set_order(pwpp_hip.ORDER_CLOUD)
    ref.set_num_streams(3)
    for w in (h, ref):
        w.estimate_ground_batch(first, mode=pwpp_hip.MODE_STREAMS)
    assert h.workspace_bytes() == ref.workspace_bytes()   # with the feature unused nothing is allocated
    before, t_before = _everything(h, 3), h.time_us()
    label = np.broadcast_to(np.arange(80 * 80, dtype=np.int32).reshape(80, 80) % 16, (3, 80, 80)).copy()   # (no labelling: the cluster buffer is the hulls' alone)
    rows, _ = on_every_path(h, grid, BAND, label, 16, 32)
    assert (rows["points"].sum(1) > 100).all()   # (every frame's points reached some row)
    assert h.workspace_bytes() > ref.workspace_bytes(), "accumulators and arena are not counted by pwpp_get_workspace_bytes"
    assert _everything(h, 3) == before and h.time_us() == t_before, "the hulls changed the results of the call they read"
    for w in (h, ref):
        w.estimate_ground_batch(second, mode=pwpp_hip.MODE_STREAMS)
    assert _everything(ref, 3) == _everything(h, 3), "the hulls between two calls changed the second call's outputs"
    h.trim_workspace()
    ref.trim_workspace()
    assert h.workspace_bytes() == ref.workspace_bytes(), "pwpp_trim_workspace did not free the cluster buffer"


def test_state_and_arguments():
    L = pwpp_hip.load()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lab = np.zeros(3 * 16, np.int32)
    out = np.zeros(3 * 2, oh.HULL_DTYPE)
    g = pwpp_hip.GroundGrid(-2.0, -2.0, 1.0, 4, 4, 0, 0)

    def hulls(h, first=0, frames=1, mem=pwpp_hip.MEM_HOST, grid=g, max_vertices=4):
        return L.pwpp_hull_obstacles(h._h, ctypes.byref(grid), 0.2, 2.5, first, frames, mem, vp(lab), vp(out), 2, None, max_vertices)

    h = pwpp_hip.Handle()
    empty = h.workspace_bytes()
    assert hulls(h) == E_STATE  # before any estimate call
    assert h.workspace_bytes() == empty
    h.estimate_ground_batch([small_cloud(5), np.zeros((0, 4), F32), inner_cloud()], mode=pwpp_hip.MODE_FRESH)
    assert hulls(h, 0, 3) == 0 and hulls(h, 2, 1) == 0
    for first, n in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2)):
        assert hulls(h, first, n) == E_ARG, (first, n)
    assert hulls(h, mem=pwpp_hip.MEM_HOST_PINNED) == E_ARG
    assert hulls(h, max_vertices=0) == E_ARG and hulls(h, max_vertices=1025) == E_ARG and hulls(h, max_vertices=1024) == 0
    for bad in (dict(nx=0), dict(cell=0.0), dict(cell=np.nan), dict(flags=2), dict(nx=1025)):
        kw = dict(dict(x0=-2.0, y0=-2.0, cell=1.0, nx=4, ny=4, flags=0, pad_=0), **bad)
        assert hulls(h, grid=pwpp_hip.GroundGrid(**kw)) == E_ARG, bad
    with pytest.raises(pwpp_hip.PwppError):
        h.set_option("hulls_path", 3)
    h.trim_workspace()
    assert hulls(h) == E_STATE  # after pwpp_trim_workspace


def test_pybind_module_agrees_with_the_ctypes_handle():
    import pypatchworkpp
    pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    h = pwpp_hip.Handle()
    grid = (-30.0, -12.0, 0.5, 120, 48)
    with pytest.raises(RuntimeError):
        pp.getObstacleHulls(*grid, 0.2, 2.5)  # no frame yet
    pts = small_cloud(5)
    pp.estimateGround(pts)
    h.estimate_ground(pts)
    for mv, min_count, conn, ground_only in ((32, 1, 8, False), (3, 2, 4, True)):
        label, table, hulls, vertices, n = pp.getObstacleHulls(*grid, 0.2, 2.5, mv, min_count, conn, ground_only)
        hl, ht, hn = h.label_obstacles(*grid, 0.2, 2.5, min_count, conn, max_clusters=256, ground_only=ground_only)
        hh, hv = h.hull_obstacles(*grid, 0.2, 2.5, hl, int(hn[0]), mv, ground_only=ground_only)
        assert label.shape == (48, 120) and n == hn[0] >= 3 and len(table) == n == len(hulls) and vertices.shape == (n, mv, 2)
        assert hulls.dtype.names == oh.HULL_DTYPE.names and hulls.dtype.itemsize == 64
        assert label.tobytes() == hl[0].tobytes() and table.tobytes() == ht[0, :n].tobytes() and hulls.tobytes() == hh[0].tobytes()
        for r in range(n):
            assert vertices[r, :hulls["stored"][r]].tobytes() == hv[0, r, :hulls["stored"][r]].tobytes()
    with pytest.raises(RuntimeError):
        pp.getObstacleHulls(0.0, 0.0, 1.0, 4, 4, 0.2, 2.5, 32, 1, 5)  # connectivity 5
