"""The obstacle boxes (pwpp_box_obstacles) on a real MI355X, byte for byte: against pwpp_box_points (the same functions on the
host) and against the restatement of tests/obstacle_boxes_ref.py, both fed from the library's own non-ground rows, ground queries
and the cell arithmetic of the obstacle grid's restatement -- on the labels of pwpp_label_obstacles and on edited label images,
with truncated and oversized tables, at every value of the option "boxes_path", far from the grid's origin where the products
need 128 bits, in every kind of call, into misaligned device memory -- and that asking changes nothing else.  No tolerance
anywhere.  The clouds have ~3 k points (the far-origin one ~11 k), the grids at most 64 x 64 cells (256 x 256 there)."""
import ctypes

import numpy as np
import pytest

import obstacle_boxes_ref as ob
import obstacle_grid_ref as og
import pwpp_hip
import pwpp_synth
from test_gpu_obstacle_clusters import GRIDS
from test_gpu_obstacle_grid import _everything, device_tensor, small_cloud, three_frames

pytestmark = pytest.mark.gpu

F32 = np.float32
E_ARG, E_STATE = -1, -4
BAND = (0.2, 2.5)
PATHS = (0, 1, 2)


def counted_points(h, f, grid, band):
    """(xyz, hgt, iy, ix) of frame f's counted points, from the library's own rows and queries."""
    x0, y0, cell, nx, ny = grid
    xyz = h.nonground(f)
    if len(xyz) == 0:
        return np.zeros((0, 3), F32), np.zeros(0, F32), np.zeros(0, np.int64), np.zeros(0, np.int64)
    s = h.query_ground(xyz, frames=f)
    kx, ix = og.cells_of(xyz[:, 0], x0, cell, nx)
    ky, iy = og.cells_of(xyz[:, 1], y0, cell, ny)
    hgt = np.ascontiguousarray(s["distance"], F32)
    with np.errstate(invalid="ignore"):
        counted = kx & ky & (s["patch"] >= 0) & (F32(band[0]) <= hgt) & (hgt <= F32(band[1]))
    return np.ascontiguousarray(xyz[counted, :3], F32), hgt[counted], iy[counted], ix[counted]


def restated(h, label, grid, band, max_boxes, first=0):
    """The (frames, max_boxes) rows twice: through pwpp_box_points and through the numpy restatement."""
    host, ref = [], []
    for fr in range(label.shape[0]):
        xyz, hgt, iy, ix = counted_points(h, first + fr, grid, band)
        row = label[fr, iy, ix].astype(np.int32)
        host.append(pwpp_hip.box_points(*grid, xyz, hgt, row, max_boxes))
        ref.append(ob.box_rows(*grid, xyz, hgt, row, max_boxes))
    return np.stack(host), np.stack(ref)


def on_every_path(h, grid, band, label, max_boxes, **kw):
    """box_obstacles at every value of "boxes_path": identical bytes; the option is left at its default."""
    runs = []
    for path in PATHS:
        h.set_option("boxes_path", path)
        runs.append(h.box_obstacles(*grid, *band, label, max_boxes, **kw))
    h.set_option("boxes_path", 0)
    for path, r in zip(PATHS[1:], runs[1:]):
        assert r.tobytes() == runs[0].tobytes(), "boxes_path %d differs from boxes_path 0" % path
    return runs[0]


def check(h, grid, band, label, max_boxes, what, **kw):
    got = on_every_path(h, grid, band, label, max_boxes, **kw)
    host, ref = restated(h, label, grid, band, max_boxes, kw.get("frame_first", 0))
    assert got.dtype == ob.BOX_DTYPE and got.shape == (label.shape[0], max_boxes), what
    assert host.tobytes() == ref.tobytes(), what + ": pwpp_box_points differs from the restatement"
    for fr in range(label.shape[0]):
        for r in range(max_boxes):
            assert got[fr, r].tobytes() == ref[fr, r].tobytes(), "%s, frame %d row %d:\n%s\n%s" % (what, fr, r, got[fr, r], ref[fr, r])
    return got


def empty_rows(rows):
    w = np.frombuffer(np.ascontiguousarray(rows).tobytes(), np.uint32).reshape(-1, 16)
    return (w[:, :2] == 0).all() and (w[:, 2:] == og.QNAN_BITS).all()


@pytest.fixture(scope="module")
def scan():
    """A handle after the three frames of the cluster tests: a 16-beam scan (its list length is no multiple of 64), an empty
    frame, a frame that is all unref."""
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(three_frames(), mode=pwpp_hip.MODE_FRESH)
    assert h.counts(0)[1] % 64 != 0
    return h


# ---- the labels of pwpp_label_obstacles ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS, ids=["64x64", "65x17"])
def test_cluster_labels_against_the_host_function_and_the_restatement(scan, grid):
    h = scan
    for min_count, conn in ((1, 8), (1, 4), (2, 8)):
        label, table, n = h.label_obstacles(*grid, *BAND, min_count, conn, max_clusters=64)
        n0 = int(n[0])
        assert 1 <= n0 <= 64 and n[1] == 0 and n[2] == 0
        what = "min_count %d connectivity %d" % (min_count, conn)
        full = check(h, grid, BAND, label, n0, what)
        # the cross-checks against the cluster table
        assert np.array_equal(full["points"][0], table["points"][0, :n0]), what + ": points differ from the cluster rows'"
        assert full["h_max"][0].tobytes() == table["top"][0, :n0].tobytes(), what + ": h_max has not the bits of the cluster rows' top"
        assert (full["points"][0] >= min_count).all() and empty_rows(full[1:])   # the empty frame, the all-unref frame
        assert (full["length"][0] >= 0).all() and (full["width"][0] >= 0).all() and (full["sigma_long"][0] >= full["sigma_short"][0]).all()
        assert (full["h_min"][0] >= F32(BAND[0])).all() and (full["h_max"][0] <= F32(BAND[1])).all()
        # a shorter table drops rows and nothing else; a longer one has empty rows behind
        for rows in sorted({max(n0 - 1, 1), 1}):
            cut = check(h, grid, BAND, label, rows, "%s, max_boxes %d of %d" % (what, rows, n0))
            assert cut.tobytes() == np.ascontiguousarray(full[:, :rows]).tobytes()
        more = check(h, grid, BAND, label, n0 + 3, what + ", three rows more")
        assert np.ascontiguousarray(more[:, :n0]).tobytes() == full.tobytes() and empty_rows(more[:, n0:])


# ---- edited label images ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS, ids=["64x64", "65x17"])
def test_edited_label_images(scan, grid):
    h = scan
    x0, y0, cell, nx, ny = grid
    cells = np.arange(nx * ny, dtype=np.int32).reshape(ny, nx)
    counted = sum(len(counted_points(h, f, grid, BAND)[0]) for f in range(3))
    # every label 0: one box of everything counted
    one = check(h, grid, BAND, np.zeros((3, ny, nx), np.int32), 1, "every label 0")
    assert one["points"][0, 0] == counted > 100 and empty_rows(one[1:])
    # up to 64 distinct rows inside a wave
    mod = np.broadcast_to(cells % 64, (3, ny, nx)).copy()
    many = check(h, grid, BAND, mod, 64, "label = cell % 64")
    assert many["points"].sum() == counted and (many["points"][0] > 0).sum() >= (8 if cell == 0.5 else 2)   # (the coarse grid sees 283 points in a few cells)
    # a checkerboard of -1
    yy, xx = np.mgrid[0:ny, 0:nx]
    board = np.where((xx + yy) % 2 == 0, -1, mod).astype(np.int32)
    half = check(h, grid, BAND, board, 64, "a checkerboard of -1")
    assert 0 < half["points"].sum() < counted
    # labels >= max_boxes are skipped, as are negative ones of every size
    wild = np.broadcast_to(cells % 7, (3, ny, nx)).copy()   # (5 and 6 are beyond a table of five rows)
    wild[:, ::3, :] = np.iinfo(np.int32).max
    wild[:, 1::3, ::2] = np.iinfo(np.int32).min
    few = check(h, grid, BAND, wild, 5, "labels beyond the table")
    assert 0 < few["points"].sum() < counted


# ---- far from the origin ----------------------------------------------------------------------------------------------------------
def test_far_origin_needs_128_bit_products():
    grid = (-1000.0, -1000.0, 4.0, 256, 256)
    band = (-np.inf, np.inf)
    h = pwpp_hip.Handle()
    h.estimate_ground_batch([pwpp_synth.make_cloud(21, beams=32, azimuth_steps=400)], mode=pwpp_hip.MODE_FRESH)
    xyz = counted_points(h, 0, grid, band)[0]
    N, Sx, Sy, Sxx, Sxy, Syy = ob.row_moments(grid[0], grid[1], xyz)
    print("far origin: N = %d, N * Sxx = 2^%.2f" % (N, np.log2(float(N * Sxx))))
    assert N >= 4096 and N * Sxx >= 1 << 64, "the cloud is too small for the case"
    got = check(h, grid, band, np.zeros((1, 256, 256), np.int32), 1, "far origin")
    assert got["points"][0, 0] == N


# ---- every kind of call -----------------------------------------------------------------------------------------------------------
def test_every_kind_of_call_gives_the_same_bytes():
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
    grid = GRIDS[0]

    def boxes(h):
        label, table, n = h.label_obstacles(*grid, *BAND, 1, 8, max_clusters=64)
        assert n[0] >= 3
        got = check(h, grid, BAND, label, int(n[0]), "")
        sub = on_every_path(h, grid, BAND, label[2:], int(n[0]), frame_first=2, frames=1)   # a frame sub-range
        assert sub.tobytes() == np.ascontiguousarray(got[2:]).tobytes()
        first = on_every_path(h, grid, BAND, label[:1], int(n[0]), frame_first=0, frames=1)
        assert first.tobytes() == np.ascontiguousarray(got[:1]).tobytes()
        return label.tobytes(), got.tobytes()

    a = pwpp_hip.Handle()
    a.set_input_transforms(T)
    a.estimate_ground_batch(sensor, mode=pwpp_hip.MODE_FRESH)
    with_transform = boxes(a)
    b = pwpp_hip.Handle()
    b.set_order(pwpp_hip.ORDER_CLOUD)
    b.estimate_ground_batch(pre, mode=pwpp_hip.MODE_FRESH)
    cloud_order = boxes(b)
    c = pwpp_hip.Handle()
    tens = [device_tensor(f) for f in pre]
    c.estimate_ground_batch_device([t.data_ptr() for t in tens], [len(f) for f in pre])
    after_device_call = boxes(c)  # (the input is alive: `tens`)
    assert with_transform == cloud_order == after_device_call
    del tens


# ---- device memory ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_device_memory_one_word_off_a_16_byte_boundary(scan, path):
    import torch
    h = scan
    grid = GRIDS[1]
    x0, y0, cell, nx, ny = grid
    label, _, n = h.label_obstacles(*grid, *BAND, 1, 8, max_clusters=64)
    rows = int(n[0]) + 2
    want = h.box_obstacles(*grid, *BAND, label, rows)
    cells = 3 * nx * ny
    d_label = torch.full((cells + 8,), -7, dtype=torch.int32, device="cuda")
    d_boxes = torch.full((3 * rows * 16 + 8,), -7, dtype=torch.int32, device="cuda")
    assert d_label.data_ptr() % 16 == 0 and d_boxes.data_ptr() % 16 == 0
    d_label[1:1 + cells] = torch.from_numpy(label.reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    h.set_option("boxes_path", path)
    h.box_obstacles_device(*grid, *BAND, d_label.data_ptr() + 4, d_boxes.data_ptr() + 4, rows)
    h.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
    h.set_option("boxes_path", 0)
    raw_l, raw_b = d_label.cpu().numpy(), d_boxes.cpu().numpy()
    assert raw_b[1:1 + 3 * rows * 16].tobytes() == want.tobytes()
    assert raw_b[0] == -7 and (raw_b[1 + 3 * rows * 16:] == -7).all(), "a word outside the box table was written"
    assert raw_l[0] == -7 and (raw_l[1 + cells:] == -7).all() and np.array_equal(raw_l[1:1 + cells], label.reshape(-1)), "the label image was written"


# ---- nothing else moves -----------------------------------------------------------------------------------------------------------
def test_asking_changes_nothing_else():
    first, second = [small_cloud(s) for s in (5, 6, 7)], [small_cloud(s) for s in (8, 9, 10)]
    grid = (-20.0, -20.0, 0.5, 80, 80)
    h = pwpp_hip.Handle()
    h.set_order(pwpp_hip.ORDER_CLOUD)
    h.set_num_streams(3)
    h.estimate_ground_batch(first, mode=pwpp_hip.MODE_STREAMS)
    before, t_before = _everything(h, 3), h.time_us()
    records = [h.nonground_records(f).tobytes() for f in range(3)]
    label, _, n = h.label_obstacles(*grid, *BAND, 1, 8, max_clusters=16)
    boxes = on_every_path(h, grid, BAND, label, 16)
    assert n.min() >= 3 and (boxes["points"][:, :3] > 0).all()
    assert _everything(h, 3) == before and h.time_us() == t_before, "the boxes changed the results of the call they read"
    assert records == [h.nonground_records(f).tobytes() for f in range(3)]
    h.estimate_ground_batch(second, mode=pwpp_hip.MODE_STREAMS)
    asked = _everything(h, 3)
    ref = pwpp_hip.Handle()
    ref.set_order(pwpp_hip.ORDER_CLOUD)
    ref.set_num_streams(3)
    ref.estimate_ground_batch(first, mode=pwpp_hip.MODE_STREAMS)
    ref.estimate_ground_batch(second, mode=pwpp_hip.MODE_STREAMS)
    assert _everything(ref, 3) == asked, "the boxes between two calls changed the second call's outputs"


def test_state_workspace_and_arguments():
    L = pwpp_hip.load()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lab = np.zeros(3 * 16, np.int32)
    box = np.zeros(3 * 2, ob.BOX_DTYPE)
    g = pwpp_hip.GroundGrid(-2.0, -2.0, 1.0, 4, 4, 0, 0)

    def boxes(h, first=0, frames=1, mem=pwpp_hip.MEM_HOST, grid=g):
        return L.pwpp_box_obstacles(h._h, ctypes.byref(grid), 0.2, 2.5, first, frames, mem, vp(lab), vp(box), 2)

    h = pwpp_hip.Handle()
    empty = h.workspace_bytes()
    assert boxes(h) == E_STATE  # before any estimate call
    assert h.workspace_bytes() == empty
    frames = three_frames()
    a, b = pwpp_hip.Handle(), pwpp_hip.Handle()
    for w in (a, b):
        w.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert a.workspace_bytes() == b.workspace_bytes()  # with the feature unused nothing is allocated
    assert boxes(b, 0, 3) == 0
    assert b.workspace_bytes() > a.workspace_bytes(), "the accumulators are not counted by pwpp_get_workspace_bytes"
    b.trim_workspace()
    a.trim_workspace()
    assert a.workspace_bytes() == b.workspace_bytes(), "pwpp_trim_workspace did not free the cluster buffer"
    assert boxes(b) == E_STATE  # after pwpp_trim_workspace
    # what pwpp_label_obstacles rejects
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert boxes(h, 0, 3) == 0 and boxes(h, 2, 1) == 0
    for first, n in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2)):
        assert boxes(h, first, n) == E_ARG, (first, n)
    assert boxes(h, mem=pwpp_hip.MEM_HOST_PINNED) == E_ARG
    for bad in (dict(nx=0), dict(cell=0.0), dict(cell=np.nan), dict(flags=2), dict(nx=1025)):
        kw = dict(dict(x0=-2.0, y0=-2.0, cell=1.0, nx=4, ny=4, flags=0, pad_=0), **bad)
        assert boxes(h, grid=pwpp_hip.GroundGrid(**kw)) == E_ARG, bad
    with pytest.raises(pwpp_hip.PwppError):
        h.set_option("boxes_path", 3)


def test_pybind_module_agrees_with_the_ctypes_handle():
    import pypatchworkpp
    pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    h = pwpp_hip.Handle()
    grid = (-30.0, -12.0, 0.5, 120, 48)
    with pytest.raises(RuntimeError):
        pp.getObstacleBoxes(*grid, 0.2, 2.5)  # no frame yet
    pts = small_cloud(5)
    pp.estimateGround(pts)
    h.estimate_ground(pts)
    for min_count, conn, ground_only in ((1, 8, False), (2, 4, True)):
        label, table, boxes, n = pp.getObstacleBoxes(*grid, 0.2, 2.5, min_count, conn, ground_only)
        hl, ht, hn = h.label_obstacles(*grid, 0.2, 2.5, min_count, conn, max_clusters=256, ground_only=ground_only)
        hb = h.box_obstacles(*grid, 0.2, 2.5, hl, int(hn[0]), ground_only=ground_only)
        assert label.shape == (48, 120) and n == hn[0] >= 3 and len(table) == n == len(boxes)
        assert boxes.dtype.names == ob.BOX_DTYPE.names and boxes.dtype.itemsize == 64
        assert label.tobytes() == hl[0].tobytes() and table.tobytes() == ht[0, :n].tobytes() and boxes.tobytes() == hb[0].tobytes()
        assert np.array_equal(boxes["points"], table["points"])
    with pytest.raises(RuntimeError):
        pp.getObstacleBoxes(0.0, 0.0, 1.0, 4, 4, 0.2, 2.5, 1, 5)
