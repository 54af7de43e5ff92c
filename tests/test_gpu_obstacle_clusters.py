"""The obstacle clusters (pwpp_label_grid, pwpp_label_obstacles) on a real MI355X: the pattern set of
tests/obstacle_clusters_ref.py through pwpp_label_grid from host and from device memory, bit for bit against the flood fill --
label image, table, number of clusters -- at both connectivities and min_count 1 and 2; several frames in one call, misaligned
device images, truncated tables, repeated calls, both values of the option "clusters_path"; and pwpp_label_obstacles against
pwpp_rasterize_obstacles + pwpp_label_grid, its per-point cluster ids against a recomputation from the library's own rows and
queries, in every kind of call -- and that asking changes nothing else.  Shapes are small here: the largest image has 4257 cells
(17 chunks: one partial round of k_cl_scan, 3 x 3 tiles), the clouds ~3 k points.  Frames of more than 65 536 cells -- a second and
third scan round, components across dozens of tiles, tables of tens of thousands of rows -- are
tests/test_gpu_obstacle_clusters_large.py's."""
import ctypes
import functools

import numpy as np
import pytest

import obstacle_clusters_ref as oc
import obstacle_grid_ref as og
import pwpp_hip
from test_gpu_obstacle_grid import _everything, device_tensor, small_cloud, three_frames

pytestmark = pytest.mark.gpu

F32 = np.float32
E_ARG, E_STATE = -1, -4
BAND = (0.2, 2.5)
CASES = [(name, m, c) for name in oc.PATTERNS for m in (1, 2) for c in (4, 8)]
shape_ids = lambda s: "%dx%d" % s


@functools.lru_cache(maxsize=None)
def reference(name, nx, ny, min_count, conn):
    """(count, top, label, table, n) of a pattern: computed once, shared by every test, never written."""
    count, top = oc.pattern(name, nx, ny, min_count)
    label, table, n = oc.flood_fill(count, top, min_count, conn)
    for a in (count, top, label, table):
        a.setflags(write=False)
    return count, top, label, table, n


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()  # (no estimate call: pwpp_label_grid needs the handle's stream and buffer only)


def check_against(got, want_label, want_table, want_n, what):
    label, table, n = got
    assert label.dtype == np.int32 and label.shape == want_label.shape, what
    assert int(n) == want_n, "%s: %d clusters, the flood fill has %d" % (what, int(n), want_n)
    assert np.array_equal(label, want_label), "%s: the label image differs from the flood fill in %d cells" % (what, (label != want_label).sum())
    assert oc.same_tables(table, n, want_table[:len(table)]), "%s: the table differs from the flood fill" % what


# ---- the pattern set --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", oc.SHAPES, ids=shape_ids)
def test_pattern_set_from_host_memory(handle, shape):
    nx, ny = shape
    clusters = 0
    for name, min_count, conn in CASES:
        count, top, label, table, n = reference(name, nx, ny, min_count, conn)
        got = handle.label_grid(count, top, min_count, conn, max_clusters=n + 2)
        check_against((got[0], got[1][0], got[2][0]), label, table, n, "%s %dx%d min_count %d connectivity %d" % (name, nx, ny, min_count, conn))
        clusters += n
    assert clusters > 0
    # the checkerboard's two faces
    count = reference("checker", nx, ny, 1, 4)[0]
    occupied = int((count >= 1).sum())
    assert handle.label_grid(count, None, 1, 4)[2][0] == occupied and handle.label_grid(count, None, 1, 8)[2][0] == 1
    # without a top image the rows' tops are the quiet NaN
    _, t, n = handle.label_grid(count, None, 1, 8, max_clusters=1)
    assert t["top"][0, :1].view(np.uint32)[0] == og.QNAN_BITS and t["cells"][0, 0] == occupied


@pytest.mark.parametrize("shape", oc.SHAPES, ids=shape_ids)
def test_pattern_set_from_device_memory_at_every_alignment(handle, shape):
    """The same from device memory; the three images start 0, 1, 2 and 3 words past a 16-byte boundary in turn (rows that are and
    are not 16-byte aligned), with poisoned words on either side that must survive."""
    import torch
    nx, ny = shape
    cells = nx * ny
    for k, (name, min_count, conn) in enumerate(CASES):
        count, top, label, table, n = reference(name, nx, ny, min_count, conn)
        rows = n + 1
        sc, st, sl = k % 4, (k // 4 + 1) % 4, (k + 2) % 4  # (every shift of 0..3 words for every image over the cases)
        d_count = torch.full((cells + 8,), -7, dtype=torch.int32, device="cuda")
        d_top = torch.full((cells + 8,), -7, dtype=torch.int32, device="cuda")
        d_label = torch.full((cells + 8,), -7, dtype=torch.int32, device="cuda")
        d_table = torch.full((rows * 12 + 4,), -7, dtype=torch.int32, device="cuda")
        d_n = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        assert all(d.data_ptr() % 16 == 0 for d in (d_count, d_top, d_label, d_table, d_n))
        d_count[sc:sc + cells] = torch.from_numpy(count.reshape(-1).copy()).cuda()
        d_top[st:st + cells] = torch.from_numpy(top.reshape(-1).view(np.int32).copy()).cuda()
        torch.cuda.synchronize()
        handle.label_grid_device(nx, ny, 1, d_count.data_ptr() + 4 * sc, d_top.data_ptr() + 4 * st, min_count, conn, d_label.data_ptr() + 4 * sl,
                                 d_table.data_ptr() + 8, d_n.data_ptr() + 4, max_clusters=rows)
        handle.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
        raw_l, raw_t, raw_n = d_label.cpu().numpy(), d_table.cpu().numpy(), d_n.cpu().numpy()
        what = "%s %dx%d min_count %d connectivity %d, shifts %d %d %d" % (name, nx, ny, min_count, conn, sc, st, sl)
        got_table = raw_t[2:2 + rows * 12].copy().view(oc.CLUSTER_DTYPE)
        check_against((raw_l[sl:sl + cells].reshape(ny, nx), got_table, raw_n[1]), label, table, n, what)
        assert (raw_l[:sl] == -7).all() and (raw_l[sl + cells:] == -7).all(), what + ": a word outside the label image was written"
        assert (raw_t[:2] == -7).all() and (raw_t[2 + rows * 12:] == -7).all() and raw_n[0] == -7 and (raw_n[2:] == -7).all(), what
        assert np.array_equal(d_count.cpu().numpy()[sc:sc + cells], count.reshape(-1)), what + ": the count image was written"


def test_three_frames_with_different_patterns_in_one_call(handle):
    nx, ny = 129, 33
    for conn in (4, 8):
        refs = [reference(name, nx, ny, 1, conn) for name in ("random0.59", "spiral", "comb", "empty", "corner")]
        count, top = np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs])
        rows = max(r[4] for r in refs) + 1
        label, table, n = handle.label_grid(count, top, 1, conn, max_clusters=rows)
        assert table.shape == (5, rows)
        for f, r in enumerate(refs):
            check_against((label[f], table[f], n[f]), r[2], r[3], r[4], "frame %d, connectivity %d" % (f, conn))


@pytest.mark.parametrize("shape", [(7, 5), (65, 17), (64, 16)], ids=shape_ids)
def test_frames_never_connect(handle, shape):
    nx, ny = shape
    count = np.zeros((3, ny, nx), np.int32)
    count[0, -1, :] = 1   # frame 0's last row and frame 1's first row are neighbours in memory
    count[1, 0, :] = 2
    count[1, -1, :] = 1
    count[2, :, :] = 3
    want = oc.label_frames(count, None, 1, 8, max_clusters=2)
    for conn in (4, 8):
        label, table, n = handle.label_grid(count, None, 1, conn, max_clusters=2)
        assert n.tolist() == [1, 2 if ny > 1 else 1, 1]
        assert np.array_equal(label, want[0])
        for f in range(3):
            assert oc.same_tables(table[f], n[f], want[1][f][:n[f]])
        assert table["first_cell"][1, 0] == 0 and table["first_cell"][0, 0] == (ny - 1) * nx


def test_max_clusters_truncates_the_table_and_nothing_else(handle):
    nx, ny = 129, 33
    count, top, label, table, n = reference("random0.3", nx, ny, 1, 4)
    assert n > 40
    for rows in (0, 1, n // 2, n - 1, n, n + 5):
        got = handle.label_grid(count, top, 1, 4, max_clusters=rows)
        assert got[1].shape == (1, rows)
        check_against((got[0], got[1][0], got[2][0]), label, table[:rows], n, "max_clusters %d of %d" % (rows, n))
        assert got[0].max() == n - 1  # the complete ranks stand in the label image
    # device memory: the rows behind max_clusters are not written
    import torch
    rows = n // 2
    d_count, d_label = device_tensor(count), device_tensor(np.zeros_like(count))
    d_table = torch.full(((rows + 3) * 12,), -7, dtype=torch.int32, device="cuda")
    handle.label_grid_device(nx, ny, 1, d_count.data_ptr(), 0, 1, 4, d_label.data_ptr(), d_table.data_ptr(), 0, max_clusters=rows)
    handle.synchronize()
    raw = d_table.cpu().numpy()
    assert (raw[rows * 12:] == -7).all()
    want = oc.flood_fill(count, None, 1, 4)[1][:rows]
    assert raw[:rows * 12].copy().view(oc.CLUSTER_DTYPE).tobytes() == want.tobytes()
    assert np.array_equal(d_label.cpu().numpy(), label)


@pytest.mark.parametrize("shape", oc.SHAPES, ids=shape_ids)
def test_two_runs_and_both_paths_give_identical_bytes(shape):
    nx, ny = shape
    h = pwpp_hip.Handle()
    for name, min_count, conn in CASES:
        count, top, label, table, n = reference(name, nx, ny, min_count, conn)
        runs = []
        for path in (0, 0, 1, 1):
            h.set_option("clusters_path", path)
            got = h.label_grid(count, top, min_count, conn, max_clusters=n + 1)
            runs.append((got[0].tobytes(), got[1][0, :n].tobytes(), got[2].tobytes()))
        what = "%s %dx%d min_count %d connectivity %d" % (name, nx, ny, min_count, conn)
        assert runs[0] == runs[1] and runs[2] == runs[3], what + ": two runs of the same call differ"
        assert runs[0] == runs[2], what + ": clusters_path 0 and 1 differ"
        assert runs[2][0] == label.tobytes() and runs[2][1] == table.tobytes(), what + ": clusters_path 1 differs from the flood fill"
    with pytest.raises(pwpp_hip.PwppError):
        h.set_option("clusters_path", 2)


# ---- pwpp_label_obstacles -------------------------------------------------------------------------------------------------------
GRIDS = [(-16.0, -16.0, 0.5, 64, 64), (2.0, -17 * 1.7 / 3, 1.7, 65, 17)]  # (x0, y0, cell, nx, ny): 64 x 64 of 0.5 m; 65 x 17 of 1.7 m that cuts the cloud


def point_clusters_restated(h, label, grid, first=0):
    """The per-point ids from the library's own non-ground rows and ground queries, the cell arithmetic of the obstacle grid's
    restatement and the label image."""
    x0, y0, cell, nx, ny = grid
    base = h.frame_base()
    out = np.full(int(base[first + label.shape[0]] - base[first]), -1, np.int32)
    for fr in range(label.shape[0]):
        f = first + fr
        xyz, idx = h.nonground(f), h.nonground_indices(f)
        if len(idx) == 0:
            continue
        s = h.query_ground(xyz, frames=f)
        kx, ix = og.cells_of(xyz[:, 0], x0, cell, nx)
        ky, iy = og.cells_of(xyz[:, 1], y0, cell, ny)
        hgt = np.ascontiguousarray(s["distance"], F32)
        with np.errstate(invalid="ignore"):
            counted = kx & ky & (s["patch"] >= 0) & (F32(BAND[0]) <= hgt) & (hgt <= F32(BAND[1]))
        out[int(base[f] - base[first]) + idx[counted]] = label[fr, iy[counted], ix[counted]]
    return out


@pytest.mark.parametrize("grid", GRIDS, ids=["64x64", "65x17"])
def test_label_obstacles_is_rasterize_plus_label_grid(grid):
    frames = three_frames()  # a 16-beam scan, an empty frame, a frame that is all unref
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    x0, y0, cell, nx, ny = grid
    rc, rt = h.rasterize_obstacles(x0, y0, cell, nx, ny, *BAND)
    for min_count, conn in ((1, 8), (1, 4), (2, 8)):
        label, table, n, count, top, pc = h.label_obstacles(x0, y0, cell, nx, ny, *BAND, min_count, conn, max_clusters=64, want_images=True,
                                                            want_point_cluster=True)
        what = "min_count %d connectivity %d" % (min_count, conn)
        assert count.tobytes() == rc.tobytes() and top.tobytes() == rt.tobytes(), what + ": the images differ from pwpp_rasterize_obstacles"
        l2, t2, n2 = h.label_grid(rc, rt, min_count, conn, max_clusters=64)
        assert label.tobytes() == l2.tobytes() and n.tobytes() == n2.tobytes(), what + ": labels differ from pwpp_label_grid on the images"
        want = oc.label_frames(rc, rt, min_count, conn, max_clusters=64)
        assert np.array_equal(label, want[0]) and np.array_equal(n, want[2]), what
        for f in range(3):
            assert oc.same_tables(table[f], n[f], want[1][f]) and oc.same_tables(t2[f], n2[f], want[1][f]), what
        print("%s, %d x %d: %s clusters" % (what, nx, ny, n.tolist()))
        # the scan frame: the scene has 40 boxes.  On cells of 0.5 m the flood fill finds 16 clusters (14 at min_count 2); cells of 1.7 m
        # with corner neighbours join everything the grid sees into ONE cluster, so there the number is the restatement's, above
        assert n[0] >= (3 if cell == 0.5 else 1)
        assert n[1] == 0 and n[2] == 0 and (label[1:] == -1).all()  # the empty frame, the all-unref frame
        # without the images and the ids: the same labels, table and counts
        l3, t3, n3 = h.label_obstacles(x0, y0, cell, nx, ny, *BAND, min_count, conn, max_clusters=64)
        assert (l3.tobytes(), t3.tobytes(), n3.tobytes()) == (label.tobytes(), table.tobytes(), n.tobytes())
        # the per-point ids
        assert pc.dtype == np.int32 and len(pc) == sum(len(f) for f in frames)
        assert np.array_equal(pc, point_clusters_restated(h, label, grid)), what + ": point_cluster differs from the recomputation"
        base = h.frame_base()
        assert (pc[h.ground_indices(0)] == -1).all() and (pc[int(base[1]):] == -1).all()
        k = min(int(n[0]), 64)
        assert np.array_equal(np.bincount(pc[:int(base[1])][pc[:int(base[1])] >= 0], minlength=k)[:k], table["points"][0, :k]), what
        assert (pc >= 0).sum() == rc[label >= 0].sum()
    # a sub-range of frames
    l1, t1, n1, pc1 = h.label_obstacles(x0, y0, cell, nx, ny, *BAND, 1, 8, max_clusters=64, frame_first=2, frames=1, want_point_cluster=True)
    assert n1.tolist() == [0] and (l1 == -1).all() and len(pc1) == len(frames[2]) and (pc1 == -1).all()


def test_point_cluster_with_a_transform_in_cloud_order_and_after_a_device_call():
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

    def everything(h):
        out = h.label_obstacles(*grid, *BAND, 1, 8, max_clusters=64, want_images=True, want_point_cluster=True)
        assert np.array_equal(out[5], point_clusters_restated(h, out[0], grid))
        assert out[2][0] >= 3 and (out[5][h.ground_indices(0)] == -1).all()
        return tuple(np.ascontiguousarray(a).tobytes() for a in out)

    a = pwpp_hip.Handle()
    a.set_input_transforms(T)
    a.estimate_ground_batch(sensor, mode=pwpp_hip.MODE_FRESH)
    with_transform = everything(a)
    b = pwpp_hip.Handle()
    b.set_order(pwpp_hip.ORDER_CLOUD)
    b.estimate_ground_batch(pre, mode=pwpp_hip.MODE_FRESH)
    cloud_order = everything(b)
    c = pwpp_hip.Handle()
    tens = [device_tensor(f) for f in pre]
    c.estimate_ground_batch_device([t.data_ptr() for t in tens], [len(f) for f in pre])
    after_device_call = everything(c)  # (the input is alive: `tens`)
    assert with_transform == cloud_order == after_device_call
    # ... and into device memory, the ids one word off a 16-byte boundary
    import torch
    x0, y0, cell, nx, ny = grid
    total = sum(len(f) for f in pre)
    d_label = torch.full((3 * nx * ny,), -7, dtype=torch.int32, device="cuda")
    d_table = torch.full((3 * 64 * 12,), -7, dtype=torch.int32, device="cuda")
    d_n = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    d_pc = torch.full((total + 8,), -7, dtype=torch.int32, device="cuda")
    c.label_obstacles_device(x0, y0, cell, nx, ny, *BAND, 1, 8, d_label.data_ptr(), 0, 0, d_table.data_ptr(), d_n.data_ptr(), 64, d_pc.data_ptr() + 4)
    c.synchronize()
    raw = d_pc.cpu().numpy()
    assert d_label.cpu().numpy().tobytes() == cloud_order[0] and d_n.cpu().numpy().tobytes() == cloud_order[2]
    n0 = int(d_n.cpu().numpy()[0])
    assert d_table.cpu().numpy()[:n0 * 12].tobytes() == cloud_order[1][:n0 * 48]
    assert raw[1:1 + total].tobytes() == cloud_order[5] and raw[0] == -7 and (raw[1 + total:] == -7).all()
    del tens


def test_asking_changes_nothing_else():
    first, second = [small_cloud(s) for s in (5, 6, 7)], [small_cloud(s) for s in (8, 9, 10)]
    h = pwpp_hip.Handle()
    h.set_order(pwpp_hip.ORDER_CLOUD)
    h.set_num_streams(3)
    h.estimate_ground_batch(first, mode=pwpp_hip.MODE_STREAMS)
    before, t_before = _everything(h, 3), h.time_us()
    records = [h.nonground_records(f).tobytes() for f in range(3)]
    out = h.label_obstacles(-20.0, -20.0, 0.5, 80, 80, *BAND, 1, 8, max_clusters=16, want_images=True, want_point_cluster=True)
    assert out[2].min() >= 3
    h.label_grid(out[3], out[4], 2, 4)
    assert _everything(h, 3) == before and h.time_us() == t_before, "labelling changed the results of the call it reads"
    assert records == [h.nonground_records(f).tobytes() for f in range(3)]
    h.estimate_ground_batch(second, mode=pwpp_hip.MODE_STREAMS)
    asked = _everything(h, 3)
    ref = pwpp_hip.Handle()
    ref.set_order(pwpp_hip.ORDER_CLOUD)
    ref.set_num_streams(3)
    ref.estimate_ground_batch(first, mode=pwpp_hip.MODE_STREAMS)
    ref.estimate_ground_batch(second, mode=pwpp_hip.MODE_STREAMS)
    assert _everything(ref, 3) == asked, "labelling between two calls changed the second call's outputs"


def test_state_workspace_and_arguments():
    L = pwpp_hip.load()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    lab = np.zeros(3 * 16, np.int32)
    g = pwpp_hip.GroundGrid(-2.0, -2.0, 1.0, 4, 4, 0, 0)

    def obstacles(h, first=0, frames=1, mem=pwpp_hip.MEM_HOST, grid=g):
        return L.pwpp_label_obstacles(h._h, ctypes.byref(grid), 0.2, 2.5, 1, 8, first, frames, mem, vp(lab), None, None, None, None, 0, None)

    h = pwpp_hip.Handle()
    empty = h.workspace_bytes()
    assert obstacles(h) == E_STATE  # before any estimate call ...
    count = reference("random0.3", 65, 17, 1, 8)
    got = h.label_grid(count[0], count[1], 1, 8, max_clusters=count[4])  # ... pwpp_label_grid works
    check_against((got[0], got[1][0], got[2][0]), count[2], count[3], count[4], "before any estimate call")
    grown = h.workspace_bytes()
    assert grown > empty, "the cluster buffer is not counted by pwpp_get_workspace_bytes"
    h.trim_workspace()
    assert h.workspace_bytes() == empty, "pwpp_trim_workspace did not free the cluster buffer"
    assert obstacles(h) == E_STATE
    # with the feature unused nothing is allocated
    a, b = pwpp_hip.Handle(), pwpp_hip.Handle()
    frames = three_frames()
    for w in (a, b):
        w.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert a.workspace_bytes() == b.workspace_bytes()
    b.label_obstacles(-20.0, -20.0, 0.5, 80, 80, *BAND)
    assert b.workspace_bytes() > a.workspace_bytes()
    b.trim_workspace()
    a.trim_workspace()
    assert a.workspace_bytes() == b.workspace_bytes()
    # what pwpp_rasterize_obstacles rejects
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert obstacles(h, 0, 3) == 0 and obstacles(h, 2, 1) == 0
    for first, n in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2)):
        assert obstacles(h, first, n) == E_ARG, (first, n)
    assert obstacles(h, mem=pwpp_hip.MEM_HOST_PINNED) == E_ARG
    for bad in (dict(nx=0), dict(cell=0.0), dict(cell=np.nan), dict(flags=2)):
        kw = dict(dict(x0=-2.0, y0=-2.0, cell=1.0, nx=4, ny=4, flags=0, pad_=0), **bad)
        assert obstacles(h, grid=pwpp_hip.GroundGrid(**kw)) == E_ARG, bad
    cnt = np.zeros(16, np.int32)
    assert L.pwpp_label_grid(h._h, 4, 4, 1, pwpp_hip.MEM_HOST_PINNED, vp(cnt), None, 1, 8, vp(lab), None, None, 0) == E_ARG


def test_pybind_module_agrees_with_the_ctypes_handle():
    import pypatchworkpp
    pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    h = pwpp_hip.Handle()
    with pytest.raises(RuntimeError):
        pp.getObstacleClusters(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5)  # no frame yet
    pts = small_cloud(5)
    pp.estimateGround(pts)
    h.estimate_ground(pts)
    for min_count, conn, ground_only in ((1, 8, False), (2, 4, True)):
        label, table, n = pp.getObstacleClusters(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5, min_count, conn, ground_only)
        hl, ht, hn = h.label_obstacles(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5, min_count, conn, max_clusters=256, ground_only=ground_only)
        assert label.dtype == np.int32 and label.shape == (48, 120) and n == hn[0] >= 3 and len(table) == n
        assert table.dtype.names == oc.CLUSTER_DTYPE.names and table.dtype.itemsize == 48
        assert label.tobytes() == hl[0].tobytes() and table.tobytes() == ht[0, :n].tobytes()
    label, table, n = pp.getObstacleClusters(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5)
    assert n == hn[0] or n >= 3
    with pytest.raises(RuntimeError):
        pp.getObstacleClusters(0.0, 0.0, 1.0, 4, 4, 0.2, 2.5, 1, 5)
