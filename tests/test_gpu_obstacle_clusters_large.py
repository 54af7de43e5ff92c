"""The obstacle clusters (pwpp_label_grid, pwpp_label_obstacles) on a real MI355X at frames of more than 65 536 cells, where
tests/test_gpu_obstacle_clusters.py stops: oc.LARGE_SHAPES are the sizes at which k_cl_scan needs a second and a third round
(256 chunk counts per round, the total carried between them, a last round that is not full), a component crosses dozens of tiles,
hundreds of border workgroups are in flight in one launch and the table has tens of thousands of rows.  Every comparison is bit for
bit against the flood fill of tests/obstacle_clusters_ref.py -- label image, table, number of clusters -- which
tests/test_obstacle_clusters_cpu.py anchors at these shapes against a second restatement and against the patterns' construction.
A rank that misses the carry is in range and wrong for every cluster whose first cell lies beyond cell 65 535; the CPU test asserts
that the patterns have hundreds of those."""
import numpy as np
import pytest

import obstacle_clusters_ref as oc
import pwpp_hip
from test_gpu_obstacle_clusters import BAND, check_against, point_clusters_restated, reference, shape_ids
from test_gpu_obstacle_grid import small_cloud

pytestmark = pytest.mark.gpu

MULTI_ROUND = [s for s in oc.LARGE_SHAPES if oc.chunk_plan(*s)[1] > oc.SCAN_BLOCK]  # (257, 256), (1030, 132)
DEVICE_CASES = [("random0.3", 1, 4), ("checker", 1, 4), ("spiral", 1, 8), ("serpentine", 1, 4)]
PATH1_PATTERNS = ("random0.1", "random0.3", "random0.59", "checker", "diagonals")


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()


def name_of(case, shape):
    return "%s %dx%d min_count %d connectivity %d" % (case[0], shape[0], shape[1], case[1], case[2])


# ---- a: the pattern set --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", oc.LARGE_SHAPES, ids=shape_ids)
def test_pattern_set_from_host_memory(handle, shape):
    nx, ny = shape
    most = 0
    for case in oc.LARGE_CASES:
        name, min_count, conn = case
        count, top, label, table, n = reference(name, nx, ny, min_count, conn)
        got = handle.label_grid(count, top, min_count, conn, max_clusters=n + 2)
        check_against((got[0], got[1][0], got[2][0]), label, table, n, name_of(case, shape))
        most = max(most, n)
    assert most == (nx * ny + 1) // 2  # the checkerboard with edge neighbours: the longest table


# ---- b: device memory ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", MULTI_ROUND, ids=shape_ids)
def test_pattern_set_from_misaligned_device_memory(handle, shape):
    """The count, top and label images start 1, 2 and 3 words past a 16-byte boundary, with poisoned words on either side of every
    array that must survive."""
    import torch
    nx, ny = shape
    cells = nx * ny
    sc, st, sl = 1, 2, 3
    for case in DEVICE_CASES:
        name, min_count, conn = case
        count, top, label, table, n = reference(name, nx, ny, min_count, conn)
        rows = n + 1
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
        handle.synchronize()
        raw_c, raw_p, raw_l, raw_t, raw_n = (d.cpu().numpy() for d in (d_count, d_top, d_label, d_table, d_n))
        what = name_of(case, shape)
        check_against((raw_l[sl:sl + cells].reshape(ny, nx), raw_t[2:2 + rows * 12].copy().view(oc.CLUSTER_DTYPE), raw_n[1]), label, table, n, what)
        assert (raw_l[:sl] == -7).all() and (raw_l[sl + cells:] == -7).all(), what + ": a word outside the label image was written"
        assert (raw_t[:2] == -7).all() and (raw_t[2 + rows * 12:] == -7).all() and raw_n[0] == -7 and (raw_n[2:] == -7).all(), what
        assert (raw_c[:sc] == -7).all() and (raw_c[sc + cells:] == -7).all() and np.array_equal(raw_c[sc:sc + cells], count.reshape(-1)), what
        assert (raw_p[:st] == -7).all() and (raw_p[st + cells:] == -7).all(), what
        assert raw_p[st:st + cells].tobytes() == top.tobytes(), what + ": the top image was written"


# ---- c: many frames in one launch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [4, 8])
def test_sixteen_frames_in_one_call(handle, conn):
    """16 frames of 257 x 256 cells: 16 * 5 * 16 = 1280 workgroups in the border launch, 16 * 257 = 4112 in the compress launch,
    and a scan of two rounds per frame.  Every frame equals its single-frame reference -- so no frame's carry reaches the next --
    and two runs of the call give the same bytes."""
    nx, ny = 257, 256
    assert oc.chunk_plan(nx, ny)[1:] == (257, [256, 1], (5, 16))
    names = [c[0] for c in oc.LARGE_CASES if c[1] == 1 and c[2] == conn]  # (one min_count per call: the cases of min_count 1)
    assert len(names) == len(oc.LARGE_PATTERNS)
    refs = [reference(names[f % len(names)], nx, ny, 1, conn) for f in range(16)]
    count, top = np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs])
    rows = max(r[4] for r in refs) + 2
    runs = []
    for _ in range(2):
        label, table, n = handle.label_grid(count, top, 1, conn, max_clusters=rows)
        assert table.shape == (16, rows)
        runs.append((label.tobytes(), n.tobytes(), b"".join(table[f, :r[4]].tobytes() for f, r in enumerate(refs))))
    for f, r in enumerate(refs):
        check_against((label[f], table[f], n[f]), r[2], r[3], r[4], "frame %d (%s), connectivity %d" % (f, names[f % len(names)], conn))
    assert runs[0] == runs[1], "two runs of the same call differ"


# ---- d: both paths -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", oc.LARGE_SHAPES, ids=shape_ids)
def test_two_runs_and_both_paths_give_identical_bytes(shape):
    """clusters_path 0 twice on every case; clusters_path 1 twice on the random patterns, the checkerboard and the diagonals ONLY.
    Path 1 is the yardstick with one global forest and no path compression in uf_find, and nobody has measured how long its
    chases get on a one-component pattern of 66 000 cells that is one cell wide: full, comb, spiral and serpentine on path 1 stay
    covered at the small shapes of tests/test_gpu_obstacle_clusters.py."""
    nx, ny = shape
    h = pwpp_hip.Handle()
    for case in oc.LARGE_CASES:
        name, min_count, conn = case
        count, top, label, table, n = reference(name, nx, ny, min_count, conn)
        what = name_of(case, shape)
        runs = []
        for path in (0, 0, 1, 1) if name in PATH1_PATTERNS else (0, 0):
            h.set_option("clusters_path", path)
            got = h.label_grid(count, top, min_count, conn, max_clusters=n + 1)
            runs.append((got[0].tobytes(), got[1][0, :n].tobytes(), got[2].tobytes()))
        assert all(r == runs[0] for r in runs[1:]), what + ": runs of the same call, or clusters_path 0 and 1, differ"
        assert runs[-1] == (label.tobytes(), table.tobytes(), np.asarray([n], np.int32).tobytes()), what + ": differs from the flood fill"


# ---- e: pwpp_label_obstacles at the cost tool's grid size ------------------------------------------------------------------------
def test_label_obstacles_on_a_grid_of_260_chunks():
    """Three scans on 260 x 256 cells of 0.25 m (66 560 cells, 260 chunks: a scan of two rounds): the images of
    pwpp_rasterize_obstacles, the labels of pwpp_label_grid on them and of the flood fill, the per-point ids of the recomputation."""
    grid = (-32.5, -60.0, 0.25, 260, 256)  # (y up to 4 m: the rows of the second scan round lie beside the sensor, not at the rim)
    x0, y0, cell, nx, ny = grid
    assert oc.chunk_plan(nx, ny)[1:3] == (260, [256, 4])
    frames = [small_cloud(s) for s in (5, 6, 7)]
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    rc, rt = h.rasterize_obstacles(x0, y0, cell, nx, ny, *BAND)
    rows = 4096
    for min_count, conn in ((1, 8), (1, 4)):
        label, table, n, count, top, pc = h.label_obstacles(x0, y0, cell, nx, ny, *BAND, min_count, conn, max_clusters=rows, want_images=True,
                                                            want_point_cluster=True)
        what = "min_count %d connectivity %d" % (min_count, conn)
        assert count.tobytes() == rc.tobytes() and top.tobytes() == rt.tobytes(), what + ": the images differ from pwpp_rasterize_obstacles"
        l2, t2, n2 = h.label_grid(rc, rt, min_count, conn, max_clusters=rows)
        assert label.tobytes() == l2.tobytes() and n.tobytes() == n2.tobytes(), what + ": labels differ from pwpp_label_grid on the images"
        want = oc.label_frames(rc, rt, min_count, conn, max_clusters=rows)
        assert np.array_equal(n, want[2]), what + ": %s clusters, the flood fill has %s" % (n.tolist(), want[2].tolist())
        assert np.array_equal(label, want[0]), what
        for f in range(3):
            assert oc.same_tables(table[f], n[f], want[1][f]) and oc.same_tables(t2[f], n2[f], want[1][f]), what
        print("%s, %d x %d: %s clusters, %s of them beyond chunk 255" % (what, nx, ny, n.tolist(), [oc.roots_beyond(t, oc.SCAN_BLOCK) for t in want[1]]))
        assert n[0] >= 3
        assert np.array_equal(pc, point_clusters_restated(h, label, grid)), what + ": point_cluster differs from the recomputation"
        assert (pc >= 0).sum() == rc[label >= 0].sum()
