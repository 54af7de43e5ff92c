"""The column pass of the obstacle distances (pwpp_distance_grid) in each of its tilings on a real MI355X: tall images of several
strips -- 130 x 577 and 65 x 513, whose last tile of the 64-row tiling has one row and whose last strip has 2 and 1 live lanes --
with the sparse patterns of tests/obstacle_distance_ref.py, whose scans run as far as the cap lets them, at the caps 0, 1, 64, 65,
223, 224, 225 and 46340: tiles with a halo in LDS under every halo from 1 to 224 rows, and the tiles read from global memory with
and without a cap.  Every comparison is of bytes with the capped brute force; the bits of metres with numpy's statement of them.
Host and device memory, several frames with several strips and several tiles at once, both values of "distance_path", repeated
calls, null outputs.  The largest call has 3 x 75 010 cells."""
import numpy as np
import pytest

import obstacle_distance_ref as od
import pwpp_hip
from test_gpu_obstacle_distance import CELLS, F32, check_against

pytestmark = pytest.mark.gpu

CASES = [(name, 1) for name in od.TALL_PATTERNS] + [("two_rows", 2), ("sparse", 2)]  # (pattern, min_count)
shape_ids = lambda s: "%dx%d" % s


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()


def want_of(name, nx, ny, min_count, max_dist):
    count, dist2, nearest = od.tall_reference(name, nx, ny, min_count)
    return count, od.capped((dist2, nearest), max_dist)


def test_the_cases_of_a_shape_reach_every_tiling():
    for nx, ny in od.TALL_SHAPES:
        hit = {(od.regime(ny, m), od.plan(ny, m)[2] if od.regime(ny, m) == "B" else m) for m in od.TALL_MAX_DISTS}
        assert hit == {("B", 1), ("B", 64), ("B", 65), ("B", 223), ("B", 224), ("C", 0), ("C", 225), ("C", 46340)}  # never A
        assert -(-nx // od.STRIP) > 1 and all(od.plan(ny, m)[3] > 1 for m in od.TALL_MAX_DISTS)
        assert od.plan(ny, 224)[1] == 64 and ny % 64 == 1 and od.plan(ny, 223)[1] == 66


@pytest.mark.parametrize("shape", od.TALL_SHAPES, ids=shape_ids)
def test_every_tiling_from_host_memory(handle, shape):
    nx, ny = shape
    for k, (name, min_count) in enumerate(CASES):
        for j, max_dist in enumerate(od.TALL_MAX_DISTS):
            cell = CELLS[(k + j) % 2]
            count, want = want_of(name, nx, ny, min_count, max_dist)
            got = handle.distance_grid(count, min_count, max_dist, cell)
            check_against(got, want, cell, "%s %dx%d min_count %d max_dist %d (%s, plan %s)"
                          % (name, nx, ny, min_count, max_dist, od.regime(ny, max_dist), od.plan(ny, max_dist)))


def test_frames_strips_and_tiles_all_above_one(handle):
    """Three frames of three strips, in ten tiles with a halo (max_dist 224) and in three from global memory (0): the block index
    is (frame * strips + strip) * row_tiles + tile with every factor above one."""
    nx, ny = 130, 577
    names = ("row_mid", None, "corners")  # an empty frame between two that are not
    refs = [od.tall_reference(name, nx, ny) if name else None for name in names]
    count = np.stack([r[0] if r else np.zeros((ny, nx), np.int32) for r in refs])
    empty = (np.full((ny, nx), od.BEYOND, np.int32), np.full((ny, nx), -1, np.int32))
    for max_dist in (224, 0):
        assert (len(names), -(-nx // od.STRIP), od.plan(ny, max_dist)[3]) == (3, 3, 10 if max_dist else 3)
        d2, near, m = handle.distance_grid(count, 1, max_dist, 0.3)
        assert d2.shape == (3, ny, nx)
        for f, r in enumerate(refs):
            want = od.capped((r[1], r[2]), max_dist) if r else empty
            check_against((d2[f], near[f], m[f]), want, 0.3, "frame %d (%s), max_dist %d" % (f, names[f], max_dist))


@pytest.mark.parametrize("max_dist", [0, 224])
def test_frames_never_see_each_other(handle, max_dist):
    nx, ny = 130, 577
    count = np.zeros((2, ny, nx), np.int32)
    count[0, -1, :] = 1   # frame 0's last row and frame 1's first row are neighbours in memory
    count[1, 0, :] = 1
    want = tuple(map(np.ascontiguousarray, od.distance_frames(count, 1, max_dist)))
    d2, near, m = handle.distance_grid(count, 1, max_dist, 0.5)
    check_against((d2, near, m), want, 0.5, "two frames of %d x %d, max_dist %d" % (nx, ny, max_dist))
    iy = np.arange(ny)[:, None].repeat(nx, 1)
    cap = max_dist if max_dist else ny
    assert np.array_equal(d2[0], np.where(ny - 1 - iy <= cap, (ny - 1 - iy) ** 2, od.BEYOND))
    assert np.array_equal(d2[1], np.where(iy <= cap, iy ** 2, od.BEYOND))
    assert (near[0][d2[0] != od.BEYOND] // nx == ny - 1).all() and (near[1][d2[1] != od.BEYOND] // nx == 0).all()


def test_two_runs_and_both_paths_give_identical_bytes():
    nx, ny = od.TALL_SHAPES[0]
    h = pwpp_hip.Handle()
    for name, min_count in CASES:
        for max_dist in od.TALL_MAX_DISTS:
            count, want = want_of(name, nx, ny, min_count, max_dist)
            runs = []
            for path in (0, 0, 1, 1):
                h.set_option("distance_path", path)
                runs.append(tuple(a.tobytes() for a in h.distance_grid(count, min_count, max_dist, 0.3)))
            what = "%s %dx%d min_count %d max_dist %d" % (name, nx, ny, min_count, max_dist)
            assert runs[0] == runs[1] and runs[2] == runs[3], what + ": two runs of the same call differ"
            assert runs[0] == runs[2], what + ": distance_path 0 and 1 differ"
            assert runs[2][0] == want[0].tobytes() and runs[2][1] == want[1].tobytes(), what + ": distance_path 1 differs from the brute force"
            assert runs[2][2] == od.metres_of(want[0], 0.3).tobytes(), what


def test_every_tiling_from_device_memory_off_the_16_byte_boundary(handle):
    """The count, dist2, nearest and metres images start 1, 2, 3 and 0 words past a 16-byte boundary, with poisoned words on
    either side that must survive; the count image is not written."""
    import torch
    nx, ny = od.TALL_SHAPES[1]
    cells = nx * ny
    shifts = sc, sd, sn, sm = (1, 2, 3, 0)
    bufs = [torch.empty((cells + 8,), dtype=torch.int32, device="cuda") for _ in range(4)]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    for k, (name, min_count) in enumerate(CASES):
        for j, max_dist in enumerate(od.TALL_MAX_DISTS):
            cell = CELLS[(k + j) % 2]
            count, want = want_of(name, nx, ny, min_count, max_dist)
            for b in bufs:
                b.fill_(-7)
            bufs[0][sc:sc + cells] = torch.from_numpy(count.reshape(-1).copy()).cuda()
            torch.cuda.synchronize()
            handle.distance_grid_device(nx, ny, 1, bufs[0].data_ptr() + 4 * sc, min_count, max_dist, cell, bufs[1].data_ptr() + 4 * sd,
                                        bufs[2].data_ptr() + 4 * sn, bufs[3].data_ptr() + 4 * sm)
            handle.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
            raw = [b.cpu().numpy() for b in bufs]
            what = "%s %dx%d min_count %d max_dist %d" % (name, nx, ny, min_count, max_dist)
            got = (raw[1][sd:sd + cells].reshape(ny, nx), raw[2][sn:sn + cells].reshape(ny, nx), raw[3][sm:sm + cells].copy().view(F32).reshape(ny, nx))
            check_against(got, want, cell, what)
            for r, s in zip(raw[1:], shifts[1:]):
                assert (r[:s] == -7).all() and (r[s + cells:] == -7).all(), what + ": a word outside an image was written"
            assert np.array_equal(raw[0][sc:sc + cells], count.reshape(-1)) and (raw[0][:sc] == -7).all() and (raw[0][sc + cells:] == -7).all(), \
                what + ": the count image was written"


def test_null_outputs_leave_the_others_unchanged(handle):
    nx, ny = od.TALL_SHAPES[0]
    max_dist = 224
    for name in ("row_mid", "sparse"):
        count, want = want_of(name, nx, ny, 1, max_dist)
        full = handle.distance_grid(count, 1, max_dist, 0.3)
        check_against(full, want, 0.3, "all three images")
        no_near = handle.distance_grid(count, 1, max_dist, 0.3, want_nearest=False)
        no_metres = handle.distance_grid(count, 1, max_dist, 0.3, want_metres=False)
        neither = handle.distance_grid(count, 1, max_dist, np.nan, want_nearest=False, want_metres=False)  # (cell is not read without metres)
        assert no_near[1] is None and no_metres[2] is None and neither[1] is None and neither[2] is None
        assert no_near[0].tobytes() == no_metres[0].tobytes() == neither[0].tobytes() == full[0].tobytes()
        assert no_near[2].tobytes() == full[2].tobytes() and no_metres[1].tobytes() == full[1].tobytes()
