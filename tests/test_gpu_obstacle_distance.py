"""The obstacle distances (pwpp_distance_grid, pwpp_distance_obstacles) on a real MI355X: the pattern set of
tests/obstacle_distance_ref.py through pwpp_distance_grid from host and from device memory, bit for bit against the brute force
-- dist2, nearest, metres -- at min_count 1 and 2 and max_dist 0, 1, 2 and 5; several frames in one call, frame borders,
misaligned device images, repeated calls, both values of the option "distance_path", null outputs; and pwpp_distance_obstacles
against pwpp_rasterize_obstacles + pwpp_distance_grid in every kind of call -- and that asking changes nothing else.  Shapes are
small on purpose: the largest image has 4257 cells, the clouds ~3 k points."""
import ctypes
import functools

import numpy as np
import pytest

import obstacle_distance_ref as od
import pwpp_hip
from test_gpu_obstacle_grid import _everything, device_tensor, small_cloud, three_frames

pytestmark = pytest.mark.gpu

F32 = np.float32
E_ARG, E_STATE = -1, -4
BAND = (0.2, 2.5)
CELLS = (0.5, 0.3)
CASES = [(name, m) for name in od.PATTERNS for m in (1, 2)]
shape_ids = lambda s: "%dx%d" % s


@functools.lru_cache(maxsize=None)
def reference(name, nx, ny, min_count):
    """(count, dist2, nearest) of a pattern, unlimited: computed once, shared by every test, never written."""
    count, _ = od.pattern(name, nx, ny, min_count)
    dist2, nearest = od.brute_force(count, min_count)
    for a in (count, dist2, nearest):
        a.setflags(write=False)
    return count, dist2, nearest


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()  # (no estimate call: pwpp_distance_grid needs the handle's stream and buffer only)


def check_against(got, want, cell, what):
    """dist2 and nearest against the restatement, the bits of metres against numpy's statement of them."""
    dist2, nearest, metres = got
    assert dist2.dtype == np.int32 and dist2.shape == want[0].shape, what
    assert np.array_equal(dist2, want[0]), "%s: dist2 differs from the brute force in %d cells" % (what, (dist2 != want[0]).sum())
    if nearest is not None:
        assert nearest.dtype == np.int32 and np.array_equal(nearest, want[1]), "%s: nearest differs in %d cells" % (what, (nearest != want[1]).sum())
    if metres is not None:
        assert metres.dtype == np.float32 and metres.tobytes() == od.metres_of(want[0], cell).tobytes(), what + ": the bits of metres differ"


# ---- the pattern set --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", od.SHAPES, ids=shape_ids)
def test_pattern_set_from_host_memory(handle, shape):
    nx, ny = shape
    occupied = 0
    for k, (name, min_count) in enumerate(CASES):
        count, dist2, nearest = reference(name, nx, ny, min_count)
        occupied += int((dist2 == 0).sum())
        for max_dist in od.MAX_DISTS:
            cell = CELLS[(k + max_dist) % 2]
            got = handle.distance_grid(count, min_count, max_dist, cell)
            check_against(got, od.capped((dist2, nearest), max_dist), cell, "%s %dx%d min_count %d max_dist %d" % (name, nx, ny, min_count, max_dist))
    assert occupied > 0
    # an empty frame: beyond, -1, +inf; a full one: 0, the cell's own index, +0.0
    d2, near, m = handle.distance_grid(np.zeros((ny, nx), np.int32), 1, 0, 0.5)
    assert (d2 == pwpp_hip.DIST_BEYOND).all() and (near == -1).all() and (m.view(np.uint32) == 0x7f800000).all()
    d2, near, m = handle.distance_grid(np.full((ny, nx), 3, np.int32), 2, 5, 0.3)
    assert (d2 == 0).all() and np.array_equal(near.reshape(-1), np.arange(nx * ny)) and (m.view(np.uint32) == 0).all()


@pytest.mark.parametrize("shape", od.SHAPES, ids=shape_ids)
def test_pattern_set_from_device_memory_at_every_alignment(handle, shape):
    """The same from device memory; the four images start 0, 1, 2 and 3 words past a 16-byte boundary in turn, with poisoned
    words on either side that must survive; the count image is not written."""
    import torch
    nx, ny = shape
    cells = nx * ny
    for k, (name, min_count) in enumerate(CASES):
        count, dist2, nearest = reference(name, nx, ny, min_count)
        max_dist, cell = od.MAX_DISTS[k % 4], CELLS[k % 2]
        shifts = [(k + j + k // 4) % 4 for j in range(4)]  # (every shift of 0..3 words for every image over the cases)
        bufs = [torch.full((cells + 8,), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
        assert all(b.data_ptr() % 16 == 0 for b in bufs)
        sc, sd, sn, sm = shifts
        bufs[0][sc:sc + cells] = torch.from_numpy(count.reshape(-1).copy()).cuda()
        torch.cuda.synchronize()
        handle.distance_grid_device(nx, ny, 1, bufs[0].data_ptr() + 4 * sc, min_count, max_dist, cell, bufs[1].data_ptr() + 4 * sd,
                                    bufs[2].data_ptr() + 4 * sn, bufs[3].data_ptr() + 4 * sm)
        handle.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
        raw = [b.cpu().numpy() for b in bufs]
        what = "%s %dx%d min_count %d max_dist %d, shifts %s" % (name, nx, ny, min_count, max_dist, shifts)
        got = (raw[1][sd:sd + cells].reshape(ny, nx), raw[2][sn:sn + cells].reshape(ny, nx), raw[3][sm:sm + cells].copy().view(F32).reshape(ny, nx))
        check_against(got, od.capped((dist2, nearest), max_dist), cell, what)
        for r, s in zip(raw[1:], shifts[1:]):
            assert (r[:s] == -7).all() and (r[s + cells:] == -7).all(), what + ": a word outside an image was written"
        assert np.array_equal(raw[0][sc:sc + cells], count.reshape(-1)) and (raw[0][:sc] == -7).all() and (raw[0][sc + cells:] == -7).all(), \
            what + ": the count image was written"


def test_frames_with_different_patterns_in_one_call(handle):
    nx, ny = 129, 33
    names = ("random0.1", "spiral", "empty", "corner", "random0.59", "full")  # an empty frame between two that are not
    refs = [reference(name, nx, ny, 1) for name in names]
    count = np.stack([r[0] for r in refs])
    for max_dist in (0, 5):
        d2, near, m = handle.distance_grid(count, 1, max_dist, 0.5)
        assert d2.shape == (len(names), ny, nx)
        for f, r in enumerate(refs):
            check_against((d2[f], near[f], m[f]), od.capped((r[1], r[2]), max_dist), 0.5, "frame %d (%s), max_dist %d" % (f, names[f], max_dist))
        assert (d2[2] == pwpp_hip.DIST_BEYOND).all() and (near[2] == -1).all()


@pytest.mark.parametrize("shape", [(7, 5), (64, 16), (65, 17)], ids=shape_ids)
def test_frames_never_see_each_other(handle, shape):
    nx, ny = shape
    count = np.zeros((2, ny, nx), np.int32)
    count[0, -1, :] = 1   # frame 0's last row and frame 1's first row are neighbours in memory
    count[1, 0, :] = 1
    want = od.distance_frames(count)
    d2, near, m = handle.distance_grid(count, 1, 0, 0.5)
    check_against((d2, near, m), want, 0.5, "two frames of %d x %d" % shape)
    iy = np.arange(ny)[:, None].repeat(nx, 1)
    assert np.array_equal(d2[0], (ny - 1 - iy) ** 2) and np.array_equal(d2[1], iy ** 2)
    assert (near[0] // nx == ny - 1).all() and (near[1] // nx == 0).all()


@pytest.mark.parametrize("shape", od.SHAPES, ids=shape_ids)
def test_two_runs_and_both_paths_give_identical_bytes(shape):
    nx, ny = shape
    h = pwpp_hip.Handle()
    for k, (name, min_count) in enumerate(CASES):
        count, dist2, nearest = reference(name, nx, ny, min_count)
        max_dist = od.MAX_DISTS[k % 4]
        runs = []
        for path in (0, 0, 1, 1):
            h.set_option("distance_path", path)
            runs.append(tuple(a.tobytes() for a in h.distance_grid(count, min_count, max_dist, 0.3)))
        what = "%s %dx%d min_count %d max_dist %d" % (name, nx, ny, min_count, max_dist)
        assert runs[0] == runs[1] and runs[2] == runs[3], what + ": two runs of the same call differ"
        assert runs[0] == runs[2], what + ": distance_path 0 and 1 differ"
        want = od.capped((dist2, nearest), max_dist)
        assert runs[2][0] == want[0].tobytes() and runs[2][1] == want[1].tobytes(), what + ": distance_path 1 differs from the brute force"
    with pytest.raises(pwpp_hip.PwppError):
        h.set_option("distance_path", 2)


def test_null_outputs_leave_the_others_unchanged(handle):
    count, dist2, nearest = reference("random0.1", 129, 33, 1)
    for max_dist in (0, 2):
        full = handle.distance_grid(count, 1, max_dist, 0.3)
        check_against(full, od.capped((dist2, nearest), max_dist), 0.3, "all three images")
        no_near = handle.distance_grid(count, 1, max_dist, 0.3, want_nearest=False)
        no_metres = handle.distance_grid(count, 1, max_dist, 0.3, want_metres=False)
        neither = handle.distance_grid(count, 1, max_dist, np.nan, want_nearest=False, want_metres=False)  # (cell is not read without metres)
        assert no_near[1] is None and no_metres[2] is None and neither[1] is None and neither[2] is None
        assert no_near[0].tobytes() == no_metres[0].tobytes() == neither[0].tobytes() == full[0].tobytes()
        assert no_near[2].tobytes() == full[2].tobytes() and no_metres[1].tobytes() == full[1].tobytes()


# ---- pwpp_distance_obstacles ----------------------------------------------------------------------------------------------------
GRIDS = [(-16.0, -16.0, 0.5, 64, 64), (2.0, -17 * 1.7 / 3, 1.7, 65, 17)]  # (x0, y0, cell, nx, ny): 64 x 64 of 0.5 m; 65 x 17 of 1.7 m that cuts the cloud


def obstacles_against_the_two_calls(h, grid, what, frames=3):
    x0, y0, cell, nx, ny = grid
    for ground_only in (False, True):
        rc = h.rasterize_obstacles(x0, y0, cell, nx, ny, *BAND, ground_only=ground_only, want_top=False)
        assert rc.shape == (frames, ny, nx)
        for min_count, max_dist in ((1, 0), (2, 0), (1, 5)):
            w = "%s, ground_only %s, min_count %d, max_dist %d" % (what, ground_only, min_count, max_dist)
            d2, near, m, count = h.distance_obstacles(x0, y0, cell, nx, ny, *BAND, min_count, max_dist, ground_only=ground_only, want_count=True)
            assert count.tobytes() == rc.tobytes(), w + ": the count image differs from pwpp_rasterize_obstacles"
            g2, gnear, gm = h.distance_grid(rc, min_count, max_dist, cell)
            assert (d2.tobytes(), near.tobytes(), m.tobytes()) == (g2.tobytes(), gnear.tobytes(), gm.tobytes()), w + ": differs from pwpp_distance_grid"
            check_against((d2, near, m), tuple(map(np.ascontiguousarray, od.distance_frames(rc, min_count, max_dist))), cell, w)
            # without the count image: the same three images
            e2, enear, em = h.distance_obstacles(x0, y0, cell, nx, ny, *BAND, min_count, max_dist, ground_only=ground_only)
            assert (e2.tobytes(), enear.tobytes(), em.tobytes()) == (d2.tobytes(), near.tobytes(), m.tobytes()), w
            # a sub-range of frames
            for first, n in ((frames - 1, 1), (1, frames - 1)):
                s2, snear, sm, scount = h.distance_obstacles(x0, y0, cell, nx, ny, *BAND, min_count, max_dist, frame_first=first, frames=n,
                                                             ground_only=ground_only, want_count=True)
                assert (s2.tobytes(), snear.tobytes(), sm.tobytes(), scount.tobytes()) == (
                    d2[first:first + n].tobytes(), near[first:first + n].tobytes(), m[first:first + n].tobytes(), rc[first:first + n].tobytes()), w
    return rc


@pytest.mark.parametrize("grid", GRIDS, ids=["64x64", "65x17"])
def test_distance_obstacles_is_rasterize_plus_distance_grid(grid):
    frames = three_frames()  # a 16-beam scan, an empty frame, a frame that is all unref
    h = pwpp_hip.Handle()
    h.set_labels(True)  # (_everything reads them)
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    before = _everything(h, 3)
    rc = obstacles_against_the_two_calls(h, grid, "fresh")
    assert (rc[0] > 0).sum() >= 3 and (rc[1:] == 0).all()  # the scan frame sees obstacles; the empty and the all-unref frame none
    d2 = h.distance_obstacles(*grid, *BAND)[0]
    assert (d2[1:] == pwpp_hip.DIST_BEYOND).all() and (d2[0] < pwpp_hip.DIST_BEYOND).all()
    assert _everything(h, 3) == before, "the distances changed the results of the call they read"


def test_distance_obstacles_after_streams_and_device_memory_calls():
    clouds = [small_cloud(s) for s in (5, 6, 7)]
    h = pwpp_hip.Handle()
    h.set_order(pwpp_hip.ORDER_CLOUD)
    h.set_num_streams(3)
    h.estimate_ground_batch(clouds, mode=pwpp_hip.MODE_STREAMS)
    before, t_before = _everything(h, 3), h.time_us()
    rc = obstacles_against_the_two_calls(h, GRIDS[0], "streams")
    assert (rc > 0).sum(axis=(1, 2)).min() >= 1
    assert _everything(h, 3) == before and h.time_us() == t_before, "the distances changed the results of the call they read"
    streams = tuple(a.tobytes() for a in h.distance_obstacles(*GRIDS[0], *BAND, 1, 5, want_count=True))
    # a device-memory estimate call (the input stays alive: `tens`), and the distances into device memory one word off a 16-byte boundary
    import torch
    c = pwpp_hip.Handle()
    c.set_labels(True)
    tens = [device_tensor(f) for f in clouds]
    c.estimate_ground_batch_device([t.data_ptr() for t in tens], [len(f) for f in clouds])
    before = _everything(c, 3)
    obstacles_against_the_two_calls(c, GRIDS[0], "device-memory call")
    assert tuple(a.tobytes() for a in c.distance_obstacles(*GRIDS[0], *BAND, 1, 5, want_count=True)) == streams
    x0, y0, cell, nx, ny = GRIDS[0]
    cells = 3 * nx * ny
    bufs = [torch.full((cells + 8,), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
    c.distance_obstacles_device(x0, y0, cell, nx, ny, *BAND, 1, 5, bufs[0].data_ptr() + 4, bufs[1].data_ptr() + 8, bufs[2].data_ptr() + 12, bufs[3].data_ptr())
    c.synchronize()
    raw = [b.cpu().numpy() for b in bufs]
    for k, r in enumerate(raw):
        s = (1, 2, 3, 0)[k]
        assert r[s:s + cells].tobytes() == streams[k], "image %d into device memory" % k
        assert (r[:s] == -7).all() and (r[s + cells:] == -7).all()
    assert _everything(c, 3) == before
    del tens


def test_the_optional_images_of_the_obstacles_entry_points_change_nothing_else():
    """pwpp_label_obstacles, pwpp_distance_obstacles and pwpp_visibility_obstacles, each on host and on device memory, with and
    without the images of the raster (count; top for the labels): kept in the handle's buffer or handed to the caller, the
    operator's own outputs are the same bytes, and a count image that is returned is pwpp_rasterize_obstacles'."""
    import torch
    x0, y0, cell, nx, ny = grid = GRIDS[1]  # 65 x 17: no multiple of 64 across, cuts the cloud
    rows, origin = 64, (3.0, 0.0)
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(three_frames(), mode=pwpp_hip.MODE_FRESH)
    rc, rtop = h.rasterize_obstacles(*grid, *BAND)
    assert (rc[0] > 0).sum() >= 3
    cells = 3 * nx * ny
    words = lambda n=cells: torch.full((n,), -7, dtype=torch.int32, device="cuda")

    def fetch(*tensors):
        h.synchronize()
        return [t.cpu().numpy() for t in tensors]

    def label_bytes(label, table, n):
        n = np.asarray(n).reshape(-1)
        assert n[0] >= 1
        table = np.asarray(table).view(np.uint8).reshape(3, rows * 48)
        return label.tobytes(), b"".join(table[f, :48 * min(n[f], rows)].tobytes() for f in range(3)), n.tobytes()  # (the rows below n)

    def labels(on_device, images):
        if not on_device:
            out = h.label_obstacles(*grid, *BAND, 1, 8, rows, want_images=images)
            return label_bytes(*out[:3]), (out[3], out[4]) if images else None
        d_label, d_table, d_n, d_count, d_top = words(), words(3 * rows * 12), words(3), words(), words()
        h.label_obstacles_device(*grid, *BAND, 1, 8, d_label.data_ptr(), d_count.data_ptr() if images else 0, d_top.data_ptr() if images else 0,
                                 d_table.data_ptr(), d_n.data_ptr(), rows)
        label, table, n, count, top = fetch(d_label, d_table, d_n, d_count, d_top)
        return label_bytes(label, table, n), (count, top.view(np.float32)) if images else None

    def distances(on_device, images):
        if not on_device:
            out = h.distance_obstacles(*grid, *BAND, 1, 0, want_count=images)
            return tuple(a.tobytes() for a in out[:3]), (out[3],) if images else None
        d_dist2, d_nearest, d_metres, d_count = words(), words(), words(), words()
        h.distance_obstacles_device(*grid, *BAND, 1, 0, d_dist2.data_ptr(), d_nearest.data_ptr(), d_metres.data_ptr(), d_count.data_ptr() if images else 0)
        dist2, nearest, metres, count = fetch(d_dist2, d_nearest, d_metres, d_count)
        return (dist2.tobytes(), nearest.tobytes(), metres.tobytes()), (count,) if images else None

    def visibility(on_device, images):
        if not on_device:
            out = h.visibility_obstacles(*grid, *BAND, origin, 1, 0, want_count=images)
            return (out[0].tobytes(), out[1].tobytes()), (out[2],) if images else None
        d_first, d_occ, d_count = words(), torch.full((cells,), -7, dtype=torch.int8, device="cuda"), words()
        h.visibility_obstacles_device(*grid, *BAND, origin, 1, 0, d_first.data_ptr(), d_occ.data_ptr(), d_count.data_ptr() if images else 0)
        first, occ, count = fetch(d_first, d_occ, d_count)
        return (first.tobytes(), occ.tobytes()), (count,) if images else None

    for operator in (labels, distances, visibility):
        want = None
        for on_device in (False, True):
            for images in (True, False):
                what = "%s, %s memory, %s the images" % (operator.__name__, "device" if on_device else "host", "with" if images else "without")
                got, raster = operator(on_device, images)
                want = got if want is None else want
                assert got == want, what
                if images:
                    assert raster[0].tobytes() == rc.tobytes(), what + ": the count image differs from pwpp_rasterize_obstacles"
                    assert len(raster) == 1 or raster[1].tobytes() == rtop.tobytes(), what + ": the top image differs from pwpp_rasterize_obstacles"


def test_state_workspace_and_arguments():
    L = pwpp_hip.load()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    d2 = np.zeros(3 * 16, np.int32)
    g = pwpp_hip.GroundGrid(-2.0, -2.0, 1.0, 4, 4, 0, 0)

    def obstacles(h, first=0, frames=1, mem=pwpp_hip.MEM_HOST, grid=g):
        return L.pwpp_distance_obstacles(h._h, ctypes.byref(grid), 0.2, 2.5, 1, 0, first, frames, mem, vp(d2), None, None, None)

    h = pwpp_hip.Handle()
    empty = h.workspace_bytes()
    assert obstacles(h) == E_STATE  # before any estimate call ...
    count, dist2, nearest = reference("random0.3", 65, 17, 1)
    check_against(h.distance_grid(count, 1, 0, 0.5), (dist2, nearest), 0.5, "before any estimate call")  # ... pwpp_distance_grid works
    grown = h.workspace_bytes()
    assert grown >= empty + 4 * 4 * 65 * 17, "the cluster buffer (working image and four staged images) is not counted by pwpp_get_workspace_bytes"
    h.trim_workspace()
    assert h.workspace_bytes() == empty, "pwpp_trim_workspace did not free the cluster buffer"
    assert obstacles(h) == E_STATE
    # with the feature unused nothing is allocated
    a, b = pwpp_hip.Handle(), pwpp_hip.Handle()
    frames = three_frames()
    for w in (a, b):
        w.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert a.workspace_bytes() == b.workspace_bytes()
    b.distance_obstacles(-20.0, -20.0, 0.5, 80, 80, *BAND)
    assert b.workspace_bytes() >= a.workspace_bytes() + 4 * 3 * 80 * 80
    b.trim_workspace()
    a.trim_workspace()
    assert a.workspace_bytes() == b.workspace_bytes()
    assert obstacles(b) == E_STATE  # after pwpp_trim_workspace the call's results are gone
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
    assert L.pwpp_distance_grid(h._h, 4, 4, 1, pwpp_hip.MEM_HOST_PINNED, vp(cnt), 1, 0, 1.0, vp(d2), None, None) == E_ARG


def test_pybind_module_agrees_with_the_ctypes_handle():
    import pypatchworkpp
    pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    h = pwpp_hip.Handle()
    with pytest.raises(RuntimeError):
        pp.getObstacleDistances(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5)  # no frame yet
    pts = small_cloud(5)
    pp.estimateGround(pts)
    h.estimate_ground(pts)
    for min_count, max_dist, ground_only in ((1, 0, False), (2, 6, True)):
        d2, near, m = pp.getObstacleDistances(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5, min_count, max_dist, ground_only)
        h2, hnear, hm = h.distance_obstacles(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5, min_count, max_dist, ground_only=ground_only)
        assert d2.dtype == np.int32 and near.dtype == np.int32 and m.dtype == np.float32 and d2.shape == near.shape == m.shape == (48, 120)
        assert (d2 == 0).sum() >= 3
        assert d2.tobytes() == h2[0].tobytes() and near.tobytes() == hnear[0].tobytes() and m.tobytes() == hm[0].tobytes()
    with pytest.raises(RuntimeError):
        pp.getObstacleDistances(0.0, 0.0, 1.0, 4, 4, 0.2, 2.5, 0)
