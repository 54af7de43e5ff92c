"""The line-of-sight free space (pwpp_visibility_grid, pwpp_visibility_obstacles) on a real MI355X, byte for byte against the brute
force of tests/obstacle_visibility_ref.py: small shapes with the whole image compared -- every occupancy from empty to full,
origins in the corners, on an edge, in the middle and on an occupied cell, min_count 1 and 3, from host and from device memory, on
both values of the option "visibility_path" -- the watertight ring, max_range, the independence of the frames of a batch, one
image on either side of the kernel's LDS limit, misaligned device images, pwpp_visibility_obstacles against
pwpp_rasterize_obstacles + pwpp_visibility_grid on a KITTI frame, and that asking changes nothing else."""
import ctypes
import functools

import numpy as np
import pytest

import obstacle_visibility_ref as ov
import pwpp_hip
from test_gpu_obstacle_grid import _everything, three_frames

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
BAND = (0.2, 2.5)
# (nx, ny, frames): a single cell; a column and a row longer than a wave; a tile's corner; 33 columns: a row of bits straddles a
# word; whole tiles; one past / one short of them; several frames of several tiles with an origin each
SHAPES = [(1, 1, 1), (1, 70, 1), (70, 1, 1), (5, 7, 1), (33, 31, 1), (64, 64, 1), (65, 63, 1), (130, 129, 3)]
FILLS = (0.0, 0.05, 0.4, 1.0)
shape_ids = lambda s: "%dx%dx%d" % s


def origin_kinds(nx, ny, count):
    """The four corners, the middle of an edge, the middle of the image, a cell of the largest count (occupied where any is)."""
    iy, ix = np.nonzero(count >= count.max()) if count.max() > 0 else (np.array([ny // 2]), np.array([nx // 2]))
    return [(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1), (nx // 2, ny - 1), (nx // 2, ny // 2), (int(ix[len(ix) // 2]), int(iy[len(iy) // 2]))]


@functools.lru_cache(maxsize=None)
def case(nx, ny, frames, fill, min_count):
    """(count, origins of each call, (first, occupancy) of each call) of a shape: computed once, shared, never written."""
    count = np.stack([ov.random_count(nx, ny, fill, min_count, 1000 * f + nx + 7 * ny + min_count) for f in range(frames)])
    kinds = origin_kinds(nx, ny, count[0])
    if frames == 1:
        calls = [np.array([k], np.int32) for k in dict.fromkeys(kinds)]
    else:  # one call, an origin per frame: which kinds rotates with the case, so that the cases together cover all of them
        r = int(fill * 20) + min_count
        calls = [np.array([kinds[(r + 2 * f) % len(kinds)] for f in range(frames)], np.int32)]
    want = [ov.visibility_frames(count, o, min_count) for o in calls]
    for a in [count] + calls + [w for pair in want for w in pair]:
        a.setflags(write=False)
    return count, calls, want


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()  # (no estimate call: pwpp_visibility_grid needs the handle's stream and buffer only)


def from_device(h, count, origins, min_count, max_range, shift_words=0, shift_bytes=0):
    """visibility_grid on device images; first and count start shift_words words, occupancy shift_bytes bytes behind a 256-byte
    boundary; the words and bytes around them are poisoned and must survive."""
    import torch
    frames, ny, nx = count.shape
    cells = count.size
    bufs = [torch.full((cells + 128,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    occ = torch.full((cells + 512,), -7, dtype=torch.int8, device="cuda")
    assert all(b.data_ptr() % 256 == 0 for b in bufs + [occ])
    bufs[0][shift_words:shift_words + cells] = torch.from_numpy(count.reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    h.visibility_grid_device(nx, ny, frames, bufs[0].data_ptr() + 4 * shift_words, origins, min_count, max_range, bufs[1].data_ptr() + 4 * shift_words,
                             occ.data_ptr() + shift_bytes)
    h.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
    raw = [b.cpu().numpy() for b in bufs] + [occ.cpu().numpy()]
    for r, s in ((raw[0], shift_words), (raw[1], shift_words), (raw[2], shift_bytes)):
        assert (r[:s] == -7).all() and (r[s + cells:] == -7).all(), "a word or byte outside an image was written"
    assert np.array_equal(raw[0][shift_words:shift_words + cells], count.reshape(-1)), "the count image was written"
    return raw[1][shift_words:shift_words + cells].reshape(count.shape), raw[2][shift_bytes:shift_bytes + cells].reshape(count.shape)


def both_paths(h, call):
    """call() at "visibility_path" 0 and 1: identical bytes; returns them."""
    res = []
    for path in (0, 1):
        h.set_option("visibility_path", path)
        res.append(call())
    h.set_option("visibility_path", 0)
    assert res[0][0].tobytes() == res[1][0].tobytes(), "first differs between visibility_path 0 and 1 in %d cells" % (res[0][0] != res[1][0]).sum()
    assert res[0][1].tobytes() == res[1][1].tobytes(), "occupancy differs between visibility_path 0 and 1"
    return res[0]


def check(got, want, what):
    first, occ = got
    assert first.dtype == np.int32 and first.shape == want[0].shape and occ.dtype == np.int8 and occ.shape == want[1].shape, what
    assert np.array_equal(first, want[0]), "%s: first differs from the brute force in %d cells" % (what, (first != want[0]).sum())
    assert np.array_equal(occ, want[1]), "%s: occupancy differs in %d cells" % (what, (occ != want[1]).sum())


# ---- small shapes, the whole image ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_small_shapes_against_the_brute_force(handle, shape):
    nx, ny, frames = shape
    seen = hidden = 0
    for fill in FILLS:
        for min_count in (1, 3):
            count, calls, want = case(nx, ny, frames, fill, min_count)
            for origins, w in zip(calls, want):
                what = "%dx%dx%d fill %g min_count %d origins %s" % (nx, ny, frames, fill, min_count, origins.tolist())
                check(both_paths(handle, lambda: handle.visibility_grid(count, origins, min_count)), w, what + ", host memory")
                check(both_paths(handle, lambda: from_device(handle, count, origins, min_count, 0)), w, what + ", device memory")
                seen += int((w[0] == ov.NONE).sum())
                hidden += int(((w[0] >= 0) & (w[1] == ov.UNKNOWN)).sum())
            if fill == 0.0:
                assert all((w[0] == ov.NONE).all() and (w[1] == ov.FREE).all() for w in want)
            if fill == 1.0:
                assert all((w[1] == ov.OCCUPIED).all() for w in want)
    assert seen > 0 and (hidden > 0 or nx * ny == 1)
    # without the occupancy image: the same first
    count, calls, want = case(nx, ny, frames, 0.05, 1)
    first, none = handle.visibility_grid(count, calls[0], 1, want_occupancy=False)
    assert none is None and np.array_equal(first, want[0][0])


# ---- the ring ---------------------------------------------------------------------------------------------------------------------
def test_the_ring_is_watertight_on_the_device(handle):
    count, disc = ov.ring_image()
    batch = np.stack([count] * len(ov.RING_ORIGINS))
    origins = np.array(ov.RING_ORIGINS, np.int32)
    first, occ = both_paths(handle, lambda: handle.visibility_grid(batch, origins))
    check((first, occ), ov.visibility_frames(batch, origins), "the ring")
    for f in range(len(origins)):
        assert (first[f][~disc] != ov.NONE).all() and (occ[f][~disc] == ov.UNKNOWN).all(), "origin %s: the ring leaks" % (ov.RING_ORIGINS[f],)
        assert (first[f][disc & (count == 0)] == ov.NONE).all()


# ---- max_range --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(33, 31, 1), (65, 63, 1), (130, 129, 3)], ids=shape_ids)
def test_max_range_changes_nothing_inside_it(handle, shape):
    nx, ny, frames = shape
    iy, ix = np.mgrid[0:ny, 0:nx]
    for fill in (0.05, 0.4):
        count, calls, want = case(nx, ny, frames, fill, 1)
        origins, (unlimited, _) = calls[-1], want[-1]
        per_frame = origins.repeat(frames, 0) if len(origins) == 1 else origins
        for max_range in (1, 7, 200):
            what = "%dx%dx%d fill %g max_range %d" % (nx, ny, frames, fill, max_range)
            first, occ = both_paths(handle, lambda: handle.visibility_grid(count, origins, 1, max_range))
            dfirst, docc = from_device(handle, count, origins, 1, max_range)
            assert dfirst.tobytes() == first.tobytes() and docc.tobytes() == occ.tobytes(), what
            for f in range(frames):
                n = np.maximum(np.abs(ix - per_frame[f][0]), np.abs(iy - per_frame[f][1]))
                assert (first[f][n > max_range] == ov.BEYOND).all(), what
                assert np.array_equal(first[f][n <= max_range], unlimited[f][n <= max_range]), what
                assert (first[f] != ov.BEYOND).all() or max_range < max(nx, ny)
            assert np.array_equal(occ, ov.occupancy_of(count, first)), what + ": occupancy does not follow first"


# ---- frames -----------------------------------------------------------------------------------------------------------------------
def test_a_batch_is_its_frames(handle):
    count, calls, want = case(130, 129, 3, 0.05, 1)
    origins = calls[0]
    first, occ = handle.visibility_grid(count, origins)
    check((first, occ), want[0], "three frames")
    for f in range(3):
        one_first, one_occ = handle.visibility_grid(count[f], origins[f])
        assert one_first.tobytes() == first[f].tobytes() and one_occ.tobytes() == occ[f].tobytes(), "frame %d alone" % f
    # one origin for every frame = the same origin repeated
    a = handle.visibility_grid(count, origins[1])
    b = handle.visibility_grid(count, origins[1][None, :].repeat(3, 0))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[0][1].tobytes() == first[1].tobytes() and not np.array_equal(a[0][0], first[0])
    with pytest.raises(pwpp_hip.PwppError):
        handle.visibility_grid(count, origins[:2])  # two origins for three frames


# ---- the LDS limit ----------------------------------------------------------------------------------------------------------------
# The kernel keeps a frame's bit image in LDS up to 128 KiB: 1024 rows of 32 words fit exactly, 1024 rows of 33 words (1056 columns)
# are the first that do not and are read from global memory.
@pytest.mark.parametrize("shape", [(1024, 1024), (1056, 1024)], ids=lambda s: "%dx%d" % s)
def test_either_side_of_the_lds_limit(handle, shape):
    nx, ny = shape
    assert ((nx + 31) // 32 * ny * 4 <= 128 * 1024) == (nx == 1024)
    count = ov.random_count(nx, ny, 0.002, 1, 5)  # sparse: most lines run for hundreds of cells
    origin = np.array([700, 300], np.int32)
    first, occ = both_paths(handle, lambda: handle.visibility_grid(count, origin))  # path 0 against path 1, the whole image
    rng = np.random.default_rng(11)
    cells = np.concatenate([np.stack([rng.integers(0, nx, 4096), rng.integers(0, ny, 4096)], 1),
                            np.stack([np.arange(nx), np.zeros(nx, int)], 1), np.stack([np.arange(nx), np.full(nx, ny - 1)], 1),
                            np.stack([np.zeros(ny, int), np.arange(ny)], 1), np.stack([np.full(ny, nx - 1), np.arange(ny)], 1)])
    want = ov.first_of(count, origin, cells=cells)
    got = first[cells[:, 1], cells[:, 0]]
    assert np.array_equal(got, want), "%d of %d sampled cells differ from the brute force" % ((got != want).sum(), len(cells))
    assert np.array_equal(occ[cells[:, 1], cells[:, 0]], ov.occupancy_of(count, want, cells=cells))
    assert (want == ov.NONE).sum() > 100 and (want >= 0).sum() > 100


# ---- alignment --------------------------------------------------------------------------------------------------------------------
def test_device_images_one_word_and_one_byte_off_a_256_byte_boundary(handle):
    for nx, ny, frames in ((65, 63, 1), (130, 129, 3)):
        count, calls, want = case(nx, ny, frames, 0.05, 1)
        for max_range in (0, 7):
            aligned = from_device(handle, count, calls[0], 1, max_range)
            shifted = both_paths(handle, lambda: from_device(handle, count, calls[0], 1, max_range, shift_words=1, shift_bytes=1))
            assert shifted[0].tobytes() == aligned[0].tobytes() and shifted[1].tobytes() == aligned[1].tobytes()
            if max_range == 0:
                check(shifted, want[0], "%dx%dx%d shifted" % (nx, ny, frames))


# ---- pwpp_visibility_obstacles ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(256, 256, 0.5), (64, 64, 2.0)], ids=["256x256", "64x64"])
def test_visibility_obstacles_is_rasterize_plus_visibility_grid(kitti, grid):
    nx, ny, cell = grid
    x0, y0 = -0.5 * nx * cell, -0.5 * ny * cell
    L = pwpp_hip.load()
    h = pwpp_hip.Handle()
    g = pwpp_hip.GroundGrid(x0, y0, cell, nx, ny, 0, 0)
    first_buf, zero = np.zeros(nx * ny, np.int32), np.zeros(2, np.float64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.pwpp_visibility_obstacles(h._h, ctypes.byref(g), BAND[0], BAND[1], 1, vp(zero), 1, 0, 0, 1, pwpp_hip.MEM_HOST, vp(first_buf), None, None) == E_STATE
    h.set_labels(True)  # (_everything reads them)
    h.estimate_ground(kitti[0])
    before = _everything(h, 1)
    rc = h.rasterize_obstacles(x0, y0, cell, nx, ny, *BAND, want_top=False)
    assert rc.shape == (1, ny, nx) and (rc > 0).sum() > 100
    for min_count, max_range in ((1, 0), (2, 0), (1, 40)):
        what = "%d x %d, min_count %d, max_range %d" % (nx, ny, min_count, max_range)
        first, occ, count = both_paths(h, lambda: h.visibility_obstacles(x0, y0, cell, nx, ny, *BAND, (0.0, 0.0), min_count, max_range, want_count=True))
        assert count.tobytes() == rc.tobytes(), what + ": the count image differs from pwpp_rasterize_obstacles"
        gfirst, gocc = h.visibility_grid(rc, (nx // 2, ny // 2), min_count, max_range)  # {0, 0} m is the cell (nx / 2, ny / 2) of this grid
        assert first.tobytes() == gfirst.tobytes() and occ.tobytes() == gocc.tobytes(), what + ": differs from pwpp_visibility_grid"
        kfirst, kocc = h.visibility_obstacles(x0, y0, cell, nx, ny, *BAND, (0.0, 0.0), min_count, max_range)  # the count image kept in the handle
        assert kfirst.tobytes() == first.tobytes() and kocc.tobytes() == occ.tobytes(), what
        want = ov.first_of(rc[0], (nx // 2, ny // 2), min_count, max_range)
        check((first[0], occ[0]), (want, ov.occupancy_of(rc[0], want, min_count)), what)
    assert (occ == ov.FREE).sum() > 100 and (occ == ov.UNKNOWN).sum() > 100 and (occ == ov.OCCUPIED).sum() > 100
    # an origin by the cell rule; one outside the grid, one that is no number
    off = h.visibility_obstacles(x0, y0, cell, nx, ny, *BAND, (3.2, -7.9))
    goff = h.visibility_grid(rc, (int(np.floor((3.2 - x0) / cell)), int(np.floor((-7.9 - y0) / cell))))
    assert off[0].tobytes() == goff[0].tobytes() and off[1].tobytes() == goff[1].tobytes()
    for xy in ((-x0, 0.0), (0.0, y0 - 1e-9), (np.nan, 0.0)):
        assert L.pwpp_visibility_obstacles(h._h, ctypes.byref(g), BAND[0], BAND[1], 1, vp(np.array(xy, np.float64)), 1, 0, 0, 1, pwpp_hip.MEM_HOST,
                                           vp(first_buf), None, None) == E_ARG, xy
        assert b"origin 0" in L.pwpp_last_error()
    # into device memory, the images one word / one byte off a 256-byte boundary
    import torch
    bufs = [torch.full((nx * ny + 128,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    docc = torch.full((nx * ny + 512,), -7, dtype=torch.int8, device="cuda")
    h.visibility_obstacles_device(x0, y0, cell, nx, ny, *BAND, (0.0, 0.0), 1, 40, bufs[0].data_ptr() + 4, docc.data_ptr() + 1, bufs[1].data_ptr() + 4)
    h.synchronize()
    raw = [b.cpu().numpy() for b in bufs] + [docc.cpu().numpy()]
    assert raw[0][1:1 + nx * ny].tobytes() == first.tobytes() and raw[2][1:1 + nx * ny].tobytes() == occ.tobytes() and raw[1][1:1 + nx * ny].tobytes() == rc.tobytes()
    for r in raw:
        assert (r[:1] == -7).all() and (r[1 + nx * ny:] == -7).all()
    assert _everything(h, 1) == before, "the visibility changed the results of the call it reads"


def test_three_frames_with_an_origin_each():
    frames = three_frames()  # a 16-beam scan, an empty frame, a frame that is all unref
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    grid = (-16.0, -16.0, 0.5, 64, 64)
    xy = np.array([[0.0, 0.0], [3.3, -2.1], [-15.9, 15.9]])
    cells = np.floor((xy + 16.0) / 0.5).astype(np.int32)
    rc = h.rasterize_obstacles(*grid, *BAND, want_top=False)
    first, occ = both_paths(h, lambda: h.visibility_obstacles(*grid, *BAND, xy))
    check((first, occ), ov.visibility_frames(rc, cells), "three frames")
    assert (occ[1:] == ov.FREE).all() and (first[0] >= 0).sum() >= 3  # the empty and the all-unref frame hold no obstacle: all seen
    sub = h.visibility_obstacles(*grid, *BAND, xy[1:], frame_first=1, frames=2)  # entry i belongs to frame frame_first + i
    assert sub[0].tobytes() == first[1:].tobytes() and sub[1].tobytes() == occ[1:].tobytes()


# ---- workspace ----------------------------------------------------------------------------------------------------------------------
def test_workspace_and_that_nothing_else_moves():
    h = pwpp_hip.Handle()
    empty = h.workspace_bytes()
    count, calls, want = case(65, 63, 1, 0.05, 1)
    check(h.visibility_grid(count, calls[0]), want[0], "before any estimate call")
    grown = h.workspace_bytes()
    # the bit image (3 words a row), the staged count and first images and the byte image in words
    assert grown >= empty + 4 * (3 * 63 + 2 * 65 * 63 + (65 * 63 + 3) // 4), "the cluster buffer is not counted by pwpp_get_workspace_bytes"
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
    b.visibility_obstacles(-20.0, -20.0, 0.5, 80, 80, *BAND, np.zeros((3, 2)))
    assert b.workspace_bytes() >= a.workspace_bytes() + 4 * (3 * 80 * 3 + 6 + 3 * 80 * 80)  # the bit image, three origins, the kept count image
    assert _everything(b, 3) == before and b.time_us() == t_before, "the visibility changed the results of the call it reads"
    for w in (a, b):
        w.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert _everything(b, 3) == _everything(a, 3), "an estimate call after a visibility call differs from one without"
    b.trim_workspace()
    a.trim_workspace()
    assert a.workspace_bytes() == b.workspace_bytes()
    with pytest.raises(pwpp_hip.PwppError):
        h.set_option("visibility_path", 2)


def test_pybind_module_agrees_with_the_ctypes_handle():
    import pypatchworkpp
    from test_gpu_obstacle_grid import small_cloud
    pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    h = pwpp_hip.Handle()
    with pytest.raises(RuntimeError):
        pp.getObstacleVisibility(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5)  # no frame yet
    pts = small_cloud(5)
    pp.estimateGround(pts)
    h.estimate_ground(pts)
    for min_count, max_range, origin, ground_only in ((1, 0, (0.0, 0.0), False), (2, 30, (2.2, -1.1), True)):
        first, occ = pp.getObstacleVisibility(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5, min_count, max_range, origin[0], origin[1], ground_only)
        hfirst, hocc = h.visibility_obstacles(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5, origin, min_count, max_range, ground_only=ground_only)
        assert first.dtype == np.int32 and occ.dtype == np.int8 and first.shape == occ.shape == (48, 120)
        assert (occ == ov.OCCUPIED).sum() >= 3
        assert first.tobytes() == hfirst[0].tobytes() and occ.tobytes() == hocc[0].tobytes()
    with pytest.raises(RuntimeError):
        pp.getObstacleVisibility(0.0, 0.0, 1.0, 4, 4, 0.2, 2.5, 1, 0, 9.0, 0.0)  # the origin outside the grid
