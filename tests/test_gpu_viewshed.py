"""The viewshed (pwpp_viewshed_grid, pwpp_rasterize_ground_returns, pwpp_viewshed_obstacles) on a real MI355X, byte for byte against
the brute force of tests/viewshed_ref.py: the visibility's small shapes with the whole image compared -- every occupancy from empty
to full, random block and target heights with a tenth PWPP_VIEW_NO_HEIGHT and rises that reach +-R and beyond, origins in the
corners, on an edge, in the middle and on an occupied cell with an eye per frame, from host and from device memory, on both values
of the option "viewshed_path", with and without shadow, seen and occupancy -- degenerate input against pwpp_visibility_grid itself,
the subset theorem, the kerb, max_range, the independence of the frames of a batch, witnessed cells, one image on either side of the
LDS path's limit, the window of rows in LDS and the launch plan that both operators share, misaligned device images, the ground-returns raster against numpy, the chained call against its four stages on
KITTI frames, and that asking changes nothing else."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import obstacle_visibility_ref as ov
import pwpp_hip
import viewshed_ref as vr
from test_gpu_obstacle_grid import _everything, small_cloud, three_frames
from test_gpu_obstacle_visibility import FILLS, SHAPES, from_device as vis_from_device, origin_kinds, shape_ids

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
BAND = (0.2, 2.5)
PATHS = (1, 2)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def case(nx, ny, frames, fill, variant):
    """(count, block, target, seen, min_count, min_seen, origins of each call, (first, shadow, occupancy) of each call) of a shape:
    computed once, shared, never written.  variant 0: all three images; 1: block alone, min_count 3; 2: target and seen alone."""
    min_count, min_seen = (1, 3, 1)[variant], (2, 1, 1)[variant]
    seed = 1000 * variant + nx + 7 * ny + int(fill * 100)
    count = np.stack([ov.random_count(nx, ny, fill, min_count, seed + 31 * f) for f in range(frames)])
    eyes = [1700, -350, 12000]
    kinds = origin_kinds(nx, ny, count[0])
    if frames == 1:
        calls = [np.array([k + (eyes[i % 3],)], np.int32) for i, k in enumerate(dict.fromkeys(kinds))]
    else:  # one call, an origin and an eye per frame
        r = int(fill * 20) + variant
        calls = [np.array([kinds[(r + 2 * f) % len(kinds)] + (eyes[f % 3],) for f in range(frames)], np.int32)]
    shape = (frames, ny, nx)
    block = vr.random_heights(shape, 1700, seed + 1) if variant in (0, 1) else None
    target = vr.random_heights(shape, 1700, seed + 2) if variant in (0, 2) else None
    seen = np.random.default_rng(seed + 3).integers(0, 4, shape).astype(np.int32) if variant in (0, 2) else None
    want = [vr.viewshed_frames(count, o, block, target, seen, min_count, min_seen) for o in calls]
    for a in [count, block, target, seen] + calls + [w for three in want for w in three]:
        if a is not None:
            a.setflags(write=False)
    return count, block, target, seen, min_count, min_seen, calls, want


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()  # (no estimate call: pwpp_viewshed_grid needs the handle's stream and buffer only)


def from_device(h, count, origins, block=None, target=None, seen=None, min_count=1, min_seen=1, max_range=0, shift_words=0, shift_bytes=0, want_shadow=True,
                want_occupancy=True):
    """viewshed_grid on device images; the int32 images start shift_words words, occupancy shift_bytes bytes behind a 256-byte boundary;
    the words and bytes around them are poisoned and must survive, and the inputs must come back unwritten."""
    import torch
    frames, ny, nx = count.shape
    cells = count.size
    ins = [count, block, target, seen]
    bufs = [torch.full((cells + 128,), -7, dtype=torch.int32, device="cuda") for _ in range(6)]  # count, block, target, seen, first, shadow
    occ = torch.full((cells + 512,), -7, dtype=torch.int8, device="cuda")
    assert all(b.data_ptr() % 256 == 0 for b in bufs + [occ])
    for b, a in zip(bufs, ins):
        if a is not None:
            b[shift_words:shift_words + cells] = torch.from_numpy(a.reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    ptr = lambda k, present=True: bufs[k].data_ptr() + 4 * shift_words if present else 0
    h.viewshed_grid_device(nx, ny, frames, ptr(0), origins, min_count, max_range, ptr(4), ptr(5, want_shadow), occ.data_ptr() + shift_bytes if want_occupancy else 0,
                           ptr(1, block is not None), ptr(2, target is not None), ptr(3, seen is not None), min_seen)
    h.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
    raw = [b.cpu().numpy() for b in bufs] + [occ.cpu().numpy()]
    for k, r in enumerate(raw):
        s = shift_bytes if k == 6 else shift_words
        assert (r[:s] == -7).all() and (r[s + cells:] == -7).all(), "a word or byte outside an image was written"
    for k, a in enumerate(ins):
        body = raw[k][shift_words:shift_words + cells]
        assert np.array_equal(body, a.reshape(-1)) if a is not None else (body == -7).all(), "an input image was written"
    if not want_shadow:
        assert (raw[5] == -7).all()
    if not want_occupancy:
        assert (raw[6] == -7).all()
    cut = lambda k, s: raw[k][s:s + cells].reshape(count.shape)
    return cut(4, shift_words), cut(5, shift_words) if want_shadow else None, cut(6, shift_bytes) if want_occupancy else None


def both_paths(h, call):
    """call() at "viewshed_path" 0, 1 and 2: identical bytes; returns them."""
    res = []
    for path in (0,) + PATHS:
        h.set_option("viewshed_path", path)
        res.append(call())
    h.set_option("viewshed_path", 0)
    for r in res[1:]:
        for a, b, name in zip(res[0], r, ("first", "shadow", "occupancy", "count")):
            assert (a is None and b is None) or a.tobytes() == b.tobytes(), "%s differs between two values of viewshed_path in %d cells" % (name, (a != b).sum())
    return res[0]


def check(got, want, what):
    for g, w, name, dt in zip(got, want, ("first", "shadow", "occupancy"), (np.int32, np.int32, np.int8)):
        assert g.dtype == dt and g.shape == w.shape, what
        assert np.array_equal(g, w), "%s: %s differs from the brute force in %d cells" % (what, name, (g != w).sum())


# ---- small shapes, the whole image ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_small_shapes_against_the_brute_force(handle, shape):
    nx, ny, frames = shape
    hidden = over = 0
    for fill in FILLS:
        for variant in (0, 1, 2):
            count, block, target, seen, min_count, min_seen, calls, want = case(nx, ny, frames, fill, variant)
            for origins, w in zip(calls, want):
                what = "%dx%dx%d fill %g variant %d origins %s" % (nx, ny, frames, fill, variant, origins.tolist())
                kw = dict(block=block, target=target, seen=seen, min_count=min_count, min_seen=min_seen)
                check(both_paths(handle, lambda: handle.viewshed_grid(count, origins, **kw)), w, what + ", host memory")
                check(both_paths(handle, lambda: from_device(handle, count, origins, **kw)), w, what + ", device memory")
                own = np.arange(nx * ny).reshape(ny, nx)
                hidden += int(((w[0] >= 0) & (w[0] != own)).sum())
                over += int(((w[1] != vr.NO_HEIGHT) & ((w[0] == vr.NONE) | (w[0] == own))).sum())
            if fill == 0.0:
                assert all((w[0] == vr.NONE).all() and (w[1] == vr.NO_HEIGHT).all() and (w[2] == vr.FREE).all() for w in want)
            if fill == 1.0:
                assert all((w[2] == vr.OCCUPIED).all() for w in want)
        # without the shadow image (the walk stops at the first blocker that hides), without the occupancy image: the same first
        count, block, target, seen, min_count, min_seen, calls, want = case(nx, ny, frames, fill, 0)
        kw = dict(block=block, target=target, seen=seen, min_count=min_count, min_seen=min_seen)
        first, none_s, occ = both_paths(handle, lambda: handle.viewshed_grid(count, calls[0], want_shadow=False, **kw))
        assert none_s is None and np.array_equal(first, want[0][0]) and np.array_equal(occ, want[0][2])
        first, none_s, none_o = both_paths(handle, lambda: from_device(handle, count, calls[0], want_shadow=False, want_occupancy=False, **kw))
        assert none_s is None and none_o is None and np.array_equal(first, want[0][0])
    assert nx * ny == 1 or (hidden > 0 and over > 0), "the cases hold no hidden cell, or no cell seen over a blocker"


# ---- theorems 1 and 2 on the device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_degenerate_input_is_pwpp_visibility_grid_itself_and_its_free_cells_stay_free(handle, shape):
    nx, ny, frames = shape
    more = 0
    for fill in FILLS:
        count, block, target, seen, min_count, min_seen, calls, want = case(nx, ny, frames, fill, 0)
        for origins in calls[:3]:
            for max_range in (0, 7):
                first2, occ2 = handle.visibility_grid(count, origins[:, :2], min_count, max_range)
                first, shadow, occ = both_paths(handle, lambda: handle.viewshed_grid(count, origins, min_count=min_count, max_range=max_range))
                assert first.tobytes() == first2.tobytes() and occ.tobytes() == occ2.tobytes(), "fill %g origins %s" % (fill, origins.tolist())
                assert set(np.unique(shadow).tolist()) <= {vr.NO_HEIGHT, vr.INT32_MAX}
                _, _, occ_h = handle.viewshed_grid(count, origins, block, target, None, min_count, 1, max_range)  # any heights
                assert (occ_h[occ2 == ov.FREE] == vr.FREE).all() and np.array_equal(occ_h == vr.OCCUPIED, occ2 == ov.OCCUPIED)
                more += int(((occ_h == vr.FREE) & (occ2 != ov.FREE)).sum())
    assert more > 0 or nx * ny < 100


# ---- the kerb ---------------------------------------------------------------------------------------------------------------------
def test_the_kerb(handle):
    count, block, target, origin = vr.kerb_row()
    first, shadow, occ = both_paths(handle, lambda: handle.viewshed_grid(count, origin, block, target))
    assert np.nonzero((first[0] == 4) & (np.arange(40) != 4))[0].tolist() == list(range(5, 34))
    assert shadow[0, 10] == 1200 and shadow[0, 34] == 0 and (shadow[0, :5] == vr.NO_HEIGHT).all()
    assert (occ[0, 5:34] == vr.UNKNOWN).all() and (occ[0, 34:] == vr.FREE).all() and occ[0, 4] == vr.OCCUPIED and (occ[0, :4] == vr.FREE).all()
    assert (handle.visibility_grid(count, origin[:2])[1][0, 5:] == ov.UNKNOWN).all()  # the 2-D shadow runs to the edge
    check((first, shadow, occ), [a[0] for a in vr.viewshed_frames(count[None], origin, block[None], target[None])], "the kerb")


# ---- max_range --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(33, 31, 1), (65, 63, 1), (130, 129, 3)], ids=shape_ids)
def test_max_range_changes_nothing_inside_it_and_witnessed_cells_hold_beyond_it(handle, shape):
    nx, ny, frames = shape
    iy, ix = np.mgrid[0:ny, 0:nx]
    for fill in (0.05, 0.4):
        count, block, target, seen, min_count, min_seen, calls, want = case(nx, ny, frames, fill, 0)
        origins, unlimited = calls[-1], want[-1]
        per_frame = origins.repeat(frames, 0) if len(origins) == 1 else origins
        kw = dict(block=block, target=target, seen=seen, min_count=min_count, min_seen=min_seen)
        for max_range in (1, 7, 200):
            what = "%dx%dx%d fill %g max_range %d" % (nx, ny, frames, fill, max_range)
            got = both_paths(handle, lambda: handle.viewshed_grid(count, origins, max_range=max_range, **kw))
            dev = from_device(handle, count, origins, max_range=max_range, **kw)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, dev)), what
            check(got, vr.viewshed_frames(count, origins, block, target, seen, min_count, min_seen, max_range), what)
            witnessed = 0
            for f in range(frames):
                far = np.maximum(np.abs(ix - per_frame[f][0]), np.abs(iy - per_frame[f][1])) > max_range
                assert (got[0][f][far] == vr.BEYOND).all() and (got[1][f][far] == vr.NO_HEIGHT).all(), what
                for a, b in zip(got, unlimited):
                    assert np.array_equal(a[f][~far], b[f][~far]), what
                occupied, wit = count[f] >= min_count, seen[f] >= min_seen
                assert np.array_equal(got[2][f][far], np.where(occupied, vr.OCCUPIED, np.where(wit, vr.FREE, vr.UNKNOWN))[far]), what
                assert (got[2][f][occupied & wit] == vr.OCCUPIED).all()  # a witnessed cell under an occupied one stays occupied
                witnessed += int((far & wit & ~occupied).sum())
            assert witnessed > 0 or max_range >= max(nx, ny)


# ---- frames -----------------------------------------------------------------------------------------------------------------------
def test_a_batch_is_its_frames(handle):
    count, block, target, seen, min_count, min_seen, calls, want = case(130, 129, 3, 0.05, 0)
    origins = calls[0]
    got = handle.viewshed_grid(count, origins, block, target, seen, min_count, min_seen)
    check(got, want[0], "three frames")
    for f in range(3):
        one = handle.viewshed_grid(count[f], origins[f], block[f], target[f], seen[f], min_count, min_seen)
        assert all(a.tobytes() == b[f].tobytes() for a, b in zip(one, got)), "frame %d alone" % f
    # one origin for every frame = the same origin repeated
    a = handle.viewshed_grid(count, origins[1], block, target, seen, min_count, min_seen)
    b = handle.viewshed_grid(count, origins[1][None, :].repeat(3, 0), block, target, seen, min_count, min_seen)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert a[0][1].tobytes() == got[0][1].tobytes() and not np.array_equal(a[1][0], got[1][0])
    with pytest.raises(pwpp_hip.PwppError):
        handle.viewshed_grid(count, origins[:2], block, target)  # two origins for three frames
    with pytest.raises(pwpp_hip.PwppError):
        handle.viewshed_grid(count, [[0, 0, 5], [0, 0, vr.NO_HEIGHT], [0, 0, 5]], block, target)  # an eye without a height


# ---- the LDS limit ----------------------------------------------------------------------------------------------------------------
def lds_bytes():
    text = open(os.path.join(ROOT, "patchwork-plusplus_amd", "csrc", "pwpp_visibility.h")).read()
    a, b = re.search(r"#define PWPP_VIS_LDS_BYTES \((\d+) \* (\d+)\)", text).groups()
    return int(a) * int(b)


@pytest.mark.parametrize("side", ["fits", "first that does not"])
def test_either_side_of_the_lds_limit(handle, side):
    ny = 1024
    words = lds_bytes() // 4 // ny  # the most words a row may have for 1024 rows to fit
    nx = 32 * words if side == "fits" else 32 * words + 1
    assert ((nx + 31) // 32 * ny * 4 <= lds_bytes()) == (side == "fits") and ((nx + 32) // 32 * ny * 4 > lds_bytes())
    count = ov.random_count(nx, ny, 0.002, 1, 5)[None]  # sparse: most lines run for hundreds of cells
    block, target = vr.random_heights(count.shape, 1700, 8), vr.random_heights(count.shape, 1700, 9)
    origin = np.array([700, 300, 1700], np.int32)
    first, shadow, occ = both_paths(handle, lambda: handle.viewshed_grid(count, origin, block, target))  # path 0 against paths 1 and 2, the whole image
    rng = np.random.default_rng(11)
    cells = np.concatenate([np.stack([rng.integers(0, nx, 2048), rng.integers(0, ny, 2048)], 1),
                            np.stack([np.arange(nx), np.zeros(nx, int)], 1), np.stack([np.arange(nx), np.full(nx, ny - 1)], 1),
                            np.stack([np.zeros(ny, int), np.arange(ny)], 1), np.stack([np.full(ny, nx - 1), np.arange(ny)], 1)])
    wf, ws, _ = vr.viewshed_of(count[0], origin, block[0], target[0], cells=cells)
    gf, gs = first[0][cells[:, 1], cells[:, 0]], shadow[0][cells[:, 1], cells[:, 0]]
    assert np.array_equal(gf, wf), "%d of %d sampled cells differ from the brute force" % ((gf != wf).sum(), len(cells))
    assert np.array_equal(gs, ws)
    assert np.array_equal(occ[0][cells[:, 1], cells[:, 0]], vr.occupancy_of(count[0], wf, cells=cells))
    assert (wf == vr.NONE).sum() > 100 and (wf >= 0).sum() > 100 and ((ws != vr.NO_HEIGHT) & (wf == vr.NONE)).sum() > 100


# ---- the window of rows in LDS and the launch plan, which both operators share ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def window_case():
    """Three frames of 70 x 37 cells: a row of three words, the last ragged; a run of 256 cells spans four rows; eleven runs, the last
    ragged.  An origin in the first row, in the last and in the middle: the window of a run grows upward, downward and both ways."""
    nx, ny = 70, 37
    count = np.stack([ov.random_count(nx, ny, 0.05, 1, 4100 + f) for f in range(3)])
    origins = np.array([[12, 0, 1700], [55, ny - 1, -350], [35, ny // 2, 12000]], np.int32)
    block, target = vr.random_heights(count.shape, 1700, 4111), vr.random_heights(count.shape, 1700, 4112)
    want = {r: (ov.visibility_frames(count, origins[:, :2], 1, r), vr.viewshed_frames(count, origins, block, target, max_range=r)) for r in (0, 9)}
    for a in [count, origins, block, target] + [x for pair in want.values() for res in pair for x in res]:
        a.setflags(write=False)
    return count, origins, block, target, want


def test_the_shared_window_and_plan(handle):
    count, origins, block, target, want = window_case()
    try:
        for vis_path, view_path in ((0, 1), (1, 2)):
            handle.set_option("visibility_path", vis_path)
            handle.set_option("viewshed_path", view_path)
            for max_range in (0, 9):
                for mem in ("host", "device"):
                    what = "visibility_path %d, viewshed_path %d, max_range %d, %s memory" % (vis_path, view_path, max_range, mem)
                    if mem == "host":
                        two = handle.visibility_grid(count, origins[:, :2], 1, max_range)
                        three = handle.viewshed_grid(count, origins, block, target, max_range=max_range)
                        flat = handle.viewshed_grid(count, origins, max_range=max_range)
                    else:
                        two = vis_from_device(handle, count, origins[:, :2], 1, max_range)
                        three = from_device(handle, count, origins, block, target, max_range=max_range)
                        flat = from_device(handle, count, origins, max_range=max_range)
                    assert all(g.tobytes() == w.tobytes() for g, w in zip(two, want[max_range][0])), what + ": the visibility differs from the brute force"
                    check(three, want[max_range][1], what)
                    assert flat[0].tobytes() == two[0].tobytes() and flat[2].tobytes() == two[1].tobytes(), what + ": without heights it is not the visibility"
    finally:
        handle.set_option("visibility_path", 0)
        handle.set_option("viewshed_path", 0)


# ---- alignment --------------------------------------------------------------------------------------------------------------------
def test_device_images_one_word_and_one_byte_off_a_256_byte_boundary(handle):
    for nx, ny, frames in ((65, 63, 1), (130, 129, 3)):
        count, block, target, seen, min_count, min_seen, calls, want = case(nx, ny, frames, 0.05, 0)
        kw = dict(block=block, target=target, seen=seen, min_count=min_count, min_seen=min_seen)
        for max_range in (0, 7):
            aligned = from_device(handle, count, calls[0], max_range=max_range, **kw)
            shifted = both_paths(handle, lambda: from_device(handle, count, calls[0], max_range=max_range, shift_words=1, shift_bytes=1, **kw))
            assert all(a.tobytes() == b.tobytes() for a, b in zip(aligned, shifted))
            if max_range == 0:
                check(shifted, want[0], "%dx%dx%d shifted" % (nx, ny, frames))


# ---- pwpp_rasterize_ground_returns -------------------------------------------------------------------------------------------------
def returns_of(pts, idx, x0, y0, cell, nx, ny):
    """The cell rule of include/pwpp.h on the listed points, in double on the float coordinates."""
    p = pts[idx]
    u, v = (p[:, 0].astype(np.float64) - x0) / cell, (p[:, 1].astype(np.float64) - y0) / cell
    keep = (u >= 0) & (u < nx) & (v >= 0) & (v < ny)
    seen = np.zeros((ny, nx), np.int32)
    np.add.at(seen, (np.floor(v[keep]).astype(int), np.floor(u[keep]).astype(int)), 1)
    return seen


def test_ground_returns_against_numpy():
    frames = three_frames()
    h = pwpp_hip.Handle()
    L = pwpp_hip.load()
    g = pwpp_hip.GroundGrid(-16.0, -16.0, 0.5, 64, 64, 0, 0)
    buf = np.zeros(64 * 64, np.int32)
    assert L.pwpp_rasterize_ground_returns(h._h, ctypes.byref(g), 0, 1, pwpp_hip.MEM_HOST, buf.ctypes.data_as(ctypes.c_void_p)) == E_STATE
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    for grid in ((-16.0, -16.0, 0.5, 64, 64), (2.0, -7.0, 1.7, 33, 9), (-150.0, -150.0, 300.0, 1, 1)):
        seen = h.rasterize_ground_returns(*grid)
        assert seen.shape == (3, grid[4], grid[3]) and seen.dtype == np.int32
        for f in range(3):
            assert np.array_equal(seen[f], returns_of(frames[f], h.ground_indices(f), *grid)), "grid %s frame %d" % (grid, f)
        assert seen[0].sum() > 100 and seen[1].sum() == 0
        sub = h.rasterize_ground_returns(*grid, frame_first=1, frames=2)
        assert sub.tobytes() == seen[1:].tobytes()
    import torch
    nx = ny = 64
    dev = torch.full((3 * nx * ny + 128,), -7, dtype=torch.int32, device="cuda")
    h.rasterize_ground_returns_device(-16.0, -16.0, 0.5, nx, ny, dev.data_ptr() + 4)
    h.synchronize()
    raw = dev.cpu().numpy()
    assert raw[1:1 + 3 * nx * ny].tobytes() == h.rasterize_ground_returns(-16.0, -16.0, 0.5, nx, ny).tobytes() and raw[0] == -7 and (raw[1 + 3 * nx * ny:] == -7).all()
    assert L.pwpp_rasterize_ground_returns(h._h, ctypes.byref(g), 2, 2, pwpp_hip.MEM_HOST, buf.ctypes.data_as(ctypes.c_void_p)) == E_ARG
    assert b"outside the last call" in L.pwpp_last_error()


# ---- pwpp_viewshed_obstacles --------------------------------------------------------------------------------------------------------
def stages(h, x0, y0, cell, nx, ny, ground_only=False, frame_first=0, frames=None):
    """(count, block, target, seen) of the chained call from its rasters, quantised in numpy."""
    count, top = h.rasterize_obstacles(x0, y0, cell, nx, ny, *BAND, frame_first=frame_first, frames=frames, ground_only=ground_only)
    ground = h.rasterize_ground(x0, y0, cell, nx, ny, frame_first=frame_first, frames=frames, ground_only=ground_only)
    seen = h.rasterize_ground_returns(x0, y0, cell, nx, ny, frame_first=frame_first, frames=frames)
    return count, vr.units_image(ground.astype(np.float64) + top.astype(np.float64)), vr.units_image(ground.astype(np.float64)), seen


@pytest.mark.parametrize("grid", [(256, 256, 0.5), (64, 64, 2.0)], ids=["256x256", "64x64"])
def test_viewshed_obstacles_is_its_four_stages_and_sees_more_than_the_2d_operator(kitti, grid):
    nx, ny, cell = grid
    x0, y0 = -0.5 * nx * cell, -0.5 * ny * cell
    L = pwpp_hip.load()
    h = pwpp_hip.Handle()
    g = pwpp_hip.GroundGrid(x0, y0, cell, nx, ny, 0, 0)
    first_buf, zero = np.zeros(nx * ny, np.int32), np.zeros(3, np.float64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.pwpp_viewshed_obstacles(h._h, ctypes.byref(g), BAND[0], BAND[1], 1, 1, vp(zero), 1, 0, 0, 1, pwpp_hip.MEM_HOST, vp(first_buf), None, None, None) == E_STATE
    h.set_labels(True)  # (_everything reads them)
    h.estimate_ground(kitti[0])
    before = _everything(h, 1)
    rc, block, target, seen = stages(h, x0, y0, cell, nx, ny)
    assert (rc > 0).sum() > 100 and (seen > 0).sum() > 100 and (block != vr.NO_HEIGHT).sum() > 100
    eye_z = 0.0  # the sensor is the origin of the model's frame; the ground lies near -sensor_height
    o_cell = (nx // 2, ny // 2, vr.units(eye_z))
    occ = None
    for min_count, min_seen, max_range in ((1, 1, 0), (2, 0, 0), (1, 3, 40)):
        what = "%d x %d, min_count %d, min_seen %d, max_range %d" % (nx, ny, min_count, min_seen, max_range)
        first, shadow, occ, count = both_paths(h, lambda: h.viewshed_obstacles(x0, y0, cell, nx, ny, *BAND, (0.0, 0.0, eye_z), min_count, min_seen, max_range,
                                                                              want_count=True))
        assert count.tobytes() == rc.tobytes(), what + ": the count image differs from pwpp_rasterize_obstacles"
        got = h.viewshed_grid(rc, o_cell, block, target, seen if min_seen else None, min_count, max(min_seen, 1), max_range)
        assert all(a.tobytes() == b.tobytes() for a, b in zip((first, shadow, occ), got)), what + ": differs from pwpp_viewshed_grid on the stages"
        kept = h.viewshed_obstacles(x0, y0, cell, nx, ny, *BAND, (0.0, 0.0, eye_z), min_count, min_seen, max_range)  # the count image kept in the handle
        assert all(a.tobytes() == b.tobytes() for a, b in zip(kept, (first, shadow, occ))), what
        check((first, shadow, occ), vr.viewshed_frames(rc, o_cell, block, target, seen if min_seen else None, min_count, max(min_seen, 1), max_range), what)
        # the point of the feature: the FREE set contains that of pwpp_visibility_obstacles (a theorem) and is strictly larger (measured here)
        occ2 = h.visibility_obstacles(x0, y0, cell, nx, ny, *BAND, (0.0, 0.0), min_count, max_range)[1]
        free, free2 = occ == vr.FREE, occ2 == ov.FREE
        print("%s: FREE %d of %d cells, 2-D %d; unknown %d, 2-D %d" % (what, free.sum(), free.size, free2.sum(), (occ == vr.UNKNOWN).sum(), (occ2 == ov.UNKNOWN).sum()))
        assert free[free2].all(), what + ": a cell the 2-D operator calls free is not free"
        assert free.sum() > free2.sum(), what + ": the viewshed's FREE set is not strictly larger than the 2-D operator's"
        assert np.array_equal(occ == vr.OCCUPIED, occ2 == ov.OCCUPIED)
    assert (occ == vr.FREE).sum() > 100 and (occ == vr.UNKNOWN).sum() > 100 and (occ == vr.OCCUPIED).sum() > 100
    # ground_only blanks patches in both rasters; an origin by the cell rule with its own height
    rc_g, block_g, target_g, seen_g = stages(h, x0, y0, cell, nx, ny, ground_only=True)
    off = h.viewshed_obstacles(x0, y0, cell, nx, ny, *BAND, (3.2, -7.9, 0.4), ground_only=True)
    goff = h.viewshed_grid(rc_g, (int(np.floor((3.2 - x0) / cell)), int(np.floor((-7.9 - y0) / cell)), vr.units(0.4)), block_g, target_g, seen_g)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(off, goff))
    for xyz in ((-x0, 0.0, 0.0), (0.0, y0 - 1e-9, 0.0), (np.nan, 0.0, 0.0), (0.0, 0.0, np.nan)):
        assert L.pwpp_viewshed_obstacles(h._h, ctypes.byref(g), BAND[0], BAND[1], 1, 1, vp(np.array(xyz, np.float64)), 1, 0, 0, 1, pwpp_hip.MEM_HOST,
                                         vp(first_buf), None, None, None) == E_ARG, xyz
        assert b"origin 0" in L.pwpp_last_error()
    # into device memory, the images one word / one byte off a 256-byte boundary
    import torch
    bufs = [torch.full((nx * ny + 128,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    docc = torch.full((nx * ny + 512,), -7, dtype=torch.int8, device="cuda")
    h.viewshed_obstacles_device(x0, y0, cell, nx, ny, *BAND, (0.0, 0.0, eye_z), 1, 3, 40, bufs[0].data_ptr() + 4, bufs[1].data_ptr() + 4, docc.data_ptr() + 1,
                                bufs[2].data_ptr() + 4)
    h.synchronize()
    raw = [b.cpu().numpy() for b in bufs] + [docc.cpu().numpy()]
    for r, want in zip(raw, (first, shadow, rc, occ)):
        assert r[1:1 + nx * ny].tobytes() == want.tobytes() and (r[:1] == -7).all() and (r[1 + nx * ny:] == -7).all()
    assert _everything(h, 1) == before, "the viewshed changed the results of the call it reads"


def test_three_frames_with_an_origin_each():
    frames = three_frames()  # a 16-beam scan, an empty frame, a frame that is all unref
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    grid = (-16.0, -16.0, 0.5, 64, 64)
    xyz = np.array([[0.0, 0.0, 0.0], [3.3, -2.1, 0.5], [-15.9, 15.9, -1.0]])
    cells = np.concatenate([np.floor((xyz[:, :2] + 16.0) / 0.5), [[vr.units(z)] for z in xyz[:, 2]]], 1).astype(np.int32)
    rc, block, target, seen = stages(h, *grid)
    got = both_paths(h, lambda: h.viewshed_obstacles(*grid, *BAND, xyz))
    check(got, vr.viewshed_frames(rc, cells, block, target, seen), "three frames")
    assert (got[2][1] == vr.FREE).all() and (got[0][0] >= 0).sum() >= 3  # the empty frame holds no obstacle: all seen
    sub = h.viewshed_obstacles(*grid, *BAND, xyz[1:], frame_first=1, frames=2)  # entry i belongs to frame frame_first + i
    assert all(a.tobytes() == b[1:].tobytes() for a, b in zip(sub, got))


# ---- workspace ----------------------------------------------------------------------------------------------------------------------
def test_workspace_and_that_nothing_else_moves():
    h = pwpp_hip.Handle()
    empty = h.workspace_bytes()
    count, block, target, seen, min_count, min_seen, calls, want = case(65, 63, 1, 0.05, 0)
    h.set_option("viewshed_path", 2)
    check(h.viewshed_grid(count, calls[0], block, target, seen, min_count, min_seen), want[0], "before any estimate call")
    grown = h.workspace_bytes()
    # the bit image (3 words a row), the staged count, block, target, seen, first and shadow images and the byte image in words
    assert grown >= empty + 4 * (3 * 63 + 6 * 65 * 63 + (65 * 63 + 3) // 4), "the cluster buffer is not counted by pwpp_get_workspace_bytes"
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
    b.viewshed_obstacles(-20.0, -20.0, 0.5, 80, 80, *BAND, np.zeros((3, 3)))
    b.rasterize_ground_returns(-20.0, -20.0, 0.5, 80, 80)
    assert b.workspace_bytes() >= a.workspace_bytes() + 4 * (9 + 6 * 3 * 80 * 80)  # three origins; the kept count, top, ground, block, target and seen images
    assert _everything(b, 3) == before and b.time_us() == t_before, "the viewshed changed the results of the call it reads"
    for w in (a, b):
        w.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert _everything(b, 3) == _everything(a, 3), "an estimate call after a viewshed call differs from one without"
    b.trim_workspace()
    a.trim_workspace()
    assert a.workspace_bytes() == b.workspace_bytes()
    with pytest.raises(pwpp_hip.PwppError):
        h.set_option("viewshed_path", 3)


def test_pybind_module_agrees_with_the_ctypes_handle():
    import pypatchworkpp
    pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    h = pwpp_hip.Handle()
    with pytest.raises(RuntimeError):
        pp.getObstacleViewshed(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5)  # no frame yet
    pts = small_cloud(5)
    pp.estimateGround(pts)
    h.estimate_ground(pts)
    for min_count, min_seen, max_range, origin, ground_only in ((1, 1, 0, (0.0, 0.0, 0.0), False), (2, 0, 30, (2.2, -1.1, 0.3), True)):
        first, shadow, occ = pp.getObstacleViewshed(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5, min_count, min_seen, max_range, origin[0], origin[1], origin[2], ground_only)
        hf, hs, ho = h.viewshed_obstacles(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5, origin, min_count, min_seen, max_range, ground_only=ground_only)
        assert first.dtype == shadow.dtype == np.int32 and occ.dtype == np.int8 and first.shape == shadow.shape == occ.shape == (48, 120)
        assert (occ == vr.OCCUPIED).sum() >= 3
        assert first.tobytes() == hf[0].tobytes() and shadow.tobytes() == hs[0].tobytes() and occ.tobytes() == ho[0].tobytes()
    with pytest.raises(RuntimeError):
        pp.getObstacleViewshed(0.0, 0.0, 1.0, 4, 4, 0.2, 2.5, 1, 1, 0, 9.0, 0.0, 0.0)  # the origin outside the grid
