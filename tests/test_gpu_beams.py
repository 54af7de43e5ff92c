"""The per-beam free space (pwpp_rasterize_beams, pwpp_beam_grid, pwpp_beam_ground) on a real MI355X, byte for byte against the brute
force of tests/beams_ref.py, on both values of the option "beams_path" and from host and from device memory -- the device images at
4-byte alignment and no more, the bytes at an odd address, the words and bytes around them poisoned.  The shapes are the smallest at
which the kernels can still go wrong: a row and a column; 33 x 31 with the origin in each corner, on each edge and in the middle (all
eight octants, the exact diagonals); 130 x 67 and 67 x 130 in three frames with an origin each -- path 2's tile is 64 x 64 cells:
more than one tile each way, sides that are no multiple of it, origins in another tile than the endpoints, a line that leaves a tile
through its corner, empty tiles; a frame without an endpoint and one where every cell is one; two beams over the same cells; hits
without a height; eyes at +-2^30 with heights at the int32 extremes; the byte rule on every combination, and a target without a
height under the widest clearance; a sum that wraps past 2^32; max_range; the update in place; the
two theorems about the bytes; the raster and the chained call on synthetic frames against the index lists and against every point's
own beam; PWPP_E_STATE; the workspace."""
import ctypes
import functools

import numpy as np
import pytest

import beams_ref as br
import pwpp_hip
from test_gpu_obstacle_grid import small_cloud, three_frames

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
PATHS = (1, 2)
NAMES = ("passes", "low", "occupancy")


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()  # (no estimate call: pwpp_beam_grid needs the handle's stream and buffer only)


def from_device(h, hits, zmin, origins, target=None, occupancy_in=None, max_range=0, min_pass=1, clearance=0, shift_words=1, shift_bytes=3, in_place=False):
    """beam_grid on device images; the int32 images start shift_words words, the byte images shift_bytes bytes behind a 256-byte
    boundary; the words and bytes around them are poisoned and must survive, and the inputs must come back unwritten.  in_place:
    occupancy is occupancy_in itself."""
    import torch
    frames, ny, nx = hits.shape
    cells = hits.size
    ins = [hits, zmin, target]
    bufs = [torch.full((cells + 128,), -7, dtype=torch.int32, device="cuda") for _ in range(5)]  # hits, zmin, target, passes, low
    bytes_ = [torch.full((cells + 512,), -7, dtype=torch.int8, device="cuda") for _ in range(2)]  # occupancy_in, occupancy
    assert all(b.data_ptr() % 256 == 0 for b in bufs + bytes_)
    for b, a in zip(bufs, ins):
        if a is not None:
            b[shift_words:shift_words + cells] = torch.from_numpy(a.reshape(-1).copy()).cuda()
    if occupancy_in is not None:
        bytes_[0][shift_bytes:shift_bytes + cells] = torch.from_numpy(occupancy_in.reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    ptr = lambda k, present=True: bufs[k].data_ptr() + 4 * shift_words if present else 0
    out = bytes_[0] if in_place else bytes_[1]
    h.beam_grid_device(nx, ny, frames, ptr(0), ptr(1), origins, max_range, min_pass, clearance, ptr(3), ptr(4), out.data_ptr() + shift_bytes,
                       ptr(2, target is not None), bytes_[0].data_ptr() + shift_bytes if occupancy_in is not None else 0)
    h.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
    raw = [b.cpu().numpy() for b in bufs]
    rawb = [b.cpu().numpy() for b in bytes_]
    for r in raw:
        assert (r[:shift_words] == -7).all() and (r[shift_words + cells:] == -7).all(), "a word outside an image was written"
    for r in rawb:
        assert (r[:shift_bytes] == -7).all() and (r[shift_bytes + cells:] == -7).all(), "a byte outside an image was written"
    for k, a in enumerate(ins):
        body = raw[k][shift_words:shift_words + cells]
        assert np.array_equal(body, a.reshape(-1)) if a is not None else (body == -7).all(), "an input image was written"
    if not in_place:
        body = rawb[0][shift_bytes:shift_bytes + cells]
        assert np.array_equal(body, occupancy_in.reshape(-1)) if occupancy_in is not None else (body == -7).all(), "the base bytes were written"
    cut = lambda r, s: r[s:s + cells].reshape(hits.shape)
    return cut(raw[3], shift_words).view(np.uint32), cut(raw[4], shift_words), cut(rawb[0 if in_place else 1], shift_bytes)


def both_paths(h, call):
    """call() at "beams_path" 0, 1 and 2: identical bytes; returns them."""
    res = []
    for path in (0,) + PATHS:
        h.set_option("beams_path", path)
        res.append(call())
    h.set_option("beams_path", 0)
    for r in res[1:]:
        for a, b, name in zip(res[0], r, NAMES):
            assert a.tobytes() == b.tobytes(), "%s differs between two values of beams_path in %d cells" % (name, (a != b).sum())
    return res[0]


def check(got, want, what):
    for g, w, name, dt in zip(got, want, NAMES, (np.uint32, np.int32, np.int8)):
        assert g.dtype == dt and g.shape == w.shape, what
        assert np.array_equal(g, w), "%s: %s differs from the brute force in %d cells" % (what, name, (g != w).sum())


def everywhere(h, hits, zmin, origins, what, **kw):
    """The call from host and from device memory on every path against the brute force; returns the brute force."""
    want = br.beams_frames(hits, zmin, origins, **kw)
    check(both_paths(h, lambda: h.beam_grid(hits, zmin, origins, **kw)), want, what + ", host memory")
    check(both_paths(h, lambda: from_device(h, hits, zmin, origins, **kw)), want, what + ", device memory")
    return want


def random_bytes(shape, seed):
    """Base bytes: free, occupied, unknown (twice as often) and one foreign value."""
    return np.random.default_rng(seed).choice(np.array([br.FREE, br.OCCUPIED, br.UNKNOWN, br.UNKNOWN, 42], np.int8), shape)


def random_target(shape, eye, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < 0.1, br.NO_HEIGHT, eye - 1700 + rng.integers(-300, 301, shape)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def scene(nx, ny, frames, fill, seed):
    """(hits, zmin, target, base) of a shape: computed once, shared, never written."""
    shape = (frames, ny, nx)
    hits, zmin = br.random_ends(shape, 1700, seed, fill)
    out = hits, zmin, random_target(shape, 1700, seed + 1), random_bytes(shape, seed + 2)
    for a in out:
        a.setflags(write=False)
    return out


def origin_kinds(nx, ny):
    """The corners, the middle of each edge and the middle, without repeats."""
    xs, ys = (0, nx // 2, nx - 1), (0, ny // 2, ny - 1)
    return list(dict.fromkeys((x, y) for y in ys for x in xs))


# ---- small shapes, the whole image -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 40), (40, 1), (33, 31)], ids=lambda s: "%dx%d" % s)
def test_small_shapes_against_the_brute_force(handle, shape):
    nx, ny = shape
    crossed = cleared = 0
    for i, (ox, oy) in enumerate(origin_kinds(nx, ny)):
        hits, zmin, target, base = scene(nx, ny, 1, (0.3, 0.05, 1.0)[i % 3], 100 + i)
        eye = (1700, -350, 12000)[i % 3]
        kw = dict(target=target, occupancy_in=base, min_pass=1 + i % 3, clearance=(0, 500, 40000)[i % 3])
        want = everywhere(handle, hits, zmin, (ox, oy, eye), "%dx%d origin (%d, %d)" % (nx, ny, ox, oy), **kw)
        crossed += int((want[0] > 0).sum())
        cleared += int(((want[2] == br.FREE) & (base == br.UNKNOWN)).sum())
    assert crossed > 20 and cleared > 0
    # without a target, without base bytes: every crossed cell with enough beams is free
    hits, zmin, _, _ = scene(nx, ny, 1, 0.3, 100)
    want = everywhere(handle, hits, zmin, (nx // 2, ny // 2, 1700), "%dx%d bare" % shape, min_pass=2)
    assert np.array_equal(want[2] == br.FREE, want[0] >= 2)


# ---- more than one tile each way -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(130, 67), (67, 130)], ids=lambda s: "%dx%d" % s)
def test_tiles(handle, shape):
    nx, ny = shape
    hits, zmin, target, base = (a.copy() for a in scene(nx, ny, 3, 0.3, 7 * nx + ny))
    # frame 1: endpoints in the last tile alone, seen from the far corner -- empty tiles, an origin in another tile than every endpoint
    far = np.zeros((ny, nx), bool)
    far[ny - 3:, nx - 2:] = True
    hits[1] = np.where(far, 2, 0)
    zmin[1] = np.where(far, 900, br.NO_HEIGHT)
    # frame 2: sparse, and the exact diagonal from (0, 0) through the tiles' common corner (63, 63) -> (64, 64)
    hits[2] = np.where(np.random.default_rng(5).random((ny, nx)) < 0.01, 1, 0)
    hits[2, 66, 66], zmin[2, 66, 66] = 4, -200
    origins = np.array([(nx // 2, ny // 2, 1700), (0, 0, 1700), (0, 0, -350)], np.int32)
    want = everywhere(handle, hits, zmin, origins, "%dx%dx3" % shape, target=target, occupancy_in=base, min_pass=2, clearance=700)
    assert (want[0][2, np.arange(1, 66), np.arange(1, 66)] >= 4).all()                    # the diagonal's cells
    tiles_hit = {(y // 64, x // 64) for y, x in zip(*np.nonzero(want[0][1]))}
    assert len(tiles_hit) >= 3 and (want[0][1] > 0).sum() > 100                              # beams from the far tile cross the others
    # one origin for all three frames, another path through the launcher
    everywhere(handle, hits, zmin, (nx - 1, 0, 1700), "%dx%dx3, one origin" % shape, min_pass=1)


def test_a_frame_without_an_endpoint_and_one_where_every_cell_is_one(handle):
    nx, ny = 67, 70
    hits, zmin, target, base = (a.copy() for a in scene(nx, ny, 3, 0.3, 11))
    hits[0] = 0
    hits[1] = np.random.default_rng(2).integers(1, 4, (ny, nx))
    zmin[1] = np.where(zmin[1] == br.NO_HEIGHT, 0, zmin[1])
    origins = np.array([(5, 5, 1700), (33, 35, 1700), (66, 0, 1700)], np.int32)
    want = everywhere(handle, hits, zmin, origins, "none, all, some", target=target, occupancy_in=base, clearance=3000)
    assert (want[0][0] == 0).all() and (want[1][0] == br.NO_HEIGHT).all() and np.array_equal(want[2][0], base[0])
    near = want[0][1][34:37, 32:35].astype(np.int64)
    assert near[1, 1] == 0 and near.sum() == hits[1].sum() - hits[1][34:37, 32:35].sum()  # every beam longer than a step crosses exactly one neighbour of the origin, none the origin's cell


# ---- single facts of the contract ---------------------------------------------------------------------------------------------------
def row(length=40):
    return np.zeros((1, 1, length), np.int32), np.full((1, 1, length), br.NO_HEIGHT, np.int32)


def test_the_worked_row(handle):
    hits, zmin = row()
    hits[0, 0, 34], zmin[0, 0, 34] = 3, 0
    want = everywhere(handle, hits, zmin, (0, 0, 1700), "the worked row")
    assert (want[0][0, 0, 1:34] == 3).all() and want[0][0, 0, 0] == 0 and (want[0][0, 0, 34:] == 0).all()
    assert want[1][0, 0, [1, 10, 17, 33]].tolist() == [1675, 1225, 875, 75]
    zmin[0, 0, 34] = 2380
    want = everywhere(handle, hits, zmin, (0, 0, 1700), "the worked row, rising")
    assert want[1][0, 0, [1, 17, 33]].tolist() == [1730, 2050, 2370]


def test_the_lower_of_two_beams_over_the_same_cells_wins(handle):
    hits, zmin = row()
    hits[0, 0, 20], zmin[0, 0, 20] = 1, 3000   # rising
    hits[0, 0, 35], zmin[0, 0, 35] = 2, 0      # falling: lower at every shared cell
    want = everywhere(handle, hits, zmin, (0, 0, 1700), "two beams")
    alone = br.beams_frames(hits * (np.arange(40) == 35), zmin, (0, 0, 1700))
    assert (want[0][0, 0, 1:20] == 3).all() and (want[0][0, 0, 20:35] == 2).all()
    assert np.array_equal(want[1][0, 0, 1:35], alone[1][0, 0, 1:35])


def test_hits_without_a_height_are_no_endpoint(handle):
    hits, zmin = row()
    hits[0, 0, 30], hits[0, 0, 12], zmin[0, 0, 5] = 4, -2, 100   # hits without a height, negative hits with none, a height without hits
    want = everywhere(handle, hits, zmin, (0, 0, 1700), "no endpoint")
    assert (want[0] == 0).all() and (want[1] == br.NO_HEIGHT).all() and (want[2] == br.UNKNOWN).all()


@pytest.mark.parametrize("eye", [2 ** 30, -2 ** 30])
def test_an_eye_at_the_limit_with_heights_at_the_int32_extremes(handle, eye):
    hits, zmin = np.zeros((1, 9, 21), np.int32), np.full((1, 9, 21), br.NO_HEIGHT, np.int32)
    hits[0, 0, 20], zmin[0, 0, 20] = 1, br.INT32_MAX
    hits[0, 8, 20], zmin[0, 8, 20] = 1, br.NO_HEIGHT + 1
    hits[0, 8, 0], zmin[0, 8, 0] = 1, eye
    want = everywhere(handle, hits, zmin, (0, 4, eye), "eye %d" % eye, target=np.full((1, 9, 21), eye, np.int32), clearance=2 ** 31 - 1)
    low = want[1][want[0] > 0].astype(np.int64)
    assert low.min() >= eye - br.R and low.max() <= eye + br.R and (low.max() - eye > br.R // 2 or low.min() - eye < -br.R // 2)
    L = pwpp_hip.load()
    bad = np.array([0, 4, eye + (1 if eye > 0 else -1)], np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros(hits.size, np.int32)
    assert L.pwpp_beam_grid(handle._h, 21, 9, 1, pwpp_hip.MEM_HOST, p(hits), p(zmin), None, None, p(bad), 1, 0, 1, 0, p(out), p(out.copy()), None) == E_ARG
    assert b"origin 0" in L.pwpp_last_error() and b"eye" in L.pwpp_last_error()


def test_a_target_without_a_height_stays_unknown_under_any_clearance(handle):
    """low far below zero and the widest clearance: low - INT32_MIN <= clearance, so only the clause that asks the target for a
    height keeps a cell without one from being called free."""
    eye = -2 ** 30
    hits, zmin = row()
    hits[0, 0, 39], zmin[0, 0, 39] = 2, br.NO_HEIGHT + 1          # the rise clamps at -R: low runs from eye down to eye - R
    target = np.full((1, 1, 40), br.NO_HEIGHT, np.int32)
    target[0, 0, 1::2] = br.INT32_MAX                              # every other cell has a ground, far above the beam
    base = np.full((1, 1, 40), br.UNKNOWN, np.int8)
    base[0, 0, 5], base[0, 0, 6] = br.OCCUPIED, 42
    want = everywhere(handle, hits, zmin, (0, 0, eye), "no height, wide clearance", target=target, occupancy_in=base, clearance=br.INT32_MAX)
    low = want[1][0, 0, 1:39].astype(np.int64)
    assert (low - br.NO_HEIGHT <= br.INT32_MAX).all() and low.min() < eye - br.R // 2
    expect = np.where(np.arange(40) % 2 == 1, br.FREE, br.UNKNOWN).astype(np.int8)
    expect[[0, 39]], expect[5], expect[6] = br.UNKNOWN, br.OCCUPIED, 42
    assert want[2][0, 0].tolist() == expect.tolist()


def test_the_byte_rule_on_every_combination(handle):
    """Base byte x passes against min_pass x target (none, at, below and above low - clearance; then no target image): four frames
    of one row, crossed by 1, 2, 3 and 4 passes (min_pass 3 splits them), the base byte cycling with x, the target's kind with x // 4."""
    hits, zmin = np.zeros((4, 1, 40), np.int32), np.full((4, 1, 40), br.NO_HEIGHT, np.int32)
    hits[:, 0, 39], zmin[:, 0, 39] = [1, 2, 3, 4], 0
    lows = br.beams_frames(hits, zmin, (0, 0, 1700))[1].astype(np.int64)
    base = np.broadcast_to(np.array([br.FREE, br.OCCUPIED, br.UNKNOWN, 42], np.int8)[np.arange(40) % 4], (4, 1, 40)).copy()
    kind = (np.arange(40) // 4) % 4                                  # no height, at, below, above
    target = np.where((kind == 0) | (lows == br.NO_HEIGHT), br.NO_HEIGHT, lows - 300 + np.array([0, 0, -1, 1])[kind]).astype(np.int32)
    want = everywhere(handle, hits, zmin, (0, 0, 1700), "the matrix", target=target, occupancy_in=base, min_pass=3, clearance=300)
    crossed = (np.arange(40) >= 1) & (np.arange(40) <= 38)
    for f in range(4):
        free = crossed & (base[f, 0] == br.UNKNOWN) & (f + 1 >= 3) & ((kind == 1) | (kind == 3))
        assert np.array_equal(want[2][f, 0], np.where(free, br.FREE, base[f, 0])), f
    assert (want[2][2:] == br.FREE).sum() > (base[2:] == br.FREE).sum() and np.array_equal(want[2][:2], base[:2])
    bare = everywhere(handle, hits, zmin, (0, 0, 1700), "the matrix without a target", occupancy_in=base, min_pass=3, clearance=300)
    assert np.array_equal(bare[2][3, 0], np.where(crossed & (base[3, 0] == br.UNKNOWN), br.FREE, base[3, 0]))


def test_a_sum_that_wraps_past_2_to_the_32(handle):
    hits, zmin = row(12)
    hits[0, 0, 9:12], zmin[0, 0, 9:12] = br.INT32_MAX, 100
    want = everywhere(handle, hits, zmin, (0, 0, 0), "wrap", min_pass=2 ** 31 - 1)
    assert want[0][0, 0, 1] == (3 * br.INT32_MAX) % 2 ** 32 == 2 ** 31 - 3 and want[0][0, 0, 9] == 2 * br.INT32_MAX and want[0][0, 0, 10] == br.INT32_MAX
    assert want[2][0, 0].tolist() == [br.UNKNOWN] + [br.UNKNOWN] * 8 + [br.FREE, br.FREE, br.UNKNOWN]   # compared unsigned: 2^32 - 2 and 2^31 - 1 reach min_pass, 2^31 - 3 does not


@pytest.mark.parametrize("max_range", [1, 5, 40])
def test_max_range_changes_nothing_inside_it(handle, max_range):
    nx, ny = 70, 45
    hits, zmin, target, base = scene(nx, ny, 2, 0.3, 77)
    origins = np.array([(3, 40, 1700), (69, 2, -350)], np.int32)   # (cells beyond 40 in both frames)
    kw = dict(target=target, occupancy_in=base, min_pass=2, clearance=900)
    unlimited = br.beams_frames(hits, zmin, origins, **kw)
    got = everywhere(handle, hits, zmin, origins, "max_range %d" % max_range, max_range=max_range, **kw)
    yy, xx = np.mgrid[0:ny, 0:nx]
    for f, (ox, oy, _) in enumerate(origins):
        inside = np.maximum(np.abs(xx - ox), np.abs(yy - oy)) <= max_range
        for g, u in zip(got, unlimited):
            assert np.array_equal(g[f][inside], u[f][inside])
        assert (got[0][f][~inside] == 0).all() and (got[1][f][~inside] == br.NO_HEIGHT).all() and np.array_equal(got[2][f][~inside], base[f][~inside])
        assert (unlimited[0][f][~inside] > 0).any()


def test_the_update_in_place(handle):
    hits, zmin, target, base = scene(70, 45, 2, 0.3, 77)
    origins = np.array([(3, 40, 1700), (35, 22, -350)], np.int32)
    kw = dict(target=target, occupancy_in=base, min_pass=1, clearance=900)
    want = br.beams_frames(hits, zmin, origins, **kw)
    check(both_paths(handle, lambda: from_device(handle, hits, zmin, origins, in_place=True, **kw)), want, "in place, device memory")
    L = pwpp_hip.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for path in PATHS:
        handle.set_option("beams_path", path)
        occ, passes, low = base.copy(), np.zeros(hits.shape, np.uint32), np.zeros(hits.shape, np.int32)
        assert L.pwpp_beam_grid(handle._h, 70, 45, 2, pwpp_hip.MEM_HOST, p(hits), p(zmin), p(target), p(occ), p(origins), 2, 0, 1, 900, p(passes), p(low), p(occ)) == 0
        check((passes, low, occ), want, "in place, host memory")
    handle.set_option("beams_path", 0)
    # any other overlap is an error, and so is an int32 image off its alignment in device memory
    occ, passes, low = base.copy(), np.zeros(hits.size + 1, np.int32), np.zeros(hits.shape, np.int32)
    assert L.pwpp_beam_grid(handle._h, 70, 45, 2, pwpp_hip.MEM_HOST, p(hits), p(zmin), None, p(occ), p(origins), 2, 0, 1, 0, p(passes), p(passes[1:]), None) == E_ARG
    assert b"overlap" in L.pwpp_last_error()
    assert L.pwpp_beam_grid(handle._h, 70, 45, 2, pwpp_hip.MEM_HOST, p(hits), p(zmin), None, p(occ), p(origins), 2, 0, 1, 0, p(passes), p(low), p(occ[0, 0, 1:])) == E_ARG
    assert b"without being equal" in L.pwpp_last_error()
    import torch
    d = torch.zeros(4 * hits.size + 64, dtype=torch.int32, device="cuda")
    a = d.data_ptr()
    n = 4 * hits.size
    with pytest.raises(pwpp_hip.PwppError, match="4-byte aligned"):
        handle.beam_grid_device(70, 45, 2, a, a + n, origins, 0, 1, 0, a + 2 * n + 2, a + 3 * n + 8)


def test_the_two_theorems_about_the_bytes(handle):
    for seed in range(4):
        hits, zmin, target, _ = scene(33, 31, 1, 0.3, 100 + seed)
        base = random_bytes(hits.shape, 900 + seed)
        for tg in (None, target):
            occ = both_paths(handle, lambda: handle.beam_grid(hits, zmin, (16, 15, 1700), target=tg, occupancy_in=base, clearance=600))[2]
            assert (occ[base == br.FREE] == br.FREE).all(), "a free cell of the input is not free in the output"
            changed = occ != base
            assert (base[changed] == br.UNKNOWN).all() and (occ[changed] == br.FREE).all() and changed.any()
            assert np.array_equal(occ[base != br.UNKNOWN], base[base != br.UNKNOWN])


# ---- the raster and the chain ----------------------------------------------------------------------------------------------------------
GRID = (-24.0, -20.0, 1.0, 48, 40)
ORIGIN = (0.0, 0.0, 0.0)


def selected(h, cloud, f, which):
    """The rows of frame f's cloud the selected index lists name."""
    idx = np.concatenate(([h.ground_indices(f)] if which & br.GROUND else []) + ([h.nonground_indices(f)] if which & br.NONGROUND else []))
    return cloud[idx.astype(np.int64)] if len(cloud) else cloud


def with_nans(cloud, seed):
    """A few z of NaN among the points: skipped and not counted."""
    c = cloud.copy()
    c[np.random.default_rng(seed).choice(len(c), 25, replace=False), 2] = np.nan
    return c


def check_chain(h, clouds, what):
    """rasterize_beams against the index lists, beam_ground against its three stages and against every point's own beam."""
    x0, y0, cell, nx, ny = GRID
    org = np.array([[ORIGIN[0] + 0.25 * f, ORIGIN[1] - 0.5 * f, ORIGIN[2] + 0.1 * f] for f in range(len(clouds))])
    cells = [(int((o[0] - x0) // cell), int((o[1] - y0) // cell), br.units(o[2])) for o in org]
    ground = h.rasterize_ground(*GRID)
    target = br.units_image(ground.astype(np.float64))
    base = random_bytes(target.shape, 5)
    for which in (br.GROUND, br.NONGROUND, br.GROUND | br.NONGROUND):
        hits, zmin = h.rasterize_beams(*GRID, which=which)
        assert hits.dtype == zmin.dtype == np.int32 and hits.shape == (len(clouds), ny, nx)
        for f, c in enumerate(clouds):
            want = br.ends_of_points(selected(h, c, f, which), GRID)
            assert np.array_equal(hits[f], want[0]) and np.array_equal(zmin[f], want[1]), "%s: which %d frame %d" % (what, which, f)
        assert hits[0].sum() > 100
        for max_range, min_pass in ((0, 1), (9, 2)):
            kw = dict(max_range=max_range, min_pass=min_pass)
            got = both_paths(h, lambda: h.beam_ground(*GRID, origin_xyz=org, which=which, occupancy_in=base, clearance=0.3, want_ends=True, **kw))
            assert got[3].tobytes() == hits.tobytes() and got[4].tobytes() == zmin.tobytes()
            stages = h.beam_grid(hits, zmin, np.array(cells, np.int32), target=target, occupancy_in=base, clearance=br.units(0.3), **kw)
            check(got[:3], stages, "%s: which %d, the chain against its stages" % (what, which))
            check(got[:3], br.beams_frames(hits, zmin, cells, target, base, max_range, min_pass, br.units(0.3)), "%s: which %d, the chain" % (what, which))
            for f, c in enumerate(clouds):
                per_point = br.beams_of_points(selected(h, c, f, which), GRID, cells[f], max_range)
                assert np.array_equal(got[0][f], per_point[0]) and np.array_equal(got[1][f], per_point[1]), "%s: which %d frame %d per point" % (what, which, f)
        assert (got[0][0] > 0).any()
    return hits, zmin


def test_the_chain_on_one_frame_and_on_a_batch():
    h = pwpp_hip.Handle()
    one = with_nans(small_cloud(5), 1)
    h.estimate_ground(one)
    check_chain(h, [one], "one frame")
    frames = three_frames()
    frames[0] = with_nans(frames[0], 2)
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    hits, zmin = check_chain(h, frames, "three frames")
    assert hits[1].sum() == 0 and (zmin[1] == br.NO_HEIGHT).all()
    # a frame range, and device memory at 4-byte alignment
    import torch
    x0, y0, cell, nx, ny = GRID
    sub = h.rasterize_beams(*GRID, which=3, frame_first=1, frames=2)
    want = h.rasterize_beams(*GRID, which=3)
    assert sub[0].tobytes() == want[0][1:].tobytes() and sub[1].tobytes() == want[1][1:].tobytes()
    cells = 3 * nx * ny
    dev = [torch.full((cells + 128,), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
    occ = torch.full((cells + 64,), -7, dtype=torch.int8, device="cuda")
    h.rasterize_beams_device(x0, y0, cell, nx, ny, dev[0].data_ptr() + 4, dev[1].data_ptr() + 4, which=3)
    h.beam_ground_device(x0, y0, cell, nx, ny, ORIGIN, 1, 0, 1, 0.3, dev[2].data_ptr() + 4, dev[3].data_ptr() + 4, occ.data_ptr() + 1)
    h.synchronize()
    raw = [d.cpu().numpy() for d in dev] + [occ.cpu().numpy()]
    host = h.beam_ground(*GRID, origin_xyz=ORIGIN, which=1, clearance=0.3)
    for r, w in zip(raw, (want[0], want[1], host[0].view(np.int32), host[1], host[2])):
        assert r[1:1 + cells].tobytes() == w.tobytes() and r[0] == -7 and (r[1 + cells:] == -7).all()
    L = pwpp_hip.load()
    g = pwpp_hip.GroundGrid(x0, y0, cell, nx, ny, 0, 0)
    buf = np.zeros(cells, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for which in (0, 4, 7, -1):
        assert L.pwpp_rasterize_beams(h._h, ctypes.byref(g), which, 0, 3, pwpp_hip.MEM_HOST, p(buf), p(buf.copy())) == E_ARG and b"which" in L.pwpp_last_error()
    g.flags = pwpp_hip.GRID_GROUND_ONLY
    assert L.pwpp_rasterize_beams(h._h, ctypes.byref(g), 1, 0, 3, pwpp_hip.MEM_HOST, p(buf), p(buf.copy())) == E_ARG and b"grid flags" in L.pwpp_last_error()
    only = h.beam_ground(*GRID, origin_xyz=ORIGIN, which=1, clearance=0.3, ground_only=True, want_ends=True)   # the ground raster takes the flag, the endpoints do not
    assert only[3].tobytes() == h.rasterize_beams(*GRID, which=1)[0].tobytes()


def test_the_chain_with_an_input_transform():
    import input_transform_ref as xf
    T = xf.rigid(np.radians(3.0), np.radians(-5.0), np.radians(20.0), t=(0.2, -0.1, 0.15))
    level = with_nans(small_cloud(5), 3)
    sensor = np.ascontiguousarray(xf.transform_cloud(xf.inverse(T), level), np.float32)
    pre = sensor.copy()
    pre[:, :3] = pwpp_hip.transform_points(T, sensor[:, :3])
    h = pwpp_hip.Handle()
    h.set_input_transforms(T)
    h.estimate_ground(sensor)
    hits, _ = check_chain(h, [pre], "transformed")
    assert not np.array_equal(hits[0], br.ends_of_points(selected(h, sensor, 0, 3), GRID)[0])  # (the tilt matters)


def test_state_before_any_estimate_call():
    h = pwpp_hip.Handle()
    L = pwpp_hip.load()
    x0, y0, cell, nx, ny = GRID
    g = pwpp_hip.GroundGrid(x0, y0, cell, nx, ny, 0, 0)
    a, b = np.zeros(nx * ny, np.int32), np.zeros(nx * ny, np.int32)
    org = np.zeros(3, np.float64)
    p = lambda v: v.ctypes.data_as(ctypes.c_void_p)
    assert L.pwpp_rasterize_beams(h._h, ctypes.byref(g), 1, 0, 1, pwpp_hip.MEM_HOST, p(a), p(b)) == E_STATE
    assert L.pwpp_beam_ground(h._h, ctypes.byref(g), 1, p(org), 1, 0, 1, 0.3, 0, 1, pwpp_hip.MEM_HOST, None, p(a), p(b), None, None, None) == E_STATE
    hits, zmin = row()
    assert h.beam_grid(hits, zmin, (0, 0, 0))[0].sum() == 0   # (the operator on images needs no estimate call)


def test_workspace_and_the_pybind_method():
    h = pwpp_hip.Handle()
    empty = h.workspace_bytes()
    hits, zmin, target, base = scene(70, 45, 2, 0.3, 77)
    h.beam_grid(hits, zmin, np.array([(3, 40, 1700), (35, 22, -350)], np.int32), target=target, occupancy_in=base)
    grown = h.workspace_bytes()
    assert grown >= empty + 4 * (6 + 5 * hits.size + 2 * (hits.size // 4)), "the cluster buffer is not counted by pwpp_get_workspace_bytes"
    h.trim_workspace()
    assert h.workspace_bytes() == empty, "pwpp_trim_workspace did not free the cluster buffer"
    import pypatchworkpp
    cloud = small_cloud(5)
    h.estimate_ground(cloud)
    want = h.beam_ground(*GRID, origin_xyz=ORIGIN, which=1, min_pass=2, clearance=0.3, max_range=30)
    pw = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    pw.estimateGround(cloud)
    got = pw.getBeamClearance(*GRID, min_pass=2, clearance=0.3, max_range=30)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tobytes() == w[0].tobytes()
