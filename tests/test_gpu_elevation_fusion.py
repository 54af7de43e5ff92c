"""The elevation fusion (pwpp_fuse_height_grid, pwpp_fuse_ground) on a real MI355X, byte for byte against the restatement of
tests/elevation_fusion_ref.py -- sum, n and the mean's bits of whole maps compared, no tolerance, for every value of the option
"elevation_path": maps of 1, 255, 256 and 257 cells (the run boundary) and 70 x 67 x 3, frame images of 1 x 1, 5 x 7 and 33 x 31,
four cell pairs of which one takes the division, n_max 1, 2, 7 and 1023 with up to 40 frames into one map so that both branches of
the update run, every form of map_of_frame, every kind of pose, heights with NaN holes, infinities, ties and the limits, host and
device memory with device arrays misaligned to their minimum in poisoned surroundings, in place, mean absent, pwpp_fuse_ground
against rasterize-then-fuse, two device calls back to back, the workspace, and that asking changes nothing else."""
import ctypes
import functools

import numpy as np
import pytest

import elevation_fusion_ref as er
import pwpp_hip
from test_gpu_obstacle_grid import _everything, small_cloud, three_frames

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
# (NX, NY, n_maps): a single cell; one short of a run, a run, one past it; several maps of several runs with a ragged last run
MAP_SHAPES = [(1, 1, 1), (255, 1, 1), (16, 16, 1), (257, 1, 1), (70, 67, 3)]
IMAGES = [(1, 1), (5, 7), (33, 31)]  # (nx, ny) of the frame images
CELLS = ((0.5, 0.5), (0.25, 0.5), (1.0, 0.5), (0.5, 0.3))  # (CELL, cell) of the maps and of the frame images; the last takes the division on every path
N_MAX = (1, 2, 7, 1023)
PER_MAP = (1, 3, 40)
PATHS = (0, 1, 2)
shape_ids = lambda s: "%dx%dx%d" % s
NAN = float("nan")


def hmap_of(mgrid, n_max):
    return pwpp_hip.HeightMap(float(mgrid[0]), float(mgrid[1]), float(mgrid[2]), int(mgrid[3]), int(mgrid[4]), int(n_max), 0)


def centred(n, cell):
    return -0.5 * n * cell


def pose_kinds(cell, reach, seed):
    """identity, a whole-cell translation, a quarter turn, two random rigid poses, a frame half outside, one wholly outside, a NaN,
    a mirror (the transpose rule as defined)."""
    r = er.random_poses(2, seed, 0.25 * reach)
    return [er.IDENTITY, (1.0, 0.0, 3 * cell, 0.0, 1.0, -2 * cell), (0.0, -1.0, 0.0, 1.0, 0.0, 0.0), r[0], r[1], er.rigid(0.4, 0.5 * reach, 0.1),
            (1.0, 0.0, 1e7, 0.0, 1.0, 0.0), (1.0, 0.0, NAN, 0.0, 1.0, 0.0), (-1.0, 0.0, 0.3, 0.0, 1.0, -0.2)]


def random_state(rng, shape, n_max):
    """Maps to start from: mostly legal states, some outside what the normalisation keeps."""
    n = rng.integers(-1, min(n_max, 40) + 2, shape).astype(np.int16)
    s = (rng.integers(-3000, 1500, shape) * np.maximum(n, 1)).astype(np.int32)
    if n.size >= 8:
        n.reshape(-1)[:4] = (32767, -32768, n_max, n_max)
        s.reshape(-1)[:4] = (2 ** 31 - 1, 5, -2 ** 31, n_max * er.M)
    return s, n


@functools.lru_cache(maxsize=None)
def case(NX, NY, n_maps, nx, ny, per_map, ratio, k):
    """The inputs and the expected maps of one combination: computed once, shared, never written.  k rotates n_max, the pose kinds,
    the number of poses, the offsets, the form of map_of_frame, the inputs and the shifts, so that the combinations together cover
    all of them."""
    CELL, cell = CELLS[ratio]
    n_max = N_MAX[k % len(N_MAX)]
    frames = per_map * n_maps
    grid, mgrid = (centred(nx, cell), centred(ny, cell), cell), (centred(NX, CELL) + CELL, centred(NY, CELL), CELL, NX, NY)
    hgt = np.concatenate([er.random_heights(1, ny, nx, 100 * k + f, holes=(0.0, 0.3, 0.9)[(k + f) % 3]) for f in range(frames)])
    kinds = pose_kinds(cell, max(NX * CELL, nx * cell), k)
    poses = [kinds[(k + 2 * f) % len(kinds)] for f in range(frames)] if k % 3 else [kinds[k % 6]]
    rng = np.random.default_rng(k)
    tz = None if k % 4 == 1 else rng.uniform(-2.0, 2.0, len(poses))
    if tz is not None and len(tz) > 2:
        tz[1], tz[2] = np.inf, 1021.0  # a frame that observes nothing; one whose sums run to the limit
    if n_maps == 1 or (per_map == 1 and k % 2 == 0):
        mof = None  # one map: a sequence; n_maps == frames: lock-step
    else:  # explicit, interleaved and unsorted, with a skipped frame
        mof = [(7 * i + k) % n_maps for i in range(frames)]
        mof[(k + 1) % frames] = -1
    sum_in, n_in = (None, None) if k % 4 == 0 else random_state(rng, (n_maps, NY, NX), n_max)
    shift = None if k % 3 == 0 else [(int(rng.integers(-3, 4)), int(rng.integers(-3, 4))) for _ in range(n_maps)]
    want = er.fuse(hgt, grid, poses, mgrid, n_max, n_maps, sum_in, n_in, tz, mof, shift)
    for a in (hgt, sum_in, n_in) + want:
        if a is not None:
            a.setflags(write=False)
    return hgt, grid, poses, mgrid, n_max, n_maps, sum_in, n_in, tz, mof, shift, want


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()  # (no estimate call: pwpp_fuse_height_grid needs the handle's stream and buffer only)


def on_host(h, hgt, grid, poses, mgrid, n_max, n_maps, sum_in, n_in, tz, mof, shift, want_mean=True):
    return h.fuse_height_grid(hgt, grid, poses, hmap_of(mgrid, n_max), n_maps, sum_in, n_in, tz, mof, shift, want_mean)


def on_device(h, hgt, grid, poses, mgrid, n_max, n_maps, sum_in, n_in, tz, mof, shift, want_mean=True, off=1, in_place=False):
    """fuse_height_grid on device arrays; every array starts `off` of its own elements behind a 256-byte boundary -- 4 bytes for the
    heights, sums and means, 2 for the counts: their minimum; what surrounds them is poisoned and must survive, the inputs must not
    be written."""
    import torch
    frames, ny, nx = hgt.shape
    cells = n_maps * mgrid[3] * mgrid[4]
    dh = torch.full((hgt.size + 128,), -77.0, dtype=torch.float32, device="cuda")
    dsum = [torch.full((cells + 128,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    dn = [torch.full((cells + 128,), -7, dtype=torch.int16, device="cuda") for _ in range(2)]
    dmean = torch.full((cells + 128,), -7, dtype=torch.int32, device="cuda")  # (the means as words: a NaN compares with nothing)
    assert all(b.data_ptr() % 256 == 0 for b in dsum + dn + [dh, dmean])
    dh[off:off + hgt.size] = torch.from_numpy(hgt.reshape(-1).copy()).cuda()
    if sum_in is not None:
        dsum[0][off:off + cells] = torch.from_numpy(sum_in.reshape(-1).copy()).cuda()
        dn[0][off:off + cells] = torch.from_numpy(n_in.reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    have = sum_in is not None
    assert not in_place or have
    so, no = (dsum[0], dn[0]) if in_place else (dsum[1], dn[1])
    h.fuse_height_grid_device(grid, nx, ny, frames, dh.data_ptr() + 4 * off, poses, hmap_of(mgrid, n_max), n_maps,
                              dsum[0].data_ptr() + 4 * off if have else 0, dn[0].data_ptr() + 2 * off if have else 0, so.data_ptr() + 4 * off,
                              no.data_ptr() + 2 * off, dmean.data_ptr() + 4 * off if want_mean else 0, tz, mof, shift)
    h.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
    rh = dh.cpu().numpy()
    assert (rh[:off] == -77).all() and (rh[off + hgt.size:] == -77).all() and rh[off:off + hgt.size].tobytes() == hgt.tobytes(), "the frames were written"
    got = [so.cpu().numpy(), no.cpu().numpy(), dmean.cpu().numpy()]
    for r in got + [dsum[0].cpu().numpy(), dn[0].cpu().numpy()]:
        assert (r[:off] == -7).all() and (r[off + cells:] == -7).all(), "an element outside a map was written"
    if not in_place:
        for r, src in ((dsum[0].cpu().numpy(), sum_in), (dn[0].cpu().numpy(), n_in)):
            assert np.array_equal(r[off:off + cells], src.reshape(-1)) if have else (r == -7).all(), "an input map was written"
    if not want_mean:
        assert (got[2] == -7).all()
    shape = (n_maps, mgrid[4], mgrid[3])
    return (got[0][off:off + cells].reshape(shape), got[1][off:off + cells].reshape(shape),
            got[2][off:off + cells].view(np.float32).reshape(shape) if want_mean else None)


def all_paths(h, call):
    """call() at "elevation_path" 0, 1 and 2: identical bytes; returns them."""
    res = []
    for path in PATHS:
        h.set_option("elevation_path", path)
        res.append(call())
    h.set_option("elevation_path", 0)
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert (a is None and b is None) or a.tobytes() == b.tobytes(), "the values of elevation_path differ"
    return res[0]


def check(got, want, what, want_mean=True):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int16 and got[0].shape == want[0].shape == got[1].shape, what
    for i, name in enumerate(("sum", "n")):
        bad = np.argwhere(got[i] != want[i])
        assert len(bad) == 0, "%s: %d cells of %s differ, the first (map, jy, jx) = %s: %d, expected %d" % (
            what, len(bad), name, bad[0], got[i][tuple(bad[0])], want[i][tuple(bad[0])])
    if want_mean:
        assert got[2].dtype == np.float32 and got[2].tobytes() == want[2].tobytes(), "%s: the mean's bits differ" % what
    else:
        assert got[2] is None


@pytest.mark.parametrize("shape", MAP_SHAPES, ids=shape_ids)
def test_map_shapes_against_the_reference(handle, shape):
    NX, NY, n_maps = shape
    k = 0
    grown = capped = 0
    for nx, ny in IMAGES:
        for ratio in range(len(CELLS)):
            k += 1
            per_map = PER_MAP[k % len(PER_MAP)]
            args = case(NX, NY, n_maps, nx, ny, per_map, ratio, k)
            what = "map %s, frames %dx%d x %d per map, cells %s, n_max %d, case %d" % (shape_ids(shape), nx, ny, per_map, CELLS[ratio], args[4], k)
            check(all_paths(handle, lambda: on_host(handle, *args[:-1])), args[-1], what)
            if k % 3 == 1:
                check(all_paths(handle, lambda: on_device(handle, *args[:-1])), args[-1], what + ", device")
            n = args[-1][1]
            grown += int(((n > 0) & (n < args[4])).sum())
            capped += int((n == args[4]).sum())
    assert grown and capped, "the cases of this shape never run one of the two branches of the update"


def test_a_frame_cell_that_is_no_power_of_two_takes_the_division_on_every_path(handle):
    """(the shapes test runs cell 0.3 on host memory at every shape; here on both memory kinds)"""
    for NX, NY, n_maps, nx, ny in ((257, 1, 1, 5, 7), (70, 67, 3, 33, 31)):
        args = case(NX, NY, n_maps, nx, ny, 3, 3, 6)
        assert (args[-1][1] > 0).sum() > 20
        for run in (on_host, on_device):
            check(all_paths(handle, lambda: run(handle, *args[:-1])), args[-1], "cells (0.5, 0.3), %dx%dx%d, %s" % (NX, NY, n_maps, run.__name__))


def test_forty_frames_into_one_map_at_every_n_max(handle):
    nx, ny, NX, NY = 33, 31, 37, 29
    grid, mgrid = (centred(nx, 0.5), centred(ny, 0.5), 0.5), (centred(NX, 0.5), centred(NY, 0.5), 0.5, NX, NY)
    hgt = er.random_heights(40, ny, nx, 11, holes=0.2)
    hgt[5] = 1023.5  # a frame at the limit: with its offset below some cells observe, the running sums reach n M
    hgt[17] = -1024.0
    poses = [er.rigid(0.02 * f, 0.1 * f - 2.0, 0.05 * f) for f in range(40)]
    tz = np.linspace(-0.6, 0.6, 40)
    for n_max in N_MAX:
        want = er.fuse(hgt, grid, poses, mgrid, n_max, 1, None, None, tz)
        assert (want[1] == n_max).any() if n_max <= 7 else 7 < want[1].max() < n_max  # capped cells; beyond 7 frames seen and none capped
        for run in (on_host, on_device):
            check(all_paths(handle, lambda: run(handle, hgt, grid, poses, mgrid, n_max, 1, None, None, tz, None, None)), want, "n_max %d, %s" % (n_max, run.__name__))


def test_map_of_frame_in_every_form(handle):
    NX, NY, nx, ny = 37, 29, 33, 31
    grid, mgrid = (centred(nx, 0.5), centred(ny, 0.5), 0.5), (centred(NX, 0.5), centred(NY, 0.5), 0.5, NX, NY)
    hgt = er.random_heights(6, ny, nx, 21)
    poses = er.random_poses(6, 22, 3.0)
    tz = [0.0, 0.5, -0.5, NAN, 1.0, -1.0]
    s4, n4 = random_state(np.random.default_rng(23), (4, NY, NX), 2)
    shift = [(1, 0), (0, -2), (-3, 3), (2, 2)]
    # NULL with one map: a sequence; NULL with n_maps == frames: lock-step
    check(all_paths(handle, lambda: on_host(handle, hgt, grid, poses, mgrid, 2, 1, s4[:1], n4[:1], tz, None, None)),
          er.fuse(hgt, grid, poses, mgrid, 2, 1, s4[:1], n4[:1], tz), "sequence")
    s6, n6 = np.concatenate([s4, s4[:2]]), np.concatenate([n4, n4[:2]])
    check(all_paths(handle, lambda: on_host(handle, hgt, grid, poses, mgrid, 2, 6, s6, n6, tz, None, None)),
          er.fuse(hgt, grid, poses, mgrid, 2, 6, s6, n6, tz), "lock-step")
    # explicit: interleaved, unsorted, skipped frames, and map 2 that no frame names: its shifted, normalised input
    mof = [3, 0, -1, 3, 1, 0]
    want = er.fuse(hgt, grid, poses, mgrid, 2, 4, s4, n4, tz, mof, shift)
    start = er.shifted(s4, n4, mgrid, 4, shift, 2)
    for run in (on_host, on_device):
        got = all_paths(handle, lambda: run(handle, hgt, grid, poses, mgrid, 2, 4, s4, n4, tz, mof, shift))
        check(got, want, "explicit map_of_frame, %s" % run.__name__)
        assert np.array_equal(got[0][2], start[0][2]) and np.array_equal(got[1][2], start[1][2])
    none = on_host(handle, hgt, grid, poses, mgrid, 2, 4, s4, n4, tz, [-1] * 6, shift)
    assert np.array_equal(none[0], start[0]) and np.array_equal(none[1], start[1])
    L = pwpp_hip.load()
    with pytest.raises(pwpp_hip.PwppError):
        on_host(handle, hgt, grid, poses, mgrid, 2, 4, s4, n4, tz, np.array([0, 4, 0, 0, 0, 0], np.int32), shift)
    assert b"map_of_frame 1 names map 4" in L.pwpp_last_error()


def test_shifts_null_input_in_place_and_mean_absent(handle):
    NX, NY, nx, ny = 33, 31, 5, 7
    grid, mgrid = (centred(nx, 0.5), centred(ny, 0.5), 0.5), (centred(NX, 0.5), centred(NY, 0.5), 0.5, NX, NY)
    hgt = er.random_heights(3, ny, nx, 31)
    poses = er.random_poses(3, 32, 2.0)
    s3, n3 = random_state(np.random.default_rng(33), (3, NY, NX), 7)
    big = 2 ** 31 - 1
    for shift in (None, [(0, 0)] * 3, [(1, 2), (-2, 1), (3, -3)], [(NX, 0), (0, -NY), (NX - 1, 1 - NY)], [(big, 0), (-big - 1, -big - 1), (0, big)]):
        want = er.fuse(hgt, grid, poses, mgrid, 7, 3, s3, n3, None, None, shift)
        for run in (on_host, on_device):
            check(all_paths(handle, lambda: run(handle, hgt, grid, poses, mgrid, 7, 3, s3, n3, None, None, shift)), want, "shift %s, %s" % (shift, run.__name__))
    # both inputs NULL: empty maps, whatever the shift; the mean absent
    want = er.fuse(hgt, grid, poses, mgrid, 7, 3)
    for run in (on_host, on_device):
        check(run(handle, hgt, grid, poses, mgrid, 7, 3, None, None, None, None, [(1, 2), (-2, 1), (3, -3)]), want, "null inputs, %s" % run.__name__)
        check(all_paths(handle, lambda: run(handle, hgt, grid, poses, mgrid, 7, 3, s3, n3, None, None, None, want_mean=False)),
              er.fuse(hgt, grid, poses, mgrid, 7, 3, s3, n3), "mean absent, %s" % run.__name__, want_mean=False)
    # in place: the outputs are the inputs, no shift or a zero one
    want = er.fuse(hgt, grid, poses, mgrid, 7, 3, s3, n3)
    for shift in (None, [(0, 0)] * 3):
        ms, mn = s3.copy(), n3.copy()
        out = handle.fuse_height_grid(hgt, grid, poses, hmap_of(mgrid, 7), 3, ms, mn, None, None, shift, sum_out=ms, n_out=mn)
        assert out[0] is ms and out[1] is mn
        check(out, want, "in place, host")
        check(all_paths(handle, lambda: on_device(handle, hgt, grid, poses, mgrid, 7, 3, s3, n3, None, None, shift, in_place=True)), want, "in place, device")
    with pytest.raises(pwpp_hip.PwppError):
        ms, mn = s3.copy(), n3.copy()
        handle.fuse_height_grid(hgt, grid, poses, hmap_of(mgrid, 7), 3, ms, mn, None, None, [(0, 0), (0, 1), (0, 0)], sum_out=ms, n_out=mn)


def test_the_order_examples_and_the_composition_of_two_calls(handle):
    g1, m1 = (0.0, 0.0, 1.0), (0.0, 0.0, 1.0, 1, 1)
    img = lambda *hs: np.array(hs, np.float32).reshape(-1, 1, 1)
    s0, n0 = np.array([[[3072]]], np.int32), np.array([[[2]]], np.int16)
    for run in (on_host, on_device):
        assert run(handle, img(1.0, 2.0), g1, er.IDENTITY, m1, 1, 1, None, None, None, None, None)[2][0, 0, 0] == 2.0
        assert run(handle, img(2.0, 1.0), g1, er.IDENTITY, m1, 1, 1, None, None, None, None, None)[2][0, 0, 0] == 1.0
        assert all_paths(handle, lambda: run(handle, img(1.0, 3.0), g1, er.IDENTITY, m1, 2, 1, s0, n0, None, None, None))[0][0, 0, 0] == 4352
        assert all_paths(handle, lambda: run(handle, img(3.0, 1.0), g1, er.IDENTITY, m1, 2, 1, s0, n0, None, None, None))[0][0, 0, 0] == 3328
    # two calls, the second on the first's output with no shift, are one call over the concatenated frames
    nx, ny, NX, NY = 33, 31, 70, 67
    grid, mgrid = (centred(nx, 0.5), centred(ny, 0.5), 0.5), (centred(NX, 0.25), centred(NY, 0.25), 0.25, NX, NY)
    hgt = er.random_heights(7, ny, nx, 51)
    poses = er.random_poses(7, 52, 3.0)
    tz = np.linspace(-1.0, 1.0, 7)
    mof = [0, 1, 1, 0, -1, 1, 0]
    s2, n2 = random_state(np.random.default_rng(53), (2, NY, NX), 2)
    shift = [(2, -1), (-1, 4)]
    whole = er.fuse(hgt, grid, poses, mgrid, 2, 2, s2, n2, tz, mof, shift)
    for run in (on_host, on_device):
        one = all_paths(handle, lambda: run(handle, hgt, grid, poses, mgrid, 2, 2, s2, n2, tz, mof, shift))
        first = run(handle, hgt[:3], grid, poses[:3], mgrid, 2, 2, s2, n2, tz[:3], mof[:3], shift)
        second = run(handle, hgt[3:], grid, poses[3:], mgrid, 2, 2, first[0], first[1], tz[3:], mof[3:], None)
        check(one, whole, "one call, %s" % run.__name__)
        check(second, whole, "two calls, %s" % run.__name__)


def test_device_arrays_at_their_minimum_alignment_give_the_aligned_bytes(handle):
    args = case(70, 67, 3, 33, 31, 3, 0, 7)
    assert args[6] is not None and args[10] is not None and args[9] is not None
    aligned = on_device(handle, *args[:-1], off=0)
    moved = all_paths(handle, lambda: on_device(handle, *args[:-1], off=1))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(aligned, moved))
    check(moved, args[-1], "70x67x3 one element off")
    L = pwpp_hip.load()
    with pytest.raises(pwpp_hip.PwppError):  # below the minimum: named, nothing launched
        handle.fuse_height_grid_device((0.0, 0.0, 1.0), 1, 1, 1, 4096, er.IDENTITY, hmap_of((0.0, 0.0, 1.0, 1, 1), 1), 1, 0, 0, 4098, 8192)
    assert b"4-byte aligned" in L.pwpp_last_error()


# ---- pwpp_fuse_ground ----------------------------------------------------------------------------------------------------------
def test_fuse_ground_is_rasterize_ground_plus_fuse_height_grid():
    nx, ny, cell = 120, 96, 0.5
    x0, y0 = -30.0, -24.0
    mgrid = (-32.0, -26.0, 0.5, 130, 104)
    hm = hmap_of(mgrid, 3)
    pose, tz = er.rigid(0.3, 1.2, -0.7), [1.7]
    L = pwpp_hip.load()
    h = pwpp_hip.Handle()
    g = pwpp_hip.GroundGrid(x0, y0, cell, nx, ny, 0, 0)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    cells = mgrid[3] * mgrid[4]
    so, no, p6 = np.zeros(cells, np.int32), np.zeros(cells, np.int16), np.array(pose, np.float64)
    assert L.pwpp_fuse_ground(h._h, ctypes.byref(g), 0, 1, pwpp_hip.MEM_HOST, vp(p6), None, 1, None, ctypes.byref(hm), 1, None, None, None, vp(so), vp(no),
                              None, None) == E_STATE
    h.set_labels(True)  # (_everything reads them)
    h.estimate_ground(small_cloud(5))
    before = _everything(h, 1)
    s1, n1 = random_state(np.random.default_rng(61), (1, mgrid[4], mgrid[3]), 3)
    shift = [(3, -2)]
    for ground_only in (False, True):
        what = "ground_only %s" % ground_only
        img = h.rasterize_ground(x0, y0, cell, nx, ny, ground_only=ground_only)
        assert np.isfinite(img).sum() > 200 and np.isnan(img).any()
        steps = h.fuse_height_grid(img, (x0, y0, cell), pose, hm, 1, s1, n1, tz, None, shift)
        got = all_paths(h, lambda: h.fuse_ground(x0, y0, cell, nx, ny, pose, hm, 1, s1, n1, tz, shift=shift, ground_only=ground_only, want_frames=True))
        assert got[3].tobytes() == img.tobytes(), what + ": the per-frame images differ from pwpp_rasterize_ground's"
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], steps)), what + ": differs from the two steps"
        kept = h.fuse_ground(x0, y0, cell, nx, ny, pose, hm, 1, s1, n1, tz, shift=shift, ground_only=ground_only)  # the images kept in the handle
        assert all(a.tobytes() == b.tobytes() for a, b in zip(kept, got[:3])), what
        check(got[:3], er.fuse(img, (x0, y0, cell), pose, mgrid, 3, 1, s1, n1, tz, None, shift), what)
    # into device memory at the minimum alignment, the frames' images kept and asked for
    import torch
    dsum = [torch.full((cells + 128,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    dn = [torch.full((cells + 128,), -7, dtype=torch.int16, device="cuda") for _ in range(2)]
    dmean = torch.full((cells + 128,), -7, dtype=torch.int32, device="cuda")
    dh = torch.full((nx * ny + 128,), -7, dtype=torch.int32, device="cuda")
    dsum[0][1:1 + cells] = torch.from_numpy(s1.reshape(-1).copy()).cuda()
    dn[0][1:1 + cells] = torch.from_numpy(n1.reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    for h_ptr in (0, dh.data_ptr() + 4):
        h.fuse_ground_device(x0, y0, cell, nx, ny, pose, hm, 1, dsum[0].data_ptr() + 4, dn[0].data_ptr() + 2, dsum[1].data_ptr() + 4, dn[1].data_ptr() + 2,
                             dmean.data_ptr() + 4, h_ptr, tz, shift=shift, ground_only=True)
        h.synchronize()
        raw = [dsum[1].cpu().numpy(), dn[1].cpu().numpy(), dmean.cpu().numpy()]
        assert all(r[1:1 + cells].tobytes() == w.tobytes() for r, w in zip(raw, got[:3]))
        for r in raw:
            assert (r[:1] == -7).all() and (r[1 + cells:] == -7).all()
    rh = dh.cpu().numpy()
    assert rh[1:1 + nx * ny].tobytes() == img.tobytes() and rh[0] == -7 and (rh[1 + nx * ny:] == -7).all()
    assert _everything(h, 1) == before, "the elevation fusion changed the results of the call it reads"


def test_three_frames_as_a_sequence_and_in_lock_step():
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(three_frames(), mode=pwpp_hip.MODE_FRESH)  # a 16-beam scan, an empty frame, a frame that is all unref
    grid = (-16.0, -16.0, 0.5, 64, 64)
    mgrid = (-20.0, -18.0, 0.5, 80, 72)
    hm = hmap_of(mgrid, 2)
    poses = [er.rigid(0.1 * f, 0.5 * f, -0.25 * f) for f in range(3)]
    tz = [0.0, 0.1, -0.1]
    img = h.rasterize_ground(*grid)
    seq = all_paths(h, lambda: h.fuse_ground(*grid, poses, hm, 1, z_offset=tz))
    check(seq, er.fuse(img, grid[:3], poses, mgrid, 2, 1, None, None, tz), "three frames into one map")
    lock = all_paths(h, lambda: h.fuse_ground(*grid, poses, hm, 3, z_offset=tz))
    check(lock, er.fuse(img, grid[:3], poses, mgrid, 2, 3, None, None, tz), "three frames into three maps")
    assert (lock[1][0] > 0).sum() > 100 and not lock[1][1].any()  # the empty frame has no ground
    sub = h.fuse_ground(*grid, poses[1:], hm, 2, z_offset=tz[1:], frame_first=1, frames=2)  # entry i belongs to frame frame_first + i
    assert all(a.tobytes() == b[1:].tobytes() for a, b in zip(sub, lock))


def test_two_device_calls_back_to_back_each_fuse_under_their_own_tables():
    """The poses and offsets of a call are uploaded from the handle's own copy, and the second call replaces that copy while the
    first may still be in flight: two calls with a pose and an offset per frame, different ones, into different maps, one
    synchronize() after both."""
    import torch
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(three_frames(), mode=pwpp_hip.MODE_FRESH)
    grid = (-16.0, -16.0, 0.5, 64, 64)
    mgrid = (-20.0, -18.0, 0.5, 80, 72)
    hm = hmap_of(mgrid, 2)
    calls = [([er.rigid(0.1 * f, 0.5 * f, -0.25 * f) for f in range(3)], [0.0, 0.5, 1.0]),
             ([er.rigid(-0.3 - 0.2 * f, 1.5 - f, 0.75 * f) for f in range(3)], [-1.0, 2.0, 0.25])]
    img = h.rasterize_ground(*grid)
    want = [er.fuse(img, grid[:3], poses, mgrid, 2, 3, None, None, tz) for poses, tz in calls]
    assert want[0][0].tobytes() != want[1][0].tobytes() and (want[0][1][0] > 0).sum() > 100
    cells = 3 * mgrid[3] * mgrid[4]
    out = [(torch.full((cells,), -7, dtype=torch.int32, device="cuda"), torch.full((cells,), -7, dtype=torch.int16, device="cuda"),
            torch.full((cells,), -7, dtype=torch.int32, device="cuda")) for _ in calls]
    torch.cuda.synchronize()
    for (poses, tz), (ds, dn, dm) in zip(calls, out):
        h.fuse_ground_device(*grid, poses, hm, 3, 0, 0, ds.data_ptr(), dn.data_ptr(), dm.data_ptr(), 0, tz)
    h.synchronize()
    for i, (ds, dn, dm) in enumerate(out):
        shape = want[i][0].shape
        check((ds.cpu().numpy().reshape(shape), dn.cpu().numpy().reshape(shape), dm.cpu().numpy().view(np.float32).reshape(shape)), want[i], "call %d of two" % i)


# ---- workspace ------------------------------------------------------------------------------------------------------------------
def test_workspace_and_that_nothing_else_moves():
    h = pwpp_hip.Handle()
    empty = h.workspace_bytes()
    args = case(70, 67, 3, 33, 31, 3, 0, 7)
    hgt, poses, cells = args[0], args[2], 3 * 70 * 67
    check(on_host(h, *args[:-1]), args[-1], "before any estimate call")
    grown = h.workspace_bytes()
    # the poses, offsets, lists and shifts, the staged frames, both sums, both counts and the mean in words
    assert grown >= empty + 4 * (14 * len(poses) + 4 + 8 + 6 + hgt.size + 3 * cells + 2 * (cells // 2)), "the cluster buffer is not counted"
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
    b.fuse_ground(-20.0, -20.0, 0.5, 80, 80, er.IDENTITY, hmap_of((-20.0, -20.0, 0.5, 80, 80), 4), 3)
    assert b.workspace_bytes() >= a.workspace_bytes() + 4 * 3 * 80 * 80  # the kept height images
    assert _everything(b, 3) == before and b.time_us() == t_before, "the elevation fusion changed the results of the call it reads"
    for w in (a, b):
        w.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert _everything(b, 3) == _everything(a, 3), "an estimate call after an elevation fusion call differs from one without"
    b.trim_workspace()
    a.trim_workspace()
    assert a.workspace_bytes() == b.workspace_bytes()
    with pytest.raises(pwpp_hip.PwppError):
        h.set_option("elevation_path", 3)


def test_pybind_module_agrees_with_the_ctypes_handle():
    import pypatchworkpp
    pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    h = pwpp_hip.Handle()
    m = pypatchworkpp.FusedElevationMap()
    m.x0, m.y0, m.cell, m.nx, m.ny, m.n_max = -32.0, -14.0, 0.5, 130, 56, 2
    pose = er.rigid(0.2, 1.0, -0.5)
    with pytest.raises(RuntimeError):
        pp.updateElevationMap(m, pose, 0.0, -30.0, -12.0, 0.5, 120, 48)  # no frame yet
    assert (m.x0, m.y0) == (-32.0, -14.0) and np.isnan(pp.getFusedElevation(m)).all()
    pts = small_cloud(5)
    pp.estimateGround(pts)
    h.estimate_ground(pts)
    hm = hmap_of((-32.0, -14.0, 0.5, 130, 56), 2)
    s1, n1, m1 = pp.updateElevationMap(m, pose, 1.7, -30.0, -12.0, 0.5, 120, 48)
    h1 = h.fuse_ground(-30.0, -12.0, 0.5, 120, 48, pose, hm, z_offset=[1.7])
    assert s1.dtype == np.int32 and n1.dtype == np.int16 and m1.dtype == np.float32 and s1.shape == n1.shape == m1.shape == (56, 130) and (n1 > 0).sum() > 100
    assert s1.tobytes() == h1[0][0].tobytes() and n1.tobytes() == h1[1][0].tobytes() and m1.tobytes() == h1[2][0].tobytes()
    # the second update rolls the map two cells east and one south: the map's origin moves with it
    s2, n2, m2 = pp.updateElevationMap(m, pose, 1.6, -30.0, -12.0, 0.5, 120, 48, True, 2, -1)
    assert (m.x0, m.y0) == (-31.0, -14.5)
    hm2 = hmap_of((-31.0, -14.5, 0.5, 130, 56), 2)
    h2 = h.fuse_ground(-30.0, -12.0, 0.5, 120, 48, pose, hm2, 1, h1[0], h1[1], [1.6], shift=[(2, -1)], ground_only=True)
    assert s2.tobytes() == h2[0][0].tobytes() and n2.tobytes() == h2[1][0].tobytes() and m2.tobytes() == h2[2][0].tobytes()
    assert pp.getFusedElevation(m).tobytes() == m2.tobytes() and (n2 == 2).any()
