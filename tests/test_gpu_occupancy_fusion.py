"""The occupancy fusion (pwpp_fuse_grid, pwpp_fuse_obstacles) on a real MI355X, byte for byte against the restatement of
tests/occupancy_fusion_ref.py -- whole maps compared, no tolerance: map shapes from one cell to several maps of several runs,
frame images from one cell to 64 x 64 with 1, 2 and 5 frames per map, every kind of pose, three cell ratios, every form of
map_of_frame, shifts of both signs and beyond the map, map_in absent and in place, the parameters at their extremes, the order
example and the composition of two calls, host and device memory with misaligned device arrays in poisoned surroundings, both
values of the option "fusion_path" on cell sizes that are powers of two (where path 0 multiplies) and on ones that are not,
pwpp_fuse_obstacles against its three steps on a KITTI frame, two device calls back to back with different origins and poses, and
that asking changes nothing else."""
import ctypes
import functools

import numpy as np
import pytest

import occupancy_fusion_ref as fr
import pwpp_hip
from test_gpu_obstacle_grid import _everything, three_frames

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
BAND = (0.2, 2.5)
# (NX, NY, n_maps): a single cell; a column and a row longer than a wave; a run boundary inside a row; one cell past and one short
# of whole runs; several maps
MAP_SHAPES = [(1, 1, 1), (1, 70, 1), (70, 1, 1), (33, 31, 1), (65, 63, 2), (70, 67, 3)]
IMAGES = [(1, 1), (5, 7), (33, 31), (64, 64)]  # (nx, ny) of the frame images
PER_MAP = (1, 2, 5)
CELLS = ((0.5, 0.5), (0.25, 0.5), (1.0, 0.5))  # (CELL, cell)
FILLS = ((0.0, 0.0, 1.0), (0.55, 0.15, 0.3), (0.9, 0.1, 0.0), (0.0, 1.0, 0.0))  # (free, occupied, unknown): all unknown .. all occupied
shape_ids = lambda s: "%dx%dx%d" % s
NAN = float("nan")


def fmap_of(mgrid, par):
    return pwpp_hip.FusionMap(float(mgrid[0]), float(mgrid[1]), float(mgrid[2]), int(mgrid[3]), int(mgrid[4]), *[int(p) for p in par])


def centred(n, cell):
    return -0.5 * n * cell


def pose_kinds(cell, reach, seed):
    """identity, a whole-cell translation, a quarter turn, two random rigid poses, a frame half outside, one wholly outside, a NaN,
    a mirror (the transpose rule as defined)."""
    r = fr.random_poses(2, seed, 0.25 * reach)
    return [fr.IDENTITY, (1.0, 0.0, 3 * cell, 0.0, 1.0, -2 * cell), (0.0, -1.0, 0.0, 1.0, 0.0, 0.0), r[0], r[1], fr.rigid(0.4, 0.5 * reach, 0.1),
            (1.0, 0.0, 1e7, 0.0, 1.0, 0.0), (1.0, 0.0, NAN, 0.0, 1.0, 0.0), (-1.0, 0.0, 0.3, 0.0, 1.0, -0.2)]


@functools.lru_cache(maxsize=None)
def case(NX, NY, n_maps, nx, ny, per_map, ratio, k):
    """The inputs and the expected maps of one combination: computed once, shared, never written.  k rotates the fills, the pose
    kinds, the number of poses and the form of map_of_frame, so that the combinations together cover all of them."""
    CELL, cell = CELLS[ratio]
    frames = per_map * n_maps
    grid, mgrid = (centred(nx, cell), centred(ny, cell), cell), (centred(NX, CELL) + CELL, centred(NY, CELL), CELL, NX, NY)
    occ = np.concatenate([fr.random_occupancy(1, ny, nx, 100 * k + f, FILLS[(k + f) % len(FILLS)], stray=(k + f) % 2 == 0) for f in range(frames)])
    kinds = pose_kinds(cell, max(NX * CELL, nx * cell), k)
    poses = [kinds[(k + 2 * f) % len(kinds)] for f in range(frames)] if k % 3 else [kinds[k % len(kinds)]]
    if n_maps == 1 or (per_map == 1 and k % 2 == 0):
        mof = None  # one map: a sequence; n_maps == frames: lock-step
    else:  # explicit, interleaved and unsorted, with skipped frames
        mof = [(7 * i + k) % n_maps for i in range(frames)]
        if frames > 2:
            mof[(k + 1) % frames] = -1
    rng = np.random.default_rng(k)
    map_in = None if k % 4 == 0 else rng.integers(-260, 420, (n_maps, NY, NX)).astype(np.int16)  # (outside the clamps of PAR too)
    shift = None if k % 3 == 0 else [(int(rng.integers(-3, 4)), int(rng.integers(-3, 4))) for _ in range(n_maps)]
    want = fr.fuse(occ, grid, poses, mgrid, fr.PAR, n_maps, map_in, mof, shift)
    for a in (occ, map_in) + want:
        if a is not None:
            a.setflags(write=False)
    return occ, grid, poses, mgrid, mof, map_in, shift, want


@pytest.fixture(scope="module")
def handle():
    return pwpp_hip.Handle()  # (no estimate call: pwpp_fuse_grid needs the handle's stream and buffer only)


def on_host(h, occ, grid, poses, mgrid, par, n_maps, map_in, mof, shift):
    return h.fuse_grid(occ, grid, poses, fmap_of(mgrid, par), n_maps, map_in, mof, shift)


def on_device(h, occ, grid, poses, mgrid, par, n_maps, map_in, mof, shift, off=0, in_place=False):
    """fuse_grid on device arrays; the maps start `off` halfwords, the bytes `off` bytes behind a 256-byte boundary; what surrounds
    them is poisoned and must survive, the inputs must not be written."""
    import torch
    frames, ny, nx = occ.shape
    cells = n_maps * mgrid[3] * mgrid[4]
    docc = torch.full((occ.size + 512,), 77, dtype=torch.int8, device="cuda")
    dmaps = [torch.full((cells + 256,), -7, dtype=torch.int16, device="cuda") for _ in range(2)]
    dbyte = torch.full((cells + 512,), -7, dtype=torch.int8, device="cuda")
    assert all(b.data_ptr() % 256 == 0 for b in dmaps + [docc, dbyte])
    docc[off:off + occ.size] = torch.from_numpy(occ.reshape(-1).copy()).cuda()
    if map_in is not None:
        dmaps[0][off:off + cells] = torch.from_numpy(map_in.reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    in_ptr = dmaps[0].data_ptr() + 2 * off if map_in is not None else 0
    assert not in_place or in_ptr
    out = dmaps[0] if in_place else dmaps[1]
    h.fuse_grid_device(grid, nx, ny, frames, docc.data_ptr() + off, poses, fmap_of(mgrid, par), n_maps, in_ptr, out.data_ptr() + 2 * off,
                       dbyte.data_ptr() + off, mof, shift)
    h.synchronize()  # (complete after pwpp_synchronize: the copies below are on another stream)
    rocc, rin, rout, rbyte = docc.cpu().numpy(), dmaps[0].cpu().numpy(), out.cpu().numpy(), dbyte.cpu().numpy()
    assert (rocc[:off] == 77).all() and (rocc[off + occ.size:] == 77).all() and np.array_equal(rocc[off:off + occ.size], occ.reshape(-1)), "the frames were written"
    for r in (rin, rout, rbyte):
        assert (r[:off] == -7).all() and (r[off + cells:] == -7).all(), "a halfword or byte outside a map was written"
    if not in_place:
        assert np.array_equal(rin[off:off + cells], map_in.reshape(-1)) if map_in is not None else (rin == -7).all(), "map_in was written"
    shape = (n_maps, mgrid[4], mgrid[3])
    return rout[off:off + cells].reshape(shape), rbyte[off:off + cells].reshape(shape)


def both_paths(h, call):
    """call() at "fusion_path" 0 and 1: identical bytes; returns them."""
    res = []
    for path in (0, 1):
        h.set_option("fusion_path", path)
        res.append(call())
    h.set_option("fusion_path", 0)
    for a, b in zip(res[0], res[1]):
        assert a.tobytes() == b.tobytes(), "the two values of fusion_path differ"
    return res[0]


def check(got, want, what):
    assert got[0].dtype == np.int16 and got[1].dtype == np.int8 and got[0].shape == want[0].shape == got[1].shape, what
    bad = np.argwhere(got[0] != want[0])
    assert len(bad) == 0, "%s: %d map cells differ, the first (map, jy, jx) = %s: %d, expected %d" % (
        what, len(bad), bad[0], got[0][tuple(bad[0])], want[0][tuple(bad[0])])
    assert np.array_equal(got[1], want[1]), "%s: the byte differs" % what


@pytest.mark.parametrize("shape", MAP_SHAPES, ids=shape_ids)
def test_map_shapes_against_the_reference(handle, shape):
    NX, NY, n_maps = shape
    k = 0
    seen = np.zeros(3, bool)
    for nx, ny in IMAGES:
        for per_map in PER_MAP:
            for ratio in range(len(CELLS)):
                k += 1
                occ, grid, poses, mgrid, mof, map_in, shift, want = case(NX, NY, n_maps, nx, ny, per_map, ratio, k)
                what = "map %s, frames %dx%d x %d per map, cells %s, case %d" % (shape_ids(shape), nx, ny, per_map, CELLS[ratio], k)
                args = (occ, grid, poses, mgrid, fr.PAR, n_maps, map_in, mof, shift)
                check(both_paths(handle, lambda: on_host(handle, *args)), want, what)
                if k % 3 == 1:
                    check(on_device(handle, *args), want, what + ", device")
                for b, v in enumerate((fr.FREE, fr.OCCUPIED, fr.UNKNOWN)):
                    seen[b] |= bool((want[1] == v).any())
    assert NX * NY == 1 or seen.all(), "the cases of this shape never produce one of the three bytes"


def test_map_of_frame_in_every_form(handle):
    NX, NY, nx, ny = 37, 29, 33, 31
    grid, mgrid = (centred(nx, 0.5), centred(ny, 0.5), 0.5), (centred(NX, 0.5), centred(NY, 0.5), 0.5, NX, NY)
    occ = fr.random_occupancy(6, ny, nx, 21)
    poses = fr.random_poses(6, 22, 3.0)
    start = np.random.default_rng(23).integers(-100, 100, (4, NY, NX)).astype(np.int16)
    shift = [(1, 0), (0, -2), (-3, 3), (2, 2)]
    # NULL with one map: a sequence; NULL with n_maps == frames: lock-step
    check(both_paths(handle, lambda: on_host(handle, occ, grid, poses, mgrid, fr.PAR, 1, start[:1], None, None)),
          fr.fuse(occ, grid, poses, mgrid, fr.PAR, 1, start[:1]), "sequence")
    six = np.concatenate([start, start[:2]])
    check(both_paths(handle, lambda: on_host(handle, occ, grid, poses, mgrid, fr.PAR, 6, six, None, None)),
          fr.fuse(occ, grid, poses, mgrid, fr.PAR, 6, six), "lock-step")
    # explicit: interleaved, unsorted, skipped frames, and map 2 that no frame names: its shifted input
    mof = [3, 0, -1, 3, 1, 0]
    want = fr.fuse(occ, grid, poses, mgrid, fr.PAR, 4, start, mof, shift)
    for run in (on_host, on_device):
        got = both_paths(handle, lambda: run(handle, occ, grid, poses, mgrid, fr.PAR, 4, start, mof, shift))
        check(got, want, "explicit map_of_frame, %s" % run.__name__)
        assert np.array_equal(got[0][2], fr.shifted(start, mgrid, 4, shift)[2])
    # every frame skipped: the shifted input alone; the order of a map's frames is ascending whatever map_of_frame looks like
    none = on_host(handle, occ, grid, poses, mgrid, fr.PAR, 4, start, [-1] * 6, shift)
    assert np.array_equal(none[0], fr.shifted(start, mgrid, 4, shift))
    L = pwpp_hip.load()
    bad = np.array([0, 4, 0, 0, 0, 0], np.int32)
    with pytest.raises(pwpp_hip.PwppError):
        on_host(handle, occ, grid, poses, mgrid, fr.PAR, 4, start, bad, shift)
    assert b"map_of_frame 1 names map 4" in L.pwpp_last_error()


def test_shifts_null_input_and_in_place(handle):
    NX, NY, nx, ny = 33, 31, 5, 7
    grid, mgrid = (centred(nx, 0.5), centred(ny, 0.5), 0.5), (centred(NX, 0.5), centred(NY, 0.5), 0.5, NX, NY)
    occ = fr.random_occupancy(3, ny, nx, 31, stray=False)
    poses = fr.random_poses(3, 32, 2.0)
    start = np.random.default_rng(33).integers(-300, 500, (3, NY, NX)).astype(np.int16)
    big = 2 ** 31 - 1
    for shift in (None, [(0, 0)] * 3, [(1, 2), (-2, 1), (3, -3)], [(NX, 0), (0, -NY), (NX - 1, 1 - NY)], [(big, 0), (-big - 1, -big - 1), (0, big)]):
        want = fr.fuse(occ, grid, poses, mgrid, fr.PAR, 3, start, None, shift)
        for run in (on_host, on_device):
            check(both_paths(handle, lambda: run(handle, occ, grid, poses, mgrid, fr.PAR, 3, start, None, shift)), want, "shift %s, %s" % (shift, run.__name__))
    # map_in NULL: all zero, whatever the shift
    want = fr.fuse(occ, grid, poses, mgrid, fr.PAR, 3)
    for run in (on_host, on_device):
        check(run(handle, occ, grid, poses, mgrid, fr.PAR, 3, None, None, [(1, 2), (-2, 1), (3, -3)]), want, "null map_in, %s" % run.__name__)
    # in place: map_out == map_in, no shift or a zero one
    want = fr.fuse(occ, grid, poses, mgrid, fr.PAR, 3, start)
    for shift in (None, [(0, 0)] * 3):
        mine = start.copy()
        out, byte = handle.fuse_grid(occ, grid, poses, fmap_of(mgrid, fr.PAR), 3, mine, None, shift, map_out=mine)
        assert out is mine
        check((mine, byte), want, "in place, host")
        check(both_paths(handle, lambda: on_device(handle, occ, grid, poses, mgrid, fr.PAR, 3, start, None, shift, off=1, in_place=True)), want, "in place, device")
    with pytest.raises(pwpp_hip.PwppError):
        mine = start.copy()
        handle.fuse_grid(occ, grid, poses, fmap_of(mgrid, fr.PAR), 3, mine, None, [(0, 0), (0, 1), (0, 0)], map_out=mine)


def test_parameters_at_their_extremes(handle):
    NX, NY, nx, ny = 33, 31, 33, 31
    grid, mgrid = (centred(nx, 0.5), centred(ny, 0.5), 0.5), (centred(NX, 0.5), centred(NY, 0.5), 0.5, NX, NY)
    occ = fr.random_occupancy(5, ny, nx, 41, (0.5, 0.4, 0.1))
    poses = [fr.IDENTITY, fr.rigid(0.2, 0.5, 0.5)] + fr.random_poses(3, 42, 2.0)
    rng = np.random.default_rng(43)
    start = rng.integers(-32768, 32768, (1, NY, NX)).astype(np.int16)  # far outside the clamps: the formulas apply as they stand
    start[0, 0, :4] = (32767, -32768, 32767, -32768)
    for par in ((0, 0, 0, 0, 1, 0), (32767, 32767, -32768, 32767, 32767, -32768), (0, 32767, -32768, 0, 0, -1), (32767, 0, 0, 32767, 32767, 32766),
                (40, 20, -50, 100, -32767, -32768), (1, 1, -1, 1, 1, -1), fr.PAR):
        for map_in in (start, None):
            want = fr.fuse(occ, grid, poses, mgrid, par, 1, map_in)
            check(both_paths(handle, lambda: on_host(handle, occ, grid, poses, mgrid, par, 1, map_in, None, None)), want, "parameters %s" % (par,))
    check(on_device(handle, occ, grid, poses, mgrid, (32767, 32767, -32768, 32767, 32767, -32768), 1, start, None, None, off=1),
          fr.fuse(occ, grid, poses, mgrid, (32767, 32767, -32768, 32767, 32767, -32768), 1, start), "extremes, device")


def test_the_order_example_and_the_composition_of_two_calls(handle):
    g4, m4 = (0.0, 0.0, 1.0), (0.0, 0.0, 1.0, 4, 4)
    start = np.full((1, 4, 4), 340, np.int16)
    hit_miss = np.stack([np.full((4, 4), fr.OCCUPIED, np.int8), np.full((4, 4), fr.FREE, np.int8)])
    for run in (on_host, on_device):
        assert (run(handle, hit_miss, g4, fr.IDENTITY, m4, fr.PAR, 1, start, None, None)[0] == 330).all()
        assert (run(handle, hit_miss[::-1].copy(), g4, fr.IDENTITY, m4, fr.PAR, 1, start, None, None)[0] == 350).all()
    # the same through map_of_frame: it names the map of a frame, never its turn
    two = np.concatenate([hit_miss, hit_miss[::-1]])
    got = on_host(handle, two, g4, fr.IDENTITY, m4, fr.PAR, 2, np.concatenate([start, start]), [1, 1, 0, 0], None)
    assert (got[0][1] == 330).all() and (got[0][0] == 350).all()
    # two calls, the second on the first's output with no shift, are one call over the concatenated frames
    nx, ny, NX, NY = 33, 31, 70, 67
    grid, mgrid = (centred(nx, 0.5), centred(ny, 0.5), 0.5), (centred(NX, 0.25), centred(NY, 0.25), 0.25, NX, NY)
    occ = fr.random_occupancy(7, ny, nx, 51)
    poses = fr.random_poses(7, 52, 3.0)
    mof = [0, 1, 1, 0, -1, 1, 0]
    start = np.random.default_rng(53).integers(-300, 500, (2, NY, NX)).astype(np.int16)
    shift = [(2, -1), (-1, 4)]
    whole = fr.fuse(occ, grid, poses, mgrid, fr.PAR, 2, start, mof, shift)
    for run in (on_host, on_device):
        one = both_paths(handle, lambda: run(handle, occ, grid, poses, mgrid, fr.PAR, 2, start, mof, shift))
        first = run(handle, occ[:3], grid, poses[:3], mgrid, fr.PAR, 2, start, mof[:3], shift)
        second = run(handle, occ[3:], grid, poses[3:], mgrid, fr.PAR, 2, first[0], mof[3:], None)
        check(one, whole, "one call, %s" % run.__name__)
        check(second, whole, "two calls, %s" % run.__name__)


def test_cell_sizes_that_are_no_power_of_two_take_the_division_on_both_paths(handle):
    """Path 0 forms a sample's cell with the reciprocal only where the frame images' cell size is a power of two."""
    NX, NY, nx, ny = 65, 63, 33, 31
    occ = fr.random_occupancy(3, ny, nx, 71)
    for cell, CELL in ((0.3, 0.3), (0.1, 0.07), (3.0, 1.0), (2.0 ** -20, 2.0 ** -20), (2.0, 0.7)):
        grid, mgrid = (centred(nx, cell), centred(ny, cell), cell), (centred(NX, CELL), centred(NY, CELL) + CELL, CELL, NX, NY)
        poses = [fr.IDENTITY, fr.rigid(0.7, 2 * cell, -cell), fr.rigid(-2.0, 0.0, 3 * cell)]
        want = fr.fuse(occ, grid, poses, mgrid)
        assert (want[0] != 0).sum() > 100
        for run in (on_host, on_device):
            check(both_paths(handle, lambda: run(handle, occ, grid, poses, mgrid, fr.PAR, 1, None, None, None)), want, "cells %s / %s, %s" % (cell, CELL, run.__name__))


def test_device_maps_one_halfword_and_bytes_one_byte_off_a_256_byte_boundary(handle):
    for NX, NY, n_maps, nx, ny in ((65, 63, 2, 33, 31), (70, 67, 3, 64, 64)):
        occ, grid, poses, mgrid, mof, map_in, shift, want = case(NX, NY, n_maps, nx, ny, 2, 0, 7)
        assert map_in is not None and shift is not None and mof is not None
        args = (occ, grid, poses, mgrid, fr.PAR, n_maps, map_in, mof, shift)
        aligned = on_device(handle, *args)
        moved = both_paths(handle, lambda: on_device(handle, *args, off=1))
        assert moved[0].tobytes() == aligned[0].tobytes() and moved[1].tobytes() == aligned[1].tobytes()
        check(moved, want, "%dx%dx%d one off" % (NX, NY, n_maps))


# ---- pwpp_fuse_obstacles -------------------------------------------------------------------------------------------------------
def test_fuse_obstacles_is_rasterize_plus_visibility_plus_fuse_grid(kitti):
    nx, ny, cell = 256, 256, 0.5
    x0, y0 = centred(nx, cell), centred(ny, cell)
    mgrid = (-70.0, -66.0, 0.5, 280, 270)
    fm = fmap_of(mgrid, fr.PAR)
    pose = fr.rigid(0.3, 4.2, -1.7)
    L = pwpp_hip.load()
    h = pwpp_hip.Handle()
    g = pwpp_hip.GroundGrid(x0, y0, cell, nx, ny, 0, 0)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out_buf, zero, p6 = np.zeros(mgrid[3] * mgrid[4], np.int16), np.zeros(2, np.float64), np.array(pose, np.float64)
    assert L.pwpp_fuse_obstacles(h._h, ctypes.byref(g), BAND[0], BAND[1], 1, vp(zero), 1, 0, 0, 1, pwpp_hip.MEM_HOST, vp(p6), 1, None, ctypes.byref(fm), 1, None,
                                 None, vp(out_buf), None, None) == E_STATE
    h.set_labels(True)  # (_everything reads them)
    h.estimate_ground(kitti[0])
    before = _everything(h, 1)
    rc = h.rasterize_obstacles(x0, y0, cell, nx, ny, *BAND, want_top=False)
    start = np.random.default_rng(61).integers(-100, 100, (1, mgrid[4], mgrid[3])).astype(np.int16)
    shift = [(3, -2)]
    for min_count, max_range in ((1, 40), (2, 0)):
        what = "min_count %d, max_range %d" % (min_count, max_range)
        _, vocc = h.visibility_grid(rc, (nx // 2, ny // 2), min_count, max_range)  # {0, 0} m is the cell (nx / 2, ny / 2) of this grid
        vo = h.visibility_obstacles(x0, y0, cell, nx, ny, *BAND, (0.0, 0.0), min_count, max_range)
        steps = h.fuse_grid(vocc, (x0, y0, cell), pose, fm, 1, start, None, shift)
        got = both_paths(h, lambda: h.fuse_obstacles(x0, y0, cell, nx, ny, *BAND, pose, fm, 1, start, (0.0, 0.0), min_count, max_range, shift=shift,
                                                     want_frames=True))
        assert got[2].tobytes() == vocc.tobytes() == vo[1].tobytes(), what + ": the per-frame bytes differ from the visibility's"
        assert got[0].tobytes() == steps[0].tobytes() and got[1].tobytes() == steps[1].tobytes(), what + ": differs from the three steps"
        kept = h.fuse_obstacles(x0, y0, cell, nx, ny, *BAND, pose, fm, 1, start, (0.0, 0.0), min_count, max_range, shift=shift)  # the bytes kept in the handle
        assert kept[0].tobytes() == got[0].tobytes() and kept[1].tobytes() == got[1].tobytes(), what
        check(got[:2], fr.fuse(vocc, (x0, y0, cell), pose, mgrid, fr.PAR, 1, start, None, shift), what)
    assert all((got[1] == v).sum() > 100 for v in (fr.FREE, fr.OCCUPIED, fr.UNKNOWN))
    # into device memory, the maps one halfword / the bytes one byte off a 256-byte boundary, the frames' bytes kept and asked for
    import torch
    cells = mgrid[3] * mgrid[4]
    dmaps = [torch.full((cells + 256,), -7, dtype=torch.int16, device="cuda") for _ in range(2)]
    dbyte = torch.full((cells + 512,), -7, dtype=torch.int8, device="cuda")
    docc = torch.full((nx * ny + 512,), -7, dtype=torch.int8, device="cuda")
    dmaps[0][1:1 + cells] = torch.from_numpy(start.reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    for occ_ptr in (0, docc.data_ptr() + 1):
        h.fuse_obstacles_device(x0, y0, cell, nx, ny, *BAND, pose, fm, 1, dmaps[0].data_ptr() + 2, dmaps[1].data_ptr() + 2, dbyte.data_ptr() + 1, occ_ptr,
                                (0.0, 0.0), 2, 0, shift=shift)
        h.synchronize()
        raw = [dmaps[1].cpu().numpy(), dbyte.cpu().numpy()]
        assert raw[0][1:1 + cells].tobytes() == got[0].tobytes() and raw[1][1:1 + cells].tobytes() == got[1].tobytes()
        for r in raw:
            assert (r[:1] == -7).all() and (r[1 + cells:] == -7).all()
    rocc = docc.cpu().numpy()
    assert rocc[1:1 + nx * ny].tobytes() == vocc.tobytes() and rocc[0] == -7 and (rocc[1 + nx * ny:] == -7).all()
    assert _everything(h, 1) == before, "the fusion changed the results of the call it reads"


def test_three_frames_as_a_sequence_and_in_lock_step():
    frames = three_frames()  # a 16-beam scan, an empty frame, a frame that is all unref
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    grid = (-16.0, -16.0, 0.5, 64, 64)
    mgrid = (-20.0, -18.0, 0.5, 80, 72)
    fm = fmap_of(mgrid, fr.PAR)
    xy = np.array([[0.0, 0.0], [3.3, -2.1], [-15.9, 15.9]])
    poses = [fr.rigid(0.1 * f, 0.5 * f, -0.25 * f) for f in range(3)]
    _, vocc = h.visibility_obstacles(*grid, *BAND, xy)
    seq = both_paths(h, lambda: h.fuse_obstacles(*grid, *BAND, poses, fm, 1, None, xy))
    check(seq, fr.fuse(vocc, grid[:3], poses, mgrid), "three frames into one map")
    lock = both_paths(h, lambda: h.fuse_obstacles(*grid, *BAND, poses, fm, 3, None, xy))
    check(lock, fr.fuse(vocc, grid[:3], poses, mgrid, fr.PAR, 3), "three frames into three maps")
    assert (lock[0][0] > 0).sum() >= 3 and (lock[0][1:] <= 0).all()  # the empty and the all-unref frame hold no obstacle
    sub = h.fuse_obstacles(*grid, *BAND, poses[1:], fm, 2, None, xy[1:], frame_first=1, frames=2)  # entry i belongs to frame frame_first + i
    assert sub[0].tobytes() == lock[0][1:].tobytes() and sub[1].tobytes() == lock[1][1:].tobytes()


def test_two_device_calls_back_to_back_each_fuse_under_their_own_tables():
    """The origins and the poses of a call are uploaded from the handle's own copy, and the second call replaces that copy while
    the first may still be in flight: two calls with an origin and a pose per frame, different ones, into different maps, one
    synchronize() after both."""
    import torch
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(three_frames(), mode=pwpp_hip.MODE_FRESH)
    grid = (-16.0, -16.0, 0.5, 64, 64)
    mgrid = (-20.0, -18.0, 0.5, 80, 72)
    fm = fmap_of(mgrid, fr.PAR)
    calls = [(np.array([[0.0, 0.0], [3.3, -2.1], [-15.9, 15.9]]), [fr.rigid(0.1 * f, 0.5 * f, -0.25 * f) for f in range(3)]),
             (np.array([[-4.2, 1.1], [0.0, 0.0], [2.5, 2.5]]), [fr.rigid(-0.3 - 0.2 * f, 1.5 - f, 0.75 * f) for f in range(3)])]
    want = [fr.fuse(h.visibility_obstacles(*grid, *BAND, xy)[1], grid[:3], poses, mgrid, fr.PAR, 3) for xy, poses in calls]
    assert want[0][0].tobytes() != want[1][0].tobytes() and (want[0][0][0] > 0).sum() >= 3
    cells = 3 * mgrid[3] * mgrid[4]
    out = [(torch.full((cells,), -7, dtype=torch.int16, device="cuda"), torch.full((cells,), -7, dtype=torch.int8, device="cuda")) for _ in calls]
    torch.cuda.synchronize()
    for (xy, poses), (dmap, dbyte) in zip(calls, out):
        h.fuse_obstacles_device(*grid, *BAND, poses, fm, 3, 0, dmap.data_ptr(), dbyte.data_ptr(), 0, xy)
    h.synchronize()
    for i, (dmap, dbyte) in enumerate(out):
        check((dmap.cpu().numpy().reshape(want[i][0].shape), dbyte.cpu().numpy().reshape(want[i][1].shape)), want[i], "call %d of two" % i)


# ---- workspace ------------------------------------------------------------------------------------------------------------------
def test_workspace_and_that_nothing_else_moves():
    h = pwpp_hip.Handle()
    empty = h.workspace_bytes()
    occ, grid, poses, mgrid, mof, map_in, shift, want = case(65, 63, 2, 33, 31, 2, 0, 7)
    check(on_host(h, occ, grid, poses, mgrid, fr.PAR, 2, map_in, mof, shift), want, "before any estimate call")
    grown = h.workspace_bytes()
    # the poses, lists and shifts, the staged frames, both maps and the byte in words
    assert grown >= empty + 4 * (12 * len(poses) + 3 + 4 + occ.size // 4 + 2 * (2 * 65 * 63 // 2) + 2 * 65 * 63 // 4), "the cluster buffer is not counted"
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
    b.fuse_obstacles(-20.0, -20.0, 0.5, 80, 80, *BAND, fr.IDENTITY, fmap_of((-20.0, -20.0, 0.5, 80, 80), fr.PAR), 3)
    assert b.workspace_bytes() >= a.workspace_bytes() + 4 * (2 * 3 * 80 * 80 + 3 * 80 * 80 // 4)  # the kept count, first and byte images
    assert _everything(b, 3) == before and b.time_us() == t_before, "the fusion changed the results of the call it reads"
    for w in (a, b):
        w.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert _everything(b, 3) == _everything(a, 3), "an estimate call after a fusion call differs from one without"
    b.trim_workspace()
    a.trim_workspace()
    assert a.workspace_bytes() == b.workspace_bytes()
    with pytest.raises(pwpp_hip.PwppError):
        h.set_option("fusion_path", 2)


def test_pybind_module_agrees_with_the_ctypes_handle():
    import pypatchworkpp
    from test_gpu_obstacle_grid import small_cloud
    pp = pypatchworkpp.patchworkpp(pypatchworkpp.Parameters())
    h = pwpp_hip.Handle()
    m = pypatchworkpp.FusedObstacleMap()
    m.x0, m.y0, m.cell, m.nx, m.ny = -32.0, -14.0, 0.5, 130, 56
    pose = fr.rigid(0.2, 1.0, -0.5)
    with pytest.raises(RuntimeError):
        pp.updateObstacleMap(m, pose, -30.0, -12.0, 0.5, 120, 48, 0.2, 2.5)  # no frame yet
    assert (m.x0, m.y0) == (-32.0, -14.0)
    pts = small_cloud(5)
    pp.estimateGround(pts)
    h.estimate_ground(pts)
    fm = fmap_of((-32.0, -14.0, 0.5, 130, 56), fr.PAR)
    L1, b1 = pp.updateObstacleMap(m, pose, -30.0, -12.0, 0.5, 120, 48, 0.2, 2.5)
    h1 = h.fuse_obstacles(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5, pose, fm)
    assert L1.dtype == np.int16 and b1.dtype == np.int8 and L1.shape == b1.shape == (56, 130) and (L1 > 0).sum() >= 3
    assert L1.tobytes() == h1[0][0].tobytes() and b1.tobytes() == h1[1][0].tobytes()
    # the second update rolls the map two cells east and one south: the map's origin moves with it
    L2, b2 = pp.updateObstacleMap(m, pose, -30.0, -12.0, 0.5, 120, 48, 0.2, 2.5, 2, 30, 2.2, -1.1, 2, -1)
    assert (m.x0, m.y0) == (-31.0, -14.5)
    fm2 = fmap_of((-31.0, -14.5, 0.5, 130, 56), fr.PAR)
    h2 = h.fuse_obstacles(-30.0, -12.0, 0.5, 120, 48, 0.2, 2.5, pose, fm2, 1, h1[0], (2.2, -1.1), 2, 30, shift=[(2, -1)])
    assert L2.tobytes() == h2[0][0].tobytes() and b2.tobytes() == h2[1][0].tobytes()
