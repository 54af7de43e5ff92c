"""No-GPU checks of the occupancy fusion (pwpp_fuse_grid, pwpp_fuse_obstacles): the exports, the feature macro, the size of
pwpp_fusion_map, the ctypes prototypes and the bindings' methods, every argument check that needs no device with its message and
its place in the order, the C++ mirror in both flavours -- the properties of the restatement the GPU tests compare against
(tests/occupancy_fusion_ref.py): lossless whole-cell translations and quarter turns, the four-sample guarantee under 200 rigid
poses and what centre sampling would lose, the order example, the composition of two calls, both clamps -- and the stand-alone
program that runs the kernel's functions on the host against a brute force of its own (tools/fusion_check.cpp), built with the
address and undefined-behaviour sanitizers where the toolchain has them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import occupancy_fusion_ref as fr
import pwpp_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")
E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pwpp_hip.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "lib/libpwpp_hip.so"], check=True, stdout=subprocess.DEVNULL)
    return pwpp_hip.load()


def test_symbols_macro_struct_and_prototypes(lib):
    hdr = open(os.path.join(ROOT, "include", "pwpp.h")).read()
    for name in ("pwpp_fuse_grid", "pwpp_fuse_obstacles"):
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr
    assert "#define PWPP_HAS_OCCUPANCY_FUSION 1" in hdr
    assert "#define PWPP_VERSION_MINOR 4 " in hdr
    assert '"fusion_path"' in hdr and "typedef struct pwpp_fusion_map {" in hdr
    assert ctypes.sizeof(pwpp_hip.FusionMap) == 56
    assert [f[0] for f in pwpp_hip.FusionMap._fields_] == ["x0", "y0", "cell", "nx", "ny", "hit", "miss", "l_min", "l_max", "occupied_at", "free_at"]
    assert len(lib.pwpp_fuse_grid.argtypes) == 14 and len(lib.pwpp_fuse_obstacles.argtypes) == 21
    assert lib.pwpp_fuse_obstacles.argtypes[2] is ctypes.c_float and lib.pwpp_fuse_obstacles.argtypes[3] is ctypes.c_float
    for name in ("fuse_grid", "fuse_grid_device", "fuse_obstacles", "fuse_obstacles_device"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    import pypatchworkpp
    assert hasattr(pypatchworkpp.patchworkpp, "updateObstacleMap")
    m = pypatchworkpp.FusedObstacleMap()
    assert (m.hit, m.miss, m.l_min, m.l_max, m.occupied_at, m.free_at) == (40, 20, -200, 350, 60, -40)


def fusion_map(**kw):
    f = dict(x0=-2.0, y0=-2.0, cell=1.0, nx=4, ny=4, hit=40, miss=20, l_min=-200, l_max=350, occupied_at=60, free_at=-40)
    f.update(kw)
    return pwpp_hip.FusionMap(**f)


def test_every_argument_is_named_before_the_device_is_touched_and_in_order(lib):
    occ = np.zeros(64, np.int8)
    maps = np.zeros(64, np.int16)    # map_in
    out = np.zeros(64, np.int16)
    byte = np.zeros(64, np.int8)
    pose = np.array(fr.IDENTITY * 4, np.float64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    at = lambda a, n: ctypes.c_void_p(a.ctypes.data + n)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    H = pwpp_hip.MEM_HOST
    err = lib.pwpp_last_error
    g = pwpp_hip.GroundGrid(-2.0, -2.0, 1.0, 4, 4, 0, 0)
    fm = fusion_map()

    def grid(h=fake, gr=ctypes.byref(g), frames=1, mem=H, occupancy=vp(occ), pose=vp(pose), n_poses=1, mof=None, m=ctypes.byref(fm), n_maps=1, shift=None,
             map_in=vp(maps), map_out=vp(out), map_occ=vp(byte)):
        return lib.pwpp_fuse_grid(h, gr, frames, mem, occupancy, pose, n_poses, mof, m, n_maps, shift, map_in, map_out, map_occ)

    def G(**kw):
        return ctypes.byref(pwpp_hip.GroundGrid(**dict(dict(x0=-2.0, y0=-2.0, cell=1.0, nx=4, ny=4, flags=0, pad_=0), **kw)))

    M = lambda **kw: ctypes.byref(fusion_map(**kw))
    # 1 null pointers
    assert grid(h=None) == E_ARG and b"null handle" in err()
    assert grid(gr=None) == E_ARG and b"null grid" in err()
    assert grid(occupancy=None) == E_ARG and b"null occupancy" in err()
    assert grid(pose=None) == E_ARG and b"null pose" in err()
    assert grid(m=None) == E_ARG and b"null map description" in err()
    assert grid(map_out=None) == E_ARG and b"null map_out" in err()
    # 2 the frame images: frames and sides < 1, sides > 32768, the cells beyond 2^31
    for kw in (dict(frames=0), dict(gr=G(nx=0)), dict(gr=G(ny=-1))):
        assert grid(**kw) == E_ARG and b"cells" in err(), kw
    for kw in (dict(nx=32769), dict(ny=32769)):
        assert grid(gr=G(**kw)) == E_ARG and b"32768 a side" in err(), kw
    assert grid(gr=G(nx=32768, ny=32768), frames=3, n_poses=3) == E_ARG and b"exceed 2^31" in err()
    # 3 the same of the maps
    for kw in (dict(n_maps=0), dict(m=M(nx=0)), dict(m=M(ny=0))):
        assert grid(**kw) == E_ARG and b"cells" in err(), kw
    for kw in (dict(nx=32769), dict(ny=40000)):
        assert grid(m=M(**kw)) == E_ARG and b"32768 a side" in err(), kw
    assert grid(m=M(nx=32768, ny=32768), n_maps=3) == E_ARG and b"exceed 2^31" in err()
    # 4 the cell sizes, 5 the flags
    for c in (0.0, -1.0, np.nan, np.inf):
        assert grid(gr=G(cell=c)) == E_ARG and b"finite and positive" in err(), c
        assert grid(m=M(cell=c)) == E_ARG and b"finite and positive" in err(), c
    assert grid(gr=G(flags=1)) == E_ARG and b"grid flags 1" in err()
    # 6 the parameters' ranges
    for kw in (dict(hit=-1), dict(hit=32768), dict(miss=-1), dict(miss=32768)):
        assert grid(m=M(**kw)) == E_ARG and b"0 .. 32767 expected" in err(), kw
    for kw in (dict(l_min=-32769), dict(l_min=1), dict(l_max=-1), dict(l_max=32768)):
        assert grid(m=M(**kw)) == E_ARG and b"clamps" in err(), kw
    for kw in (dict(free_at=-32769), dict(occupied_at=32768), dict(free_at=60, occupied_at=60), dict(free_at=10, occupied_at=0)):
        assert grid(m=M(**kw)) == E_ARG and b"thresholds" in err(), kw
    assert grid(m=M(hit=0, miss=32767, l_min=-32768, l_max=32767, free_at=-32768, occupied_at=32767), mem=2) == E_ARG and b"PWPP_MEM_HOST or" in err()
    # 7 the poses, 8 map_of_frame
    for n in (0, 2, -1):
        assert grid(n_poses=n) == E_ARG and b"poses for 1 frames" in err(), n
    assert grid(frames=4, n_poses=3) == E_ARG and b"3 poses for 4 frames" in err()
    assert grid(frames=3, n_maps=2) == E_ARG and b"null map_of_frame with 2 maps for 3 frames" in err()
    for bad, where in (([0, 1, 2], b"map_of_frame 2 names map 2"), ([0, -2, 1], b"map_of_frame 1 names map -2")):
        assert grid(frames=3, n_maps=2, mof=vp(np.array(bad, np.int32))) == E_ARG and where in err(), bad
    # 9 the overlaps
    zero, moved = np.zeros(2, np.int32), np.array([0, 1], np.int32)
    assert grid(map_out=vp(maps), shift=vp(moved)) == E_ARG and b"map_out == map_in with a shift" in err()
    assert grid(map_out=at(maps, 2)) == E_ARG and b"map_in and map_out overlap" in err()
    assert grid(map_out=at(maps, 30)) == E_ARG and b"map_in and map_out overlap" in err()
    assert grid(map_occ=at(out, 31)) == E_ARG and b"map_occupancy overlaps map_out" in err()
    assert grid(map_occ=at(maps, 0)) == E_ARG and b"map_occupancy overlaps map_in" in err()
    # 10 mem -- and with it: equal maps without a shift, a null or zero shift, touching ranges are all accepted up to here
    assert grid(mem=2) == E_ARG and b"PWPP_MEM_HOST or PWPP_MEM_DEVICE" in err()   # PWPP_MEM_HOST_PINNED
    assert grid(map_out=vp(maps), mem=2) == E_ARG and b"PWPP_MEM_HOST or" in err()
    assert grid(map_out=vp(maps), shift=vp(zero), mem=2) == E_ARG and b"PWPP_MEM_HOST or" in err()
    assert grid(map_out=at(maps, 32), map_occ=at(maps, 64), mem=2) == E_ARG and b"PWPP_MEM_HOST or" in err()
    assert grid(map_in=None, map_occ=None, mem=7) == E_ARG and b"mem 7" in err()
    assert grid(pose=vp(np.full(6, np.nan)), mem=2) == E_ARG and b"PWPP_MEM_HOST or" in err()   # a pose that is not finite is no error
    # the order
    assert grid(occupancy=None, frames=0) == E_ARG and b"null occupancy" in err()
    assert grid(frames=0, n_maps=0) == E_ARG and b"0 frames of 4 x 4" in err()
    assert grid(gr=G(nx=32769), m=M(nx=0)) == E_ARG and b"32768 a side" in err()
    assert grid(n_maps=0, gr=G(cell=0.0)) == E_ARG and b"0 frames of 4 x 4" in err()   # (the maps' own "frames" are the maps)
    assert grid(gr=G(cell=0.0, flags=1)) == E_ARG and b"grid flags" in err()  # the frame grid's own checks come before the map's
    assert grid(m=M(cell=0.0, hit=-1)) == E_ARG and b"finite and positive" in err()
    assert grid(m=M(hit=-1, l_min=1)) == E_ARG and b"0 .. 32767" in err()
    assert grid(m=M(l_min=1, free_at=99)) == E_ARG and b"clamps" in err()
    assert grid(m=M(free_at=99), n_poses=2) == E_ARG and b"thresholds" in err()
    assert grid(n_poses=2, frames=3, n_maps=2) == E_ARG and b"poses for" in err()
    assert grid(frames=3, n_poses=3, n_maps=2, map_out=vp(maps), shift=vp(moved)) == E_ARG and b"null map_of_frame" in err()
    assert grid(map_out=vp(maps), shift=vp(moved), mem=2) == E_ARG and b"with a shift" in err()

    zero2 = np.zeros(2, np.float64)

    def obstacles(h=fake, gr=ctypes.byref(g), band=(0.2, 2.5), min_count=1, origin=vp(zero2), n_origins=1, max_range=0, frames=1, pose=vp(pose), n_poses=1,
                  mof=None, m=ctypes.byref(fm), n_maps=1, shift=None, map_out=vp(out)):
        return lib.pwpp_fuse_obstacles(h, gr, band[0], band[1], min_count, origin, n_origins, max_range, 0, frames, H, pose, n_poses, mof, m, n_maps, shift,
                                       vp(maps), map_out, None, None)

    assert obstacles(h=None) == E_ARG and b"null handle" in err()
    assert obstacles(gr=None) == E_ARG and b"null grid" in err()
    assert obstacles(origin=None) == E_ARG and b"null origin" in err()
    assert obstacles(pose=None) == E_ARG and b"null pose" in err()
    assert obstacles(m=None) == E_ARG and b"null map description" in err()
    assert obstacles(map_out=None) == E_ARG and b"null map_out" in err()
    # everything pwpp_visibility_obstacles rejects, first
    assert obstacles(band=(2.5, 0.2)) == E_ARG and b"height band" in err()
    assert obstacles(gr=G(flags=2)) == E_ARG and b"grid flags" in err()
    for kw in (dict(nx=0), dict(cell=0.0), dict(cell=np.nan), dict(x0=np.inf)):
        assert obstacles(gr=G(**kw)) == E_ARG and (b"grid of" in err() or b"finite" in err()), kw
    assert obstacles(gr=G(nx=32769)) == E_ARG and b"32768 a side" in err()
    assert obstacles(min_count=0) == E_ARG and b"min_count" in err()
    assert obstacles(max_range=32769) == E_ARG and b"max_range" in err()
    assert obstacles(n_origins=2) == E_ARG and b"2 origins for 1 frames" in err()
    assert obstacles(origin=vp(np.array((2.0, 0.0)))) == E_ARG and b"origin 0" in err() and b"outside the grid" in err()
    assert obstacles(origin=vp(np.array((np.nan, 0.0)))) == E_ARG and b"not finite" in err()
    # then the map's
    assert obstacles(frames=0, n_origins=1) == E_ARG and b"0 frames" in err()
    assert obstacles(n_maps=0) == E_ARG and b"cells" in err()
    assert obstacles(m=M(cell=-1.0)) == E_ARG and b"finite and positive" in err()
    assert obstacles(m=M(hit=40000)) == E_ARG and b"0 .. 32767" in err()
    assert obstacles(n_poses=2) == E_ARG and b"2 poses for 1 frames" in err()
    assert obstacles(mof=vp(np.array([1], np.int32))) == E_ARG and b"map_of_frame 0 names map 1" in err()
    assert obstacles(map_out=vp(maps), shift=vp(moved)) == E_ARG and b"with a shift" in err()
    assert obstacles(min_count=0, m=M(hit=-1)) == E_ARG and b"min_count" in err()


CPP = r"""
#include "patchwork/patchworkpp.h"
#ifndef PWPP_HAS_OCCUPANCY_FUSION
#error "include/pwpp.h does not announce the occupancy fusion"
#endif
static_assert(sizeof(pwpp_fusion_map) == 56, "pwpp_fusion_map");
double use(patchwork::PatchWorkpp &pw) {
    patchwork::PatchWorkpp::FusedObstacleMap map;
    map.x0 = -64.0, map.y0 = -64.0, map.cell = 0.5, map.nx = 256, map.ny = 256;
    const double pose[6] = {1.0, 0.0, 3.0, 0.0, 1.0, -1.5};
    pw.updateObstacleMap(map, pose, -40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f);
    pw.updateObstacleMap(map, pose, -40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f, 2, 40, 1.5, -0.5, 2, -1);
    return map.log_odds[3 * 256 + 5] + map.occupancy[7] + map.x0 + (double)map.log_odds.size() + (map.occupancy[0] == PWPP_OCC_UNKNOWN ? 1.0 : 0.0);
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_method_compiles(tmp_path, flavour):
    src = tmp_path / "occupancy_fusion.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    cmd += ["-DPWPP_NO_EIGEN"] if flavour == "plain" else ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "fusion.c"
    src.write_text('#include "pwpp.h"\nint f(const pwpp_fusion_map *m) { return pwpp_fuse_grid(0, 0, 1, PWPP_MEM_HOST, 0, 0, 1, 0, m, 1, 0, 0, 0, 0) + '
                   'pwpp_fuse_obstacles(0, 0, 0.f, 1.f, 1, 0, 1, 0, 0, 1, PWPP_MEM_HOST, 0, 1, 0, m, 1, 0, 0, 0, 0, 0) + (int)sizeof(*m); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# ---- the restatement itself ---------------------------------------------------------------------------------------------------
GRID = (-16.0, -16.0, 0.5)
MGRID = (-16.0, -16.0, 0.5, 64, 64)


def single_update(occ, par=fr.PAR):
    """What one frame adds to a zero map where every sample falls into the one cell `occ`."""
    return np.where(occ == fr.OCCUPIED, min(par[0], par[3]), np.where(occ == fr.FREE, max(-par[1], par[2]), 0)).astype(np.int16)


def test_a_whole_cell_translation_is_the_shifted_add():
    occ = fr.random_occupancy(1, 64, 64, 1)
    got, byte = fr.fuse(occ, GRID, (1, 0, 1.5, 0, 1, -2.0), MGRID)   # +3 cells in x, -4 in y
    src = single_update(occ[0])
    want = np.zeros((64, 64), np.int16)
    want[:60, 3:] = src[4:, :61]
    assert np.array_equal(got[0], want)
    assert np.array_equal(byte[0], np.where(want >= 60, 100, np.where(want <= -40, 0, -1)))   # (-20 is above free_at: unknown)
    assert (got[0][want == 0] == 0).all() and (src == 40).sum() > 300 and (src == -20).sum() > 1500


def test_a_quarter_turn_is_rot90():
    occ = fr.random_occupancy(1, 64, 64, 2)
    # frame (x, y) -> map (-y, x): counter-clockwise in x-y; rows are y, so in array terms out[jy, jx] = src[63 - jx, jy]: rot90(-1)
    got, _ = fr.fuse(occ, GRID, (0, -1, 0, 1, 0, 0), MGRID)
    assert np.array_equal(got[0], np.rot90(single_update(occ[0]), -1))
    got, _ = fr.fuse(occ, GRID, (0, 1, 0, -1, 0, 0), MGRID)
    assert np.array_equal(got[0], np.rot90(single_update(occ[0]), 1))


def marked_by(pose, mgrid, offsets, grid=GRID, n=64):
    """For every frame cell: does it mark a map cell when it alone is occupied -- computed at once: the frame's bytes are read
    through a sampler that returns the cell index."""
    X0, Y0, CELL, NX, NY = mgrid
    jy, jx = np.mgrid[0:NY, 0:NX]
    tags = np.arange(n * n, dtype=np.int64).reshape(n, n)
    hit = np.zeros(n * n + 1, bool)
    for oy in offsets:
        for ox in offsets:
            s = sample_tags(tags, grid, pose, X0 + (jx + ox) * CELL, Y0 + (jy + oy) * CELL)
            hit[s.reshape(-1)] = True
    return hit[:-1].reshape(n, n)


def sample_tags(tags, grid, pose, mx, my):
    x0, y0, cell = grid
    ny, nx = tags.shape
    a, b, tx, c, d, ty = pose
    dx, dy = mx - tx, my - ty
    u, v = ((a * dx + c * dy) - x0) / cell, ((b * dx + d * dy) - y0) / cell
    inside = (u >= 0) & (u < nx) & (v >= 0) & (v < ny)
    return np.where(inside, tags[np.where(inside, np.floor(v), 0).astype(int), np.where(inside, np.floor(u), 0).astype(int)], nx * ny)


def discs_inside(pose, mgrid, grid=GRID, n=64):
    """The frame cells whose circumscribed disc (radius cell / sqrt 2 about the centre) lies inside the map under the pose."""
    x0, y0, cell = grid
    X0, Y0, CELL, NX, NY = mgrid
    iy, ix = np.mgrid[0:n, 0:n]
    cx, cy = x0 + (ix + 0.5) * cell, y0 + (iy + 0.5) * cell
    a, b, tx, c, d, ty = pose
    px, py = a * cx + b * cy + tx, c * cx + d * cy + ty
    r = cell * np.sqrt(0.5) + 1e-9
    return (px - r >= X0) & (px + r <= X0 + NX * CELL) & (py - r >= Y0) & (py + r <= Y0 + NY * CELL)


def test_four_samples_lose_no_occupied_cell_under_200_rigid_poses_and_the_centre_does():
    checked = 0
    for i, pose in enumerate(fr.random_poses(200, 11, 6.0)):
        mgrid = MGRID if i % 2 == 0 else (-16.0, -16.0, 0.25, 128, 128)   # CELL == cell and CELL < cell
        inside = discs_inside(pose, mgrid)
        marked = marked_by(pose, mgrid, fr.QUADRANTS)
        assert marked[inside].all(), "pose %d %s: %d occupied frame cells inside the map mark no map cell" % (i, pose, (inside & ~marked).sum())
        checked += int(inside.sum())
    assert checked > 200 * 1500   # (the test looked at cells: most of every frame lies inside)
    # the marking agrees with the restatement itself: one occupied cell marks a map cell
    pose = fr.rigid(np.pi / 4, 0.3, -0.2)
    occ = np.full((1, 64, 64), fr.UNKNOWN, np.int8)
    occ[0, 20, 33] = fr.OCCUPIED
    assert (fr.fuse(occ, GRID, pose, MGRID)[0] > 0).any() and marked_by(pose, MGRID, fr.QUADRANTS)[20, 33]
    # centre sampling at 45 degrees: about 17.7 % of the interior cells lie under no centre
    inside = discs_inside(pose, MGRID)
    lost = ~marked_by(pose, MGRID, (0.5,)) & inside
    assert 0.15 < lost.sum() / inside.sum() < 0.20, lost.sum() / inside.sum()
    iy, ix = np.argwhere(lost)[0]
    occ = np.full((1, 64, 64), fr.UNKNOWN, np.int8)
    occ[0, iy, ix] = fr.OCCUPIED
    assert not fr.fuse(occ, GRID, pose, MGRID, offsets=(0.5,))[0].any() and (fr.fuse(occ, GRID, pose, MGRID)[0] == 40).any()


def test_the_order_matters_exactly_as_the_contract_says():
    g4, m4 = (0.0, 0.0, 1.0), (0.0, 0.0, 1.0, 4, 4)
    start = np.full((1, 4, 4), 340, np.int16)
    hit_miss = np.stack([np.full((4, 4), fr.OCCUPIED, np.int8), np.full((4, 4), fr.FREE, np.int8)])
    assert (fr.fuse(hit_miss, g4, fr.IDENTITY, m4, map_in=start)[0] == 330).all()
    assert (fr.fuse(hit_miss[::-1], g4, fr.IDENTITY, m4, map_in=start)[0] == 350).all()


def test_two_calls_compose_to_one():
    occ = fr.random_occupancy(5, 31, 33, 3)
    grid, mgrid = (-8.0, -8.0, 0.5), (-9.0, -7.0, 0.5, 40, 37)
    poses = fr.random_poses(5, 4, 3.0)
    start = np.random.default_rng(5).integers(-300, 500, (1, 37, 40)).astype(np.int16)   # outside the clamps too
    whole = fr.fuse(occ, grid, poses, mgrid, map_in=start, shift=[(2, -1)])
    first = fr.fuse(occ[:2], grid, poses[:2], mgrid, map_in=start, shift=[(2, -1)])
    second = fr.fuse(occ[2:], grid, poses[2:], mgrid, map_in=first[0])
    assert np.array_equal(second[0], whole[0]) and np.array_equal(second[1], whole[1])
    assert not np.array_equal(first[0], whole[0])


def test_both_clamps_saturate_and_inputs_outside_them_follow_the_formulas():
    g1, m1 = (0.0, 0.0, 1.0), (0.0, 0.0, 1.0, 2, 1)
    par = (40, 20, -50, 100, 60, -40)
    occ = np.zeros((12, 1, 2), np.int8)
    occ[:, 0, 0] = fr.OCCUPIED
    L, byte = fr.fuse(occ, g1, fr.IDENTITY, m1, par)
    assert L[0, 0].tolist() == [100, -50] and byte[0, 0].tolist() == [100, 0]
    # above l_max a hit pulls down to l_max, a miss subtracts; below l_min a miss pulls up to l_min, a hit adds
    start = np.array([[[500, 500]]], np.int16)
    assert fr.fuse(occ[:1], g1, fr.IDENTITY, m1, par, map_in=start)[0][0, 0].tolist() == [100, 480]
    start = np.array([[[-500, -500]]], np.int16)
    assert fr.fuse(occ[:1], g1, fr.IDENTITY, m1, par, map_in=start)[0][0, 0].tolist() == [-460, -50]
    wide = (32767, 32767, -32768, 32767, 32767, -32768)
    L, byte = fr.fuse(occ[:3], g1, fr.IDENTITY, m1, wide)
    assert L[0, 0].tolist() == [32767, -32768] and byte[0, 0].tolist() == [100, 0]


# ---- the kernel's functions on the host ----------------------------------------------------------------------------------------
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def sanitizers_work(tmp_path):
    """The toolchain links the two runtimes into a program and that program starts in this environment."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        return False
    return subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0


def test_fusion_program_builds_and_passes(tmp_path):
    exe = tmp_path / "fusion_check"
    flags = SANITIZE if sanitizers_work(tmp_path) else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off"] + flags +
                   ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "fusion_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)  # (a stand-alone child process with its own main)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
    assert int(r.stdout.split("fusion_check: ")[1].split(" cases")[0]) >= 3000
