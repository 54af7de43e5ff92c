"""No-GPU checks of the elevation fusion (pwpp_fuse_height_grid, pwpp_fuse_ground): the exports, the feature macro, the size of
pwpp_height_map, the ctypes prototypes and the bindings' methods, every argument check that needs no device with its message and
its place in the order, the C++ mirror in both flavours -- the properties of the restatement the GPU tests compare against
(tests/elevation_fusion_ref.py): lossless whole-cell translations and quarter turns, the mean of k equal heights below and beyond
n_max, order-freedom below n_max and the order examples above it, the composition of two calls, shifts larger than the map, the
normalisation of out-of-range inputs, the ties, limits and non-finite values of the observation -- and the stand-alone program that
runs the kernel's functions on the host against a brute force of its own and proves the invariant and the multiply-shift
(tools/elevation_check.cpp), built with the address and undefined-behaviour sanitizers where the toolchain has them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import elevation_fusion_ref as er
import pwpp_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")
E_ARG = -1
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pwpp_hip.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "lib/libpwpp_hip.so"], check=True, stdout=subprocess.DEVNULL)
    return pwpp_hip.load()


def test_symbols_macro_struct_and_prototypes(lib):
    hdr = open(os.path.join(ROOT, "include", "pwpp.h")).read()
    for name in ("pwpp_fuse_height_grid", "pwpp_fuse_ground"):
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr
    assert "#define PWPP_HAS_ELEVATION_FUSION 1" in hdr
    assert "#define PWPP_VERSION_MINOR 4 " in hdr
    assert '"elevation_path"' in hdr and "typedef struct pwpp_height_map {" in hdr
    assert hdr.index("pwpp_match_pose(") < hdr.index("PWPP_HAS_ELEVATION_FUSION")  # declared after the scan match
    assert ctypes.sizeof(pwpp_hip.HeightMap) == 40
    assert [f[0] for f in pwpp_hip.HeightMap._fields_] == ["x0", "y0", "cell", "nx", "ny", "n_max", "pad_"]
    assert len(lib.pwpp_fuse_height_grid.argtypes) == 17 and len(lib.pwpp_fuse_ground.argtypes) == 18
    for name in ("fuse_height_grid", "fuse_height_grid_device", "fuse_ground", "fuse_ground_device"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    import pypatchworkpp
    assert hasattr(pypatchworkpp.patchworkpp, "updateElevationMap") and hasattr(pypatchworkpp.patchworkpp, "getFusedElevation")
    m = pypatchworkpp.FusedElevationMap()
    assert m.n_max == 16 and (m.nx, m.ny) == (0, 0)


def height_map(**kw):
    f = dict(x0=-2.0, y0=-2.0, cell=1.0, nx=4, ny=4, n_max=8, pad_=0)
    f.update(kw)
    return pwpp_hip.HeightMap(**f)


def test_every_argument_is_named_before_the_device_is_touched_and_in_order(lib):
    hgt = np.zeros(64, np.float32)
    sums = np.zeros(16, np.int32)   # sum_in
    cnts = np.zeros(16, np.int16)   # n_in
    sout, nout, mean = np.zeros(16, np.int32), np.zeros(16, np.int16), np.zeros(16, np.float32)
    pose = np.array(er.IDENTITY * 4, np.float64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    at = lambda a, n: ctypes.c_void_p(a.ctypes.data + n)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    H = pwpp_hip.MEM_HOST
    err = lib.pwpp_last_error
    g = pwpp_hip.GroundGrid(-2.0, -2.0, 1.0, 4, 4, 0, 0)
    hm = height_map()

    def grid(h=fake, gr=ctypes.byref(g), frames=1, mem=H, height=vp(hgt), pose=vp(pose), z_offset=None, n_poses=1, mof=None, m=ctypes.byref(hm), n_maps=1,
             shift=None, sum_in=vp(sums), n_in=vp(cnts), sum_out=vp(sout), n_out=vp(nout), mean=vp(mean)):
        return lib.pwpp_fuse_height_grid(h, gr, frames, mem, height, pose, z_offset, n_poses, mof, m, n_maps, shift, sum_in, n_in, sum_out, n_out, mean)

    def G(**kw):
        return ctypes.byref(pwpp_hip.GroundGrid(**dict(dict(x0=-2.0, y0=-2.0, cell=1.0, nx=4, ny=4, flags=0, pad_=0), **kw)))

    M = lambda **kw: ctypes.byref(height_map(**kw))
    # 1 null pointers
    assert grid(h=None) == E_ARG and b"null handle" in err()
    assert grid(gr=None) == E_ARG and b"null grid" in err()
    assert grid(height=None) == E_ARG and b"null height" in err()
    assert grid(pose=None) == E_ARG and b"null pose" in err()
    assert grid(m=None) == E_ARG and b"null map description" in err()
    assert grid(sum_out=None) == E_ARG and b"null sum_out" in err()
    assert grid(n_out=None) == E_ARG and b"null n_out" in err()
    # 2 the frame images: frames and sides < 1, sides > 32768, the cells beyond 2^31; 3 the flags
    for kw in (dict(frames=0), dict(gr=G(nx=0)), dict(gr=G(ny=-1))):
        assert grid(**kw) == E_ARG and b"cells" in err(), kw
    for kw in (dict(nx=32769), dict(ny=32769)):
        assert grid(gr=G(**kw)) == E_ARG and b"32768 a side" in err(), kw
    assert grid(gr=G(nx=32768, ny=32768), frames=3, n_poses=3) == E_ARG and b"exceed 2^31" in err()
    for flags in (1, 2):
        assert grid(gr=G(flags=flags)) == E_ARG and b"grid flags %d" % flags in err()
    # 4 the same three of the maps
    for kw in (dict(n_maps=0), dict(m=M(nx=0)), dict(m=M(ny=0))):
        assert grid(**kw) == E_ARG and b"cells" in err(), kw
    for kw in (dict(nx=32769), dict(ny=40000)):
        assert grid(m=M(**kw)) == E_ARG and b"32768 a side" in err(), kw
    assert grid(m=M(nx=32768, ny=32768), n_maps=3) == E_ARG and b"exceed 2^31" in err()
    # 5 the cell sizes
    for c in (0.0, -1.0, NAN, INF):
        assert grid(gr=G(cell=c)) == E_ARG and b"finite and positive" in err(), c
        assert grid(m=M(cell=c)) == E_ARG and b"finite and positive" in err(), c
    # 6 n_max and the padding
    for n_max in (0, -1, 1024, 32767):
        assert grid(m=M(n_max=n_max)) == E_ARG and b"n_max %d: 1 .. 1023" % n_max in err()
    assert grid(m=M(pad_=7)) == E_ARG and b"pad_ 7" in err()
    assert grid(m=M(n_max=1), mem=2) == E_ARG and b"PWPP_MEM_HOST or" in err()
    assert grid(m=M(n_max=1023), mem=2) == E_ARG and b"PWPP_MEM_HOST or" in err()
    # 7 the poses; a z_offset that is not finite is no error; 8 map_of_frame
    for n in (0, 2, -1):
        assert grid(n_poses=n) == E_ARG and b"poses for 1 frames" in err(), n
    assert grid(frames=4, n_poses=3) == E_ARG and b"3 poses for 4 frames" in err()
    for z in (NAN, INF, -INF):
        assert grid(z_offset=vp(np.array([z])), mem=2) == E_ARG and b"PWPP_MEM_HOST or" in err(), z
    assert grid(pose=vp(np.full(6, NAN)), mem=2) == E_ARG and b"PWPP_MEM_HOST or" in err()
    assert grid(frames=3, n_maps=2) == E_ARG and b"null map_of_frame with 2 maps for 3 frames" in err()
    for bad, where in (([0, 1, 2], b"map_of_frame 2 names map 2"), ([0, -2, 1], b"map_of_frame 1 names map -2")):
        assert grid(frames=3, n_maps=2, mof=vp(np.array(bad, np.int32))) == E_ARG and where in err(), bad
    # 9 exactly one of the inputs
    assert grid(sum_in=None) == E_ARG and b"null sum_in with a n_in" in err()
    assert grid(n_in=None) == E_ARG and b"null n_in with a sum_in" in err()
    # 10 the overlaps
    zero, moved = np.zeros(2, np.int32), np.array([0, 1], np.int32)
    assert grid(sum_out=vp(sums), shift=vp(moved)) == E_ARG and b"sum_out == sum_in with a shift" in err()
    assert grid(n_out=vp(cnts), shift=vp(moved)) == E_ARG and b"n_out == n_in with a shift" in err()
    assert grid(sum_out=at(sums, 4)) == E_ARG and b"sum_in and sum_out overlap without being equal" in err()
    assert grid(n_out=at(cnts, 30)) == E_ARG and b"n_in and n_out overlap without being equal" in err()
    assert grid(mean=at(sout, 60)) == E_ARG and b"sum_out and mean overlap" in err()
    assert grid(mean=vp(sums)) == E_ARG and b"sum_in and mean overlap" in err()
    assert grid(n_out=at(sout, 62)) == E_ARG and b"sum_out and n_out overlap" in err()
    assert grid(n_out=vp(sums)) == E_ARG and b"sum_in and n_out overlap" in err()
    assert grid(sum_out=at(cnts, 0)) == E_ARG and b"n_in and sum_out overlap" in err()
    # 11 mem -- and with it: in place without a shift, a null or zero shift, touching ranges, absent inputs and mean are accepted up to here
    assert grid(mem=2) == E_ARG and b"PWPP_MEM_HOST or PWPP_MEM_DEVICE" in err()   # PWPP_MEM_HOST_PINNED
    assert grid(sum_out=vp(sums), n_out=vp(cnts), mem=2) == E_ARG and b"PWPP_MEM_HOST or" in err()
    assert grid(sum_out=vp(sums), shift=vp(zero), mem=2) == E_ARG and b"PWPP_MEM_HOST or" in err()
    two = np.zeros(32, np.int32)
    assert grid(sum_in=vp(two), sum_out=at(two, 64), mem=2) == E_ARG and b"PWPP_MEM_HOST or" in err()
    assert grid(sum_in=None, n_in=None, mean=None, mem=7) == E_ARG and b"mem 7" in err()
    # 12 device alignment
    D = pwpp_hip.MEM_DEVICE
    assert grid(height=at(hgt, 2), mem=D) == E_ARG and b"height images must be 4-byte aligned" in err()
    assert grid(sum_out=at(two, 2), mem=D) == E_ARG and b"sums must be 4-byte aligned" in err()
    assert grid(mean=at(two, 66), mem=D) == E_ARG and b"mean must be 4-byte aligned" in err()
    assert grid(n_out=at(two, 1), mem=D) == E_ARG and b"counts must be 2-byte aligned" in err()
    # the order
    assert grid(height=None, frames=0) == E_ARG and b"null height" in err()
    assert grid(frames=0, n_maps=0) == E_ARG and b"0 frames of 4 x 4" in err()
    assert grid(gr=G(nx=32769), m=M(nx=0)) == E_ARG and b"32768 a side" in err()
    assert grid(gr=G(cell=0.0, flags=1)) == E_ARG and b"grid flags" in err()  # the frame grid's own checks come before the map's
    assert grid(gr=G(flags=1), n_maps=0) == E_ARG and b"grid flags" in err()
    assert grid(n_maps=0, gr=G(cell=0.0)) == E_ARG and b"0 frames of 4 x 4" in err()   # (the maps' own "frames" are the maps)
    assert grid(m=M(cell=0.0, n_max=0)) == E_ARG and b"finite and positive" in err()
    assert grid(m=M(n_max=0, pad_=1)) == E_ARG and b"n_max 0" in err()
    assert grid(m=M(pad_=1), n_poses=2) == E_ARG and b"pad_ 1" in err()
    assert grid(n_poses=2, frames=3, n_maps=2) == E_ARG and b"poses for" in err()
    assert grid(frames=3, n_poses=3, n_maps=2, sum_in=None) == E_ARG and b"null map_of_frame" in err()
    assert grid(sum_in=None, sum_out=vp(cnts)) == E_ARG and b"null sum_in" in err()
    assert grid(sum_out=vp(sums), shift=vp(moved), mem=2) == E_ARG and b"with a shift" in err()
    assert grid(mem=2, height=at(hgt, 2)) == E_ARG and b"PWPP_MEM_HOST or" in err()

    def ground(h=fake, gr=ctypes.byref(g), frames=1, pose=vp(pose), n_poses=1, mof=None, m=ctypes.byref(hm), n_maps=1, shift=None, sum_in=vp(sums),
               sum_out=vp(sout), n_out=vp(nout)):
        return lib.pwpp_fuse_ground(h, gr, 0, frames, H, pose, None, n_poses, mof, m, n_maps, shift, sum_in, vp(cnts), sum_out, n_out, None, None)

    assert ground(h=None) == E_ARG and b"null handle" in err()
    assert ground(gr=None) == E_ARG and b"null grid" in err()
    assert ground(pose=None) == E_ARG and b"null pose" in err()
    assert ground(m=None) == E_ARG and b"null map description" in err()
    assert ground(sum_out=None) == E_ARG and b"null sum_out" in err()
    assert ground(n_out=None) == E_ARG and b"null n_out" in err()
    assert ground(frames=0) == E_ARG and b"0 frames" in err()
    assert ground(gr=G(nx=0)) == E_ARG and b"cells" in err()
    assert ground(gr=G(nx=32769)) == E_ARG and b"32768 a side" in err()
    assert ground(gr=G(flags=2)) == E_ARG and b"grid flags 2" in err()
    assert ground(gr=G(flags=1), n_maps=0) == E_ARG and b"cells" in err()   # PWPP_GRID_GROUND_ONLY is accepted
    assert ground(m=M(cell=-1.0)) == E_ARG and b"finite and positive" in err()
    assert ground(m=M(n_max=2000)) == E_ARG and b"n_max 2000" in err()
    assert ground(n_poses=2) == E_ARG and b"2 poses for 1 frames" in err()
    assert ground(mof=vp(np.array([1], np.int32))) == E_ARG and b"map_of_frame 0 names map 1" in err()
    assert ground(sum_in=None) == E_ARG and b"null sum_in" in err()
    assert ground(sum_out=vp(sums), shift=vp(moved)) == E_ARG and b"with a shift" in err()


CPP = r"""
#include "patchwork/patchworkpp.h"
#ifndef PWPP_HAS_ELEVATION_FUSION
#error "include/pwpp.h does not announce the elevation fusion"
#endif
static_assert(sizeof(pwpp_height_map) == 40, "pwpp_height_map");
double use(patchwork::PatchWorkpp &pw) {
    patchwork::PatchWorkpp::FusedElevationMap map;
    map.x0 = -64.0, map.y0 = -64.0, map.cell = 0.5, map.nx = 256, map.ny = 256, map.n_max = 32;
    const double pose[6] = {1.0, 0.0, 3.0, 0.0, 1.0, -1.5};
    pw.updateElevationMap(map, pose, 0.0, -40.0, -40.0, 0.5, 160, 160);
    pw.updateElevationMap(map, pose, 1.7, -40.0, -40.0, 0.5, 160, 160, true, 2, -1);
    const auto mean = pw.getFusedElevation(map);
    return map.sum[3 * 256 + 5] + map.n[7] + map.mean[9] + map.x0 + (double)mean(3, 5) + (double)mean.rows();
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_method_compiles(tmp_path, flavour):
    src = tmp_path / "elevation_fusion.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    cmd += ["-DPWPP_NO_EIGEN"] if flavour == "plain" else ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "elevation.c"
    src.write_text('#include "pwpp.h"\nint f(const pwpp_height_map *m) { return pwpp_fuse_height_grid(0, 0, 1, PWPP_MEM_HOST, 0, 0, 0, 1, 0, m, 1, 0, 0, 0, 0, 0, 0) + '
                   'pwpp_fuse_ground(0, 0, 0, 1, PWPP_MEM_HOST, 0, 0, 1, 0, m, 1, 0, 0, 0, 0, 0, 0, 0) + (int)sizeof(*m); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# ---- the restatement itself ---------------------------------------------------------------------------------------------------
GRID = (-16.0, -16.0, 0.5)
MGRID = (-16.0, -16.0, 0.5, 64, 64)


def q_of(h):
    """The observation of a float32 height image in units of 2^-10 m, and where there is one."""
    z = h.astype(np.float64)
    seen = np.isfinite(z) & (np.abs(z) <= 1024.0)
    return seen, np.rint(np.where(seen, z, 0.0) * 1024.0).astype(np.int64)


def test_a_whole_cell_translation_moves_the_heights_losslessly():
    h = er.random_heights(1, 64, 64, 1)
    s, n, mean = er.fuse(h, GRID, (1, 0, 1.5, 0, 1, -2.0), MGRID, 4)   # +3 cells in x, -4 in y
    seen, q = q_of(h[0])
    want_s, want_n = np.zeros((64, 64), np.int64), np.zeros((64, 64), np.int64)
    want_s[:60, 3:], want_n[:60, 3:] = q[4:, :61], seen[4:, :61]
    assert np.array_equal(s[0], want_s) and np.array_equal(n[0], want_n)
    assert seen.sum() > 2500 and (mean[0].view(np.uint32)[want_n == 0] == er.NAN_BITS).all()
    # a height that is a multiple of 2^-10 m comes back exactly
    exact = np.round(h[0, 4:, :61].astype(np.float64) * 1024.0) / 1024.0
    ok = want_n[:60, 3:] == 1
    assert np.array_equal(mean[0, :60, 3:][ok], exact[ok].astype(np.float32))


def test_a_quarter_turn_is_rot90():
    h = er.random_heights(1, 64, 64, 2)
    seen, q = q_of(h[0])
    s, n, _ = er.fuse(h, GRID, (0, -1, 0, 1, 0, 0), MGRID, 4)
    assert np.array_equal(s[0], np.rot90(q, -1)) and np.array_equal(n[0], np.rot90(seen, -1))
    s, n, _ = er.fuse(h, GRID, (0, 1, 0, -1, 0, 0), MGRID, 4)
    assert np.array_equal(s[0], np.rot90(q, 1)) and np.array_equal(n[0], np.rot90(seen, 1))


@pytest.mark.parametrize("n_max", [1, 2, 7, 1023])
def test_the_mean_of_k_equal_heights_is_that_height(n_max):
    g1, m1 = (0.0, 0.0, 1.0), (0.0, 0.0, 1.0, 3, 1)
    for k in (1, n_max, n_max + 1, n_max + 30):
        h = np.tile(np.array([[[-1.7, 1024.0, 0.5 / 1024]]], np.float32), (k, 1, 1))
        s, n, mean = er.fuse(h, g1, er.IDENTITY, m1, n_max)
        q = np.rint(h[0, 0].astype(np.float64) * 1024).astype(np.int64)   # (-1741, 2^20, 0: the tie goes to even)
        assert q.tolist() == [-1741, 1 << 20, 0]
        assert n[0, 0].tolist() == [min(k, n_max)] * 3 and s[0, 0].tolist() == (q * min(k, n_max)).tolist(), (k, n_max)
        assert mean[0, 0].tolist() == [np.float32(-1741 / 1024), 1024.0, 0.0]


def test_below_n_max_the_order_is_free_and_above_it_the_contract_says_how():
    h = er.random_heights(6, 9, 11, 3)
    grid, mgrid = (-2.75, -2.25, 0.5), (-3.0, -2.5, 0.5, 12, 10)
    poses = er.random_poses(6, 4, 1.0)
    tz = np.linspace(-0.5, 0.5, 6)
    a = er.fuse(h, grid, poses, mgrid, 6, z_offset=tz)
    for perm in ([5, 4, 3, 2, 1, 0], [2, 0, 5, 1, 4, 3]):
        b = er.fuse(h[perm], grid, [poses[i] for i in perm], mgrid, 6, z_offset=tz[perm])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), perm
    assert a[1].max() >= 4
    c = er.fuse(h, grid, poses, mgrid, 2, z_offset=tz)
    d = er.fuse(h[::-1], grid, poses[::-1], mgrid, 2, z_offset=tz[::-1])
    assert c[0].tobytes() != d[0].tobytes() and c[1].tobytes() == d[1].tobytes()
    # the header's examples
    g1, m1 = (0.0, 0.0, 1.0), (0.0, 0.0, 1.0, 1, 1)
    one = lambda hs, n_max, **kw: er.fuse(np.array(hs, np.float32).reshape(-1, 1, 1), g1, er.IDENTITY, m1, n_max, **kw)
    assert one([1.0, 2.0], 1)[2][0, 0, 0] == 2.0 and one([2.0, 1.0], 1)[2][0, 0, 0] == 1.0
    start = dict(sum_in=np.array([[[3072]]], np.int32), n_in=np.array([[[2]]], np.int16))
    assert one([1.0, 3.0], 2, **start)[0][0, 0, 0] == 4352 and one([3.0, 1.0], 2, **start)[0][0, 0, 0] == 3328
    # the update in Python integers, with truncation toward zero for a negative sum
    assert er.update(3072, 2, 1024, 2) == (2560, 2) and er.update(-7, 2, 0, 2) == (-4, 2) and er.update(7, 2, 0, 2) == (4, 2)
    assert er.update(5, 1, 9, 2) == (14, 2)


def test_the_vector_update_is_the_integer_update():
    rng = np.random.default_rng(5)
    g1, m1 = (0.0, 0.0, 1.0), (0.0, 0.0, 1.0, 1, 1)
    for n_max in (1, 3, 7):
        hs = rng.uniform(-1030, 1030, 40).astype(np.float32)
        s, n = 0, 0
        for z in hs:
            if abs(float(z)) <= 1024.0:
                s, n = er.update(s, n, int(np.rint(np.float64(z) * 1024.0)), n_max)
        got = er.fuse(hs.reshape(-1, 1, 1), g1, er.IDENTITY, m1, n_max)
        assert (int(got[0][0, 0, 0]), int(got[1][0, 0, 0])) == (s, n) and n == n_max


def test_two_calls_compose_to_one():
    h = er.random_heights(7, 31, 33, 6)
    grid, mgrid = (-8.0, -8.0, 0.5), (-9.0, -7.0, 0.5, 40, 37)
    poses = er.random_poses(7, 7, 3.0)
    tz = np.linspace(-1, 1, 7)
    rng = np.random.default_rng(8)
    n_in = rng.integers(0, 4, (1, 37, 40)).astype(np.int16)
    sum_in = (rng.integers(-2000, 2000, (1, 37, 40)) * n_in).astype(np.int32)
    whole = er.fuse(h, grid, poses, mgrid, 3, 1, sum_in, n_in, tz, shift=[(2, -1)])
    first = er.fuse(h[:3], grid, poses[:3], mgrid, 3, 1, sum_in, n_in, tz[:3], shift=[(2, -1)])
    second = er.fuse(h[3:], grid, poses[3:], mgrid, 3, 1, first[0], first[1], tz[3:])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(second, whole))
    assert first[0].tobytes() != whole[0].tobytes()


def test_shifts_also_larger_than_the_map():
    mgrid = (0.0, 0.0, 1.0, 5, 4)
    n_in = np.arange(20, dtype=np.int16).reshape(1, 4, 5) % 3 + 1
    sum_in = (np.arange(20, dtype=np.int32).reshape(1, 4, 5) - 7) * 100
    none = np.full((1, 1, 1), np.nan, np.float32)   # a frame that observes nothing: the shifted input alone
    run = lambda shift: er.fuse(none, (100.0, 100.0, 1.0), er.IDENTITY, mgrid, 5, 1, sum_in, n_in, shift=shift)
    s, n, mean = run([(1, -2)])
    assert np.array_equal(s[0, 2:, :4], sum_in[0, :2, 1:]) and np.array_equal(n[0, 2:, :4], n_in[0, :2, 1:])
    assert not s[0, :2].any() and not n[0, :2].any() and not s[0, :, 4].any() and (mean[0, :2].view(np.uint32) == er.NAN_BITS).all()
    for shift in ((5, 0), (0, -4), (2 ** 31 - 1, 0), (-2 ** 31, -2 ** 31), (0, 2 ** 31 - 1)):
        s, n, mean = run([shift])
        assert not s.any() and not n.any() and (mean.view(np.uint32) == er.NAN_BITS).all(), shift
    s, n, _ = run(None)
    assert np.array_equal(s, sum_in) and np.array_equal(n, n_in)


def test_inputs_out_of_range_are_normalised():
    mgrid = (0.0, 0.0, 1.0, 6, 1)
    n_in = np.array([[[-5, 0, 3, 9, 32767, 2]]], np.int16)
    sum_in = np.array([[[77, 77, 5 * er.M, -2 ** 31, 2 ** 31 - 1, -3 * er.M]]], np.int32)
    none = np.full((1, 1, 1), np.nan, np.float32)
    s, n, mean = er.fuse(none, (100.0, 100.0, 1.0), er.IDENTITY, mgrid, 4, 1, sum_in, n_in)
    assert n[0, 0].tolist() == [0, 0, 3, 4, 4, 2]
    assert s[0, 0].tolist() == [0, 0, 3 * er.M, -4 * er.M, 4 * er.M, -2 * er.M]
    assert mean[0, 0, 2:].tolist() == [1024.0, -1024.0, 1024.0, -1024.0] and (mean[0, 0, :2].view(np.uint32) == er.NAN_BITS).all()
    # ... and then updated like any other state
    s, n, _ = er.fuse(np.full((1, 1, 1), 1.0, np.float32), (0.0, 0.0, 6.0), er.IDENTITY, mgrid, 4, 1, sum_in, n_in)
    assert n[0, 0].tolist() == [1, 1, 4, 4, 4, 3] and s[0, 0].tolist() == [1024, 1024, 3 * er.M + 1024, -3 * er.M + 1024, 3 * er.M + 1024, -2 * er.M + 1024]


def test_ties_limits_and_values_that_are_not_finite():
    g1 = (0.0, 0.0, 1.0)
    beyond = np.nextafter(np.float32(1024.0), np.float32(np.inf))
    hs = np.array([0.5 / 1024, 1.5 / 1024, 2.5 / 1024, -0.5 / 1024, -1.5 / 1024, -0.0, 1024.0, -1024.0, beyond, -beyond, INF, -INF, NAN], np.float32)
    s, n, mean = er.fuse(hs.reshape(1, 1, -1), g1, er.IDENTITY, (0.0, 0.0, 1.0, len(hs), 1), 3)
    assert s[0, 0].tolist() == [0, 2, 2, 0, -2, 0, er.M, -er.M, 0, 0, 0, 0, 0]           # ties to even
    assert n[0, 0].tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
    assert mean[0, 0, 5].tobytes() == np.float32(0.0).tobytes()                           # -0.0 observes 0: the mean is +0.0
    assert (mean[0, 0, 8:].view(np.uint32) == er.NAN_BITS).all()
    # the offset enters before the test: 1024 + 2^-20 is beyond, -1024 + 1 is not; a non-finite offset or pose observes nothing
    one = lambda z, tz, pose=er.IDENTITY: er.fuse(np.full((1, 1, 1), z, np.float32), g1, pose, (0.0, 0.0, 1.0, 1, 1), 3, z_offset=[tz])
    assert one(1024.0, 2.0 ** -20)[1][0, 0, 0] == 0 and one(-1024.0, 1.0)[0][0, 0, 0] == -1023 * 1024
    assert one(2000.0, -1000.0)[0][0, 0, 0] == 1000 * 1024
    for tz in (NAN, INF, -INF):
        assert one(1.0, tz)[1][0, 0, 0] == 0
    assert one(1.0, 0.0, (1.0, 0.0, NAN, 0.0, 1.0, 0.0))[1][0, 0, 0] == 0 and one(1.0, 0.0, (INF, 0.0, 0.0, 0.0, 1.0, 0.0))[1][0, 0, 0] == 0
    assert one(1.0, 0.0)[1][0, 0, 0] == 1


# ---- the kernel's functions on the host ----------------------------------------------------------------------------------------
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def sanitizers_work(tmp_path):
    """The toolchain links the two runtimes into a program and that program starts in this environment."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        return False
    return subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0


def test_elevation_program_builds_and_passes(tmp_path):
    exe = tmp_path / "elevation_check"
    flags = SANITIZE if sanitizers_work(tmp_path) else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off"] + flags +
                   ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "elevation_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)  # (a stand-alone child process with its own main)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches, 0 failed proof steps" in r.stdout
    assert int(r.stdout.split("elevation_check: ")[1].split(" cases")[0]) >= 3000000
