"""No-GPU checks of the line-of-sight free space (pwpp_visibility_grid, pwpp_visibility_obstacles): the exports, the feature macro
and constants, the ctypes prototypes and the bindings' methods, every argument check that needs no device with its message and
its place in the order, the C++ mirror in both flavours -- the properties of the brute force the GPU tests compare against
(tests/obstacle_visibility_ref.py): the watertight ring, the cap, the cases a caller reads off `first` -- and the stand-alone
program that runs the kernels' pack and walk on the host against a brute force of its own (tools/visibility_check.cpp), built
with the address and undefined-behaviour sanitizers where the toolchain has them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import obstacle_visibility_ref as ov
import pwpp_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")
E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pwpp_hip.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "lib/libpwpp_hip.so"], check=True, stdout=subprocess.DEVNULL)
    return pwpp_hip.load()


def test_symbols_macro_constants_and_prototypes(lib):
    hdr = open(os.path.join(ROOT, "include", "pwpp.h")).read()
    for name in ("pwpp_visibility_grid", "pwpp_visibility_obstacles"):
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr
    assert "#define PWPP_HAS_OBSTACLE_VISIBILITY 1" in hdr
    assert "#define PWPP_VIS_NONE   (-1)" in hdr and "#define PWPP_VIS_BEYOND (-2)" in hdr
    assert "enum { PWPP_OCC_FREE = 0, PWPP_OCC_OCCUPIED = 100, PWPP_OCC_UNKNOWN = -1 };" in hdr
    assert "#define PWPP_VERSION_MINOR 4 " in hdr
    assert '"visibility_path"' in hdr and "2-D LINE OF SIGHT ON A 2.5-D MAP" in hdr
    assert (pwpp_hip.VIS_NONE, pwpp_hip.VIS_BEYOND) == (ov.NONE, ov.BEYOND) == (-1, -2)
    assert (pwpp_hip.OCC_FREE, pwpp_hip.OCC_OCCUPIED, pwpp_hip.OCC_UNKNOWN) == (ov.FREE, ov.OCCUPIED, ov.UNKNOWN) == (0, 100, -1)
    assert len(lib.pwpp_visibility_grid.argtypes) == 12 and len(lib.pwpp_visibility_obstacles.argtypes) == 14
    assert lib.pwpp_visibility_obstacles.argtypes[2] is ctypes.c_float and lib.pwpp_visibility_obstacles.argtypes[3] is ctypes.c_float
    for name in ("visibility_grid", "visibility_grid_device", "visibility_obstacles", "visibility_obstacles_device"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    import pypatchworkpp
    assert hasattr(pypatchworkpp.patchworkpp, "getObstacleVisibility")


def test_every_argument_is_named_before_the_device_is_touched_and_in_order(lib):
    cnt, first, occ = np.zeros(16, np.int32), np.zeros(16, np.int32), np.zeros(16, np.int8)
    one = np.array([1, 2], np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    H = pwpp_hip.MEM_HOST
    err = lib.pwpp_last_error

    def grid(h=fake, nx=4, ny=4, frames=1, mem=H, count=vp(cnt), min_count=1, origin=vp(one), n_origins=1, max_range=0, first=vp(first)):
        return lib.pwpp_visibility_grid(h, nx, ny, frames, mem, count, min_count, origin, n_origins, max_range, first, vp(occ))

    # 1 null pointers
    assert grid(h=None) == E_ARG and b"null handle" in err()
    assert grid(count=None) == E_ARG and b"null count" in err()
    assert grid(first=None) == E_ARG and b"null first" in err()
    assert grid(origin=None) == E_ARG and b"null origin" in err()
    # 2 sides and cells
    for kw in (dict(nx=0), dict(ny=0), dict(frames=0), dict(nx=-3)):
        assert grid(**kw) == E_ARG and b"cells" in err(), kw
    for kw in (dict(nx=32769), dict(ny=32769), dict(nx=65536, ny=32768)):
        assert grid(**kw) == E_ARG and b"32768 a side" in err(), kw
    assert grid(nx=32768, ny=32768, frames=3, n_origins=3) == E_ARG and b"exceed 2^31" in err()
    # 3 min_count, 4 max_range
    for m in (0, -1):
        assert grid(min_count=m) == E_ARG and b"min_count" in err()
    for m in (-1, 32769, 1 << 30):
        assert grid(max_range=m) == E_ARG and b"max_range" in err(), m
    # 5 origins: their number, then every entry inside the image, named
    for n in (0, 2, -1):
        assert grid(n_origins=n) == E_ARG and b"origins for 1 frames" in err(), n
    assert grid(frames=3, n_origins=2) == E_ARG and b"2 origins for 3 frames" in err()
    for bad in ((4, 0), (0, 4), (-1, 0), (0, -1)):
        assert grid(origin=vp(np.array(bad, np.int32))) == E_ARG and b"origin 0" in err() and b"outside" in err(), bad
    three = np.array([0, 0, 3, 3, 3, 4], np.int32)
    assert grid(frames=3, n_origins=3, origin=vp(three)) == E_ARG and b"origin 2, cell (3, 4)" in err()
    # 6 mem
    assert grid(mem=2) == E_ARG and b"PWPP_MEM_HOST or PWPP_MEM_DEVICE" in err()   # PWPP_MEM_HOST_PINNED
    # the order: nulls before sides, sides before cells, cells before min_count, that before max_range, that before the origins, those before mem
    assert grid(count=None, nx=0) == E_ARG and b"null count" in err()
    assert grid(nx=32769, ny=32769, frames=4, min_count=0) == E_ARG and b"32768 a side" in err()
    assert grid(nx=32768, ny=32768, frames=3, min_count=0) == E_ARG and b"exceed 2^31" in err()
    assert grid(min_count=0, max_range=-1) == E_ARG and b"min_count" in err()
    assert grid(max_range=-1, n_origins=2) == E_ARG and b"max_range" in err()
    assert grid(n_origins=2, mem=2) == E_ARG and b"origins for" in err()
    assert grid(origin=vp(np.array([4, 0], np.int32)), mem=2) == E_ARG and b"outside" in err()

    g = pwpp_hip.GroundGrid(-2.0, -2.0, 1.0, 4, 4, 0, 0)
    zero = np.zeros(2, np.float64)

    def obstacles(h=fake, gr=ctypes.byref(g), band=(0.2, 2.5), min_count=1, origin=vp(zero), n_origins=1, max_range=0, frames=1, first=vp(first)):
        return lib.pwpp_visibility_obstacles(h, gr, band[0], band[1], min_count, origin, n_origins, max_range, 0, frames, H, first, None, None)

    assert obstacles(h=None) == E_ARG and b"null handle" in err()
    assert obstacles(gr=None) == E_ARG and b"null grid" in err()
    assert obstacles(first=None) == E_ARG and b"null first" in err()
    assert obstacles(origin=None) == E_ARG and b"null origin" in err()
    assert obstacles(band=(2.5, 0.2)) == E_ARG and b"height band" in err()
    assert obstacles(band=(np.nan, 1.0)) == E_ARG and b"height band" in err()
    bad = pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 4, 4, 2, 0)
    assert obstacles(gr=ctypes.byref(bad)) == E_ARG and b"grid flags" in err()
    for kw in (dict(nx=0), dict(cell=0.0), dict(cell=np.nan), dict(x0=np.inf)):
        gg = pwpp_hip.GroundGrid(**dict(dict(x0=-2.0, y0=-2.0, cell=1.0, nx=4, ny=4, flags=0, pad_=0), **kw))
        assert obstacles(gr=ctypes.byref(gg)) == E_ARG and (b"grid of" in err() or b"finite" in err()), kw
    wide = pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 32769, 4, 0, 0)
    assert obstacles(gr=ctypes.byref(wide)) == E_ARG and b"32768 a side" in err()
    assert obstacles(min_count=0) == E_ARG and b"min_count" in err()
    assert obstacles(max_range=32769) == E_ARG and b"max_range" in err()
    assert obstacles(n_origins=2) == E_ARG and b"2 origins for 1 frames" in err()
    for xy in ((2.0, 0.0), (0.0, 2.0), (-2.5, 0.0), (0.0, -2.0000001)):  # the cell rule: 0 <= (x - x0) / cell < n
        assert obstacles(origin=vp(np.array(xy, np.float64))) == E_ARG and b"origin 0" in err() and b"outside the grid" in err(), xy
    for xy in ((np.nan, 0.0), (0.0, np.inf)):
        assert obstacles(origin=vp(np.array(xy, np.float64))) == E_ARG and b"origin 0" in err() and b"not finite" in err(), xy
    two = np.array([0.0, 0.0, 1.0, 7.0], np.float64)
    assert obstacles(origin=vp(two), n_origins=2, frames=2) == E_ARG and b"origin 1" in err()
    assert obstacles(min_count=0, max_range=-1, n_origins=2) == E_ARG and b"min_count" in err()
    assert obstacles(max_range=-1, n_origins=2) == E_ARG and b"max_range" in err()


CPP = r"""
#include "patchwork/patchworkpp.h"
#ifndef PWPP_HAS_OBSTACLE_VISIBILITY
#error "include/pwpp.h does not announce the line-of-sight free space"
#endif
static_assert(PWPP_VIS_NONE == -1 && PWPP_VIS_BEYOND == -2, "first");
static_assert(PWPP_OCC_FREE == 0 && PWPP_OCC_OCCUPIED == 100 && PWPP_OCC_UNKNOWN == -1, "nav_msgs/OccupancyGrid");
double use(patchwork::PatchWorkpp &pw) {
    patchwork::PatchWorkpp::ObstacleVisibility v = pw.getObstacleVisibility(-40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f);
    patchwork::PatchWorkpp::ObstacleVisibility w = pw.getObstacleVisibility(-40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f, 2, 40, 1.5, -0.5, true);
    return v.first[3 * 160 + 5] + v.occupancy[7] + (double)w.first.size() + w.nx + w.ny + (w.occupancy[0] == PWPP_OCC_UNKNOWN ? 1.0 : 0.0);
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_method_compiles(tmp_path, flavour):
    src = tmp_path / "obstacle_visibility.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    cmd += ["-DPWPP_NO_EIGEN"] if flavour == "plain" else ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "visibility.c"
    src.write_text('#include "pwpp.h"\nint f(void) { return pwpp_visibility_grid(0, 1, 1, 1, PWPP_MEM_HOST, 0, 1, 0, 1, 0, 0, 0) + PWPP_VIS_NONE + '
                   'PWPP_VIS_BEYOND + PWPP_OCC_OCCUPIED; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# ---- the restatement itself ---------------------------------------------------------------------------------------------------
def test_the_ring_is_watertight_in_the_restatement_and_only_with_rule_a():
    count, disc = ov.ring_image()
    assert count.shape == (41, 41) and (~disc).sum() == 1240
    for origin in ov.RING_ORIGINS:
        assert disc[origin[1], origin[0]] and count[origin[1], origin[0]] == 0
        first = ov.first_of(count, origin)
        assert (first[~disc] != ov.NONE).all(), "origin %s: %d cells outside the ring are seen" % (origin, (first[~disc] == ov.NONE).sum())
        assert (count.reshape(-1)[first[~disc]] >= 1).all()  # what hides them is a cell of the ring
        assert (ov.occupancy_of(count, first)[~disc] == ov.UNKNOWN).all()
        inside = disc & (count == 0)
        assert (first[inside] == ov.NONE).all() and (ov.occupancy_of(count, first)[inside] == ov.FREE).all()  # a disc is star-shaped enough: all of it is seen
        leaks = int((ov.first_of(count, origin, rule_a=False)[~disc] == ov.NONE).sum())
        assert 200 <= leaks <= 288, "origin %s: without rule (a) %d cells outside leak: the ring no longer discriminates" % (origin, leaks)


def test_what_a_caller_reads_off_first():
    count = np.zeros((5, 9), np.int32)
    count[2, 4] = 2      # a post between the origin (1, 2) and the cells right of it
    count[2, 1] = 5      # the origin's own cell is occupied: it never blocks
    first = ov.first_of(count, (1, 2))
    own = np.arange(45).reshape(5, 9)
    assert first[2, 1] == own[2, 1] and first[2, 4] == own[2, 4]            # seen surfaces: their own index
    assert (first[2, 5:] == own[2, 4]).all()                                # hidden: the index of what hides them
    assert (first[2, 2:4] == ov.NONE).all() and (first[0] == ov.NONE).all()  # seen and free
    occ = ov.occupancy_of(count, first)
    assert occ[2, 1] == occ[2, 4] == ov.OCCUPIED and (occ[2, 5:] == ov.UNKNOWN).all() and (occ[0] == ov.FREE).all()
    assert (ov.first_of(count, (1, 2), min_count=3)[2, 5:] == ov.NONE).all()  # the post is below min_count 3
    # rule (a): two cells that touch at a corner stop the diagonal between them, the smaller index is reported
    count = np.zeros((4, 4), np.int32)
    count[0, 1] = count[1, 0] = 1
    first = ov.first_of(count, (0, 0))
    assert first[1, 1] == 1 and first[3, 3] == 1 and first[2, 2] == 1


@pytest.mark.parametrize("shape", [(5, 7), (33, 31), (65, 63)], ids=lambda s: "%dx%d" % s)
def test_max_range_changes_nothing_inside_it_in_the_restatement(shape):
    nx, ny = shape
    iy, ix = np.mgrid[0:ny, 0:nx]
    for fill, origin in ((0.05, (0, 0)), (0.4, (nx // 2, ny // 2)), (0.05, (nx - 1, ny // 3))):
        count = ov.random_count(nx, ny, fill, 1, 7 + nx)
        unlimited = ov.first_of(count, origin)
        assert (unlimited != ov.BEYOND).all()
        for max_range in (1, 7, 200):
            got = ov.first_of(count, origin, 1, max_range)
            n = np.maximum(np.abs(ix - origin[0]), np.abs(iy - origin[1]))
            assert (got[n > max_range] == ov.BEYOND).all() and np.array_equal(got[n <= max_range], unlimited[n <= max_range])
            assert np.array_equal(got, ov.capped(unlimited, origin, max_range))
            occ = ov.occupancy_of(count, got)
            assert (occ[(n > max_range) & (count < 1)] == ov.UNKNOWN).all() and (occ[count >= 1] == ov.OCCUPIED).all()
        some = np.array([(0, 0), (nx - 1, ny - 1), (nx // 2, 0), origin])
        assert np.array_equal(ov.first_of(count, origin, cells=some), unlimited[some[:, 1], some[:, 0]])  # the form over a list of cells


# ---- the kernels' functions and sequence on the host -----------------------------------------------------------------------------
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def sanitizers_work(tmp_path):
    """The toolchain links the two runtimes into a program and that program starts in this environment."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        return False
    return subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0


def test_visibility_program_builds_and_passes(tmp_path):
    exe = tmp_path / "visibility_check"
    flags = SANITIZE if sanitizers_work(tmp_path) else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags +
                   ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "visibility_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)  # (a stand-alone child process with its own main)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 mismatches" in r.stdout and "11238 cases" in r.stdout
