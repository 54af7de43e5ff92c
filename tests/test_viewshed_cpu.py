"""No-GPU checks of the viewshed (pwpp_viewshed_grid, pwpp_rasterize_ground_returns, pwpp_viewshed_obstacles, pwpp_viewshed_units):
the exports, the feature macro and constants, the ctypes prototypes and the bindings' methods, every argument check that needs no
device with its message and its place in the order, the header as C99, the C++ mirror in both flavours -- the properties of the
restatement the GPU tests compare against (tests/viewshed_ref.py): the 2-D operator on degenerate input, the subset theorem,
max_range, the kerb, hidden-iff-below-shadow, rule (a) with unequal rises -- and the stand-alone program that deals the kernels' pack
and walk on the host against a brute force of its own (tools/viewshed_check.cpp), built with the address and undefined-behaviour
sanitizers where the toolchain has them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import obstacle_visibility_ref as ov
import pwpp_hip
import viewshed_ref as vr
from test_obstacle_visibility_cpu import SANITIZE, sanitizers_work

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
    for name in ("pwpp_viewshed_grid", "pwpp_rasterize_ground_returns", "pwpp_viewshed_obstacles"):
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr
    assert hasattr(lib, "pwpp_viewshed_units") and "PWPP_API int32_t pwpp_viewshed_units(double metres);" in hdr
    assert "#define PWPP_HAS_VIEWSHED 1" in hdr
    assert "#define PWPP_VIEW_NO_HEIGHT (-2147483647 - 1)" in hdr and "#define PWPP_VIEW_MAX_RISE 1048576" in hdr
    assert "#define PWPP_VIEW_UNITS_PER_M 1024" in hdr
    assert "#define PWPP_VERSION_MINOR 4 " in hdr  # (unchanged)
    assert '"viewshed_path"' in hdr and "2-D LINE OF SIGHT ON A 2.5-D MAP" in hdr
    assert (pwpp_hip.VIEW_NO_HEIGHT, pwpp_hip.VIEW_MAX_RISE, pwpp_hip.VIEW_UNITS_PER_M) == (vr.NO_HEIGHT, vr.R, vr.UNITS_PER_M) == (-2 ** 31, 2 ** 20, 1024)
    assert len(lib.pwpp_viewshed_grid.argtypes) == 17 and len(lib.pwpp_viewshed_obstacles.argtypes) == 16
    assert len(lib.pwpp_rasterize_ground_returns.argtypes) == 6
    assert lib.pwpp_viewshed_obstacles.argtypes[2] is ctypes.c_float and lib.pwpp_viewshed_obstacles.argtypes[3] is ctypes.c_float
    for name in ("viewshed_grid", "viewshed_grid_device", "rasterize_ground_returns", "rasterize_ground_returns_device", "viewshed_obstacles",
                 "viewshed_obstacles_device"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    import pypatchworkpp
    assert hasattr(pypatchworkpp.patchworkpp, "getObstacleViewshed")
    # the one text, its translation unit (the visibility's: the walk with heights), and the kernels' constant the GPU test computes the LDS limit from
    assert os.path.exists(os.path.join(PKG, "csrc", "pwpp_viewshed.h")) and os.path.exists(os.path.join(PKG, "csrc", "pwpp_visibility.hip"))
    assert "#define PWPP_VIS_LDS_BYTES (128 * 1024)" in open(os.path.join(PKG, "csrc", "pwpp_visibility.h")).read()
    assert "csrc/pwpp_visibility.hip" in open(os.path.join(PKG, "Makefile")).read()


def test_the_quantiser(lib):
    for v, q in ((0.0, 0), (1.0, 1024), (-1.0, -1024), (0.00048828125, 1), (-0.00048828125, 0), (1.7, 1741), (1e9, 2 ** 30), (-1e9, -2 ** 30),
                 (np.inf, 2 ** 30), (-np.inf, -2 ** 30), (np.nan, vr.NO_HEIGHT), (-1.723, -1764)):
        assert pwpp_hip.viewshed_units(v) == q == vr.units(v), v
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.normal(0, 3, 500), rng.normal(0, 1e7, 50), [np.nan, np.inf, -np.inf, 0.5 / 1024, -0.5 / 1024, 1.5 / 1024]])
    assert vr.units_image(a).tolist() == [pwpp_hip.viewshed_units(v) for v in a]


def test_every_argument_is_named_before_the_device_is_touched_and_in_order(lib):
    cnt, first, occ = np.zeros(16, np.int32), np.zeros(16, np.int32), np.zeros(16, np.int8)
    one = np.array([1, 2, 1700], np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    H = pwpp_hip.MEM_HOST
    err = lib.pwpp_last_error

    def grid(h=fake, nx=4, ny=4, frames=1, mem=H, count=vp(cnt), min_count=1, seen=None, min_seen=1, origin=vp(one), n_origins=1, max_range=0,
             first=vp(first)):
        return lib.pwpp_viewshed_grid(h, nx, ny, frames, mem, count, min_count, None, None, seen, min_seen, origin, n_origins, max_range, first, None, vp(occ))

    # 1 null pointers
    assert grid(h=None) == E_ARG and b"null handle" in err()
    assert grid(count=None) == E_ARG and b"null count" in err()
    assert grid(first=None) == E_ARG and b"null first" in err()
    assert grid(origin=None) == E_ARG and b"null origin" in err()
    # 2 sides and cells: the visibility's messages
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
    # 5 min_seen, only with a seen image
    for m in (0, -1):
        assert grid(seen=vp(cnt), min_seen=m) == E_ARG and b"min_seen" in err(), m
    # 6 origins: their number, then every cell inside the image, then every eye, named
    for n in (0, 2, -1):
        assert grid(n_origins=n) == E_ARG and b"origins for 1 frames" in err(), n
    assert grid(frames=3, n_origins=2) == E_ARG and b"2 origins for 3 frames" in err()
    for bad in ((4, 0), (0, 4), (-1, 0), (0, -1)):
        assert grid(origin=vp(np.array(bad + (0,), np.int32))) == E_ARG and b"origin 0" in err() and b"outside" in err(), bad
    three = np.array([0, 0, 5, 3, 3, 5, 3, 4, 5], np.int32)
    assert grid(frames=3, n_origins=3, origin=vp(three)) == E_ARG and b"origin 2, cell (3, 4)" in err()
    blind = np.array([0, 0, 5, 3, 3, vr.NO_HEIGHT, 3, 3, vr.NO_HEIGHT], np.int32)
    assert grid(frames=3, n_origins=3, origin=vp(blind)) == E_ARG and b"origin 1" in err() and b"eye" in err()
    # 7 mem
    assert grid(mem=2) == E_ARG and b"PWPP_MEM_HOST or PWPP_MEM_DEVICE" in err()   # PWPP_MEM_HOST_PINNED
    # the order
    assert grid(count=None, nx=0) == E_ARG and b"null count" in err()
    assert grid(nx=32769, ny=32769, frames=4, min_count=0) == E_ARG and b"32768 a side" in err()
    assert grid(nx=32768, ny=32768, frames=3, min_count=0) == E_ARG and b"exceed 2^31" in err()
    assert grid(min_count=0, max_range=-1) == E_ARG and b"min_count" in err()
    assert grid(max_range=-1, seen=vp(cnt), min_seen=0) == E_ARG and b"max_range" in err()
    assert grid(seen=vp(cnt), min_seen=0, n_origins=2) == E_ARG and b"min_seen" in err()
    assert grid(n_origins=2, mem=2) == E_ARG and b"origins for" in err()
    outside_and_blind = np.array([4, 0, vr.NO_HEIGHT], np.int32)
    assert grid(origin=vp(outside_and_blind)) == E_ARG and b"outside" in err()
    assert grid(origin=vp(np.array([0, 0, vr.NO_HEIGHT], np.int32)), mem=2) == E_ARG and b"eye" in err()

    g = pwpp_hip.GroundGrid(-2.0, -2.0, 1.0, 4, 4, 0, 0)
    zero = np.zeros(3, np.float64)

    def obstacles(h=fake, gr=ctypes.byref(g), band=(0.2, 2.5), min_count=1, min_seen=1, origin=vp(zero), n_origins=1, max_range=0, frames=1, first=vp(first)):
        return lib.pwpp_viewshed_obstacles(h, gr, band[0], band[1], min_count, min_seen, origin, n_origins, max_range, 0, frames, H, first, None, None, None)

    assert obstacles(h=None) == E_ARG and b"null handle" in err()
    assert obstacles(gr=None) == E_ARG and b"null grid" in err()
    assert obstacles(first=None) == E_ARG and b"null first" in err()
    assert obstacles(origin=None) == E_ARG and b"null origin" in err()
    assert obstacles(band=(2.5, 0.2)) == E_ARG and b"height band" in err()
    bad = pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 4, 4, 2, 0)
    assert obstacles(gr=ctypes.byref(bad)) == E_ARG and b"grid flags" in err()
    for kw in (dict(nx=0), dict(cell=0.0), dict(cell=np.nan), dict(x0=np.inf)):
        gg = pwpp_hip.GroundGrid(**dict(dict(x0=-2.0, y0=-2.0, cell=1.0, nx=4, ny=4, flags=0, pad_=0), **kw))
        assert obstacles(gr=ctypes.byref(gg)) == E_ARG and (b"grid of" in err() or b"finite" in err()), kw
    wide = pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 32769, 4, 0, 0)
    assert obstacles(gr=ctypes.byref(wide)) == E_ARG and b"32768 a side" in err()
    assert obstacles(min_count=0) == E_ARG and b"min_count" in err()
    assert obstacles(max_range=32769) == E_ARG and b"max_range" in err()
    assert obstacles(min_seen=-1) == E_ARG and b"min_seen" in err()
    assert obstacles(n_origins=2) == E_ARG and b"2 origins for 1 frames" in err()
    for xyz in ((2.0, 0.0, 0.0), (0.0, 2.0, 0.0), (-2.5, 0.0, 0.0), (0.0, -2.0000001, 0.0)):  # the cell rule: 0 <= (x - x0) / cell < n
        assert obstacles(origin=vp(np.array(xyz, np.float64))) == E_ARG and b"origin 0" in err() and b"outside the grid" in err(), xyz
    for xyz in ((np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, np.nan), (0.0, 0.0, -np.inf)):
        assert obstacles(origin=vp(np.array(xyz, np.float64))) == E_ARG and b"origin 0" in err() and b"not finite" in err(), xyz
    two = np.array([0.0, 0.0, 0.0, 1.0, 7.0, 0.0], np.float64)
    assert obstacles(origin=vp(two), n_origins=2, frames=2) == E_ARG and b"origin 1" in err()
    assert obstacles(min_count=0, max_range=-1, min_seen=-1) == E_ARG and b"min_count" in err()
    assert obstacles(max_range=-1, min_seen=-1) == E_ARG and b"max_range" in err()
    assert obstacles(min_seen=-1, n_origins=2) == E_ARG and b"min_seen" in err()

    def returns(h=fake, gr=ctypes.byref(g), seen=vp(first)):
        return lib.pwpp_rasterize_ground_returns(h, gr, 0, 1, H, seen)

    assert returns(h=None) == E_ARG and b"null handle" in err()
    assert returns(gr=None) == E_ARG and b"null grid" in err()
    assert returns(seen=None) == E_ARG and b"null seen" in err()
    for flags in (1, 2):  # PWPP_GRID_GROUND_ONLY too: there is no reference to blank
        gg = pwpp_hip.GroundGrid(-2.0, -2.0, 1.0, 4, 4, flags, 0)
        assert returns(gr=ctypes.byref(gg)) == E_ARG and b"grid flags" in err()
    gg = pwpp_hip.GroundGrid(-2.0, -2.0, 0.0, 4, 4, 0, 0)
    assert returns(gr=ctypes.byref(gg)) == E_ARG and b"finite" in err()
    assert lib.pwpp_rasterize_ground_returns(fake, ctypes.byref(g), 0, 1, 2, vp(first)) == E_ARG and b"PWPP_MEM_HOST or PWPP_MEM_DEVICE" in err()


def test_an_origin_is_refused_in_the_visibilitys_words(lib):
    """The 2-D operator and the viewshed refuse the same origin with the same sentence; only the printed z is the viewshed's own."""
    first = np.zeros(16, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    H = pwpp_hip.MEM_HOST
    err = lambda: lib.pwpp_last_error().decode()
    g = pwpp_hip.GroundGrid(-2.0, -2.0, 1.0, 4, 4, 0, 0)

    def metres(xyz, n=1, frames=1):
        """the messages of (pwpp_visibility_obstacles, pwpp_viewshed_obstacles) for origins given as rows of x, y, z"""
        xyz = np.array(xyz, np.float64).reshape(n, 3)
        xy = np.ascontiguousarray(xyz[:, :2])
        assert lib.pwpp_visibility_obstacles(fake, ctypes.byref(g), 0.2, 2.5, 1, vp(xy), n, 0, 0, frames, H, vp(first), None, None) == E_ARG
        two = err()
        assert lib.pwpp_viewshed_obstacles(fake, ctypes.byref(g), 0.2, 2.5, 1, 1, vp(xyz), n, 0, 0, frames, H, vp(first), None, None, None) == E_ARG
        return two, err()

    assert metres((np.nan, 0.5, 1.5)) == ("origin 0, (nan, 0.5), is not finite", "origin 0, (nan, 0.5, 1.5), is not finite")
    assert metres((0.25, -np.inf, 1.5)) == ("origin 0, (0.25, -inf), is not finite", "origin 0, (0.25, -inf, 1.5), is not finite")
    assert metres((2.0, 0.5, 1.5)) == ("origin 0, (2, 0.5) m, lies outside the grid",) * 2          # x0 + nx * cell: outside
    assert metres((0.5, -2.0000001, 1.5)) == ("origin 0, (0.5, -2) m, lies outside the grid",) * 2  # (%g rounds the y)
    assert metres((0.0, 0.0, 0.0, 1.0, 7.0, 0.0), n=2, frames=2) == ("origin 1, (1, 7) m, lies outside the grid",) * 2
    assert metres((0.0, 0.0, 0.0, np.inf, 7.0, 0.0), n=2, frames=2) == ("origin 1, (inf, 7), is not finite", "origin 1, (inf, 7, 0), is not finite")
    # the height alone is the viewshed's to refuse, in the same sentence
    xyz = np.array((0.5, 0.5, np.nan), np.float64)
    assert lib.pwpp_viewshed_obstacles(fake, ctypes.byref(g), 0.2, 2.5, 1, 1, vp(xyz), 1, 0, 0, 1, H, vp(first), None, None, None) == E_ARG
    assert err() == "origin 0, (0.5, 0.5, nan), is not finite"

    cnt = np.zeros(16, np.int32)

    def cells(xy, n=1, frames=1):
        """the messages of (pwpp_visibility_grid, pwpp_viewshed_grid) for origin cells given as rows of ox, oy (the eye: 1700)"""
        two = np.array(xy, np.int32).reshape(n, 2)
        three = np.ascontiguousarray(np.concatenate([two, np.full((n, 1), 1700, np.int32)], 1))
        assert lib.pwpp_visibility_grid(fake, 4, 4, frames, H, vp(cnt), 1, vp(two), n, 0, vp(first), None) == E_ARG
        a = err()
        assert lib.pwpp_viewshed_grid(fake, 4, 4, frames, H, vp(cnt), 1, None, None, None, 1, vp(three), n, 0, vp(first), None, None) == E_ARG
        return a, err()

    assert cells((4, 0)) == ("origin 0, cell (4, 0), lies outside the 4 x 4 cells",) * 2
    assert cells((0, -1)) == ("origin 0, cell (0, -1), lies outside the 4 x 4 cells",) * 2
    assert cells((0, 0, 3, 3, 3, 4), n=3, frames=3) == ("origin 2, cell (3, 4), lies outside the 4 x 4 cells",) * 2


CPP = r"""
#include "patchwork/patchworkpp.h"
#ifndef PWPP_HAS_VIEWSHED
#error "include/pwpp.h does not announce the viewshed"
#endif
static_assert(PWPP_VIEW_NO_HEIGHT == INT32_MIN && PWPP_VIEW_MAX_RISE == (1 << 20) && PWPP_VIEW_UNITS_PER_M == 1024, "heights");
double use(patchwork::PatchWorkpp &pw) {
    patchwork::PatchWorkpp::ObstacleViewshed v = pw.getObstacleViewshed(-40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f);
    patchwork::PatchWorkpp::ObstacleViewshed w = pw.getObstacleViewshed(-40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f, 2, 0, 40, 1.5, -0.5, 0.1, true);
    return v.first[3 * 160 + 5] + v.shadow[9] + v.occupancy[7] + (double)w.first.size() + w.nx + w.ny + (w.shadow[0] == PWPP_VIEW_NO_HEIGHT ? 1.0 : 0.0);
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_method_compiles(tmp_path, flavour):
    src = tmp_path / "viewshed.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    cmd += ["-DPWPP_NO_EIGEN"] if flavour == "plain" else ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "viewshed.c"
    src.write_text('#include "pwpp.h"\nint f(void) { return pwpp_viewshed_grid(0, 1, 1, 1, PWPP_MEM_HOST, 0, 1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0) + '
                   'pwpp_rasterize_ground_returns(0, 0, 0, 1, PWPP_MEM_HOST, 0) + '
                   'pwpp_viewshed_obstacles(0, 0, 0.2f, 2.5f, 1, 1, 0, 1, 0, 0, 1, PWPP_MEM_HOST, 0, 0, 0, 0) + (int)pwpp_viewshed_units(1.0) + '
                   '(PWPP_VIEW_NO_HEIGHT < 0) + PWPP_VIEW_MAX_RISE + PWPP_VIEW_UNITS_PER_M; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# ---- the restatement itself ---------------------------------------------------------------------------------------------------
SHAPES = [(5, 7), (33, 31), (65, 63)]
shape_ids = lambda s: "%dx%d" % s


def scenes(nx, ny):
    """(count, origin with an eye, block, target) of a shape: three fills, origins in a corner, in the middle and on an edge."""
    for k, (fill, o) in enumerate(((0.05, (0, 0)), (0.4, (nx // 2, ny // 2)), (0.05, (nx - 1, ny // 3)))):
        eye = 1700 - 900 * k
        yield ov.random_count(nx, ny, fill, 1, 7 + nx + k), o + (eye,), vr.random_heights((ny, nx), eye, 11 + nx + k), vr.random_heights((ny, nx), eye, 23 + nx + k)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_theorem_1_degenerate_input_is_the_2d_operator(shape):
    for count, o, block, target in scenes(*shape):
        for max_range in (0, 7):
            first, shadow, occ = vr.viewshed_frames(count[None], o, max_range=max_range)
            want = ov.first_of(count, o[:2], 1, max_range)
            assert np.array_equal(first[0], want) and np.array_equal(occ[0], ov.occupancy_of(count, want))
            blocked = (want >= 0) & (want != np.arange(count.size).reshape(count.shape))
            assert ((shadow[0] == vr.INT32_MAX) == blocked).all() and (shadow[0][~blocked] == vr.NO_HEIGHT).all()


@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_theorem_2_the_2d_free_cells_are_a_subset(shape):
    more = 0
    for count, o, block, target in scenes(*shape):
        for b, t in ((block, target), (block, None), (None, target)):
            occ = vr.viewshed_frames(count[None], o, None if b is None else b[None], None if t is None else t[None])[2][0]
            occ2 = ov.occupancy_of(count, ov.first_of(count, o[:2]))
            assert (occ[occ2 == ov.FREE] == vr.FREE).all() and np.array_equal(occ == vr.OCCUPIED, occ2 == ov.OCCUPIED)
            more += int(((occ == vr.FREE) & (occ2 != ov.FREE)).sum())
            assert b is not None and t is not None or np.array_equal(occ, occ2)  # without either image every line with a blocker is hidden
    assert more > 0, "no cell is seen over an obstacle: the heights do not discriminate"


@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_theorem_3_max_range_changes_nothing_inside_it(shape):
    nx, ny = shape
    iy, ix = np.mgrid[0:ny, 0:nx]
    for count, o, block, target in scenes(nx, ny):
        seen = (np.arange(nx * ny).reshape(ny, nx) % 5 == 0).astype(np.int32)
        unlimited = vr.viewshed_frames(count[None], o, block[None], target[None], seen[None])
        assert (unlimited[0] != vr.BEYOND).all()
        n = np.maximum(np.abs(ix - o[0]), np.abs(iy - o[1]))
        for max_range in (1, 7, 200):
            got = vr.viewshed_frames(count[None], o, block[None], target[None], seen[None], max_range=max_range)
            far = n > max_range
            assert (got[0][0][far] == vr.BEYOND).all() and (got[1][0][far] == vr.NO_HEIGHT).all()
            for a, b in zip(got, unlimited):
                assert np.array_equal(a[0][~far], b[0][~far])
            # beyond range: occupied stays occupied, a witnessed cell stays free, the others are unknown
            assert np.array_equal(got[2][0][far], np.where(count >= 1, vr.OCCUPIED, np.where(seen >= 1, vr.FREE, vr.UNKNOWN))[far])
        some = np.array([(0, 0), (nx - 1, ny - 1), (nx // 2, 0), o[:2]])
        f, s, _ = vr.viewshed_of(count, o, block, target, cells=some)  # the form over a list of cells
        assert np.array_equal(f, unlimited[0][0][some[:, 1], some[:, 0]]) and np.array_equal(s, unlimited[1][0][some[:, 1], some[:, 0]])


def test_theorem_4_the_kerb():
    count, block, target, origin = vr.kerb_row()
    first, shadow, occ = vr.viewshed_frames(count[None], origin, block[None], target[None])
    assert np.nonzero((first[0, 0] == 4) & (np.arange(40) != 4))[0].tolist() == list(range(5, 34))
    assert first[0, 0, 4] == 4 and (first[0, 0, :4] == vr.NONE).all() and (first[0, 0, 34:] == vr.NONE).all()
    assert shadow[0, 0, 10] == 1200 and shadow[0, 0, 34] == 0 and (shadow[0, 0, :5] == vr.NO_HEIGHT).all()
    assert (occ[0, 0, 5:34] == vr.UNKNOWN).all() and (occ[0, 0, 34:] == vr.FREE).all() and occ[0, 0, 4] == vr.OCCUPIED
    assert (ov.occupancy_of(count, ov.first_of(count, (0, 0)))[0, 5:] == ov.UNKNOWN).all()  # the 2-D shadow runs to the edge
    seen = np.zeros((1, 40), np.int32)
    seen[0, [7, 20]] = [2, 1]
    occ = vr.viewshed_frames(count[None], origin, block[None], target[None], seen[None], min_seen=2)[2]
    assert occ[0, 0, 7] == vr.FREE and occ[0, 0, 20] == vr.UNKNOWN  # a witnessed cell in the shadow is free


@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_hidden_iff_the_target_is_below_the_shadow(shape):
    hidden_cells = seen_over = 0
    for count, o, block, target in scenes(*shape):
        first, shadow, t = vr.viewshed_of(count, o, block, target)
        hidden = vr.hidden_of(count, first)
        rise = np.where(shadow == vr.INT32_MAX, vr.OPAQUE, shadow.astype(np.int64) - o[2])
        below = (shadow != vr.NO_HEIGHT) & (t < rise)  # (t is BELOW for minus infinity: under every rise)
        assert np.array_equal(hidden, below)
        hidden_cells += int(hidden.sum())
        seen_over += int(((shadow != vr.NO_HEIGHT) & ~hidden).sum())
    assert hidden_cells > 0 and seen_over > 0


def test_rule_a_with_unequal_rises_reports_the_lower_cell():
    count = np.zeros((4, 4), np.int32)
    count[0, 1] = count[1, 0] = 1            # A = (0, 1) -> index 4, B = (1, 0) -> index 1, squeezing the diagonal from (0, 0)
    target = np.zeros((4, 4), np.int32)
    for hb, ha, want in ((500, 300, 4), (300, 500, 1), (400, 400, 1), (vr.NO_HEIGHT, 300, 4), (300, vr.NO_HEIGHT, 1), (vr.NO_HEIGHT, vr.NO_HEIGHT, 1)):
        block = np.full((4, 4), vr.NO_HEIGHT, np.int32)
        block[0, 1], block[1, 0] = hb, ha
        first, shadow, _ = vr.viewshed_of(count, (0, 0, 0), block, target)  # the eye on the ground: any positive rise hides
        assert first[1, 1] == first[2, 2] == first[3, 3] == want, (hb, ha)
        low = min(h for h in (hb, ha) if h != vr.NO_HEIGHT) if (hb, ha) != (vr.NO_HEIGHT,) * 2 else None
        # the gap is as high as its LOWER side, at D = 1: the shadow at (1, 1), n = 1, is eye + low * 2
        assert shadow[1, 1] == (vr.INT32_MAX if low is None else low * 2)
    # an eye above the lower side sees over the gap to ground far enough away; one below both does not
    block = np.full((4, 4), vr.NO_HEIGHT, np.int32)
    block[0, 1], block[1, 0] = 900, 100
    assert vr.viewshed_of(count, (0, 0, 200), block, target)[0][3, 3] == vr.NONE   # r = -100, t = -200, n = 3, D = 1: -600 > -200 is false
    assert vr.viewshed_of(count, (0, 0, 50), block, target)[0][3, 3] == 4          # r = 50 > 0 > t


# ---- the kernels' functions and sequence on the host -----------------------------------------------------------------------------
def test_viewshed_program_builds_and_passes(tmp_path):
    exe = tmp_path / "viewshed_check"
    flags = SANITIZE if sanitizers_work(tmp_path) else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags +
                   ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "viewshed_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)  # (a stand-alone child process with its own main)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout and "17252 cases" in r.stdout and " 0 theorem failures" in r.stdout
