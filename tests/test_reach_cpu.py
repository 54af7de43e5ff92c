"""No-GPU checks of the cost-to-reach field (pwpp_reach_grid, pwpp_reach_ground): the exports, the feature macro and its place, the
size of pwpp_reach_params, the ctypes prototypes and the bindings' methods, every argument check that needs no device with its
message and its place in the order -- the range bound exactly at and one past its limit, clearance2 ignored without dist2 -- the C++
mirror in both flavours; pwpp_grid_cell_of, the raster's cell rule for one position; the properties of the restatement the GPU tests compare against (tests/reach_ref.py): the symmetries of the
square, monotonicity, max_reach as a mask, from chains, the octile closed form; and the stand-alone program that runs the kernels'
functions on the host against a brute force of its own (tools/reach_check.cpp), built with the address and undefined-behaviour
sanitizers where the toolchain has them; the same program evaluates images for the restatement to compare with; rr.certify, the
check of a finished field that the frames too large for a Dijkstra are held to: accepted every result of the Dijkstra, refused every
kind of wrong field a lost or late dirty mark would leave; and the frames of many tiles of tests/test_gpu_reach_large.py, built here
and shown on the reference alone to use every tile and to cross the words of the tiled kernel's dirty bits."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import pwpp_hip
import reach_ref as rr

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
    for name in ("pwpp_reach_grid", "pwpp_reach_ground", "pwpp_grid_cell_of"):
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr
    assert "#define PWPP_HAS_REACH 1" in hdr and "#define PWPP_REACH_NONE 0x7fffffff" in hdr
    assert "#define PWPP_VERSION_MINOR 4 " in hdr
    assert '"reach_path"' in hdr and "typedef struct pwpp_reach_params {" in hdr
    # declared directly after the terrain analysis and before the input transforms
    assert hdr.index("PWPP_API int pwpp_terrain_ground(") < hdr.index("PWPP_HAS_REACH") < hdr.index("PWPP_API int pwpp_reach_grid(")
    assert hdr.index("PWPP_API int pwpp_reach_ground(") < hdr.index("PWPP_API int pwpp_grid_cell_of(") < hdr.index("pwpp_set_input_transforms(")
    between = hdr[hdr.index("PWPP_API int pwpp_terrain_ground("):hdr.index("#define PWPP_HAS_REACH")]
    assert "PWPP_API" not in between[10:] and "#define" not in between
    assert ctypes.sizeof(pwpp_hip.ReachParams) == 24 and pwpp_hip.REACH_NONE == 0x7FFFFFFF == rr.NONE
    assert [f[0] for f in pwpp_hip.ReachParams._fields_] == ["base", "lethal", "unknown", "clearance2", "max_reach", "pad_"]
    assert all(f[1] is ctypes.c_int32 for f in pwpp_hip.ReachParams._fields_)
    assert len(lib.pwpp_reach_grid.argtypes) == 12 and len(lib.pwpp_reach_ground.argtypes) == 12
    for name in ("reach_grid", "reach_grid_device", "reach_ground", "reach_ground_device"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    import pypatchworkpp
    assert hasattr(pypatchworkpp.patchworkpp, "getReach") and hasattr(pypatchworkpp.patchworkpp, "fusedReach")
    p = pypatchworkpp.ReachParams()
    assert (p.base, p.lethal, p.unknown, p.clearance2, p.max_reach) == (1, 100, -1, 0, 0)
    doc = pypatchworkpp.patchworkpp.getReach.__doc__
    assert "terrain_params:" in doc and "reach_params:" in doc and "source_x:" in doc and "= 0.0, source_y:" in doc and "= 0.0, ground_only: bool = False)" in doc
    doc = pypatchworkpp.patchworkpp.fusedReach.__doc__
    assert "terrain_params:" in doc and "reach_params:" in doc and "= 0.0, source_y:" in doc and doc.count("= 0.0") == 2
    src = open(os.path.join(PKG, "csrc", "pwpp_reach.h")).read()
    assert "#define PWPP_REACH_TILE_X %d " % TILE_X in src and "#define PWPP_REACH_TILE_Y %d\n" % TILE_Y in src


def tile_constants():
    src = open(os.path.join(PKG, "csrc", "pwpp_reach.h")).read()
    return tuple(int(src.split("#define PWPP_REACH_TILE_%s " % a)[1].split()[0]) for a in "XY")


TILE_X, TILE_Y = tile_constants()


def params(**kw):
    f = dict(base=1, lethal=100, unknown=-1, clearance2=0, max_reach=0, pad_=0)
    f.update(kw)
    return pwpp_hip.ReachParams(**f)


def tparams(**kw):
    f = dict(radius=1, min_known=3, step_max=0.2, slope_max=0.3, rough_max=0.05, pad_=0)
    f.update(kw)
    return pwpp_hip.TerrainParams(**f)


def test_every_argument_is_named_before_the_device_is_touched_and_in_order(lib):
    cost = np.zeros(16, np.int8)
    dist2, reach, frm = np.zeros(16, np.int32), np.zeros(16, np.int32), np.zeros(16, np.int32)
    src = np.array([[1, 2]], np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    at = lambda a, n: ctypes.c_void_p(a.ctypes.data + n)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    H, D = pwpp_hip.MEM_HOST, pwpp_hip.MEM_DEVICE
    err = lib.pwpp_last_error
    P = lambda **kw: ctypes.byref(params(**kw))

    def grid(h=fake, nx=4, ny=4, frames=1, mem=2, cost=vp(cost), dist2=None, p=P(), source=vp(src), n_sources=1, reach=vp(reach), frm=vp(frm)):
        return lib.pwpp_reach_grid(h, nx, ny, frames, mem, cost, dist2, p, source, n_sources, reach, frm)

    ok = b"PWPP_MEM_HOST or"  # (mem = 2, PWPP_MEM_HOST_PINNED: every check before mem has passed)
    # 1 null pointers
    assert grid(h=None) == E_ARG and b"null handle" in err()
    assert grid(cost=None) == E_ARG and b"null cost image" in err()
    assert grid(p=None) == E_ARG and b"null reach parameters" in err()
    assert grid(source=None) == E_ARG and b"null source" in err()
    assert grid(reach=None) == E_ARG and b"null reach image" in err()
    assert grid(frm=None) == E_ARG and ok in err()  # from may be absent
    # 2 the images
    for kw in (dict(frames=0), dict(nx=0), dict(ny=-1)):
        assert grid(**kw) == E_ARG and b"cells" in err(), kw
    for kw in (dict(nx=32769), dict(ny=32769)):
        assert grid(**kw) == E_ARG and b"32768 a side" in err(), kw
    assert grid(nx=32768, ny=32768, frames=3) == E_ARG and b"exceed 2^31" in err()
    # 3 the parameters, each at both ends
    for v in (0, -1, 256):
        assert grid(p=P(base=v)) == E_ARG and b"base %d: 1 .. 255" % v in err()
    for v in (0, 102, -5):
        assert grid(p=P(lethal=v)) == E_ARG and b"lethal %d: 1 .. 101" % v in err()
    for v in (-2, 101):
        assert grid(p=P(unknown=v)) == E_ARG and b"unknown %d: -1" % v in err()
    assert grid(p=P(clearance2=-1), dist2=vp(dist2)) == E_ARG and b"clearance2 -1" in err()
    assert grid(p=P(clearance2=-1)) == E_ARG and ok in err()  # read only with dist2
    assert grid(p=P(max_reach=-1)) == E_ARG and b"max_reach -1" in err()
    assert grid(p=P(pad_=7)) == E_ARG and b"pad_ 7" in err()
    for kw in (dict(base=1, lethal=1, unknown=-1), dict(base=255, lethal=101, unknown=100, max_reach=2 ** 31 - 1)):
        assert grid(p=P(**kw)) == E_ARG and ok in err(), kw
        assert grid(p=P(clearance2=2 ** 31 - 1, **kw), dist2=vp(dist2)) == E_ARG and ok in err(), kw
    # 4 the range, exactly at and one past its limit: 14 * (base + 100) * (nx * ny - 1) <= 2^31 - 2
    big, big_reach = np.zeros(1600000, np.int8), np.zeros(1600000, np.int32)  # (never read: mem = 2 stops the call; real, so that no ranges meet)
    exact = 0
    for base in (1, 2, 41, 100, 255):
        most = (2 ** 31 - 2) // (14 * (base + 100)) + 1  # the largest number of cells
        fit = [(x, most // x) for x in range(32768, 0, -1) if most % x == 0 and most // x <= 32768][:1]
        for nx, ny in fit:  # exactly at the limit, where the count factors into two sides, and one cell past it
            exact += 1
            assert rr.range_ok(base, nx, ny) and not rr.range_ok(base, nx * ny + 1, 1)
            assert grid(nx=nx, ny=ny, p=P(base=base), cost=vp(big), reach=vp(big_reach), frm=None) == E_ARG and ok in err(), (base, nx, ny)
        past = [(x, (most + 1) // x) for x in range(32768, 0, -1) if (most + 1) % x == 0 and (most + 1) // x <= 32768][:1]
        for nx, ny in past:
            exact += 1
            assert grid(nx=nx, ny=ny, p=P(base=base), cost=vp(big), reach=vp(big_reach), frm=None) == E_ARG and b"exceeds 2^31 - 2" in err(), (base, nx, ny)
        nx = 32768
        ny = most // nx  # the last whole row at the limit and the first one past it
        assert rr.range_ok(base, nx, ny) and not rr.range_ok(base, nx, ny + 1)
        assert grid(nx=nx, ny=ny, p=P(base=base), cost=vp(big), reach=vp(big_reach), frm=None) == E_ARG and ok in err(), (base, ny)
        assert grid(nx=nx, ny=ny + 1, p=P(base=base), cost=vp(big), reach=vp(big_reach), frm=None) == E_ARG and b"exceeds 2^31 - 2" in err(), (base, ny)
        assert b"= %d " % (14 * (base + 100) * (nx * (ny + 1) - 1)) in err()
    assert exact >= 4  # (most and most + 1 factor into two sides for several of the bases)
    assert not rr.range_ok(1, 1518731, 1) and rr.range_ok(1, 1518730, 1)
    assert grid(nx=1229, ny=1236, p=P(base=1), cost=vp(big), reach=vp(big_reach), frm=None) == E_ARG and b"exceeds 2^31 - 2" in err()  # 1519044 cells
    assert grid(nx=1229, ny=1235, p=P(base=1), cost=vp(big), reach=vp(big_reach), frm=None) == E_ARG and ok in err()                  # 1517815 cells
    # 5 the sources: their number, then each
    for n, frames in ((0, 1), (2, 1), (2, 3), (-1, 1)):
        assert grid(n_sources=n, frames=frames) == E_ARG and b"%d sources for %d frames" % (n, frames) in err()
    for bad in ((-1, 0), (4, 0), (0, -1), (0, 4)):
        s = np.array([[0, 0], bad], np.int32)
        assert grid(source=vp(s), n_sources=2, frames=2, cost=vp(np.zeros(32, np.int8)), reach=vp(np.zeros(32, np.int32)), frm=None) == E_ARG
        assert b"source 1, cell (%d, %d), lies outside the 4 x 4 cells" % bad in err()
    # 6 the overlaps: 16 cells, bytes of 16 and int32 of 64 bytes
    assert grid(reach=vp(frm)) == E_ARG and b"reach and from overlap" in err()
    assert grid(dist2=vp(reach)) == E_ARG and b"dist2 and reach overlap" in err()
    assert grid(cost=at(reach, 63)) == E_ARG and b"cost and reach overlap" in err()
    assert grid(cost=at(frm, 0)) == E_ARG and b"cost and from overlap" in err()
    assert grid(dist2=at(frm, 4)) == E_ARG and b"dist2 and from overlap" in err()
    both = np.zeros(32, np.int32)
    assert grid(reach=vp(both), frm=at(both, 64)) == E_ARG and ok in err()  # touching ranges do not overlap
    # 7 mem; 8 device alignment: the int32 images, not the bytes
    assert grid(mem=2) == E_ARG and b"PWPP_MEM_HOST or PWPP_MEM_DEVICE" in err()
    assert grid(mem=7) == E_ARG and b"mem 7" in err()
    assert grid(mem=D, reach=at(both, 2)) == E_ARG and b"reach image must be 4-byte aligned" in err()
    assert grid(mem=D, frm=at(both, 1)) == E_ARG and b"from image must be 4-byte aligned" in err()
    assert grid(mem=D, dist2=at(both, 67)) == E_ARG and b"dist2 image must be 4-byte aligned" in err()
    # the order
    assert grid(cost=None, frames=0) == E_ARG and b"null cost" in err()
    assert grid(frames=0, p=P(base=0)) == E_ARG and b"0 frames of 4 x 4" in err()
    assert grid(nx=32769, p=P(base=0)) == E_ARG and b"32768 a side" in err()
    assert grid(p=P(base=0, lethal=0)) == E_ARG and b"base 0" in err()
    assert grid(p=P(lethal=0, unknown=-2)) == E_ARG and b"lethal 0" in err()
    assert grid(p=P(unknown=-2, max_reach=-1)) == E_ARG and b"unknown -2" in err()
    assert grid(p=P(clearance2=-1, max_reach=-1), dist2=vp(dist2)) == E_ARG and b"clearance2 -1" in err()
    assert grid(p=P(max_reach=-1, pad_=1)) == E_ARG and b"max_reach -1" in err()
    assert grid(p=P(pad_=1), nx=32768, ny=32768) == E_ARG and b"pad_ 1" in err()
    assert grid(nx=32768, ny=32768, n_sources=0, cost=vp(big), reach=vp(big_reach), frm=None) == E_ARG and b"exceeds 2^31 - 2" in err()
    assert grid(n_sources=0, reach=vp(frm)) == E_ARG and b"0 sources" in err()
    assert grid(source=vp(np.array([[9, 9]], np.int32)), reach=vp(frm)) == E_ARG and b"source 0, cell (9, 9)" in err()
    assert grid(reach=vp(frm), mem=7) == E_ARG and b"overlap" in err()
    assert grid(mem=7, reach=at(both, 2)) == E_ARG and b"mem 7" in err()

    def G(**kw):
        return ctypes.byref(pwpp_hip.GroundGrid(**dict(dict(x0=-2.0, y0=-2.0, cell=1.0, nx=4, ny=4, flags=0, pad_=0), **kw)))

    xy = np.array([[0.5, 0.5]], np.float64)
    cst = np.zeros(16, np.int8)

    def ground(h=fake, gr=G(), frames=1, mem=2, tp=ctypes.byref(tparams()), p=P(), source=vp(xy), n_sources=1, reach=vp(reach), frm=vp(frm), cost=None):
        return lib.pwpp_reach_ground(h, gr, 0, frames, mem, tp, p, source, n_sources, reach, frm, cost)

    assert ground(h=None) == E_ARG and b"null handle" in err()
    assert ground(gr=None) == E_ARG and b"null grid" in err()
    assert ground(tp=None) == E_ARG and b"null terrain parameters" in err()
    assert ground(p=None) == E_ARG and b"null reach parameters" in err()
    assert ground(source=None) == E_ARG and b"null source" in err()
    assert ground(reach=None) == E_ARG and b"null reach image" in err()
    assert ground() == E_ARG and ok in err()
    assert ground(frm=None, cost=vp(cst)) == E_ARG and ok in err()
    assert ground(frames=0) == E_ARG and b"0 frames" in err()
    assert ground(gr=G(nx=0)) == E_ARG and b"cells" in err()
    assert ground(gr=G(nx=32769)) == E_ARG and b"32768 a side" in err()
    assert ground(gr=G(flags=2)) == E_ARG and b"grid flags 2" in err()
    assert ground(gr=G(flags=1), tp=ctypes.byref(tparams(radius=9))) == E_ARG and b"radius 9" in err()  # PWPP_GRID_GROUND_ONLY is accepted
    assert ground(tp=ctypes.byref(tparams(min_known=10)), p=P(base=0)) == E_ARG and b"min_known 10" in err()
    assert ground(tp=ctypes.byref(tparams(pad_=3)), p=P(base=0)) == E_ARG and b"pad_ 3 of the terrain" in err()
    assert ground(p=P(base=0), gr=G(cell=0.0)) == E_ARG and b"base 0" in err()
    assert ground(p=P(lethal=102)) == E_ARG and b"lethal 102" in err()
    assert ground(p=P(clearance2=-1)) == E_ARG and ok in err()  # no dist2 in this call
    assert ground(p=P(pad_=2)) == E_ARG and b"pad_ 2 of the reach" in err()
    assert ground(gr=G(nx=32768, ny=32768), n_sources=0) == E_ARG and b"exceeds 2^31 - 2" in err()
    assert ground(gr=G(cell=0.0), n_sources=0) == E_ARG and b"cell size" in err()
    assert ground(gr=G(x0=NAN)) == E_ARG and b"finite" in err()
    for n, frames in ((0, 1), (2, 1), (2, 3)):
        assert ground(n_sources=n, frames=frames) == E_ARG and b"%d sources for %d frames" % (n, frames) in err()
    for bad, text in (((NAN, 0.0), b"is not finite"), ((0.0, INF), b"is not finite"), ((2.0, 0.0), b"lies outside the grid"), ((0.0, -2.5), b"lies outside the grid")):
        s = np.array([[0.0, 0.0], bad], np.float64)
        assert ground(source=vp(s), n_sources=2, frames=2, reach=vp(both), frm=None) == E_ARG and b"source 1, " in err() and text in err(), bad
    assert ground(source=vp(np.array([[-2.0, 1.999]])), reach=vp(frm)) == E_ARG and b"reach and from overlap" in err()  # the grid's own corner cells are inside
    assert ground(cost=at(reach, 63)) == E_ARG and b"cost and reach overlap" in err()
    assert ground(cost=at(frm, 3)) == E_ARG and b"cost and from overlap" in err()
    assert ground(source=vp(np.array([[5.0, 5.0]])), reach=vp(frm)) == E_ARG and b"source 0" in err()
    assert ground(mem=2, reach=at(both, 2)) == E_ARG and ok in err()  # the raster's own checks come before the alignment


def test_the_cell_of_a_position_is_the_rasters_rule(lib):
    """pwpp_grid_cell_of: what pwpp_reach_ground does to a source in metres, for the callers of pwpp_reach_grid (fusedReach)."""
    err = lib.pwpp_last_error
    ix, iy = ctypes.c_int32(-9), ctypes.c_int32(-9)

    def cell(x, y, **kw):
        g = pwpp_hip.GroundGrid(**dict(dict(x0=-2.0, y0=-1.0, cell=0.5, nx=8, ny=6, flags=0, pad_=0), **kw))
        rc = lib.pwpp_grid_cell_of(ctypes.byref(g), x, y, ctypes.byref(ix), ctypes.byref(iy))
        return rc if rc else (ix.value, iy.value)

    assert cell(-2.0, -1.0) == (0, 0) and cell(1.999, 1.999) == (7, 5) and cell(-0.0, 0.0) == (4, 2) and cell(0.49, 0.5) == (4, 3)
    assert cell(0.3, 0.3, flags=1) == (4, 2)   # the flags are not read
    for x, y in ((2.0, 0.0), (0.0, 2.0), (-2.001, 0.0), (0.0, -1.5), (1e300, 0.0)):
        assert cell(x, y) == E_ARG and b"position 0, " in err() and b"lies outside the grid" in err(), (x, y)
    for x, y in ((NAN, 0.0), (0.0, NAN), (INF, 0.0), (0.0, -INF)):
        assert cell(x, y) == E_ARG and b"is not finite" in err(), (x, y)
    assert cell(0.0, 0.0, cell=0.0) == E_ARG and b"cell size" in err()
    assert cell(0.0, 0.0, x0=NAN) == E_ARG and b"finite" in err()
    assert cell(0.0, 0.0, nx=0) == E_ARG and b"grid of 0 x 6 cells" in err()
    assert lib.pwpp_grid_cell_of(None, 0.0, 0.0, ctypes.byref(ix), ctypes.byref(iy)) == E_ARG and b"null grid" in err()
    g = pwpp_hip.GroundGrid(-2.0, -1.0, 0.5, 8, 6, 0, 0)
    assert lib.pwpp_grid_cell_of(ctypes.byref(g), 0.0, 0.0, None, ctypes.byref(iy)) == E_ARG and b"null cell" in err()
    mirror = open(os.path.join(PKG, "include", "patchwork", "patchworkpp.h")).read()
    assert "pwpp_grid_cell_of(" in mirror and "floor" not in mirror.split("Reach fusedReach(")[1].split("return reach_sized")[0]


CPP = r"""
#include "patchwork/patchworkpp.h"
#ifndef PWPP_HAS_REACH
#error "include/pwpp.h does not announce the cost-to-reach field"
#endif
static_assert(sizeof(pwpp_reach_params) == 24, "pwpp_reach_params");
static_assert(PWPP_REACH_NONE == 2147483647, "PWPP_REACH_NONE");
long use(patchwork::PatchWorkpp &pw) {
    patchwork::PatchWorkpp::ReachParams r;
    patchwork::PatchWorkpp::TerrainParams t;
    if (r.base != 1 || r.lethal != 100 || r.unknown != -1 || r.clearance2 != 0 || r.max_reach != 0) return -1;
    r.base = 10, r.unknown = 50, r.max_reach = 4000;
    const patchwork::PatchWorkpp::Reach a = pw.getReach(-40.0, -40.0, 0.5, 160, 160), b = pw.getReach(-40.0, -40.0, 0.5, 160, 160, t, r, 1.5, -2.0, true);
    patchwork::PatchWorkpp::FusedElevationMap map;
    map.x0 = -64.0, map.y0 = -64.0, map.cell = 0.5, map.nx = 256, map.ny = 256;
    const double pose[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    pw.updateElevationMap(map, pose, 0.0, -40.0, -40.0, 0.5, 160, 160);
    const patchwork::PatchWorkpp::Reach c = pw.fusedReach(map), d = pw.fusedReach(map, t, r, 3.0, 4.0);
    return (long)a.reach[3] + a.from[4] + b.reach[5] + c.from[6] + d.reach[7] + c.nx + d.ny;
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_method_compiles(tmp_path, flavour):
    src = tmp_path / "reach.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    cmd += ["-DPWPP_NO_EIGEN"] if flavour == "plain" else ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "reach.c"
    src.write_text('#include "pwpp.h"\nint f(const pwpp_reach_params *p, const pwpp_terrain_params *t) { return pwpp_reach_grid(0, 1, 1, 1, PWPP_MEM_HOST, 0, 0, p, 0, 1, 0, 0) + '
                   'pwpp_reach_ground(0, 0, 0, 1, PWPP_MEM_HOST, t, p, 0, 1, 0, 0, 0) + (int)sizeof(*p) + (PWPP_REACH_NONE > 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# ---- the restatement itself ---------------------------------------------------------------------------------------------------
MOVES = (lambda m: m, np.rot90, lambda m: np.rot90(m, 2), lambda m: np.rot90(m, 3), np.fliplr, np.flipud, np.transpose, lambda m: np.rot90(np.transpose(m), 2))


def test_the_eight_symmetries_of_the_square_permute_reach():
    c = rr.random_cost(1, 11, 14, 3)[0]
    p = rr.params(base=7, lethal=100, unknown=30)
    src = (4, 6)
    a, _ = rr.reach(c, src, p)
    assert (a != rr.NONE).sum() > 60
    mark = np.zeros(c.shape, np.int8)
    mark[src[1], src[0]] = 1
    seen = set()
    for move in MOVES:
        mc, mm = np.ascontiguousarray(move(c)), move(mark)
        sy, sx = np.argwhere(mm == 1)[0]
        b, _ = rr.reach(mc, (sx, sy), p)
        assert np.array_equal(b, move(a))
        seen.add((mc.shape, mc.tobytes()))
    assert len(seen) == 8


def test_raising_a_cost_never_lowers_a_value():
    rng = np.random.default_rng(5)
    c = rr.random_cost(1, 12, 12, 4, lethal=0.15)[0]
    p = rr.params(base=3, unknown=10)
    a, _ = rr.reach(c, (0, 0), p)
    for _ in range(6):
        d = c.copy()
        pick = rng.random(c.shape) < 0.2
        d[pick & (c >= 0) & (c < 90)] += 10       # dearer
        d[pick & (c >= 90) & (c < 100)] = 100     # or lethal
        b, _ = rr.reach(d, (0, 0), p)
        assert (b.astype(np.int64) >= a).all() and (b != a).any()   # (NONE is the largest value)


def test_max_reach_is_the_unlimited_field_masked():
    c = rr.random_cost(1, 13, 10, 6)[0]
    a, fa = rr.reach(c, (5, 5), rr.params(base=2, unknown=0))
    values = np.unique(a[a != rr.NONE])
    assert len(values) > 30
    for limit in (int(values[len(values) // 2]), int(values[len(values) // 2]) - 1, int(values[1]), 1, int(values[-1])):
        b, fb = rr.reach(c, (5, 5), rr.params(base=2, unknown=0, max_reach=limit))
        keep = a <= limit
        assert np.array_equal(b, np.where(keep, a, rr.NONE)) and np.array_equal(fb, np.where(keep, fa, -1))
    assert b.tobytes() == a.tobytes()   # the largest value as the limit: nothing is cut


def test_from_chains_end_at_the_source_and_fall_strictly():
    c = np.concatenate([rr.random_cost(1, 12, 12, 8)[0], rr.serpentine(9, 12)], axis=0)
    a, f = rr.reach(c, (0, 20), rr.params(base=5, unknown=-1))
    ny, nx = c.shape
    assert (a != rr.NONE).sum() > 80 and f[20, 0] == 20 * nx
    for y in range(ny):
        for x in range(nx):
            if a[y, x] == rr.NONE:
                assert f[y, x] == -1
                continue
            i, hops = y * nx + x, 0
            while i != 20 * nx:
                j = int(f.flat[i])
                assert a.flat[j] < a.flat[i] and max(abs(j // nx - i // nx), abs(j % nx - i % nx)) == 1
                i, hops = j, hops + 1
                assert hops < nx * ny


@pytest.mark.parametrize("base,c", [(1, 0), (10, 0), (255, 100), (7, 33)])
def test_an_open_uniform_field_is_the_octile_distance(base, c):
    ny, nx, sx, sy = 9, 14, 3, 6
    a, f = rr.reach(np.full((ny, nx), c, np.int8), (sx, sy), rr.params(base=base, lethal=101))
    yy, xx = np.mgrid[0:ny, 0:nx]
    dx, dy = abs(xx - sx), abs(yy - sy)
    assert np.array_equal(a, 2 * (base + c) * (5 * np.maximum(dx, dy) + 2 * np.minimum(dx, dy)))
    # ties: the smallest index wins -- straight above the source the path comes from the row above only where dx == 0
    assert f[sy + 2, sx] == (sy + 1) * nx + sx and f[sy + 2, sx + 1] == (sy + 1) * nx + sx
    assert f[sy, sx] == sy * nx + sx


def test_the_source_rule_corners_unknown_and_dist2():
    p = rr.params(base=1, lethal=100, unknown=-1)
    c = np.array([[0, 100], [100, 0]], np.int8)
    a, f = rr.reach(c, (0, 0), p)
    assert a.tolist() == [[0, rr.NONE], [rr.NONE, rr.NONE]] and f.tolist() == [[0, -1], [-1, -1]]   # the diagonal gap is closed
    a, _ = rr.reach(np.array([[0, 0], [100, 0]], np.int8), (0, 0), p)
    assert a.tolist() == [[0, 10], [rr.NONE, 20]]                                                     # no corner is cut
    a, _ = rr.reach(np.array([[100, 4], [-1, 0]], np.int8), (0, 0), p)                               # the source is lethal: t = base
    assert a.tolist() == [[0, 5 * (1 + 5)], [rr.NONE, 5 * 6 + 5 * (5 + 1)]]
    a, _ = rr.reach(np.array([[100, 4], [-1, 0]], np.int8), (0, 0), rr.params(unknown=9))            # unknown as 9: the corner opens
    assert a.tolist() == [[0, 30], [5 * (1 + 10), 7 * (1 + 1)]]
    a, _ = rr.reach(np.array([[0, 0, 0]], np.int8), (0, 0), rr.params(clearance2=0), dist2=np.array([[0, 1, rr.DIST_BEYOND]]))
    assert a.tolist() == [[0, 10, 20]]                                                                # an occupied source still starts
    a, _ = rr.reach(np.array([[0, 0, 0]], np.int8), (0, 0), rr.params(clearance2=1), dist2=np.array([[4, 1, rr.DIST_BEYOND]]))
    assert a.tolist() == [[0, rr.NONE, rr.NONE]]
    assert rr.serpentine(5, 4).tolist() == [[0, 0, 0, 0], [100, 100, 100, 0], [0, 0, 0, 0], [0, 100, 100, 100], [0, 0, 0, 0]]
    s = rr.spiral(7)
    a, _ = rr.reach(s, (0, 0), p)
    assert (a[s == 0] != rr.NONE).all() and (s == 0).sum() == 7 + 6 + 6 + 4 + 4 + 2 + 2 and a[s == 0].max() == 10 * ((s == 0).sum() - 1)


# ---- the kernels' functions on the host ----------------------------------------------------------------------------------------
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def sanitizers_work(tmp_path):
    """The toolchain links the two runtimes into a program and that program starts in this environment."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        return False
    return subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("reach_check")
    exe = tmp / "reach_check"
    flags = SANITIZE if sanitizers_work(tmp) else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off"] + flags +
                   ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "reach_check.cpp"), "-o", str(exe)], check=True)
    return exe


def test_reach_program_builds_and_passes(checker):
    r = subprocess.run([str(checker)], capture_output=True, text=True)  # (a stand-alone child process with its own main)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
    assert int(r.stdout.split("reach_check: ")[1].split(" cases")[0]) >= 4400   # (the word schedule's frames among them)


@pytest.mark.parametrize("case", ["plain", "dist2", "limited", "per_frame"])
def test_the_restatement_and_the_one_text_agree_byte_for_byte(checker, tmp_path, case):
    """The kernels' functions, dealt tile by tile and sweep by sweep on the host, against the heap Dijkstra: what the GPU tests compare, without a GPU."""
    frames, ny, nx = 3, 37, 70   # more than one tile each way, ragged
    c = rr.random_cost(frames, ny, nx, 21, lethal=0.25)
    p = rr.params(base=9, lethal=90, unknown=40 if case != "plain" else -1, clearance2=2, max_reach=9000 if case == "limited" else 0)
    d2 = np.random.default_rng(2).integers(0, 60, c.shape).astype(np.int32) if case == "dist2" else None
    if d2 is not None:
        d2[0, :5] = rr.DIST_BEYOND
    src = np.array([[33, 20], [0, 0], [69, 36]] if case == "per_frame" else [[31, 32]], np.int32)
    c.tofile(tmp_path / "cost.i8")
    src.tofile(tmp_path / "src.i32")
    if d2 is not None:
        d2.tofile(tmp_path / "dist2.i32")
    args = ["dump", str(tmp_path / "cost.i8"), str(nx), str(ny), str(frames)] + [str(p[k]) for k in ("base", "lethal", "unknown", "clearance2", "max_reach")]
    args += [str(tmp_path / "dist2.i32") if d2 is not None else "-", str(tmp_path / "src.i32"), str(len(src)), str(tmp_path / "out")]
    subprocess.run([str(checker)] + args, check=True)
    got = tuple(np.fromfile(str(tmp_path / "out") + "." + name, np.int32).reshape(c.shape) for name in ("reach", "from"))
    want = rr.reach(c, src, p, d2)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    reached = (want[0] != rr.NONE).sum()
    assert 300 < reached < c.size


# ---- a finished field judged without a Dijkstra: rr.certify ----------------------------------------------------------------------
def gpu_file_cases():
    """(what, cost, source, params, dist2) for one frame each: every shape, image, source and rule of tests/test_gpu_reach.py."""
    import test_gpu_reach as G   # (imported here: that file imports this one)
    N, TX, TY = G.N, TILE_X, TILE_Y
    for shape in G.SHAPES:
        cost, src, p, _ = G.shape_case(*shape)
        for f in range(2):
            yield "shape %s, frame %d" % (G.shape_ids(shape), f), cost[f], src[f], p, None
    for kind in ("serpentine", "spiral"):
        yield kind, G.corridor(kind)[0], (0, 0), G.FREE, None
    cost = G.field().copy()
    wall = (TX, TY + 3)
    cost[wall[1], wall[0]] = 100
    for src in ((0, 0), (N - 1, 0), (0, N - 1), (N - 1, N - 1), (TX - 1, TY), (TX, TY - 1), (2 * TX, 2 * TY), wall):   # `wall`: a lethal source
        yield "source %r" % (src,), cost, src, rr.params(base=3, unknown=20), None
    cost = np.zeros((N, N), np.int8)
    sx, sy = TX, TY - 1
    cost[sy - 1:sy + 2, sx - 1:sx + 2] = 100
    yield "sealed", cost.copy(), (sx, sy), rr.params(base=1), None
    cost[sy - 1, sx - 1] = 0
    yield "diagonal gap", cost.copy(), (sx, sy), rr.params(base=1), None
    cost[sy - 1, sx] = 0
    yield "edge gap", cost.copy(), (sx, sy), rr.params(base=1), None
    cost = np.full((N, N), 100, np.int8)
    cost[TY, 2:N - 2] = 7
    cost[TY:N - 3, N - 3] = 9
    cost[N - 4, 5:N - 2] = -1
    yield "corridor", cost, (2, TY), rr.params(base=4, unknown=11), None
    cost, src = G.field(), (N // 2, N // 2)
    for unknown in (-1, 0, 55, 100):
        yield "unknown %d" % unknown, cost, src, rr.params(base=5, unknown=unknown), None
    for lethal in (1, int(cost[(cost > 30) & (cost < 60)][0]), 101):
        yield "lethal %d" % lethal, cost, src, rr.params(base=5, lethal=lethal, unknown=0), None
    rng = np.random.default_rng(9)
    d2 = rng.integers(0, 30, cost.shape).astype(np.int32)
    d2[rng.random(cost.shape) < 0.1] = rr.DIST_BEYOND
    for clearance2 in (0, 4, 12):
        yield "clearance2 %d" % clearance2, cost, src, rr.params(base=5, unknown=0, clearance2=clearance2), d2
    yield "dist2 beyond everywhere", cost, src, rr.params(base=5, unknown=0, clearance2=2 ** 31 - 2), np.full(cost.shape, rr.DIST_BEYOND, np.int32)
    free = rr.reach(cost, src, rr.params(base=5, unknown=55))[0]
    values = np.unique(free[free != rr.NONE])
    v = int(values[len(values) // 3])
    for limit in (v, v - 1):
        yield "max_reach %d" % limit, cost, src, rr.params(base=5, unknown=55, max_reach=limit), None
    for c, base, src in ((0, 1, (0, 0)), (100, 255, (N - 1, N // 2)), (33, 7, (TX, TY))):
        yield "uniform %d" % c, np.full((N, N), c, np.int8), src, rr.params(base=base, lethal=101), None
    n, frames = 40, 64
    rng = np.random.default_rng(12)
    cost = rr.random_cost(frames, n, n, 90, lethal=0.1, unknown=0.05)
    for f in range(0, frames, 2):
        cost[f, n // 2, :] = 100
        cost[f, n // 2, (7 * f) % n] = 0
    src = np.stack([rng.integers(0, n, frames), rng.integers(0, n, frames)], axis=1).astype(np.int32)
    for f in (0, 1, 2, 31, 62, 63):   # per-frame sources
        yield "frame %d of 64" % f, cost[f], src[f], rr.params(base=2, unknown=30), None


def rejected(verdict, near, reach_shape):
    """`verdict` is a reason and a cell; the cell lies in the rectangle `near` = (x0, y0, x1, y1) or beside it (a wrong value also
    spoils what its neighbours are offered, and the first cell in index order is named)."""
    assert verdict is not None, "a wrong field was accepted"
    reason, (x, y) = verdict
    assert isinstance(reason, str) and len(reason.strip()) > 10
    assert near[0] - 1 <= x <= near[2] + 1 and near[1] - 1 <= y <= near[3] + 1, (reason, near)
    assert 0 <= x < reach_shape[1] and 0 <= y < reach_shape[0]


def test_certify_accepts_the_dijkstra_result_of_every_case_of_the_gpu_file_and_the_flat_dijkstra_gives_the_same():
    seen = 0
    for what, cost, src, p, d2 in gpu_file_cases():
        reach, frm = rr.reach(cost, src, p, d2)
        assert rr.certify(cost, src, p, reach, frm, d2) is None, what
        assert rr.certify(cost, src, p, reach, None, d2) is None, what
        flat = rr.reach_flat(cost, src, p, d2)
        assert flat[0].dtype == flat[1].dtype == np.int32 and flat[0].tobytes() == reach.tobytes() and flat[1].tobytes() == frm.tobytes(), what
        t = rr.terms_array(cost, src, p, d2)
        assert t.tolist() == rr.terms(cost, (int(src[0]), int(src[1])), p, d2), what
        seen += 1
    assert seen == 64


@pytest.fixture(scope="module")
def open_field():
    """96 x 96, 3 x 3 tiles: random costs, few walls, the source in the first tile; (cost, source, params, reach, from), never written."""
    cost = rr.random_cost(1, 3 * TILE_Y, 3 * TILE_X, 31, lethal=0.04, unknown=0.0)[0]
    src, p = (5, 7), rr.params(base=2)
    out = (cost,) + rr.reach(cost, src, p)
    for a in out:
        a.setflags(write=False)
    assert (out[1] != rr.NONE).sum() > cost.size * 9 // 10 and rr.certify(cost, src, p, out[1], out[2]) is None
    return cost, src, p, out[1], out[2]


def test_certify_rejects_a_value_one_off_a_wrong_source_and_a_tied_from(open_field):
    cost, src, p, reach, frm = open_field
    for x, y in ((50, 40), (TILE_X, TILE_Y), (95, 95), (src[0] + 1, src[1])):
        assert reach[y, x] not in (0, rr.NONE)
        for delta in (1, -1):   # (a) raised, (b) lowered
            bad = reach.copy()
            bad[y, x] += delta
            rejected(rr.certify(cost, src, p, bad, frm), (x, y, x, y), reach.shape)
            rejected(rr.certify(cost, src, p, bad, None), (x, y, x, y), reach.shape)
    for v in (1, -1, rr.NONE):   # (f) a source that does not hold 0
        bad = reach.copy()
        bad[src[1], src[0]] = v
        verdict = rr.certify(cost, src, p, bad, frm)
        rejected(verdict, src + src, reach.shape)
        assert verdict[1] == src and "source" in verdict[0]
    bad = reach.copy()   # a value on an impassable cell
    y, x = np.argwhere(cost >= 100)[5]
    bad[y, x] = 12345
    rejected(rr.certify(cost, src, p, bad, frm), (x, y, x, y), reach.shape)
    # (e) a uniform open field: one from moved to another neighbour that ties
    n, s = 3 * TILE_X, (TILE_X, TILE_Y)
    flat = np.zeros((n, n), np.int8)
    q = rr.params(base=3)
    r, f = rr.reach(flat, s, q)
    x, y = s[0] + 1, s[1] + 2
    first, other = (y - 1) * n + x - 1, (y - 1) * n + x   # across the corner and across the edge: 10 b + 14 b = 14 b + 10 b
    assert f[y, x] == first and r.flat[first] + 7 * 6 == r.flat[other] + 5 * 6 == r[y, x]
    assert rr.certify(flat, s, q, r, f) is None
    bad = f.copy()
    bad[y, x] = other
    verdict = rr.certify(flat, s, q, r, bad)
    rejected(verdict, (x, y, x, y), r.shape)
    assert verdict[1] == (x, y) and "from" in verdict[0]
    bad = f.copy()
    bad[s[1], s[0]] = -1   # the source names itself
    assert rr.certify(flat, s, q, r, bad)[1] == s
    bad = f.copy()
    bad[0, 0] = -1         # a reached cell without a from
    assert rr.certify(flat, s, q, r, bad)[1] == (0, 0)


def test_certify_rejects_a_tile_that_was_never_visited_and_a_tile_that_was_not_visited_again(open_field):
    cost, src, p, reach, frm = open_field
    x0, y0, x1, y1 = TILE_X, TILE_Y, 2 * TILE_X - 1, 2 * TILE_Y - 1   # the interior tile
    tile = (slice(y0, y1 + 1), slice(x0, x1 + 1))
    # (c) a lost dirty bit: the tile keeps its start while its neighbours have their values
    lost = (reach.copy(), frm.copy())
    lost[0][tile], lost[1][tile] = rr.NONE, -1
    rejected(rr.certify(cost, src, p, *lost), (x0, y0, x1, y1), reach.shape)
    rejected(rr.certify(cost, src, p, lost[0], None), (x0, y0, x1, y1), reach.shape)
    # (d) values that are real path lengths but not the shortest: the tile as it is with a wall inside it that forces a detour
    walled = cost.copy()
    walled[y0 + 10, x0 + 1:x1] = 100
    walled[y0 + 1:y1 - 8, x0 + 16] = 100
    assert (walled[tile] != cost[tile]).any() and walled[y0, x0:x1 + 1].tobytes() == cost[y0, x0:x1 + 1].tobytes()
    detour = rr.reach(walled, src, p)
    stale = (reach.copy(), frm.copy())
    stale[0][tile], stale[1][tile] = detour[0][tile], detour[1][tile]
    assert (stale[0][tile] != reach[tile]).sum() > 100 and (stale[0][tile] >= reach[tile]).all()
    longer = (stale[0][tile] != reach[tile]) & (stale[0][tile] != rr.NONE)
    assert longer.sum() > 100, "the wall forces no detour"
    rejected(rr.certify(cost, src, p, *stale), (x0, y0, x1, y1), reach.shape)
    rejected(rr.certify(cost, src, p, stale[0], None), (x0, y0, x1, y1), reach.shape)
    # ... and with the stale values alone, the walls' cells at their true values: every value a real path length of the image itself
    only = (np.where(detour[0] == rr.NONE, reach, stale[0]), np.where(detour[0] == rr.NONE, frm, stale[1]))
    assert (only[0][tile] != reach[tile]).sum() > 100
    rejected(rr.certify(cost, src, p, *only), (x0, y0, x1, y1), reach.shape)


def test_certify_rejects_both_sides_of_max_reach(open_field):
    cost, src, p, reach, frm = open_field
    values = np.unique(reach[reach != rr.NONE])
    limit = int(values[len(values) // 2])
    q = dict(p, max_reach=limit)
    cut = (np.where(reach <= limit, reach, rr.NONE).astype(np.int32), np.where(reach <= limit, frm, -1).astype(np.int32))
    assert rr.certify(cost, src, q, *cut) is None and rr.certify(cost, src, p, *cut) is not None
    inside, outside = np.argwhere((reach <= limit) & (reach > 0)), np.argwhere((reach > limit) & (reach != rr.NONE))
    for y, x in (inside[0], inside[len(inside) // 2], inside[-1], np.argwhere(reach == limit)[0]):   # (g) d <= limit left unreached
        bad = (cut[0].copy(), cut[1].copy())
        bad[0][y, x], bad[1][y, x] = rr.NONE, -1
        rejected(rr.certify(cost, src, q, *bad), (x, y, x, y), reach.shape)
    above = np.argwhere(reach == values[len(values) // 2 + 1])[0]
    for y, x in (outside[0], outside[len(outside) // 2], outside[-1], above):   # (g) d > limit given its true d
        bad = (cut[0].copy(), cut[1].copy())
        bad[0][y, x], bad[1][y, x] = reach[y, x], frm[y, x]
        verdict = rr.certify(cost, src, q, *bad)
        rejected(verdict, (x, y, x, y), reach.shape)
        assert verdict[1] == (x, y)   # (nothing is offered to a neighbour: every candidate through it lies above the limit too)


# ---- the frames of many tiles that tests/test_gpu_reach_large.py asks the GPU for: built here, and judged here on the reference alone ----
WORD = 32   # tiles per word of k_reach_tiles' dirty bits


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def tile_of(x, y, nx):
    return (y // TILE_Y) * ((nx + TILE_X - 1) // TILE_X) + x // TILE_X


def exercised(cost, src, want, crossings=None, every_boundary=False):
    """What the issue of the many-tile tests asks of an image before a GPU sees it, on a finished field: every tile holds a reached
    cell, 3/4 of the cells are reached, and the chain from the dearest cell back to the source, walked tile by tile, passes between the
    words of the dirty bits -- `crossings` times each way at least, or over every boundary between two words."""
    ny, nx = cost.shape
    k = rr.chain(want[0], want[1], src, TILE_X, TILE_Y)
    tiles = ((nx + TILE_X - 1) // TILE_X) * ((ny + TILE_Y - 1) // TILE_Y)
    assert k["every_tile"] and 4 * k["reached"] >= 3 * nx * ny, (k["every_tile"], k["reached"])
    assert k["tiles"][0] == tile_of(src[0], src[1], nx) and len(k["tiles"]) > 1
    if crossings is not None:
        assert k["up"] >= crossings and k["down"] >= crossings, (k["up"], k["down"])
    if every_boundary:
        w = [q // WORD for q in k["tiles"]]
        met = {(min(a, b), max(a, b)) for a, b in zip(w, w[1:]) if a != b}
        assert all(any(lo <= b < hi for lo, hi in met) for b in range((tiles - 1) // WORD)), met
    return k


COMB_SHAPE = (7 * TILE_X - 5, 6 * TILE_Y - 9)   # (nx, ny): 7 x 6 = 42 tiles; the tile above or below lies 7 indices away
COMB_P = rr.params(base=2)
# the corners, a cell of tile 32 and one of tile 31 -- the nine first marks fall into both words -- and one of the ragged last tile
COMB_SOURCES = ((0, 0), (COMB_SHAPE[0] - 1, COMB_SHAPE[1] - 1), (4 * TILE_X + 27, 4 * TILE_Y + 2), (3 * TILE_X + 7, 4 * TILE_Y + 9), (6 * TILE_X + 5, 5 * TILE_Y + 3))


@functools.lru_cache(maxsize=None)
def comb_image():
    return frozen(rr.comb(COMB_SHAPE[1], COMB_SHAPE[0], 24, 3, 1))[0]


@functools.lru_cache(maxsize=None)
def comb_case(k):
    """(cost, source, params, (reach, from)) of the two-word image for source k: a Dijkstra (rr.reach_flat; the test below holds it to
    the heap Dijkstra of rr.reach on these very images), computed once."""
    cost, src = comb_image(), COMB_SOURCES[k]
    return cost, src, COMB_P, frozen(*rr.reach_flat(cost, src, COMB_P))


STRIPS = {"row": (33 * TILE_X + 1, 3), "column": (3, 33 * TILE_Y + 1), "three_words": (65 * TILE_X + 1, 2)}   # (nx, ny): 34, 34 and 66 tiles
STRIP_P = rr.params(base=2)


def strip_image(kind):
    nx, ny = STRIPS[kind]
    c = rr.comb(min(nx, ny), max(nx, ny), 37, 1, 2 + sorted(STRIPS).index(kind))
    return frozen(np.ascontiguousarray(c.T) if ny > nx else c)[0]


def strip_sources(kind):
    """Either end, and a cell of tile 31 and of tile 32."""
    nx, ny = STRIPS[kind]
    along = lambda a: (a, 1) if nx > ny else (1, a)
    return ((0, 0), (nx - 1, ny - 1), along(31 * TILE_X + 30), along(32 * TILE_X + 1))


@functools.lru_cache(maxsize=None)
def strip_case(kind, k):
    cost, src = strip_image(kind), strip_sources(kind)[k]
    return cost, src, STRIP_P, frozen(*rr.reach(cost, src, STRIP_P))


@functools.lru_cache(maxsize=None)
def limited_strip_cases():
    """The 66-tile strip from a source in tile 32 under the largest max_reach, a value of the field, that leaves the reached cells in at
    most 4 tiles, and under one less: [(cost, source, params, (reach, from))], the unlimited field masked."""
    cost, src, p, free = strip_case("three_words", 3)
    ny, nx = cost.shape
    yy, xx = np.mgrid[0:ny, 0:nx]
    tile = tile_of(xx, yy, nx)
    values = np.unique(free[0][free[0] != rr.NONE])
    fits = [int(v) for v in values if len(np.unique(tile[free[0] <= v])) <= 4]
    limit = fits[-1]
    out = []
    for lim in (limit, limit - 1):
        keep = free[0] <= lim
        want = frozen(np.where(keep, free[0], rr.NONE).astype(np.int32), np.where(keep, free[1], -1).astype(np.int32))
        out.append((cost, src, dict(p, max_reach=lim), want))
    return out


# (nx, ny): 257 tiles in 9 words.  The frame of the most tiles the entry points accept, 23365 x 65 cells at base 1 (2193 tiles in 69 words),
# passes the same checks, but k_reach_tiles, one workgroup a frame, needs 53 s a call for a comb of that size (measured on an MI355X):
# no test for a suite.
WIDE = (257 * TILE_X - 31, 9)
WIDE_P = rr.params(base=1)
WIDE_SOURCES = ((4000, 4), (WIDE[0] - 1, WIDE[1] - 1))   # frame 0, uniform; frame 1, a comb from its far end: the front moves to smaller tile indices


@functools.lru_cache(maxsize=None)
def wide_images():
    nx, ny = WIDE
    return frozen(np.stack([np.full((ny, nx), 17, np.int8), rr.comb(ny, nx, 24, 3, 3)]))[0]


def octile(nx, ny, src, t):
    """The field of a uniform open image whose every cell has the term t."""
    yy, xx = np.mgrid[0:ny, 0:nx]
    dx, dy = abs(xx - src[0]), abs(yy - src[1])
    return (2 * t * (5 * np.maximum(dx, dy) + 2 * np.minimum(dx, dy))).astype(np.int32)


def test_the_two_word_comb_runs_back_and_forth_across_the_word_boundary():
    cost = comb_image()
    nx, ny = COMB_SHAPE
    assert (nx, ny) == (219, 183) and cost.shape == (ny, nx) and len(COMB_SOURCES) == 5
    assert [tile_of(x, y, nx) for x, y in COMB_SOURCES] == [0, 41, 32, 31, 41] and tile_of(nx - 1, ny - 1, nx) == 41
    for k, src in enumerate(COMB_SOURCES):
        _, _, p, want = comb_case(k)
        assert cost[src[1], src[0]] < 100
        found = exercised(cost, src, want, crossings=4)
        assert found["reached"] == 38457 and found["words"] == [0, 1]
        assert rr.certify(cost, src, p, *want) is None
        heap = rr.reach(cost, src, p)
        assert heap[0].tobytes() == want[0].tobytes() and heap[1].tobytes() == want[1].tobytes()
    # the nine first marks of the sources in tiles 31 and 32 fall into both words
    for x, y in COMB_SOURCES[2:4]:
        marks = {tile_of(x + ex * TILE_X, y + ey * TILE_Y, nx) // WORD for ex in (-1, 0, 1) for ey in (-1, 0, 1)}
        assert marks == {0, 1}


@pytest.mark.parametrize("kind", sorted(STRIPS))
def test_the_strips_cross_every_word_boundary_from_either_end(kind):
    nx, ny = STRIPS[kind]
    tiles = ((nx + TILE_X - 1) // TILE_X) * ((ny + TILE_Y - 1) // TILE_Y)
    assert tiles == (66 if kind == "three_words" else 34) and (kind != "column" or (nx + TILE_X - 1) // TILE_X == 1)
    assert [tile_of(x, y, nx) for x, y in strip_sources(kind)] == [0, tiles - 1, 31, 32]
    for k, src in enumerate(strip_sources(kind)):
        cost, _, p, want = strip_case(kind, k)
        assert cost.shape == (ny, nx) and cost[src[1], src[0]] < 100
        found = exercised(cost, src, want, every_boundary=k < 2)
        if k == 0:
            assert found["up"] == (tiles - 1) // WORD and found["down"] == 0 and found["tiles"] == list(range(tiles))
        if k == 1:   # the front moves to smaller tile indices: every mark waits for the next pass
            assert found["down"] == (tiles - 1) // WORD and found["up"] == 0 and found["tiles"] == list(range(tiles))[::-1]
        assert rr.certify(cost, src, p, *want) is None
    if kind == "row":
        assert (strip_case(kind, 0)[3][0] != rr.NONE).sum() == 3115


def test_max_reach_leaves_most_of_the_66_tiles_unvisited():
    free = strip_case("three_words", 3)[3]
    for n, (cost, src, p, want) in enumerate(limited_strip_cases()):
        ny, nx = cost.shape
        yy, xx = np.nonzero(want[0] != rr.NONE)
        used = set(tile_of(xx, yy, nx).tolist())
        assert 2 <= len(used) <= 4 and tile_of(src[0], src[1], nx) == 32 and 32 in used
        assert ((want[0] == p["max_reach"]).sum() >= 1) == (n == 0)   # the limit is a value of the field; one less cuts that cell
        got = rr.reach(cost, src, p)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()   # the reference prunes, `want` masks
        assert rr.certify(cost, src, p, *want) is None and rr.certify(cost, src, p, *free) is not None
    a, b = (c[3][0] for c in limited_strip_cases())
    assert (a != b).sum() >= 1 and (b[a != b] == rr.NONE).all()


def test_the_frames_of_257_tiles_are_exercised_in_every_one():
    nx, ny = WIDE
    assert (nx, ny) == (8193, 9) and (nx + TILE_X - 1) // TILE_X == 257 and (257 + WORD - 1) // WORD == 9 and rr.range_ok(WIDE_P["base"], nx, ny)
    cost = wide_images()
    # frame 0: uniform, the octile closed form
    src = WIDE_SOURCES[0]
    want = rr.reach_flat(cost[0], src, WIDE_P)
    assert want[0].tobytes() == octile(nx, ny, src, WIDE_P["base"] + 17).tobytes()
    assert rr.certify(cost[0], src, WIDE_P, *want) is None
    assert exercised(cost[0], src, want)["reached"] == nx * ny
    bad = want[0].copy()
    bad[ny - 1, nx - 1] += 1   # the one cell of the last tile's last row
    assert rr.certify(cost[0], src, WIDE_P, bad, want[1])[1] == (nx - 1, ny - 1)
    # frame 1: the comb, by both Dijkstras
    src = WIDE_SOURCES[1]
    want = rr.reach(cost[1], src, WIDE_P)
    flat = rr.reach_flat(cost[1], src, WIDE_P)
    assert flat[0].tobytes() == want[0].tobytes() and flat[1].tobytes() == want[1].tobytes()
    assert rr.certify(cost[1], src, WIDE_P, *want) is None
    found = exercised(cost[1], src, want, every_boundary=True)
    assert found["words"] == list(range(9)) and sorted(set(found["tiles"])) == list(range(257)) and found["down"] >= 8 and found["hops"] > nx
    lost = want[0].copy()
    lost[:, 200 * TILE_X:201 * TILE_X] = rr.NONE   # tile 200 never visited
    verdict = rr.certify(cost[1], src, WIDE_P, lost, None)
    assert verdict is not None and 200 * TILE_X - 1 <= verdict[1][0] <= 201 * TILE_X
