"""No-GPU checks of the cost-to-reach field (pwpp_reach_grid, pwpp_reach_ground): the exports, the feature macro and its place, the
size of pwpp_reach_params, the ctypes prototypes and the bindings' methods, every argument check that needs no device with its
message and its place in the order -- the range bound exactly at and one past its limit, clearance2 ignored without dist2 -- the C++
mirror in both flavours; pwpp_grid_cell_of, the raster's cell rule for one position; the properties of the restatement the GPU tests compare against (tests/reach_ref.py): the symmetries of the
square, monotonicity, max_reach as a mask, from chains, the octile closed form; and the stand-alone program that runs the kernels'
functions on the host against a brute force of its own (tools/reach_check.cpp), built with the address and undefined-behaviour
sanitizers where the toolchain has them; the same program evaluates images for the restatement to compare with."""
import ctypes
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
    assert int(r.stdout.split("reach_check: ")[1].split(" cases")[0]) >= 3000


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
