"""No-GPU checks of the terrain analysis (pwpp_terrain_grid, pwpp_terrain_ground): the exports, the feature macro and its place, the
size of pwpp_terrain_params, the ctypes prototypes and the bindings' methods, every argument check that needs no device with its
message and its place in the order, the C++ mirror in both flavours -- the properties of the restatement the GPU tests compare
against (tests/terrain_ref.py): degenerate images, three cells, an exact integer plane, height offsets, the symmetries of the square,
limit heights, non-finite values, ties, the cost rule -- and the stand-alone program that runs the kernel's functions on the host
against a brute force of its own and proves the int64 bounds (tools/terrain_check.cpp), built with the address and
undefined-behaviour sanitizers where the toolchain has them; the same program evaluates images for the restatement to compare with."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pwpp_hip
import terrain_ref as tr

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
    for name in ("pwpp_terrain_grid", "pwpp_terrain_ground"):
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr
    assert "#define PWPP_HAS_TERRAIN 1" in hdr
    assert "#define PWPP_VERSION_MINOR 4 " in hdr
    assert '"terrain_path"' in hdr and "typedef struct pwpp_terrain_params {" in hdr
    assert hdr.index("pwpp_fuse_ground(") < hdr.index("PWPP_HAS_TERRAIN") < hdr.index("pwpp_set_input_transforms(")  # declared after the elevation fusion
    assert ctypes.sizeof(pwpp_hip.TerrainParams) == 24
    assert [f[0] for f in pwpp_hip.TerrainParams._fields_] == ["radius", "min_known", "step_max", "slope_max", "rough_max", "pad_"]
    assert len(lib.pwpp_terrain_grid.argtypes) == 13 and len(lib.pwpp_terrain_ground.argtypes) == 12
    for name in ("terrain_grid", "terrain_grid_device", "terrain_ground", "terrain_ground_device"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    import pypatchworkpp
    assert hasattr(pypatchworkpp.patchworkpp, "getTerrain") and hasattr(pypatchworkpp.patchworkpp, "fusedTerrain")
    p = pypatchworkpp.TerrainParams()
    assert (p.radius, p.min_known, p.step_max, p.slope_max, p.rough_max) == (1, 3, INF, INF, INF)


def params(**kw):
    f = dict(radius=1, min_known=3, step_max=0.2, slope_max=0.3, rough_max=0.05, pad_=0)
    f.update(kw)
    return pwpp_hip.TerrainParams(**f)


def test_every_argument_is_named_before_the_device_is_touched_and_in_order(lib):
    hgt = np.zeros(64, np.float32)
    step, slope, rough = np.zeros(64, np.float32), np.zeros(64, np.float32), np.zeros(64, np.float32)
    count, cost = np.zeros(64, np.uint8), np.zeros(64, np.int8)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    at = lambda a, n: ctypes.c_void_p(a.ctypes.data + n)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    H, D = pwpp_hip.MEM_HOST, pwpp_hip.MEM_DEVICE
    err = lib.pwpp_last_error
    P = lambda **kw: ctypes.byref(params(**kw))

    def grid(h=fake, nx=4, ny=4, frames=1, cell=0.5, mem=H, height=vp(hgt), p=P(), step=vp(step), slope=vp(slope), rough=vp(rough), count=vp(count),
             cost=vp(cost)):
        return lib.pwpp_terrain_grid(h, nx, ny, frames, cell, mem, height, p, step, slope, rough, count, cost)

    none = dict(step=None, slope=None, rough=None, count=None, cost=None)
    # 1 null pointers; 2 no output at all
    assert grid(h=None) == E_ARG and b"null handle" in err()
    assert grid(height=None) == E_ARG and b"null height" in err()
    assert grid(p=None) == E_ARG and b"null terrain parameters" in err()
    assert grid(**none) == E_ARG and b"null outputs" in err()
    # 3 the images: frames and sides < 1, sides > 32768, the cells beyond 2^31; 4 the cell size
    for kw in (dict(frames=0), dict(nx=0), dict(ny=-1)):
        assert grid(**kw) == E_ARG and b"cells" in err(), kw
    for kw in (dict(nx=32769), dict(ny=32769)):
        assert grid(**kw) == E_ARG and b"32768 a side" in err(), kw
    assert grid(nx=32768, ny=32768, frames=3) == E_ARG and b"exceed 2^31" in err()
    for c in (0.0, -1.0, NAN, INF):
        assert grid(cell=c) == E_ARG and b"finite and positive" in err(), c
    # 5 the radius; 6 min_known; 7 the limits; 8 the padding
    for r in (0, -1, 5, 100):
        assert grid(p=P(radius=r)) == E_ARG and b"radius %d: 1 .. 4" % r in err()
    for r, k in ((1, 0), (1, 10), (2, 26), (4, 82), (3, -1)):
        assert grid(p=P(radius=r, min_known=k)) == E_ARG and b"min_known %d: 1 .. %d" % (k, (2 * r + 1) ** 2) in err()
    for name in ("step_max", "slope_max", "rough_max"):
        for v in (0.0, -1.0, NAN, -INF):
            assert grid(p=P(**{name: v})) == E_ARG and b"each > 0 expected" in err(), (name, v)
    assert grid(p=P(pad_=7)) == E_ARG and b"pad_ 7" in err()
    # (accepted up to mem: the ends of every range, infinite limits, a single output)
    for kw in (dict(radius=4, min_known=81), dict(radius=2, min_known=25), dict(step_max=INF, slope_max=INF, rough_max=INF), dict(rough_max=1e-30)):
        assert grid(p=P(**kw), mem=2) == E_ARG and b"PWPP_MEM_HOST or" in err(), kw
    for keep in none:
        assert grid(mem=2, **{k: None for k in none if k != keep}) == E_ARG and b"PWPP_MEM_HOST or" in err(), keep
    # 9 the overlaps: 16 cells, floats of 64 and bytes of 16 bytes
    assert grid(step=vp(hgt)) == E_ARG and b"height and step overlap" in err()
    assert grid(cost=at(hgt, 63)) == E_ARG and b"height and cost overlap" in err()
    assert grid(slope=at(step, 60)) == E_ARG and b"step and slope overlap" in err()
    assert grid(rough=vp(slope)) == E_ARG and b"slope and rough overlap" in err()
    assert grid(count=at(rough, 63)) == E_ARG and b"rough and count overlap" in err()
    assert grid(cost=at(count, 15)) == E_ARG and b"count and cost overlap" in err()
    assert grid(step=at(hgt, 64), mem=2) == E_ARG and b"PWPP_MEM_HOST or" in err()   # touching ranges do not overlap
    assert grid(cost=at(count, 16), mem=2) == E_ARG and b"PWPP_MEM_HOST or" in err()
    assert grid(slope=None, rough=vp(step), step=None, mem=2) == E_ARG and b"PWPP_MEM_HOST or" in err()
    # 10 mem; 11 device alignment: the floats, not the bytes
    assert grid(mem=2) == E_ARG and b"PWPP_MEM_HOST or PWPP_MEM_DEVICE" in err()   # PWPP_MEM_HOST_PINNED
    assert grid(mem=7) == E_ARG and b"mem 7" in err()
    big = np.zeros(40, np.float32)
    assert grid(height=at(big, 2), mem=D) == E_ARG and b"height images must be 4-byte aligned" in err()
    assert grid(step=at(big, 1), mem=D) == E_ARG and b"step must be 4-byte aligned" in err()
    assert grid(slope=at(big, 6), mem=D) == E_ARG and b"slope must be 4-byte aligned" in err()
    assert grid(rough=at(big, 3), mem=D) == E_ARG and b"rough must be 4-byte aligned" in err()
    # the order
    assert grid(height=None, **none) == E_ARG and b"null height" in err()
    assert grid(frames=0, **none) == E_ARG and b"null outputs" in err()
    assert grid(frames=0, cell=0.0) == E_ARG and b"0 frames of 4 x 4" in err()
    assert grid(nx=32769, p=P(radius=0)) == E_ARG and b"32768 a side" in err()
    assert grid(cell=0.0, p=P(radius=0)) == E_ARG and b"finite and positive" in err()
    assert grid(p=P(radius=0, min_known=0)) == E_ARG and b"radius 0" in err()
    assert grid(p=P(min_known=0, step_max=0.0)) == E_ARG and b"min_known 0" in err()
    assert grid(p=P(slope_max=NAN, pad_=1)) == E_ARG and b"each > 0" in err()
    assert grid(p=P(pad_=1), step=vp(hgt)) == E_ARG and b"pad_ 1" in err()
    assert grid(step=vp(hgt), mem=2) == E_ARG and b"overlap" in err()
    assert grid(mem=2, height=at(big, 2)) == E_ARG and b"PWPP_MEM_HOST or" in err()

    g = pwpp_hip.GroundGrid(-2.0, -2.0, 1.0, 4, 4, 0, 0)

    def G(**kw):
        return ctypes.byref(pwpp_hip.GroundGrid(**dict(dict(x0=-2.0, y0=-2.0, cell=1.0, nx=4, ny=4, flags=0, pad_=0), **kw)))

    def ground(h=fake, gr=ctypes.byref(g), frames=1, mem=H, p=P(), step=vp(step), cost=vp(cost), height=None):
        return lib.pwpp_terrain_ground(h, gr, 0, frames, mem, p, step, None, None, None, cost, height)

    assert ground(h=None) == E_ARG and b"null handle" in err()
    assert ground(gr=None) == E_ARG and b"null grid" in err()
    assert ground(p=None) == E_ARG and b"null terrain parameters" in err()
    assert ground(step=None, cost=None) == E_ARG and b"null outputs" in err()
    assert ground(frames=0) == E_ARG and b"0 frames" in err()
    assert ground(gr=G(nx=0)) == E_ARG and b"cells" in err()
    assert ground(gr=G(nx=32769)) == E_ARG and b"32768 a side" in err()
    assert ground(gr=G(flags=2)) == E_ARG and b"grid flags 2" in err()
    assert ground(gr=G(flags=1), p=P(radius=9)) == E_ARG and b"radius 9" in err()   # PWPP_GRID_GROUND_ONLY is accepted
    assert ground(p=P(min_known=10)) == E_ARG and b"min_known 10" in err()
    assert ground(p=P(rough_max=0.0)) == E_ARG and b"each > 0" in err()
    assert ground(p=P(pad_=3)) == E_ARG and b"pad_ 3" in err()
    assert ground(height=vp(step)) == E_ARG and b"height and step overlap" in err()
    assert ground(gr=G(cell=0.0), height=vp(step)) == E_ARG and b"overlap" in err()   # the raster's own checks come last
    assert ground(gr=G(cell=0.0)) == E_ARG and b"cell size" in err()
    assert ground(gr=G(x0=NAN)) == E_ARG and b"finite" in err()
    assert ground(gr=G(x0=NAN), mem=2) == E_ARG and b"finite" in err()
    assert ground(mem=2) == E_ARG and b"PWPP_MEM_HOST or" in err()


CPP = r"""
#include "patchwork/patchworkpp.h"
#ifndef PWPP_HAS_TERRAIN
#error "include/pwpp.h does not announce the terrain analysis"
#endif
static_assert(sizeof(pwpp_terrain_params) == 24, "pwpp_terrain_params");
double use(patchwork::PatchWorkpp &pw) {
    patchwork::PatchWorkpp::TerrainParams p;
    if (p.radius != 1 || p.min_known != 3 || !(p.step_max > 1e38f) || !(p.slope_max > 1e38f) || !(p.rough_max > 1e38f)) return -1.0;
    p.radius = 2, p.step_max = 0.2f;
    const patchwork::PatchWorkpp::Terrain a = pw.getTerrain(-40.0, -40.0, 0.5, 160, 160), b = pw.getTerrain(-40.0, -40.0, 0.5, 160, 160, p, true);
    patchwork::PatchWorkpp::FusedElevationMap map;
    map.x0 = -64.0, map.y0 = -64.0, map.cell = 0.5, map.nx = 256, map.ny = 256;
    const double pose[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    pw.updateElevationMap(map, pose, 0.0, -40.0, -40.0, 0.5, 160, 160);
    const patchwork::PatchWorkpp::Terrain c = pw.fusedTerrain(map), d = pw.fusedTerrain(map, p);
    return a.step[3] + a.slope[4] + b.rough[5] + c.count[6] + d.cost[7] + c.nx + d.ny;
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_method_compiles(tmp_path, flavour):
    src = tmp_path / "terrain.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    cmd += ["-DPWPP_NO_EIGEN"] if flavour == "plain" else ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "terrain.c"
    src.write_text('#include "pwpp.h"\nint f(const pwpp_terrain_params *p) { return pwpp_terrain_grid(0, 1, 1, 1, 0.5, PWPP_MEM_HOST, 0, p, 0, 0, 0, 0, 0) + '
                   'pwpp_terrain_ground(0, 0, 0, 1, PWPP_MEM_HOST, p, 0, 0, 0, 0, 0, 0) + (int)sizeof(*p); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# ---- the restatement itself ---------------------------------------------------------------------------------------------------
def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def is_nan(a):
    return bits(a) == tr.NAN_BITS


def test_a_single_cell_and_images_one_cell_wide():
    step, slope, rough, count, cost = tr.terrain(np.full((1, 1), 2.5, np.float32), 0.5, 1, 1)
    assert step[0, 0] == 0.0 and is_nan(slope).all() and is_nan(rough).all() and count[0, 0] == 1 and cost[0, 0] == -1
    step, slope, rough, count, cost = tr.terrain(np.full((1, 1), NAN, np.float32), 0.5, 1, 1)
    assert is_nan(step).all() and count[0, 0] == 0 and cost[0, 0] == -1
    line = (0.25 * np.arange(9) ** 2).astype(np.float32)
    for r in (1, 2, 3, 4):
        for h in (line.reshape(1, 9), line.reshape(9, 1)):   # every window is collinear
            step, slope, rough, count, cost = tr.terrain(h, 0.5, r, 1, 1.0, 1.0, 1.0)
            assert is_nan(slope).all() and is_nan(rough).all() and (cost == -1).all()
            assert count.ravel().tolist() == [min(i, r) + min(8 - i, r) + 1 for i in range(9)]
            lo, hi = np.maximum(np.arange(9) - r, 0), np.minimum(np.arange(9) + r, 8)
            assert np.array_equal(step.ravel(), line[hi] - line[lo])


def test_three_cells_that_span_a_plane_leave_no_roughness():
    h = np.full((3, 3), NAN, np.float32)
    h[1, 1], h[0, 2], h[2, 1] = 1.0, 1.75, -0.5
    step, slope, rough, count, cost = tr.terrain(h, 0.5, 1, 3)
    assert count[1, 1] == 3 and rough[1, 1] == 0.0 and step[1, 1] == 2.25 and slope[1, 1] > 0 and cost[1, 1] == 0
    # (an unknown centre is undefined whatever its window sees)
    assert is_nan(step[0, 0]) and count[0, 0] == 1 and cost[0, 0] == -1
    h[2, 1] = NAN
    h[2, 0] = -0.5   # (1, 1), (2, 0), (0, 2): one line
    _, slope, rough, count, cost = tr.terrain(h, 0.5, 1, 1)
    assert count[1, 1] == 3 and is_nan(slope[1, 1]) and is_nan(rough[1, 1]) and cost[1, 1] == -1


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("cell", [0.5, 0.3, 0.125])
def test_an_exact_integer_plane(r, cell):
    yy, xx = np.mgrid[0:11, 0:13]
    h = ((3 * xx + 4 * yy - 20) / 1024.0).astype(np.float32)   # z rises 3 units per cell in x and 4 in y
    step, slope, rough, count, cost = tr.terrain(h, cell, r, 3)
    assert (bits(rough) == 0).all()                              # exactly +0.0 everywhere, clipped windows included
    assert (slope == np.float32(5.0 / (1024.0 * cell))).all()
    assert (count[r:-r, r:-r] == (2 * r + 1) ** 2).all() and count[0, 0] == (r + 1) ** 2
    assert (step[r:-r, r:-r] == np.float32(2 * r * 7 / 1024.0)).all() and step[0, 0] == np.float32(r * 7 / 1024.0)
    assert (cost == 0).all()


def test_a_height_offset_of_whole_units_changes_nothing():
    h = tr.random_heights(2, 13, 17, 1)
    q = np.rint(h.astype(np.float64) * 1024.0) / 1024.0     # heights on the 2^-10 m lattice, so that the offset is exact
    a = tr.terrain(q.astype(np.float32), 0.5, 2, 3, 0.2, 0.3, 0.05)
    for off in (1.0, -37.0 / 1024, 500.0 + 3.0 / 1024):
        b = tr.terrain((q + off).astype(np.float32), 0.5, 2, 3, 0.2, 0.3, 0.05)
        assert np.isfinite(a[1]).sum() > 200 and tr.same(a, b), off


def test_the_symmetries_of_the_square_permute_the_outputs():
    h = tr.random_heights(1, 12, 15, 2, limits=True)[0]
    for r in (1, 3):
        a = tr.terrain(h, 0.3, r, 3, 0.2, 0.3, 0.05)
        for move in (np.rot90, lambda m: np.rot90(m, 2), lambda m: np.rot90(m, 3), np.fliplr, np.flipud, np.transpose):
            b = tr.terrain(np.ascontiguousarray(move(h)), 0.3, r, 3, 0.2, 0.3, 0.05)
            assert tr.same(tuple(np.ascontiguousarray(move(x)) for x in a), b)


def test_limit_heights_non_finite_values_and_ties():
    beyond = np.nextafter(np.float32(1024.0), np.float32(np.inf))
    hs = np.array([1024.0, -1024.0, beyond, -beyond, INF, -INF, NAN, -0.0, 0.5 / 1024, 1.5 / 1024, 2.5 / 1024, -0.5 / 1024, -1.5 / 1024], np.float32)
    known, z = tr.quantise(hs)
    assert known.tolist() == [True, True, False, False, False, False, False] + [True] * 6
    assert z.tolist() == [tr.M, -tr.M, 0, 0, 0, 0, 0, 0, 0, 2, 2, 0, -2]   # ties to even
    # each of them alone in a window of three good cells: unknown ones drop out of count, step, the plane
    for i, v in enumerate(hs):
        h = np.array([[0.0, 1.0 / 1024, v], [2.0 / 1024, NAN, NAN], [NAN, NAN, NAN]], np.float32)
        step, slope, rough, count, cost = tr.terrain(h, 0.5, 1, 1)
        assert count[0, 1] == (4 if known[i] else 3)
        assert step[0, 1] == np.float32((max(2, z[i]) - min(0, z[i])) / 1024.0 if known[i] else 2.0 / 1024)
        assert is_nan(step[0, 2]) != bool(known[i])
    # -0.0 is 0: the same bits as +0.0
    a = tr.terrain(np.array([[0.0, 1.0], [2.0, -0.0]], np.float32), 0.5, 1, 1, 1.0, 1.0, 1.0)
    b = tr.terrain(np.array([[0.0, 1.0], [2.0, 0.0]], np.float32), 0.5, 1, 1, 1.0, 1.0, 1.0)
    assert tr.same(a, b)
    # the largest N: 1023.9 beside -1023.9
    h = np.where(np.indices((9, 9)).sum(0) % 2 == 0, 1023.9, -1023.9).astype(np.float32)
    D, A, B, N = tr.plane(tr.moments(h.reshape(1, 9, 9), 4))
    assert int(N[0, 4, 4]).bit_length() > 80 and 0 < D[0, 4, 4] < 2 ** 31 and all(int(n) >= 0 for n in N.ravel())
    step, slope, rough, count, cost = tr.terrain(h, 0.5, 4, 81, 1.0, 1.0, 1.0)
    assert abs(float(rough[4, 4]) - 1023.9) < 0.1 and cost[4, 4] == 100 and count[4, 4] == 81


def test_the_cost_rule():
    # a plane of slope exactly s / (1024 cell) with z = s x: step = 2 s / 1024 in a full window of r 1, rough 0
    def plane_cost(s, **kw):
        h = (s * np.mgrid[0:3, 0:3][1] / 1024.0).astype(np.float32)
        return tr.terrain(h, 1.0, 1, **kw)
    step, slope, rough, count, cost = plane_cost(512, min_known=9)
    assert step[1, 1] == 1.0 and slope[1, 1] == 0.5 and rough[1, 1] == 0.0 and count[1, 1] == 9 and cost[1, 1] == 0   # every limit infinite
    below = float(np.nextafter(np.float32(0.5), np.float32(1.0)))
    above = float(np.nextafter(np.float32(0.5), np.float32(0.0)))
    assert plane_cost(512, min_known=9, slope_max=below)[4][1, 1] == 99       # t just below 1
    assert plane_cost(512, min_known=9, slope_max=0.5)[4][1, 1] == 100        # t == 1
    assert plane_cost(512, min_known=9, slope_max=above)[4][1, 1] == 100      # t just above
    assert plane_cost(512, min_known=9, slope_max=2.0)[4][1, 1] == 25
    assert plane_cost(512, min_known=9, slope_max=2.0, step_max=3.0)[4][1, 1] == 33     # the largest ratio: floor(100 / 3)
    assert plane_cost(512, min_known=9, slope_max=2.0, step_max=INF, rough_max=1e-30)[4][1, 1] == 25   # rough is 0
    # min_known at k and k + 1: the corner of the 3 x 3 image sees 4 cells
    assert plane_cost(512, min_known=4, slope_max=2.0)[4][0, 0] == 25 and plane_cost(512, min_known=5, slope_max=2.0)[4][0, 0] == -1
    assert plane_cost(512, min_known=5, slope_max=2.0)[3][0, 0] == 4 and not is_nan(plane_cost(512, min_known=5)[1][0, 0])


# ---- the kernel's functions on the host ----------------------------------------------------------------------------------------
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
    tmp = tmp_path_factory.mktemp("terrain_check")
    exe = tmp / "terrain_check"
    flags = SANITIZE if sanitizers_work(tmp) else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off"] + flags +
                   ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "terrain_check.cpp"), "-o", str(exe)], check=True)
    return exe


def test_terrain_program_builds_and_passes(checker):
    r = subprocess.run([str(checker)], capture_output=True, text=True)  # (a stand-alone child process with its own main)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches, 0 failed proof steps" in r.stdout
    assert int(r.stdout.split("terrain_check: ")[1].split(" cases")[0]) >= 170000


@pytest.mark.parametrize("r,cell,min_known,limits,path", [(1, 0.5, 3, (0.2, 0.3, 0.05), 1), (2, 0.3, 1, (INF, 0.5, INF), 2), (3, 0.125, 20, (1.0, INF, 0.01), 1),
                                                          (4, 0.5, 20, (0.5, 0.5, 0.1), 2)])
def test_the_restatement_and_the_one_text_agree_byte_for_byte(checker, tmp_path, r, cell, min_known, limits, path):
    """The kernel's functions, dealt tile by tile on the host, against the numpy restatement: what the GPU tests compare, without a GPU."""
    h = tr.random_heights(3, 19, 70, 10 + r, holes=0.3, limits=True)
    h.tofile(tmp_path / "in.f32")
    args = ["dump", str(tmp_path / "in.f32"), "70", "19", "3", str(r), str(min_known), repr(cell)] + [repr(float(v)) for v in limits] + [str(path), str(tmp_path / "out")]
    subprocess.run([str(checker)] + args, check=True)
    got = tuple(np.fromfile(str(tmp_path / "out") + "." + name, dt).reshape(h.shape)
                for name, dt in zip(tr.NAMES, (np.float32, np.float32, np.float32, np.uint8, np.int8)))
    want = tr.terrain(h, cell, r, min_known, *limits)
    for name, g, w in zip(tr.NAMES, got, want):
        assert g.tobytes() == w.tobytes(), name
    assert (want[4] >= 0).sum() > 100 and is_nan(want[1]).sum() > 100
