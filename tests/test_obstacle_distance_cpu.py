"""No-GPU checks of the obstacle distances (pwpp_distance_grid, pwpp_distance_obstacles): the exports, the feature macro, the
ctypes prototypes and the bindings' methods, the argument checks that need no device, the C++ mirror in both flavours -- the
brute force the GPU tests compare against (tests/obstacle_distance_ref.py) against its separable restatement over the whole
pattern set -- and the stand-alone program that runs the kernels' functions and pass sequence on the host against a brute force
of its own (tools/distance_check.cpp), built with the address and undefined-behaviour sanitizers where the toolchain has them;
the tiling of the column pass (pwpp_dist_plan, dumped by that program) against a restatement in numpy, and, on the reference
alone, that the tall patterns of tests/test_gpu_obstacle_distance_tall.py are binding at every cap and in every tile."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import obstacle_distance_ref as od
import pwpp_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")
E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pwpp_hip.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "lib/libpwpp_hip.so"], check=True, stdout=subprocess.DEVNULL)
    return pwpp_hip.load()


def test_symbols_macro_and_prototypes(lib):
    hdr = open(os.path.join(ROOT, "include", "pwpp.h")).read()
    for name in ("pwpp_distance_grid", "pwpp_distance_obstacles"):
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr
    assert "#define PWPP_HAS_OBSTACLE_DISTANCE 1" in hdr and "#define PWPP_DIST_BEYOND 0x7fffffff" in hdr
    assert "#define PWPP_VERSION_MINOR 4 " in hdr
    assert pwpp_hip.DIST_BEYOND == od.BEYOND == 0x7fffffff
    assert len(lib.pwpp_distance_grid.argtypes) == 12 and len(lib.pwpp_distance_obstacles.argtypes) == 13
    assert lib.pwpp_distance_grid.argtypes[8] is ctypes.c_double
    assert lib.pwpp_distance_obstacles.argtypes[2] is ctypes.c_float and lib.pwpp_distance_obstacles.argtypes[3] is ctypes.c_float
    for name in ("distance_grid", "distance_grid_device", "distance_obstacles", "distance_obstacles_device"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    import pypatchworkpp
    assert hasattr(pypatchworkpp.patchworkpp, "getObstacleDistances")


def test_null_and_range_arguments_are_named_before_the_device_is_touched(lib):
    cnt, d2, met = np.zeros(16, np.int32), np.zeros(16, np.int32), np.zeros(16, np.float32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    H = pwpp_hip.MEM_HOST

    def grid(h=fake, nx=4, ny=4, frames=1, mem=H, count=vp(cnt), min_count=1, max_dist=0, cell=0.5, dist2=vp(d2), metres=None):
        return lib.pwpp_distance_grid(h, nx, ny, frames, mem, count, min_count, max_dist, cell, dist2, None, metres)

    assert grid(h=None) == E_ARG and b"null handle" in lib.pwpp_last_error()
    assert grid(count=None) == E_ARG and b"null count" in lib.pwpp_last_error()
    assert grid(dist2=None) == E_ARG and b"null dist2" in lib.pwpp_last_error()
    for kw in (dict(nx=0), dict(ny=0), dict(frames=0), dict(nx=-3)):
        assert grid(**kw) == E_ARG and b"cells" in lib.pwpp_last_error(), kw
    for kw in (dict(nx=32769), dict(ny=32769), dict(nx=65536, ny=32768)):
        assert grid(**kw) == E_ARG and b"32768 a side" in lib.pwpp_last_error(), kw
    assert grid(nx=32768, ny=32768, frames=3) == E_ARG and b"exceed 2^31" in lib.pwpp_last_error()
    for m in (0, -1):
        assert grid(min_count=m) == E_ARG and b"min_count" in lib.pwpp_last_error()
    for m in (-1, 46341, 1 << 30):
        assert grid(max_dist=m) == E_ARG and b"max_dist" in lib.pwpp_last_error(), m
    for cell in (0.0, -0.5, np.nan, np.inf):
        assert grid(cell=cell, metres=vp(met)) == E_ARG and b"cell size" in lib.pwpp_last_error(), cell
    assert grid(mem=2) == E_ARG and b"PWPP_MEM_HOST or PWPP_MEM_DEVICE" in lib.pwpp_last_error()   # PWPP_MEM_HOST_PINNED
    # the order of the checks: the sides before the cells, the cells before min_count, min_count before max_dist, that before the cell
    assert grid(nx=32769, ny=32769, frames=4, min_count=0) == E_ARG and b"32768 a side" in lib.pwpp_last_error()
    assert grid(nx=32768, ny=32768, frames=3, min_count=0) == E_ARG and b"exceed 2^31" in lib.pwpp_last_error()
    assert grid(min_count=0, max_dist=-1) == E_ARG and b"min_count" in lib.pwpp_last_error()
    assert grid(max_dist=-1, cell=0.0, metres=vp(met)) == E_ARG and b"max_dist" in lib.pwpp_last_error()

    g = pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 4, 4, 0, 0)

    def obstacles(h=fake, gr=ctypes.byref(g), band=(0.2, 2.5), min_count=1, max_dist=0, dist2=vp(d2)):
        return lib.pwpp_distance_obstacles(h, gr, band[0], band[1], min_count, max_dist, 0, 1, H, dist2, None, None, None)

    assert obstacles(h=None) == E_ARG and b"null handle" in lib.pwpp_last_error()
    assert obstacles(gr=None) == E_ARG and b"null grid" in lib.pwpp_last_error()
    assert obstacles(dist2=None) == E_ARG and b"null dist2" in lib.pwpp_last_error()
    assert obstacles(band=(2.5, 0.2)) == E_ARG and b"height band" in lib.pwpp_last_error()
    assert obstacles(band=(np.nan, 1.0)) == E_ARG and b"height band" in lib.pwpp_last_error()
    assert obstacles(min_count=0) == E_ARG and b"min_count" in lib.pwpp_last_error()
    assert obstacles(max_dist=46341) == E_ARG and b"max_dist" in lib.pwpp_last_error()
    bad = pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 4, 4, 2, 0)
    assert obstacles(gr=ctypes.byref(bad)) == E_ARG and b"grid flags" in lib.pwpp_last_error()
    wide = pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 32769, 4, 0, 0)
    assert obstacles(gr=ctypes.byref(wide)) == E_ARG and b"32768 a side" in lib.pwpp_last_error()


CPP = r"""
#include "patchwork/patchworkpp.h"
#ifndef PWPP_HAS_OBSTACLE_DISTANCE
#error "include/pwpp.h does not announce the obstacle distances"
#endif
static_assert(PWPP_DIST_BEYOND == 2147483647, "2^31 - 1");
double use(patchwork::PatchWorkpp &pw) {
    patchwork::PatchWorkpp::ObstacleDistances d = pw.getObstacleDistances(-40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f);
    patchwork::PatchWorkpp::ObstacleDistances e = pw.getObstacleDistances(-40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f, 2, 20, true);
    return d.dist2[3 * 160 + 5] + d.nearest[7] + (double)d.metres(3, 5) + (double)e.dist2.size() + (e.dist2[0] == PWPP_DIST_BEYOND ? 1.0 : 0.0);
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_method_compiles(tmp_path, flavour):
    src = tmp_path / "obstacle_distances.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    cmd += ["-DPWPP_NO_EIGEN"] if flavour == "plain" else ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "distance.c"
    src.write_text('#include "pwpp.h"\nint f(void) { return pwpp_distance_grid(0, 1, 1, 1, PWPP_MEM_HOST, 0, 1, 0, 1.0, 0, 0, 0) + (PWPP_DIST_BEYOND > 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# ---- the brute force against the separable restatement, over the pattern set ---------------------------------------------------
@pytest.mark.parametrize("shape", od.SHAPES, ids=lambda s: "%dx%d" % s)
def test_brute_force_against_the_separable_restatement(shape):
    nx, ny = shape
    for name in od.PATTERNS:
        for min_count in (1, 2):
            count, _ = od.pattern(name, nx, ny, min_count)
            occ = count >= min_count
            d2, near = od.brute_force(count, min_count)
            s2, snear = od.separable(count, min_count)
            what = "%s %dx%d min_count %d" % (name, nx, ny, min_count)
            assert d2.dtype == np.int32 and near.dtype == np.int32 and d2.shape == (ny, nx), what
            assert np.array_equal(d2, s2) and np.array_equal(near, snear), what
            if not occ.any():
                assert (d2 == od.BEYOND).all() and (near == -1).all(), what
                assert np.isposinf(od.metres_of(d2, 0.5)).all()
                continue
            # by the definition, another way: the nearest cell is occupied, at the stated distance, and an occupied cell is its own
            jy, jx = near // nx, near % nx
            iy, ix = np.mgrid[0:ny, 0:nx]
            assert occ[jy, jx].all() and np.array_equal((ix - jx) ** 2 + (iy - jy) ** 2, d2), what
            assert np.array_equal(d2 == 0, occ) and np.array_equal(near[occ], (iy * nx + ix)[occ]), what
            for max_dist in od.MAX_DISTS[1:]:
                c2, cnear = od.capped((d2, near), max_dist)
                far = d2 > max_dist * max_dist
                assert (c2[far] == od.BEYOND).all() and (cnear[far] == -1).all(), what
                assert np.array_equal(c2[~far], d2[~far]) and np.array_equal(cnear[~far], near[~far]), what
            m = od.metres_of(d2, 0.5)
            exact = np.sqrt(d2.astype(np.float64)) * 0.5
            assert m.dtype == np.float32 and (m[occ] == 0).all() and (np.abs(m - exact) <= exact * 2.0 ** -24).all(), what  # (one rounding to float)


def test_ties_go_to_the_smallest_index_in_the_restatement():
    count = np.zeros((5, 5), np.int32)
    count[0, 0] = count[0, 4] = count[4, 0] = count[4, 4] = 1
    d2, near = od.brute_force(count)
    assert near[2, 2] == 0 and d2[2, 2] == 8          # four at the same distance: the first
    assert near[0, 2] == 0 and near[2, 4] == 4 and near[4, 2] == 20 and near[2, 0] == 0
    assert np.array_equal(near, od.separable(count)[1])


def test_frames_never_influence_each_other_in_the_restatement():
    count = np.zeros((2, 5, 7), np.int32)
    count[0, -1, :] = 1
    count[1, 0, :] = 2
    d2, near = od.distance_frames(count)
    assert d2[0, 0, 0] == 16 and d2[1, 4, 0] == 16 and near[0, 0, 3] == 4 * 7 + 3 and near[1, 4, 3] == 3


# ---- the kernels' functions and pass sequence on the host ------------------------------------------------------------------------
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def sanitizers_work(tmp_path):
    """The toolchain links the two runtimes into a program and that program starts in this environment."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        return False
    return subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0


@pytest.fixture(scope="module")
def distance_check(tmp_path_factory):
    """The stand-alone program (its own main, a child process), built once."""
    tmp_path = tmp_path_factory.mktemp("distance_check")
    exe = tmp_path / "distance_check"
    flags = SANITIZE if sanitizers_work(tmp_path) else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags +
                   ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "distance_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_distance_program_builds_and_passes(distance_check):
    r = subprocess.run([distance_check], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    # 6160 with windows of ny and 7 rows, and 80 of 5 x 700 (caps 1, 2, 5, 20) with the launcher's own tile and halo
    assert "0 mismatches" in r.stdout and "6240 cases" in r.stdout


def test_distance_program_passes_on_the_tall_shapes(distance_check):
    r = subprocess.run([distance_check, "--tall"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 mismatches" in r.stdout and "308 tall cases" in r.stdout
    assert subprocess.run([distance_check, "--nothing"], capture_output=True).returncode == 2


# ---- the tiling of the column pass: the launcher's plan against the restatement ------------------------------------------------
def test_plan_dump_is_the_restatement_line_for_line(distance_check):
    r = subprocess.run([distance_check, "--plans"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    caps = list(range(301)) + [46340]
    want = ["%d %d %d %d %d %d %d" % ((ny, m, path) + od.plan(ny, m, path)) for ny in range(1, 1401) for m in caps for path in (0, 1)]
    assert len(lines) == len(want) == 1400 * 302 * 2
    assert lines == want, "first difference: %r" % next(((a, b) for a, b in zip(lines, want) if a != b), None)
    ny, m, path, lds, tile_rows, halo, row_tiles = np.array(r.stdout.split(), np.int64).reshape(-1, 7).T
    assert (tile_rows >= 1).all() and np.array_equal(row_tiles, -(-ny // tile_rows))
    assert (lds[path == 1] == 0).all() and np.isin(lds, (0, 1)).all()
    on = lds == 1
    assert (np.minimum(ny, tile_rows + 2 * halo)[on] <= od.LDS_ROWS).all()
    assert ((tile_rows >= ny) | ((halo >= m) & (m > 0)))[on].all()
    assert (halo[~on] == 0).all()


def test_plan_spot_values():
    assert od.plan(512, 0) == (1, 512, 0, 1) and od.regime(512, 0) == "A"
    assert od.plan(513, 224) == (1, 64, 224, 9) and od.regime(513, 224) == "B"
    assert od.plan(513, 225) == od.plan(513, 0) == (0, 256, 0, 3) and od.regime(513, 225) == od.regime(513, 0) == "C"
    assert od.plan(577, 224)[3] == 10
    assert od.plan(513, 1) == (1, 510, 1, 2) and od.plan(577, 223) == (1, 66, 223, 9)
    assert od.plan(513, 224, 1) == od.plan(512, 0, 1)[:3] + (3,) == (0, 256, 0, 3)
    for nx, ny in od.TALL_SHAPES:  # what the tall cases of one shape reach: never A, B under each halo, C with and without a cap
        assert [od.regime(ny, m) for m in od.TALL_MAX_DISTS] == ["C", "B", "B", "B", "B", "B", "C", "C"]
        assert [od.plan(ny, m)[2] for m in od.TALL_MAX_DISTS] == [0, 1, 64, 65, 223, 224, 0, 0]
        assert ny % 64 == 1 and od.plan(ny, 224)[1] == 64  # the last tile of the 64-row tiling has one row


# ---- the tall patterns: the restatement on its own, and that every case is binding ---------------------------------------------
TALL = [(shape, name) for shape in od.TALL_SHAPES for name in od.TALL_PATTERNS]
tall_ids = lambda c: "%dx%d" % c if isinstance(c, tuple) else c


@pytest.mark.parametrize("shape,name", TALL, ids=tall_ids)
def test_tall_brute_force_against_the_separable_restatement(shape, name):
    nx, ny = shape
    for min_count in (1, 2) if name in ("two_rows", "sparse") else (1,):
        count, d2, near = od.tall_reference(name, nx, ny, min_count)
        occ = count >= min_count
        assert occ.any() and set(np.unique(count).tolist()) <= {0, 1, 2} and occ.sum() <= 2 * ny  # (sparse: the brute force stays cheap)
        assert 8 * nx * ny <= 32 << 20  # (one row of cells against every row: a block of the separable restatement holds at least that)
        s2, snear = od.separable(count, min_count)
        assert np.array_equal(d2, s2) and np.array_equal(near, snear), "%s %dx%d min_count %d" % (name, nx, ny, min_count)
        assert np.array_equal(d2 == 0, occ)
    if name in ("two_rows", "sparse"):  # min_count 2 drops a part of the pattern, not all of it
        assert 0 < (count >= 2).sum() < (count >= 1).sum()


BINDING_CAPS = (1, 64, 65, 223, 224, 225)


@pytest.mark.parametrize("shape", od.TALL_SHAPES, ids=tall_ids)
def test_every_cap_cuts_at_its_own_distance(shape):
    """A cell at exactly max_dist is reported and one between max_dist and max_dist + 1 is beyond: on the reference alone."""
    nx, ny = shape
    held = 0
    for name in od.AXIS_PATTERNS:
        d2 = od.tall_reference(name, nx, ny)[1].astype(np.int64)
        far = od.farthest_along_a_column(name, nx, ny)
        assert d2.max() >= far * far, name
        for m in BINDING_CAPS:
            if m + 1 > far:  # (the image cannot hold this cap: nothing is m + 1 rows from the pattern)
                continue
            held += 1
            assert (d2 == m * m).any(), "%s: no cell at exactly %d" % (name, m)
            assert ((d2 > m * m) & (d2 <= (m + 1) * (m + 1))).any(), "%s: no cell just beyond %d" % (name, m)
            c2, cnear = od.capped(od.tall_reference(name, nx, ny)[1:], m)
            assert (c2[d2 == m * m] == m * m).all() and (cnear[d2 == m * m] >= 0).all() and (c2[d2 > m * m] == od.BEYOND).all()
    # 130 x 577 holds every cap in every pattern; 65 x 513 all but two_rows at 223 and more (220 rows below its lower row)
    assert held == (36 if ny == 577 else 33)


@pytest.mark.parametrize("shape", od.TALL_SHAPES, ids=tall_ids)
def test_every_tile_of_every_plan_has_a_nearest_cell_in_another_tile(shape):
    """... within the cap, so that the answer comes through the halo (or, in regime C, from rows of another workgroup's tile)."""
    nx, ny = shape
    refs = {name: od.tall_reference(name, nx, ny) for name in od.TALL_PATTERNS}
    iy = np.arange(ny)[:, None].repeat(nx, 1)
    for m in od.TALL_MAX_DISTS:
        _, tile_rows, _, row_tiles = od.plan(ny, m)
        assert row_tiles > 1
        crossed = np.zeros(row_tiles, bool)
        through_borders = np.zeros(row_tiles, bool)
        for name, (_, d2, near) in refs.items():
            near = od.capped((d2, near), m)[1]
            other = (near >= 0) & (near // nx // tile_rows != iy // tile_rows)
            tiles = np.unique(iy[other] // tile_rows)
            crossed[tiles] = True
            if name == "borders":
                through_borders[tiles] = True
        assert crossed.all() and through_borders.all(), "max_dist %d: tiles %s see no cell of another tile" % (m, np.nonzero(~crossed)[0])


@pytest.mark.parametrize("shape", od.TALL_SHAPES, ids=tall_ids)
def test_lattice_has_cells_exactly_on_the_circle_off_the_axes(shape):
    nx, ny = shape
    cx, cy = od.lattice_cell(nx, ny)
    assert (cx, cy) == ((65, 288) if shape == (130, 577) else (32, 256))
    count, d2, near = od.tall_reference("lattice", nx, ny)
    assert count.sum() == 1 or count.sum() == 2
    y, x = np.nonzero(d2 == 65 * 65)
    off = (x != cx) & (y != cy)
    want = {(cx + sx * dx, cy + sy * dy) for dx, dy in ((16, 63), (33, 56), (39, 52), (25, 60), (63, 16), (56, 33), (52, 39), (60, 25))
            for sx in (-1, 1) for sy in (-1, 1) if 0 <= cx + sx * dx < nx}
    assert off.sum() >= 4 and set(zip(x[off].tolist(), y[off].tolist())) == want
    beyond = od.capped((d2, near), 65)[0] == od.BEYOND
    for px, py in want:  # ... and their outward neighbours are beyond
        ox, oy = px + np.sign(px - cx), py + np.sign(py - cy)
        assert not beyond[py, px] and beyond[oy, px] and (not 0 <= ox < nx or beyond[py, ox])


def test_two_rows_tie_at_a_tile_border_goes_to_the_upper_row():
    for nx, ny in od.TALL_SHAPES:
        _, d2, near = od.tall_reference("two_rows", nx, ny)
        assert od.plan(ny, 224)[1] == 64 and 192 % 64 == 0
        assert (d2[192] == 100 * 100).all() and np.array_equal(near[192], 92 * nx + np.arange(nx))
        _, d2, near = od.tall_reference("columns", nx, ny)
        if nx % 2 == 1:
            assert d2[5, nx // 2] == (nx // 2) ** 2 and near[5, nx // 2] == 5 * nx  # the left column on a tie
