"""The costmap without a GPU: the rule of include/pwpp.h for one cell (pwpp_costmap_cell, the function the kernels are compiled from)
against the numpy restatement tests/costmap_ref.py over every pair of bytes; the curve helper; every PWPP_E_ARG of the two entry
points in the documented order (PWPP_E_STATE needs a handle, so a device: tests/test_gpu_costmap.py has it); and tools/costmap_check.cpp, which deals the rule as both kernel paths do under the sanitizers."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import costmap_ref as cr
import pwpp_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")
E_ARG = -1
CURVE = np.array([100, 100, 99, 77, 50, 50, 31, 12, 5, 1, 0, 0, 3], np.uint8)  # (not monotone at its end: the table is data)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pwpp_hip.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "lib/libpwpp_hip.so"], check=True, stdout=subprocess.DEVNULL)
    return pwpp_hip.load()


def params(**kw):
    f = dict(layers=7, occupancy_unknown=-1, terrain_unknown=-1, unknown_below=101)
    f.update(kw)
    pad = f.pop("pad_", (0, 0))
    return pwpp_hip.CostmapParams(f["layers"], f["occupancy_unknown"], f["terrain_unknown"], f["unknown_below"], (ctypes.c_int32 * 2)(*pad))


def tparams(**kw):
    f = dict(radius=1, min_known=3, step_max=0.2, slope_max=0.3, rough_max=0.05, pad_=0)
    f.update(kw)
    return pwpp_hip.TerrainParams(**f)


def group_cells():
    src = open(os.path.join(PKG, "csrc", "pwpp_costmap.h")).read()
    value = lambda name: int(src.split("#define PWPP_COSTMAP_%s " % name)[1].split()[0])
    return value("BLOCK") * value("LANE_CELLS") * value("LANE_ITEMS")


def test_symbols_macros_struct_and_prototypes(lib):
    hdr = open(os.path.join(ROOT, "include", "pwpp.h")).read()
    for name in ("pwpp_costmap_grid", "pwpp_costmap_obstacles", "pwpp_costmap_cell", "pwpp_costmap_curve"):
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr
    for text in ("#define PWPP_HAS_COSTMAP 1", "#define PWPP_COSTMAP_OCCUPANCY 1", "#define PWPP_COSTMAP_INFLATION 2", "#define PWPP_COSTMAP_TERRAIN   4",
                 "#define PWPP_COSTMAP_MAX_CURVE 4097", "typedef struct pwpp_costmap_params {", '"costmap_path"'):
        assert text in hdr, text
    assert hdr.index("PWPP_API int pwpp_evidence_verdict(") < hdr.index("PWPP_HAS_COSTMAP") < hdr.index("#define PWPP_HAS_INPUT_TRANSFORM")
    assert ctypes.sizeof(pwpp_hip.CostmapParams) == 24
    assert [f[0] for f in pwpp_hip.CostmapParams._fields_] == ["layers", "occupancy_unknown", "terrain_unknown", "unknown_below", "pad_"]
    assert (pwpp_hip.COSTMAP_OCCUPANCY, pwpp_hip.COSTMAP_INFLATION, pwpp_hip.COSTMAP_TERRAIN) == (cr.OCCUPANCY, cr.INFLATION, cr.TERRAIN) == (1, 2, 4)
    assert pwpp_hip.COSTMAP_WHY_UNKNOWN == cr.WHY_UNKNOWN == 8 and pwpp_hip.COSTMAP_MAX_CURVE == cr.MAX_CURVE == 4097
    assert len(lib.pwpp_costmap_grid.argtypes) == 13 and len(lib.pwpp_costmap_obstacles.argtypes) == 20
    for name in ("costmap_grid", "costmap_grid_device", "costmap_obstacles", "costmap_obstacles_device"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    assert callable(pwpp_hip.costmap_cell) and callable(pwpp_hip.costmap_curve)
    assert group_cells() == 4096
    kernels = open(os.path.join(PKG, "csrc", "pwpp_costmap.hip")).read()
    assert "atomic" not in kernels.split("#include <hip/hip_runtime.h>")[1] and kernels.count("__syncthreads()") == 1


# ---- pwpp_costmap_cell over every pair of bytes -----------------------------------------------------------------------------------
SWEEP_C = r"""
#include <stdio.h>
#include <stdlib.h>
#include "pwpp.h"
/* stdin: lines "layers occupancy_unknown terrain_unknown unknown_below d"; stdout: per line 65536 x {cost as int8, why as uint8},
   o the row's byte and t the column's */
int main(int argc, char **argv) {
    static uint8_t curve[PWPP_COSTMAP_MAX_CURVE], out[2 * 65536];
    pwpp_costmap_params p = {0, 0, 0, 0, {0, 0}};
    int n_curve = 0, c, o, t;
    long d;
    FILE *f = fopen(argv[1], "rb");
    if (argc != 2 || !f) return 2;
    while ((c = fgetc(f)) != EOF) curve[n_curve++] = (uint8_t)c;
    fclose(f);
    while (scanf("%d %d %d %d %ld", &p.layers, &p.occupancy_unknown, &p.terrain_unknown, &p.unknown_below, &d) == 5) {
        for (o = 0; o < 256; ++o)
            for (t = 0; t < 256; ++t) {
                int32_t cost = 77;
                uint32_t why = 77;
                if (pwpp_costmap_cell(&p, curve, n_curve, (int8_t)o, (int8_t)t, (int32_t)d, &cost, &why) != PWPP_OK) return 3;
                if (cost < -1 || cost > 100 || why > 15) return 4;
                out[2 * (o * 256 + t)] = (uint8_t)(int8_t)cost, out[2 * (o * 256 + t) + 1] = (uint8_t)why;
            }
        if (fwrite(out, 1, sizeof(out), stdout) != sizeof(out)) return 5;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def sweep(lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("costmap_sweep")
    (tmp / "sweep.c").write_text(SWEEP_C)
    CURVE.tofile(tmp / "curve.u8")
    lib_dir = os.path.dirname(pwpp_hip.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp / "sweep.c"), "-o", str(tmp / "sweep"),
                    "-L", lib_dir, "-lpwpp_hip", "-Wl,-rpath," + lib_dir], check=True)
    return tmp


@pytest.mark.parametrize("layers", range(1, 8))
def test_one_cell_equals_the_restatement_for_every_pair_of_bytes(sweep, layers):
    n = len(CURVE)
    o = np.repeat(np.arange(256, dtype=np.uint8).view(np.int8), 256)
    t = np.tile(np.arange(256, dtype=np.uint8).view(np.int8), 256)
    configs = [(layers, ou, tu, below, d) for ou in (-1, 0, 100) for tu in (-1, 0, 100) for below in (1, 50, 100, 101)
               for d in (0, 1, n - 1, n, cr.DIST_BEYOND, -1)]
    r = subprocess.run([str(sweep / "sweep"), str(sweep / "curve.u8")], input="".join("%d %d %d %d %d\n" % c for c in configs).encode(), capture_output=True)
    assert r.returncode == 0, r.stderr
    got = np.frombuffer(r.stdout, np.uint8).reshape(len(configs), 65536, 2)
    seen = set()
    for k, (_, ou, tu, below, d) in enumerate(configs):
        key = (ou if layers & 1 else None, tu if layers & 4 else None, below, d if layers & 2 else None)  # (what the rule reads under this mask)
        if key in seen:   # a parameter of a layer that is off changes nothing: the same bytes as the first of its kind
            first = next(j for j, c in enumerate(configs[:k]) if (c[1] if layers & 1 else None, c[2] if layers & 4 else None, c[3], c[4] if layers & 2 else None) == key)
            assert got[k].tobytes() == got[first].tobytes()
            continue
        seen.add(key)
        cost, why = cr.fold(layers, ou, tu, below, CURVE, o, t, np.full(65536, d, np.int64).astype(np.int32))
        assert got[k, :, 0].view(np.int8).tobytes() == cost.tobytes(), (layers, ou, tu, below, d)
        assert got[k, :, 1].tobytes() == why.tobytes(), (layers, ou, tu, below, d)


def test_the_words_of_the_rule_on_cells_worked_by_hand():
    P = lambda **kw: params(**kw)
    cell = pwpp_hip.costmap_cell
    assert cell(P(), CURVE, 100, 5, 3) == (100, 1)                      # occupied: lethal, by the occupancy alone
    assert cell(P(), CURVE, 0, 77, 3) == (77, 2 | 4)                   # curve[3] == 77 == t: both named
    assert cell(P(), CURVE, -1, 5, 2) == (-1, 8 | 2)                    # unknown wins at 101; why still names the 99 of the curve
    assert cell(P(unknown_below=100), CURVE, -1, 5, 2) == (-1, 8 | 2)  # 99 < 100
    assert cell(P(unknown_below=100), CURVE, -1, 5, 0) == (100, 8 | 2)  # a lethal cell shows through
    assert cell(P(unknown_below=1), CURVE, -1, 0, 10) == (-1, 8)        # m == 0: nothing positive, no layer named
    assert cell(P(unknown_below=1), CURVE, -1, 1, 10) == (1, 8 | 4)
    assert cell(P(occupancy_unknown=40), CURVE, 7, -5, 11) == (-1, 8 | 1)   # the terrain stayed unknown; 40 is the maximum
    assert cell(P(occupancy_unknown=40, terrain_unknown=0), CURVE, 7, -5, 11) == (40, 1)
    assert cell(P(layers=4), None, 0, 127, 0) == (100, 4)               # t > 100 counts as 100
    assert cell(P(layers=2), CURVE, 0, 0, cr.DIST_BEYOND) == (0, 0) and cell(P(layers=2), CURVE, 0, 0, -1) == (0, 0)
    assert cell(P(layers=2), CURVE, 0, 0, 12) == (3, 2) and cell(P(layers=2), CURVE, 0, 0, 13) == (0, 0)
    assert cell(P(layers=1), None, 99, 0, 0) == (-1, 8) and cell(P(layers=1), None, 100 - 256, 0, 0) == (100, 1)   # only the byte 100 is occupied; o is read as an int8


# ---- pwpp_costmap_curve --------------------------------------------------------------------------------------------------------------
def test_the_curve_helper(lib):
    for cell, inscribed, radius, decay, peak in ((0.5, 0.6, 3.0, 1.5, 99), (0.1, 0.25, 1.0, 3.0, 99), (0.05, 0.3, 3.2, 0.7, 80), (1.0, 0.0, 5.0, 0.0, 50)):
        c = pwpp_hip.costmap_curve(cell, inscribed, radius, decay, peak)
        want = cr.curve(cell, inscribed, radius, decay, peak)
        assert len(c) == len(want) and c[0] == 100 and np.all(np.diff(c.astype(int)) <= 0) and c.max() <= 100
        assert np.sqrt(float(len(c) - 1)) * cell <= radius < np.sqrt(float(len(c))) * cell
        assert np.abs(c.astype(np.int64) - want).max() <= 1   # (the one place a libm difference can show)
        inside = np.sqrt(np.arange(len(c), dtype=np.float64)) * cell <= inscribed
        assert np.all(c[inside] == 100) and np.all(c[~inside] <= peak)
    # a radius that is an exact multiple of the cell, and one ulp either side: d = 36 is inside at 3.0 and above
    cell = 0.5
    for radius, n in ((3.0, 37), (np.nextafter(3.0, 4.0), 37), (np.nextafter(3.0, 0.0), 36)):
        assert len(pwpp_hip.costmap_curve(cell, 0.5, radius, 1.0, 99)) == n, radius
    assert len(pwpp_hip.costmap_curve(1.0, 0.0, 64.0, 1.0, 99)) == 4097 and len(pwpp_hip.costmap_curve(1.0, 0.0, 0.0, 1.0, 99)) == 1
    err = lib.pwpp_last_error
    buf = np.zeros(4097, np.uint8)
    call = lambda cell=0.5, ins=0.5, rad=3.0, decay=1.0, peak=99, out=buf, cap=4097: lib.pwpp_costmap_curve(cell, ins, rad, decay, peak, out.ctypes.data_as(ctypes.c_void_p) if out is not None else None, cap)
    assert call() == 37
    assert call(cap=36) == E_ARG and b"capacity 36: the curve has 37" in err()
    assert call(cap=37) == 37
    assert call(out=None) == E_ARG and b"null curve" in err()
    for v in (0.0, -1.0, float("nan"), float("inf")):
        assert call(cell=v) == E_ARG and b"cell size" in err()
    assert call(ins=-0.1) == E_ARG and call(ins=3.5) == E_ARG and call(rad=float("inf")) == E_ARG and b"inscribed" in err()
    assert call(decay=-1.0) == E_ARG and b"decay" in err()
    assert call(peak=100) == E_ARG and call(peak=-1) == E_ARG and b"peak -1: 0 .. 99" in err()
    assert call(cell=1.0, rad=np.sqrt(4097.0) + 0.01) == E_ARG and b"more than 4097" in err()


# ---- the errors, in the documented order ----------------------------------------------------------------------------------------------
def test_every_argument_of_costmap_grid_is_named_before_the_device_is_touched_and_in_order(lib):
    cells = 16
    occ, ter, cost, why = np.zeros(cells, np.int8), np.zeros(cells, np.int8), np.zeros(cells, np.int8), np.zeros(cells, np.uint8)
    dist2 = np.zeros(cells, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    at = lambda a, n: ctypes.c_void_p(a.ctypes.data + n)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    err = lib.pwpp_last_error
    P = lambda **kw: ctypes.byref(params(**kw))
    curve = CURVE.copy()

    def grid(h=fake, nx=4, ny=4, frames=1, mem=2, o=vp(occ), t=vp(ter), d=vp(dist2), p=P(), cv=vp(curve), n=len(curve), c=vp(cost), w=vp(why)):
        return lib.pwpp_costmap_grid(h, nx, ny, frames, mem, o, t, d, p, cv, n, c, w)

    ok = b"PWPP_MEM_HOST or"  # (mem = 2, PWPP_MEM_HOST_PINNED: every check before mem has passed)
    assert grid() == E_ARG and ok in err()
    # 1 null pointers
    assert grid(h=None) == E_ARG and b"null handle" in err()
    assert grid(p=None) == E_ARG and b"null costmap parameters" in err()
    assert grid(c=None) == E_ARG and b"null cost image" in err()
    assert grid(w=None) == E_ARG and ok in err()  # why may be absent
    # 2 the images, before the parameters
    for kw in (dict(frames=0), dict(nx=0), dict(ny=-1)):
        assert grid(p=P(layers=0), **kw) == E_ARG and b"cells" in err(), kw
    for kw in (dict(nx=32769), dict(ny=32769)):
        assert grid(**kw) == E_ARG and b"32768 a side" in err(), kw
    assert grid(nx=32768, ny=32768, frames=3) == E_ARG and b"exceed 2^31" in err()
    # 3 the parameters, each at both ends, before the curve
    for v in (0, 8, -1, 16):
        assert grid(p=P(layers=v), cv=None) == E_ARG and b"layers %d:" % v in err()
    for v in (-2, 101):
        assert grid(p=P(occupancy_unknown=v), cv=None) == E_ARG and b"occupancy_unknown %d: -1" % v in err()
        assert grid(p=P(terrain_unknown=v), cv=None) == E_ARG and b"terrain_unknown %d: -1" % v in err()
    for v in (0, 102):
        assert grid(p=P(unknown_below=v), cv=None) == E_ARG and b"unknown_below %d: 1 .. 101" % v in err()
    assert grid(p=P(pad_=(0, 5)), cv=None) == E_ARG and b"pad_ {0, 5}" in err()
    assert grid(p=P(pad_=(3, 0)), cv=None) == E_ARG and b"pad_ {3, 0}" in err()
    for kw in (dict(occupancy_unknown=-1, terrain_unknown=-1, unknown_below=1), dict(occupancy_unknown=100, terrain_unknown=100, unknown_below=101)):
        assert grid(p=P(**kw)) == E_ARG and ok in err(), kw
    # 4 the curve, read only with the inflation layer, before the images
    assert grid(cv=None, o=None) == E_ARG and b"null curve" in err()
    for v in (0, -1, 4098):
        assert grid(n=v, o=None) == E_ARG and b"n_curve %d: 1 .. 4097" % v in err()
    bad = curve.copy()
    bad[5], bad[9] = 101, 255
    assert grid(cv=vp(bad), o=None) == E_ARG and b"curve entry 5 is 101" in err()
    long = np.full(4097, 100, np.uint8)
    assert grid(cv=vp(long), n=4097) == E_ARG and ok in err()
    assert grid(p=P(layers=5), cv=None, n=0) == E_ARG and ok in err()
    assert grid(p=P(layers=5), cv=vp(bad), n=-3) == E_ARG and ok in err()   # not looked at without the layer
    # 5 the image of an enabled layer
    assert grid(o=None) == E_ARG and b"null occupancy image with the occupancy layer" in err()
    assert grid(t=None) == E_ARG and b"null terrain image" in err()
    assert grid(o=None, t=None) == E_ARG and b"null occupancy" in err()   # occupancy first
    assert grid(p=P(layers=6), o=None, d=None) == E_ARG and b"null occupancy image with the inflation layer and no dist2" in err()
    assert grid(p=P(layers=6), o=None) == E_ARG and ok in err()
    assert grid(p=P(layers=6), d=None) == E_ARG and ok in err()            # the one exception: the call computes the distances
    assert grid(p=P(layers=2), t=None, d=None) == E_ARG and ok in err()
    assert grid(p=P(layers=1), t=None, d=None, cv=None) == E_ARG and ok in err()
    assert grid(p=P(layers=4), o=None, d=None, cv=None) == E_ARG and ok in err()
    # 6 the overlaps, before mem
    assert grid(c=vp(occ), mem=9) == E_ARG and b"occupancy and cost overlap" in err()
    assert grid(c=at(ter, 15), mem=9) == E_ARG and b"terrain and cost overlap" in err()
    assert grid(w=at(cost, 8), mem=9) == E_ARG and b"cost and why overlap" in err()
    assert grid(t=vp(occ), mem=9) == E_ARG and b"occupancy and terrain overlap" in err()
    wide, wide_b = np.zeros(cells * 4 + 8, np.int8), np.zeros(160, np.int8)
    assert grid(d=at(wide, 4), c=at(wide, 4 + 4 * cells - 1), mem=9) == E_ARG and b"dist2 and cost overlap" in err()
    assert grid(d=at(wide, 0), c=at(wide, 4 * cells), mem=9) == E_ARG and b"mem 9" in err()
    # 7 mem, then the alignment of dist2 in device memory; the byte images may sit anywhere
    assert grid(mem=9) == E_ARG and b"mem 9: the costmap takes" in err()
    for k in (1, 2, 3):   # (named before the fake handle is touched)
        assert grid(mem=pwpp_hip.MEM_DEVICE, d=at(wide, k), o=at(wide_b, 1), t=at(wide_b, 40), c=at(wide_b, 83), w=at(wide_b, 122)) == E_ARG
        assert b"dist2 image must be 4-byte aligned" in err()


def test_every_argument_of_costmap_obstacles_is_named_before_the_device_is_touched_and_in_order(lib):
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))
    err = lib.pwpp_last_error
    P = lambda **kw: ctypes.byref(params(**kw))
    T = lambda **kw: ctypes.byref(tparams(**kw))
    cells = 16
    cost, occ, ter, why, dist2 = np.zeros(cells, np.int8), np.zeros(cells, np.int8), np.zeros(cells, np.int8), np.zeros(cells, np.uint8), np.zeros(cells, np.int32)
    org = np.array([[1.0, 1.0]])
    curve = CURVE.copy()
    G = lambda **kw: ctypes.byref(pwpp_hip.GroundGrid(**dict(dict(x0=0.0, y0=0.0, cell=0.5, nx=4, ny=4, flags=0, pad_=0), **kw)))

    def obst(h=fake, g=G(), h_min=0.0, h_max=1.0, min_count=1, o_xy=vp(org), n_org=1, max_range=0, tp=T(), p=P(), cv=vp(curve), n=len(curve), first=0, frames=1,
             mem=2, c=vp(cost), w=vp(why), o=vp(occ), d=vp(dist2), t=vp(ter)):
        return lib.pwpp_costmap_obstacles(h, g, h_min, h_max, min_count, o_xy, n_org, max_range, tp, p, cv, n, first, frames, mem, c, w, o, d, t)

    ok = b"PWPP_MEM_HOST or"
    assert obst() == E_ARG and ok in err()
    # 1 null pointers
    assert obst(h=None) == E_ARG and b"null handle" in err()
    assert obst(g=None) == E_ARG and b"null grid" in err()
    assert obst(p=None) == E_ARG and b"null costmap parameters" in err()
    assert obst(c=None) == E_ARG and b"null cost image" in err()
    for kw in (dict(w=None), dict(o=None), dict(d=None), dict(t=None)):
        assert obst(**kw) == E_ARG and ok in err(), kw   # kept, or not wanted
    # 2 the parameters and the curve, before the layers' own pointers
    assert obst(p=P(layers=0), o_xy=None) == E_ARG and b"layers 0" in err()
    assert obst(p=P(unknown_below=0), tp=None) == E_ARG and b"unknown_below 0" in err()
    assert obst(cv=None, o_xy=None) == E_ARG and b"null curve" in err()
    assert obst(n=4098, tp=None) == E_ARG and b"n_curve 4098" in err()
    bad = curve.copy()
    bad[0] = 101
    assert obst(cv=vp(bad), frames=0) == E_ARG and b"curve entry 0 is 101" in err()
    # 3 the origin and the terrain parameters of the enabled layers
    assert obst(o_xy=None, tp=None) == E_ARG and b"null origin with the occupancy layer" in err()
    assert obst(tp=None, frames=0) == E_ARG and b"null terrain parameters with the terrain layer" in err()
    assert obst(p=P(layers=6), o_xy=None) == E_ARG and ok in err()
    assert obst(p=P(layers=3), tp=None) == E_ARG and ok in err()
    assert obst(p=P(layers=4), o_xy=None, cv=None, n=0, h_min=2.0, min_count=0, max_range=-1) == E_ARG and ok in err()  # nothing of the obstacle stages is read
    # 4 the frames, the sides, the flags
    assert obst(frames=0, h_min=2.0) == E_ARG and b"0 frames of 4 x 4 cells" in err()
    assert obst(g=G(nx=0)) == E_ARG and b"cells" in err()
    assert obst(g=G(nx=32769), min_count=0) == E_ARG and b"32768 a side" in err()
    assert obst(g=G(flags=2), min_count=0) == E_ARG and b"grid flags 2" in err()
    assert obst(g=G(flags=1)) == E_ARG and ok in err()
    # 5 the band and min_count (occupancy or inflation), then the visibility's own (occupancy)
    assert obst(h_min=2.0, min_count=0) == E_ARG and b"height band" in err()
    assert obst(min_count=0, max_range=-1) == E_ARG and b"min_count 0" in err()
    assert obst(p=P(layers=2), min_count=0) == E_ARG and b"min_count 0" in err()
    assert obst(g=G(cell=0.0), max_range=-1) == E_ARG and b"cell size" in err()
    assert obst(max_range=-1, n_org=0) == E_ARG and b"max_range -1" in err()
    assert obst(n_org=2, tp=T(radius=0)) == E_ARG and b"2 origins for 1 frames" in err()
    far = np.array([[9.0, 1.0]])
    assert obst(o_xy=vp(far), tp=T(radius=0)) == E_ARG and b"origin 0" in err() and b"outside the grid" in err()
    assert obst(p=P(layers=6), max_range=-1, n_org=0, o_xy=vp(far)) == E_ARG and ok in err()   # read with the occupancy layer only
    # 6 the terrain parameters, then the overlaps
    assert obst(tp=T(radius=0), c=vp(occ)) == E_ARG and b"radius 0" in err()
    assert obst(tp=T(min_known=10), c=vp(occ)) == E_ARG and b"min_known 10" in err()
    assert obst(p=P(layers=3), tp=T(radius=0)) == E_ARG and ok in err()
    assert obst(c=vp(occ), mem=9) == E_ARG and b"occupancy and cost overlap" in err()
    assert obst(c=vp(ter), mem=9) == E_ARG and b"terrain and cost overlap" in err()
    assert obst(p=P(layers=6), c=vp(occ)) == E_ARG and ok in err()   # the image of a layer that is off is not looked at
    # 7 what pwpp_rasterize_ground checks: the grid's origin and cell, mem -- and with a real handle the state
    assert obst(p=P(layers=4), g=G(cell=float("nan")), mem=9) == E_ARG and b"cell size" in err()
    assert obst(mem=9) == E_ARG and b"mem 9" in err()


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "costmap.c"
    src.write_text('#include "pwpp.h"\nint f(const pwpp_costmap_params *p, const pwpp_terrain_params *t, const uint8_t *c) {\n'
                   '  return pwpp_costmap_grid(0, 1, 1, 1, PWPP_MEM_HOST, 0, 0, 0, p, c, 1, 0, 0) + pwpp_costmap_obstacles(0, 0, 0.f, 1.f, 1, 0, 1, 0, t, p, c, 1, 0, 1, '
                   'PWPP_MEM_HOST, 0, 0, 0, 0, 0) + pwpp_costmap_cell(p, c, 1, 0, 0, 0, 0, 0) + pwpp_costmap_curve(1.0, 0.0, 1.0, 1.0, 99, 0, 0) + (int)sizeof(*p) + '
                   'PWPP_COSTMAP_OCCUPANCY + PWPP_COSTMAP_INFLATION + PWPP_COSTMAP_TERRAIN + PWPP_COSTMAP_WHY_UNKNOWN + PWPP_COSTMAP_MAX_CURVE + PWPP_HAS_COSTMAP; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# ---- the kernels' dealing on the host ---------------------------------------------------------------------------------------------
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
    tmp = tmp_path_factory.mktemp("costmap_check")
    if not sanitizers_work(tmp):
        pytest.skip("the sanitizer runtimes do not link or start here")
    exe = tmp / "costmap_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off"] + SANITIZE +
                   ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "costmap_check.cpp"), "-o", str(exe)], check=True)
    return exe


def test_costmap_program_builds_and_passes(checker):
    r = subprocess.run([str(checker)], capture_output=True, text=True)  # (a stand-alone child process with its own main)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
    assert int(r.stdout.split("costmap_check: ")[1].split(" cases")[0]) >= 8000   # (every offset and length 1 .. 9 under every mask among them)


@pytest.mark.parametrize("layers,n_curve", list(itertools.product(range(1, 8), (1, 26))) + [(7, 4097), (2, 2)])
def test_the_restatement_and_the_one_text_agree_byte_for_byte(checker, tmp_path, layers, n_curve):
    """The kernels' functions, dealt item by item on the host at an odd address, against the numpy restatement: what the GPU tests compare, without a GPU."""
    rng = np.random.default_rng(layers * 5000 + n_curve)
    cells = group_cells() + 5
    o = rng.integers(-128, 128, cells).astype(np.int8)
    o[rng.random(cells) < 0.5] = 0
    o[rng.random(cells) < 0.25] = 100
    t = rng.integers(-128, 128, cells).astype(np.int8)
    d = rng.integers(0, 2 * n_curve + 1, cells).astype(np.int32)
    d[:4] = (-1, cr.DIST_BEYOND, n_curve - 1, n_curve)
    curve = rng.integers(0, 101, n_curve).astype(np.uint8)
    for a, name in ((o, "o"), (t, "t"), (d, "d"), (curve, "curve")):
        a.tofile(tmp_path / name)
    ou, tu, below = int(rng.integers(-1, 101)), int(rng.integers(-1, 101)), int(rng.integers(1, 102))
    args = ["dump"] + [str(v) for v in (layers, ou, tu, below)] + [str(tmp_path / n) for n in ("curve", "o", "t", "d")] + [str(cells), str(tmp_path / "out")]
    subprocess.run([str(checker)] + args, check=True)
    want = cr.fold(layers, ou, tu, below, curve, o, t, d)
    assert np.fromfile(str(tmp_path / "out.cost"), np.int8).tobytes() == want[0].tobytes()
    assert np.fromfile(str(tmp_path / "out.why"), np.uint8).tobytes() == want[1].tobytes()
