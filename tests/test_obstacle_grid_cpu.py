"""No-GPU checks of the obstacle grid (pwpp_rasterize_obstacles): the export, the feature macro and the ctypes prototype, the
argument checks that need no device, the bindings' methods -- and the numpy restatement the GPU tests compare against
(tests/obstacle_grid_ref.py): against a plain Python loop on a hand-made set of points on every edge the rules name, and against
the oracle's non-ground set and records on a KITTI frame."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import ground_query_ref as gq
import obstacle_grid_ref as og
import oracle_lib as ol
import pwpp_hip
from test_gpu_point_planes import MAX_EDGE_POINTS, expected_distances, expected_patches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")
F32 = np.float32
NAN, INF = np.nan, np.inf


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pwpp_hip.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "lib/libpwpp_hip.so"], check=True, stdout=subprocess.DEVNULL)
    return pwpp_hip.load()


def test_symbol_macro_and_prototype(lib):
    hdr = open(os.path.join(ROOT, "include", "pwpp.h")).read()
    assert hasattr(lib, "pwpp_rasterize_obstacles")
    assert "PWPP_API int pwpp_rasterize_obstacles(" in hdr
    assert "#define PWPP_HAS_OBSTACLE_GRID 1" in hdr
    at = lib.pwpp_rasterize_obstacles.argtypes
    assert at is not None and len(at) == 10 and at[2] is ctypes.c_float and at[3] is ctypes.c_float
    for name in ("rasterize_obstacles", "rasterize_obstacles_device"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    import pypatchworkpp
    assert hasattr(pypatchworkpp.patchworkpp, "getObstacleMap")


def test_null_arguments_are_named_before_the_device_is_touched(lib):
    cnt = np.zeros(16, np.int32)
    g = pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 4, 4, 0, 0)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: the null checks come first)
    call = lambda h, grid, c: lib.pwpp_rasterize_obstacles(h, grid, 0.2, 2.5, 0, 1, pwpp_hip.MEM_HOST, c, None, None)
    assert call(None, ctypes.byref(g), vp(cnt)) == -1 and b"null handle" in lib.pwpp_last_error()
    assert call(fake, None, vp(cnt)) == -1 and b"null grid" in lib.pwpp_last_error()
    assert call(fake, ctypes.byref(g), None) == -1 and b"null count" in lib.pwpp_last_error()


CPP = r"""
#include "patchwork/patchworkpp.h"
#ifndef PWPP_HAS_OBSTACLE_GRID
#error "include/pwpp.h does not announce the obstacle grid"
#endif
float use(patchwork::PatchWorkpp &pw) {
    patchwork::PatchWorkpp::ObstacleMap m = pw.getObstacleMap(-40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f, true);
    return m.top(3, 5) + (float)m.count[3 * 160 + 5] + (float)(m.top.rows() * m.top.cols());
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_method_compiles(tmp_path, flavour):
    src = tmp_path / "obstacle_grid.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    cmd += ["-DPWPP_NO_EIGEN"] if flavour == "plain" else ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)


# ---- the restatement against a plain loop ----------------------------------------------------------------------------------
X0, Y0, CELL, NX, NY = -1.0, 0.5, 0.25, 6, 4      # x in [-1, 0.5), y in [0.5, 1.5): every edge below is exact in binary
H_MIN, H_MAX = 0.25, 2.5


def hand_made():
    """About 40 points (x, y, patch, decision, distance): cell edges, both ends of the grid, NaN / inf coordinates, heights on
    h_min and h_max, -0.0 against +0.0 in one cell, NaN heights, points without a patch and of hidden decisions."""
    rows = [
        (-1.0, 0.5, 0, 4, 1.0),        # on x0, y0: cell (0, 0)
        (0.5, 0.5, 0, 4, 1.0),         # on x0 + nx * cell: outside
        (-1.0, 1.5, 0, 4, 1.0),        # on y0 + ny * cell: outside
        (np.nextafter(F32(0.5), F32(0)), 0.5, 0, 4, 1.0),    # the last float inside: cell (5, 0)
        (np.nextafter(F32(-1.0), F32(-2)), 0.6, 0, 4, 1.0),  # the first float outside
        (-0.75, 0.75, 1, 4, 0.5),      # exactly on a cell edge in x and y: cell (1, 1)
        (-0.5, 1.0, 1, 4, 0.75), (-0.25, 1.25, 1, 2, 1.5), (0.0, 0.5, 2, 6, 2.0), (0.25, 0.75, 2, 4, 2.25),
        (NAN, 0.6, 0, 4, 1.0), (0.1, NAN, 0, 4, 1.0), (INF, 0.6, 0, 4, 1.0), (0.1, -INF, 0, 4, 1.0), (-INF, INF, 0, 4, 1.0),
        (-0.9, 0.6, 0, 4, H_MIN), (-0.9, 0.6, 0, 4, H_MAX),                                        # on the band's ends: counted
        (-0.9, 0.6, 0, 4, np.nextafter(F32(H_MIN), F32(0))), (-0.9, 0.6, 0, 4, np.nextafter(F32(H_MAX), F32(9))),  # just outside
        (-0.6, 0.9, 3, 4, NAN), (-0.6, 0.9, 3, 4, INF), (-0.6, 0.9, 3, 4, -INF), (-0.6, 0.9, 3, 4, 0.3),
        (0.3, 1.3, -1, 0, NAN), (0.3, 1.3, -1, 0, NAN), (0.3, 1.3, 5, 1, 1.0), (0.3, 1.3, 5, 3, 1.0), (0.3, 1.3, 5, 5, 1.0),
        (0.3, 1.3, 5, 4, 1.25), (0.3, 1.3, 5, 0, 0.5),
        (0.1, 1.1, 6, 4, -0.0), (0.1, 1.1, 6, 4, 0.0), (0.1, 1.1, 6, 4, -0.0),                    # -0.0 < +0.0 (a band from -1)
        (-0.1, 1.4, 6, 4, -0.0), (-0.1, 1.4, 6, 4, -0.5),                                          # a cell whose top is -0.0
        (-0.3, 0.6, 7, 4, -3.0), (-0.3, 0.6, 7, 4, -0.25), (-0.3, 0.6, 7, 4, 1e-40),               # negative heights, a subnormal
        (2.0, 1.0, 0, 4, 1.0), (0.0, 7.0, 0, 4, 1.0), (-0.999, 1.499, 8, 2, 2.4),
    ]
    a = np.array(rows, np.float64)
    xyz = np.zeros((len(a), 3), F32)
    xyz[:, 0], xyz[:, 1] = a[:, 0].astype(F32), a[:, 1].astype(F32)
    s = np.zeros(len(a), gq.SAMPLE_DTYPE)
    s["patch"], s["decision"], s["distance"] = a[:, 2].astype(np.int32), a[:, 3].astype(np.int32), a[:, 4].astype(F32)
    s["ground_z"] = np.where(s["patch"] < 0, np.nan, -1.7)
    return xyz, s


def loop_obstacles(xyz, s, x0, y0, cell, nx, ny, h_min, h_max, ground_only):
    """The rules of include/pwpp.h one point at a time, in Python floats (doubles); the order of the maximum is (value, sign)."""
    count = [[0] * nx for _ in range(ny)]
    unref = [[0] * nx for _ in range(ny)]
    top = [[None] * nx for _ in range(ny)]
    h_min, h_max = float(F32(h_min)), float(F32(h_max))
    for (x, y, _), smp in zip(xyz.tolist(), s):
        if math.isnan(x) or math.isnan(y) or math.isinf(x) or math.isinf(y):
            continue
        u, v = (x - x0) / cell, (y - y0) / cell
        if not (0 <= u < nx and 0 <= v < ny):
            continue
        ix, iy = int(math.floor(u)), int(math.floor(v))
        if smp["patch"] < 0 or (ground_only and int(smp["decision"]) in (1, 3, 5)):
            unref[iy][ix] += 1
            continue
        hgt = float(smp["distance"])
        if not (h_min <= hgt <= h_max):
            continue
        count[iy][ix] += 1
        key = (hgt, math.copysign(1.0, hgt))
        if top[iy][ix] is None or key > top[iy][ix]:
            top[iy][ix] = key
    tops = np.array([[np.nan if t is None else t[0] for t in row] for row in top], F32)
    return np.array(count, np.int32), tops, np.array(unref, np.int32)


@pytest.mark.parametrize("ground_only", [False, True])
@pytest.mark.parametrize("band", [(H_MIN, H_MAX), (-1.0, 0.5), (-INF, INF), (0.0, 0.0), (-0.0, -0.0)])
def test_restatement_against_a_plain_loop(band, ground_only):
    xyz, s = hand_made()
    assert 35 <= len(xyz) <= 48
    want = loop_obstacles(xyz, s, X0, Y0, CELL, NX, NY, band[0], band[1], ground_only)
    got = og.restate_obstacles(xyz, s, X0, Y0, CELL, NX, NY, band[0], band[1], ground_only)
    for g, w, name in zip(got, want, ("count", "top", "unref")):
        assert g.shape == (NY, NX) and g.dtype == w.dtype, name
        assert og.same_images(g, w), "%s:\n%s\nagainst the loop's\n%s" % (name, g, w)
    count, top, unref = got
    assert np.array_equal(np.isnan(top), count == 0)
    if band == (H_MIN, H_MAX):
        assert count[0, 0] == 3 and count[0, 5] == 1 and count[1, 1] == 2  # x0 / y0 and the band's two ends; the last float inside; an edge
        assert unref[3, 5] == (5 if ground_only else 2) and count[3, 5] == (2 if ground_only else 5)
    if band == (-1.0, 0.5):
        assert count[2, 4] == 3 and top[2, 4].view(np.uint32) == 0            # +0.0 beats -0.0
        assert count[3, 3] == 2 and top[3, 3].view(np.uint32) == 0x80000000   # -0.0 beats -0.5
    if band == (-INF, INF):
        assert count[1, 1] == 4 and np.isposinf(top[1, 1])  # (the NaN height of that cell is not counted, +-inf are)
    if band in ((0.0, 0.0), (-0.0, -0.0)):
        assert count.sum() == 4  # (float compares: -0.0 == +0.0, so both bands count all four zeros)


def test_height_keys_are_monotone_and_invertible():
    h = np.array([-INF, -3.0, -1e-40, -0.0, 0.0, 1e-40, 0.25, 2.5, INF], F32)
    k = og.height_keys(h)
    assert (np.diff(k.astype(np.int64)) > 0).all() and (k != 0).all()
    assert np.array_equal(og.heights_of_keys(k).view(np.uint32), h.view(np.uint32))
    assert og.heights_of_keys(np.zeros(1, np.uint32)).view(np.uint32)[0] == og.QNAN_BITS


# ---- the restatement against the oracle -----------------------------------------------------------------------------------
def test_restatement_against_the_oracle_on_a_kitti_frame(kitti, oracle_built):
    """The oracle's non-ground set and patch records of a KITTI frame through restate_query and restate_obstacles, against an
    independent route: the rows of expected_patches and the distances of expected_distances (test_gpu_point_planes.py, which
    knows RNR and the skip marker), binned into cells by integer arithmetic on a grid whose edges are exact."""
    oracle = oracle_built.restatement()
    p = oracle.default_params()
    pts = kitti[0]
    ref = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts)
    ng = np.sort(ref.nonground_idx)
    xyz = np.ascontiguousarray(pts[ng, :3], F32)
    s, near = gq.restate_query(xyz, ref.records, p)
    x0, y0, cell, nx, ny = -32.0, -24.0, 0.5, 128, 96
    # the cell another way: floor(2 c) in double is exact for a float, then an integer offset
    cx = np.floor(2.0 * xyz[:, 0].astype(np.float64)).astype(np.int64) + 64
    cy = np.floor(2.0 * xyz[:, 1].astype(np.float64)).astype(np.int64) + 48
    inside = (cx >= 0) & (cx < nx) & (cy >= 0) & (cy < ny)
    assert 20000 < inside.sum() < len(ng)
    o = cy * nx + cx
    count, top, unref = og.restate_obstacles(xyz, s, x0, y0, cell, nx, ny, -INF, INF)
    assert count.sum() + unref.sum() == inside.sum()
    assert np.array_equal((count + unref).reshape(-1), np.bincount(o[inside], minlength=nx * ny))
    assert unref.sum() == (inside & (s["patch"] < 0)).sum() > 0
    # a band above the ground: RNR points (patch -1 for expected_patches, far below the plane for the query) stay out either way
    own, _ = expected_patches(pts, ref, p, p.sensor_height)
    dist = expected_distances(pts, own, ref.records)[ng]
    with np.errstate(invalid="ignore"):
        in_band = inside & (dist >= F32(0.2)) & (dist <= F32(2.5))
    count, top, unref2 = og.restate_obstacles(xyz, s, x0, y0, cell, nx, ny, 0.2, 2.5)
    want = np.bincount(o[in_band], minlength=nx * ny).reshape(ny, nx)
    assert np.abs(count - want).sum() <= MAX_EDGE_POINTS and count.sum() > 5000
    assert np.array_equal(unref2, unref)
    wtop = np.full(nx * ny, -INF, F32)
    np.maximum.at(wtop, o[in_band], dist[in_band])
    same = (count == want) & (count > 0)
    assert same.sum() > 1000 and np.array_equal(top[same], wtop.reshape(ny, nx)[same])
    assert np.isnan(top[count == 0]).all() and not np.isnan(top[count > 0]).any()
    # ground_only moves the points of hidden patches from count to unref, cell by cell
    c3, _, u3 = og.restate_obstacles(xyz, s, x0, y0, cell, nx, ny, -INF, INF, ground_only=True)
    hidden = inside & (s["patch"] >= 0) & np.isin(s["decision"], gq.HIDDEN_DECISIONS)
    full = og.restate_obstacles(xyz, s, x0, y0, cell, nx, ny, -INF, INF)
    assert hidden.sum() > 0 and np.array_equal(c3 + u3, full[0] + full[2]) and u3.sum() - full[2].sum() == hidden.sum()
