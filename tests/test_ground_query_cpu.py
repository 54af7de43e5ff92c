"""No-GPU checks of the ground queries (pwpp_query_ground, pwpp_rasterize_ground): exports, the layout of the two structs, the
argument checks that need no device, the bindings' methods, the C++ mirror with and without Eigen types -- and the numpy
restatement the GPU tests compare against, checked here against the oracle's own records on a KITTI frame."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import pwpp_hip
import ground_query_ref as gq
from test_gpu_point_planes import EDGE_TOL, GROUND_DECISIONS, MAX_EDGE_POINTS, czm_bins, expected_distances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")
NEW_SYMBOLS = ("pwpp_query_ground", "pwpp_rasterize_ground")
F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pwpp_hip.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "lib/libpwpp_hip.so"], check=True, stdout=subprocess.DEVNULL)
    return pwpp_hip.load()


def test_new_symbols_are_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, "include", "pwpp.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr, name
    assert "#define PWPP_HAS_GROUND_QUERY 1" in hdr
    assert "#define PWPP_VERSION_MINOR 4" in hdr  # (the feature macro announces the queries, not a new minor version)
    assert "enum { PWPP_GRID_GROUND_ONLY = 1 };" in hdr


def test_struct_layouts():
    s = pwpp_hip.GroundSample
    assert ctypes.sizeof(s) == 16
    assert [(n, getattr(s, n).offset) for n, _ in s._fields_] == [("patch", 0), ("decision", 4), ("ground_z", 8), ("distance", 12)]
    assert ctypes.sizeof(pwpp_hip.GroundGrid) == 40
    assert pwpp_hip.GroundGrid.nx.offset == 24 and pwpp_hip.GroundGrid.flags.offset == 32
    dt = pwpp_hip.GROUND_SAMPLE_DTYPE
    assert dt.itemsize == 16 and dt.names == ("patch", "decision", "ground_z", "distance")
    assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12]
    assert dt == gq.SAMPLE_DTYPE


def test_arguments_checked_before_the_device_is_touched(lib):
    xyz = np.zeros((4, 3), F32)
    out = np.zeros(4, pwpp_hip.GROUND_SAMPLE_DTYPE)
    img = np.zeros(16, F32)
    g = pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 4, 4, 0, 0)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.pwpp_query_ground(None, vp(xyz), None, 4, pwpp_hip.MEM_HOST, vp(out)) == -1
    assert b"null" in lib.pwpp_last_error()
    assert lib.pwpp_rasterize_ground(None, ctypes.byref(g), 0, 1, pwpp_hip.MEM_HOST, vp(img), None) == -1
    assert b"null" in lib.pwpp_last_error()


def test_handle_and_module_methods_exist():
    for name in ("query_ground", "rasterize_ground", "query_ground_device", "rasterize_ground_device"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    import pypatchworkpp
    for name in ("queryGround", "getElevationMap"):
        assert hasattr(pypatchworkpp.patchworkpp, name), name


CPP = r"""
#include "patchwork/patchworkpp.h"
#ifndef PWPP_HAS_GROUND_QUERY
#error "include/pwpp.h does not announce the ground queries"
#endif
float use(patchwork::PatchWorkpp &pw) {
    const float xyz[6] = {5.0f, 1.0f, -1.7f, -9.0f, 2.0f, 0.3f};
    std::vector<pwpp_ground_sample> s = pw.queryGround(xyz, 2);
    float acc = s[0].ground_z + s[1].distance + (float)(s[0].patch + s[1].decision);
#ifdef PWPP_HAVE_EIGEN
    Eigen::MatrixX3f pos(2, 3);
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 3; ++j) pos(i, j) = xyz[3 * i + j];
    acc += pw.queryGround(pos)[1].ground_z;
    Eigen::MatrixXf img = pw.getElevationMap(-40.0, -40.0, 0.5, 160, 160, true);
#else
    patchwork::Points img = pw.getElevationMap(-40.0, -40.0, 0.5, 160, 160, true);
#endif
    const patchwork::Points rows = pw.elevationMapRows(-40.0, -40.0, 0.5, 160, 160);
    return acc + img(3, 5) + rows(3, 5) + (float)(img.rows() * img.cols());
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_methods_compile(tmp_path, flavour):
    src = tmp_path / "ground_query.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    if flavour == "plain":
        cmd += ["-DPWPP_NO_EIGEN"]
    else:
        cmd += ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)


def test_restatement_against_the_oracle_records(kitti, oracle_built):
    """For every oracle ground point of a patch decided ground, the restated query of the point's own position gives the
    distance of expected_distances (test_gpu_point_planes.py) bit for bit; its ground_z is the height at which the same plane
    passes the point's (x, y), so (z - ground_z) * n2 is that distance up to float rounding."""
    oracle = oracle_built.restatement()
    p = oracle.default_params()
    pts = kitti[0]
    ref = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts)
    recs = ref.records
    xyz = np.ascontiguousarray(pts[:, :3], F32)
    got, near = gq.restate_query(xyz, recs, p)
    ground = np.zeros(len(pts), bool)
    ground[ref.ground_idx] = True
    sel = ground & (got["patch"] >= 0) & np.isin(got["decision"], GROUND_DECISIONS)
    # every ground point of the oracle lies in a patch decided ground (its bin's): the restated bin finds it, edge points apart
    assert (ground & ~sel & ~near).sum() == 0 and (ground & ~sel).sum() <= MAX_EDGE_POINTS
    assert sel.sum() > 30000
    exp = expected_distances(pts, got["patch"], recs)
    assert np.array_equal(got["distance"][sel].view(np.uint32), exp[sel].view(np.uint32))
    # the counts per patch are the records' n_ground
    per = np.bincount(got["patch"][sel], minlength=len(recs))
    want = np.where(np.isin(recs["decision"], GROUND_DECISIONS), recs["n_ground"], 0)
    assert np.abs(per - want).sum() <= MAX_EDGE_POINTS
    n2 = recs["normal"][got["patch"][sel], 2].astype(np.float64)
    lift = (xyz[sel, 2].astype(np.float64) - got["ground_z"][sel].astype(np.float64)) * n2
    assert np.abs(lift - got["distance"][sel]).max() < 2e-5
    # a position with no patch: outside the range, NaN, inf
    odd = np.array([[0, 0, 0], [1e3, 0, 0], [np.nan, 1, 0], [1, np.inf, 0], [0.5, 0.5, -1.7]], F32)
    none, _ = gq.restate_query(odd, recs, p)
    assert (none["patch"] == -1).all() and (none["decision"] == 0).all()
    assert np.isnan(none["ground_z"]).all() and np.isnan(none["distance"]).all()


def test_the_uniform_draw_of_the_gpu_test_stays_off_the_edges(oracle_built):
    """The 4 000 uniform positions of tests/test_gpu_ground_query.py: fewer than MAX_EDGE_POINTS of them within EDGE_TOL of a bin
    edge, so the allowance of the GPU test is not what makes it pass."""
    from test_gpu_ground_query import FIXED_POSITIONS, uniform_positions
    p = oracle_built.restatement().default_params()
    _, near = czm_bins(uniform_positions(), p)
    assert near.sum() == 0
    code, near = czm_bins(FIXED_POSITIONS, p)
    assert (code >= 0).sum() >= 12 and (code == -1).sum() >= 5
    assert EDGE_TOL == 1e-9
