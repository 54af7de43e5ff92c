"""No-GPU checks of the per-point patch rows and plane distances (pwpp_set_point_planes): argument checks and exports of the
new entry points, the Python bindings' methods, and the C++ mirror's methods with and without Eigen types."""
import ctypes
import os
import subprocess

import pytest

import pwpp_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")
NEW_SYMBOLS = ("pwpp_set_point_planes", "pwpp_get_point_patches", "pwpp_get_point_distances", "pwpp_get_all_point_patches",
               "pwpp_get_all_point_distances", "pwpp_get_device_point_planes")


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
    assert "#define PWPP_VERSION_MINOR 4" in hdr


def test_new_entry_points_reject_a_null_handle(lib):
    pat = (ctypes.c_int32 * 16)()
    dist = (ctypes.c_float * 16)()
    pp, dp = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.pwpp_set_point_planes(None, 1) == -1
    assert lib.pwpp_set_point_planes(None, 0) == -1
    assert lib.pwpp_get_point_patches(None, 0, pat) == -1
    assert lib.pwpp_get_point_distances(None, 0, dist) == -1
    assert lib.pwpp_get_all_point_patches(None, pat) == -1
    assert lib.pwpp_get_all_point_distances(None, dist) == -1
    assert lib.pwpp_get_device_point_planes(None, ctypes.byref(pp), ctypes.byref(dp)) == -1
    assert lib.pwpp_get_device_point_planes(None, None, None) == -1


def test_handle_methods_exist():
    for name in ("set_point_planes", "point_patches", "point_distances", "all_point_patches", "all_point_distances",
                 "device_point_planes"):
        assert callable(getattr(pwpp_hip.Handle, name)), name


def test_pybind_module_has_the_point_plane_methods():
    import pypatchworkpp
    cls = pypatchworkpp.patchworkpp
    for name in ("setPointPlanes", "getPointPatches", "getPointDistances"):
        assert hasattr(cls, name), name


CPP = r"""
#include <cmath>
#include "patchwork/patchworkpp.h"
int use(patchwork::PatchWorkpp &pw) {
    pw.setPointPlanes(true);
#ifdef PWPP_HAVE_EIGEN
    Eigen::VectorXi p = pw.getPointPatches();
    Eigen::VectorXf d = pw.getPointDistances();
#else
    patchwork::Indices p = pw.getPointPatches();
    patchwork::Distances d = pw.getPointDistances();
#endif
    int above = 0;
    for (int i = 0; i < p.rows(); ++i) above += p(i) >= 0 && d(i) > 0.2f && !std::isnan(d(i));
    const patchwork::Indices pl = pw.pointPatchList();
    const patchwork::Distances dl = pw.pointDistanceList();
    return above + pl.rows() + dl.rows();
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_methods_compile(tmp_path, flavour):
    src = tmp_path / "point_planes.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    if flavour == "plain":
        cmd += ["-DPWPP_NO_EIGEN"]
    else:
        cmd += ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)
