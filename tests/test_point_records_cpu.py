"""No-GPU checks of the point records (pwpp_set_point_records, pwpp_get_*_records): exports and argument checks of the new
entry points, the Python bindings' methods, the C++ mirror's methods with and without Eigen types, and the ROS core demo."""
import ctypes
import os
import subprocess

import pytest

import pwpp_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")
NEW_SYMBOLS = ("pwpp_set_point_records", "pwpp_get_record_bytes", "pwpp_get_ground_records", "pwpp_get_nonground_records",
               "pwpp_get_all_records", "pwpp_get_device_records")


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
    assert "#define PWPP_HAS_POINT_RECORDS 1" in hdr
    assert "#define PWPP_VERSION_MINOR 4" in hdr  # (the feature macro announces the records, not a new minor version)


def test_new_entry_points_reject_a_null_handle(lib):
    buf = (ctypes.c_uint8 * 64)()
    base = (ctypes.c_int64 * 2)()
    counts = (ctypes.c_int32 * 8)()
    ptr, rb = ctypes.c_void_p(), ctypes.c_int32()
    assert lib.pwpp_set_point_records(None, 1) == -1
    assert lib.pwpp_set_point_records(None, 0) == -1
    assert lib.pwpp_get_record_bytes(None) == -1
    assert lib.pwpp_get_ground_records(None, 0, buf) == -1
    assert lib.pwpp_get_nonground_records(None, 0, buf) == -1
    assert lib.pwpp_get_all_records(None, buf, base, counts) == -1
    assert lib.pwpp_get_device_records(None, ctypes.byref(ptr), ctypes.byref(rb)) == -1
    assert lib.pwpp_get_device_records(None, None, None) == -1
    assert b"null" in lib.pwpp_last_error()


def test_handle_methods_exist():
    for name in ("set_point_records", "ground_records", "nonground_records", "all_records", "device_records"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    assert isinstance(pwpp_hip.Handle.record_bytes, property)


def test_pybind_module_has_the_point_record_methods():
    import pypatchworkpp
    cls = pypatchworkpp.patchworkpp
    for name in ("setPointRecords", "getGroundPoints", "getNongroundPoints"):
        assert hasattr(cls, name), name


CPP = r"""
#include "patchwork/patchworkpp.h"
#ifndef PWPP_HAS_POINT_RECORDS
#error "include/pwpp.h does not announce the point records"
#endif
float use(patchwork::PatchWorkpp &pw) {
    pw.setPointRecords(true);
#ifdef PWPP_HAVE_EIGEN
    Eigen::MatrixXf g = pw.getGroundPoints();
    Eigen::MatrixXf n = pw.getNongroundPoints();
#else
    patchwork::Points g = pw.getGroundPoints();
    patchwork::Points n = pw.getNongroundPoints();
#endif
    float intensity = 0.0f;
    for (int i = 0; i < g.rows(); ++i) intensity += g(i, g.cols() - 1);
    for (int i = 0; i < n.rows(); ++i) intensity += n(i, n.cols() - 1);
    const patchwork::Points gl = pw.groundPointRows(), nl = pw.nongroundPointRows();
    return intensity + (float)(gl.rows() * gl.cols() + nl.rows() * nl.cols());
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_methods_compile(tmp_path, flavour):
    src = tmp_path / "point_records.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    if flavour == "plain":
        cmd += ["-DPWPP_NO_EIGEN"]
    else:
        cmd += ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)


def test_ros_core_demo_builds_with_keep_fields(tmp_path, lib):
    """The ROS core with its keep_fields argument, and the demo around it, compile and link against the library."""
    exe = tmp_path / "ros_core_demo"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(PKG, "ros", "include"), "-I", os.path.join(PKG, "include"),
                    "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(PKG, "examples", "ros_core_demo.cpp"),
                    "-L", os.path.join(PKG, "lib"), "-lpwpp_hip", "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    assert exe.exists()
    core = open(os.path.join(PKG, "ros", "include", "patchworkpp_ros", "segmentation_core.hpp")).read()
    assert "bool keep_fields = false" in core  # (the default keeps the reference's payloads)
    glue = open(os.path.join(PKG, "ros", "src", "ground_segmentation_server.cpp")).read()
    assert 'declare_parameter<bool>("keep_fields", false)' in glue
    launch = open(os.path.join(PKG, "ros", "launch", "patchworkpp.launch.py")).read()
    assert '"keep_fields"' in launch
