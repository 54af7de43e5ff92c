"""No-GPU checks of the per-point labels and the cloud-order output mode: the header's constants, the
Python binding's, argument checks of the new entry points, and the pybind11 module's methods."""
import ctypes
import os
import re
import subprocess

import pytest

import pwpp_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pwpp_hip.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "lib/libpwpp_hip.so"], check=True, stdout=subprocess.DEVNULL)
    return pwpp_hip.load()


def header_enum(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pwpp.h")).read(), flags=re.S)
    m = re.search(r"\b%s\s*=\s*(-?\d+)" % name, hdr)
    assert m, "%s is not in pwpp.h" % name
    return int(m.group(1))


def test_header_constants_equal_the_binding():
    for name in ("LABEL_NONGROUND", "LABEL_GROUND", "LABEL_UNCLASSIFIED", "ORDER_SCATTER", "ORDER_REFERENCE", "ORDER_CLOUD"):
        assert header_enum("PWPP_" + name) == getattr(pwpp_hip, name), name
    assert (pwpp_hip.LABEL_NONGROUND, pwpp_hip.LABEL_GROUND, pwpp_hip.LABEL_UNCLASSIFIED) == (0, 1, 2)
    assert pwpp_hip.ORDER_CLOUD == 2


def test_new_entry_points_reject_a_null_handle(lib):
    buf = (ctypes.c_uint8 * 16)()
    ptr = ctypes.c_void_p()
    assert lib.pwpp_set_labels(None, 1) == -1
    assert lib.pwpp_set_labels(None, 0) == -1
    assert lib.pwpp_get_labels(None, 0, buf) == -1
    assert lib.pwpp_get_all_labels(None, buf) == -1
    assert lib.pwpp_get_device_labels(None, ctypes.byref(ptr)) == -1
    assert lib.pwpp_set_output_order(None, pwpp_hip.ORDER_CLOUD) == -1


def test_handle_methods_exist():
    for name in ("set_labels", "set_order", "labels", "all_labels", "device_labels", "set_output_order"):
        assert callable(getattr(pwpp_hip.Handle, name)), name


def test_pybind_module_has_the_label_methods():
    import pypatchworkpp
    cls = pypatchworkpp.patchworkpp
    for name in ("getLabels", "setLabels", "setCloudOrder", "setReferenceOrder"):
        assert hasattr(cls, name), name
