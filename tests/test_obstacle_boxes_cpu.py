"""No-GPU checks of the obstacle boxes (pwpp_box_obstacles, pwpp_box_points): the exports, the feature macro, the ctypes
prototypes, the 64-byte row field by field, the bindings' methods, the C99 and C++ mirror in both flavours; the argument checks
that come before the device is touched; pwpp_box_points -- the functions the kernels compile, on the host -- byte for byte
against the restatement of tests/obstacle_boxes_ref.py over shaped, degenerate and far-origin point sets, with numpy.linalg.eigh
as a guard against a wrong axis formula; and the stand-alone program that runs the same functions against a long double /
__int128 computation of its own (tools/box_arith_check.cpp), built with the address and undefined-behaviour sanitizers where the
toolchain has them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import obstacle_boxes_ref as ob
import pwpp_hip
from obstacle_grid_ref import F32, QNAN_BITS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")
E_ARG = -1
GRID = (-20.0, -20.0, 0.5, 80, 80)  # x0, y0, cell, nx, ny


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pwpp_hip.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "lib/libpwpp_hip.so"], check=True, stdout=subprocess.DEVNULL)
    return pwpp_hip.load()


def test_symbols_macro_prototypes_and_layout(lib):
    hdr = open(os.path.join(ROOT, "include", "pwpp.h")).read()
    for name in ("pwpp_box_obstacles", "pwpp_box_points"):
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr
    assert "#define PWPP_HAS_OBSTACLE_BOXES 1" in hdr
    assert len(lib.pwpp_box_obstacles.argtypes) == 10 and len(lib.pwpp_box_points.argtypes) == 7
    assert lib.pwpp_box_obstacles.argtypes[2] is ctypes.c_float and lib.pwpp_box_obstacles.argtypes[3] is ctypes.c_float
    assert lib.pwpp_box_points.argtypes[4] is ctypes.c_int64
    assert ctypes.sizeof(pwpp_hip.ObstacleBox) == 64 == pwpp_hip.OBSTACLE_BOX_DTYPE.itemsize and ctypes.alignment(pwpp_hip.ObstacleBox) == 4
    assert pwpp_hip.OBSTACLE_BOX_DTYPE == ob.BOX_DTYPE
    want = ["points", "pad_", "mean_x", "mean_y", "cx", "cy", "ax", "ay", "length", "width", "sigma_long", "sigma_short", "h_min", "h_max", "z_min", "z_max"]
    assert [n for n, _ in pwpp_hip.ObstacleBox._fields_] == want == list(ob.BOX_DTYPE.names)
    for k, (name, ctype) in enumerate(pwpp_hip.ObstacleBox._fields_):
        assert getattr(pwpp_hip.ObstacleBox, name).offset == 4 * k == ob.BOX_DTYPE.fields[name][1], name
        assert ctype is (ctypes.c_int32 if k < 2 else ctypes.c_float) and ob.BOX_DTYPE.fields[name][0] == np.dtype("<i4" if k < 2 else "<f4")
    for name in ("box_obstacles", "box_obstacles_device"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    assert callable(pwpp_hip.box_points)
    import pypatchworkpp
    assert hasattr(pypatchworkpp.patchworkpp, "getObstacleBoxes")


def test_arguments_are_named_before_the_device_is_touched(lib):
    lab = np.zeros(16, np.int32)
    box = np.zeros(4, ob.BOX_DTYPE)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    g = pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 4, 4, 0, 0)

    def boxes(h=fake, gr=g, band=(0.2, 2.5), frames=1, mem=pwpp_hip.MEM_HOST, label=vp(lab), out=vp(box), max_boxes=4):
        return lib.pwpp_box_obstacles(h, ctypes.byref(gr) if gr is not None else None, band[0], band[1], 0, frames, mem, label, out, max_boxes)

    assert boxes(h=None) == E_ARG and b"null handle" in lib.pwpp_last_error()
    assert boxes(gr=None) == E_ARG and b"null grid" in lib.pwpp_last_error()
    assert boxes(label=None) == E_ARG and b"null label" in lib.pwpp_last_error()
    assert boxes(out=None) == E_ARG and b"null box table" in lib.pwpp_last_error()
    for m in (0, -1):
        assert boxes(max_boxes=m) == E_ARG and b"max_boxes" in lib.pwpp_last_error()
    assert boxes(band=(2.5, 0.2)) == E_ARG and b"height band" in lib.pwpp_last_error()
    assert boxes(band=(np.nan, 1.0)) == E_ARG and b"height band" in lib.pwpp_last_error()
    assert boxes(gr=pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 4, 4, 2, 0)) == E_ARG and b"grid flags" in lib.pwpp_last_error()
    for nx, ny, cell in ((1025, 4, 1.0), (4, 1025, 1.0), (2049, 2048, 0.5), (4, 4, 256.5), (4, 4, np.nan)):
        assert boxes(gr=pwpp_hip.GroundGrid(0.0, 0.0, cell, nx, ny, 0, 0)) == E_ARG and b"1024 m" in lib.pwpp_last_error(), (nx, ny, cell)
    assert boxes(mem=pwpp_hip.MEM_HOST_PINNED) == E_ARG and b"PWPP_MEM_HOST or PWPP_MEM_DEVICE" in lib.pwpp_last_error()
    assert boxes(frames=(1 << 12) + 1, max_boxes=1 << 12) == E_ARG and b"2^24" in lib.pwpp_last_error()
    assert boxes(frames=2, max_boxes=(1 << 23) + 1) == E_ARG and b"2^24" in lib.pwpp_last_error()

    xyz, hgt, row = np.zeros((2, 3), F32), np.zeros(2, F32), np.zeros(2, np.int32)

    def points(gr=g, xyz=vp(xyz), hgt=vp(hgt), row=vp(row), m=2, out=vp(box), max_boxes=4):
        return lib.pwpp_box_points(ctypes.byref(gr) if gr is not None else None, xyz, hgt, row, m, out, max_boxes)

    assert points() == 0
    assert points(gr=None) == E_ARG and points(out=None) == E_ARG and points(xyz=None) == E_ARG and points(hgt=None) == E_ARG and points(row=None) == E_ARG
    assert points(max_boxes=0) == E_ARG and points(m=-1) == E_ARG and points(m=(1 << 22) + 1) == E_ARG
    assert points(m=0, xyz=None, hgt=None, row=None) == 0
    assert points(gr=pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 1025, 4, 0, 0)) == E_ARG and b"1024 m" in lib.pwpp_last_error()
    assert points(gr=pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 1024, 1024, 0, 0)) == 0   # exactly 1024 m is inside
    for bad in (dict(nx=0), dict(cell=0.0), dict(cell=np.inf), dict(x0=np.nan)):
        kw = dict(dict(x0=0.0, y0=0.0, cell=1.0, nx=4, ny=4, flags=0, pad_=0), **bad)
        assert points(gr=pwpp_hip.GroundGrid(**kw)) == E_ARG, bad


CPP = r"""
#include "patchwork/patchworkpp.h"
#ifndef PWPP_HAS_OBSTACLE_BOXES
#error "include/pwpp.h does not announce the obstacle boxes"
#endif
static_assert(sizeof(pwpp_obstacle_box) == 64 && alignof(pwpp_obstacle_box) == 4, "64 bytes of 4-byte fields");
double use(patchwork::PatchWorkpp &pw) {
    patchwork::PatchWorkpp::ObstacleBoxes b = pw.getObstacleBoxes(-40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f);
    patchwork::PatchWorkpp::ObstacleBoxes d = pw.getObstacleBoxes(-40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f, 2, 4, true);
    return b.label[3 * 160 + 5] + b.count + (double)b.clusters.size() + (b.count ? b.boxes[0].length * b.boxes[0].ax + b.clusters[0].points : 0) + d.count;
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_method_compiles(tmp_path, flavour):
    src = tmp_path / "obstacle_boxes.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    cmd += ["-DPWPP_NO_EIGEN"] if flavour == "plain" else ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "boxes.c"
    src.write_text('#include "pwpp.h"\nint f(void) { pwpp_obstacle_box b; b.points = 0; b.z_max = 0.0f; return (int)sizeof(b) + b.points + (int)b.z_max; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# ---- pwpp_box_points against the restatement, byte for byte ----------------------------------------------------------------------
def both(grid, xyz, hgt, row, max_boxes):
    """(library rows, restated rows), asserted equal as bytes."""
    got = pwpp_hip.box_points(*grid, xyz, hgt, row, max_boxes)
    want = ob.box_rows(*grid, xyz, hgt, row, max_boxes)
    assert got.dtype == ob.BOX_DTYPE and got.shape == (max_boxes,)
    for r in range(max_boxes):
        assert got[r].tobytes() == want[r].tobytes(), "row %d:\n%s\n%s" % (r, got[r], want[r])
    return got, want


def eigh_guard(grid, xyz, box):
    """The axis the library reports against numpy.linalg.eigh on the exact covariance.  The eigenvector of a symmetric 2 x 2 matrix
    moves by about |E| / gap for a perturbation E; here E is the roundings of a, b, c and of eigh itself, a few 2^-52 of the
    matrix, plus the float rounding of the reported axis, 2^-24: tolerance = 2^-23 + 64 * 2^-52 / (relative gap)."""
    a, b, c = ob.covariance(*ob.row_moments(grid[0], grid[1], xyz))
    u, rel_gap = ob.axis_by_eigh(a, b, c)
    if rel_gap <= 0:
        return None
    tol = 2.0 ** -23 + 64 * 2.0 ** -52 / rel_gap
    assert abs(float(box["ax"]) - u[0]) <= tol and abs(float(box["ay"]) - u[1]) <= tol, (box["ax"], box["ay"], u, tol)
    return tol


@pytest.mark.parametrize("yaw", [30.0, 120.0])
def test_a_rectangle_at_two_headings(lib, yaw):
    xyz = ob.rectangle(500, 4.0, 1.8, yaw, (3.0, -2.0), seed=int(yaw))
    hgt = (xyz[:, 2] + F32(1.7)).astype(F32)
    got, _ = both(GRID, xyz, hgt, np.zeros(500, np.int32), 1)
    b = got[0]
    assert b["points"] == 500 and b["pad_"] == 0
    t = np.radians(yaw if yaw < 90 else yaw - 180)  # the sign rule: ax > 0
    assert b["ax"] > 0 and abs(b["ax"] - np.cos(t)) < 0.03 and abs(b["ay"] - np.sin(t)) < 0.03
    assert 3.8 < b["length"] <= 4.1 and 1.6 < b["width"] <= 1.9 and abs(b["cx"] - 3.0) < 0.1 and abs(b["cy"] + 2.0) < 0.1
    assert abs(b["sigma_long"] - 4.0 / np.sqrt(12)) < 0.1 and abs(b["sigma_short"] - 1.8 / np.sqrt(12)) < 0.06
    assert b["h_min"] == hgt.min() and b["h_max"] == hgt.max() and b["z_min"] == xyz[:, 2].min() and b["z_max"] == xyz[:, 2].max()
    assert eigh_guard(GRID, xyz, b) < 1e-6


def test_degenerate_rows(lib):
    one = np.array([[1.25, -3.5, 0.4]], F32)
    b = both(GRID, one, [0.7], [0], 1)[0][0]
    assert (b["points"], b["ax"], b["ay"], b["length"], b["width"], b["sigma_long"], b["sigma_short"]) == (1, 1, 0, 0, 0, 0, 0)
    assert (b["mean_x"], b["mean_y"], b["cx"], b["cy"]) == (1.25, -3.5, 1.25, -3.5) and b["h_min"] == b["h_max"] == F32(0.7)
    line = np.array([[2.0, -1.0, 0.0], [2.0, 3.0, 1.0]], F32)  # a vertical line: A == 0
    assert ob.covariance(*ob.row_moments(GRID[0], GRID[1], line))[0] == 0
    b = both(GRID, line, [0.1, 0.2], [0, 0], 1)[0][0]
    assert (b["ax"], b["ay"], b["length"], b["width"], b["cx"], b["cy"]) == (0, 1, 4, 0, 2, 1) and b["sigma_short"] == 0 and b["sigma_long"] == 2
    eigh_guard(GRID, line, b)
    square = np.array([[1, 1, 0], [3, 1, 0], [1, 3, 0], [3, 3, 0]], F32)  # isotropic: the axis is (1, 0)
    b = both(GRID, square, np.zeros(4, F32), np.zeros(4, np.int32), 1)[0][0]
    assert (b["ax"], b["ay"], b["length"], b["width"], b["cx"], b["cy"]) == (1, 0, 2, 2, 2, 2) and b["sigma_long"] == b["sigma_short"] == 1
    same = np.repeat(np.array([[0.3, 0.7, -1.0]], F32), 5, 0)  # coincident points
    b = both(GRID, same, np.full(5, 0.5, F32), np.zeros(5, np.int32), 1)[0][0]
    assert (b["points"], b["ax"], b["ay"], b["length"], b["width"], b["sigma_long"]) == (5, 1, 0, 0, 0, 0)


def test_skipped_points_and_empty_rows(lib):
    rng = np.random.default_rng(7)
    xyz = np.concatenate([ob.rectangle(60, 3.0, 1.0, 75.0, (-5.0, 4.0), 1), ob.rectangle(60, 2.0, 2.0, 10.0, (8.0, 8.0), 2)])
    hgt = rng.uniform(0.2, 2.5, 120).astype(F32)
    row = np.repeat([0, 2], 60).astype(np.int32)
    row[::7] = -1          # rows outside the table
    row[3::11] = 4
    row[5::13] = 1 << 30
    hgt[1::9] = np.nan     # a NaN height
    xyz[2::17, 0] = 30.0   # outside the grid (x0 + nx * cell = 20) ...
    xyz[4::19, 1] = -20.5  # ... below it ...
    xyz[6::23, 0] = np.nan  # ... and a NaN coordinate
    got, _ = both(GRID, xyz, hgt, row, 4)
    kept = (row >= 0) & (row < 4) & ~np.isnan(hgt) & (np.abs(xyz[:, 0]) < 20) & (xyz[:, 1] >= -20)
    assert got["points"].tolist() == [int((kept & (row == 0)).sum()), 0, int((kept & (row == 2)).sum()), 0] and got["points"][0] > 20
    for r in (1, 3):  # an empty row: points 0, pad_ 0, fourteen times the quiet NaN
        words = np.frombuffer(got[r].tobytes(), np.uint32)
        assert words[0] == 0 and words[1] == 0 and (words[2:] == QNAN_BITS).all()
    # nothing at all
    none = pwpp_hip.box_points(*GRID, np.zeros((0, 3), F32), np.zeros(0, F32), np.zeros(0, np.int32), 2)
    assert (np.frombuffer(none.tobytes(), np.uint32).reshape(2, 16)[:, 2:] == QNAN_BITS).all() and (none["points"] == 0).all()


def test_signed_zeros_and_infinities(lib):
    xyz = np.array([[1, 1, 0.0], [2, 1, -0.0], [3, 2, np.inf], [4, 2, -np.inf]], F32)
    hgt = np.array([0.0, -0.0, 0.0, -0.0], F32)
    b = both(GRID, xyz, hgt, np.zeros(4, np.int32), 1)[0][0]
    bits = lambda v: int(np.asarray(v, F32).view(np.uint32))
    assert bits(b["h_min"]) == 0x80000000 and bits(b["h_max"]) == 0      # -0.0 < +0.0
    assert b["z_min"] == -np.inf and b["z_max"] == np.inf
    b = both(GRID, xyz[:2], hgt[:2], np.zeros(2, np.int32), 1)[0][0]
    assert bits(b["z_min"]) == 0x80000000 and bits(b["z_max"]) == 0
    b = both(GRID, xyz[:2], np.array([np.inf, -np.inf], F32), np.zeros(2, np.int32), 1)[0][0]
    assert b["h_min"] == -np.inf and b["h_max"] == np.inf


def test_far_origin_products_beyond_64_bits(lib):
    """70 000 points 1000 m from the grid's origin: q is near 2^20 and N * Sxx needs more than 64 bits."""
    far = (-1000.0, -1000.0, 4.0, 256, 256)
    xyz = ob.rectangle(70000, 9.0, 2.5, 52.0, (10.0, 14.0), seed=3)
    N, Sx, Sy, Sxx, Sxy, Syy = ob.row_moments(far[0], far[1], xyz)
    assert N == 70000 and N * Sxx >= 1 << 64 and Sxx < 1 << 63 and Sx // N > 1 << 19
    rng = np.random.default_rng(11)
    b = both(far, xyz, rng.uniform(0.0, 2.0, N).astype(F32), np.zeros(N, np.int32), 1)[0][0]
    assert b["points"] == N and abs(b["ax"] - np.cos(np.radians(52.0))) < 0.01 and 8.9 < b["length"] < 9.1 and 2.4 < b["width"] < 2.6
    assert abs(b["cx"] - 10.0) < 0.05 and abs(b["cy"] - 14.0) < 0.05
    assert eigh_guard(far, xyz, b) < 1e-6
    # several rows at once, in any order of the points: the same bytes
    row = (np.arange(N) % 3).astype(np.int32)
    hgt = rng.uniform(0.0, 2.0, N).astype(F32)
    perm = rng.permutation(N)
    a = pwpp_hip.box_points(*far, xyz, hgt, row, 3)
    assert a.tobytes() == pwpp_hip.box_points(*far, xyz[perm], hgt[perm], row[perm], 3).tobytes() == ob.box_rows(*far, xyz, hgt, row, 3).tobytes()


# ---- the same functions against long double and __int128, stand-alone --------------------------------------------------------------
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def sanitizers_work(tmp_path):
    """The toolchain links the two runtimes into a program and that program starts in this environment."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        return False
    return subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0


def test_box_arith_program_builds_and_passes(tmp_path):
    exe = tmp_path / "box_arith_check"
    flags = SANITIZE if sanitizers_work(tmp_path) else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags +
                   ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "box_arith_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)  # (a stand-alone child process with its own main)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 mismatches" in r.stdout and "916 cases" in r.stdout
