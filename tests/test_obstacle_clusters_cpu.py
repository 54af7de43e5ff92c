"""No-GPU checks of the obstacle clusters (pwpp_label_grid, pwpp_label_obstacles): the exports, the feature macro, the ctypes
prototypes and the bindings' methods, the argument checks that need no device, the C++ mirror in both flavours -- the flood fill
the GPU tests compare against (tests/obstacle_clusters_ref.py) against a second restatement over the whole pattern set, and at the
large shapes (more chunks than one round of the rank scan) also against the structured patterns' construction -- and the
stand-alone program that runs the kernels' union-find primitives and pass sequence on the host against a flood fill of its own
(tools/unionfind_check.cpp), built with the address and undefined-behaviour sanitizers where the toolchain has them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import obstacle_clusters_ref as oc
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
    for name in ("pwpp_label_grid", "pwpp_label_obstacles"):
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr
    assert "#define PWPP_HAS_OBSTACLE_CLUSTERS 1" in hdr
    assert len(lib.pwpp_label_grid.argtypes) == 13 and len(lib.pwpp_label_obstacles.argtypes) == 16
    assert lib.pwpp_label_obstacles.argtypes[2] is ctypes.c_float and lib.pwpp_label_obstacles.argtypes[3] is ctypes.c_float
    assert ctypes.sizeof(pwpp_hip.ObstacleCluster) == 48 == pwpp_hip.OBSTACLE_CLUSTER_DTYPE.itemsize
    assert pwpp_hip.OBSTACLE_CLUSTER_DTYPE == oc.CLUSTER_DTYPE
    for (name, ctype), (dname, (dt, off)) in zip(pwpp_hip.ObstacleCluster._fields_, sorted(oc.CLUSTER_DTYPE.fields.items(), key=lambda kv: kv[1][1])):
        assert name == dname and getattr(pwpp_hip.ObstacleCluster, name).offset == off and ctypes.sizeof(ctype) == dt.itemsize
    for name in ("label_grid", "label_grid_device", "label_obstacles", "label_obstacles_device"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    import pypatchworkpp
    assert hasattr(pypatchworkpp.patchworkpp, "getObstacleClusters")


def test_null_and_range_arguments_are_named_before_the_device_is_touched(lib):
    cnt, lab = np.zeros(16, np.int32), np.zeros(16, np.int32)
    tab = np.zeros(4, oc.CLUSTER_DTYPE)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    H = pwpp_hip.MEM_HOST

    def grid(h=fake, nx=4, ny=4, frames=1, mem=H, count=vp(cnt), min_count=1, conn=8, label=vp(lab), clusters=None, max_clusters=0):
        return lib.pwpp_label_grid(h, nx, ny, frames, mem, count, None, min_count, conn, label, clusters, None, max_clusters)

    assert grid(h=None) == E_ARG and b"null handle" in lib.pwpp_last_error()
    assert grid(label=None) == E_ARG and b"null label" in lib.pwpp_last_error()
    assert grid(count=None) == E_ARG and b"null count" in lib.pwpp_last_error()
    for kw in (dict(nx=0), dict(ny=0), dict(frames=0), dict(nx=-3)):
        assert grid(**kw) == E_ARG and b"cells" in lib.pwpp_last_error(), kw
    assert grid(nx=65536, ny=32768) == E_ARG and b"2^31 - 1" in lib.pwpp_last_error()   # nx * ny = 2^31
    assert grid(nx=65536, ny=16384, frames=3) == E_ARG and b"exceed 2^31" in lib.pwpp_last_error()
    assert grid(min_count=0) == E_ARG and b"min_count" in lib.pwpp_last_error()
    for conn in (0, 1, 6, 9, -8):
        assert grid(conn=conn) == E_ARG and b"connectivity" in lib.pwpp_last_error(), conn
    assert grid(max_clusters=-1) == E_ARG and b"max_clusters" in lib.pwpp_last_error()
    assert grid(max_clusters=4) == E_ARG and b"null cluster table" in lib.pwpp_last_error()
    assert grid(mem=pwpp_hip.MEM_DEVICE, clusters=ctypes.c_void_p(vp(tab).value + 4), max_clusters=1) == E_ARG and b"8-byte" in lib.pwpp_last_error()
    assert grid(mem=2) == E_ARG and b"PWPP_MEM_HOST or PWPP_MEM_DEVICE" in lib.pwpp_last_error()   # PWPP_MEM_HOST_PINNED

    g = pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 4, 4, 0, 0)

    def obstacles(h=fake, gr=ctypes.byref(g), band=(0.2, 2.5), min_count=1, conn=8, label=vp(lab), clusters=None, max_clusters=0):
        return lib.pwpp_label_obstacles(h, gr, band[0], band[1], min_count, conn, 0, 1, H, label, None, None, clusters, None, max_clusters, None)

    assert obstacles(h=None) == E_ARG and b"null handle" in lib.pwpp_last_error()
    assert obstacles(gr=None) == E_ARG and b"null grid" in lib.pwpp_last_error()
    assert obstacles(label=None) == E_ARG and b"null label" in lib.pwpp_last_error()
    assert obstacles(band=(2.5, 0.2)) == E_ARG and b"height band" in lib.pwpp_last_error()
    assert obstacles(band=(np.nan, 1.0)) == E_ARG and b"height band" in lib.pwpp_last_error()
    assert obstacles(min_count=0) == E_ARG and b"min_count" in lib.pwpp_last_error()
    assert obstacles(conn=5) == E_ARG and b"connectivity" in lib.pwpp_last_error()
    assert obstacles(max_clusters=-2) == E_ARG and b"max_clusters" in lib.pwpp_last_error()
    assert obstacles(max_clusters=2) == E_ARG and b"null cluster table" in lib.pwpp_last_error()
    bad = pwpp_hip.GroundGrid(0.0, 0.0, 1.0, 4, 4, 2, 0)
    assert obstacles(gr=ctypes.byref(bad)) == E_ARG and b"grid flags" in lib.pwpp_last_error()


CPP = r"""
#include "patchwork/patchworkpp.h"
#ifndef PWPP_HAS_OBSTACLE_CLUSTERS
#error "include/pwpp.h does not announce the obstacle clusters"
#endif
static_assert(sizeof(pwpp_obstacle_cluster) == 48, "48 bytes");
long use(patchwork::PatchWorkpp &pw) {
    patchwork::PatchWorkpp::ObstacleClusters c = pw.getObstacleClusters(-40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f);
    patchwork::PatchWorkpp::ObstacleClusters d = pw.getObstacleClusters(-40.0, -40.0, 0.5, 160, 160, 0.2f, 2.5f, 2, 4, true);
    return c.label[3 * 160 + 5] + c.count + (long)c.clusters.size() + (c.count ? c.clusters[0].sum_ix + c.clusters[0].first_cell : 0) + d.count;
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_method_compiles(tmp_path, flavour):
    src = tmp_path / "obstacle_clusters.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    cmd += ["-DPWPP_NO_EIGEN"] if flavour == "plain" else ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "clusters.c"
    src.write_text('#include "pwpp.h"\nint f(void) { pwpp_obstacle_cluster c; c.sum_ix = 0; return (int)sizeof(c) + (int)c.sum_ix; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# ---- the flood fill against a second restatement, over the pattern set -------------------------------------------------------
@pytest.mark.parametrize("shape", oc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_flood_fill_against_minimum_propagation(shape):
    nx, ny = shape
    seen = 0
    for name in oc.PATTERNS:
        for min_count in (1, 2):
            count, top = oc.pattern(name, nx, ny, min_count)
            assert count.min() >= 0 and count.max() <= 3
            for conn in (4, 8):
                label, table, n = oc.flood_fill(count, top, min_count, conn)
                label2, n2 = oc.min_propagation(count, min_count, conn)
                what = "%s %dx%d min_count %d connectivity %d" % (name, nx, ny, min_count, conn)
                assert n == n2 and np.array_equal(label, label2), what
                assert np.array_equal(label >= 0, count >= min_count), what
                assert len(table) == n and (np.diff(table["first_cell"]) > 0).all(), what   # ranks in ascending first_cell
                assert table["cells"].sum() == (count >= min_count).sum() and table["points"].sum() == count[count >= min_count].sum(), what
                for r in range(min(n, 3)):  # a row by its definition, another way
                    iy, ix = np.nonzero(label == r)
                    c = count[iy, ix].astype(np.int64)
                    row = table[r]
                    assert row["first_cell"] == (iy * nx + ix).min() and label.reshape(-1)[row["first_cell"]] == r, what
                    assert (row["ix_min"], row["ix_max"], row["iy_min"], row["iy_max"]) == (ix.min(), ix.max(), iy.min(), iy.max()), what
                    assert row["sum_ix"] == (c * ix).sum() and row["sum_iy"] == (c * iy).sum() and row["top"] == top[iy, ix].max(), what
                seen += n
                occ = (count >= min_count).sum()
                if name == "empty":
                    assert n == 0
                if name == "full":
                    assert n == 1
                if name == "checker":
                    assert n == (occ if conn == 4 else 1)
                if name in ("comb", "spiral", "serpentine"):
                    assert n == 1, what
                if name == "corner" and nx > oc.TILE_X and ny > oc.TILE_Y:
                    assert n == (2 if conn == 4 else 1), what
    assert seen > 0


# ---- the large shapes: more chunks than one round of the rank scan takes ------------------------------------------------------------
def test_large_shapes_need_the_scan_rounds_the_table_says():
    """The table of oc.LARGE_PLAN from the constants as the kernels have them: a retuned chunk or block fails here instead of
    quietly taking the point out of the large shapes."""
    unionfind = open(os.path.join(PKG, "csrc", "pwpp_unionfind.h")).read()
    kernels = open(os.path.join(PKG, "csrc", "pwpp_clusters.hip")).read()
    assert "#define PWPP_CL_CHUNK %d " % oc.CHUNK in unionfind
    assert "#define PWPP_CL_TILE_X %d " % oc.TILE_X in unionfind and "#define PWPP_CL_TILE_Y %d\n" % oc.TILE_Y in unionfind
    assert "constexpr int kClBlock = %d;" % oc.SCAN_BLOCK in kernels and "base += kClBlock" in kernels
    assert sorted(oc.LARGE_PLAN) == sorted(oc.LARGE_SHAPES) and not set(oc.LARGE_SHAPES) & set(oc.SHAPES)
    for shape in oc.LARGE_SHAPES:
        assert oc.chunk_plan(*shape) == oc.LARGE_PLAN[shape], shape
    assert max(oc.chunk_plan(*s)[1] for s in oc.SHAPES) == 17  # the small shapes: one round, never full
    assert oc.chunk_plan(256, 256)[2] == [oc.SCAN_BLOCK]       # one round, full
    assert oc.chunk_plan(257, 256)[2] == [oc.SCAN_BLOCK, 1] and 257 % oc.TILE_X == 1
    assert oc.chunk_plan(1030, 132)[2] == [oc.SCAN_BLOCK, oc.SCAN_BLOCK, 20] and 1030 * 132 % oc.CHUNK == 24
    assert 1030 % oc.TILE_X and 132 % oc.TILE_Y
    assert all(name in oc.PATTERNS for name in oc.LARGE_PATTERNS) and len(oc.LARGE_CASES) == 20


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", oc.LARGE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_flood_fill_at_the_large_shapes_against_anchors_that_share_nothing_with_it(shape, connectivity):
    """Minimum propagation where paths are short (the random patterns, checker, diagonals, comb: a spiral or serpentine needs an
    iteration per cell of its path), and the structured patterns by construction.  Then the two conditions that make the scan's
    carry visible in the labels: enough clusters whose first cell lies beyond chunk 255, and beyond chunk 511."""
    nx, ny = shape
    cells, chunks, rounds, _ = oc.chunk_plan(nx, ny)
    for name, min_count, conn in oc.LARGE_CASES:
        if conn != connectivity:
            continue
        count, top = oc.pattern(name, nx, ny, min_count)
        label, table, n = oc.flood_fill(count, top, min_count, conn)
        what = "%s %dx%d min_count %d connectivity %d" % (name, nx, ny, min_count, conn)
        occ = count >= min_count
        assert np.array_equal(label >= 0, occ) and len(table) == n and (np.diff(table["first_cell"]) > 0).all(), what
        assert table["cells"].sum() == occ.sum() and table["points"].sum() == count[occ].sum(), what
        anchors = 0
        if name.startswith("random") or name in ("checker", "diagonals", "comb"):
            label2, n2 = oc.min_propagation(count, min_count, conn)
            assert n == n2 and np.array_equal(label, label2), what
            anchors += 1
        built = oc.by_construction(name, conn, count, min_count)
        if built is not None:
            assert n == built[1] and np.array_equal(label, built[0]), what
            anchors += 1
        assert anchors > 0, what
        if name == "checker":
            assert n == ((cells + 1) // 2 if conn == 4 else 1), what
        beyond_1, beyond_2 = oc.roots_beyond(table, oc.SCAN_BLOCK), oc.roots_beyond(table, 2 * oc.SCAN_BLOCK)
        print("%s: n %d, roots beyond chunk 255: %d, beyond chunk 511: %d" % (what, n, beyond_1, beyond_2))
        if conn == 4 and min_count == 1 and name in ("random0.3", "checker"):
            if len(rounds) > 1:
                # the cells beyond chunk 255: 257 x 256 has only 256 of them, a part of its last row, of which random0.3 occupies
                # about 77 -- 100 roots cannot be there; at least 10 is asked of it, as of the third round below
                few = name == "random0.3" and cells - oc.CHUNK * oc.SCAN_BLOCK <= oc.CHUNK
                assert beyond_1 >= (10 if few else 100), what
            if len(rounds) > 2:
                assert beyond_2 >= 10, what


def test_frames_never_connect_in_the_restatement():
    count = np.zeros((2, 5, 7), np.int32)
    count[0, -1, :] = 1
    count[1, 0, :] = 2
    label, tables, n = oc.label_frames(count, None, 1, 8, max_clusters=4)
    assert n.tolist() == [1, 1] and tables[0]["first_cell"][0] == 4 * 7 and tables[1]["first_cell"][0] == 0
    assert np.isnan(tables[0]["top"][0])  # no top image


# ---- the kernels' primitives and pass sequence on the host ---------------------------------------------------------------------
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def sanitizers_work(tmp_path):
    """The toolchain links the two runtimes into a program and that program starts in this environment."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        return False
    return subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0


def test_unionfind_program_builds_and_passes(tmp_path):
    exe = tmp_path / "unionfind_check"
    flags = SANITIZE if sanitizers_work(tmp_path) else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags +
                   ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "unionfind_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)  # (a stand-alone child process with its own main)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 mismatches" in r.stdout and "880 cases" in r.stdout  # (10 shapes, 257 x 256 and 1030 x 132 among them)
