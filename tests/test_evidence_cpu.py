"""No-GPU checks of the map evidence (pwpp_evidence_grid, pwpp_evidence_obstacles, pwpp_evidence_verdict): the exports, the feature
macro and its place, the size of pwpp_cluster_evidence, the ctypes prototypes and the bindings' methods; every argument check of
pwpp_evidence_grid with its message and its place in the order, and those of pwpp_evidence_obstacles that come before it looks at
its handle; the host's verdict against the restatement at exact ratio boundaries; the C++ mirror in both flavours and the header as
C99; the stand-alone program that runs the kernels' functions on the host against a brute force of its own
(tools/evidence_check.cpp), built with the address and undefined-behaviour sanitizers where the toolchain has them, whose dump is
compared with the restatement (tests/evidence_ref.py); and a scenario on the restatements alone: a wall and a blob that moves through
free space, fused by tests/occupancy_fusion_ref.py, classified, masked and fused again."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import evidence_ref as er
import occupancy_fusion_ref as fr
import pwpp_hip

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
    for name in ("pwpp_evidence_grid", "pwpp_evidence_obstacles", "pwpp_evidence_verdict"):
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr
    assert "#define PWPP_HAS_MAP_EVIDENCE 1" in hdr and "typedef struct pwpp_cluster_evidence {" in hdr and "typedef struct pwpp_evidence_rule {" in hdr
    assert "#define PWPP_VERSION_MINOR 4 " in hdr
    # declared after pwpp_track_obstacles and before the input transforms
    assert hdr.index("PWPP_API int pwpp_track_obstacles(") < hdr.index("PWPP_HAS_MAP_EVIDENCE") < hdr.index("PWPP_API int pwpp_evidence_grid(")
    assert hdr.index("PWPP_API int pwpp_evidence_grid(") < hdr.index("PWPP_API int pwpp_evidence_obstacles(") < hdr.index("PWPP_API int pwpp_evidence_verdict(")
    assert hdr.index("PWPP_API int pwpp_evidence_verdict(") < hdr.index("#define PWPP_HAS_INPUT_TRANSFORM")
    section = " ".join(hdr[hdr.index("---- map evidence"):hdr.index("#define PWPP_HAS_MAP_EVIDENCE")].split()).replace(" * ", " ")
    assert "THE PRICE: a mover within `gate` cells of a mapped wall reads as wall" in section  # the price of the maximum is stated
    assert "96 of a CU's 160 KiB" in section  # ... and how PWPP_EVID_LDS_ROWS was chosen
    assert "#define PWPP_EVID_LDS_ROWS %d\n" % pwpp_hip.EVID_LDS_ROWS in hdr
    assert "PWPP_EVID_NONE = -1, PWPP_EVID_UNDECIDED = 0, PWPP_EVID_STATIC = 1, PWPP_EVID_MOVING = 2" in hdr and "PWPP_EVID_CELL_NONE = -2" in hdr
    assert (pwpp_hip.EVID_NONE, pwpp_hip.EVID_UNDECIDED, pwpp_hip.EVID_STATIC, pwpp_hip.EVID_MOVING, pwpp_hip.EVID_CELL_NONE) == (-1, 0, 1, 2, -2)
    assert (er.NONE, er.UNDECIDED, er.STATIC, er.MOVING, er.CELL_NONE) == (-1, 0, 1, 2, -2)
    assert pwpp_hip.CLUSTER_EVIDENCE_DTYPE.itemsize == 32 and er.EVIDENCE == pwpp_hip.CLUSTER_EVIDENCE_DTYPE
    assert pwpp_hip.CLUSTER_EVIDENCE_DTYPE.names == ("sum", "cells", "landed", "occupied", "free", "unknown", "verdict")
    assert ctypes.sizeof(pwpp_hip.EvidenceRule) == 16 and [f[0] for f in pwpp_hip.EvidenceRule._fields_] == ["gate", "min_cells", "moving_share", "static_share"]
    assert len(lib.pwpp_evidence_grid.argtypes) == 17 and len(lib.pwpp_evidence_obstacles.argtypes) == 27 and len(lib.pwpp_evidence_verdict.argtypes) == 6
    for name in ("evidence_grid", "evidence_grid_device", "evidence_obstacles", "evidence_verdict"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    assert callable(pwpp_hip.evidence_verdict)
    import pypatchworkpp
    assert hasattr(pypatchworkpp.patchworkpp, "getObstacleEvidence")
    doc = pypatchworkpp.patchworkpp.getObstacleEvidence.__doc__
    assert "pose:" in doc and "= [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]" in doc and "gate:" in doc and "moving_share:" in doc and "max_clusters:" in doc
    src = open(os.path.join(PKG, "csrc", "pwpp_evidence.h")).read()
    for name in ("pwpp_evid_row", "pwpp_evid_landed", "pwpp_evid_read", "pwpp_evid_class", "pwpp_evid_verdict", "pwpp_evid_mask", "pwpp_evid_rule_check"):
        assert "PWPP_HD inline" in src and name + "(" in src, name
    assert '#include "pwpp_match.h"' in src and "pwpp_match_landing<RECIP>(" in src and "floor" not in src  # the landing is called, not restated
    assert "pwpp_fuse_byte(" in src  # ... and so is the fusion's byte rule
    kernels = open(os.path.join(PKG, "csrc", "pwpp_evidence.hip")).read()
    assert '#include "pwpp_evidence.h"' in kernels and "pwpp_evid_landed<RECIP>(" in kernels and "pwpp_evid_finish(" in kernels
    assert "hipLaunchCooperativeKernel" not in kernels and "while (" not in kernels
    capi = open(os.path.join(PKG, "csrc", "pwpp_capi.cpp")).read()
    assert "pwpp_evid_verdict(R, cells, landed, occupied, free_cells)" in capi  # the host's verdict is the kernels' function


def G(**kw):
    return ctypes.byref(pwpp_hip.GroundGrid(**dict(dict(x0=-2.0, y0=-2.0, cell=1.0, nx=4, ny=4, flags=0, pad_=0), **kw)))


def M(**kw):
    return ctypes.byref(pwpp_hip.FusionMap(**dict(dict(x0=-3.0, y0=-3.0, cell=1.0, nx=6, ny=6, hit=40, miss=20, l_min=-350, l_max=350, occupied_at=100, free_at=-60), **kw)))


def R(gate=0, min_cells=1, moving_share=192, static_share=192):
    return ctypes.byref(pwpp_hip.EvidenceRule(gate, min_cells, moving_share, static_share))


def test_every_argument_is_named_before_the_device_is_touched_and_in_order(lib):
    label, occ, occ2, cls = np.zeros(16, np.int32), np.zeros(16, np.int8), np.zeros(16, np.int8), np.zeros(16, np.int8)
    maps = np.zeros(36, np.int16)
    rows = np.zeros(8, pwpp_hip.CLUSTER_EVIDENCE_DTYPE)
    pose = np.array([er.IDENTITY], np.float64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    at = lambda a, n: ctypes.c_void_p(a.ctypes.data + n)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    D = pwpp_hip.MEM_DEVICE
    err = lib.pwpp_last_error

    def grid(h=fake, g=G(), frames=1, mem=2, label=vp(label), occ_in=None, pose=vp(pose), n_poses=1, mof=None, m=M(), n_maps=1, maps=vp(maps), rule=R(), max_rows=8,
             rows=vp(rows), cls=None, occ_out=None):
        return lib.pwpp_evidence_grid(h, g, frames, mem, label, occ_in, pose, n_poses, mof, m, n_maps, maps, rule, max_rows, rows, cls, occ_out)

    ok = b"PWPP_MEM_HOST or"  # (mem = 2, PWPP_MEM_HOST_PINNED: every check before mem has passed)
    # 1 null pointers
    assert grid(h=None) == E_ARG and b"null handle" in err()
    for kw, text in ((dict(g=None), b"null grid"), (dict(label=None), b"null label image"), (dict(pose=None), b"null pose"), (dict(m=None), b"null map description"),
                     (dict(maps=None), b"null map"), (dict(rule=None), b"null rule"), (dict(rows=None), b"null rows")):
        assert grid(**kw) == E_ARG and text in err(), kw
    assert grid() == E_ARG and ok in err()
    assert grid(cls=vp(cls), occ_in=vp(occ), occ_out=vp(occ2)) == E_ARG and ok in err()
    # 2 sizes: the frame grid, then the map
    for kw in (dict(frames=0), dict(g=G(nx=0)), dict(g=G(ny=-1)), dict(n_maps=0), dict(m=M(nx=0))):
        assert grid(**kw) == E_ARG and b"cells" in err(), kw
    for kw in (dict(g=G(nx=32769)), dict(m=M(ny=32769))):
        assert grid(**kw) == E_ARG and b"32768 a side" in err(), kw
    assert grid(g=G(nx=32768, ny=32768), frames=3) == E_ARG and b"exceed 2^31" in err()
    assert grid(m=M(nx=32768, ny=32768), n_maps=3) == E_ARG and b"exceed 2^31" in err()
    # 3 flags; 4 origins and cells
    assert grid(g=G(flags=1)) == E_ARG and b"grid flags 1" in err()
    for kw in (dict(g=G(cell=0.0)), dict(g=G(x0=NAN)), dict(g=G(y0=INF)), dict(g=G(cell=NAN))):
        assert grid(**kw) == E_ARG and b"grid origin and cell size must be finite" in err(), kw
    for kw in (dict(m=M(cell=0.0)), dict(m=M(cell=-1.0)), dict(m=M(x0=NAN)), dict(m=M(y0=-INF)), dict(m=M(cell=INF))):
        assert grid(**kw) == E_ARG and b"map origin and cell size must be finite" in err(), kw
    # 5 the thresholds
    for kw in (dict(free_at=100, occupied_at=100), dict(free_at=5, occupied_at=4), dict(free_at=-32769), dict(occupied_at=32768)):
        assert grid(m=M(**kw)) == E_ARG and b"thresholds free_at" in err(), kw
    assert grid(m=M(free_at=-32768, occupied_at=32767)) == E_ARG and ok in err()
    # 6 the rule
    for v in (-1, 5):
        assert grid(rule=R(gate=v)) == E_ARG and b"gate %d: 0 .. 4" % v in err()
    for v in (0, 4):
        assert grid(rule=R(gate=v)) == E_ARG and ok in err()
    for v in (0, -3):
        assert grid(rule=R(min_cells=v)) == E_ARG and b"min_cells %d: at least 1" % v in err()
    for v in (0, 257, -1):
        assert grid(rule=R(moving_share=v)) == E_ARG and b"moving_share %d: 1 .. 256" % v in err()
        assert grid(rule=R(static_share=v)) == E_ARG and b"static_share %d: 1 .. 256" % v in err()
    assert grid(rule=R(min_cells=2 ** 31 - 1, moving_share=1, static_share=256)) == E_ARG and ok in err()
    # 7 the rows, exactly at and one past 2^24
    assert grid(max_rows=0) == E_ARG and b"max_rows 0: at least 1" in err()
    big = np.zeros(3 * 16, np.int32)
    assert grid(frames=3, label=vp(big), max_rows=2 ** 24 // 3 + 1) == E_ARG and b"3 frames x max_rows 5592406 exceed 2^24" in err()
    room = np.zeros(2 ** 24, pwpp_hip.CLUSTER_EVIDENCE_DTYPE)  # (never touched: untouched pages cost nothing)
    assert grid(max_rows=2 ** 24, rows=vp(room)) == E_ARG and ok in err()
    # 8 the poses; 9 map_of_frame
    for n, frames in ((0, 1), (2, 1), (2, 3), (-1, 1)):
        assert grid(n_poses=n, frames=frames, label=vp(big), max_rows=2) == E_ARG and b"%d poses for %d frames" % (n, frames) in err()
    bad = np.array([[NAN, 0, INF, 0, 1, 0]], np.float64)
    assert grid(pose=vp(bad)) == E_ARG and ok in err()  # a pose that is not finite is no error: its frame lands nothing
    maps3 = np.zeros(3 * 36, np.int16)
    assert grid(frames=3, label=vp(big), max_rows=2, n_maps=2, maps=vp(maps3)) == E_ARG and b"null map_of_frame with 2 maps for 3 frames" in err()
    assert grid(frames=3, label=vp(big), max_rows=2, n_maps=3, maps=vp(maps3)) == E_ARG and ok in err()
    for entry in (-2, 2):
        mof = np.array([0, entry, 1], np.int32)
        assert grid(frames=3, label=vp(big), max_rows=2, n_maps=2, maps=vp(maps3), mof=vp(mof)) == E_ARG and b"map_of_frame 1 names map %d" % entry in err()
    mof = np.array([0, -1, 1], np.int32)
    assert grid(frames=3, label=vp(big), max_rows=2, n_maps=2, maps=vp(maps3), mof=vp(mof)) == E_ARG and ok in err()
    # 10 the occupancy pair: both or neither
    assert grid(occ_in=vp(occ)) == E_ARG and b"null occupancy_out with occupancy_in given" in err()
    assert grid(occ_out=vp(occ)) == E_ARG and b"null occupancy_in with occupancy_out given" in err()
    # 11 the overlaps: only the pair may be one array
    assert grid(occ_in=vp(occ), occ_out=vp(occ)) == E_ARG and ok in err()
    assert grid(occ_in=vp(occ), occ_out=at(occ, 1)) == E_ARG and b"occupancy_in and occupancy_out overlap without being equal" in err()
    assert grid(cls=vp(occ), occ_in=vp(occ), occ_out=vp(occ2)) == E_ARG and b"occupancy_in and cell_class overlap" in err()
    assert grid(cls=vp(occ2), occ_in=vp(occ), occ_out=vp(occ2)) == E_ARG and b"cell_class and occupancy_out overlap" in err()
    assert grid(rows=at(label, 0)) == E_ARG and b"label and rows overlap" in err()
    assert grid(maps=at(label, 4)) == E_ARG and b"label and map overlap" in err()
    assert grid(cls=at(rows, 250)) == E_ARG and b"rows and cell_class overlap" in err()
    both = np.zeros(64, np.int8)
    assert grid(occ_in=vp(both), occ_out=at(both, 16)) == E_ARG and ok in err()  # touching ranges do not overlap
    # 12 mem; 13 device alignment: rows 8, label 4, map 2, bytes 1
    assert grid(mem=7) == E_ARG and b"mem 7" in err()
    wide = np.zeros(64, np.int64)
    assert grid(mem=D, rows=at(wide, 4)) == E_ARG and b"the rows must be 8-byte aligned" in err()
    assert grid(mem=D, label=at(wide, 2)) == E_ARG and b"the label image must be 4-byte aligned" in err()
    assert grid(mem=D, maps=at(wide, 257)) == E_ARG and b"the map must be 2-byte aligned" in err()
    # the order
    assert grid(label=None, frames=0) == E_ARG and b"null label image" in err()
    assert grid(frames=0, m=M(nx=0)) == E_ARG and b"0 frames of 4 x 4" in err()
    assert grid(m=M(nx=0), g=G(flags=1)) == E_ARG and b"1 frames of 0 x 6" in err()
    assert grid(g=G(flags=1, cell=0.0)) == E_ARG and b"grid flags 1" in err()
    assert grid(g=G(cell=0.0), m=M(cell=0.0)) == E_ARG and b"grid origin" in err()
    assert grid(m=M(cell=0.0, free_at=200)) == E_ARG and b"map origin" in err()
    assert grid(m=M(free_at=200), rule=R(gate=9)) == E_ARG and b"thresholds" in err()
    assert grid(rule=R(gate=9, min_cells=0)) == E_ARG and b"gate 9" in err()
    assert grid(rule=R(min_cells=0, moving_share=0)) == E_ARG and b"min_cells 0" in err()
    assert grid(rule=R(moving_share=0, static_share=0)) == E_ARG and b"moving_share 0" in err()
    assert grid(rule=R(static_share=0), max_rows=0) == E_ARG and b"static_share 0" in err()
    assert grid(max_rows=0, n_poses=0) == E_ARG and b"max_rows 0" in err()
    assert grid(max_rows=2 ** 24 + 1, n_poses=0) == E_ARG and b"max_rows 16777217 exceed" in err()
    assert grid(n_poses=0, n_maps=2, maps=vp(maps3)) == E_ARG and b"0 poses" in err()
    assert grid(n_maps=2, maps=vp(maps3), occ_in=vp(occ)) == E_ARG and b"null map_of_frame" in err()
    assert grid(occ_in=vp(occ), rows=at(label, 0)) == E_ARG and b"null occupancy_out" in err()
    assert grid(rows=at(label, 0), mem=7) == E_ARG and b"overlap" in err()
    assert grid(mem=7, label=at(wide, 2)) == E_ARG and b"mem 7" in err()

    # pwpp_evidence_obstacles: the nulls, then what pwpp_label_obstacles rejects -- up to its look at the handle (mem comes just before it)
    table, n = np.zeros(8, pwpp_hip.OBSTACLE_CLUSTER_DTYPE), np.zeros(1, np.int32)

    def obstacles(h=fake, gr=G(), h_min=0.2, h_max=2.0, min_count=1, connectivity=8, frames=1, mem=2, label=vp(label), table=vp(table), max_clusters=8, pose=vp(pose),
                  n_poses=1, m=M(), maps=vp(maps), rule=R(), rows=vp(rows)):
        return lib.pwpp_evidence_obstacles(h, gr, h_min, h_max, min_count, connectivity, 0, frames, mem, label, None, None, table, vp(n), max_clusters, None, None, pose,
                                           n_poses, None, m, 1, maps, rule, rows, None, None)

    assert obstacles(h=None) == E_ARG and b"null handle" in err()
    for kw, text in ((dict(gr=None), b"null grid"), (dict(label=None), b"null label image"), (dict(pose=None), b"null pose"), (dict(m=None), b"null map description"),
                     (dict(maps=None), b"null map"), (dict(rule=None), b"null rule"), (dict(rows=None), b"null rows")):
        assert obstacles(**kw) == E_ARG and text in err(), kw
    assert obstacles() == E_ARG and ok in err()
    assert obstacles(gr=G(flags=2)) == E_ARG and b"grid flags 2" in err()
    assert obstacles(h_min=2.0, h_max=1.0) == E_ARG and b"height band" in err()
    assert obstacles(min_count=0) == E_ARG and b"min_count 0" in err()
    assert obstacles(connectivity=6) == E_ARG and b"connectivity 6" in err()
    assert obstacles(max_clusters=-1) == E_ARG and b"max_clusters -1" in err()
    assert obstacles(table=None) == E_ARG and b"null cluster table" in err()
    assert obstacles(gr=G(cell=0.0), rule=R(gate=9)) == E_ARG and b"cell size" in err()
    assert obstacles(rule=R(gate=9)) == E_ARG and ok in err()  # the evidence's own checks come after the labelling's, which end at the handle


# ---- the host's verdict -----------------------------------------------------------------------------------------------------
def test_the_verdict_at_exact_ratio_boundaries(lib):
    V = pwpp_hip.evidence_verdict
    for share in (1, 3, 64, 100, 192, 255, 256):
        for landed in (1, 3, 4, 7, 256, 1000, 2 ** 30):
            r = er.rule(0, 1, share, share)
            at = -(-share * landed // 256)  # the smallest count with count * 256 >= share * landed
            assert at * 256 >= share * landed > (at - 1) * 256
            # moving: exactly at the boundary and one below
            assert V((0, 1, share, 256), landed, landed, 0, at) == er.MOVING == er.evidence_verdict(er.rule(0, 1, share, 256), landed, landed, 0, at)
            assert V((0, 1, share, 256), landed, landed, 0, at - 1) == er.UNDECIDED == er.evidence_verdict(er.rule(0, 1, share, 256), landed, landed, 0, at - 1)
            # static alike, with no free cell
            assert V((0, 1, 256, share), landed, landed, at, 0) == er.STATIC == er.evidence_verdict(er.rule(0, 1, 256, share), landed, landed, at, 0)
            assert V((0, 1, 256, share), landed, landed, at - 1, 0) == er.UNDECIDED == er.evidence_verdict(er.rule(0, 1, 256, share), landed, landed, at - 1, 0)
            assert er.evidence_verdict(r, landed, landed, 0, at) == er.MOVING
    # 3 of 4 is exactly 192 / 256; 191 of 255 is one below 192 * 255 / 256 rounded up
    assert V((0, 1, 192, 192), 4, 4, 0, 3) == er.MOVING and V((0, 1, 192, 192), 4, 4, 3, 0) == er.STATIC
    assert V((0, 1, 192, 192), 255, 255, 0, 192) == er.MOVING and V((0, 1, 192, 192), 255, 255, 0, 191) == er.UNDECIDED
    # landed == min_cells and one below
    assert V((0, 5, 1, 1), 9, 5, 0, 5) == er.MOVING and V((0, 5, 1, 1), 9, 4, 0, 4) == er.UNDECIDED
    assert V((0, 5, 1, 1), 9, 5, 5, 0) == er.STATIC and V((0, 5, 1, 1), 9, 4, 4, 0) == er.UNDECIDED
    # both conditions true at once: moving is asked first
    assert V((0, 1, 128, 128), 2, 2, 1, 1) == er.MOVING == er.evidence_verdict(er.rule(0, 1, 128, 128), 2, 2, 1, 1)
    # no cells: none, whatever the rule; cells that did not land: undecided
    assert V((4, 1, 1, 1), 0, 0, 0, 0) == er.NONE and V((0, 1, 1, 1), 7, 0, 0, 0) == er.UNDECIDED
    rng = np.random.default_rng(5)
    for _ in range(2000):
        cells = int(rng.integers(0, 50))
        landed = int(rng.integers(0, cells + 1))
        occupied = int(rng.integers(0, landed + 1))
        free = int(rng.integers(0, landed - occupied + 1))
        r = (int(rng.integers(0, 5)), int(rng.integers(1, 6)), int(rng.integers(1, 257)), int(rng.integers(1, 257)))
        assert V(r, cells, landed, occupied, free) == er.evidence_verdict(er.rule(*r), cells, landed, occupied, free)
    # the host function names what it refuses
    out = ctypes.c_int32(9)
    assert lib.pwpp_evidence_verdict(None, 1, 1, 0, 0, ctypes.byref(out)) == E_ARG and b"null rule" in lib.pwpp_last_error()
    assert lib.pwpp_evidence_verdict(R(), 1, 1, 0, 0, None) == E_ARG and b"null verdict" in lib.pwpp_last_error()
    assert lib.pwpp_evidence_verdict(R(gate=5), 1, 1, 0, 0, ctypes.byref(out)) == E_ARG and b"gate 5" in lib.pwpp_last_error()
    for counts in ((1, 2, 0, 0), (4, 3, 2, 2), (-1, 0, 0, 0), (3, 3, -1, 0)):
        assert lib.pwpp_evidence_verdict(R(), *counts, ctypes.byref(out)) == E_ARG and b"counts cells" in lib.pwpp_last_error(), counts
    assert out.value == 9


# ---- the mirror and the header --------------------------------------------------------------------------------------------------
CPP = r"""
#include <patchwork/patchworkpp.h>
long use(patchwork::PatchWorkpp &s, const patchwork::PatchWorkpp::FusedObstacleMap &map, const int8_t *occupancy) {
    patchwork::PatchWorkpp::EvidenceRule rule;
    rule.gate = 2, rule.min_cells = 4;
    const double pose[6] = {1.0, 0.0, 0.5, 0.0, 1.0, -0.5};
    const patchwork::PatchWorkpp::ObstacleEvidence a = s.getObstacleEvidence(map, -10.0, -10.0, 0.5, 40, 40, 0.3f, 2.5f);
    const patchwork::PatchWorkpp::ObstacleEvidence b = s.getObstacleEvidence(map, -10.0, -10.0, 0.5, 40, 40, 0.3f, 2.5f, pose, rule, occupancy, 1, 8, 64);
    long moving = 0;
    for (const pwpp_cluster_evidence &r : b.rows) moving += r.verdict == PWPP_EVID_MOVING;
    return moving + (long)a.rows.size() + (long)a.clusters.size() + (long)b.masked.size() + (long)b.cell_class.size() + a.count + b.nx + b.ny + (long)b.label.size();
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_method_compiles(tmp_path, flavour):
    src = tmp_path / "evidence.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    cmd += ["-DPWPP_NO_EIGEN"] if flavour == "plain" else ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "evidence.c"
    src.write_text('#include "pwpp.h"\nint f(pwpp_cluster_evidence *e, const pwpp_ground_grid *g, const pwpp_fusion_map *m, const pwpp_evidence_rule *r, int32_t *v) {\n'
                   '    return pwpp_evidence_grid(0, g, 1, PWPP_MEM_HOST, 0, 0, 0, 1, 0, m, 1, 0, r, PWPP_EVID_LDS_ROWS + 1, e, 0, 0) +\n'
                   '           pwpp_evidence_obstacles(0, g, 0.f, 1.f, 1, 8, 0, 1, PWPP_MEM_HOST, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, m, 1, 0, r, e, 0, 0) +\n'
                   '           pwpp_evidence_verdict(r, 1, 1, 0, 1, v) + (int)sizeof(*e) + PWPP_HAS_MAP_EVIDENCE + PWPP_EVID_MOVING + PWPP_EVID_CELL_NONE + (int)e->free;\n}\n'
                   'typedef char size_is_32[sizeof(pwpp_cluster_evidence) == 32 ? 1 : -1];\ntypedef char rule_is_16[sizeof(pwpp_evidence_rule) == 16 ? 1 : -1];\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# ---- the kernels' functions on the host ----------------------------------------------------------------------------------------
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
    tmp = tmp_path_factory.mktemp("evidence_check")
    exe = tmp / "evidence_check"
    flags = SANITIZE if sanitizers_work(tmp) else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off"] + flags +
                   ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "evidence_check.cpp"), "-o", str(exe)], check=True)
    return exe


def test_evidence_program_builds_and_passes(checker):
    r = subprocess.run([str(checker)], capture_output=True, text=True)  # (a stand-alone child process with its own main)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
    assert int(r.stdout.split("evidence_check: ")[1].split(" cases")[0]) >= 2000


def yaw(degrees, tx=0.0, ty=0.0):
    return fr.rigid(np.deg2rad(degrees), tx, ty)


def blobs(frames, ny, nx, seed, rows):
    """Label images of a few rectangles with labels 0 .. rows - 1 on a ground of -1."""
    rng = np.random.default_rng(seed)
    out = np.full((frames, ny, nx), -1, np.int32)
    for f in range(frames):
        for r in range(rows):
            y, x = int(rng.integers(0, ny)), int(rng.integers(0, nx))
            out[f, y:y + int(rng.integers(1, 7)), x:x + int(rng.integers(1, 7))] = r
    return out


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("case", ["yaw", "shift", "thresholds", "per_frame"])
def test_the_restatement_and_the_one_text_agree_byte_for_byte(checker, tmp_path, case, path):
    """The kernels' functions, dealt wave by wave on the host on both paths, against the dictionaries: what the GPU tests compare,
    without a GPU."""
    frames, rows = 3, 8
    g = er.grid(-8.0, -7.0, 0.5, 37, 29)
    m = er.fusion_map(-9.0, -8.0, 1.0 if case == "yaw" else 0.3, 21 if case == "yaw" else 70, 19 if case == "yaw" else 55, 100, -60)
    label = blobs(frames, g["ny"], g["nx"], 11, rows)
    label[0, 0, 0], label[1, 2, 2], label[2, 3, 3], label[0, 5, 5] = rows, 2 ** 31 - 1, -2 ** 31, rows - 1
    poses = {"yaw": [yaw(30, 0.4, -0.3)], "shift": [(1.0, 0.0, 1.5, 0.0, 1.0, -1.0)], "thresholds": [er.IDENTITY],
             "per_frame": [yaw(90), (NAN, 0.0, 0.0, 0.0, 1.0, 0.0), yaw(200, 1.0, 2.0)]}[case]
    gate = {"yaw": 2, "shift": 4, "thresholds": 0, "per_frame": 1}[case]
    n_maps = {"yaw": 1, "shift": 3, "thresholds": 2, "per_frame": 2}[case]
    mof = {"yaw": None, "shift": None, "thresholds": [1, -1, 0], "per_frame": [0, 1, 1]}[case]
    rng = np.random.default_rng(3)
    if case == "thresholds":
        maps = rng.choice(np.array([100, 99, -60, -59, -32768, 32767], np.int16), size=(n_maps, m["ny"], m["nx"]))
    else:
        maps = rng.integers(-300, 300, size=(n_maps, m["ny"], m["nx"])).astype(np.int16)
    occ = fr.random_occupancy(frames, g["ny"], g["nx"], 9) if case != "yaw" else None
    r = er.rule(gate, 3, 100, 60)
    want_rows, want_class, want_occ = er.evidence_grid(g, label, occ, poses, mof, m, maps, r, rows)
    assert want_rows["landed"].sum() > 20
    label.tofile(tmp_path / "label.i32")
    maps.tofile(tmp_path / "maps.i16")
    np.asarray(poses, np.float64).tofile(tmp_path / "poses.f64")
    if occ is not None:
        occ.tofile(tmp_path / "occ.i8")
    if mof is not None:
        np.asarray(mof, np.int32).tofile(tmp_path / "mof.i32")
    args = ["dump", str(tmp_path / "label.i32"), str(tmp_path / "occ.i8") if occ is not None else "-", str(tmp_path / "poses.f64"), str(len(poses)), str(frames),
            str(tmp_path / "mof.i32") if mof is not None else "-"]
    args += [repr(g[k]) for k in ("x0", "y0", "cell", "nx", "ny")] + [repr(m[k]) for k in ("x0", "y0", "cell", "nx", "ny", "occupied_at", "free_at")]
    args += [str(n_maps), str(tmp_path / "maps.i16")] + [str(r[k]) for k in ("gate", "min_cells", "moving_share", "static_share")] + [str(rows), str(path), str(tmp_path / "out")]
    subprocess.run([str(checker)] + args, check=True)
    assert np.fromfile(str(tmp_path / "out.rows"), er.EVIDENCE).tobytes() == want_rows.tobytes()
    assert np.fromfile(str(tmp_path / "out.class"), np.int8).tobytes() == want_class.tobytes()
    if occ is not None:
        assert np.fromfile(str(tmp_path / "out.occ"), np.int8).tobytes() == want_occ.tobytes()
    if case == "per_frame":
        assert want_rows["landed"][1].sum() == 0 and want_rows["cells"][1].sum() > 0  # the NaN pose lands nothing, the cells are still counted
    if case == "thresholds":
        assert want_rows["landed"][1].sum() == 0 and (want_class[1] == er.CELL_NONE).all()  # the skipped frame
        assert {int(v) for v in np.unique(want_class[0])} == {er.CELL_NONE, er.OCC_FREE, er.OCC_OCCUPIED, er.OCC_UNKNOWN}


# ---- the scenario: a wall, and a blob that moves through free space -----------------------------------------------------------------
def test_a_wall_is_static_a_mover_is_moving_and_the_masked_bytes_leave_no_trail():
    """A 48 x 48 map and frame grid of equal cells under the identity pose; hit 40, miss 20, clamps +-350, occupied_at 100,
    free_at -60.  A wall along row 40 and a 3 x 3 blob that moves 3 cells a scan along rows 10 .. 12 through cells otherwise
    observed free.  Six scans are fused; the seventh is classified at gate 0 and gate 1 with min_cells 3 and shares 192 / 192."""
    N, par = 48, (40, 20, -350, 350, 100, -60)
    grid, mgrid = (-24.0, -24.0, 1.0), (-24.0, -24.0, 1.0, N, N)

    def scan(k):
        occ = np.full((1, N, N), fr.FREE, np.int8)
        occ[0, 40, :] = fr.OCCUPIED
        occ[0, 10:13, 3 * k:3 * k + 3] = fr.OCCUPIED
        return occ

    fused = None
    for k in range(6):
        fused, _ = fr.fuse(scan(k), grid, [fr.IDENTITY], mgrid, par, map_in=fused)
    # the numbers worked out by hand: the wall, the blob's next cells, the blob's previous position
    assert (fused[0, 40, :] == 240).all() and (fused[0, 10:13, 18:21] == -120).all() and (fused[0, 10:13, 15:18] == -60).all()
    seventh = scan(6)
    label = np.full((1, N, N), -1, np.int32)
    label[0, 40, :] = 0
    label[0, 10:13, 18:21] = 1
    g, m = er.grid(*grid, N, N), er.fusion_map(*mgrid, par[4], par[5])
    for gate in (0, 1):
        rows, classes, masked = er.evidence_grid(g, label, seventh, [er.IDENTITY], None, m, fused, er.rule(gate, 3, 192, 192), 4)
        assert tuple(rows[0, 0])[1:] == (48, 48, 48, 0, 0, er.STATIC) and rows[0, 0]["sum"] == 48 * 240
        assert tuple(rows[0, 1])[1:] == (9, 9, 0, 9, 0, er.MOVING) and rows[0, 1]["sum"] == (9 * -120 if gate == 0 else 3 * -60 + 6 * -120)
        assert rows[0, 2]["verdict"] == er.NONE and rows[0, 3]["verdict"] == er.NONE
        assert (classes[0, 40, :] == er.OCC_OCCUPIED).all() and (classes[0, 10:13, 18:21] == er.OCC_FREE).all() and (classes == er.CELL_NONE).sum() == N * N - 57
        assert (masked[0, 10:13, 18:21] == er.OCC_UNKNOWN).all() and (masked[0, 40, :] == fr.OCCUPIED).all()
        assert (masked != seventh).sum() == 9
        with_mask, _ = fr.fuse(masked, grid, [fr.IDENTITY], mgrid, par, map_in=fused)
        without, _ = fr.fuse(seventh, grid, [fr.IDENTITY], mgrid, par, map_in=fused)
        assert (with_mask[0, 10:13, 18:21] == fused[0, 10:13, 18:21]).all()  # the mover is not observed at all
        assert (without[0, 10:13, 18:21] == -80).all()  # unmasked it is fused cell by cell
        assert (with_mask[0, 40, :] == 280).all() and (with_mask[0, 10:13, 15:18] == -80).all()  # the wall and the free cells are observed as before
