"""No-GPU checks of the cluster tracks (pwpp_associate_grid, pwpp_track_obstacles): the exports, the feature macro and its place,
the size of pwpp_cluster_link, the ctypes prototypes and the bindings' methods; every argument check of pwpp_associate_grid with
its message and its place in the order, and those of pwpp_track_obstacles that come before it looks at its handle; the C++ mirror
in both flavours and the header as C99; properties of the restatement the GPU tests compare against (tests/tracks_ref.py); and the
stand-alone program that runs the kernels' functions on the host against a brute force of its own (tools/tracks_check.cpp), built
with the address and undefined-behaviour sanitizers where the toolchain has them, whose dump is compared with the restatement."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pwpp_hip
import tracks_ref as tr

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
    for name in ("pwpp_associate_grid", "pwpp_track_obstacles"):
        assert hasattr(lib, name), name
        assert "PWPP_API int %s(" % name in hdr
    assert "#define PWPP_HAS_CLUSTER_TRACKS 1" in hdr and "typedef struct pwpp_cluster_link {" in hdr
    assert "#define PWPP_VERSION_MINOR 4 " in hdr
    # declared directly after pwpp_grid_cell_of and before the input transforms
    assert hdr.index("PWPP_API int pwpp_grid_cell_of(") < hdr.index("PWPP_HAS_CLUSTER_TRACKS") < hdr.index("PWPP_API int pwpp_associate_grid(")
    assert hdr.index("PWPP_API int pwpp_associate_grid(") < hdr.index("PWPP_API int pwpp_track_obstacles(") < hdr.index("#define PWPP_HAS_INPUT_TRANSFORM")
    between = hdr[hdr.index("PWPP_API int pwpp_grid_cell_of("):hdr.index("#define PWPP_HAS_CLUSTER_TRACKS")]
    assert "PWPP_API" not in between[10:] and "#define" not in between
    assert "2 * max_pairs slots cannot fill before the count of" in " ".join(between.split())  # the table-size bound is stated
    assert ctypes.sizeof(pwpp_hip.ClusterLink) == 16 and pwpp_hip.CLUSTER_LINK_DTYPE.itemsize == 16 and tr.LINK == pwpp_hip.CLUSTER_LINK_DTYPE
    assert [f[0] for f in pwpp_hip.ClusterLink._fields_] == ["other", "overlap", "cells", "links"]
    assert all(f[1] is ctypes.c_int32 for f in pwpp_hip.ClusterLink._fields_)
    assert len(lib.pwpp_associate_grid.argtypes) == 20 and len(lib.pwpp_track_obstacles.argtypes) == 29
    for name in ("associate_grid", "associate_grid_device", "track_obstacles", "track_obstacles_device"):
        assert callable(getattr(pwpp_hip.Handle, name)), name
    import pypatchworkpp
    assert hasattr(pypatchworkpp.patchworkpp, "trackObstacleClusters") and hasattr(pypatchworkpp.patchworkpp, "resetObstacleTracks")
    doc = pypatchworkpp.patchworkpp.trackObstacleClusters.__doc__
    assert "pose:" in doc and "= [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]" in doc and "max_clusters:" in doc and "gate:" in doc and "min_overlap:" in doc
    src = open(os.path.join(PKG, "csrc", "pwpp_tracks.h")).read()
    for name in ("pwpp_tracks_vote", "pwpp_tracks_gate_key", "pwpp_tracks_pack", "pwpp_tracks_continues", "pwpp_tracks_fresh_id", "pwpp_tracks_slots"):
        assert "PWPP_HD inline" in src and name + "(" in src, name
    assert "pwpp_fuse_cell_of<RECIP>(" in src and "pwpp_elev_position(" in src and "floor" not in src  # the geometry is called, not restated
    kernels = open(os.path.join(PKG, "csrc", "pwpp_tracks.hip")).read()
    assert '#include "pwpp_tracks.h"' in kernels and "pwpp_tracks_vote<RECIP>(" in kernels and "pwpp_tracks_pack(" in kernels


def G(**kw):
    return ctypes.byref(pwpp_hip.GroundGrid(**dict(dict(x0=-2.0, y0=-2.0, cell=1.0, nx=4, ny=4, flags=0, pad_=0), **kw)))


def test_every_argument_is_named_before_the_device_is_touched_and_in_order(lib):
    curr, prev = np.zeros(16, np.int32), np.zeros(16, np.int32)
    cl, pl = np.zeros(8, pwpp_hip.CLUSTER_LINK_DTYPE), np.zeros(8, pwpp_hip.CLUSTER_LINK_DTYPE)
    n_pairs, id_prev, next_id, id_curr, next_out = (np.zeros(8, np.int32) for _ in range(5))
    pose = np.array([tr.IDENTITY], np.float64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    at = lambda a, n: ctypes.c_void_p(a.ctypes.data + n)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    D = pwpp_hip.MEM_DEVICE
    err = lib.pwpp_last_error

    def grid(h=fake, gc=G(), gp=G(), frames=1, mem=2, curr=vp(curr), prev=vp(prev), pose=vp(pose), n_poses=1, gate=0, min_overlap=1, max_rows=8, max_pairs=8,
             cl=vp(cl), pl=vp(pl), n_pairs=vp(n_pairs), id_prev=None, next_id=None, id_curr=None, next_out=None):
        return lib.pwpp_associate_grid(h, gc, gp, frames, mem, curr, prev, pose, n_poses, gate, min_overlap, max_rows, max_pairs, cl, pl, n_pairs, id_prev, next_id,
                                       id_curr, next_out)

    ids = dict(id_prev=vp(id_prev), next_id=vp(next_id), id_curr=vp(id_curr), next_out=vp(next_out))
    ok = b"PWPP_MEM_HOST or"  # (mem = 2, PWPP_MEM_HOST_PINNED: every check before mem has passed)
    # 1 null pointers
    assert grid(h=None) == E_ARG and b"null handle" in err()
    for kw, text in ((dict(gc=None), b"null current grid"), (dict(gp=None), b"null previous grid"), (dict(curr=None), b"null current image"),
                     (dict(prev=None), b"null previous image"), (dict(pose=None), b"null pose"), (dict(cl=None), b"null curr_links"), (dict(pl=None), b"null prev_links")):
        assert grid(**kw) == E_ARG and text in err(), kw
    assert grid(n_pairs=None) == E_ARG and ok in err()  # n_pairs may be absent
    assert grid() == E_ARG and ok in err() and grid(**ids) == E_ARG and ok in err()
    # 2 sides and frames, as the fusion checks them: the current grid first
    for kw in (dict(frames=0), dict(gc=G(nx=0)), dict(gp=G(ny=-1))):
        assert grid(**kw) == E_ARG and b"cells" in err(), kw
    for kw in (dict(gc=G(nx=32769)), dict(gp=G(ny=32769))):
        assert grid(**kw) == E_ARG and b"32768 a side" in err(), kw
    assert grid(gc=G(nx=32768, ny=32768), frames=3) == E_ARG and b"exceed 2^31" in err()
    assert grid(gp=G(nx=32768, ny=32768), frames=3) == E_ARG and b"exceed 2^31" in err()
    # 3 flags, origins and cell sizes
    assert grid(gc=G(flags=1)) == E_ARG and b"grid flags 1 of the current grid" in err()
    assert grid(gp=G(flags=4)) == E_ARG and b"grid flags 4 of the previous grid" in err()
    for kw in (dict(gc=G(cell=0.0)), dict(gp=G(cell=-1.0)), dict(gc=G(x0=NAN)), dict(gp=G(y0=INF)), dict(gp=G(cell=NAN))):
        assert grid(**kw) == E_ARG and b"finite" in err(), kw
    # 4 gate and min_overlap
    for v in (-1, 5):
        assert grid(gate=v) == E_ARG and b"gate %d: 0 .. 4" % v in err()
    for v in (0, 4):
        assert grid(gate=v) == E_ARG and ok in err()
    for v in (0, -3):
        assert grid(min_overlap=v) == E_ARG and b"min_overlap %d: at least 1" % v in err()
    assert grid(min_overlap=2 ** 31 - 1) == E_ARG and ok in err()
    # 5 the rows and the pairs, exactly at and one past 2^24
    assert grid(max_rows=0) == E_ARG and b"max_rows 0: at least 1" in err()
    assert grid(max_pairs=0) == E_ARG and b"max_pairs 0: at least 1" in err()
    big = np.zeros(3 * 16, np.int32)
    assert grid(frames=3, curr=vp(big), prev=vp(big), max_rows=2 ** 24 // 3 + 1) == E_ARG and b"3 frames x max_rows 5592406 exceed 2^24" in err()
    assert grid(frames=3, curr=vp(big), prev=vp(big), max_pairs=2 ** 24 // 3 + 1) == E_ARG and b"3 frames x max_pairs 5592406 exceed 2^24" in err()
    assert grid(max_rows=2 ** 24 + 1) == E_ARG and b"exceed 2^24" in err()
    room = np.zeros(2 ** 24, pwpp_hip.CLUSTER_LINK_DTYPE), np.zeros(2 ** 24, pwpp_hip.CLUSTER_LINK_DTYPE)  # (never touched: untouched pages cost nothing)
    assert grid(max_rows=2 ** 24, max_pairs=2 ** 24, cl=vp(room[0]), pl=vp(room[1])) == E_ARG and ok in err()
    # 6 the poses
    for n, frames in ((0, 1), (2, 1), (2, 3), (-1, 1)):
        assert grid(n_poses=n, frames=frames, curr=vp(big), prev=vp(big), max_rows=2, max_pairs=2) == E_ARG and b"%d poses for %d frames" % (n, frames) in err()
    bad = np.array([[NAN, 0, INF, 0, 1, 0]], np.float64)
    assert grid(pose=vp(bad)) == E_ARG and ok in err()  # a pose that is not finite is no error: its frame has no votes
    # 7 the id set: all four or none
    for missing in ids:
        some = dict(ids)
        some[missing] = None
        name = {"next_out": "next_id_out"}.get(missing, missing).encode()
        assert grid(**some) == E_ARG and b"null " + name + b" with other id arrays given" in err(), missing
    assert grid(id_curr=vp(id_curr)) == E_ARG and b"null id_prev" in err()
    # 8 the overlaps
    assert grid(curr=vp(prev)) == E_ARG and b"curr and prev overlap" in err()
    assert grid(cl=vp(pl)) == E_ARG and b"curr_links and prev_links overlap" in err()
    assert grid(n_pairs=at(cl, 124)) == E_ARG and b"curr_links and n_pairs overlap" in err()
    assert grid(**dict(ids, id_curr=vp(id_prev))) == E_ARG and b"id_prev and id_curr overlap" in err()
    assert grid(**dict(ids, next_out=vp(next_id))) == E_ARG and b"next_id and next_id_out overlap" in err()
    assert grid(**dict(ids, id_prev=at(curr, 60))) == E_ARG and b"curr and id_prev overlap" in err()
    both = np.zeros(64, np.int32)
    assert grid(curr=vp(both), prev=at(both, 64)) == E_ARG and ok in err()  # touching ranges do not overlap
    # 9 mem; 10 device alignment
    assert grid(mem=7) == E_ARG and b"mem 7" in err()
    for kw, text in ((dict(curr=at(both, 2)), b"curr image"), (dict(prev=at(both, 129)), b"prev image"), (dict(cl=at(cl, 2)), b"curr_links"), (dict(pl=at(pl, 1)), b"prev_links"),
                     (dict(n_pairs=at(n_pairs, 3)), b"n_pairs"), (dict(ids, id_prev=at(both, 2)), b"id_prev"), (dict(ids, next_id=at(both, 1)), b"next_id"),
                     (dict(ids, id_curr=at(both, 6)), b"id_curr"), (dict(ids, next_out=at(both, 7)), b"next_id_out")):
        assert grid(mem=D, **kw) == E_ARG and b"the " + text + b" must be 4-byte aligned" in err(), kw
    # the order
    assert grid(curr=None, frames=0) == E_ARG and b"null current image" in err()
    assert grid(frames=0, gc=G(flags=1)) == E_ARG and b"0 frames of 4 x 4" in err()
    assert grid(gc=G(nx=32769), gp=G(nx=0)) == E_ARG and b"32768 a side" in err()
    assert grid(gp=G(nx=32769), gc=G(flags=1)) == E_ARG and b"32768 a side" in err()
    assert grid(gc=G(flags=1, cell=0.0)) == E_ARG and b"grid flags 1" in err()
    assert grid(gp=G(flags=1), gc=G(cell=0.0)) == E_ARG and b"grid flags 1 of the previous" in err()
    assert grid(gc=G(cell=0.0), gate=9) == E_ARG and b"finite" in err()
    assert grid(gate=9, min_overlap=0) == E_ARG and b"gate 9" in err()
    assert grid(min_overlap=0, max_rows=0) == E_ARG and b"min_overlap 0" in err()
    assert grid(max_rows=0, max_pairs=0) == E_ARG and b"max_rows 0" in err()
    assert grid(max_rows=2 ** 24 + 1, max_pairs=0) == E_ARG and b"max_rows 16777217 exceed" in err()
    assert grid(max_pairs=0, n_poses=0) == E_ARG and b"max_pairs 0" in err()
    assert grid(max_pairs=2 ** 24 + 1, n_poses=0) == E_ARG and b"max_pairs 16777217 exceed" in err()
    assert grid(n_poses=0, id_curr=vp(id_curr)) == E_ARG and b"0 poses" in err()
    assert grid(id_curr=vp(id_curr), curr=vp(prev)) == E_ARG and b"null id_prev" in err()
    assert grid(curr=vp(prev), mem=7) == E_ARG and b"overlap" in err()
    assert grid(mem=7, curr=at(both, 2)) == E_ARG and b"mem 7" in err()

    # pwpp_track_obstacles: the nulls, then what pwpp_label_obstacles rejects -- up to its look at the handle (mem comes just before it)
    label, table, n = np.zeros(16, np.int32), np.zeros(8, pwpp_hip.OBSTACLE_CLUSTER_DTYPE), np.zeros(1, np.int32)

    def track(h=fake, gr=G(), h_min=0.2, h_max=2.0, min_count=1, connectivity=8, frames=1, mem=2, label=vp(label), table=vp(table), max_clusters=8,
              prev=vp(prev), pose=vp(pose), n_poses=1, gate=0, min_overlap=1, max_pairs=8, cl=vp(cl), pl=vp(pl)):
        return lib.pwpp_track_obstacles(h, gr, h_min, h_max, min_count, connectivity, 0, frames, mem, label, None, None, table, vp(n), max_clusters, None, prev, pose,
                                        n_poses, gate, min_overlap, max_pairs, cl, pl, None, None, None, None, None)

    assert track(h=None) == E_ARG and b"null handle" in err()
    for kw, text in ((dict(gr=None), b"null grid"), (dict(label=None), b"null label image"), (dict(prev=None), b"null previous label image"), (dict(pose=None), b"null pose"),
                     (dict(cl=None), b"null curr_links"), (dict(pl=None), b"null prev_links")):
        assert track(**kw) == E_ARG and text in err(), kw
    assert track() == E_ARG and ok in err()
    assert track(gr=G(flags=2)) == E_ARG and b"grid flags 2" in err()
    assert track(h_min=2.0, h_max=1.0) == E_ARG and b"height band" in err()
    assert track(min_count=0) == E_ARG and b"min_count 0" in err()
    assert track(connectivity=6) == E_ARG and b"connectivity 6" in err()
    assert track(max_clusters=-1) == E_ARG and b"max_clusters -1" in err()
    assert track(table=None) == E_ARG and b"null cluster table" in err()
    assert track(gr=G(cell=0.0), gate=9) == E_ARG and b"cell size" in err()
    assert track(gate=9, max_pairs=0) == E_ARG and ok in err()  # the association's own checks come after the labelling's, which end at the handle


# ---- the restatement itself ---------------------------------------------------------------------------------------------------
def test_identity_links_every_row_to_itself_with_all_its_cells():
    img = tr.blobs(2, 13, 17, 3)
    g = tr.grid(-4.0, -3.0, 0.5, 17, 13)
    r = tr.associate(img, img, g, g, [tr.IDENTITY], 0, 1, 8, 64, id_prev=np.arange(16, dtype=np.int32).reshape(2, 8) + 100, next_id=[5, 6])
    rows = 0
    for f in range(2):
        for b in range(8):
            cells = int((img[f] == b).sum())
            for t in (r["curr_links"], r["prev_links"]):
                assert tuple(t[f, b]) == ((b, cells, cells, 1) if cells else (-1, 0, 0, 0))
            assert r["id_curr"][f, b] == (100 + 8 * f + b if cells else -1)
            rows += cells > 0
        assert r["n_pairs"][f] == sum((img[f] == b).any() for b in range(8))
    assert rows >= 6 and r["next_id_out"].tolist() == [5, 6]


@pytest.mark.parametrize("move", ["shift", "quarter"])
def test_a_whole_cell_shift_and_a_quarter_turn_are_lossless(move):
    n = 12
    g = tr.grid(-6.0, -6.0, 1.0, n, n)   # centred on the origin: a quarter turn maps cell centres onto cell centres
    prev = np.full((1, n, n), -1, np.int32)
    prev[0, 3:6, 4:9] = 0
    prev[0, 7:9, 2:4] = 1
    if move == "shift":                   # the previous frame's content lies 2 cells further in x and 1 in y in the current frame
        curr = np.full_like(prev, -1)
        curr[0, 1:, 2:] = prev[0, :-1, :-2]
        pose = (1.0, 0.0, 2.0, 0.0, 1.0, 1.0)
    else:                                 # X = -y, Y = x: np.rot90 of the image with x along the columns
        curr = np.full_like(prev, -1)
        for y in range(n):
            for x in range(n):
                curr[0, x, n - 1 - y] = prev[0, y, x]
        pose = tr.yaw(90)
    r = tr.associate(curr, prev, g, g, [pose], 0, 1, 4, 16)
    for b in (0, 1):
        cells = int((prev[0] == b).sum())
        assert tuple(r["curr_links"][0, b]) == (b, cells, cells, 1) and tuple(r["prev_links"][0, b]) == (b, cells, cells, 1)
    assert r["n_pairs"][0] == 2


def test_overlaps_sum_to_no_more_than_the_labelled_cells_and_ids_are_unique():
    for seed in range(6):
        curr, prev = tr.blobs(3, 15, 19, seed), tr.blobs(3, 11, 23, seed + 50)
        gc, gp = tr.grid(-5.0, -4.0, 0.5, 19, 15), tr.grid(-6.0, -3.0, 0.6, 23, 11)
        poses = [tr.yaw(30 * seed, 0.3, -0.2), tr.IDENTITY, tr.yaw(90, 1.0, 0.0)]
        id_prev = np.tile(np.arange(8, dtype=np.int32) + 40, (3, 1))
        id_prev[:, seed % 8] = -1
        r = tr.associate(curr, prev, gc, gp, poses, seed % 5, 1 + seed % 3, 8, 64, id_prev=id_prev, next_id=[1000, 2000, 0x7FFFFFFE])
        for f in range(3):
            n = tr.pair_counts(curr[f], prev[f], gc, gp, poses[f], seed % 5, 8)
            assert sum(n.values()) <= int(((curr[f] >= 0) & (curr[f] < 8)).sum())
            assert r["n_pairs"][f] == len(n) and sum(int(x["links"]) for x in r["curr_links"][f]) == len(n) == sum(int(x["links"]) for x in r["prev_links"][f])
            ids = [int(i) for i, l in zip(r["id_curr"][f], r["curr_links"][f]) if l["cells"] > 0]
            assert len(set(ids)) == len(ids) and all(i >= 0 for i in ids)
            assert all(int(i) == -1 for i, l in zip(r["id_curr"][f], r["curr_links"][f]) if l["cells"] == 0)


def test_the_gate_ties_merges_overflow_and_the_wrap():
    g = tr.grid(0.0, 0.0, 1.0, 5, 5)
    prev = np.full((1, 5, 5), -1, np.int32)
    prev[0, 2, 1], prev[0, 2, 3] = 1, 0          # equidistant from (2, 2): the smaller index, cell (1, 2) with row 1, wins
    curr = np.full((1, 5, 5), -1, np.int32)
    curr[0, 2, 2] = 0
    assert tuple(tr.associate(curr, prev, g, g, [tr.IDENTITY], 0, 1, 2, 4)["curr_links"][0, 0]) == (-1, 0, 1, 0)   # p itself is unlabelled
    assert tuple(tr.associate(curr, prev, g, g, [tr.IDENTITY], 1, 1, 2, 4)["curr_links"][0, 0]) == (1, 1, 1, 1)
    prev[0, 1, 2] = 0                             # as near, and a smaller index still
    assert tuple(tr.associate(curr, prev, g, g, [tr.IDENTITY], 4, 1, 2, 4)["curr_links"][0, 0]) == (0, 1, 1, 1)
    # a merge: two previous rows under one current row, equal overlaps -> the smaller label; mutual best gives its id to the merged row
    prev = np.full((1, 5, 5), -1, np.int32)
    prev[0, 0, 0:2], prev[0, 0, 2:4] = 3, 1
    curr = np.full((1, 5, 5), -1, np.int32)
    curr[0, 0, 0:4] = 2
    r = tr.associate(curr, prev, g, g, [tr.IDENTITY], 0, 2, 4, 4, id_prev=[[10, 11, 12, 13]], next_id=[0x7FFFFFFF])
    assert tuple(r["curr_links"][0, 2]) == (1, 2, 4, 2) and tuple(r["prev_links"][0, 1]) == (2, 2, 2, 1) and tuple(r["prev_links"][0, 3]) == (2, 2, 2, 1)
    assert r["id_curr"][0].tolist() == [-1, -1, 11, -1] and r["next_id_out"][0] == 0x7FFFFFFF
    r = tr.associate(curr, prev, g, g, [tr.IDENTITY], 0, 3, 4, 4, id_prev=[[10, 11, 12, 13]], next_id=[0x7FFFFFFF])   # min_overlap one above the overlap
    assert r["id_curr"][0].tolist() == [-1, -1, 0x7FFFFFFF, -1] and r["next_id_out"][0] == 0
    r = tr.associate(curr, prev, g, g, [tr.IDENTITY], 0, 1, 4, 1, id_prev=[[10, 11, 12, 13]], next_id=[7])            # two pairs, room for one
    assert r["n_pairs"][0] == 2 and [tuple(x) for x in r["curr_links"][0]] == [(-2, 0, 0, 0), (-2, 0, 0, 0), (-2, 0, 4, 0), (-2, 0, 0, 0)]
    assert [tuple(x) for x in r["prev_links"][0]] == [(-2, 0, 0, 0), (-2, 0, 2, 0), (-2, 0, 0, 0), (-2, 0, 2, 0)] and r["id_curr"][0].tolist() == [-1, -1, 7, -1]
    r = tr.associate(curr, prev, g, g, [(NAN, 0.0, 0.0, 0.0, 1.0, 0.0)], 4, 1, 4, 4)
    assert r["n_pairs"][0] == 0 and tuple(r["curr_links"][0, 2]) == (-1, 0, 4, 0) and tuple(r["prev_links"][0, 3]) == (-1, 0, 2, 0)


# ---- the C++ mirror and the header as C -------------------------------------------------------------------------------------------
CPP = r"""
#include "patchwork/patchworkpp.h"
#ifndef PWPP_HAS_CLUSTER_TRACKS
#error "include/pwpp.h does not announce the cluster tracks"
#endif
static_assert(sizeof(pwpp_cluster_link) == 16, "pwpp_cluster_link");
long use(patchwork::PatchWorkpp &pw) {
    const double pose[6] = {1.0, 0.0, 0.5, 0.0, 1.0, 0.0};
    const patchwork::PatchWorkpp::ObstacleTracks a = pw.trackObstacleClusters(-40.0, -40.0, 0.5, 160, 160, 0.2f, 2.0f);
    const patchwork::PatchWorkpp::ObstacleTracks b = pw.trackObstacleClusters(-40.0, -40.0, 0.5, 160, 160, 0.2f, 2.0f, pose, 2, 4, 128, 2, 3);
    pw.resetObstacleTracks();
    return (long)a.label[3] + a.count + b.pairs + (b.ids.empty() ? 0 : b.ids[0]) + (b.curr_links.empty() ? 0 : b.curr_links[0].other + b.prev_links[0].links) + b.nx + b.ny +
           (long)b.clusters.size();
}
"""


@pytest.mark.parametrize("flavour", ["plain", "eigen_shim"])
def test_cpp_mirror_method_compiles(tmp_path, flavour):
    src = tmp_path / "tracks.cpp"
    src.write_text(CPP)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(PKG, "include"), "-I", os.path.join(ROOT, "include")]
    cmd += ["-DPWPP_NO_EIGEN"] if flavour == "plain" else ["-I", os.path.join(ROOT, "oracle", "eigen_shim")]
    subprocess.run(cmd + [str(src)], check=True)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "tracks.c"
    src.write_text('#include "pwpp.h"\nint f(pwpp_cluster_link *l, const pwpp_ground_grid *g) { return pwpp_associate_grid(0, g, g, 1, PWPP_MEM_HOST, 0, 0, 0, 1, 0, 1, 1, 1, l, l, '
                   '0, 0, 0, 0, 0) + pwpp_track_obstacles(0, g, 0.f, 1.f, 1, 8, 0, 1, PWPP_MEM_HOST, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 1, l, l, 0, 0, 0, 0, 0) + '
                   '(int)sizeof(*l) + PWPP_HAS_CLUSTER_TRACKS; }\n')
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
    tmp = tmp_path_factory.mktemp("tracks_check")
    exe = tmp / "tracks_check"
    flags = SANITIZE if sanitizers_work(tmp) else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off"] + flags +
                   ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "tracks_check.cpp"), "-o", str(exe)], check=True)
    return exe


def test_tracks_program_builds_and_passes(checker):
    r = subprocess.run([str(checker)], capture_output=True, text=True)  # (a stand-alone child process with its own main)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
    assert int(r.stdout.split("tracks_check: ")[1].split(" cases")[0]) >= 2000


@pytest.mark.parametrize("case", ["yaw", "shift_ids", "overflow", "per_frame"])
def test_the_restatement_and_the_one_text_agree_byte_for_byte(checker, tmp_path, case):
    """The kernels' functions, dealt wave by wave on the host, against the dictionaries: what the GPU tests compare, without a GPU."""
    frames, rows = 3, 8
    gc, gp = tr.grid(-8.0, -7.0, 0.5, 37, 29), tr.grid(-9.0, -8.0, 1.0 if case == "yaw" else 0.3, 21 if case == "yaw" else 70, 19 if case == "yaw" else 55)
    curr, prev = tr.blobs(frames, gc["ny"], gc["nx"], 11, n_blobs=9), tr.blobs(frames, gp["ny"], gp["nx"], 12, n_blobs=9)
    curr[0, 0, 0], prev[0, 0, 0], curr[1, 2, 2], prev[1, 3, 3] = rows, rows, 2 ** 31 - 1, -2 ** 31
    poses = {"yaw": [tr.yaw(30, 0.4, -0.3)], "shift_ids": [(1.0, 0.0, 1.5, 0.0, 1.0, -1.0)], "overflow": [tr.IDENTITY],
             "per_frame": [tr.yaw(90), (NAN, 0.0, 0.0, 0.0, 1.0, 0.0), tr.yaw(200, 1.0, 2.0)]}[case]
    gate, min_overlap = {"yaw": (2, 1), "shift_ids": (4, 3), "overflow": (1, 1), "per_frame": (0, 2)}[case]
    with_ids = case != "yaw"
    id_prev = (np.arange(frames * rows, dtype=np.int32).reshape(frames, rows) * 3 + 7) if with_ids else None
    next_id = np.array([0x7FFFFFF0, 5, 0x7FFFFFFF], np.int32) if with_ids else None
    if with_ids:
        id_prev[0, 1] = -1
    most = int(tr.associate(curr, prev, gc, gp, poses, gate, min_overlap, rows, 4096)["n_pairs"].max())
    assert most >= 4
    max_pairs = most - 1 if case == "overflow" else most
    want = tr.associate(curr, prev, gc, gp, poses, gate, min_overlap, rows, max_pairs, id_prev, next_id)
    curr.tofile(tmp_path / "curr.i32")
    prev.tofile(tmp_path / "prev.i32")
    np.asarray(poses, np.float64).tofile(tmp_path / "poses.f64")
    if with_ids:
        np.concatenate([id_prev.ravel(), next_id]).astype(np.int32).tofile(tmp_path / "ids.i32")
    args = ["dump", str(tmp_path / "curr.i32"), str(tmp_path / "prev.i32"), str(tmp_path / "poses.f64"), str(len(poses)), str(frames)]
    args += [repr(g[k]) for g in (gc, gp) for k in ("x0", "y0", "cell", "nx", "ny")] + [str(gate), str(min_overlap), str(rows), str(max_pairs)]
    args += [str(tmp_path / "ids.i32") if with_ids else "-", str(tmp_path / "out")]
    subprocess.run([str(checker)] + args, check=True)
    for name in ("curr_links", "prev_links", "n_pairs") + (("id_curr", "next_id_out") if with_ids else ()):
        got = np.fromfile(str(tmp_path / "out") + "." + name, np.int32)
        assert got.tobytes() == np.ascontiguousarray(want[name]).tobytes(), name
    assert (want["n_pairs"] == max_pairs + 1).any() == (case == "overflow")
    if case == "per_frame":
        assert want["n_pairs"][1] == 0 and want["n_pairs"][0] > 0
