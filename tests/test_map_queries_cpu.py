"""No-GPU checks of what the post-call map queries share (pwpp_rasterize_obstacles, pwpp_label_obstacles, pwpp_box_obstacles,
pwpp_distance_obstacles, pwpp_visibility_obstacles, pwpp_fuse_obstacles, pwpp_match_obstacles; pwpp_label_grid, pwpp_distance_grid,
pwpp_visibility_grid on a caller's image; the map side of pwpp_fuse_* and pwpp_match_*): the argument checks they have in common, fed
to all of a kind through one loop -- the same code and the same message fragment from each -- and, with the restatements, that the batch of tests/test_gpu_map_query_ranges.py has clusters and boxes in the frames its
comparison is about."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ground_query_ref as gq
import obstacle_boxes_ref as ob
import obstacle_clusters_ref as oc
import obstacle_grid_ref as og
import oracle_lib as ol
import pwpp_hip
from test_gpu_map_query_ranges import BAND, CONN, FIRST, GRID, MAX_ROWS, MIN_COUNT, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchwork-plusplus_amd")
F32 = np.float32
E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pwpp_hip.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "lib/libpwpp_hip.so"], check=True, stdout=subprocess.DEVNULL)
    return pwpp_hip.load()


# (grid fields x0, y0, cell, nx, ny, flags), band, mem, a fragment of the message.  A NaN cell is the one input they do not
# name alike: pwpp_box_obstacles' extent check comes first ("... cells of nan m: ... at most 1024 m"), the others say "cell size".
SHARED_BAD_INPUTS = [
    ("grid flags 2", dict(flags=2), (0.2, 2.5), pwpp_hip.MEM_HOST, b"grid flags 2: 0 or PWPP_GRID_GROUND_ONLY"),
    ("band (2.5, 0.2)", {}, (2.5, 0.2), pwpp_hip.MEM_HOST, b"height band [2.5, 0.2]: h_min <= h_max expected"),
    ("band (NaN, 1)", {}, (np.nan, 1.0), pwpp_hip.MEM_HOST, b"h_min <= h_max expected, neither a NaN"),
    ("nx 0", dict(nx=0), (0.2, 2.5), pwpp_hip.MEM_HOST, b"grid of 0 x 4 cells"),
    ("cell 0", dict(cell=0.0), (0.2, 2.5), pwpp_hip.MEM_HOST, b"cell size must be finite, the cell size positive"),
    ("cell NaN", dict(cell=np.nan), (0.2, 2.5), pwpp_hip.MEM_HOST, b"cell"),
    ("mem PWPP_MEM_HOST_PINNED", {}, (0.2, 2.5), pwpp_hip.MEM_HOST_PINNED, b"mem 2: the "),
]


# The fused maps of the calls below: one of 4 x 4 cells of 1 m, and its int16 cells.
def fusion_map(**fields):
    return pwpp_hip.FusionMap(**dict(dict(x0=0.0, y0=0.0, cell=1.0, nx=4, ny=4, hit=40, miss=20, l_min=-200, l_max=350, occupied_at=60, free_at=-40), **fields))


def test_shared_bad_inputs_are_named_alike_by_all_seven_entry_points(lib):
    img = np.zeros(16, np.int32)
    box = np.zeros(4, ob.BOX_DTYPE)
    xy = np.array([0.5, 0.5], np.float64)  # (the sensor of the three that look first: inside every grid of the table that has cells)
    pose = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], np.float64)  # (the one pose of the fusion, the one candidate of the match)
    maps, best, fm = np.zeros(16, np.int16), np.zeros(1, pwpp_hip.MATCH_BEST_DTYPE), ctypes.byref(fusion_map())
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    entry_points = {
        "pwpp_fuse_obstacles": lambda g, band, mem: lib.pwpp_fuse_obstacles(fake, g, band[0], band[1], 1, vp(xy), 1, 0, 0, 1, mem, vp(pose), 1, None, fm, 1,
                                                                            None, None, vp(maps), None, None),
        "pwpp_match_obstacles": lambda g, band, mem: lib.pwpp_match_obstacles(fake, g, band[0], band[1], 1, vp(xy), 1, 0, 0, 1, mem, vp(pose), 1, 1, None, fm, 1,
                                                                              vp(maps), 1, 1, vp(best), None, None),
        "pwpp_rasterize_obstacles": lambda g, band, mem: lib.pwpp_rasterize_obstacles(fake, g, band[0], band[1], 0, 1, mem, vp(img), None, None),
        "pwpp_label_obstacles": lambda g, band, mem: lib.pwpp_label_obstacles(fake, g, band[0], band[1], 1, 8, 0, 1, mem, vp(img), None, None, None, None, 0, None),
        "pwpp_box_obstacles": lambda g, band, mem: lib.pwpp_box_obstacles(fake, g, band[0], band[1], 0, 1, mem, vp(img), vp(box), 4),
        "pwpp_distance_obstacles": lambda g, band, mem: lib.pwpp_distance_obstacles(fake, g, band[0], band[1], 1, 0, 0, 1, mem, vp(img), None, None, None),
        "pwpp_visibility_obstacles": lambda g, band, mem: lib.pwpp_visibility_obstacles(fake, g, band[0], band[1], 1, vp(xy), 1, 0, 0, 1, mem, vp(img), None, None),
    }
    for what, fields, band, mem, fragment in SHARED_BAD_INPUTS:
        g = pwpp_hip.GroundGrid(**dict(dict(x0=0.0, y0=0.0, cell=1.0, nx=4, ny=4, flags=0, pad_=0), **fields))
        for name, call in entry_points.items():
            assert call(ctypes.byref(g), band, mem) == E_ARG, "%s: %s" % (name, what)
            assert fragment in lib.pwpp_last_error(), "%s, %s: %s" % (name, what, lib.pwpp_last_error())
            if what.startswith("mem"):
                assert b"take PWPP_MEM_HOST or PWPP_MEM_DEVICE" in lib.pwpp_last_error(), name


# What the three operators on a caller's count image (pwpp_label_grid, pwpp_distance_grid, pwpp_visibility_grid) check alike:
# (nx, ny, frames, min_count, mem), a fragment of the message.
SHARED_BAD_IMAGES = [
    ("nx 0", dict(nx=0), b"frames of"),
    ("frames 0", dict(frames=0), b"frames of"),
    ("32768 x 32768 x 3 cells", dict(nx=32768, ny=32768, frames=3), b"exceed 2^31"),
    ("min_count 0", dict(min_count=0), b"min_count 0: at least 1 expected"),
    ("mem PWPP_MEM_HOST_PINNED", dict(mem=pwpp_hip.MEM_HOST_PINNED), b"take PWPP_MEM_HOST or PWPP_MEM_DEVICE"),
]
# The one message of the table that is not worded alike: "the visibility" is a singular, so its verb is "takes" -- and the fragment
# above is not in it.  The sentence is pinned whole instead, for all three.
MEM_SENTENCES = {
    "pwpp_label_grid": b"mem 2: the obstacle clusters take PWPP_MEM_HOST or PWPP_MEM_DEVICE",
    "pwpp_distance_grid": b"mem 2: the obstacle distances take PWPP_MEM_HOST or PWPP_MEM_DEVICE",
    "pwpp_visibility_grid": b"mem 2: the visibility takes PWPP_MEM_HOST or PWPP_MEM_DEVICE",
}


def test_shared_bad_images_are_named_alike_by_the_three_grid_entry_points(lib):
    img = np.zeros(16, np.int32)
    org = np.zeros(2, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    entry_points = {
        "pwpp_label_grid": lambda nx, ny, frames, min_count, mem: lib.pwpp_label_grid(fake, nx, ny, frames, mem, vp(img), None, min_count, 8, vp(img), None, None, 0),
        "pwpp_distance_grid": lambda nx, ny, frames, min_count, mem: lib.pwpp_distance_grid(fake, nx, ny, frames, mem, vp(img), min_count, 0, 1.0, vp(img), None, None),
        "pwpp_visibility_grid": lambda nx, ny, frames, min_count, mem: lib.pwpp_visibility_grid(fake, nx, ny, frames, mem, vp(img), min_count, vp(org), 1, 0, vp(img), None),
    }
    for what, fields, fragment in SHARED_BAD_IMAGES:
        args = dict(dict(nx=4, ny=4, frames=1, min_count=1, mem=pwpp_hip.MEM_HOST), **fields)
        for name, call in entry_points.items():
            assert call(**args) == E_ARG, "%s: %s" % (name, what)
            if what.startswith("mem"):
                assert lib.pwpp_last_error() == MEM_SENTENCES[name], "%s, %s: %s" % (name, what, lib.pwpp_last_error())
            if not (what.startswith("mem") and name == "pwpp_visibility_grid"):
                assert fragment in lib.pwpp_last_error(), "%s, %s: %s" % (name, what, lib.pwpp_last_error())


def test_the_batch_has_clusters_and_boxes_in_the_sub_range(oracle_built):
    oracle = oracle_built.restatement()
    p = oracle.default_params()
    x0, y0, cell, nx, ny = GRID
    lists = []
    for f, pts in enumerate(batch()):
        assert 2000 <= len(pts) <= 6400
        ref = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts)
        lists.append(len(ref.nonground_idx))
        xyz = np.ascontiguousarray(pts[np.sort(ref.nonground_idx), :3], F32)
        s, _ = gq.restate_query(xyz, ref.records, p)
        count, top, _ = og.restate_obstacles(xyz, s, x0, y0, cell, nx, ny, *BAND)
        label, table, n = oc.flood_fill(count, top, MIN_COUNT, CONN)
        kx, ix = og.cells_of(xyz[:, 0], x0, cell, nx)
        ky, iy = og.cells_of(xyz[:, 1], y0, cell, ny)
        hgt = np.ascontiguousarray(s["distance"], F32)
        with np.errstate(invalid="ignore"):
            counted = kx & ky & (s["patch"] >= 0) & (F32(BAND[0]) <= hgt) & (hgt <= F32(BAND[1]))
        rows = ob.box_rows(*GRID, xyz[counted], hgt[counted], label[iy[counted], ix[counted]].astype(np.int32), MAX_ROWS)
        print("frame %d: %d non-ground points, %d counted, %d clusters, %d boxes with points" % (f, lists[-1], counted.sum(), n, (rows["points"] > 0).sum()))
        if f >= FIRST:
            assert 2 <= n <= MAX_ROWS and (rows["points"][:n] > 0).all() and rows["points"].sum() == count[label >= 0].sum() > 50
    assert lists[2] > max(lists[:2]) and lists[0] != lists[1]


# What the fusion and the scan match check alike of the map side of a call of 3 frames: (fields of the map description, n_maps,
# map_of_frame), a fragment of the message.  The one message with a subject is the side limit's.
SHARED_BAD_MAPS = [
    ("a map of 0 cells a side", dict(nx=0), 1, None, b"1 frames of 0 x 4 cells"),
    ("a map of 32769 cells a side", dict(nx=32769), 1, None, b"32769 x 4 cells:  at most 32768 a side"),
    ("map cell 0", dict(cell=0.0), 1, None, b"cell sizes 1 (frames) and 0 (map): finite and positive expected"),
    ("map cell NaN", dict(cell=np.nan), 1, None, b"(map): finite and positive expected"),
    ("2 maps for 3 frames, null map_of_frame", {}, 2, None, b"null map_of_frame with 2 maps for 3 frames: 1 map or one per frame expected"),
    ("map_of_frame entry n_maps", {}, 2, [0, 2, 1], b"map_of_frame 1 names map 2: -1 (skipped) .. 1 expected"),
    ("map_of_frame entry -2", {}, 2, [0, -1, -2], b"map_of_frame 2 names map -2: -1 (skipped) .. 1 expected"),
]
SUBJECTS = {"pwpp_fuse_grid": b"the fusion takes", "pwpp_fuse_obstacles": b"the fusion takes", "pwpp_match_grid": b"the scan match takes",
            "pwpp_match_obstacles": b"the scan match takes"}


def test_shared_bad_maps_are_named_alike_by_the_fusion_and_the_scan_match(lib):
    frames, H = 3, pwpp_hip.MEM_HOST
    occ, xy = np.zeros(frames * 16, np.int8), np.array([0.5, 0.5], np.float64)
    pose = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], np.float64)  # (the one pose of the fusion, the one candidate of the match)
    maps, best = np.zeros(2 * 16, np.int16), np.zeros(frames, pwpp_hip.MATCH_BEST_DTYPE)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # (never dereferenced: these checks come first)
    g = ctypes.byref(pwpp_hip.GroundGrid(x0=0.0, y0=0.0, cell=1.0, nx=4, ny=4, flags=0, pad_=0))
    entry_points = {
        "pwpp_fuse_grid": lambda m, n_maps, mof: lib.pwpp_fuse_grid(fake, g, frames, H, vp(occ), vp(pose), 1, mof, m, n_maps, None, None, vp(maps), None),
        "pwpp_fuse_obstacles": lambda m, n_maps, mof: lib.pwpp_fuse_obstacles(fake, g, 0.2, 2.5, 1, vp(xy), 1, 0, 0, frames, H, vp(pose), 1, mof, m, n_maps,
                                                                              None, None, vp(maps), None, None),
        "pwpp_match_grid": lambda m, n_maps, mof: lib.pwpp_match_grid(fake, g, frames, H, vp(occ), vp(pose), 1, 1, mof, m, n_maps, vp(maps), 1, 1, vp(best), None),
        "pwpp_match_obstacles": lambda m, n_maps, mof: lib.pwpp_match_obstacles(fake, g, 0.2, 2.5, 1, vp(xy), 1, 0, 0, frames, H, vp(pose), 1, 1, mof, m, n_maps,
                                                                                vp(maps), 1, 1, vp(best), None, None),
    }
    for what, fields, n_maps, mof, sentence in SHARED_BAD_MAPS:
        mof = None if mof is None else np.array(mof, np.int32)
        said = set()
        for name, call in entry_points.items():
            assert call(ctypes.byref(fusion_map(**fields)), n_maps, None if mof is None else vp(mof)) == E_ARG, "%s: %s" % (name, what)
            said.add(lib.pwpp_last_error().replace(SUBJECTS[name], b""))
        assert len(said) == 1 and sentence in said.pop(), "%s: %s" % (what, lib.pwpp_last_error())
