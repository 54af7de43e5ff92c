"""ctypes binding of the C-ABI in include/pwpp.h (libpwpp_hip.so).

Thin host-side plumbing for tests, bench.py and Python callers that want the batch API;
the drop-in Python surface of the reference (module ``pypatchworkpp``) is the pybind11
module built from pybinding.cpp next to this file.  No CPU fallback: if the shared
library is missing or there is no GPU, constructing a :class:`Handle` raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libpwpp_hip.so")

LAYOUT_ROW_MAJOR, LAYOUT_COL_MAJOR = 0, 1
MEM_HOST, MEM_DEVICE = 0, 1
MODE_FRESH, MODE_STREAMS = 0, 1
MEM_HOST_PINNED = 2
NUM_KERNELS = 11
ORDER_SCATTER, ORDER_REFERENCE, ORDER_CLOUD = 0, 1, 2
LABEL_NONGROUND, LABEL_GROUND, LABEL_UNCLASSIFIED = 0, 1, 2

DEC_NAMES = {1: "not_upright", 2: "far_ground", 3: "heading", 4: "ground", 5: "tgr_reject", 6: "tgr_revert"}


class Params(ctypes.Structure):
    """pwpp_params = patchwork::Params (reference patchworkpp.h:42-112)."""

    _fields_ = (
        [(n, ctypes.c_int32) for n in
         "verbose enable_RNR enable_RVPF enable_TGR num_iter num_lpr num_min_pts num_zones "
         "num_rings_of_interest pad0_".split()]
        + [(n, ctypes.c_double) for n in
           "RNR_ver_angle_thr RNR_intensity_thr sensor_height th_seeds th_dist th_seeds_v th_dist_v "
           "max_range min_range uprightness_thr adaptive_seed_selection_margin intensity_thr".split()]
        + [("num_sectors_each_zone", ctypes.c_int32 * 4), ("num_rings_each_zone", ctypes.c_int32 * 4),
           ("max_flatness_storage", ctypes.c_int32), ("max_elevation_storage", ctypes.c_int32),
           ("elevation_thr", ctypes.c_double * 4), ("flatness_thr", ctypes.c_double * 4)]
    )


class State(ctypes.Structure):
    _fields_ = [("sensor_height", ctypes.c_double), ("elevation_thr", ctypes.c_double * 4),
                ("flatness_thr", ctypes.c_double * 4), ("elevation_len", ctypes.c_int32 * 4),
                ("flatness_len", ctypes.c_int32 * 4)]


RECORD_DTYPE = np.dtype([("bin", "<i4"), ("concentric_idx", "<i4"), ("n_points", "<i4"), ("n_ground", "<i4"),
                         ("n_nonground", "<i4"), ("decision", "<i4"), ("mean", "<f4", 3), ("normal", "<f4", 3),
                         ("sv", "<f4", 3), ("rounds", "<i4"), ("d", "<f8")])


class DeviceView(ctypes.Structure):
    _fields_ = [("indices", ctypes.c_void_p), ("frame_base", ctypes.POINTER(ctypes.c_int64)),
                ("counts", ctypes.POINTER(ctypes.c_int32)), ("frames", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class GroundSample(ctypes.Structure):  # pwpp_ground_sample
    _fields_ = [("patch", ctypes.c_int32), ("decision", ctypes.c_int32), ("ground_z", ctypes.c_float),
                ("distance", ctypes.c_float)]


class GroundGrid(ctypes.Structure):  # pwpp_ground_grid
    _fields_ = [("x0", ctypes.c_double), ("y0", ctypes.c_double), ("cell", ctypes.c_double), ("nx", ctypes.c_int32),
                ("ny", ctypes.c_int32), ("flags", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class ObstacleCluster(ctypes.Structure):  # pwpp_obstacle_cluster (48 bytes)
    _fields_ = [("first_cell", ctypes.c_int32), ("cells", ctypes.c_int32), ("points", ctypes.c_int32), ("ix_min", ctypes.c_int32),
                ("ix_max", ctypes.c_int32), ("iy_min", ctypes.c_int32), ("iy_max", ctypes.c_int32), ("top", ctypes.c_float),
                ("sum_ix", ctypes.c_int64), ("sum_iy", ctypes.c_int64)]


OBSTACLE_CLUSTER_DTYPE = np.dtype([("first_cell", "<i4"), ("cells", "<i4"), ("points", "<i4"), ("ix_min", "<i4"), ("ix_max", "<i4"),
                                   ("iy_min", "<i4"), ("iy_max", "<i4"), ("top", "<f4"), ("sum_ix", "<i8"), ("sum_iy", "<i8")])
_BOX_FLOATS = ("mean_x", "mean_y", "cx", "cy", "ax", "ay", "length", "width", "sigma_long", "sigma_short", "h_min", "h_max", "z_min", "z_max")


class ObstacleBox(ctypes.Structure):  # pwpp_obstacle_box (64 bytes)
    _fields_ = [("points", ctypes.c_int32), ("pad_", ctypes.c_int32)] + [(n, ctypes.c_float) for n in _BOX_FLOATS]


OBSTACLE_BOX_DTYPE = np.dtype([("points", "<i4"), ("pad_", "<i4")] + [(n, "<f4") for n in _BOX_FLOATS])
OBSTACLE_HULL_DTYPE = np.dtype([("points", "<i4"), ("n_vertices", "<i4"), ("stored", "<i4"), ("rect_edge", "<i4"), ("area2", "<i8"),  # pwpp_obstacle_hull (64 bytes)
                                ("qx_min", "<i4"), ("qx_max", "<i4"), ("qy_min", "<i4"), ("qy_max", "<i4")] +
                               [(n, "<f4") for n in ("cx", "cy", "ax", "ay", "length", "width")])
HULL_VERTICES_MAX = 1024  # PWPP_HULL_VERTICES_MAX
GROUND_SAMPLE_DTYPE = np.dtype([("patch", "<i4"), ("decision", "<i4"), ("ground_z", "<f4"), ("distance", "<f4")])
GRID_GROUND_ONLY = 1
DIST_BEYOND = 0x7fffffff  # PWPP_DIST_BEYOND: dist2 where no occupied cell is in reach (nearest -1, metres +inf)
VIS_NONE, VIS_BEYOND = -1, -2  # PWPP_VIS_NONE, PWPP_VIS_BEYOND: first where nothing lies on the line / the cell is beyond max_range
OCC_FREE, OCC_OCCUPIED, OCC_UNKNOWN = 0, 100, -1  # PWPP_OCC_*: the occupancy bytes, nav_msgs/OccupancyGrid values


class FusionMap(ctypes.Structure):  # pwpp_fusion_map: the grid of the fused maps in the fixed frame, the update's parameters, the byte's thresholds
    _fields_ = [("x0", ctypes.c_double), ("y0", ctypes.c_double), ("cell", ctypes.c_double), ("nx", ctypes.c_int32), ("ny", ctypes.c_int32),
                ("hit", ctypes.c_int32), ("miss", ctypes.c_int32), ("l_min", ctypes.c_int32), ("l_max", ctypes.c_int32),
                ("occupied_at", ctypes.c_int32), ("free_at", ctypes.c_int32)]


class HeightMap(ctypes.Structure):  # pwpp_height_map (40 bytes): the grid of the fused elevation maps in the fixed frame, the observations a mean remembers
    _fields_ = [("x0", ctypes.c_double), ("y0", ctypes.c_double), ("cell", ctypes.c_double), ("nx", ctypes.c_int32), ("ny", ctypes.c_int32),
                ("n_max", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class TerrainParams(ctypes.Structure):  # pwpp_terrain_params (24 bytes): the window's radius, the fewest known cells for a cost, the three limits of the cost
    _fields_ = [("radius", ctypes.c_int32), ("min_known", ctypes.c_int32), ("step_max", ctypes.c_float), ("slope_max", ctypes.c_float),
                ("rough_max", ctypes.c_float), ("pad_", ctypes.c_int32)]


class ReachParams(ctypes.Structure):  # pwpp_reach_params (24 bytes): the cost of free ground, the lethal byte, the unknown cells' byte, the clearance, the limit
    _fields_ = [("base", ctypes.c_int32), ("lethal", ctypes.c_int32), ("unknown", ctypes.c_int32), ("clearance2", ctypes.c_int32),
                ("max_reach", ctypes.c_int32), ("pad_", ctypes.c_int32)]


REACH_NONE = 0x7FFFFFFF  # PWPP_REACH_NONE: no path from the source


class RouteParams(ctypes.Structure):  # pwpp_route_params (16 bytes): the cells and waypoints stored per route, how far a shortcut looks, what its line may cross
    _fields_ = [("max_cells", ctypes.c_int32), ("max_waypoints", ctypes.c_int32), ("look", ctypes.c_int32), ("line_cost", ctypes.c_int32)]


ROUTE_OK, ROUTE_NONE, ROUTE_BROKEN = 0, 1, 2  # PWPP_ROUTE_*: the status of a route
ROUTE_DTYPE = np.dtype([(n, "<i4") for n in ("status", "cells", "cost", "edge_steps", "corner_steps", "max_term", "min_dist2", "waypoints")])  # pwpp_route (32 bytes)


class FootprintParams(ctypes.Structure):  # pwpp_footprint_params (24 bytes): the rectangle [-rear, front] x [-half_width, half_width] in ticks of 1/16 cell, the flags
    _fields_ = [("front", ctypes.c_int32), ("rear", ctypes.c_int32), ("half_width", ctypes.c_int32), ("flags", ctypes.c_int32), ("pad_", ctypes.c_int32 * 2)]


FOOT_FREE, FOOT_HIT, FOOT_SKIPPED = 0, 1, 2  # PWPP_FOOT_*: the status of a pose
FOOT_OUTSIDE_BLOCKS = 1  # PWPP_FOOT_OUTSIDE_BLOCKS: a covered cell outside the image makes the pose a HIT
FOOT_SUB = 16  # PWPP_FOOT_SUB: ticks per cell side
VIEW_NO_HEIGHT, VIEW_MAX_RISE, VIEW_UNITS_PER_M = -2 ** 31, 1 << 20, 1024  # PWPP_VIEW_*: no height, the clamp of a rise, units per metre
BEAMS_GROUND, BEAMS_NONGROUND = 1, 2  # PWPP_BEAMS_*: the index lists rasterize_beams selects (`which`, a bit set)
FOOT_POSE_DTYPE = np.dtype([(n, "<i4") for n in ("status", "covered", "outside", "blocked", "unknown", "max_term", "min_dist2", "hit")])  # pwpp_footprint_pose_row (32 bytes)
FOOT_TRAJ_DTYPE = np.dtype([(n, "<i4") for n in ("first_hit", "free_steps", "last", "max_term", "sum_term", "unknown", "min_dist2", "reach_last")])  # pwpp_footprint_traj_row (32 bytes)


class CostmapParams(ctypes.Structure):  # pwpp_costmap_params (24 bytes): the layers' mask, what an unknown occupancy / terrain byte counts as, when unknown wins
    _fields_ = [("layers", ctypes.c_int32), ("occupancy_unknown", ctypes.c_int32), ("terrain_unknown", ctypes.c_int32),
                ("unknown_below", ctypes.c_int32), ("pad_", ctypes.c_int32 * 2)]


COSTMAP_OCCUPANCY, COSTMAP_INFLATION, COSTMAP_TERRAIN = 1, 2, 4  # PWPP_COSTMAP_*: the layers, and their bits of `why`
COSTMAP_WHY_UNKNOWN = 8  # PWPP_COSTMAP_WHY_UNKNOWN: the bit of `why` of a cell with a layer that stayed unknown
COSTMAP_MAX_CURVE = 4097  # PWPP_COSTMAP_MAX_CURVE: the longest inflation table, dist2 0 .. 64^2


class ClusterLink(ctypes.Structure):  # pwpp_cluster_link (16 bytes): a row's best partner on the other side, their shared cells, its own cells, its partners
    _fields_ = [("other", ctypes.c_int32), ("overlap", ctypes.c_int32), ("cells", ctypes.c_int32), ("links", ctypes.c_int32)]


CLUSTER_LINK_DTYPE = np.dtype([("other", "<i4"), ("overlap", "<i4"), ("cells", "<i4"), ("links", "<i4")])
LINK_NONE, LINK_OVERFLOWED = -1, -2  # `other` of a row without a partner; of every row of a frame with more than max_pairs pairs


class EvidenceRule(ctypes.Structure):  # pwpp_evidence_rule (16 bytes): the gate in map cells, the fewest landed cells of a verdict, the two shares in 256ths
    _fields_ = [("gate", ctypes.c_int32), ("min_cells", ctypes.c_int32), ("moving_share", ctypes.c_int32), ("static_share", ctypes.c_int32)]


CLUSTER_EVIDENCE_DTYPE = np.dtype([("sum", "<i8"), ("cells", "<i4"), ("landed", "<i4"), ("occupied", "<i4"), ("free", "<i4"), ("unknown", "<i4"),
                                   ("verdict", "<i4")])  # pwpp_cluster_evidence (32 bytes)
EVID_NONE, EVID_UNDECIDED, EVID_STATIC, EVID_MOVING = -1, 0, 1, 2  # PWPP_EVID_*: the verdict of a row
EVID_CELL_NONE = -2  # PWPP_EVID_CELL_NONE: cell_class of a cell that is not labelled or not landed
EVID_LDS_ROWS = 512  # PWPP_EVID_LDS_ROWS: the rows the option "evidence_path" = 2 keeps in LDS


class MatchBest(ctypes.Structure):  # pwpp_match_best (24 bytes): the winning sum, its candidate (-1: skipped) and shift, the frame's occupied cells
    _fields_ = [("score", ctypes.c_int64), ("candidate", ctypes.c_int32), ("sx", ctypes.c_int32), ("sy", ctypes.c_int32), ("cells", ctypes.c_int32)]


MATCH_BEST_DTYPE = np.dtype([("score", "<i8"), ("candidate", "<i4"), ("sx", "<i4"), ("sy", "<i4"), ("cells", "<i4")])


class PwppError(RuntimeError):
    pass


_lib = None


def load():
    """Load libpwpp_hip.so (raises if it has not been built -- there is no fallback)."""
    global _lib
    if _lib is None:
        path = os.environ.get("PWPP_LIB_PATH", LIB_PATH)  # A/B runs of two builds (tools/ab_bench.sh)
        if not os.path.exists(path):
            raise PwppError("%s not built; run __graft_entry__.build() or make -C patchwork-plusplus_amd" % path)
        L = ctypes.CDLL(path)
        L.pwpp_last_error.restype = ctypes.c_char_p
        L.pwpp_kernel_name.restype = ctypes.c_char_p
        L.pwpp_get_height.restype = ctypes.c_double
        L.pwpp_get_time_us.restype = ctypes.c_double
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.pwpp_create.argtypes = [ctypes.POINTER(Params), ci, ctypes.POINTER(vp)]
        L.pwpp_destroy.argtypes = [vp]
        L.pwpp_estimate_ground.argtypes = [vp, vp, ci, ci, ci]
        L.pwpp_estimate_ground_batch.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci]
        L.pwpp_estimate_ground_fields.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci]
        L.pwpp_estimate_ground_fields_batch.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci]
        L.pwpp_synchronize.argtypes = [vp]
        L.pwpp_set_num_streams.argtypes = [vp, ci]
        L.pwpp_get_counts.argtypes = [vp, ci, vp, vp, vp]
        for name in ("pwpp_get_ground_indices", "pwpp_get_nonground_indices", "pwpp_get_ground_xyz",
                     "pwpp_get_nonground_xyz", "pwpp_get_centers", "pwpp_get_normals"):
            getattr(L, name).argtypes = [vp, ci, vp]
        L.pwpp_get_patch_records.argtypes = [vp, ci, vp, ci]
        L.pwpp_get_height.argtypes = [vp]
        L.pwpp_get_time_us.argtypes = [vp]
        L.pwpp_get_state.argtypes = [vp, ci, ctypes.POINTER(State)]
        L.pwpp_get_history.argtypes = [vp, ci, ci, ci, vp, ci]
        L.pwpp_set_state.argtypes = [vp, ci, ctypes.POINTER(State)]
        L.pwpp_set_history.argtypes = [vp, ci, ci, ci, vp, ci]
        L.pwpp_get_bin_boxes.argtypes = [vp, vp, ci]
        L.pwpp_get_fxp_geometry.argtypes = [vp, vp, vp, ci]
        L.pwpp_get_fixed_up_frames.argtypes = [vp]
        L.pwpp_get_fixed_up_frames.restype = ctypes.c_int64
        L.pwpp_get_clamped_frames.argtypes = [vp]
        L.pwpp_get_clamped_frames.restype = ctypes.c_int64
        L.pwpp_get_plane_state.argtypes = [vp, ci, vp]
        L.pwpp_set_plane_state.argtypes = [vp, ci, vp]
        L.pwpp_get_device_view.argtypes = [vp, ctypes.POINTER(DeviceView)]
        L.pwpp_set_profiling.argtypes = [vp, ci]
        L.pwpp_host_alloc.argtypes = [ctypes.POINTER(vp), ctypes.c_uint64]
        L.pwpp_host_free.argtypes = [vp]
        L.pwpp_get_all_indices.argtypes = [vp, vp, vp, vp]
        L.pwpp_get_kernel_profile.argtypes = [vp, vp, vp]
        L.pwpp_reset_kernel_profile.argtypes = [vp]
        L.pwpp_get_fxp_shift.argtypes = [vp]
        L.pwpp_get_fxp_origins.argtypes = [vp, vp, ci]
        L.pwpp_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p]
        L.pwpp_trim_workspace.argtypes = [vp]
        L.pwpp_get_workspace_bytes.argtypes = [vp]
        L.pwpp_get_workspace_bytes.restype = ctypes.c_int64
        L.pwpp_get_one_pass_stats.argtypes = [vp, vp, vp]
        L.pwpp_get_redo_stats.argtypes = [vp, vp, vp]
        L.pwpp_pipe_create.argtypes = [vp, ci, ci, ctypes.POINTER(vp)]
        L.pwpp_pipe_submit.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ctypes.POINTER(vp)]
        L.pwpp_pipe_set_num_streams.argtypes = [vp, ci]
        L.pwpp_get_arena_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
        L.pwpp_pipe_drain.argtypes = [vp]
        L.pwpp_pipe_handle.argtypes = [vp, ci]
        L.pwpp_pipe_handle.restype = vp
        L.pwpp_pipe_destroy.argtypes = [vp]
        L.pwpp_set_output_order.argtypes = [vp, ci]
        L.pwpp_set_overlap.argtypes = [vp, ci]
        L.pwpp_set_labels.argtypes = [vp, ci]
        L.pwpp_get_labels.argtypes = [vp, ci, vp]
        L.pwpp_get_all_labels.argtypes = [vp, vp]
        L.pwpp_get_device_labels.argtypes = [vp, ctypes.POINTER(vp)]
        L.pwpp_set_point_planes.argtypes = [vp, ci]
        for name in ("pwpp_get_point_patches", "pwpp_get_point_distances"):
            getattr(L, name).argtypes = [vp, ci, vp]
        for name in ("pwpp_get_all_point_patches", "pwpp_get_all_point_distances"):
            getattr(L, name).argtypes = [vp, vp]
        L.pwpp_get_device_point_planes.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp)]
        if hasattr(L, "pwpp_set_point_records"):  # (an older build named by PWPP_LIB_PATH has no point records: A/B runs against it)
            L.pwpp_set_point_records.argtypes = [vp, ci]
            L.pwpp_get_record_bytes.argtypes = [vp]
            for name in ("pwpp_get_ground_records", "pwpp_get_nonground_records"):
                getattr(L, name).argtypes = [vp, ci, vp]
            L.pwpp_get_all_records.argtypes = [vp, vp, vp, vp]
            L.pwpp_get_device_records.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int32)]
        if hasattr(L, "pwpp_query_ground"):  # (as above: an older build has no ground queries)
            L.pwpp_query_ground.argtypes = [vp, vp, vp, ctypes.c_int64, ci, vp]
            L.pwpp_rasterize_ground.argtypes = [vp, ctypes.POINTER(GroundGrid), ci, ci, ci, vp, vp]
        if hasattr(L, "pwpp_rasterize_obstacles"):  # (as above: an older build has no obstacle grid)
            L.pwpp_rasterize_obstacles.argtypes = [vp, ctypes.POINTER(GroundGrid), ctypes.c_float, ctypes.c_float, ci, ci, ci, vp, vp, vp]
        if hasattr(L, "pwpp_label_grid"):  # (as above: an older build has no obstacle clusters)
            L.pwpp_label_grid.argtypes = [vp, ci, ci, ci, ci, vp, vp, ci, ci, vp, vp, vp, ci]
            L.pwpp_label_obstacles.argtypes = [vp, ctypes.POINTER(GroundGrid), ctypes.c_float, ctypes.c_float, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp]
        if hasattr(L, "pwpp_box_obstacles"):  # (as above: an older build has no obstacle boxes)
            L.pwpp_box_obstacles.argtypes = [vp, ctypes.POINTER(GroundGrid), ctypes.c_float, ctypes.c_float, ci, ci, ci, vp, vp, ci]
            L.pwpp_box_points.argtypes = [ctypes.POINTER(GroundGrid), vp, vp, vp, ctypes.c_int64, vp, ci]
        if hasattr(L, "pwpp_hull_obstacles"):  # (as above: an older build has no obstacle hulls)
            L.pwpp_hull_obstacles.argtypes = [vp, ctypes.POINTER(GroundGrid), ctypes.c_float, ctypes.c_float, ci, ci, ci, vp, vp, ci, vp, ci]
            L.pwpp_hull_points.argtypes = [ctypes.POINTER(GroundGrid), vp, vp, ctypes.c_int64, vp, ci, vp, ci]
            L.pwpp_hull_vertex_xy.argtypes = [ctypes.POINTER(GroundGrid), vp, vp]
        if hasattr(L, "pwpp_distance_grid"):  # (as above: an older build has no obstacle distances)
            L.pwpp_distance_grid.argtypes = [vp, ci, ci, ci, ci, vp, ci, ci, ctypes.c_double, vp, vp, vp]
            L.pwpp_distance_obstacles.argtypes = [vp, ctypes.POINTER(GroundGrid), ctypes.c_float, ctypes.c_float, ci, ci, ci, ci, ci, vp, vp, vp, vp]
        if hasattr(L, "pwpp_visibility_grid"):  # (as above: an older build has no line-of-sight free space)
            L.pwpp_visibility_grid.argtypes = [vp, ci, ci, ci, ci, vp, ci, vp, ci, ci, vp, vp]
            L.pwpp_visibility_obstacles.argtypes = [vp, ctypes.POINTER(GroundGrid), ctypes.c_float, ctypes.c_float, ci, vp, ci, ci, ci, ci, ci, vp, vp, vp]
        if hasattr(L, "pwpp_fuse_grid"):  # (as above: an older build has no occupancy fusion)
            gp, mp = ctypes.POINTER(GroundGrid), ctypes.POINTER(FusionMap)
            L.pwpp_fuse_grid.argtypes = [vp, gp, ci, ci, vp, vp, ci, vp, mp, ci, vp, vp, vp, vp]
            L.pwpp_fuse_obstacles.argtypes = [vp, gp, ctypes.c_float, ctypes.c_float, ci, vp, ci, ci, ci, ci, ci, vp, ci, vp, mp, ci, vp, vp, vp, vp, vp]
        if hasattr(L, "pwpp_match_grid"):  # (as above: an older build has no scan match)
            gp, mp, cf = ctypes.POINTER(GroundGrid), ctypes.POINTER(FusionMap), ctypes.c_float
            L.pwpp_match_grid.argtypes = [vp, gp, ci, ci, vp, vp, ci, ci, vp, mp, ci, vp, ci, ci, vp, vp]
            L.pwpp_match_obstacles.argtypes = [vp, gp, cf, cf, ci, vp, ci, ci, ci, ci, ci, vp, ci, ci, vp, mp, ci, vp, ci, ci, vp, vp, vp]
            L.pwpp_match_pose.argtypes = [vp, ctypes.c_double, ci, ci, vp]
        if hasattr(L, "pwpp_fuse_height_grid"):  # (as above: an older build has no elevation fusion)
            gp, hp = ctypes.POINTER(GroundGrid), ctypes.POINTER(HeightMap)
            L.pwpp_fuse_height_grid.argtypes = [vp, gp, ci, ci, vp, vp, vp, ci, vp, hp, ci, vp, vp, vp, vp, vp, vp]
            L.pwpp_fuse_ground.argtypes = [vp, gp, ci, ci, ci, vp, vp, ci, vp, hp, ci, vp, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "pwpp_terrain_grid"):  # (as above: an older build has no terrain analysis)
            gp, tp = ctypes.POINTER(GroundGrid), ctypes.POINTER(TerrainParams)
            L.pwpp_terrain_grid.argtypes = [vp, ci, ci, ci, ctypes.c_double, ci, vp, tp, vp, vp, vp, vp, vp]
            L.pwpp_terrain_ground.argtypes = [vp, gp, ci, ci, ci, tp, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "pwpp_reach_grid"):  # (as above: an older build has no cost-to-reach field)
            gp, tp, rp = ctypes.POINTER(GroundGrid), ctypes.POINTER(TerrainParams), ctypes.POINTER(ReachParams)
            L.pwpp_reach_grid.argtypes = [vp, ci, ci, ci, ci, vp, vp, rp, vp, ci, vp, vp]
            L.pwpp_reach_ground.argtypes = [vp, gp, ci, ci, ci, tp, rp, vp, ci, vp, vp, vp]
            L.pwpp_grid_cell_of.argtypes = [gp, ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
        if hasattr(L, "pwpp_route_grid"):  # (as above: an older build has no routes)
            rp, qp = ctypes.POINTER(ReachParams), ctypes.POINTER(RouteParams)
            L.pwpp_route_grid.argtypes = [vp, ci, ci, ci, ci, vp, vp, rp, vp, ci, vp, vp, ci, ci, qp, vp, vp, vp]
            L.pwpp_plan_grid.argtypes = [vp, ci, ci, ci, ci, vp, vp, rp, vp, ci, vp, ci, ci, qp, vp, vp, vp, vp, vp]
        if hasattr(L, "pwpp_footprint_grid"):  # (as above: an older build has no footprints)
            rp, fp, i32p = ctypes.POINTER(ReachParams), ctypes.POINTER(FootprintParams), ctypes.POINTER(ctypes.c_int32)
            L.pwpp_footprint_grid.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, rp, fp, vp, ci, ci, ci, vp, vp]
            L.pwpp_footprint_covers.argtypes = [fp, i32p, ci, ci]
            L.pwpp_footprint_pose.argtypes = [ctypes.POINTER(GroundGrid), ctypes.c_double, ctypes.c_double, ctypes.c_double, i32p]
        if hasattr(L, "pwpp_viewshed_grid"):  # (as above: an older build has no viewshed)
            gp, cf = ctypes.POINTER(GroundGrid), ctypes.c_float
            L.pwpp_viewshed_grid.argtypes = [vp, ci, ci, ci, ci, vp, ci, vp, vp, vp, ci, vp, ci, ci, vp, vp, vp]
            L.pwpp_rasterize_ground_returns.argtypes = [vp, gp, ci, ci, ci, vp]
            L.pwpp_viewshed_obstacles.argtypes = [vp, gp, cf, cf, ci, ci, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp]
            L.pwpp_viewshed_units.argtypes = [ctypes.c_double]
            L.pwpp_viewshed_units.restype = ctypes.c_int32
        if hasattr(L, "pwpp_beam_grid"):  # (as above: an older build has no beams)
            gp, i32 = ctypes.POINTER(GroundGrid), ctypes.c_int32
            L.pwpp_rasterize_beams.argtypes = [vp, gp, ci, ci, ci, ci, vp, vp]
            L.pwpp_beam_grid.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp, vp, vp]
            L.pwpp_beam_ground.argtypes = [vp, gp, ci, vp, ci, ci, ci, ctypes.c_double, ci, ci, ci, vp, vp, vp, vp, vp, vp]
            L.pwpp_beam_height.argtypes = [i32, i32, ci, ci]
            L.pwpp_beam_height.restype = i32
        if hasattr(L, "pwpp_costmap_grid"):  # (as above: an older build has no costmap)
            gp, tp, cp = ctypes.POINTER(GroundGrid), ctypes.POINTER(TerrainParams), ctypes.POINTER(CostmapParams)
            cf, cd, i32 = ctypes.c_float, ctypes.c_double, ctypes.c_int32
            L.pwpp_costmap_grid.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, cp, vp, ci, vp, vp]
            L.pwpp_costmap_obstacles.argtypes = [vp, gp, cf, cf, ci, vp, ci, ci, tp, cp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp]
            L.pwpp_costmap_cell.argtypes = [cp, vp, ci, ci, ci, i32, ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_uint32)]
            L.pwpp_costmap_curve.argtypes = [cd, cd, cd, cd, ci, vp, ci]
        if hasattr(L, "pwpp_associate_grid"):  # (as above: an older build has no cluster tracks)
            gp = ctypes.POINTER(GroundGrid)
            L.pwpp_associate_grid.argtypes = [vp, gp, gp, ci, ci, vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
            L.pwpp_track_obstacles.argtypes = [vp, gp, ctypes.c_float, ctypes.c_float, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp,
                                               vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "pwpp_evidence_grid"):  # (as above: an older build has no map evidence)
            gp, mp, ep = ctypes.POINTER(GroundGrid), ctypes.POINTER(FusionMap), ctypes.POINTER(EvidenceRule)
            L.pwpp_evidence_grid.argtypes = [vp, gp, ci, ci, vp, vp, vp, ci, vp, mp, ci, vp, ep, ci, vp, vp, vp]
            L.pwpp_evidence_obstacles.argtypes = [vp, gp, ctypes.c_float, ctypes.c_float, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp,
                                                  vp, vp, ci, vp, mp, ci, vp, ep, vp, vp, vp]
            L.pwpp_evidence_verdict.argtypes = [ep, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
        if hasattr(L, "pwpp_set_input_transforms"):  # (as above: an older build has no input transforms)
            L.pwpp_set_input_transforms.argtypes = [vp, vp, ci]
            L.pwpp_transform_points.argtypes = [vp, vp, ctypes.c_int64, vp]
        L.pwpp_kernel_name.argtypes = [ci]
        _lib = L
    return _lib


def _curve(curve):  # the inflation table as the library reads it, None staying None
    return None if curve is None else np.ascontiguousarray(np.asarray(curve, np.uint8).reshape(-1))


def costmap_cell(params, curve, o, t, d):
    """(cost, why) of one cell with the occupancy byte o, the terrain byte t and the squared distance d under the CostmapParams
    `params` and the uint8 table `curve` (None without the inflation layer): pwpp_costmap_cell, the function the kernels use, on
    the host; needs no device."""
    L = load()
    cv = _curve(curve)
    c, w = ctypes.c_int32(0), ctypes.c_uint32(0)
    if L.pwpp_costmap_cell(ctypes.byref(params), _hp(cv), 0 if cv is None else len(cv), int(o), int(t), int(d), ctypes.byref(c), ctypes.byref(w)) < 0:
        raise PwppError("pwpp error: %s" % L.pwpp_last_error().decode())
    return c.value, w.value


def costmap_curve(cell, inscribed, radius, decay, peak, capacity=COSTMAP_MAX_CURVE):
    """The common inflation table for cells of `cell` metres (pwpp_costmap_curve): uint8 entries indexed by the squared distance in
    cells, 100 up to the inscribed radius, then floor(peak * exp(-decay * (distance - inscribed))) up to `radius`, all in metres;
    peak 0 .. 99.  Needs no device."""
    L = load()
    out = np.zeros(max(int(capacity), 1), np.uint8)
    n = L.pwpp_costmap_curve(float(cell), float(inscribed), float(radius), float(decay), int(peak), _vp(out), int(capacity))
    if n < 0:
        raise PwppError("pwpp error %d: %s" % (n, L.pwpp_last_error().decode()))
    return out[:n].copy()


def viewshed_units(metres):
    """A height in metres in the viewshed's units (pwpp_viewshed_units): VIEW_NO_HEIGHT for a NaN, otherwise
    floor(clamp(metres * 1024, -2^30, 2^30) + 0.5); needs no device."""
    return int(load().pwpp_viewshed_units(float(metres)))


def beam_height(eye, z, k, n):
    """The height, in the viewshed's units, at the crossed cell P_k (1 <= k < n) of a beam from an eye at `eye` into an endpoint n
    steps away whose lowest return is at z: pwpp_beam_height, the function the kernels use, on the host; needs no device."""
    L = load()
    v = int(L.pwpp_beam_height(int(eye), int(z), int(k), int(n)))
    if v == VIEW_NO_HEIGHT:
        raise PwppError("pwpp error: %s" % L.pwpp_last_error().decode())
    return v


def footprint_covers(foot_params, pose, ix, iy):
    """Whether the rectangle of the FootprintParams at the pose {px, py, ux, uy} covers cell (ix, iy): pwpp_footprint_covers, the rule
    the kernels use, on the host; needs no device."""
    L = load()
    q = (ctypes.c_int32 * 4)(*[int(v) for v in pose])
    rc = L.pwpp_footprint_covers(ctypes.byref(foot_params), q, int(ix), int(iy))
    if rc < 0:
        raise PwppError("pwpp error %d: %s" % (rc, L.pwpp_last_error().decode()))
    return bool(rc)


def footprint_pose(grid, x, y, yaw):
    """The pose {px, py, ux, uy} of a position in metres and a yaw in radians over the GroundGrid `grid` (pwpp_footprint_pose): ticks of
    1/16 cell from the grid's origin, floored, and the heading lround(1024 cos), lround(1024 sin).  A convenience; needs no device."""
    L = load()
    q = (ctypes.c_int32 * 4)()
    rc = L.pwpp_footprint_pose(ctypes.byref(grid), float(x), float(y), float(yaw), q)
    if rc < 0:
        raise PwppError("pwpp error %d: %s" % (rc, L.pwpp_last_error().decode()))
    return np.array(list(q), np.int32)


def evidence_verdict(rule, cells, landed, occupied, free):
    """The verdict (EVID_*) of a row with these counts under the rule (an EvidenceRule or its four values): pwpp_evidence_verdict,
    the function the kernels use, on the host; needs no device."""
    L = load()
    r = rule if isinstance(rule, EvidenceRule) else EvidenceRule(*[int(v) for v in rule])
    v = ctypes.c_int32(0)
    if L.pwpp_evidence_verdict(ctypes.byref(r), int(cells), int(landed), int(occupied), int(free), ctypes.byref(v)) < 0:
        raise PwppError(L.pwpp_last_error().decode())
    return int(v.value)


def pinned_empty(shape, dtype=np.float32):
    """A page-locked numpy array (pwpp_host_alloc); keep it alive while the GPU may touch it."""
    L = load()
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = ctypes.c_void_p()
    if L.pwpp_host_alloc(ctypes.byref(p), n) < 0:
        raise PwppError(L.pwpp_last_error().decode())
    buf = (ctypes.c_char * max(n, 1)).from_address(p.value)
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    _pinned_keep[arr.ctypes.data] = (p, buf)
    return arr


def pinned_free(arr):
    ent = _pinned_keep.pop(arr.ctypes.data, None)
    if ent:
        load().pwpp_host_free(ent[0])


_pinned_keep = {}


def default_params():
    p = Params()
    load().pwpp_params_default(ctypes.byref(p))
    return p


def match_pose(candidate, cell, sx, sy):
    """The candidate {a, b, tx, c, d, ty} moved by the winning shift of a scan match (pwpp_match_pose): tx + sx * cell and
    ty + sy * cell with the library's rounding, `cell` the MAP's cell size -- the pose to fuse under.  Host only."""
    cand = np.ascontiguousarray(np.asarray(candidate, np.float64).reshape(6))
    out = np.empty(6, np.float64)
    L = load()
    if L.pwpp_match_pose(_vp(cand), float(cell), int(sx), int(sy), _vp(out)) < 0:
        raise PwppError(L.pwpp_last_error().decode())
    return out


def yaw_candidates(pose, step, n):
    """(n, 6) candidate poses for a scan match: the prior `pose` first, then the prior turned by +step, -step, +2 step, -2 step ...
    radians about the frame's origin (the prior's matrix composed with the rotation; the translation stays).  Built in numpy: a
    convenience outside the library's contract."""
    a, b, tx, c, d, ty = (float(v) for v in np.asarray(pose, np.float64).reshape(6))
    out = np.empty((int(n), 6), np.float64)
    for i in range(int(n)):
        k = (i + 1) // 2 * (1 if i % 2 else -1)
        co, si = np.cos(k * float(step)), np.sin(k * float(step))
        out[i] = (a * co + b * si, b * co - a * si, tx, c * co + d * si, d * co - c * si, ty) if i else (a, b, tx, c, d, ty)
    return out


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _hp(a):
    """A host array, or None, as the library's pointer.  An empty array goes as a one-element dummy: the library is the one that
    names the bad argument."""
    if a is None:
        return None
    return _vp(a) if a.size else _vp(np.empty(1, a.dtype))


def _dp(address):
    """A device address as the library's pointer; 0: none."""
    return ctypes.c_void_p(address or None)


def _count_image(count):
    """(the (frames, ny, nx) int32 view, the shape as given) of a (frames, ny, nx) or (ny, nx) count image."""
    count = np.ascontiguousarray(count, np.int32)
    c3 = count.reshape((1,) + count.shape) if count.ndim == 2 else count
    if c3.ndim != 3:
        raise ValueError("count: a (frames, ny, nx) or (ny, nx) image expected")
    return c3, count.shape


def _occupancy_image(occupancy, grid):
    """(the (frames, ny, nx) int8 view, frames, its GroundGrid) of a (frames, ny, nx) or (ny, nx) occupancy image on the grid (x0, y0, cell)."""
    occ = np.ascontiguousarray(occupancy, np.int8)
    o3 = occ.reshape((1,) + occ.shape) if occ.ndim == 2 else occ
    if o3.ndim != 3:
        raise ValueError("occupancy: a (frames, ny, nx) or (ny, nx) image expected")
    return o3, o3.shape[0], GroundGrid(float(grid[0]), float(grid[1]), float(grid[2]), o3.shape[2], o3.shape[1], 0, 0)


def _maps_image(maps, fmap):
    """The (n_maps, NY, NX) int16 view of the (n_maps, NY, NX) or (NY, NX) maps the FusionMap `fmap` describes."""
    maps = np.ascontiguousarray(maps, np.int16)
    m3 = maps.reshape((1,) + maps.shape) if maps.ndim == 2 else maps
    if m3.ndim != 3 or m3.shape[1:] != (fmap.ny, fmap.nx):
        raise ValueError("maps: (n_maps, NY, NX) of the map description expected")
    return m3


def _host(a, dtype, *shape):  # a small host array the library reads, None staying None
    return None if a is None else np.ascontiguousarray(np.asarray(a, dtype).reshape(shape))


def _transforms(T):
    """(k, 12) float32 from (12,), (3, 4), (k, 12) or (k, 3, 4)."""
    T = np.asarray(T, dtype=np.float32)
    if T.shape in ((12,), (3, 4)):
        T = T.reshape(1, 12)
    elif (T.ndim == 2 and T.shape[1] == 12) or (T.ndim == 3 and T.shape[1:] == (3, 4)):
        T = T.reshape(T.shape[0], 12)
    else:
        raise ValueError("transforms of shape (12,), (3, 4), (k, 12) or (k, 3, 4) expected, got %s" % (T.shape,))
    return np.ascontiguousarray(T)


def transform_points(T, xyz):
    """pwpp_transform_points: xyz (m, 3) float32 through T = [R | t] ((12,) or (3, 4)) with the library's own rounding --
    fl(fl(fl(fl(r0 x) + fl(r1 y)) + fl(r2 z)) + t) per row.  Host only; no GPU needed."""
    T = _transforms(T)
    if T.shape[0] != 1:
        raise ValueError("one transform expected")
    xyz = np.ascontiguousarray(xyz, np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError("xyz: an (m, 3) array expected")
    out = np.empty_like(xyz)
    L = load()
    if L.pwpp_transform_points(_vp(T), _vp(xyz) if xyz.size else None, xyz.shape[0], _vp(out) if out.size else None) < 0:
        raise PwppError(L.pwpp_last_error().decode())
    return out


def box_points(x0, y0, cell, nx, ny, xyz, hgt, row, max_boxes):
    """pwpp_box_points: the (max_boxes,) rows (OBSTACLE_BOX_DTYPE) of pwpp_box_obstacles' arithmetic for a caller's own points --
    xyz (m, 3) float32, hgt (m,) float32 heights over ground, row (m,) int32.  Skipped: a row outside [0, max_boxes), a NaN hgt,
    a point outside the grid.  Host only; no GPU needed."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError("xyz: an (m, 3) array expected")
    hgt, row = np.ascontiguousarray(hgt, np.float32).reshape(-1), np.ascontiguousarray(row, np.int32).reshape(-1)
    if len(hgt) != len(xyz) or len(row) != len(xyz):
        raise ValueError("hgt and row: one value per point expected")
    g = GroundGrid(float(x0), float(y0), float(cell), int(nx), int(ny), 0, 0)
    boxes = np.zeros(max(int(max_boxes), 0), OBSTACLE_BOX_DTYPE)
    L = load()
    ptr = lambda a: _vp(a) if a.size else None
    if L.pwpp_box_points(ctypes.byref(g), ptr(xyz), ptr(hgt), ptr(row), len(xyz), ptr(boxes), int(max_boxes)) < 0:
        raise PwppError(L.pwpp_last_error().decode())
    return boxes


def hull_points(x0, y0, cell, nx, ny, xyz, row, max_hulls, max_vertices, with_vertices=True):
    """pwpp_hull_points: the (max_hulls,) rows (OBSTACLE_HULL_DTYPE) of pwpp_hull_obstacles' arithmetic for a caller's own points, and
    the (max_hulls, max_vertices, 2) int32 vertex lists (None without with_vertices: the library is given no list) -- xyz (m, 3)
    float32, row (m,) int32.  Skipped: a row outside [0, max_hulls), a NaN z, a point outside the grid.  Host only; no GPU needed."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError("xyz: an (m, 3) array expected")
    row = np.ascontiguousarray(row, np.int32).reshape(-1)
    if len(row) != len(xyz):
        raise ValueError("row: one value per point expected")
    g = GroundGrid(float(x0), float(y0), float(cell), int(nx), int(ny), 0, 0)
    hulls = np.zeros(max(int(max_hulls), 0), OBSTACLE_HULL_DTYPE)
    lists = np.zeros((max(int(max_hulls), 0), min(max(int(max_vertices), 0), HULL_VERTICES_MAX), 2), np.int32) if with_vertices else None
    L = load()
    ptr = lambda a: _vp(a) if a is not None and a.size else None
    if L.pwpp_hull_points(ctypes.byref(g), ptr(xyz), ptr(row), len(xyz), ptr(hulls), int(max_hulls), ptr(lists), int(max_vertices)) < 0:
        raise PwppError(L.pwpp_last_error().decode())
    return hulls, lists


def hull_vertex_xy(x0, y0, cell, nx, ny, q):
    """pwpp_hull_vertex_xy: the (..., 2) float64 metres of (..., 2) int32 hull vertices on the grid's 1/1024 m lattice.  Host only."""
    q = np.ascontiguousarray(q, np.int32)
    if q.shape[-1:] != (2,):
        raise ValueError("q: (..., 2) vertices expected")
    g = GroundGrid(float(x0), float(y0), float(cell), int(nx), int(ny), 0, 0)
    flat, out = q.reshape(-1, 2), np.zeros((q.size // 2, 2), np.float64)
    L = load()
    for k in range(len(flat)):
        pair = np.ascontiguousarray(flat[k])
        if L.pwpp_hull_vertex_xy(ctypes.byref(g), _vp(pair), _vp(out[k:k + 1])) < 0:
            raise PwppError(L.pwpp_last_error().decode())
    return out.reshape(q.shape)


class Handle:
    """One pwpp_handle: one device, one HIP stream, the workspace and the adaptive state."""

    def __init__(self, params=None, device=0):
        self._L = load()
        self.params = params if params is not None else default_params()
        h = ctypes.c_void_p()
        self._h = None
        self._check(self._L.pwpp_create(ctypes.byref(self.params), device, ctypes.byref(h)))
        self._h = h
        self._keep = None

    def _check(self, rc):
        if rc < 0:
            raise PwppError("pwpp error %d: %s" % (rc, self._L.pwpp_last_error().decode()))
        return rc

    def close(self):
        if self._h:
            if not getattr(self, "_borrowed", False):  # (a view of a Pipe's handle: the pipe destroys it)
                self._L.pwpp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the hot path -----------------------------------------------------------------
    def estimate_ground(self, pts):
        """Reference estimateGround(): one host frame, stateful (stream 0)."""
        pts = np.asarray(pts, dtype=np.float32)
        if pts.ndim != 2:
            raise PwppError("expected a 2-D array")
        if pts.flags["C_CONTIGUOUS"]:
            layout = LAYOUT_ROW_MAJOR
        elif pts.flags["F_CONTIGUOUS"]:
            layout = LAYOUT_COL_MAJOR
        else:
            pts = np.ascontiguousarray(pts)
            layout = LAYOUT_ROW_MAJOR
        self._check(self._L.pwpp_estimate_ground(self._h, _vp(pts), pts.shape[0], pts.shape[1], layout))

    def estimate_ground_batch(self, frames, mode=MODE_FRESH):
        """Host frames (list of (n,cols) float32 arrays, all C-contiguous or all Fortran-contiguous =
        Eigen::MatrixXf storage), synchronous."""
        col_major = all(f.dtype == np.float32 and f.flags["F_CONTIGUOUS"] and not f.flags["C_CONTIGUOUS"] for f in frames)
        if not col_major:
            frames = [np.ascontiguousarray(f, dtype=np.float32) for f in frames]
        cols = frames[0].shape[1]
        ptrs = (ctypes.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
        ns = (ctypes.c_int32 * len(frames))(*[f.shape[0] for f in frames])
        self._check(self._L.pwpp_estimate_ground_batch(self._h, ptrs, ns, len(frames), cols,
                                                       LAYOUT_COL_MAJOR if col_major else LAYOUT_ROW_MAJOR, MEM_HOST, mode))

    def submit_pinned_batch(self, frames, mode=MODE_FRESH):
        """Frames in page-locked host memory (pinned_empty): copies and launches are only enqueued;
        the arrays must stay untouched until synchronize() / a getter."""
        cols = frames[0].shape[1]
        ptrs = (ctypes.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
        ns = (ctypes.c_int32 * len(frames))(*[f.shape[0] for f in frames])
        self._keep = (ptrs, ns, frames)
        self._check(self._L.pwpp_estimate_ground_batch(self._h, ptrs, ns, len(frames), cols, LAYOUT_ROW_MAJOR,
                                                       MEM_HOST_PINNED, mode))

    def estimate_ground_batch_device(self, ptrs, ns, cols=4, layout=LAYOUT_ROW_MAJOR, mode=MODE_FRESH):
        """Device-resident frames: ptrs = device addresses (ints), asynchronous until synchronize()."""
        k = len(ptrs)
        cp = (ctypes.c_void_p * k)(*ptrs)
        cn = (ctypes.c_int32 * k)(*ns)
        self._keep = (cp, cn)
        self._check(self._L.pwpp_estimate_ground_batch(self._h, cp, cn, k, cols, layout, MEM_DEVICE, mode))

    def submit_batch(self, ptrs, ns, cols, layout, mem, mode=MODE_FRESH):
        """pwpp_estimate_ground_batch as it stands: frames by address (ints) in any layout and memory kind.  The memory must stay
        valid and unchanged until synchronize() unless mem is MEM_HOST."""
        k = len(ptrs)
        cp = (ctypes.c_void_p * k)(*ptrs)
        cn = (ctypes.c_int32 * k)(*ns)
        self._keep = (cp, cn)
        self._check(self._L.pwpp_estimate_ground_batch(self._h, cp, cn, k, cols, layout, mem, mode))

    def make_device_batch(self, ptrs, ns):
        """Pre-built ctypes argument arrays for repeated launches of the same batch."""
        k = len(ptrs)
        return (ctypes.c_void_p * k)(*ptrs), (ctypes.c_int32 * k)(*ns), k

    def launch_device_batch(self, batch, cols=4, layout=LAYOUT_ROW_MAJOR, mode=MODE_FRESH):
        cp, cn, k = batch
        self._check(self._L.pwpp_estimate_ground_batch(self._h, cp, cn, k, cols, layout, MEM_DEVICE, mode))

    def synchronize(self):
        self._check(self._L.pwpp_synchronize(self._h))

    def set_num_streams(self, n):
        self._check(self._L.pwpp_set_num_streams(self._h, n))

    # ---- results ----------------------------------------------------------------------
    def counts(self, frame=0):
        a, b, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.pwpp_get_counts(self._h, frame, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def _get(self, fn, frame, shape, dtype):
        out = np.zeros(shape, dtype)
        self._check(fn(self._h, frame, _vp(out) if out.size else None))
        return out

    def ground_indices(self, frame=0):
        return self._get(self._L.pwpp_get_ground_indices, frame, self.counts(frame)[0], np.int32)

    def nonground_indices(self, frame=0):
        return self._get(self._L.pwpp_get_nonground_indices, frame, self.counts(frame)[1], np.int32)

    def ground(self, frame=0):
        return self._get(self._L.pwpp_get_ground_xyz, frame, (self.counts(frame)[0], 3), np.float32)

    def nonground(self, frame=0):
        return self._get(self._L.pwpp_get_nonground_xyz, frame, (self.counts(frame)[1], 3), np.float32)

    def centers(self, frame=0):
        return self._get(self._L.pwpp_get_centers, frame, (self.counts(frame)[2], 3), np.float32)

    def normals(self, frame=0):
        return self._get(self._L.pwpp_get_normals, frame, (self.counts(frame)[2], 3), np.float32)

    def patch_records(self, frame=0):
        n = self.counts(frame)[2]
        out = np.zeros(max(n, 1), RECORD_DTYPE)
        k = self._check(self._L.pwpp_get_patch_records(self._h, frame, _vp(out), len(out)))
        return out[:k]

    def height(self):
        return self._L.pwpp_get_height(self._h)

    def time_us(self):
        return self._L.pwpp_get_time_us(self._h)

    def state(self, index=0):
        s = State()
        self._check(self._L.pwpp_get_state(self._h, index, ctypes.byref(s)))
        return s

    def set_state(self, stream, sensor_height, elevation_thr, flatness_thr):
        s = State()
        s.sensor_height = sensor_height
        for k in range(4):
            s.elevation_thr[k] = elevation_thr[k]
            s.flatness_thr[k] = flatness_thr[k]
        self._check(self._L.pwpp_set_state(self._h, stream, ctypes.byref(s)))

    def estimate_ground_fields(self, data, n, point_step, off_x, off_y, off_z, off_intensity=-1):
        """One frame handed over as a sensor_msgs/PointCloud2 data blob (bytes-like / uint8 array)."""
        buf = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data
        self._keep = buf
        self._check(self._L.pwpp_estimate_ground_fields(self._h, _vp(buf), n, point_step, off_x, off_y, off_z, off_intensity))

    def estimate_ground_fields_batch(self, datas, ns, point_step, off_x, off_y, off_z, off_intensity=-1, mem=MEM_HOST,
                                     mode=MODE_FRESH):
        """Many PointCloud2 data blobs in one call (pwpp_estimate_ground_fields_batch).  MEM_HOST / MEM_HOST_PINNED: `datas` are
        numpy byte buffers (pinned_empty for MEM_HOST_PINNED); MEM_DEVICE: device addresses (ints), as in
        estimate_ground_batch_device.  Asynchronous unless mem is MEM_HOST: synchronize() before reading results."""
        k = len(datas)
        if mem == MEM_DEVICE:
            addrs = [int(d) for d in datas]
        else:
            datas = [np.frombuffer(d, np.uint8) if not isinstance(d, np.ndarray) else d for d in datas]
            addrs = [d.ctypes.data for d in datas]
        cp = (ctypes.c_void_p * k)(*addrs)
        cn = (ctypes.c_int32 * k)(*ns)
        self._keep = (cp, cn, datas)
        self._check(self._L.pwpp_estimate_ground_fields_batch(self._h, cp, cn, k, point_step, off_x, off_y, off_z, off_intensity,
                                                              mem, mode))

    def set_history(self, stream, which, ring, values):
        v = np.ascontiguousarray(values, np.float64)
        self._check(self._L.pwpp_set_history(self._h, stream, which, ring, _vp(v) if v.size else None, int(v.size)))

    def checkpoint(self, stream=0):
        """Everything a stream carries from frame to frame (pwpp_get_state + the eight histories + the plane members)."""
        st = self.state(stream)
        return dict(sensor_height=st.sensor_height, elevation_thr=list(st.elevation_thr), flatness_thr=list(st.flatness_thr),
                    hist=[[self.history(stream, w, r) for r in range(4)] for w in range(2)], plane=self.plane_state(stream))

    def restore(self, ck, stream=0):
        self.set_state(stream, ck["sensor_height"], ck["elevation_thr"], ck["flatness_thr"])
        for w in range(2):
            for r in range(4):
                self.set_history(stream, w, r, ck["hist"][w][r])
        if "plane" in ck:
            self.set_plane_state(stream, ck["plane"])

    def clamped_frames(self):
        """Frames in which a patch's final ground set spanned more than z0 +- ZR vertically (pwpp_get_clamped_frames)."""
        return int(self._L.pwpp_get_clamped_frames(self._h))

    def fixed_up_frames(self):
        """Frames finished by the serial fix-up kernel so far (pwpp_get_fixed_up_frames)."""
        return int(self._L.pwpp_get_fixed_up_frames(self._h))

    def plane_state(self, index=0):
        """{mean[3], normal[3], singular values[3], d} of the plane the stream's last frame fitted last (pwpp_get_plane_state)."""
        out = np.zeros(10, np.float32)
        self._check(self._L.pwpp_get_plane_state(self._h, index, _vp(out)))
        return out

    def set_plane_state(self, stream, values):
        v = np.ascontiguousarray(values, np.float32)
        assert v.shape == (10,)
        self._check(self._L.pwpp_set_plane_state(self._h, stream, _vp(v)))

    def history(self, index, which, ring):
        n = self._check(self._L.pwpp_get_history(self._h, index, which, ring, None, 0))
        out = np.zeros(n, np.float64)
        if n:
            self._check(self._L.pwpp_get_history(self._h, index, which, ring, _vp(out), n))
        return out

    def device_view(self):
        v = DeviceView()
        self._check(self._L.pwpp_get_device_view(self._h, ctypes.byref(v)))
        return v

    def all_indices(self, out=None):
        """Every frame's ground + non-ground list in one device-to-host copy.

        Returns (indices, frame_base, counts): frame f's ground list is
        indices[frame_base[f] : frame_base[f] + counts[f, 0]], its non-ground list follows."""
        v = self.device_view()
        base = np.zeros(v.frames + 1, np.int64)
        counts = np.zeros((v.frames, 8), np.int32)
        total = int(np.ctypeslib.as_array(v.frame_base, shape=(v.frames + 1,))[-1])
        if out is None:
            out = np.empty(max(total, 1), np.int32)
        self._check(self._L.pwpp_get_all_indices(self._h, _vp(out), _vp(base), _vp(counts)))
        return out[:total], base, counts

    def all_counts(self):
        """(frames, 8) int32 array of per-frame counters of the last call."""
        v = self.device_view()
        return np.ctypeslib.as_array(v.counts, shape=(v.frames, 8)).copy()

    # ---- measurement --------------------------------------------------------------------
    def set_profiling(self, on):
        self._check(self._L.pwpp_set_profiling(self._h, 1 if on else 0))

    def reset_kernel_profile(self):
        self._check(self._L.pwpp_reset_kernel_profile(self._h))

    def kernel_profile(self):
        ms = np.zeros(NUM_KERNELS, np.float64)
        cnt = np.zeros(NUM_KERNELS, np.int64)
        self._check(self._L.pwpp_get_kernel_profile(self._h, _vp(ms), _vp(cnt)))
        return {self._L.pwpp_kernel_name(k).decode(): (float(ms[k]), int(cnt[k])) for k in range(NUM_KERNELS)}

    def fxp_shift(self):
        return self._L.pwpp_get_fxp_shift(self._h)

    def fxp_origins(self):
        """(B, 2) float32: the origin of every bin's fixed-point plane-fit sums."""
        nb = self._L.pwpp_get_fxp_origins(self._h, None, 0)  # size query
        self._check(nb)
        out = np.zeros((nb, 2), np.float32)
        b = self._L.pwpp_get_fxp_origins(self._h, _vp(out), out.shape[0])
        self._check(b)
        return out[:b].copy()

    def set_option(self, name, value):
        """Tuning / test switches (pwpp_set_option): fit_plan, one_pass, exact_moments, split_k5, redo_whole_batch,
        one_pass_min_frames, one_pass_scale, fit_streams, overlap_ranges, hi_split, hi_split_zones, records_path, debug_flags.
        None of them changes a result except exact_moments (include/pwpp.h)."""
        self._check(self._L.pwpp_set_option(self._h, name.encode(), str(value).encode()))

    def workspace_bytes(self):
        return int(self._L.pwpp_get_workspace_bytes(self._h))

    def trim_workspace(self):
        """Free the per-batch workspaces (results of the last call are gone afterwards)."""
        self._check(self._L.pwpp_trim_workspace(self._h))

    def set_output_order(self, reference):
        """True: the points of a patch come out in the reference's order (z-sorted bins); False: scatter order."""
        self._check(self._L.pwpp_set_output_order(self._h, 1 if reference else 0))

    def set_order(self, order):
        """ORDER_SCATTER (default), ORDER_REFERENCE or ORDER_CLOUD (both lists in ascending cloud index; implies labels)."""
        self._check(self._L.pwpp_set_output_order(self._h, int(order)))

    def set_labels(self, on):
        """True: the batches launched afterwards also write one LABEL_* byte per point (cloud order)."""
        self._check(self._L.pwpp_set_labels(self._h, 1 if on else 0))

    def labels(self, frame=0):
        """(n,) uint8 LABEL_* of the frame's points, in cloud order."""
        base = self.frame_base()
        n = int(base[frame + 1] - base[frame]) if 0 <= frame < len(base) - 1 else 0
        out = np.empty(max(n, 1), np.uint8)
        self._check(self._L.pwpp_get_labels(self._h, frame, _vp(out)))
        return out[:n]

    def all_labels(self, out=None):
        """Every frame's labels in one device-to-host copy: (labels, frame_base), frame f at labels[frame_base[f]:frame_base[f + 1]]."""
        base = self.frame_base()
        total = int(base[-1])
        if out is None:
            out = np.empty(max(total, 1), np.uint8)
        self._check(self._L.pwpp_get_all_labels(self._h, _vp(out)))
        return out[:total], base

    def device_labels(self):
        """Device address of the last call's labels (frame f at frame_base[f] of device_view())."""
        p = ctypes.c_void_p()
        self._check(self._L.pwpp_get_device_labels(self._h, ctypes.byref(p)))
        return int(p.value or 0)

    def set_point_planes(self, on):
        """True: the batches launched afterwards also write, per point, the row of its patch and its signed distance to the
        patch's plane (cloud order; include/pwpp.h)."""
        self._check(self._L.pwpp_set_point_planes(self._h, 1 if on else 0))

    def _point_frame(self, fn, frame, dtype):
        base = self.frame_base()
        n = int(base[frame + 1] - base[frame]) if 0 <= frame < len(base) - 1 else 0
        out = np.empty(max(n, 1), dtype)
        self._check(fn(self._h, frame, _vp(out)))
        return out[:n]

    def _point_batch(self, fn, out, dtype):
        base = self.frame_base()
        total = int(base[-1])
        if out is None:
            out = np.empty(max(total, 1), dtype)
        if out.dtype != dtype or not out.flags.c_contiguous or out.size < total:
            raise ValueError("out: a contiguous %s array of at least %d entries expected" % (np.dtype(dtype).name, total))
        self._check(fn(self._h, _vp(out)))
        return out[:total], base

    def point_patches(self, frame=0):
        """(n,) int32: the row of every point's patch in patch_records / centers / normals of the frame, -1 = none."""
        return self._point_frame(self._L.pwpp_get_point_patches, frame, np.int32)

    def point_distances(self, frame=0):
        """(n,) float32: every point's signed distance to its patch's plane, NaN where point_patches is -1."""
        return self._point_frame(self._L.pwpp_get_point_distances, frame, np.float32)

    def all_point_patches(self, out=None):
        """Every frame's point_patches in one device-to-host copy: (patches, frame_base)."""
        return self._point_batch(self._L.pwpp_get_all_point_patches, out, np.int32)

    def all_point_distances(self, out=None):
        """Every frame's point_distances in one device-to-host copy: (distances, frame_base)."""
        return self._point_batch(self._L.pwpp_get_all_point_distances, out, np.float32)

    def device_point_planes(self):
        """Device addresses (patches, distances) of the last call's point planes (frame f at frame_base[f])."""
        p, d = ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._L.pwpp_get_device_point_planes(self._h, ctypes.byref(p), ctypes.byref(d)))
        return int(p.value or 0), int(d.value or 0)

    def set_point_records(self, on):
        """True: the batches launched afterwards also write the whole records of their ground / non-ground points on the
        device, row for row behind the index lists (include/pwpp.h)."""
        self._check(self._L.pwpp_set_point_records(self._h, 1 if on else 0))

    def set_input_transforms(self, T):
        """An affine transform [R | t] per frame, applied to the input while it is binned (include/pwpp.h): T of shape (12,) or
        (3, 4) applies to every frame of every later call, (k, 12) or (k, 3, 4) gives frame (stream) i its own and needs calls
        of exactly k frames.  None turns it off.  Copied here; sticky."""
        if T is None:
            self._check(self._L.pwpp_set_input_transforms(self._h, None, 0))
            return
        T = _transforms(T)
        self._check(self._L.pwpp_set_input_transforms(self._h, _vp(T) if T.size else None, T.shape[0]))

    @property
    def record_bytes(self):
        """Bytes per row of the last call's records: cols * 4 for a matrix, point_step for a fields layout."""
        return self._check(self._L.pwpp_get_record_bytes(self._h))

    def _records(self, fn, frame, which):
        rb = self.record_bytes
        cnt = ctypes.c_int32(0)
        args = [None, None, None]
        args[which] = ctypes.byref(cnt)
        self._check(self._L.pwpp_get_counts(self._h, frame, *args))
        out = np.empty((max(cnt.value, 1), rb), np.uint8)
        self._check(fn(self._h, frame, _vp(out)))
        return out[:cnt.value]

    def ground_records(self, frame=0):
        """(n_ground, record_bytes) uint8: the records of the frame's ground points, rows aligned with ground_indices."""
        return self._records(self._L.pwpp_get_ground_records, frame, 0)

    def nonground_records(self, frame=0):
        """(n_nonground, record_bytes) uint8: the records of the frame's non-ground points, rows aligned with nonground_indices."""
        return self._records(self._L.pwpp_get_nonground_records, frame, 1)

    def all_records(self, out=None):
        """Every frame's records in one device-to-host copy: (records (total, record_bytes) uint8, frame_base, counts).  Frame
        f's ground rows start at frame_base[f], its non-ground rows follow; needs a call that ran with set_point_records(True)."""
        rb = self.record_bytes
        v = self.device_view()
        base = np.zeros(v.frames + 1, np.int64)
        counts = np.zeros((v.frames, 8), np.int32)
        total = int(np.ctypeslib.as_array(v.frame_base, shape=(v.frames + 1,))[-1])
        if out is None:
            out = np.empty((max(total, 1), rb), np.uint8)
        if out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < total * rb:
            raise ValueError("out: a contiguous uint8 array of at least %d bytes expected" % (total * rb))
        self._check(self._L.pwpp_get_all_records(self._h, _vp(out), _vp(base), _vp(counts)))
        return out.reshape(-1)[:total * rb].reshape(total, rb), base, counts

    def device_records(self):
        """(device address, record_bytes) of the last call's records (frame f at row frame_base[f])."""
        p, rb = ctypes.c_void_p(), ctypes.c_int32(0)
        self._check(self._L.pwpp_get_device_records(self._h, ctypes.byref(p), ctypes.byref(rb)))
        return int(p.value or 0), int(rb.value)

    def query_ground(self, xyz, frames=None):
        """The last call's ground model at arbitrary positions: xyz (m, 3) float32, frames None (frame 0), an int or (m,) int32.
        Returns a structured (m,) array with the fields patch, decision, ground_z, distance (include/pwpp.h)."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        m = xyz.shape[0]
        fr = None
        if frames is not None:
            fr = np.ascontiguousarray(np.broadcast_to(np.asarray(frames, np.int32), (m,)))
        out = np.empty(max(m, 1), GROUND_SAMPLE_DTYPE)
        self._check(self._L.pwpp_query_ground(self._h, _vp(xyz), _vp(fr) if fr is not None else None, m, MEM_HOST, _vp(out)))
        return out[:m]

    def query_ground_device(self, xyz_ptr, frames_ptr, m, out_ptr):
        """query_ground on device memory: addresses of (m, 3) float32 positions, m int32 frames (0 / None: frame 0) and m
        16-byte samples.  Enqueued on the handle's stream; complete after synchronize()."""
        self._check(self._L.pwpp_query_ground(self._h, _dp(xyz_ptr), _dp(frames_ptr), int(m), MEM_DEVICE, _dp(out_ptr)))

    def _grid(self, x0, y0, cell, nx, ny, frame_first, frames, ground_only):
        if frames is None:
            frames = self.device_view().frames - frame_first
        return GroundGrid(float(x0), float(y0), float(cell), int(nx), int(ny), GRID_GROUND_ONLY if ground_only else 0, 0), int(frames)

    def _look(self, x0, y0, cell, nx, ny, frame_first, frames, ground_only, origin_xy):  # _grid, and the (n_origins, 2) float64 positions of the sensor
        return self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only) + (_host(origin_xy, np.float64, -1, 2),)

    @staticmethod
    def _grid_shape(g, frames):
        """The shape of the images of a call over frames of the grid g; a bad argument, left to the library to name, counts as 0."""
        return (max(frames, 0), max(g.ny, 0), max(g.nx, 0))

    def rasterize_ground(self, x0, y0, cell, nx, ny, frame_first=0, frames=None, ground_only=False, with_patches=False):
        """The last call's ground model as an elevation image: (frames, ny, nx) float32 heights of the cell centres
        (x0 + (ix + 0.5) cell, y0 + (iy + 0.5) cell), NaN where no patch answers; with_patches: also the int32 patch rows.
        ground_only: NaN too where the patch was decided not_upright, heading or tgr_reject."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        shape = self._grid_shape(g, frames)
        height = np.empty(shape, np.float32)
        patch = np.empty(shape, np.int32) if with_patches else None
        self._check(self._L.pwpp_rasterize_ground(self._h, ctypes.byref(g), int(frame_first), frames, MEM_HOST, _hp(height),
                                                  _vp(patch) if with_patches and patch.size else None))
        return (height, patch) if with_patches else height

    def rasterize_ground_device(self, x0, y0, cell, nx, ny, height_ptr, patch_ptr=0, frame_first=0, frames=None, ground_only=False):
        """rasterize_ground into device memory: addresses of the (frames, ny, nx) float32 image and (0: none) the int32 one.
        Enqueued on the handle's stream; complete after synchronize()."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        self._check(self._L.pwpp_rasterize_ground(self._h, ctypes.byref(g), int(frame_first), frames, MEM_DEVICE, _dp(height_ptr), _dp(patch_ptr)))

    def rasterize_obstacles(self, x0, y0, cell, nx, ny, h_min, h_max, frame_first=0, frames=None, ground_only=False, want_top=True,
                            want_unref=False):
        """The last call's non-ground points on the grid of rasterize_ground: (frames, ny, nx) int32 counts of the points whose
        height over their patch's plane lies in [h_min, h_max]; want_top: also the float32 largest such height (NaN where the
        count is 0); want_unref: also the int32 counts of the points without a ground reference (include/pwpp.h;
        ground_only: patches decided not_upright, heading or tgr_reject give no reference either).
        Returns count, or the tuple (count[, top][, unref])."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        shape = self._grid_shape(g, frames)
        count = np.empty(shape, np.int32)
        top = np.empty(shape, np.float32) if want_top else None
        unref = np.empty(shape, np.int32) if want_unref else None
        self._check(self._L.pwpp_rasterize_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(frame_first), frames, MEM_HOST,
                                                     _hp(count), _hp(top), _hp(unref)))
        out = tuple(a for a in (count, top, unref) if a is not None)
        return out if len(out) > 1 else count

    def rasterize_obstacles_device(self, x0, y0, cell, nx, ny, h_min, h_max, count_ptr, top_ptr=0, unref_ptr=0, frame_first=0, frames=None,
                                   ground_only=False):
        """rasterize_obstacles into device memory: addresses of the (frames, ny, nx) int32 count image and (0: none) the float32
        top and int32 unref images.  Enqueued on the handle's stream; complete after synchronize()."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        self._check(self._L.pwpp_rasterize_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(frame_first), frames, MEM_DEVICE,
                                                     _dp(count_ptr), _dp(top_ptr), _dp(unref_ptr)))

    def label_grid(self, count, top=None, min_count=1, connectivity=8, max_clusters=0):
        """Connected clusters of the occupied cells (count >= min_count) of a (frames, ny, nx) or (ny, nx) int32 count image, each
        frame on its own; top: the float32 image of the same shape whose maximum the table reports, or None.  Works before any
        estimate call.  Returns (label, clusters, n_clusters): int32 labels of count's shape (-1: unoccupied, else the cluster's
        rank in ascending first_cell), the (frames, max_clusters) structured table (OBSTACLE_CLUSTER_DTYPE; rows beyond
        min(n, max_clusters) unspecified) and the (frames,) int32 true numbers of clusters (include/pwpp.h)."""
        c3, shape = _count_image(count)
        if top is not None:
            top = np.ascontiguousarray(top, np.float32)
            if top.shape != shape:
                raise ValueError("top: the shape of count expected")
        frames, ny, nx = c3.shape
        label = np.empty(c3.shape, np.int32)
        table = np.zeros((max(frames, 0), max(int(max_clusters), 0)), OBSTACLE_CLUSTER_DTYPE)
        n = np.zeros(max(frames, 1), np.int32)
        self._check(self._L.pwpp_label_grid(self._h, nx, ny, frames, MEM_HOST, _hp(c3), _hp(top), int(min_count), int(connectivity), _hp(label),
                                            _vp(table) if table.size else None, _vp(n), int(max_clusters)))
        return label.reshape(shape), table, n[:frames]

    def label_grid_device(self, nx, ny, frames, count_ptr, top_ptr, min_count, connectivity, label_ptr, clusters_ptr=0, n_clusters_ptr=0,
                          max_clusters=0):
        """label_grid on device memory: addresses of the (frames, ny, nx) int32 count, float32 top (0: none) and int32 label
        images, the (frames, max_clusters) table of 48-byte rows (8-byte aligned; 0: none) and the (frames,) int32 counts
        (0: none).  Enqueued on the handle's stream; complete after synchronize()."""
        self._check(self._L.pwpp_label_grid(self._h, int(nx), int(ny), int(frames), MEM_DEVICE, _dp(count_ptr), _dp(top_ptr), int(min_count),
                                            int(connectivity), _dp(label_ptr), _dp(clusters_ptr), _dp(n_clusters_ptr), int(max_clusters)))

    def label_obstacles(self, x0, y0, cell, nx, ny, h_min, h_max, min_count=1, connectivity=8, max_clusters=0, frame_first=0, frames=None,
                        ground_only=False, want_images=False, want_point_cluster=False):
        """rasterize_obstacles and label_grid in one call, for frames of the last estimate call.  Returns (label, clusters,
        n_clusters) as label_grid does for the (frames, ny, nx) images; want_images: then the int32 count and float32 top images
        of rasterize_obstacles; want_point_cluster: then one int32 per point of the frame range in cloud order (frame f at
        frame_base()[f] - frame_base()[frame_first]): the label of the point's cell if the obstacle grid counted the point, else -1."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        shape = self._grid_shape(g, frames)
        label = np.empty(shape, np.int32)
        count = np.empty(shape, np.int32) if want_images else None
        top = np.empty(shape, np.float32) if want_images else None
        table = np.zeros((shape[0], max(int(max_clusters), 0)), OBSTACLE_CLUSTER_DTYPE)
        n = np.zeros(max(frames, 1), np.int32)
        pc = None
        if want_point_cluster:
            base = self.frame_base()
            last = min(max(int(frame_first) + frames, 0), len(base) - 1)
            first = min(max(int(frame_first), 0), last)
            pc = np.empty(int(base[last] - base[first]), np.int32)
        self._check(self._L.pwpp_label_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(min_count), int(connectivity),
                                                 int(frame_first), frames, MEM_HOST, _hp(label), _hp(count), _hp(top),
                                                 _vp(table) if table.size else None, _vp(n), int(max_clusters), _hp(pc)))
        out = (label, table, n[:max(frames, 0)])
        if want_images:
            out += (count, top)
        if want_point_cluster:
            out += (pc,)
        return out

    def label_obstacles_device(self, x0, y0, cell, nx, ny, h_min, h_max, min_count, connectivity, label_ptr, count_ptr=0, top_ptr=0,
                               clusters_ptr=0, n_clusters_ptr=0, max_clusters=0, point_cluster_ptr=0, frame_first=0, frames=None, ground_only=False):
        """label_obstacles into device memory: addresses as in label_grid_device and rasterize_obstacles_device (0: not wanted),
        point_cluster_ptr: one int32 per point of the frame range.  Enqueued on the handle's stream; complete after synchronize()."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        self._check(self._L.pwpp_label_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(min_count), int(connectivity),
                                                 int(frame_first), frames, MEM_DEVICE, _dp(label_ptr), _dp(count_ptr), _dp(top_ptr),
                                                 _dp(clusters_ptr), _dp(n_clusters_ptr), int(max_clusters), _dp(point_cluster_ptr)))

    @staticmethod
    def _label_images(label, what):
        """The (frames, ny, nx) int32 view of a (frames, ny, nx) or (ny, nx) label image."""
        lab = np.ascontiguousarray(label, np.int32)
        l3 = lab.reshape((1,) + lab.shape) if lab.ndim == 2 else lab
        if l3.ndim != 3:
            raise ValueError("%s: a (frames, ny, nx) or (ny, nx) label image expected" % what)
        return l3

    @staticmethod
    def _id_arrays(frames, rows, id_prev, next_id):
        """(id_prev, next_id, id_curr, next_id_out) as the library takes them: four host arrays, or four times None without id_prev."""
        if id_prev is None and next_id is None:
            return None, None, None, None
        ip = np.asarray(-1 if id_prev is None else id_prev, np.int32)
        ip = np.ascontiguousarray(np.broadcast_to(ip, (frames, rows)) if ip.ndim == 0 else ip)
        if ip.shape != (frames, rows):
            raise ValueError("id_prev: (frames, max_rows) expected")
        nx = np.ascontiguousarray(np.broadcast_to(np.asarray(0 if next_id is None else next_id, np.int32), (frames,)), np.int32)
        return ip, nx, np.empty((frames, rows), np.int32), np.empty(frames, np.int32)

    def associate_grid(self, curr, prev, pose, grid_curr, grid_prev=None, gate=0, min_overlap=1, max_rows=1, max_pairs=1, id_prev=None, next_id=None,
                       want_n_pairs=True):
        """Which row of the (frames, ny, nx) or (ny, nx) int32 label images `curr` is which row of `prev`: grid_curr and grid_prev
        (None: the same) are (x0, y0, cell) of the two grids, whose sides are the images'; pose: {a, b, tx, c, d, ty} for every
        frame or (frames, 6), where a position of the previous frame lies in the current one.  Works before any estimate call.
        Returns (curr_links, prev_links, n_pairs): two (frames, max_rows) tables of CLUSTER_LINK_DTYPE and the (frames,) int32
        numbers of pairs (None when not wanted); with id_prev ((frames, max_rows) int32, or one value for all) and next_id ((frames,)
        or one value) also (id_curr, next_id_out).  The rules: include/pwpp.h."""
        c3, p3 = self._label_images(curr, "curr"), self._label_images(prev, "prev")
        frames = c3.shape[0]
        gc = GroundGrid(float(grid_curr[0]), float(grid_curr[1]), float(grid_curr[2]), c3.shape[2], c3.shape[1], 0, 0)
        gq = grid_curr if grid_prev is None else grid_prev
        gp = GroundGrid(float(gq[0]), float(gq[1]), float(gq[2]), p3.shape[2], p3.shape[1], 0, 0)
        poses = _host(pose, np.float64, -1, 6)
        rows = max(int(max_rows), 0)
        cl, pl = np.zeros((frames, rows), CLUSTER_LINK_DTYPE), np.zeros((frames, rows), CLUSTER_LINK_DTYPE)
        n = np.zeros(max(frames, 1), np.int32) if want_n_pairs else None
        ip, nxt, ic, nout = self._id_arrays(frames, rows, id_prev, next_id)
        self._check(self._L.pwpp_associate_grid(self._h, ctypes.byref(gc), ctypes.byref(gp), frames, MEM_HOST, _hp(c3), _hp(p3), _hp(poses), len(poses),
                                                int(gate), int(min_overlap), int(max_rows), int(max_pairs), _hp(cl), _hp(pl), _hp(n), _hp(ip), _hp(nxt),
                                                _hp(ic), _hp(nout)))
        out = (cl, pl, n[:frames] if want_n_pairs else None)
        return out + (ic, nout) if ip is not None else out

    def associate_grid_device(self, grid_curr, grid_prev, frames, curr_ptr, prev_ptr, pose, gate, min_overlap, max_rows, max_pairs, curr_links_ptr,
                              prev_links_ptr, n_pairs_ptr=0, id_prev_ptr=0, next_id_ptr=0, id_curr_ptr=0, next_id_out_ptr=0):
        """associate_grid on device memory: grid_curr and grid_prev are (x0, y0, cell, nx, ny); addresses of the int32 label images,
        the two (frames, max_rows) tables of 16-byte rows, the (frames,) int32 pair counts (0: none) and the four id arrays (all or
        0), every one 4-byte aligned; pose stays a host array.  Enqueued on the handle's stream; complete after synchronize()."""
        gc = GroundGrid(float(grid_curr[0]), float(grid_curr[1]), float(grid_curr[2]), int(grid_curr[3]), int(grid_curr[4]), 0, 0)
        gp = GroundGrid(float(grid_prev[0]), float(grid_prev[1]), float(grid_prev[2]), int(grid_prev[3]), int(grid_prev[4]), 0, 0)
        poses = _host(pose, np.float64, -1, 6)
        self._check(self._L.pwpp_associate_grid(self._h, ctypes.byref(gc), ctypes.byref(gp), int(frames), MEM_DEVICE, _dp(curr_ptr), _dp(prev_ptr),
                                                _vp(poses) if poses.size else None, len(poses), int(gate), int(min_overlap), int(max_rows), int(max_pairs),
                                                _dp(curr_links_ptr), _dp(prev_links_ptr), _dp(n_pairs_ptr), _dp(id_prev_ptr), _dp(next_id_ptr),
                                                _dp(id_curr_ptr), _dp(next_id_out_ptr)))

    def track_obstacles(self, x0, y0, cell, nx, ny, h_min, h_max, prev_label, pose=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0), min_count=1, connectivity=8,
                        max_clusters=1, gate=0, min_overlap=1, max_pairs=1, id_prev=None, next_id=None, frame_first=0, frames=None):
        """label_obstacles and associate_grid of its label image against the (frames, ny, nx) int32 `prev_label` on the same grid in
        one call, for frames of the last estimate call; max_rows is max_clusters.  Returns (label, clusters, n_clusters, curr_links,
        prev_links, n_pairs) and, with id_prev and next_id, (id_curr, next_id_out): feed label, id_curr and next_id_out back as
        prev_label, id_prev and next_id of the next step."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, False)
        shape = self._grid_shape(g, frames)
        label = np.empty(shape, np.int32)
        prev = np.ascontiguousarray(prev_label, np.int32)
        if prev.size != label.size:
            raise ValueError("prev_label: (frames, ny, nx) expected")
        rows = max(int(max_clusters), 0)
        table = np.zeros((shape[0], rows), OBSTACLE_CLUSTER_DTYPE)
        n = np.zeros(max(frames, 1), np.int32)
        poses = _host(pose, np.float64, -1, 6)
        cl, pl = np.zeros((shape[0], rows), CLUSTER_LINK_DTYPE), np.zeros((shape[0], rows), CLUSTER_LINK_DTYPE)
        n_pairs = np.zeros(max(frames, 1), np.int32)
        ip, nxt, ic, nout = self._id_arrays(shape[0], rows, id_prev, next_id)
        self._check(self._L.pwpp_track_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(min_count), int(connectivity), int(frame_first),
                                                 frames, MEM_HOST, _hp(label), None, None, _vp(table) if table.size else None, _vp(n), int(max_clusters), None,
                                                 _hp(prev), _hp(poses), len(poses), int(gate), int(min_overlap), int(max_pairs), _hp(cl), _hp(pl),
                                                 _hp(n_pairs), _hp(ip), _hp(nxt), _hp(ic), _hp(nout)))
        out = (label, table, n[:shape[0]], cl, pl, n_pairs[:shape[0]])
        return out + (ic, nout) if ip is not None else out

    def track_obstacles_device(self, x0, y0, cell, nx, ny, h_min, h_max, min_count, connectivity, label_ptr, prev_label_ptr, pose, gate, min_overlap,
                               max_clusters, max_pairs, curr_links_ptr, prev_links_ptr, n_pairs_ptr=0, id_prev_ptr=0, next_id_ptr=0, id_curr_ptr=0,
                               next_id_out_ptr=0, count_ptr=0, top_ptr=0, clusters_ptr=0, n_clusters_ptr=0, point_cluster_ptr=0, frame_first=0, frames=None):
        """track_obstacles into device memory: addresses as in label_obstacles_device and associate_grid_device; pose stays a host
        array.  Enqueued on the handle's stream; complete after synchronize()."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, False)
        poses = _host(pose, np.float64, -1, 6)
        self._check(self._L.pwpp_track_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(min_count), int(connectivity), int(frame_first),
                                                 frames, MEM_DEVICE, _dp(label_ptr), _dp(count_ptr), _dp(top_ptr), _dp(clusters_ptr), _dp(n_clusters_ptr),
                                                 int(max_clusters), _dp(point_cluster_ptr), _dp(prev_label_ptr), _vp(poses) if poses.size else None, len(poses),
                                                 int(gate), int(min_overlap), int(max_pairs), _dp(curr_links_ptr), _dp(prev_links_ptr), _dp(n_pairs_ptr),
                                                 _dp(id_prev_ptr), _dp(next_id_ptr), _dp(id_curr_ptr), _dp(next_id_out_ptr)))

    @staticmethod
    def evidence_verdict(rule, cells, landed, occupied, free):
        """The module's evidence_verdict: the verdict of a row with these counts, on the host."""
        return evidence_verdict(rule, cells, landed, occupied, free)

    @staticmethod
    def _evidence_rule(rule):
        """An EvidenceRule from one, or from (gate, min_cells, moving_share, static_share)."""
        return rule if isinstance(rule, EvidenceRule) else EvidenceRule(*[int(v) for v in rule])

    def evidence_grid(self, label, grid, pose, fmap, maps, rule, max_rows, occupancy=None, map_of_frame=None, want_class=False, in_place=False):
        """What the (n_maps, NY, NX) or (NY, NX) int16 log-odds maps described by the FusionMap `fmap` hold under every row of the
        (frames, ny, nx) or (ny, nx) int32 label images on the grid `grid` = (x0, y0, cell): pose is {a, b, tx, c, d, ty} for
        every frame or (frames, 6), map-from-frame as in fuse_grid; rule an EvidenceRule or (gate, min_cells, moving_share,
        static_share); map_of_frame as in fuse_grid.  Works before any estimate call.  Returns the (frames, max_rows)
        CLUSTER_EVIDENCE_DTYPE rows; with want_class then the int8 class image; with occupancy (int8, the images' shape) then the
        masked bytes -- written over a copy of `occupancy` itself with in_place.  The rules: include/pwpp.h."""
        l3 = self._label_images(label, "label")
        frames = l3.shape[0]
        g = GroundGrid(float(grid[0]), float(grid[1]), float(grid[2]), l3.shape[2], l3.shape[1], 0, 0)
        m3 = _maps_image(maps, fmap)
        poses, mof = _host(pose, np.float64, -1, 6), _host(map_of_frame, np.int32, -1)
        r = self._evidence_rule(rule)
        rows = np.zeros((frames, max(int(max_rows), 0)), CLUSTER_EVIDENCE_DTYPE)
        cls = np.empty(l3.shape, np.int8) if want_class else None
        occ_in = occ_out = None
        if occupancy is not None:
            occ_in = np.array(occupancy, np.int8).reshape(l3.shape)
            occ_out = occ_in if in_place else np.empty(l3.shape, np.int8)
        self._check(self._L.pwpp_evidence_grid(self._h, ctypes.byref(g), frames, MEM_HOST, _hp(l3), _hp(occ_in), _hp(poses), len(poses), _hp(mof), ctypes.byref(fmap),
                                               m3.shape[0], _hp(m3), ctypes.byref(r), int(max_rows), _vp(rows) if rows.size else None, _hp(cls), _hp(occ_out)))
        out = (rows,) + ((cls,) if want_class else ()) + ((occ_out,) if occupancy is not None else ())
        return out if len(out) > 1 else rows

    def evidence_grid_device(self, grid, nx, ny, frames, label_ptr, pose, fmap, n_maps, map_ptr, rule, max_rows, rows_ptr, class_ptr=0, occupancy_in_ptr=0,
                             occupancy_out_ptr=0, map_of_frame=None):
        """evidence_grid on device memory: addresses of the (frames, ny, nx) int32 label images (4-byte aligned), the (n_maps, NY, NX)
        int16 maps (2-byte aligned), the (frames, max_rows) rows of 32 bytes (8-byte aligned) and (0: not wanted) the int8 class
        image and the two int8 occupancy images, which may be one address; pose and map_of_frame stay host arrays.  Enqueued on
        the handle's stream; complete after synchronize()."""
        g = GroundGrid(float(grid[0]), float(grid[1]), float(grid[2]), int(nx), int(ny), 0, 0)
        poses, mof = _host(pose, np.float64, -1, 6), _host(map_of_frame, np.int32, -1)
        r = self._evidence_rule(rule)
        self._check(self._L.pwpp_evidence_grid(self._h, ctypes.byref(g), int(frames), MEM_DEVICE, _dp(label_ptr), _dp(occupancy_in_ptr),
                                               _vp(poses) if poses.size else None, len(poses), _hp(mof), ctypes.byref(fmap), int(n_maps), _dp(map_ptr), ctypes.byref(r),
                                               int(max_rows), _dp(rows_ptr), _dp(class_ptr), _dp(occupancy_out_ptr)))

    def evidence_obstacles(self, x0, y0, cell, nx, ny, h_min, h_max, fmap, maps, rule, pose=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0), min_count=1, connectivity=8,
                           max_clusters=1, occupancy=None, map_of_frame=None, want_class=False, frame_first=0, frames=None):
        """label_obstacles and evidence_grid of its label image in one call, for frames of the last estimate call; max_rows is
        max_clusters.  Returns (label, clusters, n_clusters, rows), then the class image with want_class, then the masked bytes
        with occupancy."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, False)
        shape = self._grid_shape(g, frames)
        label = np.empty(shape, np.int32)
        table = np.zeros((shape[0], max(int(max_clusters), 0)), OBSTACLE_CLUSTER_DTYPE)
        n = np.zeros(max(frames, 1), np.int32)
        m3 = _maps_image(maps, fmap)
        poses, mof = _host(pose, np.float64, -1, 6), _host(map_of_frame, np.int32, -1)
        r = self._evidence_rule(rule)
        rows = np.zeros((shape[0], max(int(max_clusters), 0)), CLUSTER_EVIDENCE_DTYPE)
        cls = np.empty(shape, np.int8) if want_class else None
        occ_in = None if occupancy is None else np.ascontiguousarray(occupancy, np.int8).reshape(shape)
        occ_out = None if occupancy is None else np.empty(shape, np.int8)
        self._check(self._L.pwpp_evidence_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(min_count), int(connectivity), int(frame_first), frames,
                                                    MEM_HOST, _hp(label), None, None, _vp(table) if table.size else None, _vp(n), int(max_clusters), None,
                                                    _hp(occ_in), _hp(poses), len(poses), _hp(mof), ctypes.byref(fmap), m3.shape[0], _hp(m3), ctypes.byref(r),
                                                    _vp(rows) if rows.size else None, _hp(cls), _hp(occ_out)))
        return (label, table, n[:shape[0]], rows) + ((cls,) if want_class else ()) + ((occ_out,) if occupancy is not None else ())

    def evidence_obstacles_device(self, x0, y0, cell, nx, ny, h_min, h_max, min_count, connectivity, label_ptr, pose, fmap, n_maps, map_ptr, rule, max_clusters,
                                  rows_ptr, class_ptr=0, occupancy_in_ptr=0, occupancy_out_ptr=0, count_ptr=0, top_ptr=0, clusters_ptr=0, n_clusters_ptr=0,
                                  point_cluster_ptr=0, map_of_frame=None, frame_first=0, frames=None):
        """evidence_obstacles into device memory: addresses as in label_obstacles_device and evidence_grid_device; pose and
        map_of_frame stay host arrays.  Enqueued on the handle's stream; complete after synchronize()."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, False)
        poses, mof = _host(pose, np.float64, -1, 6), _host(map_of_frame, np.int32, -1)
        r = self._evidence_rule(rule)
        self._check(self._L.pwpp_evidence_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(min_count), int(connectivity), int(frame_first), frames,
                                                    MEM_DEVICE, _dp(label_ptr), _dp(count_ptr), _dp(top_ptr), _dp(clusters_ptr), _dp(n_clusters_ptr), int(max_clusters),
                                                    _dp(point_cluster_ptr), _dp(occupancy_in_ptr), _vp(poses) if poses.size else None, len(poses), _hp(mof),
                                                    ctypes.byref(fmap), int(n_maps), _dp(map_ptr), ctypes.byref(r), _dp(rows_ptr), _dp(class_ptr), _dp(occupancy_out_ptr)))

    def distance_grid(self, count, min_count=1, max_dist=0, cell=1.0, want_nearest=True, want_metres=True):
        """The exact Euclidean distance of every cell of a (frames, ny, nx) or (ny, nx) int32 count image to the nearest occupied
        cell (count >= min_count) of its frame.  Works before any estimate call.  Returns (dist2, nearest, metres) of count's
        shape: the int32 squared distance in cells (DIST_BEYOND: none in reach), the int32 index iy * nx + ix of the nearest
        occupied cell (the smallest among several; -1: none) and float32 sqrt(dist2) * cell (+inf: none); None for an image that
        is not wanted.  max_dist > 0: cells further than max_dist cells from every occupied cell report none (include/pwpp.h)."""
        c3, shape = _count_image(count)
        frames, ny, nx = c3.shape
        dist2 = np.empty(c3.shape, np.int32)
        nearest = np.empty(c3.shape, np.int32) if want_nearest else None
        metres = np.empty(c3.shape, np.float32) if want_metres else None
        self._check(self._L.pwpp_distance_grid(self._h, nx, ny, frames, MEM_HOST, _hp(c3), int(min_count), int(max_dist), float(cell), _hp(dist2),
                                               _hp(nearest), _hp(metres)))
        return tuple(None if a is None else a.reshape(shape) for a in (dist2, nearest, metres))

    def distance_grid_device(self, nx, ny, frames, count_ptr, min_count, max_dist, cell, dist2_ptr, nearest_ptr=0, metres_ptr=0):
        """distance_grid on device memory: addresses of the (frames, ny, nx) int32 count and dist2 images and (0: not wanted) the
        int32 nearest and float32 metres images, 4-byte aligned.  Enqueued on the handle's stream; complete after synchronize()."""
        self._check(self._L.pwpp_distance_grid(self._h, int(nx), int(ny), int(frames), MEM_DEVICE, _dp(count_ptr), int(min_count), int(max_dist),
                                               float(cell), _dp(dist2_ptr), _dp(nearest_ptr), _dp(metres_ptr)))

    def distance_obstacles(self, x0, y0, cell, nx, ny, h_min, h_max, min_count=1, max_dist=0, frame_first=0, frames=None, ground_only=False,
                           want_nearest=True, want_metres=True, want_count=False):
        """rasterize_obstacles and distance_grid in one call, for frames of the last estimate call.  Returns (dist2, nearest,
        metres) as distance_grid does for the (frames, ny, nx) count image, metres with the grid's cell; want_count: then that
        int32 count image too."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        shape = self._grid_shape(g, frames)
        dist2 = np.empty(shape, np.int32)
        nearest = np.empty(shape, np.int32) if want_nearest else None
        metres = np.empty(shape, np.float32) if want_metres else None
        count = np.empty(shape, np.int32) if want_count else None
        self._check(self._L.pwpp_distance_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(min_count), int(max_dist), int(frame_first),
                                                    frames, MEM_HOST, _hp(dist2), _hp(nearest), _hp(metres), _hp(count)))
        return (dist2, nearest, metres) + ((count,) if want_count else ())

    def distance_obstacles_device(self, x0, y0, cell, nx, ny, h_min, h_max, min_count, max_dist, dist2_ptr, nearest_ptr=0, metres_ptr=0, count_ptr=0,
                                  frame_first=0, frames=None, ground_only=False):
        """distance_obstacles into device memory: addresses as in distance_grid_device, count_ptr the int32 count image (0: not
        wanted).  Enqueued on the handle's stream; complete after synchronize()."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        self._check(self._L.pwpp_distance_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(min_count), int(max_dist), int(frame_first),
                                                    frames, MEM_DEVICE, _dp(dist2_ptr), _dp(nearest_ptr), _dp(metres_ptr), _dp(count_ptr)))

    def visibility_grid(self, count, origin, min_count=1, max_range=0, want_occupancy=True):
        """The line-of-sight free space of a (frames, ny, nx) or (ny, nx) int32 count image: for every cell the first occupied cell
        (count >= min_count) on the digital line from the sensor's cell.  origin: (ox, oy) for every frame, or (frames, 2) cells.
        Works before any estimate call.  Returns (first, occupancy) of count's shape: the int32 index iy * nx + ix of that cell
        (VIS_NONE: the line is clear; VIS_BEYOND: the cell is further than max_range > 0 cells, Chebyshev) and the int8 byte
        OCC_OCCUPIED / OCC_FREE / OCC_UNKNOWN (None when not wanted).  The rules: include/pwpp.h."""
        c3, shape = _count_image(count)
        frames, ny, nx = c3.shape
        org = np.ascontiguousarray(np.asarray(origin, np.int32).reshape(-1, 2))
        first = np.empty(c3.shape, np.int32)
        occupancy = np.empty(c3.shape, np.int8) if want_occupancy else None
        self._check(self._L.pwpp_visibility_grid(self._h, nx, ny, frames, MEM_HOST, _hp(c3), int(min_count), _hp(org), len(org), int(max_range),
                                                 _hp(first), _hp(occupancy)))
        return first.reshape(shape), None if occupancy is None else occupancy.reshape(shape)

    def visibility_grid_device(self, nx, ny, frames, count_ptr, origin, min_count, max_range, first_ptr, occupancy_ptr=0):
        """visibility_grid on device memory: addresses of the (frames, ny, nx) int32 count and first images, 4-byte aligned, and
        (0: not wanted) the int8 occupancy image; origin stays a host array, (ox, oy) or (frames, 2).  Enqueued on the handle's
        stream; complete after synchronize()."""
        org = np.ascontiguousarray(np.asarray(origin, np.int32).reshape(-1, 2))
        self._check(self._L.pwpp_visibility_grid(self._h, int(nx), int(ny), int(frames), MEM_DEVICE, _dp(count_ptr), int(min_count),
                                                 _vp(org) if org.size else None, len(org), int(max_range), _dp(first_ptr), _dp(occupancy_ptr)))

    def visibility_obstacles(self, x0, y0, cell, nx, ny, h_min, h_max, origin_xy=(0.0, 0.0), min_count=1, max_range=0, frame_first=0, frames=None,
                             ground_only=False, want_occupancy=True, want_count=False):
        """rasterize_obstacles and visibility_grid in one call, for frames of the last estimate call.  origin_xy: the sensor's
        position in metres in the model's frame, (x, y) for every frame or (frames, 2).  Returns (first, occupancy) as
        visibility_grid does for the (frames, ny, nx) count image; want_count: then that int32 count image too."""
        g, frames, org = self._look(x0, y0, cell, nx, ny, frame_first, frames, ground_only, origin_xy)
        shape = self._grid_shape(g, frames)
        first = np.empty(shape, np.int32)
        occupancy = np.empty(shape, np.int8) if want_occupancy else None
        count = np.empty(shape, np.int32) if want_count else None
        self._check(self._L.pwpp_visibility_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(min_count), _hp(org), len(org),
                                                      int(max_range), int(frame_first), frames, MEM_HOST, _hp(first), _hp(occupancy), _hp(count)))
        return (first, occupancy) + ((count,) if want_count else ())

    def visibility_obstacles_device(self, x0, y0, cell, nx, ny, h_min, h_max, origin_xy, min_count, max_range, first_ptr, occupancy_ptr=0, count_ptr=0,
                                    frame_first=0, frames=None, ground_only=False):
        """visibility_obstacles into device memory: addresses as in visibility_grid_device, count_ptr the int32 count image (0: not
        wanted); origin_xy stays a host array.  Enqueued on the handle's stream; complete after synchronize()."""
        g, frames, org = self._look(x0, y0, cell, nx, ny, frame_first, frames, ground_only, origin_xy)
        self._check(self._L.pwpp_visibility_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(min_count),
                                                      _vp(org) if org.size else None, len(org), int(max_range), int(frame_first), frames, MEM_DEVICE,
                                                      _dp(first_ptr), _dp(occupancy_ptr), _dp(count_ptr)))

    def viewshed_grid(self, count, origin, block=None, target=None, seen=None, min_count=1, min_seen=1, max_range=0, want_shadow=True,
                      want_occupancy=True):
        """The height-aware line of sight of a (frames, ny, nx) or (ny, nx) int32 count image: visibility_grid's walk, in which an
        occupied cell hides a cell behind it only where the ray from the eye to that cell passes through it.  block, target, seen:
        int32 images of count's shape or None -- the height of an occupied cell's top (None or VIEW_NO_HEIGHT: opaque), the height
        of a cell's ground (None or VIEW_NO_HEIGHT: hidden by any blocker) and its ground returns (seen >= min_seen: free whatever
        the line says).  origin: (ox, oy, eye) for every frame, or (frames, 3).  Works before any estimate call.  Returns (first,
        shadow, occupancy) of count's shape: the int32 index of the nearest cell that hides (VIS_NONE, VIS_BEYOND as
        visibility_grid), the int32 lowest height seen at the cell (VIEW_NO_HEIGHT: no blocker; INT32_MAX: behind an opaque one)
        and the int8 byte; None for an image that is not wanted.  The rules: include/pwpp.h."""
        c3, shape = _count_image(count)
        frames, ny, nx = c3.shape
        imgs = [None if a is None else np.ascontiguousarray(np.asarray(a, np.int32).reshape(c3.shape)) for a in (block, target, seen)]
        org = np.ascontiguousarray(np.asarray(origin, np.int32).reshape(-1, 3))
        first = np.empty(c3.shape, np.int32)
        shadow = np.empty(c3.shape, np.int32) if want_shadow else None
        occupancy = np.empty(c3.shape, np.int8) if want_occupancy else None
        self._check(self._L.pwpp_viewshed_grid(self._h, nx, ny, frames, MEM_HOST, _hp(c3), int(min_count), _hp(imgs[0]), _hp(imgs[1]), _hp(imgs[2]),
                                               int(min_seen), _hp(org), len(org), int(max_range), _hp(first), _hp(shadow), _hp(occupancy)))
        return tuple(None if a is None else a.reshape(shape) for a in (first, shadow, occupancy))

    def viewshed_grid_device(self, nx, ny, frames, count_ptr, origin, min_count, max_range, first_ptr, shadow_ptr=0, occupancy_ptr=0, block_ptr=0,
                             target_ptr=0, seen_ptr=0, min_seen=1):
        """viewshed_grid on device memory: addresses of the (frames, ny, nx) int32 images, 4-byte aligned, and of the int8 occupancy
        image (0: none / not wanted); origin stays a host array, (ox, oy, eye) or (frames, 3).  Enqueued on the handle's stream;
        complete after synchronize()."""
        org = np.ascontiguousarray(np.asarray(origin, np.int32).reshape(-1, 3))
        self._check(self._L.pwpp_viewshed_grid(self._h, int(nx), int(ny), int(frames), MEM_DEVICE, _dp(count_ptr), int(min_count), _dp(block_ptr),
                                               _dp(target_ptr), _dp(seen_ptr), int(min_seen), _vp(org) if org.size else None, len(org), int(max_range),
                                               _dp(first_ptr), _dp(shadow_ptr), _dp(occupancy_ptr)))

    def rasterize_ground_returns(self, x0, y0, cell, nx, ny, frame_first=0, frames=None):
        """The last call's GROUND points on the grid of rasterize_obstacles: (frames, ny, nx) int32 counts of the points the frame's
        ground list names, by the same cell rule."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, False)
        seen = np.empty(self._grid_shape(g, frames), np.int32)
        self._check(self._L.pwpp_rasterize_ground_returns(self._h, ctypes.byref(g), int(frame_first), frames, MEM_HOST, _hp(seen)))
        return seen

    def rasterize_ground_returns_device(self, x0, y0, cell, nx, ny, seen_ptr, frame_first=0, frames=None):
        """rasterize_ground_returns into device memory: the address of the (frames, ny, nx) int32 image.  Enqueued on the handle's
        stream; complete after synchronize()."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, False)
        self._check(self._L.pwpp_rasterize_ground_returns(self._h, ctypes.byref(g), int(frame_first), frames, MEM_DEVICE, _dp(seen_ptr)))

    def viewshed_obstacles(self, x0, y0, cell, nx, ny, h_min, h_max, origin_xyz=(0.0, 0.0, 0.0), min_count=1, min_seen=1, max_range=0, frame_first=0,
                           frames=None, ground_only=False, want_shadow=True, want_occupancy=True, want_count=False):
        """rasterize_obstacles, rasterize_ground, rasterize_ground_returns (min_seen > 0) and viewshed_grid in one call, for frames
        of the last estimate call: target = units(ground), block = units(ground + top), eye = units(z).  origin_xyz: the sensor's
        position in metres in the model's frame, (x, y, z) for every frame or (frames, 3).  Returns (first, shadow, occupancy) as
        viewshed_grid does; want_count: then the int32 count image too."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        org = _host(origin_xyz, np.float64, -1, 3)
        shape = self._grid_shape(g, frames)
        first = np.empty(shape, np.int32)
        shadow = np.empty(shape, np.int32) if want_shadow else None
        occupancy = np.empty(shape, np.int8) if want_occupancy else None
        count = np.empty(shape, np.int32) if want_count else None
        self._check(self._L.pwpp_viewshed_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(min_count), int(min_seen), _hp(org), len(org),
                                                    int(max_range), int(frame_first), frames, MEM_HOST, _hp(first), _hp(shadow), _hp(occupancy), _hp(count)))
        return (first, shadow, occupancy) + ((count,) if want_count else ())

    def viewshed_obstacles_device(self, x0, y0, cell, nx, ny, h_min, h_max, origin_xyz, min_count, min_seen, max_range, first_ptr, shadow_ptr=0,
                                  occupancy_ptr=0, count_ptr=0, frame_first=0, frames=None, ground_only=False):
        """viewshed_obstacles into device memory: addresses as in viewshed_grid_device, count_ptr the int32 count image (0: not
        wanted); origin_xyz stays a host array.  Enqueued on the handle's stream; complete after synchronize()."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        org = _host(origin_xyz, np.float64, -1, 3)
        self._check(self._L.pwpp_viewshed_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(min_count), int(min_seen),
                                                    _vp(org) if org.size else None, len(org), int(max_range), int(frame_first), frames, MEM_DEVICE,
                                                    _dp(first_ptr), _dp(shadow_ptr), _dp(occupancy_ptr), _dp(count_ptr)))

    def rasterize_beams(self, x0, y0, cell, nx, ny, which=BEAMS_GROUND, frame_first=0, frames=None):
        """The endpoints of the last call's beams on the grid of rasterize_obstacles: (hits, zmin), (frames, ny, nx) int32 -- the
        points of the selected index lists (which: BEAMS_GROUND, BEAMS_NONGROUND or both) per cell, and the smallest
        viewshed_units(z) among them (VIEW_NO_HEIGHT: none).  The non-ground list also holds the points the reflected-noise removal
        rejected, whose beams end below the ground: BEAMS_GROUND is the safe default."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, False)
        hits, zmin = np.empty(self._grid_shape(g, frames), np.int32), np.empty(self._grid_shape(g, frames), np.int32)
        self._check(self._L.pwpp_rasterize_beams(self._h, ctypes.byref(g), int(which), int(frame_first), frames, MEM_HOST, _hp(hits), _hp(zmin)))
        return hits, zmin

    def rasterize_beams_device(self, x0, y0, cell, nx, ny, hits_ptr, zmin_ptr, which=BEAMS_GROUND, frame_first=0, frames=None):
        """rasterize_beams into device memory: the addresses of the two (frames, ny, nx) int32 images.  Enqueued on the handle's
        stream; complete after synchronize()."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, False)
        self._check(self._L.pwpp_rasterize_beams(self._h, ctypes.byref(g), int(which), int(frame_first), frames, MEM_DEVICE, _dp(hits_ptr), _dp(zmin_ptr)))

    def beam_grid(self, hits, zmin, origin, target=None, occupancy_in=None, max_range=0, min_pass=1, clearance=0, want_occupancy=True):
        """The per-beam free space of (frames, ny, nx) or (ny, nx) int32 endpoint images: every cell with hits >= 1 and a zmin is the
        end of a beam of weight hits from the origin's cell, drawn along visibility_grid's line; it crosses the cells strictly between.
        origin: (ox, oy, eye) for every frame, or (frames, 3).  target: int32 ground heights or None; occupancy_in: int8 base bytes or
        None (all OCC_UNKNOWN).  Works before any estimate call.  Returns (passes, low, occupancy) of hits' shape: the uint32 sum of
        the weights of the beams that crossed the cell, the int32 lowest of their heights there (VIEW_NO_HEIGHT: none) and the int8
        byte -- OCC_FREE where the base byte is OCC_UNKNOWN, passes >= min_pass and (with a target) low - target <= clearance, else
        the base byte; None when it is not wanted.  The rules: include/pwpp.h."""
        h3, shape = _count_image(hits)
        frames, ny, nx = h3.shape
        z3 = np.ascontiguousarray(np.asarray(zmin, np.int32).reshape(h3.shape))
        tg = None if target is None else np.ascontiguousarray(np.asarray(target, np.int32).reshape(h3.shape))
        base = None if occupancy_in is None else np.ascontiguousarray(np.asarray(occupancy_in, np.int8).reshape(h3.shape))
        org = np.ascontiguousarray(np.asarray(origin, np.int32).reshape(-1, 3))
        passes, low = np.empty(h3.shape, np.uint32), np.empty(h3.shape, np.int32)
        occupancy = np.empty(h3.shape, np.int8) if want_occupancy else None
        self._check(self._L.pwpp_beam_grid(self._h, nx, ny, frames, MEM_HOST, _hp(h3), _hp(z3), _hp(tg), _hp(base), _hp(org), len(org), int(max_range),
                                           int(min_pass), int(clearance), _hp(passes), _hp(low), _hp(occupancy)))
        return tuple(None if a is None else a.reshape(shape) for a in (passes, low, occupancy))

    def beam_grid_device(self, nx, ny, frames, hits_ptr, zmin_ptr, origin, max_range, min_pass, clearance, passes_ptr, low_ptr, occupancy_ptr=0,
                         target_ptr=0, occupancy_in_ptr=0):
        """beam_grid on device memory: addresses of the (frames, ny, nx) int32 images, 4-byte aligned, and of the int8 images (0: none
        / not wanted; occupancy_ptr may equal occupancy_in_ptr); origin stays a host array, (ox, oy, eye) or (frames, 3).  Enqueued on
        the handle's stream; complete after synchronize()."""
        org = np.ascontiguousarray(np.asarray(origin, np.int32).reshape(-1, 3))
        self._check(self._L.pwpp_beam_grid(self._h, int(nx), int(ny), int(frames), MEM_DEVICE, _dp(hits_ptr), _dp(zmin_ptr), _dp(target_ptr),
                                           _dp(occupancy_in_ptr), _vp(org) if org.size else None, len(org), int(max_range), int(min_pass), int(clearance),
                                           _dp(passes_ptr), _dp(low_ptr), _dp(occupancy_ptr)))

    def beam_ground(self, x0, y0, cell, nx, ny, origin_xyz=(0.0, 0.0, 0.0), which=BEAMS_GROUND, occupancy_in=None, max_range=0, min_pass=1, clearance=0.0,
                    frame_first=0, frames=None, ground_only=False, want_occupancy=True, want_ends=False):
        """rasterize_beams, rasterize_ground and beam_grid in one call, for frames of the last estimate call: target =
        units(ground), eye = units(z) of the sensor's position origin_xyz in metres, (x, y, z) for every frame or (frames, 3);
        clearance in metres.  occupancy_in: (frames, ny, nx) int8 base bytes -- typically viewshed_obstacles' -- or None.  Returns
        (passes, low, occupancy) as beam_grid does; want_ends: then the int32 hits and zmin images too."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        org = _host(origin_xyz, np.float64, -1, 3)
        shape = self._grid_shape(g, frames)
        base = None if occupancy_in is None else np.ascontiguousarray(np.asarray(occupancy_in, np.int8).reshape(shape))
        passes, low = np.empty(shape, np.uint32), np.empty(shape, np.int32)
        occupancy = np.empty(shape, np.int8) if want_occupancy else None
        hits, zmin = (np.empty(shape, np.int32), np.empty(shape, np.int32)) if want_ends else (None, None)
        self._check(self._L.pwpp_beam_ground(self._h, ctypes.byref(g), int(which), _hp(org), len(org), int(max_range), int(min_pass), float(clearance),
                                             int(frame_first), frames, MEM_HOST, _hp(base), _hp(passes), _hp(low), _hp(occupancy), _hp(hits), _hp(zmin)))
        return (passes, low, occupancy) + ((hits, zmin) if want_ends else ())

    def beam_ground_device(self, x0, y0, cell, nx, ny, origin_xyz, which, max_range, min_pass, clearance, passes_ptr, low_ptr, occupancy_ptr=0,
                           occupancy_in_ptr=0, hits_ptr=0, zmin_ptr=0, frame_first=0, frames=None, ground_only=False):
        """beam_ground into device memory: addresses as in beam_grid_device, hits_ptr and zmin_ptr the endpoint images (0: not
        wanted); origin_xyz stays a host array.  Enqueued on the handle's stream; complete after synchronize()."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        org = _host(origin_xyz, np.float64, -1, 3)
        self._check(self._L.pwpp_beam_ground(self._h, ctypes.byref(g), int(which), _vp(org) if org.size else None, len(org), int(max_range), int(min_pass),
                                             float(clearance), int(frame_first), frames, MEM_DEVICE, _dp(occupancy_in_ptr), _dp(passes_ptr), _dp(low_ptr),
                                             _dp(occupancy_ptr), _dp(hits_ptr), _dp(zmin_ptr)))

    @staticmethod
    def _fusion_host(pose, map_of_frame, shift):
        """The host arrays every fusion call takes: (n_poses, 6) float64, (frames,) int32 or None, (n_maps, 2) int32 or None."""
        return _host(pose, np.float64, -1, 6), _host(map_of_frame, np.int32, -1), _host(shift, np.int32, -1, 2)

    def fuse_grid(self, occupancy, grid, pose, fmap, n_maps=1, map_in=None, map_of_frame=None, shift=None, want_occupancy=True, map_out=None):
        """Fuses the (frames, ny, nx) or (ny, nx) int8 occupancy images on the grid `grid` = (x0, y0, cell) into n_maps int16 log-odds
        maps described by the FusionMap `fmap`.  pose: the map-from-frame {a, b, tx, c, d, ty}, one for every frame or (frames, 6);
        map_of_frame: None (one map: a sequence; n_maps == frames: frame i into map i) or a map index per frame, -1: skipped;
        shift: None or (n_maps, 2) cells {sx, sy}; map_in: the (n_maps, NY, NX) int16 maps to start from, None: zero; map_out: the
        array to write (map_in itself is allowed without a shift), None: a new one.  Works before any estimate call.  Returns
        (map_out, map_occupancy) of shape (n_maps, NY, NX), the int8 bytes None when not wanted.  The rules: include/pwpp.h."""
        o3, frames, g = _occupancy_image(occupancy, grid)
        pose, mof, shift = self._fusion_host(pose, map_of_frame, shift)
        shape = self._grid_shape(fmap, n_maps)
        if map_in is not None:
            map_in = np.ascontiguousarray(map_in, np.int16).reshape(shape)
        out = np.empty(shape, np.int16) if map_out is None else map_out
        byte = np.empty(shape, np.int8) if want_occupancy else None
        self._check(self._L.pwpp_fuse_grid(self._h, ctypes.byref(g), frames, MEM_HOST, _hp(o3), _hp(pose), len(pose), _hp(mof), ctypes.byref(fmap),
                                           int(n_maps), _hp(shift), _hp(map_in), _hp(out), _hp(byte)))
        return out, byte

    def fuse_grid_device(self, grid, nx, ny, frames, occupancy_ptr, pose, fmap, n_maps, map_in_ptr, map_out_ptr, map_occupancy_ptr=0, map_of_frame=None,
                         shift=None):
        """fuse_grid on device memory: addresses of the (frames, ny, nx) int8 occupancy images, the (n_maps, NY, NX) int16 maps
        (map_in_ptr 0: zero; 2-byte aligned) and (0: not wanted) the int8 map bytes; pose, map_of_frame and shift stay host arrays.
        Enqueued on the handle's stream; complete after synchronize()."""
        g = GroundGrid(float(grid[0]), float(grid[1]), float(grid[2]), int(nx), int(ny), 0, 0)
        pose, mof, shift = self._fusion_host(pose, map_of_frame, shift)
        self._check(self._L.pwpp_fuse_grid(self._h, ctypes.byref(g), int(frames), MEM_DEVICE, _dp(occupancy_ptr), _hp(pose), len(pose), _hp(mof),
                                           ctypes.byref(fmap), int(n_maps), _hp(shift), _dp(map_in_ptr), _dp(map_out_ptr), _dp(map_occupancy_ptr)))

    def fuse_obstacles(self, x0, y0, cell, nx, ny, h_min, h_max, pose, fmap, n_maps=1, map_in=None, origin_xy=(0.0, 0.0), min_count=1, max_range=0,
                       frame_first=0, frames=None, map_of_frame=None, shift=None, ground_only=False, want_occupancy=True, want_frames=False):
        """rasterize_obstacles, visibility_grid and fuse_grid in one call, for frames of the last estimate call: (map_out,
        map_occupancy) as fuse_grid gives them for the occupancy bytes of visibility_obstacles; want_frames: then those
        (frames, ny, nx) int8 bytes too."""
        g, frames, org = self._look(x0, y0, cell, nx, ny, frame_first, frames, ground_only, origin_xy)
        pose, mof, shift = self._fusion_host(pose, map_of_frame, shift)
        shape = self._grid_shape(fmap, n_maps)
        if map_in is not None:
            map_in = np.ascontiguousarray(map_in, np.int16).reshape(shape)
        out = np.empty(shape, np.int16)
        byte = np.empty(shape, np.int8) if want_occupancy else None
        occ = np.empty(self._grid_shape(g, frames), np.int8) if want_frames else None
        self._check(self._L.pwpp_fuse_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(min_count), _hp(org), len(org), int(max_range),
                                                int(frame_first), frames, MEM_HOST, _hp(pose), len(pose), _hp(mof), ctypes.byref(fmap), int(n_maps),
                                                _hp(shift), _hp(map_in), _hp(out), _hp(byte), _hp(occ)))
        return (out, byte) + ((occ,) if want_frames else ())

    def fuse_obstacles_device(self, x0, y0, cell, nx, ny, h_min, h_max, pose, fmap, n_maps, map_in_ptr, map_out_ptr, map_occupancy_ptr=0, occupancy_ptr=0,
                              origin_xy=(0.0, 0.0), min_count=1, max_range=0, frame_first=0, frames=None, map_of_frame=None, shift=None,
                              ground_only=False):
        """fuse_obstacles into device memory: addresses as in fuse_grid_device, occupancy_ptr the (frames, ny, nx) int8 bytes of the
        frames (0: kept in the handle's buffer).  Enqueued on the handle's stream; complete after synchronize()."""
        g, frames, org = self._look(x0, y0, cell, nx, ny, frame_first, frames, ground_only, origin_xy)
        pose, mof, shift = self._fusion_host(pose, map_of_frame, shift)
        self._check(self._L.pwpp_fuse_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(min_count), _hp(org), len(org), int(max_range),
                                                int(frame_first), frames, MEM_DEVICE, _hp(pose), len(pose), _hp(mof), ctypes.byref(fmap), int(n_maps),
                                                _hp(shift), _dp(map_in_ptr), _dp(map_out_ptr), _dp(map_occupancy_ptr), _dp(occupancy_ptr)))

    @staticmethod
    def _height_host(pose, z_offset, map_of_frame, shift):
        """The host arrays every elevation fusion call takes: (n_poses, 6) and (n_poses,) float64 or None, (frames,) and (n_maps, 2) int32 or None."""
        return _host(pose, np.float64, -1, 6), _host(z_offset, np.float64, -1), _host(map_of_frame, np.int32, -1), _host(shift, np.int32, -1, 2)

    def _height_maps(self, hmap, n_maps, sum_in, n_in, want_mean, sum_out=None, n_out=None):
        shape = self._grid_shape(hmap, n_maps)
        if sum_in is not None:
            sum_in = np.ascontiguousarray(sum_in, np.int32).reshape(shape)
        if n_in is not None:
            n_in = np.ascontiguousarray(n_in, np.int16).reshape(shape)
        return (sum_in, n_in, np.empty(shape, np.int32) if sum_out is None else sum_out, np.empty(shape, np.int16) if n_out is None else n_out,
                np.empty(shape, np.float32) if want_mean else None)

    def fuse_height_grid(self, height, grid, pose, hmap, n_maps=1, sum_in=None, n_in=None, z_offset=None, map_of_frame=None, shift=None, want_mean=True,
                         sum_out=None, n_out=None):
        """Fuses the (frames, ny, nx) or (ny, nx) float32 height images (NaN: no height) on the grid `grid` = (x0, y0, cell) into
        n_maps elevation maps described by the HeightMap `hmap`: an int32 sum (units of 2^-10 m) and an int16 count per cell, and
        their float32 mean.  pose, map_of_frame and shift as in fuse_grid; z_offset: the height of each frame's origin in the map's
        frame, one per pose, None: 0; sum_in, n_in: the (n_maps, NY, NX) maps to start from, both None: empty; sum_out, n_out: the
        arrays to write (the inputs themselves are allowed without a shift), None: new ones.  Works before any estimate call.
        Returns (sum_out, n_out, mean), the mean None when not wanted.  The rules: include/pwpp.h."""
        hgt = np.ascontiguousarray(height, np.float32)
        h3 = hgt.reshape((1,) + hgt.shape) if hgt.ndim == 2 else hgt
        if h3.ndim != 3:
            raise ValueError("height: a (frames, ny, nx) or (ny, nx) image expected")
        g = GroundGrid(float(grid[0]), float(grid[1]), float(grid[2]), h3.shape[2], h3.shape[1], 0, 0)
        pose, zo, mof, shift = self._height_host(pose, z_offset, map_of_frame, shift)
        sum_in, n_in, s_out, c_out, mean = self._height_maps(hmap, n_maps, sum_in, n_in, want_mean, sum_out, n_out)
        self._check(self._L.pwpp_fuse_height_grid(self._h, ctypes.byref(g), h3.shape[0], MEM_HOST, _hp(h3), _hp(pose), _hp(zo), len(pose), _hp(mof),
                                                  ctypes.byref(hmap), int(n_maps), _hp(shift), _hp(sum_in), _hp(n_in), _hp(s_out), _hp(c_out), _hp(mean)))
        return s_out, c_out, mean

    def fuse_height_grid_device(self, grid, nx, ny, frames, height_ptr, pose, hmap, n_maps, sum_in_ptr, n_in_ptr, sum_out_ptr, n_out_ptr, mean_ptr=0,
                                z_offset=None, map_of_frame=None, shift=None):
        """fuse_height_grid on device memory: addresses of the (frames, ny, nx) float32 height images, the (n_maps, NY, NX) int32 sums
        and int16 counts (inputs 0: empty maps) and (0: not wanted) the float32 means; 4-, 4- and 2-byte aligned.  pose, z_offset,
        map_of_frame and shift stay host arrays.  Enqueued on the handle's stream; complete after synchronize()."""
        g = GroundGrid(float(grid[0]), float(grid[1]), float(grid[2]), int(nx), int(ny), 0, 0)
        pose, zo, mof, shift = self._height_host(pose, z_offset, map_of_frame, shift)
        self._check(self._L.pwpp_fuse_height_grid(self._h, ctypes.byref(g), int(frames), MEM_DEVICE, _dp(height_ptr), _hp(pose), _hp(zo), len(pose), _hp(mof),
                                                  ctypes.byref(hmap), int(n_maps), _hp(shift), _dp(sum_in_ptr), _dp(n_in_ptr), _dp(sum_out_ptr),
                                                  _dp(n_out_ptr), _dp(mean_ptr)))

    def fuse_ground(self, x0, y0, cell, nx, ny, pose, hmap, n_maps=1, sum_in=None, n_in=None, z_offset=None, frame_first=0, frames=None,
                    map_of_frame=None, shift=None, ground_only=False, want_mean=True, want_frames=False):
        """rasterize_ground and fuse_height_grid in one call, for frames of the last estimate call: (sum_out, n_out, mean) as
        fuse_height_grid gives them for the elevation images of rasterize_ground; want_frames: then those (frames, ny, nx) float32
        images too."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        pose, zo, mof, shift = self._height_host(pose, z_offset, map_of_frame, shift)
        sum_in, n_in, s_out, c_out, mean = self._height_maps(hmap, n_maps, sum_in, n_in, want_mean)
        hgt = np.empty(self._grid_shape(g, frames), np.float32) if want_frames else None
        self._check(self._L.pwpp_fuse_ground(self._h, ctypes.byref(g), int(frame_first), frames, MEM_HOST, _hp(pose), _hp(zo), len(pose), _hp(mof),
                                             ctypes.byref(hmap), int(n_maps), _hp(shift), _hp(sum_in), _hp(n_in), _hp(s_out), _hp(c_out), _hp(mean), _hp(hgt)))
        return (s_out, c_out, mean) + ((hgt,) if want_frames else ())

    def fuse_ground_device(self, x0, y0, cell, nx, ny, pose, hmap, n_maps, sum_in_ptr, n_in_ptr, sum_out_ptr, n_out_ptr, mean_ptr=0, height_ptr=0,
                           z_offset=None, frame_first=0, frames=None, map_of_frame=None, shift=None, ground_only=False):
        """fuse_ground into device memory: addresses as in fuse_height_grid_device, height_ptr the (frames, ny, nx) float32 images of
        the frames (0: kept in the handle's buffer).  Enqueued on the handle's stream; complete after synchronize()."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        pose, zo, mof, shift = self._height_host(pose, z_offset, map_of_frame, shift)
        self._check(self._L.pwpp_fuse_ground(self._h, ctypes.byref(g), int(frame_first), frames, MEM_DEVICE, _hp(pose), _hp(zo), len(pose), _hp(mof),
                                             ctypes.byref(hmap), int(n_maps), _hp(shift), _dp(sum_in_ptr), _dp(n_in_ptr), _dp(sum_out_ptr), _dp(n_out_ptr),
                                             _dp(mean_ptr), _dp(height_ptr)))

    _TERRAIN_OUTPUTS = (("step", np.float32), ("slope", np.float32), ("rough", np.float32), ("count", np.uint8), ("cost", np.int8))

    @classmethod
    def _terrain_outputs(cls, shape, wants):
        """The output arrays of a terrain call, None where not wanted, in the order step, slope, rough, count, cost."""
        return tuple(np.empty(shape, dtype) if want else None for (_, dtype), want in zip(cls._TERRAIN_OUTPUTS, wants))

    def terrain_grid(self, height, cell, params, want_step=True, want_slope=True, want_rough=True, want_count=True, want_cost=True):
        """The terrain analysis of the (frames, ny, nx) or (ny, nx) float32 height images (NaN: unknown) with cells of `cell` metres
        under the TerrainParams `params`: per cell the height step, the slope (rise over run) and the roughness of the
        (2r+1) x (2r+1) window around it (float32, NaN where undefined), the uint8 count of known cells in the window and the int8
        traversability cost (-1: none, 0 .. 100).  Works before any estimate call.  Returns (step, slope, rough, count, cost) in
        the shape of `height`, None for an output that is not wanted.  The rules: include/pwpp.h."""
        hgt = np.ascontiguousarray(height, np.float32)
        h3 = hgt.reshape((1,) + hgt.shape) if hgt.ndim == 2 else hgt
        if h3.ndim != 3:
            raise ValueError("height: a (frames, ny, nx) or (ny, nx) image expected")
        out = self._terrain_outputs(hgt.shape, (want_step, want_slope, want_rough, want_count, want_cost))
        self._check(self._L.pwpp_terrain_grid(self._h, h3.shape[2], h3.shape[1], h3.shape[0], float(cell), MEM_HOST, _hp(h3), ctypes.byref(params),
                                              *[_hp(a) for a in out]))
        return out

    def terrain_grid_device(self, nx, ny, frames, cell, height_ptr, params, step_ptr=0, slope_ptr=0, rough_ptr=0, count_ptr=0, cost_ptr=0):
        """terrain_grid on device memory: addresses of the (frames, ny, nx) float32 height images and of the float32 step, slope and
        rough, the uint8 count and the int8 cost images (0: not wanted); the floats 4-byte aligned.  Enqueued on the handle's
        stream; complete after synchronize()."""
        self._check(self._L.pwpp_terrain_grid(self._h, int(nx), int(ny), int(frames), float(cell), MEM_DEVICE, _dp(height_ptr), ctypes.byref(params),
                                              _dp(step_ptr), _dp(slope_ptr), _dp(rough_ptr), _dp(count_ptr), _dp(cost_ptr)))

    def terrain_ground(self, x0, y0, cell, nx, ny, params, frame_first=0, frames=None, ground_only=False, want_step=True, want_slope=True,
                       want_rough=True, want_count=True, want_cost=True, want_frames=False):
        """rasterize_ground and terrain_grid in one call, for frames of the last estimate call: (step, slope, rough, count, cost) as
        terrain_grid gives them for the (frames, ny, nx) elevation images of rasterize_ground; want_frames: then those images too."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        shape = self._grid_shape(g, frames)
        out = self._terrain_outputs(shape, (want_step, want_slope, want_rough, want_count, want_cost))
        hgt = np.empty(shape, np.float32) if want_frames else None
        self._check(self._L.pwpp_terrain_ground(self._h, ctypes.byref(g), int(frame_first), frames, MEM_HOST, ctypes.byref(params),
                                                *([_hp(a) for a in out] + [_hp(hgt)])))
        return out + ((hgt,) if want_frames else ())

    def terrain_ground_device(self, x0, y0, cell, nx, ny, params, step_ptr=0, slope_ptr=0, rough_ptr=0, count_ptr=0, cost_ptr=0, height_ptr=0,
                              frame_first=0, frames=None, ground_only=False):
        """terrain_ground into device memory: addresses as in terrain_grid_device, height_ptr the (frames, ny, nx) float32 images of
        the frames (0: kept in the handle's buffer).  Enqueued on the handle's stream; complete after synchronize()."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        self._check(self._L.pwpp_terrain_ground(self._h, ctypes.byref(g), int(frame_first), frames, MEM_DEVICE, ctypes.byref(params), _dp(step_ptr),
                                                _dp(slope_ptr), _dp(rough_ptr), _dp(count_ptr), _dp(cost_ptr), _dp(height_ptr)))

    def reach_grid(self, cost, source, params, dist2=None, want_from=True):
        """The cost-to-reach field of the (frames, ny, nx) or (ny, nx) int8 cost images (< 0: unknown, 0 .. 100, >= params.lethal:
        impassable) under the ReachParams `params`: for every cell the cheapest sum of steps from the frame's source cell over the
        8-connected passable cells.  source: (sx, sy) for every frame, or (frames, 2) cells; dist2: None or the int32 image of
        distance_grid of cost's shape (passable then needs dist2 > params.clearance2).  Works before any estimate call.  Returns
        (reach, from) of cost's shape: int32, REACH_NONE where no path exists, and the index iy * nx + ix of the neighbour the
        cheapest path comes through (the source: its own; -1: none; None when not wanted).  The rules: include/pwpp.h."""
        cst = np.ascontiguousarray(cost, np.int8)
        c3 = cst.reshape((1,) + cst.shape) if cst.ndim == 2 else cst
        if c3.ndim != 3:
            raise ValueError("cost: a (frames, ny, nx) or (ny, nx) image expected")
        d3 = None if dist2 is None else np.ascontiguousarray(dist2, np.int32)
        if d3 is not None and d3.size != c3.size:
            raise ValueError("dist2: an image of cost's shape expected")
        src = np.ascontiguousarray(np.asarray(source, np.int32).reshape(-1, 2))
        reach = np.empty(cst.shape, np.int32)
        frm = np.empty(cst.shape, np.int32) if want_from else None
        self._check(self._L.pwpp_reach_grid(self._h, c3.shape[2], c3.shape[1], c3.shape[0], MEM_HOST, _hp(c3), _hp(d3), ctypes.byref(params), _hp(src),
                                            len(src), _hp(reach), _hp(frm)))
        return reach, frm

    def reach_grid_device(self, nx, ny, frames, cost_ptr, source, params, reach_ptr, from_ptr=0, dist2_ptr=0):
        """reach_grid on device memory: addresses of the (frames, ny, nx) int8 cost images (any address) and of the int32 reach,
        from and dist2 images (0: none; 4-byte aligned); source stays a host array, (sx, sy) or (frames, 2).  Enqueued on the
        handle's stream; complete after synchronize()."""
        src = np.ascontiguousarray(np.asarray(source, np.int32).reshape(-1, 2))
        self._check(self._L.pwpp_reach_grid(self._h, int(nx), int(ny), int(frames), MEM_DEVICE, _dp(cost_ptr), _dp(dist2_ptr), ctypes.byref(params),
                                            _vp(src) if src.size else None, len(src), _dp(reach_ptr), _dp(from_ptr)))

    def reach_ground(self, x0, y0, cell, nx, ny, terrain_params, params, source_xy=(0.0, 0.0), frame_first=0, frames=None, ground_only=False,
                     want_from=True, want_cost=False):
        """rasterize_ground, the cost of terrain_grid and reach_grid in one call, for frames of the last estimate call.  source_xy:
        the vehicle's position in metres in the model's frame, (x, y) for every frame or (frames, 2).  Returns (reach, from) as
        reach_grid gives them for the (frames, ny, nx) cost images of terrain_ground; want_cost: then those int8 images too."""
        g, frames, src = self._look(x0, y0, cell, nx, ny, frame_first, frames, ground_only, source_xy)
        shape = self._grid_shape(g, frames)
        reach = np.empty(shape, np.int32)
        frm = np.empty(shape, np.int32) if want_from else None
        cost = np.empty(shape, np.int8) if want_cost else None
        self._check(self._L.pwpp_reach_ground(self._h, ctypes.byref(g), int(frame_first), frames, MEM_HOST, ctypes.byref(terrain_params), ctypes.byref(params),
                                              _hp(src), len(src), _hp(reach), _hp(frm), _hp(cost)))
        return (reach, frm) + ((cost,) if want_cost else ())

    def reach_ground_device(self, x0, y0, cell, nx, ny, terrain_params, params, source_xy, reach_ptr, from_ptr=0, cost_ptr=0, frame_first=0, frames=None,
                            ground_only=False):
        """reach_ground into device memory: addresses as in reach_grid_device, cost_ptr the (frames, ny, nx) int8 cost images of
        the terrain analysis (0: kept in the handle's buffer); source_xy stays a host array.  Enqueued on the handle's stream;
        complete after synchronize()."""
        g, frames, src = self._look(x0, y0, cell, nx, ny, frame_first, frames, ground_only, source_xy)
        self._check(self._L.pwpp_reach_ground(self._h, ctypes.byref(g), int(frame_first), frames, MEM_DEVICE, ctypes.byref(terrain_params),
                                              ctypes.byref(params), _vp(src) if src.size else None, len(src), _dp(reach_ptr), _dp(from_ptr), _dp(cost_ptr)))

    @staticmethod
    def _starts(start, frames):
        """The starts as the calls take them: (n_starts, 2) for every frame or (frames, n_starts, 2) -> (array, n_start_sets, n_starts)."""
        st = np.ascontiguousarray(np.asarray(start, np.int32))
        if st.ndim == 1:
            st = st.reshape(1, 2)
        if st.ndim not in (2, 3) or st.shape[-1] != 2:
            raise ValueError("start: (x, y), (n_starts, 2) or (frames, n_starts, 2) cells expected")
        return st, (1 if st.ndim == 2 else st.shape[0]), st.shape[-2]

    def route_grid(self, cost, source, params, frm, start, route_params, dist2=None):
        """The routes on a reach field: for every frame of the (frames, ny, nx) or (ny, nx) int8 cost images and every start cell the
        chain of `frm` (the from image of reach_grid on the same cost, source, ReachParams `params` and dist2) from the start to the
        frame's source.  start: (x, y), (n_starts, 2) cells for every frame or (frames, n_starts, 2).  Returns (routes, cells,
        waypoints): a (frames, n_starts) array of ROUTE_DTYPE rows, the (frames, n_starts, max_cells) int32 cell indices and the
        (frames, n_starts, max_waypoints) int32 waypoint cells of the RouteParams `route_params`, -1 behind a list's end (None for a
        limit of 0).  The rules: include/pwpp.h."""
        cst = np.ascontiguousarray(cost, np.int8)
        c3 = cst.reshape((1,) + cst.shape) if cst.ndim == 2 else cst
        if c3.ndim != 3:
            raise ValueError("cost: a (frames, ny, nx) or (ny, nx) image expected")
        d3 = None if dist2 is None else np.ascontiguousarray(dist2, np.int32)
        f3 = np.ascontiguousarray(frm, np.int32)
        if f3.size != c3.size or (d3 is not None and d3.size != c3.size):
            raise ValueError("from, dist2: images of cost's shape expected")
        src = np.ascontiguousarray(np.asarray(source, np.int32).reshape(-1, 2))
        st, sets, n = self._starts(start, c3.shape[0])
        routes, cells, wps = self._route_outputs(c3.shape[0], n, route_params)
        self._check(self._L.pwpp_route_grid(self._h, c3.shape[2], c3.shape[1], c3.shape[0], MEM_HOST, _hp(c3), _hp(d3), ctypes.byref(params), _hp(src),
                                            len(src), _hp(f3), _hp(st), sets, n, ctypes.byref(route_params), _hp(routes), _hp(cells), _hp(wps)))
        return routes, cells, wps

    @staticmethod
    def _route_outputs(frames, n, q):
        routes = np.empty((frames, n), ROUTE_DTYPE)
        cells = np.empty((frames, n, q.max_cells), np.int32) if q.max_cells > 0 else None
        wps = np.empty((frames, n, q.max_waypoints), np.int32) if q.max_waypoints > 0 else None
        return routes, cells, wps

    def route_grid_device(self, nx, ny, frames, cost_ptr, source, params, from_ptr, start, route_params, routes_ptr, cells_ptr=0, waypoints_ptr=0, dist2_ptr=0):
        """route_grid on device memory: addresses of the (frames, ny, nx) int8 cost images (any address), of the int32 from and dist2
        images, of the (frames, n_starts) rows of 32 bytes and of the int32 lists (0: none; 4-byte aligned); source and start stay
        host arrays.  Enqueued on the handle's stream; complete after synchronize()."""
        src = np.ascontiguousarray(np.asarray(source, np.int32).reshape(-1, 2))
        st, sets, n = self._starts(start, frames)
        self._check(self._L.pwpp_route_grid(self._h, int(nx), int(ny), int(frames), MEM_DEVICE, _dp(cost_ptr), _dp(dist2_ptr), ctypes.byref(params),
                                            _vp(src) if src.size else None, len(src), _dp(from_ptr), _vp(st) if st.size else None, sets, n,
                                            ctypes.byref(route_params), _dp(routes_ptr), _dp(cells_ptr), _dp(waypoints_ptr)))

    def plan_grid(self, cost, source, params, start, route_params, dist2=None, want_field=False):
        """reach_grid and route_grid on its from in one call: (routes, cells, waypoints) as route_grid returns them; want_field: then
        (reach, from) as reach_grid returns them too -- otherwise the field stays on the device."""
        cst = np.ascontiguousarray(cost, np.int8)
        c3 = cst.reshape((1,) + cst.shape) if cst.ndim == 2 else cst
        if c3.ndim != 3:
            raise ValueError("cost: a (frames, ny, nx) or (ny, nx) image expected")
        d3 = None if dist2 is None else np.ascontiguousarray(dist2, np.int32)
        if d3 is not None and d3.size != c3.size:
            raise ValueError("dist2: an image of cost's shape expected")
        src = np.ascontiguousarray(np.asarray(source, np.int32).reshape(-1, 2))
        st, sets, n = self._starts(start, c3.shape[0])
        routes, cells, wps = self._route_outputs(c3.shape[0], n, route_params)
        reach = np.empty(cst.shape, np.int32) if want_field else None
        frm = np.empty(cst.shape, np.int32) if want_field else None
        self._check(self._L.pwpp_plan_grid(self._h, c3.shape[2], c3.shape[1], c3.shape[0], MEM_HOST, _hp(c3), _hp(d3), ctypes.byref(params), _hp(src), len(src),
                                           _hp(st), sets, n, ctypes.byref(route_params), _hp(routes), _hp(cells), _hp(wps), _hp(reach), _hp(frm)))
        return (routes, cells, wps) + ((reach, frm) if want_field else ())

    def plan_grid_device(self, nx, ny, frames, cost_ptr, source, params, start, route_params, routes_ptr, cells_ptr=0, waypoints_ptr=0, dist2_ptr=0,
                         reach_ptr=0, from_ptr=0):
        """plan_grid on device memory: addresses as in route_grid_device; reach_ptr, from_ptr: the int32 images of the field (0: kept in
        the handle's buffer).  Enqueued on the handle's stream; complete after synchronize()."""
        src = np.ascontiguousarray(np.asarray(source, np.int32).reshape(-1, 2))
        st, sets, n = self._starts(start, frames)
        self._check(self._L.pwpp_plan_grid(self._h, int(nx), int(ny), int(frames), MEM_DEVICE, _dp(cost_ptr), _dp(dist2_ptr), ctypes.byref(params),
                                           _vp(src) if src.size else None, len(src), _vp(st) if st.size else None, sets, n, ctypes.byref(route_params),
                                           _dp(routes_ptr), _dp(cells_ptr), _dp(waypoints_ptr), _dp(reach_ptr), _dp(from_ptr)))

    @staticmethod
    def _poses(poses, frames):
        """The poses as the call takes them: (n_steps, 4), (n_traj, n_steps, 4) for every frame or (n_sets, n_traj, n_steps, 4) -> (array, n_sets, n_traj, n_steps)."""
        q = np.ascontiguousarray(np.asarray(poses, np.int32))
        while q.ndim < 4:
            q = q.reshape((1,) + q.shape)
        if q.ndim != 4 or q.shape[-1] != 4:
            raise ValueError("poses: (n_steps, 4), (n_traj, n_steps, 4) or (n_sets, n_traj, n_steps, 4) entries {px, py, ux, uy} expected")
        return q, q.shape[0], q.shape[1], q.shape[2]

    def footprint_grid(self, cost, params, foot_params, poses, dist2=None, reach=None, want_poses=True, want_trajectories=True):
        """The oriented footprint over cost images: for every frame of the (frames, ny, nx) or (ny, nx) int8 cost images, every
        trajectory and every step the rectangle of the FootprintParams `foot_params` at the pose {px, py, ux, uy} (ticks of 1/16 cell, an
        integer heading) judged by the ReachParams `params` (and dist2 with a clearance).  poses: (n_steps, 4), (n_traj, n_steps, 4) for
        every frame or (frames, n_traj, n_steps, 4).  Returns (pose_rows, traj_rows): (frames, n_traj, n_steps) FOOT_POSE_DTYPE rows and
        (frames, n_traj) FOOT_TRAJ_DTYPE rows, None for the one not wanted.  reach: the int32 field whose value at the last free pose a
        trajectory row carries.  The rules: include/pwpp.h."""
        cst = np.ascontiguousarray(cost, np.int8)
        c3 = cst.reshape((1,) + cst.shape) if cst.ndim == 2 else cst
        if c3.ndim != 3:
            raise ValueError("cost: a (frames, ny, nx) or (ny, nx) image expected")
        d3 = None if dist2 is None else np.ascontiguousarray(dist2, np.int32)
        r3 = None if reach is None else np.ascontiguousarray(reach, np.int32)
        if (d3 is not None and d3.size != c3.size) or (r3 is not None and r3.size != c3.size):
            raise ValueError("dist2, reach: images of cost's shape expected")
        q, sets, n_traj, n_steps = self._poses(poses, c3.shape[0])
        prow = np.empty((c3.shape[0], n_traj, n_steps), FOOT_POSE_DTYPE) if want_poses else None
        trow = np.empty((c3.shape[0], n_traj), FOOT_TRAJ_DTYPE) if want_trajectories else None
        self._check(self._L.pwpp_footprint_grid(self._h, c3.shape[2], c3.shape[1], c3.shape[0], MEM_HOST, _hp(c3), _hp(d3), _hp(r3), ctypes.byref(params),
                                                ctypes.byref(foot_params), _hp(q), sets, n_traj, n_steps, _hp(prow), _hp(trow)))
        return prow, trow

    def footprint_grid_device(self, nx, ny, frames, cost_ptr, params, foot_params, poses, pose_rows_ptr=0, traj_rows_ptr=0, dist2_ptr=0, reach_ptr=0):
        """footprint_grid on device memory: addresses of the (frames, ny, nx) int8 cost images (any address), of the int32 dist2 and
        reach images and of the rows of 32 bytes (0: none; 4-byte aligned); poses stay a host array.  Enqueued on the handle's stream;
        complete after synchronize()."""
        q, sets, n_traj, n_steps = self._poses(poses, frames)
        self._check(self._L.pwpp_footprint_grid(self._h, int(nx), int(ny), int(frames), MEM_DEVICE, _dp(cost_ptr), _dp(dist2_ptr), _dp(reach_ptr), ctypes.byref(params),
                                                ctypes.byref(foot_params), _vp(q) if q.size else None, sets, n_traj, n_steps, _dp(pose_rows_ptr), _dp(traj_rows_ptr)))

    def costmap_grid(self, params, occupancy=None, terrain=None, dist2=None, curve=None, want_why=False):
        """The costmap of (frames, ny, nx) or (ny, nx) images under the CostmapParams `params`: the int8 occupancy bytes, the int8
        terrain cost bytes and the int32 dist2 image, each needed only with its layer, and the uint8 inflation table `curve`
        indexed by dist2.  With the inflation layer and dist2 None the distances are computed from (occupancy == OCC_OCCUPIED) on
        the device.  Works before any estimate call.  Returns the int8 cost image (-1: unknown, 0 .. 100), with want_why (cost,
        why): the uint8 image of the layers that set the cost.  The rules: include/pwpp.h."""
        given = [a for a in (occupancy, terrain, dist2) if a is not None]
        if not given:
            raise ValueError("at least one of occupancy, terrain and dist2 expected")
        shape = tuple(np.shape(given[0]))
        shape3 = (1,) + shape if len(shape) == 2 else shape
        if len(shape3) != 3:
            raise ValueError("(frames, ny, nx) or (ny, nx) images expected")
        imgs = []
        for a, dtype in ((occupancy, np.int8), (terrain, np.int8), (dist2, np.int32)):
            a = None if a is None else np.ascontiguousarray(a, dtype)
            if a is not None and a.shape != shape:
                raise ValueError("occupancy, terrain and dist2: images of one shape expected")
            imgs.append(a)
        cv = _curve(curve)
        cost = np.empty(shape, np.int8)
        why = np.empty(shape, np.uint8) if want_why else None
        self._check(self._L.pwpp_costmap_grid(self._h, shape3[2], shape3[1], shape3[0], MEM_HOST, _hp(imgs[0]), _hp(imgs[1]), _hp(imgs[2]),
                                              ctypes.byref(params), _hp(cv), 0 if cv is None else len(cv), _hp(cost), _hp(why)))
        return (cost, why) if want_why else cost

    def costmap_grid_device(self, nx, ny, frames, params, cost_ptr, occupancy_ptr=0, terrain_ptr=0, dist2_ptr=0, curve=None, why_ptr=0):
        """costmap_grid on device memory: addresses of the (frames, ny, nx) int8 occupancy and terrain images, the int8 cost and the
        uint8 why image (any address each) and of the int32 dist2 image (4-byte aligned); 0: none.  curve stays a host array.
        Enqueued on the handle's stream; complete after synchronize()."""
        cv = _curve(curve)
        self._check(self._L.pwpp_costmap_grid(self._h, int(nx), int(ny), int(frames), MEM_DEVICE, _dp(occupancy_ptr), _dp(terrain_ptr), _dp(dist2_ptr),
                                              ctypes.byref(params), _hp(cv), 0 if cv is None else len(cv), _dp(cost_ptr), _dp(why_ptr)))

    def costmap_obstacles(self, x0, y0, cell, nx, ny, params, h_min=-np.inf, h_max=np.inf, min_count=1, origin_xy=(0.0, 0.0), max_range=0,
                          terrain_params=None, curve=None, frame_first=0, frames=None, ground_only=False, want_why=False, want_layers=False):
        """The costmap of frames of the last estimate call in one call: rasterize_obstacles, the visibility's bytes, the distances
        (capped at the table's reach), rasterize_ground and the terrain's cost -- only what the layers of the CostmapParams `params`
        need -- and the fold.  origin_xy and max_range as visibility_obstacles takes them, terrain_params a TerrainParams (needed
        with the terrain layer), curve the uint8 inflation table.  Returns the tuple (cost,) of the int8 (frames, ny, nx) cost
        images; with want_why followed by the uint8 why images; with want_layers followed by occupancy, dist2 and terrain, None
        for a layer that is off."""
        g, frames, org = self._look(x0, y0, cell, nx, ny, frame_first, frames, ground_only, origin_xy)
        shape = self._grid_shape(g, frames)
        cv = _curve(curve)
        cost = np.empty(shape, np.int8)
        why = np.empty(shape, np.uint8) if want_why else None
        layers = [None, None, None]
        if want_layers:
            for k, (bit, dtype) in enumerate(((COSTMAP_OCCUPANCY, np.int8), (COSTMAP_INFLATION, np.int32), (COSTMAP_TERRAIN, np.int8))):
                layers[k] = np.empty(shape, dtype) if params.layers & bit else None
        self._check(self._L.pwpp_costmap_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(min_count), _hp(org), len(org), int(max_range),
                                                   None if terrain_params is None else ctypes.byref(terrain_params), ctypes.byref(params), _hp(cv),
                                                   0 if cv is None else len(cv), int(frame_first), frames, MEM_HOST, _hp(cost), _hp(why), _hp(layers[0]),
                                                   _hp(layers[1]), _hp(layers[2])))
        return (cost,) + ((why,) if want_why else ()) + (tuple(layers) if want_layers else ())

    def costmap_obstacles_device(self, x0, y0, cell, nx, ny, params, cost_ptr, h_min=-np.inf, h_max=np.inf, min_count=1, origin_xy=(0.0, 0.0), max_range=0,
                                 terrain_params=None, curve=None, why_ptr=0, occupancy_ptr=0, dist2_ptr=0, terrain_ptr=0, frame_first=0, frames=None,
                                 ground_only=False):
        """costmap_obstacles into device memory: addresses as in costmap_grid_device; occupancy_ptr, dist2_ptr and terrain_ptr the
        layers' images (0: kept in the handle's buffer).  Enqueued on the handle's stream; complete after synchronize(): a
        reach_grid_device on cost_ptr may follow at once."""
        g, frames, org = self._look(x0, y0, cell, nx, ny, frame_first, frames, ground_only, origin_xy)
        cv = _curve(curve)
        self._check(self._L.pwpp_costmap_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(min_count), _vp(org) if org.size else None,
                                                   len(org), int(max_range), None if terrain_params is None else ctypes.byref(terrain_params),
                                                   ctypes.byref(params), _hp(cv), 0 if cv is None else len(cv), int(frame_first), frames, MEM_DEVICE,
                                                   _dp(cost_ptr), _dp(why_ptr), _dp(occupancy_ptr), _dp(dist2_ptr), _dp(terrain_ptr)))

    @staticmethod
    def _match_host(candidates, frames, map_of_frame):
        """The host arrays every match call takes: (n_sets, n_candidates, 6) float64 and (frames,) int32 or None."""
        cand = np.ascontiguousarray(np.asarray(candidates, np.float64))
        cand = cand.reshape((1,) + cand.shape) if cand.ndim == 2 else cand
        if cand.ndim != 3 or cand.shape[2] != 6:
            raise ValueError("candidates: (n_candidates, 6) or (n_sets, n_candidates, 6) expected")
        return cand, _host(map_of_frame, np.int32, -1)

    def match_grid(self, occupancy, grid, candidates, fmap, maps, wx, wy, map_of_frame=None, want_scores=False):
        """Matches the (frames, ny, nx) or (ny, nx) int8 occupancy images on the grid `grid` = (x0, y0, cell) against the
        (n_maps, NY, NX) or (NY, NX) int16 log-odds maps described by the FusionMap `fmap`: for every candidate pose
        {a, b, tx, c, d, ty} -- (n_candidates, 6) for every frame, or (frames, n_candidates, 6) -- and every shift of
        [-wx, wx] x [-wy, wy] map cells, the sum of the map under the frame's occupied cells.  map_of_frame as in fuse_grid.
        Works before any estimate call.  Returns the (frames,) MATCH_BEST_DTYPE rows; want_scores: (rows, scores) with the int64
        (frames, n_candidates, 2 wy + 1, 2 wx + 1) sums.  The rules: include/pwpp.h."""
        o3, frames, g = _occupancy_image(occupancy, grid)
        m3 = _maps_image(maps, fmap)
        cand, mof = self._match_host(candidates, frames, map_of_frame)
        best = np.zeros(frames, MATCH_BEST_DTYPE)
        scores = np.zeros((frames, cand.shape[1], 2 * int(wy) + 1, 2 * int(wx) + 1), np.int64) if want_scores else None
        self._check(self._L.pwpp_match_grid(self._h, ctypes.byref(g), frames, MEM_HOST, _hp(o3), _hp(cand), cand.shape[0], cand.shape[1], _hp(mof),
                                            ctypes.byref(fmap), m3.shape[0], _hp(m3), int(wx), int(wy), _hp(best), _hp(scores)))
        return (best, scores) if want_scores else best

    def match_grid_device(self, grid, nx, ny, frames, occupancy_ptr, candidates, fmap, n_maps, map_ptr, wx, wy, best_ptr, scores_ptr=0, map_of_frame=None):
        """match_grid on device memory: addresses of the (frames, ny, nx) int8 occupancy images, the (n_maps, NY, NX) int16 maps
        (2-byte aligned), the (frames,) rows of 24 bytes and (0: not wanted) the int64 scores, both 8-byte aligned; candidates and
        map_of_frame stay host arrays.  Enqueued on the handle's stream; complete after synchronize()."""
        g = GroundGrid(float(grid[0]), float(grid[1]), float(grid[2]), int(nx), int(ny), 0, 0)
        cand, mof = self._match_host(candidates, frames, map_of_frame)
        self._check(self._L.pwpp_match_grid(self._h, ctypes.byref(g), int(frames), MEM_DEVICE, _dp(occupancy_ptr), _hp(cand), cand.shape[0], cand.shape[1],
                                            _hp(mof), ctypes.byref(fmap), int(n_maps), _dp(map_ptr), int(wx), int(wy), _dp(best_ptr), _dp(scores_ptr)))

    def match_obstacles(self, x0, y0, cell, nx, ny, h_min, h_max, candidates, fmap, maps, wx, wy, origin_xy=(0.0, 0.0), min_count=1, max_range=0,
                        frame_first=0, frames=None, map_of_frame=None, ground_only=False, want_scores=False, want_frames=False):
        """rasterize_obstacles, visibility_grid and match_grid in one call, for frames of the last estimate call: the rows (and
        scores) match_grid gives for the occupancy bytes of visibility_obstacles; want_frames: then those (frames, ny, nx) int8
        bytes too, last."""
        g, frames, org = self._look(x0, y0, cell, nx, ny, frame_first, frames, ground_only, origin_xy)
        m3 = _maps_image(maps, fmap)
        cand, mof = self._match_host(candidates, frames, map_of_frame)
        best = np.zeros(max(frames, 0), MATCH_BEST_DTYPE)
        scores = np.zeros((max(frames, 0), cand.shape[1], 2 * int(wy) + 1, 2 * int(wx) + 1), np.int64) if want_scores else None
        occ = np.empty(self._grid_shape(g, frames), np.int8) if want_frames else None
        self._check(self._L.pwpp_match_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(min_count), _hp(org), len(org), int(max_range),
                                                 int(frame_first), frames, MEM_HOST, _hp(cand), cand.shape[0], cand.shape[1], _hp(mof), ctypes.byref(fmap),
                                                 m3.shape[0], _hp(m3), int(wx), int(wy), _hp(best), _hp(scores), _hp(occ)))
        out = (best,) + ((scores,) if want_scores else ()) + ((occ,) if want_frames else ())
        return out if len(out) > 1 else best

    def match_obstacles_device(self, x0, y0, cell, nx, ny, h_min, h_max, candidates, fmap, n_maps, map_ptr, wx, wy, best_ptr, scores_ptr=0, occupancy_ptr=0,
                               origin_xy=(0.0, 0.0), min_count=1, max_range=0, frame_first=0, frames=None, map_of_frame=None, ground_only=False):
        """match_obstacles on device memory: addresses as in match_grid_device, occupancy_ptr the (frames, ny, nx) int8 bytes of the
        frames (0: kept in the handle's buffer).  Enqueued on the handle's stream; complete after synchronize()."""
        g, frames, org = self._look(x0, y0, cell, nx, ny, frame_first, frames, ground_only, origin_xy)
        cand, mof = self._match_host(candidates, frames, map_of_frame)
        self._check(self._L.pwpp_match_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(min_count), _hp(org), len(org), int(max_range),
                                                 int(frame_first), frames, MEM_DEVICE, _hp(cand), cand.shape[0], cand.shape[1], _hp(mof), ctypes.byref(fmap),
                                                 int(n_maps), _dp(map_ptr), int(wx), int(wy), _dp(best_ptr), _dp(scores_ptr), _dp(occupancy_ptr)))

    def box_obstacles(self, x0, y0, cell, nx, ny, h_min, h_max, label, max_boxes, frame_first=0, frames=None, ground_only=False):
        """The counted points of every label of a (frames, ny, nx) or (ny, nx) int32 label image on the obstacle grid as oriented
        boxes, for frames of the last estimate call: the (frames, max_boxes) structured table (OBSTACLE_BOX_DTYPE).  Row r of a
        frame takes the counted points whose cell is labelled r; other labels (-1, >= max_boxes) are skipped; a row nobody names
        has points 0 and NaN floats (include/pwpp.h has the arithmetic)."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        label = np.ascontiguousarray(label, np.int32)
        if label.shape not in ((max(frames, 0), g.ny, g.nx), (g.ny, g.nx)) or (label.ndim == 2 and frames != 1):
            raise ValueError("label: a (frames, ny, nx) image expected")
        boxes = np.zeros((max(frames, 0), max(int(max_boxes), 0)), OBSTACLE_BOX_DTYPE)
        self._check(self._L.pwpp_box_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(frame_first), frames, MEM_HOST,
                                               _vp(label) if label.size else None, _vp(boxes) if boxes.size else None, int(max_boxes)))
        return boxes

    def box_obstacles_device(self, x0, y0, cell, nx, ny, h_min, h_max, label_ptr, boxes_ptr, max_boxes, frame_first=0, frames=None, ground_only=False):
        """box_obstacles on device memory: addresses of the (frames, ny, nx) int32 label image and of the (frames, max_boxes) table
        of 64-byte rows, both 4-byte aligned.  Enqueued on the handle's stream; complete after synchronize()."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        self._check(self._L.pwpp_box_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(frame_first), frames, MEM_DEVICE,
                                               _dp(label_ptr), _dp(boxes_ptr), int(max_boxes)))

    def hull_obstacles(self, x0, y0, cell, nx, ny, h_min, h_max, label, max_hulls, max_vertices, frame_first=0, frames=None, ground_only=False, with_vertices=True):
        """The counted points of every label of a (frames, ny, nx) or (ny, nx) int32 label image on the obstacle grid as convex hulls
        with their least enclosing rectangles, for frames of the last estimate call: the (frames, max_hulls) structured table
        (OBSTACLE_HULL_DTYPE) and the (frames, max_hulls, max_vertices, 2) int32 vertex lists, of which a row's first `stored` are
        written (None without with_vertices: the library is given no list).  Rows as in box_obstacles (include/pwpp.h has the arithmetic)."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        label = np.ascontiguousarray(label, np.int32)
        if label.size != max(frames, 0) * int(nx) * int(ny):
            raise ValueError("label: %d frames of %d x %d cells expected" % (frames, ny, nx))
        hulls = np.zeros((max(frames, 0), max(int(max_hulls), 0)), OBSTACLE_HULL_DTYPE)
        lists = np.zeros(hulls.shape + (min(max(int(max_vertices), 0), HULL_VERTICES_MAX), 2), np.int32) if with_vertices else None
        self._check(self._L.pwpp_hull_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(frame_first), frames, MEM_HOST,
                                                _vp(label) if label.size else None, _vp(hulls) if hulls.size else None, int(max_hulls),
                                                _vp(lists) if lists is not None and lists.size else None, int(max_vertices)))
        return hulls, lists

    def hull_obstacles_device(self, x0, y0, cell, nx, ny, h_min, h_max, label_ptr, hulls_ptr, max_hulls, vertices_ptr, max_vertices, frame_first=0, frames=None,
                              ground_only=False):
        """hull_obstacles on device memory: addresses of the (frames, ny, nx) int32 label image (4-byte aligned), of the (frames,
        max_hulls) table of 64-byte rows (8-byte aligned) and of the vertex lists (4-byte aligned; 0 or None: no lists).  Enqueued on
        the handle's stream; complete after synchronize()."""
        g, frames = self._grid(x0, y0, cell, nx, ny, frame_first, frames, ground_only)
        self._check(self._L.pwpp_hull_obstacles(self._h, ctypes.byref(g), float(h_min), float(h_max), int(frame_first), frames, MEM_DEVICE,
                                                _dp(label_ptr), _dp(hulls_ptr), int(max_hulls), _dp(vertices_ptr) if vertices_ptr else None, int(max_vertices)))

    def frame_base(self):
        """(frames + 1,) int64: where every frame starts in the batch-wide arrays (indices, labels)."""
        v = self.device_view()
        return np.ctypeslib.as_array(v.frame_base, shape=(v.frames + 1,)).copy()

    def set_overlap(self, on):
        """True: batches of 128+ frames run as two frame ranges on the handle's two streams (same results)."""
        self._check(self._L.pwpp_set_overlap(self._h, 1 if on else 0))

    def arena_stats(self):
        """(frames whose overgrown parts were moved into the overflow arena on the device, slots per frame, arena slots per frame)."""
        a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self._L.pwpp_get_arena_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def redo_stats(self):
        """(frames that went through one-pass binning, frames redone on the two-pass path after a segment overflow)"""
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._L.pwpp_get_redo_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def one_pass_stats(self):
        """(batches launched with one-pass binning, batches redone on the two-pass path after an overflow)"""
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._L.pwpp_get_one_pass_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)


class Pipe:
    """Batches of independent frames in flight (pwpp_pipe_*): `depth` handles, each batch goes to the next one in turn.
    submit_device_batch returns a Handle VIEW of the handle that holds the batch: synchronize() it, then read the results with
    the usual getters -- before that handle comes round again, `depth` submits later."""

    def __init__(self, params=None, device=0, depth=2):
        self._L = load()
        self.params = params if params is not None else default_params()
        p = ctypes.c_void_p()
        self._p = None
        rc = self._L.pwpp_pipe_create(ctypes.byref(self.params), device, depth, ctypes.byref(p))
        if rc < 0:
            raise PwppError("pwpp error %d: %s" % (rc, self._L.pwpp_last_error().decode()))
        self._p = p
        self.depth = depth
        self._views = {}

    def _view(self, raw):
        key = raw.value if hasattr(raw, "value") else int(raw)
        if key not in self._views:
            v = Handle.__new__(Handle)  # a view: the pipe owns the handle
            v._L, v.params, v._h, v._keep, v._borrowed = self._L, self.params, ctypes.c_void_p(key), None, True
            v._pipe = self  #  a view keeps its pipe alive: the pipe owns the handle the view points at
            self._views[key] = v
        return self._views[key]

    def handle(self, index):
        raw = self._L.pwpp_pipe_handle(self._p, index)
        return self._view(ctypes.c_void_p(raw)) if raw else None

    def set_num_streams(self, streams_per_handle):
        """MODE_STREAMS through the pipe: every handle owns one GROUP of `streams_per_handle` streams; submit k must carry the next
        frames of group k mod depth."""
        rc = self._L.pwpp_pipe_set_num_streams(self._p, streams_per_handle)
        if rc < 0:
            raise PwppError("pwpp error %d: %s" % (rc, self._L.pwpp_last_error().decode()))

    def submit_device_batch(self, batch, cols=4, layout=LAYOUT_ROW_MAJOR, mode=MODE_FRESH):
        cp, cn, k = batch
        holder = ctypes.c_void_p()
        rc = self._L.pwpp_pipe_submit(self._p, cp, cn, k, cols, layout, MEM_DEVICE, mode, ctypes.byref(holder))
        if rc < 0:
            raise PwppError("pwpp error %d: %s" % (rc, self._L.pwpp_last_error().decode()))
        return self._view(holder)

    def set_input_transforms(self, T):
        """Handle.set_input_transforms on every handle of the pipe (each batch submitted afterwards runs with it)."""
        for i in range(self.depth):
            self.handle(i).set_input_transforms(T)

    def drain(self):
        rc = self._L.pwpp_pipe_drain(self._p)
        if rc < 0:
            raise PwppError("pwpp error %d: %s" % (rc, self._L.pwpp_last_error().decode()))

    def workspace_bytes(self):
        return sum(self.handle(i).workspace_bytes() for i in range(self.depth))

    def close(self):
        if self._p is not None:
            for v in self._views.values():  #  the views' handles die with the pipe: a getter on one must fail, not crash
                v._h = None
                v._pipe = None
            self._L.pwpp_pipe_destroy(self._p)
            self._p = None
            self._views = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
