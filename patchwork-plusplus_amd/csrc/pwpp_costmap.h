// pwpp_costmap.h -- the rule of the costmap (pwpp_costmap_grid, pwpp_costmap_obstacles, pwpp_costmap_cell), one text for the kernels
// (pwpp_costmap.hip), for the host side (pwpp_capi.cpp) and for the host program that deals the same functions as the kernels do
// against the rule written out again (tools/costmap_check.cpp), the way pwpp_reach.h is one text for the cost-to-reach field.
// Internal; include/pwpp.h has the contract.  Integers only: the inflation curve is a table of bytes the caller hands over, and the
// device gathers from it and folds.
//
// THE LAYERS of a cell, each read only where its bit of `layers` is set, each a value 0 .. 100 or "unknown":
//   occupancy (1)  the byte o: 100 gives 100, 0 gives 0, every other byte is unknown -- the fusion's reading of an edited image;
//   inflation (2)  the word d: curve[d] where (uint32)d < n_curve, otherwise 0 -- PWPP_DIST_BEYOND and a negative word read 0; never unknown;
//   terrain   (4)  the byte t: t < 0 is unknown, t > 100 counts as 100, otherwise t.
// An unknown occupancy or terrain value becomes occupancy_unknown / terrain_unknown where that is >= 0 and stays unknown at -1.
// THE FOLD.  m = the maximum of the known values, 0 if there is none.  cost = -1 if a layer stayed unknown and m < unknown_below,
// otherwise m.  why = bits 1, 2, 4 for every enabled layer whose known value equals m, when m > 0; bit 8 iff a layer stayed
// unknown, whatever the cost came out as.  A maximum of values in 0 .. 100: no order of evaluation can change a bit of it.
// THE DEALING of path 2 (pwpp_costmap_deal): the call's cells are one run of n bytes per image, frames end to end.  With `head` the
// cells before the first 4-byte boundary of the cost image (0 .. 3, at most n), the run is head single cells, then (n - head) / 4
// groups of four cells whose cost bytes are one aligned dword, then the rest as single cells: item i < groups is the group at cell
// head + 4 i; item groups + k is the single cell k for k < head and cell head + 4 groups + (k - head) after that.  At most 6 single
// cells a call.  Every cell belongs to exactly one item (tools/costmap_check.cpp walks every head and length).
#ifndef PWPP_COSTMAP_H
#define PWPP_COSTMAP_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#ifndef PWPP_HD
#define PWPP_HD __host__ __device__
#endif
#else
#ifndef PWPP_HD
#define PWPP_HD
#endif
#endif

#define PWPP_COSTMAP_LAYER_OCCUPANCY 1
#define PWPP_COSTMAP_LAYER_INFLATION 2
#define PWPP_COSTMAP_LAYER_TERRAIN 4
#define PWPP_COSTMAP_WHY_UNKNOWN_BIT 8u
#define PWPP_COSTMAP_CURVE_MAX 4097                                   // PWPP_COSTMAP_MAX_CURVE: dist2 0 .. 64^2
#define PWPP_COSTMAP_CURVE_WORDS ((PWPP_COSTMAP_CURVE_MAX + 3) / 4)   // the table as the kernels hold it: whole dwords, the rest 0
#define PWPP_COSTMAP_BLOCK 256       // lanes of a workgroup, both paths
#define PWPP_COSTMAP_LANE_CELLS 4    // path 2: the cells of one item (one dword of a byte image, four of dist2)
#define PWPP_COSTMAP_LANE_ITEMS 4    // path 2: the items a lane takes, PWPP_COSTMAP_BLOCK apart, behind one staging of the table
// the cells one workgroup of path 2 folds (4096): where its dealing changes hands
#define PWPP_COSTMAP_GROUP_CELLS (PWPP_COSTMAP_BLOCK * PWPP_COSTMAP_LANE_CELLS * PWPP_COSTMAP_LANE_ITEMS)
// What option "costmap_path" = 0 means: path 2 for a call of at least this many cells, path 1 (the yardstick) below.  Decided by
// tools/costmap_cost.py (profiles/costmap_cost.txt), not in advance: the cells of the smallest measured call at which path 2 wins
// beyond the A/A floor.
#define PWPP_COSTMAP_QUADS_FROM_CELLS 16777216

// what a call fixes for every cell (the checked pwpp_costmap_params and the table's length; 0 without the inflation layer)
struct PwppCostmapRule {
    int32_t layers, occupancy_unknown, terrain_unknown, unknown_below, n_curve;
};

// The rule for one cell.  `curve`: n_curve bytes wherever they lie (global memory, LDS, the host); read only with the inflation
// layer and only at d < n_curve.  o, t: the bytes as int8 values; each input is ignored where its layer is off.
PWPP_HD inline void pwpp_costmap_fold(const PwppCostmapRule &R, const uint8_t *curve, int o, int t, int32_t d, int32_t &cost, uint32_t &why) {
    int32_t vo = -1, vi = -1, vt = -1;  // (-1: the layer is off or stayed unknown; it never wins the maximum)
    uint32_t unknown = 0;
    if (R.layers & PWPP_COSTMAP_LAYER_OCCUPANCY) {
        vo = o == 100 ? 100 : (o == 0 ? 0 : R.occupancy_unknown);
        if (vo < 0) unknown = PWPP_COSTMAP_WHY_UNKNOWN_BIT;
    }
    if (R.layers & PWPP_COSTMAP_LAYER_INFLATION) vi = (uint32_t)d < (uint32_t)R.n_curve ? (int32_t)curve[(uint32_t)d] : 0;
    if (R.layers & PWPP_COSTMAP_LAYER_TERRAIN) {
        vt = t < 0 ? R.terrain_unknown : (t > 100 ? 100 : t);
        if (vt < 0) unknown = PWPP_COSTMAP_WHY_UNKNOWN_BIT;
    }
    int32_t m = vo > vi ? vo : vi;
    m = m > vt ? m : vt;
    m = m > 0 ? m : 0;
    why = unknown;
    if (m > 0) why |= (vo == m ? 1u : 0u) | (vi == m ? 2u : 0u) | (vt == m ? 4u : 0u);
    cost = (unknown != 0 && m < R.unknown_below) ? -1 : m;
}

// The dealing of path 2 (above).  `cost_address`: the low bits of the cost image's address; n: the call's cells (1 .. 2^31).
struct PwppCostmapDeal {
    uint32_t head, groups, singles;  // singles = head + tail <= 6; items = groups + singles
};
PWPP_HD inline PwppCostmapDeal pwpp_costmap_deal(uint64_t cost_address, uint64_t n) {
    PwppCostmapDeal D;
    const uint64_t to_boundary = (4u - (cost_address & 3u)) & 3u;
    D.head = (uint32_t)(to_boundary < n ? to_boundary : n);
    D.groups = (uint32_t)((n - D.head) / PWPP_COSTMAP_LANE_CELLS);
    D.singles = (uint32_t)(n - (uint64_t)D.groups * PWPP_COSTMAP_LANE_CELLS);
    return D;
}
// item i of the dealing: its first cell; `cells`: 4 for a group, 1 for a single cell
PWPP_HD inline uint64_t pwpp_costmap_item(const PwppCostmapDeal &D, uint32_t i, int &cells) {
    if (i < D.groups) {
        cells = PWPP_COSTMAP_LANE_CELLS;
        return (uint64_t)D.head + (uint64_t)i * PWPP_COSTMAP_LANE_CELLS;
    }
    const uint32_t k = i - D.groups;
    cells = 1;
    return k < D.head ? (uint64_t)k : (uint64_t)D.head + (uint64_t)D.groups * PWPP_COSTMAP_LANE_CELLS + (uint64_t)(k - D.head);
}

// R of the distances a call computes itself: the least integer with R * R >= n_curve - 1; the launcher's max_dist is max(1, R).
// Every dist2 the cap turns into PWPP_DIST_BEYOND exceeds R * R >= n_curve - 1, so it reads 0 from the table either way.
PWPP_HD inline int32_t pwpp_costmap_cap(int32_t n_curve) {
    int32_t r = 0;
    while (r * r < n_curve - 1) ++r;  // (n_curve <= 4097: at most 64 rounds)
    return r > 1 ? r : 1;
}

#endif
