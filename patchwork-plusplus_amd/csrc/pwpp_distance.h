// pwpp_distance.h -- the arithmetic of the obstacle distances (pwpp_distance_grid, pwpp_distance_obstacles), one text for the
// kernels (pwpp_distance.hip) and for the host program that runs the same pass sequence against a brute force of its own
// (tools/distance_check.cpp), the way pwpp_unionfind.h is one text for the clusters.  Internal; include/pwpp.h has the contract.
//
// The exact Euclidean distance transform of an occupancy image is separable, and both passes are integer arithmetic:
//   pass 1, rows     gx[iy][ix] = the column of the occupied cell of row iy nearest to column ix; of a left and a right one at the
//                    same distance the LEFT (the smaller index); -1 when the row has none.  A wave takes the row in chunks of 64
//                    columns: the chunk's occupancy is one 64-bit mask, the neighbours inside the chunk are a leading- and a
//                    trailing-zero count on the masked word, and the last / next occupied column is carried across the chunks.
//   pass 2, columns  for the cell (ix, iy) the minimum over the rows jy of the 64-bit KEY
//                        ((gx[jy][ix] - ix)^2 + (iy - jy)^2) << 32 | (jy * nx + gx[jy][ix])
//                    whose high half is dist2 and whose low half is nearest.
// WHY THE KEY GIVES THE TIE RULE.  The nearest occupied cell of (ix, iy) inside row jy is one of the row's cells nearest to
// column ix; pass 1 kept the one with the smaller index.  Any occupied cell of row jy that attains the global minimum is such a
// row-nearest cell, so the global minimum over all occupied cells of (dist2, index) equals the minimum over the rows of the key.
// RANGES.  nx, ny <= 32768: a squared distance is at most 2 * 32767^2 < 2^31 - 1 = PWPP_DIST_BEYOND, a cell index below 2^30.
#ifndef PWPP_DISTANCE_H
#define PWPP_DISTANCE_H

#include <math.h>
#include <stdint.h>

#include "pwpp_unionfind.h"  // PWPP_HD

#define PWPP_DIST_NONE 0x7fffffffu                // = PWPP_DIST_BEYOND of include/pwpp.h
#define PWPP_DIST_KEY_NONE 0x7fffffffffffffffull  // dist2 PWPP_DIST_BEYOND, nearest -1: larger than the key of every occupied cell
#define PWPP_DIST_MAX_SIDE 32768                  // nx, ny
#define PWPP_DIST_MAX_CAP 46340                   // max_dist: the largest integer whose square is below 2^31

// max_dist as the kernels take it: the largest dist2 that is reported (0 = unlimited: every real dist2 is below PWPP_DIST_NONE)
PWPP_HD inline uint32_t pwpp_dist_cap2(int max_dist) { return max_dist > 0 ? (uint32_t)max_dist * (uint32_t)max_dist : PWPP_DIST_NONE; }

// ---- pass 1: inside a chunk of 64 columns whose occupancy is `mask` (bit l = column l of the chunk) ----------------------------
// the occupied column at or left of `lane` (-1: none) ...
PWPP_HD inline int pwpp_dist_left_in_chunk(unsigned long long mask, int lane) {
    const unsigned long long m = mask & (~0ull >> (63 - lane));
    return m ? 63 - __builtin_clzll(m) : -1;
}
// ... and at or right of it
PWPP_HD inline int pwpp_dist_right_in_chunk(unsigned long long mask, int lane) {
    const unsigned long long m = mask >> lane;
    return m ? lane + __builtin_ctzll(m) : -1;
}
// of the nearest occupied columns left (<= ix) and right (>= ix) of ix, -1 where none: the nearer, the left one on a tie
PWPP_HD inline int32_t pwpp_dist_row_pick(int32_t left, int32_t right, int32_t ix) {
    if (left < 0) return right;
    if (right < 0) return left;
    return ix - left <= right - ix ? left : right;
}

// ---- pass 2 --------------------------------------------------------------------------------------------------------------------
// the key of row jy for the cell (ix, iy), from gx = gx[jy][ix]
PWPP_HD inline unsigned long long pwpp_dist_key(int32_t gx, int ix, int iy, int jy, int nx) {
    if (gx < 0) return PWPP_DIST_KEY_NONE;
    const int dx = gx - ix, dy = iy - jy;
    return ((unsigned long long)((uint32_t)(dx * dx) + (uint32_t)(dy * dy)) << 32) | (uint32_t)(jy * nx + gx);
}

// The minimum key of the cell (ix, iy) over the rows, going OUTWARD from its own row: rows at distance d are looked at only
// while d * d <= the best dist2 so far (a row further away cannot hold a nearer cell, and none at the same distance once d * d
// exceeds it: a tie needs dy^2 <= dist2) and d * d <= cap2 (a cell beyond the cap is reported as beyond anyway).  Exact; the
// loop is bounded by ny.  `col.gx(jy)` is gx[jy][ix]; it is asked for rows 0 <= jy < ny with |jy - iy| <= sqrt(cap2) only.
template <class Column>
PWPP_HD inline unsigned long long pwpp_dist_scan_outward(Column &col, int ix, int iy, int nx, int ny, uint32_t cap2) {
    unsigned long long best = pwpp_dist_key(col.gx(iy), ix, iy, iy, nx);
    for (int d = 1; d < ny; ++d) {
        const uint32_t d2 = (uint32_t)d * (uint32_t)d;
        if (d2 > (uint32_t)(best >> 32) || d2 > cap2 || (iy - d < 0 && iy + d >= ny)) break;
        if (iy - d >= 0) {
            const unsigned long long k = pwpp_dist_key(col.gx(iy - d), ix, iy, iy - d, nx);
            best = k < best ? k : best;
        }
        if (iy + d < ny) {
            const unsigned long long k = pwpp_dist_key(col.gx(iy + d), ix, iy, iy + d, nx);
            best = k < best ? k : best;
        }
    }
    return best;
}

// the same minimum over every row, top to bottom, with no early exit: the yardstick
template <class Column>
PWPP_HD inline unsigned long long pwpp_dist_scan_all(Column &col, int ix, int iy, int nx, int ny) {
    unsigned long long best = PWPP_DIST_KEY_NONE;
    for (int jy = 0; jy < ny; ++jy) {
        const unsigned long long k = pwpp_dist_key(col.gx(jy), ix, iy, jy, nx);
        best = k < best ? k : best;
    }
    return best;
}

// ---- how pass 2 is dealt -------------------------------------------------------------------------------------------------------
#define PWPP_DIST_STRIP 64       // columns of a strip = lanes of a wave
#define PWPP_DIST_LDS_ROWS 512   // rows of a strip in LDS at most: 128 KiB of the CU's 160
#define PWPP_DIST_TALL_TILE 256  // rows of a workgroup's tile when the strip is read from global memory

// A column is cut into row_tiles tiles of tile_rows rows.  With lds != 0 the tile's rows and `halo` more on either side, clipped
// to the image, min(ny, tile_rows + 2 * halo) <= PWPP_DIST_LDS_ROWS of them, are in LDS: the whole column when it fits; a taller
// one with a cap in tiles with a halo of max_dist rows (pwpp_dist_scan_outward never leaves it); else, and on path 1 (the
// yardstick), the rows are read from global memory.
struct PwppDistPlan {
    int32_t lds, tile_rows, halo, row_tiles;
};
PWPP_HD inline PwppDistPlan pwpp_dist_plan(int ny, int max_dist, int path) {
    PwppDistPlan p;
    if (path == 0 && ny <= PWPP_DIST_LDS_ROWS) {
        p.lds = 1, p.tile_rows = ny, p.halo = 0;
    } else if (path == 0 && max_dist > 0 && 2 * max_dist + PWPP_DIST_STRIP <= PWPP_DIST_LDS_ROWS) {
        p.lds = 1, p.tile_rows = PWPP_DIST_LDS_ROWS - 2 * max_dist, p.halo = max_dist;
    } else {
        p.lds = 0, p.tile_rows = PWPP_DIST_TALL_TILE, p.halo = 0;
    }
    p.row_tiles = (ny + p.tile_rows - 1) / p.tile_rows;
    return p;
}

// the two integer outputs of a cell from its minimum key: beyond the cap (or no occupied cell at all) PWPP_DIST_NONE and -1
PWPP_HD inline void pwpp_dist_of_key(unsigned long long key, uint32_t cap2, int32_t &dist2, int32_t &nearest) {
    const uint32_t d2 = (uint32_t)(key >> 32);
    const bool beyond = d2 == PWPP_DIST_NONE || d2 > cap2;
    dist2 = beyond ? (int32_t)PWPP_DIST_NONE : (int32_t)d2;
    nearest = beyond ? -1 : (int32_t)(uint32_t)key;
}

// metres: one correctly rounded square root, one multiply in double, one rounding to float; +inf beyond
PWPP_HD inline float pwpp_dist_metres(int32_t dist2, double cell) {
    if (dist2 == (int32_t)PWPP_DIST_NONE) return __builtin_huge_valf();
    return (float)(sqrt((double)dist2) * cell);
}

#endif
