// pwpp_visibility.h -- the arithmetic of the line-of-sight free space (pwpp_visibility_grid, pwpp_visibility_obstacles), one text
// for the kernels (pwpp_visibility.hip), for the host side's origin cells (pwpp_capi.cpp) and for the host program that runs the
// same pack and walk against a brute force of its own (tools/visibility_check.cpp), the way pwpp_distance.h is one text for the
// distances.  Internal; include/pwpp.h has the contract.
//
// THE LINE from the sensor's cell o to the cell c, with dx = cx - ox, dy = cy - oy, n = max(|dx|, |dy|), is the points
//     P_k = (ox + sgn(dx) * ((2k|dx| + n) / (2n)), oy + sgn(dy) * ((2k|dy| + n) / (2n))),  k = 0 .. n   (integer division)
// -- the closed form is the definition.  The walk does not divide: per axis it keeps e_k = (2k|d| + n) mod 2n, e_0 = n, and adds
// 2|d| per step; since 2|d| <= 2n the quotient grows by at most one per step, exactly when e reaches 2n (pwpp_vis_step).  On the
// major axis |d| = n: e stays n and the coordinate moves every step.  2|d| + e < 4n <= 2^17: no overflow anywhere.
// THE TWO RULES of a step, in order: (a) when both coordinates moved, the two cells the step squeezes between, A = (x_{k-1}, y_k)
// and B = (x_k, y_{k-1}); both occupied: blocked, first = the smaller of their indices; (b) P_k occupied: first = its index.  The
// origin's own cell never blocks (k starts at 1).  An unblocked walk is therefore a 4-connected path through free cells once the
// free one of A and B is put between P_{k-1} and P_k: a wall that is only 8-connected is still opaque.
// WHAT A WALK TOUCHES.  P_k, A and B lie in the bounding rectangle of o and c, which lies in the image when both do; the
// accessors compare every index with nx and ny all the same before they form an address.
// THE BIT IMAGE.  Bit x & 31 of word row * row_words + (x >> 5), row_words = ceil(nx / 32): rows padded to whole words, the pad
// bits zero.  A wave packs 64 cells with one ballot: the low half is word 2k of the row, the high half word 2k + 1 (where the row
// has one).
#ifndef PWPP_VISIBILITY_H
#define PWPP_VISIBILITY_H

#include <math.h>
#include <stdint.h>

#include "pwpp_unionfind.h"  // PWPP_HD

#define PWPP_VIS_FIRST_NONE (-1)    // = PWPP_VIS_NONE of include/pwpp.h
#define PWPP_VIS_FIRST_BEYOND (-2)  // = PWPP_VIS_BEYOND
#define PWPP_VIS_FREE 0             // = PWPP_OCC_FREE, PWPP_OCC_OCCUPIED, PWPP_OCC_UNKNOWN
#define PWPP_VIS_OCCUPIED 100
#define PWPP_VIS_UNKNOWN (-1)
#define PWPP_VIS_MAX_SIDE 32768  // nx, ny and max_range
#define PWPP_VIS_LDS_BYTES (128 * 1024)  // the largest bit image of a frame a walk (the visibility's, the viewshed's) keeps in LDS: 1024 x 1024 cells, of the CU's 160 KiB

// ---- the origin's cell: the cell rule of the obstacle raster, u = (c - c0) / cell in double (one subtraction, one IEEE division),
// inside iff 0 <= u < n (a NaN: not), the cell floor(u)
PWPP_HD inline bool pwpp_vis_cell_of(double c, double c0, double cell, int n, int &i) {
    const double u = (c - c0) / cell;
    if (!(u >= 0.0 && u < (double)n)) return false;
    i = (int)floor(u);
    return true;
}

// ---- the bit image --------------------------------------------------------------------------------------------------------------
PWPP_HD inline int pwpp_vis_row_words(int nx) { return (nx + 31) >> 5; }
// the word `half` (0, 1) of the chunk of 64 cells whose occupancy is `mask` (bit l = cell l of the chunk)
PWPP_HD inline uint32_t pwpp_vis_ballot_word(unsigned long long mask, int half) { return (uint32_t)(mask >> (32 * half)); }

// Occupancy accessors: at(x, y) of a cell that may lie anywhere -- outside the image nothing is occupied and nothing is read.
// The bit image of one frame, or the rows [row0, row0 + rows) of it (what a workgroup keeps in LDS) ...
struct PwppVisBits {
    const uint32_t *w;  // word 0 of row `row0`
    int32_t row_words, row0, rows, nx;
    PWPP_HD inline bool at(int x, int y) const {
        const int r = y - row0;
        if ((unsigned)x >= (unsigned)nx || (unsigned)r >= (unsigned)rows) return false;
        return (w[(size_t)r * (size_t)row_words + (size_t)(x >> 5)] >> (x & 31)) & 1u;
    }
};
// ... and the count image itself: the yardstick
struct PwppVisCounts {
    const int32_t *c;  // cell 0 of the frame
    int32_t nx, ny, min_count;
    PWPP_HD inline bool at(int x, int y) const {
        if ((unsigned)x >= (unsigned)nx || (unsigned)y >= (unsigned)ny) return false;
        return c[(size_t)y * (size_t)nx + (size_t)x] >= min_count;
    }
};

// ---- the line ---------------------------------------------------------------------------------------------------------------------
struct PwppVisLine {
    int32_t x, y;        // P_k
    int32_t sx, sy;      // sgn(dx), sgn(dy)
    uint32_t ax2, ay2;   // 2|dx|, 2|dy|
    uint32_t ex, ey;     // (2k|dx| + n) mod 2n, (2k|dy| + n) mod 2n
    uint32_t n, n2;      // n, 2n
};

PWPP_HD inline void pwpp_vis_line(int ox, int oy, int cx, int cy, PwppVisLine &L) {
    const int dx = cx - ox, dy = cy - oy;
    const uint32_t ax = (uint32_t)(dx < 0 ? -dx : dx), ay = (uint32_t)(dy < 0 ? -dy : dy);
    L.x = ox, L.y = oy;
    L.sx = (dx > 0) - (dx < 0), L.sy = (dy > 0) - (dy < 0);
    L.ax2 = 2u * ax, L.ay2 = 2u * ay;
    L.n = ax > ay ? ax : ay, L.n2 = 2u * L.n;
    L.ex = L.ey = L.n;
}

// P_{k-1} -> P_k; true when BOTH coordinates moved
PWPP_HD inline bool pwpp_vis_step(PwppVisLine &L) {
    L.ex += L.ax2, L.ey += L.ay2;
    const bool mx = L.ex >= L.n2, my = L.ey >= L.n2;
    if (mx) L.ex -= L.n2, L.x += L.sx;
    if (my) L.ey -= L.n2, L.y += L.sy;
    return mx && my;
}

// P_0 -> P_k in one move, by the closed form itself: only on a line as pwpp_vis_line left it, with n >= 1 and k <= n.  The same
// state k calls of pwpp_vis_step leave (tools/beams_check.cpp compares them).  2k|d| + n < 2^31: sides are at most 32768.
PWPP_HD inline void pwpp_vis_jump(PwppVisLine &L, uint32_t k) {
    const uint32_t tx = k * L.ax2 + L.n, ty = k * L.ay2 + L.n;
    L.x += L.sx * (int32_t)(tx / L.n2), L.ex = tx % L.n2;
    L.y += L.sy * (int32_t)(ty / L.n2), L.ey = ty % L.n2;
}

// first of the cell c = (cx, cy) seen from o = (ox, oy), both inside the image of nx columns: the index jy * nx + jx of the first
// occupied cell on the line by the rules (a) and (b), PWPP_VIS_FIRST_NONE when there is none, PWPP_VIS_FIRST_BEYOND when
// n > max_range > 0 (nothing is read then).  The loop is bounded by n <= max(nx, ny).
template <class Occ>
PWPP_HD inline int32_t pwpp_vis_walk(const Occ &occ, int ox, int oy, int cx, int cy, int nx, int max_range) {
    PwppVisLine L;
    pwpp_vis_line(ox, oy, cx, cy, L);
    if (max_range > 0 && L.n > (uint32_t)max_range) return PWPP_VIS_FIRST_BEYOND;
    if (L.n == 0) return occ.at(cx, cy) ? cy * nx + cx : PWPP_VIS_FIRST_NONE;
    for (uint32_t k = 1; k <= L.n; ++k) {
        const int px = L.x, py = L.y;
        if (pwpp_vis_step(L) && occ.at(px, L.y) && occ.at(L.x, py)) {  // (a): A = (x_{k-1}, y_k), B = (x_k, y_{k-1})
            const int32_t a = L.y * nx + px, b = py * nx + L.x;
            return a < b ? a : b;
        }
        if (occ.at(L.x, L.y)) return L.y * nx + L.x;  // (b)
    }
    return PWPP_VIS_FIRST_NONE;
}

// the tri-state byte of a cell: occupied wherever it holds returns, seen or not; free where the line to it is clear; else unknown
PWPP_HD inline int8_t pwpp_vis_occupancy(bool occupied, int32_t first) {
    return occupied ? (int8_t)PWPP_VIS_OCCUPIED : (first == PWPP_VIS_FIRST_NONE ? (int8_t)PWPP_VIS_FREE : (int8_t)PWPP_VIS_UNKNOWN);
}

#endif
