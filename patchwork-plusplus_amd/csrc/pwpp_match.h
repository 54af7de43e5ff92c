// pwpp_match.h -- the arithmetic of the correlative scan match (pwpp_match_grid, pwpp_match_obstacles), one text for the kernels
// (pwpp_match.hip), for the host side (pwpp_capi.cpp) and for the host program that runs the same functions against a brute force
// of its own (tools/match_check.cpp), the way pwpp_fusion.h is one text for the fusion.  Internal; include/pwpp.h has the contract.
//
// THE LANDING.  An occupied cell (ix, iy) of a frame image lies, under the candidate {a, b, tx, c, d, ty} (map-from-frame, the
// fusion's pose), in the map cell (Jx, Jy):
//     x = x0 + ((double)ix + 0.5) * cell                 y alike           (the cell's centre; ix + 0.5 is exact)
//     X = (a * x + b * y) + tx                           Y = (c * x + d * y) + ty
//     U = (X - X0) / CELL                                V alike
//     lands iff -1048576 <= U < 1048576 and the same for V (a NaN does not);   Jx = (int)floor(U), Jy = (int)floor(V)
// all in double, every product, sum and quotient rounded on its own: the build's -ffp-contract=off is part of the contract.  The
// bound of 2^20 keeps Jx + sx inside an int32 for every shift the host lets through (|sx| <= 64) with room to spare.
// THE QUOTIENT WITHOUT A DIVISION.  Where CELL passes pwpp_fuse_reciprocal, (X - X0) * (1 / CELL) is the same bits as the division:
// the fusion's argument (pwpp_fusion.h).  RECIP = false, the division as written, is what every other CELL takes.
// THE CONTRIBUTION of a landed cell to the shift (sx, sy): map[Jy + sy][Jx + sx] where 0 <= Jx + sx < NX and 0 <= Jy + sy < NY,
// else 0; the two sums are compared with their bounds before an address is formed.
// THE WINDOW.  Along one axis the landed cells of a (frame, candidate) span [lo_J, hi_J]; every contribution of every shift of the
// window reads a map cell of [lo_J - w, hi_J + w] cut to [0, N).  Where that rectangle of the map fits a workgroup's LDS it is
// copied there once and pwpp_match_contribution runs on the copy, with J moved by the rectangle's corner and the rectangle's sides
// for NX and NY: the cells it finds inside are the same cells, so the sums are the same integers.
// THE KEY.  A (score, candidate, sx, sy) beats another by: the larger score; then the smaller sx * sx + sy * sy; then the smaller
// candidate; then the smaller sy; then the smaller sx.  A total order on distinct (candidate, sx, sy): the maximum is unique, so
// the order in which a reduction meets the entries cannot change it.
#ifndef PWPP_MATCH_H
#define PWPP_MATCH_H

#include <math.h>
#include <stdint.h>

#include "pwpp_fusion.h"  // PWPP_HD, pwpp_fuse_reciprocal

#define PWPP_MATCH_OCCUPIED 100       // = PWPP_OCC_OCCUPIED of include/pwpp.h
#define PWPP_MATCH_MAX_SIDE 32768     // NX, NY, nx, ny
#define PWPP_MATCH_MAX_CANDIDATES 256
#define PWPP_MATCH_MAX_WINDOW 64      // wx, wy
#define PWPP_MATCH_REACH 1048576.0    // |U|, |V| of a landing (2^20)
#define PWPP_MATCH_NOWHERE (-(1 << 30))  // Jx, Jy of a cell that does not land: no shift brings it back into a map
#define PWPP_MATCH_CHUNK 256          // occupied cells a workgroup lands at a time, a lane per cell
#define PWPP_MATCH_TILE 256           // shifts of a workgroup, a lane per shift

// The geometry of a call: the map's grid in the fixed frame and the frame images' grid.
struct PwppMatchGeometry {
    double X0, Y0, CELL;  // the map
    double x0, y0, cell;  // the frame images
    int32_t NX, NY, nx, ny;
    double inv_CELL;      // 1 / CELL where pwpp_fuse_reciprocal allows the product, else 0
};

// One entry of the argmax, and one row of the result: the layout of pwpp_match_best (24 bytes, 8-byte aligned).
struct PwppMatchKey {
    int64_t score;
    int32_t candidate, sx, sy, cells;
};

// ---- an occupied cell as one word, and back: iy in the upper half, ix in the lower (both < 32768)
PWPP_HD inline int32_t pwpp_match_pack(int ix, int iy) { return (int32_t)(((uint32_t)iy << 16) | (uint32_t)ix); }
PWPP_HD inline void pwpp_match_unpack(int32_t w, int &ix, int &iy) { ix = (int)((uint32_t)w & 0xffffu), iy = (int)((uint32_t)w >> 16); }

// ---- the landing of the frame cell (ix, iy) under a candidate; false: it lands nowhere (Jx = Jy = PWPP_MATCH_NOWHERE)
template <bool RECIP>
PWPP_HD inline bool pwpp_match_landing(const PwppMatchGeometry &G, const double *cand, int ix, int iy, int32_t &Jx, int32_t &Jy) {
    const double a = cand[0], b = cand[1], tx = cand[2], c = cand[3], d = cand[4], ty = cand[5];
    const double x = G.x0 + ((double)ix + 0.5) * G.cell, y = G.y0 + ((double)iy + 0.5) * G.cell;
    const double X = (a * x + b * y) + tx, Y = (c * x + d * y) + ty;
    const double U = RECIP ? (X - G.X0) * G.inv_CELL : (X - G.X0) / G.CELL, V = RECIP ? (Y - G.Y0) * G.inv_CELL : (Y - G.Y0) / G.CELL;
    Jx = Jy = PWPP_MATCH_NOWHERE;
    if (!(U >= -PWPP_MATCH_REACH && U < PWPP_MATCH_REACH && V >= -PWPP_MATCH_REACH && V < PWPP_MATCH_REACH)) return false;  // (a NaN: nowhere)
    Jx = (int32_t)floor(U), Jy = (int32_t)floor(V);
    return true;
}

// ---- what a landing adds to the sum of the shift (sx, sy); |Jx|, |Jy| <= 2^30 and |sx|, |sy| <= 64: the sums stay in an int32
PWPP_HD inline int32_t pwpp_match_contribution(const int16_t *map /* one map */, int32_t Jx, int32_t Jy, int sx, int sy, int NX, int NY) {
    const int32_t qx = Jx + sx, qy = Jy + sy;
    if (qx < 0 || qx >= NX || qy < 0 || qy >= NY) return 0;
    return (int32_t)map[(size_t)qy * (size_t)NX + (size_t)qx];
}

// ---- the map cells along one axis that the landings [lo_J, hi_J] (lo_J > hi_J: none landed) reach under the shifts -w .. w:
// [first, first + n) inside [0, N); false: none, every contribution is 0
PWPP_HD inline bool pwpp_match_window(int32_t lo_J, int32_t hi_J, int w, int N, int32_t &first, int32_t &n) {
    first = 0, n = 0;
    if (lo_J > hi_J) return false;
    const int32_t lo = lo_J - w > 0 ? lo_J - w : 0, hi = hi_J + w < N - 1 ? hi_J + w : N - 1;  // (|J| <= 2^20, w <= 64)
    if (lo > hi) return false;
    first = lo, n = hi - lo + 1;
    return true;
}

// ---- the order of the argmax: whether p beats q (`cells` takes no part)
PWPP_HD inline bool pwpp_match_better(const PwppMatchKey &p, const PwppMatchKey &q) {
    if (p.score != q.score) return p.score > q.score;
    const int32_t dp = p.sx * p.sx + p.sy * p.sy, dq = q.sx * q.sx + q.sy * q.sy;
    if (dp != dq) return dp < dq;
    if (p.candidate != q.candidate) return p.candidate < q.candidate;
    if (p.sy != q.sy) return p.sy < q.sy;
    return p.sx < q.sx;
}

// ---- the pose to fuse under: the candidate moved by the winning shift, one product and one sum for each of tx and ty
inline void pwpp_match_shifted_pose(const double cand[6], double CELL, int sx, int sy, double out[6]) {
    const double tx = cand[2] + (double)sx * CELL, ty = cand[5] + (double)sy * CELL;
    out[0] = cand[0], out[1] = cand[1], out[2] = tx, out[3] = cand[3], out[4] = cand[4], out[5] = ty;
}

#endif
