// pwpp_terrain.h -- the arithmetic of the terrain analysis (pwpp_terrain_grid, pwpp_terrain_ground), one text for the kernel
// (pwpp_terrain.hip), for the host side (pwpp_capi.cpp) and for the host program that runs the same functions against a brute
// force of its own (tools/terrain_check.cpp), the way pwpp_elevation.h is one text for the elevation fusion.  Internal;
// include/pwpp.h has the contract.
//
// THE CELL.  known iff its height is finite and |height| <= 1024; then z = rint((double)height * 1024), ties to even: the elevation
// fusion's observation with tz = 0 (pwpp_elev_observation), units of 2^-10 m, |z| <= M = 2^20.  Unknown cells are PWPP_TERRAIN_UNKNOWN.
// THE WINDOW of a cell: the known cells at (dx, dy), |dx|, |dy| <= r <= 4, inside the image; k <= 81 of them.  With x = dx, y = dy the
// sums Sx .. Szz are integers, and so are Cuv = k Suv - Su Sv, D = Cxx Cyy - Cxy^2, A = Cxz Cyy - Cyz Cxy, B = Cyz Cxx - Cxz Cxy and
// N = D Czz - A Cxz - B Cyz.  The least-squares plane has the gradient (A / D, B / D) and the mean squared residual N / (D k^2):
// the normal equations of the centred sums are [Cxx Cxy; Cxy Cyy] (a, b)' = (Cxz, Cyz)', and SSR / k = (Czz - a Cxz - b Cyz) / k^2.
// THE BOUNDS, r <= 4.  In the sums: |Sx|, |Sy| <= 81 * 4, Sxx, Syy <= 540 (a full window: 9 * 2 * (1 + 4 + 9 + 16)), |Sz| <= 81 M <
// 2^27, |Sxz|, |Syz| <= 81 * 4 M < 2^29: int32.  Szz <= 81 M^2 < 2^47: int64.  In the C's (a C is k^2 times a covariance, so it does
// not change when a constant is added to a coordinate, and Cuv^2 <= Cuu Cvv, Cauchy-Schwarz):
//   Cxx, Cyy <= 81 * 540 = 43740 < 2^15.42 (k Sxx - Sx^2 <= k Sxx, and k, Sxx are largest for the full window, where Sx = 0)
//   |Cxy| <= sqrt(Cxx Cyy) <= 43740;  0 <= D <= Cxx Cyy <= 43740^2 = 1913187600 < 2^31
//   0 <= Czz <= k Szz <= 81^2 M^2 = 6561 * 2^40 < 2^53; k Szz and Sz^2 <= (81 M)^2 are below 2^53 themselves
//   |Cxz|, |Cyz| <= sqrt(43740 * 6561 * 2^40) < 2^34.1 < 2^35; k |Sxz| < 2^36 and |Sx Sz| < 2^36: int64
//   |A|, |B| <= 2 * 2^34.1 * 43740 < 2^50.6 < 2^51: int64, and exact in a double
//   N: D Czz < 2^84, |A Cxz|, |B Cyz| < 2^86: __int128.  N = D k^3 SSR >= 0, and N <= D Czz < 2^84.
// D == 0 iff the known cells lie on one line (or there are fewer than three): the covariance of (x, y) is singular.
// THE OUTPUTS, in double, every operation rounded on its own, no FMA (the files that include this are compiled with
// -ffp-contract=off); + - * / sqrt only, each correctly rounded on host and device:
//   step  = (float)((double)(zmax - zmin) / 1024.0)                                         (exact: below 2^21 units)
//   slope = (float)(sqrt((double)A * (double)A + (double)B * (double)B) / ((double)D * (1024.0 * cell)))
//   rough = (float)(sqrt(Nd / ((double)D * (double)(k * k))) / 1024.0),  Nd the nearest double of N (pwpp_box_i128_to_double)
//   cost  = -1 where the centre is unknown, D == 0 or k < min_known; else t = max(step / step_max, slope / slope_max, rough /
//           rough_max) in double from the float outputs and the float limits, an infinite limit giving the ratio 0;
//           cost = t >= 1 ? 100 : (int)floor(t * 100.0)
// TWO WAYS TO THE SAME SUMS.  pwpp_terrain_add puts one cell into the moments.  Or a ROW of a window is summed first
// (pwpp_terrain_row_add: k, sx, sxx, sz, sxz, szz, min, max over dx) and the rows are combined with their dy
// (pwpp_terrain_add_row): Sy += dy k, Sxy += dy sx, Syy += dy^2 k, Syz += dy sz, the rest adds up.  Integer adds, minima and maxima
// commute, so both give the same moments, bit for bit.
#ifndef PWPP_TERRAIN_H
#define PWPP_TERRAIN_H

#include <math.h>
#include <stdint.h>

#include "pwpp_boxes.h"      // pwpp_box_i128_to_double
#include "pwpp_elevation.h"  // pwpp_elev_observation, PWPP_HD

#define PWPP_TERRAIN_TILE_X 32  // the output cells of one workgroup: a half wave per row (LDS reads of a row never meet on a bank)
#define PWPP_TERRAIN_TILE_Y 8
#define PWPP_TERRAIN_MAX_R 4
#define PWPP_TERRAIN_UNKNOWN INT32_MIN  // an unknown cell among the quantised ones (|z| <= 2^20)
#define PWPP_TERRAIN_NAN 0x7fc00000u

// what a call fixes for every cell
struct PwppTerrainRule {
    int32_t radius, min_known;
    float step_max, slope_max, rough_max;
    double run;  // 1024.0 * cell: a cell's side in height units (the product is exact)
};

// ---- the quantisation
PWPP_HD inline int32_t pwpp_terrain_quantise(float height) {
    int32_t z = 0;
    return pwpp_elev_observation(height, 0.0, z) ? z : PWPP_TERRAIN_UNKNOWN;
}

// ---- the sums of a window, and of one row of it
struct PwppTerrainMoments {
    int32_t k, Sx, Sy, Sxx, Sxy, Syy, Sz, Sxz, Syz, zmin, zmax;
    int64_t Szz;
};
struct PwppTerrainRow {
    int32_t k, sx, sxx, sz, sxz, zmin, zmax;
    int64_t szz;
};
PWPP_HD inline void pwpp_terrain_clear(PwppTerrainMoments &M) {
    M.k = M.Sx = M.Sy = M.Sxx = M.Sxy = M.Syy = M.Sz = M.Sxz = M.Syz = 0;
    M.zmin = INT32_MAX, M.zmax = INT32_MIN, M.Szz = 0;
}
PWPP_HD inline void pwpp_terrain_row_clear(PwppTerrainRow &W) {
    W.k = W.sx = W.sxx = W.sz = W.sxz = 0;
    W.zmin = INT32_MAX, W.zmax = INT32_MIN, W.szz = 0;
}
// one known cell at (dx, dy) of the window
PWPP_HD inline void pwpp_terrain_add(PwppTerrainMoments &M, int32_t dx, int32_t dy, int32_t z) {
    M.k += 1, M.Sx += dx, M.Sy += dy, M.Sxx += dx * dx, M.Sxy += dx * dy, M.Syy += dy * dy;
    M.Sz += z, M.Sxz += dx * z, M.Syz += dy * z, M.Szz += (int64_t)z * (int64_t)z;
    M.zmin = z < M.zmin ? z : M.zmin, M.zmax = z > M.zmax ? z : M.zmax;
}
// one known cell at dx of a row
PWPP_HD inline void pwpp_terrain_row_add(PwppTerrainRow &W, int32_t dx, int32_t z) {
    W.k += 1, W.sx += dx, W.sxx += dx * dx, W.sz += z, W.sxz += dx * z, W.szz += (int64_t)z * (int64_t)z;
    W.zmin = z < W.zmin ? z : W.zmin, W.zmax = z > W.zmax ? z : W.zmax;
}
// a summed row at dy of the window
PWPP_HD inline void pwpp_terrain_add_row(PwppTerrainMoments &M, int32_t dy, const PwppTerrainRow &W) {
    M.k += W.k, M.Sx += W.sx, M.Sy += dy * W.k, M.Sxx += W.sxx, M.Sxy += dy * W.sx, M.Syy += dy * dy * W.k;
    M.Sz += W.sz, M.Sxz += W.sxz, M.Syz += dy * W.sz, M.Szz += W.szz;
    M.zmin = W.zmin < M.zmin ? W.zmin : M.zmin, M.zmax = W.zmax > M.zmax ? W.zmax : M.zmax;
}
// the sums of a row that depend on the known mask alone, in one word: k <= 9 | sx + 32 (|sx| <= 20) | sxx <= 60
PWPP_HD inline uint32_t pwpp_terrain_row_pack(const PwppTerrainRow &W) { return (uint32_t)W.k | ((uint32_t)(W.sx + 32) << 8) | ((uint32_t)W.sxx << 16); }
PWPP_HD inline void pwpp_terrain_row_unpack(uint32_t w, PwppTerrainRow &W) {
    W.k = (int32_t)(w & 0xffu), W.sx = (int32_t)((w >> 8) & 0xffu) - 32, W.sxx = (int32_t)(w >> 16);
}

// ---- the plane of a window: D, A, B in int64, N in 128 bits
struct PwppTerrainPlane {
    int64_t D, A, B;
    __int128 N;
};
PWPP_HD inline void pwpp_terrain_plane(const PwppTerrainMoments &M, PwppTerrainPlane &P) {
    const int64_t k = M.k, Sx = M.Sx, Sy = M.Sy, Sz = M.Sz;
    const int64_t Cxx = k * M.Sxx - Sx * Sx, Cxy = k * M.Sxy - Sx * Sy, Cyy = k * M.Syy - Sy * Sy;
    const int64_t Cxz = k * M.Sxz - Sx * Sz, Cyz = k * M.Syz - Sy * Sz, Czz = k * M.Szz - Sz * Sz;
    P.D = Cxx * Cyy - Cxy * Cxy;
    P.A = Cxz * Cyy - Cyz * Cxy;
    P.B = Cyz * Cxx - Cxz * Cxy;
    P.N = (__int128)P.D * (__int128)Czz - (__int128)P.A * (__int128)Cxz - (__int128)P.B * (__int128)Cyz;
}

// ---- the outputs
PWPP_HD inline uint32_t pwpp_terrain_bits(float v) {
    uint32_t bits;
    __builtin_memcpy(&bits, &v, sizeof(bits));
    return bits;
}
PWPP_HD inline float pwpp_terrain_step(const PwppTerrainMoments &M) { return (float)((double)(M.zmax - M.zmin) / 1024.0); }  // (k >= 1)
PWPP_HD inline float pwpp_terrain_slope(const PwppTerrainPlane &P, double run) {                                              // (D > 0)
    const double a = (double)P.A, b = (double)P.B;
    return (float)(sqrt(a * a + b * b) / ((double)P.D * run));
}
PWPP_HD inline float pwpp_terrain_rough(const PwppTerrainPlane &P, int32_t k) {  // (D > 0)
    return (float)(sqrt(pwpp_box_i128_to_double(P.N) / ((double)P.D * (double)(k * k))) / 1024.0);
}
PWPP_HD inline double pwpp_terrain_ratio(float v, float limit) { return __builtin_isinf(limit) ? 0.0 : (double)v / (double)limit; }
PWPP_HD inline int32_t pwpp_terrain_cost(const PwppTerrainRule &R, float step, float slope, float rough) {
    const double a = pwpp_terrain_ratio(step, R.step_max), b = pwpp_terrain_ratio(slope, R.slope_max), c = pwpp_terrain_ratio(rough, R.rough_max);
    const double ab = a > b ? a : b, t = ab > c ? ab : c;
    return t >= 1.0 ? 100 : (int32_t)floor(t * 100.0);
}

// ---- one cell from the moments of its window: the bits of step, slope and rough, and the cost
PWPP_HD inline void pwpp_terrain_cell(const PwppTerrainRule &R, const PwppTerrainMoments &M, bool centre_known, uint32_t &step, uint32_t &slope,
                                      uint32_t &rough, int32_t &cost) {
    step = slope = rough = PWPP_TERRAIN_NAN, cost = -1;
    if (!centre_known) return;  // (known: k >= 1)
    const float s = pwpp_terrain_step(M);
    step = pwpp_terrain_bits(s);
    PwppTerrainPlane P;
    pwpp_terrain_plane(M, P);
    if (P.D == 0) return;
    const float g = pwpp_terrain_slope(P, R.run), q = pwpp_terrain_rough(P, M.k);
    slope = pwpp_terrain_bits(g), rough = pwpp_terrain_bits(q);
    if (M.k >= R.min_known) cost = pwpp_terrain_cost(R, s, g, q);
}

#endif
