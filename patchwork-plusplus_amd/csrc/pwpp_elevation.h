// pwpp_elevation.h -- the arithmetic of the elevation fusion (pwpp_fuse_height_grid, pwpp_fuse_ground), one text for the kernel
// (pwpp_elevation.hip), for the host side (pwpp_capi.cpp) and for the host program that runs the same functions against a brute
// force of its own (tools/elevation_check.cpp), the way pwpp_fusion.h is one text for the occupancy fusion.  Internal;
// include/pwpp.h has the contract.
//
// THE SAMPLE.  A map cell (jx, jy) asks a frame at its centre: mx = X0 + ((double)jx + 0.5) * CELL, then the frame cell under it by
// pwpp_fuse_cell_of (pwpp_fusion.h): the occupancy fusion's pose, transpose and cell rule, in double, no FMA, with the same choice
// between the division by cell and the product with its exact reciprocal (RECIP).
// THE OBSERVATION.  Z = (double)height + tz, one add; observed iff Z is finite and |Z| <= 1024; q = the nearest integer of Z * 1024,
// ties to even (the product by 2^10 is exact): |q| <= M = 2^20, units of 2^-10 m.
// THE STATE of a cell: n observations remembered and the sum of their q.  An input is normalised first: n into [0, n_max], sum into
// [-n M, n M].  THE UPDATE: below n_max the exact running sum, sum += q, n += 1; at n_max the mean forgets one share of itself,
// sum = sum - sum / n + q with the division truncating toward zero.  |sum| <= n M stays true: |s - trunc(s / n)| = |s| -
// floor(|s| / n) <= (n - 1) M for |s| <= n M, and |q| <= M.  With n_max <= 1023 that is below 2^30: int32 never overflows.
// THE DIVISION WITHOUT A DIVISION.  At n_max the divisor is n_max itself, a constant of the call.  For d in 1 .. 1023 take l with
// 2^l >= d, sh = 30 + l and m = ceil(2^sh / d) <= 2^31: m d = 2^sh + e with 0 <= e < d, so x m / 2^sh = x / d + x e / (d 2^sh), and
// for 0 <= x < 2^30 the second term is below 1 / d: floor(x m / 2^sh) = floor(x / d), the product below 2^61 (Granlund and
// Montgomery 1994).  pwpp_elev_magic computes (m, sh) on the host; FAST = false, the division as written, is the yardstick.
#ifndef PWPP_ELEVATION_H
#define PWPP_ELEVATION_H

#include <math.h>
#include <stdint.h>

#include "pwpp_fusion.h"  // PwppFusionGeometry, pwpp_fuse_reciprocal, pwpp_fuse_cell_of, PWPP_FUSE_RUN

#define PWPP_ELEV_M 1048576       // 2^20: |q| of one observation, 1024 m in units of 2^-10 m
#define PWPP_ELEV_MAX_N 1023      // n_max
#define PWPP_ELEV_NAN 0x7fc00000u  // the mean of a cell with no observation

// the update's parameters: n_max, and the multiply-shift that divides 0 .. 2^30 - 1 by it
struct PwppElevationParams {
    int32_t n_max;
    uint32_t shift;  // 30 + l
    uint64_t magic;  // ceil(2^shift / n_max)
};

inline PwppElevationParams pwpp_elev_magic(int32_t n_max) {
    PwppElevationParams P{n_max, 30u, (uint64_t)1 << 30};
    if (n_max < 1 || n_max > PWPP_ELEV_MAX_N) return P;
    uint32_t l = 0;
    while (((int32_t)1 << l) < n_max) ++l;
    P.shift = 30u + l;
    P.magic = (((uint64_t)1 << P.shift) + (uint64_t)n_max - 1) / (uint64_t)n_max;
    return P;
}

// ---- the centre of a cell along one axis, in the map's frame
PWPP_HD inline double pwpp_elev_position(double X0, int j, double CELL) { return X0 + ((double)j + 0.5) * CELL; }

// ---- the start of a cell: the shifted read of both words, normalised.  (jx + sx, jy + sy) in 64 bits, as in pwpp_fuse_start.
PWPP_HD inline void pwpp_elev_start(const int32_t *sum_in, const int16_t *n_in /* one map, or both null */, int jx, int jy, int32_t sx, int32_t sy, int NX, int NY,
                                    int32_t n_max, int32_t &sum, int32_t &n) {
    const int64_t qx = (int64_t)jx + (int64_t)sx, qy = (int64_t)jy + (int64_t)sy;
    sum = 0, n = 0;
    if (!sum_in || !n_in || qx < 0 || qx >= (int64_t)NX || qy < 0 || qy >= (int64_t)NY) return;
    const size_t at = (size_t)qy * (size_t)NX + (size_t)qx;
    const int32_t n0 = (int32_t)n_in[at];
    n = n0 < 0 ? 0 : (n0 > n_max ? n_max : n0);
    const int64_t bound = (int64_t)n * PWPP_ELEV_M, s0 = (int64_t)sum_in[at];
    sum = (int32_t)(s0 < -bound ? -bound : (s0 > bound ? bound : s0));
}

// ---- the observation: false where the sample observes nothing
PWPP_HD inline bool pwpp_elev_observation(float height, double tz, int32_t &q) {
    const double Z = (double)height + tz;
    if (!(fabs(Z) <= 1024.0)) return false;  // (a NaN or an infinity: no observation)
    q = (int32_t)rint(Z * 1024.0);           // (round to nearest, ties to even; |Z * 1024| <= 2^20, exact)
    return true;
}

// ---- trunc(sum / n_max) for |sum| <= n_max M
template <bool FAST>
PWPP_HD inline int32_t pwpp_elev_share(int32_t sum, const PwppElevationParams &P) {
    if (!FAST) return sum / P.n_max;
    const uint64_t x = (uint64_t)(sum < 0 ? -(int64_t)sum : (int64_t)sum);
    const int32_t s = (int32_t)((x * P.magic) >> P.shift);
    return sum < 0 ? -s : s;
}

// ---- the update
template <bool FAST>
PWPP_HD inline void pwpp_elev_update(int32_t &sum, int32_t &n, int32_t q, const PwppElevationParams &P) {
    if (n < P.n_max) sum += q, n += 1;
    else sum = sum - pwpp_elev_share<FAST>(sum, P) + q;
}

// ---- the bits of the mean
PWPP_HD inline uint32_t pwpp_elev_mean_bits(int32_t sum, int32_t n) {
    if (n <= 0) return PWPP_ELEV_NAN;
    const float mean = (float)(((double)sum / (double)n) / 1024.0);
    uint32_t bits;
    __builtin_memcpy(&bits, &mean, sizeof(bits));
    return bits;
}

// ---- one map cell from its start to its end: the frames list[first .. last) of the cell's map in that order; `frames`: the number
// of frame images, every entry of the list is compared with it; `n_poses`: 1 (poses[0 .. 6) and z_offset[0] for every frame) or frames.
template <bool RECIP, bool FAST>
PWPP_HD inline void pwpp_elev_cell(const PwppFusionGeometry &G, const PwppElevationParams &P, int32_t &sum, int32_t &n, int jx, int jy, const float *height,
                                   int32_t frames, const double *poses, const double *z_offset, int32_t n_poses, const int32_t *list, int32_t first, int32_t last) {
    const double mx = pwpp_elev_position(G.X0, jx, G.CELL), my = pwpp_elev_position(G.Y0, jy, G.CELL);
    const size_t per_frame = (size_t)G.nx * (size_t)G.ny;
    for (int32_t i = first; i < last; ++i) {
        const int32_t f = list[i];
        if ((uint32_t)f >= (uint32_t)frames) continue;  // (the host never lists one)
        const size_t p = n_poses == 1 ? (size_t)0 : (size_t)f;
        int ix = 0, iy = 0;
        int32_t q = 0;
        if (!pwpp_fuse_cell_of<RECIP>(G, poses + p * 6, mx, my, ix, iy)) continue;
        if (!pwpp_elev_observation(height[(size_t)f * per_frame + (size_t)iy * (size_t)G.nx + (size_t)ix], z_offset[p], q)) continue;
        pwpp_elev_update<FAST>(sum, n, q, P);
    }
}

#endif
