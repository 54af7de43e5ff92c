// pwpp_boxes.h -- the arithmetic of the obstacle boxes (pwpp_box_obstacles, pwpp_box_points), one text for the kernels
// (k_box_moments / k_box_extents in pwpp_kernels.hip, the row kernels in pwpp_clusters.hip), for the host function
// pwpp_box_points and for the host program that checks it against a long double / __int128 computation of its own
// (tools/box_arith_check.cpp), the way pwpp_unionfind.h is one text for the clusters.  Internal; include/pwpp.h has the contract.
//
// A row (one box) is reduced from its points in two passes.  Both passes accumulate INTEGERS -- sums of coordinates on a
// 1/1024 m grid, minima and maxima of the monotone keys of floats -- so a row is a function of the SET of its points: integer
// adds, minima and maxima commute.  Between and behind the passes every output is rounded once from exact or double operands,
// with + - * / sqrt only and no FMA (the files that include this are compiled with -ffp-contract=off).
#ifndef PWPP_BOXES_H
#define PWPP_BOXES_H

#include <math.h>
#include <stdint.h>

#include "pwpp_unionfind.h"  // PWPP_HD, pwpp_height_key

// The accumulators of one row in the handle's cluster buffer: 20 words, 8-byte aligned.
//   words 0..11   six int64 sums: N, Sx, Sy, Sxx, Sxy, Syy                                 (first pass)
//   words 12..19  eight keys: p min, p max, q min, q max, hgt min, hgt max, z min, z max     (second pass)
#define PWPP_BOX_SUMS 6
#define PWPP_BOX_KEYS 8
#define PWPP_BOX_ACC_WORDS (2 * PWPP_BOX_SUMS + PWPP_BOX_KEYS)
#define PWPP_BOX_KEY_NO_MIN 0xffffffffu  // the empty minimum: the key of a NaN that is never counted
#define PWPP_BOX_KEY_NO_MAX 0u           // the empty maximum, as in pwpp_rasterize_obstacles
#define PWPP_BOX_MAX_EXTENT 1024.0       // nx * cell and ny * cell, metres: keeps |q| <= 2^20 + 1 and every sum of 2^22 points below 2^63

// step 1: a coordinate relative to the grid's origin on the 1/1024 m grid, ties to even (d * 1024 is exact)
PWPP_HD inline long long pwpp_box_quantise(double d) { return llrint(d * 1024.0); }

// one rounding, to nearest even (the text of pwpp_common.hpp's i128_to_double, for host and device)
PWPP_HD inline double pwpp_box_i128_to_double(__int128 v) {
    const bool neg = v < 0;
    const unsigned __int128 a = neg ? (unsigned __int128)(-v) : (unsigned __int128)v;
    const unsigned long long hi = (unsigned long long)(a >> 64), lo = (unsigned long long)a;
    double r;
    if (hi == 0) {
        r = (double)lo;
    } else {
        const int sh = 64 - __builtin_clzll(hi);  // bits above bit 63
        unsigned long long top = (unsigned long long)(a >> sh);
        const unsigned __int128 rest = a & ((((unsigned __int128)1) << sh) - 1);
        top |= (rest != 0) ? 1ull : 0ull;  // sticky bit, far below the 53-bit mantissa
        r = ldexp((double)top, sh);
    }
    return neg ? -r : r;
}

// step 2: N^2 times the covariance, exact in 128-bit integers, each entry rounded once
PWPP_HD inline void pwpp_box_covariance(long long N, long long Sx, long long Sy, long long Sxx, long long Sxy, long long Syy, double &a, double &b,
                                        double &c) {
    const __int128 n = N, sx = Sx, sy = Sy;
    a = pwpp_box_i128_to_double(n * (__int128)Sxx - sx * sx);
    b = pwpp_box_i128_to_double(n * (__int128)Sxy - sx * sy);
    c = pwpp_box_i128_to_double(n * (__int128)Syy - sy * sy);
}

// step 3: the unit eigenvector of [[a, b], [b, c]] for its larger eigenvalue, ux > 0 or (ux == 0 and uy > 0); r = the half gap.
// (1, 0) when the matrix has no direction: one point, coincident points, an isotropic set.
PWPP_HD inline void pwpp_box_axis(double a, double b, double c, double &r, double &ux, double &uy) {
    const double d = (a - c) * 0.5;
    r = sqrt(d * d + b * b);
    const double vx = d >= 0.0 ? d + r : b, vy = d >= 0.0 ? b : r - d;
    const double n = sqrt(vx * vx + vy * vy);
    if (!(n > 0.0) || !(n <= 1.7976931348623157e308)) {  // (not finite and positive)
        ux = 1.0, uy = 0.0;
        return;
    }
    ux = vx / n, uy = vy / n;
    if (ux < 0.0 || (ux == 0.0 && uy < 0.0)) ux = -ux, uy = -uy;
}

// what is known of a row between the passes
struct PwppBoxAxis {
    float mean_x, mean_y, ax, ay, sigma_long, sigma_short;
};

// steps 2 to 4 for a row with N > 0
PWPP_HD inline PwppBoxAxis pwpp_box_solve(long long N, long long Sx, long long Sy, long long Sxx, long long Sxy, long long Syy, double x0, double y0) {
    double a, b, c, r, ux, uy;
    pwpp_box_covariance(N, Sx, Sy, Sxx, Sxy, Syy, a, b, c);
    pwpp_box_axis(a, b, c, r, ux, uy);
    const double m = (a + c) * 0.5, scale = (double)N * 1024.0, low = m - r;
    PwppBoxAxis o;
    o.ax = (float)ux, o.ay = (float)uy;
    o.sigma_long = (float)(sqrt(m + r) / scale);
    o.sigma_short = (float)(sqrt(low > 0.0 ? low : 0.0) / scale);
    o.mean_x = (float)(x0 + ((double)Sx / (double)N) / 1024.0);
    o.mean_y = (float)(y0 + ((double)Sy / (double)N) / 1024.0);
    return o;
}

// step 5, per point: along (p) and across (q) the FLOAT axis
PWPP_HD inline void pwpp_box_project(double dx, double dy, float ax, float ay, float &p, float &q) {
    const double uxf = (double)ax, uyf = (double)ay;
    p = (float)(dx * uxf + dy * uyf);
    q = (float)(dy * uxf - dx * uyf);
}

// step 5, per row: an extent and its middle from the two keys' floats
PWPP_HD inline void pwpp_box_span(float lo, float hi, float &extent, double &middle) {
    extent = (float)((double)hi - (double)lo);
    middle = ((double)lo + (double)hi) * 0.5;
}
PWPP_HD inline void pwpp_box_centre(double pc, double qc, float ax, float ay, double x0, double y0, float &cx, float &cy) {
    const double uxf = (double)ax, uyf = (double)ay;
    cx = (float)(x0 + (pc * uxf - qc * uyf));
    cy = (float)(y0 + (pc * uyf + qc * uxf));
}

// A finished row as its sixteen 4-byte words (pwpp_obstacle_box: points, pad_, then fourteen floats).  keys: the row's eight keys.
PWPP_HD inline void pwpp_box_row(long long N, const PwppBoxAxis &s, const uint32_t *keys, double x0, double y0, uint32_t *out) {
    if (N <= 0) {
        out[0] = 0u, out[1] = 0u;
        for (int k = 2; k < 16; ++k) out[k] = 0x7fc00000u;
        return;
    }
    float f[14];
    double pc, qc;
    f[0] = s.mean_x, f[1] = s.mean_y, f[4] = s.ax, f[5] = s.ay, f[8] = s.sigma_long, f[9] = s.sigma_short;
    pwpp_box_span(pwpp_height_of_key(keys[0]), pwpp_height_of_key(keys[1]), f[6], pc);
    pwpp_box_span(pwpp_height_of_key(keys[2]), pwpp_height_of_key(keys[3]), f[7], qc);
    pwpp_box_centre(pc, qc, s.ax, s.ay, x0, y0, f[2], f[3]);
    for (int k = 0; k < 4; ++k) f[10 + k] = pwpp_height_of_key(keys[4 + k]);
    out[0] = (uint32_t)N, out[1] = 0u;
    for (int k = 0; k < 14; ++k) out[2 + k] = __builtin_bit_cast(uint32_t, f[k]);
}

#endif
