// box_arith_check.cpp -- the arithmetic of the obstacle boxes (patchwork-plusplus_amd/csrc/pwpp_boxes.h: the functions the kernels
// and pwpp_box_points compile) on the host, against a computation of its own in __int128 and long double, over random and
// adversarial rows.  Stand-alone: its own main, no library, no device.  tests/test_obstacle_boxes_cpu.py builds it with the address
// and undefined-behaviour sanitizers where the toolchain links them and runs it as a child process.
//   g++ -std=c++17 -O1 -g -I patchwork-plusplus_amd/csrc tools/box_arith_check.cpp -o box_arith_check && ./box_arith_check
// What is checked per row:
//   * the integer moments summed here in __int128 from pwpp_box_quantise, the covariance's three 128-bit integers and their
//     conversion bit for bit against the compiler's own __int128 -> double conversion (correctly rounded);
//   * the axis: unit length, the sign rule, and that it IS the eigenvector of the larger eigenvalue -- the residual of
//     (M - lambda I) u in long double, relative to the matrix, within 2^-48;
//   * sigma_long >= sigma_short >= 0 and both against long double within 2^-22 relative (they are floats);
//   * the box: every point's (p, q) lies inside [min, max] taken through the keys, length, width and the centre against long double.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "pwpp_boxes.h"

namespace {

typedef long double ld;
int cases = 0, mismatches = 0;

void fail(const char *what, int id) {
    if (++mismatches <= 20) std::printf("MISMATCH case %d: %s\n", id, what);
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

void check_conversion(__int128 v, int id) {
    if (!same_bits(pwpp_box_i128_to_double(v), (double)v)) fail("i128_to_double differs from the compiler's conversion", id);
}

struct Pt {
    double dx, dy;
    float hgt, z;
};

void check_row(const std::vector<Pt> &pts, double x0, double y0) {
    const int id = cases++;
    __int128 N = 0, Sx = 0, Sy = 0, Sxx = 0, Sxy = 0, Syy = 0;
    for (const Pt &p : pts) {
        const long long qx = pwpp_box_quantise(p.dx), qy = pwpp_box_quantise(p.dy);
        if (std::fabs((ld)qx - (ld)p.dx * 1024.0L) > 0.5L || std::fabs((ld)qy - (ld)p.dy * 1024.0L) > 0.5L) fail("quantise is off the nearest integer", id);
        N += 1, Sx += qx, Sy += qy, Sxx += (__int128)qx * qx, Sxy += (__int128)qx * qy, Syy += (__int128)qy * qy;
    }
    if (Sxx >= ((__int128)1 << 63)) return fail("a sum beyond 2^63: the case is outside the contract", id);
    const __int128 A = N * Sxx - Sx * Sx, B = N * Sxy - Sx * Sy, C = N * Syy - Sy * Sy;
    double a, b, c;
    pwpp_box_covariance((long long)N, (long long)Sx, (long long)Sy, (long long)Sxx, (long long)Sxy, (long long)Syy, a, b, c);
    if (!same_bits(a, (double)A) || !same_bits(b, (double)B) || !same_bits(c, (double)C)) fail("covariance differs from the 128-bit integers", id);
    check_conversion(A, id), check_conversion(-A, id), check_conversion(B, id), check_conversion(C, id);
    if (A < 0 || C < 0) fail("a negative variance", id);
    double r, ux, uy;
    pwpp_box_axis(a, b, c, r, ux, uy);
    if (std::fabs((ld)ux * ux + (ld)uy * uy - 1.0L) > 0x1p-50L) fail("the axis is not a unit vector", id);
    if (ux < 0.0 || (ux == 0.0 && uy <= 0.0)) fail("the sign rule", id);
    const ld d = ((ld)a - (ld)c) / 2, gap = std::sqrt(d * d + (ld)b * b), mean = ((ld)a + (ld)c) / 2, lambda = mean + gap;
    const ld size = std::fabs((ld)a) + std::fabs((ld)c) + std::fabs((ld)b);
    if (gap > 0) {
        const ld rx = ((ld)a - lambda) * ux + (ld)b * uy, ry = (ld)b * ux + ((ld)c - lambda) * uy;
        // (the residual of an eigenvector whose direction is off by e is e * 2 gap: the bound is on the residual, relative to the matrix)
        if (std::sqrt(rx * rx + ry * ry) > 0x1p-48L * size) fail("the axis is not the eigenvector of the larger eigenvalue", id);
    } else if (!(ux == 1.0 && uy == 0.0)) {
        fail("no direction: (1, 0) expected", id);
    }
    const PwppBoxAxis s = pwpp_box_solve((long long)N, (long long)Sx, (long long)Sy, (long long)Sxx, (long long)Sxy, (long long)Syy, x0, y0);
    if (s.ax != (float)ux || s.ay != (float)uy) fail("solve and axis disagree", id);
    const ld scale = (ld)N * 1024.0L, sl = std::sqrt(lambda) / scale, ss = std::sqrt(mean - gap > 0 ? mean - gap : 0.0L) / scale;
    if (!(s.sigma_long >= s.sigma_short && s.sigma_short >= 0.0f)) fail("sigma_long >= sigma_short >= 0", id);
    if (std::fabs((ld)s.sigma_long - sl) > 0x1p-22L * sl + 0x1p-140L) fail("sigma_long", id);
    // (m - r cancels: its absolute error is that of m and r, 2^-52 of lambda; under the root and against the float's own rounding)
    if (std::fabs((ld)s.sigma_short * s.sigma_short - ss * ss) > 0x1p-21L * ss * ss + 0x1p-50L * sl * sl + 0x1p-140L) fail("sigma_short", id);
    const ld mx = (ld)x0 + ((ld)Sx / (ld)N) / 1024.0L, my = (ld)y0 + ((ld)Sy / (ld)N) / 1024.0L;
    if (std::fabs((ld)s.mean_x - mx) > 0x1p-23L * std::fabs(mx) + 0x1p-40L || std::fabs((ld)s.mean_y - my) > 0x1p-23L * std::fabs(my) + 0x1p-40L) fail("mean", id);
    uint32_t keys[PWPP_BOX_KEYS];
    for (int k = 0; k < PWPP_BOX_KEYS; ++k) keys[k] = (k & 1) ? PWPP_BOX_KEY_NO_MAX : PWPP_BOX_KEY_NO_MIN;
    std::vector<float> ps, qs;
    for (const Pt &p : pts) {
        float pp, qq;
        pwpp_box_project(p.dx, p.dy, s.ax, s.ay, pp, qq);
        if (std::fabs((ld)pp - ((ld)p.dx * s.ax + (ld)p.dy * s.ay)) > 0x1p-22L * 2048.0L) fail("projection", id);
        ps.push_back(pp), qs.push_back(qq);
        const uint32_t k[4] = {pwpp_height_key(pp), pwpp_height_key(qq), pwpp_height_key(p.hgt), pwpp_height_key(p.z)};
        for (int j = 0; j < 4; ++j) {
            keys[2 * j] = k[j] < keys[2 * j] ? k[j] : keys[2 * j];
            keys[2 * j + 1] = k[j] > keys[2 * j + 1] ? k[j] : keys[2 * j + 1];
        }
    }
    uint32_t w[16];
    pwpp_box_row((long long)N, s, keys, x0, y0, w);
    float f[14];
    std::memcpy(f, w + 2, sizeof f);
    if (w[0] != (uint32_t)N || w[1] != 0u) fail("points / pad_", id);
    float pmin = ps[0], pmax = ps[0], qmin = qs[0], qmax = qs[0], hmin = pts[0].hgt, hmax = pts[0].hgt, zmin = pts[0].z, zmax = pts[0].z;
    for (size_t i = 0; i < pts.size(); ++i) {
        pmin = std::fmin(pmin, ps[i]), pmax = std::fmax(pmax, ps[i]), qmin = std::fmin(qmin, qs[i]), qmax = std::fmax(qmax, qs[i]);
        hmin = std::fmin(hmin, pts[i].hgt), hmax = std::fmax(hmax, pts[i].hgt), zmin = std::fmin(zmin, pts[i].z), zmax = std::fmax(zmax, pts[i].z);
    }
    if (f[6] != (float)((double)pmax - (double)pmin) || f[7] != (float)((double)qmax - (double)qmin)) fail("length / width", id);
    if (f[10] != hmin || f[11] != hmax || f[12] != zmin || f[13] != zmax) fail("vertical extent", id);
    const ld pc = ((ld)pmin + pmax) / 2, qc = ((ld)qmin + qmax) / 2;
    const ld cx = (ld)x0 + (pc * s.ax - qc * s.ay), cy = (ld)y0 + (pc * s.ay + qc * s.ax);
    if (std::fabs((ld)f[2] - cx) > 0x1p-23L * std::fabs(cx) + 0x1p-40L || std::fabs((ld)f[3] - cy) > 0x1p-23L * std::fabs(cy) + 0x1p-40L) fail("centre", id);
}

}  // namespace

int main() {
    std::mt19937_64 rng(20261018);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    // conversions at the rounding boundaries: 53, 54 and 55 significant bits at every shift, ties and their neighbours
    for (int sh = 0; sh <= 62; ++sh)
        for (unsigned long long m : {(1ull << 53) + 1, (1ull << 54) + 1, (1ull << 54) + 2, (1ull << 54) + 3, (1ull << 55) + 4, (1ull << 55) + 5, ~0ull, 1ull}) {
            const __int128 v = (__int128)m << sh;
            for (int e = -1; e <= 1; ++e) check_conversion(v + e, cases), check_conversion(-(v + e), cases);
            ++cases;
        }
    // random rows: rectangles at every heading, near and far from the grid's origin (q up to 2^20)
    for (int k = 0; k < 400; ++k) {
        const int n = 1 + (int)(uni(rng) * (k % 7 == 0 ? 3000 : 60));
        const double off = k % 3 == 0 ? 1000.0 : (k % 3 == 1 ? 500.0 : 15.0), len = 0.01 + uni(rng) * 20.0, wid = k % 5 == 0 ? 0.0 : uni(rng) * len;
        const double yaw = uni(rng) * 6.283185307179586, x0 = -1000.0 - uni(rng), y0 = -1000.0 + uni(rng);
        std::vector<Pt> pts;
        for (int i = 0; i < n; ++i) {  // (float coordinates, as the library reads them; 0 < dx, dy < 1024)
            const double u = (uni(rng) - 0.5) * len, v = (uni(rng) - 0.5) * wid;
            const float x = (float)(x0 + off + u * std::cos(yaw) - v * std::sin(yaw)), y = (float)(y0 + off + u * std::sin(yaw) + v * std::cos(yaw));
            pts.push_back({(double)x - x0, (double)y - y0, (float)(uni(rng) * 3.0 - 0.5), (float)(uni(rng) * 2.0 - 1.7)});
        }
        check_row(pts, x0, y0);
    }
    // adversarial rows
    const double far = 1023.0;
    check_row({{3.25, 7.5, 0.5f, -1.0f}}, -10.0, -10.0);                                             // one point
    check_row({{3.25, 7.5, 0.5f, -1.0f}, {3.25, 7.5, -0.0f, 0.0f}, {3.25, 7.5, 0.0f, -0.0f}}, 0.0, 0.0);  // coincident, signed zeros
    check_row({{2.0, 1.0, 0.1f, 0.1f}, {2.0, 5.0, 0.2f, 0.3f}}, 0.0, 0.0);                             // a vertical line: A == 0
    check_row({{1.0, 5.0, 0.1f, 0.1f}, {9.0, 5.0, 0.2f, 0.3f}}, 0.0, 0.0);                             // a horizontal line: C == 0
    check_row({{1.0, 1.0, 0.f, 0.f}, {3.0, 1.0, 0.f, 0.f}, {1.0, 3.0, 0.f, 0.f}, {3.0, 3.0, 0.f, 0.f}}, 0.0, 0.0);  // a square: isotropic
    check_row({{1.0, 3.0, 0.f, 0.f}, {3.0, 1.0, 0.f, 0.f}}, 5.0, 5.0);                                 // the falling diagonal: uy < 0 before the sign rule
    check_row({{1.0, 1.0, 0.f, 0.f}, {3.0, 3.0, 0.f, 0.f}}, 5.0, 5.0);                                 // the rising diagonal
    check_row({{0.0, 0.0, 0.f, 0.f}, {1024.0, 1024.0, 1.f, 1.f}}, -1000.0, -1000.0);                   // the grid's two corners
    check_row({{0.00048828125, 0.00146484375, 0.f, 0.f}, {0.00244140625, 0.0, 0.f, 0.f}}, 0.0, 0.0);   // ties of the quantiser: 0.5, 1.5, 2.5
    check_row({{far, far, -INFINITY, -INFINITY}, {far + 0.5, far + 0.25, INFINITY, INFINITY}}, 0.0, 0.0);  // infinite heights and z
    {  // 2^17 points at the far corner in a thin line: N * Sxx far beyond 2^64
        std::vector<Pt> pts;
        for (int i = 0; i < (1 << 17); ++i) pts.push_back({far + (i % 1024) / 1024.0, far + (i % 1024) / 4096.0 + (i % 3) / 1024.0, 0.1f * (i % 7), 0.01f * (i % 5)});
        check_row(pts, -1000.0, -1000.0);
    }
    uint32_t w[16], keys[PWPP_BOX_KEYS] = {0};  // an empty row
    pwpp_box_row(0, PwppBoxAxis{0, 0, 0, 0, 0, 0}, keys, 0.0, 0.0, w);
    ++cases;
    for (int k = 0; k < 16; ++k)
        if (w[k] != (k < 2 ? 0u : 0x7fc00000u)) fail("the empty row", cases);
    std::printf("%d cases, %d mismatches\n", cases, mismatches);
    return mismatches ? 1 : 0;
}
