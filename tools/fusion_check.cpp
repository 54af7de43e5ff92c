// fusion_check.cpp -- the occupancy fusion's arithmetic on the host, against a brute force.
//
// The kernel of patchwork-plusplus_amd/csrc/pwpp_fusion.hip is built from the functions of pwpp_fusion.h (the shifted start, the
// sample positions, the sample's cell under the transposed pose, the observation from four bytes, the clamped update, the derived
// byte).  This program runs the same sequence with the same functions over plain memory, dealt as the kernel deals it -- a map, a
// run of 256 cells, a lane per cell, the map's frames from a CSR in ascending order -- with every array allocated at EXACTLY its
// size (an index outside one is a sanitizer error), on many small random cases: poses that are identities, whole-cell
// translations, quarter turns, mirrors, random rotations, far away and not finite; shifts of both signs and larger than the map;
// skipped frames, maps no frame names; parameters at their extremes; inputs outside the clamps.  It compares the maps and bytes
// with a brute force written separately below: frame by frame over whole maps, its own formulas.  Exit status 0: all equal.
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -I patchwork-plusplus_amd/csrc tools/fusion_check.cpp -o fusion_check
// (tests/test_occupancy_fusion_cpu.py builds and runs it; it needs no GPU and no HIP.)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "pwpp_fusion.h"

namespace {

struct Case {
    PwppFusionGeometry G;
    PwppFusionParams P;
    int frames, n_maps, n_poses;
    std::vector<int8_t> occupancy;      // frames * ny * nx
    std::vector<double> poses;          // n_poses * 6
    std::vector<int32_t> map_of_frame;  // frames
    std::vector<int32_t> shift;         // n_maps * 2
    std::vector<int16_t> map_in;        // n_maps * NY * NX, or empty: null
};

struct Maps {
    std::vector<int16_t> L;
    std::vector<int8_t> byte;
    bool operator==(const Maps &o) const { return L == o.L && byte == o.byte; }
};

// the definition, frame by frame over whole maps
Maps brute_force(const Case &c) {
    const int NX = c.G.NX, NY = c.G.NY, nx = c.G.nx, ny = c.G.ny;
    std::vector<long long> L((size_t)c.n_maps * NY * NX, 0);
    for (int k = 0; k < c.n_maps; ++k)
        for (int jy = 0; jy < NY; ++jy)
            for (int jx = 0; jx < NX; ++jx) {
                const long long qx = (long long)jx + c.shift[2 * k], qy = (long long)jy + c.shift[2 * k + 1];
                if (!c.map_in.empty() && qx >= 0 && qx < NX && qy >= 0 && qy < NY) L[((size_t)k * NY + jy) * NX + jx] = c.map_in[((size_t)k * NY + qy) * NX + qx];
            }
    for (int f = 0; f < c.frames; ++f) {
        const int k = c.map_of_frame[f];
        if (k < 0) continue;
        const double *p = &c.poses[c.n_poses == 1 ? 0 : (size_t)f * 6];
        for (int jy = 0; jy < NY; ++jy)
            for (int jx = 0; jx < NX; ++jx) {
                bool any_occupied = false, all_free = true;
                for (int q = 0; q < 4; ++q) {
                    const double ox = (q & 1) ? 0.75 : 0.25, oy = (q & 2) ? 0.75 : 0.25;
                    const double cx = (double)jx + ox, cy = (double)jy + oy;
                    const double sx = cx * c.G.CELL, sy = cy * c.G.CELL;
                    const double mx = c.G.X0 + sx, my = c.G.Y0 + sy;
                    const double dx = mx - p[2], dy = my - p[5];
                    const double t0 = p[0] * dx, t1 = p[3] * dy, t2 = p[1] * dx, t3 = p[4] * dy;
                    const double fx = t0 + t1, fy = t2 + t3;
                    const double u = (fx - c.G.x0) / c.G.cell, v = (fy - c.G.y0) / c.G.cell;
                    int byte = -1;
                    if (u >= 0.0 && u < nx && v >= 0.0 && v < ny) byte = c.occupancy[((size_t)f * ny + (size_t)std::floor(v)) * nx + (size_t)std::floor(u)];
                    any_occupied = any_occupied || byte == 100;
                    all_free = all_free && byte == 0;
                }
                long long &l = L[((size_t)k * NY + jy) * NX + jx];
                if (any_occupied) l = std::min<long long>(l + c.P.hit, c.P.l_max);
                else if (all_free) l = std::max<long long>(l - c.P.miss, c.P.l_min);
            }
    }
    Maps m{std::vector<int16_t>(L.size()), std::vector<int8_t>(L.size())};
    for (size_t i = 0; i < L.size(); ++i) {
        if (L[i] < -32768 || L[i] > 32767) std::abort();  // (the update keeps an int16)
        m.L[i] = (int16_t)L[i];
        m.byte[i] = L[i] >= c.P.occupied_at ? 100 : (L[i] <= c.P.free_at ? 0 : -1);
    }
    return m;
}

// the kernel's sequence with the header's functions
template <bool RECIP>
Maps as_the_kernel(const Case &c, bool in_place) {
    // the CSR, the counts and the dealing are the shipped ones (pwpp_map_lists, pwpp_map_runs, pwpp_map_lane)
    std::vector<int32_t> begin, list;
    pwpp_map_lists(c.map_of_frame.data(), c.n_maps, c.frames, begin, list);
    PwppMapRuns R;
    const int64_t blocks = pwpp_map_runs(c.G, c.n_maps, c.frames, c.n_poses, (int)list.size(), R);
    const size_t all = (size_t)c.n_maps * R.per_map;
    Maps m{std::vector<int16_t>(all), std::vector<int8_t>(all)};
    if (in_place) m.L = c.map_in;  // (map_out == map_in: every cell read and written by its own lane)
    const int16_t *in = c.map_in.empty() ? nullptr : (in_place ? m.L.data() : c.map_in.data());
    std::vector<int> dealt(all, 0);
    for (int64_t b = 0; b < blocks; ++b)
        for (unsigned lane = 0; lane < PWPP_FUSE_RUN; ++lane)
            pwpp_map_lane(R, c.G.NX, (unsigned)b, lane, c.shift.data(), begin.data(), [&](const PwppMapLane &l) {
                int32_t L = pwpp_fuse_start(in ? in + l.mbase : nullptr, l.jx, l.jy, l.sx, l.sy, c.G.NX, c.G.NY);
                L = pwpp_fuse_cell<RECIP>(c.G, c.P, L, l.jx, l.jy, c.occupancy.data(), c.frames, c.poses.data(), c.n_poses, list.data(), l.first, l.last);
                m.L[l.mbase + l.c] = (int16_t)L;
                m.byte[l.mbase + l.c] = pwpp_fuse_byte(L, c.P);
                ++dealt[l.mbase + l.c];
            });
    for (int n : dealt)
        if (n != 1) std::abort();  // (every cell of every map dealt to exactly one lane)
    return m;
}

}  // namespace

int main() {
    std::mt19937_64 rng(20261019);
    const auto uni = [&](int lo, int hi) { return (int)(lo + (long long)(rng() % (unsigned long long)(hi - lo + 1))); };
    const auto real = [&](double lo, double hi) { return lo + (hi - lo) * (double)(rng() >> 11) / 9007199254740992.0; };
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    long long cases = 0, mismatches = 0;
    for (int t = 0; t < 3000; ++t) {
        Case c;
        const double cells[3] = {0.5, 0.25, 1.0}, frame_cells[4] = {0.5, 0.5, 0.3, 2.0};
        c.G.cell = frame_cells[uni(0, 3)], c.G.CELL = cells[uni(0, 2)];
        const bool recip = pwpp_fuse_reciprocal(c.G.cell, c.G.inv_cell);  // (0.3: the division alone)
        if (recip != (c.G.cell != 0.3)) ++mismatches;
        c.G.nx = uni(1, 20), c.G.ny = uni(1, 20), c.G.NX = t % 7 == 0 ? uni(250, 300) : uni(1, 24), c.G.NY = t % 7 == 0 ? uni(1, 3) : uni(1, 24);
        // the shapes at which the dealing can go wrong: one cell; a lane short of a run, a run, a run and a lane; the last in two maps
        const int edge[5][3] = {{1, 1, 1}, {255, 1, 1}, {256, 1, 1}, {257, 1, 1}, {257, 1, 2}};
        if (t < 5) c.G.NX = edge[t][0], c.G.NY = edge[t][1];
        c.G.x0 = -0.5 * c.G.cell * c.G.nx, c.G.y0 = -0.5 * c.G.cell * c.G.ny;
        c.G.X0 = -0.5 * c.G.CELL * c.G.NX + uni(-2, 2) * c.G.CELL, c.G.Y0 = -0.5 * c.G.CELL * c.G.NY;
        const bool extreme = t % 5 == 0;
        c.P.hit = extreme ? (uni(0, 1) ? 32767 : 0) : uni(0, 300), c.P.miss = extreme ? (uni(0, 1) ? 32767 : 0) : uni(0, 300);
        c.P.l_min = extreme ? -32768 : -uni(0, 500), c.P.l_max = extreme ? 32767 : uni(0, 500);
        c.P.free_at = extreme ? -32768 : uni(-300, 100), c.P.occupied_at = extreme ? 32767 : c.P.free_at + uni(1, 200);
        c.frames = uni(1, 6), c.n_maps = t < 5 ? edge[t][2] : uni(1, 3);
        c.n_poses = uni(0, 1) ? 1 : c.frames;
        c.occupancy.resize((size_t)c.frames * c.G.nx * c.G.ny);
        const int fill = uni(0, 3);
        for (int8_t &b : c.occupancy) {
            const int r = uni(0, 99);
            b = fill == 0 ? -1 : (fill == 1 ? 100 : (r < 2 ? 50 : (r < 55 ? 0 : (r < 75 ? 100 : -1))));
        }
        for (int i = 0; i < c.n_poses; ++i) {
            double p[6] = {1, 0, 0, 0, 1, 0};
            const int kind = uni(0, 7);
            if (kind == 1) p[2] = uni(-6, 6) * c.G.cell, p[5] = uni(-6, 6) * c.G.cell;
            if (kind == 2) p[0] = 0, p[1] = -1, p[3] = 1, p[4] = 0;
            if (kind == 3) p[0] = -1;  // a mirror
            if (kind == 4 || kind == 5) {
                const double th = real(-3.2, 3.2);
                p[0] = std::cos(th), p[1] = -std::sin(th), p[3] = std::sin(th), p[4] = std::cos(th), p[2] = real(-4, 4), p[5] = real(-4, 4);
            }
            if (kind == 6) p[2] = 1e6;                              // wholly outside
            if (kind == 7) p[uni(0, 5)] = uni(0, 1) ? nan : inf;    // not finite: observes nothing
            c.poses.insert(c.poses.end(), p, p + 6);
        }
        for (int f = 0; f < c.frames; ++f) c.map_of_frame.push_back(uni(-1, c.n_maps - 1));
        for (int k = 0; k < c.n_maps; ++k) {
            const int kind = uni(0, 3);
            c.shift.push_back(kind == 0 ? 0 : (kind == 3 ? (uni(0, 1) ? INT32_MAX : INT32_MIN) : uni(-4, 4)));
            c.shift.push_back(kind == 0 ? 0 : uni(-30, 30));
        }
        if (uni(0, 3)) {
            c.map_in.resize((size_t)c.n_maps * c.G.NX * c.G.NY);
            for (int16_t &l : c.map_in) l = (int16_t)(uni(0, 9) == 0 ? (uni(0, 1) ? 32767 : -32768) : uni(-600, 600));  // (outside the clamps too)
        }
        const Maps want = brute_force(c);
        ++cases, mismatches += !(as_the_kernel<false>(c, false) == want);
        if (recip) ++cases, mismatches += !(as_the_kernel<true>(c, false) == want);
        bool still = !c.map_in.empty();
        for (int32_t s : c.shift) still = still && s == 0;
        if (still) ++cases, mismatches += !(as_the_kernel<false>(c, true) == want);
    }
    // the order example of the contract: clamping makes the order matter
    {
        Case c;
        c.G = PwppFusionGeometry{0, 0, 1, 0, 0, 1, 1, 1, 1, 1, 1.0};
        c.P = PwppFusionParams{40, 20, -200, 350, 60, -40};
        c.frames = 2, c.n_maps = 1, c.n_poses = 1;
        c.poses = {1, 0, 0, 0, 1, 0}, c.map_of_frame = {0, 0}, c.shift = {0, 0}, c.map_in = {340};
        c.occupancy = {100, 0};
        ++cases, mismatches += as_the_kernel<true>(c, false).L[0] != 330 || brute_force(c).L[0] != 330;
        c.occupancy = {0, 100};
        ++cases, mismatches += as_the_kernel<true>(c, false).L[0] != 350 || brute_force(c).L[0] != 350;
    }
    // the product with the reciprocal is the quotient: the same bits for numerators of every size, for every power of two that passes
    {
        const double num[] = {0.0, -0.0, 1.0, 3.3, -7.123e-3, 1e308, -1e308, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, inf, -inf, nan, 123456.789};
        for (int e = -1030; e <= 1030; ++e) {
            const double cell = std::ldexp(1.0, e);
            double inv = 0.0;
            if (!pwpp_fuse_reciprocal(cell, inv)) continue;
            for (double n : num) {
                const double q = n / cell, r = n * inv;
                ++cases, mismatches += std::memcmp(&q, &r, sizeof(q)) != 0 && !(std::isnan(q) && std::isnan(r));
            }
        }
        double inv = 0.0;
        for (double cell : {0.3, 0.1, 3.0, 0.0, -0.5, inf, nan, 5e-324, std::ldexp(1.0, 1023), std::ldexp(1.0, -1022)})
            ++cases, mismatches += pwpp_fuse_reciprocal(cell, inv) || inv != 0.0;
    }
    std::printf("fusion_check: %lld cases, %lld mismatches\n", cases, mismatches);
    return mismatches == 0 ? 0 : 1;
}
