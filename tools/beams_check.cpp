// beams_check.cpp -- the walks of the per-beam free space on the host, against a brute force.
//
// The kernels of patchwork-plusplus_amd/csrc/pwpp_beams.hip are built from the functions of pwpp_beams.h and, for the line, of
// pwpp_visibility.h.  This program deals the same functions over plain memory as the kernels deal them: path 1 as a walk per endpoint
// cell over the whole image (pwpp_beams_walk), path 2 as a walk per (tile, endpoint) over a buffer of EXACTLY the tile's size
// (pwpp_beams_walk_tile into what k_beam_tile keeps in LDS: a word outside it is a sanitizer error), the tile then copied out with
// the byte -- and compares passes, low and occupancy with a brute force of its own: the closed form of every point with its own
// divisions, every beam traced whole.  Random endpoint images with heights that reach +-R and beyond, cells with hits but no
// height, weights that wrap the sum, origins in corners, on edges and inside, eyes at +-2^30, max_range 0, 1, 5 and 40, with and
// without target and base bytes.  It also checks pwpp_vis_jump against k steps, that the height is monotone in z, the worked row of
// include/pwpp.h, max_range against the unlimited call, the two theorems about the bytes, and the byte rule on every combination of
// base byte, passes against min_pass and target (none, no height, at, below and above low - clearance; clearances up to INT32_MAX).
// Exit status 0: all equal.  With --bytes it prints that matrix instead, a row per combination.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I patchwork-plusplus_amd/csrc tools/beams_check.cpp -o beams_check
// (tests/test_beams_cpu.py builds and runs it; it needs no GPU and no HIP.)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "pwpp_beams.h"

namespace {

constexpr long long kR = 1 << 20;
constexpr int32_t kNoHeight = INT32_MIN;
constexpr int8_t kFree = 0, kOccupied = 100, kUnknown = -1;

struct Scene {
    int nx, ny;
    std::vector<int32_t> hits, zmin, target;
    std::vector<int8_t> base;
    bool has_target, has_base;
    uint32_t min_pass;
    int32_t clearance;
};

struct Result {
    std::vector<uint32_t> passes;
    std::vector<int32_t> low;
    std::vector<int8_t> occupancy;
    bool operator==(const Result &o) const { return passes == o.passes && low == o.low && occupancy == o.occupancy; }
};

long long ceil_div(long long num, long long d) { return num >= 0 ? (num + d - 1) / d : -((-num) / d); }

// the definition
Result brute_force(const Scene &s, int ox, int oy, int32_t eye, int max_range) {
    const int nx = s.nx, ny = s.ny;
    const size_t cells = (size_t)nx * ny;
    std::vector<unsigned long long> sum(cells, 0);
    std::vector<long long> low(cells, INT64_MAX);
    for (int ey = 0; ey < ny; ++ey)
        for (int ex = 0; ex < nx; ++ex) {
            const size_t e = (size_t)ey * nx + ex;
            if (s.hits[e] < 1 || s.zmin[e] == kNoHeight) continue;
            const long long dx = ex - ox, dy = ey - oy, ax = std::llabs(dx), ay = std::llabs(dy), n = std::max(ax, ay);
            const long long sx = dx > 0 ? 1 : (dx < 0 ? -1 : 0), sy = dy > 0 ? 1 : (dy < 0 ? -1 : 0);
            const long long r = std::min(kR, std::max(-kR, (long long)s.zmin[e] - eye));
            for (long long k = 1; k < n; ++k) {
                if (max_range > 0 && k > max_range) break;
                const long long x = ox + sx * ((2 * k * ax + n) / (2 * n)), y = oy + sy * ((2 * k * ay + n) / (2 * n));
                if (x < 0 || y < 0 || x >= nx || y >= ny) std::abort();  // (the line never leaves the image)
                const size_t c = (size_t)(y * nx + x);
                sum[c] += (unsigned long long)s.hits[e];
                low[c] = std::min(low[c], eye + ceil_div(r * (r < 0 ? 2 * k - 1 : 2 * k + 1), 2 * n));
            }
        }
    Result res{std::vector<uint32_t>(cells), std::vector<int32_t>(cells), std::vector<int8_t>(cells)};
    for (size_t c = 0; c < cells; ++c) {
        const uint32_t p = (uint32_t)(sum[c] & 0xffffffffull);
        res.passes[c] = p;
        res.low[c] = p == 0 ? kNoHeight : (int32_t)low[c];
        const int8_t base = s.has_base ? s.base[c] : kUnknown;
        bool free_ = base == kUnknown && p >= s.min_pass;
        if (free_ && s.has_target) free_ = s.target[c] != kNoHeight && (long long)res.low[c] - (long long)s.target[c] <= (long long)s.clearance;
        res.occupancy[c] = free_ ? kFree : base;
    }
    return res;
}

void cell_out(const Scene &s, size_t c, uint32_t p, int32_t l, Result &res) {  // beam_cell_out of the kernels
    l = pwpp_beams_low(p, l);
    res.passes[c] = p, res.low[c] = l;
    res.occupancy[c] = pwpp_beams_occupancy(s.has_base ? s.base[c] : kUnknown, p, l, s.has_target, s.has_target ? s.target[c] : 0, s.min_pass, s.clearance);
}

// a sink over plain memory of exactly w x h words whose cell (0, 0) is the image's (x0, y0): a write outside aborts
struct Sink {
    std::vector<uint32_t> &passes;
    std::vector<int32_t> &low;
    int x0, y0, w, h;
    uint32_t weight;
    void cross(int x, int y, int32_t height) {
        if (x < x0 || y < y0 || x >= x0 + w || y >= y0 + h) std::abort();
        const size_t i = (size_t)(y - y0) * w + (size_t)(x - x0);
        passes.at(i) += weight;
        low.at(i) = std::min(low.at(i), height);
    }
};

// PATH 1: fill, a walk per endpoint cell, finish
Result path1(const Scene &s, int ox, int oy, int32_t eye, int max_range) {
    const size_t cells = (size_t)s.nx * s.ny;
    std::vector<uint32_t> p(cells, 0u);
    std::vector<int32_t> l(cells, INT32_MAX);
    for (size_t c = 0; c < cells; ++c) {
        if (!pwpp_beams_endpoint(s.hits[c], s.zmin[c])) continue;
        Sink sink{p, l, 0, 0, s.nx, s.ny, (uint32_t)s.hits[c]};
        pwpp_beams_walk(sink, ox, oy, (int)(c % s.nx), (int)(c / s.nx), eye, s.zmin[c], max_range);
    }
    Result res{std::vector<uint32_t>(cells), std::vector<int32_t>(cells), std::vector<int8_t>(cells)};
    for (size_t c = 0; c < cells; ++c) cell_out(s, c, p[c], l[c], res);
    return res;
}

// PATH 2: per tile, the endpoints the kernel would queue, each walked over the tile alone
Result path2(const Scene &s, int ox, int oy, int32_t eye, int max_range, int tile, long long &queued) {
    const size_t cells = (size_t)s.nx * s.ny;
    Result res{std::vector<uint32_t>(cells), std::vector<int32_t>(cells), std::vector<int8_t>(cells)};
    for (int y0 = 0; y0 < s.ny; y0 += tile)
        for (int x0 = 0; x0 < s.nx; x0 += tile) {
            const int x1 = std::min(s.nx, x0 + tile) - 1, y1 = std::min(s.ny, y0 + tile) - 1, w = x1 - x0 + 1, h = y1 - y0 + 1;
            std::vector<uint32_t> p((size_t)w * h, 0u);
            std::vector<int32_t> l((size_t)w * h, INT32_MAX);
            for (size_t c = 0; c < cells; ++c) {
                if (!pwpp_beams_endpoint(s.hits[c], s.zmin[c])) continue;
                const int ex = (int)(c % s.nx), ey = (int)(c / s.nx);
                bool take = false;
                if (pwpp_beams_near_tile(ox, oy, ex, ey, x0, y0, x1, y1)) {
                    PwppVisLine L;
                    pwpp_vis_line(ox, oy, ex, ey, L);
                    uint32_t k0, k1;
                    take = pwpp_beams_tile_span(L, max_range, x0, y0, x1, y1, k0, k1);
                }
                Sink sink{p, l, x0, y0, w, h, (uint32_t)s.hits[c]};
                if (take) {
                    ++queued;
                    pwpp_beams_walk_tile(sink, ox, oy, ex, ey, eye, s.zmin[c], max_range, x0, y0, x1, y1);
                } else {  // what is not queued crosses no cell of the tile: a full walk that touched one would abort in the sink
                    struct Probe {
                        int x0, y0, x1, y1;
                        void cross(int x, int y, int32_t) {
                            if (x >= x0 && x <= x1 && y >= y0 && y <= y1) std::abort();
                        }
                    } probe{x0, y0, x1, y1};
                    pwpp_beams_walk(probe, ox, oy, ex, ey, eye, s.zmin[c], max_range);
                }
            }
            for (int y = y0; y <= y1; ++y)
                for (int x = x0; x <= x1; ++x) cell_out(s, (size_t)y * s.nx + x, p[(size_t)(y - y0) * w + (x - x0)], l[(size_t)(y - y0) * w + (x - x0)], res);
        }
    return res;
}

Scene random_scene(int nx, int ny, double fill, int32_t eye, bool has_target, bool has_base, std::mt19937 &rng) {
    Scene s{nx, ny, {}, {}, {}, {}, has_target, has_base, 1u + (uint32_t)(rng() % 3u), (int32_t)(rng() % 4000u)};
    const size_t cells = (size_t)nx * ny;
    std::uniform_real_distribution<double> u(0.0, 1.0);
    s.hits.resize(cells), s.zmin.resize(cells), s.target.resize(cells), s.base.resize(cells);
    const long long special[] = {-kR - 1, -kR, kR, kR + 1, 3 * kR, -3 * kR};
    const int8_t bytes[] = {kFree, kOccupied, kUnknown, kUnknown, 42};
    for (size_t c = 0; c < cells; ++c) {
        s.hits[c] = u(rng) < fill ? 1 + (int32_t)(rng() % 5u) : (u(rng) < 0.05 ? -3 : 0);
        long long rise;
        switch (rng() % 4u) {
            case 0: rise = (long long)(rng() % 81u) - 40; break;
            case 1: rise = (long long)(rng() % 6001u) - 3000; break;
            case 2: rise = (long long)(rng() % (2 * kR + 11)) - kR - 5; break;
            default: rise = special[rng() % 6u];
        }
        s.zmin[c] = u(rng) < 0.1 ? kNoHeight : (int32_t)std::min<long long>(INT32_MAX, std::max<long long>(INT32_MIN + 1, eye + rise));
        s.target[c] = u(rng) < 0.1 ? kNoHeight : (int32_t)(eye - 1700 + (long long)(rng() % 600u) - 300);
        s.base[c] = bytes[rng() % 5u];
    }
    return s;
}

// THE BYTE RULE, every combination: base byte x passes against min_pass x (low, clearance) x target (no image, no height, and
// at, one below and one above low - clearance), through cell_out -- pwpp_beams_low and pwpp_beams_occupancy as the kernels call
// them.  Among them a target without a height under a clearance so large that low - INT32_MIN <= clearance: only the clause that
// asks for a height keeps that cell from being called free.  visit(base, raw passes, raw low, has_target, target, min_pass,
// clearance, reported low, byte) sees every row.
template <class Visit>
void byte_matrix(Visit visit) {
    const uint32_t min_pass = 3;
    const int8_t bases[] = {kFree, kOccupied, kUnknown, 42};
    const uint32_t passes[] = {0u, 2u, 3u, 4u, 0xffffffffu};
    const int32_t lows[] = {1200, -(1 << 30) - (1 << 20), (1 << 30) + (1 << 20)};
    const int32_t clearances[] = {0, 300, INT32_MAX};
    for (int8_t base : bases)
        for (uint32_t p : passes)
            for (int32_t low : lows)
                for (int32_t clearance : clearances) {
                    const long long edge = (long long)low - clearance;  // low - target <= clearance  <=>  target >= edge
                    const long long targets[] = {edge - 1, edge, edge + 1};
                    for (int t = -2; t < 3; ++t) {  // -2: no target image; -1: a target without a height
                        const bool has_target = t != -2;
                        const int32_t target = t < 0 ? kNoHeight : (int32_t)std::min<long long>(INT32_MAX, std::max<long long>((long long)INT32_MIN + 1, targets[t]));
                        for (int wrapped = 0; wrapped < (p == 0u ? 2 : 1); ++wrapped) {  // passes 0: nothing passed (low still INT32_MAX), or a sum that wrapped to 0
                            Scene s{1, 1, {0}, {kNoHeight}, {target}, {base}, has_target, true, min_pass, clearance};
                            Result r{std::vector<uint32_t>(1), std::vector<int32_t>(1), std::vector<int8_t>(1)};
                            const int32_t raw = p == 0u && !wrapped ? INT32_MAX : low;
                            cell_out(s, 0, p, raw, r);
                            visit(base, p, raw, has_target, target, min_pass, clearance, r.low[0], r.occupancy[0]);
                        }
                    }
                }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "--bytes") {  // the matrix as text, for tests/test_beams_cpu.py to compare with its restatement
        byte_matrix([](int8_t base, uint32_t p, int32_t raw, bool has_target, int32_t target, uint32_t min_pass, int32_t clearance, int32_t low, int8_t byte) {
            std::printf("%d %u %d %d %d %u %d %d %d\n", (int)base, p, raw, (int)has_target, target, min_pass, clearance, low, (int)byte);
        });
        return 0;
    }
    long long cases = 0, mismatches = 0, theorem_failures = 0, queued = 0;
    // the byte rule against the rule in other words
    byte_matrix([&](int8_t base, uint32_t p, int32_t raw, bool has_target, int32_t target, uint32_t min_pass, int32_t clearance, int32_t low, int8_t byte) {
        const int32_t want_low = p == 0u ? kNoHeight : raw;
        bool free_ = base == kUnknown && p >= min_pass;
        if (free_ && has_target) free_ = target != kNoHeight && (long long)want_low - (long long)target <= (long long)clearance;
        ++cases;
        if (low != want_low || byte != (free_ ? kFree : base)) ++mismatches;
    });
    std::mt19937 rng(20240607u);

    // pwpp_vis_jump against k steps, on every line of a 41 x 37 image from three origins
    for (const auto &o : {std::pair<int, int>{0, 0}, {40, 36}, {17, 20}})
        for (int cy = 0; cy < 37; ++cy)
            for (int cx = 0; cx < 41; ++cx) {
                PwppVisLine S;
                pwpp_vis_line(o.first, o.second, cx, cy, S);
                for (uint32_t k = 1; k <= S.n; ++k) {
                    pwpp_vis_step(S);
                    PwppVisLine J;
                    pwpp_vis_line(o.first, o.second, cx, cy, J);
                    pwpp_vis_jump(J, k);
                    ++cases;
                    if (J.x != S.x || J.y != S.y || J.ex != S.ex || J.ey != S.ey) ++mismatches;
                }
            }

    // the height: against the closed form, and monotone in z
    for (uint32_t n = 2; n <= 40; ++n)
        for (uint32_t k = 1; k < n; ++k) {
            const int32_t eye = 1700;
            int32_t before = INT32_MIN;
            for (long long rise : {-3 * kR, -kR - 1, -kR, -kR + 1, -3000ll, -41ll, -1ll, 0ll, 1ll, 41ll, 3000ll, kR - 1, kR, kR + 1, 3 * kR}) {
                const int32_t z = (int32_t)(eye + rise), got = pwpp_beams_height(eye, z, k, n);
                const long long r = std::min(kR, std::max(-kR, rise));
                ++cases;
                if (got != eye + ceil_div(r * (r < 0 ? 2 * (long long)k - 1 : 2 * (long long)k + 1), 2 * (long long)n)) ++mismatches;
                if (got < before) ++theorem_failures;
                before = got;
            }
        }

    // the worked row of include/pwpp.h
    {
        Scene s{40, 1, std::vector<int32_t>(40, 0), std::vector<int32_t>(40, kNoHeight), {}, {}, false, false, 1u, 0};
        s.hits[34] = 3, s.zmin[34] = 0;
        const Result a = path1(s, 0, 0, 1700, 0);
        ++cases;
        for (int c = 0; c < 40; ++c)
            if (a.passes[c] != (c >= 1 && c <= 33 ? 3u : 0u)) ++mismatches;
        if (a.low[1] != 1675 || a.low[10] != 1225 || a.low[17] != 875 || a.low[33] != 75 || a.low[0] != kNoHeight || a.low[34] != kNoHeight) ++mismatches;
        s.zmin[34] = 2380;
        const Result b = path1(s, 0, 0, 1700, 0);
        if (b.low[1] != 1730 || b.low[17] != 2050 || b.low[33] != 2370) ++mismatches;
    }

    // a sum that wraps: three beams of weight 2^31 - 1 over the same cells
    {
        Scene s{12, 1, std::vector<int32_t>(12, 0), std::vector<int32_t>(12, 100), {}, {}, false, false, 1u, 0};
        s.hits[9] = s.hits[10] = s.hits[11] = INT32_MAX;
        long long q = 0;
        const Result want = brute_force(s, 0, 0, 0, 0);
        ++cases;
        if (want.passes[1] != (uint32_t)(3ull * INT32_MAX) || !(path1(s, 0, 0, 0, 0) == want) || !(path2(s, 0, 0, 0, 0, 4, q) == want)) ++mismatches;
    }

    const int shapes[][2] = {{1, 40}, {40, 1}, {33, 31}, {70, 45}, {17, 66}};
    for (const auto &shape : shapes) {
        const int nx = shape[0], ny = shape[1];
        const int origins[][2] = {{0, 0}, {nx - 1, 0}, {0, ny - 1}, {nx - 1, ny - 1}, {nx / 2, 0}, {0, ny / 2}, {nx / 2, ny / 2}, {nx - 1, ny / 2}, {nx / 2, ny - 1}};
        for (double fill : {0.0, 0.05, 0.3, 1.0})
            for (int variant = 0; variant < 4; ++variant) {
                const int32_t eyes[] = {1700, -350, 1 << 30, -(1 << 30)};
                const int32_t eye = eyes[variant];
                const Scene s = random_scene(nx, ny, fill, eye, variant & 1, variant & 2, rng);
                for (const auto &o : origins) {
                    Result unlimited;
                    for (int max_range : {0, 1, 5, 40}) {
                        const Result want = brute_force(s, o[0], o[1], eye, max_range);
                        cases += 3;
                        if (!(path1(s, o[0], o[1], eye, max_range) == want)) ++mismatches;
                        if (!(path2(s, o[0], o[1], eye, max_range, 16, queued) == want)) ++mismatches;  // (a small tile: several each way on these shapes)
                        if (!(path2(s, o[0], o[1], eye, max_range, PWPP_BEAMS_TILE, queued) == want)) ++mismatches;
                        if (max_range == 0) unlimited = want;
                        for (int y = 0; y < ny; ++y)
                            for (int x = 0; x < nx; ++x) {
                                const size_t c = (size_t)y * nx + x;
                                const int8_t base = s.has_base ? s.base[c] : kUnknown;
                                // max_range: the unlimited values inside, nothing and the base byte outside
                                const bool beyond = max_range > 0 && std::max(std::abs(x - o[0]), std::abs(y - o[1])) > max_range;
                                if (beyond ? (want.passes[c] != 0 || want.low[c] != kNoHeight || want.occupancy[c] != base)
                                           : (want.passes[c] != unlimited.passes[c] || want.low[c] != unlimited.low[c] || want.occupancy[c] != unlimited.occupancy[c]))
                                    ++theorem_failures;
                                // the bytes: free stays free, occupied stays occupied, only unknown may change, and only to free
                                if (want.occupancy[c] != base && !(base == kUnknown && want.occupancy[c] == kFree)) ++theorem_failures;
                            }
                    }
                }
            }
    }
    std::printf("beams_check: %lld cases, %lld mismatches, %lld theorem failures, %lld beams queued by the tiles\n", cases, mismatches, theorem_failures, queued);
    return mismatches == 0 && theorem_failures == 0 ? 0 : 1;
}
