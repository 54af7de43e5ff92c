// viewshed_check.cpp -- the viewshed kernels' pack and walk on the host, against a brute force.
//
// The kernels of patchwork-plusplus_amd/csrc/pwpp_viewshed.hip are built from the functions of pwpp_viewshed.h and, for the line and
// the bit image, of pwpp_visibility.h.  This program runs the same sequence with the same functions over plain memory -- the pack
// chunk by chunk as k_view_pack does it, then the walk in runs of 256 cells on both paths: over the count image (path 1) and over the
// rows between the origin and the run copied into a buffer of EXACTLY that size (what path 2 keeps in LDS: a word outside it is a
// sanitizer error), and over the whole bit image (path 2 beyond the LDS limit) -- with and without a shadow image, with and without
// each of block, target and seen, and compares first, shadow and occupancy with a brute force of its own: the closed form of every
// point with its own divisions, every blocker of the line met, nothing stopped early.  It also checks the degenerate case against
// pwpp_vis_walk itself, the hidden-iff-below-shadow theorem on every cell, the kerb and the quantiser.  Exit status 0: all equal.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I patchwork-plusplus_amd/csrc tools/viewshed_check.cpp -o viewshed_check
// (tests/test_viewshed_cpu.py builds and runs it; it needs no GPU and no HIP.)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "pwpp_viewshed.h"

namespace {

constexpr long long kR = 1 << 20, kOpaque = 1ll << 40, kBelow = -(1ll << 40);
constexpr int32_t kNoHeight = INT32_MIN;

struct Scene {
    int nx, ny, min_count, min_seen;
    std::vector<int32_t> count, block, target, seen;
    bool has_block, has_target, has_seen;
};

struct Result {
    std::vector<int32_t> first, shadow;
    std::vector<int8_t> occupancy;
    bool operator==(const Result &o) const { return first == o.first && shadow == o.shadow && occupancy == o.occupancy; }
};

long long clamp_rise(long long d) { return std::min(kR, std::max(-kR, d)); }
long long ceil_div(long long num, long long d) { return num >= 0 ? (num + d - 1) / d : -((-num) / d); }

// the definition.  `theorem_bad` counts cells where "hidden iff target rise < shadow rise" fails.
Result brute_force(const Scene &s, int ox, int oy, int32_t eye, int max_range, int &theorem_bad) {
    const int nx = s.nx, ny = s.ny;
    const auto at = [&](long long x, long long y) {
        if (x < 0 || y < 0 || x >= nx || y >= ny) std::abort();  // (the line never leaves the image)
        return (size_t)(y * nx + x);
    };
    const auto occ = [&](long long x, long long y) { return s.count[at(x, y)] >= s.min_count; };
    const auto blocker = [&](long long x, long long y) {
        return !s.has_block || s.block[at(x, y)] == kNoHeight ? kOpaque : clamp_rise((long long)s.block[at(x, y)] - eye);
    };
    Result r{std::vector<int32_t>((size_t)nx * ny), std::vector<int32_t>((size_t)nx * ny), std::vector<int8_t>((size_t)nx * ny)};
    for (int cy = 0; cy < ny; ++cy)
        for (int cx = 0; cx < nx; ++cx) {
            const size_t c = (size_t)cy * nx + cx;
            const long long dx = cx - ox, dy = cy - oy, ax = std::llabs(dx), ay = std::llabs(dy), n = std::max(ax, ay);
            const long long sx = dx > 0 ? 1 : (dx < 0 ? -1 : 0), sy = dy > 0 ? 1 : (dy < 0 ? -1 : 0);
            const bool own = occ(cx, cy);
            long long t = kBelow;
            if (own) {
                const long long b = blocker(cx, cy);
                t = b == kOpaque ? kBelow : b;
            } else if (s.has_target && s.target[c] != kNoHeight) {
                t = clamp_rise((long long)s.target[c] - eye);
            }
            long long first = own ? (long long)c : -1, shadow = kNoHeight;
            if (max_range > 0 && n > max_range) {
                first = -2;
            } else {
                long long px = ox, py = oy, hider = -1, cast = -(1ll << 62);
                bool any = false, dark = false;
                const auto meet = [&](long long rr, long long D, long long cell) {
                    any = true;
                    const bool hides = rr == kOpaque || t == kBelow || rr * 2 * n > t * D;
                    if (hides && hider < 0) hider = cell;
                    if (rr == kOpaque) dark = true;
                    else cast = std::max(cast, ceil_div(rr * 2 * n, D));
                };
                for (long long k = 1; k <= n; ++k) {
                    const long long x = ox + sx * ((2 * k * ax + n) / (2 * n)), y = oy + sy * ((2 * k * ay + n) / (2 * n));
                    if (std::llabs(x - px) > 1 || std::llabs(y - py) > 1) std::abort();
                    if (x != px && y != py && occ(px, y) && occ(x, py)) {
                        const long long ra = blocker(px, y), rb = blocker(x, py), ia = y * nx + px, ib = py * nx + x;
                        meet(std::min(ra, rb), 2 * k - 1, ra < rb ? ia : (rb < ra ? ib : std::min(ia, ib)));
                    }
                    if (k < n && occ(x, y)) meet(blocker(x, y), 2 * k, y * nx + x);
                    px = x, py = y;
                }
                if (px != cx || py != cy) std::abort();  // P_n = c
                if (hider >= 0) first = hider;
                if (any) shadow = dark ? (long long)INT32_MAX : std::min((long long)INT32_MAX - 1, std::max((long long)INT32_MIN + 1, eye + std::min(kR + 1, std::max(-kR, cast))));
                // the theorem, in rises: hidden iff t < shadow rise (opaque: +infinity; no blocker: nothing hides)
                const bool hidden = hider >= 0;
                const bool below = any && (dark || t == kBelow || t < std::min(kR + 1, std::max(-kR, cast)));
                if (hidden != below) ++theorem_bad;
            }
            r.first[c] = (int32_t)first;
            r.shadow[c] = (int32_t)shadow;
            const bool witnessed = s.has_seen && s.seen[c] >= s.min_seen;
            r.occupancy[c] = own ? 100 : (witnessed || first == -1 ? 0 : -1);
        }
    return r;
}

// pass 1 as k_view_pack runs it: a chunk of 64 cells of a row -> one mask -> two words; a buffer of exactly ny * row_words words
std::vector<uint32_t> pack(const Scene &s) {
    const int nx = s.nx, rw = pwpp_vis_row_words(nx), chunks = (nx + 63) / 64;
    std::vector<uint32_t> bits((size_t)rw * s.ny, 0xdeadbeefu);  // (every word must be written)
    for (int y = 0; y < s.ny; ++y)
        for (int k = 0; k < chunks; ++k) {
            unsigned long long mask = 0;
            for (int l = 0; l < 64; ++l)
                if (k * 64 + l < nx && s.count[(size_t)y * nx + k * 64 + l] >= s.min_count) mask |= 1ull << l;
            bits[(size_t)y * rw + 2 * k] = pwpp_vis_ballot_word(mask, 0);
            if (2 * k + 1 < rw) bits[(size_t)y * rw + 2 * k + 1] = pwpp_vis_ballot_word(mask, 1);
        }
    return bits;
}

// pass 2 in runs of 256 cells.  how 0: path 2 on the whole bit image; 1: path 2, per run the rows from the origin's to the run's,
// copied; 2: path 1, the count image.  with_shadow false: the walk stops at the first blocker that hides; shadow is left 0.
Result walk(const Scene &s, const std::vector<uint32_t> &bits, int ox, int oy, int32_t eye, int max_range, int how, bool with_shadow) {
    const int nx = s.nx, ny = s.ny, rw = pwpp_vis_row_words(nx);
    Result r{std::vector<int32_t>((size_t)nx * ny), std::vector<int32_t>((size_t)nx * ny), std::vector<int8_t>((size_t)nx * ny)};
    const PwppViewHeights H{s.has_block ? s.block.data() : nullptr, s.has_target ? s.target.data() : nullptr, nx, ny, eye};
    for (int c0 = 0; c0 < nx * ny; c0 += 256) {
        const int c1 = std::min(nx * ny, c0 + 256) - 1, t0 = c0 / nx, t1 = c1 / nx, r0 = std::min(oy, t0), r1 = std::max(oy, t1);
        std::vector<uint32_t> window;
        PwppVisBits occ{bits.data(), rw, 0, ny, nx};
        if (how == 1) {
            window.assign(bits.begin() + (size_t)r0 * rw, bits.begin() + (size_t)(r1 + 1) * rw);
            occ = PwppVisBits{window.data(), rw, r0, r1 - r0 + 1, nx};
        }
        const PwppVisCounts cnt{s.count.data(), nx, ny, s.min_count};
        for (int i = c0; i <= c1; ++i) {
            const int cy = i / nx, cx = i - cy * nx;
            const size_t c = (size_t)i;
            const PwppViewResult res = how == 2 ? pwpp_view_walk(cnt, H, ox, oy, cx, cy, nx, max_range, with_shadow)
                                                : pwpp_view_walk(occ, H, ox, oy, cx, cy, nx, max_range, with_shadow);
            r.first[c] = res.first;
            r.shadow[c] = with_shadow ? res.shadow : 0;
            r.occupancy[c] = pwpp_view_occupancy(how == 2 ? cnt.at(cx, cy) : occ.at(cx, cy), s.has_seen && s.seen[c] >= s.min_seen, r.first[c]);
        }
    }
    return r;
}

}  // namespace

int main() {
    const int shapes[][2] = {{1, 1}, {1, 70}, {70, 1}, {5, 7}, {33, 31}, {64, 16}, {65, 17}, {31, 33}, {96, 9}, {130, 3}};
    const double fills[] = {0.0, 0.05, 0.4, 1.0};
    const int ranges[] = {0, 7};
    std::mt19937 rng(20261021u);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    int cases = 0, bad = 0, theorem_bad = 0;
    long hidden = 0, overseen = 0;
    for (const auto &sh : shapes)
        for (double fill : fills)
            for (int variant = 0; variant < 4; ++variant) {  // 0: all three images; 1: none (the 2-D case); 2: block alone; 3: target and seen alone
                const int nx = sh[0], ny = sh[1], min_count = 1 + 2 * (variant & 1);
                const int32_t eye = (int32_t)(rng() % 4001u) - 2000;
                Scene s{nx, ny, min_count, 2, {}, {}, {}, {}, variant == 0 || variant == 2, variant == 0 || variant == 3, variant == 0 || variant == 3};
                const size_t cells = (size_t)nx * ny;
                s.count.resize(cells), s.block.resize(cells), s.target.resize(cells), s.seen.resize(cells);
                const auto height = [&]() -> int32_t {
                    if (uni(rng) < 0.1) return kNoHeight;
                    switch (rng() % 4u) {
                        case 0: return eye + (int32_t)(rng() % 81u) - 40;
                        case 1: return eye + (int32_t)(rng() % 6001u) - 3000;
                        case 2: return eye + (int32_t)(rng() % (2u * (unsigned)kR + 11u)) - (int32_t)kR - 5;
                        default: return eye + (int32_t)((rng() & 1u) ? 3 * kR : -3 * kR) + (int32_t)(rng() % 3u) - 1;
                    }
                };
                for (size_t c = 0; c < cells; ++c) {
                    s.count[c] = uni(rng) < fill ? min_count + (int)(rng() % 3u) : (int)(rng() % (unsigned)min_count);
                    s.block[c] = height(), s.target[c] = height(), s.seen[c] = (int32_t)(rng() % 4u);
                }
                const std::vector<uint32_t> bits = pack(s);
                for (int y = 0; y < ny; ++y)  // the pack against the count image, bit by bit, the pad bits zero
                    for (int x = 0; x < 32 * pwpp_vis_row_words(nx); ++x) {
                        const bool bit = (bits[(size_t)y * pwpp_vis_row_words(nx) + (x >> 5)] >> (x & 31)) & 1u;
                        if (bit != (x < nx && s.count[(size_t)y * nx + x] >= min_count)) ++bad, std::fprintf(stderr, "MISMATCH pack %dx%d (%d, %d)\n", nx, ny, x, y);
                    }
                // the four corners, the middle of an edge, the middle, one random cell, one occupied cell where there is one
                std::vector<std::pair<int, int>> origins = {{0, 0}, {nx - 1, 0}, {0, ny - 1}, {nx - 1, ny - 1}, {nx / 2, 0}, {nx / 2, ny / 2}};
                origins.push_back({(int)(rng() % (unsigned)nx), (int)(rng() % (unsigned)ny)});
                for (size_t c = 0; c < cells; ++c)
                    if (s.count[c] >= min_count) {
                        origins.push_back({(int)(c % (size_t)nx), (int)(c / (size_t)nx)});
                        break;
                    }
                for (const auto &o : origins)
                    for (int range : ranges) {
                        const Result want = brute_force(s, o.first, o.second, eye, range, theorem_bad);
                        Result blind = want;  // what a call without a shadow image computes
                        std::fill(blind.shadow.begin(), blind.shadow.end(), 0);
                        for (size_t c = 0; c < cells; ++c) hidden += want.first[c] >= 0 && want.first[c] != (int32_t)c;
                        for (int how = 0; how < 3; ++how)
                            for (int with_shadow = 0; with_shadow < 2; ++with_shadow) {
                                ++cases;
                                if (!(walk(s, bits, o.first, o.second, eye, range, how, with_shadow != 0) == (with_shadow ? want : blind))) {
                                    ++bad;
                                    std::fprintf(stderr, "MISMATCH %dx%d fill %g variant %d origin (%d, %d) max_range %d how %d shadow %d\n", nx, ny, fill, variant,
                                                 o.first, o.second, range, how, with_shadow);
                                }
                            }
                        // theorem 1: without images, first and occupancy are the visibility's; theorem 2: its free cells stay free
                        const PwppVisCounts cnt{s.count.data(), nx, ny, min_count};
                        for (int cy = 0; cy < ny; ++cy)
                            for (int cx = 0; cx < nx; ++cx) {
                                const size_t c = (size_t)cy * nx + cx;
                                const int32_t f2 = pwpp_vis_walk(cnt, o.first, o.second, cx, cy, nx, range);
                                const int8_t o2 = pwpp_vis_occupancy(cnt.at(cx, cy), f2);
                                if (variant == 1 && (f2 != want.first[c] || o2 != want.occupancy[c])) ++bad, std::fprintf(stderr, "MISMATCH 2-D (%d, %d)\n", cx, cy);
                                if (o2 == 0 && want.occupancy[c] != 0) ++bad, std::fprintf(stderr, "MISMATCH subset (%d, %d)\n", cx, cy);
                                overseen += o2 != 0 && want.occupancy[c] == 0;
                            }
                        ++cases;
                    }
            }
    // theorem 4: the kerb
    {
        Scene s{40, 1, 1, 1, std::vector<int32_t>(40, 0), std::vector<int32_t>(40, kNoHeight), std::vector<int32_t>(40, 0), {}, true, true, false};
        s.count[4] = 1, s.block[4] = 1500;
        const std::vector<uint32_t> bits = pack(s);
        for (int how = 0; how < 3; ++how) {
            const Result r = walk(s, bits, 0, 0, 1700, 0, how, true);
            for (int c = 0; c < 40; ++c) {
                const int32_t f = c == 4 || (c >= 5 && c <= 33) ? 4 : -1, sh = c <= 4 ? kNoHeight : (int32_t)(1700 + ceil_div(-200ll * 2 * c, 8));
                if (r.first[(size_t)c] != f || r.shadow[(size_t)c] != sh) ++bad, std::fprintf(stderr, "MISMATCH kerb cell %d how %d\n", c, how);
            }
            if (r.shadow[10] != 1200 || r.shadow[34] != 0) ++bad, std::fprintf(stderr, "MISMATCH kerb shadow\n");
            ++cases;
        }
    }
    // the quantiser
    {
        const double v[] = {0.0, 1.0, -1.0, 0.00048828125, -0.00048828125, 0.000488, 1.7, 1e9, -1e9, 1048576.0, INFINITY, -INFINITY};
        const int32_t q[] = {0, 1024, -1024, 1, 0, 0, 1741, 1 << 30, -(1 << 30), 1 << 30, 1 << 30, -(1 << 30)};
        for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i)
            if (pwpp_view_units(v[i]) != q[i]) ++bad, std::fprintf(stderr, "MISMATCH units %g: %d\n", v[i], pwpp_view_units(v[i]));
        if (pwpp_view_units(NAN) != kNoHeight) ++bad, std::fprintf(stderr, "MISMATCH units NaN\n");
        ++cases;
    }
    bad += theorem_bad;
    std::printf("viewshed_check: %d cases, %ld hidden cells, %ld cells the 2-D walk leaves unknown seen free, %d theorem failures, %d mismatches\n", cases,
                hidden, overseen, theorem_bad, bad);
    return bad ? 1 : 0;
}
