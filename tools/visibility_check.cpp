// visibility_check.cpp -- the line-of-sight kernels' pack and walk on the host, against a brute force.
//
// The kernels of patchwork-plusplus_amd/csrc/pwpp_visibility.hip are built from the functions of pwpp_visibility.h (the words of a
// 64-cell ballot, the bit image's addressing, the error-accumulator step, the walk with its rules (a) and (b), the occupancy
// byte).  This program runs the same sequence with the same functions over plain memory -- the pack chunk by chunk as k_vis_pack
// does it, the walk over the whole bit image, over the rows between the origin and a run of 256 cells copied into a buffer of
// EXACTLY that size (what k_vis_walk keeps in LDS: a word outside it is a sanitizer error), and over the count image (the
// yardstick) -- on many small images with origins in the corners, on the edges, inside, and on occupied cells, and compares first
// and occupancy with a brute force written from the closed form of the line, with its own divisions.  Exit status 0: all equal.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I patchwork-plusplus_amd/csrc tools/visibility_check.cpp -o visibility_check
// (tests/test_obstacle_visibility_cpu.py builds and runs it; it needs no GPU and no HIP.)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "pwpp_visibility.h"

namespace {

struct Image {
    int nx, ny;
    std::vector<int32_t> count;
};

struct Result {
    std::vector<int32_t> first;
    std::vector<int8_t> occupancy;
    bool operator==(const Result &o) const { return first == o.first && occupancy == o.occupancy; }
};

// the definition: the closed form of every point, in 64-bit arithmetic
Result brute_force(const Image &im, int min_count, int ox, int oy, int max_range) {
    const int nx = im.nx, ny = im.ny;
    const auto occ = [&](long long x, long long y) {
        if (x < 0 || y < 0 || x >= nx || y >= ny) std::abort();  // (the line never leaves the image)
        return im.count[(size_t)(y * nx + x)] >= min_count;
    };
    Result r{std::vector<int32_t>((size_t)nx * ny), std::vector<int8_t>((size_t)nx * ny)};
    for (int cy = 0; cy < ny; ++cy)
        for (int cx = 0; cx < nx; ++cx) {
            const long long dx = cx - ox, dy = cy - oy, ax = std::llabs(dx), ay = std::llabs(dy), n = std::max(ax, ay);
            const long long sx = dx > 0 ? 1 : (dx < 0 ? -1 : 0), sy = dy > 0 ? 1 : (dy < 0 ? -1 : 0);
            long long first = -1;
            if (max_range > 0 && n > max_range) {
                first = -2;
            } else if (n == 0) {
                first = occ(cx, cy) ? (long long)cy * nx + cx : -1;
            } else {
                long long px = ox, py = oy;
                for (long long k = 1; k <= n && first == -1; ++k) {
                    const long long x = ox + sx * ((2 * k * ax + n) / (2 * n)), y = oy + sy * ((2 * k * ay + n) / (2 * n));
                    if (std::llabs(x - px) > 1 || std::llabs(y - py) > 1) std::abort();
                    if (x != px && y != py && occ(px, y) && occ(x, py)) first = std::min(y * nx + px, py * nx + x);
                    else if (occ(x, y)) first = y * nx + x;
                    px = x, py = y;
                }
                if (first == -1 && (px != cx || py != cy)) std::abort();  // P_n = c
            }
            const size_t c = (size_t)cy * nx + cx;
            r.first[c] = (int32_t)first;
            r.occupancy[c] = occ(cx, cy) ? 100 : (first == -1 ? 0 : -1);
        }
    return r;
}

// pass 1 as k_vis_pack runs it: a chunk of 64 cells of a row -> one mask -> two words; a buffer of exactly ny * row_words words
std::vector<uint32_t> pack(const Image &im, int min_count) {
    const int nx = im.nx, rw = pwpp_vis_row_words(nx), chunks = (nx + 63) / 64;
    std::vector<uint32_t> bits((size_t)rw * im.ny, 0xdeadbeefu);  // (every word must be written)
    for (int y = 0; y < im.ny; ++y)
        for (int k = 0; k < chunks; ++k) {
            unsigned long long mask = 0;
            for (int l = 0; l < 64; ++l)
                if (k * 64 + l < nx && im.count[(size_t)y * nx + k * 64 + l] >= min_count) mask |= 1ull << l;
            bits[(size_t)y * rw + 2 * k] = pwpp_vis_ballot_word(mask, 0);
            if (2 * k + 1 < rw) bits[(size_t)y * rw + 2 * k + 1] = pwpp_vis_ballot_word(mask, 1);
        }
    return bits;
}

// pass 2.  how 0: the whole bit image; 1: per run of 256 cells the rows from the origin's to the run's, copied; 2: the count image
Result walk(const Image &im, const std::vector<uint32_t> &bits, int min_count, int ox, int oy, int max_range, int how) {
    const int nx = im.nx, ny = im.ny, rw = pwpp_vis_row_words(nx);
    Result r{std::vector<int32_t>((size_t)nx * ny), std::vector<int8_t>((size_t)nx * ny)};
    for (int c0 = 0; c0 < nx * ny; c0 += 256) {
        const int c1 = std::min(nx * ny, c0 + 256) - 1, t0 = c0 / nx, t1 = c1 / nx, r0 = std::min(oy, t0), r1 = std::max(oy, t1);
        std::vector<uint32_t> window;
        PwppVisBits occ{bits.data(), rw, 0, ny, nx};
        if (how == 1) {
            window.assign(bits.begin() + (size_t)r0 * rw, bits.begin() + (size_t)(r1 + 1) * rw);
            occ = PwppVisBits{window.data(), rw, r0, r1 - r0 + 1, nx};
        }
        const PwppVisCounts cnt{im.count.data(), nx, ny, min_count};
        for (int i = c0; i <= c1; ++i) {
            const int cy = i / nx, cx = i - cy * nx;
            const size_t c = (size_t)i;
            if (how == 2) {
                r.first[c] = pwpp_vis_walk(cnt, ox, oy, cx, cy, nx, max_range);
                r.occupancy[c] = pwpp_vis_occupancy(cnt.at(cx, cy), r.first[c]);
            } else {
                r.first[c] = pwpp_vis_walk(occ, ox, oy, cx, cy, nx, max_range);
                r.occupancy[c] = pwpp_vis_occupancy(occ.at(cx, cy), r.first[c]);
            }
        }
    }
    return r;
}

}  // namespace

int main() {
    const int shapes[][2] = {{1, 1}, {1, 70}, {70, 1}, {5, 7}, {33, 31}, {64, 16}, {65, 17}, {31, 33}, {96, 9}, {130, 3}};
    const double fills[] = {0.0, 0.05, 0.4, 1.0};
    const int ranges[] = {0, 1, 7, 200};
    std::mt19937 rng(20240917u);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    int cases = 0, bad = 0;
    long blocked_a = 0;
    for (const auto &sh : shapes)
        for (double fill : fills)
            for (int min_count = 1; min_count <= 3; min_count += 2) {
                const int nx = sh[0], ny = sh[1];
                Image im{nx, ny, std::vector<int32_t>((size_t)nx * ny)};
                for (auto &c : im.count) c = uni(rng) < fill ? min_count + (int)(rng() % 3u) : (int)(rng() % (unsigned)min_count);
                const std::vector<uint32_t> bits = pack(im, min_count);
                // the pack against the count image, bit by bit, the pad bits zero
                for (int y = 0; y < ny; ++y)
                    for (int x = 0; x < 32 * pwpp_vis_row_words(nx); ++x) {
                        const bool bit = (bits[(size_t)y * pwpp_vis_row_words(nx) + (x >> 5)] >> (x & 31)) & 1u;
                        if (bit != (x < nx && im.count[(size_t)y * nx + x] >= min_count)) ++bad, std::fprintf(stderr, "MISMATCH pack %dx%d (%d, %d)\n", nx, ny, x, y);
                    }
                // the four corners, the middles of the four edges, the middle, two random cells, one occupied cell where there is one
                std::vector<std::pair<int, int>> origins = {{0, 0}, {nx - 1, 0}, {0, ny - 1}, {nx - 1, ny - 1}, {nx / 2, 0}, {nx / 2, ny - 1},
                                                            {0, ny / 2}, {nx - 1, ny / 2}, {nx / 2, ny / 2}};
                for (int j = 0; j < 2; ++j) origins.push_back({(int)(rng() % (unsigned)nx), (int)(rng() % (unsigned)ny)});
                for (size_t c = 0; c < im.count.size(); ++c)
                    if (im.count[c] >= min_count) {
                        origins.push_back({(int)(c % (size_t)nx), (int)(c / (size_t)nx)});
                        break;
                    }
                for (const auto &o : origins)
                    for (int range : ranges) {
                        const Result want = brute_force(im, min_count, o.first, o.second, range);
                        for (size_t c = 0; c < want.first.size(); ++c)  // (hidden behind a squeeze or a cell: for the statistics line)
                            blocked_a += want.first[c] >= 0 && want.first[c] != (int32_t)c;
                        for (int how = 0; how < 3; ++how) {
                            ++cases;
                            if (!(walk(im, bits, min_count, o.first, o.second, range, how) == want)) {
                                ++bad;
                                std::fprintf(stderr, "MISMATCH %dx%d fill %g min_count %d origin (%d, %d) max_range %d how %d\n", nx, ny, fill, min_count,
                                             o.first, o.second, range, how);
                            }
                        }
                    }
            }
    // the step against the closed form at the largest sides: 2k|d| + n needs more than 31 bits there
    {
        const int ends[][2] = {{32767, 32767}, {32767, 1}, {32767, 16384}, {32767, 32766}, {1, 32767}, {12345, 32767}};
        for (const auto &e : ends) {
            PwppVisLine L;
            pwpp_vis_line(0, 0, e[0], e[1], L);
            const unsigned long long n = L.n;
            for (unsigned long long k = 1; k <= n; ++k) {
                pwpp_vis_step(L);
                const long long x = (long long)((2 * k * (unsigned long long)e[0] + n) / (2 * n)), y = (long long)((2 * k * (unsigned long long)e[1] + n) / (2 * n));
                if (L.x != x || L.y != y) {
                    ++bad;
                    std::fprintf(stderr, "MISMATCH step (%d, %d) k %llu\n", e[0], e[1], k);
                    break;
                }
            }
            ++cases;
        }
    }
    // the origin's cell by the raster's rule
    {
        int i = -1;
        if (!pwpp_vis_cell_of(0.0, -64.0, 0.5, 256, i) || i != 128 || pwpp_vis_cell_of(64.0, -64.0, 0.5, 256, i) || pwpp_vis_cell_of(-64.1, -64.0, 0.5, 256, i) ||
            !pwpp_vis_cell_of(63.99, -64.0, 0.5, 256, i) || i != 255 || pwpp_vis_cell_of(NAN, 0.0, 1.0, 4, i))
            ++bad, std::fprintf(stderr, "MISMATCH cell_of\n");
    }
    std::printf("visibility_check: %d cases, %ld hidden cells, %d mismatches\n", cases, blocked_a, bad);
    return bad ? 1 : 0;
}
