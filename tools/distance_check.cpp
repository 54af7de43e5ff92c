// distance_check.cpp -- the obstacle distances' sequence of passes on the host, against a brute force.
//
// The kernels of patchwork-plusplus_amd/csrc/pwpp_distance.hip are built from the functions of pwpp_distance.h (the neighbours
// inside a 64-column chunk from its occupancy mask, the left / right pick, the 64-bit key, the outward scan with its early exit,
// the scan over every row, the cap).  This program runs the same sequence with the same functions over plain memory -- the row
// pass chunk by chunk with the carries of the kernel, the column pass from the whole column, from the rows of a tile with a halo
// of max_dist rows copied into a buffer of exactly that size (what the kernel keeps in LDS: a row outside it is a sanitizer
// error), and over every row -- on random and patterned images, ties included, and compares dist2 and nearest with the minimum
// of (distance, index) over all occupied cells, capped by the definition.  Wherever the launcher (pwpp_dist_plan) would keep
// tiles with a halo in LDS, the window is also run with the launcher's own tile and halo.  Exit status 0: all equal.
//   distance_check          the small shapes
//   distance_check --tall   tall images of several strips: every tiling of the column pass, scans that reach the halo
//   distance_check --plans  pwpp_dist_plan as a table: ny max_dist path lds tile_rows halo row_tiles
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I patchwork-plusplus_amd/csrc tools/distance_check.cpp -o distance_check
// (tests/test_obstacle_distance_cpu.py builds and runs it; it needs no GPU and no HIP.)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "pwpp_distance.h"

namespace {

struct Image {
    int nx, ny;
    std::vector<int32_t> count;
};

struct Result {
    std::vector<int32_t> dist2, nearest;
    bool operator==(const Result &o) const { return dist2 == o.dist2 && nearest == o.nearest; }
};

// the definition: the minimum over all occupied cells of (dist2, index)
Result brute_force(const Image &im, int min_count, long &ties) {
    const int N = im.nx * im.ny;
    std::vector<int> occ, ox, oy;
    for (int c = 0; c < N; ++c)
        if (im.count[c] >= min_count) occ.push_back(c), ox.push_back(c % im.nx), oy.push_back(c / im.nx);
    Result r{std::vector<int32_t>((size_t)N, (int32_t)PWPP_DIST_NONE), std::vector<int32_t>((size_t)N, -1)};
    for (int c = 0; c < N; ++c) {
        const int x = c % im.nx, y = c / im.nx;
        long long best = -1;
        int at = -1, same = 0;
        for (size_t k = 0; k < occ.size(); ++k) {  // (ascending index: the first of several at the same distance stays)
            const long long dx = ox[k] - x, dy = oy[k] - y, d = dx * dx + dy * dy;
            if (best < 0 || d < best) best = d, at = occ[k], same = 1;
            else if (d == best) ++same;
        }
        if (same > 1) ++ties;
        if (at >= 0) r.dist2[c] = (int32_t)best, r.nearest[c] = at;
    }
    return r;
}

// ... and the cap: a cell whose true dist2 exceeds max_dist^2 reports beyond, every other what the unlimited result has
Result capped(Result r, int max_dist) {
    for (size_t c = 0; c < r.dist2.size() && max_dist > 0; ++c)
        if ((long long)r.dist2[c] > (long long)max_dist * max_dist) r.dist2[c] = (int32_t)PWPP_DIST_NONE, r.nearest[c] = -1;
    return r;
}

// pass 1 as k_dist_rows runs it: right to left, then left to right, a chunk of 64 columns at a time
void row_pass(const Image &im, int min_count, std::vector<int32_t> &gx) {
    const int nx = im.nx, chunks = (nx + 63) / 64;
    gx.assign(im.count.size(), -2);
    for (int y = 0; y < im.ny; ++y) {
        const int32_t *c = im.count.data() + (size_t)y * nx;
        int32_t *g = gx.data() + (size_t)y * nx;
        const auto mask_of = [&](int k) {
            unsigned long long m = 0;
            for (int l = 0; l < 64; ++l)
                if (k * 64 + l < nx && c[k * 64 + l] >= min_count) m |= 1ull << l;
            return m;
        };
        int32_t next = -1, last = -1;
        for (int k = chunks - 1; k >= 0; --k) {
            const unsigned long long mask = mask_of(k);
            for (int l = 0; l < 64 && k * 64 + l < nx; ++l) {
                const int in = pwpp_dist_right_in_chunk(mask, l);
                g[k * 64 + l] = in >= 0 ? k * 64 + in : next;
            }
            if (mask) next = k * 64 + __builtin_ctzll(mask);
        }
        for (int k = 0; k < chunks; ++k) {
            const unsigned long long mask = mask_of(k);
            for (int l = 0; l < 64 && k * 64 + l < nx; ++l) {
                const int in = pwpp_dist_left_in_chunk(mask, l), x = k * 64 + l;
                g[x] = pwpp_dist_row_pick(in >= 0 ? k * 64 + in : last, g[x], x);
            }
            if (mask) last = k * 64 + 63 - __builtin_clzll(mask);
        }
    }
}

struct WholeColumn {  // gx of the image + ix
    const int32_t *g;
    int nx;
    int32_t gx(int jy) const { return g[(size_t)jy * nx]; }
};
struct WindowColumn {  // the rows [row0, row1) of one column, copied: the kernel's LDS window
    std::unique_ptr<int32_t[]> rows;  // an allocation of exactly row1 - row0 words: a row outside it is a sanitizer error
    int row0;
    int32_t gx(int jy) const { return rows[(ptrdiff_t)jy - row0]; }
};

// pass 2.  how 0: outward, the whole column; 1: outward from a window of tile_rows rows and `halo` more on either side
// (k_dist_cols' row0 and row1; max_dist > 0); 2: every row
Result column_pass(const Image &im, const std::vector<int32_t> &gx, int max_dist, int how, int tile_rows, int halo) {
    const int nx = im.nx, ny = im.ny;
    const uint32_t cap2 = pwpp_dist_cap2(max_dist);
    Result r{std::vector<int32_t>(gx.size()), std::vector<int32_t>(gx.size())};
    for (int x = 0; x < nx; ++x) {
        WholeColumn whole{gx.data() + x, nx};
        for (int t0 = 0; t0 < ny; t0 += tile_rows) {
            const int t1 = std::min(ny, t0 + tile_rows), row0 = std::max(0, t0 - halo), row1 = std::min(ny, t1 + halo);
            WindowColumn win{nullptr, row0};
            if (how == 1) {
                win.rows.reset(new int32_t[(size_t)(row1 - row0)]);
                for (int jy = row0; jy < row1; ++jy) win.rows[jy - row0] = whole.gx(jy);
            }
            for (int y = t0; y < t1; ++y) {
                const unsigned long long key = how == 0   ? pwpp_dist_scan_outward(whole, x, y, nx, ny, cap2)
                                               : how == 1 ? pwpp_dist_scan_outward(win, x, y, nx, ny, cap2)
                                                          : pwpp_dist_scan_all(whole, x, y, nx, ny);
                pwpp_dist_of_key(key, cap2, r.dist2[(size_t)y * nx + x], r.nearest[(size_t)y * nx + x]);
            }
        }
    }
    return r;
}

Image pattern(const std::string &name, int nx, int ny, int min_count, std::mt19937 &rng) {
    Image im{nx, ny, std::vector<int32_t>((size_t)nx * ny, 0)};
    std::vector<char> occ((size_t)nx * ny, 0);
    auto at = [&](int x, int y) -> char & { return occ[(size_t)y * nx + x]; };
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    if (name == "full") {
        std::fill(occ.begin(), occ.end(), 1);
    } else if (name == "checker") {  // every free cell has two to four nearest cells
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) at(x, y) = (x + y) % 2 == 0;
    } else if (name == "corners") {  // the four corners: the middle lines are all ties
        at(0, 0) = at(nx - 1, 0) = at(0, ny - 1) = at(nx - 1, ny - 1) = 1;
    } else if (name == "single") {
        at((int)(rng() % (unsigned)nx), (int)(rng() % (unsigned)ny)) = 1;
    } else if (name == "last_row") {
        for (int x = 0; x < nx; ++x) at(x, ny - 1) = 1;
    } else if (name == "columns") {  // every 64th column and the last: left / right ties at the chunk edges
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) at(x, y) = x % 64 == 0 || x == nx - 1;
    } else if (name.rfind("random", 0) == 0) {
        const float p = std::stof(name.substr(6));
        for (auto &o : occ) o = uni(rng) < p;
    }  // "empty": nothing
    for (size_t i = 0; i < occ.size(); ++i)
        im.count[i] = occ[i] ? min_count + (int)(rng() % (unsigned)(4 - min_count)) : (int)(rng() % (unsigned)min_count);
    return im;
}

// the tall patterns of tests/obstacle_distance_ref.py (TALL_PATTERNS): all sparse; counts 1 and 2, so that min_count 2 keeps a part
Image tall_pattern(const std::string &name, int nx, int ny, const int *caps, int ncaps) {
    Image im{nx, ny, std::vector<int32_t>((size_t)nx * ny, 0)};
    std::vector<char> occ((size_t)nx * ny, 0);
    auto at = [&](int x, int y) -> char & { return occ[(size_t)y * nx + x]; };
    auto row = [&](int y) {
        for (int x = 0; x < nx; ++x) at(x, y) = 1;
    };
    if (name == "row_top") {
        row(0);
    } else if (name == "row_bottom") {
        row(ny - 1);
    } else if (name == "row_mid") {
        row(ny / 2);
    } else if (name == "two_rows") {  // (their midpoint 192 is a border of the 64-row tiling)
        row(92), row(292);
    } else if (name == "lattice") {
        at(nx / 2, ny / 2) = 1;
    } else if (name == "columns") {
        for (int y = 0; y < ny; ++y) at(0, y) = at(nx - 1, y) = 1;
    } else if (name == "corners") {
        at(0, 0) = at(nx - 1, 0) = at(0, ny - 1) = at(nx - 1, ny - 1) = 1;
    } else if (name == "sparse") {
        std::mt19937 rng(577u);
        std::uniform_real_distribution<float> uni(0.0f, 1.0f);
        for (auto &o : occ) o = uni(rng) < 0.003f;
    } else if (name == "borders") {  // a cell either side of every tile border of every plan, columns of its own for every cap
        for (int k = 0; k < ncaps; ++k) {
            const PwppDistPlan p = pwpp_dist_plan(ny, caps[k], 0);
            for (int t = 1; t < p.row_tiles; ++t) at(3 + 7 * k, t * p.tile_rows - 1) = at(nx - 4 - 7 * k, t * p.tile_rows) = 1;
        }
    }
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x)
            if (at(x, y)) im.count[(size_t)y * nx + x] = name == "two_rows" ? 1 + (y == 292) : 1 + (x + y) % 2;
    return im;
}

struct Tally {
    int cases = 0, bad = 0;
    long ties = 0;
    void compare(const Result &got, const Result &want, const char *name, const Image &im, int min_count, int cap, int how, int tile, int halo) {
        ++cases;
        if (got == want) return;
        ++bad;
        std::fprintf(stderr, "MISMATCH %s %dx%d min_count %d max_dist %d how %d tile %d halo %d\n", name, im.nx, im.ny, min_count, cap, how, tile, halo);
    }
};

// the window of how 1 with the tiling the launcher chooses, where it keeps a tile with a halo in LDS
void launcher_window(Tally &t, const Image &im, const std::vector<int32_t> &gx, const Result &want, const char *name, int min_count, int cap) {
    const PwppDistPlan p = pwpp_dist_plan(im.ny, cap, 0);
    if (p.lds && p.halo > 0) t.compare(column_pass(im, gx, cap, 1, p.tile_rows, p.halo), want, name, im, min_count, cap, 1, p.tile_rows, p.halo);
}

// --plans: ny max_dist path lds tile_rows halo row_tiles
int print_plans() {
    for (int ny = 1; ny <= 1400; ++ny)
        for (int m = 0; m <= 301; ++m)
            for (int path = 0; path < 2; ++path) {
                const int max_dist = m <= 300 ? m : PWPP_DIST_MAX_CAP;
                const PwppDistPlan p = pwpp_dist_plan(ny, max_dist, path);
                std::printf("%d %d %d %d %d %d %d\n", ny, max_dist, path, p.lds, p.tile_rows, p.halo, p.row_tiles);
            }
    return 0;
}

// --tall: the shapes, caps and patterns at which the column pass takes each of its tilings (several strips, several tiles).  The
// pass over every row has no tiling and is left to the small shapes.
void run_tall(Tally &t) {
    const int shapes[][2] = {{130, 577}, {65, 513}};
    const char *names[] = {"row_top", "row_bottom", "row_mid", "two_rows", "lattice", "columns", "corners", "sparse", "borders"};
    const int caps[] = {0, 1, 64, 65, 223, 224, 225, PWPP_DIST_MAX_CAP};
    for (const auto &sh : shapes)
        for (const char *name : names) {
            const Image im = tall_pattern(name, sh[0], sh[1], caps, 8);
            for (int min_count = 1; min_count <= 2; ++min_count) {
                if (min_count == 2 && std::string(name) != "two_rows" && std::string(name) != "sparse") continue;
                std::vector<int32_t> gx;
                row_pass(im, min_count, gx);
                const Result unlimited = brute_force(im, min_count, t.ties);
                for (int cap : caps) {
                    const Result want = capped(unlimited, cap);
                    if (!pwpp_dist_plan(sh[1], cap, 0).lds)  // (the launcher reads the whole column)
                        t.compare(column_pass(im, gx, cap, 0, PWPP_DIST_TALL_TILE, 0), want, name, im, min_count, cap, 0, PWPP_DIST_TALL_TILE, 0);
                    if (cap == 0) continue;  // (a window needs a cap)
                    launcher_window(t, im, gx, want, name, min_count, cap);
                    if (cap > 65) continue;  // (the windows of ny and 7 rows under a long halo are nearly the whole column each: left out)
                    for (int tile : {sh[1], 7}) t.compare(column_pass(im, gx, cap, 1, tile, cap), want, name, im, min_count, cap, 1, tile, cap);
                }
            }
        }
}

}  // namespace

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "--plans") return print_plans();
    Tally t;
    if (mode == "--tall") {
        run_tall(t);
        std::printf("distance_check: %d tall cases, %ld cells with more than one nearest cell, %d mismatches\n", t.cases, t.ties, t.bad);
        return t.bad ? 1 : 0;
    }
    if (!mode.empty()) {
        std::fprintf(stderr, "usage: distance_check [--tall | --plans]\n");
        return 2;
    }
    const int shapes[][2] = {{1, 1}, {7, 5}, {64, 16}, {65, 17}, {129, 33}, {257, 3}, {3, 257}, {5, 700}, {130, 2}, {64, 1}, {63, 2}};
    const char *names[] = {"empty", "full", "checker", "corners", "single", "last_row", "columns", "random0.003", "random0.03", "random0.3"};
    const int caps[] = {0, 1, 2, 5, 20};
    std::mt19937 rng(20240611u);
    for (const auto &sh : shapes)
        for (const char *name : names)
            for (int min_count = 1; min_count <= 2; ++min_count) {
                const Image im = pattern(name, sh[0], sh[1], min_count, rng);
                std::vector<int32_t> gx;
                row_pass(im, min_count, gx);
                const Result unlimited = brute_force(im, min_count, t.ties);
                for (int cap : caps) {
                    const Result want = capped(unlimited, cap);
                    for (int how = 0; how < 3; ++how) {
                        if (how == 1 && cap == 0) continue;  // (a window needs a cap)
                        for (int tile : {sh[1], 7}) t.compare(column_pass(im, gx, cap, how, tile, cap), want, name, im, min_count, cap, how, tile, cap);
                    }
                    launcher_window(t, im, gx, want, name, min_count, cap);
                }
            }
    // the metres of a few squared distances: the bits of sqrt in double, times the cell, rounded once
    {
        const float m5 = pwpp_dist_metres(25, 0.5), m2 = pwpp_dist_metres(2, 0.3), none = pwpp_dist_metres((int32_t)PWPP_DIST_NONE, 0.5);
        const float want2 = (float)(1.4142135623730951 * 0.3);
        if (m5 != 2.5f || std::memcmp(&m2, &want2, 4) != 0 || !(none > 3.4e38f) || pwpp_dist_metres(0, 0.3) != 0.0f) {
            ++t.bad;
            std::fprintf(stderr, "MISMATCH metres\n");
        }
    }
    std::printf("distance_check: %d cases, %ld cells with more than one nearest cell, %d mismatches\n", t.cases, t.ties, t.bad);
    return t.bad ? 1 : 0;
}
