// reach_check.cpp -- the functions of csrc/pwpp_reach.h on the host, dealt as the kernels of pwpp_reach.hip deal them, against a
// brute-force Dijkstra of its own (an array scan for the nearest open cell, no heap, the step rule written out again).
//   * the sweeps of k_reach_sweep, forwards and backwards, in place;
//   * the tiles of k_reach_tiles: a dirty tile and its clipped halo copied out, relaxed to its fixed point, the changed cells
//     written back, the neighbours whose halo holds a changed border cell marked -- with small tiles on small images, so that every
//     image has many, and with the kernel's own tile on larger ones; the dirty set dealt twice, as a flag per tile that is read again
//     for every tile (relax_tiles) and as the kernel deals it, in words of 32 bits of which a pass walks a copy (relax_words), on frames
//     of up to 625 tiles (20 words) and, with the kernel's own tile, of 34, 36 and 66 tiles: the two agree byte for byte;
//   * the sweep bound of every schedule; the from rule; max_reach against the unlimited field masked;
//   * the range bound at its edge, and the largest candidate it lets the kernels form in uint32.
// Inputs: random images with lethal and unknown cells, every kind of rule, and adversarial ones (serpentines, diagonal gaps, sealed
// and impassable sources, uniform fields full of ties).
//   reach_check dump cost.i8 nx ny frames base lethal unknown clearance2 max_reach dist2.i32|- sources.i32 n_sources out
// writes out.reach and out.from (int32) for the images of a file, which tests/test_reach_cpu.py compares with tests/reach_ref.py.
// Build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I patchwork-plusplus_amd/csrc tools/reach_check.cpp -o reach_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "pwpp_reach.h"

namespace {

long g_cases = 0, g_bad = 0;
void expect(bool ok, const char *what) {
    if (!ok && g_bad++ < 20) std::printf("MISMATCH: %s\n", what);
}

struct Frame {
    int nx, ny, sx, sy;
    std::vector<int8_t> cost;
    std::vector<int32_t> dist2;  // empty: none
    PwppReachRule R;
};

std::vector<uint16_t> terms_of(const Frame &F) {
    std::vector<uint16_t> t((size_t)F.nx * F.ny);
    for (int i = 0; i < F.nx * F.ny; ++i)
        t[i] = (uint16_t)pwpp_reach_term(F.R, F.cost[i], F.dist2.empty() ? 0 : F.dist2[i], i == F.sy * F.nx + F.sx);
    return t;
}
std::vector<uint32_t> start_of(const Frame &F) {
    std::vector<uint32_t> v((size_t)F.nx * F.ny, PWPP_REACH_UNREACHED);
    v[(size_t)F.sy * F.nx + F.sx] = 0;
    return v;
}

// k_reach_sweep: in place, every cell once a sweep; returns the sweeps run
int64_t relax_sweeps(const Frame &F, const std::vector<uint16_t> &t, std::vector<uint32_t> &v, bool backwards) {
    const int cells = F.nx * F.ny;
    PwppReachImageView n{t.data(), v.data(), F.nx, F.ny, 0, 0};
    for (int64_t sweep = 1;; ++sweep) {
        bool changed = false;
        for (int k = 0; k < cells; ++k) {
            const int i = backwards ? cells - 1 - k : k;
            if (t[i] == 0) continue;
            n.y = i / F.nx, n.x = i - n.y * F.nx;
            const uint32_t best = pwpp_reach_best(n, (uint32_t)F.R.max_reach);
            if (best < v[i]) v[i] = best, changed = true;
        }
        if (!changed) return sweep;
        if (sweep > pwpp_reach_sweep_bound(cells)) return -1;
    }
}

// k_reach_tiles with tiles of tx x ty cells; returns the passes run
struct TileView {
    const uint16_t *term;
    const uint32_t *value;
    int w, at;
    uint32_t t(int dx, int dy) const { return term[at + dy * w + dx]; }
    uint32_t v(int dx, int dy) const { return value[at + dy * w + dx]; }
};
// one visit of tile q: the tile and its clipped halo copied out, relaxed to its fixed point, the changed cells written back; `loaded()`
// is called once the copy is made (where the kernel clears the tile's bit) and `mark(u)` for every neighbour tile whose halo holds a
// changed border cell.  false: the visit ran past its bound.
struct TileVisit {
    const Frame &F;
    const std::vector<uint16_t> &t;
    std::vector<uint32_t> &v;
    int tx, ty, tiles_x, tiles_y, w, h;
    std::vector<uint16_t> lt;
    std::vector<uint32_t> lv;
    TileVisit(const Frame &F_, const std::vector<uint16_t> &t_, std::vector<uint32_t> &v_, int tx_, int ty_)
        : F(F_), t(t_), v(v_), tx(tx_), ty(ty_), tiles_x((F_.nx + tx_ - 1) / tx_), tiles_y((F_.ny + ty_ - 1) / ty_), w(tx_ + 2), h(ty_ + 2), lt((size_t)w * h), lv((size_t)w * h) {}
    // the source's tile and the tiles around it: the source's 0 may lie in their halo, and it never changes
    template <class Mark>
    void first_marks(Mark mark) const {
        for (int ey = -1; ey <= 1; ++ey)
            for (int ex = -1; ex <= 1; ++ex) {
                const int ux = F.sx / tx + ex, uy = F.sy / ty + ey;
                if (ux >= 0 && ux < tiles_x && uy >= 0 && uy < tiles_y) mark(uy * tiles_x + ux);
            }
    }
    template <class Loaded, class Mark>
    bool operator()(int q, Loaded loaded, Mark mark) {
        const int qx = q % tiles_x, qy = q / tiles_x, x0 = qx * tx, y0 = qy * ty;
        for (int i = 0; i < w * h; ++i) {
            const int ly = i / w, lx = i - ly * w, gx = x0 + lx - 1, gy = y0 + ly - 1;
            const bool in = gx >= 0 && gx < F.nx && gy >= 0 && gy < F.ny;
            lt[i] = in ? t[(size_t)gy * F.nx + gx] : (uint16_t)0;
            lv[i] = lt[i] ? v[(size_t)gy * F.nx + gx] : PWPP_REACH_UNREACHED;
        }
        loaded();
        std::vector<char> mine((size_t)tx * ty, 0);
        for (int sweep = 1;; ++sweep) {
            bool changed = false;
            for (int c = 0; c < tx * ty; ++c) {
                const int at = (c / tx + 1) * w + c % tx + 1;
                if (lt[at] == 0) continue;
                const TileView n{lt.data(), lv.data(), w, at};
                const uint32_t best = pwpp_reach_best(n, (uint32_t)F.R.max_reach);
                if (best < lv[at]) lv[at] = best, changed = true, mine[c] = 1;
            }
            if (!changed) break;
            if (sweep > tx * ty + 1) return false;
        }
        for (int c = 0; c < tx * ty; ++c) {
            if (!mine[c]) continue;
            const int lx = c % tx, ly = c / tx;
            v[(size_t)(y0 + ly) * F.nx + x0 + lx] = lv[(ly + 1) * w + lx + 1];
            const int ddx = lx == 0 ? -1 : (lx == tx - 1 ? 1 : 0), ddy = ly == 0 ? -1 : (ly == ty - 1 ? 1 : 0);
            // (a tile one cell wide or high: the cell is on both borders; the kernel's tile is wider than that)
            for (int ey = -1; ey <= 1; ++ey)
                for (int ex = -1; ex <= 1; ++ex) {
                    const bool bx = ex == 0 || ex == ddx || (tx == 1), by = ey == 0 || ey == ddy || (ty == 1);
                    if ((ex == 0 && ey == 0) || !bx || !by) continue;
                    const int ux = qx + ex, uy = qy + ey;
                    if (ux >= 0 && ux < tiles_x && uy >= 0 && uy < tiles_y) mark(uy * tiles_x + ux);
                }
        }
        return true;
    }
};

// a flag per tile, read again for every tile: a mark on a later tile is seen in the same pass, one on an earlier tile in the next
int64_t relax_tiles(const Frame &F, const std::vector<uint16_t> &t, std::vector<uint32_t> &v, int tx, int ty) {
    TileVisit visit(F, t, v, tx, ty);
    std::vector<char> dirty((size_t)visit.tiles_x * visit.tiles_y, 0);
    const auto mark = [&](int u) { dirty[u] = 1; };
    visit.first_marks(mark);
    for (int64_t pass = 1;; ++pass) {
        bool any = false;
        for (int q = 0; q < visit.tiles_x * visit.tiles_y; ++q) {
            if (!dirty[q]) continue;
            any = true;
            if (!visit(q, [&] { dirty[q] = 0; }, mark)) return -1;
        }
        if (!any) return pass;
        if (pass > pwpp_reach_sweep_bound((int64_t)F.nx * F.ny)) return -1;
    }
}

// k_reach_tiles' own deal of the dirty set: a bit per tile in words of 32.  Per pass and word a COPY of the word is taken once and
// its tiles are visited lowest bit first; the visited tile's bit is cleared in the live word after its load; marks are OR-ed into the
// live words, so one in a later word is seen in this pass and one in the word being walked or an earlier word in the next.  A pass
// ends after the last word; the run ends with the first pass that found no bit.  `most_words`: the words of the bitmap.
int64_t relax_words(const Frame &F, const std::vector<uint16_t> &t, std::vector<uint32_t> &v, int tx, int ty, int *most_words = nullptr) {
    TileVisit visit(F, t, v, tx, ty);
    const int tiles = visit.tiles_x * visit.tiles_y, words = (tiles + 31) >> 5;
    if (most_words) *most_words = words;
    std::vector<uint32_t> dirty((size_t)words, 0u);
    const auto mark = [&](int u) { dirty[(size_t)(u >> 5)] |= 1u << (u & 31); };
    visit.first_marks(mark);
    const int64_t bound = pwpp_reach_sweep_bound((int64_t)F.nx * F.ny);
    for (int64_t pass = 0;; ++pass) {
        if (pass >= bound) return -1;
        bool any = false;
        for (int w = 0; w < words; ++w) {
            uint32_t bits = dirty[(size_t)w];
            while (bits != 0) {
                const int low = __builtin_ctz(bits), q = (w << 5) + low;
                bits &= bits - 1;
                any = true;
                if (q >= tiles) return -2;  // (a bit beyond the last tile: never set)
                if (!visit(q, [&] { dirty[(size_t)w] &= ~(1u << low); }, mark)) return -1;
            }
        }
        if (!any) return pass + 1;  // (the passes run, the empty one among them)
    }
}

std::vector<int32_t> from_of(const Frame &F, const std::vector<uint16_t> &t, const std::vector<uint32_t> &v) {
    std::vector<int32_t> from((size_t)F.nx * F.ny, -1);
    for (int i = 0; i < F.nx * F.ny; ++i) {
        if (v[i] == PWPP_REACH_UNREACHED) continue;
        const int y = i / F.nx, x = i - y * F.nx;
        if (x == F.sx && y == F.sy) {
            from[i] = i;
            continue;
        }
        const PwppReachImageView n{t.data(), v.data(), F.nx, F.ny, x, y};
        const int k = pwpp_reach_from(n, v[i]);
        from[i] = k < 0 ? -2 : (y + pwpp_reach_dy(k)) * F.nx + x + pwpp_reach_dx(k);
    }
    return from;
}

// ---- the brute force: the contract written out again -----------------------------------------------------------------------------
bool brute_passable(const Frame &F, int x, int y) {
    if (x < 0 || x >= F.nx || y < 0 || y >= F.ny) return false;
    if (x == F.sx && y == F.sy) return true;
    int c = F.cost[(size_t)y * F.nx + x];
    if (c < 0) {
        if (F.R.unknown < 0) return false;
        c = F.R.unknown;
    }
    if (c >= F.R.lethal) return false;
    return F.dist2.empty() || F.dist2[(size_t)y * F.nx + x] > F.R.clearance2;
}
long brute_t(const Frame &F, int x, int y) {
    int c = F.cost[(size_t)y * F.nx + x];
    if (c < 0) c = F.R.unknown;
    const bool own = c >= 0 && c < F.R.lethal && (F.dist2.empty() || F.dist2[(size_t)y * F.nx + x] > F.R.clearance2);
    return own ? F.R.base + c : F.R.base;  // (a source that is passable by its rule alone)
}
// the step from (x, y) to (x + dx, y + dy), or -1
long brute_step(const Frame &F, int x, int y, int dx, int dy) {
    if (!brute_passable(F, x, y) || !brute_passable(F, x + dx, y + dy)) return -1;
    if (dx != 0 && dy != 0 && (!brute_passable(F, x + dx, y) || !brute_passable(F, x, y + dy))) return -1;
    return (dx != 0 && dy != 0 ? 7 : 5) * (brute_t(F, x, y) + brute_t(F, x + dx, y + dy));
}
void brute(const Frame &F, std::vector<int64_t> &d, std::vector<int32_t> &from) {
    const int cells = F.nx * F.ny;
    const int64_t inf = INT64_MAX;
    d.assign(cells, inf);
    std::vector<char> done(cells, 0);
    d[F.sy * F.nx + F.sx] = 0;
    for (;;) {
        int u = -1;
        for (int i = 0; i < cells; ++i)
            if (!done[i] && d[i] != inf && (u < 0 || d[i] < d[u])) u = i;
        if (u < 0) break;
        done[u] = 1;
        const int y = u / F.nx, x = u % F.nx;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (!dx && !dy) continue;
                const long s = brute_step(F, x, y, dx, dy);
                if (s >= 0 && d[u] + s < d[(y + dy) * F.nx + x + dx]) d[(y + dy) * F.nx + x + dx] = d[u] + s;
            }
    }
    if (F.R.max_reach > 0)
        for (int i = 0; i < cells; ++i)
            if (d[i] != inf && d[i] > F.R.max_reach) d[i] = inf;
    from.assign(cells, -1);
    for (int i = 0; i < cells; ++i) {
        if (d[i] == inf) continue;
        const int y = i / F.nx, x = i % F.nx;
        if (i == F.sy * F.nx + F.sx) {
            from[i] = i;
            continue;
        }
        for (int dy = -1; dy <= 1 && from[i] < 0; ++dy)  // (rows first: the index order)
            for (int dx = -1; dx <= 1 && from[i] < 0; ++dx) {
                if (!dx && !dy) continue;
                const long s = brute_step(F, x + dx, y + dy, -dx, -dy);
                const int j = (y + dy) * F.nx + x + dx;
                if (s >= 0 && d[j] != inf && d[j] + s == d[i]) from[i] = j;
            }
    }
}

void check_frame(const Frame &F) {
    ++g_cases;
    const std::vector<uint16_t> t = terms_of(F);
    std::vector<int64_t> d;
    std::vector<int32_t> bf;
    brute(F, d, bf);
    std::vector<uint32_t> want((size_t)F.nx * F.ny);
    for (size_t i = 0; i < want.size(); ++i) {
        expect(d[i] == INT64_MAX || d[i] < (int64_t)PWPP_REACH_UNREACHED, "a true value at or beyond PWPP_REACH_NONE");
        want[i] = d[i] == INT64_MAX ? PWPP_REACH_UNREACHED : (uint32_t)d[i];
    }
    const int small[4][2] = {{4, 3}, {1, 1}, {5, 2}, {PWPP_REACH_TILE_X, PWPP_REACH_TILE_Y}};
    for (int schedule = 0; schedule < 6; ++schedule) {
        std::vector<uint32_t> v = start_of(F);
        const int64_t n = schedule < 2 ? relax_sweeps(F, t, v, schedule == 1) : relax_tiles(F, t, v, small[schedule - 2][0], small[schedule - 2][1]);
        expect(n > 0 && n <= pwpp_reach_sweep_bound((int64_t)F.nx * F.ny), "a schedule ran past its bound");
        expect(v == want, "reach differs from the brute force");
        if (v != want && g_bad < 4)
            for (size_t i = 0; i < v.size(); ++i)
                if (v[i] != want[i]) {
                    std::printf("  schedule %d, %d x %d, source (%d, %d), cell %zu: %u, brute %u; rule %d %d %d %d %d %d\n", schedule, F.nx, F.ny, F.sx, F.sy, i, v[i], want[i],
                                F.R.base, F.R.lethal, F.R.unknown, F.R.clearance2, F.R.max_reach, F.R.use_dist2);
                    break;
                }
        if (schedule == 0 || schedule == 5) {
            const std::vector<int32_t> from = from_of(F, t, v);
            expect(from == bf, "from differs from the brute force");
            for (size_t i = 0; i < from.size(); ++i)  // the chain falls strictly
                if (from[i] >= 0 && (int)i != F.sy * F.nx + F.sx) expect(v[from[i]] < v[i], "from does not fall");
        }
    }
}

// The word schedule against the brute force, against its bound and, byte for byte, against relax_tiles, for every tile size given.
int g_most_words = 0;
void check_words(const Frame &F, const std::vector<std::pair<int, int>> &tile_sizes) {
    ++g_cases;
    const std::vector<uint16_t> t = terms_of(F);
    std::vector<int64_t> d;
    std::vector<int32_t> bf;
    brute(F, d, bf);
    std::vector<uint32_t> want((size_t)F.nx * F.ny);
    for (size_t i = 0; i < want.size(); ++i) want[i] = d[i] == INT64_MAX ? PWPP_REACH_UNREACHED : (uint32_t)d[i];
    for (const auto &ts : tile_sizes) {
        std::vector<uint32_t> a = start_of(F), b = a;
        int words = 0;
        const int64_t na = relax_tiles(F, t, a, ts.first, ts.second), nb = relax_words(F, t, b, ts.first, ts.second, &words);
        g_most_words = std::max(g_most_words, words);
        expect(na > 0 && nb > 0 && nb <= pwpp_reach_sweep_bound((int64_t)F.nx * F.ny), "the word schedule ran past its bound");
        expect(b == want, "the word schedule's reach differs from the brute force");
        expect(a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(uint32_t)) == 0, "the word schedule and the flag schedule differ");
        if (b != want && g_bad < 4)
            for (size_t i = 0; i < b.size(); ++i)
                if (b[i] != want[i]) {
                    std::printf("  words, tile %d x %d, %d x %d, source (%d, %d), cell %zu: %u, brute %u\n", ts.first, ts.second, F.nx, F.ny, F.sx, F.sy, i, b[i], want[i]);
                    break;
                }
        expect(from_of(F, t, b) == bf, "from of the word schedule differs from the brute force");
    }
}

Frame random_frame(std::mt19937 &rng, int nx, int ny) {
    Frame F;
    F.nx = nx, F.ny = ny;
    F.sx = (int)(rng() % nx), F.sy = (int)(rng() % ny);
    F.cost.resize((size_t)nx * ny);
    const int kind = (int)(rng() % 4);  // 0: every byte; 1: few walls; 2: many walls; 3: uniform (ties everywhere)
    const int same = (int)(rng() % 101);
    for (auto &c : F.cost) {
        const int u = (int)(rng() % 100);
        if (kind == 0) c = (int8_t)(rng() % 256);
        else if (kind == 3) c = (int8_t)(u < 10 ? 127 : same);
        else c = (int8_t)(u < (kind == 1 ? 15 : 40) ? 100 + rng() % 28 : (u > 92 ? -1 - (int)(rng() % 128) : rng() % 100));
    }
    const int lethals[4] = {101, 100, 1, 1 + (int)(rng() % 101)};
    F.R = PwppReachRule{1 + (int)(rng() % 255), lethals[rng() % 4], (int)(rng() % 102) - 1, 0, 0, 0};
    if (rng() % 3 == 0) {
        F.dist2.resize(F.cost.size());
        for (auto &q : F.dist2) q = rng() % 5 == 0 ? PWPP_REACH_DIST_BEYOND : (int32_t)(rng() % 9);
        F.R.clearance2 = (int)(rng() % 6), F.R.use_dist2 = 1;
    }
    return F;
}

void random_cases() {
    std::mt19937 rng(20261);
    for (int k = 0; k < 1500; ++k) {
        Frame F = random_frame(rng, 1 + (int)(rng() % 13), 1 + (int)(rng() % 11));
        check_frame(F);
        // max_reach at a value of the field, one below it, and far beyond: the unlimited field masked (the brute force masks, the schedules prune)
        std::vector<uint32_t> v = start_of(F);
        const std::vector<uint16_t> t = terms_of(F);
        relax_sweeps(F, t, v, false);
        const uint32_t pick = v[rng() % v.size()];
        if (pick != PWPP_REACH_UNREACHED && pick > 1) {
            F.R.max_reach = (int32_t)pick;
            check_frame(F);
            F.R.max_reach = (int32_t)pick - 1;
            check_frame(F);
        }
    }
    for (int k = 0; k < 12; ++k) {  // larger ones: several of the kernel's tiles
        Frame F = random_frame(rng, 30 + (int)(rng() % 40), 30 + (int)(rng() % 40));
        check_frame(F);
    }
}

void adversarial_cases() {
    const PwppReachRule R{3, 100, -1, 0, 0, 0};
    for (int nx = 1; nx <= 9; ++nx)
        for (int ny = 1; ny <= 9; ++ny) {
            Frame F{nx, ny, 0, 0, std::vector<int8_t>((size_t)nx * ny, 100), {}, R};  // a serpentine from (0, 0)
            for (int y = 0; y < ny; ++y)
                for (int x = 0; x < nx; ++x)
                    if (y % 2 == 0 || x == ((y / 2) % 2 == 0 ? nx - 1 : 0)) F.cost[(size_t)y * nx + x] = (int8_t)(x % 3);
            check_frame(F);
            F.sx = nx - 1, F.sy = ny - 1;  // from the far corner, on a wall or not
            check_frame(F);
            std::fill(F.cost.begin(), F.cost.end(), (int8_t)0);  // open and uniform: ties everywhere; the closed form
            check_frame(F);
            std::vector<uint32_t> v = start_of(F);
            relax_sweeps(F, terms_of(F), v, false);
            for (int y = 0; y < ny; ++y)
                for (int x = 0; x < nx; ++x) {
                    const int dx = nx - 1 - x, dy = ny - 1 - y;
                    expect(v[(size_t)y * nx + x] == (uint32_t)(2 * 3 * (5 * std::max(dx, dy) + 2 * std::min(dx, dy))), "the octile closed form");
                }
            std::fill(F.cost.begin(), F.cost.end(), (int8_t)100);  // sealed: only the source, itself lethal
            check_frame(F);
        }
    {  // a diagonal gap between two lethal cells is closed, from either side
        Frame F{2, 2, 0, 0, {0, 100, 100, 0}, {}, R};
        check_frame(F);
        std::vector<uint32_t> v = start_of(F);
        relax_sweeps(F, terms_of(F), v, false);
        expect(v[3] == PWPP_REACH_UNREACHED, "a path squeezed through a diagonal gap");
        F.cost = {0, 0, 100, 0};  // one blocked cell: the corner is not cut, the way round costs two edges
        v = start_of(F);
        relax_sweeps(F, terms_of(F), v, false);
        expect(v[3] == 2u * 5u * 6u, "a corner was cut");
    }
}

// walls one cell thick across the image every `pitch` cells, each open for `gap` cells alternately at one end and the other: the path runs
// the whole image back and forth, through every tile, and on into tiles of smaller index as often as into tiles of larger index
void comb_walls(Frame &F, int pitch, int gap, bool across_x) {
    const int along = across_x ? F.nx : F.ny, other = across_x ? F.ny : F.nx;
    for (int k = 0, p = pitch; p < along - 1; p += pitch, ++k)
        for (int o = 0; o < other; ++o) {
            const bool open = k % 2 == 0 ? o >= other - gap : o < gap;
            const int x = across_x ? p : o, y = across_x ? o : p;
            if (x == F.sx && y == F.sy) continue;
            F.cost[(size_t)y * F.nx + x] = (int8_t)(open ? 0 : 100);
        }
}

// frames of hundreds of tiles: the dirty bitmap has many words, the source's first marks and a tile's marks fall into two of them
void word_cases() {
    std::mt19937 rng(40077);
    const std::vector<std::pair<int, int>> small = {{2, 2}, {3, 2}};
    for (int k = 0; k < 48; ++k) {
        Frame F = random_frame(rng, 20 + (int)(rng() % 31), 20 + (int)(rng() % 31));
        if (k % 3 != 0) comb_walls(F, 3 + (int)(rng() % 6), 1 + (int)(rng() % 2), k % 3 == 1);
        if (k % 4 == 0) F.sx = F.nx - 1, F.sy = F.ny - 1;  // the front moves to smaller tile indices: every mark waits a pass
        check_words(F, small);
        if (k % 6 == 0) {  // under max_reach most tiles are never visited
            std::vector<uint32_t> v = start_of(F);
            relax_sweeps(F, terms_of(F), v, false);
            std::vector<uint32_t> got;
            for (uint32_t x : v)
                if (x != PWPP_REACH_UNREACHED && x > 1) got.push_back(x);
            if (!got.empty()) {
                std::sort(got.begin(), got.end());
                F.R.max_reach = (int32_t)got[got.size() / 4];
                check_words(F, small);
            }
        }
    }
    {
        Frame F = random_frame(rng, 50, 50);  // 625 and 425 tiles
        comb_walls(F, 4, 1, true);
        check_words(F, small);
    }
    // the kernel's own tile on frames of more than 32 tiles: rows and columns of 34 and 66 tiles from either end, 6 x 6 tiles
    const std::vector<std::pair<int, int>> own = {{PWPP_REACH_TILE_X, PWPP_REACH_TILE_Y}};
    const int sides[4][2] = {{33 * PWPP_REACH_TILE_X + 1, 3}, {3, 33 * PWPP_REACH_TILE_Y + 1}, {65 * PWPP_REACH_TILE_X + 1, 2}, {5 * PWPP_REACH_TILE_X + 3, 5 * PWPP_REACH_TILE_Y + 1}};
    for (int k = 0; k < 4; ++k)
        for (int end = 0; end < 2; ++end) {
            if (k == 3 && end == 1) continue;  // (the brute force scans every cell for every cell)
            Frame F = random_frame(rng, sides[k][0], sides[k][1]);
            F.R = PwppReachRule{2, 100, 30, 0, 0, 0};
            F.dist2.clear();
            for (auto &c : F.cost) c = (int8_t)(rng() % 100);
            F.sx = end ? F.nx - 1 : 0, F.sy = end ? F.ny - 1 : 0;
            comb_walls(F, k == 3 ? 24 : 37, k == 3 ? 3 : 1, F.nx >= F.ny);
            check_words(F, own);
        }
    expect(g_most_words > 13, "no frame with more than 13 words of dirty bits");
}

void range_cases() {
    int64_t worst = 0;
    // the largest image of every base: accepted at the edge, refused one cell beyond
    for (int base = 1; base <= 255; ++base) {
        const int64_t cells = ((int64_t)0x7ffffffe) / (14 * ((int64_t)base + 100)) + 1;  // the largest count with 14 (base + 100) (cells - 1) <= 2^31 - 2
        ++g_cases;
        expect(cells <= 1518730 && pwpp_reach_range_ok(base, 1, 1, worst) && worst == 0, "one cell");
        // (as one row, whatever the entry points' side limit: the function reads the product alone)
        expect(pwpp_reach_range_ok(base, (int)cells, 1, worst) && worst <= 0x7ffffffeLL, "the range at its edge");
        expect(!pwpp_reach_range_ok(base, 1, (int)cells + 1, worst) && worst > 0x7ffffffeLL, "the range one past its edge");
        // a candidate: a stored value plus a step, in uint32
        const uint64_t cand = (uint64_t)0x7ffffffe + pwpp_reach_step((uint32_t)base + 100, (uint32_t)base + 100, true);
        expect(cand < ((uint64_t)1 << 32) && pwpp_reach_step((uint32_t)base + 100, (uint32_t)base + 100, true) == 14u * ((uint32_t)base + 100), "a candidate in uint32");
    }
    expect(pwpp_reach_range_ok(1, 1518501 / 3, 3, worst), "1518501 cells at base 1");  // 14 * 101 * 1518500 = 2147159000 <= 2^31 - 2
    expect(!pwpp_reach_range_ok(255, 32768, 32768, worst) && worst > 0, "the largest image in 64 bits");
    // a chain that is as dear as the bound lets it be: every step a corner between cells of cost 100
    for (int base : {1, 100, 255}) {
        const int n = 40;
        Frame F{n, n, 0, 0, std::vector<int8_t>((size_t)n * n, 100), {}, PwppReachRule{base, 101, -1, 0, 0, 0}};
        check_frame(F);
        std::vector<uint32_t> v = start_of(F);
        relax_sweeps(F, terms_of(F), v, false);
        expect(v[(size_t)n * n - 1] == (uint32_t)(14 * (base + 100) * (n - 1)), "the diagonal of a field of cost 100");
    }
    // the tiles of the largest frames the entry points accept (sides <= 32768, the range at base 1): PWPP_REACH_MAX_TILES holds them
    int64_t most_tiles = 0;
    for (int64_t ny = 1; ny <= 32768; ++ny) {
        const int64_t nx = std::min<int64_t>(32768, 1518730 / ny);
        if (nx < ny) break;  // (the count is symmetric in the sides)
        ++g_cases;
        expect(pwpp_reach_range_ok(1, (int)nx, (int)ny, worst) && (nx == 32768 || !pwpp_reach_range_ok(1, (int)nx + 1, (int)ny, worst)), "the widest frame of a height");
        // (a narrower frame of this height may end a tile later in x: every width down to the start of the last tile column counts the same)
        most_tiles = std::max(most_tiles, ((nx + PWPP_REACH_TILE_X - 1) / PWPP_REACH_TILE_X) * ((ny + PWPP_REACH_TILE_Y - 1) / PWPP_REACH_TILE_Y));
    }
    expect(most_tiles == 2193 && most_tiles <= PWPP_REACH_MAX_TILES && PWPP_REACH_MAX_TILES % 32 == 0, "the largest number of tiles");
    // the neighbour order is the index order
    for (int k = 0; k + 1 < 8; ++k) expect(pwpp_reach_dy(k) * 3 + pwpp_reach_dx(k) < pwpp_reach_dy(k + 1) * 3 + pwpp_reach_dx(k + 1), "the neighbour order");
}

template <class T>
std::vector<T> read_file(const char *path, size_t n) {
    std::vector<T> v(n);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "reach_check: cannot read %zu elements from %s\n", n, path);
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

int dump(char **a) {
    const int nx = std::atoi(a[1]), ny = std::atoi(a[2]), frames = std::atoi(a[3]);
    const size_t per = (size_t)nx * ny;
    const std::vector<int8_t> cost = read_file<int8_t>(a[0], per * frames);
    const bool with_dist2 = std::strcmp(a[9], "-") != 0;
    const std::vector<int32_t> dist2 = with_dist2 ? read_file<int32_t>(a[9], per * frames) : std::vector<int32_t>();
    const int n_sources = std::atoi(a[11]);
    const std::vector<int32_t> src = read_file<int32_t>(a[10], 2 * (size_t)n_sources);
    const PwppReachRule R{std::atoi(a[4]), std::atoi(a[5]), std::atoi(a[6]), with_dist2 ? std::atoi(a[7]) : 0, std::atoi(a[8]), with_dist2 ? 1 : 0};
    int64_t worst = 0;
    if (!pwpp_reach_range_ok(R.base, nx, ny, worst)) return 3;
    FILE *fr = std::fopen((std::string(a[12]) + ".reach").c_str(), "wb"), *ff = std::fopen((std::string(a[12]) + ".from").c_str(), "wb");
    if (!fr || !ff) return 2;
    for (int f = 0; f < frames; ++f) {
        Frame F{nx, ny, src[n_sources > 1 ? 2 * f : 0], src[n_sources > 1 ? 2 * f + 1 : 1], std::vector<int8_t>(cost.begin() + f * per, cost.begin() + (f + 1) * per),
                with_dist2 ? std::vector<int32_t>(dist2.begin() + f * per, dist2.begin() + (f + 1) * per) : std::vector<int32_t>(), R};
        const std::vector<uint16_t> t = terms_of(F);
        std::vector<uint32_t> v = start_of(F), w = v;
        if (relax_tiles(F, t, v, PWPP_REACH_TILE_X, PWPP_REACH_TILE_Y) < 0 || relax_sweeps(F, t, w, false) < 0 || v != w) return 4;
        const std::vector<int32_t> from = from_of(F, t, v);
        std::fwrite(v.data(), 4, per, fr), std::fwrite(from.data(), 4, per, ff);
    }
    std::fclose(fr), std::fclose(ff);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 15 && std::strcmp(argv[1], "dump") == 0) return dump(argv + 2);
    if (argc != 1) {
        std::fprintf(stderr, "usage: reach_check | reach_check dump cost.i8 nx ny frames base lethal unknown clearance2 max_reach dist2.i32|- sources.i32 n_sources out\n");
        return 2;
    }
    random_cases();
    adversarial_cases();
    range_cases();
    word_cases();
    std::printf("reach_check: %ld cases, %ld mismatches\n", g_cases, g_bad);
    return g_bad == 0 ? 0 : 1;
}
