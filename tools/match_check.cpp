// match_check.cpp -- the scan match's arithmetic on the host, against a brute force.
//
// The kernels of patchwork-plusplus_amd/csrc/pwpp_match.hip are built from the functions of pwpp_match.h (the packed cell, the
// landing of a cell under a candidate, what a landing adds to a shift's sum, the order of the argmax, the shifted pose).  This
// program runs the same sequence with the same functions over plain memory, dealt as the kernels deal it -- the frame's occupied
// cells compacted into packed words, a workgroup per (frame, candidate, tile of 256 shifts), chunks of 256 cells landed once, an
// int32 partial per chunk widened into an int64, the tile's best, then the best of the frame's tiles; on path 0 the rectangle of the
// map in reach copied into a buffer of its own, or not where it is larger than a cap -- with every array allocated
// at EXACTLY its size (an index outside one is a sanitizer error), on many small random cases: candidates that are identities,
// whole-cell translations, quarter turns, mirrors, random rotations, half outside, far away and not finite; windows from (0, 0) to
// more shifts than a tile; map values over the whole int16 range; skipped and empty frames.  It compares every score and every
// best row with a brute force written separately below: its own formulas, its own lexicographic maximum.  Exit status 0: all equal.
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -I patchwork-plusplus_amd/csrc tools/match_check.cpp -o match_check
// (tests/test_scan_match_cpu.py builds and runs it; it needs no GPU and no HIP.)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <tuple>
#include <vector>

#include "pwpp_match.h"

namespace {

struct Case {
    PwppMatchGeometry G;
    int frames, n_sets, n_candidates, n_maps, wx, wy;
    std::vector<int8_t> occupancy;      // frames * ny * nx
    std::vector<double> candidates;     // n_sets * n_candidates * 6
    std::vector<int32_t> map_of_frame;  // frames
    std::vector<int16_t> map;           // n_maps * NY * NX
};

struct Result {
    std::vector<int64_t> scores;        // frames * n_candidates * H * W
    std::vector<PwppMatchKey> best;     // frames
    bool operator==(const Result &o) const {
        if (scores != o.scores || best.size() != o.best.size()) return false;
        for (size_t i = 0; i < best.size(); ++i)
            if (best[i].score != o.best[i].score || best[i].candidate != o.best[i].candidate || best[i].sx != o.best[i].sx || best[i].sy != o.best[i].sy ||
                best[i].cells != o.best[i].cells)
                return false;
        return true;
    }
};

// the definition: every (frame, candidate, shift) on its own over the whole image
Result brute_force(const Case &c) {
    const int NX = c.G.NX, NY = c.G.NY, nx = c.G.nx, ny = c.G.ny, W = 2 * c.wx + 1, H = 2 * c.wy + 1;
    Result R{std::vector<int64_t>((size_t)c.frames * c.n_candidates * H * W, 0), std::vector<PwppMatchKey>((size_t)c.frames)};
    for (int f = 0; f < c.frames; ++f) {
        int cells = 0;
        for (int i = 0; i < nx * ny; ++i) cells += c.occupancy[(size_t)f * nx * ny + i] == 100;
        const int k = c.map_of_frame[f];
        if (k < 0) {
            R.best[f] = PwppMatchKey{0, -1, 0, 0, cells};
            continue;
        }
        typedef std::tuple<long long, long long, int, int, int> Key;  // (-score, d2, candidate, sy, sx): the smallest wins
        Key top(std::numeric_limits<long long>::max(), 0, 0, 0, 0);
        for (int r = 0; r < c.n_candidates; ++r) {
            const double *p = &c.candidates[((size_t)(c.n_sets == 1 ? 0 : f) * c.n_candidates + r) * 6];
            for (int sy = -c.wy; sy <= c.wy; ++sy)
                for (int sx = -c.wx; sx <= c.wx; ++sx) {
                    long long sum = 0;
                    for (int iy = 0; iy < ny; ++iy)
                        for (int ix = 0; ix < nx; ++ix) {
                            if (c.occupancy[((size_t)f * ny + iy) * nx + ix] != 100) continue;
                            const double hx = (double)ix + 0.5, hy = (double)iy + 0.5;
                            const double px = hx * c.G.cell, py = hy * c.G.cell;
                            const double x = c.G.x0 + px, y = c.G.y0 + py;
                            const double t0 = p[0] * x, t1 = p[1] * y, t2 = p[3] * x, t3 = p[4] * y;
                            const double s0 = t0 + t1, s1 = t2 + t3;
                            const double X = s0 + p[2], Y = s1 + p[5];
                            const double U = (X - c.G.X0) / c.G.CELL, V = (Y - c.G.Y0) / c.G.CELL;
                            if (!(U >= -1048576.0 && U < 1048576.0 && V >= -1048576.0 && V < 1048576.0)) continue;
                            const long long qx = (long long)std::floor(U) + sx, qy = (long long)std::floor(V) + sy;
                            if (qx >= 0 && qx < NX && qy >= 0 && qy < NY) sum += c.map[((size_t)k * NY + (size_t)qy) * NX + (size_t)qx];
                        }
                    R.scores[(((size_t)f * c.n_candidates + r) * H + (sy + c.wy)) * W + (sx + c.wx)] = sum;
                    top = std::min(top, Key(-sum, (long long)sx * sx + (long long)sy * sy, r, sy, sx));
                }
        }
        R.best[f] = PwppMatchKey{-std::get<0>(top), std::get<2>(top), std::get<4>(top), std::get<3>(top), cells};
    }
    return R;
}

long long staged_windows = 0, unstaged_windows = 0;  // (what the staged runs of main met: both must occur)

// the kernels' sequence with the header's functions
// `stage_cap` > 0: path 0, the rectangle of the map in reach copied into a buffer of EXACTLY its size where it holds at most so many
// cells, the map itself where it holds more; 0: path 1
template <bool RECIP>
Result as_the_kernels(const Case &c, int stage_cap = 0) {
    const int per_frame = c.G.nx * c.G.ny, per_map = c.G.NX * c.G.NY, W = 2 * c.wx + 1, H = 2 * c.wy + 1, shifts = W * H;
    const int tiles = (shifts + PWPP_MATCH_TILE - 1) / PWPP_MATCH_TILE;
    // k_match_compact
    std::vector<int32_t> cells((size_t)c.frames * per_frame), count((size_t)c.frames, 0);
    for (int f = 0; f < c.frames; ++f)
        for (int i = 0; i < per_frame; ++i)
            if (c.occupancy[(size_t)f * per_frame + i] == (int8_t)PWPP_MATCH_OCCUPIED) {
                const int iy = i / c.G.nx, ix = i - iy * c.G.nx;
                cells[(size_t)f * per_frame + count[f]++] = pwpp_match_pack(ix, iy);
            }
    // k_match_score
    Result R{std::vector<int64_t>((size_t)c.frames * c.n_candidates * shifts, 0), std::vector<PwppMatchKey>((size_t)c.frames)};
    std::vector<PwppMatchKey> partial((size_t)c.frames * c.n_candidates * tiles);
    std::vector<int32_t> Jx(PWPP_MATCH_CHUNK), Jy(PWPP_MATCH_CHUNK);
    for (int b = 0; b < c.frames * c.n_candidates * tiles; ++b) {
        const int tile = b % tiles, fr = b / tiles, r = fr % c.n_candidates, f = fr / c.n_candidates, k = c.map_of_frame[f];
        std::vector<int64_t> sum(PWPP_MATCH_TILE, 0);
        if (k >= 0) {
            const double *cand = &c.candidates[((size_t)(c.n_sets == 1 ? 0 : f) * c.n_candidates + r) * 6];
            const int16_t *m = c.map.data() + (size_t)k * per_map;
            const int16_t *src = m;
            int32_t ox = 0, oy = 0, SX = c.G.NX, SY = c.G.NY;
            bool any = true;
            std::vector<int16_t> stage;
            if (stage_cap > 0) {
                int32_t lo_x = INT32_MAX, hi_x = INT32_MIN, lo_y = INT32_MAX, hi_y = INT32_MIN, jx, jy, fx, fy, wn, hn;
                for (int i = 0; i < count[f]; ++i) {
                    int ix, iy;
                    pwpp_match_unpack(cells[(size_t)f * per_frame + i], ix, iy);
                    if (pwpp_match_landing<RECIP>(c.G, cand, ix, iy, jx, jy))
                        lo_x = std::min(lo_x, jx), hi_x = std::max(hi_x, jx), lo_y = std::min(lo_y, jy), hi_y = std::max(hi_y, jy);
                }
                const bool some_x = pwpp_match_window(lo_x, hi_x, c.wx, c.G.NX, fx, wn), some_y = pwpp_match_window(lo_y, hi_y, c.wy, c.G.NY, fy, hn);
                any = some_x && some_y;
                if (any && wn * hn <= stage_cap) {
                    stage.resize((size_t)wn * hn);
                    for (int i = 0; i < wn * hn; ++i) stage[i] = m[(size_t)(fy + i / wn) * c.G.NX + (size_t)(fx + i % wn)];
                    src = stage.data(), ox = fx, oy = fy, SX = wn, SY = hn, ++staged_windows;
                } else if (any) ++unstaged_windows;
            }
            for (int c0 = 0; any && c0 < count[f]; c0 += PWPP_MATCH_CHUNK) {
                const int here = std::min(count[f] - c0, PWPP_MATCH_CHUNK);
                for (int lane = 0; lane < PWPP_MATCH_CHUNK; ++lane) {
                    Jx[lane] = Jy[lane] = PWPP_MATCH_NOWHERE;
                    if (lane >= here) continue;
                    int ix, iy;
                    pwpp_match_unpack(cells[(size_t)f * per_frame + c0 + lane], ix, iy);
                    pwpp_match_landing<RECIP>(c.G, cand, ix, iy, Jx[lane], Jy[lane]);
                    Jx[lane] -= ox, Jy[lane] -= oy;
                }
                for (int lane = 0; lane < PWPP_MATCH_TILE; ++lane) {
                    const int s = tile * PWPP_MATCH_TILE + lane;
                    if (s >= shifts) continue;
                    const int sy = s / W - c.wy, sx = s % W - c.wx;
                    int32_t part = 0;
                    for (int j = 0; j < here; ++j) part += pwpp_match_contribution(src, Jx[j], Jy[j], sx, sy, SX, SY);
                    sum[lane] += part;
                }
            }
        }
        PwppMatchKey top{INT64_MIN, INT32_MAX, 0, 0, 0};
        for (int lane = PWPP_MATCH_TILE - 1; lane >= 0; --lane) {  // (any order: the key order is total)
            const int s = tile * PWPP_MATCH_TILE + lane;
            if (s >= shifts) continue;
            R.scores[(size_t)fr * shifts + s] = sum[lane];
            const PwppMatchKey key{sum[lane], r, s % W - c.wx, s / W - c.wy, 0};
            if (pwpp_match_better(key, top)) top = key;
        }
        partial[b] = top;
    }
    // k_match_best
    for (int f = 0; f < c.frames; ++f) {
        PwppMatchKey top{INT64_MIN, INT32_MAX, 0, 0, 0};
        for (int i = 0; i < c.n_candidates * tiles; ++i)
            if (pwpp_match_better(partial[(size_t)f * c.n_candidates * tiles + i], top)) top = partial[(size_t)f * c.n_candidates * tiles + i];
        R.best[f] = c.map_of_frame[f] < 0 ? PwppMatchKey{0, -1, 0, 0, count[f]} : PwppMatchKey{top.score, top.candidate, top.sx, top.sy, count[f]};
    }
    return R;
}

}  // namespace

int main() {
    std::mt19937_64 rng(20261019);
    const auto uni = [&](int lo, int hi) { return (int)(lo + (long long)(rng() % (unsigned long long)(hi - lo + 1))); };
    const auto real = [&](double lo, double hi) { return lo + (hi - lo) * (double)(rng() >> 11) / 9007199254740992.0; };
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    long long cases = 0, mismatches = 0;
    for (int t = 0; t < 2500; ++t) {
        Case c;
        const double map_cells[4] = {0.5, 0.5, 0.3, 0.25}, frame_cells[3] = {0.5, 0.25, 1.0};
        c.G.cell = frame_cells[uni(0, 2)], c.G.CELL = map_cells[uni(0, 3)];
        const bool recip = pwpp_fuse_reciprocal(c.G.CELL, c.G.inv_CELL);  // (0.3: the division alone)
        if (recip != (c.G.CELL != 0.3)) ++mismatches;
        const bool big = t % 50 == 0;  // more cells than a chunk
        c.G.nx = big ? uni(17, 24) : uni(1, 12), c.G.ny = big ? uni(17, 24) : uni(1, 12), c.G.NX = uni(1, 24), c.G.NY = uni(1, 24);
        c.G.x0 = -0.5 * c.G.cell * c.G.nx, c.G.y0 = -0.5 * c.G.cell * c.G.ny;
        c.G.X0 = -0.5 * c.G.CELL * c.G.NX + uni(-2, 2) * c.G.CELL, c.G.Y0 = -0.5 * c.G.CELL * c.G.NY;
        c.frames = uni(1, 3), c.n_maps = uni(1, 3), c.n_candidates = uni(1, 4);
        c.n_sets = uni(0, 1) ? 1 : c.frames;
        const bool wide = t % 100 == 1;  // more shifts than a tile
        c.wx = wide ? 8 : uni(0, 3), c.wy = wide ? 8 : uni(0, 3);
        c.occupancy.resize((size_t)c.frames * c.G.nx * c.G.ny);
        const int fill = big ? 1 : uni(0, 3);
        for (int8_t &b : c.occupancy) {
            const int r = uni(0, 99);
            b = fill == 0 ? -1 : (fill == 1 ? 100 : (r < 2 ? 50 : (r < 40 ? 0 : (r < 75 ? 100 : -1))));
        }
        for (int i = 0; i < c.n_sets * c.n_candidates; ++i) {
            double p[6] = {1, 0, 0, 0, 1, 0};
            const int kind = uni(0, 8);
            if (kind == 1) p[2] = uni(-6, 6) * c.G.CELL, p[5] = uni(-6, 6) * c.G.CELL;
            if (kind == 2) p[0] = 0, p[1] = -1, p[3] = 1, p[4] = 0;
            if (kind == 3) p[0] = -1;  // a mirror
            if (kind == 4 || kind == 5) {
                const double th = real(-3.2, 3.2);
                p[0] = std::cos(th), p[1] = -std::sin(th), p[3] = std::sin(th), p[4] = std::cos(th), p[2] = real(-4, 4), p[5] = real(-4, 4);
            }
            if (kind == 6) p[2] = uni(0, 1) ? 1e6 : 1e300;         // wholly outside: beyond the map, beyond the reach
            if (kind == 7) p[uni(0, 5)] = uni(0, 1) ? nan : inf;    // not finite: lands nowhere
            if (kind == 8) p[2] = 0.5 * c.G.CELL * c.G.NX;          // half outside
            c.candidates.insert(c.candidates.end(), p, p + 6);
        }
        for (int f = 0; f < c.frames; ++f) c.map_of_frame.push_back(uni(-1, c.n_maps - 1));
        c.map.resize((size_t)c.n_maps * c.G.NX * c.G.NY);
        const int values = uni(0, 3);
        for (int16_t &l : c.map) l = (int16_t)(values == 0 ? 7 : (uni(0, 9) == 0 ? (uni(0, 1) ? 32767 : -32768) : uni(-32768, 32767)));  // (a constant map: ties)
        const Result want = brute_force(c);
        ++cases, mismatches += !(as_the_kernels<false>(c) == want);
        if (recip) ++cases, mismatches += !(as_the_kernels<true>(c) == want);
        const int cap = t % 3 == 0 ? 1 << 20 : (t % 3 == 1 ? 40 : 150);  // every rectangle staged; few; some
        ++cases, mismatches += !(as_the_kernels<false>(c, cap) == want);
        if (recip) ++cases, mismatches += !(as_the_kernels<true>(c, cap) == want);
    }
    // the order of the argmax on equal scores: the smaller d2, then the candidate, then sy, then sx
    {
        const PwppMatchKey a{5, 1, 0, 0, 0}, b{5, 0, 1, 0, 0}, c{5, 0, 0, -1, 0}, d{5, 0, -1, 0, 0}, e{6, 9, 3, 3, 0}, f{5, 0, 0, 1, 0};
        ++cases, mismatches += !pwpp_match_better(a, b) || pwpp_match_better(b, a);  // d2 before the candidate
        ++cases, mismatches += !pwpp_match_better(c, b) || !pwpp_match_better(c, d) || !pwpp_match_better(c, f);  // sy before sx; the smaller sy
        ++cases, mismatches += !pwpp_match_better(d, b);                              // the smaller sx
        ++cases, mismatches += !pwpp_match_better(e, a) || pwpp_match_better(a, a);   // the score first; irreflexive
    }
    // the shifted pose: one product and one sum
    {
        const double cand[6] = {0.1, 0.2, 0.3, 0.4, 0.5, 0.7};
        double out[6];
        pwpp_match_shifted_pose(cand, 0.3, 7, -3, out);
        const double px = 7.0 * 0.3, py = -3.0 * 0.3;
        ++cases, mismatches += out[2] != 0.3 + px || out[5] != 0.7 + py || out[0] != 0.1 || out[1] != 0.2 || out[3] != 0.4 || out[4] != 0.5;
    }
    ++cases, mismatches += staged_windows < 1000 || unstaged_windows < 1000;
    // the window along one axis: cut to the map, empty where the landings are out of reach or there are none
    {
        int32_t first = -1, n = -1;
        ++cases, mismatches += !pwpp_match_window(3, 5, 2, 10, first, n) || first != 1 || n != 7;
        ++cases, mismatches += !pwpp_match_window(-4, 20, 3, 10, first, n) || first != 0 || n != 10;
        ++cases, mismatches += pwpp_match_window(-9, -4, 3, 10, first, n) || n != 0;
        ++cases, mismatches += !pwpp_match_window(-9, -4, 4, 10, first, n) || first != 0 || n != 1;
        ++cases, mismatches += pwpp_match_window(14, 30, 4, 10, first, n) || !pwpp_match_window(13, 30, 4, 10, first, n) || first != 9 || n != 1;
        ++cases, mismatches += pwpp_match_window(INT32_MAX, INT32_MIN, 64, 10, first, n);
        ++cases, mismatches += !pwpp_match_window(-1048576, 1048575, 64, 32768, first, n) || first != 0 || n != 32768;
    }
    // the packed word at the largest sides
    {
        int ix = 0, iy = 0;
        pwpp_match_unpack(pwpp_match_pack(32767, 32767), ix, iy);
        ++cases, mismatches += ix != 32767 || iy != 32767;
        pwpp_match_unpack(pwpp_match_pack(5, 0), ix, iy);
        ++cases, mismatches += ix != 5 || iy != 0;
    }
    std::printf("match_check: %lld cases, %lld mismatches\n", cases, mismatches);
    return mismatches == 0 ? 0 : 1;
}
