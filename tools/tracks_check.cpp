// tracks_check.cpp -- the functions of csrc/pwpp_tracks.h on the host, dealt as the kernels of csrc/pwpp_tracks.hip deal them: a lane
// per cell index in waves of 64, equal keys of a wave combined before they reach the frame's open-addressed table, the workgroups
// in a shuffled order (the result may not depend on it), a pass over the slots for the packed argmax, the rows in runs of 256 with
// the fresh ranks from a running prefix count -- against a brute force of its own: the gate by sorting every candidate cell, the
// pairs in a std::map, the links by scanning it.  Random label images, grids of different sides and cell sizes (powers of two and
// not: both forms of the quotient), every kind of pose (identity, shifts, quarter turns, yaw, non-finite), every gate, labels
// outside the rows, max_pairs below, at and above the number of pairs, ids with negative entries and a counter at the wrap.
// Also: the gate's key is a total order over the window, the packed key orders as the contract says, the table-size bound.
//   tracks_check                 runs the cases; prints "tracks_check: N cases, M mismatches"; exit status 1 on a mismatch
//   tracks_check dump ...        evaluates files for tests/test_tracks_cpu.py to compare with tests/tracks_ref.py (usage below)
// Built with -fsanitize=address,undefined by the test.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "pwpp_tracks.h"

static long g_cases = 0, g_bad = 0;
static void expect(bool ok, const char *what) {
    if (!ok && g_bad++ < 20) std::printf("MISMATCH: %s\n", what);
}

struct Problem {
    PwppFusionGeometry G;
    PwppTracksRule R;
    int frames = 0, n_poses = 0;
    std::vector<int32_t> curr, prev;  // [frames][NY][NX], [frames][ny][nx]
    std::vector<double> poses;
    std::vector<int32_t> id_prev, next_id;  // with R.with_ids
};
struct Result {
    std::vector<PwppClusterLink> curr_links, prev_links;
    std::vector<int32_t> n_pairs, id_curr, next_id_out;
};
static bool same(const PwppClusterLink &a, const PwppClusterLink &b) { return a.other == b.other && a.overlap == b.overlap && a.cells == b.cells && a.links == b.links; }

// ---- as the kernels deal it ------------------------------------------------------------------------------------------------
template <bool RECIP>
static Result dealt(const Problem &P, std::mt19937 &rng) {
    const size_t rows = (size_t)P.R.max_rows, slots = P.R.slots, cells_c = (size_t)P.G.NX * P.G.NY, cells_p = (size_t)P.G.nx * P.G.ny;
    Result out;
    out.curr_links.assign(P.frames * rows, PwppClusterLink{0, 0, 0, 0}), out.prev_links = out.curr_links;
    out.n_pairs.assign(P.frames, 0);
    std::vector<uint64_t> keys(P.frames * slots, PWPP_TRACKS_EMPTY), best_curr(P.frames * rows, 0), best_prev(P.frames * rows, 0);
    std::vector<uint32_t> counts(P.frames * slots, 0), distinct(P.frames, 0);
    const size_t per_frame = (std::max(cells_c, cells_p) + 255) / 256;
    std::vector<size_t> blocks(per_frame * P.frames);
    for (size_t i = 0; i < blocks.size(); ++i) blocks[i] = i;
    std::shuffle(blocks.begin(), blocks.end(), rng);
    // the lanes of a wave with one key become one: (key, lanes) in the order of their first lanes
    auto combine = [](const uint64_t key[64], const bool valid[64], std::vector<std::pair<uint64_t, uint32_t>> &groups) {
        groups.clear();
        for (int l = 0; l < 64; ++l) {
            if (!valid[l]) continue;
            auto it = std::find_if(groups.begin(), groups.end(), [&](const std::pair<uint64_t, uint32_t> &g) { return g.first == key[l]; });
            if (it == groups.end()) groups.emplace_back(key[l], 1u);
            else ++it->second;
        }
    };
    std::vector<std::pair<uint64_t, uint32_t>> groups;
    for (size_t block : blocks) {
        const size_t f = block / per_frame, run = block % per_frame;
        const int32_t *prev_f = P.prev.data() + f * cells_p;
        PwppClusterLink *curr_rows = out.curr_links.data() + f * rows, *prev_rows = out.prev_links.data() + f * rows;
        for (int wave = 0; wave < 4; ++wave) {
            uint64_t key[64];
            bool valid[64];
            int32_t b_of[64];
            for (int l = 0; l < 64; ++l) {
                const size_t i = run * 256 + wave * 64 + l;
                const int32_t a = i < cells_p ? prev_f[i] : -1;
                valid[l] = pwpp_tracks_row(a, P.R.max_rows), key[l] = (uint32_t)a;
            }
            combine(key, valid, groups);
            for (auto &g : groups) prev_rows[(int32_t)g.first].cells += (int32_t)g.second;
            for (int l = 0; l < 64; ++l) {
                const size_t i = run * 256 + wave * 64 + l;
                b_of[l] = i < cells_c ? P.curr[f * cells_c + i] : -1;
                valid[l] = pwpp_tracks_row(b_of[l], P.R.max_rows), key[l] = (uint32_t)b_of[l];
            }
            combine(key, valid, groups);
            for (auto &g : groups) curr_rows[(int32_t)g.first].cells += (int32_t)g.second;
            for (int l = 0; l < 64; ++l) {
                const size_t i = run * 256 + wave * 64 + l;
                int32_t a = -1;
                if (valid[l]) {
                    const int jy = (int)(i / (size_t)P.G.NX), jx = (int)(i - (size_t)jy * P.G.NX);
                    a = pwpp_tracks_vote<RECIP>(P.G, P.poses.data() + (P.n_poses == 1 ? 0 : f * 6), jx, jy, prev_f, P.R.gate, P.R.max_rows);
                }
                key[l] = pwpp_tracks_pair(b_of[l], a), valid[l] = a >= 0;
            }
            combine(key, valid, groups);
            for (auto &g : groups) {
                uint32_t s = pwpp_tracks_hash(g.first, P.R.slots);
                for (uint32_t probe = 0; probe < P.R.slots; ++probe) {
                    uint64_t &held = keys[f * slots + s];
                    if (held == PWPP_TRACKS_EMPTY) {
                        held = g.first, ++distinct[f];
                        ++curr_rows[pwpp_tracks_pair_curr(g.first)].links, ++prev_rows[pwpp_tracks_pair_prev(g.first)].links;
                    }
                    if (held == g.first) {
                        counts[f * slots + s] += g.second;
                        break;
                    }
                    s = s + 1 == P.R.slots ? 0 : s + 1;
                }
            }
        }
    }
    for (size_t i = 0; i < keys.size(); ++i) {
        if (keys[i] == PWPP_TRACKS_EMPTY) continue;
        const size_t f = i / slots;
        const int32_t b = pwpp_tracks_pair_curr(keys[i]), a = pwpp_tracks_pair_prev(keys[i]);
        best_curr[f * rows + b] = std::max(best_curr[f * rows + b], pwpp_tracks_pack(counts[i], a));
        best_prev[f * rows + a] = std::max(best_prev[f * rows + a], pwpp_tracks_pack(counts[i], b));
    }
    if (P.R.with_ids) out.id_curr.assign(P.frames * rows, -7), out.next_id_out.assign(P.frames, -7);
    for (int f = 0; f < P.frames; ++f) {
        const bool over = pwpp_tracks_overflowed(distinct[f], P.R.max_pairs);
        PwppClusterLink *curr_rows = out.curr_links.data() + f * rows, *prev_rows = out.prev_links.data() + f * rows;
        const uint64_t *bc = best_curr.data() + f * rows, *bp = best_prev.data() + f * rows;
        uint32_t fresh_below = 0;
        for (size_t r0 = 0; r0 < rows; r0 += 256) {
            bool fresh[256] = {false};
            int32_t id[256];
            for (size_t t = 0; t < 256 && r0 + t < rows; ++t) {
                const size_t r = r0 + t;
                const PwppClusterLink c = pwpp_tracks_link(curr_rows[r].cells, curr_rows[r].links, bc[r], over);
                curr_rows[r] = c, prev_rows[r] = pwpp_tracks_link(prev_rows[r].cells, prev_rows[r].links, bp[r], over);
                id[t] = -1;
                if (c.cells > 0 && P.R.with_ids) {
                    fresh[t] = true;
                    if (c.other >= 0 && c.other < P.R.max_rows) {
                        const int32_t ip = P.id_prev[f * rows + c.other];
                        if (pwpp_tracks_continues(c, (int32_t)r, pwpp_tracks_link(0, 0, bp[c.other], over), ip, P.R.min_overlap)) fresh[t] = false, id[t] = ip;
                    }
                }
            }
            uint32_t k = fresh_below;
            for (size_t t = 0; t < 256 && r0 + t < rows; ++t) {
                if (P.R.with_ids) out.id_curr[f * rows + r0 + t] = fresh[t] ? pwpp_tracks_fresh_id(P.next_id[f], k) : id[t];
                k += fresh[t] ? 1u : 0u;
            }
            fresh_below = k;
        }
        out.n_pairs[f] = pwpp_tracks_n_pairs(distinct[f], P.R.max_pairs);
        if (P.R.with_ids) out.next_id_out[f] = pwpp_tracks_fresh_id(P.next_id[f], fresh_below);
    }
    return out;
}

// ---- the contract written out again ---------------------------------------------------------------------------------------------
static Result brute(const Problem &P) {
    const int rows = P.R.max_rows;
    const size_t cells_c = (size_t)P.G.NX * P.G.NY, cells_p = (size_t)P.G.nx * P.G.ny;
    Result out;
    out.curr_links.assign((size_t)P.frames * rows, PwppClusterLink{-1, 0, 0, 0}), out.prev_links = out.curr_links;
    out.n_pairs.assign(P.frames, 0);
    if (P.R.with_ids) out.id_curr.assign((size_t)P.frames * rows, -1), out.next_id_out.assign(P.frames, 0);
    for (int f = 0; f < P.frames; ++f) {
        const int32_t *curr = P.curr.data() + f * cells_c, *prev = P.prev.data() + f * cells_p;
        const double *pose = P.poses.data() + (P.n_poses == 1 ? 0 : (size_t)f * 6);
        PwppClusterLink *cl = out.curr_links.data() + (size_t)f * rows, *pl = out.prev_links.data() + (size_t)f * rows;
        std::map<std::pair<int, int>, int> n;  // (a, b)
        for (int jy = 0; jy < P.G.NY; ++jy)
            for (int jx = 0; jx < P.G.NX; ++jx) {
                const int32_t b = curr[(size_t)jy * P.G.NX + jx];
                if (b < 0 || b >= rows) continue;
                ++cl[b].cells;
                int px = 0, py = 0;  // (the geometry is the fusion's one text: pwpp_fusion.h has its own checker)
                if (!pwpp_fuse_cell_of<false>(P.G, pose, pwpp_elev_position(P.G.X0, jx, P.G.CELL), pwpp_elev_position(P.G.Y0, jy, P.G.CELL), px, py)) continue;
                std::vector<std::pair<std::pair<int, int>, int>> found;  // ((distance, index), row)
                for (int y = py - P.R.gate; y <= py + P.R.gate; ++y)
                    for (int x = px - P.R.gate; x <= px + P.R.gate; ++x) {
                        if (x < 0 || y < 0 || x >= P.G.nx || y >= P.G.ny) continue;
                        const int32_t l = prev[(size_t)y * P.G.nx + x];
                        if (l >= 0 && l < rows) found.push_back({{(x - px) * (x - px) + (y - py) * (y - py), y * P.G.nx + x}, l});
                    }
                if (found.empty()) continue;
                std::sort(found.begin(), found.end());
                ++n[{found[0].second, b}];
            }
        for (size_t i = 0; i < cells_p; ++i)
            if (prev[i] >= 0 && prev[i] < rows) ++pl[prev[i]].cells;
        const bool over = (long)n.size() > (long)P.R.max_pairs;
        out.n_pairs[f] = over ? P.R.max_pairs + 1 : (int32_t)n.size();
        for (int r = 0; r < rows; ++r) {
            if (over) {
                cl[r].other = pl[r].other = -2;
                continue;
            }
            for (auto &kv : n) {
                const int a = kv.first.first, b = kv.first.second, v = kv.second;
                if (b == r) {
                    ++cl[r].links;
                    if (v > cl[r].overlap || (v == cl[r].overlap && a < cl[r].other)) cl[r].overlap = v, cl[r].other = a;
                }
                if (a == r) {
                    ++pl[r].links;
                    if (v > pl[r].overlap || (v == pl[r].overlap && b < pl[r].other)) pl[r].overlap = v, pl[r].other = b;
                }
            }
        }
        if (!P.R.with_ids) continue;
        uint32_t fresh = 0;
        for (int b = 0; b < rows; ++b) {
            if (cl[b].cells <= 0) continue;
            const int a = cl[b].other;
            if (a >= 0 && pl[a].other == b && cl[b].overlap >= P.R.min_overlap && P.id_prev[(size_t)f * rows + a] >= 0) out.id_curr[(size_t)f * rows + b] = P.id_prev[(size_t)f * rows + a];
            else out.id_curr[(size_t)f * rows + b] = (int32_t)(((uint32_t)P.next_id[f] + fresh++) & 0x7fffffffu);
        }
        out.next_id_out[f] = (int32_t)(((uint32_t)P.next_id[f] + fresh) & 0x7fffffffu);
    }
    return out;
}

static bool agree(const Result &a, const Result &b) {
    if (a.curr_links.size() != b.curr_links.size() || a.n_pairs != b.n_pairs || a.id_curr != b.id_curr || a.next_id_out != b.next_id_out) return false;
    for (size_t i = 0; i < a.curr_links.size(); ++i)
        if (!same(a.curr_links[i], b.curr_links[i]) || !same(a.prev_links[i], b.prev_links[i])) return false;
    return true;
}

static void set_geometry(Problem &P, double X0, double Y0, double CELL, int NX, int NY, double x0, double y0, double cell, int nx, int ny) {
    P.G = PwppFusionGeometry{X0, Y0, CELL, x0, y0, cell, NX, NY, nx, ny, 0.0};
    pwpp_fuse_reciprocal(cell, P.G.inv_cell);
}

static void paint(std::vector<int32_t> &image, int frames, int nx, int ny, int rows, std::mt19937 &rng) {
    image.assign((size_t)frames * nx * ny, -1);
    const int kinds = (int)(rng() % 3);  // rectangles; every cell its own label; noise
    for (int f = 0; f < frames; ++f) {
        int32_t *im = image.data() + (size_t)f * nx * ny;
        if (kinds == 1) {
            for (int i = 0; i < nx * ny; ++i) im[i] = i;
        } else if (kinds == 2) {
            for (int i = 0; i < nx * ny; ++i) im[i] = (int32_t)(rng() % (unsigned)(rows + 3)) - 2;
        } else {
            for (int k = 0; k < 6; ++k) {
                const int x = (int)(rng() % nx), y = (int)(rng() % ny), w = 1 + (int)(rng() % (nx / 2 + 1)), h = 1 + (int)(rng() % (ny / 2 + 1));
                const int32_t l = (int32_t)(rng() % (unsigned)(rows + 2)) - 1;
                for (int yy = y; yy < std::min(ny, y + h); ++yy)
                    for (int xx = x; xx < std::min(nx, x + w); ++xx) im[(size_t)yy * nx + xx] = l;
            }
        }
        if (rng() % 4 == 0) im[rng() % (unsigned)(nx * ny)] = 0x7fffffff;
    }
}

static void random_case(std::mt19937 &rng) {
    Problem P;
    const int NX = 1 + (int)(rng() % 40), NY = 1 + (int)(rng() % 40), same_grid = (int)(rng() % 2);
    const int nx = same_grid ? NX : 1 + (int)(rng() % 40), ny = same_grid ? NY : 1 + (int)(rng() % 40);
    const double cells[4] = {0.5, 1.0, 0.3, 2.0};
    const double CELL = cells[rng() % 4], cell = same_grid ? CELL : cells[rng() % 4];
    set_geometry(P, -0.5 * NX * CELL, -0.5 * NY * CELL, CELL, NX, NY, same_grid ? -0.5 * NX * CELL : -0.5 * nx * cell, same_grid ? -0.5 * NY * CELL : -0.5 * ny * cell, cell, nx, ny);
    P.frames = 1 + (int)(rng() % 3), P.n_poses = rng() % 2 ? 1 : P.frames;
    const int rows = 1 + (int)(rng() % 12);
    for (int i = 0; i < P.n_poses; ++i) {
        const int kind = (int)(rng() % 6);
        const double deg = kind == 3 ? 30.0 * (double)(rng() % 12) : 0.0, co = cos(deg * M_PI / 180.0), si = sin(deg * M_PI / 180.0);
        double pose[6] = {1, 0, 0, 0, 1, 0};
        if (kind == 1) pose[2] = CELL * (double)((int)(rng() % 7) - 3), pose[5] = CELL * (double)((int)(rng() % 7) - 3);
        if (kind == 2) pose[0] = 0, pose[1] = -1, pose[3] = 1, pose[4] = 0;
        if (kind == 3) pose[0] = co, pose[1] = -si, pose[3] = si, pose[4] = co, pose[2] = 0.37, pose[5] = -0.21;
        if (kind == 4) pose[rng() % 6] = rng() % 2 ? NAN : INFINITY;
        if (kind == 5) pose[2] = 1e6;
        P.poses.insert(P.poses.end(), pose, pose + 6);
    }
    paint(P.curr, P.frames, NX, NY, rows, rng), paint(P.prev, P.frames, nx, ny, rows, rng);
    P.R = PwppTracksRule{(int32_t)(rng() % 5), 1 + (int32_t)(rng() % 4), rows, 1, 0, (int32_t)(rng() % 2)};
    if (P.R.with_ids) {
        for (int i = 0; i < P.frames * rows; ++i) P.id_prev.push_back(rng() % 5 == 0 ? -1 : 100 + i);
        for (int f = 0; f < P.frames; ++f) P.next_id.push_back(rng() % 3 == 0 ? 0x7ffffffe : (int32_t)(rng() % 1000));
    }
    P.R.max_pairs = 4096, P.R.slots = pwpp_tracks_slots(4096);  // (more than rows^2: every pair is counted)
    const Result want_all = brute(P);
    int most = 1;
    for (int32_t v : want_all.n_pairs) most = std::max(most, (int)v);
    const int choices[4] = {most, std::max(1, most - 1), 2 * most, 1};
    for (int c = 0; c < 4; ++c) {
        P.R.max_pairs = choices[c], P.R.slots = pwpp_tracks_slots(choices[c]);
        const Result want = brute(P);
        const Result a = dealt<false>(P, rng), b = P.G.inv_cell != 0.0 ? dealt<true>(P, rng) : dealt<false>(P, rng);
        ++g_cases;
        if (!agree(a, want) || !agree(b, want)) {
            expect(false, "the dealt functions and the brute force differ");
            std::printf("  %d x %d on %d x %d, %d frames, gate %d, rows %d, max_pairs %d, ids %d\n", NX, NY, nx, ny, P.frames, P.R.gate, rows, P.R.max_pairs, P.R.with_ids);
        }
    }
}

static void fixed_properties() {
    // the gate's key: distinct over the window, ordered by distance first
    for (int gate = 0; gate <= PWPP_TRACKS_MAX_GATE; ++gate) {
        std::vector<uint64_t> keys;
        for (int ey = -gate; ey <= gate; ++ey)
            for (int ex = -gate; ex <= gate; ++ex) keys.push_back(pwpp_tracks_gate_key(ex, ey, (10 + ey) * 32768 + 10 + ex));
        std::sort(keys.begin(), keys.end());
        expect(std::adjacent_find(keys.begin(), keys.end()) == keys.end(), "two cells of a window share a gate key");
        expect(keys[0] == pwpp_tracks_gate_key(0, 0, 10 * 32768 + 10), "the cell itself is not the smallest gate key");
        ++g_cases;
    }
    expect(pwpp_tracks_gate_key(1, 0, 0x3fffffff) < pwpp_tracks_gate_key(1, 1, 0), "a nearer cell with a larger index loses");
    expect(pwpp_tracks_gate_key(-1, 0, 5) < pwpp_tracks_gate_key(1, 0, 7), "equal distances: the smaller index loses");
    // the packed argmax: the larger overlap, then the smaller label; 0 is below every pair
    expect(pwpp_tracks_pack(2, 16777215) > pwpp_tracks_pack(1, 0), "a larger overlap loses");
    expect(pwpp_tracks_pack(5, 3) > pwpp_tracks_pack(5, 4), "on a tie the smaller label loses");
    expect(pwpp_tracks_pack(1, 16777215) > 0, "a pair packs to 0");
    expect(pwpp_tracks_best_label(pwpp_tracks_pack(9, 1234)) == 1234 && pwpp_tracks_best_overlap(pwpp_tracks_pack(9, 1234)) == 9, "a packed key does not unpack");
    expect(pwpp_tracks_best_label(0) == -1 && pwpp_tracks_best_overlap(0) == 0, "no pair does not unpack to -1, 0");
    expect(pwpp_tracks_best_overlap(pwpp_tracks_pack(1u << 30, 0)) == (1 << 30), "the largest overlap, 2^30 cells, does not fit");
    // the table: at least max_pairs + 1 slots, so distinct passes max_pairs before an insertion can fail
    for (int32_t m : {1, 2, 3, 1000, 16777216}) {
        expect(pwpp_tracks_slots(m) >= (uint32_t)m + 1 && pwpp_tracks_slots(m) == 2u * (uint32_t)m, "the table-size bound");
        expect(pwpp_tracks_n_pairs((uint32_t)m, m) == m && pwpp_tracks_n_pairs((uint32_t)m + 1, m) == m + 1 && pwpp_tracks_n_pairs(2u * (uint32_t)m, m) == m + 1, "n_pairs");
        for (uint64_t k : {(uint64_t)0, pwpp_tracks_pair(16777215, 16777215), pwpp_tracks_pair(1, 2)}) expect(pwpp_tracks_hash(k, pwpp_tracks_slots(m)) < pwpp_tracks_slots(m), "a hash outside the table");
        ++g_cases;
    }
    expect(pwpp_tracks_pair(16777215, 16777215) != PWPP_TRACKS_EMPTY, "a pair is the empty slot");
    expect(pwpp_tracks_pair_curr(pwpp_tracks_pair(7, 9)) == 7 && pwpp_tracks_pair_prev(pwpp_tracks_pair(7, 9)) == 9, "a pair does not unpack");
    expect(pwpp_tracks_fresh_id(0x7ffffff0, 0x10) == 0 && pwpp_tracks_fresh_id(0x7fffffff, 0) == 0x7fffffff && pwpp_tracks_fresh_id(-1, 2) == 1, "the id wrap");
}

// ---- dump: files in, files out ---------------------------------------------------------------------------------------------------
template <class T>
static bool read_file(const char *path, std::vector<T> &v, size_t n) {
    v.assign(n, T());
    FILE *f = std::fopen(path, "rb");
    const size_t got = f ? std::fread(v.data(), sizeof(T), n, f) : 0;
    if (f) std::fclose(f);
    if (got != n) std::fprintf(stderr, "tracks_check: cannot read %zu elements from %s\n", n, path);
    return got == n;
}
template <class T>
static bool write_file(const std::string &path, const std::vector<T> &v) {
    FILE *f = std::fopen(path.c_str(), "wb");
    const size_t put = f ? std::fwrite(v.data(), sizeof(T), v.size(), f) : 0;
    if (f) std::fclose(f);
    return put == v.size();
}

// curr.i32 prev.i32 poses.f64 n_poses frames X0 Y0 CELL NX NY x0 y0 cell nx ny gate min_overlap max_rows max_pairs ids.i32|- out
static int dump(char **a) {
    Problem P;
    P.n_poses = std::atoi(a[3]), P.frames = std::atoi(a[4]);
    set_geometry(P, std::atof(a[5]), std::atof(a[6]), std::atof(a[7]), std::atoi(a[8]), std::atoi(a[9]), std::atof(a[10]), std::atof(a[11]), std::atof(a[12]),
                 std::atoi(a[13]), std::atoi(a[14]));
    P.R = PwppTracksRule{std::atoi(a[15]), std::atoi(a[16]), std::atoi(a[17]), std::atoi(a[18]), 0, std::strcmp(a[19], "-") != 0};
    if (P.frames < 1 || P.R.max_rows < 1 || P.R.max_pairs < 1 || P.G.NX < 1 || P.G.NY < 1 || P.G.nx < 1 || P.G.ny < 1 || (P.n_poses != 1 && P.n_poses != P.frames)) return 2;
    P.R.slots = pwpp_tracks_slots(P.R.max_pairs);
    const size_t rows = (size_t)P.frames * P.R.max_rows;
    if (!read_file(a[0], P.curr, (size_t)P.frames * P.G.NX * P.G.NY) || !read_file(a[1], P.prev, (size_t)P.frames * P.G.nx * P.G.ny) ||
        !read_file(a[2], P.poses, (size_t)P.n_poses * 6))
        return 2;
    if (P.R.with_ids) {
        std::vector<int32_t> ids;
        if (!read_file(a[19], ids, rows + P.frames)) return 2;
        P.id_prev.assign(ids.begin(), ids.begin() + rows), P.next_id.assign(ids.begin() + rows, ids.end());
    }
    std::mt19937 rng(1);
    const Result r = P.G.inv_cell != 0.0 ? dealt<true>(P, rng) : dealt<false>(P, rng);
    const std::string out = a[20];
    std::vector<int32_t> cl, pl;
    for (const PwppClusterLink &l : r.curr_links) cl.insert(cl.end(), {l.other, l.overlap, l.cells, l.links});
    for (const PwppClusterLink &l : r.prev_links) pl.insert(pl.end(), {l.other, l.overlap, l.cells, l.links});
    bool ok = write_file(out + ".curr_links", cl) && write_file(out + ".prev_links", pl) && write_file(out + ".n_pairs", r.n_pairs);
    if (P.R.with_ids) ok = ok && write_file(out + ".id_curr", r.id_curr) && write_file(out + ".next_id_out", r.next_id_out);
    return ok ? 0 : 2;
}

int main(int argc, char **argv) {
    if (argc == 23 && std::strcmp(argv[1], "dump") == 0) return dump(argv + 2);
    if (argc != 1) {
        std::fprintf(stderr, "usage: tracks_check | tracks_check dump curr.i32 prev.i32 poses.f64 n_poses frames X0 Y0 CELL NX NY x0 y0 cell nx ny gate min_overlap "
                             "max_rows max_pairs ids.i32|- out\n");
        return 2;
    }
    fixed_properties();
    std::mt19937 rng(20261020);
    for (int i = 0; i < 600; ++i) random_case(rng);
    std::printf("tracks_check: %ld cases, %ld mismatches\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
