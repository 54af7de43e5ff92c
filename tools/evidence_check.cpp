// evidence_check.cpp -- the functions of csrc/pwpp_evidence.h on the host, dealt as the kernels of csrc/pwpp_evidence.hip deal them: a
// lane per cell in waves of 64, the lanes of a wave with one row combined before their counters are added, the workgroups in a
// shuffled order (the result may not depend on it); path 1 adds to the output rows, path 2 to a table per run of 2048 cells that
// is flushed, its rows in a shuffled order, where a counter is not zero -- against a brute force of its own: the landing written out
// again with the quotient as written, the window's values collected and their maximum taken, the rows in a std::map, the verdict by
// cross-multiplication in __int128.  Random label images (rectangles, noise, labels outside the rows), grids and maps of different
// sides and cell sizes (powers of two and not: both forms of the quotient), every kind of pose (identity, shifts, quarter turns,
// yaw, non-finite, far away), every gate, maps with values at the thresholds and at the ends of int16, skipped frames, shared maps
// and a map per frame.  Also: the verdict at exact ratio boundaries and the range checks of the rule.
//   evidence_check               runs the cases; prints "evidence_check: N cases, M mismatches"; exit status 1 on a mismatch
//   evidence_check dump ...      evaluates files for tests/test_evidence_cpu.py to compare with tests/evidence_ref.py (usage below)
// Built with -fsanitize=address,undefined by the test.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "pwpp_evidence.h"

static long g_cases = 0, g_bad = 0;
static void expect(bool ok, const char *what) {
    if (!ok && g_bad++ < 20) std::printf("MISMATCH: %s\n", what);
}

struct Problem {
    PwppMatchGeometry G;
    PwppEvidenceRule R;
    int32_t occupied_at = 0, free_at = 0, max_rows = 1;
    int frames = 0, n_poses = 0, n_maps = 0;
    std::vector<int32_t> label;   // [frames][ny][nx]
    std::vector<int8_t> occ_in;   // the same shape, or empty: no masked bytes
    std::vector<double> poses;    // [n_poses][6]
    std::vector<int32_t> map_of;  // [frames], resolved
    std::vector<int16_t> maps;    // [n_maps][NY][NX]
};
struct Result {
    std::vector<PwppClusterEvidence> rows;
    std::vector<int8_t> cell_class, occ_out;
};
static bool same(const PwppClusterEvidence &a, const PwppClusterEvidence &b) {
    return a.sum == b.sum && a.cells == b.cells && a.landed == b.landed && a.occupied == b.occupied && a.free == b.free && a.unknown == b.unknown && a.verdict == b.verdict;
}

// ---- as the kernels deal it ------------------------------------------------------------------------------------------------
struct Lane {
    int32_t row = -1, E = 0;
    bool is_row = false, landed = false, occupied = false, free_ = false;
};
struct Group {
    int32_t row, cells, landed, occupied, free_;
    int64_t sum;
};

template <bool RECIP>
static Result dealt(const Problem &P, int path, std::mt19937 &rng) {
    const size_t rows = (size_t)P.max_rows, cells = (size_t)P.G.nx * P.G.ny, map_cells = (size_t)P.G.NX * P.G.NY;
    Result out;
    out.rows.assign(P.frames * rows, PwppClusterEvidence{0, 0, 0, 0, 0, 0, 0});
    const bool lds = path == 2 && P.max_rows <= PWPP_EV_LDS_ROWS;
    const size_t per_block = lds ? 2048 : 256, per_frame = (cells + per_block - 1) / per_block;
    std::vector<size_t> blocks(per_frame * P.frames);
    for (size_t i = 0; i < blocks.size(); ++i) blocks[i] = i;
    std::shuffle(blocks.begin(), blocks.end(), rng);
    auto lane_of = [&](size_t f, size_t i) {
        Lane L;
        if (i >= cells) return L;
        L.row = P.label[f * cells + i];
        L.is_row = pwpp_evid_row(L.row, P.max_rows);
        const int32_t k = P.map_of[f];
        if (!L.is_row || k < 0) return L;
        const int iy = (int)(i / (size_t)P.G.nx), ix = (int)(i % (size_t)P.G.nx);
        int32_t Jx = 0, Jy = 0;
        if (!pwpp_evid_landed<RECIP>(P.G, P.poses.data() + (P.n_poses == 1 ? 0 : f * 6), ix, iy, Jx, Jy)) return L;
        L.landed = true;
        L.E = pwpp_evid_read(P.maps.data() + (size_t)k * map_cells, Jx, Jy, P.R.gate, P.G.NX, P.G.NY);
        const int8_t cls = pwpp_evid_class(L.E, P.occupied_at, P.free_at);
        L.occupied = cls == PWPP_FUSE_OCCUPIED, L.free_ = cls == PWPP_FUSE_FREE;
        return L;
    };
    // the lanes of a wave with one row become one group, in the order of their first lanes
    auto wave_groups = [](const Lane w[64], std::vector<Group> &groups) {
        groups.clear();
        for (int l = 0; l < 64; ++l) {
            if (!w[l].is_row) continue;
            auto it = std::find_if(groups.begin(), groups.end(), [&](const Group &g) { return g.row == w[l].row; });
            if (it == groups.end()) groups.push_back(Group{w[l].row, 0, 0, 0, 0, 0}), it = groups.end() - 1;
            it->cells += 1, it->landed += w[l].landed, it->occupied += w[l].occupied, it->free_ += w[l].free_, it->sum += w[l].landed ? w[l].E : 0;
        }
    };
    auto row_add = [](PwppClusterEvidence &r, int32_t cells_, int32_t landed, int32_t occupied, int32_t free_, int64_t sum) {
        r.cells += cells_, r.landed += landed, r.occupied += occupied, r.free += free_, r.sum += sum;
    };
    std::vector<Group> groups;
    std::vector<PwppClusterEvidence> table;
    std::vector<size_t> order;
    for (const size_t block : blocks) {
        const size_t f = block / per_frame, run = block % per_frame;
        if (lds) table.assign(rows, PwppClusterEvidence{0, 0, 0, 0, 0, 0, 0});
        for (size_t wave = 0; wave < per_block / 64; ++wave) {
            Lane w[64];
            for (int l = 0; l < 64; ++l) w[l] = lane_of(f, run * per_block + wave * 64 + (size_t)l);
            wave_groups(w, groups);
            for (const Group &g : groups) row_add(lds ? table[(size_t)g.row] : out.rows[f * rows + (size_t)g.row], g.cells, g.landed, g.occupied, g.free_, g.sum);
        }
        if (!lds) continue;
        order.resize(rows);
        for (size_t r = 0; r < rows; ++r) order[r] = r;
        std::shuffle(order.begin(), order.end(), rng);
        for (const size_t r : order)
            if (table[r].cells != 0) row_add(out.rows[f * rows + r], table[r].cells, table[r].landed, table[r].occupied, table[r].free, table[r].sum);
    }
    for (PwppClusterEvidence &r : out.rows) r = pwpp_evid_finish(P.R, r.sum, r.cells, r.landed, r.occupied, r.free);
    out.cell_class.assign(P.frames * cells, 0);
    if (!P.occ_in.empty()) out.occ_out.assign(P.frames * cells, 0);
    for (size_t f = 0; f < (size_t)P.frames; ++f)
        for (size_t i = 0; i < cells; ++i) {
            const int32_t k = P.map_of[f], l = P.label[f * cells + i];
            out.cell_class[f * cells + i] = pwpp_evid_cell_class<RECIP>(P.G, P.poses.data() + (P.n_poses == 1 ? 0 : f * 6), (int)(i % (size_t)P.G.nx), (int)(i / (size_t)P.G.nx), l,
                                                                        P.max_rows, k < 0 ? nullptr : P.maps.data() + (size_t)k * map_cells, P.R.gate, P.occupied_at, P.free_at);
            if (!P.occ_in.empty()) out.occ_out[f * cells + i] = pwpp_evid_mask(l, P.max_rows, out.rows.data() + f * rows, P.occ_in[f * cells + i]);
        }
    return out;
}
static Result dealt(const Problem &P, int path, std::mt19937 &rng) { return P.G.inv_CELL != 0.0 ? dealt<true>(P, path, rng) : dealt<false>(P, path, rng); }

// ---- the brute force: the contract of include/pwpp.h written out again ---------------------------------------------------------
static int32_t brute_verdict(const PwppEvidenceRule &R, int64_t cells, int64_t landed, int64_t occupied, int64_t free_) {
    if (cells == 0) return -1;
    const bool enough = landed >= R.min_cells;
    if (enough && (__int128)free_ * 256 >= (__int128)R.moving_share * landed) return 2;
    if (enough && (__int128)occupied * 256 >= (__int128)R.static_share * landed) return 1;
    return 0;
}
static Result brute(const Problem &P) {
    const size_t rows = (size_t)P.max_rows, cells = (size_t)P.G.nx * P.G.ny, map_cells = (size_t)P.G.NX * P.G.NY;
    Result out;
    out.rows.assign(P.frames * rows, PwppClusterEvidence{0, 0, 0, 0, 0, 0, 0});
    out.cell_class.assign(P.frames * cells, (int8_t)-2);
    out.occ_out = P.occ_in;
    for (size_t f = 0; f < (size_t)P.frames; ++f) {
        std::map<int32_t, std::vector<int64_t>> acc;  // row -> {sum, cells, landed, occupied, free, unknown}
        const double *p = P.poses.data() + (P.n_poses == 1 ? 0 : f * 6);
        bool finite = true;
        for (int k = 0; k < 6; ++k) finite = finite && std::isfinite(p[k]);
        for (int iy = 0; iy < P.G.ny; ++iy)
            for (int ix = 0; ix < P.G.nx; ++ix) {
                const size_t at = f * cells + (size_t)iy * P.G.nx + ix;
                const int32_t l = P.label[at];
                if (l < 0 || l >= P.max_rows) continue;
                std::vector<int64_t> &a = acc[l];
                a.resize(6, 0);
                a[1] += 1;
                if (P.map_of[f] < 0 || !finite) continue;
                volatile double hx = (double)ix + 0.5, hy = (double)iy + 0.5;
                volatile double sx = hx * P.G.cell, sy = hy * P.G.cell;
                volatile double x = P.G.x0 + sx, y = P.G.y0 + sy;
                volatile double ax = p[0] * x, by = p[1] * y, cx = p[3] * x, dy = p[4] * y;
                volatile double rx = ax + by, ry = cx + dy;
                volatile double X = rx + p[2], Y = ry + p[5];
                volatile double nu = X - P.G.X0, nv = Y - P.G.Y0;
                const double U = nu / P.G.CELL, V = nv / P.G.CELL;
                if (!(U >= -1048576.0 && U < 1048576.0 && V >= -1048576.0 && V < 1048576.0)) continue;
                const long Jx = (long)std::floor(U), Jy = (long)std::floor(V);
                if (Jx < 0 || Jx >= P.G.NX || Jy < 0 || Jy >= P.G.NY) continue;
                std::vector<int16_t> window;
                for (long yy = Jy - P.R.gate; yy <= Jy + P.R.gate; ++yy)
                    for (long xx = Jx - P.R.gate; xx <= Jx + P.R.gate; ++xx)
                        if (xx >= 0 && xx < P.G.NX && yy >= 0 && yy < P.G.NY) window.push_back(P.maps[(size_t)P.map_of[f] * map_cells + (size_t)yy * P.G.NX + (size_t)xx]);
                const int64_t E = *std::max_element(window.begin(), window.end());
                const int8_t cls = E >= P.occupied_at ? 100 : (E <= P.free_at ? 0 : -1);
                a[0] += E, a[2] += 1, a[cls == 100 ? 3 : (cls == 0 ? 4 : 5)] += 1;
                out.cell_class[at] = cls;
            }
        for (const auto &kv : acc) {
            const std::vector<int64_t> &a = kv.second;
            out.rows[f * rows + (size_t)kv.first] =
                PwppClusterEvidence{a[0], (int32_t)a[1], (int32_t)a[2], (int32_t)a[3], (int32_t)a[4], (int32_t)a[5], brute_verdict(P.R, a[1], a[2], a[3], a[4])};
        }
        for (size_t r = 0; r < rows; ++r)
            if (!acc.count((int32_t)r)) out.rows[f * rows + r].verdict = -1;
        if (!P.occ_in.empty())
            for (size_t i = 0; i < cells; ++i) {
                const int32_t l = P.label[f * cells + i];
                if (l >= 0 && l < P.max_rows && out.rows[f * rows + (size_t)l].verdict == 2) out.occ_out[f * cells + i] = -1;
            }
    }
    return out;
}

static void compare(const Problem &P, const Result &a, const Result &b, const char *what) {
    bool ok = a.rows.size() == b.rows.size() && a.cell_class == b.cell_class && a.occ_out == b.occ_out;
    for (size_t i = 0; ok && i < a.rows.size(); ++i) ok = same(a.rows[i], b.rows[i]);
    for (size_t i = 0; ok && i < a.rows.size(); ++i) ok = a.rows[i].occupied + a.rows[i].free + a.rows[i].unknown == a.rows[i].landed && a.rows[i].landed <= a.rows[i].cells;
    (void)P;
    expect(ok, what);
}

// ---- random problems -------------------------------------------------------------------------------------------------------
static Problem random_problem(std::mt19937 &rng, int round) {
    auto uni = [&](int lo, int hi) { return (int)(rng() % (uint32_t)(hi - lo + 1)) + lo; };
    Problem P;
    const double cells[] = {0.5, 1.0, 0.3, 0.7, 2.0, 0.25};
    const bool big = round % 97 == 0;
    P.G.nx = big ? 70 : uni(1, 24), P.G.ny = big ? 61 : uni(1, 24), P.G.NX = uni(1, 30), P.G.NY = uni(1, 30);
    P.G.cell = cells[uni(0, 5)], P.G.CELL = cells[uni(0, 5)];
    P.G.x0 = -0.5 * P.G.nx * P.G.cell + 0.25 * uni(-3, 3), P.G.y0 = -0.5 * P.G.ny * P.G.cell + 0.25 * uni(-3, 3);
    P.G.X0 = -0.5 * P.G.NX * P.G.CELL + 0.25 * uni(-3, 3), P.G.Y0 = -0.5 * P.G.NY * P.G.CELL + 0.25 * uni(-3, 3);
    pwpp_fuse_reciprocal(P.G.CELL, P.G.inv_CELL);
    P.frames = uni(1, 3), P.n_poses = uni(0, 1) ? 1 : P.frames;
    const int row_choices[] = {1, 2, 5, 8, 64, 257, PWPP_EV_LDS_ROWS, PWPP_EV_LDS_ROWS + 1};
    P.max_rows = row_choices[uni(0, 7)];
    P.R = PwppEvidenceRule{uni(0, 4), uni(1, 6), uni(1, 256), uni(1, 256)};
    P.occupied_at = uni(-50, 200), P.free_at = P.occupied_at - uni(1, 150);
    const int map_mode = uni(0, 2);  // one shared map | one per frame | explicit with skips
    P.n_maps = map_mode == 0 ? 1 : (map_mode == 1 ? P.frames : uni(1, 3));
    for (int f = 0; f < P.frames; ++f) P.map_of.push_back(map_mode == 0 ? 0 : (map_mode == 1 ? f : uni(-1, P.n_maps - 1)));
    for (int k = 0; k < P.n_poses; ++k) {
        const int kind = uni(0, 7);
        double a = 1, b = 0, c = 0, d = 1, tx = 0.25 * uni(-8, 8), ty = 0.25 * uni(-8, 8);
        if (kind == 1) a = 0, b = -1, c = 1, d = 0;
        if (kind == 2 || kind == 3) {
            const double th = 0.01 * uni(-314, 314);
            a = std::cos(th), b = -std::sin(th), c = std::sin(th), d = std::cos(th);
        }
        if (kind == 4) tx = NAN;
        if (kind == 5) (uni(0, 1) ? a : ty) = INFINITY;
        if (kind == 6) tx = 1e9 * uni(-1, 1), ty = 3e5;
        const double pose[6] = {a, b, tx, c, d, ty};
        P.poses.insert(P.poses.end(), pose, pose + 6);
    }
    const size_t cells_f = (size_t)P.G.nx * P.G.ny, map_cells = (size_t)P.G.NX * P.G.NY;
    P.label.assign(P.frames * cells_f, -1);
    const int style = uni(0, 2);
    for (int f = 0; f < P.frames; ++f) {
        int32_t *img = P.label.data() + f * cells_f;
        if (style == 0)
            for (int k = 0, n = uni(1, 6); k < n; ++k) {  // rectangles
                const int x0 = uni(0, P.G.nx - 1), y0 = uni(0, P.G.ny - 1), w = uni(1, 9), hgt = uni(1, 9), l = uni(0, std::min(P.max_rows, 9));
                for (int y = y0; y < std::min(P.G.ny, y0 + hgt); ++y)
                    for (int x = x0; x < std::min(P.G.nx, x0 + w); ++x) img[y * P.G.nx + x] = l;
            }
        else
            for (size_t i = 0; i < cells_f; ++i) img[i] = style == 1 ? uni(-1, P.max_rows) : (uni(0, 3) ? 0 : -1);  // noise | one row
        const int32_t odd[] = {-1, P.max_rows, INT32_MAX, INT32_MIN, P.max_rows - 1};
        for (int k = 0; k < 3; ++k) img[uni(0, (int)cells_f - 1)] = odd[uni(0, 4)];
    }
    const int16_t special[] = {(int16_t)P.occupied_at, (int16_t)(P.occupied_at - 1), (int16_t)P.free_at, (int16_t)(P.free_at + 1), -32768, 32767};
    const int fill = uni(0, 3);
    P.maps.resize(P.n_maps * map_cells);
    for (int16_t &v : P.maps) v = fill == 0 ? special[uni(0, 5)] : (fill == 1 ? (int16_t)uni(-400, 400) : (fill == 2 ? (int16_t)(uni(0, 9) ? P.free_at - 5 : 32767) : (int16_t)-32768));
    if (uni(0, 1)) {
        P.occ_in.resize(P.frames * cells_f);
        for (int8_t &v : P.occ_in) v = (int8_t)(uni(0, 4) == 0 ? uni(-128, 127) : (uni(0, 1) ? 100 : (uni(0, 1) ? 0 : -1)));
    }
    return P;
}

static void verdict_cases() {
    for (int share = 1; share <= 256; share += 5)
        for (int landed = 1; landed <= 40; ++landed) {
            const PwppEvidenceRule R{0, 3, share, 257 - share};
            for (int free_ = 0; free_ <= landed; ++free_) {
                const int occupied = landed - free_;
                ++g_cases;
                expect(pwpp_evid_verdict(R, landed + 2, landed, occupied, free_) == brute_verdict(R, landed + 2, landed, occupied, free_), "verdict");
            }
            ++g_cases;
            expect(pwpp_evid_verdict(R, 0, 0, 0, 0) == PWPP_EV_NONE, "verdict of a row without cells");
        }
    const PwppEvidenceRule R{0, 3, 192, 192};
    expect(pwpp_evid_verdict(R, 4, 4, 1, 3) == PWPP_EV_MOVING && pwpp_evid_verdict(R, 8, 8, 2, 5) == PWPP_EV_UNDECIDED, "3/4 is 192/256, 5/8 is below");
    expect(pwpp_evid_verdict(R, 4, 4, 3, 1) == PWPP_EV_STATIC && pwpp_evid_verdict(R, 9, 2, 2, 0) == PWPP_EV_UNDECIDED, "static at the share; too few landed");
    const PwppEvidenceRule both{0, 1, 128, 128};
    expect(pwpp_evid_verdict(both, 2, 2, 1, 1) == PWPP_EV_MOVING, "both conditions: moving first");
    expect(pwpp_evid_verdict(R, 1 << 30, 1 << 30, 0, 1 << 30) == PWPP_EV_MOVING, "2^30 cells do not overflow");
    const PwppEvidenceRule bad[] = {{5, 1, 1, 1}, {-1, 1, 1, 1}, {0, 0, 1, 1}, {0, 1, 0, 1}, {0, 1, 257, 1}, {0, 1, 1, 0}, {0, 1, 1, 257}};
    const int which[] = {1, 1, 2, 3, 3, 4, 4};
    for (int k = 0; k < 7; ++k) expect(pwpp_evid_rule_check(bad[k]) == which[k], "rule range");
    expect(pwpp_evid_rule_check(PwppEvidenceRule{4, 1, 256, 1}) == 0, "rule in range");
    g_cases += 12;
}

// ---- dump ------------------------------------------------------------------------------------------------------------------
template <class T>
static std::vector<T> read_file(const char *path) {
    std::vector<T> v;
    if (std::strcmp(path, "-") == 0) return v;
    FILE *f = std::fopen(path, "rb");
    if (!f) std::printf("cannot read %s\n", path), std::exit(2);
    T x;
    while (std::fread(&x, sizeof(T), 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return v;
}
template <class T>
static void write_file(const std::string &path, const std::vector<T> &v) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) std::printf("cannot write %s\n", path.c_str()), std::exit(2);
    std::fclose(f);
}

// evidence_check dump label.i32 occ.i8|- poses.f64 n_poses frames map_of.i32|- x0 y0 cell nx ny X0 Y0 CELL NX NY occupied_at free_at n_maps maps.i16
//                     gate min_cells moving_share static_share max_rows path out   -> out.rows, out.class, out.occ (with occ)
static int dump(int argc, char **argv) {
    if (argc != 29) return std::printf("dump: 27 arguments expected\n"), 2;
    Problem P;
    P.label = read_file<int32_t>(argv[2]), P.occ_in = read_file<int8_t>(argv[3]), P.poses = read_file<double>(argv[4]);
    P.n_poses = std::atoi(argv[5]), P.frames = std::atoi(argv[6]);
    const std::vector<int32_t> map_of = read_file<int32_t>(argv[7]);
    P.G.x0 = std::atof(argv[8]), P.G.y0 = std::atof(argv[9]), P.G.cell = std::atof(argv[10]), P.G.nx = std::atoi(argv[11]), P.G.ny = std::atoi(argv[12]);
    P.G.X0 = std::atof(argv[13]), P.G.Y0 = std::atof(argv[14]), P.G.CELL = std::atof(argv[15]), P.G.NX = std::atoi(argv[16]), P.G.NY = std::atoi(argv[17]);
    pwpp_fuse_reciprocal(P.G.CELL, P.G.inv_CELL);
    P.occupied_at = std::atoi(argv[18]), P.free_at = std::atoi(argv[19]), P.n_maps = std::atoi(argv[20]);
    P.maps = read_file<int16_t>(argv[21]);
    P.R = PwppEvidenceRule{std::atoi(argv[22]), std::atoi(argv[23]), std::atoi(argv[24]), std::atoi(argv[25])};
    P.max_rows = std::atoi(argv[26]);
    const int path = std::atoi(argv[27]);
    const size_t cells = (size_t)P.G.nx * P.G.ny * (size_t)P.frames;
    if (P.frames < 1 || P.label.size() != cells || (!P.occ_in.empty() && P.occ_in.size() != cells) || P.poses.size() != (size_t)P.n_poses * 6 ||
        P.maps.size() != (size_t)P.G.NX * P.G.NY * (size_t)P.n_maps || (!map_of.empty() && map_of.size() != (size_t)P.frames))
        return std::printf("dump: the files do not have the stated sizes\n"), 2;
    for (int f = 0; f < P.frames; ++f) P.map_of.push_back(pwpp_map_of_frame(map_of.empty() ? nullptr : map_of.data(), P.n_maps, f));
    for (const int32_t k : P.map_of)
        if (k < -1 || k >= P.n_maps) return std::printf("dump: map_of_frame names map %d\n", k), 2;
    std::mt19937 rng(7u);
    const Result r = dealt(P, path, rng);
    const std::string out = argv[28];
    write_file(out + ".rows", r.rows), write_file(out + ".class", r.cell_class);
    if (!P.occ_in.empty()) write_file(out + ".occ", r.occ_out);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "dump") == 0) return dump(argc, argv);
    std::mt19937 rng(20261020u);
    verdict_cases();
    for (int round = 0; round < 2400; ++round) {
        const Problem P = random_problem(rng, round);
        const Result want = brute(P);
        compare(P, dealt(P, 1, rng), want, "path 1 against the brute force");
        compare(P, dealt(P, 2, rng), want, "path 2 against the brute force");
        ++g_cases;
    }
    std::printf("evidence_check: %ld cases, %ld mismatches\n", g_cases, g_bad);
    return g_bad == 0 ? 0 : 1;
}
