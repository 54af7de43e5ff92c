// route_check.cpp -- the functions of csrc/pwpp_route.h on the host, dealt the way both kernels of csrc/pwpp_route.hip deal them (a lane
// per route: walk, then pwpp_route_scan_ahead; a wave per route: a window of PWPP_ROUTE_WINDOW cells, the candidates from the far end
// 64 at a time, the lowest set lane of the round), against a brute force of its own: terms, steps, a Bellman-Ford field, the chain, the closed form of THE LINE and a search that tries every candidate.  Good and
// damaged from images, routes of a few cells and routes that wrap the wave's window.  No GPU.  Built by tests/test_route_cpu.py with the address and undefined-behaviour sanitizers.
//   route_check                    random cases; prints "route_check: N cases, M mismatches"; exit status 1 with a mismatch
//   route_check dump cost nx ny frames base lethal unknown clearance2 dist2|- sources n_sources from starts n_start_sets n_starts
//               max_cells max_waypoints look line_cost deal out
//                                  the routes of the images in the files, by deal 1 or 2, into out.rows, out.cells, out.waypoints;
//                                  prints the time the deals took
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "pwpp_route.h"

namespace {

struct Frame {
    int nx, ny, sx, sy;
    PwppReachRule R;
    std::vector<int8_t> cost;
    std::vector<int32_t> dist2;  // empty: none
    std::vector<int32_t> from;
};

struct Result {
    PwppRouteRow row;
    std::vector<int32_t> cells, wps;
    bool operator==(const Result &o) const { return std::memcmp(&row, &o.row, sizeof(row)) == 0 && cells == o.cells && wps == o.wps; }
};

// ---- the deals, as the kernels have them ----------------------------------------------------------------------------------------
template <class View>
Result deal_lanes(const View &V, const Frame &F, const PwppRouteRule &P, int32_t start) {
    Result out;
    out.cells.assign((size_t)P.max_cells, -7), out.wps.assign((size_t)P.max_waypoints, -7);
    const int32_t source = F.sy * F.nx + F.sx;
    PwppRouteWalk W;
    if (pwpp_route_begin(V, F.from.data(), F.nx, start, W)) {
        do {
            if (W.row.cells <= P.max_cells) out.cells[(size_t)W.row.cells - 1] = W.c;
        } while (pwpp_route_next(V, F.from.data(), F.nx, F.ny, source, W));
    }
    for (int32_t i = W.row.cells; i < P.max_cells; ++i) out.cells[(size_t)i] = -1;
    int32_t nw = 0;
    if (W.row.status == PWPP_ROUTE_STATUS_OK && P.max_waypoints > 0) {
        const uint32_t limit = (uint32_t)(F.R.base + P.line_cost);
        const int32_t last = W.row.cells - 1;
        int32_t a = 0, ca = start;
        out.wps[(size_t)nw++] = ca;
        while (a < last) {
            int32_t cb = ca;
            a += pwpp_route_scan_ahead(V, F.from.data(), F.nx, ca, last - a < P.look ? last - a : P.look, limit, cb);
            ca = cb;
            if (nw < P.max_waypoints) out.wps[(size_t)nw] = ca;
            ++nw;
        }
    }
    for (int32_t i = nw; i < P.max_waypoints; ++i) out.wps[(size_t)i] = -1;
    W.row.waypoints = nw;
    out.row = W.row;
    return out;
}

template <class View>
Result deal_waves(const View &V, const Frame &F, const PwppRouteRule &P, int32_t start) {
    Result out;
    out.cells.assign((size_t)P.max_cells, -7), out.wps.assign((size_t)P.max_waypoints, -7);
    std::vector<int32_t> win(PWPP_ROUTE_WINDOW, -9);
    const int mask = PWPP_ROUTE_WINDOW - 1;
    const int32_t source = F.sy * F.nx + F.sx;
    const uint32_t limit = (uint32_t)(F.R.base + P.line_cost);
    const bool search = P.max_waypoints > 0;
    PwppRouteWalk W;
    int32_t nw = 0;
    if (pwpp_route_begin(V, F.from.data(), F.nx, start, W)) {
        int32_t a = 0;
        if (search) out.wps[0] = start, nw = 1;
        for (;;) {
            const int32_t i = W.row.cells - 1;
            win[(size_t)(i & mask)] = W.c;
            if (i < P.max_cells) out.cells[(size_t)i] = W.c;
            const bool more = pwpp_route_next(V, F.from.data(), F.nx, F.ny, source, W);
            while (search && a < i && (i - a >= P.look || (!more && W.row.status == PWPP_ROUTE_STATUS_OK))) {
                const int32_t hi = i - a < P.look ? i : a + P.look, ca = win[(size_t)(a & mask)];
                const int ay = ca / F.nx, ax = ca - ay * F.nx;
                int32_t b = a + 1;
                for (int32_t top = hi; top > a + 1; top -= 64) {
                    unsigned long long found = 0;
                    for (int lane = 0; lane < 64; ++lane) {  // (the lanes of the round)
                        const int32_t mine = top - lane;
                        if (mine <= a + 1) continue;
                        const int32_t cb = win[(size_t)(mine & mask)];
                        const int by = cb / F.nx;
                        if (pwpp_route_line_clear(V, ax, ay, cb - by * F.nx, by, limit)) found |= 1ull << lane;
                    }
                    if (found != 0) {
                        b = top - __builtin_ctzll(found);
                        break;
                    }
                }
                a = b;
                if (nw < P.max_waypoints) out.wps[(size_t)nw] = win[(size_t)(a & mask)];
                ++nw;
            }
            if (!more) break;
        }
    }
    const int32_t stored = W.row.cells < P.max_cells ? W.row.cells : P.max_cells;
    for (int32_t i = stored; i < P.max_cells; ++i) out.cells[(size_t)i] = -1;
    const int32_t kept = nw < P.max_waypoints ? nw : P.max_waypoints;
    if (W.row.status != PWPP_ROUTE_STATUS_OK) {
        for (int32_t i = 0; i < kept; ++i) out.wps[(size_t)i] = -1;
        nw = 0;
    }
    for (int32_t i = kept; i < P.max_waypoints; ++i) out.wps[(size_t)i] = -1;
    W.row.waypoints = nw;
    out.row = W.row;
    return out;
}

PwppRouteBytes bytes_of(const Frame &F) { return PwppRouteBytes{F.R, F.cost.data(), F.dist2.empty() ? nullptr : F.dist2.data(), F.nx, F.ny, F.sx, F.sy}; }

// ---- the brute force: its own text of every rule ----------------------------------------------------------------------------------
int bf_term(const Frame &F, int x, int y) {
    if (x < 0 || y < 0 || x >= F.nx || y >= F.ny) return 0;
    const size_t i = (size_t)y * (size_t)F.nx + (size_t)x;
    int c = F.cost[i];
    if (c < 0) c = F.R.unknown;
    bool ok = c >= 0 && c < F.R.lethal;
    if (!F.dist2.empty() && F.dist2[i] <= F.R.clearance2) ok = false;
    if (ok) return F.R.base + c;
    return x == F.sx && y == F.sy ? F.R.base : 0;
}
// the step between two cells (x, y) and (u, v), 0: none
int bf_step(const Frame &F, int x, int y, int u, int v) {
    const int dx = u - x, dy = v - y;
    if (std::max(std::abs(dx), std::abs(dy)) != 1) return 0;
    const int ta = bf_term(F, x, y), tb = bf_term(F, u, v);
    if (ta == 0 || tb == 0) return 0;
    if (dx != 0 && dy != 0) return bf_term(F, u, y) != 0 && bf_term(F, x, v) != 0 ? 7 * (ta + tb) : 0;
    return 5 * (ta + tb);
}
void bf_field(Frame &F) {
    const int n = F.nx * F.ny;
    const int64_t none = INT64_MAX / 4;
    std::vector<int64_t> v((size_t)n, none);
    v[(size_t)(F.sy * F.nx + F.sx)] = 0;
    for (bool changed = true; changed;) {
        changed = false;
        for (int c = 0; c < n; ++c)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int x = c % F.nx, y = c / F.nx, st = bf_step(F, x, y, x + dx, y + dy);
                    if (st == 0) continue;
                    const int64_t cand = v[(size_t)((y + dy) * F.nx + x + dx)] + st;
                    if (cand < v[(size_t)c]) v[(size_t)c] = cand, changed = true;
                }
    }
    F.from.assign((size_t)n, -1);
    for (int c = 0; c < n; ++c) {
        if (v[(size_t)c] >= none) continue;
        const int x = c % F.nx, y = c / F.nx;
        if (x == F.sx && y == F.sy) {
            F.from[(size_t)c] = c;
            continue;
        }
        for (int dy = -1; dy <= 1 && F.from[(size_t)c] < 0; ++dy)
            for (int dx = -1; dx <= 1 && F.from[(size_t)c] < 0; ++dx) {
                const int st = bf_step(F, x, y, x + dx, y + dy);
                if (st != 0 && v[(size_t)((y + dy) * F.nx + x + dx)] + st == v[(size_t)c]) F.from[(size_t)c] = (y + dy) * F.nx + x + dx;
            }
    }
}
bool bf_clear(const Frame &F, int32_t ca, int32_t cb, int limit) {
    const int ax = ca % F.nx, ay = ca / F.nx, dx = cb % F.nx - ax, dy = cb / F.nx - ay, n = std::max(std::abs(dx), std::abs(dy));
    int px = ax, py = ay;
    for (int k = 1; k <= n; ++k) {
        const int x = ax + (dx > 0 ? 1 : -1) * ((2 * k * std::abs(dx) + n) / (2 * n)), y = ay + (dy > 0 ? 1 : -1) * ((2 * k * std::abs(dy) + n) / (2 * n));
        if (x != px && y != py && (bf_term(F, px, y) == 0 || bf_term(F, x, py) == 0)) return false;
        const int t = bf_term(F, x, y);
        if (t == 0 || t > limit) return false;
        px = x, py = y;
    }
    return true;
}
Result brute(const Frame &F, const PwppRouteRule &P, int32_t start) {
    Result out;
    out.cells.assign((size_t)P.max_cells, -1), out.wps.assign((size_t)P.max_waypoints, -1);
    out.row = PwppRouteRow{PWPP_ROUTE_STATUS_NONE, 0, 0, 0, 0, 0, PWPP_REACH_DIST_BEYOND, 0};
    if (F.from[(size_t)start] == -1) return out;
    std::vector<int32_t> route{start};
    const int n = F.nx * F.ny;
    int status = -1;
    while (status < 0) {
        const int32_t c = route.back(), to = F.from[(size_t)c];
        if (to == c) status = c == F.sy * F.nx + F.sx ? PWPP_ROUTE_STATUS_OK : PWPP_ROUTE_STATUS_BROKEN;
        else if ((int)route.size() - 1 >= n - 1 || to < 0 || to >= n) status = PWPP_ROUTE_STATUS_BROKEN;
        else {
            const int st = bf_step(F, c % F.nx, c / F.nx, to % F.nx, to / F.nx);
            if (st == 0) status = PWPP_ROUTE_STATUS_BROKEN;
            else {
                out.row.cost += st;
                (to % F.nx != c % F.nx && to / F.nx != c / F.nx ? out.row.corner_steps : out.row.edge_steps) += 1;
                route.push_back(to);
            }
        }
    }
    out.row.status = status, out.row.cells = (int32_t)route.size();
    for (const int32_t c : route) {
        out.row.max_term = std::max(out.row.max_term, bf_term(F, c % F.nx, c / F.nx));
        if (!F.dist2.empty()) out.row.min_dist2 = std::min(out.row.min_dist2, F.dist2[(size_t)c]);
    }
    for (size_t i = 0; i < route.size() && i < out.cells.size(); ++i) out.cells[i] = route[i];
    if (status == PWPP_ROUTE_STATUS_OK && P.max_waypoints > 0) {
        std::vector<int32_t> w{0};
        const int last = (int)route.size() - 1;
        while (w.back() < last) {
            const int a = w.back();
            int b = a + 1;
            for (int cand = a + 2; cand <= std::min(a + P.look, last); ++cand)  // (every candidate, the largest clear one stays)
                if (bf_clear(F, route[(size_t)a], route[(size_t)cand], F.R.base + P.line_cost)) b = cand;
            w.push_back(b);
        }
        out.row.waypoints = (int32_t)w.size();
        for (size_t i = 0; i < w.size() && i < out.wps.size(); ++i) out.wps[i] = route[(size_t)w[i]];
    }
    return out;
}

int self_test() {
    std::mt19937 rng(20250);
    auto pick = [&](int lo, int hi) { return (int)(rng() % (unsigned)(hi - lo + 1)) + lo; };
    long cases = 0, mismatches = 0, broken = 0, shortcuts = 0;
    for (int round = 0; round < 260; ++round) {
        Frame F;
        F.nx = pick(1, 15), F.ny = pick(1, 15);
        if (round % 13 == 0) F.nx = pick(1, 3) == 1 ? 1 : 40, F.ny = F.nx == 1 ? 33 : 9;
        F.sx = pick(0, F.nx - 1), F.sy = pick(0, F.ny - 1);
        const bool with_d2 = round % 3 == 0;
        F.R = PwppReachRule{pick(1, 20), pick(50, 101), pick(-1, 60), with_d2 ? pick(0, 4) : 0, 0, with_d2 ? 1 : 0};
        const int n = F.nx * F.ny, wall = pick(0, 30), open = round % 5 == 0;
        F.cost.resize((size_t)n);
        for (auto &c : F.cost) c = open ? 0 : (pick(0, 99) < wall ? (int8_t)pick(100, 127) : (pick(0, 9) == 0 ? (int8_t)pick(-128, -1) : (int8_t)pick(0, 99)));
        if (with_d2) {
            F.dist2.resize((size_t)n);
            for (auto &d : F.dist2) d = pick(0, 9) == 0 ? PWPP_REACH_DIST_BEYOND : pick(0, 40);
        }
        bf_field(F);
        if (round % 4 == 3)  // a damaged from: any value anywhere
            for (int k = pick(1, 4); k > 0; --k) F.from[(size_t)pick(0, n - 1)] = pick(0, 5) == 0 ? pick(-3, n + 2) : pick(0, n - 1);
        for (int k = 0; k < 12; ++k) {
            PwppRouteRule P{pick(0, 3) == 0 ? 0 : pick(1, 40), pick(0, 4) == 0 ? 0 : pick(1, 12), pick(0, 2) == 0 ? pick(1, 3) : pick(1, 256), pick(0, 100)};
            if (round % 7 == 0) P.look = 64 + pick(-1, 1);
            const int32_t start = pick(0, n - 1);
            const Result want = brute(F, P, start);
            const Result got[2] = {deal_lanes(bytes_of(F), F, P, start), deal_waves(bytes_of(F), F, P, start)};
            ++cases;
            broken += want.row.status == PWPP_ROUTE_STATUS_BROKEN;
            shortcuts += want.row.status == PWPP_ROUTE_STATUS_OK && want.row.waypoints > 0 && want.row.waypoints < want.row.cells;
            for (int d = 0; d < 2; ++d)
                if (!(got[d] == want)) {
                    if (++mismatches <= 5)
                        std::printf("mismatch: round %d, %d x %d, start %d, deal %d: status %d/%d cells %d/%d cost %d/%d waypoints %d/%d\n", round, F.nx, F.ny, start, d,
                                    got[d].row.status, want.row.status, got[d].row.cells, want.row.cells, got[d].row.cost, want.row.cost, got[d].row.waypoints,
                                    want.row.waypoints);
                }
        }
    }
    // Routes past the wave's window of PWPP_ROUTE_WINDOW cells: a serpentine corridor, a strip with dear cells whose lines of `look` cells
    // straddle cell 512, and a 2-cycle walked to the hop bound of a 30 x 30 image.
    long wrapped = 0;
    for (int kind = 0; kind < 3; ++kind) {
        Frame F;
        F.R = PwppReachRule{2, 100, -1, 0, 0, 0};
        F.sx = F.sy = 0;
        if (kind == 0) {
            F.nx = 41, F.ny = 33;
            F.cost.assign((size_t)(F.nx * F.ny), 100);
            for (int y = 0; y < F.ny; y += 2)
                for (int x = 0; x < F.nx; ++x) F.cost[(size_t)(y * F.nx + x)] = 0;
            for (int y = 1, k = 0; y < F.ny; y += 2, ++k) F.cost[(size_t)(y * F.nx + (k % 2 == 0 ? F.nx - 1 : 0))] = 0;
        } else if (kind == 1) {
            F.nx = 700, F.ny = 3, F.sy = 1;
            F.cost.resize((size_t)(F.nx * F.ny));
            for (int i = 0; i < F.nx * F.ny; ++i) F.cost[(size_t)i] = i / F.nx == 1 ? (pick(0, 60) == 0 ? 60 : 0) : (pick(0, 3) == 0 ? 60 : 0);
        } else {
            F.nx = F.ny = 30;
            F.cost.assign(900, 0);
        }
        bf_field(F);
        const int n = F.nx * F.ny;
        int32_t start = kind == 0 ? (F.ny - 1) * F.nx + (((F.ny - 1) / 2) % 2 == 0 ? F.nx - 1 : 0) : (kind == 1 ? F.nx + F.nx - 1 : 15 * 30 + 15);
        if (kind == 2) F.from[(size_t)start] = start + 1, F.from[(size_t)start + 1] = start;
        for (const int look : {1, 3, 63, 64, 65, 255, 256})
            for (const int lists : {0, 1}) {
                const PwppRouteRule P{lists ? n : 0, lists ? n : 7, look, 20};
                const Result want = brute(F, P, start);
                const Result got[2] = {deal_lanes(bytes_of(F), F, P, start), deal_waves(bytes_of(F), F, P, start)};
                ++cases;
                wrapped += want.row.cells > PWPP_ROUTE_WINDOW + 150;
                if (want.row.status != (kind == 2 ? PWPP_ROUTE_STATUS_BROKEN : PWPP_ROUTE_STATUS_OK) || (kind == 2 && want.row.cells != n)) ++mismatches;
                if (kind != 2 && look > 1 && !(want.row.waypoints > 2 && want.row.waypoints < want.row.cells)) ++mismatches;
                for (int d = 0; d < 2; ++d)
                    if (!(got[d] == want) && ++mismatches <= 5)
                        std::printf("mismatch: long route %d, look %d, deal %d: status %d/%d cells %d/%d waypoints %d/%d\n", kind, look, d, got[d].row.status, want.row.status,
                                    got[d].row.cells, want.row.cells, got[d].row.waypoints, want.row.waypoints);
            }
    }
    std::printf("route_check: %ld cases, %ld mismatches (%ld broken chains, %ld routes with a shortcut, %ld routes past the window)\n", cases, mismatches, broken, shortcuts,
                wrapped);
    return mismatches == 0 && broken > 20 && shortcuts > 100 && wrapped == 42 ? 0 : 1;
}

template <class T>
std::vector<T> read_file(const char *path, size_t n) {
    std::vector<T> v(n);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "route_check: cannot read %zu items from %s\n", n, path);
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

int dump(char **a) {
    const int nx = std::atoi(a[1]), ny = std::atoi(a[2]), frames = std::atoi(a[3]), n_sources = std::atoi(a[10]), n_sets = std::atoi(a[13]), n_starts = std::atoi(a[14]);
    const size_t per = (size_t)nx * (size_t)ny;
    const bool with_d2 = std::strcmp(a[8], "-") != 0;
    const PwppReachRule R{std::atoi(a[4]), std::atoi(a[5]), std::atoi(a[6]), with_d2 ? std::atoi(a[7]) : 0, 0, with_d2 ? 1 : 0};
    const PwppRouteRule P{std::atoi(a[15]), std::atoi(a[16]), std::atoi(a[17]), std::atoi(a[18])};
    const int deal = std::atoi(a[19]);
    const auto cost = read_file<int8_t>(a[0], per * (size_t)frames);
    const auto dist2 = with_d2 ? read_file<int32_t>(a[8], per * (size_t)frames) : std::vector<int32_t>();
    const auto src = read_file<int32_t>(a[9], 2 * (size_t)n_sources), from = read_file<int32_t>(a[11], per * (size_t)frames);
    const auto starts = read_file<int32_t>(a[12], 2 * (size_t)n_sets * (size_t)n_starts);
    FILE *fr = std::fopen((std::string(a[20]) + ".rows").c_str(), "wb"), *fc = std::fopen((std::string(a[20]) + ".cells").c_str(), "wb"),
         *fw = std::fopen((std::string(a[20]) + ".waypoints").c_str(), "wb");
    if (!fr || !fc || !fw) return 2;
    double walk_us = 0.0;  // the deals alone: what tools/route_cost.py reports as the walk on the host
    for (int f = 0; f < frames; ++f) {
        Frame F;
        F.nx = nx, F.ny = ny, F.R = R;
        F.sx = src[2 * (size_t)(n_sources > 1 ? f : 0)], F.sy = src[2 * (size_t)(n_sources > 1 ? f : 0) + 1];
        F.cost.assign(cost.begin() + (long)(per * (size_t)f), cost.begin() + (long)(per * (size_t)(f + 1)));
        if (with_d2) F.dist2.assign(dist2.begin() + (long)(per * (size_t)f), dist2.begin() + (long)(per * (size_t)(f + 1)));
        F.from.assign(from.begin() + (long)(per * (size_t)f), from.begin() + (long)(per * (size_t)(f + 1)));
        for (int k = 0; k < n_starts; ++k) {
            const int32_t *s = starts.data() + 2 * ((size_t)(n_sets > 1 ? f : 0) * (size_t)n_starts + (size_t)k);
            const auto t0 = std::chrono::steady_clock::now();
            const Result r = deal == 2 ? deal_waves(bytes_of(F), F, P, s[1] * nx + s[0]) : deal_lanes(bytes_of(F), F, P, s[1] * nx + s[0]);
            walk_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            std::fwrite(&r.row, sizeof(r.row), 1, fr);
            if (!r.cells.empty()) std::fwrite(r.cells.data(), 4, r.cells.size(), fc);  // (a list without entries has no data pointer)
            if (!r.wps.empty()) std::fwrite(r.wps.data(), 4, r.wps.size(), fw);
        }
    }
    std::fclose(fr), std::fclose(fc), std::fclose(fw);
    std::printf("route_check: %lld routes walked in %.1f us\n", (long long)frames * n_starts, walk_us);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 23 && std::strcmp(argv[1], "dump") == 0) return dump(argv + 2);
    if (argc != 1) {
        std::fprintf(stderr, "usage: route_check | route_check dump ... (see the head of tools/route_check.cpp)\n");
        return 2;
    }
    return self_test();
}
