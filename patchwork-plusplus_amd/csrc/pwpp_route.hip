// pwpp_route.hip -- the gfx950 (MI355X) kernels of the routes on the reach field: for every (frame, start) the chain of `from` from
// the start to the frame's source, its row of sums, its cells and the few waypoints a controller tracks (pwpp_route_grid,
// pwpp_plan_grid; include/pwpp.h has the rules, pwpp_route.h the arithmetic and the proofs).  Reads the cost bytes, dist2
// and from; writes rows and lists.  Integers only.
//
// One launch per call, one of two kernels with the same bytes:
//   k_route_lanes   (option "route_path" = 1, the yardstick) a lane per route, wholly serial: the walk, then -- for a route that arrived
//            and with max_waypoints > 0 -- the waypoints, every search walking `look` cells ahead through from again and testing one
//            line after the other (pwpp_route_scan_ahead).
//   k_route_waves   ("route_path" = 2) a wave per route.  Every lane takes the same hops (the chain is the serial part: one dependent
//            load per hop, a broadcast); the route's last PWPP_ROUTE_WINDOW cells lie in LDS, 2 KB per wave, so the waypoints need
//            neither the cell list nor a second walk.  As soon as the walk is `look` cells ahead of the last waypoint (or has
//            arrived) the lanes take the candidates from the far end, 64 at a time, one line each, and a ballot picks the largest
//            clear one.  A route that then turns out BROKEN has its stored waypoints taken back by the lane that wrote them.
// The walk is a dependent chain: a route takes its hops times one L2 or HBM latency, and a call's time is set by the routes in
// flight.  No atomics, no barriers (a wave never waits for another; the window's cells are written by every lane of the wave
// with the same value, so a lane reads what it wrote itself), every output has one writer.  The hop bound nx ny - 1 of
// pwpp_route_next is the only bound of the walk; a line has at most `look` cells, a search `look` candidates, a route at most
// `cells` waypoints.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwpp_dev.h"  // the launchers' prototypes
#include "pwpp_route.h"

namespace {

constexpr int kLaneBlock = 64;    // k_route_lanes: routes diverge at once, small blocks spread them over the CUs
constexpr int kWaveBlock = 256;   // k_route_waves: 4 waves, 4 routes
constexpr int kWavesPerBlock = kWaveBlock / 64;
constexpr int kWindowMask = PWPP_ROUTE_WINDOW - 1;
static_assert((PWPP_ROUTE_WINDOW & kWindowMask) == 0 && PWPP_ROUTE_WINDOW > PWPP_ROUTE_MAX_LOOK, "r_a .. r_{a + look} lie in the window");
// What option "route_path" = 0 means: the wave per route (true) or the lane per route (false).  Decided by tools/route_cost.py
// (profiles/route_cost.txt), not in advance: per 1024 frames of 256 x 256 cells the waves take 58 to 67 us against 110 to 182 us with one
// start a frame and 166 to 212 against 188 to 353 us with 16, with lines that nearly all fail (line_cost 0) and lines that are nearly all
// clear (100); at 64 x 64 cells, routes of 8 hops, 1 to 20 us less; in every one of the 16 cases beyond an A/A floor of under 1 us.
constexpr bool kRouteDefaultWaves = true;

struct RouteCall {
    PwppReachRule R;
    PwppRouteRule P;
    int32_t nx, ny, frames;
    int32_t sx, sy;  // the source where one serves every frame (sources == nullptr)
    int32_t n_start_sets, n_starts;
    int64_t routes;  // frames * n_starts
};

struct RouteImages {
    const int8_t *cost;
    const int32_t *dist2;
    const int32_t *sources, *from, *starts;
};

// the view of frame f
__device__ inline PwppRouteBytes view_of(const RouteCall &C, const RouteImages &I, int f, int sx, int sy) {
    const size_t base = (size_t)f * (size_t)C.nx * (size_t)C.ny;
    return PwppRouteBytes{C.R, I.cost + base, I.dist2 ? I.dist2 + base : nullptr, C.nx, C.ny, sx, sy};
}

// what both kernels know of route r before they walk
struct RouteTask {
    int f;
    int32_t start, source;
    const int32_t *from;  // the frame's
};
__device__ inline RouteTask task_of(const RouteCall &C, const RouteImages &I, int64_t r, int &sx, int &sy) {
    RouteTask T;
    T.f = (int)(r / C.n_starts);
    const int k = (int)(r - (int64_t)T.f * C.n_starts);
    sx = I.sources ? I.sources[2 * (size_t)T.f] : C.sx, sy = I.sources ? I.sources[2 * (size_t)T.f + 1] : C.sy;
    const int32_t *s = I.starts + 2 * ((size_t)(C.n_start_sets > 1 ? T.f : 0) * (size_t)C.n_starts + (size_t)k);
    T.start = s[1] * C.nx + s[0], T.source = sy * C.nx + sx;
    T.from = I.from + (size_t)T.f * (size_t)C.nx * (size_t)C.ny;
    return T;
}

__device__ inline void store_row(PwppRouteRow *rows, int64_t r, const PwppRouteRow &row) {
    int32_t *o = reinterpret_cast<int32_t *>(rows) + 8 * r;  // (4-byte aligned: eight stores)
    o[0] = row.status, o[1] = row.cells, o[2] = row.cost, o[3] = row.edge_steps, o[4] = row.corner_steps, o[5] = row.max_term, o[6] = row.min_dist2,
    o[7] = row.waypoints;
}

// grid (ceil(routes / kLaneBlock))
__global__ __launch_bounds__(kLaneBlock) void k_route_lanes(RouteCall C, RouteImages I, PwppRouteRow *rows, int32_t *cells, int32_t *waypoints) {
    const int64_t r = (int64_t)blockIdx.x * kLaneBlock + threadIdx.x;
    if (r >= C.routes) return;
    int sx, sy;
    const RouteTask T = task_of(C, I, r, sx, sy);
    const PwppRouteBytes V = view_of(C, I, T.f, sx, sy);
    int32_t *my_cells = cells + (size_t)r * (size_t)C.P.max_cells, *my_wps = waypoints + (size_t)r * (size_t)C.P.max_waypoints;  // (not formed into an address where the limit is 0)
    PwppRouteWalk W;
    if (pwpp_route_begin(V, T.from, C.nx, T.start, W)) {
        do {
            if (W.row.cells <= C.P.max_cells) my_cells[W.row.cells - 1] = W.c;
        } while (pwpp_route_next(V, T.from, C.nx, C.ny, T.source, W));
    }
    for (int32_t i = W.row.cells; i < C.P.max_cells; ++i) my_cells[i] = -1;
    int32_t nw = 0;
    if (W.row.status == PWPP_ROUTE_STATUS_OK && C.P.max_waypoints > 0) {
        const uint32_t limit = (uint32_t)(C.R.base + C.P.line_cost);
        const int32_t last = W.row.cells - 1;
        int32_t a = 0, ca = T.start;
        my_wps[nw++] = ca;
        while (a < last) {  // (a grows by at least 1)
            int32_t cb = ca;
            a += pwpp_route_scan_ahead(V, T.from, C.nx, ca, last - a < C.P.look ? last - a : C.P.look, limit, cb);
            ca = cb;
            if (nw < C.P.max_waypoints) my_wps[nw] = ca;
            ++nw;
        }
    }
    for (int32_t i = nw; i < C.P.max_waypoints; ++i) my_wps[i] = -1;
    W.row.waypoints = nw;
    store_row(rows, r, W.row);
}

// grid (ceil(routes / kWavesPerBlock))
__global__ __launch_bounds__(kWaveBlock) void k_route_waves(RouteCall C, RouteImages I, PwppRouteRow *rows, int32_t *cells, int32_t *waypoints) {
    __shared__ int32_t s_window[kWavesPerBlock][PWPP_ROUTE_WINDOW];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    if (r >= C.routes) return;  // (the whole wave; the kernel has no barrier)
    int32_t *win = s_window[wave];
    int sx, sy;
    const RouteTask T = task_of(C, I, r, sx, sy);
    const PwppRouteBytes V = view_of(C, I, T.f, sx, sy);
    int32_t *my_cells = cells + (size_t)r * (size_t)C.P.max_cells, *my_wps = waypoints + (size_t)r * (size_t)C.P.max_waypoints;
    const uint32_t limit = (uint32_t)(C.R.base + C.P.line_cost);
    const bool search = C.P.max_waypoints > 0;
    PwppRouteWalk W;
    int32_t nw = 0;  // the waypoints found so far; min(nw, max_waypoints) are stored, by lane 0
    if (pwpp_route_begin(V, T.from, C.nx, T.start, W)) {  // (everything about the walk is uniform over the wave)
        int32_t a = 0;  // the newest waypoint's index into the route
        if (search) {
            if (lane == 0) my_wps[0] = T.start;
            nw = 1;
        }
        for (;;) {
            const int32_t i = W.row.cells - 1;  // W.c = r_i
            win[i & kWindowMask] = W.c;         // (every lane, the same value: a lane reads back what it wrote itself)
            if (lane == 0 && i < C.P.max_cells) my_cells[i] = W.c;
            const bool more = pwpp_route_next(V, T.from, C.nx, C.ny, T.source, W);
            // the searches that can be decided now: with `look` cells beyond r_a known, or all of a route that has arrived
            while (search && a < i && (i - a >= C.P.look || (!more && W.row.status == PWPP_ROUTE_STATUS_OK))) {
                const int32_t hi = i - a < C.P.look ? i : a + C.P.look, ca = win[a & kWindowMask];
                const int ay = ca / C.nx, ax = ca - ay * C.nx;
                int32_t b = a + 1;
                for (int32_t top = hi; top > a + 1; top -= 64) {  // (uniform: at most 4 rounds)
                    const int32_t mine = top - lane;
                    bool clear = false;
                    if (mine > a + 1) {
                        const int32_t cb = win[mine & kWindowMask];
                        const int by = cb / C.nx;
                        clear = pwpp_route_line_clear(V, ax, ay, cb - by * C.nx, by, limit);
                    }
                    const unsigned long long found = __ballot(clear);
                    if (found != 0ull) {
                        b = top - (__ffsll((long long)found) - 1);
                        break;
                    }
                }
                a = b;
                if (lane == 0 && nw < C.P.max_waypoints) my_wps[nw] = win[a & kWindowMask];
                ++nw;
            }
            if (!more) break;
        }
    }
    const int32_t stored = W.row.cells < C.P.max_cells ? W.row.cells : C.P.max_cells;
    for (int32_t i = stored + lane; i < C.P.max_cells; i += 64) my_cells[i] = -1;
    const int32_t kept = nw < C.P.max_waypoints ? nw : C.P.max_waypoints;
    if (W.row.status != PWPP_ROUTE_STATUS_OK) {  // (NONE: nothing was stored; BROKEN: what the searches before the break stored goes)
        if (lane == 0)
            for (int32_t i = 0; i < kept; ++i) my_wps[i] = -1;  // (the lane that wrote them)
        nw = 0;
    }
    for (int32_t i = kept + lane; i < C.P.max_waypoints; i += 64) my_wps[i] = -1;
    if (lane == 0) {
        W.row.waypoints = nw;
        store_row(rows, r, W.row);
    }
}

}  // namespace

// pwpp_route_grid on device memory.  The caller has checked what pwpp_launch_reach asks for and the route's own: P (look 1 .. 256, the
// limits >= 0), the starts (inside the image; n_start_sets x n_starts x {x, y} on the device), frames * n_starts * max(limits, 1) <=
// 2^31 - 1; from, rows, cells (null with max_cells == 0) and waypoints (null with max_waypoints == 0) are 4-byte aligned.
extern "C" int pwpp_launch_routes(const PwppReachRule *R, const PwppRouteRule *P, int nx, int ny, int frames, const int8_t *cost, const int32_t *dist2, int sx, int sy,
                                  const int32_t *sources, const int32_t *from, const int32_t *starts, int n_start_sets, int n_starts, void *rows, int32_t *cells,
                                  int32_t *waypoints, int path, hipStream_t stream) {
    if ((R->use_dist2 != 0) != (dist2 != nullptr) || !cost || (P->max_cells > 0 && !cells) || (P->max_waypoints > 0 && !waypoints) || P->look < 1 ||
        P->look > PWPP_ROUTE_MAX_LOOK)
        return (int)hipErrorInvalidValue;
    RouteCall C;
    C.R = *R, C.P = *P;
    C.nx = nx, C.ny = ny, C.frames = frames, C.sx = sx, C.sy = sy, C.n_start_sets = n_start_sets, C.n_starts = n_starts;
    C.routes = (int64_t)frames * (int64_t)n_starts;
    const RouteImages I{cost, dist2, sources, from, starts};
    PwppRouteRow *out = static_cast<PwppRouteRow *>(rows);
    if (path == 0 ? kRouteDefaultWaves : path == 2)
        hipLaunchKernelGGL(k_route_waves, dim3((unsigned)((C.routes + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kWaveBlock), 0, stream, C, I, out, cells, waypoints);
    else
        hipLaunchKernelGGL(k_route_lanes, dim3((unsigned)((C.routes + kLaneBlock - 1) / kLaneBlock)), dim3(kLaneBlock), 0, stream, C, I, out, cells, waypoints);
    return (int)hipGetLastError();
}
