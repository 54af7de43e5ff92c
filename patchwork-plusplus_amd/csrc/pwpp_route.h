// pwpp_route.h -- the arithmetic of the routes on the reach field (pwpp_route_grid, pwpp_plan_grid), one text for the kernels
// (pwpp_route.hip), for the host side (pwpp_capi.cpp) and for the host program that runs the same functions against a brute force of
// its own (tools/route_check.cpp), the way pwpp_reach.h is one text for the field.  Internal; include/pwpp.h has the contract.
// Integers only.
//
// THE TERM t and THE STEP are those of pwpp_reach.h, through pwpp_reach_term and pwpp_reach_step: the same bytes, rule and corner
// rule.  A view gives t(x, y) of a cell that may lie anywhere -- 0 outside the image -- and is_source is true for the frame's source
// wherever the view is asked, on a line that merely passes over it too.
// THE ROUTE of a start s: r_0 = s, r_{i+1} = from[r_i], until a cell names itself.  A HOP c -> n = from[c] is a step of the contract
// iff n lies in [0, nx ny), is one of the 8 neighbours of c, t(c) > 0, t(n) > 0 and, across a corner, both cells that share an edge
// with c and with n have t > 0 (pwpp_route_hop: the step, >= 10, or 0).  The walk (pwpp_route_begin, pwpp_route_next) takes at most
// nx ny - 1 hops: THE ONLY LOOP BOUND.  A chain that visits no cell twice has at most that many, so only a chain with a cycle meets
// it.  WHY A FIELD'S OWN from NEVER BREAKS: pwpp_reach_from names a neighbour with t > 0 across an existing step whose value plus the
// step is the cell's value, so every hop is a step onto a strictly smaller value; the chain visits no cell twice and can only end
// where no predecessor is asked for, the source, which names itself.
// THE SUMS.  cost is the sum of the steps taken: at most nx ny - 1 steps of at most 14 (base + 100), below 2^31 by
// pwpp_reach_range_ok -- for ANY from image, a broken one too, because the hop bound holds for all.  On a field's own from the sum
// telescopes: reach[r_i] = reach[r_{i+1}] + step, so cost = reach[s].
// THE WAYPOINTS are indices into the route: w_0 = 0; from w_i = a < cells - 1, w_{i+1} is the largest b in (a, min(a + look, cells - 1)]
// with b == a + 1 or a CLEAR LINE r_a -> r_b.  The line is THE LINE of pwpp_visibility.h from r_a to r_b (pwpp_vis_line, pwpp_vis_step);
// clear iff for every k = 1 .. n: 0 < t(P_k) <= base + line_cost, and wherever both coordinates moved both squeezed cells
// A = (x_{k-1}, y_k) and B = (x_k, y_{k-1}) have t > 0 -- the reach's corner rule, stricter than the visibility's (there one free
// cell of the two is enough).  r_b is b - a <= look king moves from r_a, so n <= look <= 256: the bound of the line's loop.
// WHY THE POLYLINE IS A LEGAL PATH.  Every step of THE LINE moves each coordinate by at most one and the major one by exactly one:
// P_{k-1} -> P_k is a move to one of the 8 neighbours.  P_0 = r_a lies on a route whose hops were steps: t > 0.  Clear gives
// t(P_k) > 0 and the corner rule at every diagonal move: each move is a step of the reach contract.  Where b == a + 1 the segment
// is the hop itself.  The last waypoint is cells - 1, the source: the search always advances by at least 1 and never past cells - 1.
// look = 1: the interval is {a + 1}, so the waypoints are the route.  An open field of one cost byte <= line_cost with look >= cells - 1:
// every line is clear, the first search returns cells - 1: two waypoints, one where the start is the source.
// THE TWO DEALS.  A lane that has the route only through from walks look cells ahead of r_a and keeps the last clear candidate
// (pwpp_route_scan_ahead); a wave that keeps the route in a window tests candidates from the far end, 64 at a time, and takes the
// first clear one.  Both return the largest clear b: the same waypoint.
#ifndef PWPP_ROUTE_H
#define PWPP_ROUTE_H

#include <stdint.h>

#include "pwpp_reach.h"
#include "pwpp_visibility.h"

#define PWPP_ROUTE_STATUS_OK 0      // = PWPP_ROUTE_OK, PWPP_ROUTE_NONE, PWPP_ROUTE_BROKEN of include/pwpp.h
#define PWPP_ROUTE_STATUS_NONE 1
#define PWPP_ROUTE_STATUS_BROKEN 2
#define PWPP_ROUTE_MAX_LOOK 256
#define PWPP_ROUTE_MAX_STARTS 65536
#define PWPP_ROUTE_WINDOW 512  // the cells a wave keeps of its route, a power of two > PWPP_ROUTE_MAX_LOOK: r_a .. r_{a + look} never wrap onto each other

// the checked pwpp_route_params
struct PwppRouteRule {
    int32_t max_cells, max_waypoints, look, line_cost;
};
// pwpp_route: one row per (frame, start)
struct PwppRouteRow {
    int32_t status, cells, cost, edge_steps, corner_steps, max_term, min_dist2, waypoints;
};

// The views a route reads its frame through: t(x, y) of a cell anywhere, d2(i) of the cell with the index i inside the image.
// The view from the caller's bytes (the only one: kernels, host and checker are templates over it).
struct PwppRouteBytes {
    PwppReachRule R;
    const int8_t *cost;    // cell 0 of the frame
    const int32_t *dist2;  // ... or null
    int32_t nx, ny, sx, sy;
    PWPP_HD uint32_t t(int x, int y) const {
        if ((unsigned)x >= (unsigned)nx || (unsigned)y >= (unsigned)ny) return 0u;  // (before an address is formed)
        const int64_t i = (int64_t)y * nx + x;
        return pwpp_reach_term(R, (int)cost[i], R.use_dist2 ? dist2[i] : 0, x == sx && y == sy);
    }
    PWPP_HD int32_t d2(int32_t i) const { return dist2 ? dist2[i] : PWPP_REACH_DIST_BEYOND; }
};
// the hop c -> n, c inside the image and n any value: its step, or 0 where it is no step of the contract; tn: t(n) with a step
template <class View>
PWPP_HD inline uint32_t pwpp_route_hop(const View &V, int nx, int ny, int32_t c, int32_t n, bool &corner, uint32_t &tn) {
    if (n < 0 || n >= nx * ny) return 0u;  // (nx ny <= 1518730: the range check)
    const int cy = c / nx, cx = c - cy * nx, ey = n / nx, ex = n - ey * nx, dx = ex - cx, dy = ey - cy;
    if (dx < -1 || dx > 1 || dy < -1 || dy > 1 || (dx == 0 && dy == 0)) return 0u;
    const uint32_t tc = V.t(cx, cy);
    tn = V.t(ex, ey);
    if (tc == 0 || tn == 0) return 0u;
    corner = dx != 0 && dy != 0;
    if (corner && (V.t(ex, cy) == 0 || V.t(cx, ey) == 0)) return 0u;
    return pwpp_reach_step(tc, tn, corner);
}

// A walk in progress: `c` is the route's newest cell, r_{row.cells - 1}, and `n` its from.
struct PwppRouteWalk {
    PwppRouteRow row;
    int32_t c, n, hops;
};

// r_0 = start (inside the image).  False: no route (PWPP_ROUTE_NONE), the row is final.
template <class View>
PWPP_HD inline bool pwpp_route_begin(const View &V, const int32_t *from, int nx, int32_t start, PwppRouteWalk &W) {
    W.row = PwppRouteRow{PWPP_ROUTE_STATUS_NONE, 0, 0, 0, 0, 0, PWPP_REACH_DIST_BEYOND, 0};
    W.c = start, W.n = from[start], W.hops = 0;
    if (W.n == -1) return false;
    const int y = start / nx;
    W.row.cells = 1, W.row.max_term = (int32_t)V.t(start - y * nx, y), W.row.min_dist2 = V.d2(start);
    return true;
}

// One hop further.  True: W.c is the next cell of the route.  False: the route has ended and row.status says how.
template <class View>
PWPP_HD inline bool pwpp_route_next(const View &V, const int32_t *from, int nx, int ny, int32_t source, PwppRouteWalk &W) {
    if (W.n == W.c) {
        W.row.status = W.c == source ? PWPP_ROUTE_STATUS_OK : PWPP_ROUTE_STATUS_BROKEN;
        return false;
    }
    bool corner = false;
    uint32_t tn = 0, step = 0;
    if (W.hops >= nx * ny - 1 || (step = pwpp_route_hop(V, nx, ny, W.c, W.n, corner, tn)) == 0) {
        W.row.status = PWPP_ROUTE_STATUS_BROKEN;
        return false;
    }
    W.row.cost += (int32_t)step;
    if (corner) ++W.row.corner_steps;
    else ++W.row.edge_steps;
    W.c = W.n, W.n = from[W.c], ++W.hops, ++W.row.cells;
    if ((int32_t)tn > W.row.max_term) W.row.max_term = (int32_t)tn;
    const int32_t d = V.d2(W.c);
    if (d < W.row.min_dist2) W.row.min_dist2 = d;
    return true;
}

// whether the line from a to b, both on a route and at most PWPP_ROUTE_MAX_LOOK king moves apart, is clear; limit = base + line_cost
template <class View>
PWPP_HD inline bool pwpp_route_line_clear(const View &V, int ax, int ay, int bx, int by, uint32_t limit) {
    PwppVisLine L;
    pwpp_vis_line(ax, ay, bx, by, L);
    for (uint32_t k = 1; k <= L.n; ++k) {
        const int px = L.x, py = L.y;
        if (pwpp_vis_step(L) && (V.t(px, L.y) == 0 || V.t(L.x, py) == 0)) return false;  // A = (x_{k-1}, y_k), B = (x_k, y_{k-1})
        const uint32_t t = V.t(L.x, L.y);
        if (t == 0 || t > limit) return false;
    }
    return true;
}

// The next waypoint after r_a = `ca` of a route that is PWPP_ROUTE_OK, for the deal that has the route through from alone: `ahead` =
// min(look, cells - 1 - a) >= 1 cells are walked and the last clear candidate kept.  Returns b - a; cb: r_b.
template <class View>
PWPP_HD inline int32_t pwpp_route_scan_ahead(const View &V, const int32_t *from, int nx, int32_t ca, int32_t ahead, uint32_t limit, int32_t &cb) {
    const int ay = ca / nx, ax = ca - ay * nx;
    int32_t cur = ca, best = 1;
    for (int32_t j = 1; j <= ahead; ++j) {
        cur = from[cur];
        const int y = cur / nx;
        if (j == 1 || pwpp_route_line_clear(V, ax, ay, cur - y * nx, y, limit)) best = j, cb = cur;
    }
    return best;
}

#endif  // PWPP_ROUTE_H
