// pwpp_reach.h -- the arithmetic of the cost-to-reach field (pwpp_reach_grid, pwpp_reach_ground), one text for the kernels
// (pwpp_reach.hip), for the host side (pwpp_capi.cpp) and for the host program that runs the same functions against a Dijkstra of
// its own (tools/reach_check.cpp), the way pwpp_terrain.h is one text for the terrain analysis.  Internal; include/pwpp.h has the
// contract.  Integers only.
//
// THE TERM of a cell, t: 0 where the cell is impassable, base + cost (1 .. 355) where it is passable -- its cost byte, or the
// substitute of an unknown one, lies in 0 .. lethal - 1 and (with a dist2 image) dist2 > clearance2.  The frame's source is passable
// whatever its bytes say: t = base there if the rule refuses it.  A cell outside the image has t = 0.
// THE STEP from a to one of its 8 neighbours b, both with t > 0: 5 (t(a) + t(b)) across an edge, 7 (t(a) + t(b)) across a corner, and
// across a corner only where both cells that share an edge with a and with b have t > 0.  Symmetric in a and b; 10 .. 4970.
// THE FIELD, v: 0 at the source, PWPP_REACH_NONE elsewhere, then relaxed -- v(c) = min(v(c), v(n) + step(n, c)) over the neighbours
// n with v(n) != PWPP_REACH_NONE, a candidate above max_reach (where that is > 0) dropped -- in ANY order and with values of any age
// until nothing changes.  WHY THE ORDER DOES NOT MATTER.  (1) Every value ever stored is the length of a real step path from the
// source, by induction over the stores, so it is >= the true minimum d(c).  (2) Values only fall.  (3) At a fixed point v(c) <=
// v(n) + step(n, c) for every step, so along a shortest path s = c0, c1 .. ck: v(ci) <= d(ci) by induction from v(s) = 0; with (1),
// v = d.  With max_reach every prefix of a shortest path is no dearer than the path, so the cells with d <= max_reach get exactly d
// and no other cell ever gets a value: a stored value is >= d > max_reach, and such a candidate is dropped.
// HOW MANY SWEEPS.  If every sweep relaxes every cell at least once against values no older than the end of the sweep before,
// then after k sweeps every cell whose shortest path has k steps or fewer is final (induction along the path).  A shortest path
// has at most cells - 1 steps (steps cost > 0: it visits no cell twice), so sweep number `cells` changes nothing: pwpp_reach_sweep_bound.
// For the tiled schedule a pass visits every dirty tile and relaxes it to ITS fixed point against its halo; a tile whose border
// changed marks the neighbours that read it.  The same induction holds per pass, and per visit with the tile's own cells.
// THE RANGE.  A stored value is the length of a path that visits no cell twice (a walk that came back to c would have left a
// smaller value at c already, and values only fall): at most cells - 1 steps of at most 7 * 2 * (base + 100), so
//     v <= 14 (base + 100) (cells - 1) <= 2^31 - 2 < PWPP_REACH_NONE              (pwpp_reach_range_ok, in 64 bits)
// and a candidate v(n) + step <= 2^31 - 2 + 4970 < 2^32: the kernels add and compare in uint32.
// FROM.  Among the neighbours n of c with a step and v(n) + step(n, c) == v(c), the one with the smallest index jy * nx + jx -- the
// first in the order (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1) of pwpp_reach_dx / _dy; the source names itself; -1
// where v is PWPP_REACH_NONE.  v strictly falls along it, so the chain ends at the source.
#ifndef PWPP_REACH_H
#define PWPP_REACH_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#ifndef PWPP_HD
#define PWPP_HD __host__ __device__
#endif
#else
#ifndef PWPP_HD
#define PWPP_HD
#endif
#endif

#define PWPP_REACH_TILE_X 32  // the cells of one tile of the tiled schedule (option "reach_path" = 2): held in LDS with a halo of one cell
#define PWPP_REACH_TILE_Y 32
// The tiles of a frame that the entry points accept: sides <= 32768 and, by the range check at base 1, nx ny <= 1518730, so
// ceil(nx / 32) ceil(ny / 32) <= (nx / 32 + 1) (ny / 32 + 1) = nx ny / 1024 + (nx + ny) / 32 + 1 <= 1483.2 + (32768 + 46) / 32 + 1 < 2511
// (the sum of the sides is largest at the side limit).  The largest count there is is 2193, at 23365 x 65 (tools/reach_check.cpp).
#define PWPP_REACH_MAX_TILES 2560
#define PWPP_REACH_UNREACHED 0x7fffffffu  // PWPP_REACH_NONE as the kernels' uint32
#define PWPP_REACH_W_EDGE 5u
#define PWPP_REACH_W_CORNER 7u
#define PWPP_REACH_DIST_BEYOND 0x7fffffff  // PWPP_DIST_BEYOND: farther than every clearance

// what a call fixes for every cell (the checked pwpp_reach_params; use_dist2: a dist2 image was given)
struct PwppReachRule {
    int32_t base, lethal, unknown, clearance2, max_reach, use_dist2;
};

// the neighbours in the order of their index jy * nx + jx
PWPP_HD inline int pwpp_reach_dx(int k) { return k < 3 ? k - 1 : (k == 3 ? -1 : (k == 4 ? 1 : k - 6)); }
PWPP_HD inline int pwpp_reach_dy(int k) { return k < 3 ? -1 : (k < 5 ? 0 : 1); }

// t of a cell from its bytes; dist2 is read only with R.use_dist2
PWPP_HD inline uint32_t pwpp_reach_term(const PwppReachRule &R, int cost, int32_t dist2, bool is_source) {
    int c = cost;
    bool ok = true;
    if (c < 0) {
        c = R.unknown;
        ok = c >= 0;
    }
    ok = ok && c < R.lethal;  // (lethal <= 101: the bytes 101 .. 127 are lethal under every rule)
    if (R.use_dist2 && !(dist2 > R.clearance2)) ok = false;
    if (ok) return (uint32_t)(R.base + c);
    return is_source ? (uint32_t)R.base : 0u;
}

PWPP_HD inline uint32_t pwpp_reach_step(uint32_t ta, uint32_t tb, bool corner) { return (corner ? PWPP_REACH_W_CORNER : PWPP_REACH_W_EDGE) * (ta + tb); }

// 14 (base + 100) (nx ny - 1) <= 2^31 - 2; `worst`: the product
PWPP_HD inline bool pwpp_reach_range_ok(int base, int nx, int ny, int64_t &worst) {
    worst = 14 * ((int64_t)base + 100) * ((int64_t)nx * (int64_t)ny - 1);  // (base <= 255, sides <= 2^15: below 2^44)
    return worst <= (int64_t)0x7ffffffe;
}

// sweeps after which a schedule that has not stopped has a defect: the last one that can change a value is cells - 1
PWPP_HD inline int64_t pwpp_reach_sweep_bound(int64_t cells) { return cells + 1; }

// The views the functions below read a neighbourhood through: t(dx, dy) and v(dx, dy) of the cell at (dx, dy) from the centre,
// t = 0 for a cell outside the image (v is then not read).
//
// The smallest candidate for the centre over its neighbours, or PWPP_REACH_UNREACHED; the centre has t > 0.
template <class View>
PWPP_HD inline uint32_t pwpp_reach_best(const View &n, uint32_t max_reach) {
    const uint32_t tc = n.t(0, 0);
    const bool left = n.t(-1, 0) != 0, right = n.t(1, 0) != 0, up = n.t(0, -1) != 0, down = n.t(0, 1) != 0;
    uint32_t best = PWPP_REACH_UNREACHED;
    for (int k = 0; k < 8; ++k) {
        const int dx = pwpp_reach_dx(k), dy = pwpp_reach_dy(k);
        const uint32_t tn = n.t(dx, dy);
        if (tn == 0) continue;
        const bool corner = dx != 0 && dy != 0;
        if (corner && !((dx < 0 ? left : right) && (dy < 0 ? up : down))) continue;
        const uint32_t vn = n.v(dx, dy);
        if (vn == PWPP_REACH_UNREACHED) continue;
        const uint32_t cand = vn + pwpp_reach_step(tn, tc, corner);
        if (cand < best && (max_reach == 0 || cand <= max_reach)) best = cand;
    }
    return best;
}

// from of a centre with t > 0 and the final value vc != PWPP_REACH_UNREACHED that is not the source: the neighbour's k (0 .. 7), or -1 (a defect)
template <class View>
PWPP_HD inline int pwpp_reach_from(const View &n, uint32_t vc) {
    const uint32_t tc = n.t(0, 0);
    const bool left = n.t(-1, 0) != 0, right = n.t(1, 0) != 0, up = n.t(0, -1) != 0, down = n.t(0, 1) != 0;
    for (int k = 0; k < 8; ++k) {
        const int dx = pwpp_reach_dx(k), dy = pwpp_reach_dy(k);
        const uint32_t tn = n.t(dx, dy);
        if (tn == 0) continue;
        const bool corner = dx != 0 && dy != 0;
        if (corner && !((dx < 0 ? left : right) && (dy < 0 ? up : down))) continue;
        const uint32_t vn = n.v(dx, dy);
        if (vn != PWPP_REACH_UNREACHED && vn + pwpp_reach_step(tn, tc, corner) == vc) return k;
    }
    return -1;
}

// a frame's images in memory, clipped: what the global-memory kernels and the host read through
struct PwppReachImageView {
    const uint16_t *term;  // [ny][nx]
    const uint32_t *value;
    int nx, ny, x, y;
    PWPP_HD uint32_t t(int dx, int dy) const {
        const int gx = x + dx, gy = y + dy;
        return gx >= 0 && gx < nx && gy >= 0 && gy < ny ? term[(int64_t)gy * nx + gx] : 0u;
    }
    PWPP_HD uint32_t v(int dx, int dy) const { return value[(int64_t)(y + dy) * nx + (x + dx)]; }  // (after t(dx, dy) != 0)
};

#endif  // PWPP_REACH_H
