// pwpp_hull.h -- the arithmetic of the obstacle hulls (pwpp_hull_obstacles, pwpp_hull_points), one text for the kernels (the point
// passes k_hull_extremes / k_hull_candidates in pwpp_kernels.hip, the row kernels in pwpp_hull.hip), for the host function
// pwpp_hull_points and for the host program that runs the same functions against a brute force of its own (tools/hull_check.cpp), the
// way pwpp_boxes.h is one text for the boxes.  Internal; include/pwpp.h has the contract.  Integers first; six floats derived once.
//
// POINTS.  A point is the pair (qx, qy) of pwpp_box_quantise, 0 <= q <= QMAX = 2^20 + 1, packed as (qy << 32) | qx: the order of the
// packed words IS the order (qy, qx) of the contract.
// CROSS.  cross(a, b, c) = (bx - ax)(cy - ay) - (by - ay)(cx - ax): every difference is at most QMAX in size, each product at most
// QMAX^2 < 2^40 + 2^22, so |cross| < 2^41 + 2^23 < 2^43: exact in int64.  A squared distance is at most 2 QMAX^2 < 2^41 + 2^23 = D2MAX.
// NEXT VERTEX.  From a vertex c of the strict hull every other distinct point lies in a half plane through c that is closed on one
// side only (c is a corner, or an end of a collinear set), so "b beats a iff cross(c, a, b) < 0, or cross == 0 and b is farther
// from c" is a TOTAL order on the points other than c, and its maximum is the next vertex counter-clockwise: the point with all
// others on its left or behind it on the same ray.  c itself (a duplicate among the candidates, or the initial value of a search)
// has distance 0 and cross 0 against everything: it loses to every other point and beats none.  A maximum under a total order does
// not depend on how the candidates are dealt or in which order partial maxima are merged (pwpp_hull_beats is all a deal needs).
// THE MARCH starts at the smallest packed word, takes next vertices until the start comes back, and has taken every strict vertex
// once, in counter-clockwise order: 1 vertex for one distinct point, 2 for a collinear set (the largest word is its far end).
// THE OCTAGON.  The eight points of a row that are extreme along (0,-1), (1,-1), (1,0), (1,1), (0,1), (-1,1), (-1,0), (-1,-1) -- in
// this order -- are points of the hull's boundary in counter-clockwise order (the support point turns with the direction; a tie
// picks some point of a hull edge), so they are the corners, some repeated or collinear, of a convex polygon inside the hull.  A
// point with cross > 0 against every edge between two DIFFERENT corners -- and there must be such an edge -- lies strictly inside
// that polygon, hence strictly inside the hull: no vertex.  A polygon without area has two opposite edges on one line, and no
// point is strictly left of both.  Dropping such points changes no row; what is left are the CANDIDATES.
// THE KEYS of those eight points: proj << 42 | qx << 21 | qy with proj = qx, qy, qx + qy, qx - qy + 2^21 (each below 2^22), a 64-bit
// minimum and maximum of each.  Minima and maxima commute: the octagon is a function of the row's set of points.
// SHOELACE.  area2 = the sum over the edges (a, b) of ax by - bx ay, accumulated along the march: every partial sum is twice the
// signed area of a polygon inside the square of side QMAX, at most 2 QMAX^2 < 2^42 in size.
// THE RECTANGLE of edge direction e (normalised to ex > 0, or ex == 0 and ey > 0; |ex|, |ey| <= QMAX): p = ex vx + ey vy and q = ex vy -
// ey vx are at most 2 QMAX^2 < 2^41 + 2^23 in size; W = pmax - pmin and H = qmax - qmin are diam * L times a cosine each (L = |e|, diam
// the set's diameter), so W H <= diam^2 L2, and L2 <= diam^2 <= D2MAX.  Edge i is better than edge j iff W_i H_i L2_j < W_j H_j L2_i
// (its area W H / L2 is smaller): both sides are at most diam^2 L2_i L2_j <= D2MAX^3 < (2^41 + 2^23)^3 < 2^124: exact in unsigned 128-bit
// integers, W H itself below 2^83.  The centre: U = (pmin + pmax) ex - (qmin + qmax) ey, V = (pmin + pmax) ey + (qmin + qmax) ex,
// below 2^66 in size: 128-bit integers, rounded once (pwpp_box_i128_to_double); the centre is (U, V) / (2 L2) on the 1/1024 m grid.
// THE DEALS.  A lane per row marches and then tries every edge, serially (pwpp_hull_row_serial: path 1, and pwpp_hull_points).  A
// wave per row sweeps the candidates with 64 lanes per march step and merges the lanes' maxima, keeps the hull in LDS, then deals
// the edges to its lanes and merges their best (path 2).  The same functions, the same bytes.
#ifndef PWPP_HULL_H
#define PWPP_HULL_H

#include <stdint.h>

#include "pwpp_boxes.h"  // PWPP_HD, pwpp_box_i128_to_double

#define PWPP_HULL_QMAX ((1 << 20) + 1)
#define PWPP_HULL_MAX_VERTICES 1024  // = the limit of max_vertices in include/pwpp.h; the LDS of a wave of path 2 holds as many
#define PWPP_HULL_ROW_WORDS 16       // pwpp_obstacle_hull
// The accumulators of one row in the handle's cluster buffer: 20 words, 8-byte aligned.
//   words 0..15   eight 64-bit keys: {min, max} of the keys of qx, qy, qx + qy, qx - qy     (first pass)
//   word 16       points: the counted points that named the row                             (first pass)
//   word 17       first entry of the row's candidates in its frame's part of the arena      (k_hull_offsets: exclusive scan of `points`)
//   word 18       candidates written                                                        (second pass)
//   word 19       0
#define PWPP_HULL_ACC_WORDS 20
#define PWPP_HULL_ACC_POINTS 16
#define PWPP_HULL_ACC_FIRST 17
#define PWPP_HULL_ACC_CANDS 18
#define PWPP_HULL_KEY_NO_MIN 0xffffffffffffffffull
#define PWPP_HULL_KEY_NO_MAX 0ull

typedef unsigned long long pwpp_hull_pt;

PWPP_HD inline pwpp_hull_pt pwpp_hull_pack(long long qx, long long qy) { return ((unsigned long long)qy << 32) | (unsigned long long)qx; }
PWPP_HD inline int32_t pwpp_hull_x(pwpp_hull_pt p) { return (int32_t)(uint32_t)p; }
PWPP_HD inline int32_t pwpp_hull_y(pwpp_hull_pt p) { return (int32_t)(uint32_t)(p >> 32); }

PWPP_HD inline long long pwpp_hull_cross(pwpp_hull_pt a, pwpp_hull_pt b, pwpp_hull_pt c) {
    const int32_t ax = pwpp_hull_x(a), ay = pwpp_hull_y(a);
    return (long long)(pwpp_hull_x(b) - ax) * (long long)(pwpp_hull_y(c) - ay) - (long long)(pwpp_hull_y(b) - ay) * (long long)(pwpp_hull_x(c) - ax);
}
PWPP_HD inline long long pwpp_hull_dist2(pwpp_hull_pt a, pwpp_hull_pt b) {
    const long long dx = pwpp_hull_x(b) - pwpp_hull_x(a), dy = pwpp_hull_y(b) - pwpp_hull_y(a);
    return dx * dx + dy * dy;
}
// from the vertex c: does candidate b beat candidate a?
PWPP_HD inline bool pwpp_hull_beats(pwpp_hull_pt c, pwpp_hull_pt a, pwpp_hull_pt b) {
    const long long x = pwpp_hull_cross(c, a, b);
    return x < 0 || (x == 0 && pwpp_hull_dist2(c, b) > pwpp_hull_dist2(c, a));
}
PWPP_HD inline long long pwpp_hull_shoelace(pwpp_hull_pt a, pwpp_hull_pt b) {
    return (long long)pwpp_hull_x(a) * (long long)pwpp_hull_y(b) - (long long)pwpp_hull_x(b) * (long long)pwpp_hull_y(a);
}

// the four keys of a point (minimum and maximum of each are kept per row)
PWPP_HD inline void pwpp_hull_keys(long long qx, long long qy, unsigned long long *k) {
    const unsigned long long low = ((unsigned long long)qx << 21) | (unsigned long long)qy;
    k[0] = ((unsigned long long)qx << 42) | low;
    k[1] = ((unsigned long long)qy << 42) | low;
    k[2] = ((unsigned long long)(qx + qy) << 42) | low;
    k[3] = ((unsigned long long)(qx - qy + (1 << 21)) << 42) | low;
}
PWPP_HD inline pwpp_hull_pt pwpp_hull_key_point(unsigned long long key) { return pwpp_hull_pack((long long)((key >> 21) & 0x1fffffull), (long long)(key & 0x1fffffull)); }

// one edge of the octagon, from corner a to the corner of `key`; a becomes that corner
PWPP_HD inline void pwpp_hull_octagon_edge(pwpp_hull_pt &a, unsigned long long key, pwpp_hull_pt p, bool &any, bool &inside) {
    const pwpp_hull_pt b = pwpp_hull_key_point(key);
    if (b != a) {
        any = true;
        inside = inside && pwpp_hull_cross(a, b, p) > 0;
    }
    a = b;
}
// keys: the row's eight ({min, max} of the four).  True: p is strictly inside the octagon, no vertex of the hull.
PWPP_HD inline bool pwpp_hull_inside_octagon(const unsigned long long *keys, pwpp_hull_pt p) {
    // counter-clockwise from (0,-1): min qy, max qx - qy, max qx, max qx + qy, max qy, min qx - qy, min qx, min qx + qy, and round
    pwpp_hull_pt a = pwpp_hull_key_point(keys[2]);
    bool any = false, inside = true;
    pwpp_hull_octagon_edge(a, keys[7], p, any, inside);
    pwpp_hull_octagon_edge(a, keys[1], p, any, inside);
    pwpp_hull_octagon_edge(a, keys[5], p, any, inside);
    pwpp_hull_octagon_edge(a, keys[3], p, any, inside);
    pwpp_hull_octagon_edge(a, keys[6], p, any, inside);
    pwpp_hull_octagon_edge(a, keys[0], p, any, inside);
    pwpp_hull_octagon_edge(a, keys[4], p, any, inside);
    pwpp_hull_octagon_edge(a, keys[2], p, any, inside);
    return any && inside;
}

// ---- the rectangle of one edge direction ------------------------------------------------------------------------------------------
struct PwppHullEdge {
    long long ex, ey, pmin, pmax, qmin, qmax;
    unsigned long long L2;
    unsigned __int128 WH;
    int i;  // the edge; -1: none
};
// v: n vertices as {qx, qy} pairs.  The rectangle of edge i (vertex i to vertex i + 1 mod n; n == 1: the direction (1, 0)).
PWPP_HD inline PwppHullEdge pwpp_hull_edge_of(const int32_t *v, int n, int i) {
    PwppHullEdge E;
    const int j = i + 1 < n ? i + 1 : 0;
    long long ex = (long long)v[2 * j] - (long long)v[2 * i], ey = (long long)v[2 * j + 1] - (long long)v[2 * i + 1];
    if (n == 1) ex = 1, ey = 0;
    if (ex < 0 || (ex == 0 && ey < 0)) ex = -ex, ey = -ey;
    E.ex = ex, E.ey = ey, E.i = i;
    E.pmin = E.qmin = INT64_MAX, E.pmax = E.qmax = INT64_MIN;
    for (int k = 0; k < n; ++k) {
        const long long vx = v[2 * k], vy = v[2 * k + 1];
        const long long p = ex * vx + ey * vy, q = ex * vy - ey * vx;
        E.pmin = p < E.pmin ? p : E.pmin, E.pmax = p > E.pmax ? p : E.pmax;
        E.qmin = q < E.qmin ? q : E.qmin, E.qmax = q > E.qmax ? q : E.qmax;
    }
    E.L2 = (unsigned long long)(ex * ex + ey * ey);
    E.WH = (unsigned __int128)(unsigned long long)(E.pmax - E.pmin) * (unsigned __int128)(unsigned long long)(E.qmax - E.qmin);
    return E;
}
// is the rectangle of a smaller than that of b?  (W_a H_a / L2_a < W_b H_b / L2_b, exactly)
PWPP_HD inline bool pwpp_hull_edge_smaller(unsigned __int128 WHa, unsigned long long L2a, unsigned __int128 WHb, unsigned long long L2b) {
    return WHa * (unsigned __int128)L2b < WHb * (unsigned __int128)L2a;
}
// does b take a's place as the best edge?  Ties go to the lower edge; an edge beats none (i < 0).
PWPP_HD inline bool pwpp_hull_edge_takes(unsigned __int128 WHa, unsigned long long L2a, int ia, unsigned __int128 WHb, unsigned long long L2b, int ib) {
    if (ib < 0) return false;
    if (ia < 0) return true;
    if (pwpp_hull_edge_smaller(WHb, L2b, WHa, L2a)) return true;
    return !pwpp_hull_edge_smaller(WHa, L2a, WHb, L2b) && ib < ia;
}
// the six floats of the chosen edge: cx, cy, ax, ay, length, width
PWPP_HD inline void pwpp_hull_rect_floats(const PwppHullEdge &E, double x0, double y0, float *f) {
    const double L = sqrt((double)E.L2);
    f[2] = (float)((double)E.ex / L), f[3] = (float)((double)E.ey / L);
    f[4] = (float)(((double)(E.pmax - E.pmin) / L) / 1024.0);
    f[5] = (float)(((double)(E.qmax - E.qmin) / L) / 1024.0);
    const __int128 ps = (__int128)(E.pmin + E.pmax), qs = (__int128)(E.qmin + E.qmax);
    const double u = pwpp_box_i128_to_double(ps * (__int128)E.ex - qs * (__int128)E.ey);
    const double v = pwpp_box_i128_to_double(ps * (__int128)E.ey + qs * (__int128)E.ex);
    const double d = 2.0 * (double)E.L2;
    f[0] = (float)(x0 + (u / d) / 1024.0);
    f[1] = (float)(y0 + (v / d) / 1024.0);
}

// ---- a finished row as its sixteen 4-byte words (pwpp_obstacle_hull) --------------------------------------------------------------
// What the march leaves of a row; the four bounds are those of its vertices, which are those of its points.
struct PwppHullMarch {
    int32_t n, stored, qx_min, qx_max, qy_min, qy_max;
    long long area2;
};
PWPP_HD inline void pwpp_hull_march_begin(PwppHullMarch &M) {
    M.n = M.stored = 0, M.area2 = 0;
    M.qx_min = M.qy_min = INT32_MAX, M.qx_max = M.qy_max = INT32_MIN;
}
// vertex v follows vertex `prev` (the first vertex: prev == v, a term of 0)
PWPP_HD inline void pwpp_hull_march_add(PwppHullMarch &M, pwpp_hull_pt prev, pwpp_hull_pt v) {
    const int32_t x = pwpp_hull_x(v), y = pwpp_hull_y(v);
    M.n += 1;
    M.area2 += pwpp_hull_shoelace(prev, v);
    M.qx_min = x < M.qx_min ? x : M.qx_min, M.qx_max = x > M.qx_max ? x : M.qx_max;
    M.qy_min = y < M.qy_min ? y : M.qy_min, M.qy_max = y > M.qy_max ? y : M.qy_max;
}
// E: the chosen edge; E.i < 0: none (a truncated row).  points == 0: the empty row, whatever else is given.
PWPP_HD inline void pwpp_hull_row(int32_t points, const PwppHullMarch &M, const PwppHullEdge *E, double x0, double y0, uint32_t *out) {
    if (points <= 0) {
        for (int k = 0; k < 10; ++k) out[k] = 0u;
        out[3] = 0xffffffffu;
        for (int k = 10; k < 16; ++k) out[k] = 0x7fc00000u;
        return;
    }
    out[0] = (uint32_t)points, out[1] = (uint32_t)M.n, out[2] = (uint32_t)M.stored, out[3] = (uint32_t)(E ? E->i : -1);
    out[4] = (uint32_t)(unsigned long long)M.area2, out[5] = (uint32_t)((unsigned long long)M.area2 >> 32);
    out[6] = (uint32_t)M.qx_min, out[7] = (uint32_t)M.qx_max, out[8] = (uint32_t)M.qy_min, out[9] = (uint32_t)M.qy_max;
    if (!E || E->i < 0) {
        out[3] = 0xffffffffu;
        for (int k = 10; k < 16; ++k) out[k] = 0x7fc00000u;
        return;
    }
    float f[6];
    pwpp_hull_rect_floats(*E, x0, y0, f);
    for (int k = 0; k < 6; ++k) out[10 + k] = __builtin_bit_cast(uint32_t, f[k]);
}

// ---- the serial deal: a lane (or the host) per row --------------------------------------------------------------------------------
// cand: the row's candidates, any order, duplicates allowed, every strict vertex among them; verts: room for max_vertices {qx, qy}
// pairs, the first min(n_vertices, max_vertices) written.  out: the row's sixteen words.
PWPP_HD inline void pwpp_hull_row_serial(const pwpp_hull_pt *cand, int64_t n_cand, int32_t points, int max_vertices, int32_t *verts, double x0, double y0,
                                         uint32_t *out) {
    PwppHullMarch M;
    pwpp_hull_march_begin(M);
    if (points <= 0 || n_cand <= 0) {
        pwpp_hull_row(0, M, nullptr, x0, y0, out);
        return;
    }
    pwpp_hull_pt start = cand[0];
    for (int64_t k = 1; k < n_cand; ++k) start = cand[k] < start ? cand[k] : start;
    pwpp_hull_pt c = start, prev = start;
    for (int64_t step = 0; step < n_cand; ++step) {  // (a hull has at most n_cand vertices)
        pwpp_hull_march_add(M, prev, c);
        if (M.n <= max_vertices) verts[2 * (M.n - 1)] = pwpp_hull_x(c), verts[2 * (M.n - 1) + 1] = pwpp_hull_y(c), M.stored = M.n;
        pwpp_hull_pt best = c;
        for (int64_t k = 0; k < n_cand; ++k) best = pwpp_hull_beats(c, best, cand[k]) ? cand[k] : best;
        prev = c, c = best;
        if (c == start) break;
    }
    M.area2 += pwpp_hull_shoelace(prev, start);  // (the closing edge; 0 for one vertex)
    if (M.n > max_vertices) {
        pwpp_hull_row(points, M, nullptr, x0, y0, out);
        return;
    }
    PwppHullEdge best = pwpp_hull_edge_of(verts, M.n, 0);
    for (int i = 1; i < M.n; ++i) {
        const PwppHullEdge E = pwpp_hull_edge_of(verts, M.n, i);
        if (pwpp_hull_edge_takes(best.WH, best.L2, best.i, E.WH, E.L2, E.i)) best = E;
    }
    pwpp_hull_row(points, M, &best, x0, y0, out);
}

// What option "hulls_path" = 0 means for a call of `rows` rows: 1 a lane per row, 2 a wave per row.  Decided by
// tools/obstacle_hulls_cost.py (profiles/obstacle_hulls_cost.txt), not in advance.
inline int pwpp_hull_path_of(int path, int64_t rows) {
    (void)rows;
    return path == 0 ? 2 : path;
}

#endif
