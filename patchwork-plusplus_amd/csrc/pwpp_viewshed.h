// pwpp_viewshed.h -- the arithmetic of the height-aware line of sight (pwpp_viewshed_grid, pwpp_viewshed_obstacles), one text for
// the kernels (pwpp_visibility.hip), for the host side's quantiser and origins (pwpp_capi.cpp) and for the host program that deals
// the same pack and walk against a brute force of its own (tools/viewshed_check.cpp).  Internal; include/pwpp.h has the contract.
//
// THE WALK is the visibility's own: pwpp_vis_line and pwpp_vis_step of pwpp_visibility.h are called, the points P_k, the cells A
// and B of rule (a) and the bit image are theirs.  What is new is that an occupied cell on the line is a BLOCKER with a rise, not
// the end of the walk:
//   rise      r = clamp(block - eye, -R, R) in 64 bits, R = 2^20; an occupied cell without a height is OPAQUE (PWPP_VIEW_OPAQUE,
//             above every rise).  The target's rise t is the cell's own block where it is occupied, else its target height; no
//             height: minus infinity (PWPP_VIEW_BELOW, under every rise).
//   blockers  at step k, in this order: (a) both coordinates moved, A and B occupied: the gap between them, at D = 2k - 1, with the
//             smaller of the two rises and that cell's index (equal rises: the smaller index); (b) for k < n, P_k occupied: at
//             D = 2k with its own rise.  D counts half steps: the gap lies half a step before P_k.
//   hides     a blocker (r, D) hides the target iff it is opaque, or t is minus infinity, or r * 2n > t * D -- the ray from the
//             eye to the target, at rise t * D / 2n when it passes the blocker, goes through it.  Strict: a grazing ray sees.
//             |r|, |t| <= 2^20 and D <= 2n <= 2^16: every product stays below 2^38.
//   shadow    the lowest rise seen at the cell: max over the blockers of ceil(r * 2n / D), clamped to [-R, R + 1].
//             THEOREM: hidden iff t < that maximum.  t is an integer, so r * 2n > t * D  <=>  t < r * 2n / D  <=>  t < ceil(r * 2n / D);
//             the clamp changes neither side: t <= R < R + 1, and a value below -R hides no t >= -R, as -R itself does not.
// WHAT A WALK READS.  The occupancy of P_k, A and B through the accessor it is given (the bit image, its rows in LDS, or count
// itself); a height only of a cell that accessor called occupied, and of the target.  All lie in the bounding rectangle of o and
// c; every accessor compares the index with nx and ny all the same before it forms an address.
#ifndef PWPP_VIEWSHED_H
#define PWPP_VIEWSHED_H

#include <math.h>
#include <stdint.h>

#include "pwpp_visibility.h"

#define PWPP_VIEW_NONE_HEIGHT INT32_MIN   // = PWPP_VIEW_NO_HEIGHT of include/pwpp.h
#define PWPP_VIEW_RISE_MAX (1 << 20)      // = PWPP_VIEW_MAX_RISE
#define PWPP_VIEW_UNITS 1024              // = PWPP_VIEW_UNITS_PER_M
#define PWPP_VIEW_OPAQUE INT32_MAX        // the rise of an occupied cell without a height: above every rise
#define PWPP_VIEW_BELOW INT32_MIN         // the rise of a target without a height: under every rise

// ---- the quantiser: metres -> units.  NaN: no height.  One multiplication, one clamp, one addition, one floor, in double.
PWPP_HD inline int32_t pwpp_view_units(double metres) {
    if (metres != metres) return PWPP_VIEW_NONE_HEIGHT;
    double v = metres * (double)PWPP_VIEW_UNITS;
    const double lim = 1073741824.0;  // 2^30
    v = v < -lim ? -lim : (v > lim ? lim : v);
    return (int32_t)floor(v + 0.5);
}

// ---- rises ------------------------------------------------------------------------------------------------------------------------
PWPP_HD inline int32_t pwpp_view_rise(int32_t height, int32_t eye) {
    const int64_t d = (int64_t)height - (int64_t)eye;
    return (int32_t)(d < -(int64_t)PWPP_VIEW_RISE_MAX ? -(int64_t)PWPP_VIEW_RISE_MAX : (d > (int64_t)PWPP_VIEW_RISE_MAX ? (int64_t)PWPP_VIEW_RISE_MAX : d));
}

// The heights of one frame: at(x, y) of any cell -- outside the image, or without an image, there is no height and nothing is read.
struct PwppViewHeights {
    const int32_t *block, *target;  // cell 0 of the frame; either may be null
    int32_t nx, ny, eye;
    PWPP_HD inline int32_t height(const int32_t *img, int x, int y) const {
        if (!img || (unsigned)x >= (unsigned)nx || (unsigned)y >= (unsigned)ny) return PWPP_VIEW_NONE_HEIGHT;
        return img[(size_t)y * (size_t)nx + (size_t)x];
    }
    // the rise of an OCCUPIED cell as a blocker
    PWPP_HD inline int32_t blocker(int x, int y) const {
        const int32_t b = height(block, x, y);
        return b == PWPP_VIEW_NONE_HEIGHT ? PWPP_VIEW_OPAQUE : pwpp_view_rise(b, eye);
    }
    // the rise of a cell as a target: is its top seen where it is occupied, its ground where it is not
    PWPP_HD inline int32_t aim(int x, int y, bool occupied) const {
        const int32_t t = height(occupied ? block : target, x, y);
        return t == PWPP_VIEW_NONE_HEIGHT ? PWPP_VIEW_BELOW : pwpp_view_rise(t, eye);
    }
};

PWPP_HD inline bool pwpp_view_hides(int32_t r, uint32_t D, int32_t t, uint32_t n2) {
    return r == PWPP_VIEW_OPAQUE || t == PWPP_VIEW_BELOW || (int64_t)r * (int64_t)n2 > (int64_t)t * (int64_t)D;
}

// ceil(r * 2n / D), exact, D > 0
PWPP_HD inline int64_t pwpp_view_cast(int32_t r, uint32_t D, uint32_t n2) {
    const int64_t num = (int64_t)r * (int64_t)n2, d = (int64_t)D;
    return num >= 0 ? (num + d - 1) / d : -((-num) / d);
}

// what the walk has gathered of a line's blockers
struct PwppViewLine {
    int32_t first;   // the reported cell of the nearest blocker that hides; < 0: none yet
    bool any, dark;  // a blocker was met | an opaque one
    int32_t r;       // the steepest blocker that is not opaque, as the fraction r / D: ceil is monotone, so the largest
    uint32_t D;      // pwpp_view_cast is that of the largest r / D -- compared by cross products (< 2^37), divided once at the end.  D == 0: none yet
    // true: the walk may stop -- first is known and shadow is not wanted, or nothing further changes it
    PWPP_HD inline bool meet(int32_t r, uint32_t D, int32_t cell, int32_t t, uint32_t n2, bool want_shadow) {
        any = true;
        if (first < 0 && pwpp_view_hides(r, D, t, n2)) first = cell;
        if (r == PWPP_VIEW_OPAQUE) {
            dark = true;
            return true;  // (an opaque blocker hides: first is set, shadow is INT32_MAX whatever follows)
        }
        if (this->D == 0 || (int64_t)r * (int64_t)this->D > (int64_t)this->r * (int64_t)D) this->r = r, this->D = D;
        return first >= 0 && !want_shadow;
    }
};

// first and shadow of the cell c = (cx, cy) seen from o = (ox, oy) at height H.eye, both inside the image of nx columns.  Without
// want_shadow the walk stops at the first blocker that hides and `shadow` is not meaningful.  The loop is bounded by n <= max(nx, ny).
struct PwppViewResult {
    int32_t first, shadow;
};
template <class Occ>
PWPP_HD inline PwppViewResult pwpp_view_walk(const Occ &occ, const PwppViewHeights &H, int ox, int oy, int cx, int cy, int nx, int max_range, bool want_shadow) {
    PwppVisLine L;
    pwpp_vis_line(ox, oy, cx, cy, L);
    if (max_range > 0 && L.n > (uint32_t)max_range) return PwppViewResult{PWPP_VIS_FIRST_BEYOND, PWPP_VIEW_NONE_HEIGHT};
    const bool own = occ.at(cx, cy);
    const int32_t t = H.aim(cx, cy, own);
    PwppViewLine V{-1, false, false, 0, 0};
    for (uint32_t k = 1; k <= L.n; ++k) {
        const int px = L.x, py = L.y;
        if (pwpp_vis_step(L) && occ.at(px, L.y) && occ.at(L.x, py)) {  // (a): A = (x_{k-1}, y_k), B = (x_k, y_{k-1})
            const int32_t a = L.y * nx + px, b = py * nx + L.x;
            const int32_t ra = H.blocker(px, L.y), rb = H.blocker(L.x, py);
            const int32_t r = ra < rb ? ra : rb, cell = ra < rb ? a : (rb < ra ? b : (a < b ? a : b));
            if (V.meet(r, 2u * k - 1u, cell, t, L.n2, want_shadow)) break;
        }
        if (k < L.n && occ.at(L.x, L.y) && V.meet(H.blocker(L.x, L.y), 2u * k, L.y * nx + L.x, t, L.n2, want_shadow)) break;  // (b)
    }
    PwppViewResult res;
    res.first = V.first >= 0 ? V.first : (own ? cy * nx + cx : PWPP_VIS_FIRST_NONE);
    if (!V.any) {
        res.shadow = PWPP_VIEW_NONE_HEIGHT;
    } else if (V.dark) {
        res.shadow = INT32_MAX;
    } else {
        const int64_t lo = -(int64_t)PWPP_VIEW_RISE_MAX, hi = (int64_t)PWPP_VIEW_RISE_MAX + 1, cast = pwpp_view_cast(V.r, V.D, L.n2);
        const int64_t s = (int64_t)H.eye + (cast < lo ? lo : (cast > hi ? hi : cast));
        res.shadow = (int32_t)(s <= (int64_t)INT32_MIN ? (int64_t)INT32_MIN + 1 : (s >= (int64_t)INT32_MAX ? (int64_t)INT32_MAX - 1 : s));  // (|eye| beyond 2^31 - 2^20 - 2: saturated)
    }
    return res;
}

// the tri-state byte: occupied wherever the cell holds returns; free where a return came back from its ground (witnessed), or the
// line to it is clear or passes over everything on it; else unknown
PWPP_HD inline int8_t pwpp_view_occupancy(bool occupied, bool witnessed, int32_t first) {
    if (occupied) return (int8_t)PWPP_VIS_OCCUPIED;
    return witnessed || first == PWPP_VIS_FIRST_NONE ? (int8_t)PWPP_VIS_FREE : (int8_t)PWPP_VIS_UNKNOWN;
}

#endif
