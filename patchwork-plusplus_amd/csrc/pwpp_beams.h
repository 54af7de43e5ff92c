// pwpp_beams.h -- the arithmetic of the per-beam free space (pwpp_beam_grid, pwpp_beam_ground), one text for the kernels
// (pwpp_beams.hip), for the host's pwpp_beam_height (pwpp_capi.cpp) and for the host program that deals the same walks against a
// brute force of its own (tools/beams_check.cpp).  Internal; include/pwpp.h has the contract.
//
// THE LINE is the visibility's own: pwpp_vis_line, pwpp_vis_step and pwpp_vis_jump of pwpp_visibility.h are called, the points
// P_k, k = 0 .. n, are theirs.  A beam that ended in the cell e = P_n CROSSES the interior points P_1 .. P_{n-1}: the origin's cell
// holds the vehicle, the endpoint's the return.  n <= 1: nothing is crossed.  Occupied cells do not stop a beam -- it returned.
//   rise      r = clamp(z - eye, -R, R) in 64 bits, R = 2^20 (pwpp_view_rise): the beam's height over the eye at its endpoint.
//   height    at P_k: eye + ceil(r * D / 2n), D = 2k - 1 where r < 0, else 2k + 1 -- the end of the cell's stretch of the beam,
//             half a step either side of P_k, where the beam is HIGHEST: an upper bound over the whole cell.  The division is exact.
//             |r| <= 2^20, D < 2n <= 2^16: every product stays below 2^37.  |ceil(..)| <= R, so with |eye| <= 2^30 the height
//             never leaves int32.  For fixed k and n it is non-decreasing in z: r is, and D changes only where r changes sign,
//             between ceil(-D / 2n) = 0 and 0.
//   range     a beam is traced for k <= max_range only (0: unlimited).  On the major axis the coordinate moves every step, so P_k has
//             the Chebyshev distance k from the origin: the cells beyond the range are exactly those no walk reaches.
//   a tile    the walk over the cells of a rectangle alone (pwpp_beams_walk_tile): on the major axis the coordinate of P_k is
//             o + sgn * k, so the k whose P_k can lie in the rectangle are an interval known in advance; pwpp_vis_jump lands on
//             its first point.  Both coordinates are monotone in k: once the line has left the rectangle it does not come back.
// WHAT A WALK TOUCHES.  P_k lies in the bounding rectangle of the origin and the endpoint, which lies in the image when both do;
// the sinks of the kernels compare every index with the image or the tile all the same before they form an address.
#ifndef PWPP_BEAMS_H
#define PWPP_BEAMS_H

#include <stdint.h>

#include "pwpp_viewshed.h"  // (and pwpp_visibility.h)

#define PWPP_BEAMS_EYE_MAX (1 << 30)  // |eye| beyond it: PWPP_E_ARG
#define PWPP_BEAMS_TILE 64            // path 2: a workgroup's tile is 64 x 64 cells, passes and low of it 32 KiB of LDS

// ceil(r * D / n2), exact, n2 > 0
PWPP_HD inline int32_t pwpp_beams_lift(int32_t r, uint32_t D, uint32_t n2) {
    const int64_t num = (int64_t)r * (int64_t)D, d = (int64_t)n2;
    return (int32_t)(num >= 0 ? (num + d - 1) / d : -((-num) / d));
}

// the height at P_k, 1 <= k < n, of a beam of rise r from an eye at `eye` (n2 = 2n)
PWPP_HD inline int32_t pwpp_beams_at(int32_t eye, int32_t r, uint32_t k, uint32_t n2) {
    return eye + pwpp_beams_lift(r, r < 0 ? 2u * k - 1u : 2u * k + 1u, n2);
}

// = pwpp_beam_height of include/pwpp.h
PWPP_HD inline int32_t pwpp_beams_height(int32_t eye, int32_t z, uint32_t k, uint32_t n) { return pwpp_beams_at(eye, pwpp_view_rise(z, eye), k, 2u * n); }

// whether a cell of the two images is an endpoint
PWPP_HD inline bool pwpp_beams_endpoint(int32_t hits, int32_t zmin) { return hits >= 1 && zmin != PWPP_VIEW_NONE_HEIGHT; }

// the last k a beam of n steps is traced at (0: none)
PWPP_HD inline uint32_t pwpp_beams_last(uint32_t n, int max_range) {
    const uint32_t last = n >= 1 ? n - 1u : 0u;
    return max_range > 0 && (uint32_t)max_range < last ? (uint32_t)max_range : last;
}

// The beam from o = (ox, oy) at `eye` into the endpoint cell e = (ex, ey) with height z, both inside the image:
// sink.cross(x, y, height) for every crossed cell.  The loop is bounded by n <= max(nx, ny).
template <class Sink>
PWPP_HD inline void pwpp_beams_walk(Sink &sink, int ox, int oy, int ex, int ey, int32_t eye, int32_t z, int max_range) {
    PwppVisLine L;
    pwpp_vis_line(ox, oy, ex, ey, L);
    const uint32_t last = pwpp_beams_last(L.n, max_range);
    const int32_t r = pwpp_view_rise(z, eye);
    for (uint32_t k = 1; k <= last; ++k) {
        pwpp_vis_step(L);
        sink.cross(L.x, L.y, pwpp_beams_at(eye, r, k, L.n2));
    }
}

// The k, k0 <= k <= k1, at which the beam L (as pwpp_vis_line left it, from o) can cross a cell of the rectangle [x0, x1] x [y0, y1]:
// those whose major coordinate o + sgn * k lies in it, among 1 .. last.  False: none -- the beam does not touch the rectangle.
PWPP_HD inline bool pwpp_beams_tile_span(const PwppVisLine &L, int max_range, int x0, int y0, int x1, int y1, uint32_t &k0, uint32_t &k1) {
    const uint32_t last = pwpp_beams_last(L.n, max_range);
    if (last == 0) return false;
    const bool xmajor = L.ax2 >= L.ay2;
    const int o = xmajor ? L.x : L.y, s = xmajor ? L.sx : L.sy, lo = xmajor ? x0 : y0, hi = xmajor ? x1 : y1;  // (n >= 2: s != 0)
    int64_t a = s > 0 ? (int64_t)lo - o : (int64_t)o - hi, b = s > 0 ? (int64_t)hi - o : (int64_t)o - lo;
    if (a < 1) a = 1;
    if (b > (int64_t)last) b = (int64_t)last;
    if (a > b) return false;
    k0 = (uint32_t)a, k1 = (uint32_t)b;
    return true;
}

// whether the bounding rectangle of o and e meets the rectangle [x0, x1] x [y0, y1] at all: the cheap test before a line is set up
PWPP_HD inline bool pwpp_beams_near_tile(int ox, int oy, int ex, int ey, int x0, int y0, int x1, int y1) {
    return !((ox < x0 && ex < x0) || (ox > x1 && ex > x1) || (oy < y0 && ey < y0) || (oy > y1 && ey > y1));
}

// The same beam over the cells of that rectangle alone: exactly the calls of pwpp_beams_walk whose (x, y) lie in it.
template <class Sink>
PWPP_HD inline void pwpp_beams_walk_tile(Sink &sink, int ox, int oy, int ex, int ey, int32_t eye, int32_t z, int max_range, int x0, int y0, int x1, int y1) {
    if (!pwpp_beams_near_tile(ox, oy, ex, ey, x0, y0, x1, y1)) return;
    PwppVisLine L;
    pwpp_vis_line(ox, oy, ex, ey, L);
    uint32_t k0, k1;
    if (!pwpp_beams_tile_span(L, max_range, x0, y0, x1, y1, k0, k1)) return;
    const int32_t r = pwpp_view_rise(z, eye);
    pwpp_vis_jump(L, k0);
    bool entered = false;
    for (uint32_t k = k0;; ++k) {
        if (L.x >= x0 && L.x <= x1 && L.y >= y0 && L.y <= y1) {
            entered = true;
            sink.cross(L.x, L.y, pwpp_beams_at(eye, r, k, L.n2));
        } else if (entered) {
            break;
        }
        if (k >= k1) break;
        pwpp_vis_step(L);
    }
}

// low as it is reported: no height where nothing passed
PWPP_HD inline int32_t pwpp_beams_low(uint32_t passes, int32_t low) { return passes == 0u ? PWPP_VIEW_NONE_HEIGHT : low; }

// The byte of a cell: free iff the base byte is unknown, enough beams passed and (with a target) the lowest of them cleared the
// target by no more than `clearance`; everywhere else the base byte, verbatim.  `low` as reported; has_target: a target image was given.
PWPP_HD inline int8_t pwpp_beams_occupancy(int8_t base, uint32_t passes, int32_t low, bool has_target, int32_t target, uint32_t min_pass, int32_t clearance) {
    if (base != (int8_t)PWPP_VIS_UNKNOWN || passes < min_pass) return base;
    if (has_target && (target == PWPP_VIEW_NONE_HEIGHT || (int64_t)low - (int64_t)target > (int64_t)clearance)) return base;
    return (int8_t)PWPP_VIS_FREE;
}

#endif
