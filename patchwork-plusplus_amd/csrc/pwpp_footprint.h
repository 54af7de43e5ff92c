// pwpp_footprint.h -- the arithmetic of the oriented vehicle footprint (pwpp_footprint_grid, pwpp_footprint_covers), one text for the
// kernels (pwpp_footprint.hip), for the host side (pwpp_capi.cpp) and for the host program that runs the same functions against a
// brute force of its own (tools/footprint_check.cpp), the way pwpp_route.h is one text for the routes.  Internal; include/pwpp.h
// has the contract.  Integers only: no angle, no square root, no floating point.
//
// TICKS.  A tick is 1/16 of a cell side (PWPP_FOOT_TICKS); cell (ix, iy) covers the ticks [16 ix, 16 ix + 16) in x and has its centre
// at q = (16 ix + 8, 16 iy + 8).  The cell of a tick is tick >> 4 with an arithmetic shift: the floor, for negative ticks too.
// THE POSE {px, py, ux, uy}: the reference point p in ticks, |px|, |py| <= 2^20; the heading u, any integer vector with |ux|, |uy| <=
// 1024; u == (0, 0) is no pose (SKIPPED).  THE FOOTPRINT is [-rear, front] along u and [-half_width, half_width] across it, each 0 ..
// PWPP_FOOT_EXTENT_MAX = 1024 ticks.
// COVERED.  With d = q - p, a = ux dx + uy dy, b = ux dy - uy dx, n2 = ux^2 + uy^2 (a / sqrt(n2) and b / sqrt(n2) are d's coordinates
// along and across u): a cell is covered iff (a >= 0 ? a^2 <= front^2 n2 : a^2 <= rear^2 n2) and b^2 <= half_width^2 n2; equality is
// inside.  Both sides scale with the square of |u|: only the direction of u matters.
// LEMMA 1 (the window).  A covered cell has max(|dx|, |dy|) <= E + W with E = max(front, rear), W = half_width.  Proof: with n =
// sqrt(n2), covered gives |a| <= E n and |b| <= W n.  (u, u') with u' = (-uy, ux) is an orthogonal basis of length n, so d = (a u +
// b u') / n2: dx = (a ux - b uy) / n2, dy = (a uy + b ux) / n2, and with |ux|, |uy| <= n: |dx|, |dy| <= (E n n + W n n) / n2 = E + W.
// The same equations give the rectangle's own bounding box: a covered centre is p + (s u + w u') / n with s in [-rear, front], w in
// [-W, W], so dx = (s ux - w uy) / n <= Sx / n with Sx = max(front ux, -rear ux) + W |uy| >= 0, and alike for -dx, dy, -dy (the support
// of the rectangle along the axes).  pwpp_foot_over_norm gives the smallest integer m with m^2 n2 >= S^2, that is ceil(S / n), by 12
// bisection steps in integers; m <= E + W.  A heading along an axis gets the rectangle itself: uy == 0 makes Sx / n = front or rear,
// Sy / n = W.  pwpp_foot_window returns the cells whose centre lies within those bounds of p where the E + W square has more than 5
// cells a side, and the E + W square below (for at most 25 cells the bisection would cost more than the cells it saves):
// never more than the E + W square, at most 257 x 257 = 66049 cells.  ONLY THAT WINDOW IS VISITED.  pwpp_foot_covers applies
// the E + W bound first, in 64 bits, so that it may be asked about any int cell: behind it |dx|, |dy| <= 2048, |a|, |b| <= 2 * 1024 *
// 2048 = 2^22, a^2, b^2 <= 2^44, n2 <= 2^21, front^2 n2 <= 2^41 -- every product stays below 2^45 (the bisection's too: S <= 2^21,
// S^2 <= 2^42, m < 4096, m^2 n2 <= 2^45).
// LEMMA 2 (the conservative check).  A footprint padded by 12 ticks on every side (front, rear and half_width each + 12) covers every
// cell that the unpadded rectangle touches at all.  Proof: a cell is the square of half-side 8 round q, so a point of it within the
// rectangle is at most 8 sqrt(2) < 11.32 from q; moving by less than 12 changes the coordinate along u and the one across u by
// less than 12 each, so q lies within the padded rectangle.  A caller who wants "no part of the vehicle over a blocked cell" pads
// by 12; who wants "the centre rule" does not.
// THE FOLD of a pose over its covered cells (PwppFootAcc): counts (covered, outside, blocked, unknown -- at most 66049 each), the
// largest term, the smallest dist2, the smallest index of a blocked cell.  Sums, a max and two mins: associative and commutative,
// so any deal of the window's cells to lanes and any order of the merges gives the same row (pwpp_foot_acc_merge).
// THE TRAJECTORY (PwppFootTraj) is the summary of a run of consecutive steps: its first HIT step, and over its steps that are not
// skipped and lie before that HIT the count, the largest k, max and sum of max_term, the sum of unknown, the min of min_dist2.
// pwpp_foot_traj_merge(A, B), A the earlier run: A where A has a hit, else A's sums folded with B's and B's hit.  Associative
// (three runs: the first hit of the whole is the first hit of the first run that has one, and only runs before it contribute), NOT
// commutative: an ordered pick.  The same bytes whatever the deal.  THE SUMS stay below 2^31: at most 4096 steps of max_term <= 355
// (below 2^21) and of unknown <= 66049 (270 536 704 < 2^31).  Nothing is summed over the image, so the range check of
// pwpp_reach_grid (14 (base + 100) (nx ny - 1)) is not needed here.
// THE DEALS.  A lane per pose walks its window row by row (path 1).  A wave per trajectory takes its steps in rounds of 64 / slot
// consecutive steps; a pose has a SLOT of 1, 2 .. 64 lanes, which take the cells i = c0, c0 + slot .. of its window, i -> (i mod w, i / w)
// by pwpp_foot_div (a multiplication by ceil(2^32 / w), exact for i < 2^17, w <= 257: the error of the quotient is i (w inv - 2^32) /
// (w 2^32) < i / 2^32 < 1 / w); the pose is folded over its slot's lanes, then the round's poses in step order (path 2).  What a pose
// costs a lane before its first cell (the edges, the window: some hundred operations) is paid by every lane of its slot, so the
// cheapest slot is the smallest that leaves no lane idle: pwpp_foot_slot gives 64 / min(64, n_steps rounded up to a power of two) --
// the cells are dealt to the lanes that the steps leave over.  Where no pose rows are asked for a wave may stop at the round of
// the first HIT; with windows of 64 x 64 cells and more (pwpp_foot_large) a round then has at most 8 steps: the setup is small
// beside such a window, and a trajectory that hits early costs one round, not all of them.  The slot changes no byte.
#ifndef PWPP_FOOTPRINT_H
#define PWPP_FOOTPRINT_H

#include <stdint.h>

#include "pwpp_reach.h"

#define PWPP_FOOT_TICKS 16          // = PWPP_FOOT_SUB of include/pwpp.h
#define PWPP_FOOT_EXTENT_MAX 1024   // = PWPP_FOOT_MAX_EXTENT
#define PWPP_FOOT_STEPS_MAX 4096    // = PWPP_FOOT_MAX_STEPS
#define PWPP_FOOT_TRAJ_MAX 65536
#define PWPP_FOOT_POSES_MAX ((int64_t)1 << 26)  // frames x n_traj x n_steps
#define PWPP_FOOT_P_MAX (1 << 20)
#define PWPP_FOOT_U_MAX 1024
#define PWPP_FOOT_STATUS_FREE 0     // = PWPP_FOOT_FREE, PWPP_FOOT_HIT, PWPP_FOOT_SKIPPED
#define PWPP_FOOT_STATUS_HIT 1
#define PWPP_FOOT_STATUS_SKIPPED 2
#define PWPP_FOOT_FLAG_OUTSIDE_BLOCKS 1  // = PWPP_FOOT_OUTSIDE_BLOCKS
#define PWPP_FOOT_NO_CELL 0x7fffffff     // `hit` and `first_hit` while none is known: above every index and every step

// the checked pwpp_footprint_params
struct PwppFootRule {
    int32_t front, rear, half_width, flags;
};
// pwpp_footprint_pose_row and pwpp_footprint_traj_row
struct PwppFootPoseRow {
    int32_t status, covered, outside, blocked, unknown, max_term, min_dist2, hit;
};
struct PwppFootTrajRow {
    int32_t first_hit, free_steps, last, max_term, sum_term, unknown, min_dist2, reach_last;
};
struct PwppFootPose {
    int32_t px, py, ux, uy;
};

PWPP_HD inline bool pwpp_foot_pose_in_range(const int32_t p[4]) {
    return p[0] >= -PWPP_FOOT_P_MAX && p[0] <= PWPP_FOOT_P_MAX && p[1] >= -PWPP_FOOT_P_MAX && p[1] <= PWPP_FOOT_P_MAX && p[2] >= -PWPP_FOOT_U_MAX &&
           p[2] <= PWPP_FOOT_U_MAX && p[3] >= -PWPP_FOOT_U_MAX && p[3] <= PWPP_FOOT_U_MAX;
}
PWPP_HD inline bool pwpp_foot_skipped(const PwppFootPose &p) { return p.ux == 0 && p.uy == 0; }

// What a pose fixes for all of its cells: the right sides of the coverage rule.
struct PwppFootEdges {
    int64_t front2, rear2, width2;  // front^2 n2, rear^2 n2, half_width^2 n2: at most 2^41
};
PWPP_HD inline PwppFootEdges pwpp_foot_edges(const PwppFootRule &F, const PwppFootPose &p) {
    const int64_t n2 = (int64_t)p.ux * p.ux + (int64_t)p.uy * p.uy;
    return PwppFootEdges{(int64_t)F.front * F.front * n2, (int64_t)F.rear * F.rear * n2, (int64_t)F.half_width * F.half_width * n2};
}
// COVERED for a cell of the pose's window: |dx|, |dy| <= 2048 (Lemma 1), so a and b fit 32 bits
PWPP_HD inline bool pwpp_foot_covers_near(const PwppFootEdges &e, const PwppFootPose &p, int32_t dx, int32_t dy) {
    const int64_t a = (int64_t)(p.ux * dx + p.uy * dy), b = (int64_t)(p.ux * dy - p.uy * dx);
    return a * a <= (a >= 0 ? e.front2 : e.rear2) && b * b <= e.width2;
}
// COVERED for any cell (ix, iy) of int range: Lemma 1's bound first, in 64 bits
PWPP_HD inline bool pwpp_foot_covers(const PwppFootRule &F, const PwppFootPose &p, int ix, int iy) {
    if (pwpp_foot_skipped(p)) return false;
    const int64_t dx = (int64_t)PWPP_FOOT_TICKS * ix + PWPP_FOOT_TICKS / 2 - p.px, dy = (int64_t)PWPP_FOOT_TICKS * iy + PWPP_FOOT_TICKS / 2 - p.py;
    const int64_t m = (F.front > F.rear ? F.front : F.rear) + F.half_width;
    if (dx > m || dx < -m || dy > m || dy < -m) return false;
    return pwpp_foot_covers_near(pwpp_foot_edges(F, p), p, (int32_t)dx, (int32_t)dy);
}

// the most cells a side of any window of the rule has: the centres 16 apart within an interval of 2 (E + W) ticks
PWPP_HD inline int32_t pwpp_foot_side_max(const PwppFootRule &F) { return 2 * ((F.front > F.rear ? F.front : F.rear) + F.half_width) / PWPP_FOOT_TICKS + 1; }
// ceil(S / sqrt(n2)) for 0 <= S <= 2^21, 1 <= n2 <= 2^21: the smallest m with m^2 n2 >= S^2
PWPP_HD inline int32_t pwpp_foot_over_norm(int32_t S, int64_t n2) {
    if (S <= 0) return 0;
    const int64_t S2 = (int64_t)S * S;
    int32_t r = 0;  // the largest r < 4096 with r^2 n2 < S^2
    for (int32_t b = 1 << 11; b; b >>= 1) {
        const int64_t c = r | b;
        if (c * c * n2 < S2) r = (int32_t)c;
    }
    return r + 1;
}
// THE WINDOW of a pose: the cells [x0, x0 + w) x [y0, y0 + h) whose centres lie within the bounds above of p; w or h may be 0.
struct PwppFootWindow {
    int32_t x0, y0, w, h;
};
PWPP_HD inline PwppFootWindow pwpp_foot_window(const PwppFootRule &F, const PwppFootPose &p) {
    const int32_t both = (F.front > F.rear ? F.front : F.rear) + F.half_width;
    int32_t xm = both, xp = both, ym = both, yp = both;  // how far a covered centre lies before and behind p
    if (pwpp_foot_side_max(F) > 5) {
        const int64_t n2 = (int64_t)p.ux * p.ux + (int64_t)p.uy * p.uy;
        const int32_t fx = F.front * p.ux, rx = F.rear * p.ux, fy = F.front * p.uy, ry = F.rear * p.uy;  // (at most 2^20 each)
        const int32_t wx = F.half_width * (p.uy < 0 ? -p.uy : p.uy), wy = F.half_width * (p.ux < 0 ? -p.ux : p.ux);
        xp = pwpp_foot_over_norm((fx > -rx ? fx : -rx) + wx, n2), xm = pwpp_foot_over_norm((-fx > rx ? -fx : rx) + wx, n2);
        yp = pwpp_foot_over_norm((fy > -ry ? fy : -ry) + wy, n2), ym = pwpp_foot_over_norm((-fy > ry ? -fy : ry) + wy, n2);
        xp = xp < both ? xp : both, xm = xm < both ? xm : both, yp = yp < both ? yp : both, ym = ym < both ? ym : both;
    }
    // 16 ix + 8 >= px - xm  <=>  ix >= ceil((px - xm - 8) / 16) = (px - xm + 7) >> 4;  16 ix + 8 <= px + xp  <=>  ix <= (px + xp - 8) >> 4
    PwppFootWindow w;
    w.x0 = (p.px - xm + 7) >> 4, w.y0 = (p.py - ym + 7) >> 4;
    w.w = ((p.px + xp - 8) >> 4) - w.x0 + 1, w.h = ((p.py + yp - 8) >> 4) - w.y0 + 1;
    return w;
}
// whether the rule's E + W square has 64 x 64 cells or more: where the wave's deal shortens its rounds, and what "footprint_path" 0 asks
PWPP_HD inline bool pwpp_foot_large(const PwppFootRule &F) { return pwpp_foot_side_max(F) >= 64; }
// THE SLOT of the wave's deal: the lanes a pose gets, 64 / the steps of a round (see THE DEALS above)
PWPP_HD inline int32_t pwpp_foot_slot(const PwppFootRule &F, int32_t n_steps, bool pose_rows) {
    int32_t per = 1;  // the steps of a round: n_steps rounded up to a power of two, at most 64
    while (per < 64 && per < n_steps) per <<= 1;
    if (!pose_rows && pwpp_foot_large(F) && per > 8) per = 8;
    return 64 / per;
}
// i / w for i < 2^17, 1 <= w <= 257, with inv = pwpp_foot_inv(w)
PWPP_HD inline uint32_t pwpp_foot_inv(uint32_t w) { return w <= 1 ? 0xffffffffu : (uint32_t)(((uint64_t)1 << 32) / w) + 1u; }  // (w inv - 2^32 is 1 .. w: the bound above)
PWPP_HD inline uint32_t pwpp_foot_div(uint32_t i, uint32_t w, uint32_t inv) { return w <= 1 ? i : (uint32_t)(((uint64_t)i * inv) >> 32); }

// A frame's images as a pose reads them (cost: [ny][nx] bytes; dist2, reach: null or the same shape).
struct PwppFootFrame {
    PwppReachRule R;
    const int8_t *cost;
    const int32_t *dist2;
    int32_t nx, ny;
};

// THE FOLD.
struct PwppFootAcc {
    int32_t covered, outside, blocked, unknown, max_term, min_dist2, hit;
};
PWPP_HD inline PwppFootAcc pwpp_foot_acc_none() { return PwppFootAcc{0, 0, 0, 0, 0, PWPP_REACH_DIST_BEYOND, PWPP_FOOT_NO_CELL}; }
PWPP_HD inline void pwpp_foot_acc_merge(PwppFootAcc &a, const PwppFootAcc &b) {
    a.covered += b.covered, a.outside += b.outside, a.blocked += b.blocked, a.unknown += b.unknown;
    a.max_term = a.max_term > b.max_term ? a.max_term : b.max_term;
    a.min_dist2 = a.min_dist2 < b.min_dist2 ? a.min_dist2 : b.min_dist2;
    a.hit = a.hit < b.hit ? a.hit : b.hit;
}
// one cell (ix, iy) of the window into the fold; no address is formed for a cell outside the image
PWPP_HD inline void pwpp_foot_cell(const PwppFootFrame &V, const PwppFootEdges &e, const PwppFootPose &p, int32_t ix, int32_t iy, PwppFootAcc &acc) {
    if (!pwpp_foot_covers_near(e, p, PWPP_FOOT_TICKS * ix + PWPP_FOOT_TICKS / 2 - p.px, PWPP_FOOT_TICKS * iy + PWPP_FOOT_TICKS / 2 - p.py)) return;
    ++acc.covered;
    if (ix < 0 || ix >= V.nx || iy < 0 || iy >= V.ny) {
        ++acc.outside;
        return;
    }
    const int32_t at = iy * V.nx + ix;  // (one frame's cells fit an int32: sides <= 32768 and the reach's image checks)
    const int c = V.cost[at];
    const int32_t d2 = V.dist2 ? V.dist2[at] : PWPP_REACH_DIST_BEYOND;
    const int32_t t = (int32_t)pwpp_reach_term(V.R, c, d2, false);
    if (c < 0) ++acc.unknown;
    if (t == 0) {
        ++acc.blocked;
        if (at < acc.hit) acc.hit = at;
    }
    if (t > acc.max_term) acc.max_term = t;
    if (d2 < acc.min_dist2) acc.min_dist2 = d2;
}
PWPP_HD inline PwppFootPoseRow pwpp_foot_row_skipped() {
    return PwppFootPoseRow{PWPP_FOOT_STATUS_SKIPPED, 0, 0, 0, 0, 0, PWPP_REACH_DIST_BEYOND, -1};
}
PWPP_HD inline PwppFootPoseRow pwpp_foot_row(const PwppFootRule &F, const PwppFootAcc &a) {
    const bool hit = a.blocked > 0 || (a.outside > 0 && (F.flags & PWPP_FOOT_FLAG_OUTSIDE_BLOCKS));
    return PwppFootPoseRow{hit ? PWPP_FOOT_STATUS_HIT : PWPP_FOOT_STATUS_FREE, a.covered, a.outside, a.blocked, a.unknown, a.max_term, a.min_dist2,
                           a.hit == PWPP_FOOT_NO_CELL ? -1 : a.hit};
}
// a pose's whole row, its window walked row by row: the serial deal (path 1, the host)
PWPP_HD inline PwppFootPoseRow pwpp_foot_pose_serial(const PwppFootFrame &V, const PwppFootRule &F, const PwppFootPose &p) {
    if (pwpp_foot_skipped(p)) return pwpp_foot_row_skipped();
    const PwppFootEdges e = pwpp_foot_edges(F, p);
    const PwppFootWindow w = pwpp_foot_window(F, p);
    PwppFootAcc acc = pwpp_foot_acc_none();
    for (int32_t y = 0; y < w.h; ++y)
        for (int32_t x = 0; x < w.w; ++x) pwpp_foot_cell(V, e, p, w.x0 + x, w.y0 + y, acc);
    return pwpp_foot_row(F, acc);
}

// THE TRAJECTORY.  `last` is -1 and first_hit PWPP_FOOT_NO_CELL while there is none.
struct PwppFootTraj {
    int32_t first_hit, free_steps, last, max_term, sum_term, unknown, min_dist2;
};
PWPP_HD inline PwppFootTraj pwpp_foot_traj_none() { return PwppFootTraj{PWPP_FOOT_NO_CELL, 0, -1, 0, 0, 0, PWPP_REACH_DIST_BEYOND}; }
// the summary of the one step k
PWPP_HD inline PwppFootTraj pwpp_foot_traj_of(const PwppFootPoseRow &r, int32_t k) {
    if (r.status == PWPP_FOOT_STATUS_SKIPPED) return pwpp_foot_traj_none();
    if (r.status == PWPP_FOOT_STATUS_HIT) {
        PwppFootTraj t = pwpp_foot_traj_none();
        t.first_hit = k;
        return t;
    }
    return PwppFootTraj{PWPP_FOOT_NO_CELL, 1, k, r.max_term, r.max_term, r.unknown, r.min_dist2};
}
// a <- a then b (b the later run)
PWPP_HD inline void pwpp_foot_traj_merge(PwppFootTraj &a, const PwppFootTraj &b) {
    if (a.first_hit != PWPP_FOOT_NO_CELL) return;
    a.first_hit = b.first_hit, a.free_steps += b.free_steps, a.sum_term += b.sum_term, a.unknown += b.unknown;
    a.last = a.last > b.last ? a.last : b.last;
    a.max_term = a.max_term > b.max_term ? a.max_term : b.max_term;
    a.min_dist2 = a.min_dist2 < b.min_dist2 ? a.min_dist2 : b.min_dist2;
}
// the row; `last_pose`: pose `last` (read only where last >= 0); reach: the frame's image or null
PWPP_HD inline PwppFootTrajRow pwpp_foot_traj_row(const PwppFootTraj &t, const int32_t *reach, int32_t nx, int32_t ny, const PwppFootPose *last_pose) {
    int32_t rl = (int32_t)PWPP_REACH_UNREACHED;
    if (reach && t.last >= 0) {
        const int32_t cx = last_pose->px >> 4, cy = last_pose->py >> 4;  // (arithmetic: the floor)
        if (cx >= 0 && cx < nx && cy >= 0 && cy < ny) rl = reach[cy * nx + cx];
    }
    return PwppFootTrajRow{t.first_hit == PWPP_FOOT_NO_CELL ? -1 : t.first_hit, t.free_steps, t.last, t.max_term, t.sum_term, t.unknown, t.min_dist2, rl};
}

#endif  // PWPP_FOOTPRINT_H
