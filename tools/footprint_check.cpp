// footprint_check.cpp -- the functions of csrc/pwpp_footprint.h run on the host, dealt as each kernel of pwpp_footprint.hip deals them,
// against a brute force of its own.  A stand-alone program with its own main; tests/test_footprint_cpu.py builds it with
// -fsanitize=address,undefined and runs it as a plain executable.
//
//   deal 1  (k_foot_poses, k_foot_trajs) pwpp_foot_pose_serial per pose, its row stored; then per trajectory the rows merged in step
//           order up to the first HIT.
//   deal 2  (k_foot_waves) per trajectory 64 lanes in rounds of 64 / slot steps (pwpp_foot_slot): lane l has the pose of step k0 + l / slot
//           and the cells c0 = l % slot, c0 + slot .. of its window through pwpp_foot_div; the fold crosses the slot by the butterfly
//           acc[l] <- merge(acc[l], acc[l ^ off]), off = 1 .. slot / 2; the round's steps by the ordered butterfly off = slot .. 32
//           (the lower block first); without pose rows the rounds end at the first HIT.  That all 64 lanes end a round with the same
//           summary is checked for every round.
// The brute force shares no code with the header: the coverage rule written out again in __int128, asked of EVERY cell of the image
// and of every cell within the rectangle's diagonal of p (an integer square root of front^2 .. + half_width^2, not Lemma 1's bound),
// the row and the free prefix by their definitions.
// Also: pwpp_foot_div against / for every w 1 .. 257 and i < 2^17; Lemma 1 and the visited window on random poses over a domain of
// 150 cells round p; pwpp_foot_traj_merge's associativity on random triples.
//
//   footprint_check                      the random cases; prints "footprint_check: N cases, M mismatches ..."
//   footprint_check dump COST NX NY FRAMES BASE LETHAL UNKNOWN CLEARANCE2 DIST2|- REACH|- FRONT REAR HALF_WIDTH FLAGS POSES N_SETS N_TRAJ
//                   N_STEPS DEAL WANT_POSE_ROWS OUT     raw files in, OUT.pose (where wanted) and OUT.traj out; prints the time of the fold
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "pwpp_footprint.h"

namespace {

struct Case {
    PwppReachRule R;
    PwppFootRule F;
    int nx, ny, frames, n_sets, n_traj, n_steps;
    std::vector<int8_t> cost;
    std::vector<int32_t> dist2, reach;  // empty: none
    std::vector<PwppFootPose> poses;
};
struct Rows {
    std::vector<PwppFootPoseRow> pose;  // frames x n_traj x n_steps
    std::vector<PwppFootTrajRow> traj;
};

PwppFootFrame frame_of(const Case &c, int f) {
    const size_t base = (size_t)f * (size_t)c.nx * (size_t)c.ny;
    return PwppFootFrame{c.R, c.cost.data() + base, c.dist2.empty() ? nullptr : c.dist2.data() + base, c.nx, c.ny};
}
const PwppFootPose *poses_of(const Case &c, int f, int j) { return c.poses.data() + ((size_t)(c.n_sets > 1 ? f : 0) * (size_t)c.n_traj + (size_t)j) * (size_t)c.n_steps; }
const int32_t *reach_of(const Case &c, int f) { return c.reach.empty() ? nullptr : c.reach.data() + (size_t)f * (size_t)c.nx * (size_t)c.ny; }

const PwppFootPoseRow kUntouched{-7, -7, -7, -7, -7, -7, -7, -7};

void deal_lanes(const Case &c, Rows &out) {
    const size_t trajs = (size_t)c.frames * (size_t)c.n_traj;
    out.pose.assign(trajs * (size_t)c.n_steps, kUntouched), out.traj.resize(trajs);
    for (size_t id = 0; id < out.pose.size(); ++id) {
        const size_t t = id / (size_t)c.n_steps;
        const int k = (int)(id - t * (size_t)c.n_steps), f = (int)(t / (size_t)c.n_traj), j = (int)(t % (size_t)c.n_traj);
        out.pose[id] = pwpp_foot_pose_serial(frame_of(c, f), c.F, poses_of(c, f, j)[k]);
    }
    for (size_t t = 0; t < trajs; ++t) {
        const int f = (int)(t / (size_t)c.n_traj), j = (int)(t % (size_t)c.n_traj);
        PwppFootTraj T = pwpp_foot_traj_none();
        for (int k = 0; k < c.n_steps && T.first_hit == PWPP_FOOT_NO_CELL; ++k) pwpp_foot_traj_merge(T, pwpp_foot_traj_of(out.pose[t * (size_t)c.n_steps + (size_t)k], k));
        PwppFootPose last{0, 0, 0, 0};
        if (T.last >= 0) last = poses_of(c, f, j)[T.last];
        out.traj[t] = pwpp_foot_traj_row(T, reach_of(c, f), c.nx, c.ny, &last);
    }
}

long g_slot_overflows = 0, g_packed_rounds = 0, g_early_exits = 0;

void deal_waves(const Case &c, bool want_pose, Rows &out) {
    const size_t trajs = (size_t)c.frames * (size_t)c.n_traj;
    out.pose.assign(want_pose ? trajs * (size_t)c.n_steps : 0, kUntouched), out.traj.resize(trajs);
    const int slot = pwpp_foot_slot(c.F, c.n_steps, want_pose), per = 64 / slot;
    for (size_t t = 0; t < trajs; ++t) {
        const int f = (int)(t / (size_t)c.n_traj), j = (int)(t % (size_t)c.n_traj);
        const PwppFootFrame V = frame_of(c, f);
        const PwppFootPose *P = poses_of(c, f, j);
        PwppFootTraj T = pwpp_foot_traj_none();
        for (int k0 = 0; k0 < c.n_steps; k0 += per) {
            PwppFootAcc acc[64];
            PwppFootTraj r[64];
            bool skipped[64], valid[64];
            if (per > 1) ++g_packed_rounds;
            for (int lane = 0; lane < 64; ++lane) {
                const int sub = lane / slot, c0 = lane % slot, k = k0 + sub;
                valid[lane] = k < c.n_steps;
                const PwppFootPose p = valid[lane] ? P[k] : PwppFootPose{0, 0, 0, 0};
                skipped[lane] = pwpp_foot_skipped(p);
                acc[lane] = pwpp_foot_acc_none();
                if (skipped[lane]) continue;
                const PwppFootEdges e = pwpp_foot_edges(c.F, p);
                const PwppFootWindow w = pwpp_foot_window(c.F, p);
                const uint32_t n = (uint32_t)(w.w * w.h), inv = pwpp_foot_inv((uint32_t)w.w);
                for (uint32_t i = (uint32_t)c0; i < n; i += (uint32_t)slot) {
                    const uint32_t y = pwpp_foot_div(i, (uint32_t)w.w, inv), x = i - y * (uint32_t)w.w;
                    pwpp_foot_cell(V, e, p, w.x0 + (int32_t)x, w.y0 + (int32_t)y, acc[lane]);
                }
            }
            for (int off = 1; off < slot; off <<= 1) {
                PwppFootAcc was[64];
                std::memcpy(was, acc, sizeof(acc));
                for (int lane = 0; lane < 64; ++lane) pwpp_foot_acc_merge(acc[lane], was[lane ^ off]);
            }
            for (int lane = 0; lane < 64; ++lane) {
                const int k = k0 + lane / slot;
                const PwppFootPoseRow row = skipped[lane] ? pwpp_foot_row_skipped() : pwpp_foot_row(c.F, acc[lane]);
                if (want_pose && valid[lane] && lane % slot == 0) out.pose[t * (size_t)c.n_steps + (size_t)k] = row;
                r[lane] = valid[lane] ? pwpp_foot_traj_of(row, k) : pwpp_foot_traj_none();
            }
            for (int off = slot; off < 64; off <<= 1) {
                PwppFootTraj was[64];
                std::memcpy(was, r, sizeof(r));
                for (int lane = 0; lane < 64; ++lane) {
                    if (lane & off) {
                        PwppFootTraj first = was[lane ^ off];
                        pwpp_foot_traj_merge(first, was[lane]);
                        r[lane] = first;
                    } else {
                        pwpp_foot_traj_merge(r[lane], was[lane ^ off]);
                    }
                }
            }
            for (int lane = 1; lane < 64; ++lane)
                if (std::memcmp(&r[lane], &r[0], sizeof(r[0])) != 0) ++g_slot_overflows;  // (the wave's lanes must agree: a defect of the deal otherwise)
            pwpp_foot_traj_merge(T, r[0]);
            if (!want_pose && T.first_hit != PWPP_FOOT_NO_CELL) {
                if (k0 + per < c.n_steps) ++g_early_exits;
                break;
            }
        }
        PwppFootPose last{0, 0, 0, 0};
        if (T.last >= 0) last = P[T.last];
        out.traj[t] = pwpp_foot_traj_row(T, reach_of(c, f), c.nx, c.ny, &last);
    }
}

// ---- the brute force -------------------------------------------------------------------------------------------------------------
bool brute_covers(const PwppFootRule &F, const PwppFootPose &p, long ix, long iy) {
    const __int128 dx = 16 * (__int128)ix + 8 - p.px, dy = 16 * (__int128)iy + 8 - p.py;
    const __int128 a = p.ux * dx + p.uy * dy, b = p.ux * dy - p.uy * dx, n2 = (__int128)p.ux * p.ux + (__int128)p.uy * p.uy;
    const __int128 along = a >= 0 ? F.front : F.rear;
    return a * a <= along * along * n2 && b * b <= (__int128)F.half_width * F.half_width * n2;
}
int brute_term(const PwppReachRule &R, int cost, bool with_d2, int32_t d2) {
    int c = cost < 0 ? R.unknown : cost;
    if (c < 0 || c >= R.lethal) return 0;
    if (with_d2 && d2 <= R.clearance2) return 0;
    return R.base + c;
}
long isqrt_up(long v) {
    long r = 0;
    while (r * r < v) ++r;
    return r;
}
PwppFootPoseRow brute_pose(const Case &c, int f, const PwppFootPose &p) {
    if (p.ux == 0 && p.uy == 0) return PwppFootPoseRow{2, 0, 0, 0, 0, 0, 0x7fffffff, -1};
    const long e = c.F.front > c.F.rear ? c.F.front : c.F.rear;
    const long reach_cells = isqrt_up(e * e + (long)c.F.half_width * c.F.half_width) / 16 + 2;
    const long cx = p.px >= 0 ? p.px / 16 : -((-(long)p.px + 15) / 16), cy = p.py >= 0 ? p.py / 16 : -((-(long)p.py + 15) / 16);
    PwppFootPoseRow r{0, 0, 0, 0, 0, 0, 0x7fffffff, -1};
    const size_t base = (size_t)f * (size_t)c.nx * (size_t)c.ny;
    for (long iy = 0; iy < c.ny; ++iy)  // every cell of the image
        for (long ix = 0; ix < c.nx; ++ix) {
            if (!brute_covers(c.F, p, ix, iy)) continue;
            const size_t at = base + (size_t)iy * (size_t)c.nx + (size_t)ix;
            const bool with_d2 = !c.dist2.empty();
            const int t = brute_term(c.R, c.cost[at], with_d2, with_d2 ? c.dist2[at] : 0);
            ++r.covered;
            if (c.cost[at] < 0) ++r.unknown;
            if (t == 0) {
                ++r.blocked;
                if (r.hit < 0) r.hit = (int32_t)(iy * c.nx + ix);
            }
            if (t > r.max_term) r.max_term = t;
            if (with_d2 && c.dist2[at] < r.min_dist2) r.min_dist2 = c.dist2[at];
        }
    for (long iy = cy - reach_cells; iy <= cy + reach_cells; ++iy)  // and every cell outside it that the rectangle can reach
        for (long ix = cx - reach_cells; ix <= cx + reach_cells; ++ix)
            if ((ix < 0 || ix >= c.nx || iy < 0 || iy >= c.ny) && brute_covers(c.F, p, ix, iy)) ++r.covered, ++r.outside;
    r.status = r.blocked > 0 || (r.outside > 0 && (c.F.flags & 1)) ? 1 : 0;
    return r;
}
void brute(const Case &c, Rows &out) {
    const size_t trajs = (size_t)c.frames * (size_t)c.n_traj;
    out.pose.resize(trajs * (size_t)c.n_steps), out.traj.resize(trajs);
    for (int f = 0; f < c.frames; ++f)
        for (int j = 0; j < c.n_traj; ++j) {
            const size_t t = (size_t)f * (size_t)c.n_traj + (size_t)j;
            const PwppFootPose *P = poses_of(c, f, j);
            PwppFootPoseRow *rows = out.pose.data() + t * (size_t)c.n_steps;
            int first = -1;
            for (int k = 0; k < c.n_steps; ++k) {
                rows[k] = brute_pose(c, f, P[k]);
                if (first < 0 && rows[k].status == 1) first = k;
            }
            PwppFootTrajRow r{first, 0, -1, 0, 0, 0, 0x7fffffff, 0x7fffffff};
            for (int k = 0; k < (first < 0 ? c.n_steps : first); ++k) {
                if (rows[k].status == 2) continue;
                ++r.free_steps, r.last = k, r.sum_term += rows[k].max_term, r.unknown += rows[k].unknown;
                if (rows[k].max_term > r.max_term) r.max_term = rows[k].max_term;
                if (rows[k].min_dist2 < r.min_dist2) r.min_dist2 = rows[k].min_dist2;
            }
            if (!c.reach.empty() && r.last >= 0) {
                const long px = P[r.last].px, py = P[r.last].py;
                const long x = px >= 0 ? px / 16 : -((-px + 15) / 16), y = py >= 0 ? py / 16 : -((-py + 15) / 16);
                if (x >= 0 && x < c.nx && y >= 0 && y < c.ny) r.reach_last = reach_of(c, f)[y * c.nx + x];
            }
            out.traj[t] = r;
        }
}

// ---- the random cases ------------------------------------------------------------------------------------------------------------
using Rng = std::mt19937_64;
int pick(Rng &g, int lo, int hi) { return lo + (int)(g() % (uint64_t)(hi - lo + 1)); }

Case random_case(Rng &g, int round) {
    Case c;
    c.nx = pick(g, 1, 20), c.ny = pick(g, 1, 20), c.frames = pick(g, 1, 2);
    if (round % 7 == 0) c.nx = 1;
    if (round % 11 == 0) c.ny = 1;
    c.R = PwppReachRule{pick(g, 1, 255), pick(g, 1, 101), pick(g, -1, 100), 0, 0, 0};
    const size_t cells = (size_t)c.nx * (size_t)c.ny * (size_t)c.frames;
    c.cost.resize(cells);
    const int wall = pick(g, 0, 40), unknown = pick(g, 0, 25);
    for (auto &v : c.cost) {
        const int u = pick(g, 0, 99);
        v = (int8_t)(u < wall ? pick(g, 100, 127) : (u < wall + unknown ? pick(g, -128, -1) : pick(g, 0, 99)));
    }
    if (pick(g, 0, 1)) {
        c.dist2.resize(cells);
        for (auto &v : c.dist2) v = pick(g, 0, 5) == 0 ? 0x7fffffff : pick(g, 0, 40);
        c.R.clearance2 = pick(g, 0, 20), c.R.use_dist2 = 1;
    }
    if (pick(g, 0, 2)) {
        c.reach.resize(cells);
        for (auto &v : c.reach) v = pick(g, 0, 6) == 0 ? 0x7fffffff : pick(g, 0, 100000);
    }
    const int kind = pick(g, 0, 9);  // windows of one cell, of up to 3 x 3, 5 x 5 and 21 x 21 cells (the square window below 6 cells a side), and the largest
    const int top = kind < 2 ? 7 : (kind < 4 ? 23 : (kind < 6 ? 39 : (kind < 9 ? 160 : 2048)));
    const int ew = pick(g, 0, top), w = pick(g, 0, ew > 1024 ? 1024 : ew), e = ew - w > 1024 ? 1024 : ew - w;
    c.F = PwppFootRule{pick(g, 0, 1) ? e : pick(g, 0, e), 0, w, pick(g, 0, 1)};
    c.F.rear = pick(g, 0, 1) ? e : pick(g, 0, e);
    if (pick(g, 0, 1)) std::swap(c.F.front, c.F.rear);
    c.n_sets = c.frames > 1 && pick(g, 0, 1) ? c.frames : 1, c.n_traj = pick(g, 1, 3);
    c.n_steps = top >= 2048 ? pick(g, 1, 12) : (pick(g, 0, 4) == 0 ? pick(g, 62, 67) : (pick(g, 0, 3) == 0 ? pick(g, 1, 40) : pick(g, 1, 12)));
    c.poses.resize((size_t)c.n_sets * (size_t)c.n_traj * (size_t)c.n_steps);
    static const int compass[8][2] = {{1, 0}, {1, 1}, {0, 1}, {-1, 1}, {-1, 0}, {-1, -1}, {0, -1}, {1, -1}};
    const int hit_share = pick(g, 0, 3);  // (how often a pose may wander off: trajectories with and without a hit)
    for (auto &p : c.poses) {
        const int where = pick(g, 0, 9);
        const int margin = where < hit_share ? 16 * 12 : 0;
        p.px = pick(g, -margin, 16 * c.nx + margin), p.py = pick(g, -margin, 16 * c.ny + margin);
        if (where == 9 && pick(g, 0, 3) == 0) p.px = pick(g, 0, 1) ? -(1 << 20) : (1 << 20), p.py = pick(g, -(1 << 20), 1 << 20);
        const int h = pick(g, 0, 9);
        if (h < 2) p.ux = p.uy = 0;
        else if (h < 5) { const int s = pick(g, 1, 1024), k = pick(g, 0, 7); p.ux = compass[k][0] * s, p.uy = compass[k][1] * s; }
        else if (h < 7) { const int s = pick(g, 1, 204) * (pick(g, 0, 1) ? 1 : -1); p.ux = 3 * s, p.uy = 4 * s; if (pick(g, 0, 1)) std::swap(p.ux, p.uy); }
        else p.ux = pick(g, -1024, 1024), p.uy = pick(g, -1024, 1024);
    }
    return c;
}

bool same_pose(const PwppFootPoseRow &a, const PwppFootPoseRow &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }
bool same_traj(const PwppFootTrajRow &a, const PwppFootTrajRow &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

long compare(const Case &c, const Rows &want, const Rows &got, bool has_pose, int deal, int round) {
    long bad = 0;
    if (has_pose)
        for (size_t i = 0; i < want.pose.size(); ++i)
            if (!same_pose(want.pose[i], got.pose[i])) {
                if (++bad < 4)
                    std::printf("mismatch: round %d deal %d pose %zu: status %d/%d covered %d/%d outside %d/%d blocked %d/%d unknown %d/%d max_term %d/%d min_dist2 %d/%d hit %d/%d\n",
                                round, deal, i, got.pose[i].status, want.pose[i].status, got.pose[i].covered, want.pose[i].covered, got.pose[i].outside, want.pose[i].outside,
                                got.pose[i].blocked, want.pose[i].blocked, got.pose[i].unknown, want.pose[i].unknown, got.pose[i].max_term, want.pose[i].max_term,
                                got.pose[i].min_dist2, want.pose[i].min_dist2, got.pose[i].hit, want.pose[i].hit);
            }
    for (size_t i = 0; i < want.traj.size(); ++i)
        if (!same_traj(want.traj[i], got.traj[i])) {
            if (++bad < 4)
                std::printf("mismatch: round %d deal %d trajectory %zu (%d steps): first_hit %d/%d free_steps %d/%d last %d/%d max_term %d/%d sum_term %d/%d unknown %d/%d reach_last %d/%d\n",
                            round, deal, i, c.n_steps, got.traj[i].first_hit, want.traj[i].first_hit, got.traj[i].free_steps, want.traj[i].free_steps, got.traj[i].last,
                            want.traj[i].last, got.traj[i].max_term, want.traj[i].max_term, got.traj[i].sum_term, want.traj[i].sum_term, got.traj[i].unknown,
                            want.traj[i].unknown, got.traj[i].reach_last, want.traj[i].reach_last);
        }
    return bad;
}

int run_cases() {
    long cases = 0, mismatches = 0, n_free = 0, n_hit = 0, n_skipped = 0, with_hit = 0, without_hit = 0;
    // the division of the deal
    for (uint32_t w = 1; w <= 257; ++w) {
        const uint32_t inv = pwpp_foot_inv(w);
        for (uint32_t i = 0; i < (1u << 17); ++i)
            if (pwpp_foot_div(i, w, inv) != i / w) ++mismatches;
        ++cases;
    }
    Rng g(20261021);
    // Lemma 1 and the refinement: no covered cell outside the window, over a domain of 150 cells round p
    for (int round = 0; round < 160; ++round) {
        Case c = random_case(g, 1);
        const PwppFootPose p = c.poses[0];
        if (pwpp_foot_skipped(p)) continue;
        const PwppFootWindow w = pwpp_foot_window(c.F, p);
        const long e = c.F.front > c.F.rear ? c.F.front : c.F.rear;
        const long cx = p.px >> 4, cy = p.py >> 4;
        for (long iy = cy - 150; iy <= cy + 150; ++iy)
            for (long ix = cx - 150; ix <= cx + 150; ++ix) {
                const bool cov = brute_covers(c.F, p, ix, iy), in_window = ix >= w.x0 && ix < w.x0 + w.w && iy >= w.y0 && iy < w.y0 + w.h;
                const long dx = 16 * ix + 8 - p.px, dy = 16 * iy + 8 - p.py;
                if (cov && (!in_window || std::labs(dx) > e + c.F.half_width || std::labs(dy) > e + c.F.half_width)) ++mismatches;
                if (cov != pwpp_foot_covers(c.F, p, (int)ix, (int)iy)) ++mismatches;
            }
        if (w.w > pwpp_foot_side_max(c.F) || w.h > pwpp_foot_side_max(c.F)) ++mismatches;
        ++cases;
    }
    // the trajectory merge is associative
    for (int round = 0; round < 400; ++round) {
        PwppFootTraj t[3];
        for (int i = 0; i < 3; ++i) {
            PwppFootPoseRow r{pick(g, 0, 2), 0, 0, 0, pick(g, 0, 9), pick(g, 0, 300), pick(g, 0, 50), -1};
            t[i] = pwpp_foot_traj_of(r, 10 * i + pick(g, 0, 9));
        }
        PwppFootTraj ab = t[0], bc = t[1], left, right = t[0];
        pwpp_foot_traj_merge(ab, t[1]), left = ab, pwpp_foot_traj_merge(left, t[2]);
        pwpp_foot_traj_merge(bc, t[2]), pwpp_foot_traj_merge(right, bc);
        if (std::memcmp(&left, &right, sizeof(left)) != 0) ++mismatches;
        ++cases;
    }
    for (int round = 0; round < 3200; ++round) {
        const Case c = random_case(g, round);
        Rows want, lanes, waves, waves_only;
        brute(c, want);
        deal_lanes(c, lanes);
        deal_waves(c, true, waves);
        deal_waves(c, false, waves_only);
        mismatches += compare(c, want, lanes, true, 1, round) + compare(c, want, waves, true, 2, round) + compare(c, want, waves_only, false, 3, round);
        for (const auto &r : want.pose) (r.status == 0 ? n_free : (r.status == 1 ? n_hit : n_skipped))++;
        for (const auto &r : want.traj) (r.first_hit >= 0 ? with_hit : without_hit)++;
        ++cases;
    }
    mismatches += g_slot_overflows;
    std::printf("footprint_check: %ld cases, %ld mismatches (%ld free, %ld hit and %ld skipped poses; %ld trajectories with a hit, %ld without; %ld packed rounds, %ld early ends, "
                "%ld rounds whose lanes disagree)\n",
                cases, mismatches, n_free, n_hit, n_skipped, with_hit, without_hit, g_packed_rounds, g_early_exits, g_slot_overflows);
    const bool thin = n_free == 0 || n_hit == 0 || n_skipped == 0 || with_hit == 0 || without_hit == 0 || g_packed_rounds == 0 || g_early_exits == 0;
    if (thin) std::printf("footprint_check: the cases miss a kind\n");
    return mismatches == 0 && !thin ? 0 : 1;
}

// ---- dump ------------------------------------------------------------------------------------------------------------------------
template <class T>
bool read_file(const char *path, size_t n, std::vector<T> &out) {
    out.resize(n);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(out.data(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "footprint_check: cannot read %zu items from %s\n", n, path);
        if (f) std::fclose(f);
        return false;
    }
    std::fclose(f);
    return true;
}

int dump(char **a) {
    Case c;
    c.nx = std::atoi(a[1]), c.ny = std::atoi(a[2]), c.frames = std::atoi(a[3]);
    const bool with_d2 = std::strcmp(a[8], "-") != 0, with_reach = std::strcmp(a[9], "-") != 0;
    c.R = PwppReachRule{std::atoi(a[4]), std::atoi(a[5]), std::atoi(a[6]), with_d2 ? std::atoi(a[7]) : 0, 0, with_d2 ? 1 : 0};
    c.F = PwppFootRule{std::atoi(a[10]), std::atoi(a[11]), std::atoi(a[12]), std::atoi(a[13])};
    c.n_sets = std::atoi(a[15]), c.n_traj = std::atoi(a[16]), c.n_steps = std::atoi(a[17]);
    const int deal = std::atoi(a[18]);
    const bool want_pose = std::atoi(a[19]) != 0;
    if (c.nx < 1 || c.ny < 1 || c.frames < 1 || c.n_traj < 1 || c.n_steps < 1 || (c.n_sets != 1 && c.n_sets != c.frames) || c.F.front < 0 || c.F.front > PWPP_FOOT_EXTENT_MAX ||
        c.F.rear < 0 || c.F.rear > PWPP_FOOT_EXTENT_MAX || c.F.half_width < 0 || c.F.half_width > PWPP_FOOT_EXTENT_MAX || (deal != 1 && deal != 2)) {
        std::fprintf(stderr, "footprint_check: arguments out of range\n");
        return 2;
    }
    const size_t cells = (size_t)c.nx * (size_t)c.ny * (size_t)c.frames, n_given = (size_t)c.n_sets * (size_t)c.n_traj * (size_t)c.n_steps;
    std::vector<int32_t> raw;
    if (!read_file(a[0], cells, c.cost) || (with_d2 && !read_file(a[8], cells, c.dist2)) || (with_reach && !read_file(a[9], cells, c.reach)) || !read_file(a[14], 4 * n_given, raw))
        return 2;
    c.poses.resize(n_given);
    for (size_t i = 0; i < n_given; ++i) {
        if (!pwpp_foot_pose_in_range(raw.data() + 4 * i)) {
            std::fprintf(stderr, "footprint_check: pose %zu out of range\n", i);
            return 2;
        }
        c.poses[i] = PwppFootPose{raw[4 * i], raw[4 * i + 1], raw[4 * i + 2], raw[4 * i + 3]};
    }
    Rows out;
    const auto t0 = std::chrono::steady_clock::now();
    if (deal == 1) deal_lanes(c, out);
    else deal_waves(c, want_pose, out);
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (want_pose) {
        FILE *f = std::fopen((std::string(a[20]) + ".pose").c_str(), "wb");
        if (!f || std::fwrite(out.pose.data(), sizeof(PwppFootPoseRow), out.pose.size(), f) != out.pose.size()) return 2;
        std::fclose(f);
    }
    FILE *f = std::fopen((std::string(a[20]) + ".traj").c_str(), "wb");
    if (!f || std::fwrite(out.traj.data(), sizeof(PwppFootTrajRow), out.traj.size(), f) != out.traj.size()) return 2;
    std::fclose(f);
    std::printf("footprint_check: %zu poses folded in %.1f us\n", (size_t)c.frames * (size_t)c.n_traj * (size_t)c.n_steps, us);
    return g_slot_overflows == 0 ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 23 && std::strcmp(argv[1], "dump") == 0) return dump(argv + 2);
    if (argc != 1) {
        std::fprintf(stderr, "usage: footprint_check | footprint_check dump ... (see the head of tools/footprint_check.cpp)\n");
        return 2;
    }
    return run_cases();
}
