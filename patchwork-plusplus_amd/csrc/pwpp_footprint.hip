// pwpp_footprint.hip -- the gfx950 (MI355X) kernels of the oriented vehicle footprint: for every (frame, trajectory, step) the fold of
// the frame's cost bytes and dist2 under the rectangle of the pose, and for every (frame, trajectory) the summary of its free prefix
// (pwpp_footprint_grid; include/pwpp.h has the rules, pwpp_footprint.h the arithmetic and the proofs).  Reads the cost bytes, dist2,
// reach and the uploaded poses; writes the rows.  Integers only.
//
// One of two deals with the same bytes:
//   k_foot_poses, k_foot_trajs   (option "footprint_path" = 1, the yardstick) a lane per pose, serial over its window row by row, its
//            row to global memory (the caller's array, or working memory where the caller asked for none); then a lane per
//            trajectory over those rows in step order, up to the first HIT.
//   k_foot_waves   ("footprint_path" = 2) one launch; a wave owns a (frame, trajectory) and takes its steps in rounds of 64 / slot
//            consecutive steps, a pose per slot of 1 .. 64 lanes (pwpp_foot_slot: the steps fill the wave first, the window's cells are
//            dealt to the lanes they leave over, i = c0, c0 + slot ..).  The pose's fold crosses its slot's lanes by a butterfly of
//            __shfl_xor, the round's poses are folded in step order by the butterfly's upper levels (the lower block first:
//            pwpp_foot_traj_merge is ordered), and the trajectory's summary stays in registers: the trajectory row never waits on a pose
//            row in memory.  Pose rows are written only where asked for; without them the wave stops at the round of the first HIT
//            (nothing behind it enters the trajectory row), and rounds of large windows are kept to 8 steps for that.
// No atomics, no barriers, no LDS (a wave never waits for another); every output has one writer.  Every loop is bounded by the
// window of Lemma 1 (at most 257 x 257 cells) or by n_steps.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwpp_dev.h"  // the launchers' prototypes
#include "pwpp_footprint.h"

namespace {

constexpr int kLaneBlock = 64;   // k_foot_poses, k_foot_trajs: windows and prefixes differ from lane to lane, small blocks spread them over the CUs
constexpr int kWaveBlock = 256;  // k_foot_waves: 4 waves, 4 trajectories
constexpr int kWavesPerBlock = kWaveBlock / 64;
// What option "footprint_path" = 0 means, decided by tools/footprint_cost.py (profiles/footprint_cost.txt), not in advance: the wave
// per trajectory where the windows are large (pwpp_foot_large) and either no pose rows are asked for or a dist2 image is read, the
// lane per pose otherwise.  Per 1024
// frames x 64 arcs x 32 poses: a footprint of 36 x 16 cells without pose rows 1.02 to 1.05 ms on path 2 (it stops a trajectory at
// its first hit) against 3.25 ms and, with dist2, 5.65 ms on path 1; with pose rows 3.93 against 3.24 ms and, with dist2, 4.11
// against 5.66 ms; a footprint of 9 x 4 cells 0.37 to 0.38 ms on path 2 against 0.29 ms and, with dist2, 0.34 ms on path 1, pose rows or not.

struct FootCall {
    PwppReachRule R;
    PwppFootRule F;
    int32_t nx, ny, frames;
    int32_t n_sets, n_traj, n_steps;
    int32_t slot, slot_shift;  // pwpp_foot_slot and its log2
    int64_t trajs, poses;      // frames * n_traj, trajs * n_steps
};

struct FootImages {
    const int8_t *cost;
    const int32_t *dist2, *reach;
    const PwppFootPose *poses;
};

__device__ inline PwppFootFrame frame_of(const FootCall &C, const FootImages &I, int f) {
    const size_t base = (size_t)f * (size_t)C.nx * (size_t)C.ny;
    return PwppFootFrame{C.R, I.cost + base, I.dist2 ? I.dist2 + base : nullptr, C.nx, C.ny};
}
// the poses of trajectory t = f * n_traj + j
__device__ inline const PwppFootPose *poses_of(const FootCall &C, const FootImages &I, int64_t t, int f) {
    const int64_t j = t - (int64_t)f * C.n_traj;
    return I.poses + ((size_t)(C.n_sets > 1 ? f : 0) * (size_t)C.n_traj + (size_t)j) * (size_t)C.n_steps;
}
__device__ inline void store_pose_row(PwppFootPoseRow *rows, int64_t at, const PwppFootPoseRow &r) {
    int32_t *o = reinterpret_cast<int32_t *>(rows) + 8 * at;  // (4-byte aligned: eight stores)
    o[0] = r.status, o[1] = r.covered, o[2] = r.outside, o[3] = r.blocked, o[4] = r.unknown, o[5] = r.max_term, o[6] = r.min_dist2, o[7] = r.hit;
}
__device__ inline PwppFootPoseRow load_pose_row(const PwppFootPoseRow *rows, int64_t at) {
    const int32_t *o = reinterpret_cast<const int32_t *>(rows) + 8 * at;
    return PwppFootPoseRow{o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]};
}
__device__ inline void store_traj_row(PwppFootTrajRow *rows, int64_t at, const FootCall &C, const FootImages &I, int f, const PwppFootPose *P, const PwppFootTraj &T) {
    const int32_t *reach = I.reach ? I.reach + (size_t)f * (size_t)C.nx * (size_t)C.ny : nullptr;
    PwppFootPose last{0, 0, 0, 0};
    if (T.last >= 0) last = P[T.last];
    const PwppFootTrajRow r = pwpp_foot_traj_row(T, reach, C.nx, C.ny, &last);
    int32_t *o = reinterpret_cast<int32_t *>(rows) + 8 * at;
    o[0] = r.first_hit, o[1] = r.free_steps, o[2] = r.last, o[3] = r.max_term, o[4] = r.sum_term, o[5] = r.unknown, o[6] = r.min_dist2, o[7] = r.reach_last;
}

// grid (ceil(poses / kLaneBlock))
__global__ __launch_bounds__(kLaneBlock) void k_foot_poses(FootCall C, FootImages I, PwppFootPoseRow *rows) {
    const int64_t id = (int64_t)blockIdx.x * kLaneBlock + threadIdx.x;
    if (id >= C.poses) return;
    const int64_t t = id / C.n_steps;
    const int k = (int)(id - t * C.n_steps), f = (int)(t / C.n_traj);
    store_pose_row(rows, id, pwpp_foot_pose_serial(frame_of(C, I, f), C.F, poses_of(C, I, t, f)[k]));
}

// grid (ceil(trajs / kLaneBlock)); after k_foot_poses on the same stream
__global__ __launch_bounds__(kLaneBlock) void k_foot_trajs(FootCall C, FootImages I, const PwppFootPoseRow *rows, PwppFootTrajRow *out) {
    const int64_t t = (int64_t)blockIdx.x * kLaneBlock + threadIdx.x;
    if (t >= C.trajs) return;
    const int f = (int)(t / C.n_traj);
    PwppFootTraj T = pwpp_foot_traj_none();
    for (int k = 0; k < C.n_steps && T.first_hit == PWPP_FOOT_NO_CELL; ++k) pwpp_foot_traj_merge(T, pwpp_foot_traj_of(load_pose_row(rows, t * C.n_steps + k), k));
    store_traj_row(out, t, C, I, f, poses_of(C, I, t, f), T);
}

__device__ inline PwppFootAcc shfl_xor_acc(const PwppFootAcc &a, int off) {
    return PwppFootAcc{__shfl_xor(a.covered, off), __shfl_xor(a.outside, off), __shfl_xor(a.blocked, off), __shfl_xor(a.unknown, off),
                       __shfl_xor(a.max_term, off), __shfl_xor(a.min_dist2, off), __shfl_xor(a.hit, off)};
}
__device__ inline PwppFootTraj shfl_xor_traj(const PwppFootTraj &a, int off) {
    return PwppFootTraj{__shfl_xor(a.first_hit, off), __shfl_xor(a.free_steps, off), __shfl_xor(a.last, off), __shfl_xor(a.max_term, off),
                        __shfl_xor(a.sum_term, off), __shfl_xor(a.unknown, off), __shfl_xor(a.min_dist2, off)};
}

// grid (ceil(trajs / kWavesPerBlock)); pose_rows and traj_rows: null where not asked for
__global__ __launch_bounds__(kWaveBlock) void k_foot_waves(FootCall C, FootImages I, PwppFootPoseRow *pose_rows, PwppFootTrajRow *traj_rows) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    if (t >= C.trajs) return;  // (the whole wave; the kernel has no barrier)
    const int f = (int)(t / C.n_traj);
    const PwppFootFrame V = frame_of(C, I, f);
    const PwppFootPose *P = poses_of(C, I, t, f);
    const int per = 64 >> C.slot_shift, sub = lane >> C.slot_shift, c0 = lane & (C.slot - 1);
    PwppFootTraj T = pwpp_foot_traj_none();
    for (int k0 = 0; k0 < C.n_steps; k0 += per) {
        const int k = k0 + sub;
        const bool valid = k < C.n_steps;
        PwppFootPose p{0, 0, 0, 0};
        if (valid) p = P[k];
        const bool skipped = pwpp_foot_skipped(p);  // (a step behind the trajectory's end counts as one: it adds nothing, and no row is stored)
        PwppFootAcc acc = pwpp_foot_acc_none();
        if (!skipped) {
            const PwppFootEdges e = pwpp_foot_edges(C.F, p);
            const PwppFootWindow w = pwpp_foot_window(C.F, p);
            const uint32_t n = (uint32_t)(w.w * w.h), inv = pwpp_foot_inv((uint32_t)w.w);  // (w.w and w.h are >= 0)
            for (uint32_t i = (uint32_t)c0; i < n; i += (uint32_t)C.slot) {
                const uint32_t y = pwpp_foot_div(i, (uint32_t)w.w, inv), x = i - y * (uint32_t)w.w;
                pwpp_foot_cell(V, e, p, w.x0 + (int32_t)x, w.y0 + (int32_t)y, acc);
            }
        }
        for (int off = 1; off < C.slot; off <<= 1) {  // the pose over its slot's lanes: every lane of the slot ends with the whole
            const PwppFootAcc o = shfl_xor_acc(acc, off);
            pwpp_foot_acc_merge(acc, o);
        }
        const PwppFootPoseRow row = skipped ? pwpp_foot_row_skipped() : pwpp_foot_row(C.F, acc);
        if (pose_rows && valid && c0 == 0) store_pose_row(pose_rows, t * C.n_steps + k, row);
        PwppFootTraj r = valid ? pwpp_foot_traj_of(row, k) : pwpp_foot_traj_none();
        for (int off = C.slot; off < 64; off <<= 1) {  // the round's poses in step order: the partner's block is the later one where the lane's bit is clear
            const PwppFootTraj o = shfl_xor_traj(r, off);
            if (lane & off) {
                PwppFootTraj first = o;
                pwpp_foot_traj_merge(first, r);
                r = first;
            } else {
                pwpp_foot_traj_merge(r, o);
            }
        }
        pwpp_foot_traj_merge(T, r);  // (uniform over the wave from here)
        if (!pose_rows && T.first_hit != PWPP_FOOT_NO_CELL) break;
    }
    if (traj_rows && lane == 0) store_traj_row(traj_rows, t, C, I, f, P, T);
}

}  // namespace

// what option "footprint_path" resolves to for a call: 1 or 2
extern "C" int pwpp_footprint_path_of(int path, const PwppFootRule *F, int pose_rows, int with_dist2) {
    return path != 0 ? path : (pwpp_foot_large(*F) && (!pose_rows || with_dist2) ? 2 : 1);
}

// pwpp_footprint_grid on device memory.  The caller has checked the image's shape (sides <= 32768, nx ny frames <= 2^31), R, F (extents 0 ..
// 1024), the counts (n_sets 1 or frames, n_traj 1 .. 65536, n_steps 1 .. 4096, frames n_traj n_steps <= 2^26) and every pose's range; poses:
// n_sets x n_traj x n_steps x {px, py, ux, uy} on the device; dist2, reach and the rows are 4-byte aligned.  `work_rows`: frames x n_traj x
// n_steps rows of working memory, needed on path 1 for trajectory rows without pose rows.
extern "C" int pwpp_launch_footprints(const PwppReachRule *R, const PwppFootRule *F, int nx, int ny, int frames, const int8_t *cost, const int32_t *dist2,
                                      const int32_t *reach, const int32_t *poses, int n_sets, int n_traj, int n_steps, void *pose_rows, void *traj_rows,
                                      void *work_rows, int path, hipStream_t stream) {
    if ((R->use_dist2 != 0) != (dist2 != nullptr) || !cost || !poses || (!pose_rows && !traj_rows) || F->front < 0 || F->front > PWPP_FOOT_EXTENT_MAX || F->rear < 0 ||
        F->rear > PWPP_FOOT_EXTENT_MAX || F->half_width < 0 || F->half_width > PWPP_FOOT_EXTENT_MAX || n_steps < 1 || n_steps > PWPP_FOOT_STEPS_MAX)
        return (int)hipErrorInvalidValue;
    FootCall C;
    C.R = *R, C.F = *F;
    C.nx = nx, C.ny = ny, C.frames = frames, C.n_sets = n_sets, C.n_traj = n_traj, C.n_steps = n_steps;
    C.slot = pwpp_foot_slot(*F, n_steps, pose_rows != nullptr), C.slot_shift = 0;
    while ((1 << C.slot_shift) < C.slot) ++C.slot_shift;
    C.trajs = (int64_t)frames * (int64_t)n_traj, C.poses = C.trajs * (int64_t)n_steps;
    const FootImages I{cost, dist2, reach, reinterpret_cast<const PwppFootPose *>(poses)};
    PwppFootPoseRow *prow = static_cast<PwppFootPoseRow *>(pose_rows);
    PwppFootTrajRow *trow = static_cast<PwppFootTrajRow *>(traj_rows);
    if (pwpp_footprint_path_of(path, F, pose_rows != nullptr, dist2 != nullptr) == 2) {
        hipLaunchKernelGGL(k_foot_waves, dim3((unsigned)((C.trajs + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kWaveBlock), 0, stream, C, I, prow, trow);
        return (int)hipGetLastError();
    }
    PwppFootPoseRow *rows = prow ? prow : static_cast<PwppFootPoseRow *>(work_rows);
    if (!rows) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_foot_poses, dim3((unsigned)((C.poses + kLaneBlock - 1) / kLaneBlock)), dim3(kLaneBlock), 0, stream, C, I, rows);
    if (trow) hipLaunchKernelGGL(k_foot_trajs, dim3((unsigned)((C.trajs + kLaneBlock - 1) / kLaneBlock)), dim3(kLaneBlock), 0, stream, C, I, rows, trow);
    return (int)hipGetLastError();
}
