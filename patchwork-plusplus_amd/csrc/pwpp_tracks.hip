// pwpp_tracks.hip -- the gfx950 kernels of the cluster association (pwpp_associate_grid, pwpp_track_obstacles): which cluster of
// the current label image is which cluster of the previous one.  The rule is csrc/pwpp_tracks.h, one text with the host and
// tools/tracks_check.cpp; include/pwpp.h has the contract.
//
// Four launches on the caller's stream, all over global memory:
//   k_tracks_init    empties the frames' tables and zeroes the argmax words, the counters and both link tables.
//   k_tracks_count   a lane per cell index of a frame.  The lane of a current cell adds 1 to `cells` of its row, takes the cell's
//                    vote (pwpp_tracks_vote) and inserts or increments the pair in the frame's open-addressed table; a NEW key adds
//                    1 to the frame's `distinct` and to `links` of both rows.  The lane of a previous cell adds 1 to `cells` of its
//                    row.  Neighbouring cells of one cluster hit one word, so the lanes of a wave that hold the same key are
//                    combined first (wave_combine): one atomic per distinct key of a wave, with the number of its lanes.
//   k_tracks_reduce  a lane per slot: the 64-bit atomic maximum of pwpp_tracks_pack per row, on both sides.
//   k_tracks_rows    a workgroup per frame walks the frame's rows in runs of 256: unpacks, applies the overflow rule, and gives the
//                    ids, the fresh ranks from a running prefix count of the run's ballots.
// Every count is an integer sum and every choice a maximum or minimum of distinct keys, so the bytes do not depend on the order in
// which the atomics arrive.  Every loop is bounded: a probe sequence by the table's slots, the combining by the 64 lanes of a wave,
// the rows' walk by max_rows.  No kernel waits for another workgroup; every __syncthreads stands in uniform control flow (the
// loop of k_tracks_rows runs the same number of times for every lane).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwpp_dev.h"  // the launchers' prototypes
#include "pwpp_tracks.h"

namespace {
constexpr int kBlock = 256;

struct TracksCall {
    PwppFusionGeometry G;  // the current grid as the map, the previous one as the frame images
    PwppTracksRule R;
    int32_t frames, n_poses;
    uint32_t cells_c, cells_p;  // of one frame: NX * NY, nx * ny (<= 2^30)
    uint32_t per_frame;         // workgroups of k_tracks_count for one frame
};

// the working words of a call, in this order (the 64-bit ones first: the section starts at a multiple of 16 bytes)
struct TracksWork {
    unsigned long long *keys, *best_curr, *best_prev;
    uint32_t *counts, *distinct;
};
__host__ __device__ inline TracksWork tracks_work(uint32_t *work, size_t frames, size_t rows, size_t slots) {
    TracksWork w;
    w.keys = reinterpret_cast<unsigned long long *>(work);
    w.best_curr = w.keys + frames * slots;
    w.best_prev = w.best_curr + frames * rows;
    w.counts = reinterpret_cast<uint32_t *>(w.best_prev + frames * rows);
    w.distinct = w.counts + frames * slots;
    return w;
}

__global__ __launch_bounds__(kBlock) void k_tracks_init(TracksCall C, uint32_t *work, int32_t *curr_links, int32_t *prev_links) {
    const size_t frames = (size_t)C.frames, rows = (size_t)C.R.max_rows, slots = (size_t)C.R.slots;
    const TracksWork w = tracks_work(work, frames, rows, slots);
    const size_t n_keys = frames * slots, n_best = 2 * frames * rows, n_words = frames * slots + frames, n_link = frames * rows * 4;
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_keys; i += stride) w.keys[i] = PWPP_TRACKS_EMPTY;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_best; i += stride) w.best_curr[i] = 0;  // (best_prev follows it)
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_words; i += stride) w.counts[i] = 0;    // (distinct follows it)
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_link; i += stride) curr_links[i] = 0, prev_links[i] = 0;
}

// The lanes of a wave that hold the same key become one: the first of them gets their number, the others 0.  The group loop of
// pwpp_wave.h under its contract, kept on its own text: as wave_for_each_group with the count in its body the compiler rotates the
// three loops of k_tracks_count (27 scalar instructions more) and pwpp_associate_grid measured 1.4 to 3.1 % slower on 64 x 64 cells
// in four sessions of four (profiles/wave_primitives_refactor_ab.txt).
__device__ inline uint32_t wave_combine(uint64_t key, bool valid) {
    const unsigned lane = threadIdx.x & 63u;
    uint64_t pending = __ballot(valid);
    uint32_t mine = 0;
    for (int it = 0; it < 64 && pending != 0; ++it) {
        const int lead = __ffsll((unsigned long long)pending) - 1;
        const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)key, lead), hi = (uint32_t)__shfl((int)(uint32_t)(key >> 32), lead);
        const uint64_t k = ((uint64_t)hi << 32) | lo;
        const uint64_t same = __ballot(valid && key == k) & pending;
        if ((int)lane == lead) mine = (uint32_t)__popcll(same);
        pending &= ~same;
    }
    return mine;
}

// n cells more for the pair `key` in one frame's table; a new key counts for the frame and for both rows.  At most `slots` probes:
// a full table drops the cells, which only a frame beyond max_pairs can see (pwpp_tracks.h, THE TABLE).
__device__ inline void table_add(unsigned long long *keys, uint32_t *counts, uint32_t slots, uint64_t key, uint32_t n, uint32_t *distinct,
                                 PwppClusterLink *curr_rows, PwppClusterLink *prev_rows) {
    uint32_t s = pwpp_tracks_hash(key, slots);
    for (uint32_t probe = 0; probe < slots; ++probe) {
        unsigned long long held = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (held == PWPP_TRACKS_EMPTY) {
            held = atomicCAS(&keys[s], PWPP_TRACKS_EMPTY, (unsigned long long)key);
            if (held == PWPP_TRACKS_EMPTY) {
                atomicAdd(distinct, 1u);
                atomicAdd(&curr_rows[pwpp_tracks_pair_curr(key)].links, 1);
                atomicAdd(&prev_rows[pwpp_tracks_pair_prev(key)].links, 1);
                held = key;
            }
        }
        if (held == key) {
            atomicAdd(&counts[s], n);
            return;
        }
        s = s + 1 == slots ? 0 : s + 1;
    }
}

template <bool RECIP>
__global__ __launch_bounds__(kBlock) void k_tracks_count(TracksCall C, const int32_t *curr, const int32_t *prev, const double *poses, uint32_t *work,
                                                         PwppClusterLink *curr_links, PwppClusterLink *prev_links) {
    const uint32_t f = blockIdx.x / C.per_frame, run = blockIdx.x % C.per_frame;
    if (f >= (uint32_t)C.frames) return;  // (the whole workgroup)
    const size_t frames = (size_t)C.frames, rows = (size_t)C.R.max_rows, slots = (size_t)C.R.slots;
    const TracksWork w = tracks_work(work, frames, rows, slots);
    const uint32_t i = run * kBlock + threadIdx.x;
    const int32_t *prev_f = prev + (size_t)f * C.cells_p;
    PwppClusterLink *curr_rows = curr_links + (size_t)f * rows, *prev_rows = prev_links + (size_t)f * rows;

    // the previous cell i: one more cell of its row
    const int32_t a_here = i < C.cells_p ? prev_f[i] : -1;
    const bool a_row = pwpp_tracks_row(a_here, C.R.max_rows);
    const uint32_t n_a = wave_combine((uint64_t)(uint32_t)a_here, a_row);
    if (n_a != 0) atomicAdd(&prev_rows[a_here].cells, (int32_t)n_a);

    // the current cell i: one more cell of its row, and its vote
    const int32_t b = i < C.cells_c ? curr[(size_t)f * C.cells_c + i] : -1;
    const bool b_row = pwpp_tracks_row(b, C.R.max_rows);
    const uint32_t n_b = wave_combine((uint64_t)(uint32_t)b, b_row);
    if (n_b != 0) atomicAdd(&curr_rows[b].cells, (int32_t)n_b);
    int32_t a = -1;
    if (b_row) {
        const int jy = (int)(i / (uint32_t)C.G.NX), jx = (int)(i - (uint32_t)jy * (uint32_t)C.G.NX);
        a = pwpp_tracks_vote<RECIP>(C.G, poses + (C.n_poses == 1 ? (size_t)0 : (size_t)f * 6), jx, jy, prev_f, C.R.gate, C.R.max_rows);
    }
    const uint64_t key = pwpp_tracks_pair(b, a);
    const uint32_t n = wave_combine(key, a >= 0);
    if (n != 0) table_add(w.keys + (size_t)f * slots, w.counts + (size_t)f * slots, C.R.slots, key, n, w.distinct + f, curr_rows, prev_rows);
}

__global__ __launch_bounds__(kBlock) void k_tracks_reduce(TracksCall C, uint32_t *work) {
    const size_t frames = (size_t)C.frames, rows = (size_t)C.R.max_rows, slots = (size_t)C.R.slots;
    const TracksWork w = tracks_work(work, frames, rows, slots);
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= frames * slots) return;
    const uint64_t key = w.keys[i];
    if (key == PWPP_TRACKS_EMPTY) return;
    const size_t f = i / slots;
    const int32_t b = pwpp_tracks_pair_curr(key), a = pwpp_tracks_pair_prev(key);
    if (!pwpp_tracks_row(b, C.R.max_rows) || !pwpp_tracks_row(a, C.R.max_rows)) return;  // (no such key is ever stored)
    const uint32_t n = w.counts[i];
    atomicMax(&w.best_curr[f * rows + (size_t)b], (unsigned long long)pwpp_tracks_pack(n, a));
    atomicMax(&w.best_prev[f * rows + (size_t)a], (unsigned long long)pwpp_tracks_pack(n, b));
}

__global__ __launch_bounds__(kBlock) void k_tracks_rows(TracksCall C, const uint32_t *work, PwppClusterLink *curr_links, PwppClusterLink *prev_links, int32_t *n_pairs,
                                                        const int32_t *id_prev, const int32_t *next_id, int32_t *id_curr, int32_t *next_id_out) {
    __shared__ uint32_t wave_fresh[kBlock / 64];
    const size_t frames = (size_t)C.frames, rows = (size_t)C.R.max_rows, slots = (size_t)C.R.slots;
    const TracksWork w = tracks_work(const_cast<uint32_t *>(work), frames, rows, slots);
    const uint32_t f = blockIdx.x;  // (one workgroup per frame: the grid is `frames`)
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t distinct = w.distinct[f];
    const bool over = pwpp_tracks_overflowed(distinct, C.R.max_pairs);
    const unsigned long long *best_curr = w.best_curr + (size_t)f * rows, *best_prev = w.best_prev + (size_t)f * rows;
    PwppClusterLink *curr_rows = curr_links + (size_t)f * rows, *prev_rows = prev_links + (size_t)f * rows;
    const int32_t first_id = C.R.with_ids ? next_id[f] : 0;
    uint32_t fresh_below = 0;  // the fresh rows below this run: the same in every lane
    for (uint32_t r0 = 0; r0 < (uint32_t)C.R.max_rows; r0 += kBlock) {
        const uint32_t r = r0 + threadIdx.x;
        const bool in = r < (uint32_t)C.R.max_rows;
        bool exists = false, fresh = false;
        int32_t id = -1;
        if (in) {
            const PwppClusterLink c = pwpp_tracks_link(curr_rows[r].cells, curr_rows[r].links, best_curr[r], over);
            const PwppClusterLink p = pwpp_tracks_link(prev_rows[r].cells, prev_rows[r].links, best_prev[r], over);
            curr_rows[r] = c, prev_rows[r] = p;
            exists = c.cells > 0;
            if (exists && C.R.with_ids) {
                fresh = true;
                if (c.other >= 0 && c.other < C.R.max_rows) {
                    const PwppClusterLink po = pwpp_tracks_link(0, 0, best_prev[c.other], over);
                    const int32_t ip = id_prev[(size_t)f * rows + (size_t)c.other];
                    if (pwpp_tracks_continues(c, (int32_t)r, po, ip, C.R.min_overlap)) fresh = false, id = ip;
                }
            }
        }
        const uint64_t m = __ballot(fresh);
        if (lane == 0) wave_fresh[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t k = fresh_below + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), run_total = 0;
        for (unsigned v = 0; v < kBlock / 64; ++v) {
            if (v < wave) k += wave_fresh[v];
            run_total += wave_fresh[v];
        }
        __syncthreads();  // (the next run writes wave_fresh again)
        if (in && C.R.with_ids) id_curr[(size_t)f * rows + r] = fresh ? pwpp_tracks_fresh_id(first_id, k) : id;
        fresh_below += run_total;
    }
    if (threadIdx.x == 0) {
        if (n_pairs) n_pairs[f] = pwpp_tracks_n_pairs(distinct, C.R.max_pairs);
        if (C.R.with_ids) next_id_out[f] = pwpp_tracks_fresh_id(first_id, fresh_below);
    }
}
}  // namespace

static_assert(sizeof(PwppClusterLink) == 16, "a row of a link table is 16 bytes");

size_t pwpp_tracks_work_words(int frames, int max_rows, int max_pairs) {
    const size_t f = (size_t)frames, rows = (size_t)max_rows, slots = (size_t)pwpp_tracks_slots(max_pairs);
    return 2 * f * slots + 4 * f * rows + f * slots + f;
}

int pwpp_launch_tracks(const PwppFusionGeometry *G, const PwppTracksRule *R, int frames, const int32_t *curr, const int32_t *prev, const double *poses, int n_poses,
                       void *curr_links, void *prev_links, int32_t *n_pairs, const int32_t *id_prev, const int32_t *next_id, int32_t *id_curr,
                       int32_t *next_id_out, uint32_t *work, hipStream_t stream) {
    if (frames < 1 || R->max_rows < 1 || R->max_pairs < 1 || R->slots != pwpp_tracks_slots(R->max_pairs) || R->gate < 0 || R->gate > PWPP_TRACKS_MAX_GATE)
        return (int)hipErrorInvalidValue;
    if ((int64_t)frames * R->max_rows > PWPP_TRACKS_MAX_TOTAL || (int64_t)frames * R->max_pairs > PWPP_TRACKS_MAX_TOTAL) return (int)hipErrorInvalidValue;
    if (R->with_ids && (!id_prev || !next_id || !id_curr || !next_id_out)) return (int)hipErrorInvalidValue;
    TracksCall C;
    C.G = *G, C.R = *R, C.frames = frames, C.n_poses = n_poses;
    C.cells_c = (uint32_t)G->NX * (uint32_t)G->NY, C.cells_p = (uint32_t)G->nx * (uint32_t)G->ny;  // (sides <= 32768)
    const uint32_t most = C.cells_c > C.cells_p ? C.cells_c : C.cells_p;
    C.per_frame = (most + kBlock - 1) / kBlock;
    const uint64_t count_blocks = (uint64_t)C.per_frame * (uint64_t)frames;
    if (count_blocks > 0x7fffffffull) return (int)hipErrorInvalidValue;  // (the caller's checks exclude it: cells * frames <= 2^31)
    PwppClusterLink *cl = static_cast<PwppClusterLink *>(curr_links), *pl = static_cast<PwppClusterLink *>(prev_links);
    const size_t slots_all = (size_t)frames * R->slots, rows_all = (size_t)frames * (size_t)R->max_rows;
    const size_t init_items = slots_all > 4 * rows_all ? slots_all : 4 * rows_all;
    const unsigned init_blocks = (unsigned)((init_items + kBlock - 1) / kBlock < 4096 ? (init_items + kBlock - 1) / kBlock : 4096);
    hipLaunchKernelGGL(k_tracks_init, dim3(init_blocks), dim3(kBlock), 0, stream, C, work, reinterpret_cast<int32_t *>(cl), reinterpret_cast<int32_t *>(pl));
    int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    if (G->inv_cell != 0.0) hipLaunchKernelGGL(k_tracks_count<true>, dim3((unsigned)count_blocks), dim3(kBlock), 0, stream, C, curr, prev, poses, work, cl, pl);
    else hipLaunchKernelGGL(k_tracks_count<false>, dim3((unsigned)count_blocks), dim3(kBlock), 0, stream, C, curr, prev, poses, work, cl, pl);
    if ((rc = (int)hipGetLastError()) != 0) return rc;
    hipLaunchKernelGGL(k_tracks_reduce, dim3((unsigned)((slots_all + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, C, work);
    if ((rc = (int)hipGetLastError()) != 0) return rc;
    hipLaunchKernelGGL(k_tracks_rows, dim3((unsigned)frames), dim3(kBlock), 0, stream, C, work, cl, pl, n_pairs, id_prev, next_id, id_curr, next_id_out);
    return (int)hipGetLastError();
}
