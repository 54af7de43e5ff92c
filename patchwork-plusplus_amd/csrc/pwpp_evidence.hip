// pwpp_evidence.hip -- the gfx950 kernels of the per-cluster map evidence (pwpp_evidence_grid, pwpp_evidence_obstacles): what the
// fused map holds under the cells of every cluster of a label image.  The rule is csrc/pwpp_evidence.h, one text with the host and
// tools/evidence_check.cpp; include/pwpp.h has the contract.
//
// Up to four launches on the caller's stream:
//   k_evid_init    zeroes the rows.
//   k_evid_count   a lane per cell of a frame: the cell's row, its landing (pwpp_evid_landed), the gated read and its class.  The
//                  lanes of a wave that hold the same row are combined first (wave_rows: one ballot per distinct row of the wave, the
//                  counters from the popcounts of its lanes, the sum of E by a butterfly over the wave), so a row of a wave costs one
//                  atomic per counter.  Path 1: those atomics go to the output rows in global memory, a workgroup per 256 cells.
//                  Path 2: a workgroup owns a run of 2048 cells of one frame and a table of max_rows rows in LDS (24 bytes a row,
//                  max_rows <= PWPP_EV_LDS_ROWS), adds there with LDS atomics and flushes the rows that are not zero with one global
//                  atomic per counter; with more rows than the table holds path 2 runs path 1.
//   k_evid_rows    a lane per row: unknown and the verdict (pwpp_evid_finish).
//   k_evid_images  a lane per cell, only where the class image or the masked bytes are asked for: the class byte by the same
//                  functions, the masked byte from the finished rows.  Every byte is read and written by one lane, so the masked
//                  bytes may be written over the input.
// Every count is an integer sum, so the bytes do not depend on the path or on the order in which the atomics arrive.  Every loop
// is bounded: the combining by the 64 lanes of a wave, the gate's window by 81 cells, a run by 8 cells a lane, the flush by the
// table's rows.  No kernel waits for another workgroup; every __syncthreads stands in control flow that is uniform over the
// workgroup (the only early return is taken by whole workgroups, and the loops around a barrier run the same number of times in
// every lane).  A map address is formed only after the clip to the map.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwpp_dev.h"  // the launcher's prototype
#include "pwpp_evidence.h"
#include "pwpp_wave.h"

namespace {
constexpr int kBlock = 256;
constexpr int kRunCells = 8;           // cells a lane of path 2 visits: a run of 2048 cells a workgroup
constexpr bool kEvidDefaultLds = false;  // the meaning of path 0, by tools/evidence_cost.py: path 1 wins 256 x 256 cells (profiles/evidence_cost.txt)

struct EvidCall {
    PwppMatchGeometry G;  // the map, and the label images' grid as the frame
    PwppEvidenceRule R;
    int32_t frames, n_poses, max_rows, occupied_at, free_at;
    uint32_t cells;      // of one frame: nx * ny (<= 2^30)
    uint32_t map_cells;  // of one map: NX * NY (<= 2^30)
    uint32_t per_frame;  // workgroups of the launch for one frame
};

__global__ __launch_bounds__(kBlock) void k_evid_init(EvidCall C, unsigned long long *rows) {
    const size_t n = (size_t)C.frames * (size_t)C.max_rows * (sizeof(PwppClusterEvidence) / 8);
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) rows[i] = 0;
}

// what a lane knows of its cell
struct EvidLane {
    int32_t row, E;
    bool is_row, landed, occupied, free_;
};

template <bool RECIP>
__device__ inline EvidLane evid_lane(const EvidCall &C, const int32_t *label_f, const double *pose, const int16_t *map_k, uint32_t i) {
    EvidLane L = {-1, 0, false, false, false, false};
    if (i >= C.cells) return L;
    L.row = label_f[i];
    L.is_row = pwpp_evid_row(L.row, C.max_rows);
    if (!L.is_row || !map_k) return L;
    const int iy = (int)(i / (uint32_t)C.G.nx), ix = (int)(i - (uint32_t)iy * (uint32_t)C.G.nx);
    int32_t Jx = 0, Jy = 0;
    if (!pwpp_evid_landed<RECIP>(C.G, pose, ix, iy, Jx, Jy)) return L;
    L.landed = true;
    L.E = pwpp_evid_read(map_k, Jx, Jy, C.R.gate, C.G.NX, C.G.NY);
    const int8_t cls = pwpp_evid_class(L.E, C.occupied_at, C.free_at);
    L.occupied = cls == (int8_t)PWPP_FUSE_OCCUPIED, L.free_ = cls == (int8_t)PWPP_FUSE_FREE;
    return L;
}

// The lanes of a wave that hold the same row become one (wave_for_each_group, pwpp_wave.h; every lane of the wave calls it, is_row
// = false: the lane holds no row): the first of them hands the group's counters and sum to `add`.  |E| <= 2^15, so a wave's sum
// stays in an int32.
template <class Add>
__device__ inline void wave_rows(const EvidLane &L, Add add) {
    const uint64_t m_landed = __ballot(L.landed), m_occupied = __ballot(L.occupied), m_free = __ballot(L.free_);
    wave_for_each_group(L.row, L.is_row, [&](int lead, unsigned long long same, bool mine) {
        const int32_t s = wave_sum<int32_t>(L.landed && mine ? L.E : 0);
        if (lane_id() == lead)  // (a lane of the group: L.row is the group's row)
            add(L.row, (int32_t)__popcll(same), (int32_t)__popcll(same & m_landed), (int32_t)__popcll(same & m_occupied), (int32_t)__popcll(same & m_free), (int64_t)s);
    });
}

__device__ inline void row_add(PwppClusterEvidence *row, int32_t cells, int32_t landed, int32_t occupied, int32_t free_, int64_t sum) {
    atomicAdd(&row->cells, cells);
    if (landed == 0) return;  // (then the others are 0 too)
    atomicAdd(&row->landed, landed);
    if (occupied != 0) atomicAdd(&row->occupied, occupied);
    if (free_ != 0) atomicAdd(&row->free, free_);
    if (sum != 0) atomicAdd(reinterpret_cast<unsigned long long *>(&row->sum), (unsigned long long)sum);  // (two's complement: the sum of the bits is the bits of the sum)
}

// what a workgroup of either path needs of its frame
struct EvidFrame {
    const int32_t *label_f;
    const double *pose;
    const int16_t *map_k;
    PwppClusterEvidence *rows_f;
};
__device__ inline EvidFrame evid_frame(const EvidCall &C, uint32_t f, const int32_t *label, const double *poses, const int32_t *map_of, const int16_t *map,
                                       PwppClusterEvidence *rows) {
    const int32_t k = map_of[f];
    return EvidFrame{label + (size_t)f * C.cells, poses + (C.n_poses == 1 ? (size_t)0 : (size_t)f * 6), k < 0 ? nullptr : map + (size_t)k * C.map_cells,
                     rows + (size_t)f * (size_t)C.max_rows};
}

// path 1: the output rows take the atomics
template <bool RECIP>
__global__ __launch_bounds__(kBlock) void k_evid_count(EvidCall C, const int32_t *label, const double *poses, const int32_t *map_of, const int16_t *map,
                                                       PwppClusterEvidence *rows) {
    const uint32_t f = blockIdx.x / C.per_frame, run = blockIdx.x % C.per_frame;
    if (f >= (uint32_t)C.frames) return;  // (the whole workgroup)
    const EvidFrame F = evid_frame(C, f, label, poses, map_of, map, rows);
    const EvidLane L = evid_lane<RECIP>(C, F.label_f, F.pose, F.map_k, run * kBlock + threadIdx.x);
    wave_rows(L, [&](int32_t r, int32_t cells, int32_t landed, int32_t occupied, int32_t free_, int64_t sum) {
        row_add(F.rows_f + r, cells, landed, occupied, free_, sum);
    });
}

// path 2: a table of max_rows rows in LDS takes them: the 64-bit sums first, then four counters a row
template <bool RECIP>
__global__ __launch_bounds__(kBlock) void k_evid_count_lds(EvidCall C, const int32_t *label, const double *poses, const int32_t *map_of, const int16_t *map,
                                                           PwppClusterEvidence *rows) {
    extern __shared__ unsigned long long evid_lds[];
    unsigned long long *t_sum = evid_lds;
    int32_t *t_count = reinterpret_cast<int32_t *>(evid_lds + C.max_rows);
    const uint32_t f = blockIdx.x / C.per_frame, run = blockIdx.x % C.per_frame;
    if (f >= (uint32_t)C.frames) return;  // (the whole workgroup)
    const EvidFrame F = evid_frame(C, f, label, poses, map_of, map, rows);
    for (int r = threadIdx.x; r < C.max_rows; r += kBlock) {
        t_sum[r] = 0;
        t_count[4 * r] = 0, t_count[4 * r + 1] = 0, t_count[4 * r + 2] = 0, t_count[4 * r + 3] = 0;
    }
    __syncthreads();
    for (int k = 0; k < kRunCells; ++k) {
        const uint64_t i = ((uint64_t)run * kRunCells + (uint64_t)k) * kBlock + threadIdx.x;  // (beyond the frame: no cell)
        const EvidLane L = evid_lane<RECIP>(C, F.label_f, F.pose, F.map_k, i < (uint64_t)C.cells ? (uint32_t)i : C.cells);
        wave_rows(L, [&](int32_t r, int32_t cells, int32_t landed, int32_t occupied, int32_t free_, int64_t sum) {
            atomicAdd(&t_count[4 * r], cells);
            if (landed == 0) return;
            atomicAdd(&t_count[4 * r + 1], landed);
            if (occupied != 0) atomicAdd(&t_count[4 * r + 2], occupied);
            if (free_ != 0) atomicAdd(&t_count[4 * r + 3], free_);
            if (sum != 0) atomicAdd(&t_sum[r], (unsigned long long)sum);
        });
    }
    __syncthreads();
    for (int r = threadIdx.x; r < C.max_rows; r += kBlock)
        if (t_count[4 * r] != 0) row_add(F.rows_f + r, t_count[4 * r], t_count[4 * r + 1], t_count[4 * r + 2], t_count[4 * r + 3], (int64_t)t_sum[r]);
}

__global__ __launch_bounds__(kBlock) void k_evid_rows(EvidCall C, PwppClusterEvidence *rows) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (size_t)C.frames * (size_t)C.max_rows) return;
    const PwppClusterEvidence r = rows[i];
    rows[i] = pwpp_evid_finish(C.R, r.sum, r.cells, r.landed, r.occupied, r.free);
}

template <bool RECIP>
__global__ __launch_bounds__(kBlock) void k_evid_images(EvidCall C, const int32_t *label, const int8_t *occ_in, const double *poses, const int32_t *map_of,
                                                        const int16_t *map, const PwppClusterEvidence *rows, int8_t *cell_class, int8_t *occ_out) {
    const uint32_t f = blockIdx.x / C.per_frame, run = blockIdx.x % C.per_frame;
    const uint32_t i = run * kBlock + threadIdx.x;
    if (f >= (uint32_t)C.frames || i >= C.cells) return;
    const EvidFrame F = evid_frame(C, f, label, poses, map_of, map, const_cast<PwppClusterEvidence *>(rows));
    const int32_t l = F.label_f[i];
    const size_t at = (size_t)f * C.cells + i;
    if (cell_class) {
        const int iy = (int)(i / (uint32_t)C.G.nx), ix = (int)(i - (uint32_t)iy * (uint32_t)C.G.nx);
        cell_class[at] = pwpp_evid_cell_class<RECIP>(C.G, F.pose, ix, iy, l, C.max_rows, F.map_k, C.R.gate, C.occupied_at, C.free_at);
    }
    if (occ_out) occ_out[at] = pwpp_evid_mask(l, C.max_rows, F.rows_f, occ_in[at]);
}
}  // namespace

static_assert(sizeof(PwppClusterEvidence) == 32, "a row of the evidence is 32 bytes");
static_assert(PWPP_EV_LDS_ROWS * 24 * 8 <= 160 * 1024, "eight workgroups' tables fit a CU's LDS");

int pwpp_launch_evidence(const PwppMatchGeometry *G, const PwppEvidenceRule *R, int occupied_at, int free_at, int frames, const int32_t *label, const int8_t *occ_in,
                         const double *poses, int n_poses, const int32_t *map_of, const int16_t *map, int max_rows, void *rows, int8_t *cell_class, int8_t *occ_out,
                         int path, hipStream_t stream) {
    if (frames < 1 || max_rows < 1 || (int64_t)frames * max_rows > PWPP_EV_MAX_TOTAL || pwpp_evid_rule_check(*R) != 0) return (int)hipErrorInvalidValue;
    if ((occ_in == nullptr) != (occ_out == nullptr)) return (int)hipErrorInvalidValue;
    EvidCall C;
    C.G = *G, C.R = *R, C.frames = frames, C.n_poses = n_poses, C.max_rows = max_rows, C.occupied_at = occupied_at, C.free_at = free_at;
    C.cells = (uint32_t)G->nx * (uint32_t)G->ny, C.map_cells = (uint32_t)G->NX * (uint32_t)G->NY;  // (sides <= 32768)
    const bool lds = (path == 0 ? kEvidDefaultLds : path == 2) && max_rows <= PWPP_EV_LDS_ROWS;
    const uint32_t per_block = lds ? kBlock * kRunCells : kBlock;
    C.per_frame = (C.cells + per_block - 1) / per_block;
    const uint64_t count_blocks = (uint64_t)C.per_frame * (uint64_t)frames;
    if (count_blocks > 0x7fffffffull) return (int)hipErrorInvalidValue;  // (the caller's checks exclude it: cells * frames <= 2^31)
    PwppClusterEvidence *out = static_cast<PwppClusterEvidence *>(rows);
    const size_t rows_all = (size_t)frames * (size_t)max_rows;
    const unsigned row_blocks = (unsigned)((rows_all + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_evid_init, dim3(row_blocks < 4096 ? row_blocks : 4096), dim3(kBlock), 0, stream, C, reinterpret_cast<unsigned long long *>(out));
    int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    const bool recip = G->inv_CELL != 0.0;
    if (lds) {
        const size_t bytes = (size_t)max_rows * 24;
        if (recip) hipLaunchKernelGGL(k_evid_count_lds<true>, dim3((unsigned)count_blocks), dim3(kBlock), bytes, stream, C, label, poses, map_of, map, out);
        else hipLaunchKernelGGL(k_evid_count_lds<false>, dim3((unsigned)count_blocks), dim3(kBlock), bytes, stream, C, label, poses, map_of, map, out);
    } else {
        if (recip) hipLaunchKernelGGL(k_evid_count<true>, dim3((unsigned)count_blocks), dim3(kBlock), 0, stream, C, label, poses, map_of, map, out);
        else hipLaunchKernelGGL(k_evid_count<false>, dim3((unsigned)count_blocks), dim3(kBlock), 0, stream, C, label, poses, map_of, map, out);
    }
    if ((rc = (int)hipGetLastError()) != 0) return rc;
    hipLaunchKernelGGL(k_evid_rows, dim3(row_blocks), dim3(kBlock), 0, stream, C, out);
    if ((rc = (int)hipGetLastError()) != 0 || (!cell_class && !occ_out)) return rc;
    C.per_frame = (C.cells + kBlock - 1) / kBlock;
    const uint64_t image_blocks = (uint64_t)C.per_frame * (uint64_t)frames;
    if (image_blocks > 0x7fffffffull) return (int)hipErrorInvalidValue;
    if (recip) hipLaunchKernelGGL(k_evid_images<true>, dim3((unsigned)image_blocks), dim3(kBlock), 0, stream, C, label, occ_in, poses, map_of, map, out, cell_class, occ_out);
    else hipLaunchKernelGGL(k_evid_images<false>, dim3((unsigned)image_blocks), dim3(kBlock), 0, stream, C, label, occ_in, poses, map_of, map, out, cell_class, occ_out);
    return (int)hipGetLastError();
}
