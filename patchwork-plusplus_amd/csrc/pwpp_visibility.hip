// pwpp_visibility.hip -- gfx950 (MI355X) kernels of the line-of-sight free space: for every cell of an occupancy image the first
// occupied cell on the digital line from the sensor's cell, and the tri-state occupancy byte derived from it
// (pwpp_visibility_grid, pwpp_visibility_obstacles; include/pwpp.h has the rules, pwpp_visibility.h the arithmetic).  Pure image
// operations on the handle's stream, like the distances: nothing of the estimate pipeline is read or written.
//
// Two launches per call, each frame on its own:
//   1  k_vis_pack   a wave per 64 cells of an image row: count >= min_count -> one ballot -> two words of the bit image (the working
//                   image in the handle's cluster buffer, rows padded to whole words: 8 KiB for 256 x 256 cells)
//   2  k_vis_walk   a workgroup per (frame, run of 256 cells in row-major order), a lane per cell: the lane order that measured
//                   fastest (profiles/obstacle_visibility_cost.txt: against tiles of 64 x 4, 32 x 8 and 16 x 16 cells) -- a wave's
//                   cells lie in one row, their lines stay close together.  The rows of the bit image between the origin's row and
//                   the run's rows -- all a walk of the run can touch -- are copied into LDS first when the frame's whole bit image
//                   fits (the furthest run needs all of it); a larger image is read from global memory.  Each lane then walks its
//                   cell's line from the origin outward and stops at the first hit (pwpp_vis_walk).
//                   Option "visibility_path" = 1, the yardstick: no bit image, no LDS, every test reads count in global memory.
// Every word of `first` and every byte of `occupancy` is written by exactly one lane, every loop is bounded by max(nx, ny) or by the
// words of the copy, no workgroup waits for another, every index is compared with nx and ny before an address is formed
// (pwpp_visibility.h's accessors), nothing is retried: the outputs are functions of the count image and the origins alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwpp_dev.h"  // the launchers' prototypes
#include "pwpp_visibility.h"

namespace {

constexpr int kPackBlock = 256;                 // pass 1: four waves, 64 cells each
constexpr int kWalkBlock = 256;                 // pass 2: 256 lanes
#ifndef PWPP_VIS_CELLS_PER_LANE  // (tools/ab_build.sh <name> -DPWPP_VIS_CELLS_PER_LANE=..: what profiles/obstacle_visibility_cost.txt compares)
#define PWPP_VIS_CELLS_PER_LANE 1
#endif
constexpr int kCellsPerLane = PWPP_VIS_CELLS_PER_LANE;
constexpr int kRun = kWalkBlock * kCellsPerLane;  // cells of a workgroup: a run of the frame in row-major order; lane l takes cells l, l + 256, ...
constexpr size_t kLdsBytes = 128 * 1024;        // the largest bit image of a frame kept in LDS: 1024 x 1024 cells, of the CU's 160 KiB

struct VisImage {
    int32_t nx, ny;
    int32_t per_frame;  // nx * ny (<= 2^30)
    int32_t min_count, max_range;
    int32_t row_words;  // pwpp_vis_row_words(nx)
    int32_t ox, oy;     // the origin of every frame when `origins` is null
    // how pass 2 is dealt: block = frame * runs + run
    int32_t runs, lds;
};

// 1: grid ceil(units / 4), units = frames * ny * chunks waves, chunks = ceil(nx / 64).
__global__ __launch_bounds__(kPackBlock) void k_vis_pack(VisImage I, int64_t units, int32_t chunks, const int32_t *count, uint32_t *bits) {
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * (kPackBlock / 64) + (threadIdx.x >> 6);
    if (u >= units) return;  // (the whole wave)
    const int64_t r = u / chunks;  // the row among frames * ny
    const int k = (int)(u % chunks), x = k * 64 + lane;
    const unsigned long long mask = __ballot(x < I.nx && count[(size_t)r * (size_t)I.nx + (size_t)x] >= I.min_count);
    uint32_t *row = bits + (size_t)r * (size_t)I.row_words;
    if (lane == 0) row[2 * k] = pwpp_vis_ballot_word(mask, 0);
    if (lane == 32 && 2 * k + 1 < I.row_words) row[2 * k + 1] = pwpp_vis_ballot_word(mask, 1);
}

// 2: grid (frames * runs).  PATH 1 never uses the bit image or LDS.
template <int PATH>
__global__ __launch_bounds__(kWalkBlock) void k_vis_walk(VisImage I, const int32_t *count, const uint32_t *bits, const int32_t *origins, int32_t *first,
                                                         int8_t *occupancy) {
    extern __shared__ uint32_t s_bits[];
    const unsigned b = blockIdx.x, run = b % (unsigned)I.runs, f = b / (unsigned)I.runs;
    const int ox = origins ? origins[2 * (size_t)f] : I.ox, oy = origins ? origins[2 * (size_t)f + 1] : I.oy;  // (inside the image: the host checked)
    const int c0 = (int)run * kRun, c1 = min(I.per_frame, c0 + kRun);  // the run's cells, row-major (per_frame <= 2^30)
    const size_t fbase = (size_t)f * (size_t)I.per_frame;
    PwppVisBits bit{nullptr, I.row_words, 0, I.ny, I.nx};
    if (PATH == 0) {
        bit.w = bits + (size_t)f * (size_t)I.ny * (size_t)I.row_words;
        if (I.lds) {  // the rows from the origin's to the run's: at most ny * row_words words, the launch's LDS
            const int t0 = c0 / I.nx, t1 = (c1 - 1) / I.nx;
            const int r0 = min(oy, t0), r1 = max(oy, t1);
            const int words = (r1 - r0 + 1) * I.row_words;
            const uint32_t *src = bit.w + (size_t)r0 * (size_t)I.row_words;
            for (int w = threadIdx.x; w < words; w += kWalkBlock) s_bits[w] = src[w];
            __syncthreads();
            bit.w = s_bits, bit.row0 = r0, bit.rows = r1 - r0 + 1;
        }
    }
    const PwppVisCounts cnt{count + fbase, I.nx, I.ny, I.min_count};
    for (int c = c0 + (int)threadIdx.x; c < c1; c += kWalkBlock) {
        const int cy = c / I.nx, cx = c - cy * I.nx;
        const int32_t hit = PATH == 1 ? pwpp_vis_walk(cnt, ox, oy, cx, cy, I.nx, I.max_range) : pwpp_vis_walk(bit, ox, oy, cx, cy, I.nx, I.max_range);
        first[fbase + (size_t)c] = hit;
        if (occupancy) occupancy[fbase + (size_t)c] = pwpp_vis_occupancy(PATH == 1 ? cnt.at(cx, cy) : bit.at(cx, cy), hit);
    }
}

}  // namespace

// Words of the handle's cluster buffer the kernels need for an image of nx * ny * frames cells: the bit image (none on path 1).
extern "C" size_t pwpp_visibility_work_words(int nx, int ny, int frames, int path) {
    return path == 1 ? 0 : (size_t)pwpp_vis_row_words(nx) * (size_t)ny * (size_t)frames;
}

// pwpp_visibility_grid on device memory.  `work`: pwpp_visibility_work_words words.  `origins`: device memory, {ox, oy} per frame,
// or null: (ox, oy) for every frame.  The caller has checked nx, ny <= 32768, nx * ny * frames <= 2^31, min_count, max_range and
// that every origin lies inside the image; occupancy may be null.
extern "C" int pwpp_launch_visibility_grid(int nx, int ny, int frames, const int32_t *count, int min_count, int ox, int oy, const int32_t *origins,
                                           int max_range, int path, int32_t *first, int8_t *occupancy, uint32_t *work, hipStream_t stream) {
    VisImage I;
    I.nx = nx, I.ny = ny, I.per_frame = nx * ny, I.min_count = min_count, I.max_range = max_range;
    I.row_words = pwpp_vis_row_words(nx);
    I.ox = ox, I.oy = oy;
    I.runs = (I.per_frame + kRun - 1) / kRun;
    const size_t frame_bytes = (size_t)I.row_words * (size_t)ny * sizeof(uint32_t);
    I.lds = path == 0 && frame_bytes <= kLdsBytes;
    const int64_t walk_blocks = (int64_t)frames * I.runs;
    const int32_t chunks = (nx + 63) / 64;
    const int64_t units = (int64_t)frames * ny * chunks, pack_blocks = (units + kPackBlock / 64 - 1) / (kPackBlock / 64);
    if (walk_blocks > INT32_MAX || pack_blocks > INT32_MAX) return (int)hipErrorInvalidConfiguration;
    if (path == 1) {
        hipLaunchKernelGGL(k_vis_walk<1>, dim3((unsigned)walk_blocks), dim3(kWalkBlock), 0, stream, I, count, nullptr, origins, first, occupancy);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(k_vis_pack, dim3((unsigned)pack_blocks), dim3(kPackBlock), 0, stream, I, units, chunks, count, work);
    const size_t lds_bytes = I.lds ? frame_bytes : 0;
    if (lds_bytes > 64 * 1024) {  // (beyond the 64 KiB a kernel may ask for unannounced)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_vis_walk<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k_vis_walk<0>, dim3((unsigned)walk_blocks), dim3(kWalkBlock), lds_bytes, stream, I, count, work, origins, first, occupancy);
    return (int)hipGetLastError();
}
