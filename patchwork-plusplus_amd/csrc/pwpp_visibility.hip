// pwpp_visibility.hip -- gfx950 (MI355X) kernels of the two lines of sight on an occupancy image.  The 2-D one: for every cell the
// first occupied cell on the digital line from the sensor's cell, and the tri-state occupancy byte derived from it
// (pwpp_visibility_grid, pwpp_visibility_obstacles; pwpp_visibility.h has the arithmetic).  The viewshed, the same walk with heights:
// the nearest occupied cell that HIDES the cell from an eye at a given height, the lowest height seen at it, and the byte
// (pwpp_viewshed_grid, pwpp_viewshed_obstacles; pwpp_viewshed.h).  include/pwpp.h has the rules of both.  Pure image operations on
// the handle's stream, like the distances: nothing of the estimate pipeline is read or written.
//
// Stated once for both: the dealt image (VisImage; the viewshed adds its two fields), the pack kernel, the window of rows a
// workgroup keeps in LDS (vis_window), the launch plan (vis_plan) and the words of the bit image (vis_work_words).  The walks are
// two kernels, k_vis_walk and k_view_walk: the viewshed's costs 2.2 to 5.6 times the other (profiles/viewshed_cost.txt).
//
// Two launches per call, each frame on its own:
//   1  k_vis_pack   a wave per 64 cells of an image row: count >= min_count -> one ballot -> two words of the bit image (the working
//                   image in the handle's cluster buffer, rows padded to whole words: 8 KiB for 256 x 256 cells)
//   2  k_vis_walk<2>, k_view_walk<2>
//                   a workgroup per (frame, run of 256 cells in row-major order), a lane per cell: the lane order that measured
//                   fastest (profiles/obstacle_visibility_cost.txt: against tiles of 64 x 4, 32 x 8 and 16 x 16 cells) -- a wave's
//                   cells lie in one row, their lines stay close together.  The rows of the bit image between the origin's row and
//                   the run's rows -- all a walk of the run can touch -- are copied into LDS first when the frame's whole bit image
//                   fits (PWPP_VIS_LDS_BYTES; the furthest run needs all of it); a larger image is read from global memory.  Each
//                   lane then walks its cell's line from the origin outward: the visibility stops at the first hit (pwpp_vis_walk);
//                   the viewshed fetches a rise from global memory only where a bit is set, and without a shadow image stops at
//                   the first blocker that hides its cell, with one walks the whole line or up to an opaque blocker (pwpp_view_walk).
// The yardstick of either, one launch: k_vis_walk<1>, k_view_walk<1> -- no bit image, no LDS, every test reads count in global
// memory.  Options "visibility_path" = 1 and "viewshed_path" = 1 ask for it; "viewshed_path" = 0 chooses per call (pwpp_viewshed_path_of).
// k_view_quantise turns the chained call's float rasters into the viewshed's two height images.
// Every word of `first` and `shadow` and every byte of `occupancy` is written by exactly one lane, every loop is bounded by
// max(nx, ny) or by the words of the copy, no workgroup waits for another, there are no atomics, every index is compared with nx and
// ny before an address is formed (the accessors of pwpp_visibility.h and pwpp_viewshed.h), nothing is retried: the outputs are
// functions of the inputs alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwpp_dev.h"  // the launchers' prototypes
#include "pwpp_viewshed.h"  // (and pwpp_visibility.h)

namespace {

constexpr int kPackBlock = 256;                 // pass 1: four waves, 64 cells each
constexpr int kWalkBlock = 256;                 // pass 2: 256 lanes
#ifndef PWPP_VIS_CELLS_PER_LANE  // (tools/ab_build.sh <name> -DPWPP_VIS_CELLS_PER_LANE=..: what profiles/obstacle_visibility_cost.txt compares)
#define PWPP_VIS_CELLS_PER_LANE 1
#endif
constexpr int kVisRun = kWalkBlock * PWPP_VIS_CELLS_PER_LANE;  // cells of a workgroup of the visibility: a run of the frame in row-major order; lane l takes cells l, l + 256, ...
constexpr int kViewRun = kWalkBlock;                           // ... and of the viewshed: a cell per lane

struct VisImage {
    int32_t nx, ny;
    int32_t per_frame;  // nx * ny (<= 2^30)
    int32_t min_count, max_range;
    int32_t row_words;  // pwpp_vis_row_words(nx)
    int32_t ox, oy;     // the origin of every frame when `origins` is null
    // how pass 2 is dealt: block = frame * runs + run
    int32_t runs, lds;
};
struct ViewImage : VisImage {
    int32_t min_seen, eye;  // (the eye of every frame when `origins` is null)
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

// What the run [c0, c1) of frame f walks from an origin in row oy: the frame's bit image, or (I.lds) its window in LDS, copied
// here by the whole workgroup -- the rows from the origin's to the run's: at most ny * row_words words, the launch's LDS.
__device__ __forceinline__ PwppVisBits vis_window(const VisImage &I, const uint32_t *bits, unsigned f, int oy, int c0, int c1) {
    extern __shared__ uint32_t s_bits[];
    PwppVisBits bit{bits + (size_t)f * (size_t)I.ny * (size_t)I.row_words, I.row_words, 0, I.ny, I.nx};
    if (I.lds) {
        const int t0 = c0 / I.nx, t1 = (c1 - 1) / I.nx;
        const int r0 = min(oy, t0), r1 = max(oy, t1);
        const int words = (r1 - r0 + 1) * I.row_words;
        const uint32_t *src = bit.w + (size_t)r0 * (size_t)I.row_words;
        for (int w = threadIdx.x; w < words; w += kWalkBlock) s_bits[w] = src[w];
        __syncthreads();
        bit.w = s_bits, bit.row0 = r0, bit.rows = r1 - r0 + 1;
    }
    return bit;
}

// 2: grid (frames * runs).  PATH 1 reads count: it never uses the bit image or LDS.  PATH 2 reads the bit image.
template <int PATH>
__global__ __launch_bounds__(kWalkBlock) void k_vis_walk(VisImage I, const int32_t *count, const uint32_t *bits, const int32_t *origins, int32_t *first,
                                                         int8_t *occupancy) {
    const unsigned b = blockIdx.x, run = b % (unsigned)I.runs, f = b / (unsigned)I.runs;
    const int ox = origins ? origins[2 * (size_t)f] : I.ox, oy = origins ? origins[2 * (size_t)f + 1] : I.oy;  // (inside the image: the host checked)
    const int c0 = (int)run * kVisRun, c1 = min(I.per_frame, c0 + kVisRun);  // the run's cells, row-major (per_frame <= 2^30)
    const size_t fbase = (size_t)f * (size_t)I.per_frame;
    PwppVisBits bit{nullptr, I.row_words, 0, I.ny, I.nx};
    if (PATH == 2) bit = vis_window(I, bits, f, oy, c0, c1);
    const PwppVisCounts cnt{count + fbase, I.nx, I.ny, I.min_count};
    for (int c = c0 + (int)threadIdx.x; c < c1; c += kWalkBlock) {
        const int cy = c / I.nx, cx = c - cy * I.nx;
        const int32_t hit = PATH == 1 ? pwpp_vis_walk(cnt, ox, oy, cx, cy, I.nx, I.max_range) : pwpp_vis_walk(bit, ox, oy, cx, cy, I.nx, I.max_range);
        first[fbase + (size_t)c] = hit;
        if (occupancy) occupancy[fbase + (size_t)c] = pwpp_vis_occupancy(PATH == 1 ? cnt.at(cx, cy) : bit.at(cx, cy), hit);
    }
}

template <int PATH>
__global__ __launch_bounds__(kWalkBlock) void k_view_walk(ViewImage I, const int32_t *count, const int32_t *block, const int32_t *target, const int32_t *seen,
                                                          const uint32_t *bits, const int32_t *origins, int32_t *first, int32_t *shadow, int8_t *occupancy) {
    const unsigned b = blockIdx.x, run = b % (unsigned)I.runs, f = b / (unsigned)I.runs;
    const int ox = origins ? origins[3 * (size_t)f] : I.ox, oy = origins ? origins[3 * (size_t)f + 1] : I.oy;  // (inside the image: the host checked)
    const int eye = origins ? origins[3 * (size_t)f + 2] : I.eye;
    const int c0 = (int)run * kViewRun, c1 = min(I.per_frame, c0 + kViewRun);  // the run's cells, row-major (per_frame <= 2^30)
    const size_t fbase = (size_t)f * (size_t)I.per_frame;
    PwppVisBits bit{nullptr, I.row_words, 0, I.ny, I.nx};
    if (PATH == 2) bit = vis_window(I, bits, f, oy, c0, c1);
    const PwppVisCounts cnt{count + fbase, I.nx, I.ny, I.min_count};
    const PwppViewHeights H{block ? block + fbase : nullptr, target ? target + fbase : nullptr, I.nx, I.ny, eye};
    const int c = c0 + (int)threadIdx.x;
    if (c >= c1) return;
    const int cy = c / I.nx, cx = c - cy * I.nx;
    const PwppViewResult res = PATH == 1 ? pwpp_view_walk(cnt, H, ox, oy, cx, cy, I.nx, I.max_range, shadow != nullptr)
                                         : pwpp_view_walk(bit, H, ox, oy, cx, cy, I.nx, I.max_range, shadow != nullptr);
    const int32_t hit = res.first;
    first[fbase + (size_t)c] = hit;
    if (shadow) shadow[fbase + (size_t)c] = res.shadow;
    if (occupancy) {
        const bool occupied = PATH == 1 ? cnt.at(cx, cy) : bit.at(cx, cy);
        occupancy[fbase + (size_t)c] = pwpp_view_occupancy(occupied, seen && seen[fbase + (size_t)c] >= I.min_seen, hit);
    }
}

// The chained call's height images from its float rasters: target = units(ground), block = units((double)ground + (double)top).
// Without `block` (the beams' chain) `top` is not read.
__global__ __launch_bounds__(256) void k_view_quantise(int64_t cells, const float *ground, const float *top, int32_t *target, int32_t *block) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= cells) return;
    const float g = ground[c];
    target[c] = pwpp_view_units((double)g);
    if (block) block[c] = pwpp_view_units((double)g + (double)top[c]);
}

// Words of the handle's cluster buffer a walk on PATH needs for an image of nx * ny * frames cells: the bit image (none on path 1).
size_t vis_work_words(int nx, int ny, int frames, int PATH) { return PATH == 1 ? 0 : (size_t)pwpp_vis_row_words(nx) * (size_t)ny * (size_t)frames; }

// The launch plan of a walk in runs of `run` cells.  Fills the image's shape and deal into I -- the caller has set what the walk
// compares: the thresholds, max_range, the origin -- and returns the walk's grid and LDS bytes.  `bit_walk`: the kernel that walks
// the bit image (PATH 2; null: PATH 1); the pack that writes that image into `work` is enqueued here, ahead of it.
int vis_plan(VisImage &I, int nx, int ny, int frames, int run, const void *bit_walk, const int32_t *count, uint32_t *work, hipStream_t stream,
             unsigned &walk_blocks, size_t &lds_bytes) {
    I.nx = nx, I.ny = ny, I.per_frame = nx * ny;
    I.row_words = pwpp_vis_row_words(nx);
    I.runs = (I.per_frame + run - 1) / run;
    const size_t frame_bytes = (size_t)I.row_words * (size_t)ny * sizeof(uint32_t);
    I.lds = bit_walk && frame_bytes <= (size_t)PWPP_VIS_LDS_BYTES;
    const int64_t blocks = (int64_t)frames * I.runs;
    const int32_t chunks = (nx + 63) / 64;
    const int64_t units = (int64_t)frames * ny * chunks, pack_blocks = (units + kPackBlock / 64 - 1) / (kPackBlock / 64);
    if (blocks > INT32_MAX || pack_blocks > INT32_MAX) return (int)hipErrorInvalidConfiguration;
    walk_blocks = (unsigned)blocks, lds_bytes = I.lds ? frame_bytes : 0;
    if (!bit_walk) return 0;
    hipLaunchKernelGGL(k_vis_pack, dim3((unsigned)pack_blocks), dim3(kPackBlock), 0, stream, I, units, chunks, count, work);
    if (lds_bytes > 64 * 1024)  // (beyond the 64 KiB a kernel may ask for unannounced)
        return (int)hipFuncSetAttribute(bit_walk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    return 0;
}

}  // namespace

// ("visibility_path" 0 is the bit image, PATH 2 of the kernels)
extern "C" size_t pwpp_visibility_work_words(int nx, int ny, int frames, int path) { return vis_work_words(nx, ny, frames, path == 1 ? 1 : 2); }

// pwpp_visibility_grid on device memory.  `work`: pwpp_visibility_work_words words.  `origins`: device memory, {ox, oy} per frame,
// or null: (ox, oy) for every frame.  The caller has checked nx, ny <= 32768, nx * ny * frames <= 2^31, min_count, max_range and
// that every origin lies inside the image; occupancy may be null.
extern "C" int pwpp_launch_visibility_grid(int nx, int ny, int frames, const int32_t *count, int min_count, int ox, int oy, const int32_t *origins,
                                           int max_range, int path, int32_t *first, int8_t *occupancy, uint32_t *work, hipStream_t stream) {
    VisImage I;
    I.min_count = min_count, I.max_range = max_range, I.ox = ox, I.oy = oy;
    unsigned blocks = 0;
    size_t lds_bytes = 0;
    if (const int rc = vis_plan(I, nx, ny, frames, kVisRun, path == 1 ? nullptr : reinterpret_cast<const void *>(&k_vis_walk<2>), count, work, stream, blocks, lds_bytes))
        return rc;
    if (path == 1)
        hipLaunchKernelGGL(k_vis_walk<1>, dim3(blocks), dim3(kWalkBlock), 0, stream, I, count, nullptr, origins, first, occupancy);
    else
        hipLaunchKernelGGL(k_vis_walk<2>, dim3(blocks), dim3(kWalkBlock), lds_bytes, stream, I, count, work, origins, first, occupancy);
    return (int)hipGetLastError();
}

// What "viewshed_path" resolves to for a call.  0 is a per-call rule, what profiles/viewshed_cost.txt measured: path 2 wins the
// unlimited walk (3 to 4 % on 256 x 256 cells) and loses under max_range 40 (1 to 4 %: the pack and the copy into LDS are paid for
// lines that are short or not walked at all); on 64 x 64 cells the two are within the noise.
extern "C" int pwpp_viewshed_path_of(int path, int max_range) { return path != 0 ? path : (max_range == 0 ? 2 : 1); }

extern "C" size_t pwpp_viewshed_work_words(int nx, int ny, int frames, int path, int max_range) {
    return vis_work_words(nx, ny, frames, pwpp_viewshed_path_of(path, max_range));
}

// pwpp_viewshed_grid on device memory.  `work`: pwpp_viewshed_work_words words.  `origins`: device memory, {ox, oy, eye} per frame, or
// null: (ox, oy, eye) for every frame.  The caller has checked nx, ny <= 32768, nx * ny * frames <= 2^31, min_count, min_seen,
// max_range and that every origin lies inside the image; block, target, seen, shadow and occupancy may be null.
extern "C" int pwpp_launch_viewshed_grid(int nx, int ny, int frames, const int32_t *count, int min_count, const int32_t *block, const int32_t *target,
                                         const int32_t *seen, int min_seen, int ox, int oy, int eye, const int32_t *origins, int max_range, int path,
                                         int32_t *first, int32_t *shadow, int8_t *occupancy, uint32_t *work, hipStream_t stream) {
    ViewImage I;
    I.min_count = min_count, I.max_range = max_range, I.ox = ox, I.oy = oy, I.min_seen = min_seen, I.eye = eye;
    path = pwpp_viewshed_path_of(path, max_range);
    unsigned blocks = 0;
    size_t lds_bytes = 0;
    if (const int rc = vis_plan(I, nx, ny, frames, kViewRun, path == 1 ? nullptr : reinterpret_cast<const void *>(&k_view_walk<2>), count, work, stream, blocks, lds_bytes))
        return rc;
    if (path == 1)
        hipLaunchKernelGGL(k_view_walk<1>, dim3(blocks), dim3(kWalkBlock), 0, stream, I, count, block, target, seen, nullptr, origins, first, shadow, occupancy);
    else
        hipLaunchKernelGGL(k_view_walk<2>, dim3(blocks), dim3(kWalkBlock), lds_bytes, stream, I, count, block, target, seen, work, origins, first, shadow, occupancy);
    return (int)hipGetLastError();
}

extern "C" int pwpp_launch_viewshed_quantise(size_t cells, const float *ground, const float *top, int32_t *target, int32_t *block, hipStream_t stream) {
    if (cells > 0)
        hipLaunchKernelGGL(k_view_quantise, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, (int64_t)cells, ground, top, target, block);
    return (int)hipGetLastError();
}
