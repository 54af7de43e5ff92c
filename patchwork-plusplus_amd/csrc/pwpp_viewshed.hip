// pwpp_viewshed.hip -- gfx950 (MI355X) kernels of the height-aware line of sight: for every cell of an occupancy image with heights
// the nearest occupied cell on the digital line from the sensor's cell that HIDES it from an eye at a given height, the lowest
// height seen at the cell, and the tri-state occupancy byte (pwpp_viewshed_grid, pwpp_viewshed_obstacles; include/pwpp.h has the
// rules, pwpp_viewshed.h the arithmetic).  Pure image operations on the handle's stream, like the visibility: nothing of the
// estimate pipeline is read or written.
//
// "viewshed_path" 1, the yardstick: one launch, k_view_walk<1>, a workgroup per (frame, run of 256 cells in row-major order), a lane
//     per cell; every test of a cell reads count, every rise reads block, in global memory.
// "viewshed_path" 2: two launches, each frame on its own:
//   1  k_view_pack   k_vis_pack's deal: a wave per 64 cells of an image row, count >= min_count -> one ballot -> two words of the
//                    bit image (the handle's cluster buffer, rows padded to whole words)
//   2  k_view_walk<2>  the same runs and lanes as path 1.  The rows of the bit image between the origin's row and the run's rows --
//                    all a walk of the run can touch -- are copied into LDS first when the frame's whole bit image fits
//                    (PWPP_VIEW_LDS_BYTES; the furthest run needs all of it); a larger image is read from global memory.  A lane
//                    tests its line's cells in LDS and fetches a rise from global memory only where a bit is set.
// Without a shadow image a lane stops at the first blocker that hides its cell; with one it walks the whole line, or up to an opaque
// blocker.  k_view_quantise turns the chained call's float rasters into the two height images.
// Every word of `first` and `shadow` and every byte of `occupancy` is written by exactly one lane, every loop is bounded by
// max(nx, ny) or by the words of the copy, no workgroup waits for another, there are no atomics, every index is compared with nx and
// ny before an address is formed (the accessors of pwpp_visibility.h and pwpp_viewshed.h): the outputs are functions of the inputs alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwpp_dev.h"  // the launchers' prototypes
#include "pwpp_viewshed.h"

namespace {

constexpr int kPackBlock = 256;  // pass 1: four waves, 64 cells each
constexpr int kWalkBlock = 256;  // pass 2: 256 lanes, a cell each
constexpr int kRun = kWalkBlock;

struct ViewImage {
    int32_t nx, ny;
    int32_t per_frame;  // nx * ny (<= 2^30)
    int32_t min_count, min_seen, max_range;
    int32_t row_words;  // pwpp_vis_row_words(nx)
    int32_t ox, oy, eye;  // the origin of every frame when `origins` is null
    int32_t runs, lds;    // how the walk is dealt: block = frame * runs + run
};

// 1: grid ceil(units / 4), units = frames * ny * chunks waves, chunks = ceil(nx / 64).
__global__ __launch_bounds__(kPackBlock) void k_view_pack(ViewImage I, int64_t units, int32_t chunks, const int32_t *count, uint32_t *bits) {
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
__global__ __launch_bounds__(kWalkBlock) void k_view_walk(ViewImage I, const int32_t *count, const int32_t *block, const int32_t *target, const int32_t *seen,
                                                          const uint32_t *bits, const int32_t *origins, int32_t *first, int32_t *shadow, int8_t *occupancy) {
    extern __shared__ uint32_t s_bits[];
    const unsigned b = blockIdx.x, run = b % (unsigned)I.runs, f = b / (unsigned)I.runs;
    const int ox = origins ? origins[3 * (size_t)f] : I.ox, oy = origins ? origins[3 * (size_t)f + 1] : I.oy;  // (inside the image: the host checked)
    const int eye = origins ? origins[3 * (size_t)f + 2] : I.eye;
    const int c0 = (int)run * kRun, c1 = min(I.per_frame, c0 + kRun);  // the run's cells, row-major (per_frame <= 2^30)
    const size_t fbase = (size_t)f * (size_t)I.per_frame;
    PwppVisBits bit{nullptr, I.row_words, 0, I.ny, I.nx};
    if (PATH == 2) {
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
__global__ __launch_bounds__(256) void k_view_quantise(int64_t cells, const float *ground, const float *top, int32_t *target, int32_t *block) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= cells) return;
    const float g = ground[c];
    target[c] = pwpp_view_units((double)g);
    block[c] = pwpp_view_units((double)g + (double)top[c]);
}

}  // namespace

// What "viewshed_path" resolves to for a call.  0 is a per-call rule, what profiles/viewshed_cost.txt measured: path 2 wins the
// unlimited walk (3 to 4 % on 256 x 256 cells) and loses under max_range 40 (1 to 4 %: the pack and the copy into LDS are paid for
// lines that are short or not walked at all); on 64 x 64 cells the two are within the noise.
extern "C" int pwpp_viewshed_path_of(int path, int max_range) { return path != 0 ? path : (max_range == 0 ? 2 : 1); }

// Words of the handle's cluster buffer the kernels need for an image of nx * ny * frames cells: the bit image (none on path 1).
extern "C" size_t pwpp_viewshed_work_words(int nx, int ny, int frames, int path, int max_range) {
    return pwpp_viewshed_path_of(path, max_range) == 1 ? 0 : (size_t)pwpp_vis_row_words(nx) * (size_t)ny * (size_t)frames;
}

// pwpp_viewshed_grid on device memory.  `work`: pwpp_viewshed_work_words words.  `origins`: device memory, {ox, oy, eye} per frame, or
// null: (ox, oy, eye) for every frame.  The caller has checked nx, ny <= 32768, nx * ny * frames <= 2^31, min_count, min_seen,
// max_range and that every origin lies inside the image; block, target, seen, shadow and occupancy may be null.
extern "C" int pwpp_launch_viewshed_grid(int nx, int ny, int frames, const int32_t *count, int min_count, const int32_t *block, const int32_t *target,
                                         const int32_t *seen, int min_seen, int ox, int oy, int eye, const int32_t *origins, int max_range, int path,
                                         int32_t *first, int32_t *shadow, int8_t *occupancy, uint32_t *work, hipStream_t stream) {
    ViewImage I;
    I.nx = nx, I.ny = ny, I.per_frame = nx * ny, I.min_count = min_count, I.min_seen = min_seen, I.max_range = max_range;
    I.row_words = pwpp_vis_row_words(nx);
    I.ox = ox, I.oy = oy, I.eye = eye;
    I.runs = (I.per_frame + kRun - 1) / kRun;
    path = pwpp_viewshed_path_of(path, max_range);
    const size_t frame_bytes = (size_t)I.row_words * (size_t)ny * sizeof(uint32_t);
    I.lds = path == 2 && frame_bytes <= (size_t)PWPP_VIEW_LDS_BYTES;
    const int64_t walk_blocks = (int64_t)frames * I.runs;
    const int32_t chunks = (nx + 63) / 64;
    const int64_t units = (int64_t)frames * ny * chunks, pack_blocks = (units + kPackBlock / 64 - 1) / (kPackBlock / 64);
    if (walk_blocks > INT32_MAX || pack_blocks > INT32_MAX) return (int)hipErrorInvalidConfiguration;
    if (path == 1) {
        hipLaunchKernelGGL(k_view_walk<1>, dim3((unsigned)walk_blocks), dim3(kWalkBlock), 0, stream, I, count, block, target, seen, nullptr, origins, first,
                           shadow, occupancy);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(k_view_pack, dim3((unsigned)pack_blocks), dim3(kPackBlock), 0, stream, I, units, chunks, count, work);
    const size_t lds_bytes = I.lds ? frame_bytes : 0;
    if (lds_bytes > 64 * 1024) {  // (beyond the 64 KiB a kernel may ask for unannounced)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_view_walk<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k_view_walk<2>, dim3((unsigned)walk_blocks), dim3(kWalkBlock), lds_bytes, stream, I, count, block, target, seen, work, origins, first,
                       shadow, occupancy);
    return (int)hipGetLastError();
}

extern "C" int pwpp_launch_viewshed_quantise(size_t cells, const float *ground, const float *top, int32_t *target, int32_t *block, hipStream_t stream) {
    if (cells > 0)
        hipLaunchKernelGGL(k_view_quantise, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, (int64_t)cells, ground, top, target, block);
    return (int)hipGetLastError();
}
