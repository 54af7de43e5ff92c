// pwpp_distance.hip -- gfx950 (MI355X) kernels of the obstacle distances: the exact Euclidean distance transform of an occupancy
// image with the nearest occupied cell of every cell (pwpp_distance_grid, pwpp_distance_obstacles; include/pwpp.h has the rules,
// pwpp_distance.h the arithmetic and the argument why the two passes are exact).  Pure image operations on the handle's stream,
// like the clusters: nothing of the estimate pipeline is read or written.
//
// Two launches per call, each frame on its own:
//   1  k_dist_rows   a wave per image row: count -> gx, the nearest occupied column of the cell's own row (the working image in
//                    the handle's cluster buffer, one int32 per cell)
//   2  k_dist_cols   a workgroup per strip of 64 adjacent columns (lane = column) and tile of rows: gx -> dist2, nearest, metres.
//                    The rows of gx the tile can need are copied into LDS first when they fit -- a row of the strip is 64
//                    consecutive words, one per lane: every bank once, no conflict -- and each wave then walks outward from its
//                    cell's own row until the rows are further away than the best cell so far (pwpp_dist_scan_outward).
//                    Option "distance_path" = 1, the yardstick: gx from global memory, every row, no early exit.
// Every word of an output is written by exactly one lane, every loop is bounded by ny or by the chunks of a row, no workgroup
// waits for another, nothing is retried: the outputs are functions of the count image alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "pwpp_dev.h"  // the launchers' prototypes
#include "pwpp_distance.h"

namespace {

constexpr int kRowBlock = 256;   // pass 1: four waves, a row each
constexpr int kColBlock = 1024;  // pass 2: sixteen waves share the strip's rows in LDS: 64 KiB for 256 rows, two workgroups a CU
constexpr int kColWaves = kColBlock / 64;
constexpr int kStrip = PWPP_DIST_STRIP;  // columns of a strip = lanes of a wave

struct DistImage {
    int32_t nx, ny;
    int32_t per_frame;  // nx * ny (<= 2^30)
    int32_t min_count;
    uint32_t cap2;      // pwpp_dist_cap2(max_dist)
    // how pass 2 is dealt: block = (frame * strips + strip) * row_tiles + tile; the tile's rows [t0, t0 + tile_rows) and, with
    // lds != 0, `halo` more on either side are in LDS
    int32_t strips, row_tiles, tile_rows, halo, lds;
};

// 1: grid ceil(frames * ny / 4).  Right to left for the next occupied column at or right of every cell, then left to right for
// the last one at or left of it: the carry crosses the chunks, a lane reads back only the word it wrote itself.
__global__ __launch_bounds__(kRowBlock) void k_dist_rows(DistImage I, int64_t rows, const int32_t *count, int32_t *gx) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (kRowBlock / 64) + (threadIdx.x >> 6);
    if (r >= rows) return;  // (the whole wave)
    const int32_t *c = count + r * I.nx;
    int32_t *g = gx + r * I.nx;
    const int chunks = (I.nx + 63) / 64;
    int32_t next = -1;
    for (int k = chunks - 1; k >= 0; --k) {
        const int x = k * 64 + lane;
        const unsigned long long mask = __ballot(x < I.nx && c[x] >= I.min_count);
        const int in = pwpp_dist_right_in_chunk(mask, lane);
        if (x < I.nx) g[x] = in >= 0 ? k * 64 + in : next;
        if (mask) next = k * 64 + __builtin_ctzll(mask);
    }
    int32_t last = -1;
    for (int k = 0; k < chunks; ++k) {
        const int x = k * 64 + lane;
        const unsigned long long mask = __ballot(x < I.nx && c[x] >= I.min_count);
        const int in = pwpp_dist_left_in_chunk(mask, lane);
        if (x < I.nx) g[x] = pwpp_dist_row_pick(in >= 0 ? k * 64 + in : last, g[x], x);
        if (mask) last = k * 64 + 63 - __builtin_clzll(mask);
    }
}

// a lane's column of gx: in the frame's working image ...
struct GlobalColumn {
    const int32_t *g;  // gx of the frame + ix
    int32_t nx;
    __device__ __forceinline__ int32_t gx(int jy) const { return g[jy * nx]; }
};
// ... and in the rows [row0, ...) of the strip in LDS
struct LdsColumn {
    const int32_t *s;  // s_gx + lane
    int32_t row0;
    __device__ __forceinline__ int32_t gx(int jy) const { return s[(jy - row0) * kStrip]; }
};

// 2: grid (frames * strips * row_tiles).  PATH 1 never uses LDS.
template <int PATH>
__global__ __launch_bounds__(kColBlock) void k_dist_cols(DistImage I, double cell, const int32_t *gx, int32_t *dist2, int32_t *nearest, float *metres) {
    extern __shared__ int32_t s_gx[];
    const unsigned b = blockIdx.x, t = b % (unsigned)I.row_tiles, fs = b / (unsigned)I.row_tiles;
    const unsigned f = fs / (unsigned)I.strips, s = fs % (unsigned)I.strips;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ix = (int)s * kStrip + lane;
    const size_t fbase = (size_t)f * (size_t)I.per_frame;
    const int32_t *g = gx + fbase;
    const int t0 = (int)t * I.tile_rows, t1 = min(I.ny, t0 + I.tile_rows);
    const int row0 = max(0, t0 - I.halo), row1 = min(I.ny, t1 + I.halo);
    const bool lds = PATH == 0 && I.lds != 0;
    if (lds) {  // (row1 - row0 <= PWPP_DIST_LDS_ROWS: pwpp_dist_plan's choice of tile_rows and halo)
        for (int jy = row0 + w; jy < row1; jy += kColWaves) s_gx[(jy - row0) * kStrip + lane] = ix < I.nx ? g[jy * I.nx + ix] : -1;
        __syncthreads();
    }
    if (ix >= I.nx) return;
    for (int iy = t0 + w; iy < t1; iy += kColWaves) {
        unsigned long long key;
        if (PATH == 1) {
            GlobalColumn col{g + ix, I.nx};
            key = pwpp_dist_scan_all(col, ix, iy, I.nx, I.ny);
        } else if (lds) {
            LdsColumn col{s_gx + lane, row0};
            key = pwpp_dist_scan_outward(col, ix, iy, I.nx, I.ny, I.cap2);
        } else {
            GlobalColumn col{g + ix, I.nx};
            key = pwpp_dist_scan_outward(col, ix, iy, I.nx, I.ny, I.cap2);
        }
        int32_t d2, near;
        pwpp_dist_of_key(key, I.cap2, d2, near);
        const size_t at = fbase + (size_t)(iy * I.nx + ix);
        dist2[at] = d2;
        if (nearest) nearest[at] = near;
        if (metres) metres[at] = pwpp_dist_metres(d2, cell);
    }
}

}  // namespace

// Words of the handle's cluster buffer the kernels need for an image of nx * ny * frames cells: gx, one per cell.
extern "C" size_t pwpp_distance_work_words(int nx, int ny, int frames) { return (size_t)nx * (size_t)ny * (size_t)frames; }

// pwpp_distance_grid on device memory.  `work`: pwpp_distance_work_words words.  The caller has checked nx, ny <= 32768,
// nx * ny * frames <= 2^31, min_count and max_dist; nearest and metres may be null.
extern "C" int pwpp_launch_distance_grid(int nx, int ny, int frames, const int32_t *count, int min_count, int max_dist, double cell, int path, int32_t *dist2,
                                         int32_t *nearest, float *metres, uint32_t *work, hipStream_t stream) {
    DistImage I;
    I.nx = nx, I.ny = ny, I.per_frame = nx * ny, I.min_count = min_count, I.cap2 = pwpp_dist_cap2(max_dist);
    I.strips = (nx + kStrip - 1) / kStrip;
    const PwppDistPlan plan = pwpp_dist_plan(ny, max_dist, path);  // (the rows of a tile in LDS, or from global memory)
    I.lds = plan.lds, I.tile_rows = plan.tile_rows, I.halo = plan.halo, I.row_tiles = plan.row_tiles;
    const int64_t rows = (int64_t)frames * ny, row_blocks = (rows + kRowBlock / 64 - 1) / (kRowBlock / 64);
    const int64_t col_blocks = (int64_t)frames * I.strips * I.row_tiles;
    if (row_blocks > INT32_MAX || col_blocks > INT32_MAX) return (int)hipErrorInvalidConfiguration;
    int32_t *gx = reinterpret_cast<int32_t *>(work);
    hipLaunchKernelGGL(k_dist_rows, dim3((unsigned)row_blocks), dim3(kRowBlock), 0, stream, I, rows, count, gx);
    if (path == 1) {
        hipLaunchKernelGGL(k_dist_cols<1>, dim3((unsigned)col_blocks), dim3(kColBlock), 0, stream, I, cell, gx, dist2, nearest, metres);
    } else {
        const size_t lds_bytes = I.lds ? (size_t)std::min(ny, I.tile_rows + 2 * I.halo) * kStrip * sizeof(int32_t) : 0;
        if (lds_bytes > 64 * 1024) {  // (beyond the 64 KiB a kernel may ask for unannounced)
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dist_cols<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            if (e != hipSuccess) return (int)e;
        }
        hipLaunchKernelGGL(k_dist_cols<0>, dim3((unsigned)col_blocks), dim3(kColBlock), lds_bytes, stream, I, cell, gx, dist2, nearest, metres);
    }
    return (int)hipGetLastError();
}
