// pwpp_beams.hip -- gfx950 (MI355X) kernels of the per-beam free space: every endpoint cell's beam traced from the sensor's cell
// through the grid, per crossed cell the number of beams that passed and the lowest of them, and the occupancy byte derived from
// them (pwpp_beam_grid, pwpp_beam_ground; pwpp_beams.h has the arithmetic, include/pwpp.h the rules).  Pure image operations on the
// handle's stream, like the two lines of sight: nothing of the estimate pipeline is read or written.
//
// A scatter: the work is the sum of n over the endpoint cells, and many beams cross the same cells near the origin.  Two paths:
//   PATH 1, the yardstick, three launches:
//     k_beam_fill     passes = 0, low = INT32_MAX
//     k_beam_scatter  a lane per cell of the image; the lane of an endpoint cell walks its beam (pwpp_beams_walk) with an atomicAdd
//                     and an atomicMin in global memory at every crossed cell
//     k_beam_finish   a lane per cell: low becomes PWPP_VIEW_NO_HEIGHT where passes == 0, and the byte
//   PATH 2, one launch, k_beam_tile: a workgroup owns one tile of 64 x 64 cells of one frame and keeps the tile's passes and low in
//     LDS (32 KiB).  It visits the frame's cells in chunks of 256, a lane per cell; an endpoint whose beam can cross the tile
//     (pwpp_beams_near_tile, pwpp_beams_tile_span) is appended to a queue in LDS at the place a block scan gives it, and as soon
//     as 256 are queued every lane walks one of them over the k that lie in the tile (pwpp_beams_walk_tile: a jump to the first,
//     steps to the last), with LDS atomics.  Then the tile is written out with plain stores, the byte with it.  No fill, no global
//     atomics, every word of the outputs written by exactly one lane.
// Sums and minima of integers: the result is the same in whatever order the atomics land, a function of the inputs alone.  Every
// loop is bounded by max(nx, ny) or by the cells of a frame, no workgroup waits for another, every index is compared with the image
// (path 1) or the tile (path 2) before an address is formed, nothing is retried.  "beams_path" = 0 is path 2 (pwpp_beams_path_of).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwpp_beams.h"
#include "pwpp_dev.h"  // the launchers' prototypes
#include "pwpp_wave.h"

namespace {

constexpr int kBeamBlock = 256;
constexpr int kTile = PWPP_BEAMS_TILE, kTileCells = kTile * kTile;
constexpr int kQueue = 2 * kBeamBlock;  // at most 255 wait when a chunk's 256 arrive

struct BeamImage {
    int32_t nx, ny;
    int32_t per_frame;  // nx * ny (<= 2^30)
    int32_t max_range;
    int32_t ox, oy, eye;  // the origin of every frame when `origins` is null
    uint32_t min_pass;
    int32_t clearance;
    int32_t runs;              // path 1: block = frame * runs + run of 256 cells
    int32_t tiles_x, tiles_y;  // path 2: block = (frame * tiles_y + ty) * tiles_x + tx
};

struct BeamOrigin {
    int ox, oy, eye;
};
__device__ __forceinline__ BeamOrigin beam_origin(const BeamImage &I, const int32_t *origins, unsigned f) {  // (inside the image: the host checked)
    if (!origins) return BeamOrigin{I.ox, I.oy, I.eye};
    return BeamOrigin{origins[3 * (size_t)f], origins[3 * (size_t)f + 1], origins[3 * (size_t)f + 2]};
}

__global__ __launch_bounds__(kBeamBlock) void k_beam_fill(int64_t cells, uint32_t *passes, int32_t *low) {
    const int64_t c = (int64_t)blockIdx.x * kBeamBlock + threadIdx.x;
    if (c >= cells) return;
    passes[c] = 0u;
    low[c] = INT32_MAX;
}

// the crossed cells of one frame in global memory
struct GlobalSink {
    uint32_t *passes;
    int32_t *low;
    int32_t nx, ny;
    uint32_t weight;
    __device__ __forceinline__ void cross(int x, int y, int32_t height) const {
        if ((unsigned)x >= (unsigned)nx || (unsigned)y >= (unsigned)ny) return;
        const size_t c = (size_t)y * (size_t)nx + (size_t)x;
        atomicAdd(passes + c, weight);
        atomicMin(low + c, height);
    }
};

// PATH 1.  grid (frames * runs)
__global__ __launch_bounds__(kBeamBlock) void k_beam_scatter(BeamImage I, const int32_t *hits, const int32_t *zmin, const int32_t *origins, uint32_t *passes,
                                                              int32_t *low) {
    const unsigned b = blockIdx.x, run = b % (unsigned)I.runs, f = b / (unsigned)I.runs;
    const int c = (int)run * kBeamBlock + (int)threadIdx.x;
    if (c >= I.per_frame) return;
    const size_t fbase = (size_t)f * (size_t)I.per_frame;
    const int32_t h = hits[fbase + (size_t)c], z = zmin[fbase + (size_t)c];
    if (!pwpp_beams_endpoint(h, z)) return;
    const BeamOrigin o = beam_origin(I, origins, f);
    const int ey = c / I.nx, ex = c - ey * I.nx;
    GlobalSink sink{passes + fbase, low + fbase, I.nx, I.ny, (uint32_t)h};
    pwpp_beams_walk(sink, o.ox, o.oy, ex, ey, o.eye, z, I.max_range);
}

// what both paths write of a cell once its sums stand
__device__ __forceinline__ void beam_cell_out(const BeamImage &I, size_t c, uint32_t p, int32_t l, const int32_t *target, const int8_t *occ_in, uint32_t *passes,
                                              int32_t *low, int8_t *occupancy) {
    l = pwpp_beams_low(p, l);
    passes[c] = p;
    low[c] = l;
    if (occupancy) {
        const int8_t base = occ_in ? occ_in[c] : (int8_t)PWPP_VIS_UNKNOWN;
        occupancy[c] = pwpp_beams_occupancy(base, p, l, target != nullptr, target ? target[c] : 0, I.min_pass, I.clearance);
    }
}

__global__ __launch_bounds__(kBeamBlock) void k_beam_finish(BeamImage I, int64_t cells, const int32_t *target, const int8_t *occ_in, uint32_t *passes, int32_t *low,
                                                             int8_t *occupancy) {
    const int64_t c = (int64_t)blockIdx.x * kBeamBlock + threadIdx.x;
    if (c >= cells) return;
    beam_cell_out(I, (size_t)c, passes[c], low[c], target, occ_in, passes, low, occupancy);
}

// the crossed cells of one tile in LDS
struct TileSink {
    uint32_t *passes;
    int32_t *low;
    int32_t x0, y0;
    uint32_t weight;
    __device__ __forceinline__ void cross(int x, int y, int32_t height) const {
        const unsigned lx = (unsigned)(x - x0), ly = (unsigned)(y - y0);
        if (lx >= (unsigned)kTile || ly >= (unsigned)kTile) return;
        atomicAdd(passes + ly * kTile + lx, weight);
        atomicMin(low + ly * kTile + lx, height);
    }
};

// PATH 2.  grid (frames * tiles_y * tiles_x)
__global__ __launch_bounds__(kBeamBlock) void k_beam_tile(BeamImage I, const int32_t *hits, const int32_t *zmin, const int32_t *target, const int8_t *occ_in,
                                                           const int32_t *origins, uint32_t *passes, int32_t *low, int8_t *occupancy) {
    __shared__ uint32_t s_pass[kTileCells];
    __shared__ int32_t s_low[kTileCells];
    __shared__ int32_t s_cell[kQueue], s_z[kQueue], s_hits[kQueue];
    __shared__ unsigned s_wave[kBeamBlock / 64][1];
    const unsigned b = blockIdx.x, tx = b % (unsigned)I.tiles_x, ty = (b / (unsigned)I.tiles_x) % (unsigned)I.tiles_y;
    const unsigned f = b / ((unsigned)I.tiles_x * (unsigned)I.tiles_y);
    const int x0 = (int)tx * kTile, y0 = (int)ty * kTile, x1 = min(I.nx, x0 + kTile) - 1, y1 = min(I.ny, y0 + kTile) - 1;
    const size_t fbase = (size_t)f * (size_t)I.per_frame;
    const BeamOrigin o = beam_origin(I, origins, f);
    for (int i = threadIdx.x; i < kTileCells; i += kBeamBlock) s_pass[i] = 0u, s_low[i] = INT32_MAX;
    __syncthreads();
    const auto walk = [&](int q) {
        const int c = s_cell[q], ey = c / I.nx, ex = c - ey * I.nx;
        TileSink sink{s_pass, s_low, x0, y0, (uint32_t)s_hits[q]};
        pwpp_beams_walk_tile(sink, o.ox, o.oy, ex, ey, o.eye, s_z[q], I.max_range, x0, y0, x1, y1);
    };
    int queued = 0;  // (the same in every lane)
    for (int base = 0; base < I.per_frame; base += kBeamBlock) {
        const int c = base + (int)threadIdx.x;
        int32_t h = 0, z = PWPP_VIEW_NONE_HEIGHT;
        bool take = false;
        if (c < I.per_frame) {
            h = hits[fbase + (size_t)c], z = zmin[fbase + (size_t)c];
            if (pwpp_beams_endpoint(h, z)) {
                const int ey = c / I.nx, ex = c - ey * I.nx;
                if (pwpp_beams_near_tile(o.ox, o.oy, ex, ey, x0, y0, x1, y1)) {
                    PwppVisLine L;
                    pwpp_vis_line(o.ox, o.oy, ex, ey, L);
                    uint32_t k0, k1;
                    take = pwpp_beams_tile_span(L, I.max_range, x0, y0, x1, y1, k0, k1);
                }
            }
        }
        unsigned v[1] = {take ? 1u : 0u}, total[1];
        block_excl_scan<1, kBeamBlock / 64>(v, s_wave, total);
        if (take) {
            const int q = queued + (int)v[0];  // (< kQueue: queued <= 255)
            s_cell[q] = c, s_z[q] = z, s_hits[q] = h;
        }
        queued += (int)total[0];
        __syncthreads();
        if (queued >= kBeamBlock) {
            queued -= kBeamBlock;
            walk(queued + (int)threadIdx.x);
            __syncthreads();  // (the queue's top is free again)
        }
    }
    if ((int)threadIdx.x < queued) walk((int)threadIdx.x);
    __syncthreads();
    for (int i = threadIdx.x; i < kTileCells; i += kBeamBlock) {
        const int x = x0 + (i & (kTile - 1)), y = y0 + i / kTile;
        if (x > x1 || y > y1) continue;
        beam_cell_out(I, fbase + (size_t)y * (size_t)I.nx + (size_t)x, s_pass[i], s_low[i], target, occ_in, passes, low, occupancy);
    }
}

}  // namespace

// What "beams_path" resolves to.  0 is what profiles/beams_cost.txt measured: path 2 wins every configuration, by far more than the
// noise -- on 1024 KITTI frames 7.7 against 13.9 ms unlimited and 6.3 against 10.7 ms within 20 m on 256 x 256 cells, 0.09 against 1.4 ms
// and 0.06 against 1.0 ms on 64 x 64 -- so there is no per-call rule to state.
extern "C" int pwpp_beams_path_of(int path) { return path != 0 ? path : 2; }

// pwpp_beam_grid on device memory.  `origins`: device memory, {ox, oy, eye} per frame, or null: (ox, oy, eye) for every frame.  The
// caller has checked nx, ny <= 32768, nx * ny * frames <= 2^31, max_range, min_pass, clearance, that every origin lies inside the image
// and every eye within +-2^30; target, occ_in and occupancy may be null, occupancy may be occ_in.
extern "C" int pwpp_launch_beam_grid(int nx, int ny, int frames, const int32_t *hits, const int32_t *zmin, const int32_t *target, const int8_t *occ_in, int ox,
                                     int oy, int eye, const int32_t *origins, int max_range, int min_pass, int clearance, int path, int32_t *passes, int32_t *low,
                                     int8_t *occupancy, hipStream_t stream) {
    BeamImage I;
    I.nx = nx, I.ny = ny, I.per_frame = nx * ny, I.max_range = max_range, I.ox = ox, I.oy = oy, I.eye = eye;
    I.min_pass = (uint32_t)min_pass, I.clearance = clearance;
    I.runs = (I.per_frame + kBeamBlock - 1) / kBeamBlock;
    I.tiles_x = (nx + kTile - 1) / kTile, I.tiles_y = (ny + kTile - 1) / kTile;
    const int64_t cells = (int64_t)I.per_frame * frames;
    uint32_t *upasses = reinterpret_cast<uint32_t *>(passes);
    if (pwpp_beams_path_of(path) == 1) {
        const int64_t blocks = (int64_t)frames * I.runs;
        if (blocks > INT32_MAX) return (int)hipErrorInvalidConfiguration;
        const unsigned flat = (unsigned)((cells + kBeamBlock - 1) / kBeamBlock);
        hipLaunchKernelGGL(k_beam_fill, dim3(flat), dim3(kBeamBlock), 0, stream, cells, upasses, low);
        hipLaunchKernelGGL(k_beam_scatter, dim3((unsigned)blocks), dim3(kBeamBlock), 0, stream, I, hits, zmin, origins, upasses, low);
        hipLaunchKernelGGL(k_beam_finish, dim3(flat), dim3(kBeamBlock), 0, stream, I, cells, target, occ_in, upasses, low, occupancy);
    } else {
        const int64_t blocks = (int64_t)frames * I.tiles_x * I.tiles_y;
        if (blocks > INT32_MAX) return (int)hipErrorInvalidConfiguration;
        hipLaunchKernelGGL(k_beam_tile, dim3((unsigned)blocks), dim3(kBeamBlock), 0, stream, I, hits, zmin, target, occ_in, origins, upasses, low, occupancy);
    }
    return (int)hipGetLastError();
}
