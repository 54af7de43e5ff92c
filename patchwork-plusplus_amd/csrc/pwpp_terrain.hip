// pwpp_terrain.hip -- the gfx950 (MI355X) kernel of the terrain analysis: the height step, the slope and the roughness of a
// (2r+1) x (2r+1) window around every cell of a height image, and a traversability cost from them (pwpp_terrain_grid,
// pwpp_terrain_ground; include/pwpp.h has the rules, pwpp_terrain.h the arithmetic).  A pure image operation on the handle's
// stream, like the elevation fusion: nothing of the estimate pipeline is read or written.
//
// One launch per call (more only where a call has more than 2^30 tiles):
//   k_terrain   a workgroup per (frame, tile of 32 x 8 output cells), a lane per output cell.  The tile and its halo of r cells are
//            quantised once into LDS as int32, PWPP_TERRAIN_UNKNOWN for a cell that is unknown or outside the image: the halo is
//            CLIPPED to the frame's image -- every (gx, gy) is compared with nx and ny before an address is formed -- so a window
//            never sees the neighbouring frame or the far end of the previous row.  Then every lane sums the known cells of its
//            window in integers, solves its plane in int64 and __int128 and stores each output the caller asked for once, with
//            ordinary stores.  No atomics, no workgroup waits for another, nothing is retried.
// LDS.  A half wave is one row of the tile: its 32 lanes read 32 consecutive words (ds_read_b32 banks by 32 dwords per half wave)
// or 32 consecutive 8-byte words (ds_read_b64: 64 dwords), at any row stride and any (dx, dy): no bank conflicts in either path.
// Option "terrain_path" = 1, the yardstick: k_terrain<R, false>, every lane walks its whole window, (2r+1)^2 reads.  "2":
// k_terrain<R, true>, separable -- for every row of the tile plus halo and every column of the tile the row's sums over dx are
// formed first and kept in LDS as arrays of their own (one packed word of k, sx, sxx; sz; sxz; min; max; the 64-bit szz), then a
// lane combines 2r+1 rows with their dy: (2r+1) (8 + 2r) / 8 + 6 (2r+1) reads per lane against (2r+1)^2, and a second barrier.
// "0" (default): per radius what tools/terrain_cost.py decided, kTerrainDefaultSeparable below.  All give the same bytes: integer
// sums commute.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwpp_dev.h"  // the launcher's prototype
#include "pwpp_terrain.h"

namespace {

constexpr int kTX = PWPP_TERRAIN_TILE_X, kTY = PWPP_TERRAIN_TILE_Y, kTerrainBlock = kTX * kTY;
// What option "terrain_path" = 0 means for r = 1 .. 4 (entry 0 is unused): path 2 (true) or path 1 (false).  Decided by
// tools/terrain_cost.py (profiles/terrain_cost.txt), not in advance: at r = 1 path 2 is 9 to 10 us SLOWER per 1024 frames against an
// A/A floor of 3.4 us, at r = 2, 3 and 4 it is 150, 370 and 670 us faster against floors of 4 to 12 us, with all five outputs and
// with cost alone.
constexpr bool kTerrainDefaultSeparable[PWPP_TERRAIN_MAX_R + 1] = {false, false, true, true, true};

struct TerrainCall {
    PwppTerrainRule R;
    int32_t nx, ny, frames;         // frames: of the whole call
    int32_t tiles_x, tiles;         // per frame: tiles = tiles_x * tiles_y (<= 2^22)
    int32_t frame_first, frame_end;  // this launch's frames
};

// grid ((frame_end - frame_first) * tiles)
template <int R, bool SEP>
__global__ __launch_bounds__(kTerrainBlock) void k_terrain(TerrainCall C, const float *height, uint32_t *step, uint32_t *slope, uint32_t *rough,
                                                           uint8_t *count, int8_t *cost) {
    constexpr int W = kTX + 2 * R, H = kTY + 2 * R, E = SEP ? H * kTX : 1;
    __shared__ int32_t tile[H * W];
    __shared__ uint32_t r_mask[E];
    __shared__ int32_t r_sz[E], r_sxz[E], r_min[E], r_max[E];
    __shared__ int64_t r_szz[E];

    const unsigned b = blockIdx.x, t = b % (unsigned)C.tiles;
    const int f = C.frame_first + (int)(b / (unsigned)C.tiles);
    if (f >= C.frame_end || f >= C.frames) return;  // (the whole workgroup: no barrier is missed)
    const int x0 = (int)(t % (unsigned)C.tiles_x) * kTX, y0 = (int)(t / (unsigned)C.tiles_x) * kTY;
    const size_t base = (size_t)f * ((size_t)C.nx * (size_t)C.ny);
    const int tid = (int)threadIdx.x;

    for (int i = tid; i < H * W; i += kTerrainBlock) {
        const int ly = i / W, lx = i - ly * W, gx = x0 + lx - R, gy = y0 + ly - R;
        int32_t z = PWPP_TERRAIN_UNKNOWN;
        if (gx >= 0 && gx < C.nx && gy >= 0 && gy < C.ny) z = pwpp_terrain_quantise(height[base + (size_t)gy * (size_t)C.nx + (size_t)gx]);
        tile[i] = z;
    }
    __syncthreads();

    const int tx = tid % kTX, ty = tid / kTX;
    PwppTerrainMoments M;
    pwpp_terrain_clear(M);
    if (!SEP) {
#pragma unroll
        for (int dy = -R; dy <= R; ++dy)
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) {
                const int32_t z = tile[(ty + R + dy) * W + tx + R + dx];
                if (z != PWPP_TERRAIN_UNKNOWN) pwpp_terrain_add(M, dx, dy, z);
            }
    } else {
        for (int e = tid; e < H * kTX; e += kTerrainBlock) {  // (H * kTX is a multiple of the tile's row: e keeps its column)
            const int row = e / kTX, col = e - row * kTX;
            PwppTerrainRow Wr;
            pwpp_terrain_row_clear(Wr);
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) {
                const int32_t z = tile[row * W + col + R + dx];
                if (z != PWPP_TERRAIN_UNKNOWN) pwpp_terrain_row_add(Wr, dx, z);
            }
            r_mask[e] = pwpp_terrain_row_pack(Wr), r_sz[e] = Wr.sz, r_sxz[e] = Wr.sxz, r_min[e] = Wr.zmin, r_max[e] = Wr.zmax, r_szz[e] = Wr.szz;
        }
        __syncthreads();
#pragma unroll
        for (int dy = -R; dy <= R; ++dy) {
            const int e = (ty + R + dy) * kTX + tx;
            PwppTerrainRow Wr;
            pwpp_terrain_row_unpack(r_mask[e], Wr);
            Wr.sz = r_sz[e], Wr.sxz = r_sxz[e], Wr.zmin = r_min[e], Wr.zmax = r_max[e], Wr.szz = r_szz[e];
            pwpp_terrain_add_row(M, dy, Wr);
        }
    }

    const int ix = x0 + tx, iy = y0 + ty;
    if (ix >= C.nx || iy >= C.ny) return;  // (behind the last barrier)
    const size_t at = base + (size_t)iy * (size_t)C.nx + (size_t)ix;
    if (count) count[at] = (uint8_t)M.k;
    if (!step && !slope && !rough && !cost) return;
    uint32_t s, g, q;
    int32_t c;
    pwpp_terrain_cell(C.R, M, tile[(ty + R) * W + tx + R] != PWPP_TERRAIN_UNKNOWN, s, g, q, c);
    if (step) step[at] = s;
    if (slope) slope[at] = g;
    if (rough) rough[at] = q;
    if (cost) cost[at] = (int8_t)c;
}

template <int R>
void launch_r(bool separable, const TerrainCall &C, dim3 grid, hipStream_t stream, const float *height, uint32_t *step, uint32_t *slope, uint32_t *rough,
              uint8_t *count, int8_t *cost) {
    if (separable) hipLaunchKernelGGL((k_terrain<R, true>), grid, dim3(kTerrainBlock), 0, stream, C, height, step, slope, rough, count, cost);
    else hipLaunchKernelGGL((k_terrain<R, false>), grid, dim3(kTerrainBlock), 0, stream, C, height, step, slope, rough, count, cost);
}

}  // namespace

// pwpp_terrain_grid on device memory.  The caller has checked the sides (<= 32768), nx * ny * frames <= 2^31, the rule (radius
// 1 .. 4, min_known, the limits, run = 1024 * cell) and that not every output is null; height, step, slope and rough are 4-byte aligned.
extern "C" int pwpp_launch_terrain(const PwppTerrainRule *R, int nx, int ny, int frames, const float *height, float *step, float *slope, float *rough,
                                   uint8_t *count, int8_t *cost, int path, hipStream_t stream) {
    if (R->radius < 1 || R->radius > PWPP_TERRAIN_MAX_R) return (int)hipErrorInvalidValue;
    TerrainCall C;
    C.R = *R;
    C.nx = nx, C.ny = ny, C.frames = frames;
    C.tiles_x = (nx + kTX - 1) / kTX;
    C.tiles = C.tiles_x * ((ny + kTY - 1) / kTY);
    const int per_launch = ((int32_t)1 << 30) / C.tiles;  // (>= 256: a launch has at most 2^30 workgroups)
    const bool separable = path == 0 ? kTerrainDefaultSeparable[R->radius] : path == 2;
    uint32_t *s = reinterpret_cast<uint32_t *>(step), *g = reinterpret_cast<uint32_t *>(slope), *q = reinterpret_cast<uint32_t *>(rough);
    for (int64_t first = 0; first < (int64_t)frames; first += per_launch) {
        C.frame_first = (int32_t)first, C.frame_end = (int32_t)(first + per_launch < (int64_t)frames ? first + per_launch : (int64_t)frames);
        const dim3 grid((unsigned)(C.frame_end - C.frame_first) * (unsigned)C.tiles);
        switch (R->radius) {
        case 1: launch_r<1>(separable, C, grid, stream, height, s, g, q, count, cost); break;
        case 2: launch_r<2>(separable, C, grid, stream, height, s, g, q, count, cost); break;
        case 3: launch_r<3>(separable, C, grid, stream, height, s, g, q, count, cost); break;
        default: launch_r<4>(separable, C, grid, stream, height, s, g, q, count, cost); break;
        }
        const int rc = (int)hipGetLastError();
        if (rc != 0) return rc;
    }
    return 0;
}
