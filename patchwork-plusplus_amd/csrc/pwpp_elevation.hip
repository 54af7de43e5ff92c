// pwpp_elevation.hip -- the gfx950 (MI355X) kernel of the elevation fusion: per-frame ground heights, resampled under a pose per
// frame, accumulated into persistent elevation maps -- an int32 sum and an int16 count per cell, and the float mean derived from
// them (pwpp_fuse_height_grid, pwpp_fuse_ground; include/pwpp.h has the rules, pwpp_elevation.h the arithmetic).  A pure image
// operation on the handle's stream, like the occupancy fusion: nothing of the estimate pipeline is read or written.
//
// One launch per call:
//   k_fuse_height   a workgroup per (map, run of 256 cells in row-major order), a lane per map cell, as in k_fuse.  The lane reads
//            its start -- the shifted cell of sum_in and n_in, normalised, or nothing -- keeps sum and n in registers while it walks
//            the frames of its map in ascending order (the CSR the host built from map_of_frame), and stores sum, n and the mean
//            once.  A gather: a map cell asks the frames at its centre, a frame cell never writes.  The pose and the offset of a
//            frame and the list are the same for every lane of a workgroup: scalar loads.
// Option "elevation_path" = 1, the yardstick: k_fuse_height<false, false>, the quotients u and v by double divisions and the share
// the capped mean forgets by a 32-bit integer division.  "2": the share by the multiply-shift of pwpp_elevation.h, and the quotients
// by the product with the exact reciprocal where the frame images' cell size is a power of two (the division for every other cell
// size).  "0" (default): what tools/elevation_fusion_cost.py decided, kElevationDefaultFast below.
// Every word of sum_out and mean and every halfword of n_out is written by exactly one lane, with ordinary stores; in place (no
// shift) that lane is also the only one that reads the cell.  The loop is bounded by the list's length, which the host checked
// (<= frames); every frame index is compared with frames, every sample's cell with nx and ny, the shifted cell with NX and NY before
// an address is formed (pwpp_elevation.h, pwpp_fusion.h).  No atomics, no workgroup waits for another, nothing is retried: the maps
// are functions of the inputs alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwpp_dev.h"  // the launcher's prototype
#include "pwpp_elevation.h"

namespace {

constexpr int kElevBlock = PWPP_FUSE_RUN;
// What option "elevation_path" = 0 means: path 2 (true) or path 1 (false).  Decided by tools/elevation_fusion_cost.py
// (profiles/elevation_fusion_cost.txt), not in advance.
constexpr bool kElevationDefaultFast = true;

struct ElevCall {
    PwppFusionGeometry G;
    PwppElevationParams P;
    int32_t per_map;  // NX * NY (<= 2^30)
    int32_t runs;     // ceil(per_map / 256): block = map * runs + run
    int32_t n_maps, frames, n_poses, listed;
};

// grid (n_maps * runs)
template <bool RECIP, bool FAST>
__global__ __launch_bounds__(kElevBlock) void k_fuse_height(ElevCall C, const float *height, const double *poses, const double *z_offset, const int32_t *begin,
                                                            const int32_t *list, const int32_t *shift, const int32_t *sum_in, const int16_t *n_in,
                                                            int32_t *sum_out, int16_t *n_out, uint32_t *mean) {
    const unsigned b = blockIdx.x, run = b % (unsigned)C.runs, k = b / (unsigned)C.runs;
    if (k >= (unsigned)C.n_maps) return;
    const int c = (int)run * kElevBlock + (int)threadIdx.x;  // (per_map <= 2^30)
    if (c >= C.per_map) return;
    const int jy = c / C.G.NX, jx = c - jy * C.G.NX;
    const size_t mbase = (size_t)k * (size_t)C.per_map;
    const int32_t sx = shift ? shift[2 * (size_t)k] : 0, sy = shift ? shift[2 * (size_t)k + 1] : 0;
    int32_t sum = 0, n = 0;
    pwpp_elev_start(sum_in ? sum_in + mbase : nullptr, n_in ? n_in + mbase : nullptr, jx, jy, sx, sy, C.G.NX, C.G.NY, C.P.n_max, sum, n);
    // the map's frames: begin is ascending and ends at `listed` (the host built it); the clamps bound the loop all the same
    const int32_t first = max(begin[k], 0), last = min(begin[(size_t)k + 1], C.listed);
    pwpp_elev_cell<RECIP, FAST>(C.G, C.P, sum, n, jx, jy, height, C.frames, poses, z_offset, C.n_poses, list, first, last);
    sum_out[mbase + (size_t)c] = sum;
    n_out[mbase + (size_t)c] = (int16_t)n;
    if (mean) mean[mbase + (size_t)c] = pwpp_elev_mean_bits(sum, n);
}

}  // namespace

// pwpp_fuse_height_grid on device memory.  `poses` (n_poses x 6 doubles), `z_offset` (n_poses doubles; both 8-byte aligned), `begin`
// (n_maps + 1), `list` (`listed` frame indices, each map's ascending) and `shift` (n_maps x {sx, sy}, or null: none) are device
// memory; the caller has checked the sides (<= 32768), nx * ny * frames and NX * NY * n_maps <= 2^31, n_max (1 .. 1023, P from
// pwpp_elev_magic), n_poses (1 or frames), listed <= frames and every list entry in [0, frames).  sum_in and n_in are both null or
// neither; mean may be null.
extern "C" int pwpp_launch_fuse_height(const PwppFusionGeometry *G, const PwppElevationParams *P, int frames, const float *height, const double *poses,
                                       const double *z_offset, int n_poses, int n_maps, const int32_t *begin, const int32_t *list, int listed,
                                       const int32_t *shift, const int32_t *sum_in, const int16_t *n_in, int32_t *sum_out, int16_t *n_out, float *mean,
                                       int path, hipStream_t stream) {
    ElevCall C;
    C.G = *G, C.P = *P;
    C.per_map = G->NX * G->NY;
    C.runs = (C.per_map + kElevBlock - 1) / kElevBlock;
    C.n_maps = n_maps, C.frames = frames, C.n_poses = n_poses, C.listed = listed;
    const int64_t blocks = (int64_t)n_maps * C.runs;
    if (blocks > INT32_MAX) return (int)hipErrorInvalidConfiguration;
    const bool fast = path == 0 ? kElevationDefaultFast : path == 2;
    uint32_t *bits = reinterpret_cast<uint32_t *>(mean);
    const dim3 grid((unsigned)blocks), block(kElevBlock);
    if (!fast)
        hipLaunchKernelGGL((k_fuse_height<false, false>), grid, block, 0, stream, C, height, poses, z_offset, begin, list, shift, sum_in, n_in, sum_out, n_out, bits);
    else if (G->inv_cell != 0.0)
        hipLaunchKernelGGL((k_fuse_height<true, true>), grid, block, 0, stream, C, height, poses, z_offset, begin, list, shift, sum_in, n_in, sum_out, n_out, bits);
    else
        hipLaunchKernelGGL((k_fuse_height<false, true>), grid, block, 0, stream, C, height, poses, z_offset, begin, list, shift, sum_in, n_in, sum_out, n_out, bits);
    return (int)hipGetLastError();
}
