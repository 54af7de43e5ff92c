// pwpp_elevation.hip -- the gfx950 (MI355X) kernel of the elevation fusion: per-frame ground heights, resampled under a pose per
// frame, accumulated into persistent elevation maps -- an int32 sum and an int16 count per cell, and the float mean derived from
// them (pwpp_fuse_height_grid, pwpp_fuse_ground; include/pwpp.h has the rules, pwpp_elevation.h the arithmetic).  A pure image
// operation on the handle's stream, like the occupancy fusion: nothing of the estimate pipeline is read or written.
//
// One launch per call:
//   k_fuse_height   a workgroup per (map, run of 256 cells in row-major order), a lane per map cell, as in k_fuse (pwpp_map_lane of
//            pwpp_fusion.h).  The lane reads its start -- the shifted cell of sum_in and n_in, normalised, or nothing -- keeps sum and n in registers while it walks
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

// What option "elevation_path" = 0 means: path 2 (true) or path 1 (false).  Decided by tools/elevation_fusion_cost.py
// (profiles/elevation_fusion_cost.txt), not in advance.
constexpr bool kElevationDefaultFast = true;

struct ElevCall {
    PwppFusionGeometry G;
    PwppElevationParams P;
    PwppMapRuns R;
};

// grid (n_maps * runs)
template <bool RECIP, bool FAST>
__global__ __launch_bounds__(PWPP_FUSE_RUN) void k_fuse_height(ElevCall C, const float *height, const double *poses, const double *z_offset, const int32_t *begin,
                                                               const int32_t *list, const int32_t *shift, const int32_t *sum_in, const int16_t *n_in,
                                                               int32_t *sum_out, int16_t *n_out, uint32_t *mean) {
    pwpp_map_lane(C.R, C.G.NX, blockIdx.x, threadIdx.x, shift, begin, [&](const PwppMapLane &l) {
        int32_t sum = 0, n = 0;
        pwpp_elev_start(sum_in ? sum_in + l.mbase : nullptr, n_in ? n_in + l.mbase : nullptr, l.jx, l.jy, l.sx, l.sy, C.G.NX, C.G.NY, C.P.n_max, sum, n);
        pwpp_elev_cell<RECIP, FAST>(C.G, C.P, sum, n, l.jx, l.jy, height, C.R.frames, poses, z_offset, C.R.n_poses, list, l.first, l.last);
        sum_out[l.mbase + (size_t)l.c] = sum;
        n_out[l.mbase + (size_t)l.c] = (int16_t)n;
        if (mean) mean[l.mbase + (size_t)l.c] = pwpp_elev_mean_bits(sum, n);
    });
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
    const int64_t blocks = pwpp_map_runs(*G, n_maps, frames, n_poses, listed, C.R);
    if (blocks < 0) return (int)hipErrorInvalidConfiguration;
    const bool fast = path == 0 ? kElevationDefaultFast : path == 2;
    uint32_t *bits = reinterpret_cast<uint32_t *>(mean);
    const dim3 grid((unsigned)blocks), block(PWPP_FUSE_RUN);
    if (!fast)
        hipLaunchKernelGGL((k_fuse_height<false, false>), grid, block, 0, stream, C, height, poses, z_offset, begin, list, shift, sum_in, n_in, sum_out, n_out, bits);
    else if (G->inv_cell != 0.0)
        hipLaunchKernelGGL((k_fuse_height<true, true>), grid, block, 0, stream, C, height, poses, z_offset, begin, list, shift, sum_in, n_in, sum_out, n_out, bits);
    else
        hipLaunchKernelGGL((k_fuse_height<false, true>), grid, block, 0, stream, C, height, poses, z_offset, begin, list, shift, sum_in, n_in, sum_out, n_out, bits);
    return (int)hipGetLastError();
}
