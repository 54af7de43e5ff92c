// pwpp_fusion.hip -- the gfx950 (MI355X) kernel of the occupancy fusion: per-frame occupancy bytes, resampled under a pose per
// frame, accumulated into persistent int16 log-odds maps (pwpp_fuse_grid, pwpp_fuse_obstacles; include/pwpp.h has the rules,
// pwpp_fusion.h the arithmetic).  A pure image operation on the handle's stream, like the visibility: nothing of the estimate
// pipeline is read or written.
//
// One launch per call:
//   k_fuse   a workgroup per (map, run of 256 cells in row-major order), a lane per map cell: the dealing that pwpp_map_lane of
//            pwpp_fusion.h states, for the elevation fusion's kernel as well.  The lane reads its start -- the
//            shifted cell of map_in, or 0 -- keeps L in a register while it walks the frames of its map in ascending order (the CSR
//            the host built from map_of_frame: begin[n_maps + 1], list[]), and stores L once as an int16 and once as the derived
//            byte.  The operator is a gather: a map cell asks the frames, a frame cell never writes.  The pose of a frame and the
//            list are the same for every lane of a workgroup: scalar loads.
// Option "fusion_path" = 1, the yardstick: k_fuse<false>, every quotient u = (fx - x0) / cell a double division -- eight per map
// cell and frame, and what bounds the kernel (profiles/occupancy_fusion_cost.txt).  Path 0 (default): k_fuse<true> where the frame
// images' cell size is a power of two, so that the product with its exact reciprocal is the same bits (pwpp_fusion.h); the
// yardstick kernel for every other cell size.
// Every halfword of map_out and every byte of map_occupancy is written by exactly one lane, with ordinary stores; with
// map_out == map_in (no shift) that lane is also the only one that reads the cell.  The loop is bounded by the list's length, which
// the host checked (<= frames); every frame index is compared with frames, every sample's cell with nx and ny, the shifted cell
// with NX and NY before an address is formed (pwpp_fusion.h).  No atomics, no workgroup waits for another, nothing is retried: the
// maps are functions of the inputs alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwpp_dev.h"  // the launcher's prototype
#include "pwpp_fusion.h"

namespace {

struct FuseCall {
    PwppFusionGeometry G;
    PwppFusionParams P;
    PwppMapRuns R;
};

// grid (n_maps * runs)
template <bool RECIP>
__global__ __launch_bounds__(PWPP_FUSE_RUN) void k_fuse(FuseCall C, const int8_t *occupancy, const double *poses, const int32_t *begin, const int32_t *list,
                                                        const int32_t *shift, const int16_t *map_in, int16_t *map_out, int8_t *map_occupancy) {
    // pwpp_map_lane spelt out: every form of the call moved this kernel's frame loop and slowed it (profiles/map_plan_refactor_ab.txt)
    const unsigned b = blockIdx.x, run = b % (unsigned)C.R.runs, k = b / (unsigned)C.R.runs;
    if (k >= (unsigned)C.R.n_maps) return;
    const int c = (int)run * PWPP_FUSE_RUN + (int)threadIdx.x;  // (per_map <= 2^30)
    if (c >= C.R.per_map) return;
    const int jy = c / C.G.NX, jx = c - jy * C.G.NX;
    const size_t mbase = (size_t)k * (size_t)C.R.per_map;
    const int32_t sx = shift ? shift[2 * (size_t)k] : 0, sy = shift ? shift[2 * (size_t)k + 1] : 0;
    int32_t L = pwpp_fuse_start(map_in ? map_in + mbase : nullptr, jx, jy, sx, sy, C.G.NX, C.G.NY);
    const int32_t first = max(begin[k], 0), last = min(begin[(size_t)k + 1], C.R.listed);
    L = pwpp_fuse_cell<RECIP>(C.G, C.P, L, jx, jy, occupancy, C.R.frames, poses, C.R.n_poses, list, first, last);
    map_out[mbase + (size_t)c] = (int16_t)L;
    if (map_occupancy) map_occupancy[mbase + (size_t)c] = pwpp_fuse_byte(L, C.P);
}

}  // namespace

// pwpp_fuse_grid on device memory.  `poses` (n_poses x 6 doubles, 8-byte aligned), `begin` (n_maps + 1), `list` (`listed` frame
// indices, each map's ascending) and `shift` (n_maps x {sx, sy}, or null: none) are device memory; the caller has checked the
// sides (<= 32768), nx * ny * frames and NX * NY * n_maps <= 2^31, the parameters' ranges, n_poses (1 or frames), listed <= frames
// and every list entry in [0, frames).  map_in and map_occupancy may be null.
extern "C" int pwpp_launch_fuse_grid(const PwppFusionGeometry *G, const PwppFusionParams *P, int frames, const int8_t *occupancy, const double *poses,
                                     int n_poses, int n_maps, const int32_t *begin, const int32_t *list, int listed, const int32_t *shift,
                                     const int16_t *map_in, int16_t *map_out, int8_t *map_occupancy, int path, hipStream_t stream) {
    FuseCall C;
    C.G = *G, C.P = *P;
    const int64_t blocks = pwpp_map_runs(*G, n_maps, frames, n_poses, listed, C.R);
    if (blocks < 0) return (int)hipErrorInvalidConfiguration;
    if (path == 0 && G->inv_cell != 0.0)
        hipLaunchKernelGGL(k_fuse<true>, dim3((unsigned)blocks), dim3(PWPP_FUSE_RUN), 0, stream, C, occupancy, poses, begin, list, shift, map_in, map_out, map_occupancy);
    else
        hipLaunchKernelGGL(k_fuse<false>, dim3((unsigned)blocks), dim3(PWPP_FUSE_RUN), 0, stream, C, occupancy, poses, begin, list, shift, map_in, map_out, map_occupancy);
    return (int)hipGetLastError();
}
