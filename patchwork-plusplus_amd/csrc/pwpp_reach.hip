// pwpp_reach.hip -- the gfx950 (MI355X) kernels of the cost-to-reach field: for every cell of a cost image the cheapest sum of
// steps from the frame's source cell, and the neighbour it comes through (pwpp_reach_grid, pwpp_reach_ground; include/pwpp.h has the
// rules, pwpp_reach.h the arithmetic and the proofs).  A pure image operation on the handle's stream, like the terrain analysis:
// nothing of the estimate pipeline is read or written.  Integers only.
//
// Three launches per call (more only where a call has more than 2^22 frames):
//   k_reach_terms   a lane per cell of the batch: the cell's term t (0: impassable) as a uint16 in the working image, and the field's
//            start, 0 at the frame's source and PWPP_REACH_NONE elsewhere; clears the defect word.
//   k_reach_sweep   (option "reach_path" = 1, the yardstick) a workgroup per frame: sweeps over the frame's cells in global memory,
//            every lane relaxing its cells against their 8 neighbours in place, until a sweep changes nothing.
//   k_reach_tiles   ("reach_path" = 2) a workgroup per frame that walks the frame's tiles of 32 x 32 cells itself: a dirty tile and
//            its halo of one cell -- values and terms, CLIPPED to the frame's image -- are copied into LDS, relaxed there until they
//            stop changing and the cells that changed are written back; a changed border cell marks the up to three tiles that read
//            it in their halo.  One bit per tile in LDS says dirty; at first the source's tile and the eight around it are (the
//            source's 0 never changes, so nothing else would tell them).  Passes over the bits until a pass finds none.
//   k_reach_from    a lane per cell of the batch over the finished field: the first neighbour in index order whose value plus its
//            step is the cell's value.
// Every schedule gives the same bytes: the field is the one fixed point of the relaxation (pwpp_reach.h).  A frame is one workgroup's
// alone, so no workgroup waits for another: no spinning, no grid-wide barrier, no atomics in global memory.  Every __syncthreads
// stands in control flow that is uniform over the workgroup (the loop conditions are workgroup-wide ORs or values read from LDS
// behind a barrier).  Every loop has a bound from the image (pwpp_reach_sweep_bound: cells + 1 sweeps or passes, tile cells + 1 sweeps
// per visit); a kernel that reaches it -- only a defect can -- sets the defect word, puts PWPP_REACH_NONE at the frame's source, which
// no result has, and ends.  k_reach_from cannot touch the field it reads: a cell whose value has no predecessor -- a defect again --
// sets the defect word and keeps from = -1 beside its value, which no result has either.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwpp_dev.h"  // the launchers' prototypes
#include "pwpp_reach.h"

namespace {

constexpr int kTX = PWPP_REACH_TILE_X, kTY = PWPP_REACH_TILE_Y, kW = kTX + 2, kH = kTY + 2;
constexpr int kCellBlock = 256;   // k_reach_terms, k_reach_from
constexpr int kSweepBlock = 512;  // k_reach_sweep
constexpr int kTileBlock = 256;   // k_reach_tiles: a lane has kTX * kTY / kTileBlock = 4 cells, one column of every 8th row
constexpr int kRowsPerLane = kTX * kTY / kTileBlock, kRowStride = kTileBlock / kTX;
constexpr int kDirtyWords = PWPP_REACH_MAX_TILES / 32;  // a dirty bit per tile of the largest frame the side limit and the range check allow (pwpp_reach.h)
static_assert(kDirtyWords * 32 == PWPP_REACH_MAX_TILES, "whole words");
static_assert(kTX == 32 && kTileBlock % kTX == 0 && kRowsPerLane * kRowStride == kTY, "a lane keeps its column");
// What option "reach_path" = 0 means: the tiled schedule (true) or the sweeps (false).  Decided by tools/reach_cost.py
// (profiles/reach_cost.txt), not in advance: per 1024 frames the tiles take 21.1 ms against 172.0 ms at 256 x 256 cells, 0.72 against
// 12.2 ms with max_reach at 20 m, 517 against 1809 us at 64 x 64 cells and 108 against 133 us there with max_reach, every
// difference beyond its A/A floor.
constexpr bool kReachDefaultTiled = true;

struct ReachCall {
    PwppReachRule R;
    int32_t nx, ny, frames;     // frames: of the whole call
    int32_t sx, sy;             // the source where one serves every frame (sources == nullptr)
    int32_t frame_first;        // this launch's first frame
    int32_t tiles_x, tiles_y;
};

__device__ inline void source_of(const ReachCall &C, const int32_t *sources, int f, int &sx, int &sy) {
    sx = sources ? sources[2 * (size_t)f] : C.sx, sy = sources ? sources[2 * (size_t)f + 1] : C.sy;
}
__device__ inline void defect(const ReachCall &C, const int32_t *sources, int f, uint32_t *frame_value, uint32_t *flag) {
    int sx, sy;
    source_of(C, sources, f, sx, sy);
    frame_value[(size_t)sy * (size_t)C.nx + (size_t)sx] = PWPP_REACH_UNREACHED;
    *flag = 1u;
}

// grid (ceil(cells of the batch / kCellBlock))
__global__ __launch_bounds__(kCellBlock) void k_reach_terms(ReachCall C, const int8_t *cost, const int32_t *dist2, const int32_t *sources, uint16_t *term,
                                                            uint32_t *value, uint32_t *flag) {
    const size_t per_frame = (size_t)C.nx * (size_t)C.ny, i = (size_t)blockIdx.x * kCellBlock + threadIdx.x;
    if (i == 0) *flag = 0u;
    if (i >= per_frame * (size_t)C.frames) return;
    const int f = (int)(i / per_frame);
    const size_t c = i - (size_t)f * per_frame;
    int sx, sy;
    source_of(C, sources, f, sx, sy);
    const bool is_source = c == (size_t)sy * (size_t)C.nx + (size_t)sx;
    term[i] = (uint16_t)pwpp_reach_term(C.R, (int)cost[i], C.R.use_dist2 ? dist2[i] : 0, is_source);
    value[i] = is_source ? 0u : PWPP_REACH_UNREACHED;
}

// grid (frames of this launch)
__global__ __launch_bounds__(kSweepBlock) void k_reach_sweep(ReachCall C, const int32_t *sources, const uint16_t *term, uint32_t *value, uint32_t *flag) {
    const int f = C.frame_first + (int)blockIdx.x, tid = (int)threadIdx.x;
    if (f >= C.frames) return;  // (the whole workgroup)
    const int cells = C.nx * C.ny;  // (<= 1518730: the range bound)
    const size_t base = (size_t)f * (size_t)cells;
    PwppReachImageView n{term + base, value + base, C.nx, C.ny, 0, 0};
    uint32_t *v = value + base;
    const int64_t bound = pwpp_reach_sweep_bound(cells);
    for (int64_t sweep = 0;; ++sweep) {
        if (sweep >= bound) {  // (uniform)
            if (tid == 0) defect(C, sources, f, v, flag);
            break;
        }
        int changed = 0;
        for (int i = tid; i < cells; i += kSweepBlock) {
            if (n.term[i] == 0) continue;
            n.y = i / C.nx, n.x = i - n.y * C.nx;
            const uint32_t best = pwpp_reach_best(n, (uint32_t)C.R.max_reach);
            if (best < v[i]) v[i] = best, changed = 1;
        }
        if (!__syncthreads_or(changed)) break;
    }
}

// a tile and its halo in LDS: the view of the cell at `at`
struct ReachTileView {
    const uint16_t *term;
    const uint32_t *value;
    int at;
    __device__ uint32_t t(int dx, int dy) const { return term[at + dy * kW + dx]; }
    __device__ uint32_t v(int dx, int dy) const { return value[at + dy * kW + dx]; }
};

// grid (frames of this launch); tiles_x * tiles_y <= PWPP_REACH_MAX_TILES
__global__ __launch_bounds__(kTileBlock) void k_reach_tiles(ReachCall C, const int32_t *sources, const uint16_t *term, uint32_t *value, uint32_t *flag) {
    __shared__ uint32_t s_value[kH * kW];
    __shared__ uint16_t s_term[kH * kW];
    __shared__ uint32_t s_dirty[kDirtyWords];

    const int f = C.frame_first + (int)blockIdx.x, tid = (int)threadIdx.x;
    if (f >= C.frames) return;  // (the whole workgroup)
    const int cells = C.nx * C.ny, tiles = C.tiles_x * C.tiles_y, words = (tiles + 31) >> 5;
    const size_t base = (size_t)f * (size_t)cells;
    const uint16_t *ft = term + base;
    uint32_t *fv = value + base;
    const int tx = tid % kTX, ty0 = tid / kTX;

    for (int w = tid; w < words; w += kTileBlock) s_dirty[w] = 0u;
    __syncthreads();
    if (tid == 0) {
        int sx, sy;
        source_of(C, sources, f, sx, sy);
        // the source's tile and the tiles around it: the source's 0 may lie in their halo, and it never changes
        for (int ey = -1; ey <= 1; ++ey)
            for (int ex = -1; ex <= 1; ++ex) {
                const int ux = sx / kTX + ex, uy = sy / kTY + ey;
                if (ux < 0 || ux >= C.tiles_x || uy < 0 || uy >= C.tiles_y) continue;
                const int t = uy * C.tiles_x + ux;
                s_dirty[t >> 5] |= 1u << (t & 31);
            }
    }
    __syncthreads();

    const int64_t pass_bound = pwpp_reach_sweep_bound(cells);
    constexpr int kVisitBound = kTX * kTY + 1;
    bool failed = false;
    for (int64_t pass = 0; !failed; ++pass) {
        if (pass >= pass_bound) {  // (uniform)
            failed = true;
            break;
        }
        bool any = false;
        for (int w = 0; w < words && !failed; ++w) {
            // (every lane reads the same word: the bits were last written before the barrier that ended the visit before)
            uint32_t bits = s_dirty[w];
            while (bits != 0 && !failed) {
                const int t = (w << 5) + (__ffs((int)bits) - 1);
                bits &= bits - 1;
                any = true;
                const int x0 = (t % C.tiles_x) * kTX, y0 = (t / C.tiles_x) * kTY;
                for (int i = tid; i < kH * kW; i += kTileBlock) {
                    const int ly = i / kW, lx = i - ly * kW, gx = x0 + lx - 1, gy = y0 + ly - 1;
                    const bool in = gx >= 0 && gx < C.nx && gy >= 0 && gy < C.ny;  // (before an address is formed)
                    const size_t g = (size_t)(in ? gy : 0) * (size_t)C.nx + (size_t)(in ? gx : 0);
                    const uint16_t tt = in ? ft[g] : (uint16_t)0;
                    s_term[i] = tt;
                    s_value[i] = tt != 0 ? fv[g] : PWPP_REACH_UNREACHED;
                }
                __syncthreads();  // (and every lane has read the word of this tile's bit)
                if (tid == 0) atomicAnd(&s_dirty[w], ~(1u << (t & 31)));
                unsigned mine = 0;  // bit r: this lane's cell of row ty0 + r * kRowStride changed in this visit
                for (int sweep = 0;; ++sweep) {
                    if (sweep >= kVisitBound) {  // (uniform)
                        failed = true;
                        break;
                    }
                    int changed = 0;
#pragma unroll
                    for (int r = 0; r < kRowsPerLane; ++r) {
                        const int at = (ty0 + r * kRowStride + 1) * kW + tx + 1;
                        if (s_term[at] == 0) continue;  // (a cell beyond a ragged edge too)
                        const ReachTileView n{s_term, s_value, at};
                        const uint32_t best = pwpp_reach_best(n, (uint32_t)C.R.max_reach);
                        if (best < s_value[at]) s_value[at] = best, changed = 1, mine |= 1u << r;
                    }
                    if (!__syncthreads_or(changed)) break;
                }
#pragma unroll
                for (int r = 0; r < kRowsPerLane; ++r) {
                    if (!(mine & (1u << r))) continue;
                    const int ly = ty0 + r * kRowStride;
                    fv[(size_t)(y0 + ly) * (size_t)C.nx + (size_t)(x0 + tx)] = s_value[(ly + 1) * kW + tx + 1];
                    // the tiles that hold this cell in their halo
                    const int ddx = tx == 0 ? -1 : (tx == kTX - 1 ? 1 : 0), ddy = ly == 0 ? -1 : (ly == kTY - 1 ? 1 : 0);
                    const int qx = t % C.tiles_x, qy = t / C.tiles_x;
                    for (int k = 0; k < 3; ++k) {
                        const int ex = k == 1 ? 0 : ddx, ey = k == 0 ? 0 : ddy;
                        if ((ex == 0 && ey == 0) || (k == 2 && (ddx == 0 || ddy == 0))) continue;
                        const int ux = qx + ex, uy = qy + ey;
                        if (ux < 0 || ux >= C.tiles_x || uy < 0 || uy >= C.tiles_y) continue;
                        const int u = uy * C.tiles_x + ux;
                        atomicOr(&s_dirty[u >> 5], 1u << (u & 31));
                    }
                }
                __syncthreads();  // (the marks, and the tile in LDS is free again)
            }
        }
        if (!any) break;
    }
    if (failed && tid == 0) defect(C, sources, f, fv, flag);
}

// grid (ceil(cells of the batch / kCellBlock))
__global__ __launch_bounds__(kCellBlock) void k_reach_from(ReachCall C, const int32_t *sources, const uint16_t *term, const uint32_t *value, int32_t *from,
                                                           uint32_t *flag) {
    const size_t per_frame = (size_t)C.nx * (size_t)C.ny, i = (size_t)blockIdx.x * kCellBlock + threadIdx.x;
    if (i >= per_frame * (size_t)C.frames) return;
    const int f = (int)(i / per_frame);
    const int c = (int)(i - (size_t)f * per_frame);
    const uint32_t vc = value[i];
    int32_t out = -1;
    if (vc != PWPP_REACH_UNREACHED) {
        int sx, sy;
        source_of(C, sources, f, sx, sy);
        const int y = c / C.nx, x = c - y * C.nx;
        if (x == sx && y == sy) out = c;
        else {
            const PwppReachImageView n{term + (size_t)f * per_frame, value + (size_t)f * per_frame, C.nx, C.ny, x, y};
            const int k = pwpp_reach_from(n, vc);
            if (k >= 0) out = (y + pwpp_reach_dy(k)) * C.nx + x + pwpp_reach_dx(k);
            else *flag = 1u;  // (a value without a predecessor, a defect: from stays -1 beside a reach that is not PWPP_REACH_NONE)
        }
    }
    from[i] = out;
}

}  // namespace

// the words of the working image: a uint16 term per cell of the batch
extern "C" size_t pwpp_reach_work_words(int nx, int ny, int frames) { return ((size_t)nx * (size_t)ny * (size_t)frames + 1) / 2; }

// pwpp_reach_grid on device memory.  The caller has checked the sides (<= 32768), nx * ny * frames <= 2^31, the rule, the range bound (so a
// frame has at most 1518730 cells and PWPP_REACH_MAX_TILES tiles) and the sources (inside the image; `sources`: one per frame on the device, or null: (sx, sy)
// for every frame); dist2 (null without R->use_dist2), reach and from (may be null) are 4-byte aligned; term: pwpp_reach_work_words;
// flag: one word, not 0 after the call where a kernel met a defect.
extern "C" int pwpp_launch_reach(const PwppReachRule *R, int nx, int ny, int frames, const int8_t *cost, const int32_t *dist2, int sx, int sy,
                                 const int32_t *sources, int32_t *reach, int32_t *from, uint16_t *term, uint32_t *flag, int path, hipStream_t stream) {
    if ((R->use_dist2 != 0) != (dist2 != nullptr)) return (int)hipErrorInvalidValue;
    ReachCall C;
    C.R = *R;
    C.nx = nx, C.ny = ny, C.frames = frames, C.sx = sx, C.sy = sy, C.frame_first = 0;
    C.tiles_x = (nx + kTX - 1) / kTX, C.tiles_y = (ny + kTY - 1) / kTY;
    const size_t cells = (size_t)nx * (size_t)ny * (size_t)frames;
    const dim3 cell_grid((unsigned)((cells + kCellBlock - 1) / kCellBlock));
    uint32_t *value = reinterpret_cast<uint32_t *>(reach);
    const bool tiled = path == 0 ? kReachDefaultTiled : path == 2;
    if ((int64_t)C.tiles_x * (int64_t)C.tiles_y > (int64_t)PWPP_REACH_MAX_TILES) return (int)hipErrorInvalidValue;  // (the caller's checks exclude it)
    hipLaunchKernelGGL(k_reach_terms, cell_grid, dim3(kCellBlock), 0, stream, C, cost, dist2, sources, term, value, flag);
    int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    constexpr int kPerLaunch = 1 << 22;
    for (int64_t first = 0; first < (int64_t)frames; first += kPerLaunch) {
        C.frame_first = (int32_t)first;
        const dim3 grid((unsigned)(first + kPerLaunch < (int64_t)frames ? kPerLaunch : (int64_t)frames - first));
        if (tiled) hipLaunchKernelGGL(k_reach_tiles, grid, dim3(kTileBlock), 0, stream, C, sources, term, value, flag);
        else hipLaunchKernelGGL(k_reach_sweep, grid, dim3(kSweepBlock), 0, stream, C, sources, term, value, flag);
        if ((rc = (int)hipGetLastError()) != 0) return rc;
    }
    if (from) {
        C.frame_first = 0;
        hipLaunchKernelGGL(k_reach_from, cell_grid, dim3(kCellBlock), 0, stream, C, sources, term, value, from, flag);
        rc = (int)hipGetLastError();
    }
    return rc;
}
