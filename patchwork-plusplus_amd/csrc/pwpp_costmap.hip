// pwpp_costmap.hip -- the gfx950 (MI355X) kernels of the costmap: the occupancy byte, the inflated obstacle distance and the terrain's
// cost byte of every cell folded into one int8 cost image and an optional uint8 `why` (pwpp_costmap_grid, pwpp_costmap_obstacles;
// include/pwpp.h has the rules, pwpp_costmap.h the arithmetic and the dealing).  A pure image operation on the handle's stream, like
// the terrain analysis: nothing of the estimate pipeline is read or written.  The call's frames are one run of cells: no kernel
// here knows a row or a frame.
//
//   k_costmap_cells     option "costmap_path" = 1, the yardstick: a lane per cell, byte loads and stores, the inflation curve read
//                    from global memory (the uploaded table: it stays in L2).
//   k_costmap_quads     "2": the table is staged once per workgroup into LDS as whole dwords (at most 1025), then every lane takes
//                    PWPP_COSTMAP_LANE_ITEMS items of the dealing, PWPP_COSTMAP_BLOCK apart.  An item is four consecutive cells whose
//                    cost bytes are one aligned dword: the cost is stored as that dword; occupancy, terrain and why go as one dword
//                    where their own address at the item is a multiple of 4 and as four bytes otherwise (the images may start at
//                    any address, each at its own); dist2 as one 16-byte load where aligned and as four dwords otherwise.  Which
//                    of these holds is the same for every item of a call and travels as a flag: no lane diverges on it.  The up to
//                    3 cells before the first boundary and the up to 3 behind the last group are single-cell items of the same grid.
//                    The one barrier stands behind the staging loop, which every lane of the workgroup leaves after the same
//                    number of rounds; nothing returns before it.
//   k_costmap_occupied  the count image the distance launcher reads, from an occupancy byte image: (o == 100) as int32, four cells a
//                    lane, one 16-byte store (the count lies in the cluster buffer: 16-byte aligned), the last n % 4 cells by one lane.
// No atomics, no workgroup waits for another, nothing is retried.  "0" (default): what tools/costmap_cost.py decided,
// kCostmapQuadsFromCells below.  Both paths give the same bytes: they evaluate pwpp_costmap_fold on the same inputs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwpp_dev.h"  // the launchers' prototypes
#include "pwpp_costmap.h"

namespace {

constexpr int kBlock = PWPP_COSTMAP_BLOCK;
// What option "costmap_path" = 0 means: path 2 for a call of at least this many cells, path 1 below (pwpp_costmap.h has the figure
// and where it comes from).
constexpr uint64_t kCostmapQuadsFromCells = PWPP_COSTMAP_QUADS_FROM_CELLS;

enum : uint32_t { kWordO = 1, kWordT = 2, kWordWhy = 4, kQuadD = 8 };

// grid (ceil(n / kBlock))
__global__ __launch_bounds__(kBlock) void k_costmap_cells(PwppCostmapRule R, uint64_t n, const int8_t *o, const int8_t *t, const int32_t *d,
                                                          const uint8_t *curve, int8_t *cost, uint8_t *why) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int vo = (R.layers & PWPP_COSTMAP_LAYER_OCCUPANCY) ? o[i] : 0, vt = (R.layers & PWPP_COSTMAP_LAYER_TERRAIN) ? t[i] : 0;
    const int32_t vd = (R.layers & PWPP_COSTMAP_LAYER_INFLATION) ? d[i] : 0;
    int32_t c;
    uint32_t w;
    pwpp_costmap_fold(R, curve, vo, vt, vd, c, w);
    cost[i] = (int8_t)c;
    if (why) why[i] = (uint8_t)w;
}

// four consecutive bytes as a little-endian word; `word`: p is a multiple of 4
__device__ inline uint32_t load_bytes4(const int8_t *p, bool word) {
    if (word) return *reinterpret_cast<const uint32_t *>(p);
    const uint8_t *q = reinterpret_cast<const uint8_t *>(p);
    return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
}

// grid (ceil(items / (kBlock * PWPP_COSTMAP_LANE_ITEMS))); D: the dealing of the call's n cells; flags: kWord*, kQuadD
__global__ __launch_bounds__(kBlock) void k_costmap_quads(PwppCostmapRule R, PwppCostmapDeal D, uint32_t flags, const int8_t *o, const int8_t *t,
                                                          const int32_t *d, const uint32_t *curve_words, int8_t *cost, uint8_t *why) {
    __shared__ uint32_t table[PWPP_COSTMAP_CURVE_WORDS];
    const uint32_t words = (R.layers & PWPP_COSTMAP_LAYER_INFLATION) ? ((uint32_t)R.n_curve + 3u) / 4u : 0u;  // (<= PWPP_COSTMAP_CURVE_WORDS: n_curve is checked)
    for (uint32_t w = threadIdx.x; w < words; w += kBlock) table[w] = curve_words[w];
    __syncthreads();
    const uint8_t *curve = reinterpret_cast<const uint8_t *>(table);
    const bool use_o = (R.layers & PWPP_COSTMAP_LAYER_OCCUPANCY) != 0, use_d = (R.layers & PWPP_COSTMAP_LAYER_INFLATION) != 0,
               use_t = (R.layers & PWPP_COSTMAP_LAYER_TERRAIN) != 0;
    const uint32_t items = D.groups + D.singles;
#pragma unroll
    for (int k = 0; k < PWPP_COSTMAP_LANE_ITEMS; ++k) {
        const uint32_t i = (blockIdx.x * (uint32_t)PWPP_COSTMAP_LANE_ITEMS + (uint32_t)k) * (uint32_t)kBlock + threadIdx.x;  // (< 2^30 + 2^20)
        if (i >= items) break;  // (behind the barrier)
        int cells;
        const uint64_t at = pwpp_costmap_item(D, i, cells);
        int32_t c;
        uint32_t w;
        if (cells == 1) {
            pwpp_costmap_fold(R, curve, use_o ? o[at] : 0, use_t ? t[at] : 0, use_d ? d[at] : 0, c, w);
            cost[at] = (int8_t)c;
            if (why) why[at] = (uint8_t)w;
            continue;
        }
        const uint32_t ow = use_o ? load_bytes4(o + at, flags & kWordO) : 0u, tw = use_t ? load_bytes4(t + at, flags & kWordT) : 0u;
        int32_t dv[4] = {0, 0, 0, 0};
        if (use_d) {
            if (flags & kQuadD) {
                const int4 q = *reinterpret_cast<const int4 *>(d + at);
                dv[0] = q.x, dv[1] = q.y, dv[2] = q.z, dv[3] = q.w;
            } else {
                dv[0] = d[at], dv[1] = d[at + 1], dv[2] = d[at + 2], dv[3] = d[at + 3];
            }
        }
        uint32_t cw = 0, ww = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pwpp_costmap_fold(R, curve, (int)(int8_t)(ow >> (8 * j)), (int)(int8_t)(tw >> (8 * j)), dv[j], c, w);
            cw |= ((uint32_t)c & 0xffu) << (8 * j), ww |= w << (8 * j);
        }
        *reinterpret_cast<uint32_t *>(cost + at) = cw;  // (aligned: the dealing's groups begin at the cost image's boundaries)
        if (why) {
            if (flags & kWordWhy) *reinterpret_cast<uint32_t *>(why + at) = ww;
            else why[at] = (uint8_t)ww, why[at + 1] = (uint8_t)(ww >> 8), why[at + 2] = (uint8_t)(ww >> 16), why[at + 3] = (uint8_t)(ww >> 24);
        }
    }
}

// grid (ceil((n / 4 + 1) / kBlock)); count: 16-byte aligned; word: o is a multiple of 4
__global__ __launch_bounds__(kBlock) void k_costmap_occupied(uint64_t n, const int8_t *o, bool word, int32_t *count) {
    const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x, groups = n / 4;
    if (g < groups) {
        const uint32_t ow = load_bytes4(o + 4 * g, word);
        int4 q;
        q.x = (int8_t)ow == 100, q.y = (int8_t)(ow >> 8) == 100, q.z = (int8_t)(ow >> 16) == 100, q.w = (int8_t)(ow >> 24) == 100;
        *reinterpret_cast<int4 *>(count + 4 * g) = q;
    } else if (g == groups) {
        for (uint64_t i = 4 * groups; i < n; ++i) count[i] = o[i] == 100;
    }
}

inline bool multiple_of(const void *p, uint64_t offset, unsigned bytes) { return ((reinterpret_cast<uintptr_t>(p) + offset) & (bytes - 1u)) == 0; }

}  // namespace

// The count image of an occupancy byte image (1 where the byte is PWPP_OCC_OCCUPIED, else 0).  cells: 1 .. 2^31; count 16-byte aligned.
extern "C" int pwpp_launch_costmap_occupied(size_t cells, const int8_t *occupancy, int32_t *count, hipStream_t stream) {
    if (!multiple_of(count, 0, 16)) return (int)hipErrorInvalidValue;
    const uint64_t lanes = (uint64_t)cells / 4 + 1;
    hipLaunchKernelGGL(k_costmap_occupied, dim3((unsigned)((lanes + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, (uint64_t)cells, occupancy,
                       multiple_of(occupancy, 0, 4), count);
    return (int)hipGetLastError();
}

// The fold on device memory.  The caller has checked the rule (layers, the substitutes, unknown_below, 1 <= n_curve <= 4097 with the
// inflation layer), cells in 1 .. 2^31 and that every enabled layer has its image; dist2 is 4-byte aligned; curve_words: the table
// in whole dwords, 4-byte aligned, the bytes behind n_curve 0 (null without the inflation layer).
extern "C" int pwpp_launch_costmap(const PwppCostmapRule *R, size_t cells, const int8_t *occupancy, const int8_t *terrain, const int32_t *dist2,
                                   const uint32_t *curve_words, int8_t *cost, uint8_t *why, int path, hipStream_t stream) {
    if ((R->layers & PWPP_COSTMAP_LAYER_INFLATION) && (R->n_curve < 1 || R->n_curve > PWPP_COSTMAP_CURVE_MAX)) return (int)hipErrorInvalidValue;
    const uint64_t n = (uint64_t)cells;
    if (path == 0 ? n < kCostmapQuadsFromCells : path == 1) {
        hipLaunchKernelGGL(k_costmap_cells, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, *R, n, occupancy, terrain, dist2,
                           reinterpret_cast<const uint8_t *>(curve_words), cost, why);
        return (int)hipGetLastError();
    }
    const PwppCostmapDeal D = pwpp_costmap_deal((uint64_t)reinterpret_cast<uintptr_t>(cost), n);
    const uint32_t flags = (multiple_of(occupancy, D.head, 4) ? kWordO : 0u) | (multiple_of(terrain, D.head, 4) ? kWordT : 0u) |
                           (multiple_of(why, D.head, 4) ? kWordWhy : 0u) | (multiple_of(dist2, 4 * (uint64_t)D.head, 16) ? kQuadD : 0u);
    const uint64_t items = (uint64_t)D.groups + D.singles, per_group = (uint64_t)kBlock * PWPP_COSTMAP_LANE_ITEMS;
    hipLaunchKernelGGL(k_costmap_quads, dim3((unsigned)((items + per_group - 1) / per_group)), dim3(kBlock), 0, stream, *R, D, flags, occupancy, terrain,
                       dist2, curve_words, cost, why);
    return (int)hipGetLastError();
}
