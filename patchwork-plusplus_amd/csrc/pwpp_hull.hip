// pwpp_hull.hip -- the ROW kernels of the obstacle hulls (pwpp_hull_obstacles): what happens to a row once the point passes of
// pwpp_kernels.hip (k_hull_extremes, k_hull_candidates) have counted its points and written its candidates.  pwpp_hull.h has the
// arithmetic, the accumulators and the proofs; include/pwpp.h has the contract.
//
//   k_hull_init        the accumulators' initial values, a lane per word
//   k_hull_offsets     between the passes, a wave per frame: the exclusive scan of the rows' `points` -- where a row's candidates begin
//   k_hull_rows_lane   option "hulls_path" 1, the yardstick: a lane per row, pwpp_hull_row_serial as the host runs it
//   k_hull_rows_wave   option "hulls_path" 2: a wave per row.  A march step is one strided sweep of the candidates by 64 lanes and a
//                      butterfly of six shuffles under the total order of pwpp_hull_beats; every lane keeps the (wave-uniform) state
//                      of the march, lane 0 stores the vertex.  The hull lies in LDS, 8 bytes a vertex: the rectangle's edges are
//                      dealt to the lanes, every lane reads the same vertex at a time (a broadcast, no bank conflict), and the
//                      lanes' best edges are merged by a second butterfly; the lane that owns the winner writes the row.
// The same bytes on both paths: maxima under a total order, and an ordered pick with ties to the lower edge.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwpp_dev.h"  // the launchers' prototypes
#include "pwpp_hull.h"
#include "pwpp_wave.h"

namespace {

constexpr int kHullBlock = 64;

__global__ __launch_bounds__(256) void k_hull_init(int64_t rows, uint32_t *acc) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * PWPP_HULL_ACC_WORDS) return;
    const int w = (int)(i % PWPP_HULL_ACC_WORDS);
    acc[i] = (w < 16 && ((w >> 1) & 1) == 0) ? 0xffffffffu : 0u;  // (the minima: PWPP_HULL_KEY_NO_MIN; the maxima and the counts: 0)
}

__global__ __launch_bounds__(kHullBlock) void k_hull_offsets(int max_hulls, uint32_t *acc) {
    const int lane = threadIdx.x;
    uint32_t *frame = acc + (size_t)blockIdx.x * (size_t)max_hulls * PWPP_HULL_ACC_WORDS;
    uint32_t carry = 0;  // (at most the frame's counted points: below 2^31)
    for (int base = 0; base < max_hulls; base += kHullBlock) {
        const int r = base + lane;
        const bool in = r < max_hulls;  // (base + 63 < 2^24 + 64: no overflow)
        const uint32_t v = in ? frame[(size_t)r * PWPP_HULL_ACC_WORDS + PWPP_HULL_ACC_POINTS] : 0u;
        const uint32_t incl = wave_incl_scan(v);  // (one whole wave, no lane has left: all 64 active)
        if (in) frame[(size_t)r * PWPP_HULL_ACC_WORDS + PWPP_HULL_ACC_FIRST] = carry + incl - v;
        carry += __shfl(incl, 63, 64);
    }
}

// What the row kernels read of row i: its points, its candidates.
struct HullRowIn {
    int32_t points;
    int64_t n_cand;
    const pwpp_hull_pt *cand;
};
__device__ __forceinline__ HullRowIn hull_row_in(const PwppHullRows &R, int64_t i) {
    const uint32_t *acc = R.acc + (size_t)i * PWPP_HULL_ACC_WORDS;
    HullRowIn in;
    const uint32_t points = acc[PWPP_HULL_ACC_POINTS], cands = acc[PWPP_HULL_ACC_CANDS];
    in.points = (int32_t)points;
    in.n_cand = (int64_t)(cands < points ? cands : points);  // (never more were written)
    in.cand = R.arena + (size_t)(i / R.max_hulls) * (size_t)R.arena_stride + (size_t)acc[PWPP_HULL_ACC_FIRST];
    return in;
}
__device__ __forceinline__ void hull_store_row(uint32_t *row, const uint32_t *out) {
#pragma unroll
    for (int k = 0; k < PWPP_HULL_ROW_WORDS; ++k) row[k] = out[k];
}

__global__ __launch_bounds__(kHullBlock) void k_hull_rows_lane(int64_t rows, PwppHullRows R, double x0, double y0, uint32_t *hulls, int32_t *vertices, int max_vertices) {
    const int64_t i = (int64_t)blockIdx.x * kHullBlock + threadIdx.x;
    if (i >= rows) return;
    const HullRowIn in = hull_row_in(R, i);
    uint32_t out[PWPP_HULL_ROW_WORDS];
    pwpp_hull_row_serial(in.cand, in.n_cand, in.points, max_vertices, vertices + (size_t)i * (size_t)max_vertices * 2, x0, y0, out);
    hull_store_row(hulls + (size_t)i * PWPP_HULL_ROW_WORDS, out);
}

// vertices: may be null (the lists are not asked for: the hull lives in LDS alone)
__global__ __launch_bounds__(kHullBlock) void k_hull_rows_wave(PwppHullRows R, double x0, double y0, uint32_t *hulls, int32_t *vertices, int max_vertices) {
    __shared__ int32_t s_v[2 * PWPP_HULL_MAX_VERTICES];
    const int64_t i = blockIdx.x;
    const int lane = threadIdx.x;
    const HullRowIn in = hull_row_in(R, i);
    uint32_t *row = hulls + (size_t)i * PWPP_HULL_ROW_WORDS;
    int32_t *list = vertices ? vertices + (size_t)i * (size_t)max_vertices * 2 : nullptr;
    uint32_t out[PWPP_HULL_ROW_WORDS];
    PwppHullMarch M;
    pwpp_hull_march_begin(M);
    if (in.points <= 0 || in.n_cand <= 0) {  // (wave-uniform, like everything the march decides on)
        if (lane == 0) {
            pwpp_hull_row(0, M, nullptr, x0, y0, out);
            hull_store_row(row, out);
        }
        return;
    }
    pwpp_hull_pt start = PWPP_HULL_KEY_NO_MIN;
    for (int64_t k = lane; k < in.n_cand; k += kHullBlock) start = in.cand[k] < start ? in.cand[k] : start;
    start = wave_min(start);
    pwpp_hull_pt c = start, prev = start;
    for (int64_t step = 0; step < in.n_cand; ++step) {  // (a hull has at most n_cand vertices)
        pwpp_hull_march_add(M, prev, c);
        if (M.n <= max_vertices) {  // (max_vertices <= PWPP_HULL_MAX_VERTICES: checked by the caller)
            M.stored = M.n;
            if (lane == 0) {
                s_v[2 * (M.n - 1)] = pwpp_hull_x(c), s_v[2 * (M.n - 1) + 1] = pwpp_hull_y(c);
                if (list) list[2 * (M.n - 1)] = pwpp_hull_x(c), list[2 * (M.n - 1) + 1] = pwpp_hull_y(c);
            }
        }
        pwpp_hull_pt best = c;
        for (int64_t k = lane; k < in.n_cand; k += kHullBlock) {
            const pwpp_hull_pt b = in.cand[k];
            best = pwpp_hull_beats(c, best, b) ? b : best;
        }
        best = wave_reduce(best, [c](pwpp_hull_pt best, pwpp_hull_pt o) { return pwpp_hull_beats(c, best, o) ? o : best; });
        prev = c, c = best;
        if (c == start) break;
    }
    M.area2 += pwpp_hull_shoelace(prev, start);  // (the closing edge)
    if (M.n > max_vertices) {
        if (lane == 0) {
            pwpp_hull_row(in.points, M, nullptr, x0, y0, out);
            hull_store_row(row, out);
        }
        return;
    }
    __syncthreads();  // (lane 0's vertices, for every lane)
    PwppHullEdge best;
    best.i = -1, best.WH = 0, best.L2 = 1, best.ex = 1, best.ey = 0, best.pmin = best.pmax = best.qmin = best.qmax = 0;
    for (int e = lane; e < M.n; e += kHullBlock) {
        const PwppHullEdge E = pwpp_hull_edge_of(s_v, M.n, e);
        if (pwpp_hull_edge_takes(best.WH, best.L2, best.i, E.WH, E.L2, E.i)) best = E;
    }
    struct EdgeKey {  // what pwpp_hull_edge_takes orders the edges by (32 bytes: the four bytes of padding behind `i` move with it)
        unsigned long long wh_lo, wh_hi, l2;
        int i;
    };
    const int bi = wave_reduce(EdgeKey{(unsigned long long)best.WH, (unsigned long long)(best.WH >> 64), best.L2, best.i}, [](EdgeKey m, EdgeKey o) {
                       const unsigned __int128 mine = ((unsigned __int128)m.wh_hi << 64) | m.wh_lo, theirs = ((unsigned __int128)o.wh_hi << 64) | o.wh_lo;
                       return pwpp_hull_edge_takes(mine, m.l2, m.i, theirs, o.l2, o.i) ? o : m;
                   }).i;
    if (bi >= 0 && best.i == bi) {  // (one lane: edge bi was dealt to lane bi % 64, and is that lane's best)
        pwpp_hull_row(in.points, M, &best, x0, y0, out);
        hull_store_row(row, out);
    }
}

}  // namespace

extern "C" int pwpp_launch_hull_rows(int step, int path, int frames, const PwppHullRows *rows, double x0, double y0, void *hulls, int32_t *vertices,
                                     int max_vertices, hipStream_t stream) {
    const int64_t n = (int64_t)frames * (int64_t)rows->max_hulls;  // (<= 2^24: checked by the caller)
    if (step == 0)
        hipLaunchKernelGGL(k_hull_init, dim3((unsigned)((n * PWPP_HULL_ACC_WORDS + 255) / 256)), dim3(256), 0, stream, n, rows->acc);
    else if (step == 1)
        hipLaunchKernelGGL(k_hull_offsets, dim3((unsigned)frames), dim3(kHullBlock), 0, stream, rows->max_hulls, rows->acc);
    else if (path == 1)
        hipLaunchKernelGGL(k_hull_rows_lane, dim3((unsigned)((n + kHullBlock - 1) / kHullBlock)), dim3(kHullBlock), 0, stream, n, *rows, x0, y0,
                           static_cast<uint32_t *>(hulls), vertices, max_vertices);
    else
        hipLaunchKernelGGL(k_hull_rows_wave, dim3((unsigned)n), dim3(kHullBlock), 0, stream, *rows, x0, y0, static_cast<uint32_t *>(hulls), vertices, max_vertices);
    return (int)hipGetLastError();
}
