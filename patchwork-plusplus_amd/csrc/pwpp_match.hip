// pwpp_match.hip -- the gfx950 (MI355X) kernels of the correlative scan match: for every frame, every candidate pose and every
// whole-cell shift of a window, the sum of the map's log-odds under the frame's occupied cells, and the best of them
// (pwpp_match_grid, pwpp_match_obstacles; include/pwpp.h has the rules, pwpp_match.h the arithmetic).  A pure image operation on
// the handle's stream, like the fusion: nothing of the estimate pipeline is read or written.
//
// Three launches per call:
//   k_match_compact  a workgroup per frame walks the frame's bytes 256 at a time and writes every byte that is exactly
//                    PWPP_OCC_OCCUPIED as one packed word (iy << 16 | ix) into the frame's row of the cell list, in image order
//                    (a ballot and the waves' counts give every lane its place: no atomics), then the frame's count.  Landings are
//                    NOT stored: they depend on the candidate, frames x candidates x cells words.
//   k_match_score    a workgroup per (frame, candidate, tile of 256 shifts), a lane per shift (consecutive lanes: consecutive sx, so a
//                    wave's reads of one landing are consecutive halfwords of a map row).  The workgroup walks the frame's list in
//                    chunks of 256: every lane lands one cell under the candidate -- the double arithmetic, once per cell and
//                    workgroup -- into LDS; then every lane reads the chunk's landings as broadcasts and gathers
//                    map[Jy + sy][Jx + sx] into an int32 partial, widened into its int64 sum after every chunk (256 * 32768 = 2^23).
//                    It stores the sum (where the caller wants the scores) and the workgroup's best entry by the key order.
//   k_match_best     a workgroup per frame takes the best of the frame's candidates x tiles entries and writes the result row.
// The sums are integers and the key order is total: neither the order of the walk nor the shape of a reduction can change a bit.
// Every loop is bounded by a count the host checked (the frame's count is clamped to nx * ny all the same); Jx + sx and Jy + sy are
// compared with NX and NY, the frame's map with n_maps, the candidate set with n_sets before an address is formed.  No atomics, no
// workgroup waits for another, nothing is retried.
// Option "match_path" = 1, the yardstick: k_match_score<., false>, every map read comes from global memory.  "2":
// k_match_score<., true> first lands the frame's cells once more to find the rectangle of the map its shifts can reach
// (pwpp_match_window), copies that rectangle into LDS where it holds at most kStageHalfwords, and gathers from the copy; a larger
// rectangle is read from global memory as on path 1.  Which of the two "0" means is kMatchDefaultStage, decided by
// tools/scan_match_cost.py (profiles/scan_match_cost.txt): staging lost in every case measured, so "0" is path 1.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pwpp_dev.h"  // the launcher's prototype
#include "pwpp_match.h"
#include "pwpp_wave.h"

namespace {

constexpr int kMatchBlock = 256;
// What option "match_path" = 0 means: whether the rectangle of the map a workgroup reads is staged in LDS.  Decided by
// tools/scan_match_cost.py (profiles/scan_match_cost.txt), not in advance: the staged kernel took 19 to 20 ms where global reads
// took 8 to 9, in all three cases, so it is false.
constexpr bool kMatchDefaultStage = false;
constexpr int kStageHalfwords = 64 * 1024;  // the staged rectangle: 128 KiB of the 160 KiB of a CU, beside 8 KiB of landings and keys
static_assert(PWPP_MATCH_CHUNK == kMatchBlock && PWPP_MATCH_TILE == kMatchBlock, "a lane per cell of a chunk and per shift of a tile");

struct MatchCall {
    PwppMatchGeometry G;
    int32_t per_frame;  // nx * ny (<= 2^30)
    int32_t per_map;    // NX * NY (<= 2^30)
    int32_t frames, n_sets, n_candidates, n_maps;
    int32_t wx, wy, W, H;  // W = 2 wx + 1, H = 2 wy + 1
    int32_t shifts, tiles; // W * H, ceil(shifts / 256): block = (frame * n_candidates + candidate) * tiles + tile
};

__device__ inline int32_t frame_count(const MatchCall &C, const int32_t *count, unsigned f) {
    const int32_t n = count[f];
    return n < 0 ? 0 : (n > C.per_frame ? C.per_frame : n);
}

// the best of the workgroup's 256 keys, left in keys[0]
__device__ inline void block_best(PwppMatchKey *keys, const PwppMatchKey &mine) {
    const unsigned t = threadIdx.x;
    keys[t] = mine;
    __syncthreads();
    for (unsigned stride = kMatchBlock / 2; stride > 0; stride >>= 1) {
        if (t < stride && pwpp_match_better(keys[t + stride], keys[t])) keys[t] = keys[t + stride];
        __syncthreads();
    }
}

// an entry every live one beats
__device__ inline PwppMatchKey no_key() { return PwppMatchKey{INT64_MIN, INT32_MAX, 0, 0, 0}; }

// grid (frames)
__global__ __launch_bounds__(kMatchBlock) void k_match_compact(MatchCall C, const int8_t *occupancy, int32_t *cells, int32_t *count) {
    __shared__ int wave_n[kMatchBlock / 64];
    const unsigned f = blockIdx.x, t = threadIdx.x, lane = t & 63u, w = t >> 6;
    if (f >= (unsigned)C.frames) return;
    const int8_t *image = occupancy + (size_t)f * (size_t)C.per_frame;
    int32_t *row = cells + (size_t)f * (size_t)C.per_frame;
    int32_t base = 0;  // occupied cells before this round: <= c0
    for (int32_t c0 = 0; c0 < C.per_frame; c0 += kMatchBlock) {  // (per_frame <= 2^30)
        const int32_t c = c0 + (int32_t)t;
        const bool on = c < C.per_frame && image[c] == (int8_t)PWPP_MATCH_OCCUPIED;
        const unsigned long long m = __ballot(on);
        if (lane == 0) wave_n[w] = __popcll(m);
        __syncthreads();
        int32_t before = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
        for (unsigned k = 0; k < kMatchBlock / 64; ++k) {
            const int32_t n = wave_n[k];
            before += k < w ? n : 0;
            total += n;
        }
        if (on) {  // base + before counts occupied cells before c: < per_frame
            const int iy = c / C.G.nx, ix = c - iy * C.G.nx;
            row[base + before] = pwpp_match_pack(ix, iy);
        }
        base += total;
        __syncthreads();
    }
    if (t == 0) count[f] = base;
}

// grid (frames * n_candidates * tiles)
template <bool RECIP, bool STAGE>
__global__ __launch_bounds__(kMatchBlock) void k_match_score(MatchCall C, const int32_t *cells, const int32_t *count, const double *candidates,
                                                             const int32_t *map_of_frame, const int16_t *map, PwppMatchKey *partial, int64_t *scores) {
    __shared__ int2 land[kMatchBlock];
    __shared__ PwppMatchKey keys[kMatchBlock];
    __shared__ int4 box[kMatchBlock / 64];
    extern __shared__ int16_t stage[];  // STAGE: min(NX * NY, kStageHalfwords) halfwords
    const unsigned b = blockIdx.x, t = threadIdx.x;
    const unsigned tile = b % (unsigned)C.tiles, fr = b / (unsigned)C.tiles, r = fr % (unsigned)C.n_candidates, f = fr / (unsigned)C.n_candidates;
    if (f >= (unsigned)C.frames) return;
    const int32_t s = (int32_t)(tile * kMatchBlock + t);  // (shifts <= 129 * 129)
    const bool live = s < C.shifts;
    const int syi = live ? s / C.W : 0, sxi = live ? s - syi * C.W : 0, sx = sxi - C.wx, sy = syi - C.wy;
    const int32_t k = map_of_frame[f];
    const unsigned set = C.n_sets == 1 ? 0u : f;
    int64_t sum = 0;
    if (k >= 0 && k < C.n_maps && set < (unsigned)C.n_sets) {
        const double *cand = candidates + ((size_t)set * (size_t)C.n_candidates + (size_t)r) * 6;
        const int16_t *m = map + (size_t)k * (size_t)C.per_map;
        const int32_t *row = cells + (size_t)f * (size_t)C.per_frame;
        const int32_t n = frame_count(C, count, f);
        // what the gather reads: the map, or the rectangle of it in LDS (then the landings move by its corner)
        const int16_t *src = m;
        int32_t ox = 0, oy = 0, SX = C.G.NX, SY = C.G.NY;
        bool any = true;
        if (STAGE) {
            int32_t lo_x = INT32_MAX, hi_x = INT32_MIN, lo_y = INT32_MAX, hi_y = INT32_MIN;
            for (int32_t c = (int32_t)t; c < n; c += kMatchBlock) {
                int ix, iy;
                int32_t Jx, Jy;
                pwpp_match_unpack(row[c], ix, iy);
                if (ix < C.G.nx && iy < C.G.ny && pwpp_match_landing<RECIP>(C.G, cand, ix, iy, Jx, Jy))
                    lo_x = min(lo_x, Jx), hi_x = max(hi_x, Jx), lo_y = min(lo_y, Jy), hi_y = max(hi_y, Jy);
            }
            const int4 wave = wave_reduce(make_int4(lo_x, hi_x, lo_y, hi_y), [](int4 m, int4 o) { return make_int4(min(m.x, o.x), max(m.y, o.y), min(m.z, o.z), max(m.w, o.w)); });
            lo_x = wave.x, hi_x = wave.y, lo_y = wave.z, hi_y = wave.w;
            if (lane_id() == 0) box[wave_id()] = wave;
            __syncthreads();
            for (unsigned w = 0; w < kMatchBlock / 64; ++w)
                lo_x = min(lo_x, box[w].x), hi_x = max(hi_x, box[w].y), lo_y = min(lo_y, box[w].z), hi_y = max(hi_y, box[w].w);
            int32_t fx, fy, wn, hn;
            const bool some_x = pwpp_match_window(lo_x, hi_x, C.wx, C.G.NX, fx, wn), some_y = pwpp_match_window(lo_y, hi_y, C.wy, C.G.NY, fy, hn);
            any = some_x && some_y;  // (the same for every lane: no cell of the map is in reach, every sum is 0)
            if (any && wn * hn <= kStageHalfwords) {  // (wn, hn <= 32768: compared as a product of two int32 below 2^30)
                for (int32_t i = (int32_t)t; i < wn * hn; i += kMatchBlock) {
                    const int32_t y = i / wn, x = i - y * wn;  // fy + y < NY, fx + x < NX: the window lies inside the map
                    stage[i] = m[(size_t)(fy + y) * (size_t)C.G.NX + (size_t)(fx + x)];
                }
                src = stage, ox = fx, oy = fy, SX = wn, SY = hn;
            }
            __syncthreads();
        }
        for (int32_t c0 = 0; any && c0 < n; c0 += kMatchBlock) {
            int32_t Jx = PWPP_MATCH_NOWHERE, Jy = PWPP_MATCH_NOWHERE;
            if (c0 + (int32_t)t < n) {
                int ix, iy;
                pwpp_match_unpack(row[c0 + (int32_t)t], ix, iy);
                if (ix < C.G.nx && iy < C.G.ny) pwpp_match_landing<RECIP>(C.G, cand, ix, iy, Jx, Jy);
            }
            land[t] = make_int2(Jx - ox, Jy - oy);  // (-2^30 - 32767: still nowhere)
            __syncthreads();
            const int32_t here = n - c0 < kMatchBlock ? n - c0 : kMatchBlock;
            int32_t part = 0;  // |part| <= 256 * 32768
            if (live)
                for (int32_t j = 0; j < here; ++j) {
                    const int2 L = land[j];
                    part += pwpp_match_contribution(src, L.x, L.y, sx, sy, SX, SY);
                }
            sum += (int64_t)part;
            __syncthreads();
        }
    }
    if (scores && live) scores[((size_t)fr * (size_t)C.H + (size_t)syi) * (size_t)C.W + (size_t)sxi] = sum;
    block_best(keys, live ? PwppMatchKey{sum, (int32_t)r, sx, sy, 0} : no_key());
    if (t == 0) partial[(size_t)fr * (size_t)C.tiles + tile] = keys[0];
}

// grid (frames)
__global__ __launch_bounds__(kMatchBlock) void k_match_best(MatchCall C, const int32_t *count, const int32_t *map_of_frame, const PwppMatchKey *partial,
                                                            PwppMatchKey *best) {
    __shared__ PwppMatchKey keys[kMatchBlock];
    const unsigned f = blockIdx.x, t = threadIdx.x;
    if (f >= (unsigned)C.frames) return;
    const uint32_t per = (uint32_t)C.n_candidates * (uint32_t)C.tiles;  // (<= 256 * 66)
    const PwppMatchKey *mine = partial + (size_t)f * (size_t)per;
    PwppMatchKey key = no_key();
    for (uint32_t i = t; i < per; i += kMatchBlock)
        if (pwpp_match_better(mine[i], key)) key = mine[i];
    block_best(keys, key);
    if (t != 0) return;
    const int32_t k = map_of_frame[f], n = frame_count(C, count, f);
    if (k < 0 || k >= C.n_maps) best[f] = PwppMatchKey{0, -1, 0, 0, n};  // skipped
    else best[f] = PwppMatchKey{keys[0].score, keys[0].candidate, keys[0].sx, keys[0].sy, n};
}

}  // namespace

// the words of the working section: the workgroups' bests first (8-byte aligned), then the frames' counts, then the cell list
extern "C" size_t pwpp_match_work_words(int nx, int ny, int frames, int n_candidates, int wx, int wy) {
    const size_t tiles = ((size_t)(2 * wx + 1) * (size_t)(2 * wy + 1) + kMatchBlock - 1) / kMatchBlock;
    const size_t partial = (size_t)frames * (size_t)n_candidates * tiles * (sizeof(PwppMatchKey) / 4);
    return partial + (((size_t)frames + 1) & ~(size_t)1) + (size_t)frames * (size_t)nx * (size_t)ny;
}

// pwpp_match_grid on device memory.  `candidates` (n_sets x n_candidates x 6 doubles, 8-byte aligned) and `map_of_frame` (frames
// entries, each in [-1, n_maps): the host resolved the rule) are device memory, `work` pwpp_match_work_words words; the caller has
// checked the sides (<= 32768), nx * ny * frames and NX * NY * n_maps <= 2^31, n_candidates (1 .. 256), n_sets (1 or frames), wx and
// wy (0 .. 64), frames * n_candidates <= 2^24 and the scores' element count.  `best` is 8-byte aligned; `scores` may be null.
extern "C" int pwpp_launch_match_grid(const PwppMatchGeometry *G, int frames, const int8_t *occupancy, const double *candidates, int n_sets, int n_candidates,
                                      const int32_t *map_of_frame, int n_maps, const int16_t *map, int wx, int wy, void *best, int64_t *scores,
                                      uint32_t *work, int path, hipStream_t stream) {
    MatchCall C;
    C.G = *G;
    C.per_frame = G->nx * G->ny, C.per_map = G->NX * G->NY;
    C.frames = frames, C.n_sets = n_sets, C.n_candidates = n_candidates, C.n_maps = n_maps;
    C.wx = wx, C.wy = wy, C.W = 2 * wx + 1, C.H = 2 * wy + 1;
    C.shifts = C.W * C.H, C.tiles = (C.shifts + kMatchBlock - 1) / kMatchBlock;
    const int64_t blocks = (int64_t)frames * n_candidates * C.tiles;
    if (blocks > INT32_MAX) return (int)hipErrorInvalidConfiguration;
    PwppMatchKey *partial = reinterpret_cast<PwppMatchKey *>(work);
    int32_t *count = reinterpret_cast<int32_t *>(work) + (size_t)blocks * (sizeof(PwppMatchKey) / 4);
    int32_t *cells = count + (((size_t)frames + 1) & ~(size_t)1);
    hipLaunchKernelGGL(k_match_compact, dim3((unsigned)frames), dim3(kMatchBlock), 0, stream, C, occupancy, cells, count);
    const bool stage = path == 2 || (path == 0 && kMatchDefaultStage);
    const size_t lds_bytes = stage ? (size_t)(C.per_map < kStageHalfwords ? C.per_map : kStageHalfwords) * sizeof(int16_t) : 0;
    const auto score = G->inv_CELL != 0.0 ? (stage ? k_match_score<true, true> : k_match_score<true, false>)
                                          : (stage ? k_match_score<false, true> : k_match_score<false, false>);
    if (lds_bytes > 56 * 1024) {  // (with the 8 KiB of static LDS: beyond the 64 KiB a kernel may ask for unannounced)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(score), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(score, dim3((unsigned)blocks), dim3(kMatchBlock), lds_bytes, stream, C, cells, count, candidates, map_of_frame, map, partial, scores);
    hipLaunchKernelGGL(k_match_best, dim3((unsigned)frames), dim3(kMatchBlock), 0, stream, C, count, map_of_frame, partial, static_cast<PwppMatchKey *>(best));
    return (int)hipGetLastError();
}
