// pwpp_wave.h -- the cross-lane primitives of the gfx950 kernels, stated once (device code only).
// Names for the DPP and swizzle controls, lane_id / wave_id, ONE butterfly reduction (wave_reduce) with the sums, minima and maxima
// on top of it, the DPP inclusive scan of a wave with the block scan built on it, the group loop (wave_for_each_group) and the few
// other wave-wide helpers.  A wave is 64 lanes everywhere in this library.
#ifndef PWPP_WAVE_H
#define PWPP_WAVE_H

#include <stdint.h>

#include <type_traits>

#include <hip/hip_runtime.h>

// ---- DPP and ds_swizzle controls -------------------------------------------------------------------------------------------------
// The four steps inside a 16-lane DPP row are register-to-register (v_*_dpp quad_perm / row_half_mirror / row_mirror, ~8 cycles
// each); 16 <-> 16 goes through ds_swizzle(SWAP,16).
#define PWPP_DPP_XOR1 0xB1        // quad_perm [1,0,3,2]
#define PWPP_DPP_XOR2 0x4E        // quad_perm [2,3,0,1]
#define PWPP_DPP_QMIR 0x1B        // quad_perm [3,2,1,0]: the mirror of a quad
#define PWPP_DPP_HMIR 0x141       // row_half_mirror
#define PWPP_DPP_MIR 0x140        // row_mirror
#define PWPP_DPP_SHL4 0x104       // row_shl:4
#define PWPP_DPP_SHR1 0x111       // row_shr:1
#define PWPP_DPP_SHR2 0x112       // row_shr:2
#define PWPP_DPP_SHR4 0x114       // row_shr:4
#define PWPP_DPP_SHR8 0x118       // row_shr:8
#define PWPP_DPP_ROR8 0x128       // row_ror:8
#define PWPP_DPP_WAVE_SHR1 0x138  // wave_shr:1
#define PWPP_DPP_BCAST15 0x142    // row_bcast:15: a row's last lane into the row behind it (row mask 0xA: rows 1 and 3)
#define PWPP_DPP_BCAST31 0x143    // row_bcast:31: lane 31 into rows 2 and 3 (row mask 0xC)
#define PWPP_SWZ8 0x201F          // ds_swizzle BITMASK_PERM xor 8
#define PWPP_SWZ16 0x401F         // ds_swizzle BITMASK_PERM xor 16
// a 32-bit move under a control: every lane has a source (bound_ctrl), signed and unsigned
#define PWPP_DPP(x, ctrl) __builtin_amdgcn_update_dpp(0, (x), (ctrl), 0xF, 0xF, true)
#define PWPP_DPPU(x, ctrl) ((unsigned)__builtin_amdgcn_update_dpp(0, (int)(x), (ctrl), 0xF, 0xF, true))
// ... and where a lane without a source adds 0 (the scans' shifts and broadcasts: row mask `rows`)
#define PWPP_DPP_OR0(x, ctrl, rows) __builtin_amdgcn_update_dpp(0, (x), (ctrl), (rows), 0xF, false)

namespace {

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ int wave_id() { return threadIdx.x >> 6; }

// two moved 32-bit halves as the register pair of ONE 64-bit operand (v_lshl_add_u64 takes it as it stands); written with shifts
// and ORs the compiler splits a following add into two 64-bit adds plus a move
__device__ __forceinline__ long long dpp_pair_i64(int lo, int hi) {
    typedef int v2i __attribute__((ext_vector_type(2)));
    const v2i pair = {lo, hi};
    return __builtin_bit_cast(long long, pair);
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, 0xf, 0xf, true);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

// ---- the butterfly ---------------------------------------------------------------------------------------------------------------
// Six rounds, the partner at xor 32 first: v = combine(v, the partner's v).  Every lane of the wave calls it; with a combine that
// is associative and commutative (sums, minima and maxima, a maximum under a total order) every lane ends with the wave's result.
// T: whatever __shfl_xor takes, or a struct of several values folded together (whole 32-bit words: it moves word by word, in order, its padding too).
template <class T>
__device__ __forceinline__ T wave_xor_lane(T v, int d) {
    if constexpr (std::is_arithmetic<T>::value) {
        return __shfl_xor(v, d, 64);
    } else {
        static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0, "whole 32-bit words");
        int w[sizeof(T) / 4];
        __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
        for (unsigned i = 0; i < sizeof(T) / 4; ++i) w[i] = __shfl_xor(w[i], d, 64);
        __builtin_memcpy(&v, w, sizeof(T));
        return v;
    }
}
template <class T, class Combine>
__device__ __forceinline__ T wave_reduce(T v, Combine combine) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = combine(v, wave_xor_lane(v, d));
    return v;
}
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
    return wave_reduce(v, [](T a, T b) { return a + b; });
}
template <class T>
__device__ __forceinline__ T wave_min(T v) {
    return wave_reduce(v, [](T a, T b) { return b < a ? b : a; });
}
template <class T>
__device__ __forceinline__ T wave_max(T v) {
    return wave_reduce(v, [](T a, T b) { return b > a ? b : a; });
}

// ---- scans -----------------------------------------------------------------------------------------------------------------------
// Cross-lane moves on the VALU (DPP) instead of through the LDS crossbar (ds_bpermute).  The inclusive prefix sum of a 16-lane row
// in four adds (row_shr 1/2/4/8; lanes without a source add 0) ...
__device__ __forceinline__ int row16_incl_scan(int x) {
    x += PWPP_DPP_OR0(x, PWPP_DPP_SHR1, 0xF);
    x += PWPP_DPP_OR0(x, PWPP_DPP_SHR2, 0xF);
    x += PWPP_DPP_OR0(x, PWPP_DPP_SHR4, 0xF);
    x += PWPP_DPP_OR0(x, PWPP_DPP_SHR8, 0xF);
    return x;
}
// ... and of a wave in six: then the rows' last lanes broadcast into the rows behind.  The broadcasts read lanes 15, 31 and 47 whatever
// the caller's EXEC is: ALL 64 LANES MUST BE ACTIVE at the call.
__device__ __forceinline__ unsigned wave_incl_scan(unsigned v) {
    int x = row16_incl_scan((int)v);
    x += PWPP_DPP_OR0(x, PWPP_DPP_BCAST15, 0xA);
    x += PWPP_DPP_OR0(x, PWPP_DPP_BCAST31, 0xC);
    return (unsigned)x;
}
// lane i reads lane i - 1 of the wave (lane 0 gets `first`)
__device__ __forceinline__ unsigned wave_prev_lane(unsigned x, unsigned first) {
    return (unsigned)__builtin_amdgcn_update_dpp((int)first, (int)x, PWPP_DPP_WAVE_SHR1, 0xF, 0xF, false);
}
// A workgroup of WAVES whole waves, every thread at the call (two barriers inside; wave_incl_scan: all lanes active).  v[q]: this
// thread's sum of quantity q; returns the exclusive prefix over the threads in v and the block's totals in `total`, in every thread.
// s_wave: LDS, free again at the return.
template <int K, int WAVES>
__device__ __forceinline__ void block_excl_scan(unsigned v[K], unsigned (*s_wave)[K], unsigned total[K]) {
    const int ln = lane_id(), wv = wave_id();
    unsigned incl[K];
#pragma unroll
    for (int q = 0; q < K; ++q) {
        incl[q] = wave_incl_scan(v[q]);
        if (ln == 63) s_wave[wv][q] = incl[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < K; ++q) {
        unsigned before = 0, all = 0;
        for (int w = 0; w < WAVES; ++w) {
            const unsigned t = s_wave[w][q];
            if (w < wv) before += t;
            all += t;
        }
        v[q] = incl[q] - v[q] + before;
        total[q] = all;
    }
    __syncthreads();
}

// ---- the group loop --------------------------------------------------------------------------------------------------------------
// The lanes of a wave that hold the same key become one group per round, the group of the first lane still pending, and
// body(leader, same, mine) runs for it: the group's first lane, the ballot of its lanes, and whether the calling lane is one of them.
// THE CONTRACT:
//   - every lane of the wave that is active at the call calls it together; valid = false: the lane holds no key and joins no group;
//   - `pending` starts as the ballot of `valid` and loses a whole group per round (the lanes of one key are pending together or not
//     at all), so it is the same in every lane: all lanes leave the loop in the same round;
//   - at most 64 rounds, one per distinct key of the wave; the bound stands in the loop itself;
//   - body runs in EVERY lane, in uniform control flow, and may itself call wave-wide functions (ballots, wave_sum, a shuffle from
//     `leader`); what only one lane may do -- the atomic for the group -- it puts under `lane_id() == leader`.
// Key: 32 or 64 bits, an integer type __shfl takes (a 64-bit key moves as two 32-bit shuffles).
template <class Key, class Body>
__device__ __forceinline__ void wave_for_each_group(Key key, bool valid, Body body) {
    static_assert(sizeof(Key) == 4 || sizeof(Key) == 8, "a key of 32 or 64 bits");
    unsigned long long pending = __ballot(valid);
    for (int round = 0; round < 64 && pending; ++round) {
        const int leader = __ffsll((long long)pending) - 1;
        const bool mine = valid && key == __shfl(key, leader, 64);
        const unsigned long long same = __ballot(mine);
        pending &= ~same;
        body(leader, same, mine);
    }
}

// ---- other wave-wide helpers -----------------------------------------------------------------------------------------------------
// the largest of the lanes' values in 0..255: a binary search over the bits with ballots (scalar work, no cross-lane data path)
__device__ __forceinline__ int wave_max_u8(int v) {
    int cur = 0;
#pragma unroll
    for (int bit = 7; bit >= 0; --bit) {
        const int cand = cur | (1 << bit);
        if (__ballot(v >= cand)) cur = cand;
    }
    return cur;
}
// Sum over the wave in butterfly order (quad_perm xor 1, xor 2, row_half_mirror, row_mirror, then the four rows): ONLY for sums
// that are exact in every order (k_gle_tgr's first pass over a history).  The result is wave-uniform.
__device__ __forceinline__ double wave_sum_f64_any_order(double v) {
    v += dpp_f64<PWPP_DPP_XOR1>(v);
    v += dpp_f64<PWPP_DPP_XOR2>(v);
    v += dpp_f64<PWPP_DPP_HMIR>(v);
    v += dpp_f64<PWPP_DPP_MIR>(v);
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    double r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, 16 * k), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), 16 * k);
        r[k] = __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    }
    return (r[0] + r[1]) + (r[2] + r[3]);
}
// hand-over through LDS between the lanes of ONE wave (no workgroup barrier)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace

#endif  // PWPP_WAVE_H
