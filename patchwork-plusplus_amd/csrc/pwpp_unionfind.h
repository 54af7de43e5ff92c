// pwpp_unionfind.h -- the union-find primitives of the obstacle clusters (pwpp_label_grid), one text for the kernels
// (pwpp_clusters.hip), and for the host program that checks the whole sequence against a flood fill (tools/unionfind_check.cpp),
// the way pwpp_transform_point is one function for host and kernels.  Internal; the public boundary is include/pwpp.h.
//
// A forest over the occupied cells of ONE frame, stored as one int32 word per cell: the word of an occupied cell is the index of
// its parent, and a parent is never a LARGER index than its child; a root names itself; an unoccupied cell holds -1 and is never
// followed.  The words are reached through a policy type M:
//     int32_t M::load(int32_t i)                    the word of cell i
//     int32_t M::fetch_min(int32_t i, int32_t v)    word = min(word, v), the old value returned, as ONE atomic step
// -- plain memory on the host, LDS words inside a tile, agent-scope atomics on the label image (pwpp_clusters.hip says why).
//
// Why concurrent unions are safe with nothing but load and fetch_min.  (1) A word only ever decreases, and only to the index of
// a cell of its own component: uf_union links a root to a root of a cell that IS connected to it.  (2) So a chase from x visits
// strictly smaller indices and ends, after at most x steps, at a cell that named itself when it was read: a stale or racing read
// makes the chase longer or ends it at a cell that has stopped being a root meanwhile -- never in another component.
// (3) uf_union only believes a link it made itself: fetch_min returns the old word, and only old == a proves that a was still a
// root when it was linked below b.  Otherwise somebody else linked a first, to `old`: the word now holds min(old, b), one of the
// two equivalences {a ~ old, a ~ b} is stored in it and the OTHER is owed, and in both cases what is owed is old ~ b: the loop
// goes on with that pair.  No equivalence is dropped, so when every union of a launch has returned, two cells have one root iff
// they are connected, and that root is the component's smallest cell (every link points downwards).
// Every loop has an explicit bound: a chase is at most `bound` = cells per frame steps by construction, a union retries only
// when another union succeeded on the same word.  A defect shows as a wrong label, not as a kernel that never ends.
#ifndef PWPP_UNIONFIND_H
#define PWPP_UNIONFIND_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PWPP_HD __host__ __device__
#else
#define PWPP_HD
#endif

// the root of x as far as the words read say: the first cell on the chain from x that names itself (or whose word does not
// point downwards: -1 or a larger index can only be a defect, and end the chase)
template <class M>
PWPP_HD inline int32_t uf_find(M &m, int32_t x, int32_t bound) {
    for (int32_t s = 0; s < bound; ++s) {
        const int32_t p = m.load(x);
        if (p < 0 || p >= x) break;
        x = p;
    }
    return x;
}

// a ~ b
template <class M>
PWPP_HD inline void uf_union(M &m, int32_t a, int32_t b, int32_t bound) {
    for (int32_t s = 0; s <= bound; ++s) {
        a = uf_find(m, a, bound);
        b = uf_find(m, b, bound);
        if (a == b) return;
        if (a < b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        const int32_t old = m.fetch_min(a, b);  // the larger root below the smaller
        if (old == a) return;                   // a was a root: linked
        a = old;                                // somebody linked a to `old` first: old ~ b is owed (see above)
    }
}

// the word of x becomes its root (a decrease like every other write); the root is returned
template <class M>
PWPP_HD inline int32_t uf_compress(M &m, int32_t x, int32_t bound) {
    const int32_t r = uf_find(m, x, bound);
    if (r != x) (void)m.fetch_min(x, r);
    return r;
}

// The neighbours a cell (x, y) of an nx-wide image looks at: W, N and, for 8-connectivity, NW and NE.  Every pair of neighbouring
// cells is looked at from exactly one side.  k = 0..3; false: no such neighbour.
PWPP_HD inline bool uf_neighbour(int k, int connectivity, int x, int y, int nx, int &qx, int &qy) {
    if (k >= (connectivity == 8 ? 4 : 2)) return false;
    qx = x + (k == 0 || k == 2 ? -1 : (k == 3 ? 1 : 0));
    qy = y - (k == 0 ? 0 : 1);
    return qx >= 0 && qx < nx && qy >= 0;
}

// the monotone integer key of a height (pwpp_rasterize_obstacles: -0.0 < +0.0; 0 = empty, it would be the key of the NaN
// 0xffffffff) and its inverse
PWPP_HD inline uint32_t pwpp_height_key(float h) {
    const uint32_t b = __builtin_bit_cast(uint32_t, h);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
PWPP_HD inline float pwpp_height_of_key(uint32_t k) {
    return __builtin_bit_cast(float, k == 0u ? 0x7fc00000u : (k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)));
}

// geometry of the passes, shared with the host program
#define PWPP_CL_TILE_X 64    // a tile of the tile pass: 64 x 16 cells of one frame
#define PWPP_CL_TILE_Y 16
#define PWPP_CL_CHUNK 256    // cells per counting unit of the rank: a run of the frame's cells in ROW-MAJOR order

#endif
