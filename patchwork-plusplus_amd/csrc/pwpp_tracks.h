// pwpp_tracks.h -- the rule of the cluster association (pwpp_associate_grid, pwpp_track_obstacles), one text for the kernels
// (pwpp_tracks.hip), for the host side (pwpp_capi.cpp) and for the host program that runs the same functions against a brute force
// of its own (tools/tracks_check.cpp), the way pwpp_reach.h is one text for the cost-to-reach field.  Internal; include/pwpp.h has
// the contract.
//
// THE PREVIOUS CELL of a current cell (jx, jy): its centre by the elevation fusion's rule (pwpp_elev_position) carried into the
// previous grid by pwpp_fuse_cell_of, with the current grid in the role of the map (X0, Y0, CELL, NX, NY of PwppFusionGeometry) and
// the previous image in the role of the frame (x0, y0, cell, nx, ny).  Nothing of that is restated here.
// THE GATE'S ORDER.  Among the labelled previous cells d = p + (ex, ey), |ex|, |ey| <= gate, inside the image, the vote goes to
// the smallest ex^2 + ey^2, then the smallest index.  ex^2 + ey^2 <= 32 and an index is below 2^30 (sides <= 32768), so
// (ex^2 + ey^2) << 32 | index is one 64-bit key whose minimum is that winner: a total order, no two cells share a key.
// THE ARGMAX.  "The largest overlap, the smallest label on a tie" is the maximum of overlap << 32 | (0x7fffffff - label): overlap
// >= 1 for a pair that exists, so 0 says "no pair", and labels are below 2^24.  A 64-bit atomic maximum per row computes it in
// any order of arrival.
// THE TABLE.  Per frame an open-addressed table of SLOTS = 2 * max_pairs slots holds the pairs (b, a) as b << 32 | a (never
// PWPP_TRACKS_EMPTY: rows are below 2^24) with their counts, linear probing from pwpp_tracks_hash % SLOTS, at most SLOTS probes.
// A frame's counter `distinct` counts the insertions of a new key.  BOUND: an insertion fails only when all 2 * max_pairs slots
// hold other keys, that is after 2 * max_pairs >= max_pairs + 1 distinct insertions.  So (1) with D <= max_pairs distinct pairs no
// insertion ever fails and distinct ends at D; (2) with D > max_pairs either every pair went in and distinct = D, or one failed
// and distinct = 2 * max_pairs: both exceed max_pairs.  distinct > max_pairs <=> D > max_pairs, whatever the schedule; the table's
// contents are read only where distinct <= max_pairs, where they are complete.
// THE IDS.  Existing row b (cells > 0) continues a iff curr.other == a >= 0, prev[a].other == b, overlap >= min_overlap and
// id_prev[a] >= 0; a mutual best is unique (b names one a, a names one b), so continued ids stay distinct.  Every other existing
// row takes (next_id + k) & 0x7fffffff in unsigned 32-bit arithmetic, k = the fresh rows below it.
#ifndef PWPP_TRACKS_H
#define PWPP_TRACKS_H

#include <stdint.h>

#include "pwpp_elevation.h"  // pwpp_elev_position; pwpp_fusion.h: PwppFusionGeometry, pwpp_fuse_cell_of, pwpp_fuse_reciprocal

#define PWPP_TRACKS_MAX_GATE 4
#define PWPP_TRACKS_MAX_TOTAL 16777216            // frames * max_rows, frames * max_pairs: 2^24
#define PWPP_TRACKS_EMPTY 0xffffffffffffffffull   // a slot without a key
#define PWPP_TRACKS_OVERFLOWED (-2)               // `other` of every row of a frame with more than max_pairs pairs

// a row of a link table: pwpp_cluster_link of include/pwpp.h
struct PwppClusterLink {
    int32_t other, overlap, cells, links;
};

// the parameters of a call, checked by the host
struct PwppTracksRule {
    int32_t gate, min_overlap, max_rows, max_pairs;
    uint32_t slots;  // pwpp_tracks_slots(max_pairs)
    int32_t with_ids;
};

// ---- whether a label names a row
PWPP_HD inline bool pwpp_tracks_row(int32_t l, int32_t max_rows) { return l >= 0 && l < max_rows; }

// ---- the slots of a frame's table: twice max_pairs (THE TABLE above has the argument); max_pairs <= 2^24
PWPP_HD inline uint32_t pwpp_tracks_slots(int32_t max_pairs) { return 2u * (uint32_t)max_pairs; }

// ---- the gate's total order: smaller is better
PWPP_HD inline uint64_t pwpp_tracks_gate_key(int ex, int ey, int32_t index) { return ((uint64_t)(uint32_t)(ex * ex + ey * ey) << 32) | (uint64_t)(uint32_t)index; }

// ---- the vote of the current cell (jx, jy): the row of the winning labelled previous cell, or -1: no vote.  `prev`: one frame's image.
template <bool RECIP>
PWPP_HD inline int32_t pwpp_tracks_vote(const PwppFusionGeometry &G, const double *pose, int jx, int jy, const int32_t *prev, int gate, int32_t max_rows) {
    const double mx = pwpp_elev_position(G.X0, jx, G.CELL), my = pwpp_elev_position(G.Y0, jy, G.CELL);
    int px = 0, py = 0;
    if (!pwpp_fuse_cell_of<RECIP>(G, pose, mx, my, px, py)) return -1;
    const int32_t here = prev[(size_t)py * (size_t)G.nx + (size_t)px];
    if (pwpp_tracks_row(here, max_rows)) return here;  // (ex = ey = 0: the smallest key there is)
    uint64_t best = PWPP_TRACKS_EMPTY;
    int32_t vote = -1;
    for (int ey = -gate; ey <= gate; ++ey) {
        const int y = py + ey;
        if (y < 0 || y >= G.ny) continue;
        for (int ex = -gate; ex <= gate; ++ex) {
            const int x = px + ex;
            if (x < 0 || x >= G.nx) continue;
            const int32_t index = y * G.nx + x;  // (< 2^30)
            const int32_t l = prev[index];
            if (!pwpp_tracks_row(l, max_rows)) continue;
            const uint64_t key = pwpp_tracks_gate_key(ex, ey, index);
            if (key < best) best = key, vote = l;
        }
    }
    return vote;
}

// ---- a pair as the table's key, and where its probing starts
PWPP_HD inline uint64_t pwpp_tracks_pair(int32_t b, int32_t a) { return ((uint64_t)(uint32_t)b << 32) | (uint64_t)(uint32_t)a; }
PWPP_HD inline int32_t pwpp_tracks_pair_curr(uint64_t key) { return (int32_t)(key >> 32); }
PWPP_HD inline int32_t pwpp_tracks_pair_prev(uint64_t key) { return (int32_t)(key & 0xffffffffu); }
PWPP_HD inline uint32_t pwpp_tracks_hash(uint64_t key, uint32_t slots) {
    uint64_t x = key * 0x9e3779b97f4a7c15ull;  // (Fibonacci hashing; any function of the key would do: it moves no result)
    x ^= x >> 29;
    return (uint32_t)(x % (uint64_t)slots);
}

// ---- the packed argmax key and what it unpacks to
PWPP_HD inline uint64_t pwpp_tracks_pack(uint32_t overlap, int32_t label) { return ((uint64_t)overlap << 32) | (uint64_t)(uint32_t)(0x7fffffff - label); }
PWPP_HD inline int32_t pwpp_tracks_best_label(uint64_t best) { return best == 0 ? -1 : 0x7fffffff - (int32_t)(best & 0xffffffffu); }
PWPP_HD inline int32_t pwpp_tracks_best_overlap(uint64_t best) { return (int32_t)(best >> 32); }

// ---- what a frame reports for its pairs
PWPP_HD inline bool pwpp_tracks_overflowed(uint32_t distinct, int32_t max_pairs) { return distinct > (uint32_t)max_pairs; }
PWPP_HD inline int32_t pwpp_tracks_n_pairs(uint32_t distinct, int32_t max_pairs) { return pwpp_tracks_overflowed(distinct, max_pairs) ? max_pairs + 1 : (int32_t)distinct; }

// ---- a row of a link table from its counts and its argmax
PWPP_HD inline PwppClusterLink pwpp_tracks_link(int32_t cells, int32_t links, uint64_t best, bool overflowed) {
    if (overflowed) return PwppClusterLink{PWPP_TRACKS_OVERFLOWED, 0, cells, 0};
    return PwppClusterLink{pwpp_tracks_best_label(best), pwpp_tracks_best_overlap(best), cells, links};
}

// ---- the ids: whether the existing current row b continues its best previous row (`curr`: row b of the current table; `prev_of_other`:
// row curr.other of the previous table, read only where curr.other >= 0; `id_prev_of_other`: that row's id)
PWPP_HD inline bool pwpp_tracks_continues(const PwppClusterLink &curr, int32_t b, const PwppClusterLink &prev_of_other, int32_t id_prev_of_other, int32_t min_overlap) {
    return curr.other >= 0 && prev_of_other.other == b && curr.overlap >= min_overlap && id_prev_of_other >= 0;
}
PWPP_HD inline int32_t pwpp_tracks_fresh_id(int32_t next_id, uint32_t k) { return (int32_t)(((uint32_t)next_id + k) & 0x7fffffffu); }

#endif
