// pwpp_evidence.h -- the rule of the per-cluster map evidence (pwpp_evidence_grid, pwpp_evidence_obstacles), one text for the kernels
// (pwpp_evidence.hip), for the host side (pwpp_capi.cpp) and for the host program that runs the same functions against a brute force
// of its own (tools/evidence_check.cpp), the way pwpp_tracks.h is one text for the cluster association.  Internal; include/pwpp.h has
// the contract.
//
// THE LANDING of a labelled frame cell (ix, iy) is the scan match's: pwpp_match_landing of pwpp_match.h under the frame's pose, with
// its choice between the product with the exact reciprocal and the quotient.  Nothing of it is restated here.  The cell is LANDED
// iff that function says so and (Jx, Jy) lies inside the map.  A pose with an element that is not finite lands nothing: every
// element enters X or Y, a product of an infinity is an infinity or a NaN, and neither passes the landing's range test.
// THE READING.  E = the maximum of map[Jy + ey][Jx + ex] over |ex|, |ey| <= gate cut to the map: at most 81 cells, the bounds
// compared before an address is formed.  (Jx, Jy) itself is inside, so the window is never empty.
// THE CLASS of E is the fusion's byte rule, pwpp_fuse_byte of pwpp_fusion.h, with the map's occupied_at and free_at.
// THE COUNTS of a row are integer sums over its cells: cells, landed, occupied, free (32 bits: a frame has at most 2^30 cells) and
// the 64-bit sum of E (|E| <= 2^15, at most 2^30 cells: below 2^46).  Sums have no order, so the bytes do not depend on how the
// kernels deal the cells.  unknown = landed - occupied - free.
// THE VERDICT is evaluated in int64: the shares are 256ths, free * 256 and moving_share * landed stay below 2^39.
#ifndef PWPP_EVIDENCE_H
#define PWPP_EVIDENCE_H

#include <stdint.h>

#include "pwpp_match.h"  // pwpp_match_landing, PwppMatchGeometry; pwpp_fusion.h: PWPP_HD, pwpp_fuse_byte, PwppFusionParams

#define PWPP_EV_MAX_GATE 4
#define PWPP_EV_MAX_TOTAL 16777216  // frames * max_rows: 2^24
#define PWPP_EV_SHARE_ONE 256       // the shares are 1 .. 256, in 256ths
// the verdicts and the byte of a cell without a class: PWPP_EVID_* of include/pwpp.h
#define PWPP_EV_NONE (-1)
#define PWPP_EV_UNDECIDED 0
#define PWPP_EV_STATIC 1
#define PWPP_EV_MOVING 2
#define PWPP_EV_CELL_NONE (-2)
// The rows a workgroup of the count kernel's path 2 keeps in LDS: 24 bytes a row (the 64-bit sum and four counters).  8 waves a SIMD
// are 32 waves a CU, 8 workgroups of 256 lanes; a CU has 160 KiB of LDS, 20 KiB a workgroup: 853 rows.  512 rows are 12 KiB, 96 KiB
// for the eight, and a power of two.  = PWPP_EVID_LDS_ROWS of include/pwpp.h
#define PWPP_EV_LDS_ROWS 512

// a row of the result: pwpp_cluster_evidence of include/pwpp.h (32 bytes, 8-byte aligned)
struct PwppClusterEvidence {
    int64_t sum;
    int32_t cells, landed, occupied, free, unknown, verdict;
};

// the parameters of the verdict: pwpp_evidence_rule of include/pwpp.h
struct PwppEvidenceRule {
    int32_t gate, min_cells, moving_share, static_share;
};

// ---- whether a label names a row
PWPP_HD inline bool pwpp_evid_row(int32_t l, int32_t max_rows) { return l >= 0 && l < max_rows; }

// ---- the range checks of a rule: 0 = in range, else the first parameter outside its range (1 gate, 2 min_cells, 3 moving_share, 4 static_share)
PWPP_HD inline int pwpp_evid_rule_check(const PwppEvidenceRule &R) {
    if (R.gate < 0 || R.gate > PWPP_EV_MAX_GATE) return 1;
    if (R.min_cells < 1) return 2;
    if (R.moving_share < 1 || R.moving_share > PWPP_EV_SHARE_ONE) return 3;
    if (R.static_share < 1 || R.static_share > PWPP_EV_SHARE_ONE) return 4;
    return 0;
}

// ---- whether the frame cell (ix, iy) is landed, and where
template <bool RECIP>
PWPP_HD inline bool pwpp_evid_landed(const PwppMatchGeometry &G, const double *pose, int ix, int iy, int32_t &Jx, int32_t &Jy) {
    if (!pwpp_match_landing<RECIP>(G, pose, ix, iy, Jx, Jy)) return false;
    return Jx >= 0 && Jx < G.NX && Jy >= 0 && Jy < G.NY;
}

// ---- the gated read of a landed cell: `map` is one map, (Jx, Jy) inside it
PWPP_HD inline int32_t pwpp_evid_read(const int16_t *map, int32_t Jx, int32_t Jy, int gate, int NX, int NY) {
    int32_t E = -32768;  // (the smallest value a cell holds; the window has a cell)
    for (int ey = -gate; ey <= gate; ++ey) {
        const int32_t y = Jy + ey;
        if (y < 0 || y >= NY) continue;
        for (int ex = -gate; ex <= gate; ++ex) {
            const int32_t x = Jx + ex;
            if (x < 0 || x >= NX) continue;
            const int32_t v = (int32_t)map[(size_t)y * (size_t)NX + (size_t)x];
            if (v > E) E = v;
        }
    }
    return E;
}

// ---- the class of a reading: the fusion's byte under the map's thresholds
PWPP_HD inline int8_t pwpp_evid_class(int32_t E, int32_t occupied_at, int32_t free_at) {
    const PwppFusionParams P = {0, 0, 0, 0, occupied_at, free_at};
    return pwpp_fuse_byte(E, P);
}

// ---- the verdict of a row from its counts
PWPP_HD inline int32_t pwpp_evid_verdict(const PwppEvidenceRule &R, int32_t cells, int32_t landed, int32_t occupied, int32_t free_) {
    if (cells == 0) return PWPP_EV_NONE;
    const int64_t n = (int64_t)landed;
    if (landed >= R.min_cells && (int64_t)free_ * PWPP_EV_SHARE_ONE >= (int64_t)R.moving_share * n) return PWPP_EV_MOVING;
    if (landed >= R.min_cells && (int64_t)occupied * PWPP_EV_SHARE_ONE >= (int64_t)R.static_share * n) return PWPP_EV_STATIC;
    return PWPP_EV_UNDECIDED;
}

// ---- a finished row from the four sums
PWPP_HD inline PwppClusterEvidence pwpp_evid_finish(const PwppEvidenceRule &R, int64_t sum, int32_t cells, int32_t landed, int32_t occupied, int32_t free_) {
    return PwppClusterEvidence{sum, cells, landed, occupied, free_, landed - occupied - free_, pwpp_evid_verdict(R, cells, landed, occupied, free_)};
}

// ---- the masked occupancy byte of a cell: unknown where the cell's label names a row of a moving verdict, else the input byte
// (`rows`: one frame's finished rows)
PWPP_HD inline int8_t pwpp_evid_mask(int32_t label, int32_t max_rows, const PwppClusterEvidence *rows, int8_t in) {
    return pwpp_evid_row(label, max_rows) && rows[label].verdict == PWPP_EV_MOVING ? (int8_t)PWPP_FUSE_UNKNOWN : in;
}

// ---- the class byte of a cell of the class image: `map` is the frame's map, or null for a skipped frame
template <bool RECIP>
PWPP_HD inline int8_t pwpp_evid_cell_class(const PwppMatchGeometry &G, const double *pose, int ix, int iy, int32_t label, int32_t max_rows, const int16_t *map, int gate,
                                           int32_t occupied_at, int32_t free_at) {
    int32_t Jx = 0, Jy = 0;
    if (!map || !pwpp_evid_row(label, max_rows) || !pwpp_evid_landed<RECIP>(G, pose, ix, iy, Jx, Jy)) return (int8_t)PWPP_EV_CELL_NONE;
    return pwpp_evid_class(pwpp_evid_read(map, Jx, Jy, gate, G.NX, G.NY), occupied_at, free_at);
}

#endif
