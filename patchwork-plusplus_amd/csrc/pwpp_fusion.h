// pwpp_fusion.h -- the arithmetic of the occupancy fusion (pwpp_fuse_grid, pwpp_fuse_obstacles), one text for the kernel
// (pwpp_fusion.hip), for the host side (pwpp_capi.cpp) and for the host program that runs the same functions against a brute force
// of its own (tools/fusion_check.cpp), the way pwpp_visibility.h is one text for the visibility.  Internal; include/pwpp.h has the
// contract.
//
// THE SAMPLES.  A map cell (jx, jy) asks a frame at the centres of its four quadrants, q = (qx, qy) in {0, 1}^2:
//     mx = X0 + ((double)jx + (0.25 + 0.5 * qx)) * CELL      (0.25 + 0.5 * qx and the sum with jx are exact; one product, one sum)
//     dx = mx - tx, dy = my - ty;   fx = a * dx + c * dy,  fy = b * dx + d * dy      (the TRANSPOSE of the pose's matrix)
//     u = (fx - x0) / cell, inside iff 0 <= u && u < nx, ix = (int)floor(u)           (the cell rule of the obstacle raster)
// all in double, every product, sum and quotient rounded on its own: the build's -ffp-contract=off is part of the contract.  mx
// and my do not depend on the frame: pwpp_fuse_cell computes the two of each once per cell.  A sample outside the image, or
// with a NaN for u or v, reads PWPP_FUSE_UNKNOWN and forms no address.
// THE QUOTIENT WITHOUT A DIVISION.  Where cell is a power of two whose reciprocal is a normal double (0.5 m, 0.25 m, 1 m ...),
// inv = 1 / cell is exact, and (fx - x0) * inv and (fx - x0) / cell are both the correctly rounded value of the same real number:
// the same bits for every operand, infinities, NaNs, overflow and underflow included.  pwpp_fuse_reciprocal decides it on the host;
// the functions below take RECIP as a template argument, and RECIP = false, the division as written, is the yardstick.
// THE OBSERVATION of a cell in a frame: occupied if any sample reads exactly 100, else free if all four read exactly 0, else none.
// THE UPDATE in int32: occupied L = min(L + hit, l_max), free L = max(L - miss, l_min).  With an int16 L and hit, miss in
// 0 .. 32767 neither sum leaves int32, and the result lies in the int16 range again: min(L + hit, l_max) <= 32767 and >= L,
// max(L - miss, l_min) >= -32768 and <= L.
// THE DEALING of map cells to lanes and the CSR of each map's frames, for this fusion and pwpp_elevation.h's: pwpp_map_runs, _lane, _lists.
#ifndef PWPP_FUSION_H
#define PWPP_FUSION_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "pwpp_unionfind.h"  // PWPP_HD

#define PWPP_FUSE_FREE 0  // = PWPP_OCC_FREE, PWPP_OCC_OCCUPIED, PWPP_OCC_UNKNOWN of include/pwpp.h
#define PWPP_FUSE_OCCUPIED 100
#define PWPP_FUSE_UNKNOWN (-1)
#define PWPP_FUSE_MAX_SIDE 32768  // NX, NY, nx, ny
#define PWPP_FUSE_RUN 256         // map cells of a workgroup: a run of the map in row-major order, a lane per cell

// The geometry of a call: the map's grid in the fixed frame and the frame images' grid (the first 56 + 32 bytes are plain copies of
// the caller's structures' fields).
struct PwppFusionGeometry {
    double X0, Y0, CELL;  // the map
    double x0, y0, cell;  // the frame images
    int32_t NX, NY, nx, ny;
    double inv_cell;      // 1 / cell where pwpp_fuse_reciprocal allows the product, else 0
};

// the update's parameters and the thresholds of the derived byte, checked by the host
struct PwppFusionParams {
    int32_t hit, miss, l_min, l_max, occupied_at, free_at;
};

// ---- whether u = n / cell may be formed as n * inv: cell a normal power of two with a normal reciprocal (both exact)
inline bool pwpp_fuse_reciprocal(double cell, double &inv) {
    int e = 0;
    inv = 0.0;
    if (!(cell > 0.0) || !isfinite(cell) || frexp(cell, &e) != 0.5 || e < -1020 || e > 1020) return false;
    inv = 1.0 / cell;
    return true;
}

// ---- THE LANE OF A MAP RUN, for both fusions: a workgroup per (map, run of PWPP_FUSE_RUN cells in row-major order), block = map * runs +
// run, a lane per map cell, each map's frames from the CSR of map_of_frame.  The counts of a call, the tail of the kernels' argument structs:
struct PwppMapRuns {
    int32_t per_map, runs;  // NX * NY (<= 2^30); ceil(per_map / PWPP_FUSE_RUN)
    int32_t n_maps, frames, n_poses, listed;
};

// fills the counts; returns the number of workgroups, or -1 where a grid cannot hold them
inline int64_t pwpp_map_runs(const PwppFusionGeometry &G, int n_maps, int frames, int n_poses, int listed, PwppMapRuns &R) {
    R.per_map = G.NX * G.NY, R.runs = (R.per_map + PWPP_FUSE_RUN - 1) / PWPP_FUSE_RUN;
    R.n_maps = n_maps, R.frames = frames, R.n_poses = n_poses, R.listed = listed;
    const int64_t blocks = (int64_t)n_maps * R.runs;
    return blocks > INT32_MAX ? -1 : blocks;
}

// What a lane works on: cell c = (jx, jy) of map k, whose cells begin at mbase; the map's shift; its frames list[first .. last).
struct PwppMapLane {
    int32_t k, c, jx, jy, sx, sy, first, last;
    size_t mbase;
};
// Calls cell(const PwppMapLane &) for the cell of lane `lane` of workgroup `block`, or not at all: the lane has no cell.  `shift`: n_maps x
// {sx, sy}, or null: none.  `begin` is ascending and ends at `listed` (the host built it); the clamps bound the loop all the same.
template <class Cell>
PWPP_HD inline void pwpp_map_lane(const PwppMapRuns &R, int NX, unsigned block, unsigned lane, const int32_t *shift, const int32_t *begin, Cell cell) {
    const unsigned run = block % (unsigned)R.runs, k = block / (unsigned)R.runs;
    if (k >= (unsigned)R.n_maps) return;
    const int c = (int)run * PWPP_FUSE_RUN + (int)lane;  // (per_map <= 2^30)
    if (c >= R.per_map) return;
    PwppMapLane l;
    l.k = (int32_t)k, l.c = c;
    l.jy = c / NX, l.jx = c - l.jy * NX;
    l.mbase = (size_t)k * (size_t)R.per_map;
    l.sx = shift ? shift[2 * (size_t)k] : 0, l.sy = shift ? shift[2 * (size_t)k + 1] : 0;
    const int32_t b0 = begin[k], b1 = begin[(size_t)k + 1];
    l.first = b0 > 0 ? b0 : 0, l.last = b1 < R.listed ? b1 : R.listed;
    cell(l);
}

// ---- which map frame i updates under the caller's map_of_frame (null: one map for all, or frame i's is map i; -1: none), and the
// CSR of that rule: a counting sort of the frames by their map keeps each map's frames in ascending order.  begin[n_maps + 1], list[].
inline int32_t pwpp_map_of_frame(const int32_t *map_of_frame, int n_maps, int i) { return map_of_frame ? map_of_frame[i] : (n_maps == 1 ? 0 : i); }
inline void pwpp_map_lists(const int32_t *map_of_frame, int n_maps, int frames, std::vector<int32_t> &begin, std::vector<int32_t> &list) {
    begin.assign((size_t)n_maps + 1, 0);
    int listed = 0;
    for (int i = 0; i < frames; ++i)
        if (pwpp_map_of_frame(map_of_frame, n_maps, i) >= 0) ++begin[(size_t)pwpp_map_of_frame(map_of_frame, n_maps, i) + 1], ++listed;
    for (int k = 0; k < n_maps; ++k) begin[(size_t)k + 1] += begin[k];
    list.assign((size_t)listed, 0);
    std::vector<int32_t> next(begin.begin(), begin.end() - 1);
    for (int i = 0; i < frames; ++i)
        if (pwpp_map_of_frame(map_of_frame, n_maps, i) >= 0) list[(size_t)next[(size_t)pwpp_map_of_frame(map_of_frame, n_maps, i)]++] = i;
}

// ---- the start of a cell: the shifted read.  (jx + sx, jy + sy) in 64 bits: |sx| may be anything an int32 holds.
PWPP_HD inline int32_t pwpp_fuse_start(const int16_t *map_in /* one map, or null */, int jx, int jy, int32_t sx, int32_t sy, int NX, int NY) {
    const int64_t qx = (int64_t)jx + (int64_t)sx, qy = (int64_t)jy + (int64_t)sy;
    if (!map_in || qx < 0 || qx >= (int64_t)NX || qy < 0 || qy >= (int64_t)NY) return 0;
    return (int32_t)map_in[(size_t)qy * (size_t)NX + (size_t)qx];
}

// ---- the sample positions of a cell along one axis, in the map's frame: p[0] the lower quadrants', p[1] the upper ones'
PWPP_HD inline double pwpp_fuse_position(double X0, int j, int q, double CELL) { return X0 + ((double)j + (0.25 + 0.5 * (double)q)) * CELL; }

// ---- where the position (mx, my) of the map's frame lies in a frame image, in cells: the pose {a, b, tx, c, d, ty}, transposed
template <bool RECIP>
PWPP_HD inline void pwpp_fuse_uv(const PwppFusionGeometry &G, const double *pose, double mx, double my, double &u, double &v) {
    const double a = pose[0], b = pose[1], tx = pose[2], c = pose[3], d = pose[4], ty = pose[5];
    const double dx = mx - tx, dy = my - ty;
    const double fx = a * dx + c * dy, fy = b * dx + d * dy;
    u = RECIP ? (fx - G.x0) * G.inv_cell : (fx - G.x0) / G.cell, v = RECIP ? (fy - G.y0) * G.inv_cell : (fy - G.y0) / G.cell;
}

// ---- the frame cell under that position: false where it lies outside the image (a NaN: outside).  What the elevation fusion
// (pwpp_elevation.h) asks at a cell's centre.
template <bool RECIP>
PWPP_HD inline bool pwpp_fuse_cell_of(const PwppFusionGeometry &G, const double *pose, double mx, double my, int &ix, int &iy) {
    double u, v;
    pwpp_fuse_uv<RECIP>(G, pose, mx, my, u, v);
    if (!(u >= 0.0 && u < (double)G.nx && v >= 0.0 && v < (double)G.ny)) return false;
    ix = (int)floor(u), iy = (int)floor(v);
    return (unsigned)ix < (unsigned)G.nx && (unsigned)iy < (unsigned)G.ny;  // (always: 0 <= floor(u) <= u < nx)
}

// ---- the byte one sample reads
template <bool RECIP>
PWPP_HD inline int8_t pwpp_fuse_sample(const PwppFusionGeometry &G, const double *pose, double mx, double my, const int8_t *image /* one frame */) {
    double u, v;
    pwpp_fuse_uv<RECIP>(G, pose, mx, my, u, v);
    if (!(u >= 0.0 && u < (double)G.nx && v >= 0.0 && v < (double)G.ny)) return (int8_t)PWPP_FUSE_UNKNOWN;  // (a NaN: outside)
    const int ix = (int)floor(u), iy = (int)floor(v);
    if ((unsigned)ix >= (unsigned)G.nx || (unsigned)iy >= (unsigned)G.ny) return (int8_t)PWPP_FUSE_UNKNOWN;  // (cannot happen: 0 <= floor(u) <= u < nx)
    return image[(size_t)iy * (size_t)G.nx + (size_t)ix];
}

// ---- the observation from the four bytes: +1 occupied, -1 free, 0 none
PWPP_HD inline int pwpp_fuse_observation(int8_t s00, int8_t s10, int8_t s01, int8_t s11) {
    if (s00 == PWPP_FUSE_OCCUPIED || s10 == PWPP_FUSE_OCCUPIED || s01 == PWPP_FUSE_OCCUPIED || s11 == PWPP_FUSE_OCCUPIED) return 1;
    if (s00 == PWPP_FUSE_FREE && s10 == PWPP_FUSE_FREE && s01 == PWPP_FUSE_FREE && s11 == PWPP_FUSE_FREE) return -1;
    return 0;
}

// the observation of the cell whose sample positions are (mx[qx], my[qy]) in one frame
template <bool RECIP>
PWPP_HD inline int pwpp_fuse_observe(const PwppFusionGeometry &G, const double *pose, const double mx[2], const double my[2], const int8_t *image) {
    const int8_t s00 = pwpp_fuse_sample<RECIP>(G, pose, mx[0], my[0], image), s10 = pwpp_fuse_sample<RECIP>(G, pose, mx[1], my[0], image);
    const int8_t s01 = pwpp_fuse_sample<RECIP>(G, pose, mx[0], my[1], image), s11 = pwpp_fuse_sample<RECIP>(G, pose, mx[1], my[1], image);
    return pwpp_fuse_observation(s00, s10, s01, s11);
}

// ---- the update
PWPP_HD inline int32_t pwpp_fuse_update(int32_t L, int observation, const PwppFusionParams &P) {
    if (observation > 0) {
        const int32_t s = L + P.hit;
        return s < P.l_max ? s : P.l_max;
    }
    if (observation < 0) {
        const int32_t s = L - P.miss;
        return s > P.l_min ? s : P.l_min;
    }
    return L;
}

// ---- the derived byte
PWPP_HD inline int8_t pwpp_fuse_byte(int32_t L, const PwppFusionParams &P) {
    return L >= P.occupied_at ? (int8_t)PWPP_FUSE_OCCUPIED : (L <= P.free_at ? (int8_t)PWPP_FUSE_FREE : (int8_t)PWPP_FUSE_UNKNOWN);
}

// ---- one map cell from its start to its end: the frames list[first .. last) of the cell's map in that order; `frames`: the number
// of frame images, every entry of the list is compared with it; `n_poses`: 1 (poses[0 .. 6) for every frame) or frames.
template <bool RECIP>
PWPP_HD inline int32_t pwpp_fuse_cell(const PwppFusionGeometry &G, const PwppFusionParams &P, int32_t L, int jx, int jy, const int8_t *occupancy,
                                      int32_t frames, const double *poses, int32_t n_poses, const int32_t *list, int32_t first, int32_t last) {
    const double mx[2] = {pwpp_fuse_position(G.X0, jx, 0, G.CELL), pwpp_fuse_position(G.X0, jx, 1, G.CELL)};
    const double my[2] = {pwpp_fuse_position(G.Y0, jy, 0, G.CELL), pwpp_fuse_position(G.Y0, jy, 1, G.CELL)};
    const size_t per_frame = (size_t)G.nx * (size_t)G.ny;
    for (int32_t i = first; i < last; ++i) {
        const int32_t f = list[i];
        if ((uint32_t)f >= (uint32_t)frames) continue;  // (the host never lists one)
        const double *pose = poses + (n_poses == 1 ? (size_t)0 : (size_t)f * 6);
        L = pwpp_fuse_update(L, pwpp_fuse_observe<RECIP>(G, pose, mx, my, occupancy + (size_t)f * per_frame), P);
    }
    return L;
}

#endif
