// pwpp_clusters.hip -- gfx950 (MI355X) kernels of the obstacle clusters: connected-component labelling of an occupancy image
// (pwpp_label_grid, pwpp_label_obstacles; include/pwpp.h has the rules).  Pure image operations on the handle's stream: nothing of
// the estimate pipeline is read or written.  The per-point scatter (k_point_cluster) sits beside k_obstacle_raster in
// pwpp_kernels.hip, because it needs load_point and ground_sample.
//
// Per frame the label image is a union-find forest over the occupied cells (pwpp_unionfind.h: a word is the FRAME-LOCAL linear
// index iy * nx + ix of the cell's parent, never a larger one; -1 = unoccupied).  Five steps, each a launch of its own:
//   1  k_cl_tile     a workgroup per tile of 64 x 16 cells: occupancy into LDS, union-find inside the tile on LDS words, every
//                    cell's tile root out as a frame-local index, plain stores (option "clusters_path" = 1 instead:
//                    k_cl_init writes every occupied cell as its own root)
//   2  k_cl_border   only the cells on a tile's edges: unions across the edges, in the global image
//                    ("clusters_path" = 1: k_cl_merge, every cell with all its neighbours)
//   3  k_cl_compress every word becomes its root; a cell that is its own root is a cluster: roots counted per CHUNK of 256
//                    consecutive cells of the frame in row-major order, every root's rank inside its chunk kept in a working image
//      k_cl_scan     one workgroup per frame: exclusive scan of the chunk counts, n_clusters
//   4  k_cl_relabel  label = scanned count of the root's chunk + the root's rank inside it; the table rows accumulated
//      k_cl_rows / k_cl_tops  the rows' initial values before, their key-form tops as floats after
// RANKS.  The rank of a cluster is the number of roots with a smaller cell index, and a root IS its cluster's first_cell.  Tiles are
// not intervals of the row-major order (a tile's second row lies behind the first row of the tile to its right), so roots are NOT
// counted per tile: the counting unit is a chunk of PWPP_CL_CHUNK consecutive cells, which is an interval of that order -- the
// scan over chunks plus the position inside the chunk is the rank, with no sort.
//
// VISIBILITY (steps 2 and 3).  Workgroups of one launch read and write the same label words, they run on eight XCDs with private
// L2s, and a CU's L1 is never refreshed by another CU's stores.  So inside these kernels EVERY read of a label word is an
// agent-scope relaxed atomic load and EVERY write an agent-scope atomic minimum; there is no plain load or store of a label word
// in them (GlobalWords below is their only door to the image).  Relaxed is enough, and no fence is needed, because nothing is
// handed over THROUGH a label word: pwpp_unionfind.h's argument needs only that a word is read and written whole and that its
// values decrease -- labels only decrease and never leave their component, so a stale or racing read costs a longer chase or a
// retry, never a wrong merge; and the root of a finished component is its smallest cell.  Plain stores (steps 1, 4) and plain
// loads (step 4) touch label words only in launches where no other workgroup touches the same word, and the launch boundary on
// the stream orders them against the atomic steps.
//
// The ROW kernels of the obstacle boxes (pwpp_box_obstacles) live here too, at the end: k_box_init / k_box_solve / k_box_finish, one
// lane per accumulator word or per row, around the two point passes of pwpp_kernels.hip.  pwpp_boxes.h has their arithmetic.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "pwpp_boxes.h"
#include "pwpp_dev.h"  // the launchers' prototypes
#include "pwpp_unionfind.h"
#include "pwpp_wave.h"

namespace {

constexpr int kClBlock = 256;
constexpr int kTileCells = PWPP_CL_TILE_X * PWPP_CL_TILE_Y;  // 1024 LDS words
constexpr int kBorderBlock = 128;                            // 64 north + 16 west + 16 east edge cells of a tile, one lane each

// the label words of one frame in global memory: the ONLY access path of the kernels that share them inside a launch
struct GlobalWords {
    int32_t *w;
    __device__ __forceinline__ int32_t load(int32_t i) { return __hip_atomic_load(w + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int32_t fetch_min(int32_t i, int32_t v) {
        return __hip_atomic_fetch_min(w + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// the words of a tile in LDS (tile-local index: row * 64 + column, which orders the cells of a tile as the frame does)
struct TileWords {
    int32_t *w;
    __device__ __forceinline__ int32_t load(int32_t i) { return __hip_atomic_load(w + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ int32_t fetch_min(int32_t i, int32_t v) {
        return __hip_atomic_fetch_min(w + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};

struct ClImage {
    int32_t nx, ny;
    int32_t per_frame;  // nx * ny  (<= 2^31 - 1)
    int32_t tiles_x, tiles_y;
    int32_t chunks;     // ceil(per_frame / PWPP_CL_CHUNK)
    int32_t min_count, connectivity;
};

// 1: grid (tiles_x * tiles_y * frames), 4 waves.  Lane = column, wave w takes the rows w, w + 4, w + 8, w + 12 of the tile: a
// wave reads 256 contiguous bytes of a count row and writes 256 of a label row, one dword per lane -- the same request for every
// alignment of the image, so there is no second path for rows that are not 16-byte aligned.
__global__ __launch_bounds__(kClBlock) void k_cl_tile(ClImage I, const int32_t *count, int32_t *label) {
    __shared__ int32_t s_par[kTileCells];
    const unsigned b = blockIdx.x, tpf = (unsigned)I.tiles_x * (unsigned)I.tiles_y;
    const unsigned f = b / tpf, t = b - f * tpf;
    const int ty0 = (int)(t / (unsigned)I.tiles_x) * PWPP_CL_TILE_Y, tx0 = (int)(t % (unsigned)I.tiles_x) * PWPP_CL_TILE_X;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t fbase = (size_t)f * (size_t)I.per_frame;
    const int x = tx0 + lane;
#pragma unroll
    for (int k = 0; k < PWPP_CL_TILE_Y / 4; ++k) {
        const int r = w + 4 * k, y = ty0 + r;
        const bool occ = x < I.nx && y < I.ny && count[fbase + (size_t)y * (size_t)I.nx + (size_t)x] >= I.min_count;
        s_par[r * PWPP_CL_TILE_X + lane] = occ ? r * PWPP_CL_TILE_X + lane : -1;
    }
    __syncthreads();
    TileWords m{s_par};
#pragma unroll
    for (int k = 0; k < PWPP_CL_TILE_Y / 4; ++k) {
        const int r = w + 4 * k, c = r * PWPP_CL_TILE_X + lane;
        if (m.load(c) < 0) continue;
        for (int j = 0; j < 4; ++j) {
            int qx, qy;
            if (!uf_neighbour(j, I.connectivity, lane, r, PWPP_CL_TILE_X, qx, qy)) continue;
            const int q = qy * PWPP_CL_TILE_X + qx;
            if (m.load(q) >= 0) uf_union(m, c, q, kTileCells);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PWPP_CL_TILE_Y / 4; ++k) {
        const int r = w + 4 * k, y = ty0 + r, c = r * PWPP_CL_TILE_X + lane;
        if (x >= I.nx || y >= I.ny) continue;
        int32_t out = -1;
        if (m.load(c) >= 0) {
            const int root = uf_find(m, c, kTileCells);  // (nobody writes any more: the chase reads a finished forest)
            out = (ty0 + (root >> 6)) * I.nx + tx0 + (root & 63);
        }
        label[fbase + (size_t)y * (size_t)I.nx + (size_t)x] = out;
    }
}

// 2: grid (tiles * frames), one lane per edge cell of the tile.  Lane 0..63: the cells of the tile's first row look at N (and NW,
// NE); 64..79: the first column at W (and NW, except in the first row, which has looked already); 80..95 (8-connectivity): the
// last column, from the second row on, at NE.  These are exactly the pairs of uf_neighbour whose two cells lie in different tiles.
__global__ __launch_bounds__(kBorderBlock) void k_cl_border(ClImage I, int32_t *label) {
    const unsigned b = blockIdx.x, tpf = (unsigned)I.tiles_x * (unsigned)I.tiles_y;
    const unsigned f = b / tpf, t = b - f * tpf;
    const int ty0 = (int)(t / (unsigned)I.tiles_x) * PWPP_CL_TILE_Y, tx0 = (int)(t % (unsigned)I.tiles_x) * PWPP_CL_TILE_X;
    const int l = threadIdx.x;
    int x, y;
    unsigned looks;  // bit k: neighbour k of uf_neighbour (0 W, 1 N, 2 NW, 3 NE)
    if (l < 64) {
        x = tx0 + l, y = ty0, looks = 2u | 4u | 8u;
    } else if (l < 80) {
        x = tx0, y = ty0 + (l - 64), looks = 1u | (l > 64 ? 4u : 0u);
    } else if (l < 96) {
        x = tx0 + PWPP_CL_TILE_X - 1, y = ty0 + (l - 80), looks = l > 80 ? 8u : 0u;
    } else {
        return;
    }
    if (x >= I.nx || y >= I.ny) return;
    GlobalWords m{label + (size_t)f * (size_t)I.per_frame};
    const int32_t c = y * I.nx + x;
    if (m.load(c) < 0) return;
    for (int k = 0; k < 4; ++k) {
        int qx, qy;
        if (!((looks >> k) & 1u) || !uf_neighbour(k, I.connectivity, x, y, I.nx, qx, qy)) continue;
        const int32_t q = qy * I.nx + qx;
        if (m.load(q) >= 0) uf_union(m, c, q, I.per_frame);
    }
}

// "clusters_path" = 1, the yardstick: no tiles, no LDS.  Every occupied cell its own root ...
__global__ __launch_bounds__(kClBlock) void k_cl_init(ClImage I, int64_t cells, const int32_t *count, int32_t *label) {
    const int64_t i = (int64_t)blockIdx.x * kClBlock + threadIdx.x;
    if (i >= cells) return;
    label[i] = count[i] >= I.min_count ? (int32_t)(i % I.per_frame) : -1;
}
// ... and every cell with all its neighbours, under the same atomic-only rule.  Grid (chunks * frames).
__global__ __launch_bounds__(kClBlock) void k_cl_merge(ClImage I, int32_t *label) {
    const unsigned f = blockIdx.x / (unsigned)I.chunks, ch = blockIdx.x % (unsigned)I.chunks;
    const int64_t c64 = (int64_t)ch * PWPP_CL_CHUNK + threadIdx.x;
    if (c64 >= I.per_frame) return;
    const int32_t c = (int32_t)c64;
    GlobalWords m{label + (size_t)f * (size_t)I.per_frame};
    if (m.load(c) < 0) return;
    const int y = c / I.nx, x = c - y * I.nx;
    for (int k = 0; k < 4; ++k) {
        int qx, qy;
        if (!uf_neighbour(k, I.connectivity, x, y, I.nx, qx, qy)) continue;
        const int32_t q = qy * I.nx + qx;
        if (m.load(q) >= 0) uf_union(m, c, q, I.per_frame);
    }
}

// 3: grid (chunks * frames), one lane per cell of the chunk.  Other workgroups compress the words this one chases through: the
// atomic-only rule again.  rank_in[cell] (a root's number of roots before it in its chunk) and chunk_count are this launch's own.
__global__ __launch_bounds__(kClBlock) void k_cl_compress(ClImage I, int32_t *label, int32_t *rank_in, int32_t *chunk_count) {
    __shared__ unsigned s_wave[kClBlock / 64][1];
    const unsigned f = blockIdx.x / (unsigned)I.chunks, ch = blockIdx.x % (unsigned)I.chunks;
    const int64_t c64 = (int64_t)ch * PWPP_CL_CHUNK + threadIdx.x;
    const size_t fbase = (size_t)f * (size_t)I.per_frame;
    GlobalWords m{label + fbase};
    bool root = false;
    if (c64 < I.per_frame) {
        const int32_t c = (int32_t)c64;
        if (m.load(c) >= 0) root = uf_compress(m, c, I.per_frame) == c;
    }
    unsigned before[1] = {root ? 1u : 0u}, total[1];
    block_excl_scan<1, kClBlock / 64>(before, s_wave, total);  // (no thread has returned: every lane of every wave is active, as the DPP scan needs)
    if (root) rank_in[fbase + (size_t)c64] = (int32_t)before[0];
    if (threadIdx.x == 0) chunk_count[(size_t)f * (size_t)I.chunks + ch] = (int32_t)total[0];
}

// one workgroup per frame: chunk_count becomes its exclusive scan, n_clusters[f] the sum
__global__ __launch_bounds__(kClBlock) void k_cl_scan(ClImage I, int32_t *chunk_count, int32_t *n_clusters) {
    __shared__ unsigned s_wave[kClBlock / 64][1];
    __shared__ int s_carry;
    const unsigned f = blockIdx.x;
    int32_t *cc = chunk_count + (size_t)f * (size_t)I.chunks;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < I.chunks; base += kClBlock) {  // (the same trips for every thread: all lanes active at the scan, as its DPP steps need)
        const int64_t i = base + threadIdx.x;
        unsigned before[1] = {i < I.chunks ? (unsigned)cc[i] : 0u}, total[1];  // (counts: >= 0, a frame's sum below 2^31)
        block_excl_scan<1, kClBlock / 64>(before, s_wave, total);
        if (i < I.chunks) cc[i] = s_carry + (int32_t)before[0];
        __syncthreads();
        if (threadIdx.x == 0) s_carry += (int32_t)total[0];  // (read again behind the two barriers of the next trip's scan)
    }
    if (threadIdx.x == 0 && n_clusters) n_clusters[f] = s_carry;
}

// a table row, word by word (pwpp_obstacle_cluster, 48 bytes; the sums 8-byte aligned because `clusters` is)
enum { kRowFirst = 0, kRowCells, kRowPoints, kRowIxMin, kRowIxMax, kRowIyMin, kRowIyMax, kRowTop, kRowSumIx, kRowSumIy = 10, kRowWords = 12 };

// 4a: every row < max_clusters of every frame: minima INT_MAX, maxima -1, sums 0, the top's key 0 (= empty), first_cell -1
__global__ __launch_bounds__(kClBlock) void k_cl_rows(int64_t rows, int32_t *table) {
    const int64_t i = (int64_t)blockIdx.x * kClBlock + threadIdx.x;
    if (i >= rows * kRowWords) return;
    const int k = (int)(i % kRowWords);
    table[i] = k == kRowFirst ? -1 : (k == kRowIxMin || k == kRowIyMin) ? INT_MAX : (k == kRowIxMax || k == kRowIyMax) ? -1 : 0;
}

// 4b: grid (chunks * frames).  Every word is read and written by its own lane only; the roots' words are final since step 3.
// Integer atomics on the rows: sums, minima, maxima and the key maximum are functions of the SET of cells.  Plain atomics: the
// cells of a wave mostly belong to a few clusters, as the points of a wave do in k_obstacle_raster.
__global__ __launch_bounds__(kClBlock) void k_cl_relabel(ClImage I, const int32_t *count, const float *top, int32_t *label, const int32_t *rank_in,
                                                         const int32_t *chunk_excl, int32_t *table, int max_clusters) {
    const unsigned f = blockIdx.x / (unsigned)I.chunks, ch = blockIdx.x % (unsigned)I.chunks;
    const int64_t c64 = (int64_t)ch * PWPP_CL_CHUNK + threadIdx.x;
    if (c64 >= I.per_frame) return;
    const int32_t c = (int32_t)c64;
    const size_t fbase = (size_t)f * (size_t)I.per_frame;
    const int32_t r = label[fbase + c];
    if (r < 0 || r >= I.per_frame) return;  // (unoccupied; a word beyond the frame could only be a defect and forms no address)
    const int32_t rank = chunk_excl[(size_t)f * (size_t)I.chunks + (unsigned)(r / PWPP_CL_CHUNK)] + rank_in[fbase + r];
    label[fbase + c] = rank;
    if (!table || rank < 0 || rank >= max_clusters) return;
    int32_t *row = table + ((size_t)f * (size_t)max_clusters + (size_t)rank) * kRowWords;
    const int y = c / I.nx, x = c - y * I.nx;
    const int32_t n = count[fbase + c];
    if (c == r) row[kRowFirst] = c;
    atomicAdd(row + kRowCells, 1);
    atomicAdd(row + kRowPoints, n);
    atomicMin(row + kRowIxMin, x);
    atomicMax(row + kRowIxMax, x);
    atomicMin(row + kRowIyMin, y);
    atomicMax(row + kRowIyMax, y);
    if (top) atomicMax(reinterpret_cast<uint32_t *>(row + kRowTop), pwpp_height_key(top[fbase + c]));
    atomicAdd(reinterpret_cast<unsigned long long *>(row + kRowSumIx), (unsigned long long)((int64_t)n * x));
    atomicAdd(reinterpret_cast<unsigned long long *>(row + kRowSumIy), (unsigned long long)((int64_t)n * y));
}

// 4c: the rows' tops from keys to floats (key 0, also "no top image": the quiet NaN)
__global__ __launch_bounds__(kClBlock) void k_cl_tops(int64_t rows, int32_t *table) {
    const int64_t i = (int64_t)blockIdx.x * kClBlock + threadIdx.x;
    if (i >= rows) return;
    uint32_t *p = reinterpret_cast<uint32_t *>(table + i * kRowWords + kRowTop);
    *p = __builtin_bit_cast(uint32_t, pwpp_height_of_key(*p));
}

// ---- the row kernels of the obstacle boxes (pwpp_box_obstacles; pwpp_boxes.h has the arithmetic and the accumulators) -----------------
// One lane per accumulator word: the sums 0, the keys empty.
__global__ __launch_bounds__(kClBlock) void k_box_init(int64_t rows, uint32_t *acc) {
    const int64_t i = (int64_t)blockIdx.x * kClBlock + threadIdx.x;
    if (i >= rows * PWPP_BOX_ACC_WORDS) return;
    const int k = (int)(i % PWPP_BOX_ACC_WORDS) - 2 * PWPP_BOX_SUMS;
    acc[i] = k < 0 ? 0u : ((k & 1) ? PWPP_BOX_KEY_NO_MAX : PWPP_BOX_KEY_NO_MIN);
}

// Between the passes, one lane per row: covariance, axis, spread and mean of a row with points into its place in `boxes` (words,
// 4-byte aligned and no more).  A row without points is never read by the second pass.
__global__ __launch_bounds__(kClBlock) void k_box_solve(int64_t rows, const uint32_t *acc, double x0, double y0, uint32_t *boxes) {
    const int64_t i = (int64_t)blockIdx.x * kClBlock + threadIdx.x;
    if (i >= rows) return;
    const long long *s = reinterpret_cast<const long long *>(acc + i * PWPP_BOX_ACC_WORDS);
    if (s[0] <= 0) return;
    const PwppBoxAxis a = pwpp_box_solve(s[0], s[1], s[2], s[3], s[4], s[5], x0, y0);
    float *row = reinterpret_cast<float *>(boxes + i * 16);
    row[2] = a.mean_x, row[3] = a.mean_y, row[6] = a.ax, row[7] = a.ay, row[10] = a.sigma_long, row[11] = a.sigma_short;
}

// Behind the second pass, one lane per row: the sixteen words of the finished row; a row without points: 0, 0 and the quiet NaN.
__global__ __launch_bounds__(kClBlock) void k_box_finish(int64_t rows, const uint32_t *acc, double x0, double y0, uint32_t *boxes) {
    const int64_t i = (int64_t)blockIdx.x * kClBlock + threadIdx.x;
    if (i >= rows) return;
    const uint32_t *w = acc + i * PWPP_BOX_ACC_WORDS;
    const long long n = *reinterpret_cast<const long long *>(w);
    uint32_t *row = boxes + i * 16;
    PwppBoxAxis a = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (n > 0) {
        const float *f = reinterpret_cast<const float *>(row);
        a.mean_x = f[2], a.mean_y = f[3], a.ax = f[6], a.ay = f[7], a.sigma_long = f[10], a.sigma_short = f[11];
    }
    uint32_t out[16];
    pwpp_box_row(n, a, w + 2 * PWPP_BOX_SUMS, x0, y0, out);
#pragma unroll
    for (int k = 0; k < 16; ++k) row[k] = out[k];
}

}  // namespace

// The row steps of pwpp_box_obstacles on `rows` rows.  step 0: the accumulators' initial values; 1: steps 2 to 4 of every row
// between the passes; 2: the finished rows.  acc: PWPP_BOX_ACC_WORDS words per row, 8-byte aligned; boxes: 16 words per row.
extern "C" int pwpp_launch_box_rows(int step, int64_t rows, uint32_t *acc, double x0, double y0, void *boxes, hipStream_t stream) {
    const dim3 per_row((unsigned)((rows + kClBlock - 1) / kClBlock)), per_word((unsigned)((rows * PWPP_BOX_ACC_WORDS + kClBlock - 1) / kClBlock));
    if (step == 0)
        hipLaunchKernelGGL(k_box_init, per_word, dim3(kClBlock), 0, stream, rows, acc);
    else if (step == 1)
        hipLaunchKernelGGL(k_box_solve, per_row, dim3(kClBlock), 0, stream, rows, acc, x0, y0, static_cast<uint32_t *>(boxes));
    else
        hipLaunchKernelGGL(k_box_finish, per_row, dim3(kClBlock), 0, stream, rows, acc, x0, y0, static_cast<uint32_t *>(boxes));
    return (int)hipGetLastError();
}

// Words of the handle's cluster buffer the kernels need for an image of nx * ny * frames cells: the roots' ranks inside their
// chunks (one per cell), then the chunk counts.
extern "C" size_t pwpp_cluster_work_words(int nx, int ny, int frames) {
    const size_t per_frame = (size_t)nx * (size_t)ny, chunks = (per_frame + PWPP_CL_CHUNK - 1) / PWPP_CL_CHUNK;
    return ((per_frame * (size_t)frames + 3) & ~(size_t)3) + chunks * (size_t)frames;
}

// pwpp_label_grid on device memory.  `work`: pwpp_cluster_work_words words.  The caller has checked nx * ny <= 2^31 - 1,
// nx * ny * frames <= 2^31, min_count, connectivity and max_clusters; `clusters` may be null with max_clusters == 0.
extern "C" int pwpp_launch_label_grid(int nx, int ny, int frames, const int32_t *count, const float *top, int min_count, int connectivity, int path,
                                      int32_t *label, void *clusters, int32_t *n_clusters, int max_clusters, uint32_t *work, hipStream_t stream) {
    ClImage I;
    I.nx = nx, I.ny = ny, I.per_frame = nx * ny;
    I.tiles_x = (nx + PWPP_CL_TILE_X - 1) / PWPP_CL_TILE_X, I.tiles_y = (ny + PWPP_CL_TILE_Y - 1) / PWPP_CL_TILE_Y;
    I.chunks = (int32_t)(((int64_t)I.per_frame + PWPP_CL_CHUNK - 1) / PWPP_CL_CHUNK);
    I.min_count = min_count, I.connectivity = connectivity;
    const int64_t cells = (int64_t)I.per_frame * frames;
    int32_t *rank_in = reinterpret_cast<int32_t *>(work);
    int32_t *chunk_count = rank_in + (((size_t)cells + 3) & ~(size_t)3);
    const unsigned tiles = (unsigned)((int64_t)I.tiles_x * I.tiles_y * frames), chunk_blocks = (unsigned)((int64_t)I.chunks * frames);
    if (path == 1) {
        hipLaunchKernelGGL(k_cl_init, dim3((unsigned)((cells + kClBlock - 1) / kClBlock)), dim3(kClBlock), 0, stream, I, cells, count, label);
        hipLaunchKernelGGL(k_cl_merge, dim3(chunk_blocks), dim3(kClBlock), 0, stream, I, label);
    } else {
        hipLaunchKernelGGL(k_cl_tile, dim3(tiles), dim3(kClBlock), 0, stream, I, count, label);
        if (I.tiles_x > 1 || I.tiles_y > 1) hipLaunchKernelGGL(k_cl_border, dim3(tiles), dim3(kBorderBlock), 0, stream, I, label);
    }
    hipLaunchKernelGGL(k_cl_compress, dim3(chunk_blocks), dim3(kClBlock), 0, stream, I, label, rank_in, chunk_count);
    hipLaunchKernelGGL(k_cl_scan, dim3((unsigned)frames), dim3(kClBlock), 0, stream, I, chunk_count, n_clusters);
    int32_t *table = max_clusters > 0 ? static_cast<int32_t *>(clusters) : nullptr;
    const int64_t rows = (int64_t)frames * max_clusters;
    if (table) hipLaunchKernelGGL(k_cl_rows, dim3((unsigned)((rows * kRowWords + kClBlock - 1) / kClBlock)), dim3(kClBlock), 0, stream, rows, table);
    hipLaunchKernelGGL(k_cl_relabel, dim3(chunk_blocks), dim3(kClBlock), 0, stream, I, count, top, label, rank_in, chunk_count, table, max_clusters);
    if (table) hipLaunchKernelGGL(k_cl_tops, dim3((unsigned)((rows + kClBlock - 1) / kClBlock)), dim3(kClBlock), 0, stream, rows, table);
    return (int)hipGetLastError();
}
