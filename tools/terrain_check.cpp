// terrain_check.cpp -- the arithmetic of the terrain analysis (csrc/pwpp_terrain.h, the one text the gfx950 kernel k_terrain is
// compiled from) run on the host, dealt as the kernel deals it -- a tile of 32 x 8 cells with its clipped halo quantised into a
// buffer, then per cell either the whole window (path 1) or the rows' sums first and 2r+1 rows combined (path 2) -- against a
// brute force of its own that works per cell on the image in __int128, and the contract's formulas written out again.
//   1  random images with holes and limit heights, every radius, ragged tiles, several frames: both paths give the brute force's
//      k, zmin, zmax, D, A, B, N exactly and the same bits of step, slope, rough and cost as the formulas written here in double;
//      a long double evaluation agrees to a float's rounding; N >= 0 in every case
//   2  the stated bounds at the extremes: every r, full and partial windows of +-2^20 in the sign patterns that maximise |Cxz|,
//      |A| and Czz, and random ones: Cxx, Cyy <= 43740, D < 2^31, Czz < 2^53, |Cxz|, |Cyz| < 2^35, |A|, |B| < 2^51, 0 <= N < 2^85,
//      and the header's int32 / int64 sums equal the 128-bit ones
//   3  adding one integer constant to every z leaves D, A, B, N unchanged
// Last line: "terrain_check: <cases> cases, <m> mismatches, <p> failed proof steps"; exit status 0 iff both are 0.
//   terrain_check dump in.f32 nx ny frames r min_known cell step_max slope_max rough_max path prefix
// instead writes the five images the header's functions give for a raw float32 image to prefix.step, .slope, .rough, .count, .cost.
//   g++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -I patchwork-plusplus_amd/csrc tools/terrain_check.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "pwpp_terrain.h"

namespace {

typedef __int128 i128;
long long cases = 0, mismatches = 0, proofs_failed = 0;

void mismatch(const char *what, int r, int path, int ix, int iy, int f) {
    if (++mismatches <= 10) std::printf("MISMATCH %s: r %d path %d cell (%d, %d) frame %d\n", what, r, path, ix, iy, f);
}
void proof(bool ok, const char *what, int r) {
    if (!ok && ++proofs_failed <= 10) std::printf("PROOF FAILED %s: r %d\n", what, r);
}

struct Images {
    std::vector<uint32_t> step, slope, rough;
    std::vector<uint8_t> count;
    std::vector<int8_t> cost;
    std::vector<PwppTerrainMoments> moments;
    explicit Images(size_t n) : step(n), slope(n), rough(n), count(n), cost(n), moments(n) {}
};

// ---- the header's functions, dealt as k_terrain deals them
void by_header(const float *height, int nx, int ny, int frames, const PwppTerrainRule &R, int path, Images &out) {
    const int r = R.radius, TX = PWPP_TERRAIN_TILE_X, TY = PWPP_TERRAIN_TILE_Y, W = TX + 2 * r, H = TY + 2 * r;
    std::vector<int32_t> tile((size_t)W * H);
    std::vector<PwppTerrainRow> rows((size_t)H * TX);
    for (int f = 0; f < frames; ++f)
        for (int y0 = 0; y0 < ny; y0 += TY)
            for (int x0 = 0; x0 < nx; x0 += TX) {
                const size_t base = (size_t)f * nx * ny;
                for (int i = 0; i < W * H; ++i) {
                    const int ly = i / W, lx = i - ly * W, gx = x0 + lx - r, gy = y0 + ly - r;
                    tile[i] = gx >= 0 && gx < nx && gy >= 0 && gy < ny ? pwpp_terrain_quantise(height[base + (size_t)gy * nx + gx]) : PWPP_TERRAIN_UNKNOWN;
                }
                if (path == 2)
                    for (int e = 0; e < H * TX; ++e) {
                        const int row = e / TX, col = e - row * TX;
                        PwppTerrainRow w;
                        pwpp_terrain_row_clear(w);
                        for (int dx = -r; dx <= r; ++dx) {
                            const int32_t z = tile[row * W + col + r + dx];
                            if (z != PWPP_TERRAIN_UNKNOWN) pwpp_terrain_row_add(w, dx, z);
                        }
                        // (through the packed word, as the kernel keeps it)
                        PwppTerrainRow kept = w;
                        pwpp_terrain_row_unpack(pwpp_terrain_row_pack(w), kept);
                        rows[e] = kept;
                    }
                for (int ty = 0; ty < TY && y0 + ty < ny; ++ty)
                    for (int tx = 0; tx < TX && x0 + tx < nx; ++tx) {
                        PwppTerrainMoments M;
                        pwpp_terrain_clear(M);
                        for (int dy = -r; dy <= r; ++dy) {
                            if (path == 2) {
                                pwpp_terrain_add_row(M, dy, rows[(ty + r + dy) * TX + tx]);
                                continue;
                            }
                            for (int dx = -r; dx <= r; ++dx) {
                                const int32_t z = tile[(ty + r + dy) * W + tx + r + dx];
                                if (z != PWPP_TERRAIN_UNKNOWN) pwpp_terrain_add(M, dx, dy, z);
                            }
                        }
                        const size_t at = base + (size_t)(y0 + ty) * nx + (x0 + tx);
                        int32_t c;
                        pwpp_terrain_cell(R, M, tile[(ty + r) * W + tx + r] != PWPP_TERRAIN_UNKNOWN, out.step[at], out.slope[at], out.rough[at], c);
                        out.count[at] = (uint8_t)M.k, out.cost[at] = (int8_t)c, out.moments[at] = M;
                    }
            }
}

// ---- a brute force of its own: 128-bit sums per cell, straight from the image
struct Brute {
    i128 k = 0, Sx = 0, Sy = 0, Sz = 0, Sxx = 0, Sxy = 0, Syy = 0, Sxz = 0, Syz = 0, Szz = 0, zmin = 0, zmax = 0;
    i128 Cxx, Cxy, Cyy, Cxz, Cyz, Czz, D, A, B, N;
    void add(int dx, int dy, long long z) {
        zmin = k == 0 || z < zmin ? (i128)z : zmin, zmax = k == 0 || z > zmax ? (i128)z : zmax;
        k += 1, Sx += dx, Sy += dy, Sz += z, Sxx += dx * dx, Sxy += dx * dy, Syy += dy * dy, Sxz += (i128)dx * z, Syz += (i128)dy * z, Szz += (i128)z * z;
    }
    void solve() {
        Cxx = k * Sxx - Sx * Sx, Cxy = k * Sxy - Sx * Sy, Cyy = k * Syy - Sy * Sy;
        Cxz = k * Sxz - Sx * Sz, Cyz = k * Syz - Sy * Sz, Czz = k * Szz - Sz * Sz;
        D = Cxx * Cyy - Cxy * Cxy, A = Cxz * Cyy - Cyz * Cxy, B = Cyz * Cxx - Cxz * Cxy;
        N = D * Czz - A * Cxz - B * Cyz;
    }
};
i128 iabs(i128 v) { return v < 0 ? -v : v; }
const i128 kOne = 1;

// the stated bounds of one solved window
void bounds(const Brute &b, int r) {
    proof(b.Cxx >= 0 && b.Cxx <= 43740 && b.Cyy >= 0 && b.Cyy <= 43740, "Cxx, Cyy <= 43740", r);
    proof(b.D >= 0 && b.D < (kOne << 31), "0 <= D < 2^31", r);
    proof(b.Czz >= 0 && b.Czz < (kOne << 53), "0 <= Czz < 2^53", r);
    proof(iabs(b.Cxz) < (kOne << 35) && iabs(b.Cyz) < (kOne << 35), "|Cxz|, |Cyz| < 2^35", r);
    proof(iabs(b.A) < (kOne << 51) && iabs(b.B) < (kOne << 51), "|A|, |B| < 2^51", r);
    proof(b.N >= 0, "N >= 0", r);
    proof(b.N < (kOne << 85), "N < 2^85", r);
}

bool same_integers(const PwppTerrainMoments &M, const Brute &b) {
    PwppTerrainPlane P;
    pwpp_terrain_plane(M, P);
    const bool sums = M.k == b.k && M.Sx == b.Sx && M.Sy == b.Sy && M.Sxx == b.Sxx && M.Sxy == b.Sxy && M.Syy == b.Syy && M.Sz == b.Sz && M.Sxz == b.Sxz &&
                      M.Syz == b.Syz && M.Szz == b.Szz && (b.k == 0 || (M.zmin == b.zmin && M.zmax == b.zmax));
    return sums && P.D == b.D && P.A == b.A && P.B == b.B && P.N == b.N;
}

uint32_t bits_of(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

// 1: images
void check_image(int nx, int ny, int frames, int r, double cell, int min_known, float step_max, float slope_max, float rough_max, double holes,
                 unsigned seed) {
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const float beyond = std::nextafter(1024.0f, INFINITY);
    const float special[] = {1024.0f, -1024.0f, beyond, -beyond, INFINITY, -INFINITY, -0.0f, 0.5f / 1024, 1.5f / 1024, -2.5f / 1024, 1023.9f, -1023.9f};
    const size_t cells = (size_t)nx * ny * frames;
    std::vector<float> h(cells);
    for (size_t i = 0; i < cells; ++i) {
        const int ix = (int)(i % nx), iy = (int)(i / nx % ny);
        const double u = U(rng);
        h[i] = (float)(0.3 * std::sin(0.4 * ix) + 0.05 * iy + 0.03 * (U(rng) - 0.5));
        if (u < 0.1) h[i] = special[rng() % 12];
        if (U(rng) < holes) h[i] = NAN;
    }
    const PwppTerrainRule R{r, min_known, step_max, slope_max, rough_max, 1024.0 * cell};
    Images one(cells), two(cells);
    by_header(h.data(), nx, ny, frames, R, 1, one);
    by_header(h.data(), nx, ny, frames, R, 2, two);
    for (int f = 0; f < frames; ++f)
        for (int iy = 0; iy < ny; ++iy)
            for (int ix = 0; ix < nx; ++ix) {
                ++cases;
                const size_t base = (size_t)f * nx * ny, at = base + (size_t)iy * nx + ix;
                Brute b;
                for (int dy = -r; dy <= r; ++dy)
                    for (int dx = -r; dx <= r; ++dx) {
                        const int gx = ix + dx, gy = iy + dy;
                        if (gx < 0 || gx >= nx || gy < 0 || gy >= ny) continue;
                        const double Z = (double)h[base + (size_t)gy * nx + gx];
                        if (!std::isfinite(Z) || std::fabs(Z) > 1024.0) continue;
                        b.add(dx, dy, std::llrint(Z * 1024.0));
                    }
                b.solve();
                bounds(b, r);
                const double centre = (double)h[at];
                const bool known = std::isfinite(centre) && std::fabs(centre) <= 1024.0;
                // the contract written out again
                uint32_t step = PWPP_TERRAIN_NAN, slope = PWPP_TERRAIN_NAN, rough = PWPP_TERRAIN_NAN;
                int cost = -1;
                if (known) {
                    const float s = (float)((double)(long long)(b.zmax - b.zmin) / 1024.0);
                    step = bits_of(s);
                    if (b.D != 0) {
                        const double A = (double)(long long)b.A, B = (double)(long long)b.B, D = (double)(long long)b.D, k = (double)(long long)b.k;
                        const float g = (float)(std::sqrt(A * A + B * B) / (D * (1024.0 * cell)));
                        const float q = (float)(std::sqrt((double)b.N / (D * (k * k))) / 1024.0);  // (the compiler's i128 -> double rounds to nearest even)
                        slope = bits_of(g), rough = bits_of(q);
                        if (b.k >= min_known) {
                            double t = 0.0;
                            const float v[3] = {s, g, q}, lim[3] = {step_max, slope_max, rough_max};
                            for (int i = 0; i < 3; ++i)
                                if (!std::isinf(lim[i])) t = std::fmax(t, (double)v[i] / (double)lim[i]);
                            cost = t >= 1.0 ? 100 : (int)std::floor(t * 100.0);
                        }
                        // a long double evaluation agrees to a float's rounding
                        const long double Al = (long double)b.A, Bl = (long double)b.B, Dl = (long double)b.D;
                        const long double gl = sqrtl(Al * Al + Bl * Bl) / (Dl * 1024.0L * (long double)cell);
                        const long double ql = sqrtl((long double)b.N / (Dl * (long double)(b.k * b.k))) / 1024.0L;
                        if (std::isfinite(g) && fabsl((long double)g - gl) > ldexpl(fabsl(gl), -23) + 1e-45L) mismatch("slope against long double", r, 0, ix, iy, f);
                        if (fabsl((long double)q - ql) > ldexpl(fabsl(ql), -23) + 1e-45L) mismatch("rough against long double", r, 0, ix, iy, f);
                    }
                }
                const Images *both[2] = {&one, &two};
                for (int p = 0; p < 2; ++p) {
                    const Images &o = *both[p];
                    if (!same_integers(o.moments[at], b)) mismatch("integers", r, p + 1, ix, iy, f);
                    if (o.count[at] != (uint8_t)b.k) mismatch("count", r, p + 1, ix, iy, f);
                    if (o.step[at] != step) mismatch("step", r, p + 1, ix, iy, f);
                    if (o.slope[at] != slope) mismatch("slope", r, p + 1, ix, iy, f);
                    if (o.rough[at] != rough) mismatch("rough", r, p + 1, ix, iy, f);
                    if (o.cost[at] != (int8_t)cost) mismatch("cost", r, p + 1, ix, iy, f);
                }
            }
}

// 2 and 3: windows given cell by cell (PWPP_TERRAIN_UNKNOWN: none), through the header's sums and the 128-bit ones
struct Extremes {
    i128 Cxz = 0, A = 0, Czz = 0, N = 0, D = 0;
} seen[PWPP_TERRAIN_MAX_R + 1];

void check_window(int r, const std::vector<int32_t> &z /* (2r+1)^2, row-major */, long long shift = 0) {
    ++cases;
    const int w = 2 * r + 1;
    PwppTerrainMoments M, Ms;
    pwpp_terrain_clear(M), pwpp_terrain_clear(Ms);
    Brute b;
    for (int dy = -r; dy <= r; ++dy) {
        PwppTerrainRow row;
        pwpp_terrain_row_clear(row);
        for (int dx = -r; dx <= r; ++dx) {
            const int32_t v = z[(size_t)(dy + r) * w + (dx + r)];
            if (v == PWPP_TERRAIN_UNKNOWN) continue;
            pwpp_terrain_add(M, dx, dy, v), pwpp_terrain_row_add(row, dx, v), b.add(dx, dy, v);
        }
        pwpp_terrain_add_row(Ms, dy, row);
    }
    b.solve();
    bounds(b, r);
    if (!same_integers(M, b)) mismatch("window integers", r, 1, 0, 0, 0);
    if (!same_integers(Ms, b)) mismatch("window integers", r, 2, 0, 0, 0);
    Extremes &e = seen[r];
    e.Cxz = iabs(b.Cxz) > e.Cxz ? iabs(b.Cxz) : e.Cxz, e.Cxz = iabs(b.Cyz) > e.Cxz ? iabs(b.Cyz) : e.Cxz;
    e.A = iabs(b.A) > e.A ? iabs(b.A) : e.A, e.A = iabs(b.B) > e.A ? iabs(b.B) : e.A;
    e.Czz = b.Czz > e.Czz ? b.Czz : e.Czz, e.N = b.N > e.N ? b.N : e.N, e.D = b.D > e.D ? b.D : e.D;
    if (shift != 0) {  // 3: the same window, every z moved by one constant
        PwppTerrainMoments Mc;
        pwpp_terrain_clear(Mc);
        for (int dy = -r; dy <= r; ++dy)
            for (int dx = -r; dx <= r; ++dx) {
                const int32_t v = z[(size_t)(dy + r) * w + (dx + r)];
                if (v != PWPP_TERRAIN_UNKNOWN) pwpp_terrain_add(Mc, dx, dy, (int32_t)(v + shift));
            }
        PwppTerrainPlane P, Pc;
        pwpp_terrain_plane(M, P), pwpp_terrain_plane(Mc, Pc);
        proof(P.D == Pc.D && P.A == Pc.A && P.B == Pc.B && P.N == Pc.N, "a constant added to every z changes D, A, B or N", r);
    }
}

void check_extremes(int r) {
    const int w = 2 * r + 1, n = w * w, Mx = PWPP_ELEV_M;
    std::vector<int32_t> z((size_t)n);
    const auto at = [&](int dx, int dy) -> int32_t & { return z[(size_t)(dy + r) * w + (dx + r)]; };
    const auto sgn = [](int v) { return v > 0 ? 1 : (v < 0 ? -1 : 0); };
    // the sign patterns: by dx, by dy, by dx + dy, by dx - dy (|Cxz|, |Cyz|, |A|, |B|), with the middle line at either sign;
    // halves, a checkerboard and one cell against the rest (Czz)
    for (int pattern = 0; pattern < 10; ++pattern)
        for (int middle = -1; middle <= 1; middle += 2) {
            for (int dy = -r; dy <= r; ++dy)
                for (int dx = -r; dx <= r; ++dx) {
                    int s = 0;
                    switch (pattern) {
                    case 0: s = sgn(dx); break;
                    case 1: s = sgn(dy); break;
                    case 2: s = sgn(dx + dy); break;
                    case 3: s = sgn(dx - dy); break;
                    case 4: s = sgn(2 * dx + dy); break;
                    case 5: s = sgn(dx + 2 * dy); break;
                    case 6: s = ((dx + dy) & 1) ? 1 : -1; break;
                    case 7: s = dx == 0 && dy == 0 ? 1 : -1; break;
                    case 8: s = sgn(dx) * sgn(dy); break;
                    default: s = (dy * w + dx + n) % 2 ? 1 : -1; break;
                    }
                    at(dx, dy) = (s == 0 ? middle : s) * Mx;
                }
            check_window(r, z);
            for (int32_t &v : z) v = -v;
            check_window(r, z);
        }
    // random +-2^20 windows, full and with holes; random small windows with a constant added
    std::mt19937_64 rng(1234u + (unsigned)r);
    for (int it = 0; it < 20000; ++it) {
        const bool holes = it % 2 == 1;
        for (int32_t &v : z) v = holes && rng() % 4 == 0 ? PWPP_TERRAIN_UNKNOWN : (rng() % 2 ? Mx : -Mx);
        check_window(r, z);
    }
    for (int it = 0; it < 20000; ++it) {
        for (int32_t &v : z) v = rng() % 5 == 0 ? PWPP_TERRAIN_UNKNOWN : (int32_t)(rng() % (Mx + 1)) - Mx / 2;
        check_window(r, z, (long long)(rng() % (Mx + 1)) - Mx / 2);
    }
}

void print128(const char *name, i128 v) {
    std::printf("  %s %.6g (2^%.2f)", name, (double)v, v > 0 ? std::log2((double)v) : 0.0);
}

int dump(char **a) {
    const int nx = std::atoi(a[1]), ny = std::atoi(a[2]), frames = std::atoi(a[3]), r = std::atoi(a[4]), min_known = std::atoi(a[5]);
    const double cell = std::strtod(a[6], nullptr);
    const float lim[3] = {(float)std::strtod(a[7], nullptr), (float)std::strtod(a[8], nullptr), (float)std::strtod(a[9], nullptr)};
    const int path = std::atoi(a[10]);
    if (nx < 1 || ny < 1 || frames < 1 || r < 1 || r > PWPP_TERRAIN_MAX_R || (path != 1 && path != 2)) return 2;
    const size_t cells = (size_t)nx * ny * frames;
    std::vector<float> h(cells);
    FILE *in = std::fopen(a[0], "rb");
    if (!in || std::fread(h.data(), 4, cells, in) != cells) return 2;
    std::fclose(in);
    Images out(cells);
    by_header(h.data(), nx, ny, frames, PwppTerrainRule{r, min_known, lim[0], lim[1], lim[2], 1024.0 * cell}, path, out);
    const struct {
        const char *ext;
        const void *p;
        size_t bytes;
    } files[5] = {{".step", out.step.data(), cells * 4}, {".slope", out.slope.data(), cells * 4}, {".rough", out.rough.data(), cells * 4},
                  {".count", out.count.data(), cells},   {".cost", out.cost.data(), cells}};
    for (const auto &f : files) {
        FILE *o = std::fopen((std::string(a[11]) + f.ext).c_str(), "wb");
        if (!o || std::fwrite(f.p, 1, f.bytes, o) != f.bytes) return 2;
        std::fclose(o);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 14 && std::strcmp(argv[1], "dump") == 0) return dump(argv + 2);
    unsigned seed = 1;
    for (int r = 1; r <= PWPP_TERRAIN_MAX_R; ++r) {
        // ragged tiles, several frames, holes of 0, 30 and 90 per cent, finite and infinite limits, min_known at its ends
        check_image(70, 19, 2, r, 0.5, 3, 0.2f, 0.3f, 0.05f, 0.3, seed++);
        check_image(33, 9, 1, r, 0.3, 1, INFINITY, 0.5f, INFINITY, 0.0, seed++);
        check_image(31, 17, 1, r, 0.125, (2 * r + 1) * (2 * r + 1), 1.0f, INFINITY, 0.01f, 0.9, seed++);
        check_image(1, 9, 1, r, 0.5, 1, INFINITY, INFINITY, INFINITY, 0.1, seed++);
        check_image(9, 1, 1, r, 0.5, 1, INFINITY, INFINITY, INFINITY, 0.1, seed++);
        check_image(1, 1, 3, r, 0.5, 1, 1.0f, 1.0f, 1.0f, 0.3, seed++);
        check_extremes(r);
        std::printf("r %d: the largest seen:", r);
        print128("|Cxz|", seen[r].Cxz), print128("|A|", seen[r].A), print128("Czz", seen[r].Czz), print128("D", seen[r].D), print128("N", seen[r].N);
        std::printf("\n");
    }
    std::printf("terrain_check: %lld cases, %lld mismatches, %lld failed proof steps\n", cases, mismatches, proofs_failed);
    return mismatches == 0 && proofs_failed == 0 ? 0 : 1;
}
