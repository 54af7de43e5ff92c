// costmap_check.cpp -- a stand-alone host program: the functions of csrc/pwpp_costmap.h dealt as the kernels of pwpp_costmap.hip deal
// them -- a lane per cell with the curve where the caller left it (path 1); the table copied into whole words with the rest 0, then
// the dealing's items, four cells as one word per byte image where its address is a multiple of 4 and as four bytes where not, the
// head and tail as single cells (path 2); the widening of the occupancy byte four cells a lane -- against the rule of include/pwpp.h
// written out a second time.  Every image of a case sits at its own start offset 0 .. 3 behind an allocation of exactly its size,
// so a read or a write outside it is the sanitizer's finding, and the bytes before the start are checked to be untouched.
//   costmap_check                  the built-in cases; prints "costmap_check: N cases, M mismatches"
//   costmap_check dump LAYERS OCC_UNKNOWN TERRAIN_UNKNOWN UNKNOWN_BELOW CURVE O T D CELLS OUT
//                                  the fold of raw image files (uint8 curve, int8 o and t, int32 d; "-": none) on both paths, which
//                                  must agree, written to OUT.cost (int8) and OUT.why (uint8)
// Built with -fsanitize=address,undefined and run by tests/test_costmap_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "pwpp_costmap.h"

namespace {

// ---- the rule a second time, from the header's words: a list of the known values, their maximum, the bits ------------------------
void rule_again(const PwppCostmapRule &R, const uint8_t *curve, int o, int t, int32_t d, int &cost, unsigned &why) {
    int value[3], bit[3], n = 0;
    bool unknown = false;
    if (R.layers & 1) {
        if (o == 100 || o == 0) value[n] = o, bit[n++] = 1;
        else if (R.occupancy_unknown >= 0) value[n] = R.occupancy_unknown, bit[n++] = 1;
        else unknown = true;
    }
    if (R.layers & 2) {
        const uint64_t index = (uint64_t)(uint32_t)d;
        value[n] = index < (uint64_t)R.n_curve ? curve[index] : 0, bit[n++] = 2;
    }
    if (R.layers & 4) {
        if (t >= 0) value[n] = t > 100 ? 100 : t, bit[n++] = 4;
        else if (R.terrain_unknown >= 0) value[n] = R.terrain_unknown, bit[n++] = 4;
        else unknown = true;
    }
    int m = 0;
    for (int k = 0; k < n; ++k)
        if (value[k] > m) m = value[k];
    why = unknown ? 8u : 0u;
    for (int k = 0; k < n; ++k)
        if (m > 0 && value[k] == m) why |= (unsigned)bit[k];
    cost = unknown && m < R.unknown_below ? -1 : m;
}

// ---- the kernels' dealing on the host --------------------------------------------------------------------------------------------
uint32_t load_bytes4(const int8_t *p, bool word) {
    uint32_t v;
    if (word) {
        if (reinterpret_cast<uintptr_t>(p) & 3u) std::abort();  // (the flag lied)
        std::memcpy(&v, p, 4);
        return v;
    }
    const uint8_t *q = reinterpret_cast<const uint8_t *>(p);
    return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
}
bool multiple_of(const void *p, uint64_t offset, unsigned bytes) { return ((reinterpret_cast<uintptr_t>(p) + offset) & (bytes - 1u)) == 0; }

// k_costmap_cells
void path_cells(const PwppCostmapRule &R, uint64_t n, const int8_t *o, const int8_t *t, const int32_t *d, const uint8_t *curve, int8_t *cost, uint8_t *why) {
    for (uint64_t i = 0; i < n; ++i) {
        int32_t c;
        uint32_t w;
        pwpp_costmap_fold(R, curve, (R.layers & 1) ? o[i] : 0, (R.layers & 4) ? t[i] : 0, (R.layers & 2) ? d[i] : 0, c, w);
        cost[i] = (int8_t)c;
        if (why) why[i] = (uint8_t)w;
    }
}

// k_costmap_quads with its launcher; `seen`: how often each cell was written
void path_quads(const PwppCostmapRule &R, uint64_t n, const int8_t *o, const int8_t *t, const int32_t *d, const uint8_t *curve_bytes, int8_t *cost,
                uint8_t *why, std::vector<int> &seen) {
    const uint32_t words = (R.layers & 2) ? ((uint32_t)R.n_curve + 3u) / 4u : 0u;
    std::vector<uint32_t> table(words ? words : 1, 0u);  // (exactly the words the kernel stages: a gather behind them is a finding)
    if (words) std::memcpy(table.data(), curve_bytes, (size_t)R.n_curve);
    const uint8_t *curve = reinterpret_cast<const uint8_t *>(table.data());
    const PwppCostmapDeal D = pwpp_costmap_deal((uint64_t)reinterpret_cast<uintptr_t>(cost), n);
    const bool word_o = multiple_of(o, D.head, 4), word_t = multiple_of(t, D.head, 4), word_why = multiple_of(why, D.head, 4);
    const bool use_o = R.layers & 1, use_d = R.layers & 2, use_t = R.layers & 4;
    const uint32_t items = D.groups + D.singles;
    const uint32_t per_group = PWPP_COSTMAP_BLOCK * PWPP_COSTMAP_LANE_ITEMS, groups = (items + per_group - 1) / per_group;
    for (uint32_t block = 0; block < groups; ++block)
        for (uint32_t lane = 0; lane < PWPP_COSTMAP_BLOCK; ++lane)
            for (uint32_t k = 0; k < PWPP_COSTMAP_LANE_ITEMS; ++k) {
                const uint32_t i = (block * PWPP_COSTMAP_LANE_ITEMS + k) * PWPP_COSTMAP_BLOCK + lane;
                if (i >= items) break;
                int cells;
                const uint64_t at = pwpp_costmap_item(D, i, cells);
                int32_t c;
                uint32_t w;
                for (int j = 0; j < cells; ++j) ++seen[at + j];
                if (cells == 1) {
                    pwpp_costmap_fold(R, curve, use_o ? o[at] : 0, use_t ? t[at] : 0, use_d ? d[at] : 0, c, w);
                    cost[at] = (int8_t)c;
                    if (why) why[at] = (uint8_t)w;
                    continue;
                }
                if (reinterpret_cast<uintptr_t>(cost + at) & 3u) std::abort();  // (the group's cost bytes are one aligned word)
                const uint32_t ow = use_o ? load_bytes4(o + at, word_o) : 0u, tw = use_t ? load_bytes4(t + at, word_t) : 0u;
                uint32_t cw = 0, ww = 0;
                for (int j = 0; j < 4; ++j) {
                    pwpp_costmap_fold(R, curve, (int)(int8_t)(ow >> (8 * j)), (int)(int8_t)(tw >> (8 * j)), use_d ? d[at + j] : 0, c, w);
                    cw |= ((uint32_t)c & 0xffu) << (8 * j), ww |= w << (8 * j);
                }
                std::memcpy(cost + at, &cw, 4);
                if (why) {
                    if (word_why) std::memcpy(why + at, &ww, 4);
                    else
                        for (int j = 0; j < 4; ++j) why[at + j] = (uint8_t)(ww >> (8 * j));
                }
            }
}

// k_costmap_occupied
void widen(uint64_t n, const int8_t *o, int32_t *count) {
    const uint64_t groups = n / 4;
    const bool word = multiple_of(o, 0, 4);
    for (uint64_t g = 0; g <= groups; ++g) {
        if (g < groups) {
            const uint32_t ow = load_bytes4(o + 4 * g, word);
            for (int j = 0; j < 4; ++j) count[4 * g + j] = (int8_t)(ow >> (8 * j)) == 100;
        } else {
            for (uint64_t i = 4 * groups; i < n; ++i) count[i] = o[i] == 100;
        }
    }
}

// an image of n elements that starts `offset` elements into an allocation of exactly offset + n: the bytes before it are poison
template <class T>
struct Image {
    std::vector<T> store;
    size_t offset;
    Image(size_t n, size_t off, T poison) : store(off + n, poison), offset(off) {}
    T *p() { return store.data() + offset; }
    bool head_intact(T poison) const {
        for (size_t i = 0; i < offset; ++i)
            if (store[i] != poison) return false;
        return true;
    }
};

long g_cases = 0, g_bad = 0;

void one_case(const PwppCostmapRule &R, const std::vector<uint8_t> &curve, size_t n, const int8_t *o_src, const int8_t *t_src, const int32_t *d_src, size_t off_o,
              size_t off_t, size_t off_c, size_t off_w, bool with_why) {
    Image<int8_t> o(n, off_o, 0x55), t(n, off_t, 0x55), c1(n, off_c, 0x66), c2(n, off_c, 0x66);
    Image<uint8_t> w1(n, off_w, 0x77), w2(n, off_w, 0x77);
    Image<int32_t> d(n, off_o, 0x55555555);  // (4-byte aligned at any offset)
    std::memcpy(o.p(), o_src, n), std::memcpy(t.p(), t_src, n), std::memcpy(d.p(), d_src, 4 * n);
    std::vector<uint8_t> exact(curve);  // (exactly n_curve bytes: path 1 reads the caller's table)
    std::vector<int> seen(n, 0);
    path_cells(R, n, o.p(), t.p(), d.p(), exact.data(), c1.p(), with_why ? w1.p() : nullptr);
    path_quads(R, n, o.p(), t.p(), d.p(), exact.data(), c2.p(), with_why ? w2.p() : nullptr, seen);
    bool ok = c1.head_intact(0x66) && c2.head_intact(0x66) && w1.head_intact(0x77) && w2.head_intact(0x77) && o.head_intact(0x55) && t.head_intact(0x55);
    ok = ok && std::memcmp(o.p(), o_src, n) == 0 && std::memcmp(t.p(), t_src, n) == 0 && std::memcmp(d.p(), d_src, 4 * n) == 0;  // (inputs are not written)
    for (size_t i = 0; i < n && ok; ++i) {
        int want_c;
        unsigned want_w;
        rule_again(R, exact.data(), o_src[i], t_src[i], d_src[i], want_c, want_w);
        ok = seen[i] == 1 && c1.p()[i] == (int8_t)want_c && c2.p()[i] == (int8_t)want_c;
        if (with_why) ok = ok && w1.p()[i] == (uint8_t)want_w && w2.p()[i] == (uint8_t)want_w;
        else ok = ok && w1.p()[i] == 0x77 && w2.p()[i] == 0x77;
    }
    ++g_cases;
    if (!ok) {
        ++g_bad;
        std::fprintf(stderr, "mismatch: layers %d unknowns %d %d below %d n_curve %d cells %zu offsets %zu %zu %zu %zu why %d\n", R.layers, R.occupancy_unknown,
                     R.terrain_unknown, R.unknown_below, R.n_curve, n, off_o, off_t, off_c, off_w, (int)with_why);
    }
}

std::vector<uint8_t> random_curve(std::mt19937 &rng, int n) {
    std::vector<uint8_t> c((size_t)n);
    for (auto &v : c) v = (uint8_t)(rng() % 101);
    return c;
}

int built_in() {
    std::mt19937 rng(20261020);
    // 1 every start offset 0 .. 3 of every image and every length 1 .. 9, every layers mask, random bytes over the whole int8 range
    for (int layers = 1; layers <= 7; ++layers)
        for (size_t n = 1; n <= 9; ++n)
            for (size_t off_c = 0; off_c < 4; ++off_c)
                for (size_t off_o = 0; off_o < 4; ++off_o)
                    for (size_t off_t = 0; off_t < 4; ++off_t) {
                        const int n_curve = 1 + (int)(rng() % 9);
                        const std::vector<uint8_t> curve = random_curve(rng, n_curve);
                        std::vector<int8_t> o(n), t(n);
                        std::vector<int32_t> d(n);
                        for (size_t i = 0; i < n; ++i) {
                            o[i] = rng() % 3 == 0 ? (int8_t)(rng() % 2 * 100) : (int8_t)rng(), t[i] = (int8_t)rng();
                            d[i] = rng() % 8 == 0 ? (rng() % 2 ? 0x7fffffff : -(int32_t)(rng() % 5) - 1) : (int32_t)(rng() % (2 * n_curve));
                        }
                        const PwppCostmapRule R{layers, (int)(rng() % 102) - 1, (int)(rng() % 102) - 1, 1 + (int)(rng() % 101), (layers & 2) ? n_curve : 0};
                        one_case(R, curve, n, o.data(), t.data(), d.data(), off_o, off_t, off_c, (off_c + off_o + n) % 4, (n + off_t) % 2 == 0);
                    }
    // 2 around the cells of one workgroup of path 2 and of several, the longest table, every offset of the cost image
    const size_t G = PWPP_COSTMAP_GROUP_CELLS;
    for (size_t n : {G - 1, G, G + 1, G + 7, 3 * G + 2, (size_t)257})
        for (size_t off_c = 0; off_c < 4; ++off_c)
            for (int n_curve : {1, 2, 26, PWPP_COSTMAP_CURVE_MAX}) {
                const std::vector<uint8_t> curve = random_curve(rng, n_curve);
                std::vector<int8_t> o(n), t(n);
                std::vector<int32_t> d(n);
                for (size_t i = 0; i < n; ++i) o[i] = rng() % 2 ? (int8_t)(rng() % 2 * 100) : (int8_t)rng(), t[i] = (int8_t)rng(), d[i] = (int32_t)(rng() % (2 * n_curve + 1));
                d[n / 2] = n_curve - 1, d[n / 3] = n_curve, d[0] = 0x7fffffff;
                const PwppCostmapRule R{7, off_c % 2 ? -1 : 30, off_c / 2 ? -1 : 60, (int)(1 + 25 * off_c + (off_c == 3)), n_curve};
                one_case(R, curve, n, o.data(), t.data(), d.data(), (off_c + 1) % 4, (off_c + 2) % 4, off_c, (off_c + 3) % 4, true);
            }
    // 3 every pair (o, t) under every mask and the corner values of the parameters
    {
        const size_t n = 65536;
        std::vector<int8_t> o(n), t(n);
        std::vector<int32_t> d(n);
        const std::vector<uint8_t> curve = random_curve(rng, 40);
        for (size_t i = 0; i < n; ++i) o[i] = (int8_t)(i >> 8), t[i] = (int8_t)(i & 255), d[i] = (int32_t)(rng() % 80);
        for (int layers = 1; layers <= 7; ++layers)
            for (int ou : {-1, 0, 100})
                for (int tu : {-1, 0, 100})
                    for (int below : {1, 50, 100, 101}) one_case(PwppCostmapRule{layers, ou, tu, below, (layers & 2) ? 40 : 0}, curve, n, o.data(), t.data(), d.data(), 1, 2, 3, 0, true);
    }
    // 4 the widening, every offset and length 1 .. 9 and a long one
    for (size_t n : {1, 2, 3, 4, 5, 6, 7, 8, 9, 1027})
        for (size_t off = 0; off < 4; ++off) {
            Image<int8_t> o(n, off, 0x55);
            std::vector<int32_t> count(n, -7);
            for (size_t i = 0; i < n; ++i) o.p()[i] = rng() % 2 ? 100 : (int8_t)rng();
            widen(n, o.p(), count.data());
            bool ok = true;
            for (size_t i = 0; i < n; ++i) ok = ok && count[i] == (o.p()[i] == 100 ? 1 : 0);
            ++g_cases;
            if (!ok) ++g_bad, std::fprintf(stderr, "mismatch: widening of %zu cells at offset %zu\n", n, off);
        }
    // 5 the cap of the own distances: the least R with R * R >= n_curve - 1, at least 1; and the dealing's sums
    for (int n_curve = 1; n_curve <= PWPP_COSTMAP_CURVE_MAX; ++n_curve) {
        int r = 0;
        while (r * r < n_curve - 1) ++r;
        ++g_cases;
        if (pwpp_costmap_cap(n_curve) != (r > 1 ? r : 1)) ++g_bad, std::fprintf(stderr, "mismatch: cap of n_curve %d\n", n_curve);
    }
    for (uint64_t address = 0; address < 4; ++address)
        for (uint64_t n : {(uint64_t)1, (uint64_t)2, (uint64_t)3, (uint64_t)4, (uint64_t)1 << 31}) {
            const PwppCostmapDeal D = pwpp_costmap_deal(address, n);
            ++g_cases;
            if ((uint64_t)D.groups * 4 + D.singles != n || D.singles > 6 || D.head > 3) ++g_bad, std::fprintf(stderr, "mismatch: dealing of %llu cells\n", (unsigned long long)n);
        }
    std::printf("costmap_check: %ld cases, %ld mismatches\n", g_cases, g_bad);
    return g_bad == 0 ? 0 : 1;
}

template <class T>
bool read_file(const char *path, size_t n, std::vector<T> &out) {
    out.assign(n, T());
    if (std::string(path) == "-") return true;
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    const size_t got = std::fread(out.data(), sizeof(T), n, f);
    std::fclose(f);
    return got == n;
}
template <class T>
bool write_file(const std::string &path, const T *p, size_t n) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const size_t put = std::fwrite(p, sizeof(T), n, f);
    return std::fclose(f) == 0 && put == n;
}

int dump(char **a) {
    PwppCostmapRule R{std::atoi(a[0]), std::atoi(a[1]), std::atoi(a[2]), std::atoi(a[3]), 0};
    const size_t n = (size_t)std::atoll(a[8]);
    std::vector<uint8_t> curve;
    if (std::string(a[4]) != "-") {
        FILE *f = std::fopen(a[4], "rb");
        if (!f) return 2;
        uint8_t b;
        while (std::fread(&b, 1, 1, f) == 1) curve.push_back(b);
        std::fclose(f);
    }
    R.n_curve = (R.layers & 2) ? (int)curve.size() : 0;
    std::vector<int8_t> o, t;
    std::vector<int32_t> d;
    if (!read_file(a[5], n, o) || !read_file(a[6], n, t) || !read_file(a[7], n, d)) return 2;
    Image<int8_t> c1(n, 0, 0), c2(n, 1, 0);  // (path 2 at an odd address: head, groups and tail)
    Image<uint8_t> w1(n, 0, 0), w2(n, 3, 0);
    std::vector<int> seen(n, 0);
    path_cells(R, n, o.data(), t.data(), d.data(), curve.data(), c1.p(), w1.p());
    path_quads(R, n, o.data(), t.data(), d.data(), curve.data(), c2.p(), w2.p(), seen);
    if (std::memcmp(c1.p(), c2.p(), n) != 0 || std::memcmp(w1.p(), w2.p(), n) != 0) return 3;
    return write_file(std::string(a[9]) + ".cost", c2.p(), n) && write_file(std::string(a[9]) + ".why", w2.p(), n) ? 0 : 2;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 1) return built_in();
    if (argc == 12 && std::string(argv[1]) == "dump") return dump(argv + 2);
    std::fprintf(stderr, "usage: costmap_check | costmap_check dump LAYERS OCC_UNKNOWN TERRAIN_UNKNOWN UNKNOWN_BELOW CURVE O T D CELLS OUT\n");
    return 2;
}
