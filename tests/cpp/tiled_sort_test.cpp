// Standalone driver of the tiled sort (mauvealigner_amd/csrc/tiled_sort.hpp), built with hipcc --offload-arch=gfx950 -x hip.
//   tiled_sort_test check   every case of the matrix against std::stable_sort; prints "ok <cases>" or the first mismatch, exit 1
//   tiled_sort_test bench   device time per launch (hipEvent around each, min / median of the repeats) at the shape of the seed pass's
//                           sort in C3 (25 M pairs, 32-bit key and value, bits 14 .. 30, first pass from the strand bitmap) and in C5
//                           (222 M pairs, 64-bit key, three passes); one JSON line per shape.  Build with -DRS_SWZ=0 to take
//                           the tile order out: the line names the switch it was built with.
#include "../../mauvealigner_amd/csrc/tiled_sort.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#define CK(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e__)); exit(2); } } while (0)

struct NoBook { template <typename F> void operator()(int, F &&f) const { f(); } };

enum { P_RANDOM, P_EQUAL, P_TWO, P_SORTED, P_REVERSED, P_LANE, P_LANE2, P_HALVES, N_PATTERNS };
static const char *const PNAME[N_PATTERNS] = {"random", "equal", "two", "sorted", "reversed", "digit=lane", "digit=lane/2", "halves"};

// P_LANE, P_LANE2, P_HALVES put the same digit into every byte of the key, so the first pass sees it whatever shift_lo is: the key at index
// x sits in lane x % 64 of its wave (rs_scatter_tile's wave-striped load)
template <typename KeyT>
static std::vector<KeyT> make_keys(uint32_t n, int key_bits, int pattern, std::mt19937_64 &rng)
{
    const KeyT mask = key_bits >= (int)(8 * sizeof(KeyT)) ? (KeyT)~(KeyT)0 : (KeyT)(((KeyT)1 << key_bits) - 1);
    const KeyT ones = (KeyT)0x0101010101010101ULL;
    std::vector<KeyT> k(n);
    const KeyT a = (KeyT)rng() & mask, b = (KeyT)rng() & mask;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t lane = i & 63u;
        switch (pattern) {
        case P_EQUAL: k[i] = a; break;
        case P_TWO: k[i] = (rng() & 1) ? a : b; break;
        case P_LANE: k[i] = (KeyT)(ones * (KeyT)lane) & mask; break;
        case P_LANE2: k[i] = (KeyT)(ones * (KeyT)(lane / 2)) & mask; break;
        case P_HALVES: k[i] = (KeyT)(ones * (KeyT)(lane < 32 ? 0x5a : 0xa5)) & mask; break;
        default: k[i] = (KeyT)rng() & mask; break;                                    // random; then sorted / reversed
        }
    }
    if (pattern == P_SORTED) std::sort(k.begin(), k.end());
    if (pattern == P_REVERSED) std::sort(k.begin(), k.end(), [](KeyT x, KeyT y) { return x > y; });
    return k;
}

// device buffers of the largest case, made once
struct Bufs {
    void *k[2], *v[2]; uint32_t *hist, *totals;
    void init(size_t nmax)
    {
        for (int b = 0; b < 2; b++) { CK(hipMalloc(&k[b], nmax * 8)); CK(hipMalloc(&v[b], nmax * 8)); }
        CK(hipMalloc(&hist, rs_hist_words((uint32_t)nmax) * 4)); CK(hipMalloc(&totals, 256 * 4));
    }
};

// iota: no values go in -- the first pass takes a random strand bitmap (whole tiles, zero behind n) and the tile histograms of that pass,
// made here on the host, as the seed pass does; the value of key x is x | bit x << (top bit of ValT)
template <typename KeyT, typename ValT>
static bool run_case(Bufs &B, uint32_t n, int key_bits, int shift_lo, int pattern, bool iota, uint64_t seed, std::string *why)
{
    std::mt19937_64 rng(seed);
    const uint32_t nblk = rs_tiles(n);
    std::vector<KeyT> k = make_keys<KeyT>(n, key_bits, pattern, rng);
    std::vector<ValT> v(n);
    std::vector<uint64_t> bits((size_t)nblk * (RS_TILE / 64), 0);
    if (iota) {
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t bit = rng() & 1;
            bits[i >> 6] |= bit << (i & 63);
            v[i] = (ValT)i | ((ValT)bit << (8 * sizeof(ValT) - 1));
        }
    } else {
        std::vector<uint32_t> p(n);
        std::iota(p.begin(), p.end(), 0u);
        std::shuffle(p.begin(), p.end(), rng);                                        // values: a permutation, so stability shows
        for (uint32_t i = 0; i < n; i++) v[i] = (ValT)p[i] | (sizeof(ValT) == 8 ? (ValT)((uint64_t)p[i] << 33) : (ValT)0);
    }
    // expected: stable sort by the digits the passes look at, bits [shift_lo, shift_lo + 8 * passes)
    const int passes = (key_bits - shift_lo + 7) / 8, fb = 8 * passes;
    const uint64_t fmask = fb >= 64 ? ~0ULL : ((1ULL << fb) - 1);
    std::vector<uint32_t> idx(n);
    std::iota(idx.begin(), idx.end(), 0u);
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) {
        return (((uint64_t)k[x] >> shift_lo) & fmask) < (((uint64_t)k[y] >> shift_lo) & fmask); });

    KeyT *dk[2] = {(KeyT *)B.k[0], (KeyT *)B.k[1]}; ValT *dv[2] = {(ValT *)B.v[0], (ValT *)B.v[1]};
    CK(hipMemset(B.hist, 0xa5, rs_hist_words(n) * 4));                                // the sort must not rely on the workspace's contents
    CK(hipMemset(B.totals, 0xa5, 256 * 4));
    CK(hipMemcpy(dk[0], k.data(), (size_t)n * sizeof(KeyT), hipMemcpyHostToDevice));
    if (iota) {
        std::vector<uint32_t> h((size_t)nblk * 256, 0);
        for (uint32_t i = 0; i < n; i++) h[(size_t)((uint32_t)(k[i] >> shift_lo) & 255u) * nblk + i / RS_TILE]++;
        CK(hipMemcpy(B.hist, h.data(), h.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(dv[0], bits.data(), bits.size() * 8, hipMemcpyHostToDevice));
    } else
        CK(hipMemcpy(dv[0], v.data(), (size_t)n * sizeof(ValT), hipMemcpyHostToDevice));
    KeyT *ko = dk[0]; ValT *vo = dv[0];
    tiled_sort<KeyT, ValT>(0, n, key_bits, shift_lo, &ko, &vo, dk[1], dv[1], B.hist, B.totals, iota, nblk <= 64, iota, NoBook());
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<KeyT> gk(n); std::vector<ValT> gv(n);
    CK(hipMemcpy(gk.data(), ko, (size_t)n * sizeof(KeyT), hipMemcpyDeviceToHost));
    CK(hipMemcpy(gv.data(), vo, (size_t)n * sizeof(ValT), hipMemcpyDeviceToHost));
    bool ok = (ko == dk[passes & 1]) && (vo == dv[passes & 1]);
    if (!ok) *why = "result not in the buffers the pass parity implies";
    for (uint32_t i = 0; ok && i < n; i++)
        if (gk[i] != k[idx[i]] || gv[i] != v[idx[i]]) {
            ok = false;
            *why = "first difference at " + std::to_string(i) + ": got (" + std::to_string((uint64_t)gk[i]) + ", " + std::to_string((uint64_t)gv[i]) +
                   ") want (" + std::to_string((uint64_t)k[idx[i]]) + ", " + std::to_string((uint64_t)v[idx[i]]) + ")";
        }
    return ok;
}

struct Case { int kw, vw; uint32_t n; int key_bits, shift_lo, pattern; bool iota; };

static bool run(Bufs &B, const Case &c, std::string *why)
{
    const uint64_t seed = 1469598103934665603ULL ^ ((uint64_t)c.n << 20) ^ ((uint64_t)c.key_bits << 8) ^ ((uint64_t)c.shift_lo << 14) ^ (uint64_t)c.pattern ^
                          ((uint64_t)(c.kw + 2 * c.vw + 4 * c.iota) << 50);
    if (c.kw == 4 && c.vw == 4) return run_case<uint32_t, uint32_t>(B, c.n, c.key_bits, c.shift_lo, c.pattern, c.iota, seed, why);
    if (c.kw == 4 && c.vw == 8) return run_case<uint32_t, uint64_t>(B, c.n, c.key_bits, c.shift_lo, c.pattern, c.iota, seed, why);
    if (c.kw == 8 && c.vw == 4) return run_case<uint64_t, uint32_t>(B, c.n, c.key_bits, c.shift_lo, c.pattern, c.iota, seed, why);
    return run_case<uint64_t, uint64_t>(B, c.n, c.key_bits, c.shift_lo, c.pattern, c.iota, seed, why);
}

// The matrix goes by where the tile order, the ranking and the histogram can go wrong, not by size:
//   A  every tile count x last tile (full, one key short, one key long) x every key pattern, 4 + 4 bytes, 16 key bits (two passes);
//   B  every pair width x every bit range x {random, halves} at 9 tiles (raw histograms) and 73 (row scan), ragged last tile;
//   C  the first pass from a strand bitmap: every tile count x last tile, 32- and 64-bit values, and 64-bit keys at 9 and 73 tiles.
static int check()
{
    const uint32_t tiles[] = {1, 7, 8, 9, 64, 65, 71, 72, 73};
    struct Bits { int key_bits, shift_lo; };
    const Bits bits[] = {{8, 0}, {16, 0}, {24, 0}, {32, 0}, {30, 14}};
    const int widths[4][2] = {{4, 4}, {4, 8}, {8, 4}, {8, 8}};
    auto sizes = [](uint32_t t) { return std::vector<uint32_t>{t * RS_TILE, t * RS_TILE - 1, (t - 1) * RS_TILE + 1}; };
    std::vector<Case> cases;
    for (uint32_t t : tiles)
        for (uint32_t n : sizes(t))
            for (int pat = 0; pat < N_PATTERNS; pat++) cases.push_back({4, 4, n, 16, 0, pat, false});
    for (const auto &w : widths)
        for (const Bits &b : bits)
            for (int pat : {(int)P_RANDOM, (int)P_HALVES}) {
                cases.push_back({w[0], w[1], 9 * RS_TILE - 1, b.key_bits, b.shift_lo, pat, false});
                cases.push_back({w[0], w[1], 72 * RS_TILE + 1, b.key_bits, b.shift_lo, pat, false});
            }
    for (uint32_t t : tiles)
        for (uint32_t n : sizes(t))
            for (int vw : {4, 8}) cases.push_back({4, vw, n, 30, 14, P_RANDOM, true});
    for (uint32_t n : {9 * (uint32_t)RS_TILE - 1, 72 * (uint32_t)RS_TILE + 1})
        for (int vw : {4, 8}) { cases.push_back({8, vw, n, 30, 14, P_RANDOM, true}); cases.push_back({8, vw, n, 22, 14, P_TWO, true}); }
    Bufs B;
    B.init((size_t)73 * RS_TILE);
    int bad = 0;
    for (const Case &c : cases) {
        std::string why;
        if (!run(B, c, &why)) {
            bad++;
            printf("FAIL n=%u key=u%d val=u%d bits=%d shift_lo=%d pattern=%s iota=%d: %s\n", c.n, 8 * c.kw, 8 * c.vw, c.key_bits, c.shift_lo, PNAME[c.pattern],
                   (int)c.iota, why.c_str());
        }
    }
    printf("%s %d cases, %d failed\n", bad ? "FAIL" : "ok", (int)cases.size(), bad);
    return bad ? 1 : 0;
}

// ---- bench ----
struct EventBook {
    struct Rec { int kind; hipEvent_t e0, e1; };
    std::vector<Rec> recs;
    template <typename F> void operator()(int kind, F &&f)
    {
        Rec r; r.kind = kind;
        CK(hipEventCreate(&r.e0)); CK(hipEventCreate(&r.e1));
        CK(hipEventRecord(r.e0, 0)); f(); CK(hipEventRecord(r.e1, 0));
        recs.push_back(r);
    }
};

template <typename KeyT>
__global__ void fill_keys(KeyT *k, uint32_t n, uint64_t mask)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        uint64_t z = (uint64_t)i * 0x9e3779b97f4a7c15ULL + 0x632be59bd9b4e019ULL;                // splitmix64
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL; z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL; z ^= z >> 31;
        k[i] = (KeyT)(z & mask);
    }
}

template <typename KeyT>
static void bench_shape(const char *name, uint32_t n, int key_bits, int shift_lo, int reps)
{
    const uint32_t nblk = rs_tiles(n);
    KeyT *src, *dk[2]; uint32_t *dv[2], *hist, *totals;
    const size_t vbytes = std::max((size_t)n * 4, (size_t)nblk * (RS_TILE / 8));
    CK(hipMalloc(&src, (size_t)n * sizeof(KeyT)));
    for (int b = 0; b < 2; b++) { CK(hipMalloc(&dk[b], (size_t)n * sizeof(KeyT))); CK(hipMalloc(&dv[b], vbytes)); }
    CK(hipMalloc(&hist, rs_hist_words(n) * 4)); CK(hipMalloc(&totals, 256 * 4));
    hipLaunchKernelGGL(fill_keys<KeyT>, dim3(4096), dim3(256), 0, 0, src, n, key_bits >= 64 ? ~0ULL : ((1ULL << key_bits) - 1));
    const int passes = (key_bits - shift_lo + 7) / 8;
    std::vector<std::vector<float>> us;                      // per launch of a sort, over the repeats
    std::vector<int> kinds;
    for (int r = 0; r < reps + 2; r++) {
        // a sort as the seed pass runs it: fresh keys, the strand bitmap in the value buffer, the first histogram made on the way in
        CK(hipMemcpyAsync(dk[0], src, (size_t)n * sizeof(KeyT), hipMemcpyDeviceToDevice, 0));
        CK(hipMemsetAsync(dv[0], 0x5a, (size_t)nblk * (RS_TILE / 8), 0));
        EventBook book;
        book(RS_K_HIST, [&] { hipLaunchKernelGGL(rs_hist<KeyT>, dim3(nblk), dim3(RS_THREADS), 0, 0, dk[0], n, shift_lo, hist, nblk); });
        KeyT *ko = dk[0]; uint32_t *vo = dv[0];
        tiled_sort<KeyT, uint32_t>(0, n, key_bits, shift_lo, &ko, &vo, dk[1], dv[1], hist, totals, true, nblk <= 64, true, book);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        if (us.empty()) { us.resize(book.recs.size()); for (auto &q : book.recs) kinds.push_back(q.kind); }
        for (size_t i = 0; i < book.recs.size(); i++) {
            float ms = 0.f;
            CK(hipEventElapsedTime(&ms, book.recs[i].e0, book.recs[i].e1));
            if (r >= 2) us[i].push_back(1000.f * ms);                                  // (two warm-up sorts)
            CK(hipEventDestroy(book.recs[i].e0)); CK(hipEventDestroy(book.recs[i].e1));
        }
    }
    printf("{\"shape\": \"%s\", \"n\": %u, \"key_bytes\": %d, \"passes\": %d, \"RS_SWZ\": %d, \"launches\": [", name, n, (int)sizeof(KeyT), passes,
           (int)RS_SWZ);
    static const char *const KN[3] = {"rs_hist", "rs_rowscan", "rs_scatter"};
    float sum_med = 0.f;
    for (size_t i = 0; i < us.size(); i++) {
        std::sort(us[i].begin(), us[i].end());
        const float med = us[i][us[i].size() / 2];
        if (i > 0) sum_med += med;                                                       // (launch 0 stands in for seed_extract_all's histogram)
        printf("%s{\"kernel\": \"%s\", \"us_min\": %.1f, \"us_med\": %.1f, \"us_max\": %.1f}", i ? ", " : "", KN[kinds[i]], us[i].front(), med, us[i].back());
    }
    printf("], \"sort_us_med\": %.1f}\n", sum_med);
    fflush(stdout);
    CK(hipFree(src));
    for (int b = 0; b < 2; b++) { CK(hipFree(dk[b])); CK(hipFree(dv[b])); }
    CK(hipFree(hist)); CK(hipFree(totals));
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "check";
    if (mode == "check") return check();
    if (mode == "bench") {
        const int reps = argc > 2 ? atoi(argv[2]) : 20;
        bench_shape<uint32_t>("C3", 25000000u, 30, 14, reps);
        bench_shape<uint64_t>("C5", 222000000u, 38, 14, std::max(3, reps / 4));
        return 0;
    }
    fprintf(stderr, "usage: %s check|bench [repeats]\n", argv[0]);
    return 2;
}
