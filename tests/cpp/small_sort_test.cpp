// Standalone driver of the small-sort engine (mauvealigner_amd/csrc/small_sort.hpp), built with hipcc --offload-arch=gfx950 -x hip.
//   small_sort_test check   every case of the matrix against std::stable_sort; prints "ok <cases>" or the first mismatch, exit 1
//   small_sort_test bench   device time per sort (hipEvent, mean of many) for every tile size at n = 4 k .. 262 k, one JSON line each
#include "../../mauvealigner_amd/csrc/small_sort.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#define CK(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e__)); exit(2); } } while (0)

struct NoBook { template <typename F> void operator()(bool, F &&f) const { f(); } };

template <typename KeyT>
static std::vector<KeyT> make_keys(uint32_t n, int key_bits, int pattern, std::mt19937_64 &rng)
{
    const KeyT mask = key_bits >= (int)(8 * sizeof(KeyT)) ? (KeyT)~(KeyT)0 : (KeyT)(((KeyT)1 << key_bits) - 1);
    std::vector<KeyT> k(n);
    const KeyT a = (KeyT)rng() & mask, b = (KeyT)rng() & mask;
    for (uint32_t i = 0; i < n; i++) {
        switch (pattern) {
        case 0: k[i] = (KeyT)rng() & mask; break;                                     // random
        case 1: k[i] = a; break;                                                      // all equal
        case 2: k[i] = (rng() & 1) ? a : b; break;                                    // two values
        default: k[i] = (KeyT)rng() & mask; break;                                   // 3, 4: random, then sorted / reversed
        }
    }
    if (pattern == 3) std::sort(k.begin(), k.end());
    if (pattern == 4) std::sort(k.begin(), k.end(), [](KeyT x, KeyT y) { return x > y; });
    return k;
}

template <typename KeyT>
static bool run_case(uint32_t n, int key_bits, int shift_lo, int pattern, uint64_t seed, std::string *why)
{
    std::mt19937_64 rng(seed);
    std::vector<KeyT> k = make_keys<KeyT>(n, key_bits, pattern, rng);
    std::vector<uint32_t> v(n);
    std::iota(v.begin(), v.end(), 0u);
    std::shuffle(v.begin(), v.end(), rng);                                           // values: a permutation, so stability shows
    // expected: stable sort by the digits the passes look at, bits [shift_lo, shift_lo + 8 * passes)
    const int passes = (key_bits - shift_lo + 7) / 8, fb = 8 * passes;
    const uint64_t fmask = fb >= 64 ? ~0ULL : ((1ULL << fb) - 1);
    std::vector<uint32_t> idx(n);
    std::iota(idx.begin(), idx.end(), 0u);
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) {
        return (((uint64_t)k[x] >> shift_lo) & fmask) < (((uint64_t)k[y] >> shift_lo) & fmask); });

    KeyT *dk[2]; uint32_t *dv[2], *ws;
    for (int b = 0; b < 2; b++) { CK(hipMalloc(&dk[b], (size_t)n * sizeof(KeyT))); CK(hipMalloc(&dv[b], (size_t)n * 4)); }
    CK(hipMalloc(&ws, ss_ws_words(n) * 4));
    CK(hipMemset(ws, 0xa5, ss_ws_words(n) * 4));                                      // the engine must not rely on its contents
    CK(hipMemcpy(dk[0], k.data(), (size_t)n * sizeof(KeyT), hipMemcpyHostToDevice));
    CK(hipMemcpy(dv[0], v.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    KeyT *ko = dk[0]; uint32_t *vo = dv[0];
    small_sort<KeyT>(0, n, key_bits, shift_lo, &ko, &vo, dk[1], dv[1], ws, NoBook());
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<KeyT> gk(n); std::vector<uint32_t> gv(n);
    CK(hipMemcpy(gk.data(), ko, (size_t)n * sizeof(KeyT), hipMemcpyDeviceToHost));
    CK(hipMemcpy(gv.data(), vo, (size_t)n * 4, hipMemcpyDeviceToHost));
    bool ok = (ko == dk[passes & 1]) && (vo == dv[passes & 1]);
    if (!ok) *why = "result not in the buffers the pass parity implies";
    for (uint32_t i = 0; ok && i < n; i++)
        if (gk[i] != k[idx[i]] || gv[i] != v[idx[i]]) {
            ok = false;
            *why = "first difference at " + std::to_string(i) + ": got (" + std::to_string((uint64_t)gk[i]) + ", " + std::to_string(gv[i]) +
                   ") want (" + std::to_string((uint64_t)k[idx[i]]) + ", " + std::to_string(v[idx[i]]) + ")";
        }
    for (int b = 0; b < 2; b++) { CK(hipFree(dk[b])); CK(hipFree(dv[b])); }
    CK(hipFree(ws));
    return ok;
}

static int check()
{
    const uint32_t ns[] = {1, 255, 256, 257, 4095, 56502, SS_CAP, SS_CAP + 1};
    struct Bits { bool wide; int key_bits, shift_lo; };
    const Bits bits[] = {{false, 3, 0}, {false, 6, 0}, {false, 9, 0}, {false, 24, 0}, {false, 32, 0},
                         {true, 24, 0}, {true, 48, 0}, {true, 48, 5}, {true, 40, 16}};
    int cases = 0, bad = 0;
    for (uint32_t n : ns)
        for (const Bits &b : bits)
            for (int pat = 0; pat < 5; pat++) {
                std::string why;
                const uint64_t seed = 1469598103934665603ULL ^ ((uint64_t)n << 20) ^ ((uint64_t)b.key_bits << 8) ^ ((uint64_t)b.shift_lo << 14) ^ pat;
                const bool ok = b.wide ? run_case<uint64_t>(n, b.key_bits, b.shift_lo, pat, seed, &why)
                                       : run_case<uint32_t>(n, b.key_bits, b.shift_lo, pat, seed, &why);
                cases++;
                if (!ok) {
                    bad++;
                    printf("FAIL n=%u key=%s bits=%d shift_lo=%d pattern=%d: %s\n", n, b.wide ? "u64" : "u32", b.key_bits, b.shift_lo, pat, why.c_str());
                }
            }
    printf("%s %d cases, %d failed\n", bad ? "FAIL" : "ok", cases, bad);
    return bad ? 1 : 0;
}

template <typename KeyT, int ITEMS>
static double time_sort(uint32_t n, int key_bits, KeyT *k0, uint32_t *v0, KeyT *k1, uint32_t *v1, uint32_t *ws, int reps)
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    NoBook nb;
    for (int r = 0; r < 10; r++) ss_run<KeyT, ITEMS>(0, n, key_bits, 0, k0, v0, k1, v1, ws, nb);
    CK(hipEventRecord(e0, 0));
    for (int r = 0; r < reps; r++) ss_run<KeyT, ITEMS>(0, n, key_bits, 0, k0, v0, k1, v1, ws, nb);
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, e0, e1));
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
    return 1000.0 * ms / reps;
}

static int bench()
{
    // u32 keys of 24 bits (the chain's per-genome sorts: three passes) and of 6 bits (the DP launch list: one pass); random
    // input, and sorted input (whole tiles share their next digit)
    const uint32_t ns[] = {4096, 16384, 56502, 131072, 262144};
    for (uint32_t n : ns)
        for (int key_bits : {6, 24})
        for (int pattern : {0, 3}) {
            std::mt19937_64 rng(n);
            std::vector<uint32_t> k = make_keys<uint32_t>(n, key_bits, pattern, rng), v(n);
            std::iota(v.begin(), v.end(), 0u);
            uint32_t *dk[2], *dv[2], *ws;
            for (int b = 0; b < 2; b++) { CK(hipMalloc(&dk[b], (size_t)n * 4)); CK(hipMalloc(&dv[b], (size_t)n * 4)); }
            const size_t wsw = (size_t)3 * ss_tiles(n, 1) * 256;                     // the largest workspace (256-key tiles)
            CK(hipMalloc(&ws, wsw * 4));
            // the sort is timed on its own output after the first run: keys stay a permutation of the same multiset
            CK(hipMemcpy(dk[0], k.data(), (size_t)n * 4, hipMemcpyHostToDevice));
            CK(hipMemcpy(dv[0], v.data(), (size_t)n * 4, hipMemcpyHostToDevice));
            CK(hipMemcpy(dk[1], k.data(), (size_t)n * 4, hipMemcpyHostToDevice));
            CK(hipMemcpy(dv[1], v.data(), (size_t)n * 4, hipMemcpyHostToDevice));
            const int reps = 200;
            const double t[5] = {time_sort<uint32_t, 1>(n, key_bits, dk[0], dv[0], dk[1], dv[1], ws, reps),
                                 time_sort<uint32_t, 2>(n, key_bits, dk[0], dv[0], dk[1], dv[1], ws, reps),
                                 time_sort<uint32_t, 4>(n, key_bits, dk[0], dv[0], dk[1], dv[1], ws, reps),
                                 time_sort<uint32_t, 8>(n, key_bits, dk[0], dv[0], dk[1], dv[1], ws, reps),
                                 time_sort<uint32_t, 16>(n, key_bits, dk[0], dv[0], dk[1], dv[1], ws, reps)};
            printf("{\"n\": %u, \"key_bits\": %d, \"input\": \"%s\", \"chosen_tile\": %d, \"us_per_sort\": {\"256\": %.2f, \"512\": %.2f, \"1024\": %.2f, \"2048\": %.2f, \"4096\": %.2f}}\n",
                   n, key_bits, pattern ? "sorted" : "random", 256 * ss_items(n), t[0], t[1], t[2], t[3], t[4]);
            for (int b = 0; b < 2; b++) { CK(hipFree(dk[b])); CK(hipFree(dv[b])); }
            CK(hipFree(ws));
        }
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "check";
    if (mode == "check") return check();
    if (mode == "bench") return bench();
    fprintf(stderr, "usage: %s check|bench\n", argv[0]);
    return 2;
}
