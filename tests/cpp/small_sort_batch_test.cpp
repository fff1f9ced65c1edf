// Standalone driver of the batched small sort (small_sort_batch, mauvealigner_amd/csrc/small_sort.hpp), built with
// hipcc --offload-arch=gfx950 -x hip.  S independent sorts of n pairs each in one set of launches, the segments a fixed stride apart:
// every segment must come out as std::stable_sort of that segment alone, in the buffers the pass parity implies, and nothing
// outside the segments (the gaps the stride leaves, the guard words around every buffer) may change.
//   small_sort_batch_test check   prints "ok <cases>" or the failing cases, exit 1
#include "../../mauvealigner_amd/csrc/small_sort.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>
#include <thread>
#include <vector>

#define CK(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e__)); exit(2); } } while (0)

struct NoBook { template <typename F> void operator()(bool, F &&f) const { f(); } };

constexpr uint32_t GUARD = 64;                       // sentinel words in front of and behind every buffer
constexpr uint32_t PAD = 3;                          // the stride leaves PAD unused words behind every segment
constexpr uint32_t SENT_K = 0xdeadbeefu, SENT_V = 0xfeedf00du, SENT_H = 0xa5a5a5a5u;

enum { UNIFORM = 0, EQUAL = 1, SORTED = 2 };

// device buffers of one size class, reused by all its cases
struct Bufs {
    size_t words = 0, ws_words = 0;
    uint32_t *k[2] = {nullptr, nullptr}, *v[2] = {nullptr, nullptr}, *ws = nullptr;
    void ensure(size_t w, size_t wsw)
    {
        if (w <= words && wsw <= ws_words) return;
        release();
        words = w; ws_words = wsw;
        for (int b = 0; b < 2; b++) { CK(hipMalloc(&k[b], (w + 2 * GUARD) * 4)); CK(hipMalloc(&v[b], (w + 2 * GUARD) * 4)); }
        CK(hipMalloc(&ws, (wsw + 2 * GUARD) * 4));
    }
    void release()
    {
        for (int b = 0; b < 2; b++) { if (k[b]) CK(hipFree(k[b])); if (v[b]) CK(hipFree(v[b])); k[b] = v[b] = nullptr; }
        if (ws) CK(hipFree(ws));
        ws = nullptr; words = ws_words = 0;
    }
};

static bool run_case(Bufs &B, uint32_t S, uint32_t n, int key_bits, int pattern, uint64_t seed, std::string *why)
{
    const size_t stride = (size_t)n + PAD, words = (size_t)S * stride, wsw = ss_ws_words_batch(S, n);
    B.ensure(words, wsw);
    std::mt19937_64 rng(seed);
    const uint32_t mask = key_bits >= 32 ? ~0u : ((1u << key_bits) - 1u);
    // host images of the four buffers, guards and gaps filled with the sentinels
    std::vector<uint32_t> hk(words + 2 * GUARD, SENT_K), hv(words + 2 * GUARD, SENT_V);
    for (uint32_t s = 0; s < S; s++) {
        uint32_t *k = hk.data() + GUARD + s * stride, *v = hv.data() + GUARD + s * stride;
        const uint32_t a = (uint32_t)rng() & mask;
        for (uint32_t i = 0; i < n; i++) { k[i] = pattern == EQUAL ? a : (uint32_t)rng() & mask; v[i] = i; }   // values = index: stability shows
        if (pattern == SORTED) std::sort(k, k + n);
    }
    std::vector<uint32_t> sent_k(words + 2 * GUARD, SENT_K), sent_v(words + 2 * GUARD, SENT_V), sent_h(wsw + 2 * GUARD, SENT_H);
    CK(hipMemcpy(B.k[0], hk.data(), hk.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(B.v[0], hv.data(), hv.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(B.k[1], sent_k.data(), sent_k.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(B.v[1], sent_v.data(), sent_v.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(B.ws, sent_h.data(), sent_h.size() * 4, hipMemcpyHostToDevice));          // (the engine must not rely on the workspace's contents)

    uint32_t *ko = B.k[0] + GUARD, *vo = B.v[0] + GUARD;
    small_sort_batch<uint32_t>(0, S, n, stride, key_bits, 0, &ko, &vo, B.k[1] + GUARD, B.v[1] + GUARD, B.ws + GUARD, NoBook());
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());

    const int passes = (key_bits + 7) / 8, res = passes & 1;
    if (ko != B.k[res] + GUARD || vo != B.v[res] + GUARD) { *why = "result not in the buffers the pass parity implies"; return false; }
    std::vector<uint32_t> gk[2], gv[2], gh(wsw + 2 * GUARD);
    for (int b = 0; b < 2; b++) {
        gk[b].resize(words + 2 * GUARD); gv[b].resize(words + 2 * GUARD);
        CK(hipMemcpy(gk[b].data(), B.k[b], gk[b].size() * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(gv[b].data(), B.v[b], gv[b].size() * 4, hipMemcpyDeviceToHost));
    }
    CK(hipMemcpy(gh.data(), B.ws, gh.size() * 4, hipMemcpyDeviceToHost));
    // guards of every buffer and the gaps between the segments
    for (int b = 0; b < 2; b++) {
        for (size_t i = 0; i < words + 2 * GUARD; i++) {
            const bool guard = i < GUARD || i >= GUARD + words, gap = !guard && (i - GUARD) % stride >= n;
            if ((guard || gap) && (gk[b][i] != SENT_K || gv[b][i] != SENT_V)) {
                *why = std::string(guard ? "guard" : "gap") + " word " + std::to_string(i) + " of buffer pair " + std::to_string(b) + " changed";
                return false;
            }
        }
    }
    for (size_t i = 0; i < GUARD; i++)
        if (gh[i] != SENT_H || gh[GUARD + wsw + i] != SENT_H) { *why = "guard word of the histogram workspace changed"; return false; }
    // every segment against std::stable_sort of that segment alone (the segments are independent: a few host threads share them)
    const uint32_t nthr = std::min<uint32_t>(S, 8);
    std::vector<std::string> errs(nthr);
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < nthr; t++)
        pool.emplace_back([&, t] {
            std::vector<uint32_t> idx(n);
            for (uint32_t s = t; s < S && errs[t].empty(); s += nthr) {
                const uint32_t *k = hk.data() + GUARD + s * stride, *v = hv.data() + GUARD + s * stride;
                const uint32_t *rk = gk[res].data() + GUARD + s * stride, *rv = gv[res].data() + GUARD + s * stride;
                std::iota(idx.begin(), idx.end(), 0u);
                std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return k[x] < k[y]; });
                for (uint32_t i = 0; i < n; i++)
                    if (rk[i] != k[idx[i]] || rv[i] != v[idx[i]]) {
                        errs[t] = "segment " + std::to_string(s) + ", first difference at " + std::to_string(i) + ": got (" + std::to_string(rk[i]) + ", " +
                                  std::to_string(rv[i]) + ") want (" + std::to_string(k[idx[i]]) + ", " + std::to_string(v[idx[i]]) + ")";
                        break;
                    }
            }
        });
    for (std::thread &th : pool) th.join();
    for (const std::string &e : errs) if (!e.empty()) { *why = e; return false; }
    return true;
}

static int check()
{
    // ragged tiles and the tile-class edges (ss_items: 8192, 32768, 98304); one .. four passes, both result parities
    const uint32_t ns[] = {1, 255, 256, 257, 8192, 8193, 32768, 32769, 56000, 98304, 98305};
    const uint32_t Ss[] = {1, 3, 4, 31};
    const int bits[] = {8, 9, 24, 25};
    Bufs B;
    int cases = 0, bad = 0;
    for (uint32_t n : ns)
        for (uint32_t S : Ss)
            for (int kb : bits)
                for (int pat : {UNIFORM, EQUAL, SORTED}) {
                    std::string why;
                    const uint64_t seed = 1469598103934665603ULL ^ ((uint64_t)n << 24) ^ ((uint64_t)S << 16) ^ ((uint64_t)kb << 8) ^ (uint64_t)pat;
                    cases++;
                    if (!run_case(B, S, n, kb, pat, seed, &why)) {
                        bad++;
                        printf("FAIL S=%u n=%u bits=%d pattern=%d: %s\n", S, n, kb, pat, why.c_str());
                    }
                }
    B.release();
    printf("%s %d cases, %d failed\n", bad ? "FAIL" : "ok", cases, bad);
    return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "check";
    if (mode == "check") return check();
    fprintf(stderr, "usage: %s check\n", argv[0]);
    return 2;
}
