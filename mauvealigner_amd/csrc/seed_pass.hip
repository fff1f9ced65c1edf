// seed_pass.hip -- the seed pass of the hot path on gfx950:
//   seed_extract  : 2-bit packed genomes -> (canonical masked mer, global position | strand)
//   (radix_sort.hip: LSD radix sort of the pairs -- the sorted mer list of all genomes at once)
//   mum_join      : runs of identical mers -> seed hits by the MatchFinder subclass rule
//   mum_candidates / mum_extend : ungapped extension of every hit into its maximal match
//
// Stands behind mems::MatchFinder::FindMatches [EXT] (call sites mauveAligner.cpp:523-589,
// progressiveMauve.cpp:490-501), with the in-tree rules of UniqueMatchFinder.cpp:36-60 and
// SeedMatchEnumerator.h:71-141.  Semantics are frozen in DESIGN.md S3/S4 and checked bit-exactly
// against oracle/ by tests/ (the oracle is never linked here).
// The host side runs a pass in stages (seedpass_stages); what follows the extension -- the guide tree's sums, the canonical order --
// does not depend on the key and index widths and lives in seed_finish.hip.
//
// All kernels are HBM-bound integer work: coalesced 4/8-byte streams, LDS staging for
// the scatter, wave64 ballots for ranking and for the extension walk.  No MFMA by design.
#include "common.hpp"
#include "dev_scan.hpp"
#include "radix_sort.hpp"
#include "seed_dev.hpp"
#include <algorithm>
#include <cstring>
#include <cstdlib>
#include <type_traits>

// ------------------------------------------------------------------------------------------------
// seed_extract: one thread per window.  Reads 0.25 B/position (L1-shared), writes key + val.
// val = global window index | strand << 31.
// ------------------------------------------------------------------------------------------------
// Segmented mode (recursive anchoring): genome g is a concatenation of nseg gap
// sub-sequences; seg[g*(nseg+1)+k] is the first base of segment k.  A window is valid only inside one
// segment and its key is prefixed with the segment id, so mers only meet inside their own gap; invalid
// windows get the all-ones key, which the join ignores.
__device__ __forceinline__ uint32_t seg_of(const uint32_t *__restrict__ segs, uint32_t nseg, uint32_t p)
{
    uint32_t lo = 0, hi = nseg;            // segs[lo] <= p < segs[hi]
    while (hi - lo > 1) { uint32_t mid = (lo + hi) >> 1; if (segs[mid] <= p) lo = mid; else hi = mid; }
    return lo;
}
// the segment rule: does the window at base p of genome g lie inside one segment?  *id: the segment p is in (it rides above the mer in the key)
__device__ __forceinline__ bool window_segment(const uint32_t *__restrict__ seg, uint32_t nseg, int g, uint32_t p, int span, uint32_t *id)
{
    const uint32_t *sg = seg + (size_t)g * (nseg + 1);
    const uint32_t k = *id = seg_of(sg, nseg, p);
    return p + span <= sg[k + 1];
}

template <typename KeyT, bool SEG, typename ValT = uint32_t>
__global__ void __launch_bounds__(256) seed_extract(const uint64_t *__restrict__ packed, GenomeTab tab,
                                                    SeedShape sh, int g, KeyT *__restrict__ keys,
                                                    ValT *__restrict__ vals, uint32_t out_base,
                                                    const uint32_t *__restrict__ seg, uint32_t nseg)
{
    const uint32_t n = tab.nwin[g], goff = tab.gpos_off[g];
    const uint64_t *G = packed + tab.word_off[g];
    const SeedRuns<false> runs(sh);
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        const MerKey m = mer_at<false>(G, p, runs);
        uint64_t key = m.key;
        if (SEG) {
            uint32_t k;
            key = window_segment(seg, nseg, g, p, sh.span, &k) ? (((uint64_t)k << (2 * sh.weight)) | key) : ~0ULL;
        }
        keys[out_base + p] = (KeyT)key;
        vals[out_base + p] = win_make<ValT>(goff + p, m.strand);
    }
}

// All genomes in one launch, tiled exactly like the radix sort (4096 windows per workgroup), with the digit
// histogram of the first sort pass accumulated on the way out: saves two launches and one re-read of the keys.
// sbits != nullptr: no value array.  A window's value is its own index plus its strand bit, and the index is where the key lies: the
// workgroup writes the strand bits of its tile instead (bit gp of a bitmap of 64-bit words, here as 32-bit halves; all 128 halves of the
// tile, zero at and behind P) and the first sort pass makes the values from them (rs_scatter IOTA) -- 1/8 byte per window stored
// instead of 4 or 8, and nothing for that pass to read back but the bits.
template <typename KeyT, bool SEG, bool NARROW, typename ValT = uint32_t>
__global__ void __launch_bounds__(256) seed_extract_all(const uint64_t *__restrict__ packed, GenomeTab tab, SeedShape sh,
                                                        KeyT *__restrict__ keys, ValT *__restrict__ vals, uint32_t P,
                                                        const uint32_t *__restrict__ seg, uint32_t nseg,
                                                        uint32_t *__restrict__ hist, uint32_t nblk,
                                                        const uint64_t *__restrict__ vmask, int hist_shift,
                                                        const uint64_t *__restrict__ cmask, uint32_t *__restrict__ sbits)
{
    // A thread takes FOUR CONSECUTIVE windows at a time (four such groups: 4096 windows per workgroup, the sort's tile): their bases come from the
    // same three or four packed words (one set of loads instead of four), and the keys and values leave as 16-byte stores.  With one window per
    // thread and 4-byte stores the kernel ran at 1.6 TB/s, waiting on its own store issue (wait share 0.71), not on the arithmetic.
    __shared__ uint32_t h[256];
    __shared__ uint32_t sb[4096 / 32];
    h[threadIdx.x] = 0;
    if (threadIdx.x < 4096 / 32) sb[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * 4096u;
    const SeedRuns<NARROW> runs(sh);
#pragma unroll 2
    for (int i = 0; i < 4; i++) {
        const uint32_t gp0 = base + i * 1024 + threadIdx.x * 4;
        if (gp0 >= P) break;
        const GenomeAt at0 = genome_at(gp0, tab);
        const int g0 = at0.g;
        const bool together = gp0 + 3 < P && gp0 + 3 < at0.hi;                        // all four in the buffer and in one genome
        uint64_t key[4]; uint32_t sf[4];
        if (together) {
            const uint32_t p0 = gp0 - at0.lo;
            const uint64_t *G = packed + at0.word;
            const uint32_t q = p0 >> 5; const int r0 = (p0 & 31) * 2;                 // p0 is a multiple of 4 only relative to gp0: r0 is any even offset
            const uint64_t w0 = G[q], w1 = G[q + 1], w2 = G[q + 2], w3 = NARROW ? 0ULL : G[q + 3];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int r = r0 + 2 * j;                                             // 0 .. 68
                uint64_t a0 = w0, a1 = w1, a2 = w2; int rr = r;
                if (r >= 64) { a0 = w1; a1 = w2; a2 = w3; rr = r - 64; }
                const MerKey m = canonical_mer<NARROW>({funnel64(a0, a1, rr), NARROW ? 0ULL : funnel64(a1, a2, rr)}, runs);
                key[j] = m.key; sf[j] = m.strand;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t gp = gp0 + j;
                key[j] = ~0ULL; sf[j] = 0;
                if (gp >= P) continue;
                const GenomeAt at = genome_at(gp, tab);
                const MerKey m = mer_at<NARROW>(packed + at.word, gp - at.lo, runs);
                key[j] = m.key; sf[j] = m.strand;
            }
        }
        if (SEG || vmask || cmask) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t gp = gp0 + j;
                if (gp >= P) continue;
                const int g = together ? g0 : genome_of(gp, tab);
                const uint32_t p = gp - tab.gpos_off[g];
                if (SEG) {
                    uint32_t k;
                    key[j] = window_segment(seg, nseg, g, p, sh.span, &k) ? (((uint64_t)k << (2 * sh.weight)) | key[j]) : ~0ULL;
                }
                if ((vmask || cmask) && window_blocked(vmask ? vmask + tab.mask_off[g] : nullptr, cmask ? cmask + tab.mask_off[g] : nullptr, p, sh.span)) key[j] = ~0ULL;
            }
        }
        // (a thread's four windows are one nibble of a bitmap half: gp0 - base is a multiple of 4; sf is 0 at and behind P)
        if (sbits) atomicOr(&sb[(gp0 - base) >> 5], (sf[0] | sf[1] << 1 | sf[2] << 2 | sf[3] << 3) << ((gp0 - base) & 31u));
        if (gp0 + 3 < P) {
            if (sizeof(KeyT) == 4) *reinterpret_cast<uint4 *>(keys + gp0) = make_uint4((uint32_t)key[0], (uint32_t)key[1], (uint32_t)key[2], (uint32_t)key[3]);
            else {
                reinterpret_cast<ulonglong2 *>(keys + gp0)[0] = make_ulonglong2(key[0], key[1]);
                reinterpret_cast<ulonglong2 *>(keys + gp0)[1] = make_ulonglong2(key[2], key[3]);
            }
            if (sbits) {}
            else if constexpr (sizeof(ValT) == 4)
                *reinterpret_cast<uint4 *>(vals + gp0) = make_uint4(gp0 | (sf[0] << 31), (gp0 + 1) | (sf[1] << 31), (gp0 + 2) | (sf[2] << 31), (gp0 + 3) | (sf[3] << 31));
            else {
                reinterpret_cast<ulonglong2 *>(vals + gp0)[0] = make_ulonglong2(win_make<ValT>(gp0, sf[0]), win_make<ValT>(gp0 + 1, sf[1]));
                reinterpret_cast<ulonglong2 *>(vals + gp0)[1] = make_ulonglong2(win_make<ValT>(gp0 + 2, sf[2]), win_make<ValT>(gp0 + 3, sf[3]));
            }
#pragma unroll
            for (int j = 0; j < 4; j++) atomicAdd(&h[(uint32_t)((KeyT)key[j] >> hist_shift) & 255u], 1u);
        } else {
            for (int j = 0; j < 4 && gp0 + j < P; j++) {
                keys[gp0 + j] = (KeyT)key[j];
                if (!sbits) vals[gp0 + j] = win_make<ValT>(gp0 + j, sf[j]);
                atomicAdd(&h[(uint32_t)((KeyT)key[j] >> hist_shift) & 255u], 1u);
            }
        }
    }
    __syncthreads();
    hist[threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
    if (sbits && threadIdx.x < 4096 / 32) sbits[(size_t)blockIdx.x * (4096 / 32) + threadIdx.x] = sb[threadIdx.x];
}

// ------------------------------------------------------------------------------------------------
// Masked seed passes (guide-tree nodes below the root, LCB extension): most windows touch a masked base and
// would only be carried through the sort as dead all-ones keys.  Instead the valid windows are compacted, in
// position order (so equal mers still arrive in ascending position, as the join expects): count per tile,
// one-block scan over the tiles, then an extract that writes each tile's valid (key, val) pairs at the tile's
// offset.  A thread owns 16 consecutive windows, so one block scan of per-thread counts gives the order.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool window_valid(uint32_t gp, uint32_t P, const GenomeTab &tab, int span, const uint64_t *__restrict__ vmask,
                                             const uint64_t *__restrict__ cmask)
{
    if (gp >= P) return false;
    const int g = genome_of(gp, tab);
    return !window_blocked(vmask ? vmask + tab.mask_off[g] : nullptr, cmask ? cmask + tab.mask_off[g] : nullptr, gp - tab.gpos_off[g], span);
}

__global__ void __launch_bounds__(256) valid_count(GenomeTab tab, int span, uint32_t P, const uint64_t *__restrict__ vmask,
                                                   uint32_t *__restrict__ tile_cnt, const uint64_t *__restrict__ cmask)
{
    __shared__ uint32_t lds[8];
    const uint32_t first = blockIdx.x * 4096u + threadIdx.x * 16u;
    uint32_t c = 0;
    for (int i = 0; i < 16; i++) c += window_valid(first + i, P, tab, span, vmask, cmask) ? 1u : 0u;
    uint32_t total;
    (void)block_excl_scan(c, &total, lds);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// exclusive scan of tile_cnt[0..nblk) in place, total -> *total_out (one workgroup)
__global__ void __launch_bounds__(256) tile_scan(uint32_t *__restrict__ tile_cnt, uint32_t nblk, uint32_t *__restrict__ total_out)
{
    __shared__ uint32_t lds[8];
    const uint32_t chunk = (nblk + 255) / 256, lo = threadIdx.x * chunk, hi = min(lo + chunk, nblk);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; i++) sum += tile_cnt[i];
    uint32_t total;
    uint32_t run = block_excl_scan(sum, &total, lds);
    for (uint32_t i = lo; i < hi; i++) { const uint32_t v = tile_cnt[i]; tile_cnt[i] = run; run += v; }
    if (threadIdx.x == 0) *total_out = total;
}

template <typename KeyT, bool NARROW, typename ValT = uint32_t>
__global__ void __launch_bounds__(256) seed_extract_compact(const uint64_t *__restrict__ packed, GenomeTab tab, SeedShape sh,
                                                            KeyT *__restrict__ keys, ValT *__restrict__ vals, uint32_t P,
                                                            const uint64_t *__restrict__ vmask, const uint32_t *__restrict__ tile_off,
                                                            const uint64_t *__restrict__ cmask)
{
    __shared__ uint32_t lds[8];
    const uint32_t first = blockIdx.x * 4096u + threadIdx.x * 16u;
    uint32_t ok = 0;
    for (int i = 0; i < 16; i++) ok |= (window_valid(first + i, P, tab, sh.span, vmask, cmask) ? 1u : 0u) << i;
    uint32_t total;
    uint32_t o = tile_off[blockIdx.x] + block_excl_scan((uint32_t)__popc(ok), &total, lds);
    const SeedRuns<NARROW> runs(sh);
    for (int i = 0; i < 16; i++) {
        if (!(ok >> i & 1)) continue;
        const uint32_t gp = first + i;
        const GenomeAt at = genome_at(gp, tab);
        const MerKey m = mer_at<NARROW>(packed + at.word, gp - at.lo, runs);
        keys[o] = (KeyT)m.key; vals[o] = win_make<ValT>(gp, m.strand);
        o++;
    }
}

// ------------------------------------------------------------------------------------------------
// mum_join: one thread per sorted entry; the thread at the first entry of a run of identical mers decides
// the hit by the finder's rule and scatters the hit into the dense HIT TABLE, indexed by the global
// window index of the hit's anchor (lowest genome of its component set):
//   tmask[p]    = component set (0 = no hit anchored at p)
//   tpos[p*N+g] = component g's window: global index | strand << 31, local to genome g in a wide pass (hit_word)   (one record of N words per anchor:
//                 a hit is written, and later read, as one contiguous record instead of N scattered words)
//   MODE_MEM    : MemHash -- a genome with more than one copy kills the seed
//   MODE_UNIQUE : UniqueMatchFinder.cpp:44-58 -- genomes with more than one copy are dropped, >= 2 stay
// A position carries at most one mer, so at most one hit is anchored at it: no atomics, no compaction.
// ------------------------------------------------------------------------------------------------
// the finder's rule for one mer: once / multi = the genomes that hold it at all / more than once.  The component set, or 0 for no hit
__device__ __forceinline__ uint32_t finder_components(int mode, uint32_t once, uint32_t multi, uint32_t want_mask)
{
    const uint32_t m = once & ~multi;
    const bool repeat_kills = (mode == MAUVE_MODE_MEM) & (multi != 0), too_few = __popc(m) < 2, other_set = (want_mask != 0) & (m != want_mask);
    return (repeat_kills | too_few | other_set) ? 0u : m;      // (no short circuit: the joins apply the rule to a dozen rows without a branch)
}
// entry i of a sorted list of n entries (the whole list, or one slice join_hash handed back)
template <typename KeyT, bool SEG, typename ValT>
__device__ __forceinline__ void mum_join_at(const KeyT *__restrict__ keys, const ValT *__restrict__ vals, uint32_t n, uint32_t i,
                                            const GenomeTab &tab, int mode, uint32_t want_mask, uint32_t consider,
                                            uint32_t *__restrict__ tmask, uint32_t *__restrict__ tpos, int has_invalid)
{
    const KeyT k = keys[i];
    if ((SEG || has_invalid) && k == (KeyT)~0ULL) return;
    if (i > 0 && keys[i - 1] == k) return;
    if (i + 1 >= n || keys[i + 1] != k) return;        // singleton run
    // `consider` restricts the finder to a subset of the genomes (PairwiseMatchFinder: one pair at a time);
    // entries of the other genomes are invisible to it
    uint32_t once = 0, multi = 0, j = i;
    while (j < n && keys[j] == k) {
        uint32_t bit = (1u << genome_of(win_idx(vals[j]), tab)) & consider;
        multi |= once & bit; once |= bit; j++;
        if (mode == MAUVE_MODE_MEM && multi) return;   // MemHash: a repeat kills the seed, no need to finish the run
    }
    const uint32_t m = finder_components(mode, once, multi, want_mask);
    if (!m) return;
    // entries of a run are in ascending global position (stable sort), so the anchor comes first
    uint32_t ap = 0xFFFFFFFFu;
    for (uint32_t t = i; t < j; t++) {
        const ValT v = vals[t]; const uint32_t gp = win_idx(v);
        const int g = genome_of(gp, tab);
        if (!(m >> g & 1)) continue;
        if (ap == 0xFFFFFFFFu) { ap = gp; tmask[ap] = m; }
        tpos[(size_t)ap * tab.nseq + g] = hit_word(v, tab.gpos_off[g]);
    }
}
template <typename KeyT, bool SEG, typename ValT = uint32_t>
__global__ void __launch_bounds__(256) mum_join(const KeyT *__restrict__ keys, const ValT *__restrict__ vals,
                                                uint32_t n, GenomeTab tab, int mode, uint32_t want_mask,
                                                uint32_t consider, uint32_t *__restrict__ tmask,
                                                uint32_t *__restrict__ tpos, uint32_t P, int has_invalid)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    mum_join_at<KeyT, SEG, ValT>(keys, vals, n, i, tab, mode, want_mask, consider, tmask, tpos, has_invalid);
}
// The slices join_hash handed back, all in one launch: thread t of the concatenated slices takes entry t - pre[q] of slice q (pre: running
// slice lengths, nsl + 1 of them; lo: slice starts in the list).  A launch per slice ran the slices one after the other, and the head of a
// run of millions of copies of one mer (a satellite repeat: UNIQUE and the pairwise finder walk the whole run) walks for seconds -- side by
// side their walks overlap.
template <typename KeyT, bool SEG, typename ValT = uint32_t>
__global__ void __launch_bounds__(256) mum_join_slices(const KeyT *__restrict__ keys, const ValT *__restrict__ vals,
                                                       const uint32_t *__restrict__ lo, const uint32_t *__restrict__ pre, uint32_t nsl,
                                                       GenomeTab tab, int mode, uint32_t want_mask, uint32_t consider,
                                                       uint32_t *__restrict__ tmask, uint32_t *__restrict__ tpos, int has_invalid)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= pre[nsl]) return;
    uint32_t a = 0, b = nsl;                           // pre[a] <= t < pre[b]
    while (b - a > 1) { const uint32_t m = (a + b) >> 1; if (pre[m] <= t) a = m; else b = m; }
    mum_join_at<KeyT, SEG, ValT>(keys + lo[a], vals + lo[a], pre[a + 1] - pre[a], t - pre[a], tab, mode, want_mask, consider, tmask, tpos, has_invalid);
}

// ------------------------------------------------------------------------------------------------
// join_hash: the finder rule without a full sort.  The (mer, position) pairs are radix-sorted on their HIGH bits
// only (bits [L, key_bits): as many 8-bit passes as bring the average bucket -- entries sharing those bits -- down to
// a few hundred); every occurrence of a mer then lies in one bucket, and a workgroup groups the mers of a range of
// whole buckets in an LDS hash table instead of ordering them: the finder rules only ask, per distinct mer, which
// genomes hold it once and which more than once -- the order of the mers is irrelevant, and the anchor (lowest genome
// of the component set) is found by genome id, not by position.  Two 8-bit passes and the join's read replace four
// passes, three histogram sweeps and a join that walked every run serially (C2: 30-bit mers, 15 M windows).
//
// Workgroup c owns [bound(c), bound(c+1)) -- the buckets that start in its chunk; bound(c) = first bucket boundary at
// or after c*HJ_T (chunk_bound; two waves look the two edges up side by side).  A range longer than the
// HJ_CAP entries its table takes (a bucket blown up by a repeat family or low-complexity sequence) is not processed:
// it goes to the overflow list and the host gives that slice to the full sort and the serial join below
// (rs_* of radix_sort.hip + mum_join), which have no size limit.
// Slot = {mer (later the anchor's value), once | multi << 16 genome sets}; 4096 slots, at most 3072 entries (load <= 0.75).
// ------------------------------------------------------------------------------------------------
constexpr int HJ_T = 2048;                   // nominal entries per workgroup
constexpr int HJ_ROWS = 12;                  // rows of 256 entries a workgroup can take
constexpr int HJ_CAP = HJ_ROWS * 256;        // 3072
constexpr int HJ_SLOTS = 4096;
static_assert(HJ_CAP * 4 <= 3 * HJ_SLOTS, "join_hash: table load factor above 0.75");
constexpr uint32_t HJ_NONE = 0xffffffffu;
constexpr int HJ_OVF_CAP = 4096;            // ranges the overflow list holds; beyond that the whole list goes the old way

// first bucket boundary at or after chunk edge c (wave-uniform result): 64 entries per probe, a binary search (the
// list is ordered by the high bits) when a bucket is long
template <typename KeyT>
__device__ __forceinline__ uint32_t chunk_bound(const KeyT *__restrict__ keys, uint32_t n, int L, uint32_t c, int lane)
{
    const uint32_t start = c * (uint32_t)HJ_T;
    if (c == 0) return 0u;
    if (start >= n) return n;
    // 256 entries, 64 per probe, in two steps: the first probe together with the edge's own entry, then -- no boundary there -- the loads of
    // the other three together (a bucket of a few hundred entries has its boundary two or three probes out: one probe after the other, that
    // was as many dependent round trips).  An index at or past n is clamped for the load and counts as a boundary; the first boundary in
    // probe order is taken.  (All four at once costs the lists with short buckets three probes of traffic they never look at: measured,
    // profiles/run_tiles_summary.md.)
    auto probe = [&](int step, KeyT k, uint64_t h0) -> uint32_t {
        const uint32_t idx = start + (uint32_t)step * 64u + (uint32_t)lane;
        const uint64_t b = __ballot(idx >= n || ((uint64_t)k >> L) != h0);
        return b ? start + (uint32_t)step * 64u + (uint32_t)(__ffsll((unsigned long long)b) - 1) : HJ_NONE;
    };
    const KeyT k0 = keys[min(start + (uint32_t)lane, n - 1u)];
    const uint64_t h0 = (uint64_t)keys[start - 1] >> L;                  // the bucket the edge falls into (or just behind)
    uint32_t res = probe(0, k0, h0);
    if (res == HJ_NONE) {
        KeyT k[4];
#pragma unroll
        for (int step = 1; step < 4; step++) k[step] = keys[min(start + (uint32_t)step * 64u + (uint32_t)lane, n - 1u)];
#pragma unroll
        for (int step = 3; step >= 1; step--) {
            const uint32_t r = probe(step, k[step], h0);
            if (r != HJ_NONE) res = r;
        }
    }
    if (res == HJ_NONE) {
        // long bucket: first index in (lo, hi] whose high bits differ (keys[lo] still belongs to the bucket, index n counts)
        uint32_t lo = start + 255u, hi = n;
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (((uint64_t)keys[mid] >> L) != h0) hi = mid; else lo = mid;
        }
        res = hi;
    }
    return min(res, n);
}

template <typename KeyT>
__global__ void __launch_bounds__(256) join_bounds(const KeyT *__restrict__ keys, uint32_t n, int L, uint32_t nchunk,
                                                   uint32_t *__restrict__ bound)
{
    const uint32_t c = (blockIdx.x * 256u + threadIdx.x) >> 6;           // one wave per chunk edge 0 .. nchunk
    if (c > nchunk) return;
    const uint32_t res = chunk_bound(keys, n, L, c, threadIdx.x & 63);
    if ((threadIdx.x & 63) == 0) bound[c] = res;
}

// Grouping by mer in an LDS table of SLOTS slots (join_hash, tiny_join).  group_claim: the key's slot, claimed from slot s on (compare-and-swap
// on the key word, linear probing).  group_note: OR the entry's genome bit into that slot's once / multi sets; multi is the high half of som's
// word, or -- WIDE, more than 16 genomes -- the word of som2.  (Two steps: join_hash takes the genome from the entry's value between
// them, so the wait for that load stays behind the claim loop.)
template <typename KeyT, int SLOTS>
__device__ __forceinline__ uint32_t group_claim(KeyT *skey, KeyT key, uint32_t s)
{
    constexpr KeyT EMPTY = (KeyT)~0ULL;
    for (;;) {
        const KeyT old = atomicCAS(&skey[s], EMPTY, key);
        if (old == EMPTY || old == key) break;
        s = (s + 1) & (SLOTS - 1);
    }
    return s;
}
template <bool WIDE>
__device__ __forceinline__ void group_note(uint32_t *som, uint32_t *som2, uint32_t s, uint32_t bit)
{
    const uint32_t old = atomicOr(&som[s], bit);
    if (old & bit) { if (WIDE) atomicOr(&som2[s], bit); else atomicOr(&som[s], bit << 16); }
}

// (ValT = uint64_t: the values ride in registers only -- the slot that takes the anchor gets its window INDEX, which fits the key word --
// so the LDS table is the narrow pass's)
template <typename KeyT, bool WIDE, typename ValT = uint32_t>
__global__ void __launch_bounds__(256) join_hash(const KeyT *__restrict__ keys, const ValT *__restrict__ vals, uint32_t n,
                                                 const uint32_t *__restrict__ bound, GenomeTab tab, int mode, uint32_t want_mask,
                                                 uint32_t *__restrict__ tmask, uint32_t *__restrict__ tpos,
                                                 uint32_t *__restrict__ ovf_cnt, uint32_t *__restrict__ ovf, uint32_t P)
{
    __shared__ KeyT skey[HJ_SLOTS];
    __shared__ uint32_t som[HJ_SLOTS];                       // once (low half) | multi (high half); WIDE: once only
    __shared__ uint32_t som2[WIDE ? HJ_SLOTS : 1];           // WIDE (> 16 genomes): multi
    constexpr KeyT EMPTY = (KeyT)~0ULL;                       // never a canonical mer; also the invalid-window key
    const int tid = threadIdx.x;
    const uint32_t cs = blockIdx.x * (uint32_t)HJ_T;
    // the rows sit at fixed places (cs + r*256 + tid), so their loads do not wait for the range: the first nine go out
    // at once; the range only decides which entries take part
    KeyT k[HJ_ROWS]; ValT v[HJ_ROWS];
#pragma unroll
    for (int r = 0; r <= HJ_T / 256; r++) {
        const uint32_t idx = cs + (uint32_t)r * 256u + (uint32_t)tid;
        k[r] = idx < n ? keys[idx] : EMPTY; v[r] = idx < n ? vals[idx] : (ValT)0;
    }
    for (int i = tid; i < HJ_SLOTS; i += 256) { skey[i] = EMPTY; som[i] = 0; if (WIDE) som2[i] = 0; }
    __syncthreads();
    const uint32_t lo = bound[blockIdx.x], hi = bound[blockIdx.x + 1];
    if (lo >= hi) return;                                     // no bucket starts in this chunk
    if (hi > cs + (uint32_t)HJ_CAP) {                         // oversize: hand the range to the host
        if (tid == 0) {
            const uint32_t o = atomicAdd(&ovf_cnt[0], 1u);
            if (o < (uint32_t)HJ_OVF_CAP) { ovf[2 + 2 * o] = lo; ovf[3 + 2 * o] = hi; }
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < HJ_ROWS; r++) {
        const uint32_t idx = cs + (uint32_t)r * 256u + (uint32_t)tid;
        if (r > HJ_T / 256) {                                 // rows the range rarely reaches
            k[r] = EMPTY; v[r] = (ValT)0;
            if (cs + (uint32_t)r * 256u < hi && idx < hi) { k[r] = keys[idx]; v[r] = vals[idx]; }
        }
        if (idx < lo || idx >= hi) k[r] = EMPTY;
    }
    // ---- pass 1: group by mer (group_claim, group_note) ----
    uint32_t slot[HJ_ROWS]; uint32_t gbit[HJ_ROWS];
#pragma unroll
    for (int r = 0; r < HJ_ROWS; r++) {
        slot[r] = HJ_NONE; gbit[r] = 0;
        if (k[r] == EMPTY) continue;                          // beyond the range, or an invalid window
        const uint32_t s = ((uint32_t)k[r] ^ (uint32_t)((uint64_t)k[r] >> 32)) * 0x9E3779B1u >> 20;       // 12 bits
        slot[r] = group_claim<KeyT, HJ_SLOTS>(skey, k[r], s);
        gbit[r] = 1u << genome_of(win_idx(v[r]), tab);
        group_note<WIDE>(som, som2, slot[r], gbit[r]);
    }
    __syncthreads();
    // ---- pass 2: the finder rule per mer; the entry of the lowest component genome is the anchor ----
    uint32_t mm[HJ_ROWS];
#pragma unroll
    for (int r = 0; r < HJ_ROWS; r++) {
        mm[r] = 0;
        if (slot[r] == HJ_NONE) continue;
        const uint32_t om = som[slot[r]];
        const uint32_t once = WIDE ? om : (om & 0xffffu), multi = WIDE ? som2[slot[r]] : (om >> 16);
        const uint32_t m = finder_components(mode, once, multi, want_mask);
        if (!(m & gbit[r])) continue;
        mm[r] = m;
        if ((m & (0u - m)) == gbit[r]) skey[slot[r]] = sizeof(ValT) == 4 ? (KeyT)v[r] : (KeyT)win_idx(v[r]);   // grouping is over: the slot's mer makes room for the anchor
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < HJ_ROWS; r++) {
        if (!mm[r]) continue;
        const uint32_t ap = sizeof(ValT) == 4 ? (uint32_t)skey[slot[r]] & 0x7fffffffu : (uint32_t)skey[slot[r]];
        if (ap >= P) { atomicAdd(&ovf_cnt[1], 1u); continue; }   // cannot happen; a wild store could take the device down
        const int g = __ffs(gbit[r]) - 1;
        tpos[(size_t)ap * tab.nseq + g] = hit_word(v[r], tab.gpos_off[g]);
        if ((mm[r] & (0u - mm[r])) == gbit[r]) tmask[ap] = mm[r];
    }
}

// What a finder pass clears before its join, in one launch instead of two fills: the n words from t (its range of the hit table) and the
// pass's counter block of 16 words.  A thread takes the four words of one 16-byte line of t, those outside [t, t + n) left alone.
__global__ void __launch_bounds__(256) pass_clear(uint32_t *__restrict__ t, uint32_t n, uint32_t *__restrict__ counters)
{
    if (blockIdx.x == 0 && threadIdx.x < 16) counters[threadIdx.x] = 0;
    const uint32_t head = (uint32_t)((reinterpret_cast<uintptr_t>(t) >> 2) & 3u);          // words between the line's start and t
    const uint64_t w = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 4u;                    // first word of this thread's line, from t - head
    if (w >= (uint64_t)head + n) return;
    uint32_t *line = t - head + w;
    if (w >= head && w + 4 <= (uint64_t)head + n) *reinterpret_cast<uint4 *>(line) = make_uint4(0u, 0u, 0u, 0u);
    else for (uint32_t j = 0; j < 4; j++) if (w + j >= head && w + j < (uint64_t)head + n) line[j] = 0;
}

// hits found by a host-side finder (mauve_extend_hits): record h = {component set, value of genome 0 .. N-1} -> hit table
// ---- tiny passes: extract + group + rule in ONE workgroup ------------------------------------------------------------------
// A seed pass over a few thousand windows (a round of the LCB extension over the pieces between the LCBs, a small guide-tree
// node) spends its time in launches: count, scan, extract, four sort passes, bounds, join -- a dozen kernels of 5-20 us each
// for a few kilobytes.  Here one workgroup of 1024 threads computes the canonical mers of ALL valid windows, groups them in an
// LDS hash table (group_claim / group_note: join_hash's once / multi genome sets; then finder_components, the rule every join applies)
// and writes the hit table -- no key array, no sort.  <= TJ_MAX windows, <= 16 genomes, mer (+ gap id of a segmented
// set: the small batches of the deeper recursion levels) of <= 32 bits.
constexpr int TJ_SLOTS = 16384;                  // 128 KB of LDS: key word + genome sets per slot
constexpr int TJ_MAX = 9216;                     // load factor <= 0.5625
constexpr int TJ_ROWS = TJ_MAX / 1024;
constexpr uint32_t TJ_EMPTY = 0xffffffffu;       // never a canonical mer (the smaller of a mer and its reverse complement)
// the thread's windows, one per row: key (TJ_EMPTY: no valid window), hit-table word and genome bit
template <bool LOCAL, bool NARROW>
__device__ __forceinline__ void tiny_extract(const uint64_t *__restrict__ packed, const GenomeTab &tab, const SeedShape &sh, uint32_t P,
                                             const uint64_t *__restrict__ vmask, const uint64_t *__restrict__ cmask, const uint32_t *__restrict__ seg,
                                             uint32_t nseg, int tid, uint32_t (&key)[TJ_ROWS], uint32_t (&v)[TJ_ROWS], uint32_t (&gbit)[TJ_ROWS])
{
    const SeedRuns<NARROW> runs(sh);
#pragma unroll
    for (int r = 0; r < TJ_ROWS; r++) {
        const uint32_t gp = (uint32_t)r * 1024u + (uint32_t)tid;
        key[r] = TJ_EMPTY; v[r] = 0; gbit[r] = 0;
        if (gp >= P) continue;
        const GenomeAt at = genome_at(gp, tab);
        const int g = at.g;
        const uint32_t p = gp - at.lo;
        if (window_blocked(vmask ? vmask + tab.mask_off[g] : nullptr, cmask ? cmask + tab.mask_off[g] : nullptr, p, sh.span)) continue;      // (window_valid, the genome looked up once)
        const MerKey m = mer_at<NARROW>(packed + at.word, p, runs);
        uint32_t k = (uint32_t)m.key;
        if (seg) {                                  // segmented set (a batch of recursion gaps): the gap id rides above the mer, no window across gaps
            uint32_t sk;
            if (!window_segment(seg, nseg, g, p, sh.span, &sk)) continue;
            k |= sk << (2 * sh.weight);
        }
        key[r] = k; v[r] = (LOCAL ? p : gp) | (m.strand << 31); gbit[r] = 1u << g;
    }
}
template <bool LOCAL = false>
__global__ void __launch_bounds__(1024) tiny_join(const uint64_t *__restrict__ packed, GenomeTab tab, SeedShape sh, uint32_t P,
                                                  const uint64_t *__restrict__ vmask, const uint64_t *__restrict__ cmask, int mode, uint32_t want_mask,
                                                  uint32_t *__restrict__ tmask, uint32_t *__restrict__ tpos, uint32_t *__restrict__ err_cnt,
                                                  const uint32_t *__restrict__ seg, uint32_t nseg, uint32_t *__restrict__ counters, uint32_t clr_lo, uint32_t clr_hi)
{
    extern __shared__ uint32_t tj_lds[];
    uint32_t *skey = tj_lds, *som = tj_lds + TJ_SLOTS;
    constexpr uint32_t EMPTY = TJ_EMPTY;
    const int tid = threadIdx.x;
    // the pass's clears, here instead of two 5 us fill launches: the counter block and the slice of the hit table (the barriers below order them
    // before this workgroup's own stores to the table)
    if (counters && tid < 16) counters[tid] = 0;
    for (uint32_t i = clr_lo + tid; i < clr_hi; i += 1024) tmask[i] = 0;
    for (int i = tid; i < TJ_SLOTS; i += 1024) { skey[i] = EMPTY; som[i] = 0; }
    uint32_t v[TJ_ROWS], slot[TJ_ROWS], gbit[TJ_ROWS], key[TJ_ROWS];
    // (one run table at a time: the two of them together do not fit the scalar registers)
    if (seed_narrow(sh)) tiny_extract<LOCAL, true>(packed, tab, sh, P, vmask, cmask, seg, nseg, tid, key, v, gbit);
    else tiny_extract<LOCAL, false>(packed, tab, sh, P, vmask, cmask, seg, nseg, tid, key, v, gbit);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TJ_ROWS; r++) {
        slot[r] = EMPTY;
        if (key[r] == EMPTY) continue;
        slot[r] = group_claim<uint32_t, TJ_SLOTS>(skey, key[r], (key[r] * 0x9E3779B1u) >> 18);          // 14 bits
        group_note<false>(som, nullptr, slot[r], gbit[r]);
    }
    __syncthreads();
    uint32_t mm[TJ_ROWS];
#pragma unroll
    for (int r = 0; r < TJ_ROWS; r++) {
        mm[r] = 0;
        if (slot[r] == EMPTY) continue;
        const uint32_t om = som[slot[r]], m = finder_components(mode, om & 0xffffu, om >> 16, want_mask);
        if (!(m & gbit[r])) continue;
        mm[r] = m;
        if ((m & (0u - m)) == gbit[r])                                 // grouping is over: the slot's mer makes room for the anchor
            skey[slot[r]] = LOCAL ? (v[r] & 0x7fffffffu) + tab.gpos_off[__ffs(gbit[r]) - 1] : v[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TJ_ROWS; r++) {
        if (!mm[r]) continue;
        const uint32_t ap = LOCAL ? skey[slot[r]] : skey[slot[r]] & 0x7fffffffu;
        if (ap >= P) { atomicAdd(err_cnt, 1u); continue; }     // cannot happen (the anchor is one of the group's own windows)
        tpos[(size_t)ap * tab.nseq + (__ffs(gbit[r]) - 1)] = v[r];
        if ((mm[r] & (0u - mm[r])) == gbit[r]) tmask[ap] = mm[r];
    }
}

// (LOCAL: a wide pass -- the records carry windows local to their genome, as the hit table does; the anchor's global index is rebuilt)
template <bool LOCAL = false>
__global__ void __launch_bounds__(256) hits_scatter(const uint32_t *__restrict__ rec, uint32_t nh, int N, uint32_t P,
                                                    uint32_t *__restrict__ tmask, uint32_t *__restrict__ tpos, GenomeTab tab)
{
    const uint32_t h = blockIdx.x * 256u + threadIdx.x;
    if (h >= nh) return;
    const uint32_t *r = rec + (size_t)h * (N + 1);
    const uint32_t m = r[0];
    const uint32_t ap = (r[1 + (__ffs(m) - 1)] & 0x7fffffffu) + (LOCAL ? tab.gpos_off[__ffs(m) - 1] : 0u);
    if (ap >= P) return;                                      // validated on the host; never a wild store
    tmask[ap] = m;
    for (int g = 0; g < N; g++) if (m >> g & 1) tpos[(size_t)ap * N + g] = r[1 + g];
}

// ------------------------------------------------------------------------------------------------
// PairwiseMatchFinder: N(N-1)/2 finder passes over ONE sorted mer list.  Instead of re-reading all P sorted entries
// per pair, one pass (run_summary) lists the runs of identical mers that could matter to any pair -- where the run
// starts, how long it is, which genomes occur in it exactly once -- and the join of a group of pairs (join_pair_group) walks that
// list: a run is a hit of pair (i, j) iff both genomes are in its exactly-once set (MemHash restricted to the two
// genomes: entries of the others are invisible to it).  The order of the list does not matter: hits go to the
// dense table by anchor position.
// ------------------------------------------------------------------------------------------------
template <typename KeyT, typename ValT = uint32_t>
__global__ void __launch_bounds__(256) run_summary(const KeyT *__restrict__ keys, const ValT *__restrict__ vals, uint32_t n,
                                                   GenomeTab tab, int has_invalid, uint32_t *__restrict__ rstart,
                                                   uint32_t *__restrict__ rlen, uint32_t *__restrict__ runiq,
                                                   uint32_t *__restrict__ counter, uint32_t cap)
{
    // 1024 entries per workgroup (four per thread, strided), one block scan and ONE global atomic per workgroup: with one atomic per
    // wave, 250 k of them on the same counter were the kernel's whole run time (2.9 ms for 16 M entries)
    __shared__ uint32_t lds[8];
    __shared__ uint32_t s_base;
    constexpr int ITEMS = 4;
    const uint32_t base = blockIdx.x * (256u * ITEMS);
    uint32_t uniq[ITEMS], len[ITEMS], cnt = 0;
#pragma unroll
    for (int it = 0; it < ITEMS; it++) {
        const uint32_t i = base + it * 256 + threadIdx.x;
        uniq[it] = 0; len[it] = 0;
        if (i < n) {
            const KeyT k = keys[i];
            const bool valid = !(has_invalid && k == (KeyT)~0ULL);
            if (valid && (i == 0 || keys[i - 1] != k) && i + 1 < n && keys[i + 1] == k) {
                uint32_t once = 0, multi = 0, j = i;
                while (j < n && keys[j] == k) {
                    const uint32_t bit = 1u << genome_of(win_idx(vals[j]), tab);
                    multi |= once & bit; once |= bit; j++;
                }
                uniq[it] = once & ~multi; len[it] = j - i;
            }
        }
        if (__popc(uniq[it]) >= 2) cnt++; else uniq[it] = 0;
    }
    uint32_t total;
    const uint32_t off = block_excl_scan(cnt, &total, lds);
    if (threadIdx.x == 0) s_base = total ? atomicAdd(counter, total) : 0u;
    __syncthreads();
    uint32_t r = s_base + off;
#pragma unroll
    for (int it = 0; it < ITEMS; it++)
        if (uniq[it]) { if (r < cap) { rstart[r] = base + it * 256 + threadIdx.x; rlen[r] = len[it]; runiq[r] = uniq[it]; } r++; }   // (the counter keeps counting: the host sees a list that outgrew its buffer)
}

// ------------------------------------------------------------------------------------------------
// SeedMatchEnumerator on the device (SeedMatchEnumerator.h:59-141): the sorted mer list of ONE sequence is cut into
// runs of identical mers; a run of m occurrences, min_multi <= m <= max_multi, becomes one match of m components in
// position order (the stable sort keeps them so), 1-based, a component negative when its strand flag differs from
// the first component's (SetDirection, :127-141); with direct_only a run that has reverse components keeps only the
// forward ones, if two or more remain (:88-117).  Output CSR: mult[r], start_off[r], starts[].
//   enum_runs  : the head of every run walks it and notes how many starts it will emit (0: no match)
//   vscan_*    : start offsets; cmp_* (EnumRuns): the emitting runs in list order -> mult / start_off
//   enum_write : the heads walk again and write the starts
// ------------------------------------------------------------------------------------------------
template <typename KeyT, typename ValT = uint32_t>
__global__ void __launch_bounds__(256) enum_runs(const KeyT *__restrict__ keys, const ValT *__restrict__ vals, uint32_t n, int64_t min_multi,
                                                 int64_t max_multi, int direct_only, uint32_t *__restrict__ emit)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const KeyT k = keys[i];
    uint32_t e = 0;
    if (i == 0 || keys[i - 1] != k) {
        const uint32_t ref = win_strand(vals[i]);
        uint32_t j = i, kept = 0; bool found_rev = false;
        while (j < n && keys[j] == k) { if (win_strand(vals[j]) != ref) found_rev = true; else kept++; j++; }
        const int64_t m = (int64_t)(j - i);
        if (m >= 2 && m >= min_multi && m <= max_multi) e = (direct_only && found_rev) ? (kept > 1 ? kept : 0u) : (uint32_t)m;
    }
    emit[i] = e;
}
struct EmitVal { const uint32_t *e; __device__ int64_t value(uint32_t i) const { return e[i]; } };
struct EnumRuns {
    const uint32_t *cnt; const int64_t *soff; uint32_t n; int64_t *mult, *start_off; int64_t *tot /* [0] runs, [1] starts */;
    __device__ uint32_t domain(int) const { return n; }
    __device__ bool flag(uint32_t i, int) const { return cnt[i] != 0; }
    __device__ void each(uint32_t, uint32_t, bool, int) const {}
    __device__ void emit(uint32_t i, uint32_t r, int) const { mult[r] = cnt[i]; start_off[r] = soff[i]; }
    __device__ void total(uint32_t runs, int) const { tot[0] = runs; start_off[runs] = soff[n]; }
};
template <typename KeyT, typename ValT = uint32_t>
__global__ void __launch_bounds__(256) enum_write(const KeyT *__restrict__ keys, const ValT *__restrict__ vals, uint32_t n, int direct_only,
                                                  const uint32_t *__restrict__ emit, const int64_t *__restrict__ soff, uint32_t gpos0,
                                                  int64_t *__restrict__ starts)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || emit[i] == 0) return;
    const KeyT k = keys[i];
    const uint32_t ref = win_strand(vals[i]);
    uint32_t j = i; bool found_rev = false;
    while (j < n && keys[j] == k) { if (win_strand(vals[j]) != ref) found_rev = true; j++; }
    int64_t o = soff[i];
    for (uint32_t t = i; t < j; t++) {
        const bool rv = win_strand(vals[t]) != ref;
        const int64_t p1 = (int64_t)(win_idx(vals[t]) - gpos0) + 1;
        if (direct_only && found_rev) { if (!rv) starts[o++] = p1; }
        else starts[o++] = rv ? -p1 : p1;
    }
}

// ------------------------------------------------------------------------------------------------
// extension.  A hit fixes a generalized diagonal: component c moves +k (same strand as the
// anchor) or -k (opposite strand) when the anchor moves +k.  Offset k "agrees" when the masked windows of
// all components are equal there.  Agreeing offsets at most `span` apart chain into a cluster; the match
// is the cluster through the hit, emitted by its leftmost same-mask hit.
// ------------------------------------------------------------------------------------------------
// (ExtComp, ext_mismatch, walk_round, ext_window_clean, ext_blocked: seed_dev.hpp)

// phase A (streaming, no genome access): one thread per window position.  A hit anchored at p that has a
// same-mask hit on the same diagonal at p-d, d <= span, cannot be the leftmost hit of its cluster (the
// left walk of S4 never jumps over an agreeing offset, and that hit agrees).  Everything else is a
// candidate for phase B.  all != 0 (no extension): every hit is a candidate.
// The windows a thread takes (ITEMS: 4, 8 or 16; a tile is 256 * ITEMS windows) are chosen per launch, runs_items below: a tile ends in one
// returning atomic on one counter, which the largest launches must keep rare, and the small ones need more workgroups than 4096 windows each give.
constexpr uint32_t RUNS_HALO = 64 /* >= MAUVE_MAX_SEED_SPAN */;
constexpr uint32_t runs_tile(int items) { return 256u * (uint32_t)items; }
static_assert(RUNS_HALO >= MAUVE_MAX_SEED_SPAN && RUNS_HALO == 64, "mum_runs looks back at most one span, and reads the mask word 64 positions in front of every lane");

// same generalized diagonal: every component of hit p sits d windows after (forward) / before (reverse) the
// corresponding component of hit q = p - d, with the same relative strands
__device__ __forceinline__ bool same_diagonal(const uint32_t *__restrict__ rp, const uint32_t *__restrict__ rq, uint32_t m, int a,
                                              int nseq, uint32_t d)
{
    const uint32_t sa = rp[a] >> 31, sq = rq[a] >> 31;
    for (int g = a + 1; g < nseq; g++) {
        if (!(m >> g & 1)) continue;
        const uint32_t vp = rp[g], vq = rq[g];
        const uint32_t o = (vp >> 31) ^ sa;
        if (((vq >> 31) ^ sq) != o) return false;
        const uint32_t pp = vp & 0x7fffffffu, pq = vq & 0x7fffffffu;
        if (!(o ? (pq == pp + d) : (pq + d == pp))) return false;
    }
    return true;
}

template <bool SEG, int RUNS_ITEMS>
__device__ __forceinline__ void mum_runs_body(const GenomeTab &tab, int span, const uint32_t *__restrict__ tmask,
                                              const uint32_t *__restrict__ tpos, uint32_t P, int all,
                                              uint32_t *__restrict__ cand, uint32_t *__restrict__ counters,
                                              const uint32_t *__restrict__ seg, uint32_t nseg, uint32_t p0, uint32_t cand_cap)
{
    static_assert(RUNS_ITEMS >= 1 && RUNS_ITEMS <= 32, "one bit per item in the hit / pending / flag words");
    constexpr uint32_t RUNS_TILE = runs_tile(RUNS_ITEMS);
    __shared__ uint32_t lds[8];
    __shared__ uint32_t s_base;
    __shared__ uint32_t s_mask[RUNS_HALO + RUNS_TILE];
    // RUNS_TILE windows per workgroup: one block scan and ONE global atomic per tile.  [p0, P): the positions looked at (a pass of
    // the pairwise finder only has hits in its lower genome)
    const uint32_t base = p0 + blockIdx.x * RUNS_TILE;
    const int N = tab.nseq;
    uint32_t flags = 0, cnt = 0;
    uint32_t mm[RUNS_ITEMS];
    uint32_t hits = 0;
#pragma unroll
    for (int it = 0; it < RUNS_ITEMS; it++) {
        const uint32_t p = base + it * 256 + threadIdx.x;
        mm[it] = p < P ? tmask[p] : 0u;
        if (mm[it]) hits |= 1u << it;
    }
    if (all) { flags = hits; cnt = __popc(hits); }
    else if (__syncthreads_or(hits != 0)) {
        // Three phases, each with all its memory operations in flight at once (a hit-by-hit walk with dependent loads is what this kernel used
        // to spend its time in): (1) the mask words of the tile (and RUNS_HALO words in front of it) in LDS: every hit finds the nearest
        // earlier position with the same mask inside its genome / gap segment, at most span away -- none: a candidate; (2) the records of the
        // hit and of that position, all items together: on the same diagonal, the hit is not the leftmost of its cluster; (3) the rare hit
        // whose nearest same-mask neighbour lies on ANOTHER diagonal walks on from there, one offset at a time.
#pragma unroll
        for (int it = 0; it < RUNS_ITEMS; it++) s_mask[RUNS_HALO + it * 256 + threadIdx.x] = mm[it];
        if (threadIdx.x < RUNS_HALO) {
            const int64_t q = (int64_t)base - RUNS_HALO + threadIdx.x;
            s_mask[threadIdx.x] = (q >= 0 && q < (int64_t)P) ? tmask[q] : 0u;
        }
        __syncthreads();
        // (phases 1 and 2 are written without per-lane branches: the exec-mask bookkeeping of sixteen unrolled items was what the scalar unit
        // -- one per compute unit -- spent the kernel on)
        const int lane = threadIdx.x & 63;
        uint32_t dd[RUNS_ITEMS];
        uint32_t pend = 0, any = 0;
#pragma unroll
        for (int it = 0; it < RUNS_ITEMS; it++) {
            dd[it] = 0;
            const uint32_t m = mm[it];
            uint64_t left = __ballot(m != 0);
            if (left == 0) continue;                          // (wave-uniform)
            const uint32_t p = base + it * 256 + threadIdx.x;
            const int a = m ? __ffs(m) - 1 : 0;
            uint32_t g0 = tab.gpos_off[a];
            if (SEG) { if (m) { const uint32_t *sg = seg + (size_t)a * (nseg + 1); g0 += sg[seg_of(sg, nseg, p - g0)]; } }
            const uint32_t lim = m ? min((uint32_t)span, p - g0) : 0u;
            // the nearest earlier position with the same mask, from ballots: one pair per distinct mask among the wave's hits (few), the 64
            // positions in front of a lane as one word with p - 1 at bit 63
            const uint32_t mprev = s_mask[RUNS_HALO + it * 256 + threadIdx.x - 64];
            uint32_t d = 0;
            while (left) {
                const uint32_t mv = (uint32_t)__builtin_amdgcn_readlane((int32_t)m, __ffsll((unsigned long long)left) - 1);
                const uint64_t Bc = __ballot(m == mv), Bp = __ballot(mprev == mv);
                left &= ~Bc;
                const uint64_t W = lane ? ((Bp >> lane) | (Bc << (64 - lane))) : Bp;
                const uint32_t dist = W ? (uint32_t)__clzll((long long)W) + 1u : 0u;
                d = m == mv ? dist : d;
            }
            const bool pd = d != 0 && d <= lim, cd = m != 0 && !pd;      // has such a neighbour / is a candidate already
            dd[it] = pd ? d : 0u;
            pend |= (pd ? 1u : 0u) << it; any |= pd ? m : 0u;
            flags |= (cd ? 1u : 0u) << it; cnt += cd ? 1u : 0u;
        }
        uint32_t sa_bits = 0, sq_bits = 0, bad = 0;
        // (32-bit offsets from a wave-uniform base keep the sixteen address pairs out of the register file)
        const uint32_t base_h = base >= RUNS_HALO ? base - RUNS_HALO : 0u;
        const uint32_t *tb = tpos + (size_t)base_h * N;
        constexpr int RB = RUNS_ITEMS < 8 ? RUNS_ITEMS : 8;   // items per batch of loads
#pragma unroll
        for (int i0 = 0; i0 < RUNS_ITEMS; i0 += RB) {
            if (!__any((pend >> i0) & ((1u << RB) - 1u))) continue;
            for (int g = 0; g < N; g++) {
                if (!__any((any >> g) & 1u)) continue;        // (wave-uniform: no pending hit of this wave has a component in genome g)
                uint32_t vp[RB], vq[RB];
#pragma unroll
                for (int i = 0; i < RB; i++) {                // (a lane with nothing to ask reads word 0 of the stretch: no branch)
                    const int it = i0 + i;
                    const uint32_t po = base - base_h + it * 256 + threadIdx.x;
                    const bool mine = ((pend >> it) & 1u) && ((mm[it] >> g) & 1u);
                    vp[i] = tb[mine ? po * (uint32_t)N + (uint32_t)g : 0u];
                    vq[i] = tb[mine ? (po - dd[it]) * (uint32_t)N + (uint32_t)g : 0u];
                }
#pragma unroll
                for (int i = 0; i < RB; i++) {
                    const int it = i0 + i;
                    const bool mine = ((pend >> it) & 1u) && ((mm[it] >> g) & 1u);
                    const bool first = g == __ffs(mm[it]) - 1;             // the anchor's component: its strands are the reference
                    sa_bits |= (mine && first) ? (vp[i] >> 31) << it : 0u; sq_bits |= (mine && first) ? (vq[i] >> 31) << it : 0u;
                    // same_diagonal(p, p - d), component g
                    const uint32_t o = (vp[i] >> 31) ^ ((sa_bits >> it) & 1u);
                    const uint32_t pp = vp[i] & 0x7fffffffu, pq = vq[i] & 0x7fffffffu;
                    const bool off = (((vq[i] >> 31) ^ ((sq_bits >> it) & 1u)) != o) || !(o ? (pq == pp + dd[it]) : (pq + dd[it] == pp));
                    bad |= (mine && !first && off) ? 1u << it : 0u;
                }
            }
        }
        const uint32_t again = pend & bad;
#pragma unroll
        for (int it = 0; it < RUNS_ITEMS; it++) {             // (unrolled: a run-time index would put mm / dd into scratch memory)
            if (!((again >> it) & 1u)) continue;
            const uint32_t p = base + it * 256 + threadIdx.x, m = mm[it];
            const int a = __ffs(m) - 1;
            uint32_t g0 = tab.gpos_off[a];
            if (SEG) { const uint32_t *sg = seg + (size_t)a * (nseg + 1); g0 += sg[seg_of(sg, nseg, p - g0)]; }
            const uint32_t *sm = s_mask + RUNS_HALO + it * 256 + threadIdx.x;
            const uint32_t lim = min((uint32_t)span, p - g0);
            bool is_cand = true;
            for (uint32_t d = dd[it] + 1; d <= lim && is_cand; d++) {
                if (sm[-(int)d] != m) continue;
                if (same_diagonal(tpos + (size_t)p * N, tpos + (size_t)(p - d) * N, m, a, N, d)) is_cand = false;
            }
            if (is_cand) { flags |= 1u << it; cnt++; }
        }
    }
    uint32_t total;
    const uint32_t off = block_excl_scan(cnt, &total, lds);
    if (threadIdx.x == 0) s_base = total ? atomicAdd(&counters[1], total) : 0u;
    __syncthreads();
    uint32_t o = s_base + off;
#pragma unroll
    for (int it = 0; it < RUNS_ITEMS; it++)
        if (flags >> it & 1) { if (o < cand_cap) cand[o] = base + it * 256 + threadIdx.x; o++; }     // never past the list: counters[1] still counts, the host refuses a list that outgrew its buffer
}
template <bool SEG, int ITEMS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) mum_runs(GenomeTab tab, int span, const uint32_t *__restrict__ tmask,
                                                const uint32_t *__restrict__ tpos, uint32_t P, int all,
                                                uint32_t *__restrict__ cand, uint32_t *__restrict__ counters,
                                                const uint32_t *__restrict__ seg, uint32_t nseg, uint32_t cand_cap, uint32_t p0 = 0)
{
    mum_runs_body<SEG, ITEMS>(tab, span, tmask, tpos, P, all, cand, counters, seg, nseg, p0, cand_cap);
}
// Several passes of the pairwise finder at once: pairs with DIFFERENT lower genomes write disjoint slices of the hit table, so a group of
// them shares the table, one candidate list and one counter (mum_extend tells the pairs apart by the hit's mask).  blockIdx.y = pair.
struct PairGroup { int n; int ga[MAUVE_MAX_SEQ], gb[MAUVE_MAX_SEQ]; uint32_t lo[MAUVE_MAX_SEQ], hi[MAUVE_MAX_SEQ]; };
template <int ITEMS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) mum_runs_group(GenomeTab tab, int span, const uint32_t *__restrict__ tmask, const uint32_t *__restrict__ tpos, PairGroup grp, int all,
                                                      uint32_t *__restrict__ cand, uint32_t *__restrict__ counters, uint32_t cand_cap)
{
    const uint32_t lo = grp.lo[blockIdx.y], hi = grp.hi[blockIdx.y];
    if (lo + blockIdx.x * runs_tile(ITEMS) >= hi) return;              // (workgroup-uniform: the grid covers the longest slice)
    mum_runs_body<false, ITEMS>(tab, span, tmask, tpos, hi, all, cand, counters, nullptr, 0u, lo, cand_cap);
}
template <typename ValT = uint32_t>
__global__ void __launch_bounds__(256) join_pair_group(const ValT *__restrict__ vals, GenomeTab tab, const uint32_t *__restrict__ rstart,
                                                       const uint32_t *__restrict__ rlen, const uint32_t *__restrict__ runiq,
                                                       uint32_t nruns, PairGroup grp, uint32_t *__restrict__ tmask, uint32_t *__restrict__ tpos)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nruns) return;
    const uint32_t u = runiq[r];
    uint32_t hit = 0;                                   // the pairs of the group this run is a hit of
    for (int y = 0; y < grp.n; y++) if ((u >> grp.ga[y]) & (u >> grp.gb[y]) & 1u) hit |= 1u << y;
    if (!hit) return;
    const uint32_t s = rstart[r], L = rlen[r];
    // the run's entries once (nearly every run has at most one entry per genome: <= 8 of them stay in registers)
    constexpr int RC = 8;
    ValT ev[RC]; int eg[RC];
#pragma unroll
    for (int t = 0; t < RC; t++) {
        ev[t] = 0; eg[t] = -1;
        if ((uint32_t)t < L) { ev[t] = vals[s + t]; eg[t] = genome_of(win_idx(ev[t]), tab); }
    }
    for (; hit; hit &= hit - 1) {
        const int y = __ffs(hit) - 1, gi = grp.ga[y], gj = grp.gb[y];
        ValT vi = 0, vj = 0;
#pragma unroll
        for (int t = 0; t < RC; t++) { if (eg[t] == gi) vi = ev[t]; if (eg[t] == gj) vj = ev[t]; }
        for (uint32_t t = s + RC; t < s + L; t++) {     // (longer runs: the rest from memory)
            const ValT v = vals[t];
            const int g = genome_of(win_idx(v), tab);
            if (g == gi) vi = v;
            if (g == gj) vj = v;
        }
        const uint32_t ap = win_idx(vi);                // gi < gj: the anchor is genome gi's window
        tmask[ap] = (1u << gi) | (1u << gj);
        tpos[(size_t)ap * tab.nseq + gi] = hit_word(vi, tab.gpos_off[gi]);
        tpos[(size_t)ap * tab.nseq + gj] = hit_word(vj, tab.gpos_off[gj]);
    }
}

// phase B: one wave per candidate; the 64 lanes test 64 consecutive offsets at a time and the resulting
// agreement bitmap is walked with scalar bit operations.  Record slot = candidate index; length 0 marks a
// candidate that turned out not to be the leftmost hit of its cluster.
#ifdef MAUVE_EXT_STATS
// measurement build only (-DMAUVE_EXT_STATS): [0] rounds, [2] sum of wave times, [3] longest wave time (10 ns ticks), [4] waves, [5] most rounds of one wave, [1] / [6] / [7] time in set-up / left walk / right walk
__device__ unsigned long long g_ext_stats[8];
#endif
template <bool SEG, bool LOCAL = false>
__global__ void __launch_bounds__(256) mum_extend(const uint64_t *__restrict__ packed, GenomeTab tab, SeedShape sh,
                                                  const uint32_t *__restrict__ tmask, const uint32_t *__restrict__ tpos,
                                                  uint32_t P, const uint32_t *__restrict__ cand, uint32_t ncand,
                                                  int extend, int32_t *__restrict__ mlen, int32_t *__restrict__ mstart,
                                                  const uint32_t *__restrict__ seg, uint32_t nseg,
                                                  const uint64_t *__restrict__ vmask, const uint64_t *__restrict__ cmask,
                                                  const uint32_t *__restrict__ ncand_dev = nullptr, uint32_t *__restrict__ counters_out = nullptr)
{
    __shared__ ExtComp s_comp[4][MAUVE_MAX_SEQ];
    // ncand_dev: the count is still on the device (a tiny pass launches this kernel without having looked at it: ncand is then the capacity of the list);
    // counters_out: page-locked host memory that receives the pass's counter block (ncand_dev - 1 .. + 11) -- with mlen / mstart in host memory
    // too, such a pass needs no copy at all
    if (counters_out && blockIdx.x == 0 && threadIdx.x < 12) counters_out[threadIdx.x] = ncand_dev[(int)threadIdx.x - 1];
    if (ncand_dev) ncand = min(ncand, *ncand_dev);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t wave_global = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    const int N = tab.nseq;
    ExtComp *comp = s_comp[wv];
#ifdef MAUVE_EXT_STATS
    const unsigned long long st_t0 = __builtin_amdgcn_s_memrealtime(); unsigned long long st_rounds = 0, st_setup = 0, st_left = 0, st_right = 0;
#endif
    for (uint32_t ci = wave_global; ci < ncand; ci += nwaves) {
#ifdef MAUVE_EXT_STATS
        unsigned long long st_r = 0; const unsigned long long st_c0 = __builtin_amdgcn_s_memrealtime(); unsigned long long st_c1 = st_c0, st_c2 = st_c0;
#define EXT_STAT_ROUND st_r++
#else
#define EXT_STAT_ROUND
#endif
        const uint32_t ap = cand[ci];
        const uint32_t mask = tmask[ap];
        const int anchor = __ffs(mask) - 1;
        const int nc = __popc(mask);
        const uint32_t segid = SEG ? seg_of(seg + (size_t)anchor * (nseg + 1), nseg, ap - tab.gpos_off[anchor]) : 0u;
        // component table: lane g fills the entry of genome g (entries in ascending genome order, anchor first)
        const uint32_t sa = tpos[(size_t)ap * N + anchor] >> 31;
        if (lane < N && (mask >> lane & 1)) {
            const int g = lane;
            const uint32_t vg = tpos[(size_t)ap * N + g];
            ExtComp C;
            C.G = packed + tab.word_off[g];
            C.VM = vmask ? vmask + tab.mask_off[g] : nullptr;
            C.CM = cmask ? cmask + tab.mask_off[g] : nullptr;
            C.pos = (int64_t)((vg & 0x7fffffffu) - (LOCAL ? 0u : tab.gpos_off[g]));      // (LOCAL: a wide pass's table word, hit_word)
            C.rev = (vg >> 31) ^ sa; C.g = (uint32_t)g; C.pad = 0;
            C.lo = 0; C.hi = (int64_t)tab.nwin[g] - 1;
            C.maxw = (uint32_t)(((uint64_t)tab.nwin[g] + (uint32_t)sh.span - 1 + 31) / 32 + 2);       // mauve_packed_words - 1
            if (SEG) { const uint32_t *sg = seg + (size_t)g * (nseg + 1) + segid; C.lo = sg[0]; C.hi = (int64_t)sg[1] - sh.span; }
            comp[__popc(mask & ((1u << g) - 1u))] = C;
        }
        __threadfence_block();          // the table is read by every lane of this wave
#ifdef MAUVE_EXT_STATS
        st_c1 = __builtin_amdgcn_s_memrealtime(); st_setup += st_c1 - st_c0;
#endif
        int64_t klo = 0, khi = 0;
        bool leftmost = true;
        if (extend) {
            // offsets every component's window stays inside its genome / gap segment for
            int64_t kmin = INT64_MIN, kmax = INT64_MAX;
            for (int c = 0; c < nc; c++) {
                const ExtComp &C = comp[c];
                const int64_t a = C.rev ? C.pos - C.hi : C.lo - C.pos, b = C.rev ? C.pos - C.lo : C.hi - C.pos;
                kmin = max(kmin, a); kmax = min(kmax, b);
            }
            const bool masks = vmask || cmask;
            const uint32_t revset = (uint32_t)__ballot(lane < nc && comp[lane].rev != 0u);
            const int rev_at = revset ? __builtin_amdgcn_readfirstlane((int)comp[__ffs(revset) - 1].g) : -1;      // a component on the other strand, if there is one
            const uint32_t ap_s = (uint32_t)__builtin_amdgcn_readfirstlane((int)ap); const int anchor_s = __builtin_amdgcn_readfirstlane(anchor);
            // the first round of either walk: offsets -64 .. -1 and 1 .. 64, fetched together
            uint64_t M2[2][4];
            { const int64_t jj[2] = {-64, 1}; ext_mismatch<2>(comp, nc, sh.span, jj, lane, M2); }
            // ---- left walk: offsets cur-1 .. cur-64 per round ----
            int64_t cur = 0;
            for (bool done = false; !done;) {
                const int64_t k = cur - 1 - lane;
                const int64_t hq = (int64_t)ap + k;
                const uint32_t hm = (hq >= 0) ? tmask[hq] : 0u;       // issued beside the genome words
                EXT_STAT_ROUND;
                uint64_t M1[1][4];
                if (cur != 0) { const int64_t jj[1] = {cur - 64}; ext_mismatch<1>(comp, nc, sh.span, jj, lane, M1); }
                else { for (int q = 0; q < 4; q++) M1[0][q] = M2[0][q]; }
                bool a = k >= kmin && k <= kmax && ext_window_clean(M1[0], 63 - lane, sh);
                if (masks) a = a && !ext_blocked(comp, nc, sh.span, k);
                const bool hh = a && hm == mask;
                const uint64_t A = __ballot(a), H = __ballot(hh);
                const int p = walk_round(A, sh.span, done);                          // offsets consumed in this round
                // A same-mask hit among the visited offsets sits on this diagonal's windows (its offset agrees, and every component genome holds
                // the mer once), but it is a hit OF this diagonal (S4) only with the candidate's strand relations.  They can differ in one way: the
                // mer is its own reverse complement (even weight) -- it agrees on a reverse diagonal and is a forward hit, of another cluster --
                // and then in every component, so one reversed component of the candidate decides.  Wave-uniform: scalar loads, no vector register.
                uint64_t Hv = H & (p >= 64 ? ~0ULL : ((1ULL << p) - 1ULL));
                if (Hv && rev_at >= 0) {
                    bool met = false;
                    for (; Hv && !met; Hv &= Hv - 1) {
                        const uint32_t *rq = tpos + ((size_t)ap_s + (size_t)cur - (size_t)__ffsll((unsigned long long)Hv)) * (size_t)N;
                        met = ((rq[rev_at] ^ rq[anchor_s]) >> 31) != 0u;
                    }
                    Hv = met;
                }
                if (Hv) { leftmost = false; done = true; }
                cur -= p;
                if (p == 0) done = true;                   // (p == 0 only happens with done set; keeps cur != 0 a valid "not the first round" test)
            }
            if (!leftmost) {
#ifdef MAUVE_EXT_STATS
                st_rounds += st_r; st_left += __builtin_amdgcn_s_memrealtime() - st_c1;
#endif
                if (lane == 0) mlen[ci] = 0; __threadfence_block(); continue;
            }
            klo = cur;
#ifdef MAUVE_EXT_STATS
            st_c2 = __builtin_amdgcn_s_memrealtime(); st_left += st_c2 - st_c1;
#endif
            // ---- right walk ----
            cur = 0;
            for (bool done = false; !done;) {
                const int64_t k = cur + 1 + lane;
                EXT_STAT_ROUND;
                uint64_t M1[1][4];
                if (cur != 0) { const int64_t jj[1] = {cur + 1}; ext_mismatch<1>(comp, nc, sh.span, jj, lane, M1); }
                else { for (int q = 0; q < 4; q++) M1[0][q] = M2[1][q]; }
                bool a = k >= kmin && k <= kmax && ext_window_clean(M1[0], lane, sh);
                if (masks) a = a && !ext_blocked(comp, nc, sh.span, k);
                const uint64_t A = __ballot(a);
                const int p = walk_round(A, sh.span, done);
                cur += p;
            }
            khi = cur;
        }
        if (lane == 0) mlen[ci] = (int32_t)(khi - klo) + sh.span;
        if (lane < N) {
            int32_t st = 0;
            if (mask >> lane & 1) {
                const ExtComp &C = comp[__popc(mask & ((1u << lane) - 1u))];
                st = C.rev ? (int32_t)(-(C.pos - khi + 1)) : (int32_t)(C.pos + klo + 1);
            }
            mstart[(size_t)ci * N + lane] = st;
        }
        __threadfence_block();          // the next candidate overwrites the table
#ifdef MAUVE_EXT_STATS
        st_rounds += st_r; st_right += __builtin_amdgcn_s_memrealtime() - st_c2;
#endif
    }
#ifdef MAUVE_EXT_STATS
    if (lane == 0) {
        const unsigned long long dt = __builtin_amdgcn_s_memrealtime() - st_t0;
        atomicAdd(&g_ext_stats[0], st_rounds); atomicAdd(&g_ext_stats[2], dt); atomicMax(&g_ext_stats[3], dt); atomicAdd(&g_ext_stats[4], 1ULL); atomicMax(&g_ext_stats[5], st_rounds);
        atomicAdd(&g_ext_stats[1], st_setup); atomicAdd(&g_ext_stats[6], st_left); atomicAdd(&g_ext_stats[7], st_right);
    }
#endif
}
// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// The switches that tests and tools set are fields of switches() (switches.hpp; DESIGN.md section 4, "Seed pass host side", names who sets which).
// Index width of a seed pass: wide values when the pass has 2^31 windows or more; MAUVE_WIDE_INDEX=1 forces them for every
// pass (test switch: small inputs take the wide kernels against the oracle).  Every other pass runs the narrow instantiations.
bool seedpass_wide(int64_t total_windows)
{
    return switches().wide_index || total_windows >= (1LL << 31);
}

bool make_seed_shape(uint64_t pattern, SeedShape *sh)
{
    memset(sh, 0, sizeof *sh);
    int span = mauve_seed_length(pattern), w = mauve_seed_weight(pattern);
    if (span < 1 || span > MAUVE_MAX_SEED_SPAN || w < 1 || w > 31) return false;
    // palindromic, first and last set
    for (int t = 0; t < span; t++)
        if (((pattern >> t) & 1) != ((pattern >> (span - 1 - t)) & 1)) return false;
    if (!(pattern & 1)) return false;
    sh->span = span; sh->weight = w; sh->keymask = (1ULL << (2 * w)) - 1ULL;
    const bool narrow = seed_narrow(*sh);
    int j = 0, nr = 0;
    for (int t = 0; t < span;) {
        if (!((pattern >> (span - 1 - t)) & 1)) { t++; continue; }
        int t0 = t;
        while (t < span && ((pattern >> (span - 1 - t)) & 1)) t++;
        int len = t - t0;
        if (nr >= (narrow ? SEED_RUNS_NARROW : SEED_RUNS_MAX)) return false;       // (cannot happen: runs are at least two offsets apart)
        const uint32_t shift = (uint32_t)(2 * (t0 - j));
        if (narrow) { sh->run_shift[nr] = shift; sh->run_mask[nr] = (uint32_t)(((1ULL << (2 * len)) - 1ULL) << (2 * j)); }
        sh->run_wide[nr] = shift | (uint32_t)(2 * j) << 8 | (uint32_t)(2 * len) << 16;
        nr++; j += len;
    }
    sh->nruns = nr;
    for (int t = 0; t < span; t++) {
        if (!((pattern >> (span - 1 - t)) & 1)) continue;
        if (2 * t < 64) sh->care_lo |= 3ULL << (2 * t); else sh->care_hi |= 3ULL << (2 * t - 64);
    }
    return true;
}

static int build_tab(mauve_ctx *ctx, const GenomeSet &gs, int span, GenomeTab *tab, int64_t *total_windows)
{
    memset(tab, 0, sizeof *tab);
    tab->nseq = gs.nseq;
    int64_t tot = 0;
    for (int g = 0; g < gs.nseq; g++) {
        int64_t nw = gs.lens[g] - span + 1; if (nw < 0) nw = 0;
        tab->gpos_off[g] = (uint32_t)tot; tab->nwin[g] = (uint32_t)nw; tab->word_off[g] = gs.word_off[g];
        tab->mask_off[g] = (gs.vmask || gs.cmask) ? gs.mask_off[g] : 0;
        tot += nw;
        if (gs.word_off[g] >> 32) { ctx->err = "seed pass: a genome starts 2^32 words or more into its buffer"; return MAUVE_ERR_LIMIT; }     // (genome_at; the total limit below keeps every set far under it)
        if (gs.lens[g] >= MAUVE_MAX_GENOME_LEN) { ctx->err = "seed pass: a genome holds 2^31 bases or more (per-genome limit)"; return MAUVE_ERR_LIMIT; }
        if (tot >= MAUVE_MAX_TOTAL_LEN) { ctx->err = "seed pass: the genomes together hold 2^32 - 2^20 windows or more (total limit)"; return MAUVE_ERR_LIMIT; }
    }
    tab->gpos_off[gs.nseq] = (uint32_t)tot;
    for (int g = gs.nseq + 1; g <= MAUVE_MAX_SEQ; g++) tab->gpos_off[g] = 0xffffffffu;      // see genome_of
    *total_windows = tot;
    return MAUVE_OK;
}

// ---- what the stages of a pass share ----
struct FinderPass { uint32_t consider, want; int rule; };

// The decisions of a pass, made once (seed_plan) and read by the stages.
struct SeedPlan {
    bool seg;           // segmented set
    bool hash_path;     // partial sort + join_hash (else: full sort)
    bool tiny;          // no key arrays at all: tiny_join
    bool compact;       // only the valid windows go into the sort (valid_count / seed_extract_compact)
    bool has_invalid;   // some windows are unusable (placed or ambiguous bases, contig joins) and sit in the sorted list, with all-ones keys
    bool use_summary;   // pairwise finder over several pairs: one run list for all of them (run_summary)
    bool strand_bitmap; // seed_extract_all writes no value array: the first sort pass makes the values from the window index and a strand bitmap
    int segbits;        // segmented keys: segment id above the mer; ids 0 .. nseg-1, the all-ones id is left to the invalid (all-ones) key
    int full_bits;      // key bits a full sort orders
    // globally sorted bits: 8-bit passes until a bucket averages <= 512 entries; a segmented list sorts at least the
    // segment id, so that the invalid windows form the last bucket on their own.  The passes order bits [low_bits, full_bits); 0 = full sort
    int low_bits(uint32_t entries) const
    {
        if (!hash_path) return 0;
        int G = 0;
        while (G < full_bits && ((uint64_t)entries >> G) > 512) G += 8;
        if (seg) G = std::max(G, (segbits + 7) / 8 * 8);
        return full_bits - std::min(G, full_bits);
    }
};

// Which join a pass runs, in the order the stages ask:
//   host-supplied hits            : none (hits_scatter fills the hit table)
//   use_summary                   : run_summary once, then join_pair_group per group of pairs
//   tiny                          : tiny_join, a pass of a few thousand windows
//   hash_path                     : the LDS hash join over a partial sort (join_hash) for the one-pass finders; the slices it hands
//                                   back are sorted in full and joined by mum_join_slices
//   otherwise                     : the full sort and the serial join (mum_join): a single pair of PairwiseMatchFinder (its run
//                                   list needs sorted order), the two exports (sort only), segmented masked passes
static int seed_plan(mauve_ctx *ctx, const SeedShape &sh, const GenomeTab &tab, const SeedRequest &rq, uint32_t n, bool masked, bool seg,
                     int key_type_bits, SeedPlan *pl, std::vector<FinderPass> *passes)
{
    pl->seg = seg;
    pl->hash_path = !rq.hits && rq.mode != MAUVE_MODE_PAIRWISE && !rq.out_keys && !rq.enumerate && rq.only_seq < 0 && !(masked && seg);
    pl->segbits = 0;
    if (seg) while (pl->segbits < 32 && (1ull << pl->segbits) <= (uint64_t)rq.nseg) pl->segbits++;
    if (seg && 2 * sh.weight + pl->segbits > 64) { ctx->err = "recursive anchoring: segment id and mer do not fit 64 bits"; return MAUVE_ERR_LIMIT; }
    pl->full_bits = seg ? 2 * sh.weight + pl->segbits : ((masked && rq.only_seq >= 0) ? key_type_bits : 2 * sh.weight);
    pl->tiny = pl->hash_path && !switches().no_tiny && n <= (uint32_t)TJ_MAX && tab.nseq <= 16 && 2 * sh.weight + pl->segbits <= 32;
    pl->compact = !rq.hits && !pl->tiny && rq.only_seq < 0 && masked && !seg;
    pl->has_invalid = masked && !pl->compact;
    // Only where seed_extract_all feeds a tiled sort pass (extract's third branch, and bits left to sort: a pass without a sort pass joins
    // the list as extracted).  The compacted and single-genome extractions, the exports (only_seq), the multiplicity pass and host hits
    // keep the value array: their values are not their own indices, or nothing would make them.
    pl->strand_bitmap = !rq.hits && !pl->tiny && !pl->compact && rq.only_seq < 0 && pl->low_bits(n) < pl->full_bits;
    // one pass, or one per genome pair for PairwiseMatchFinder
    const int N = tab.nseq;
    if (rq.mode == MAUVE_MODE_PAIRWISE) {
        // (guide tree over several contexts, mauve_set_shard: this rank's share of the pairs, dealt round robin; the sums are exchanged)
        int pi = 0;
        for (int i = 0; i < N; i++) for (int j = i + 1; j < N; j++, pi++)
            if (!ctx->pair_sums_only || !ctx->shard_on || pi % ctx->shard_world == ctx->shard_rank)
                passes->push_back({(1u << i) | (1u << j), (1u << i) | (1u << j), MAUVE_MODE_MEM});
    } else passes->push_back({0xffffffffu, (uint32_t)rq.mask, rq.mode});
    pl->use_summary = rq.mode == MAUVE_MODE_PAIRWISE && !seg && !rq.hits && (passes->size() > 1 || (ctx->pair_sums_only && ctx->shard_on && !passes->empty()));
    return MAUVE_OK;
}

// State of one pass.  KeyT / ValT: key and sort-value types; ValT is uint32_t (narrow) or uint64_t (wide: a pass of 2^31 windows or
// more, or MAUVE_WIDE_INDEX=1).  A wide pass's hit table and host-side hit records hold windows local to their genome
// (hit_word); out_vals are then local too.
struct SeedState {
    mauve_ctx *ctx; const GenomeSet &gs; const SeedShape &sh; const GenomeTab &tab; const SeedRequest &rq;
    uint32_t P;                                    // windows of the set
    const uint64_t *packed, *vmask, *cmask;
    SeedPlan pl;
    std::vector<FinderPass> passes;
    uint32_t ns = 0;                               // entries of the sorted list (all windows, or the valid ones)
    int L = 0;                                     // pl.low_bits(ns)
    uint32_t *tmask = nullptr, *tpos = nullptr;    // the hit table: [P] component sets, [P][N] values
    uint32_t cand_cap = 0;
    uint32_t cand_total = 0;                       // one record slot per candidate of every pass; length 0 = not a leftmost hit
    bool records_on_host = false;                  // ctx->sdh.hl / hs hold the candidates' records already (tiny_pass)
    double trace_t0 = 0;
};
template <typename KeyT, typename ValT>
struct SeedPass : SeedState {
    KeyT *keys = nullptr; ValT *vals = nullptr;    // the list the sort takes and leaves
    bool have_hist0 = false;                       // ctx->hist holds the tile histograms of the first sort pass (seed_extract_all)
    bool iota = false;                             // pl.strand_bitmap took effect: vals holds the strand bitmap, the first sort pass makes the values
    SeedPass(const SeedState &s) : SeedState(s) {}
};

template <typename KeyT, typename ValT>
static int ensure_sort_buffers(mauve_ctx *ctx, uint32_t n)
{
    HIPCHK(ctx, ctx->keysA.ensure((size_t)n * sizeof(KeyT)));
    HIPCHK(ctx, ctx->keysB.ensure((size_t)n * sizeof(KeyT)));
    HIPCHK(ctx, ctx->valsA.ensure((size_t)n * sizeof(ValT)));
    HIPCHK(ctx, ctx->valsB.ensure((size_t)n * sizeof(ValT)));
    return MAUVE_OK;
}

// The NARROW instantiations of seed_extract_all / seed_extract_compact: launch(std::true_type) when the seed fits them
template <typename F>
static void launch_narrow_or_not(const SeedShape &sh, F &&launch)
{
    if (seed_narrow(sh)) launch(std::true_type{});
    else launch(std::false_type{});
}

// keys and values of all n windows into keys / vals, the tile histograms of the first sort pass (digit at hshift) into ctx->hist
// bitmap: no values -- the strand bitmap goes to the front of the vals buffer (see extract)
template <typename KeyT, bool SEG, typename ValT>
static int extract_all(mauve_ctx *ctx, const GenomeSet &gs, const SeedShape &sh, const GenomeTab &tab, uint32_t n, const uint32_t *seg, uint32_t nseg,
                       int hshift, KeyT *keys, ValT *vals, bool bitmap = false)
{
    const uint32_t nblk = (n + RS_TILE - 1) / RS_TILE;
    HIPCHK(ctx, ctx->hist.ensure((size_t)nblk * 256 * sizeof(uint32_t)));
    const uint64_t *packed = gs.buf->as<uint64_t>();
    const uint64_t *vmask = gs.vmask ? gs.vmask->as<uint64_t>() : nullptr;      // placed or ambiguous bases
    const uint64_t *cmask = gs.cmask ? gs.cmask->as<uint64_t>() : nullptr;      // contig joins
    KernelTimer t(ctx, MAUVE_K_EXTRACT, n);
    launch_narrow_or_not(sh, [&](auto narrow) {
        hipLaunchKernelGGL((seed_extract_all<KeyT, SEG, decltype(narrow)::value, ValT>), dim3(nblk), dim3(256), 0, ctx->stream, packed, tab, sh, keys,
                           vals, n, seg, nseg, ctx->hist.as<uint32_t>(), nblk, vmask, hshift, cmask, bitmap ? reinterpret_cast<uint32_t *>(vals) : nullptr);
    });
    return MAUVE_OK;
}

// Stage 1: the (key, value) list the sort takes: ps.keys / vals / ns / have_hist0
template <typename KeyT, bool SEG, typename ValT>
static int extract(SeedPass<KeyT, ValT> &ps)
{
    mauve_ctx *ctx = ps.ctx; const SeedRequest &rq = ps.rq; const uint32_t n = ps.P;
    if (int rc = ensure_sort_buffers<KeyT, ValT>(ctx, n)) return rc;
    HIPCHK(ctx, ctx->counters.ensure(64));
    KeyT *keys = ps.keys = ctx->keysA.as<KeyT>(); ValT *vals = ps.vals = ctx->valsA.as<ValT>();
    if (rq.hits) ps.ns = 1;
    else if (ps.pl.tiny) ps.ns = n;
    else if (ps.pl.compact) {
        // masked pass: only the valid windows go into the sort (see valid_count / seed_extract_compact)
        const uint32_t nblk = (n + 4095) / 4096;
        HIPCHK(ctx, ctx->hist.ensure((size_t)nblk * 256 * sizeof(uint32_t)));     // the tile counts live in the histogram buffer
        uint32_t *tile_cnt = ctx->hist.as<uint32_t>();
        {
            KernelTimer t(ctx, MAUVE_K_EXTRACT, n);
            hipLaunchKernelGGL(valid_count, dim3(nblk), dim3(256), 0, ctx->stream, ps.tab, ps.sh.span, n, ps.vmask, tile_cnt, ps.cmask);
            hipLaunchKernelGGL(tile_scan, dim3(1), dim3(256), 0, ctx->stream, tile_cnt, nblk, ctx->counters.as<uint32_t>());
            launch_narrow_or_not(ps.sh, [&](auto narrow) {
                hipLaunchKernelGGL((seed_extract_compact<KeyT, decltype(narrow)::value, ValT>), dim3(nblk), dim3(256), 0, ctx->stream, ps.packed, ps.tab, ps.sh,
                                   keys, vals, n, ps.vmask, tile_cnt, ps.cmask);
            });
        }
        HIPCHK(ctx, hipGetLastError());
        const uint32_t *cw;
        if (int rc = seed_counters(ctx, 16, &cw)) return rc;       // (ctx->shadow stays for the pass's wait behind the run detection)
        ps.ns = cw[0];
    } else if (rq.only_seq < 0) {
        // The strand bitmap (512 bytes per tile of 4096 windows) lies at the front of valsA, where the values would have gone.  Nothing
        // else is in that buffer: extraction writes it, the first sort pass reads it and writes valsB, and valsA is written again only by
        // the second pass, a launch later on the same stream.  It is at most the size of the values except for a list far shorter than a tile.
        if (ps.pl.strand_bitmap) HIPCHK(ctx, ctx->valsA.ensure(std::max((size_t)n * sizeof(ValT), (size_t)((n + RS_TILE - 1) / RS_TILE) * (RS_TILE / 8))));
        vals = ps.vals = ctx->valsA.as<ValT>();
        if (int rc = extract_all<KeyT, SEG, ValT>(ctx, ps.gs, ps.sh, ps.tab, n, rq.seg, rq.nseg, ps.pl.low_bits(n), keys, vals, ps.pl.strand_bitmap)) return rc;
        ps.ns = n; ps.have_hist0 = true; ps.iota = ps.pl.strand_bitmap;
    } else {
        const int g = rq.only_seq;
        uint32_t nw = ps.tab.nwin[g];
        if (nw) {
            uint32_t blocks = std::min<uint32_t>((nw + 255) / 256, 256 * 16);
            KernelTimer t(ctx, MAUVE_K_EXTRACT, nw);
            hipLaunchKernelGGL((seed_extract<KeyT, SEG, ValT>), dim3(blocks), dim3(256), 0, ctx->stream, ps.packed, ps.tab, ps.sh, g, keys,
                               vals, 0u, rq.seg, rq.nseg);
            ps.ns = nw;
        }
    }
    HIPCHK(ctx, hipGetLastError());
    seed_trace(ctx, "extract", ps.trace_t0);
    return MAUVE_OK;
}

// SeedMatchEnumerator: runs -> matches on the device, only the CSR result goes to the host
template <typename KeyT, typename ValT>
static int export_enumerator(SeedPass<KeyT, ValT> &ps)
{
    mauve_ctx *ctx = ps.ctx; const uint32_t sorted_n = ps.ns; KeyT *keys = ps.keys; ValT *vals = ps.vals;
    EnumRequest &q = *ps.rq.enumerate;
    using namespace devscan;
    const uint32_t nb = (sorted_n + TILE - 1) / TILE, blocks = (sorted_n + 255) / 256;
    HIPCHK(ctx, ctx->run_sum.ensure((size_t)sorted_n * 4 + 64 + ((size_t)sorted_n + 2) * 8 * 3 + (size_t)nb * 16 + 256));
    uint32_t *emit = ctx->run_sum.as<uint32_t>();
    int64_t *soff = reinterpret_cast<int64_t *>(ctx->run_sum.as<char>() + (((size_t)sorted_n * 4 + 63) & ~(size_t)63));
    int64_t *d_mult = soff + sorted_n + 2, *d_off = d_mult + sorted_n + 2, *bsum = d_off + sorted_n + 2, *tot = bsum + nb + 2;
    uint32_t *bcnt = reinterpret_cast<uint32_t *>(tot + 4);
    hipLaunchKernelGGL((enum_runs<KeyT, ValT>), dim3(blocks), dim3(256), 0, ctx->stream, keys, vals, sorted_n, q.min_multi, q.max_multi, q.direct_only, emit);
    hipLaunchKernelGGL((vscan_partial<int64_t, EmitVal>), dim3(nb), dim3(256), 0, ctx->stream, EmitVal{emit}, sorted_n, bsum);
    hipLaunchKernelGGL((vscan_write<int64_t, EmitVal>), dim3(nb), dim3(256), 0, ctx->stream, EmitVal{emit}, sorted_n, bsum, soff, tot + 1);
    const EnumRuns er{emit, soff, sorted_n, d_mult, d_off, tot};
    hipLaunchKernelGGL((cmp_count<EnumRuns>), dim3(nb), dim3(256), 0, ctx->stream, er, bcnt);
    hipLaunchKernelGGL((cmp_write<EnumRuns>), dim3(nb), dim3(256), 0, ctx->stream, er, bcnt);
    HIPCHK(ctx, hipGetLastError());
    int64_t ht[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(ht, tot, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    q.n = ht[0]; q.ns = ht[1];
    if (q.starts) {
        HIPCHK(ctx, ctx->sorted_rec.ensure(((size_t)q.ns + 1) * 8));
        hipLaunchKernelGGL((enum_write<KeyT, ValT>), dim3(blocks), dim3(256), 0, ctx->stream, keys, vals, sorted_n, q.direct_only, emit, soff,
                           ps.tab.gpos_off[ps.rq.only_seq], ctx->sorted_rec.as<int64_t>());
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(q.mult, d_mult, (size_t)q.n * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(q.start_off, d_off, ((size_t)q.n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(q.starts, ctx->sorted_rec.p, (size_t)q.ns * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MAUVE_OK;
}

// sorted-mer-list export: hand the sorted pairs to the host
template <typename KeyT, typename ValT>
static int export_sorted_list(SeedPass<KeyT, ValT> &ps)
{
    constexpr bool WIDEV = sizeof(ValT) == 8;
    mauve_ctx *ctx = ps.ctx; const uint32_t sorted_n = ps.ns;
    std::vector<uint64_t> *out_keys = ps.rq.out_keys; std::vector<uint32_t> *out_vals = ps.rq.out_vals;
    std::vector<KeyT> hk(sorted_n);
    out_vals->resize(sorted_n);
    std::vector<ValT> hv(WIDEV ? sorted_n : 0);
    HIPCHK(ctx, hipMemcpyAsync(hk.data(), ps.keys, (size_t)sorted_n * sizeof(KeyT), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(WIDEV ? (void *)hv.data() : (void *)out_vals->data(), ps.vals, (size_t)sorted_n * sizeof(ValT), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    out_keys->resize(sorted_n);
    for (uint32_t i = 0; i < sorted_n; i++) (*out_keys)[i] = (uint64_t)hk[i];
    if (WIDEV) {                                // wide: local to the genome already (index | strand << 31), as the narrow caller makes them
        const uint32_t g0 = ps.tab.gpos_off[ps.rq.only_seq];
        for (uint32_t i = 0; i < sorted_n; i++) (*out_vals)[i] = ((uint32_t)hv[i] - g0) | ((uint32_t)((uint64_t)hv[i] >> 63) << 31);
    }
    return MAUVE_OK;
}

// ---- launchers and checks the finder stages share ----
// Capacities of the compacted lists are handed to the kernels that fill them (a store past the end is skipped, the counter still counts)
// and checked against the counts that come back.
static bool cand_overflow(SeedState &st, uint32_t nc)
{
    if (nc > st.cand_cap) st.ctx->err = "seed pass: " + std::to_string(nc) + " candidates for a list of " + std::to_string(st.cand_cap);
    return nc > st.cand_cap;
}

// The windows [lo, hi) in which a hit of a finder pass can be anchored.  The joins write tmask only at a hit's anchor, the window of the
// lowest genome of its component set m (join_hash, mum_join_at), and m has at least two genomes (finder_components):
//   want != 0 : m == want, so the anchor lies in genome ctz(want)  (the hot path: mauve_align, the LCB extension, the recursion and the
//               progressive nodes all ask for the full set -- genome 0, a fifth of the windows of five genomes);
//   want == 0 : m is any subset of `consider` within the set's genomes: from the lowest of them to just before the highest.
// Hits the host supplies (hits_scatter) may be anchored anywhere.  A pass clears and scans this range only (finder_pass).
// That leaves stale entries of earlier passes outside it, so every reader of tmask was checked:
//   mum_runs   looks at [lo - RUNS_HALO, hi): the range and the halo in front of its first tile, which the pass clears as well;
//   mum_extend reads tmask[ap] at candidates, which mum_runs took from the range, and on its left walk tmask[ap + k], k < 0 -- also in front of
//              the range, but such a word only counts where k >= kmin (`a`), that is inside the anchor's own genome or gap segment,
//              which lies in [lo, ap);
//   tiny_join and the pair groups clear what they scan themselves, and nothing outside this file reads the table.
// (A range that comes out empty -- a mask beyond the set, a genome shorter than the seed -- has no hit either way: the whole table then.)
struct WinRange { uint32_t lo, hi; };
static WinRange anchor_range(const GenomeTab &tab, uint32_t P, const FinderPass &fp, bool host_hits)
{
    const int N = tab.nseq;
    const uint32_t in_set = N >= 32 ? 0xffffffffu : (1u << N) - 1u;
    WinRange r{0u, P};
    if (host_hits) return r;
    if (fp.want) {
        const int g = __builtin_ctz(fp.want);
        if (g < N) r = {tab.gpos_off[g], tab.gpos_off[g + 1]};
    } else if (const uint32_t c = fp.consider & in_set)
        r = {tab.gpos_off[__builtin_ctz(c)], tab.gpos_off[31 - __builtin_clz(c)]};
    r.hi = std::min(r.hi, P);
    if (r.lo >= r.hi) r = {0u, P};
    return r;
}

// Windows per thread of a run-detection launch over `windows` windows (the longest slice of a pair group), from that size and the
// device's compute units alone.  Measured per launch size in profiles/run_tiles_summary.md: 16 (tiles of 4096) only where a compute unit
// has RUNS_CU_16 windows or more -- there the one counter every tile ends on is the limit, and a smaller tile doubles the atomics on it;
// 8 from RUNS_CU_8 windows per compute unit; 4 below, where tiles of 4096 windows leave most of the device without a workgroup.
constexpr uint64_t RUNS_CU_16 = 131072, RUNS_CU_8 = 6144;
static int runs_items(const mauve_ctx *ctx, uint64_t windows)
{
    if (const int forced = switches().runs_items) return forced;
    const uint64_t per_cu = windows / (uint64_t)std::max(ctx->cus, 1);
    return per_cu >= RUNS_CU_16 ? 16 : (per_cu >= RUNS_CU_8 ? 8 : 4);
}
// f(std::integral_constant<int, ITEMS>) for the instantiation that runs_items chose
template <typename F>
static void with_runs_items(int items, F &&f)
{
    if (items == 16) f(std::integral_constant<int, 16>());
    else if (items == 8) f(std::integral_constant<int, 8>());
    else f(std::integral_constant<int, 4>());
}

// extension phase A: run starts from the windows [r.lo, r.hi) of the hit table
template <bool SEG>
static int launch_runs(SeedState &st, WinRange r)
{
    mauve_ctx *ctx = st.ctx;
    { KernelTimer t(ctx, MAUVE_K_RUNS, r.hi - r.lo);
      with_runs_items(runs_items(ctx, r.hi - r.lo), [&](auto items) {
          constexpr int ITEMS = decltype(items)::value;
          hipLaunchKernelGGL((mum_runs<SEG, ITEMS>), dim3((r.hi - r.lo + runs_tile(ITEMS) - 1) / runs_tile(ITEMS)), dim3(256), 0, ctx->stream, st.tab,
                             st.sh.span, st.tmask, st.tpos, r.hi, st.rq.extend ? 0 : 1, ctx->cand.as<uint32_t>(), ctx->counters.as<uint32_t>(), st.rq.seg,
                             st.rq.nseg, st.cand_cap, r.lo);
      }); }
    HIPCHK(ctx, hipGetLastError());
    return MAUVE_OK;
}

// extension phase B over the first ncand entries of the candidate list (ncand_dev / counters_out: see mum_extend)
template <bool SEG, bool WIDEV>
static int launch_extend(SeedState &st, uint32_t blocks, uint32_t ncand, int32_t *o_len, int32_t *o_start, const uint32_t *ncand_dev = nullptr,
                         uint32_t *counters_out = nullptr)
{
    mauve_ctx *ctx = st.ctx;
    KernelTimer t(ctx, MAUVE_K_EXTEND, ncand);
    hipLaunchKernelGGL((mum_extend<SEG, WIDEV>), dim3(blocks), dim3(256), 0, ctx->stream, st.packed, st.tab, st.sh, st.tmask, st.tpos, st.P,
                       ctx->cand.as<uint32_t>(), ncand, st.rq.extend, o_len, o_start, st.rq.seg, st.rq.nseg, st.vmask, st.cmask, ncand_dev, counters_out);
    HIPCHK(ctx, hipGetLastError());
#ifdef MAUVE_EXT_STATS
    if (switches().trace) {
        unsigned long long h[8]; hipStreamSynchronize(ctx->stream);
        hipMemcpyFromSymbol(h, HIP_SYMBOL(g_ext_stats), sizeof h); unsigned long long z[8] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(g_ext_stats), z, sizeof z);
        fprintf(stderr, "[trace]   extend stats: %llu rounds, %llu waves, wave time mean %.1f us max %.1f us (setup %.1f, left walk %.1f, right walk %.1f), most rounds of a wave %llu\n", h[0], h[4],
                h[4] ? h[2] / (double)h[4] / 100.0 : 0.0, h[3] / 100.0, h[4] ? h[1] / (double)h[4] / 100.0 : 0.0, h[4] ? h[6] / (double)h[4] / 100.0 : 0.0,
                h[4] ? h[7] / (double)h[4] / 100.0 : 0.0, h[5]);
    }
#endif
    return MAUVE_OK;
}

// the records of all passes accumulate on the device: nc more behind the cand_total there are
template <bool SEG, bool WIDEV>
static int extend_candidates(SeedState &st, uint32_t nc, uint32_t max_blocks)
{
    mauve_ctx *ctx = st.ctx; const int N = st.tab.nseq;
    HIPCHK(ctx, ctx->mlen.ensure_keep((size_t)(st.cand_total + nc) * 4 + 4, (size_t)st.cand_total * 4, ctx->stream));
    HIPCHK(ctx, ctx->mstart.ensure_keep((size_t)(st.cand_total + nc) * 4 * N + 4, (size_t)st.cand_total * 4 * N, ctx->stream));
    if (int rc = launch_extend<SEG, WIDEV>(st, std::min<uint32_t>((nc + 3) / 4, max_blocks), nc, ctx->mlen.as<int32_t>() + st.cand_total,
                                           ctx->mstart.as<int32_t>() + (size_t)st.cand_total * N)) return rc;
    st.cand_total += nc;
    seed_trace(ctx, "extend", st.trace_t0);
    return MAUVE_OK;
}

// PairwiseMatchFinder over several pairs.  The runs that can matter to any pair are listed once (see run_summary); then the passes run
// in groups: pairs with different lower genomes write disjoint slices of the hit table, so up to
// N - 1 of them share one join launch (the run list is read once per group instead of once per pair), one run-detection launch
// (blockIdx.y = pair), one candidate list, one round trip and one extension launch: 28 passes of an 8-genome guide tree are 7 groups.
template <typename KeyT, typename ValT>
static int pairwise_passes(SeedPass<KeyT, ValT> &ps)
{
    constexpr bool WIDEV = sizeof(ValT) == 8;
    mauve_ctx *ctx = ps.ctx; const GenomeTab &tab = ps.tab; const uint32_t P = ps.P, ns = ps.ns, list_cap = switches().list_cap;
    const std::vector<FinderPass> &passes = ps.passes;
    const size_t cap = (size_t)ns / 2 + 1;
    const uint32_t run_cap = list_cap ? std::min<uint32_t>((uint32_t)cap, list_cap) : (uint32_t)cap;
    HIPCHK(ctx, ctx->run_sum.ensure(3 * cap * 4));
    uint32_t *rstart = ctx->run_sum.as<uint32_t>(), *rlen = rstart + cap, *runiq = rlen + cap;
    HIPCHK(ctx, hipMemsetAsync(ctx->counters.p, 0, 64, ctx->stream));
    { KernelTimer t(ctx, MAUVE_K_JOIN, ns);
      hipLaunchKernelGGL((run_summary<KeyT, ValT>), dim3((ns + 1023) / 1024), dim3(256), 0, ctx->stream, ps.keys, ps.vals, ns, tab,
                         (int)ps.pl.has_invalid, rstart, rlen, runiq, ctx->counters.as<uint32_t>() + 2, run_cap); }
    HIPCHK(ctx, hipGetLastError());
    const uint32_t *cw;
    if (int rc = seed_counters(ctx, 16, &cw)) return rc;
    const uint32_t nruns = cw[2];
    if (nruns > run_cap) { ctx->err = "seed pass: " + std::to_string(nruns) + " runs for a list of " + std::to_string(run_cap); return MAUVE_ERR_LIMIT; }
    seed_trace(ctx, "run summary", ps.trace_t0);
    if (!nruns) return MAUVE_OK;                               // no run that matters to any pair: no candidate
    // one candidate list per group: a pair has at most one hit per window of its lower genome, the lower genomes of a group are
    // different, so a group has at most P candidates (a single pass: P / 2, "a hit needs two entries" -- not enough here)
    HIPCHK(ctx, ctx->cand.ensure(((size_t)P + 1) * 4));
    ps.cand_cap = list_cap ? std::min<uint32_t>(P + 1, list_cap) : P + 1;
    std::vector<char> used(passes.size(), 0);
    for (size_t left = passes.size(); left;) {
        PairGroup grp; memset(&grp, 0, sizeof grp);
        uint32_t amask = 0, maxslice = 0, slices = 0;
        for (size_t q = 0; q < passes.size(); q++) {
            if (used[q]) continue;
            const int ga = __builtin_ctz(passes[q].consider), gb = 31 - __builtin_clz(passes[q].consider);
            if (amask >> ga & 1u) continue;
            used[q] = 1; left--;
            // the hit table is indexed by the anchor's window = a window of the lowest genome of the pass: a pass over one genome pair
            // (the guide tree runs N (N - 1) / 2 of them) clears and scans that genome's slice only
            const uint32_t lo = tab.gpos_off[ga], hi = std::min<uint32_t>(tab.gpos_off[ga + 1], P);
            if (hi <= lo) continue;                            // (a genome shorter than the seed has no window: nothing can be anchored in it)
            grp.ga[grp.n] = ga; grp.gb[grp.n] = gb; grp.lo[grp.n] = lo; grp.hi[grp.n] = hi; grp.n++;
            amask |= 1u << ga; maxslice = std::max(maxslice, hi - lo); slices += hi - lo;
        }
        if (!grp.n) continue;
        for (int y = 0; y < grp.n; y++) HIPCHK(ctx, hipMemsetAsync(ps.tmask + grp.lo[y], 0, (size_t)(grp.hi[y] - grp.lo[y]) * 4, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(ctx->counters.p, 0, 64, ctx->stream));
        { KernelTimer t(ctx, MAUVE_K_JOIN, nruns);
          hipLaunchKernelGGL(join_pair_group<ValT>, dim3((nruns + 255) / 256), dim3(256), 0, ctx->stream, ps.vals, tab, rstart, rlen, runiq, nruns, grp, ps.tmask, ps.tpos); }
        HIPCHK(ctx, hipGetLastError());
        seed_trace(ctx, "join", ps.trace_t0);
        { KernelTimer t(ctx, MAUVE_K_RUNS, slices);
          with_runs_items(runs_items(ctx, maxslice), [&](auto items) {
              constexpr int ITEMS = decltype(items)::value;
              hipLaunchKernelGGL(mum_runs_group<ITEMS>, dim3((maxslice + runs_tile(ITEMS) - 1) / runs_tile(ITEMS), (uint32_t)grp.n), dim3(256), 0, ctx->stream, tab, ps.sh.span, ps.tmask,
                                 ps.tpos, grp, ps.rq.extend ? 0 : 1, ctx->cand.as<uint32_t>(), ctx->counters.as<uint32_t>(), ps.cand_cap);
          }); }
        HIPCHK(ctx, hipGetLastError());
        if (ctx->shadow) { std::function<void()> f; f.swap(ctx->shadow); f(); }
        if (int rc = seed_counters(ctx, 16, &cw)) return rc;
        const uint32_t nc = cw[1];
        if (cand_overflow(ps, nc)) return MAUVE_ERR_LIMIT;
        seed_trace(ctx, "runs", ps.trace_t0);
        if (switches().trace) fprintf(stderr, "[trace]   %u candidates of %u windows (%d pairs at once)\n", nc, slices, grp.n);
        if (nc == 0) continue;
        if (int rc = extend_candidates<false, WIDEV>(ps, nc, 256 * 8)) return rc;
    }
    return MAUVE_OK;
}

// A tiny pass (a round of the LCB extension, a small guide-tree node, a small recursion batch) is a handful of 5-10 us kernels: the round
// trip that fetched the candidate count before the extension kernel could be launched cost as much as the pass.  Its candidate list has
// at most a few thousand entries, so the extension is launched for the CAPACITY of the list with the count left on the device, and the
// counters come back together with the records: one synchronisation per pass instead of two.
// The records and the counters go straight into page-locked host memory (the device writes it in place: a handful of candidates), so the
// round trip is one synchronisation and no copy kernel.  (Not when the canonical order is to be made on the device -- a test setting for
// lists this small: then the records stay in device memory and are copied as well.)
// (A tiny pass is the only finder pass of its call -- seed_plan: no host hits, not pairwise -- and tiny_join clears the hit table for itself.)
static_assert(TJ_MAX / 2 + 1 <= 8192, "a tiny pass's candidate list: extension launched for its capacity");
template <bool SEG, bool WIDEV>
static int tiny_pass(SeedState &st, const FinderPass &fp)
{
    mauve_ctx *ctx = st.ctx; const uint32_t P = st.P, cand_cap = st.cand_cap; const int N = st.tab.nseq;
    // (tiny_join needs more LDS than a launch gets by default.  A static of every instantiation: asked for at least once for each of the two kernels)
    static const bool tj_attr = hipFuncSetAttribute(reinterpret_cast<const void *>(tiny_join<WIDEV>), hipFuncAttributeMaxDynamicSharedMemorySize, TJ_SLOTS * 8) == hipSuccess;
    if (!tj_attr) { ctx->err = "tiny_join: cannot reserve its LDS"; return MAUVE_ERR_HIP; }
    { KernelTimer t(ctx, MAUVE_K_JOIN, P);
      hipLaunchKernelGGL(tiny_join<WIDEV>, dim3(1), dim3(1024), TJ_SLOTS * 8, ctx->stream, st.packed, st.tab, st.sh, P, st.vmask, st.cmask, fp.rule, fp.want, st.tmask, st.tpos,
                         ctx->counters.as<uint32_t>() + 9, SEG ? st.rq.seg : (const uint32_t *)nullptr, st.rq.nseg, ctx->counters.as<uint32_t>(), 0u, P); }
    HIPCHK(ctx, hipGetLastError());
    seed_trace(ctx, "join", st.trace_t0);
    if (int rc = launch_runs<SEG>(st, WinRange{0u, P})) return rc;
    if (ctx->shadow) { std::function<void()> f; f.swap(ctx->shadow); f(); }     // host work that does not depend on the pass: the kernels above are still running
    const size_t lbytes = ((size_t)cand_cap * 4 + 63) & ~(size_t)63, sbytes = (size_t)cand_cap * 4 * N;
    HIPCHK(ctx, ctx->pin_seed.ensure(64 + lbytes + sbytes));
    char *pin = ctx->pin_seed.as<char>();
    const bool host_out = cand_cap < (uint32_t)switches().canon_device_min;
    if (!host_out) { HIPCHK(ctx, ctx->mlen.ensure((size_t)cand_cap * 4 + 4)); HIPCHK(ctx, ctx->mstart.ensure((size_t)cand_cap * 4 * N + 4)); }
    int32_t *o_len = host_out ? reinterpret_cast<int32_t *>(pin + 64) : ctx->mlen.as<int32_t>();
    int32_t *o_st = host_out ? reinterpret_cast<int32_t *>(pin + 64 + lbytes) : ctx->mstart.as<int32_t>();
    if (int rc = launch_extend<SEG, WIDEV>(st, std::min<uint32_t>((cand_cap + 3) / 4, 512), cand_cap, o_len, o_st, ctx->counters.as<uint32_t>() + 1,
                                           reinterpret_cast<uint32_t *>(pin))) return rc;
    if (!host_out) {
        HIPCHK(ctx, hipMemcpyAsync(pin + 64, ctx->mlen.p, (size_t)cand_cap * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(pin + 64 + lbytes, ctx->mstart.p, sbytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t nc = reinterpret_cast<const uint32_t *>(pin)[1];
    if (reinterpret_cast<const uint32_t *>(pin)[9]) { ctx->err = "tiny_join: anchor out of range (internal error)"; return MAUVE_ERR_HIP; }
    if (cand_overflow(st, nc)) return MAUVE_ERR_LIMIT;
    seed_trace(ctx, "runs + extend (one round trip)", st.trace_t0);
    if (switches().trace) fprintf(stderr, "[trace]   %u candidates of %u windows\n", nc, P);
    ctx->sdh.hl.assign(reinterpret_cast<const int32_t *>(pin + 64), reinterpret_cast<const int32_t *>(pin + 64) + nc);
    ctx->sdh.hs.assign(reinterpret_cast<const int32_t *>(pin + 64 + lbytes), reinterpret_cast<const int32_t *>(pin + 64 + lbytes) + (size_t)nc * N);
    st.cand_total = nc; st.records_on_host = true;
    return MAUVE_OK;
}

// Ranges join_hash declined (a bucket beyond its LDS table): full sort + serial join of each slice, or of the whole list when there
// are more of them than the list holds; then the run detection again.  *nc: the candidates after it.
template <typename KeyT, bool SEG, typename ValT>
static int join_overflow_slices(SeedPass<KeyT, ValT> &ps, const FinderPass &fp, uint32_t novf, uint32_t *nc)
{
    mauve_ctx *ctx = ps.ctx; KeyT *keys = ps.keys; ValT *vals = ps.vals;
    std::vector<uint32_t> rng;
    if (novf > (uint32_t)HJ_OVF_CAP) rng = {0u, ps.ns};
    else {
        rng.resize(2 * (size_t)novf);
        HIPCHK(ctx, hipMemcpy(rng.data(), ctx->join_ovf.as<uint32_t>() + 2, rng.size() * 4, hipMemcpyDeviceToHost));
    }
    KeyT *alt_k = keys == ctx->keysA.as<KeyT>() ? ctx->keysB.as<KeyT>() : ctx->keysA.as<KeyT>();
    ValT *alt_v = vals == ctx->valsA.as<ValT>() ? ctx->valsB.as<ValT>() : ctx->valsA.as<ValT>();
    // each slice sorted in full where it lies (the sorted pairs end up in this buffer or the other one), then ONE join over all slices
    const size_t nsl = rng.size() / 2;
    std::vector<uint32_t> sl_lo(nsl), sl_pre(nsl + 1, 0);
    uint64_t tot_sl = 0;
    for (size_t q = 0; q < nsl; q++) {
        const uint32_t s0 = rng[2 * q], cnt = rng[2 * q + 1] - rng[2 * q];
        KeyT *kp = keys + s0; ValT *vp = vals + s0;
        if (int rc = sort_pairs<KeyT, ValT>(ctx, cnt, ps.pl.full_bits, &kp, &vp, alt_k + s0, alt_v + s0, false, MAUVE_K_JOIN)) return rc;
        if (kp != keys + s0) {           // an odd number of passes: the slice now lies in the other buffer -- copy it back
            HIPCHK(ctx, hipMemcpyAsync(keys + s0, kp, (size_t)cnt * sizeof(KeyT), hipMemcpyDeviceToDevice, ctx->stream));
            HIPCHK(ctx, hipMemcpyAsync(vals + s0, vp, (size_t)cnt * sizeof(ValT), hipMemcpyDeviceToDevice, ctx->stream));
        }
        sl_lo[q] = s0; tot_sl += cnt; sl_pre[q + 1] = (uint32_t)tot_sl;
    }
    if (tot_sl) {
        HIPCHK(ctx, ctx->join_bound.ensure((2 * nsl + 1) * 4));
        HIPCHK(ctx, ctx->pin_seed.ensure(64 + (2 * nsl + 1) * 4));
        uint32_t *hp = reinterpret_cast<uint32_t *>(ctx->pin_seed.as<char>() + 64);
        memcpy(hp, sl_lo.data(), nsl * 4); memcpy(hp + nsl, sl_pre.data(), (nsl + 1) * 4);
        HIPCHK(ctx, hipMemcpyAsync(ctx->join_bound.p, hp, (2 * nsl + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
        KernelTimer t(ctx, MAUVE_K_JOIN, (uint32_t)tot_sl);
        hipLaunchKernelGGL((mum_join_slices<KeyT, SEG, ValT>), dim3((uint32_t)((tot_sl + 255) / 256)), dim3(256), 0, ctx->stream, (const KeyT *)keys, (const ValT *)vals,
                           ctx->join_bound.as<uint32_t>(), ctx->join_bound.as<uint32_t>() + nsl, (uint32_t)nsl, ps.tab, fp.rule, fp.want,
                           fp.consider, ps.tmask, ps.tpos, (int)ps.pl.has_invalid);
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));     // the page-locked slice table is reused by the counter copy below
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemsetAsync(ctx->counters.p, 0, 64, ctx->stream));
    if (int rc = launch_runs<SEG>(ps, anchor_range(ps.tab, ps.P, fp, false))) return rc;
    const uint32_t *cw;
    if (int rc = seed_counters(ctx, 16, &cw)) return rc;
    *nc = cw[1];
    if (switches().trace) fprintf(stderr, "[trace]   join_hash handed back %u range(s)\n", novf);
    return MAUVE_OK;
}

// One finder pass that is neither tiny nor part of a pair group: clear the hit table where the pass can anchor a hit (anchor_range), fill
// it (host hits, join_hash or mum_join: seed_plan), run detection over that range, extension.
template <typename KeyT, bool SEG, typename ValT>
static int finder_pass(SeedPass<KeyT, ValT> &ps, const FinderPass &fp)
{
    constexpr bool WIDEV = sizeof(ValT) == 8;
    mauve_ctx *ctx = ps.ctx; const uint32_t P = ps.P, ns = ps.ns; const int N = ps.tab.nseq;
    const HostHits *hh = ps.rq.hits;
    const WinRange ar = anchor_range(ps.tab, P, fp, hh != nullptr);
    const uint32_t clr_lo = ar.lo >= RUNS_HALO ? ar.lo - RUNS_HALO : 0u;       // mum_runs reads the mask words one halo in front of its first tile
    hipLaunchKernelGGL(pass_clear, dim3((ar.hi - clr_lo + 3) / 1024 + 1), dim3(256), 0, ctx->stream, ps.tmask + clr_lo, ar.hi - clr_lo, ctx->counters.as<uint32_t>());
    if (hh) {
        HIPCHK(ctx, ctx->run_sum.ensure((size_t)hh->n * (N + 1) * 4 + 64));
        HIPCHK(ctx, hipMemcpyAsync(ctx->run_sum.p, hh->rec, (size_t)hh->n * (N + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
        if (hh->n) hipLaunchKernelGGL(hits_scatter<WIDEV>, dim3((hh->n + 255) / 256), dim3(256), 0, ctx->stream, ctx->run_sum.as<uint32_t>(), hh->n, N, P, ps.tmask, ps.tpos, ps.tab);
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // the host records must outlive the copy
    } else if (ps.pl.hash_path) {
        const uint32_t nchunk = (ns + HJ_T - 1) / HJ_T;
        HIPCHK(ctx, ctx->join_ovf.ensure((2 + 2 * (size_t)HJ_OVF_CAP) * 4));        // the ranges; their count sits in the counter block (words 8, 9)
        KernelTimer t(ctx, MAUVE_K_JOIN, ns);
        HIPCHK(ctx, ctx->join_bound.ensure(((size_t)nchunk + 2) * 4));
        hipLaunchKernelGGL((join_bounds<KeyT>), dim3((nchunk + 1 + 3) / 4), dim3(256), 0, ctx->stream, ps.keys, ns, ps.L, nchunk,
                           ctx->join_bound.as<uint32_t>());
#define JH_LAUNCH(W) hipLaunchKernelGGL((join_hash<KeyT, W, ValT>), dim3(nchunk), dim3(256), 0, ctx->stream, ps.keys, ps.vals, ns, \
                                           ctx->join_bound.as<uint32_t>(), ps.tab, fp.rule, fp.want, ps.tmask, ps.tpos, ctx->counters.as<uint32_t>() + 8, ctx->join_ovf.as<uint32_t>(), P)
        if (N > 16) JH_LAUNCH(true);
        else JH_LAUNCH(false);
#undef JH_LAUNCH
    } else
    { KernelTimer t(ctx, MAUVE_K_JOIN, ns);
      hipLaunchKernelGGL((mum_join<KeyT, SEG, ValT>), dim3((ns + 255) / 256), dim3(256), 0, ctx->stream, ps.keys, ps.vals, ns, ps.tab, fp.rule,
                         fp.want, fp.consider, ps.tmask, ps.tpos, P, (int)ps.pl.has_invalid); }
    HIPCHK(ctx, hipGetLastError());
    seed_trace(ctx, "join", ps.trace_t0);
    if (int rc = launch_runs<SEG>(ps, ar)) return rc;
    if (ctx->shadow) { std::function<void()> f; f.swap(ctx->shadow); f(); }     // host work that does not depend on the pass: the kernels above are still running
    const uint32_t *cw;
    if (int rc = seed_counters(ctx, 48, &cw)) return rc;     // run counters + join_hash's overflow count
    uint32_t nc = cw[1];
    const uint32_t novf = ps.pl.hash_path ? cw[8] : 0u;
    if (ps.pl.hash_path && cw[9]) { ctx->err = "join_hash: anchor out of range (internal error)"; return MAUVE_ERR_HIP; }
    if (novf) if (int rc = join_overflow_slices<KeyT, SEG, ValT>(ps, fp, novf, &nc)) return rc;
    if (cand_overflow(ps, nc)) return MAUVE_ERR_LIMIT;
    seed_trace(ctx, "runs", ps.trace_t0);
    if (switches().trace) fprintf(stderr, "[trace]   %u candidates of %u windows\n", nc, P);
    if (nc == 0) return MAUVE_OK;
    // six waves per SIMD fit (77 registers); two rounds of workgroups even out the candidates' different lengths (measured: 5 .. 8 per compute unit
    // within 5 % of each other, 12 .. 14 another 10 % faster)
    constexpr int EXT_BLOCKS_PER_CU = 12;
    return extend_candidates<SEG, WIDEV>(ps, nc, (uint32_t)(ctx->cus * EXT_BLOCKS_PER_CU));
}

// One seed pass over a genome set: extraction, sort, then an export or the finder passes and the common finish (seed_finish.hip).
// SEG: the set is segmented (recursive anchoring).  Results land in ctx->match_len / match_start (canonical order).
template <typename KeyT, bool SEG, typename ValT>
static int seedpass_stages(const SeedState &st0)
{
    constexpr bool WIDEV = sizeof(ValT) == 8;
    SeedPass<KeyT, ValT> ps(st0);
    mauve_ctx *ctx = ps.ctx; const SeedRequest &rq = ps.rq; const uint32_t P = ps.P; const int N = ps.tab.nseq;
    if (switches().trace) fprintf(stderr, "[trace] seed pass: %u windows, %d-bit keys, %s window index (%d-bit values)\n", P, (int)sizeof(KeyT) * 8,
                                  WIDEV ? "wide" : "narrow", (int)sizeof(ValT) * 8);
    if (int rc = seed_plan(ctx, ps.sh, ps.tab, rq, P, ps.vmask || ps.cmask, SEG, (int)sizeof(KeyT) * 8, &ps.pl, &ps.passes)) return rc;
    if (int rc = extract<KeyT, SEG, ValT>(ps)) return rc;
    if (ps.ns == 0) { if (rq.n_matches) *rq.n_matches = 0; return MAUVE_OK; }
    ps.L = ps.pl.low_bits(ps.ns);
    if (!rq.hits && !ps.pl.tiny)
        if (int rc = sort_pairs<KeyT, ValT>(ctx, ps.ns, ps.pl.full_bits, &ps.keys, &ps.vals, ctx->keysB.as<KeyT>(), ctx->valsB.as<ValT>(), ps.have_hist0, -1, ps.L, ps.iota)) return rc;
    seed_trace(ctx, "sort", ps.trace_t0);
    if (rq.enumerate) return export_enumerator(ps);
    if (rq.out_keys) return export_sorted_list(ps);

    // ---- join + extension, once per finder pass ----
    HIPCHK(ctx, ctx->posmask.ensure((size_t)P * 4));             // tmask
    HIPCHK(ctx, ctx->hit_pos.ensure((size_t)P * 4 * N));         // tpos [P][N]
    ps.tmask = ctx->posmask.as<uint32_t>(); ps.tpos = ctx->hit_pos.as<uint32_t>();
    ps.cand_cap = P / 2 + 1;                                     // a hit needs >= 2 entries
    HIPCHK(ctx, ctx->cand.ensure((size_t)ps.cand_cap * 4));
    if (switches().list_cap) ps.cand_cap = std::min(ps.cand_cap, switches().list_cap);
    ctx->sdh.hl.clear(); ctx->sdh.hs.clear();                    // (host scratch kept across calls)
    if (ps.pl.tiny) {
        if (int rc = tiny_pass<SEG, WIDEV>(ps, ps.passes[0])) return rc;
    } else if (ps.pl.use_summary) {
        if (int rc = pairwise_passes(ps)) return rc;
    } else {
        for (const FinderPass &fp : ps.passes)
            if (int rc = finder_pass<KeyT, SEG, ValT>(ps, fp)) return rc;
    }
    return seed_finish(ctx, ps.gs, rq, ps.cand_total, ps.records_on_host, ps.trace_t0);
}

// what every entry point starts with: the seed's shape, the genomes the request is about (seq: one sequence; nullptr: all of them), the window table
static int seedpass_prologue(mauve_ctx *ctx, const GenomeSet &gs, uint64_t pattern, const int *seq, SeedShape *sh, GenomeTab *tab, int64_t *total)
{
    if (!make_seed_shape(pattern, sh)) { ctx->err = "seed pattern must be palindromic, span <= 49, weight <= 31"; return MAUVE_ERR_ARG; }
    if (!seq && gs.nseq < 1) { ctx->err = "no genomes set"; return MAUVE_ERR_STATE; }
    if (seq && (*seq < 0 || *seq >= gs.nseq)) { ctx->err = "sequence index out of range"; return MAUVE_ERR_ARG; }
    return build_tab(ctx, gs, sh->span, tab, total);
}

static void reset_match_list(mauve_ctx *ctx, int64_t *n_matches)
{
    ctx->n_matches = 0; ctx->match_len.clear(); ctx->match_start.clear(); ctx->matches_pending = false;
    ctx->dev_rec_n = -1;
    if (n_matches) *n_matches = 0;
}

// the instantiation of a pass: key width by the seed weight (64 bits when segmented), value width by seedpass_wide
static int seedpass_dispatch(mauve_ctx *ctx, const GenomeSet &gs, const SeedShape &sh, const GenomeTab &tab, int64_t total, const SeedRequest &rq)
{
    SeedState st{ctx, gs, sh, tab, rq, (uint32_t)total, gs.buf->as<uint64_t>(), gs.vmask ? gs.vmask->as<uint64_t>() : nullptr,
                 gs.cmask ? gs.cmask->as<uint64_t>() : nullptr};
    st.trace_t0 = now_ms();
    const bool wide = seedpass_wide(total);
    if (rq.seg) return wide ? seedpass_stages<uint64_t, true, uint64_t>(st) : seedpass_stages<uint64_t, true, uint32_t>(st);
    if (2 * sh.weight <= 32) return wide ? seedpass_stages<uint32_t, false, uint64_t>(st) : seedpass_stages<uint32_t, false, uint32_t>(st);
    return wide ? seedpass_stages<uint64_t, false, uint64_t>(st) : seedpass_stages<uint64_t, false, uint32_t>(st);
}

int seedpass_run(mauve_ctx *ctx, const GenomeSet &gs, uint64_t pattern, int mode, uint64_t mask, int extend,
                 const uint32_t *seg_dev, uint32_t nseg, int64_t *n_matches)
{
    SeedShape sh; GenomeTab tab; int64_t total = 0;
    if (int rc = seedpass_prologue(ctx, gs, pattern, nullptr, &sh, &tab, &total)) return rc;
    reset_match_list(ctx, n_matches);
    if (total == 0) return MAUVE_OK;
    SeedRequest rq;
    rq.mode = mode; rq.mask = mask; rq.extend = extend; rq.n_matches = n_matches;
    if (seg_dev) { rq.seg = seg_dev; rq.nseg = nseg; }
    return seedpass_dispatch(ctx, gs, sh, tab, total, rq);
}

// extension + canonical order of hits a host-side finder supplies (records of 1 + nseq words: component set, values -- global window
// index | strand << 31, or local to the genome when seedpass_wide says so for the genome set: api.cpp builds them by the same rule)
int seedpass_from_hits(mauve_ctx *ctx, const GenomeSet &gs, uint64_t pattern, const HostHits &hits, int extend, int64_t *n_matches)
{
    SeedShape sh; GenomeTab tab; int64_t total = 0;
    if (int rc = seedpass_prologue(ctx, gs, pattern, nullptr, &sh, &tab, &total)) return rc;
    reset_match_list(ctx, n_matches);
    if (total == 0 || hits.n == 0) return MAUVE_OK;
    SeedRequest rq;
    rq.mode = MAUVE_MODE_MEM; rq.extend = extend; rq.hits = &hits; rq.n_matches = n_matches;
    return seedpass_dispatch(ctx, gs, sh, tab, total, rq);
}

// SeedMatchEnumerator::FindMatches of sequence `seq` on the device; q carries the rule in and the CSR result out
int seedpass_enumerate(mauve_ctx *ctx, const GenomeSet &gs, int seq, uint64_t pattern, EnumRequest &q)
{
    SeedShape sh; GenomeTab tab; int64_t total = 0;
    if (int rc = seedpass_prologue(ctx, gs, pattern, &seq, &sh, &tab, &total)) return rc;
    q.n = 0; q.ns = 0;
    if (tab.nwin[seq] == 0) { if (q.start_off) q.start_off[0] = 0; return MAUVE_OK; }
    SeedRequest rq;
    rq.mode = 0; rq.only_seq = seq; rq.enumerate = &q;
    return seedpass_dispatch(ctx, gs, sh, tab, total, rq);
}

int seedpass_sorted_list(mauve_ctx *ctx, const GenomeSet &gs, int seq, uint64_t pattern, std::vector<uint64_t> *keys,
                         std::vector<uint32_t> *vals, int *weight)
{
    SeedShape sh; GenomeTab tab; int64_t total = 0;
    if (int rc = seedpass_prologue(ctx, gs, pattern, &seq, &sh, &tab, &total)) return rc;
    *weight = sh.weight;
    keys->clear(); vals->clear();
    if (tab.nwin[seq] == 0) return MAUVE_OK;
    SeedRequest rq;
    rq.mode = 0; rq.only_seq = seq; rq.out_keys = keys; rq.out_vals = vals;
    if (int rc = seedpass_dispatch(ctx, gs, sh, tab, total, rq)) return rc;
    // vals carry global window indices; make them local to the genome (a wide pass hands them out local already)
    if (!seedpass_wide(total))
        for (auto &v : *vals) v = ((v & 0x7fffffffu) - tab.gpos_off[seq]) | (v & 0x80000000u);
    return MAUVE_OK;
}

// ------------------------------------------------------------------------------------------------
// repeat multiplicity of every base: the extract and the radix sort of the seed pass over all windows of the
// resident genomes, then
//   rp_count    : every window learns the size of its (canonical mer, genome) run in the sorted list -- the sort is stable on the
//                 global window index, so a genome's windows of one mer are contiguous inside the mer's run -- saturated at 255,
//                 and stores it at its window index (a byte per window; 0 = invalid window: contig join or ambiguous base)
//   rp_span_min : per genome, 4096 positions per workgroup: the window counts of the tile and its span-1 halo in LDS, each thread
//                 the minimum over the covering windows of four consecutive positions (1 where none is valid), one 4-byte store
// ------------------------------------------------------------------------------------------------
template <typename KeyT, typename ValT = uint32_t>
__global__ void __launch_bounds__(256) rp_count(const KeyT *__restrict__ keys, const ValT *__restrict__ vals, uint32_t n, GenomeTab tab,
                                                uint8_t *__restrict__ wcnt)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const KeyT k = keys[i];
        const uint32_t w = win_idx(vals[i]);
        if (k == (KeyT)~0ULL) { wcnt[w] = 0; continue; }
        const int g = genome_of(w, tab);
        const uint32_t lo = tab.gpos_off[g], hi = tab.gpos_off[g + 1];
        uint32_t c = 1;                                        // the walks stop at the saturation count: at most 254 steps each way
        for (uint32_t j = i; j > 0 && c < 255u; j--) {
            const uint32_t v = win_idx(vals[j - 1]);
            if (keys[j - 1] != k || v < lo || v >= hi) break;
            c++;
        }
        for (uint32_t j = i + 1; j < n && c < 255u; j++) {
            const uint32_t v = win_idx(vals[j]);
            if (keys[j] != k || v < lo || v >= hi) break;
            c++;
        }
        wcnt[w] = (uint8_t)c;
    }
}

constexpr int RP_TILE = 4096;
struct RpOut { int64_t len[MAUVE_MAX_SEQ]; uint64_t off[MAUVE_MAX_SEQ]; };
__global__ void __launch_bounds__(256) rp_span_min(const uint8_t *__restrict__ wcnt, GenomeTab tab, RpOut o, int span, uint8_t *__restrict__ mult)
{
    // c[t] = count of window p0 - (span - 1) + t, t < RP_TILE + span - 1 (0 outside the genome's windows)
    __shared__ uint8_t c[RP_TILE + MAUVE_MAX_SEED_SPAN];
    const int g = blockIdx.y;
    const int64_t L = o.len[g];
    const int64_t p0 = (int64_t)blockIdx.x * RP_TILE;
    if (p0 >= L) return;                                       // (the grid is sized for the longest genome; uniform per workgroup)
    const int64_t nw = tab.nwin[g], w0 = p0 - (span - 1);
    const uint8_t *W = wcnt + tab.gpos_off[g];
    for (int t = threadIdx.x; t < RP_TILE + span - 1; t += 256) {
        const int64_t w = w0 + t;
        c[t] = (w >= 0 && w < nw) ? W[w] : (uint8_t)0;
    }
    __syncthreads();
    uint8_t *out = mult + o.off[g];
#pragma unroll 1
    for (int i = 0; i < 4; i++) {
        const int j = i * 1024 + (int)threadIdx.x * 4;        // position p0 + j + k covers the windows at t = j + k .. j + k + span - 1
        const int64_t p = p0 + j;
        if (p >= L) break;
        uint32_t m0 = 256, m1 = 256, m2 = 256, m3 = 256;       // 256: no valid window yet
        for (int t = 0; t < span + 3; t++) {
            uint32_t v = c[j + t]; v = v ? v : 256u;
            if (t < span) m0 = min(m0, v);
            if (t >= 1 && t < span + 1) m1 = min(m1, v);
            if (t >= 2 && t < span + 2) m2 = min(m2, v);
            if (t >= 3) m3 = min(m3, v);
        }
        const uint32_t b = (m0 & 255u ? m0 : 1u) | (m1 & 255u ? m1 : 1u) << 8 | (m2 & 255u ? m2 : 1u) << 16 | (m3 & 255u ? m3 : 1u) << 24;
        if (p + 3 < L) *reinterpret_cast<uint32_t *>(out + p) = b;     // (o.off and p are multiples of 4)
        else for (int k = 0; k < 4 && p + k < L; k++) out[p + k] = (uint8_t)(b >> (8 * k));
    }
}
static_assert(RP_TILE == RS_TILE, "the multiplicity pass sorts with the histograms seed_extract_all leaves, tiled like the radix sort");

template <typename KeyT, typename ValT>
static int rp_windows(mauve_ctx *c, const GenomeSet &gs, const SeedShape &sh, const GenomeTab &tab, uint32_t n)
{
    if (switches().trace) fprintf(stderr, "[trace] multiplicity pass: %u windows, %s window index (%d-bit values)\n", n, sizeof(ValT) == 8 ? "wide" : "narrow", (int)sizeof(ValT) * 8);
    if (int rc = ensure_sort_buffers<KeyT, ValT>(c, n)) return rc;
    KeyT *keys = c->keysA.as<KeyT>(); ValT *vals = c->valsA.as<ValT>();
    if (int rc = extract_all<KeyT, false, ValT>(c, gs, sh, tab, n, nullptr, 0u, 0, keys, vals)) return rc;
    HIPCHK(c, hipGetLastError());
    // the mer bits only: an invalid window's all-ones key has ones there that no canonical mer has (min(F, R) is never all T),
    // so the invalid windows end the list
    if (int rc = sort_pairs<KeyT, ValT>(c, n, 2 * sh.weight, &keys, &vals, c->keysB.as<KeyT>(), c->valsB.as<ValT>(), true)) return rc;
    hipLaunchKernelGGL((rp_count<KeyT, ValT>), dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)c->cus * 16)), dim3(256), 0, c->stream, keys, vals, n, tab,
                       c->rp_wcnt.as<uint8_t>());
    HIPCHK(c, hipGetLastError());
    return MAUVE_OK;
}

int repeat_multiplicity(mauve_ctx *c, uint64_t pattern)
{
    const GenomeSet gs = main_genome_set(c);
    SeedShape sh; GenomeTab tab; int64_t total = 0;
    if (int rc = seedpass_prologue(c, gs, pattern, nullptr, &sh, &tab, &total)) return rc;
    if (c->rp_gen == c->genome_gen && c->rp_pat == pattern) return MAUVE_OK;
    c->rp_gen = 0;                                             // (nothing valid while it is rebuilt)
    RpOut o; memset(&o, 0, sizeof o);
    c->rp_off.assign((size_t)c->nseq, 0);
    uint64_t bytes = 0; int64_t maxlen = 0;
    for (int g = 0; g < c->nseq; g++) {
        o.len[g] = c->lens[(size_t)g]; o.off[g] = bytes; c->rp_off[(size_t)g] = bytes;
        bytes += ((uint64_t)c->lens[(size_t)g] + 15) & ~(uint64_t)15;
        maxlen = std::max(maxlen, c->lens[(size_t)g]);
    }
    HIPCHK(c, c->rp_mult.ensure(bytes + 16));
    HIPCHK(c, c->rp_wcnt.ensure((size_t)total + 16));
    if (total > 0) {
        const bool wide = seedpass_wide(total);
        int rc;
        if (2 * sh.weight <= 32) rc = wide ? rp_windows<uint32_t, uint64_t>(c, gs, sh, tab, (uint32_t)total) : rp_windows<uint32_t, uint32_t>(c, gs, sh, tab, (uint32_t)total);
        else rc = wide ? rp_windows<uint64_t, uint64_t>(c, gs, sh, tab, (uint32_t)total) : rp_windows<uint64_t, uint32_t>(c, gs, sh, tab, (uint32_t)total);
        if (rc) return rc;
    }
    if (maxlen > 0) {
        hipLaunchKernelGGL(rp_span_min, dim3((uint32_t)((maxlen + RP_TILE - 1) / RP_TILE), (uint32_t)c->nseq), dim3(256), 0, c->stream,
                           c->rp_wcnt.as<uint8_t>(), tab, o, sh.span, c->rp_mult.as<uint8_t>());
        HIPCHK(c, hipGetLastError());
    }
    c->rp_gen = c->genome_gen; c->rp_pat = pattern;
    return MAUVE_OK;
}
