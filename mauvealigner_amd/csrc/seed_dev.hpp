// seed_dev.hpp -- device helpers of the seed pass that more than one translation unit needs: windows, canonical mers and sort values
// (seed_pass.hip's extraction; the repeat map's, repeat_dev.hip) and the diagonal walk of the ungapped extension (mum_extend, DESIGN.md S4;
// rm_extend, S20): the component table, the agreement test of 64 offsets at a time and the walk over its bitmap.
#pragma once
#include "common.hpp"

// ------------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------------
// bits [r, r + 64) of the word pair w1:w0, r < 64
__device__ __forceinline__ uint64_t funnel64(uint64_t w0, uint64_t w1, int r) { return r ? ((w0 >> r) | (w1 << (64 - r))) : w0; }

// placed-base bitmap: is any of the `span` bases from p on already placed?
__device__ __forceinline__ bool window_masked(const uint64_t *__restrict__ M, uint32_t p, int span)
{
    const uint32_t q = p >> 6; const int r = p & 63;
    const uint64_t m0 = M[q], m1 = M[q + 1];
    const uint64_t v = r ? ((m0 >> r) | (m1 << (64 - r))) : m0;      // (written out: through funnel64, valid_count compiles to 16 VGPRs instead of 12)
    return (v & ((span >= 64) ? ~0ULL : ((1ULL << span) - 1ULL))) != 0;
}

// Is the window starting at base p unusable?  VM: 1 bit per base, set = no window may touch it (an ancestor placed it,
// DESIGN.md S9; or it is an ambiguous base, mauve_set_genomes_contigs); CM: 1 bit per base, set = a contig starts
// here -- a window may begin at such a base but not run across it (RepeatHashCat.h:19-20).  Either may be null.
__device__ __forceinline__ bool window_blocked(const uint64_t *__restrict__ VM, const uint64_t *__restrict__ CM, uint32_t p, int span)
{
    bool b = false;
    if (VM) b = window_masked(VM, p, span);
    if (CM && span > 1) b |= window_masked(CM, p + 1, span - 1);
    return b;
}

__device__ __forceinline__ uint32_t digit_reverse32(uint32_t k, int weight)
{
    uint32_t x = __brev(k) >> (32 - 2 * weight);
    return ((x & 0xAAAAAAAAu) >> 1) | ((x & 0x55555555u) << 1);
}

__device__ __forceinline__ uint64_t digit_reverse64(uint64_t x)
{
    x = __brevll(x);
    return ((x & 0xAAAAAAAAAAAAAAAAULL) >> 1) | ((x & 0x5555555555555555ULL) << 1);
}

// reverse the order of the 2-bit digits of a 2*weight-bit value
__device__ __forceinline__ uint64_t digit_reverse(uint64_t k, int weight)
{
    uint64_t x = __brevll(k) >> (64 - 2 * weight);
    return ((x & 0xAAAAAAAAAAAAAAAAULL) >> 1) | ((x & 0x5555555555555555ULL) << 1);
}

// The canonical mer of a window, in the two steps every extraction site shares.  NARROW (seed_narrow): the window is one 64-bit word and
// K' fits 32 bits, so the arithmetic is 32-bit; otherwise the window is a 128-bit digit string.
__host__ __device__ inline bool seed_narrow(const SeedShape &sh) { return sh.span <= 32 && sh.weight <= 15; }
struct WinDigits { uint64_t lo, hi; };      // (hi: unused when NARROW)
struct MerKey { uint64_t key; uint32_t strand; };
// 1. the digit string of the window starting at base p of the genome whose packed words start at G
template <bool NARROW>
__device__ __forceinline__ WinDigits window_digits(const uint64_t *__restrict__ G, uint32_t p)
{
    const uint32_t q = p >> 5; const int r = (p & 31) * 2;
    const uint64_t w0 = G[q], w1 = G[q + 1], w2 = NARROW ? 0ULL : G[q + 2];
    return {funnel64(w0, w1, r), NARROW ? 0ULL : funnel64(w1, w2, r)};
}
// The seed's run table in registers: a kernel makes one at its entry, in front of its window loops, and hands it to canonical_mer / mer_at.
// Every index below is a constant once the loops are unrolled, so the words are scalar loads from the kernel-argument segment that no window
// waits for.  (Read where they are used, inside a loop over the runs, every trip of every window waits for its own loads: the run count is
// a run-time value.)
template <bool NARROW>
struct SeedRuns {
    static constexpr int N = NARROW ? SEED_RUNS_NARROW : SEED_RUNS_MAX;
    uint32_t w[N], m[NARROW ? N : 1];       // NARROW: shift and mask; else the packed word of SeedShape::run_wide
    int nruns, weight; uint64_t keymask;
    __device__ __forceinline__ explicit SeedRuns(const SeedShape &sh) : nruns(sh.nruns), weight(sh.weight), keymask(sh.keymask)
    {
        m[0] = 0;
#pragma unroll
        for (int i = 0; i < N; i++) {
            if constexpr (NARROW) { w[i] = sh.run_shift[i]; m[i] = sh.run_mask[i]; }
            else w[i] = sh.run_wide[i];
        }
    }
};
// 2. K' = the seed's runs of digits, packed; forward mer = digit reverse of K', reverse mer = ~K' (masked).  The smaller one is the key,
// strand = 1 when that is the reverse mer (a mer that is its own reverse complement: strand 0).  The loop over the runs is unrolled over the
// whole table and left, wave-uniformly, after a group of SEED_RUN_GROUP runs: the table's zero entries behind the last run add nothing.
template <bool NARROW>
__device__ __forceinline__ MerKey canonical_mer(const WinDigits &d, const SeedRuns<NARROW> &R)
{
    if constexpr (NARROW) {
        uint32_t kp = 0;
#pragma unroll
        for (int i = 0; i < SeedRuns<NARROW>::N; i++) {
            if (i && i % SEED_RUN_GROUP == 0 && i >= R.nruns) break;
            kp |= (uint32_t)(d.lo >> R.w[i]) & R.m[i];
        }
        const uint32_t f = digit_reverse32(kp, R.weight), r = (~kp) & (uint32_t)R.keymask;
        return {r < f ? r : f, r < f};
    } else {
        uint64_t kp = 0;
#pragma unroll
        for (int i = 0; i < SeedRuns<NARROW>::N; i++) {
            if (i && i % SEED_RUN_GROUP == 0 && i >= R.nruns) break;
            // The word is unpacked here, by the scalar unit (it is wave-uniform), for every window anew: the empty statement keeps the compiler
            // from moving the unpacked values -- nine scalars a run -- in front of the window loops, where they do not fit the scalar
            // registers (more than 200 of them spilled into vector lanes).
            uint32_t w = R.w[i];
            asm volatile("" : "+s"(w));
            const uint32_t s = w & 0xffu, dst = (w >> 8) & 0xffu, bits = w >> 16;
            const uint64_t mask = ((1ULL << bits) - 1ULL) << dst;                                        // bits <= 62
            const bool up = s >= 64; const int r = (int)(s & 63u);
            const uint64_t a = up ? d.hi : d.lo, b = up ? 0ULL : d.hi;
            kp |= ((a >> r) | ((b << 1) << (63 - r))) & mask;                                            // bits [s, s + 64) of hi:lo
        }
        const uint64_t f = digit_reverse(kp, R.weight), r = (~kp) & R.keymask;
        return {r < f ? r : f, r < f};
    }
}
template <bool NARROW>
__device__ __forceinline__ MerKey mer_at(const uint64_t *__restrict__ G, uint32_t p, const SeedRuns<NARROW> &R) { return canonical_mer<NARROW>(window_digits<NARROW>(G, p), R); }

// genome of a global window index.  gpos_off[i] for i > nseq is all ones (build_tab), so up to eight genomes need no
// loop: seven compares against values the scalar unit loads once per kernel.
__device__ __forceinline__ int genome_of(uint32_t gpos, const GenomeTab &t)
{
    int g = 0;
    if (t.nseq <= 8) {
#pragma unroll
        for (int i = 1; i < 8; i++) g += (gpos >= t.gpos_off[i]) ? 1 : 0;
    } else
        for (int i = 1; i < t.nseq; i++) g += (gpos >= t.gpos_off[i]) ? 1 : 0;
    return g;
}
// ... and that genome's window range [lo, hi) and first packed word.  Up to eight genomes: the same seven compares pick the three values out
// of the scalar copies of the table, no memory access (indexed by a lane's genome, they are gathers from the kernel-argument segment that
// the window's own loads wait for); above eight, the indexed form.
struct GenomeAt { int g; uint32_t lo, hi, word; };               // (word: below 2^32, build_tab -- half the scalars and selects of the 64-bit offset)
__device__ __forceinline__ GenomeAt genome_at(uint32_t gpos, const GenomeTab &t)
{
    if (t.nseq <= 8) {
        GenomeAt a = {0, t.gpos_off[0], t.gpos_off[1], (uint32_t)t.word_off[0]};
#pragma unroll
        for (int i = 1; i < 8; i++) {
            const bool in = gpos >= t.gpos_off[i];
            a.g += in ? 1 : 0; a.lo = in ? t.gpos_off[i] : a.lo; a.hi = in ? t.gpos_off[i + 1] : a.hi; a.word = in ? (uint32_t)t.word_off[i] : a.word;
        }
        return a;
    }
    const int g = genome_of(gpos, t);
    return {g, t.gpos_off[g], t.gpos_off[g + 1], (uint32_t)t.word_off[g]};
}

// A sort value: global window index | strand flag.  The narrow form (uint32_t) keeps the flag in bit 31, so a pass over it holds fewer
// than 2^31 windows; the wide form (uint64_t, a pass of 2^31 windows or more) keeps it in bit 63 -- the index itself is below
// 2^32 either way, so every decoded index, and genome_of, stays 32-bit.
__device__ __forceinline__ uint32_t win_idx(uint32_t v) { return v & 0x7fffffffu; }
__device__ __forceinline__ uint32_t win_idx(uint64_t v) { return (uint32_t)v; }
__device__ __forceinline__ uint32_t win_strand(uint32_t v) { return v >> 31; }
__device__ __forceinline__ uint32_t win_strand(uint64_t v) { return (uint32_t)(v >> 63); }
template <typename ValT> __device__ __forceinline__ ValT win_make(uint32_t gp, uint32_t s)
{
    if constexpr (sizeof(ValT) == 4) return gp | (s << 31);
    else return (uint64_t)gp | ((uint64_t)s << 63);
}
// The hit table's word for a component in genome g (tpos, see mum_join): narrow, the value itself (global index | strand << 31); wide, the
// window index LOCAL to genome g | strand << 31 -- the slot names the genome and a genome holds fewer than 2^31 bases, so the table keeps
// four bytes per entry.  Only differences of two indices of the same genome (mum_runs) or the local index (mum_extend) are read back.
__device__ __forceinline__ uint32_t hit_word(uint32_t v, uint32_t) { return v; }
__device__ __forceinline__ uint32_t hit_word(uint64_t v, uint32_t goff) { return (win_idx(v) - goff) | (win_strand(v) << 31); }

// ------------------------------------------------------------------------------------------------
// the diagonal walk
// ------------------------------------------------------------------------------------------------
// One component of the hit a wave is extending: where its windows live, the window index at offset 0, its walking
// direction relative to the anchor and the window range it may use.  Built once per candidate (LDS, per wave).
struct ExtComp { const uint64_t *G; const uint64_t *VM; const uint64_t *CM; int64_t pos, lo, hi; uint32_t rev, maxw /* last word of the genome's buffer */, g, pad; };

// ---- does offset k agree? ----
// Offset k agrees when, for every component c and every care position t of the seed, S_c(k + t) == S_0(k + t), where S_c(j) is the
// component's base stream along the generalized diagonal: base(pos_c + j) for a component on the anchor's strand, the COMPLEMENT of
// base(pos_c + span - 1 - j) for one on the opposite strand (its window at pos_c - k against the reverse complement of the anchor's; the
// pattern is a palindrome, so t and span - 1 - t are care positions together).  A round of 64 offsets from j0 on needs S(j0 .. j0 + 63 +
// span - 1): 128 digits, four words per component.  The wave builds them with its lanes side by side -- eight lanes per component, lane i
// of a group fetches word i of the stretch (ONE load instruction for up to eight components) -- XORs each with the anchor's, ORs the
// differences over the components and hands the four words out as wave-uniform values; a lane then cuts its window out of them and tests
// it under the care mask.  (Every lane fetching its own window, three words per component, and a version with the streams built by the
// scalar unit, both spent their time issuing instructions: 800 and 550 per round against about 200.)
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src)
{
    return (uint64_t)(uint32_t)__shfl((int)(uint32_t)v, src) | ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src) << 32);
}
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l)
{
    return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)v, l) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)(v >> 32), l) << 32);
}
// lane l <- lane l + 1 inside its row of 16 (the groups of eight never need the word of the next row)
__device__ __forceinline__ uint64_t row_next64(uint64_t v)
{
    return (uint64_t)(uint32_t)__builtin_amdgcn_update_dpp(0, (int32_t)(uint32_t)v, 0x101, 0xf, 0xf, true) |
           ((uint64_t)(uint32_t)__builtin_amdgcn_update_dpp(0, (int32_t)(uint32_t)(v >> 32), 0x101, 0xf, 0xf, true) << 32);
}
// M: OR over the components of S_c ^ S_0 for j = j0 .. j0 + 127 (two bits per digit), wave-uniform.  NJ stretches at once (the first left and
// the first right round of a candidate: their loads travel together).
template <int NJ>
__device__ __forceinline__ void ext_mismatch(const ExtComp *__restrict__ comp, int nc, int span, const int64_t (&j0)[NJ], int lane, uint64_t (&M)[NJ][4])
{
    typedef const uint64_t __attribute__((address_space(1))) *gptr;
    const int i = lane & 7, grp = lane >> 3;
    uint64_t acc[NJ], A[NJ];
#pragma unroll
    for (int t = 0; t < NJ; t++) { acc[t] = 0; A[t] = 0; }
    for (int c0 = 0; c0 < nc; c0 += 8) {                   // (wave-uniform: more than eight components only with more than eight genomes)
        const int c = c0 + grp;
        const ExtComp &C = comp[min(c, nc - 1)];
        const uint32_t rev = C.rev;
        const bool any_rev = __any(rev != 0);
        const gptr G = (gptr)(uintptr_t)C.G;
        const int64_t pos = C.pos, maxw = (int64_t)C.maxw;
        uint64_t w[NJ]; int r[NJ];
#pragma unroll
        for (int t = 0; t < NJ; t++) {
            // opposite strand: the forward stretch F that ends at base top = pos + span - 1 - j0; S digit k = ~F digit (127 - k)
            const int64_t b = rev ? pos + span - 1 - j0[t] - 127 : pos + j0[t];
            const int64_t q = b >> 5; r[t] = (int)(b & 31) * 2;
            // (b may lie outside the genome: word indices are clamped into its buffer; what they hold there only reaches offsets the bounds
            // test rejects anyway)
            int64_t x = q + i; x = x < 0 ? 0 : (x > maxw ? maxw : x);
            w[t] = G[x];
        }
#pragma unroll
        for (int t = 0; t < NJ; t++) {
            const uint64_t wn = row_next64(w[t]);          // (lanes i >= 4 compute along, unused)
            const uint64_t W = r[t] ? ((w[t] >> r[t]) | (wn << (64 - r[t]))) : w[t];
            uint64_t S = W;
            if (any_rev) { const uint64_t Wr = ~digit_reverse64(shfl64(W, (lane & ~7) | (3 - (i & 3)))); S = rev ? Wr : W; }
            if (c0 == 0) A[t] = shfl64(S, i & 3);          // the anchor (component 0, never reversed) word i, in every group
            if (c > 0 && c < nc && i < 4) acc[t] |= S ^ A[t];
        }
    }
#pragma unroll
    for (int t = 0; t < NJ; t++) {
        uint64_t v = acc[t];
        v |= shfl64(v, lane ^ 8); v |= shfl64(v, lane ^ 16); v |= shfl64(v, lane ^ 32);      // over the groups
#pragma unroll
        for (int k = 0; k < 4; k++) M[t][k] = readlane64(v, k);
    }
}
// The walk over one round's agreement bitmap A (bit i: offset i of the round agrees), from bit 0: jump to the next agreeing offset at most
// `span` away and over its run, until `span` offsets in a row disagree (done) or the bitmap cannot tell any more (the caller starts a fresh
// round at the returned position).  Closed form of that loop: the walk stops at the first run of >= span zeros that the 64 bits show whole,
// else at the first end of a run of ones beyond bit 64 - span.  Returns the offsets consumed; every agreeing offset below it was visited.
__device__ __forceinline__ int walk_round(uint64_t A, int span, bool &done)
{
    uint64_t R = ~A; int len = 1;
    while (2 * len <= span) { R &= R >> len; len *= 2; }
    if (len < span) R &= R >> (span - len);                // R bit i: offsets i .. i + span - 1 all disagree (zeros shifted in: never across bit 63)
    if (R) { done = true; return __ffsll((unsigned long long)R) - 1; }
    const uint64_t ends = A & ~(A >> 1) & (~0ULL << (64 - span));     // last offsets of the runs that reach beyond 64 - span (not empty when R is)
    return __ffsll((unsigned long long)ends);
}
// the window of the lane's offset: digits d .. d + span - 1 of M (0 <= d < 64), under the care mask
__device__ __forceinline__ bool ext_window_clean(const uint64_t M[4], int d, const SeedShape &sh)
{
    const bool up = d >= 32; const int r = (d & 31) * 2;
    const uint64_t a = up ? M[1] : M[0], b = up ? M[2] : M[1], c = up ? M[3] : M[2];
    const uint64_t lo = r ? ((a >> r) | (b << (64 - r))) : a, hi = r ? ((b >> r) | (c << (64 - r))) : b;
    return ((lo & sh.care_lo) | (hi & sh.care_hi)) == 0;
}
// placed / ambiguous bases and contig starts under the windows of offset k (only when the pass has such bitmaps)
__device__ __forceinline__ bool ext_blocked(const ExtComp *__restrict__ comp, int nc, int span, int64_t k)
{
    bool b = false;
    for (int c = 0; c < nc; c++) {
        const ExtComp &C = comp[c];
        const int64_t q = C.rev ? C.pos - k : C.pos + k;
        if ((C.VM || C.CM) && q >= C.lo && q <= C.hi) b |= window_blocked(C.VM, C.CM, (uint32_t)q, span);
    }
    return b;
}
