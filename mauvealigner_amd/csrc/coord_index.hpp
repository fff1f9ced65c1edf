// coord_index.hpp -- the coordinate index as its kernels see it: shared by coord_dev.hip, which builds and queries it,
// extract_dev.hip and pairstat_dev.hip, which read ranks from it, score_dev.hip, which looks bases up in it (S17), and
// feature_dev.hip, which maps ranges through it (S21), and repeat_score_dev.hip, which reads the positions of the truth's rows from it (S22).
// The one column -> position rule (co_column, co_residue), the one position -> column rule (co_find), and the one error flag of the four
// stages: a word with the bits CO_BAD_ARG and CO_BAD_INDEX, set with atomicOr by a thread that found something, read by co_flag_result.
#pragma once
#include "common.hpp"
#include <string>

constexpr int CO_WORDS = 7;                       // 64-column words per block record (with the rank: 64 bytes)
constexpr int CO_BLOCK = CO_WORDS * 64;           // columns per block
constexpr int CO_SAMPLE = 512;                    // residues between two samples; more than a block holds, so a block carries at most one
constexpr uint32_t CO_BAD_ARG = 1u, CO_BAD_INDEX = 2u;      // the error flag: a query out of range; columns that disagree with the interval ends

struct alignas(64) CoordRec { int64_t rank; uint64_t w[CO_WORDS]; };
struct alignas(32) CoordIv { int64_t left, right, base, col0_rev; };      // base: rank at the interval's first column; col0_rev: that column << 1 | reverse

// the index as the kernels see it (by value); the context keeps the host copy (mauve_ctx::CoordIndex::dev, coord_index_release)
struct CoordDev {
    const CoordRec *rec;                          // [(nb1) * N], block-major
    const CoordIv *ivt;                           // [n_iv * N]
    const int64_t *col_off;                       // [n_iv + 1]
    const int64_t *tleft, *tright, *tiv;          // genome tables, genome after genome (tab_off)
    const uint32_t *samp;                         // samples, genome after genome (samp_off)
    int64_t n_iv, nb1;                            // nb1: blocks, the one that holds column n_cols included
    int N;
    uint32_t tab_off[MAUVE_MAX_SEQ + 1], samp_off[MAUVE_MAX_SEQ + 1];
};

__device__ __forceinline__ uint64_t co_below(int p) { return p >= 64 ? ~0ull : (1ull << p) - 1; }

// residues in front of column `off` of the record's block (whole array); *present: the bit of that column
__device__ __forceinline__ int64_t co_rank(const CoordRec &r, int off, bool *present)
{
    const int wi = off >> 6, bit = off & 63;
    int64_t n = r.rank; bool p = false;
#pragma unroll
    for (int k = 0; k < CO_WORDS; k++) {
        const uint64_t m = k < wi ? ~0ull : (k == wi ? co_below(bit) : 0ull);
        n += __popcll(r.w[k] & m);
        if (k == wi) p = r.w[k] >> bit & 1;
    }
    *present = p;
    return n;
}

// rule 1, first half: column x (whole array) of interval i in genome g.  false: the genome has no row in the interval (I.left == 0); else
// *present: the genome's bit of that column, *k: residues of the row in front of the column (rank - base).  The caller has checked i and x.
// The first form takes the column as block b and offset in it, for a caller that asks about many genomes at one column.
__device__ __forceinline__ bool co_column(const CoordDev &D, int64_t i, int64_t b, int off, int g, CoordIv *I, bool *present, int64_t *k)
{
    *I = D.ivt[(size_t)i * D.N + g];
    *present = false; *k = 0;
    if (!I->left) return false;
    const CoordRec r = D.rec[(size_t)b * D.N + g];
    *k = co_rank(r, off, present) - I->base;
    return true;
}
__device__ __forceinline__ bool co_column(const CoordDev &D, int64_t i, int64_t x, int g, CoordIv *I, bool *present, int64_t *k)
{
    const int64_t b = x / CO_BLOCK;
    return co_column(D, i, b, (int)(x - b * CO_BLOCK), g, I, present, k);
}

// rule 1, second half: the position of residue k of an interval row (unsigned; the caller checks k and the result as its stage requires)
__device__ __forceinline__ int64_t co_residue(const CoordIv &I, int64_t k) { return (I.col0_rev & 1) ? I.right - k : I.left + k; }

// position of the k-th (0-based) set bit of x; x holds more than k
__device__ __forceinline__ int co_select64(uint64_t x, int k)
{
    int pos = 0;
#pragma unroll
    for (int s = 32; s; s >>= 1) {
        const int c = __popcll((x >> pos) & ((1ull << s) - 1));
        if (k >= c) { k -= c; pos += s; }
    }
    return pos;
}

// rule 2: the interval and the (whole-array) column of base p of genome g, and the interval's first column.  0 found, 1 no interval covers p, else an error flag
__device__ __forceinline__ uint32_t co_find(const CoordDev &D, int64_t g, int64_t p, int64_t *iv, int64_t *x, int64_t *col0, uint32_t *bad)
{
    if (g < 0 || g >= D.N || p < 1) { *bad = CO_BAD_ARG; return 2; }
    uint32_t a = D.tab_off[g], e = D.tab_off[g + 1];
    if (a == e || D.tleft[a] > p) return 1;
    while (e - a > 1) { const uint32_t mid = (a + e) >> 1; if (D.tleft[mid] <= p) a = mid; else e = mid; }
    if (p > D.tright[a]) return 1;
    const int64_t i = D.tiv[a];
    const CoordIv I = D.ivt[(size_t)i * D.N + g];
    const int64_t T = I.base + ((I.col0_rev & 1) ? I.right - p : p - I.left);          // rank of the residue in the whole array
    const int64_t j = T / CO_SAMPLE, cap = (int64_t)D.samp_off[g + 1] - D.samp_off[g];
    if (j + 1 >= cap) { *bad = CO_BAD_INDEX; return 2; }
    int64_t lo = D.samp[D.samp_off[g] + j], hi = D.samp[D.samp_off[g] + j + 1];
    if (hi >= D.nb1) hi = D.nb1 - 1;
    while (hi > lo) { const int64_t mid = (lo + hi + 1) >> 1; if (D.rec[(size_t)mid * D.N + g].rank <= T) lo = mid; else hi = mid - 1; }
    const CoordRec r = D.rec[(size_t)lo * D.N + g];
    int64_t rem = T - r.rank;
    uint64_t ww = 0; int wk = -1;
#pragma unroll
    for (int k = 0; k < CO_WORDS; k++) {
        const int c = __popcll(r.w[k]);
        if (wk < 0) { if (rem >= 0 && rem < c) { wk = k; ww = r.w[k]; } else rem -= c; }
    }
    if (wk < 0) { *bad = CO_BAD_INDEX; return 2; }
    *iv = i; *x = lo * CO_BLOCK + wk * 64 + co_select64(ww, (int)rem); *col0 = I.col0_rev >> 1;
    return 0;
}

// the flag word a stage read back -> the result of its call.  outside: the stage's sentence for CO_BAD_ARG (nullptr: the stage takes nothing
// from the caller that a kernel checks, any bit speaks of an index); which: whose index CO_BAD_INDEX speaks of
inline int co_flag_result(mauve_ctx *c, uint32_t f, const char *who, const char *outside, const char *which = "the index")
{
    if (outside && (f & CO_BAD_ARG)) { c->err = std::string(who) + ": " + outside; return MAUVE_ERR_ARG; }
    if (f & (outside ? CO_BAD_INDEX : ~0u)) { c->err = std::string(who) + ": " + which + " is inconsistent with its interval table"; return MAUVE_ERR_STATE; }
    return MAUVE_OK;
}

// the flag word fetched from the device through the staging (one synchronise) and judged
inline int co_flag_read(mauve_ctx *c, const uint32_t *d_flag, const char *who, const char *outside, const char *which = "the index")
{
    HIPCHK(c, c->pin_stage.ensure(64));
    HIPCHK(c, hipMemcpyAsync(c->pin_stage.p, d_flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return co_flag_result(c, *c->pin_stage.as<uint32_t>(), who, outside, which);
}
