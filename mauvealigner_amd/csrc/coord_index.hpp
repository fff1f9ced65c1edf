// coord_index.hpp -- the coordinate index as its kernels see it: shared by coord_dev.hip, which builds and queries it, and
// extract_dev.hip, which reads ranks from it.
#pragma once
#include "common.hpp"

constexpr int CO_WORDS = 7;                       // 64-column words per block record (with the rank: 64 bytes)
constexpr int CO_BLOCK = CO_WORDS * 64;           // columns per block
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
