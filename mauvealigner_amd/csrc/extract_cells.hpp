// extract_cells.hpp -- what the stages that read letters through the coordinate index share: extract_dev.hip and
// pairstat_dev.hip (S16).  The cell rule, the resident genomes as a kernel argument, the range check with its flag words, the state check
// and the copy-out.  Internal linkage: every stage compiles its own copy.
#pragma once
#include "common.hpp"
#include "coord_index.hpp"
#include <algorithm>
#include <cstring>
#include <string>

namespace {

// the resident genomes: 2-bit codes and the ambiguity bitmap (inv == nullptr: none)
struct ExGenomes { const uint64_t *words, *inv; uint64_t word_off[MAUVE_MAX_SEQ], mask_off[MAUVE_MAX_SEQ]; int64_t len[MAUVE_MAX_SEQ]; };
struct ExLen { const int64_t *v; __device__ int64_t value(uint32_t i) const { return v[i]; } };

inline size_t up64(size_t x) { return (x + 63) & ~(size_t)63; }

// flag words: [0] a range outside the alignment or an interval end beyond its genome (MAUVE_ERR_ARG), [1] an index that contradicts itself
__device__ __forceinline__ void ex_report(uint32_t *flag, uint32_t bad) { if (bad & CO_BAD_ARG) flag[0] = 1u; if (bad & CO_BAD_INDEX) flag[1] = 1u; }

__global__ void __launch_bounds__(256) ex_ranges(CoordDev D, ExGenomes G, int64_t R, const int64_t *__restrict__ r_iv, const int64_t *__restrict__ r_col,
                                                 const int64_t *__restrict__ r_len, int64_t *__restrict__ gstart, int64_t *__restrict__ clen, uint32_t *__restrict__ flag)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t bad = 0;
    if (t < R) {
        const int64_t i = r_iv ? r_iv[t] : t;
        int64_t x = 0, n = 0;
        if (i < 0 || i >= D.n_iv) bad = CO_BAD_ARG;
        else {
            const int64_t o0 = D.col_off[i], o1 = D.col_off[i + 1], c = r_iv ? r_col[t] : 0, l = r_iv ? r_len[t] : o1 - o0;
            if (c < 0 || l < 0 || c > o1 - o0 || l > o1 - o0 - c) bad = CO_BAD_ARG; else { x = o0 + c; n = l; }
        }
        gstart[t] = x; clen[t] = n;
    }
    if (t < D.n_iv * D.N) {
        const CoordIv I = D.ivt[t];
        if (I.left && I.right > G.len[t % D.N]) bad |= CO_BAD_ARG;
    }
    if (bad) ex_report(flag, bad);
}

// the letter of column x (whole array) of interval i in genome g (S15 cell rule); *code: 0..3 for a letter of ACGT, else -1
__device__ __forceinline__ char ex_cell(const CoordDev &D, const ExGenomes &G, int64_t i, int64_t x, int g, int *code, uint32_t *bad)
{
    *code = -1;
    const CoordIv I = D.ivt[(size_t)i * D.N + g];
    if (!I.left) return '-';
    const int64_t b = x / CO_BLOCK;
    const CoordRec r = D.rec[(size_t)b * D.N + g];
    bool present;
    const int64_t k = co_rank(r, (int)(x - b * CO_BLOCK), &present) - I.base;
    if (!present) return '-';
    const bool rev = I.col0_rev & 1;
    const int64_t p = rev ? I.right - k : I.left + k;
    if (k < 0 || p < 1 || p > G.len[g]) { *bad |= CO_BAD_INDEX; return '-'; }
    const int64_t q = p - 1;
    if (G.inv && (G.inv[G.mask_off[g] + (uint64_t)(q >> 6)] >> (q & 63) & 1)) return 'N';
    const int v = (int)(G.words[G.word_off[g] + (uint64_t)(q >> 5)] >> (2 * (q & 31)) & 3);
    const int o = rev ? 3 - v : v;
    *code = o;
    return (char)(0x54474341u >> (8 * o));                   // "ACGT"
}

// candidate t -> its range (the last one that starts at or before t: empty ranges in front share that start)
__device__ __forceinline__ int64_t ex_range_of(const int64_t *__restrict__ cand_off, int64_t R, int64_t t)
{
    int64_t a = 0, e = R;
    while (e - a > 1) { const int64_t mid = (a + e) >> 1; if (cand_off[mid] <= t) a = mid; else e = mid; }
    return a;
}

// the resident genomes as a kernel argument
ExGenomes ex_genomes(const mauve_ctx *c)
{
    ExGenomes G; memset(&G, 0, sizeof G);
    G.words = c->genomes.as<uint64_t>();
    G.inv = c->has_invalid ? c->base_invalid.as<uint64_t>() : nullptr;
    for (int g = 0; g < c->nseq; g++) {
        G.word_off[g] = c->word_off[(size_t)g]; G.len[g] = c->lens[(size_t)g];
        G.mask_off[g] = c->has_invalid ? c->base_mask_off[(size_t)g] : 0;
    }
    return G;
}

int ex_flag_result(mauve_ctx *c, const uint32_t *f, const char *who)
{
    if (f[0]) { c->err = std::string(who) + ": a range lies outside the alignment (interval id, column, length) or an interval of the index ends beyond its resident genome"; return MAUVE_ERR_ARG; }
    if (f[1]) { c->err = std::string(who) + ": the index is inconsistent with its interval table"; return MAUVE_ERR_STATE; }
    return MAUVE_OK;
}

// the index and the genomes a selection or a fetch works on
int ex_check_state(mauve_ctx *c, const char *who)
{
    const mauve_ctx::CoordIndex &X = c->co;
    if (!X.valid) { c->err = std::string(who) + ": no index in this context (mauve_coord_index first)"; return MAUVE_ERR_STATE; }
    if (X.N != c->nseq) { c->err = std::string(who) + ": the index was built for " + std::to_string(X.N) + " genomes, the context holds " + std::to_string(c->nseq); return MAUVE_ERR_STATE; }
    if (X.genome_gen != c->genome_gen) { c->err = std::string(who) + ": the genomes were replaced after the index was built"; return MAUVE_ERR_STATE; }
    return MAUVE_OK;
}

// device -> caller: page-locked destinations directly, pageable ones through ctx->pin_ex in pieces
int ex_copy_out(mauve_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (!bytes) return MAUVE_OK;
    if (host_pointer_is_pinned(dst)) { HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream)); return MAUVE_OK; }
    const size_t piece = (size_t)64 << 20;
    HIPCHK(c, c->pin_ex.ensure(std::min(bytes, piece)));
    for (size_t o = 0; o < bytes; o += piece) {
        const size_t n = std::min(piece, bytes - o);
        HIPCHK(c, hipMemcpyAsync(c->pin_ex.p, static_cast<const char *>(src) + o, n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        memcpy(static_cast<char *>(dst) + o, c->pin_ex.p, n);
    }
    return MAUVE_OK;
}

}  // namespace
