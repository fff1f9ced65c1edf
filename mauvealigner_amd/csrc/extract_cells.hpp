// extract_cells.hpp -- what the stages that read letters through the coordinate index share: extract_dev.hip,
// pairstat_dev.hip (S16) and excursion_dev.hip (S18).  The cell rule, the run rule of two rows (ps_run_mask, ps_look_back), the resident genomes as a kernel argument, the state check, and the range front end (ex_front): the
// caller's ranges checked against the index on the device and a count per range scanned, up to the stage's first own kernel.  Errors go
// through the flag word of coord_index.hpp.  Internal linkage: every stage compiles its own copy.
#pragma once
#include "common.hpp"
#include "coord_index.hpp"
#include "dev_scan.hpp"
#include <algorithm>
#include <cstring>
#include <string>

namespace {

// the resident genomes: 2-bit codes and the ambiguity bitmap (inv == nullptr: none)
struct ExGenomes { const uint64_t *words, *inv; uint64_t word_off[MAUVE_MAX_SEQ], mask_off[MAUVE_MAX_SEQ]; int64_t len[MAUVE_MAX_SEQ]; };

// CO_BAD_ARG in these stages
constexpr const char *EX_OUTSIDE = "a range lies outside the alignment (interval id, column, length) or an interval of the index ends beyond its resident genome";

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
    if (bad) atomicOr(flag, bad);
}

// the letter of column x (whole array) of interval i in genome g (S15 cell rule); *code: 0..3 for a letter of ACGT, else -1
__device__ __forceinline__ char ex_cell(const CoordDev &D, const ExGenomes &G, int64_t i, int64_t x, int g, int *code, uint32_t *bad)
{
    *code = -1;
    CoordIv I; bool present; int64_t k;
    if (!co_column(D, i, x, g, &I, &present, &k) || !present) return '-';
    const bool rev = I.col0_rev & 1;
    const int64_t p = co_residue(I, k);
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

// ---- the run rule of S16, shared with the excursions of S18 (excursion_dev.hip) ----
// the columns of X that open a run, for X = the columns where one genome alone has a residue and Y = the columns where either has one.
// "The previous occupied column was an X column" is a carry chain -- X generates, an unoccupied column propagates, any other kills -- so one add
// gives the state in front of all 64 columns; cin: the state in front of the word, replaced by the state behind it.
__device__ __forceinline__ uint64_t ps_run_mask(uint64_t X, uint64_t Y, uint32_t &cin)
{
    const uint64_t a = X | ~Y, s = a + X, t = s + cin;
    const uint64_t into = t ^ a ^ X;
    cin = (uint32_t)((s < a) | (t < s));
    return X & ~into;
}
__device__ __forceinline__ uint32_t ps_runs(uint64_t X, uint64_t Y, uint32_t &cin) { return (uint32_t)__popcll(ps_run_mask(X, Y, cin)); }

// the presence word w (whole array) of genome g, which interval i holds (has) or not
__device__ __forceinline__ uint64_t ps_word(const CoordDev &D, bool has, int g, int64_t w)
{
    if (!has) return 0;
    const int64_t b = w / CO_WORDS;
    return D.rec[(size_t)b * D.N + g].w[w - b * CO_WORDS];
}

// the run state in front of word aw for the pair (a, b) in a range of interval i that starts at column gs: from the nearest earlier occupied
// column of the range, none open when there is none
__device__ __forceinline__ void ps_look_back(const CoordDev &D, int64_t i, int a, int b, int64_t gs, int64_t aw, uint32_t &ca, uint32_t &cb)
{
    const bool ha = D.ivt[(size_t)i * D.N + a].left != 0, hb = D.ivt[(size_t)i * D.N + b].left != 0;
    const int64_t w0 = gs >> 6;
    ca = cb = 0;
    for (int64_t w = aw - 1; w >= w0; w--) {
        uint64_t qa = ps_word(D, ha, a, w), qb = ps_word(D, hb, b, w);
        if (w == w0) { const uint64_t m = ~co_below((int)(gs & 63)); qa &= m; qb &= m; }
        const uint64_t y = qa | qb;
        if (y) { const int h = 63 - __clzll((long long)y); ca = (uint32_t)((qa & ~qb) >> h & 1); cb = (uint32_t)((qb & ~qa) >> h & 1); return; }
    }
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

// the index and the genomes a selection or a fetch works on
int ex_check_state(mauve_ctx *c, const char *who)
{
    const mauve_ctx::CoordIndex &X = c->co;
    if (!X.valid) { c->err = std::string(who) + ": no index in this context (mauve_coord_index first)"; return MAUVE_ERR_STATE; }
    if (X.N != c->nseq) { c->err = std::string(who) + ": the index was built for " + std::to_string(X.N) + " genomes, the context holds " + std::to_string(c->nseq); return MAUVE_ERR_STATE; }
    if (X.genome_gen != c->genome_gen) { c->err = std::string(who) + ": the genomes were replaced after the index was built"; return MAUVE_ERR_STATE; }
    return MAUVE_OK;
}

// what the range front end hands to its stage
struct ExFront {
    int64_t R;                                    // ranges (the caller's, or every interval whole)
    ExGenomes G;
    const int64_t *d_iv;                          // the ranges' intervals (nullptr: range r is interval r)
    int64_t *gstart, *clen, *off;                 // first column (whole array) and length of every range; the scan of the stage's count [R + 1]
    int64_t total;                                // off[R]
    char *tail;                                   // the stage's bytes behind the ranges
    uint32_t *flag;                               // the error flag, first word of the work area
};

// The front end of a stage that works on column ranges: the range arguments checked, the ranges and `tail_bytes` of the stage's own (`tail`)
// packed and uploaded into `work`, ex_ranges, the scan of F::of(gstart, clen) over the ranges, the flag and the total read back and the flag
// judged.  One synchronise.  It leaves ctx->pin_stage at least 256 bytes long.
template <class F>
int ex_front(mauve_ctx *c, const char *who, DevBuf &work, int64_t n_range, const int64_t *range_iv, const int64_t *range_col, const int64_t *range_len,
             const void *tail, size_t tail_bytes, ExFront *out)
{
    const int64_t R = range_iv ? n_range : c->co.n_iv;
    if (R < 0 || (range_iv && R && (!range_col || !range_len))) { c->err = std::string(who) + ": missing range arrays"; return MAUVE_ERR_ARG; }
    if (R >= ((int64_t)1 << 31)) { c->err = std::string(who) + ": too many ranges"; return MAUVE_ERR_LIMIT; }
    const CoordDev &D = *c->co.dev;
    out->R = R; out->G = ex_genomes(c);
    HIPCHK(c, hipSetDevice(c->device));
    // work area: flag | the caller's ranges | the tail | first column and length of every range | the scan | its tile sums
    const size_t nR = (size_t)R, n_ivg = (size_t)(D.n_iv * D.N);
    const uint32_t tilesR = (uint32_t)((nR + devscan::TILE - 1) / devscan::TILE);
    const size_t w_iv = 64, w_col = w_iv + up64(nR * 8), w_len = w_col + up64(nR * 8), w_tail = w_len + up64(nR * 8), w_gs = w_tail + up64(tail_bytes),
                 w_cl = w_gs + up64(nR * 8), w_off = w_cl + up64(nR * 8), w_bs = w_off + up64((nR + 1) * 8), w_total = w_bs + up64((size_t)tilesR * 8 + 8);
    HIPCHK(c, work.ensure(w_total));
    HIPCHK(c, c->pin_stage.ensure(std::max<size_t>(w_gs, 256)));
    char *wk = work.as<char>(), *hb = c->pin_stage.as<char>();
    HIPCHK(c, hipMemsetAsync(wk, 0, 64, c->stream));
    const bool own = range_iv && R;
    if (own) { memcpy(hb + w_iv, range_iv, nR * 8); memcpy(hb + w_col, range_col, nR * 8); memcpy(hb + w_len, range_len, nR * 8); }
    if (tail_bytes) memcpy(hb + w_tail, tail, tail_bytes);
    const size_t up0 = own ? w_iv : w_tail;
    if (w_gs > up0) HIPCHK(c, hipMemcpyAsync(wk + up0, hb + up0, w_gs - up0, hipMemcpyHostToDevice, c->stream));
    out->flag = reinterpret_cast<uint32_t *>(wk);
    out->d_iv = range_iv ? reinterpret_cast<const int64_t *>(wk + w_iv) : nullptr;
    out->tail = wk + w_tail;
    out->gstart = reinterpret_cast<int64_t *>(wk + w_gs); out->clen = reinterpret_cast<int64_t *>(wk + w_cl); out->off = reinterpret_cast<int64_t *>(wk + w_off);
    int64_t *bsum = reinterpret_cast<int64_t *>(wk + w_bs);
    const size_t n_chk = std::max(nR, n_ivg);
    if (n_chk)
        hipLaunchKernelGGL(ex_ranges, dim3((uint32_t)((n_chk + 255) / 256)), dim3(256), 0, c->stream, D, out->G, R, out->d_iv, reinterpret_cast<const int64_t *>(wk + w_col),
                           reinterpret_cast<const int64_t *>(wk + w_len), out->gstart, out->clen, out->flag);
    if (R) {
        const F in = F::of(out->gstart, out->clen);
        hipLaunchKernelGGL((devscan::vscan_partial<int64_t, F>), dim3(tilesR), dim3(256), 0, c->stream, in, (uint32_t)R, bsum);
        hipLaunchKernelGGL((devscan::vscan_write<int64_t, F>), dim3(tilesR), dim3(256), 0, c->stream, in, (uint32_t)R, bsum, out->off, (int64_t *)nullptr);
    } else HIPCHK(c, hipMemsetAsync(out->off, 0, 8, c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hb, wk, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hb + 64, out->off + R, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->total = *reinterpret_cast<const int64_t *>(hb + 64);
    return co_flag_result(c, *reinterpret_cast<const uint32_t *>(hb), who, EX_OUTSIDE);
}

}  // namespace
