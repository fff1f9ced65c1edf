// extract_dev.hip -- alignment columns as a base matrix: choose columns, choose rows, write the letters.  The stage stands in
// for the GetAlignment loops of stripGapColumns.cpp:32-64, projectAndStrip.cpp:75-101, stripSubsetLCBs.cpp:125-142, createBackboneMFA.cpp:28-37
// and alignmentProjector.cpp:58-77, which walk every column of an interval on the host to print the letters of a few.
// It reads the coordinate index in force (S14, coord_index.hpp) and the resident genomes; a cell is the letter mauve_write_xmfa prints.
//   ex_ranges   a thread per range: the range against its interval (the error flag), its first column in the whole array, its length;
//               a thread per (interval, genome): the interval ends against the resident genome's length
//   ex_flags    the candidates are the columns of the ranges one after another (scan of the lengths, dev_scan.hpp); a thread per candidate
//               evaluates the selection rule, a wave's 64 answers leave as one word (ballot)
//   ex_compact  the scanned word counts give every selected column its slot: (interval, column) lists, and range_off from the same scan
//   ex_fill     a thread per 4 consecutive selected columns of one row: rank from the block record, the base from the packed genome,
//               one dword store; rows have a pitch of their own (a multiple of 16 bytes), the copy-out is 2-D
// Every index formed from caller data is checked before it is used; the kernels report through the flag word of coord_index.hpp.  The
// selection (ex_sel, device memory) is what the stage keeps between a select and its fetches; the staging holds nothing between calls.
#include "common.hpp"
#include "extract_cells.hpp"
#include <algorithm>
#include <cstring>

namespace {

// the request as the kernels see it
struct ExReq { int n_keep; int32_t keep[MAUVE_MAX_SEQ]; uint32_t require, keepmask; int drop_empty, polymorphic; };

struct ExLen { const int64_t *v; static ExLen of(const int64_t *, const int64_t *cl) { return ExLen{cl}; } __device__ int64_t value(uint32_t i) const { return v[i]; } };
struct ExPop { const uint64_t *w; __device__ int64_t value(uint32_t i) const { return __popcll(w[i]); } };

__global__ void __launch_bounds__(256) ex_flags(CoordDev D, ExGenomes G, ExReq Q, int64_t R, int64_t n_cand, const int64_t *__restrict__ r_iv, const int64_t *__restrict__ gstart,
                                                const int64_t *__restrict__ cand_off, uint64_t *__restrict__ words, int64_t n_words,
                                                uint32_t *__restrict__ flag)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool sel = false; uint32_t bad = 0;
    if (t < n_cand) {
        const int64_t r = ex_range_of(cand_off, R, t), i = r_iv ? r_iv[r] : r, x = gstart[r] + (t - cand_off[r]);
        // conditions 1 and 2 need the column's genome set alone: one bit of every genome's record
        const int64_t b = x / CO_BLOCK; const int off = (int)(x - b * CO_BLOCK);
        uint32_t m = 0;
        if (Q.require || Q.drop_empty || Q.polymorphic)
            for (int g = 0; g < D.N; g++) if ((Q.require | Q.keepmask) >> g & 1) m |= (uint32_t)(D.rec[(size_t)b * D.N + g].w[off >> 6] >> (off & 63) & 1) << g;
        sel = (m & Q.require) == Q.require && (!Q.drop_empty || (m & Q.keepmask));
        if (sel && Q.polymorphic) {
            uint32_t seen = 0;
            for (int k = 0; k < Q.n_keep; k++) {
                const int g = Q.keep[k];
                if (!(m >> g & 1)) continue;
                int code;
                (void)ex_cell(D, G, i, x, g, &code, &bad);
                if (code >= 0) seen |= 1u << code;
            }
            sel = (seen & (seen - 1)) != 0;
        }
    }
    const uint64_t B = __ballot(sel);
    if ((threadIdx.x & 63) == 0 && (t >> 6) < n_words) words[t >> 6] = B;
    if (bad) atomicOr(flag, bad);
}

__global__ void __launch_bounds__(256) ex_compact(CoordDev D, int64_t R, int64_t n_cand, const int64_t *__restrict__ r_iv, const int64_t *__restrict__ gstart,
                                                  const int64_t *__restrict__ cand_off, const uint64_t *__restrict__ words, const int64_t *__restrict__ pre, int64_t n_words,
                                                  int64_t *__restrict__ sel_iv, int64_t *__restrict__ sel_col, int64_t *__restrict__ range_off)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n_cand) {
        const uint64_t w = words[t >> 6];
        if (w >> (t & 63) & 1) {
            const int64_t r = ex_range_of(cand_off, R, t), i = r_iv ? r_iv[r] : r, x = gstart[r] + (t - cand_off[r]);
            const int64_t slot = pre[t >> 6] + __popcll(w & co_below((int)(t & 63)));
            sel_iv[slot] = i; sel_col[slot] = x - D.col_off[i];
        }
    }
    if (t <= R) {
        const int64_t t0 = cand_off[t], w = t0 >> 6;
        range_off[t] = pre[w] + (w < n_words ? __popcll(words[w] & co_below((int)(t0 & 63))) : 0);
    }
}

// row blockIdx.y of the matrix; thread = 4 consecutive selected columns, a wave = 256 consecutive bytes of the row
__global__ void __launch_bounds__(256) ex_fill(CoordDev D, ExGenomes G, ExReq Q, int64_t n_sel, const int64_t *__restrict__ sel_iv, const int64_t *__restrict__ sel_col,
                                               uint32_t *__restrict__ mat, int64_t pitch4, uint32_t *__restrict__ flag)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= pitch4) return;
    const int g = Q.keep[blockIdx.y];
    uint32_t out = 0, bad = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int64_t j = t * 4 + k;
        if (j >= n_sel) break;
        const int64_t i = sel_iv[j], c = sel_col[j];
        char ch = '-';
        if (i < 0 || i >= D.n_iv) bad |= CO_BAD_INDEX;
        else {
            const int64_t o0 = D.col_off[i];
            int code;
            if (c < 0 || c >= D.col_off[i + 1] - o0) bad |= CO_BAD_INDEX; else ch = ex_cell(D, G, i, o0 + c, g, &code, &bad);
        }
        out |= (uint32_t)(uint8_t)ch << (8 * k);
    }
    mat[(size_t)blockIdx.y * (size_t)pitch4 + (size_t)t] = out;
    if (bad) atomicOr(flag, bad);
}

ExReq ex_request(const mauve_ctx::ExtractSel &S, uint32_t require, int drop_empty, int polymorphic)
{
    ExReq Q; memset(&Q, 0, sizeof Q);
    Q.n_keep = S.n_keep;
    for (int k = 0; k < S.n_keep; k++) { Q.keep[k] = S.keep[k]; Q.keepmask |= 1u << S.keep[k]; }
    Q.require = require; Q.drop_empty = drop_empty; Q.polymorphic = polymorphic;
    return Q;
}

}  // namespace

extern "C" {

int mauve_extract_select(mauve_ctx *c, const mauve_extract_params *p, int64_t n_range, const int64_t *range_iv, const int64_t *range_col, const int64_t *range_len, int64_t *n_sel)
{
    if (!c) return MAUVE_ERR_ARG;
    mauve_ctx::ExtractSel &S = c->ex;
    S.valid = false;
    if (const int rs = ex_check_state(c, "extract_select")) return rs;
    const int N = c->nseq;
    if (!p || p->n_keep < 1 || p->n_keep > N) { c->err = "extract_select: n_keep outside [1, nseq]"; return MAUVE_ERR_ARG; }
    uint32_t keepmask = 0;
    for (int k = 0; k < p->n_keep; k++) {
        const int g = p->keep[k];
        if (g < 0 || g >= N || (keepmask >> g & 1)) { c->err = "extract_select: keep[" + std::to_string(k) + "] is outside [0, nseq) or repeated"; return MAUVE_ERR_ARG; }
        keepmask |= 1u << g;
    }
    if (N < 32 && (p->require >> N)) { c->err = "extract_select: a require bit at or above nseq"; return MAUVE_ERR_ARG; }
    S.n_keep = p->n_keep; S.n_sel = 0;
    for (int k = 0; k < p->n_keep; k++) S.keep[k] = p->keep[k];
    ExFront F;                                               // the candidates are the columns of the ranges one after another: the scan of the lengths
    if (const int rf = ex_front<ExLen>(c, "extract_select", c->ex_work, n_range, range_iv, range_col, range_len, nullptr, 0, &F)) return rf;
    const int64_t R = S.n_range = F.R, n_cand = F.total, *d_iv = F.d_iv, *gstart = F.gstart, *cand_off = F.off;
    if (n_cand >= ((int64_t)1 << 34)) { c->err = "extract_select: the ranges hold 2^34 columns or more"; return MAUVE_ERR_LIMIT; }
    const CoordDev &D = *c->co.dev;
    const ExReq Q = ex_request(S, p->require, p->drop_empty != 0, p->polymorphic != 0);
    const size_t nR = (size_t)R;
    char *hb = c->pin_stage.as<char>();
    HIPCHK(c, c->ex_sel.ensure(up64((nR + 1) * 8)));
    int64_t *range_off = c->ex_sel.as<int64_t>();
    int64_t ns = 0;
    if (n_cand == 0) HIPCHK(c, hipMemsetAsync(range_off, 0, (nR + 1) * 8, c->stream));
    else {
        // flag words | their scan | its tile sums;  then the lists: range_off | sel_iv | sel_col
        const int64_t n_words = (n_cand + 63) / 64;
        const uint32_t tilesW = (uint32_t)((n_words + devscan::TILE - 1) / devscan::TILE);
        const size_t b_pre = up64((size_t)n_words * 8), b_bs = b_pre + up64(((size_t)n_words + 1) * 8), b_total = b_bs + up64((size_t)tilesW * 8);
        HIPCHK(c, c->ex_bits.ensure(b_total));
        char *bb = c->ex_bits.as<char>();
        uint64_t *words = reinterpret_cast<uint64_t *>(bb);
        int64_t *pre = reinterpret_cast<int64_t *>(bb + b_pre), *bsw = reinterpret_cast<int64_t *>(bb + b_bs);
        const uint32_t blocks = (uint32_t)((n_cand + 255) / 256);
        hipLaunchKernelGGL(ex_flags, dim3(blocks), dim3(256), 0, c->stream, D, F.G, Q, R, n_cand, d_iv, gstart, cand_off, words, n_words, F.flag);
        const ExPop in{words};
        hipLaunchKernelGGL((devscan::vscan_partial<int64_t, ExPop>), dim3(tilesW), dim3(256), 0, c->stream, in, (uint32_t)n_words, bsw);
        hipLaunchKernelGGL((devscan::vscan_write<int64_t, ExPop>), dim3(tilesW), dim3(256), 0, c->stream, in, (uint32_t)n_words, bsw, pre, (int64_t *)nullptr);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(hb + 64, pre + n_words, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        ns = *reinterpret_cast<const int64_t *>(hb + 64);
        const size_t s_iv = up64((nR + 1) * 8), s_col = s_iv + up64((size_t)ns * 8), s_total = s_col + up64((size_t)ns * 8);
        HIPCHK(c, c->ex_sel.ensure(s_total));
        char *sb = c->ex_sel.as<char>();
        range_off = reinterpret_cast<int64_t *>(sb);
        hipLaunchKernelGGL(ex_compact, dim3((uint32_t)((std::max<int64_t>(n_cand, R + 1) + 255) / 256)), dim3(256), 0, c->stream, D, R, n_cand, d_iv, gstart, cand_off, words, pre, n_words,
                           reinterpret_cast<int64_t *>(sb + s_iv), reinterpret_cast<int64_t *>(sb + s_col), range_off);
        HIPCHK(c, hipGetLastError());
        if (const int rf = co_flag_read(c, F.flag, "extract_select", EX_OUTSIDE)) return rf;
    }
    S.n_sel = ns; S.genome_gen = c->genome_gen; S.valid = true;
    if (n_sel) *n_sel = ns;
    return MAUVE_OK;
}

int mauve_extract_fetch(mauve_ctx *c, char *rows, int64_t row_stride, int64_t *sel_iv, int64_t *sel_col, int64_t *range_off)
{
    if (!c) return MAUVE_ERR_ARG;
    const mauve_ctx::ExtractSel &S = c->ex;
    if (!S.valid || S.genome_gen != c->genome_gen) { c->err = "extract_fetch: no selection in force (mauve_extract_select first; an index call or a genome upload ends it)"; return MAUVE_ERR_STATE; }
    if (const int rs = ex_check_state(c, "extract_fetch")) return rs;
    if (rows && row_stride < S.n_sel) { c->err = "extract_fetch: row_stride is smaller than the number of selected columns"; return MAUVE_ERR_ARG; }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nR = (size_t)S.n_range, ns = (size_t)S.n_sel;
    const size_t s_iv = up64((nR + 1) * 8), s_col = s_iv + up64(ns * 8);
    const char *sb = c->ex_sel.as<char>();
    if (rows && ns) {
        const CoordDev &D = *c->co.dev;
        const ExGenomes G = ex_genomes(c);
        const ExReq Q = ex_request(S, 0, 0, 0);
        const size_t pitch = (ns + 15) & ~(size_t)15;
        HIPCHK(c, c->ex_mat.ensure(pitch * (size_t)S.n_keep + 64));
        HIPCHK(c, c->ex_work.ensure(64));
        uint32_t *flag = c->ex_work.as<uint32_t>();
        HIPCHK(c, hipMemsetAsync(flag, 0, 64, c->stream));
        char *mat = c->ex_mat.as<char>();
        hipLaunchKernelGGL(ex_fill, dim3((uint32_t)((pitch / 4 + 255) / 256), (uint32_t)S.n_keep), dim3(256), 0, c->stream, D, G, Q, (int64_t)ns,
                           reinterpret_cast<const int64_t *>(sb + s_iv), reinterpret_cast<const int64_t *>(sb + s_col), reinterpret_cast<uint32_t *>(mat), (int64_t)(pitch / 4), flag);
        HIPCHK(c, hipGetLastError());
        if (host_pointer_is_pinned(rows))
            HIPCHK(c, hipMemcpy2DAsync(rows, (size_t)row_stride, mat, pitch, ns, (size_t)S.n_keep, hipMemcpyDeviceToHost, c->stream));
        else {
            // pieces of whole columns, 16-byte aligned in the device rows, through the staging
            const size_t wmax = std::max<size_t>(16, (((size_t)64 << 20) / (size_t)S.n_keep) & ~(size_t)15);
            HIPCHK(c, c->pin_stage.ensure(std::min(wmax, pitch) * (size_t)S.n_keep + 256));
            char *hb = c->pin_stage.as<char>() + 256;
            for (size_t c0 = 0; c0 < ns; c0 += wmax) {
                const size_t w = std::min(wmax, ns - c0);
                HIPCHK(c, hipMemcpy2DAsync(hb, w, mat + c0, pitch, w, (size_t)S.n_keep, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                for (int k = 0; k < S.n_keep; k++) memcpy(rows + (size_t)k * (size_t)row_stride + c0, hb + (size_t)k * w, w);
            }
        }
        if (const int rf = co_flag_read(c, flag, "extract_fetch", EX_OUTSIDE)) return rf;
    }
    if (sel_iv) if (const int rc = copy_to_caller(c, c->pin_stage, sel_iv, sb + s_iv, ns * 8)) return rc;
    if (sel_col) if (const int rc = copy_to_caller(c, c->pin_stage, sel_col, sb + s_col, ns * 8)) return rc;
    if (range_off) if (const int rc = copy_to_caller(c, c->pin_stage, range_off, sb, (nR + 1) * 8)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MAUVE_OK;
}

}  // extern "C"
