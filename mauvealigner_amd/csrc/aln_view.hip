// aln_view.hip -- the one front end of the stages that take an alignment in (backbone S12, homology pass S12b, coordinate index S14):
// the two makers of an AlnView (described in common.hpp) and the checks they run -- for a caller's arrays check_columns, whose kernel
// bb_iv_residues counts every genome's residues per interval.
#include "common.hpp"
#include "column_counts.hpp"

namespace {

// residues of every genome in every interval of a caller's column array (check_columns): a tile inside one interval adds its ballot
// counts once, a tile that spans interval borders adds per column
__global__ void __launch_bounds__(256) bb_iv_residues(const uint32_t *__restrict__ cols, int64_t n, int N, const int64_t *__restrict__ off, int64_t n_iv,
                                                      unsigned long long *__restrict__ cnt, uint32_t *__restrict__ bad)
{
    auto iv_of = [&](int64_t c) {                              // the last interval whose first column is <= c (empty intervals are skipped over)
        int64_t lo = 0, hi = n_iv;                             // off[lo] <= c < off[hi]
        while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (off[mid] <= c) lo = mid; else hi = mid; }
        return lo;
    };
    const int lane = threadIdx.x & 63;
    const int64_t t0 = (int64_t)blockIdx.x * BB_CHUNK, t1 = min(n, t0 + (int64_t)BB_CHUNK);
    if (t0 >= t1) return;
    const int64_t iv0 = iv_of(t0), iv1 = iv_of(t1 - 1);
    const uint32_t above = N >= 32 ? 0u : ~0u << N;
    uint32_t mine = 0; bool wrong = false;
    for (int k = 0; k < BB_CHUNK / 256; k++) {
        const int64_t c = t0 + k * 256 + threadIdx.x;
        const uint32_t v = c < t1 ? cols[c] : 0u;
        wrong |= (v & above) != 0;
        if (iv0 == iv1) mine = wave_genome_counts(v, N, lane, mine);
        else if (v) {
            const int64_t iv = iv_of(c);
            for (uint32_t m = v & ~above; m; m &= m - 1) atomicAdd(&cnt[(size_t)iv * N + (__ffs(m) - 1)], 1ull);
        }
    }
    if (iv0 == iv1 && lane < N && mine) atomicAdd(&cnt[(size_t)iv0 * N + lane], (unsigned long long)mine);
    if (wrong) atomicOr(bad, 1u);
}

}  // namespace

int coord_check_offsets(mauve_ctx *c, const char *who, int64_t n_iv, const int64_t *col_off)
{
    bool ok = col_off[0] == 0;
    for (int64_t i = 0; i < n_iv && ok; i++) ok = col_off[i + 1] >= col_off[i];
    if (!ok) c->err = std::string(who) + ": col_off must ascend from 0";
    return ok ? MAUVE_OK : MAUVE_ERR_ARG;
}

// Every genome's residue count in an interval's columns must be what its ends say -- right - left + 1, none for an absent genome -- and no
// column may carry a bit at or above nseq.  The homology pass turns these counts into base addresses (hom_column), so an inconsistent
// array would read outside the genomes.  bb_work is scratch of the check
int check_columns(mauve_ctx *c, const char *who, const AlnView &A)
{
    const int N = A.N; const int64_t n_iv = A.n_iv, n_cols = A.col_off[n_iv];
    // work area: column offsets | counts | flag
    const size_t o_cnt = up64(((size_t)n_iv + 1) * 8), o_bad = o_cnt + up64((size_t)n_iv * N * 8), total = o_bad + 64;
    HIPCHK(c, c->bb_work.ensure(total));
    char *wk = c->bb_work.as<char>();
    HIPCHK(c, hipMemcpyAsync(wk, A.col_off, ((size_t)n_iv + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(wk + o_cnt, 0, total - o_cnt, c->stream));
    if (n_cols) {
        hipLaunchKernelGGL(bb_iv_residues, dim3((uint32_t)((n_cols + BB_CHUNK - 1) / BB_CHUNK)), dim3(256), 0, c->stream, A.d_cols, n_cols, N, reinterpret_cast<const int64_t *>(wk), n_iv,
                           reinterpret_cast<unsigned long long *>(wk + o_cnt), reinterpret_cast<uint32_t *>(wk + o_bad));
        HIPCHK(c, hipGetLastError());
    }
    std::vector<unsigned long long> cnt((size_t)n_iv * N); uint32_t bad = 0;
    HIPCHK(c, hipMemcpyAsync(cnt.data(), wk + o_cnt, cnt.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&bad, wk + o_bad, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bad) { c->err = std::string(who) + ": a column carries a genome bit at or above nseq"; return MAUVE_ERR_ARG; }
    for (int64_t iv = 0; iv < n_iv; iv++) for (int g = 0; g < N; g++) {
        const int64_t l = A.left[(size_t)(iv * N + g)], r = A.right[(size_t)(iv * N + g)];
        const int64_t want = l ? r - l + 1 : 0;
        if (l < 0 || want < 0 || (int64_t)cnt[(size_t)(iv * N + g)] != want) {
            c->err = std::string(who) + ": the columns of interval " + std::to_string(iv) + " hold " + std::to_string(cnt[(size_t)(iv * N + g)]) + " residues of genome " + std::to_string(g) +
                     ", its ends say " + std::to_string(want);
            return MAUVE_ERR_ARG;
        }
    }
    return MAUVE_OK;
}

// n_cols columns on the host to `buf` on the context's stream (not waited for)
static int upload_columns(mauve_ctx *c, DevBuf &buf, const uint32_t *cols, int64_t n_cols)
{
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, buf.ensure(((size_t)n_cols + 64) * 4));
    if (n_cols) HIPCHK(c, hipMemcpyAsync(buf.p, cols, (size_t)n_cols * 4, hipMemcpyHostToDevice, c->stream));
    return MAUVE_OK;
}

int aln_from_context(mauve_ctx *c, const char *who, bool refuse_replaced, DevBuf &upload_to, AlnView *out)
{
    const AlignResult &R = c->res;
    if (R.stale || (refuse_replaced && R.genomes_replaced)) { c->err = std::string(who) + ": the genomes were replaced after this alignment was made"; return MAUVE_ERR_STATE; }
    const int64_t n_iv = R.sz.n_iv;
    if ((int64_t)R.col_off.size() != n_iv + 1) { c->err = std::string(who) + ": no alignment in this context"; return MAUVE_ERR_STATE; }
    *out = AlnView{n_iv ? (int)(R.iv_left.size() / (size_t)n_iv) : c->nseq, n_iv, R.iv_left.data(), R.iv_right.data(), R.iv_reverse.data(), R.col_off.data(), nullptr};
    if (n_iv == 0) return MAUVE_OK;                                          // nothing was aligned
    if (R.cols_pending) { HIPCHK(c, hipSetDevice(c->device)); out->d_cols = c->res_cols.as<uint32_t>(); }     // still where the assembly stage wrote them
    else {
        if (const int rc = upload_columns(c, upload_to, R.cols_data(), out->col_off[n_iv])) return rc;
        out->d_cols = upload_to.as<uint32_t>();
    }
    return MAUVE_OK;
}

int aln_from_arrays(mauve_ctx *c, const char *who, int nseq, int64_t n_iv, const int64_t *left, const int64_t *right, const int8_t *reverse, const int64_t *col_off,
                    const uint32_t *cols, AlnView *out)
{
    if (nseq < 1 || nseq > MAUVE_MAX_SEQ || n_iv < 0 || !col_off || (n_iv && (!left || !right || !reverse)) || (n_iv && col_off[n_iv] > 0 && !cols)) {
        c->err = std::string(who) + ": bad arguments"; return MAUVE_ERR_ARG;
    }
    if (const int rco = coord_check_offsets(c, who, n_iv, col_off)) return rco;
    if (const int rc = upload_columns(c, c->bb_cols, cols, col_off[n_iv])) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));                            // cols is the caller's (pageable) memory
    *out = AlnView{nseq, n_iv, left, right, reverse, col_off, c->bb_cols.as<uint32_t>()};
    return n_iv ? check_columns(c, who, *out) : MAUVE_OK;
}
