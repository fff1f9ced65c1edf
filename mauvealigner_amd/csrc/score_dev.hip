// score_dev.hip -- an alignment scored against a correct one: the counts of the reference's accuracy harness
// (scoreAlignment.cpp:99-457) for every ordered genome pair, from two coordinate indices (S14) -- the correct alignment T in the context's
// second slot (mauve_score_truth) and the calculated alignment C, the index in force.  No genome data is read.
//   sc_count   a wave per 64-column word of T, a lane per column.  The lane finds its interval of T (binary search of T's col_off) and keeps
//              T's position of every genome at its column in LDS (co_column per genome on T's block record).  Then for every genome i with
//              a residue there: co_find on C for that base, and for every j != i C's presence and rank of j at the found column against T's
//              position of j -> one of six classes; a ballot and a popcount per class go into an LDS table [N][N][6] of 32-bit counters.
//              The table leaves with one 64-bit integer atomic per non-zero counter at the workgroup's end.
// A workgroup takes a span of consecutive words, bounded so that a 32-bit counter cannot overflow.  All counts are integers and no result
// depends on the tiling.  Every index formed into T or C is checked first: a violation sets CO_BAD_INDEX and never becomes a load.
#include "common.hpp"
#include "coord_index.hpp"
#include <algorithm>
#include <cstring>

namespace {

constexpr int SC_W = MAUVE_SCORE_WORDS;
constexpr int SC_CLASSES = 6;
constexpr int SC_MAX_GROUPS = 4096;               // workgroups of sc_count at the most
constexpr int64_t SC_MAX_POS = (int64_t)1 << 31;  // positions of T are kept in 32 bits

// LDS: the table [N * N * 6] of counters, then T's positions [4 waves][N][64 lanes] (0: no residue of that genome in the lane's column)
__global__ void __launch_bounds__(256) sc_count(CoordDev T, CoordDev Cx, int64_t n_cols, int64_t n_words, int64_t wpg, unsigned long long *__restrict__ out,
                                                uint32_t *__restrict__ flag)
{
    extern __shared__ uint32_t s_mem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, N = T.N;
    const int n_cnt = N * N * SC_CLASSES;
    uint32_t *s_tab = s_mem, *s_pos = s_mem + n_cnt + wave * N * 64;
    for (int t = threadIdx.x; t < n_cnt; t += 256) s_tab[t] = 0;
    __syncthreads();
    uint32_t bad = 0;
    const int64_t w0 = (int64_t)blockIdx.x * wpg, w1 = min(w0 + wpg, n_words);
    for (int64_t w = w0 + wave; w < w1; w += 4) {
        const int64_t x = w * 64 + lane;
        const bool valid = x < n_cols && T.n_iv > 0;
        // the lane's interval of T: the last one that starts at or before x (empty intervals in front share that start)
        int64_t a = 0, e = T.n_iv;
        if (valid) while (e - a > 1) { const int64_t mid = (a + e) >> 1; if (T.col_off[mid] <= x) a = mid; else e = mid; }
        const int64_t b = x / CO_BLOCK;
        const bool ok = valid && b < T.nb1;
        if (valid && !ok) bad |= CO_BAD_INDEX;
        for (int g = 0; g < N; g++) {
            uint32_t p = 0;
            if (ok) {
                CoordIv I; bool present; int64_t k;
                if (co_column(T, a, x, g, &I, &present, &k) && present) {
                    const int64_t q = co_residue(I, k);
                    if (k < 0 || q < I.left || q > I.right || q >= SC_MAX_POS) bad |= CO_BAD_INDEX; else p = (uint32_t)q;
                }
            }
            s_pos[g * 64 + lane] = p;                          // (a lane reads back only what it wrote itself)
        }
        for (int i = 0; i < N; i++) {
            const uint32_t pi = s_pos[i * 64 + lane];
            if (!__ballot(pi != 0)) continue;
            int64_t civ = -1, xc = 0, c0 = 0;
            bool found = false;
            if (pi) {
                uint32_t fb = 0;
                found = co_find(Cx, i, (int64_t)pi, &civ, &xc, &c0, &fb) == 0;
                if (fb) bad |= CO_BAD_INDEX;                   // (i and pi are in range: whatever co_find objects to lies in the index)
                if (found && (civ < 0 || civ >= Cx.n_iv || xc < 0 || xc / CO_BLOCK >= Cx.nb1)) { bad |= CO_BAD_INDEX; found = false; }
            }
            const int64_t cb = xc / CO_BLOCK;
            const int coff = (int)(xc - cb * CO_BLOCK);
            for (int j = 0; j < N; j++) {
                if (j == i) continue;
                int cls = -1;
                if (pi) {
                    const int64_t tj = s_pos[j * 64 + lane];
                    int64_t pj = 0;
                    bool inside = false;
                    if (found) {
                        CoordIv J; bool present; int64_t k;
                        inside = co_column(Cx, civ, cb, coff, j, &J, &present, &k);
                        if (present) {
                            pj = co_residue(J, k);
                            if (k < 0 || pj < J.left || pj > J.right) { bad |= CO_BAD_INDEX; pj = 0; }
                        }
                    }
                    cls = tj ? (pj ? (pj == tj ? 0 : 1) : (inside ? 2 : 3)) : (pj ? 4 : 5);
                }
                uint32_t mine = 0;                             // (the popcount of a ballot is one scalar instruction: it stays ahead of the lane's choice)
#pragma unroll
                for (int l = 0; l < SC_CLASSES; l++) { const uint64_t m = __ballot(cls == l); if (lane == l) mine = (uint32_t)__popcll(m); }
                if (lane < SC_CLASSES && mine) atomicAdd(&s_tab[(i * N + j) * SC_CLASSES + lane], mine);
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < n_cnt; t += 256) {
        const uint32_t v = s_tab[t];
        if (v) atomicAdd(&out[(size_t)(t / SC_CLASSES) * SC_W + t % SC_CLASSES], (unsigned long long)v);
    }
    if (bad) atomicOr(flag, bad);
}

}  // namespace

extern "C" {

int mauve_score_truth(mauve_ctx *c, int nseq, int64_t n_iv, const int64_t *left, const int64_t *right, const int8_t *reverse, const int64_t *col_off, const uint32_t *cols)
{
    if (!c) return MAUVE_ERR_ARG;
    c->co_truth.valid = false;
    if (nseq >= 1 && nseq <= MAUVE_MAX_SEQ && n_iv > 0 && right)
        for (int64_t k = 0; k < n_iv * nseq; k++)
            if (right[k] >= SC_MAX_POS) { c->err = "score_truth: a position of 2^31 or more"; return MAUVE_ERR_LIMIT; }
    return coord_index_arrays(c, "score_truth", c->co_truth, c->co_truth_index, nseq, n_iv, left, right, reverse, col_off, cols);
}

int mauve_score_alignment(mauve_ctx *c, int64_t *records)
{
    if (!c) return MAUVE_ERR_ARG;
    const mauve_ctx::CoordIndex &XT = c->co_truth, &XC = c->co;
    if (!XT.valid) { c->err = "score_alignment: no correct alignment in this context (mauve_score_truth first)"; return MAUVE_ERR_STATE; }
    if (!XC.valid) { c->err = "score_alignment: no index in this context (mauve_coord_index first)"; return MAUVE_ERR_STATE; }
    if (XT.N != XC.N) {
        c->err = "score_alignment: the correct alignment has " + std::to_string(XT.N) + " genomes, the index in force " + std::to_string(XC.N);
        return MAUVE_ERR_STATE;
    }
    if (!records) { c->err = "score_alignment: records is NULL"; return MAUVE_ERR_ARG; }
    const int N = XT.N;
    const size_t bytes = (size_t)N * N * SC_W * 8;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->sc_out.ensure(64 + bytes));
    char *d = c->sc_out.as<char>();
    HIPCHK(c, hipMemsetAsync(d, 0, 64 + bytes, c->stream));
    const int64_t n_cols = XT.n_cols, n_words = (n_cols + 63) / 64;
    if (n_words) {
        // a counter gains at most one per column: a workgroup's span stays below 2^32 columns
        const int64_t wpg = std::max<int64_t>(4, (n_words + SC_MAX_GROUPS - 1) / SC_MAX_GROUPS), groups = (n_words + wpg - 1) / wpg;
        if (wpg >= ((int64_t)1 << 26)) { c->err = "score_alignment: the correct alignment is too long"; return MAUVE_ERR_LIMIT; }
        const size_t lds = ((size_t)N * N * SC_CLASSES + (size_t)4 * N * 64) * 4;
        hipLaunchKernelGGL(sc_count, dim3((uint32_t)groups), dim3(256), lds, c->stream, *XT.dev, *XC.dev, n_cols, n_words, wpg, reinterpret_cast<unsigned long long *>(d + 64),
                           reinterpret_cast<uint32_t *>(d));
        HIPCHK(c, hipGetLastError());
    }
    // page-locked records are queued in front of the flag's one synchronise; pageable ones are written only once the flag is judged
    const bool direct = host_pointer_is_pinned(records);
    if (direct) if (const int rc = copy_to_caller(c, c->pin_stage, records, d + 64, bytes)) return rc;
    if (const int rf = co_flag_read(c, reinterpret_cast<const uint32_t *>(d), "score_alignment", nullptr, "an index")) return rf;
    return direct ? MAUVE_OK : copy_to_caller(c, c->pin_stage, records, d + 64, bytes);
}

}  // extern "C"
