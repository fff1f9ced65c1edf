// feature_dev.hip -- annotated ranges mapped through the alignment, and the interval-overlap join behind them.  The stage
// stands in for the walk four of libMems' tools are built around (getOrthologList.cpp:137-313, randomGeneSample.cpp:118-157,
// bbBreakOnGenes.cpp:140-160, scoreProcrastAlignment.cpp:285-305): the intervals a range [lo, hi] of one genome intersects, the range clipped
// to each, SeqPosToColumn on both ends, copyRange, LeftEnd / RightEnd of every row, and the annotated feature of every genome that shares
// the most bases with that extent.  The range map reads the coordinate index in force (S14, coord_index.hpp) and no genome data; the join
// reads neither.
//   fm_count    a thread per query: two binary searches in its genome's table slice = first piece and count (the pieces of a query are
//               a contiguous slice of the table: a base lies in at most one interval), the arguments checked
//   vscan       over the counts (dev_scan.hpp) = piece_off; the total comes back once, with the flag, to size the piece arrays
//   fm_pieces   a thread per (piece, genome), the 64 / N pieces of a wave in consecutive lanes: the piece's query by a search of piece_off,
//               co_find on both clipped ends (every lane of a piece runs the same search: the loads are the same addresses), then lane g
//               ranks its own bit plane at col and at col + len = n_res and, through co_residue, the two extents.  Lane 0 adds the clipped
//               length to covered and raises the query's (clipped length, interval id) maximum, both with 64-bit integer atomics
//   fm_best     a thread per piece: the one that holds its query's maximum is best (an interval occurs once among a query's pieces)
// Nothing loops over the columns or bases of a range: a whole-genome query costs what a one-base query costs per piece.
//   fo_keys     the join's table as (genome << 31 | lo, table index) pairs, the entries checked; sorted by the project's sort (fo_keys, FoHi, fm_put and fm_flag_result
//               live in interval_join.hpp: repeat_score_dev.hip, S22, builds the same table over component extents)
//   vmax        (dev_scan.hpp) the inclusive running maximum of (genome << 31 | hi) over the sorted table: the genome in the high bits
//               makes it the prefix maximum of hi inside every genome's slice;  fo_bounds  the slices' first entries, a search per genome
//   fo_query    a thread per query: the last slice entry with lo <= the query's hi by a search, then backward while the prefix maximum
//               reaches the query's lo, every entry tested; the walk ends at the slice's first entry
// Every index a kernel forms is checked first; a thread that finds something wrong sets a bit of the flag word (CO_BAD_ARG, CO_BAD_INDEX,
// and FM_LIMIT for a position of 2^31 or more).  All results are integers placed by scanned offsets or by order-free maxima and sums:
// two calls return identical bytes.
#include "common.hpp"
#include "coord_index.hpp"
#include "dev_scan.hpp"
#include "interval_join.hpp"
#include <algorithm>
#include <cstring>

namespace {

struct FmCnt { const uint32_t *v; __device__ int64_t value(uint32_t i) const { return v[i]; } };

// the result of a range map of n queries and P pieces over N genomes (fm_res): piece_off | covered | best | piece_query | piece_iv |
// piece_col | piece_len | clip_lo | clip_hi | n_res | ext_left | ext_right (P = 0: what exists before the pieces are counted)
struct FmLayout {
    size_t covered, best, pq, piv, pcol, plen, clo, chi, nres, el, er, total;
    FmLayout(size_t n, size_t P, size_t N)
    {
        covered = up64((n + 1) * 8); best = covered + up64(n * 8); pq = best + up64(n * 8);
        piv = pq + up64(P * 8); pcol = piv + up64(P * 8); plen = pcol + up64(P * 8); clo = plen + up64(P * 8); chi = clo + up64(P * 8);
        nres = chi + up64(P * 8); el = nres + up64(P * N * 8); er = el + up64(P * N * 8); total = er + up64(P * N * 8);
    }
};
struct FmOut { int64_t *pq, *piv, *pcol, *plen, *clo, *chi, *nres, *el, *er; };

__global__ void __launch_bounds__(256) fm_count(CoordDev D, int64_t n, const int32_t *__restrict__ seq, const int64_t *__restrict__ lo, const int64_t *__restrict__ hi,
                                                uint32_t *__restrict__ first, uint32_t *__restrict__ cnt, uint32_t *__restrict__ flag)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const int64_t g = seq[q], a = lo[q], b = hi[q];
    uint32_t f = 0, c = 0, bad = 0;
    if (g < 0 || g >= D.N || a < 1 || a > b) bad = CO_BAD_ARG;
    else if (b >= FM_MAX_POS) bad = FM_LIMIT;
    else {
        const uint32_t t1 = D.tab_off[g + 1];
        uint32_t x = D.tab_off[g], y = t1;
        while (x < y) { const uint32_t mid = (x + y) >> 1; if (D.tright[mid] < a) x = mid + 1; else y = mid; }     // the first interval that ends at or behind lo
        f = x; y = t1;
        while (x < y) { const uint32_t mid = (x + y) >> 1; if (D.tleft[mid] <= b) x = mid + 1; else y = mid; }     // the first one that starts behind hi
        c = x - f;
    }
    first[q] = f; cnt[q] = c;
    if (bad) atomicOr(flag, bad);
}

__global__ void __launch_bounds__(256) fm_pieces(CoordDev D, int64_t n, int64_t P, const int32_t *__restrict__ seq, const int64_t *__restrict__ lo,
                                                 const int64_t *__restrict__ hi, const uint32_t *__restrict__ first, const int64_t *__restrict__ piece_off, FmOut O,
                                                 unsigned long long *__restrict__ covered, unsigned long long *__restrict__ best_key, uint32_t *__restrict__ flag)
{
    const int lane = threadIdx.x & 63, ppw = 64 / D.N, slot = lane / D.N, g = lane - slot * D.N;
    const int64_t p = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * ppw + slot;
    if (slot >= ppw || p >= P) return;
    int64_t qa = 0, qe = n;                                   // the last query whose pieces start at or before p (piece_off[0] = 0; empty queries repeat an offset)
    while (qe - qa > 1) { const int64_t mid = (qa + qe) >> 1; if (piece_off[mid] <= p) qa = mid; else qe = mid; }
    const int64_t q = qa, t = (int64_t)first[q] + (p - piece_off[q]);
    const int s = seq[q];
    uint32_t bad = 0;
    int64_t i = 0, cl = 0, ch = 0, xa = 0, xb = -1;
    bool ok = s >= 0 && s < D.N && t >= D.tab_off[s] && t < D.tab_off[s + 1];
    if (ok) {
        i = D.tiv[t];
        cl = max(lo[q], D.tleft[t]); ch = min(hi[q], D.tright[t]);
        int64_t i1 = -1, i2 = -1, x1 = 0, x2 = 0, c0 = 0, c1 = 0;
        ok = cl <= ch && co_find(D, s, cl, &i1, &x1, &c0, &bad) == 0 && co_find(D, s, ch, &i2, &x2, &c1, &bad) == 0 && i1 == i && i2 == i;
        if (ok) { xa = min(x1, x2); xb = max(x1, x2); if (g == 0) { O.pcol[p] = xa - c0; O.plen[p] = xb - xa + 1; } }     // (a reverse row: the two columns swap)
    }
    int64_t nr = 0, el = 0, er = 0;
    if (ok) {
        const CoordIv I = D.ivt[(size_t)i * D.N + g];
        const int64_t ba = xa / CO_BLOCK, xe = xb + 1, be = xe / CO_BLOCK;
        if (be >= D.nb1) ok = false;
        else if (I.left) {
            bool pr;
            const CoordRec ra = D.rec[(size_t)ba * D.N + g], re = D.rec[(size_t)be * D.N + g];
            const int64_t ka = co_rank(ra, (int)(xa - ba * CO_BLOCK), &pr) - I.base, ke = co_rank(re, (int)(xe - be * CO_BLOCK), &pr) - I.base;
            if (ka < 0 || ke < ka || ke > I.right - I.left + 1) ok = false;
            else if (ke > ka) {
                const int64_t pa = co_residue(I, ka), pe = co_residue(I, ke - 1);
                nr = ke - ka;
                if (I.col0_rev & 1) { el = -pe; er = -pa; } else { el = pa; er = pe; }
            }
        }
        if (g == s && (nr != ch - cl + 1 || (el < 0 ? -el : el) != cl || (er < 0 ? -er : er) != ch)) ok = false;     // the query's own row is exactly the clip
    }
    if (!ok) { bad |= CO_BAD_INDEX; nr = el = er = 0; }
    O.nres[(size_t)p * D.N + g] = nr; O.el[(size_t)p * D.N + g] = el; O.er[(size_t)p * D.N + g] = er;
    if (g == 0) {
        O.pq[p] = q; O.piv[p] = ok ? i : -1; O.clo[p] = cl; O.chi[p] = ch;
        if (!ok) { O.pcol[p] = 0; O.plen[p] = 0; }
        else {
            const unsigned long long len = (unsigned long long)(ch - cl + 1);
            atomicAdd(&covered[q], len);
            atomicMax(&best_key[q], len << 31 | (unsigned long long)i);
        }
    }
    if (bad) atomicOr(flag, bad);
}

__global__ void __launch_bounds__(256) fm_best(int64_t P, FmOut O, const unsigned long long *__restrict__ best_key, int64_t *__restrict__ best)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P || O.piv[p] < 0) return;
    const int64_t q = O.pq[p];
    if (((unsigned long long)(O.chi[p] - O.clo[p] + 1) << 31 | (unsigned long long)O.piv[p]) == best_key[q]) best[q] = p;
}

__global__ void __launch_bounds__(64) fo_bounds(int64_t m, const unsigned long long *__restrict__ keys, uint32_t *__restrict__ bound)
{
    const int g = threadIdx.x;
    if (g > MAUVE_MAX_SEQ) return;
    const unsigned long long k = (unsigned long long)g << 31;
    int64_t x = 0, y = m;
    while (x < y) { const int64_t mid = (x + y) >> 1; if (keys[mid] < k) x = mid + 1; else y = mid; }
    bound[g] = (uint32_t)x;
}

__global__ void __launch_bounds__(256) fo_query(int64_t n, const int32_t *__restrict__ qs, const int64_t *__restrict__ qlo, const int64_t *__restrict__ qhi,
                                                const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ vals, const int64_t *__restrict__ thi,
                                                const unsigned long long *__restrict__ pmax, const uint32_t *__restrict__ bound, int64_t *__restrict__ n_hit,
                                                int64_t *__restrict__ best, int64_t *__restrict__ overlap, uint32_t *__restrict__ flag)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const int64_t s = qs[q], a0 = qlo[q], b0 = qhi[q];
    int64_t hit = 0, bst = -1, ov = 0; uint32_t bad = 0;
    if (s < 0 || s >= MAUVE_MAX_SEQ) bad = CO_BAD_ARG;
    else if (a0 == 0 && b0 == 0) { }                          // "nothing": a row of extents whose genome is absent
    else if (a0 == 0 || b0 == 0 || (a0 < 0) != (b0 < 0)) bad = CO_BAD_ARG;
    else {
        const unsigned long long a = a0 < 0 ? 0ull - (unsigned long long)a0 : (unsigned long long)a0, b = b0 < 0 ? 0ull - (unsigned long long)b0 : (unsigned long long)b0;
        if (a > b) bad = CO_BAD_ARG;
        else if (b >= (unsigned long long)FM_MAX_POS) bad = FM_LIMIT;
        else {
            const uint32_t s0 = bound[s], s1 = bound[s + 1];
            const unsigned long long kq = (unsigned long long)s << 31 | b;
            uint32_t x = s0, y = s1;
            while (x < y) { const uint32_t mid = (x + y) >> 1; if (keys[mid] <= kq) x = mid + 1; else y = mid; }      // the first entry that starts behind the query
            for (uint32_t j = x; j > s0;) {                   // (never below the slice's first entry: the entry before it is another genome's)
                --j;
                if ((pmax[j] & FO_POS) < a) break;            // no entry at or before j reaches the query
                const uint32_t idx = vals[j];
                const int64_t tl = (int64_t)(keys[j] & FO_POS), th = thi[idx];
                const int64_t o = min(th, (int64_t)b) - max(tl, (int64_t)a) + 1;
                if (o > 0) { hit++; if (o > ov || (o == ov && (int64_t)idx > bst)) { ov = o; bst = idx; } }
            }
        }
    }
    n_hit[q] = hit; best[q] = bst; overlap[q] = ov;
    if (bad) atomicOr(flag, bad);
}

const char *const FM_OUTSIDE = "a query lies outside its domain (genome index, lo < 1 or lo > hi)";
const char *const FO_OUTSIDE = "a table entry or a query lies outside its domain (genome id, lo < 1, lo > hi, one end 0 or ends of different sign)";

}  // namespace

extern "C" {

int mauve_map_ranges(mauve_ctx *c, int64_t n, const int32_t *seq, const int64_t *lo, const int64_t *hi, mauve_range_map_sizes *sz)
{
    if (!c) return MAUVE_ERR_ARG;
    mauve_ctx::RangeMap &R = c->fm;
    R.valid = false;
    const mauve_ctx::CoordIndex &X = c->co;
    if (!X.valid) { c->err = "map_ranges: no index in this context (mauve_coord_index first)"; return MAUVE_ERR_STATE; }
    if (n < 0 || (n && (!seq || !lo || !hi))) { c->err = "map_ranges: missing query arrays"; return MAUVE_ERR_ARG; }
    if (n > FM_MAX_N) { c->err = "map_ranges: more than 2^24 queries"; return MAUVE_ERR_LIMIT; }
    const CoordDev &D = *X.dev;
    const size_t nq = (size_t)n, N = (size_t)X.N;
    const uint32_t tiles = (uint32_t)((nq + devscan::TILE - 1) / devscan::TILE);
    // work area: flag | seq | lo | hi | first pieces | counts | tile sums | the queries' (clipped length, interval) maxima
    const size_t w_seq = 64, w_lo = w_seq + up64(nq * 4), w_hi = w_lo + up64(nq * 8), w_first = w_hi + up64(nq * 8), w_cnt = w_first + up64(nq * 4),
                 w_bs = w_cnt + up64(nq * 4), w_key = w_bs + up64((size_t)tiles * 8), w_total = w_key + up64(nq * 8);
    const FmLayout H(nq, 0, N);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->fm_work.ensure(w_total));
    HIPCHK(c, c->fm_res.ensure(H.total + 64));
    const bool direct = n == 0 || (host_pointer_is_pinned(seq) && host_pointer_is_pinned(lo) && host_pointer_is_pinned(hi));
    HIPCHK(c, c->pin_stage.ensure(direct ? 64 : w_first));
    char *wk = c->fm_work.as<char>();
    uint32_t *flag = reinterpret_cast<uint32_t *>(wk), *first = reinterpret_cast<uint32_t *>(wk + w_first), *cnt = reinterpret_cast<uint32_t *>(wk + w_cnt);
    const int32_t *d_seq = reinterpret_cast<const int32_t *>(wk + w_seq);
    const int64_t *d_lo = reinterpret_cast<const int64_t *>(wk + w_lo), *d_hi = reinterpret_cast<const int64_t *>(wk + w_hi);
    int64_t *bs = reinterpret_cast<int64_t *>(wk + w_bs);
    unsigned long long *key = reinterpret_cast<unsigned long long *>(wk + w_key);
    HIPCHK(c, hipMemsetAsync(wk, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(c->fm_res.p, 0, 8, c->stream));  // piece_off[0] (n = 0: all of it)
    int64_t n_piece = 0;
    if (n) {
        size_t used = 64;
        if (const int r1 = fm_put(c, wk + w_seq, seq, nq * 4, direct, &used)) return r1;
        if (const int r2 = fm_put(c, wk + w_lo, lo, nq * 8, direct, &used)) return r2;
        if (const int r3 = fm_put(c, wk + w_hi, hi, nq * 8, direct, &used)) return r3;
        hipLaunchKernelGGL(fm_count, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, c->stream, D, n, d_seq, d_lo, d_hi, first, cnt, flag);
        const FmCnt in{cnt};
        int64_t *piece_off = c->fm_res.as<int64_t>();
        hipLaunchKernelGGL((devscan::vscan_partial<int64_t, FmCnt>), dim3(tiles), dim3(256), 0, c->stream, in, (uint32_t)nq, bs);
        hipLaunchKernelGGL((devscan::vscan_write<int64_t, FmCnt>), dim3(tiles), dim3(256), 0, c->stream, in, (uint32_t)nq, bs, piece_off, (int64_t *)nullptr);
        HIPCHK(c, hipGetLastError());
        // the one round trip: the flag and the number of pieces (behind the queries' upload on the same stream, so the staging is free again)
        char *hb = c->pin_stage.as<char>();
        HIPCHK(c, hipMemcpyAsync(hb, flag, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(hb + 8, piece_off + nq, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (const int rf = fm_flag_result(c, *reinterpret_cast<const uint32_t *>(hb), "map_ranges", FM_OUTSIDE)) return rf;
        n_piece = *reinterpret_cast<const int64_t *>(hb + 8);
        if (n_piece >= FM_MAX_POS) { c->err = "map_ranges: 2^31 pieces or more"; return MAUVE_ERR_LIMIT; }
    }
    if (n_piece) {
        const size_t P = (size_t)n_piece;
        const FmLayout L(nq, P, N);
        HIPCHK(c, c->fm_res.ensure_keep(L.total + 64, (nq + 1) * 8, c->stream));
        char *rs = c->fm_res.as<char>();
        const FmOut O{reinterpret_cast<int64_t *>(rs + L.pq), reinterpret_cast<int64_t *>(rs + L.piv), reinterpret_cast<int64_t *>(rs + L.pcol), reinterpret_cast<int64_t *>(rs + L.plen),
                      reinterpret_cast<int64_t *>(rs + L.clo), reinterpret_cast<int64_t *>(rs + L.chi), reinterpret_cast<int64_t *>(rs + L.nres), reinterpret_cast<int64_t *>(rs + L.el),
                      reinterpret_cast<int64_t *>(rs + L.er)};
        HIPCHK(c, hipMemsetAsync(rs + L.covered, 0, nq * 8, c->stream));
        HIPCHK(c, hipMemsetAsync(rs + L.best, 0xff, nq * 8, c->stream));
        HIPCHK(c, hipMemsetAsync(key, 0, nq * 8, c->stream));
        const size_t waves = (P + (64 / N) - 1) / (64 / N);
        hipLaunchKernelGGL(fm_pieces, dim3((uint32_t)((waves + 3) / 4)), dim3(256), 0, c->stream, D, n, n_piece, d_seq, d_lo, d_hi, first, reinterpret_cast<const int64_t *>(rs), O,
                           reinterpret_cast<unsigned long long *>(rs + L.covered), key, flag);
        hipLaunchKernelGGL(fm_best, dim3((uint32_t)((P + 255) / 256)), dim3(256), 0, c->stream, n_piece, O, key, reinterpret_cast<int64_t *>(rs + L.best));
        HIPCHK(c, hipGetLastError());
        if (const int rf = co_flag_read(c, flag, "map_ranges", FM_OUTSIDE)) return rf;
    } else if (n) {
        char *rs = c->fm_res.as<char>();
        HIPCHK(c, hipMemsetAsync(rs + H.covered, 0, nq * 8, c->stream));
        HIPCHK(c, hipMemsetAsync(rs + H.best, 0xff, nq * 8, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    R.N = X.N; R.n_query = n; R.n_piece = n_piece; R.valid = true;
    if (sz) { sz->n_query = n; sz->n_piece = n_piece; }
    return MAUVE_OK;
}

int mauve_map_ranges_fetch(mauve_ctx *c, int64_t *piece_off, int64_t *covered, int64_t *best, int64_t *piece_query, int64_t *piece_iv, int64_t *piece_col,
                           int64_t *piece_len, int64_t *clip_lo, int64_t *clip_hi, int64_t *n_res, int64_t *ext_left, int64_t *ext_right)
{
    if (!c) return MAUVE_ERR_ARG;
    const mauve_ctx::RangeMap &R = c->fm;
    if (!R.valid) { c->err = "map_ranges_fetch: no range map in this context (mauve_map_ranges first)"; return MAUVE_ERR_STATE; }
    const size_t n = (size_t)R.n_query, P = (size_t)R.n_piece, N = (size_t)R.N;
    const FmLayout L(n, P, N);
    const char *rs = c->fm_res.as<char>();
    const struct { void *dst; size_t off, bytes; } outs[12] = {
        {piece_off, 0, (n + 1) * 8}, {covered, L.covered, n * 8}, {best, L.best, n * 8}, {piece_query, L.pq, P * 8}, {piece_iv, L.piv, P * 8}, {piece_col, L.pcol, P * 8},
        {piece_len, L.plen, P * 8}, {clip_lo, L.clo, P * 8}, {clip_hi, L.chi, P * 8}, {n_res, L.nres, P * N * 8}, {ext_left, L.el, P * N * 8}, {ext_right, L.er, P * N * 8}};
    HIPCHK(c, hipSetDevice(c->device));
    for (const auto &o : outs)
        if (o.dst) if (const int rc = copy_to_caller(c, c->pin_stage, o.dst, rs + o.off, o.bytes)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MAUVE_OK;
}

int mauve_range_overlaps(mauve_ctx *c, int64_t m, const int32_t *tab_seq, const int64_t *tab_lo, const int64_t *tab_hi, int64_t n, const int32_t *q_seq,
                         const int64_t *q_lo, const int64_t *q_hi, int64_t *n_hit, int64_t *best, int64_t *overlap)
{
    if (!c) return MAUVE_ERR_ARG;
    if (m < 0 || n < 0 || (m && (!tab_seq || !tab_lo || !tab_hi)) || (n && (!q_seq || !q_lo || !q_hi))) { c->err = "range_overlaps: missing table or query arrays"; return MAUVE_ERR_ARG; }
    if (m > FM_MAX_N || n > FM_MAX_N) { c->err = "range_overlaps: more than 2^24 table entries or queries"; return MAUVE_ERR_LIMIT; }
    if (!m && !n) return MAUVE_OK;
    const size_t M = (size_t)m, nq = (size_t)n;
    const uint32_t tiles = (uint32_t)((M + devscan::TILE - 1) / devscan::TILE);
    // work area: flag | slice bounds | table seq, lo, hi | keys x 2 | values x 2 | prefix maxima | tile maxima | query seq, lo, hi | n_hit | best | overlap
    const size_t w_bound = 64, w_ts = w_bound + up64((MAUVE_MAX_SEQ + 1) * 4), w_tl = w_ts + up64(M * 4), w_th = w_tl + up64(M * 8), w_k1 = w_th + up64(M * 8), w_k2 = w_k1 + up64(M * 8),
                 w_v1 = w_k2 + up64(M * 8), w_v2 = w_v1 + up64(M * 4), w_pm = w_v2 + up64(M * 4), w_bm = w_pm + up64(M * 8), w_qs = w_bm + up64((size_t)tiles * 8),
                 w_ql = w_qs + up64(nq * 4), w_qh = w_ql + up64(nq * 8), w_oh = w_qh + up64(nq * 8), w_ob = w_oh + up64(nq * 8), w_oo = w_ob + up64(nq * 8), w_total = w_oo + up64(nq * 8);
    const bool direct = (!m || (host_pointer_is_pinned(tab_seq) && host_pointer_is_pinned(tab_lo) && host_pointer_is_pinned(tab_hi))) &&
                        (!n || (host_pointer_is_pinned(q_seq) && host_pointer_is_pinned(q_lo) && host_pointer_is_pinned(q_hi)));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->fo_work.ensure(w_total));
    HIPCHK(c, c->pin_stage.ensure(direct ? 64 : 64 + up64(M * 4) + 2 * up64(M * 8) + up64(nq * 4) + 2 * up64(nq * 8)));
    char *wk = c->fo_work.as<char>();
    uint32_t *flag = reinterpret_cast<uint32_t *>(wk), *bound = reinterpret_cast<uint32_t *>(wk + w_bound);
    HIPCHK(c, hipMemsetAsync(wk, 0, w_ts, c->stream));        // the flag, and the bounds of a table without entries
    size_t used = 64;
    if (const int r1 = fm_put(c, wk + w_ts, tab_seq, M * 4, direct, &used)) return r1;
    if (const int r2 = fm_put(c, wk + w_tl, tab_lo, M * 8, direct, &used)) return r2;
    if (const int r3 = fm_put(c, wk + w_th, tab_hi, M * 8, direct, &used)) return r3;
    if (const int r4 = fm_put(c, wk + w_qs, q_seq, nq * 4, direct, &used)) return r4;
    if (const int r5 = fm_put(c, wk + w_ql, q_lo, nq * 8, direct, &used)) return r5;
    if (const int r6 = fm_put(c, wk + w_qh, q_hi, nq * 8, direct, &used)) return r6;
    const int64_t *d_th = reinterpret_cast<const int64_t *>(wk + w_th);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(wk + w_k1), *pmax = reinterpret_cast<unsigned long long *>(wk + w_pm);
    uint32_t *vals = reinterpret_cast<uint32_t *>(wk + w_v1);
    if (m) {
        hipLaunchKernelGGL(fo_keys, dim3((uint32_t)((M + 255) / 256)), dim3(256), 0, c->stream, m, reinterpret_cast<const int32_t *>(wk + w_ts), reinterpret_cast<const int64_t *>(wk + w_tl), d_th,
                           keys, vals, flag);
        HIPCHK(c, hipGetLastError());
        uint64_t *k = reinterpret_cast<uint64_t *>(keys);
        if (const int rs = sort_pairs_u64(c, (uint32_t)M, FO_KEY_BITS, &k, &vals, reinterpret_cast<uint64_t *>(wk + w_k2), reinterpret_cast<uint32_t *>(wk + w_v2), MAUVE_K_MISC)) return rs;
        keys = reinterpret_cast<unsigned long long *>(k);
        const FoHi in{keys, vals, d_th};
        unsigned long long *bm = reinterpret_cast<unsigned long long *>(wk + w_bm);
        hipLaunchKernelGGL((devscan::vmax_partial<unsigned long long, FoHi>), dim3(tiles), dim3(256), 0, c->stream, in, (uint32_t)M, bm);
        hipLaunchKernelGGL((devscan::vmax_write<unsigned long long, FoHi>), dim3(tiles), dim3(256), 0, c->stream, in, (uint32_t)M, bm, pmax);
        hipLaunchKernelGGL(fo_bounds, dim3(1), dim3(64), 0, c->stream, m, keys, bound);
    }
    if (n) {
        hipLaunchKernelGGL(fo_query, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, c->stream, n, reinterpret_cast<const int32_t *>(wk + w_qs), reinterpret_cast<const int64_t *>(wk + w_ql),
                           reinterpret_cast<const int64_t *>(wk + w_qh), keys, vals, d_th, pmax, bound, reinterpret_cast<int64_t *>(wk + w_oh), reinterpret_cast<int64_t *>(wk + w_ob),
                           reinterpret_cast<int64_t *>(wk + w_oo), flag);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, c->pin_stage.ensure(64));
    HIPCHK(c, hipMemcpyAsync(c->pin_stage.p, flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));               // (the staging held the inputs until here)
    if (const int rf = fm_flag_result(c, *c->pin_stage.as<uint32_t>(), "range_overlaps", FO_OUTSIDE)) return rf;
    if (n_hit) if (const int r7 = copy_to_caller(c, c->pin_stage, n_hit, wk + w_oh, nq * 8)) return r7;
    if (best) if (const int r8 = copy_to_caller(c, c->pin_stage, best, wk + w_ob, nq * 8)) return r8;
    if (overlap) if (const int r9 = copy_to_caller(c, c->pin_stage, overlap, wk + w_oo, nq * 8)) return r9;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MAUVE_OK;
}

}  // extern "C"
