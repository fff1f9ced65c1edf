// coord_dev.hip -- coordinate translation through the alignment: a rank/select index over the column array and three
// batched queries on it.  The stage stands in for Interval::GetColumn (coordinateTranslate.cpp:36-46) and for
// CompactGappedAlignment::SeqPosToColumn (getOrthologList.cpp:219-220, bbBreakOnGenes.cpp:154-155, randomGeneSample.cpp:139-140,
// scoreProcrastAlignment.cpp:293-303), which both walk the columns of an interval once per question.
// The index is a snapshot with buffers of its own (ctx->co_index); nothing below reads the genomes or res_cols once it is built:
//   block records  the column array cut into blocks of 448 columns; per (block, genome) one 64-byte record: the genome's residue count
//                  in front of the block (whole array) and the 7 x 64 presence bits of the block.  The records of one block lie genome
//                  after genome, so what one query reads for all genomes is one run of nseq x 64 bytes.  Rank = one record.
//   interval rows  per (interval, genome): ends, the rank at the interval's first column, that column and the strand, 32 bytes
//   genome tables  per genome its intervals sorted by left end (position -> interval: a binary search)
//   samples        per genome the block that holds every 512th residue (rank -> block: two samples bracket the block, a block holds
//                  fewer residues than lie between two samples, so the bracket is nearly always one or two blocks wide)
//   coord_build    one wave per block: seven coalesced 256-byte loads, a ballot per genome and word, lane g keeps genome g's words
//   coord_finish   ranks from the scanned block counts (dev_scan.hpp), the samples;  coord_iv_rows  the interval rows
//   coord_positions / coord_select   the queries: a thread per (query, genome) resp. per query; every index they form is checked first.
//                  Column -> position is co_column / co_residue, position -> column co_find (coord_index.hpp, shared with S15 to S17);
//                  a thread that finds something wrong sets a bit of the flag word, which co_flag_read turns into the call's result
#include "common.hpp"
#include "coord_index.hpp"
#include "dev_scan.hpp"
#include <algorithm>
#include <cstring>

void coord_index_release(mauve_ctx *c)
{
    for (mauve_ctx::CoordIndex *X : {&c->co, &c->co_truth}) { delete X->dev; X->dev = nullptr; X->valid = false; }
}

namespace {

struct CoordTotals { int64_t v[MAUVE_MAX_SEQ]; };  // residues of every genome by the interval ends

__global__ void __launch_bounds__(256) coord_build(const uint32_t *__restrict__ cols, int64_t n_cols, int N, int64_t nb1, CoordRec *__restrict__ rec, uint32_t *__restrict__ cnt)
{
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= nb1) return;
    const int64_t x0 = b * CO_BLOCK;
    uint32_t v[CO_WORDS];
#pragma unroll
    for (int k = 0; k < CO_WORDS; k++) { const int64_t c = x0 + 64 * k + lane; v[k] = c < n_cols ? cols[c] : 0u; }
    uint64_t w[CO_WORDS];
#pragma unroll
    for (int k = 0; k < CO_WORDS; k++) w[k] = 0;
    for (int g = 0; g < N; g++) {
#pragma unroll
        for (int k = 0; k < CO_WORDS; k++) { const uint64_t B = __ballot(v[k] >> g & 1u); if (lane == g) w[k] = B; }
    }
    if (lane < N) {
        CoordRec *r = &rec[(size_t)b * N + lane];
        uint32_t n = 0;
#pragma unroll
        for (int k = 0; k < CO_WORDS; k++) { r->w[k] = w[k]; n += (uint32_t)__popcll(w[k]); }
        cnt[(size_t)b * N + lane] = n;
    }
}

// the block counts genome after genome: one scan over this order gives every genome's ranks up to a constant
struct CoCnt {
    const uint32_t *cnt; uint32_t nb1; int N;
    __device__ int64_t value(uint32_t i) const { const uint32_t g = i / nb1, b = i - g * nb1; return cnt[(size_t)b * N + g]; }
};

__global__ void __launch_bounds__(256) coord_finish(const int64_t *__restrict__ pre, CoordDev D, CoordTotals want, CoordRec *__restrict__ rec, uint32_t *__restrict__ samp,
                                                    uint32_t *__restrict__ flag)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= D.nb1 * D.N) return;
    const int64_t b = t / D.N; const int g = (int)(t - b * D.N);
    const int64_t p0 = pre[(size_t)g * D.nb1], rank = pre[(size_t)g * D.nb1 + b] - p0, next = pre[(size_t)g * D.nb1 + b + 1] - p0;
    rec[t].rank = rank;
    const int64_t cap = (int64_t)D.samp_off[g + 1] - D.samp_off[g], m = (rank + CO_SAMPLE - 1) / CO_SAMPLE;
    bool bad = false;
    if (m * CO_SAMPLE < next) { if (m < cap) samp[D.samp_off[g] + m] = (uint32_t)b; else bad = true; }
    if (b == D.nb1 - 1) {                                     // behind the last residue: the last block closes the bracket of the last sample
        const int64_t M = (next + CO_SAMPLE - 1) / CO_SAMPLE;
        if (next == want.v[g] && M < cap) samp[D.samp_off[g] + M] = (uint32_t)b; else bad = true;
    }
    if (bad) atomicOr(flag, CO_BAD_INDEX);
}

__global__ void __launch_bounds__(256) coord_iv_rows(CoordDev D, const int64_t *__restrict__ left, const int64_t *__restrict__ right, const int8_t *__restrict__ rev,
                                                     CoordIv *__restrict__ ivt)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= D.n_iv * D.N) return;
    const int64_t i = t / D.N; const int g = (int)(t - i * D.N);
    const int64_t x = D.col_off[i], b = x / CO_BLOCK;         // (the host checked the offsets: 0 <= x <= n_cols, so b < nb1)
    bool present;
    const CoordRec r = D.rec[(size_t)b * D.N + g];
    ivt[t] = CoordIv{left[t], right[t], co_rank(r, (int)(x - b * CO_BLOCK), &present), x << 1 | (rev[t] ? 1 : 0)};
}

// rules 1 and 3: a thread per (query, genome); the 64 / N queries of a wave lie in consecutive lanes, so a query's `defined` mask is a
// piece of one ballot and the positions leave in one coalesced store.  FROM_POS: the column comes from rule 2 (every lane of a query
// runs the same search: the loads are the same addresses)
template <bool FROM_POS>
__global__ void __launch_bounds__(256) coord_positions(CoordDev D, int64_t n, const int64_t *__restrict__ qa, const int64_t *__restrict__ qb, const int32_t *__restrict__ qs,
                                                       int nearest, int64_t *__restrict__ out, uint32_t *__restrict__ defined, int64_t *__restrict__ iv_out, uint32_t *__restrict__ flag)
{
    const int lane = threadIdx.x & 63, qpw = 64 / D.N, slot = lane / D.N, g = lane - slot * D.N;
    const int64_t q = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * qpw + slot;
    const bool live = slot < qpw && q < n;
    int64_t i = -1, x = 0; uint32_t bad = 0;
    if (live) {
        if (FROM_POS) { int64_t c0; if (co_find(D, qs[q], qa[q], &i, &x, &c0, &bad)) i = -1; }
        else {
            const int64_t qi = qa[q], c = qb[q];
            if (qi < 0 || qi >= D.n_iv) bad = CO_BAD_ARG;
            else {
                const int64_t o0 = D.col_off[qi], o1 = D.col_off[qi + 1];
                if (c < 0 || c >= o1 - o0) bad = CO_BAD_ARG; else { i = qi; x = o0 + c; }
            }
        }
    }
    int64_t pos = 0; bool present = false;
    if (live && i >= 0) {
        CoordIv I; int64_t k;
        if (co_column(D, i, x, g, &I, &present, &k) && (present || nearest)) {
            const int64_t p = co_residue(I, present ? k : (k > 0 ? k - 1 : 0));   // gapped here: the residue before the column, else the first one
            pos = (I.col0_rev & 1) ? -p : p;
        }
    }
    const uint64_t B = __ballot(present);
    if (live) {
        out[(size_t)q * D.N + g] = pos;
        if (g == 0) {
            defined[q] = (uint32_t)(B >> (slot * D.N)) & (D.N >= 32 ? ~0u : (1u << D.N) - 1u);
            if (FROM_POS) iv_out[q] = i;
        }
    }
    if (bad && g == 0) atomicOr(flag, bad);                  // (every lane of a query finds the same: one of them reports)
}

__global__ void __launch_bounds__(256) coord_select(CoordDev D, int64_t n, const int32_t *__restrict__ qs, const int64_t *__restrict__ qp, int64_t *__restrict__ iv_out,
                                                    int64_t *__restrict__ col_out, uint32_t *__restrict__ flag)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    int64_t i = -1, x = 0, c0 = 0; uint32_t bad = 0;
    if (co_find(D, qs[q], qp[q], &i, &x, &c0, &bad) == 0) { iv_out[q] = i; col_out[q] = x - c0; }
    else { iv_out[q] = -1; col_out[q] = -1; }
    if (bad) atomicOr(flag, bad);
}

// Build the index of an alignment whose columns are on the device (d_cols) and whose interval table is on the host, into the slot X with
// its buffer (the index in force: ctx->co / co_index; the correct alignment of DESIGN.md S17: ctx->co_truth / co_truth_index).  bb_work is
// scratch of the build: the call ends in a stream synchronise.
int coord_build_index(mauve_ctx *c, const char *who, mauve_ctx::CoordIndex &X, DevBuf &index, const AlnView &A)
{
    const int N = A.N; const int64_t n_iv = A.n_iv, *left = A.left, *right = A.right, *col_off = A.col_off;
    X.valid = false;
    const std::string w = who;
    if (N < 1 || N > MAUVE_MAX_SEQ) { c->err = w + ": genome count out of range"; return MAUVE_ERR_ARG; }
    const int64_t n_cols = col_off[n_iv], nb1 = n_cols / CO_BLOCK + 1;
    if (n_iv * N > 0x7fffffff || nb1 * N > 0x7fffffff) { c->err = w + ": alignment too large for the index"; return MAUVE_ERR_LIMIT; }
    // the genome tables: every genome's intervals by left end; a base lies in at most one of them (rule 2 needs that)
    struct Row { int64_t left, right, iv; };
    std::vector<int64_t> tleft, tright, tiv;
    CoordDev D; memset(&D, 0, sizeof D);
    CoordTotals want; memset(&want, 0, sizeof want);
    std::vector<Row> rows;
    for (int g = 0; g < N; g++) {
        rows.clear();
        for (int64_t i = 0; i < n_iv; i++) {
            const int64_t l = left[(size_t)(i * N + g)], r = right[(size_t)(i * N + g)];
            if (l < 0 || (l && r < l)) { c->err = w + ": interval " + std::to_string(i) + " has ends out of order in genome " + std::to_string(g); return MAUVE_ERR_ARG; }
            if (l) { rows.push_back(Row{l, r, i}); want.v[g] += r - l + 1; }
        }
        std::sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) { return a.left != b.left ? a.left < b.left : a.iv < b.iv; });
        for (size_t k = 1; k < rows.size(); k++)
            if (rows[k].left <= rows[k - 1].right) {
                c->err = w + ": intervals " + std::to_string(rows[k - 1].iv) + " and " + std::to_string(rows[k].iv) + " overlap in genome " + std::to_string(g);
                return MAUVE_ERR_ARG;
            }
        D.tab_off[g] = (uint32_t)tleft.size();
        for (const Row &r : rows) { tleft.push_back(r.left); tright.push_back(r.right); tiv.push_back(r.iv); }
        D.samp_off[g + 1] = D.samp_off[g] + (uint32_t)(want.v[g] / CO_SAMPLE + 2);
    }
    D.tab_off[N] = (uint32_t)tleft.size();
    const size_t n_tab = tleft.size(), n_samp = D.samp_off[N], n_rec = (size_t)nb1 * N, n_ivg = (size_t)n_iv * N;
    // the index: records | interval rows | column offsets | genome tables | samples
    const size_t o_ivt = up64(n_rec * sizeof(CoordRec)), o_off = o_ivt + up64(n_ivg * sizeof(CoordIv)), o_tl = o_off + up64(((size_t)n_iv + 1) * 8), o_tr = o_tl + up64(n_tab * 8),
                 o_ti = o_tr + up64(n_tab * 8), o_samp = o_ti + up64(n_tab * 8), total = o_samp + up64(n_samp * 4);
    // work area: block counts | their scan | tile sums | raw ends and strands | flag
    const uint32_t n_scan = (uint32_t)n_rec, n_tiles = (n_scan + devscan::TILE - 1) / devscan::TILE;
    const size_t w_pre = up64(n_rec * 4), w_bsum = w_pre + up64((n_rec + 1) * 8), w_left = w_bsum + up64((size_t)n_tiles * 8), w_right = w_left + up64(n_ivg * 8),
                 w_rev = w_right + up64(n_ivg * 8), w_flag = w_rev + up64(n_ivg), w_total = w_flag + 64;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, index.ensure(total + 64));
    HIPCHK(c, c->bb_work.ensure(w_total));
    char *ix = index.as<char>(), *wk = c->bb_work.as<char>();
    D.rec = reinterpret_cast<const CoordRec *>(ix); D.ivt = reinterpret_cast<const CoordIv *>(ix + o_ivt); D.col_off = reinterpret_cast<const int64_t *>(ix + o_off);
    D.tleft = reinterpret_cast<const int64_t *>(ix + o_tl); D.tright = reinterpret_cast<const int64_t *>(ix + o_tr); D.tiv = reinterpret_cast<const int64_t *>(ix + o_ti);
    D.samp = reinterpret_cast<const uint32_t *>(ix + o_samp);
    D.n_iv = n_iv; D.nb1 = nb1; D.N = N;
    HIPCHK(c, hipMemcpyAsync(ix + o_off, col_off, ((size_t)n_iv + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (n_tab) {
        HIPCHK(c, hipMemcpyAsync(ix + o_tl, tleft.data(), n_tab * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(ix + o_tr, tright.data(), n_tab * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(ix + o_ti, tiv.data(), n_tab * 8, hipMemcpyHostToDevice, c->stream));
    }
    if (n_ivg) {
        HIPCHK(c, hipMemcpyAsync(wk + w_left, left, n_ivg * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(wk + w_right, right, n_ivg * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(wk + w_rev, A.reverse, n_ivg, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMemsetAsync(ix + o_samp, 0, n_samp * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(wk + w_flag, 0, 64, c->stream));
    CoordRec *rec = reinterpret_cast<CoordRec *>(ix);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(wk);
    int64_t *pre = reinterpret_cast<int64_t *>(wk + w_pre), *bsum = reinterpret_cast<int64_t *>(wk + w_bsum);
    hipLaunchKernelGGL(coord_build, dim3((uint32_t)((nb1 + 3) / 4)), dim3(256), 0, c->stream, A.d_cols, n_cols, N, nb1, rec, cnt);
    const CoCnt in{cnt, (uint32_t)nb1, N};
    hipLaunchKernelGGL((devscan::vscan_partial<int64_t, CoCnt>), dim3(n_tiles), dim3(256), 0, c->stream, in, n_scan, bsum);
    hipLaunchKernelGGL((devscan::vscan_write<int64_t, CoCnt>), dim3(n_tiles), dim3(256), 0, c->stream, in, n_scan, bsum, pre, (int64_t *)nullptr);
    hipLaunchKernelGGL(coord_finish, dim3((uint32_t)((n_rec + 255) / 256)), dim3(256), 0, c->stream, pre, D, want, rec, reinterpret_cast<uint32_t *>(ix + o_samp),
                       reinterpret_cast<uint32_t *>(wk + w_flag));
    if (n_ivg)
        hipLaunchKernelGGL(coord_iv_rows, dim3((uint32_t)((n_ivg + 255) / 256)), dim3(256), 0, c->stream, D, reinterpret_cast<const int64_t *>(wk + w_left),
                           reinterpret_cast<const int64_t *>(wk + w_right), reinterpret_cast<const int8_t *>(wk + w_rev), reinterpret_cast<CoordIv *>(ix + o_ivt));
    HIPCHK(c, hipGetLastError());
    uint32_t flag = 0;
    HIPCHK(c, hipMemcpyAsync(&flag, wk + w_flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));               // (the tables above are host vectors of this call)
    if (flag) { c->err = w + ": the columns do not hold the residues the interval ends announce"; return MAUVE_ERR_ARG; }
    if (!X.dev) X.dev = new CoordDev;
    *X.dev = D;
    X.N = N; X.n_iv = n_iv; X.n_cols = n_cols; X.genome_gen = c->genome_gen; X.valid = true;
    return MAUVE_OK;
}

enum { CO_COLUMNS = 0, CO_SELECT = 1, CO_TRANSLATE = 2 };

// One batch of queries: in chunks through ctx->co_q (inputs | outputs), page-locked caller arrays copied directly, pageable ones through
// ctx->pin_stage.  a / b / s: the 64-bit and 32-bit query arrays of the kind; o_pos [n*N], o_def [n], o_iv [n], o_col [n]: outputs, any may be NULL.
int coord_run(mauve_ctx *c, int kind, int64_t n, const int64_t *a, const int64_t *b, const int32_t *s, int nearest, int64_t *o_pos, uint32_t *o_def, int64_t *o_iv,
              int64_t *o_col)
{
    const mauve_ctx::CoordIndex &X = c->co;
    if (!X.valid) { c->err = "coord query: no index in this context (mauve_coord_index first)"; return MAUVE_ERR_STATE; }
    if (n < 0 || (n && (!a || (kind == CO_COLUMNS ? !b : !s)))) { c->err = "coord query: missing query arrays"; return MAUVE_ERR_ARG; }
    if (n == 0) return MAUVE_OK;
    const CoordDev &D = *X.dev;
    const int N = X.N;
    const bool has_pos = kind != CO_SELECT, has_col = kind == CO_SELECT, has_iv = kind != CO_COLUMNS;
    const size_t per_in = 8 + (kind == CO_COLUMNS ? 8 : 4), per_out = (has_pos ? (size_t)N * 8 + 4 : 0) + (has_iv ? 8 : 0) + (has_col ? 8 : 0);
    // queries per launch: below the grid limit, and a chunk of at most 256 MiB
    const size_t m = (size_t)std::min<int64_t>(n, std::min<int64_t>((int64_t)1 << 22, std::max<int64_t>(4096, ((int64_t)256 << 20) / (int64_t)(per_in + per_out))));
    const size_t i_a = 64, i_b = i_a + up64(m * 8), i_end = i_b + up64(m * (kind == CO_COLUMNS ? 8 : 4));
    const size_t r_pos = i_end, r_def = r_pos + (has_pos ? up64(m * N * 8) : 0), r_iv = r_def + (has_pos ? up64(m * 4) : 0), r_col = r_iv + (has_iv ? up64(m * 8) : 0),
                 r_end = r_col + (has_col ? up64(m * 8) : 0);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->co_q.ensure(r_end));
    char *qd = c->co_q.as<char>();
    const bool in_direct = host_pointer_is_pinned(a) && host_pointer_is_pinned(kind == CO_COLUMNS ? (const void *)b : (const void *)s);
    const bool out_direct = (!o_pos || host_pointer_is_pinned(o_pos)) && (!o_def || host_pointer_is_pinned(o_def)) && (!o_iv || host_pointer_is_pinned(o_iv)) &&
                            (!o_col || host_pointer_is_pinned(o_col));
    HIPCHK(c, c->pin_stage.ensure(in_direct && out_direct ? 64 : r_end));
    char *hb = c->pin_stage.as<char>();
    // the outputs: the caller's array (NULL: not wanted), its place in a chunk, bytes per query
    const struct { void *dst; size_t off, per; } outs[4] = {{o_pos, r_pos, (size_t)N * 8}, {o_def, r_def, 4}, {o_iv, r_iv, 8}, {o_col, r_col, 8}};
    HIPCHK(c, hipMemsetAsync(qd, 0, 64, c->stream));          // the error flag
    uint32_t *flag = reinterpret_cast<uint32_t *>(qd);
    for (int64_t q0 = 0; q0 < n; q0 += (int64_t)m) {
        const size_t nq = (size_t)std::min<int64_t>((int64_t)m, n - q0), nb2 = nq * (kind == CO_COLUMNS ? 8 : 4);
        const void *src2 = kind == CO_COLUMNS ? (const void *)(b + q0) : (const void *)(s + q0);
        if (in_direct) {
            HIPCHK(c, hipMemcpyAsync(qd + i_a, a + q0, nq * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(qd + i_b, src2, nb2, hipMemcpyHostToDevice, c->stream));
        } else {
            memcpy(hb + i_a, a + q0, nq * 8); memcpy(hb + i_b, src2, nb2);
            HIPCHK(c, hipMemcpyAsync(qd + i_a, hb + i_a, i_b - i_a + nb2, hipMemcpyHostToDevice, c->stream));
        }
        const int64_t *d_a = reinterpret_cast<const int64_t *>(qd + i_a), *d_b = reinterpret_cast<const int64_t *>(qd + i_b);
        const int32_t *d_s = reinterpret_cast<const int32_t *>(qd + i_b);
        int64_t *d_pos = reinterpret_cast<int64_t *>(qd + r_pos), *d_iv = reinterpret_cast<int64_t *>(qd + r_iv), *d_col = reinterpret_cast<int64_t *>(qd + r_col);
        uint32_t *d_def = reinterpret_cast<uint32_t *>(qd + r_def);
        const size_t waves = (nq + (size_t)(64 / N) - 1) / (size_t)(64 / N);
        if (kind == CO_COLUMNS)
            hipLaunchKernelGGL(coord_positions<false>, dim3((uint32_t)((waves + 3) / 4)), dim3(256), 0, c->stream, D, (int64_t)nq, d_a, d_b, (const int32_t *)nullptr, nearest, d_pos, d_def,
                               (int64_t *)nullptr, flag);
        else if (kind == CO_TRANSLATE)
            hipLaunchKernelGGL(coord_positions<true>, dim3((uint32_t)((waves + 3) / 4)), dim3(256), 0, c->stream, D, (int64_t)nq, d_a, (const int64_t *)nullptr, d_s, nearest, d_pos, d_def,
                               d_iv, flag);
        else
            hipLaunchKernelGGL(coord_select, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, c->stream, D, (int64_t)nq, d_s, d_a, d_iv, d_col, flag);
        HIPCHK(c, hipGetLastError());
        for (const auto &o : outs)
            if (o.dst) HIPCHK(c, hipMemcpyAsync(out_direct ? static_cast<char *>(o.dst) + (size_t)q0 * o.per : hb + o.off, qd + o.off, nq * o.per, hipMemcpyDeviceToHost, c->stream));
        if (!in_direct || !out_direct) HIPCHK(c, hipStreamSynchronize(c->stream));     // the staging is reused by the next chunk
        if (!out_direct)
            for (const auto &o : outs) if (o.dst) memcpy(static_cast<char *>(o.dst) + (size_t)q0 * o.per, hb + o.off, nq * o.per);
    }
    return co_flag_read(c, flag, "coord query", "a query lies outside the alignment (interval id, column, genome index or a position below 1)");
}

}  // namespace

// The index of a caller's alignment (the arrays of mauve_align_fetch) in the slot X: the front end's checks (aln_from_arrays), the build.
// bb_cols holds the caller's columns during the call.
int coord_index_arrays(mauve_ctx *c, const char *who, mauve_ctx::CoordIndex &X, DevBuf &index, int nseq, int64_t n_iv, const int64_t *left, const int64_t *right,
                       const int8_t *reverse, const int64_t *col_off, const uint32_t *cols)
{
    X.valid = false;
    AlnView A;
    if (const int rc = aln_from_arrays(c, who, nseq, n_iv, left, right, reverse, col_off, cols, &A)) return rc;
    return coord_build_index(c, who, X, index, A);
}

// The index in force from columns that are on the device already and an interval table on the host (project_dev.hip)
int coord_index_device(mauve_ctx *c, const char *who, const AlnView &A) { return coord_build_index(c, who, c->co, c->co_index, A); }

extern "C" {

int mauve_coord_index(mauve_ctx *c)
{
    if (!c) return MAUVE_ERR_ARG;
    c->co.valid = false; c->ex.valid = false; c->exc.valid = false; c->fm.valid = false; c->tx.valid = false;      // (a selection, DESIGN.md S15, an excursion result, S18, a range map, S21, and a text, S23, belong to the index they were made on)
    AlnView A;
    if (const int rc = aln_from_context(c, "coord_index", false, c->bb_cols, &A)) return rc;
    if (const int rco = coord_check_offsets(c, "coord_index", A.n_iv, A.col_off)) return rco;
    return coord_build_index(c, "coord_index", c->co, c->co_index, A);    // (an empty alignment has an index, too)
}

int mauve_coord_index_alignment(mauve_ctx *c, int nseq, int64_t n_iv, const int64_t *left, const int64_t *right, const int8_t *reverse, const int64_t *col_off, const uint32_t *cols)
{
    if (!c) return MAUVE_ERR_ARG;
    c->co.valid = false; c->ex.valid = false; c->exc.valid = false; c->fm.valid = false; c->tx.valid = false;      // (a selection, DESIGN.md S15, an excursion result, S18, a range map, S21, and a text, S23, belong to the index they were made on)
    return coord_index_arrays(c, "coord_index", c->co, c->co_index, nseq, n_iv, left, right, reverse, col_off, cols);
}

int mauve_coord_index_size(mauve_ctx *c, int *nseq, int64_t *n_iv, int64_t *n_cols)
{
    if (!c) return MAUVE_ERR_ARG;
    if (!c->co.valid) { c->err = "coord_index_size: no index in this context (mauve_coord_index first)"; return MAUVE_ERR_STATE; }
    if (nseq) *nseq = c->co.N;
    if (n_iv) *n_iv = c->co.n_iv;
    if (n_cols) *n_cols = c->co.n_cols;
    return MAUVE_OK;
}

int mauve_column_positions(mauve_ctx *c, int64_t n, const int64_t *iv, const int64_t *col, int nearest, int64_t *pos, uint32_t *defined)
{
    if (!c) return MAUVE_ERR_ARG;
    return coord_run(c, CO_COLUMNS, n, iv, col, nullptr, nearest != 0, pos, defined, nullptr, nullptr);
}

int mauve_seqpos_to_column(mauve_ctx *c, int64_t n, const int32_t *seq, const int64_t *pos, int64_t *iv, int64_t *col)
{
    if (!c) return MAUVE_ERR_ARG;
    return coord_run(c, CO_SELECT, n, pos, nullptr, seq, 0, nullptr, nullptr, iv, col);
}

int mauve_translate_positions(mauve_ctx *c, int64_t n, const int32_t *seq, const int64_t *pos, int nearest, int64_t *out, uint32_t *defined, int64_t *iv)
{
    if (!c) return MAUVE_ERR_ARG;
    return coord_run(c, CO_TRANSLATE, n, pos, nullptr, seq, nearest != 0, out, defined, iv, nullptr);
}

}  // extern "C"
