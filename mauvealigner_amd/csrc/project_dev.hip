// project_dev.hip -- the alignment projected onto a subset of the genomes, what becomes collinear coalesced into new intervals.
// The stage stands in for libMems' projectIntervalList (alignmentProjector.cpp:58-77, multiEVD.cpp:142-172, bbBreakOnGenes.cpp:54) and for the
// loop projectAndStrip writes out by hand (projectAndStrip.cpp:75-122).  It reads the coordinate index in force (S14, coord_index.hpp): the
// interval rows come back to the host (10^2 .. 10^4 of them), where rules 1 to 4 make a piece table in output order; the columns never leave
// the device.
//   piece       a kept source interval (its columns [x0, x0 + len) of the whole array, taken descending when flipped) or a filler (len
//               columns with the one bit of its genome)
//   unit        a 64-column word of the index that a source piece touches, or up to PJ_FILL columns of a filler: the work of one wave
//   pj_count    a thread per unit: the words of the projected genomes ORed, both ends masked = the unit's kept columns, a word that stays in
//               the work area; their number
//   vscan       over the units' counts (dev_scan.hpp): every unit's first output column; pj_firsts picks every piece's out of it, which the
//               host turns into col_off (one synchronise brings them and the flag back)
//   pj_write    a wave per unit, a lane per source column: its bits from the planes (the lanes of a wave share the addresses), its rank among
//               the kept columns of the word by a popcount below it; stores ascend, or descend for a flipped piece
//   pj_source   the same walk without the index, from the kept words alone: every output column's source column.  Made by the first fetch
//               that asks for src_col (a caller who only indexes the projection never pays its 8 bytes per column)
//   pj_permute  the compact form of a fetch: bit k = genome proj[k]
// Every index a kernel forms is checked first (block against the index, destination against the output); a thread that finds something
// wrong sets CO_BAD_INDEX in the flag word.  The result (columns and the work area on the device, the tables on the host) stays in the
// context for its fetches and for mauve_project_index, which hands it to coord_build_index.
#include "common.hpp"
#include "coord_index.hpp"
#include "dev_scan.hpp"
#include <algorithm>
#include <cstring>

namespace {

constexpr int PJ_FILL = 1024;                     // filler columns per unit

struct alignas(32) PjPiece { int64_t x0, len, unit0; int32_t fill_g, flip; };      // fill_g < 0: a source piece
struct PjReq { int n_proj; int32_t proj[MAUVE_MAX_SEQ]; int drop_empty; };
struct PjCnt { const uint32_t *v; __device__ int64_t value(uint32_t i) const { return v[i]; } };

// the work area of a projection of n_piece pieces and n_unit units (pj_work; it stays with the result: pj_source reads it):
// flag | pieces | unit counts | their scan | tile sums | the pieces' first columns | the units' kept words
struct PjWork {
    size_t pc, cnt, pre, bs, first, kept, total; uint32_t tiles;
    PjWork(size_t nP, size_t nU) : tiles((uint32_t)((nU + devscan::TILE - 1) / devscan::TILE))
    {
        pc = 64; cnt = pc + up64(nP * sizeof(PjPiece)); pre = cnt + up64(nU * 4); bs = pre + up64((nU + 1) * 8); first = bs + up64((size_t)tiles * 8);
        kept = first + up64(nP * 8); total = kept + up64(nU * 8);
    }
};

// unit u -> its piece (the last one that starts at or before u; pieces hold at least one unit each, entry n_piece closes the table)
__device__ __forceinline__ int64_t pj_piece_of(const PjPiece *__restrict__ pc, int64_t n_piece, int64_t u)
{
    int64_t a = 0, e = n_piece;
    while (e - a > 1) { const int64_t mid = (a + e) >> 1; if (pc[mid].unit0 <= u) a = mid; else e = mid; }
    return a;
}

// the columns of word W (whole array) that belong to the piece
__device__ __forceinline__ uint64_t pj_inside(const PjPiece &P, int64_t W)
{
    const int64_t lo = P.x0 - W * 64, hi = P.x0 + P.len - W * 64;
    return co_below(hi > 64 ? 64 : (int)hi) & ~co_below(lo < 0 ? 0 : (int)lo);
}

__global__ void __launch_bounds__(256) pj_count(CoordDev D, PjReq Q, const PjPiece *__restrict__ pc, int64_t n_piece, int64_t n_unit, uint32_t *__restrict__ cnt,
                                                uint64_t *__restrict__ kept, uint32_t *__restrict__ flag)
{
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= n_unit) return;
    const PjPiece P = pc[pj_piece_of(pc, n_piece, u)];
    const int64_t r = u - P.unit0;
    if (P.fill_g >= 0) { cnt[u] = (uint32_t)min((int64_t)PJ_FILL, P.len - r * PJ_FILL); kept[u] = 0; return; }
    const int64_t W = (P.x0 >> 6) + r, b = W / CO_WORDS;
    if (b < 0 || b >= D.nb1) { cnt[u] = 0; kept[u] = 0; atomicOr(flag, CO_BAD_INDEX); return; }
    uint64_t m = pj_inside(P, W);
    if (Q.drop_empty) {
        uint64_t any = 0;
        for (int k = 0; k < Q.n_proj; k++) any |= D.rec[(size_t)b * D.N + Q.proj[k]].w[W - b * CO_WORDS];
        m &= any;
    }
    cnt[u] = (uint32_t)__popcll(m); kept[u] = m;
}

__global__ void __launch_bounds__(256) pj_firsts(const PjPiece *__restrict__ pc, int64_t n_piece, const int64_t *__restrict__ pre, int64_t *__restrict__ first)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p <= n_piece) first[p] = pre[pc[p].unit0];
}

__global__ void __launch_bounds__(256) pj_write(CoordDev D, PjReq Q, const PjPiece *__restrict__ pc, int64_t n_piece, int64_t n_unit, const int64_t *__restrict__ pre,
                                                const int64_t *__restrict__ first, const uint64_t *__restrict__ kept, int64_t n_out, uint32_t *__restrict__ out,
                                                uint32_t *__restrict__ flag)
{
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= n_unit) return;
    const int64_t p = pj_piece_of(pc, n_piece, u);
    const PjPiece P = pc[p];
    const int64_t r = u - P.unit0, o0 = pre[u], pf = first[p], pe = first[p + 1];
    bool bad = false;
    if (P.fill_g >= 0) {
        const int64_t n = min((int64_t)PJ_FILL, P.len - r * PJ_FILL);
        for (int64_t j = lane; j < n; j += 64) {
            const int64_t dst = o0 + j;
            if (dst < 0 || dst >= n_out) { bad = true; break; }
            out[dst] = 1u << P.fill_g;
        }
    } else {
        const int64_t W = (P.x0 >> 6) + r, b = W / CO_WORDS;
        if (b < 0 || b >= D.nb1) bad = true;
        else {
            uint32_t mask = 0;
            for (int k = 0; k < Q.n_proj; k++) {
                const int g = Q.proj[k];
                mask |= (uint32_t)(D.rec[(size_t)b * D.N + g].w[W - b * CO_WORDS] >> lane & 1) << g;
            }
            const uint64_t m = kept[u];
            if (m >> lane & 1) {
                const int64_t k = o0 - pf + __popcll(m & co_below(lane)), dst = P.flip ? pe - 1 - k : pf + k;
                if (k < 0 || dst < pf || dst >= pe || dst >= n_out) bad = true; else out[dst] = mask;
            }
        }
    }
    if (bad) atomicOr(flag, CO_BAD_INDEX);
}

__global__ void __launch_bounds__(256) pj_source(const PjPiece *__restrict__ pc, int64_t n_piece, int64_t n_unit, const int64_t *__restrict__ pre, const int64_t *__restrict__ first,
                                                 const uint64_t *__restrict__ kept, int64_t n_out, int64_t *__restrict__ src_col, uint32_t *__restrict__ flag)
{
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= n_unit) return;
    const int64_t p = pj_piece_of(pc, n_piece, u);
    const PjPiece P = pc[p];
    const int64_t r = u - P.unit0, o0 = pre[u], pf = first[p], pe = first[p + 1];
    bool bad = false;
    if (P.fill_g >= 0) {
        const int64_t n = min((int64_t)PJ_FILL, P.len - r * PJ_FILL);
        for (int64_t j = lane; j < n; j += 64) {
            const int64_t dst = o0 + j;
            if (dst < 0 || dst >= n_out) { bad = true; break; }
            src_col[dst] = -1;
        }
    } else {
        const uint64_t m = kept[u];
        if (m >> lane & 1) {
            const int64_t k = o0 - pf + __popcll(m & co_below(lane)), dst = P.flip ? pe - 1 - k : pf + k;
            if (k < 0 || dst < pf || dst >= pe || dst >= n_out) bad = true; else src_col[dst] = ((P.x0 >> 6) + r) * 64 + lane;
        }
    }
    if (bad) atomicOr(flag, CO_BAD_INDEX);
}

__global__ void __launch_bounds__(256) pj_permute(PjReq Q, int64_t n, const uint32_t *__restrict__ in, uint32_t *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const uint32_t m = in[t];
    uint32_t o = 0;
    for (int k = 0; k < Q.n_proj; k++) o |= (m >> Q.proj[k] & 1u) << k;
    out[t] = o;
}

PjReq pj_request(const mauve_ctx::Projection &R)
{
    PjReq Q; memset(&Q, 0, sizeof Q);
    Q.n_proj = R.n_proj; Q.drop_empty = R.drop_empty;
    for (int k = 0; k < R.n_proj; k++) Q.proj[k] = R.proj[k];
    return Q;
}

// rules 1 to 4 on the interval rows of the index: the tables of the result (all but col_off) and the piece table in output order, closed
// by an entry that holds the number of units.  out_piece[o]: the first piece of output interval o.
int pj_plan(mauve_ctx *c, mauve_ctx::Projection &R, const CoordIv *iv, int64_t n_iv, std::vector<PjPiece> &pieces, std::vector<int64_t> &out_piece)
{
    const int N = R.N, np = R.n_proj, g0 = R.proj[0];
    std::vector<int64_t> kept;
    for (int64_t i = 0; i < n_iv; i++) {
        bool all = true;
        for (int k = 0; k < np && all; k++) all = iv[(size_t)i * N + R.proj[k]].left != 0;
        if (all) kept.push_back(i);
    }
    std::sort(kept.begin(), kept.end(), [&](int64_t a, int64_t b) { return iv[(size_t)a * N + g0].left < iv[(size_t)b * N + g0].left; });
    const size_t K = kept.size();
    auto row = [&](int64_t i, int g) -> const CoordIv & { return iv[(size_t)i * N + g]; };
    auto flipped = [&](int64_t i) { return (int)(row(i, g0).col0_rev & 1); };
    auto rev_of = [&](int64_t i, int g) { return (int)(row(i, g).col0_rev & 1) ^ flipped(i); };
    // rule 3: S5's rule on records of length 1 at the signed left ends
    MatchVec m(np); m.resize(K);
    for (size_t q = 0; q < K; q++) {
        m.len(q) = 1;
        for (int k = 0; k < np; k++) { const int64_t l = row(kept[q], R.proj[k]).left; m.st(q)[k] = rev_of(kept[q], R.proj[k]) ? -l : l; }
    }
    std::vector<int64_t> label; int64_t n_lcb = 0;
    host_lcb_chain(m, 0, false, label, n_lcb);
    R.left.clear(); R.right.clear(); R.reverse.clear(); R.src_off.assign(1, 0); R.src_iv.clear(); R.src_flip.clear(); R.n_fill = 0;
    pieces.clear(); out_piece.clear();
    int64_t n_unit = 0;
    auto push = [&](int64_t x0, int64_t len, int fill_g, int flip) {
        pieces.push_back(PjPiece{x0, len, n_unit, fill_g, flip});
        n_unit += fill_g >= 0 ? (len + PJ_FILL - 1) / PJ_FILL : ((x0 + len - 1) >> 6) - (x0 >> 6) + 1;
    };
    for (size_t q = 0; q < K; q++) {
        const int64_t i = kept[q];
        const bool first = q == 0 || label[q] != label[q - 1];
        if (first) {
            out_piece.push_back((int64_t)pieces.size());
            if (q) R.src_off.push_back((int64_t)R.src_iv.size());
            const size_t o = R.left.size();
            R.left.resize(o + (size_t)N, 0); R.right.resize(o + (size_t)N, 0); R.reverse.resize(o + (size_t)N, 0);
            for (int k = 0; k < np; k++) { const int g = R.proj[k]; R.left[o + g] = row(i, g).left; R.right[o + g] = row(i, g).right; R.reverse[o + g] = (int8_t)rev_of(i, g); }
        } else {
            const int64_t a = kept[q - 1];
            const size_t o = R.left.size() - (size_t)N;
            for (int k = 0; k < np; k++) {                    // rule 4: the bases strictly between the two pieces, genome after genome
                const int g = R.proj[k];
                const int64_t d = rev_of(i, g) ? row(a, g).left - row(i, g).right - 1 : row(i, g).left - row(a, g).right - 1;
                if (d < 0 || rev_of(i, g) != R.reverse[o + g]) { c->err = "project: the interval table of the index is inconsistent"; return MAUVE_ERR_STATE; }
                if (d) { push(0, d, g, 0); R.n_fill += d; }
                R.left[o + g] = std::min(R.left[o + g], row(i, g).left); R.right[o + g] = std::max(R.right[o + g], row(i, g).right);
            }
        }
        const int64_t x0 = row(i, g0).col0_rev >> 1, x1 = i + 1 < n_iv ? row(i + 1, g0).col0_rev >> 1 : c->co.n_cols;
        if (x1 <= x0) { c->err = "project: a kept interval of the index has no columns"; return MAUVE_ERR_STATE; }
        push(x0, x1 - x0, -1, flipped(i));
        R.src_iv.push_back(i); R.src_flip.push_back((int8_t)flipped(i));
    }
    R.src_off.push_back((int64_t)R.src_iv.size());
    if (!K) R.src_off.assign(1, 0);
    pieces.push_back(PjPiece{0, 0, n_unit, -1, 0});
    R.n_iv = (int64_t)out_piece.size();
    return MAUVE_OK;
}

}  // namespace

extern "C" {

void mauve_default_project_params(int nseq, mauve_project_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->n_proj = std::max(0, std::min(nseq, MAUVE_MAX_SEQ));
    for (int k = 0; k < p->n_proj; k++) p->proj[k] = k;
    p->drop_empty = 1;
}

int mauve_project(mauve_ctx *c, const mauve_project_params *p, mauve_project_sizes *sz)
{
    if (!c) return MAUVE_ERR_ARG;
    mauve_ctx::Projection &R = c->pj;
    R.valid = false;
    const mauve_ctx::CoordIndex &X = c->co;
    if (!X.valid) { c->err = "project: no index in this context (mauve_coord_index first)"; return MAUVE_ERR_STATE; }
    const int N = X.N;
    if (!p || p->n_proj < 1 || p->n_proj > N) { c->err = "project: n_proj outside [1, nseq]"; return MAUVE_ERR_ARG; }
    uint32_t seen = 0;
    for (int k = 0; k < p->n_proj; k++) {
        const int g = p->proj[k];
        if (g < 0 || g >= N || (seen >> g & 1)) { c->err = "project: proj[" + std::to_string(k) + "] is outside [0, nseq) or repeated"; return MAUVE_ERR_ARG; }
        seen |= 1u << g;
    }
    R.N = N; R.n_proj = p->n_proj; R.drop_empty = p->drop_empty != 0; R.genome_gen = X.genome_gen;
    for (int k = 0; k < p->n_proj; k++) R.proj[k] = p->proj[k];
    const CoordDev &D = *X.dev;
    const int64_t n_iv = X.n_iv;
    const size_t b_iv = (size_t)n_iv * (size_t)N * sizeof(CoordIv);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->pin_stage.ensure(b_iv + 64));
    if (b_iv) HIPCHK(c, hipMemcpyAsync(c->pin_stage.p, D.ivt, b_iv, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<PjPiece> pieces; std::vector<int64_t> out_piece;
    if (const int rp = pj_plan(c, R, c->pin_stage.as<CoordIv>(), n_iv, pieces, out_piece)) return rp;
    const int64_t n_piece = (int64_t)pieces.size() - 1, n_unit = pieces.back().unit0;
    if (n_unit >= ((int64_t)1 << 31) - devscan::TILE) { c->err = "project: the projection has 2^31 units of work or more"; return MAUVE_ERR_LIMIT; }
    R.col_off.assign((size_t)R.n_iv + 1, 0);
    R.n_cols = 0; R.n_piece = n_piece; R.n_unit = n_unit; R.have_src = false;
    HIPCHK(c, c->pj_cols.ensure(64));
    if (n_unit) {
        const size_t nP = (size_t)n_piece + 1, nU = (size_t)n_unit;
        const PjWork L(nP, nU);
        const uint32_t tiles = L.tiles;
        const size_t w_pc = L.pc, w_cnt = L.cnt, w_pre = L.pre, w_bs = L.bs, w_first = L.first;
        HIPCHK(c, c->pj_work.ensure(L.total));
        HIPCHK(c, c->pin_stage.ensure(std::max(nP * sizeof(PjPiece), nP * 8 + 64)));
        char *wk = c->pj_work.as<char>(), *hb = c->pin_stage.as<char>();
        uint32_t *flag = reinterpret_cast<uint32_t *>(wk), *cnt = reinterpret_cast<uint32_t *>(wk + w_cnt);
        const PjPiece *pc = reinterpret_cast<const PjPiece *>(wk + w_pc);
        int64_t *pre = reinterpret_cast<int64_t *>(wk + w_pre), *bs = reinterpret_cast<int64_t *>(wk + w_bs), *first = reinterpret_cast<int64_t *>(wk + w_first);
        uint64_t *kept = reinterpret_cast<uint64_t *>(wk + L.kept);
        const PjReq Q = pj_request(R);
        memcpy(hb, pieces.data(), nP * sizeof(PjPiece));
        HIPCHK(c, hipMemsetAsync(wk, 0, 64, c->stream));
        HIPCHK(c, hipMemcpyAsync(wk + w_pc, hb, nP * sizeof(PjPiece), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(pj_count, dim3((uint32_t)((nU + 255) / 256)), dim3(256), 0, c->stream, D, Q, pc, n_piece, n_unit, cnt, kept, flag);
        const PjCnt in{cnt};
        hipLaunchKernelGGL((devscan::vscan_partial<int64_t, PjCnt>), dim3(tiles), dim3(256), 0, c->stream, in, (uint32_t)nU, bs);
        hipLaunchKernelGGL((devscan::vscan_write<int64_t, PjCnt>), dim3(tiles), dim3(256), 0, c->stream, in, (uint32_t)nU, bs, pre, (int64_t *)nullptr);
        hipLaunchKernelGGL(pj_firsts, dim3((uint32_t)((nP + 255) / 256)), dim3(256), 0, c->stream, pc, n_piece, pre, first);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(hb + 64, first, nP * 8, hipMemcpyDeviceToHost, c->stream));     // (behind the upload of the pieces on the same stream)
        if (const int rf = co_flag_read(c, flag, "project", nullptr)) return rf;
        const int64_t *h_first = reinterpret_cast<const int64_t *>(c->pin_stage.as<char>() + 64);
        for (int64_t o = 0; o < R.n_iv; o++) R.col_off[(size_t)o] = h_first[out_piece[(size_t)o]];
        const int64_t n_out = R.col_off[(size_t)R.n_iv] = R.n_cols = h_first[n_piece];
        HIPCHK(c, c->pj_cols.ensure((size_t)n_out * 4 + 64));
        hipLaunchKernelGGL(pj_write, dim3((uint32_t)((nU + 3) / 4)), dim3(256), 0, c->stream, D, Q, pc, n_piece, n_unit, pre, first, kept, n_out, c->pj_cols.as<uint32_t>(), flag);
        HIPCHK(c, hipGetLastError());
        if (const int rf = co_flag_read(c, flag, "project", nullptr)) return rf;
    }
    R.valid = true;
    if (sz) { sz->n_iv = R.n_iv; sz->n_cols = R.n_cols; sz->n_src = (int64_t)R.src_iv.size(); sz->n_fill = R.n_fill; }
    return MAUVE_OK;
}

int mauve_project_fetch(mauve_ctx *c, int compact, int64_t *left, int64_t *right, int8_t *reverse, int64_t *col_off, uint32_t *cols, int64_t *src_off, int64_t *src_iv,
                        int8_t *src_flip, int64_t *src_col)
{
    if (!c) return MAUVE_ERR_ARG;
    mauve_ctx::Projection &R = c->pj;
    if (!R.valid) { c->err = "project_fetch: no projection in this context (mauve_project first)"; return MAUVE_ERR_STATE; }
    const size_t n_iv = (size_t)R.n_iv, N = (size_t)R.N, np = (size_t)R.n_proj, n_cols = (size_t)R.n_cols;
    for (size_t o = 0; o < n_iv; o++) {
        if (!compact) {
            if (left) std::copy_n(&R.left[o * N], N, left + o * N);
            if (right) std::copy_n(&R.right[o * N], N, right + o * N);
            if (reverse) std::copy_n(&R.reverse[o * N], N, reverse + o * N);
        } else
            for (size_t k = 0; k < np; k++) {
                const size_t s = o * N + (size_t)R.proj[k];
                if (left) left[o * np + k] = R.left[s];
                if (right) right[o * np + k] = R.right[s];
                if (reverse) reverse[o * np + k] = R.reverse[s];
            }
    }
    if (col_off) std::copy(R.col_off.begin(), R.col_off.end(), col_off);
    if (src_off) std::copy(R.src_off.begin(), R.src_off.end(), src_off);
    if (src_iv) std::copy(R.src_iv.begin(), R.src_iv.end(), src_iv);
    if (src_flip) std::copy(R.src_flip.begin(), R.src_flip.end(), src_flip);
    HIPCHK(c, hipSetDevice(c->device));
    if (cols && n_cols) {
        const uint32_t *d = c->pj_cols.as<uint32_t>();
        if (compact) {
            HIPCHK(c, c->pj_out.ensure(n_cols * 4));
            hipLaunchKernelGGL(pj_permute, dim3((uint32_t)((n_cols + 255) / 256)), dim3(256), 0, c->stream, pj_request(R), (int64_t)n_cols, d, c->pj_out.as<uint32_t>());
            HIPCHK(c, hipGetLastError());
            d = c->pj_out.as<uint32_t>();
        }
        if (const int rc = copy_to_caller(c, c->pin_stage, cols, d, n_cols * 4)) return rc;
    }
    if (src_col && n_cols) {
        if (!R.have_src) {                                    // the first fetch that wants them: from the work area the projection left, no index needed
            const PjWork L((size_t)R.n_piece + 1, (size_t)R.n_unit);
            char *wk = c->pj_work.as<char>();
            HIPCHK(c, c->pj_src.ensure(n_cols * 8 + 64));
            HIPCHK(c, hipMemsetAsync(wk, 0, 64, c->stream));
            hipLaunchKernelGGL(pj_source, dim3((uint32_t)(((size_t)R.n_unit + 3) / 4)), dim3(256), 0, c->stream, reinterpret_cast<const PjPiece *>(wk + L.pc), R.n_piece, R.n_unit,
                               reinterpret_cast<const int64_t *>(wk + L.pre), reinterpret_cast<const int64_t *>(wk + L.first), reinterpret_cast<const uint64_t *>(wk + L.kept),
                               (int64_t)n_cols, c->pj_src.as<int64_t>(), reinterpret_cast<uint32_t *>(wk));
            HIPCHK(c, hipGetLastError());
            if (const int rf = co_flag_read(c, reinterpret_cast<uint32_t *>(wk), "project_fetch", nullptr, "the projection")) return rf;
            R.have_src = true;
        }
        if (const int rc = copy_to_caller(c, c->pin_stage, src_col, c->pj_src.p, n_cols * 8)) return rc;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MAUVE_OK;
}

int mauve_project_index(mauve_ctx *c)
{
    if (!c) return MAUVE_ERR_ARG;
    const mauve_ctx::Projection &R = c->pj;
    if (!R.valid) { c->err = "project_index: no projection in this context (mauve_project first)"; return MAUVE_ERR_STATE; }
    if (R.N != c->nseq) { c->err = "project_index: the projection is over " + std::to_string(R.N) + " genomes, the context holds " + std::to_string(c->nseq); return MAUVE_ERR_STATE; }
    if (R.genome_gen != c->genome_gen) { c->err = "project_index: the genomes were replaced after the projected index was built"; return MAUVE_ERR_STATE; }
    c->co.valid = false; c->ex.valid = false; c->exc.valid = false; c->fm.valid = false; c->tx.valid = false;      // (a selection, DESIGN.md S15, an excursion result, S18, a range map, S21, and a text, S23, belong to the index they were made on)
    HIPCHK(c, hipSetDevice(c->device));
    return coord_index_device(c, "project_index", AlnView{R.N, R.n_iv, R.left.data(), R.right.data(), R.reverse.data(), R.col_off.data(), c->pj_cols.as<uint32_t>()});
}

}  // extern "C"
