// homology_dev.hip -- the homology pass in front of the backbone: the two-state pair HMM of detectAndApplyBackbone, on the device.
// The clamp form of the recurrence and the two scans are derived in DESIGN.md S12b.  Intervals are cut into segments of 4096 columns
// (64 steps of 64 lanes); every (interval, pair, segment) is one wave:
//   hom_seg_count  residues of every genome per segment (base positions at the segment starts: host prefix per interval)
//   hom_fn         the segment's composed function                      -> host: x at every segment start, final state
//   hom_pred       the same sweep with x known: predecessor words (2 x 64 bits per step), step maps, the segment's map
//                                                                       -> host: state at every segment end
//   hom_keep       states of all columns from the words and the end state; ORs the pair's bits into keep[column] where the
//                  state is H and both genomes have a base
//   hom_count / hom_write / hom_offsets  the columns split by keep: tile totals, (host prefix over the tiles), the new
//                columns written in order, the new column offset of every interval.
// The host steps between the kernels (work items, the two chaining loops) are in backbone_host.hpp.
#include "common.hpp"
#include "column_counts.hpp"
#include <algorithm>
#include <cstring>
#include <cmath>

namespace {

struct HomGenomes { uint64_t word_off[MAUVE_MAX_SEQ]; };
struct HomScores { int32_t match, mismatch, gap, go_h, go_u; };
constexpr int32_t HOM_MINF = -(1 << 30), HOM_PINF = 1 << 30;

__device__ __forceinline__ int hom_base(const uint64_t *__restrict__ G, int64_t pos0) { return (int)(G[pos0 >> 5] >> ((pos0 & 31) * 2) & 3u); }
__device__ __forceinline__ int32_t hom_clamp(int32_t x, int32_t lo, int32_t hi) { return x < lo ? lo : (x > hi ? hi : x); }
// g2 after g1
__device__ __forceinline__ void hom_compose(int32_t &t, int32_t &lo, int32_t &hi, int32_t t1, int32_t lo1, int32_t hi1)
{
    const int32_t t2 = t, lo2 = lo, hi2 = hi;
    t = t1 + t2; lo = hom_clamp(lo1 + t2, lo2, hi2); hi = hom_clamp(hi1 + t2, lo2, hi2);
    if (lo1 == HOM_MINF && lo2 == HOM_MINF) lo = HOM_MINF;      // two identities stay the identity
    if (hi1 == HOM_PINF && hi2 == HOM_PINF) hi = HOM_PINF;
}
// maps on {U = 0, H = 1} as two bits (bit s = image of s); p after q
__device__ __forceinline__ uint32_t hom_map_after(uint32_t p, uint32_t q) { return ((p >> (q & 1u)) & 1u) | (((p >> (q >> 1 & 1u)) & 1u) << 1); }

struct HomPair {          // what a wave knows about its (interval, pair, segment)
    const uint64_t *Ga, *Gb; int64_t la, ra, lb, rb; bool rva, rvb; int a, b; int64_t c0, n; int64_t ka, kb;
};
__device__ __forceinline__ HomPair hom_setup(const HomItem &item, const HomIv &iv, const int64_t *__restrict__ left, const int64_t *__restrict__ right,
                                             const int8_t *__restrict__ rev, int N, const uint64_t *__restrict__ genomes, const HomGenomes &gw,
                                             const int64_t *__restrict__ rank0)
{
    HomPair P;
    P.a = item.a; P.b = item.b;
    P.la = left[(size_t)iv.iv * N + P.a]; P.ra = right[(size_t)iv.iv * N + P.a]; P.lb = left[(size_t)iv.iv * N + P.b]; P.rb = right[(size_t)iv.iv * N + P.b];
    P.rva = rev[(size_t)iv.iv * N + P.a] != 0; P.rvb = rev[(size_t)iv.iv * N + P.b] != 0;
    P.Ga = genomes + gw.word_off[P.a]; P.Gb = genomes + gw.word_off[P.b];
    P.c0 = iv.col0 + (int64_t)item.seg * HOM_SEG;
    P.n = min((int64_t)HOM_SEG, iv.ncols - (int64_t)item.seg * HOM_SEG);
    P.ka = rank0[(size_t)(iv.seg0 + item.seg) * N + P.a]; P.kb = rank0[(size_t)(iv.seg0 + item.seg) * N + P.b];
    return P;
}
// the column of this lane in step `ch` as a function (identity where neither genome has a base); advances the base counters
__device__ __forceinline__ void hom_column(HomPair &P, const uint32_t *__restrict__ cols, int ch, int lane, const HomScores &sc, int32_t &t, int32_t &lo, int32_t &hi,
                                           bool &none, bool &both)
{
    const int64_t c = (int64_t)ch * 64 + lane;
    const uint32_t m = c < P.n ? cols[P.c0 + c] : 0u;
    const bool ha = m >> P.a & 1u, hb = m >> P.b & 1u;
    none = !(ha || hb); both = ha && hb;
    const uint64_t BA = __ballot(ha), BB = __ballot(hb);
    int32_t s = sc.gap;
    if (both) {
        const int64_t ia = P.ka + __popcll(BA & below(lane)), ib = P.kb + __popcll(BB & below(lane));
        int xa = hom_base(P.Ga, (P.rva ? P.ra - ia : P.la + ia) - 1), xb = hom_base(P.Gb, (P.rvb ? P.rb - ib : P.lb + ib) - 1);
        if (P.rva) xa = 3 - xa;
        if (P.rvb) xb = 3 - xb;
        s = xa == xb ? sc.match : sc.mismatch;
    }
    t = none ? 0 : s; lo = none ? HOM_MINF : sc.go_h + s; hi = none ? HOM_PINF : -sc.go_u + s;
    P.ka += __popcll(BA); P.kb += __popcll(BB);
}
// inclusive scan over the lanes: lane l gets (column l) after ... after (column 0)
__device__ __forceinline__ void hom_scan(int lane, int32_t &t, int32_t &lo, int32_t &hi)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t t1 = __shfl_up(t, d, 64), lo1 = __shfl_up(lo, d, 64), hi1 = __shfl_up(hi, d, 64);
        if (lane >= d) hom_compose(t, lo, hi, t1, lo1, hi1);
    }
}

__global__ void __launch_bounds__(64) hom_seg_count(const uint32_t *__restrict__ cols, const HomIv *__restrict__ ivs, uint32_t n_ivs, int N, uint32_t *__restrict__ cnt)
{
    const int lane = threadIdx.x;
    // which interval: the segment rows are consecutive per interval
    uint32_t lo = 0, hi = n_ivs;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (ivs[mid].seg0 <= blockIdx.x) lo = mid; else hi = mid; }
    const HomIv iv = ivs[lo];
    const uint32_t seg = blockIdx.x - iv.seg0;
    const int64_t c0 = iv.col0 + (int64_t)seg * HOM_SEG, n = min((int64_t)HOM_SEG, iv.ncols - (int64_t)seg * HOM_SEG);
    uint32_t mine = 0;
    for (int ch = 0; ch * 64 < n; ch++) {
        const int64_t c = (int64_t)ch * 64 + lane;
        const uint32_t v = c < n ? cols[c0 + c] : 0u;
        mine = wave_genome_counts(v, N, lane, mine);
    }
    if (lane < N) cnt[(size_t)blockIdx.x * N + lane] = mine;
}

__global__ void __launch_bounds__(64) hom_fn(const uint32_t *__restrict__ cols, const HomItem *__restrict__ items, uint32_t n_items, const HomIv *__restrict__ ivs,
                                             const int64_t *__restrict__ left, const int64_t *__restrict__ right, const int8_t *__restrict__ rev, int N,
                                             const uint64_t *__restrict__ genomes, HomGenomes gw, HomScores sc, const int64_t *__restrict__ rank0, HomFn *__restrict__ fn)
{
    const int lane = threadIdx.x;
    for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const HomItem item = items[it];
        HomPair P = hom_setup(item, ivs[item.ivx], left, right, rev, N, genomes, gw, rank0);
        int32_t ft = 0, flo = HOM_MINF, fhi = HOM_PINF;          // the segment so far
        for (int ch = 0; (int64_t)ch * 64 < P.n; ch++) {
            int32_t t, lo, hi; bool none, both;
            hom_column(P, cols, ch, lane, sc, t, lo, hi, none, both);
            hom_scan(lane, t, lo, hi);
            int32_t ct = __shfl(t, 63, 64), clo = __shfl(lo, 63, 64), chi = __shfl(hi, 63, 64);        // the step as a whole ...
            hom_compose(ct, clo, chi, ft, flo, fhi);                                                  // ... after the segment so far
            ft = ct; flo = clo; fhi = chi;
        }
        if (lane == 0) fn[it] = HomFn{ft, flo, fhi, 0};
    }
}

__global__ void __launch_bounds__(64) hom_pred(const uint32_t *__restrict__ cols, const HomItem *__restrict__ items, uint32_t n_items, const HomIv *__restrict__ ivs,
                                               const int64_t *__restrict__ left, const int64_t *__restrict__ right, const int8_t *__restrict__ rev, int N,
                                               const uint64_t *__restrict__ genomes, HomGenomes gw, HomScores sc, const int64_t *__restrict__ rank0,
                                               const int32_t *__restrict__ xin, uint64_t *__restrict__ pred, uint8_t *__restrict__ stepmap, uint8_t *__restrict__ segmap)
{
    const int lane = threadIdx.x;
    for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const HomItem item = items[it];
        HomPair P = hom_setup(item, ivs[item.ivx], left, right, rev, N, genomes, gw, rank0);
        int32_t x = xin[it];
        uint32_t my_step = 2u;                                  // lane k keeps the map of step k (identity = 0b10)
        for (int ch = 0; (int64_t)ch * 64 < P.n; ch++) {
            int32_t t, lo, hi; bool none, both;
            hom_column(P, cols, ch, lane, sc, t, lo, hi, none, both);
            hom_scan(lane, t, lo, hi);
            const int32_t after = hom_clamp(x + t, lo, hi);     // x behind this lane's column
            int32_t before = __shfl_up(after, 1, 64);
            if (lane == 0) before = x;
            const bool ph = none || before >= sc.go_h, pu = none || before <= -sc.go_u;
            const uint64_t PH = __ballot(ph), PU = __ballot(pu);
            if (lane == 0) { pred[((size_t)it * 64 + ch) * 2] = PH; pred[((size_t)it * 64 + ch) * 2 + 1] = PU; }
            // the way back through this step: m_c(state) = state ? ph : !pu; lanes compose m_l after ... wait: m_l o m_{l+1} o .. o m_63
            uint32_t mp = (ph ? 2u : 0u) | (pu ? 0u : 1u);
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_down(mp, d, 64); if (lane + d < 64) mp = hom_map_after(mp, o); }
            const uint32_t whole = __shfl(mp, 0, 64);           // state behind the step -> state behind the previous step
            if (lane == ch) my_step = whole;
            x = __shfl(after, 63, 64);
        }
        stepmap[(size_t)it * 64 + lane] = (uint8_t)my_step;
        uint32_t sm = my_step;                                  // segment: step 0 after step 1 after ... (state behind the segment -> behind the previous one)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_down(sm, d, 64); if (lane + d < 64) sm = hom_map_after(sm, o); }
        if (lane == 0) segmap[it] = (uint8_t)sm;
    }
}

__global__ void __launch_bounds__(64) hom_keep(const uint32_t *__restrict__ cols, const HomItem *__restrict__ items, uint32_t n_items, const HomIv *__restrict__ ivs,
                                               const uint64_t *__restrict__ pred, const uint8_t *__restrict__ stepmap, const uint8_t *__restrict__ send,
                                               uint32_t *__restrict__ keep)
{
    const int lane = threadIdx.x;
    for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const HomItem item = items[it];
        const HomIv iv = ivs[item.ivx];
        const int64_t c0 = iv.col0 + (int64_t)item.seg * HOM_SEG, n = min((int64_t)HOM_SEG, iv.ncols - (int64_t)item.seg * HOM_SEG);
        // state behind every step: lane k = behind step k, from the state behind the segment and the maps of the steps after k
        uint32_t sm = stepmap[(size_t)it * 64 + lane];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_down(sm, d, 64); if (lane + d < 64) sm = hom_map_after(sm, o); }
        const uint32_t e = send[it];                            // state behind the segment
        const uint32_t nxt = __shfl_down(sm, 1, 64);            // steps k+1 .. 63 as one map
        const uint32_t behind = lane == 63 ? e : ((nxt >> e) & 1u);
        for (int ch = 0; (int64_t)ch * 64 < n; ch++) {
            const int64_t c = (int64_t)ch * 64 + lane;
            const uint32_t m = c < n ? cols[c0 + c] : 0u;
            const uint64_t PH = pred[((size_t)it * 64 + ch) * 2], PU = pred[((size_t)it * 64 + ch) * 2 + 1];
            const uint32_t eb = __shfl(behind, ch, 64);         // state of the step's last column... behind the step = state AT its last column
            uint32_t mp = ((PH >> lane & 1ull) ? 2u : 0u) | ((PU >> lane & 1ull) ? 0u : 1u);
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_down(mp, d, 64); if (lane + d < 64) mp = hom_map_after(mp, o); }
            const uint32_t nx = __shfl_down(mp, 1, 64);         // columns l+1 .. 63 as one map: state at column 63 -> state at column l
            const uint32_t st = lane == 63 ? eb : ((nx >> eb) & 1u);
            if (st && (m >> item.a & 1u) && (m >> item.b & 1u)) atomicOr(&keep[c0 + c], 1u << item.a | 1u << item.b);
        }
    }
}

// columns a column becomes: the genomes that stay (one column, if any) + one column per genome that leaves
__device__ __forceinline__ uint32_t hom_out_count(uint32_t m, uint32_t k) { return (k ? 1u : 0u) + (uint32_t)__popc(m & ~k); }

__global__ void __launch_bounds__(256) hom_count(const uint32_t *__restrict__ cols, const uint32_t *__restrict__ keep, int64_t n, uint32_t *__restrict__ tile_out,
                                                 unsigned long long *__restrict__ moved)
{
    __shared__ uint32_t acc[2];
    if (threadIdx.x < 2) acc[threadIdx.x] = 0;
    __syncthreads();
    const int64_t t0 = (int64_t)blockIdx.x * BB_CHUNK;
    uint32_t mine = 0, mv = 0;
    for (int k = 0; k < BB_CHUNK / 256; k++) {
        const int64_t c = t0 + k * 256 + threadIdx.x;
        if (c >= n) break;
        const uint32_t m = cols[c], kp = keep[c] & m;
        mine += hom_out_count(m, kp);
        if (m & (m - 1)) mv += (uint32_t)__popc(m & ~kp);
    }
    atomicAdd(&acc[0], mine); atomicAdd(&acc[1], mv);
    __syncthreads();
    if (threadIdx.x == 0) { tile_out[blockIdx.x] = acc[0]; if (acc[1]) atomicAdd(moved, (unsigned long long)acc[1]); }
}

__global__ void __launch_bounds__(256) hom_write(const uint32_t *__restrict__ cols, const uint32_t *__restrict__ keep, int64_t n, const int64_t *__restrict__ tile_base,
                                                 uint32_t *__restrict__ out)
{
    __shared__ uint32_t wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t base = tile_base[blockIdx.x];
    const int64_t t0 = (int64_t)blockIdx.x * BB_CHUNK;
    for (int k = 0; k < BB_CHUNK / 256; k++) {                // 256 columns per round, in column order
        const int64_t c = t0 + k * 256 + threadIdx.x;
        const uint32_t m = c < n ? cols[c] : 0u, kp = c < n ? keep[c] & m : 0u;
        const uint32_t cnt = c < n ? hom_out_count(m, kp) : 0u;
        uint32_t x = cnt;                                     // inclusive scan over the wave, then over the four waves
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int w = 0; w < 4; w++) { if (w < wave) before += wsum[w]; total += wsum[w]; }
        int64_t o = base + before + x - cnt;
        if (kp) out[o++] = kp;
        for (uint32_t r = m & ~kp; r; r &= r - 1) out[o++] = r & (0u - r);
        base += total;
        __syncthreads();
    }
}

// new offset of every interval start: the tile's base + the columns the tile puts out before it
__global__ void __launch_bounds__(64) hom_offsets(const uint32_t *__restrict__ cols, const uint32_t *__restrict__ keep, int64_t n, const int64_t *__restrict__ tile_base,
                                                  const int64_t *__restrict__ col_off, int64_t n_off, int64_t *__restrict__ out)
{
    const int lane = threadIdx.x;
    (void)n;
    for (int64_t q = blockIdx.x; q < n_off; q += gridDim.x) {
        const int64_t x = col_off[q], t0 = x & ~(int64_t)(BB_CHUNK - 1);
        uint32_t mine = 0;
        for (int64_t c = t0 + lane; c < x; c += 64) { const uint32_t m = cols[c]; mine += hom_out_count(m, keep[c] & m); }
#pragma unroll
        for (int d = 32; d; d >>= 1) mine += __shfl_xor(mine, d, 64);
        if (lane == 0) out[q] = tile_base[x / BB_CHUNK] + mine;          // (tile_base has one entry behind the last tile: x == n on a tile boundary)
    }
}

}  // namespace

extern "C" void mauve_hmm_params_from(double identity, double pgh, double pgu, mauve_hmm_params *h)
{
    if (!h) return;
    if (!(identity > 0.25 && identity < 1.0) || !(pgh > 0.0 && pgh <= 1.0) || !(pgu > 0.0 && pgu <= 1.0)) {
        h->match = h->mismatch = h->gap = 0; h->go_homologous = h->go_unrelated = 1;
        return;
    }
    h->match = (int32_t)lround(1000.0 * log(identity / 0.25));
    h->mismatch = (int32_t)lround(1000.0 * log((1.0 - identity) / 0.75));
    h->gap = -500;
    h->go_homologous = (int32_t)lround(1000.0 * log(pgh));
    h->go_unrelated = (int32_t)lround(1000.0 * log(pgu));
}

namespace {

// the parts of the pass's work area (bb_work), laid out by homology_core
struct HomArea {
    HomIv *ivs; HomItem *items; int64_t *left, *right; int8_t *rev; int64_t *off, *noff; uint32_t *tile; int64_t *base; unsigned long long *moved; uint32_t *keep, *scnt;
    int64_t *rank; HomFn *fn; int32_t *xin; uint8_t *smap, *send, *step; uint64_t *pred;
};

// the Viterbi paths of all (interval, pair)s: keep[column] gets the genomes that are homologous to another one there
int hom_paths(mauve_ctx *c, const AlnView &A, const HomWork &W, const mauve_hmm_params *h, const HomArea &L)
{
    const int N = A.N; const uint32_t n_items = (uint32_t)W.items.size(), grid = std::min<uint32_t>(n_items, 256 * 64);
    HomGenomes gw; memset(&gw, 0, sizeof gw);
    for (int g = 0; g < c->nseq; g++) gw.word_off[g] = c->word_off[(size_t)g];
    const HomScores sc{h->match, h->mismatch, h->gap, h->go_homologous, h->go_unrelated};
    const uint64_t *genomes = c->genomes.as<uint64_t>();
    // residues per segment -> base positions at the segment starts
    hipLaunchKernelGGL(hom_seg_count, dim3(W.n_segs), dim3(64), 0, c->stream, A.d_cols, L.ivs, (uint32_t)W.ivs.size(), N, L.scnt);
    HIPCHK(c, hipGetLastError());
    std::vector<uint32_t> scnt((size_t)W.n_segs * N); std::vector<int64_t> rank0(scnt.size());
    HIPCHK(c, hipMemcpyAsync(scnt.data(), L.scnt, scnt.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (const HomIv &iv : W.ivs)
        for (int g = 0; g < N; g++) { int64_t run = 0; for (uint32_t k = 0; k < iv.nseg; k++) { rank0[(size_t)(iv.seg0 + k) * N + g] = run; run += scnt[(size_t)(iv.seg0 + k) * N + g]; } }
    HIPCHK(c, hipMemcpyAsync(L.rank, rank0.data(), rank0.size() * 8, hipMemcpyHostToDevice, c->stream));
    // forwards: every segment's function, chained on the host
    hipLaunchKernelGGL(hom_fn, dim3(grid), dim3(64), 0, c->stream, A.d_cols, L.items, n_items, L.ivs, L.left, L.right, L.rev, N, genomes, gw, sc, L.rank, L.fn);
    HIPCHK(c, hipGetLastError());
    std::vector<HomFn> fn(n_items); std::vector<int32_t> xin; std::vector<uint8_t> fin;
    HIPCHK(c, hipMemcpyAsync(fn.data(), L.fn, n_items * sizeof(HomFn), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hom_chain_forward(W.runs, fn, h->go_homologous, xin, fin);
    HIPCHK(c, hipMemcpyAsync(L.xin, xin.data(), (size_t)n_items * 4, hipMemcpyHostToDevice, c->stream));
    // backwards: every segment's map, chained on the host
    hipLaunchKernelGGL(hom_pred, dim3(grid), dim3(64), 0, c->stream, A.d_cols, L.items, n_items, L.ivs, L.left, L.right, L.rev, N, genomes, gw, sc, L.rank, L.xin, L.pred, L.step, L.smap);
    HIPCHK(c, hipGetLastError());
    std::vector<uint8_t> smap(n_items), send;
    HIPCHK(c, hipMemcpyAsync(smap.data(), L.smap, n_items, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hom_chain_backward(W.runs, smap, fin, send);
    HIPCHK(c, hipMemcpyAsync(L.send, send.data(), n_items, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(hom_keep, dim3(grid), dim3(64), 0, c->stream, A.d_cols, L.items, n_items, L.ivs, L.pred, L.step, L.send, L.keep);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));             // (send / xin are host vectors)
    return MAUVE_OK;
}

// the columns split by keep into c->hom_cols, unless nothing moves: *moved_out residues, *n_new_out columns, their offsets in noff
int hom_resplit(mauve_ctx *c, const AlnView &A, int64_t residues, size_t n_tiles, const HomArea &L, std::vector<int64_t> &noff, int64_t *n_new_out, int64_t *moved_out)
{
    const int64_t n_off = A.n_iv + 1, n_cols = A.col_off[A.n_iv];
    hipLaunchKernelGGL(hom_count, dim3((uint32_t)n_tiles), dim3(256), 0, c->stream, A.d_cols, L.keep, n_cols, L.tile, L.moved);
    HIPCHK(c, hipGetLastError());
    std::vector<uint32_t> tile_out(n_tiles); unsigned long long moved = 0;
    HIPCHK(c, hipMemcpyAsync(tile_out.data(), L.tile, n_tiles * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&moved, L.moved, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *moved_out = (int64_t)moved;
    if (moved == 0) return MAUVE_OK;                          // every residue stays where it is
    std::vector<int64_t> tile_base(n_tiles + 1, 0);
    for (size_t t = 0; t < n_tiles; t++) tile_base[t + 1] = tile_base[t] + tile_out[t];
    const int64_t n_new = tile_base[n_tiles];
    if (n_new > residues) { c->err = "apply_homology: more columns than residues"; return MAUVE_ERR_STATE; }
    HIPCHK(c, c->hom_cols.ensure(((size_t)n_new + 64) * 4));
    HIPCHK(c, hipMemcpyAsync(L.base, tile_base.data(), (n_tiles + 1) * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(hom_write, dim3((uint32_t)n_tiles), dim3(256), 0, c->stream, A.d_cols, L.keep, n_cols, L.base, c->hom_cols.as<uint32_t>());
    hipLaunchKernelGGL(hom_offsets, dim3((uint32_t)std::min<int64_t>(n_off, 4096)), dim3(64), 0, c->stream, A.d_cols, L.keep, n_cols, L.base, L.off, n_off, L.noff);
    HIPCHK(c, hipGetLastError());
    noff.resize((size_t)n_off);
    HIPCHK(c, hipMemcpyAsync(noff.data(), L.noff, (size_t)n_off * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (noff[0] != 0 || noff[(size_t)A.n_iv] != n_new) { c->err = "apply_homology: column offsets do not add up"; return MAUVE_ERR_STATE; }
    *n_new_out = n_new;
    return MAUVE_OK;
}

// the work behind mauve_apply_homology / mauve_apply_homology_alignment: the re-split columns are left in c->hom_cols (*n_new_out of
// them, offsets in noff) unless nothing moved
int homology_core(mauve_ctx *c, const AlnView &A, const mauve_hmm_params *h, std::vector<int64_t> &noff, int64_t *n_new_out, int64_t *moved_out)
{
    const int N = A.N; const int64_t n_iv = A.n_iv, n_cols = A.col_off[n_iv];
    *moved_out = 0; *n_new_out = n_cols;
    if (h->go_homologous > 0 || h->go_unrelated > 0) { c->err = "apply_homology: transition scores are log probabilities (<= 0)"; return MAUVE_ERR_ARG; }
    if (N != c->nseq) { c->err = "apply_homology: the alignment does not belong to the genomes of this context"; return MAUVE_ERR_STATE; }
    if (n_cols == 0) return MAUVE_OK;
    if (std::abs((int64_t)h->match) > 65536 || std::abs((int64_t)h->mismatch) > 65536 || std::abs((int64_t)h->gap) > 65536 || h->go_homologous < -(1 << 28) || h->go_unrelated < -(1 << 28)) {
        c->err = "apply_homology: scores beyond +-65536 (transitions beyond -2^28) are not supported"; return MAUVE_ERR_ARG;
    }
    HomWork W; const char *why = nullptr;
    if (const int rc = hom_work_items(N, n_iv, A.left, A.right, A.col_off, c->lens.data(), W, &why)) { c->err = why; return rc; }
    const size_t n_items = W.items.size(), n_tiles = (size_t)((n_cols + BB_CHUNK - 1) / BB_CHUNK), n_ivg = (size_t)n_iv * N, n_off = (size_t)n_iv + 1, n_seg = (size_t)W.n_segs * N;
    // work area: work items | interval table | column offsets, old and new | columns every tile puts out, their prefix | residues moved | per column the genomes that stay |
    // per segment every genome's residues in it and in front of it | per item its function, x at its start, backward map, end state, step maps, predecessor words
    const size_t o_items = up64(W.ivs.size() * sizeof(HomIv)), o_left = o_items + up64(n_items * sizeof(HomItem)), o_right = o_left + up64(n_ivg * 8), o_rev = o_right + up64(n_ivg * 8),
                 o_off = o_rev + up64(n_ivg), o_noff = o_off + up64(n_off * 8), o_tile = o_noff + up64(n_off * 8), o_base = o_tile + up64(n_tiles * 4), o_moved = o_base + up64((n_tiles + 1) * 8),
                 o_keep = o_moved + 64, o_scnt = o_keep + up64((size_t)n_cols * 4), o_rank = o_scnt + up64(n_seg * 4), o_fn = o_rank + up64(n_seg * 8), o_xin = o_fn + up64(n_items * sizeof(HomFn)),
                 o_smap = o_xin + up64(n_items * 4), o_send = o_smap + up64(n_items), o_step = o_send + up64(n_items), o_pred = o_step + up64(n_items * 64), total = o_pred + n_items * 64 * 16 + 64;
    HIPCHK(c, c->bb_work.ensure(total));
    char *wk = c->bb_work.as<char>();
    auto at = [wk](size_t o) { return static_cast<void *>(wk + o); };
    const HomArea L{(HomIv *)at(0), (HomItem *)at(o_items), (int64_t *)at(o_left), (int64_t *)at(o_right), (int8_t *)at(o_rev), (int64_t *)at(o_off), (int64_t *)at(o_noff), (uint32_t *)at(o_tile),
                    (int64_t *)at(o_base), (unsigned long long *)at(o_moved), (uint32_t *)at(o_keep), (uint32_t *)at(o_scnt), (int64_t *)at(o_rank), (HomFn *)at(o_fn), (int32_t *)at(o_xin),
                    (uint8_t *)at(o_smap), (uint8_t *)at(o_send), (uint8_t *)at(o_step), (uint64_t *)at(o_pred)};
    HIPCHK(c, hipMemcpyAsync(L.ivs, W.ivs.data(), W.ivs.size() * sizeof(HomIv), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(L.items, W.items.data(), n_items * sizeof(HomItem), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(L.left, A.left, n_ivg * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(L.right, A.right, n_ivg * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(L.rev, A.reverse, n_ivg, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(L.off, A.col_off, n_off * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(L.moved, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(L.keep, 0, (size_t)n_cols * 4, c->stream));
    if (n_items) if (const int rc = hom_paths(c, A, W, h, L)) return rc;
    return hom_resplit(c, A, W.residues, n_tiles, L, noff, n_new_out, moved_out);
}

}  // namespace

extern "C" {

int mauve_apply_homology(mauve_ctx *c, const mauve_hmm_params *h, mauve_align_sizes *sizes, int64_t *n_moved)
{
    if (!c || !h) return MAUVE_ERR_ARG;
    AlignResult &R = c->res;
    AlnView A;       // refused, too, when the genomes were replaced under a host-side result: the pass reads bases; the columns go back to where the assembly stage keeps them
    if (const int rc = aln_from_context(c, "apply_homology", true, c->res_cols, &A)) return rc;
    if (n_moved) *n_moved = 0;
    if (sizes) *sizes = R.sz;
    if (A.n_iv == 0) return MAUVE_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));               // an upload from the result's host memory is not left queued behind a refusal
    std::vector<int64_t> noff; int64_t n_new = 0, moved = 0;
    if (const int rc = homology_core(c, A, h, noff, &n_new, &moved)) return rc;
    if (n_moved) *n_moved = moved;
    if (moved == 0) return MAUVE_OK;
    // the new columns are the result's columns from here on, resident like a device-assembled result
    std::swap(c->res_cols, c->hom_cols);
    R.col_off.swap(noff);
    R.n_cols = (size_t)n_new; R.sz.n_cols = n_new;
    R.cols_pending = true; R.cols_ext = nullptr; R.cols_fill = 0; R.cols_dirty.clear();
    c->bb = BackboneResult();                                  // a backbone of the old columns no longer applies
    if (sizes) *sizes = R.sz;
    return MAUVE_OK;
}

int mauve_apply_homology_alignment(mauve_ctx *c, int nseq, int64_t n_iv, const int64_t *left, const int64_t *right, const int8_t *reverse, const int64_t *col_off,
                                   const uint32_t *cols, const mauve_hmm_params *h, int64_t *col_off_out, uint32_t *cols_out, int64_t *n_moved)
{
    if (!c || !h || nseq < 1 || nseq > MAUVE_MAX_SEQ || n_iv < 0 || !col_off_out || (n_iv && (!left || !right || !reverse || !col_off || !cols || !cols_out))) return MAUVE_ERR_ARG;
    { const int rg = refuse_past_2g(c, "apply_homology_alignment"); if (rg) return rg; }
    if (n_moved) *n_moved = 0;
    col_off_out[0] = 0;
    if (n_iv == 0) return MAUVE_OK;
    // the order of the refusals: the offsets, then the genome count, then the columns (aln_from_arrays repeats the first on its way)
    if (const int rco = coord_check_offsets(c, "apply_homology", n_iv, col_off)) return rco;
    if (nseq != c->nseq) { c->err = "apply_homology: the alignment does not belong to the genomes of this context"; return MAUVE_ERR_STATE; }
    AlnView A;
    if (const int rc = aln_from_arrays(c, "apply_homology", nseq, n_iv, left, right, reverse, col_off, cols, &A)) return rc;
    const int64_t n_cols = col_off[n_iv];
    std::vector<int64_t> noff; int64_t n_new = 0, moved = 0;
    if (const int rc = homology_core(c, A, h, noff, &n_new, &moved)) return rc;
    if (n_moved) *n_moved = moved;
    if (moved == 0) { memcpy(col_off_out, col_off, ((size_t)n_iv + 1) * 8); if (n_cols) memcpy(cols_out, cols, (size_t)n_cols * 4); return MAUVE_OK; }
    memcpy(col_off_out, noff.data(), ((size_t)n_iv + 1) * 8);
    HIPCHK(c, hipMemcpy(cols_out, c->hom_cols.p, (size_t)n_new * 4, hipMemcpyDeviceToHost));
    return MAUVE_OK;
}

}  // extern "C"
