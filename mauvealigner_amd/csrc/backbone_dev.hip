// backbone_dev.hip -- backbone segments and pairwise islands of an alignment: the stage that stands in
// for libMems' detectBackbone(iv_list, bb_list, &BigGapsDetector(island_gap_size)) (progressiveMauve.cpp:242-243) and
// for simpleFindIslands (mauveAligner.cpp:844).  The alignment comes in as an AlnView (aln_view.hip): the interval table on the host,
// the column array in HBM (one uint32 presence mask per column); everything that touches columns runs on the device:
//   bb_chunk_last what the last pair-column of every (chunk, pair) is: the state in front of a chunk without walking back over columns
//   bb_pair_gaps  one wave (= one workgroup) per (4096-column chunk, genome pair): the pair's gap regions that start in the chunk are
//                 walked 64 columns at a time on wave ballots (all bookkeeping is wave-uniform, i.e. scalar), and the
//                 open regions and the islands are appended to a record list;
//   bb_tile_count per-genome residue counts of every 4096-column tile;  bb_rank  residue counts at query columns
//                 (a wave per query, inside one tile) -- sequence coordinates of the segment and island ends.
// The host only sweeps the region boundaries (10^3..10^4 records) into components and segments: backbone_run is the list of stages, its
// host steps are backbone_host.hpp's (bb_sort_records, bb_sweep, bb_query_slots, bb_tables).  Entry points: mauve_backbone,
// mauve_backbone_alignment, mauve_backbone_fetch.  The homology pass that precedes the stage (S12b) is homology_dev.hip.
#include "common.hpp"
#include "column_counts.hpp"
#include <algorithm>
#include <cstring>

namespace {

// does m hold a run of at least `need` consecutive ones?  (AND with itself shifted, doubling the length known so far)
__device__ __forceinline__ bool has_run(uint64_t m, int need)
{
    if (need > 64) return false;
    int have = 1;
    while (have < need && m) { const int sh = have < need - have ? have : need - have; m &= m >> sh; have += sh; }
    return m != 0;
}

// the k-th genome pair (a < b) among the genomes of gmask, in the order (g0,g1), (g0,g2), .., (g1,g2), ..
__device__ __forceinline__ void bb_pair_of(uint32_t gmask, uint32_t p, int *a, int *b)
{
    int g[32], n = 0;
    for (int x = 0; x < 32; x++) if (gmask >> x & 1) g[n++] = x;
    int x = 0;
    while (p >= (uint32_t)(n - 1 - x)) { p -= (uint32_t)(n - 1 - x); x++; }
    *a = g[x]; *b = g[x + 1 + (int)p];
}

// what the last pair-column of every (chunk, pair) is: 0 none in the chunk, 1 both genomes, 2 one of them.  bb_pair_gaps finds the
// state in front of its chunk from these bytes, 64 chunks per step, instead of walking back over the columns themselves (a pair
// that is absent over a long stretch of an interval would make every chunk of the stretch walk back to its start)
__global__ void __launch_bounds__(64) bb_chunk_last(const uint32_t *__restrict__ cols, const BbIv *__restrict__ ivs, uint32_t n_ivs, uint32_t max_pairs, uint8_t *__restrict__ last)
{
    const int lane = threadIdx.x & 63;
    uint32_t lo = 0, hi = n_ivs;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) / 2; if (ivs[mid].chunk0 <= blockIdx.x) lo = mid; else hi = mid; }
    const BbIv d = ivs[lo];
    const int64_t nc = d.ncols, cs = (int64_t)(blockIdx.x - d.chunk0) * BB_CHUNK, ce = cs + BB_CHUNK < nc ? cs + BB_CHUNK : nc;
    const uint32_t *m = cols + d.col0;
    // one wave per chunk: the last column of every genome in the chunk (lane g keeps genome g's; the chunk's last 64 columns settle nearly
    // all of them, the rest walk further back), then a pair's last column is the later of its two genomes' -- both if they coincide
    int64_t lastpos = -1;
    uint32_t pending = d.gmask;
    for (int64_t w = (ce - 1) & ~(int64_t)63; w >= cs && pending; w -= 64) {
        const int64_t c = w + lane;
        const uint32_t v = c < ce ? m[c] : 0u;
        for (uint32_t mg = pending; mg; mg &= mg - 1) {
            const int g = __ffs(mg) - 1;
            const uint64_t B = __ballot(v >> g & 1u);
            if (B) { if (lane == g) lastpos = w + 63 - __clzll((long long)B); pending &= ~(1u << g); }
        }
    }
    uint32_t p = 0;
    for (uint32_t ma = d.gmask; ma; ma &= ma - 1)                // pairs in bb_pair_of's order: (g0,g1), (g0,g2), .., (g1,g2), ..
        for (uint32_t mb = ma & (ma - 1); mb; mb &= mb - 1, p++) {
            const int64_t la = __shfl(lastpos, __ffs(ma) - 1, 64), lb = __shfl(lastpos, __ffs(mb) - 1, 64);
            if (lane == 0) last[(size_t)blockIdx.x * max_pairs + p] = (la < 0 && lb < 0) ? 0 : (la == lb ? 1 : 2);
        }
}

__global__ void __launch_bounds__(64) bb_pair_gaps(const uint32_t *__restrict__ cols, const BbIv *__restrict__ ivs, uint32_t n_ivs, uint32_t island_gap,
                                                    BbRec *__restrict__ rec, uint32_t cap, uint32_t *__restrict__ count, const uint8_t *__restrict__ last, uint32_t max_pairs)
{
    const int lane = threadIdx.x & 63;
    // which interval this chunk belongs to
    uint32_t lo = 0, hi = n_ivs;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) / 2; if (ivs[mid].chunk0 <= blockIdx.x) lo = mid; else hi = mid; }
    const BbIv d = ivs[lo];
    const int64_t nc = d.ncols, cs = (int64_t)(blockIdx.x - d.chunk0) * BB_CHUNK, ce = cs + BB_CHUNK < nc ? cs + BB_CHUNK : nc;
    const uint32_t *m = cols + d.col0;
    for (uint32_t p = blockIdx.y; p < d.npairs; p += gridDim.y) {
        int a, b;
        bb_pair_of(d.gmask, p, &a, &b);
        // the nearest column before the chunk that holds a residue of the pair: a both-column (or none) means a region that
        // starts with the chunk's first column is this chunk's to report; a one-sided column means it began earlier
        bool seen_both = false, skipping = false;
        if (!last) {                                     // A/B (MAUVE_BB_COLUMN_SCAN): walk back over the columns themselves
            for (int64_t w = cs - 64; w > -64; w -= 64) {
                const int64_t c = w + lane;
                const uint32_t v = c >= 0 ? m[c] : 0u;
                const bool ra = v >> a & 1, rb = v >> b & 1;
                const uint64_t any = __ballot(ra || rb), both = __ballot(ra && rb);
                if (any) { const int top = 63 - __clzll((long long)any); if (both >> top & 1) seen_both = true; else skipping = true; break; }
            }
        } else
        for (int64_t k0 = (int64_t)blockIdx.x - 1; k0 >= (int64_t)d.chunk0; k0 -= 64) {       // the chunks in front of this one, nearest first, 64 per step
            const int64_t k = k0 - lane;
            const uint32_t stv = k >= (int64_t)d.chunk0 ? last[(size_t)k * max_pairs + p] : 0u;
            const uint64_t any = __ballot(stv != 0);
            if (any) { const int near = __ffsll((long long)any) - 1; if (__shfl((int)stv, near, 64) == 1) seen_both = true; else skipping = true; break; }
        }
        bool in_region = false, leading = false, has_island = false, done = false;
        int run_t = 0;                                   // 1: only a has residues, 2: only b
        int64_t first = 0, last = 0, run_first = 0, run_last = 0, run_n = 0;
        auto emit = [&](uint32_t kind, uint32_t who, int64_t c0, int64_t c1) {
            if (lane == 0) {
                const uint32_t k = atomicAdd(count, 1u);
                if (k < cap) rec[k] = BbRec{d.iv, (uint32_t)a | (uint32_t)b << 8 | who << 16 | kind << 24, (uint32_t)c0, (uint32_t)c1};
            }
        };
        auto close_run = [&]() {
            if (run_n > (int64_t)island_gap) { has_island = true; emit(1u, (uint32_t)(run_t == 1 ? a : b), run_first, run_last); }
        };
        // four words (256 columns) are fetched at a time, one batch ahead; the walk itself stays word by word
        uint32_t nx[4];                                          // the next four words are on their way while these four are walked
#pragma unroll
        for (int k = 0; k < 4; k++) { const int64_t c = cs + 64 * k + lane; nx[k] = c < nc ? m[c] : 0u; }
        for (int64_t w0 = cs; w0 < nc && !done && (w0 < ce || in_region); w0 += 256) {
          uint32_t vv[4];
#pragma unroll
          for (int k = 0; k < 4; k++) { vv[k] = nx[k]; const int64_t c = w0 + 256 + 64 * k + lane; nx[k] = c < nc ? m[c] : 0u; }
          if (!in_region && !skipping) {                         // the common batch: 256 columns without a one-sided one, no region open
              bool one = false, both = false;
#pragma unroll
              for (int k = 0; k < 4; k++) { const bool ra = vv[k] >> a & 1, rb = vv[k] >> b & 1; one |= ra != rb; both |= ra && rb; }
              if (!__ballot(one)) { if (__ballot(both)) seen_both = true; continue; }
          }
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const int64_t w = w0 + 64 * k;
            if (!(w < nc && !done && (w < ce || in_region))) break;
            const uint32_t v = vv[k];
            const bool ra = v >> a & 1, rb = v >> b & 1;
            const uint64_t mOne = __ballot(ra != rb);
            if (!mOne && !in_region && !skipping) {              // the common word: nothing one-sided in it and no region open
                if (__ballot(ra && rb)) seen_both = true;
                continue;
            }
            const uint64_t mA = __ballot(ra && !rb), mB = mOne & ~mA, mBoth = __ballot(ra && rb);
            if (!in_region && !skipping) {
                // the usual gapped word: every column holds a base of the pair, the gaps open after a both-column and close
                // before the word's last column, and none of them is an island -- nothing to report, nothing carried over
                const uint64_t valid = __ballot(w + lane < nc);
                const int top = 63 - __clzll((long long)valid);
                if ((mA | mB | mBoth) == valid && (mBoth >> top & 1) && (seen_both || (mBoth & 1)) &&
                    !has_run(mA, (int)island_gap + 1) && !has_run(mB, (int)island_gap + 1)) { seen_both = true; continue; }
            }
            int pos = 0;
            while (pos < 64) {
                if (skipping) {
                    const uint64_t r = mBoth & ~below(pos);
                    if (!r) break;
                    skipping = false; seen_both = true; pos = __ffsll((long long)r);       // the column after the both-column
                    continue;
                }
                if (!in_region) {
                    const uint64_t r = (mA | mB) & ~below(pos);
                    if (!r) { if (mBoth & ~below(pos)) seen_both = true; break; }
                    const int s = __ffsll((long long)r) - 1;
                    if (mBoth & ~below(pos) & below(s)) seen_both = true;
                    if (w + s >= ce) { done = true; break; }             // starts in the next chunk
                    in_region = true; leading = !seen_both; has_island = false;
                    first = last = run_first = run_last = w + s; run_n = 0; run_t = (mA >> s & 1) ? 1 : 2;
                    pos = s;
                }
                // inside a region: one-sided columns up to the next both-column
                const uint64_t rb2 = mBoth & ~below(pos);
                const int q = rb2 ? __ffsll((long long)rb2) - 1 : 64;
                const uint64_t range = below(q) & ~below(pos);
                uint64_t ba = mA & range, bbits = mB & range;
                while (ba | bbits) {
                    const uint64_t same = run_t == 1 ? ba : bbits, other = run_t == 1 ? bbits : ba;
                    const int e = other ? __ffsll((long long)other) - 1 : 64;
                    const uint64_t take = same & below(e);
                    if (take) { run_n += __popcll(take); run_last = w + 63 - __clzll((long long)take); last = run_last; }
                    ba &= ~below(e); bbits &= ~below(e);
                    if (other) { close_run(); run_t = 3 - run_t; run_first = w + e; run_n = 0; }
                }
                if (q < 64) {                                            // the region ends before a both-column
                    close_run();
                    if (has_island || leading) emit(0u, 0u, first, last);
                    in_region = false; seen_both = true; pos = q + 1;
                    if (w + q >= ce) { done = true; break; }
                } else break;
            }
          }
        }
        if (in_region) { close_run(); emit(0u, 0u, first, last); }       // ran into the end of the interval
    }
}

// residues of every genome in every 4096-column tile of the whole column array
__global__ void __launch_bounds__(256) bb_tile_count(const uint32_t *__restrict__ cols, int64_t n, int N, uint32_t *__restrict__ tile_cnt)
{
    __shared__ uint32_t acc[32];
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 32) acc[threadIdx.x] = 0;
    __syncthreads();
    const int64_t t0 = (int64_t)blockIdx.x * BB_CHUNK;
    uint32_t mine = 0;
    for (int k = 0; k < BB_CHUNK / 256; k++) {
        const int64_t c = t0 + k * 256 + threadIdx.x;
        const uint32_t v = c < n ? cols[c] : 0u;
        mine = wave_genome_counts(v, N, lane, mine);
    }
    if (lane < N) atomicAdd(&acc[lane], mine);
    __syncthreads();
    if ((int)threadIdx.x < N) tile_cnt[(size_t)blockIdx.x * N + threadIdx.x] = acc[threadIdx.x];
}

// residues of every genome in [tile start of x, x) for every query column x: the tile's 64 words are split over the four
// waves of the workgroup, four words in flight per lane
__global__ void __launch_bounds__(256) bb_rank(const uint32_t *__restrict__ cols, const int64_t *__restrict__ query, int N, uint32_t *__restrict__ out)
{
    __shared__ uint32_t acc[32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 32) acc[threadIdx.x] = 0;
    __syncthreads();
    const int64_t x = query[blockIdx.x], t0 = (x & ~(int64_t)(BB_CHUNK - 1)) + (int64_t)wave * (BB_CHUNK / 4);
    uint32_t mine = 0;
    for (int64_t w = t0; w < x && w < t0 + BB_CHUNK / 4; w += 256) {
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) { const int64_t c = w + 64 * k + lane; v[k] = c < x ? cols[c] : 0u; }
#pragma unroll
        for (int k = 0; k < 4; k++) mine = wave_genome_counts(v[k], N, lane, mine);
    }
    if (lane < N && mine) atomicAdd(&acc[lane], mine);
    __syncthreads();
    if ((int)threadIdx.x < N) out[(size_t)blockIdx.x * N + threadIdx.x] = acc[threadIdx.x];
}

}  // namespace

namespace {

// The kernels over the columns: the record list of all (chunk, pair)s -- the launch is repeated with room when the list did not fit --
// and, the first time round, every tile's residue counts
int bb_collect(mauve_ctx *c, const AlnView &A, const std::vector<BbIv> &ivs, uint32_t chunks, uint32_t max_pairs, uint32_t island_gap, std::vector<BbRec> &recs,
               std::vector<uint32_t> &tile_cnt)
{
    const int N = A.N; const int64_t n_cols = A.col_off[A.n_iv];
    const size_t n_tiles = (size_t)((n_cols + BB_CHUNK - 1) / BB_CHUNK);
    // work area: interval table | counter | tile counts | the chunks' last pair-columns | records
    const size_t o_cnt = up64(ivs.size() * sizeof(BbIv)), o_tile = o_cnt + 64, o_last = o_tile + up64(n_tiles * (size_t)N * 4), o_rec = o_last + up64((size_t)chunks * max_pairs);
    size_t cap = std::max<size_t>(1u << 16, c->bb_rec_cap);
    tile_cnt.resize(n_tiles * (size_t)N);
    for (int attempt = 0;; attempt++) {
        HIPCHK(c, c->bb_work.ensure(o_rec + cap * sizeof(BbRec)));
        char *wk = c->bb_work.as<char>();                             // (every attempt: a grown work area is a new allocation)
        struct { BbIv *ivs; uint32_t *count, *tiles; uint8_t *last; BbRec *rec; } a{(BbIv *)wk, (uint32_t *)(wk + o_cnt), (uint32_t *)(wk + o_tile), (uint8_t *)(wk + o_last), (BbRec *)(wk + o_rec)};
        HIPCHK(c, hipMemcpyAsync(a.ivs, ivs.data(), ivs.size() * sizeof(BbIv), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(a.count, 0, 64, c->stream));
        const uint32_t gy = std::min<uint32_t>(max_pairs, 64);        // one wave per (chunk, pair): with few pairs, too, every resident wave works
        const bool column_scan = switches().bb_column_scan;
        if (!column_scan) hipLaunchKernelGGL(bb_chunk_last, dim3(chunks), dim3(64), 0, c->stream, A.d_cols, a.ivs, (uint32_t)ivs.size(), max_pairs, a.last);
        hipLaunchKernelGGL(bb_pair_gaps, dim3(chunks, gy), dim3(64), 0, c->stream, A.d_cols, a.ivs, (uint32_t)ivs.size(), island_gap, a.rec, (uint32_t)cap, a.count,
                           column_scan ? (const uint8_t *)nullptr : a.last, max_pairs);
        if (attempt == 0) hipLaunchKernelGGL(bb_tile_count, dim3((uint32_t)n_tiles), dim3(256), 0, c->stream, A.d_cols, n_cols, N, a.tiles);
        HIPCHK(c, hipGetLastError());
        uint32_t n_rec = 0;
        HIPCHK(c, hipMemcpyAsync(&n_rec, a.count, 4, hipMemcpyDeviceToHost, c->stream));
        if (attempt == 0) HIPCHK(c, hipMemcpyAsync(tile_cnt.data(), a.tiles, tile_cnt.size() * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (n_rec > cap) { cap = (size_t)n_rec + 1024; c->bb_rec_cap = cap; continue; }    // the list did not fit: once more with room
        recs.resize(n_rec);
        if (n_rec) HIPCHK(c, hipMemcpy(recs.data(), a.rec, (size_t)n_rec * sizeof(BbRec), hipMemcpyDeviceToHost));
        return MAUVE_OK;
    }
}

// residue counts of every genome between the tile start and each query column: *qcnt [qcol.size()][N], in page-locked memory
int bb_rank_queries(mauve_ctx *c, const AlnView &A, const std::vector<int64_t> &qcol, const uint32_t **qcnt)
{
    const int N = A.N;
    const size_t nq_all = qcol.size(), o_out = up64(nq_all * 8), n_out = nq_all * (size_t)N * 4;      // queries | counts
    HIPCHK(c, c->bb_query.ensure(o_out + n_out + 64));
    HIPCHK(c, c->pin_bb.ensure(o_out + n_out + 64));                // page-locked staging, same layout
    char *qb = c->bb_query.as<char>(), *hb = c->pin_bb.as<char>();
    memcpy(hb, qcol.data(), nq_all * 8);
    HIPCHK(c, hipMemcpyAsync(qb, hb, nq_all * 8, hipMemcpyHostToDevice, c->stream));
    for (size_t q0 = 0; q0 < nq_all; q0 += (size_t)1 << 22) {      // grid x block stays below 2^32 threads per launch
        const size_t nq = std::min<size_t>((size_t)1 << 22, nq_all - q0);
        hipLaunchKernelGGL(bb_rank, dim3((uint32_t)nq), dim3(256), 0, c->stream, A.d_cols, reinterpret_cast<const int64_t *>(qb) + q0, N, reinterpret_cast<uint32_t *>(qb + o_out) + q0 * (size_t)N);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hb + o_out, qb + o_out, n_out, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *qcnt = reinterpret_cast<const uint32_t *>(hb + o_out);
    return MAUVE_OK;
}

// The work behind mauve_backbone / mauve_backbone_alignment, stage by stage; the host steps are backbone_host.hpp's
int backbone_run(mauve_ctx *c, const AlnView &A, int64_t island_gap)
{
    BackboneResult &B = c->bb;
    B = BackboneResult(); B.N = A.N;
    if (island_gap < 0 || island_gap > 0x7fffffff) { c->err = "backbone: island_gap_size out of range"; return MAUVE_ERR_ARG; }
    std::vector<BbIv> ivs; uint32_t chunks = 0, max_pairs = 0;
    if (!bb_intervals(A.N, A.n_iv, A.left, A.col_off, ivs, &chunks, &max_pairs)) { c->err = "backbone: interval too long"; return MAUVE_ERR_LIMIT; }
    if (ivs.empty()) { B.valid = true; return MAUVE_OK; }
    const bool trace = switches().trace;
    const double tb0 = now_ms();
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<BbRec> recs, islands; std::vector<uint32_t> tile_cnt;
    if (const int rc = bb_collect(c, A, ivs, chunks, max_pairs, (uint32_t)island_gap, recs, tile_cnt)) return rc;
    const double tb1 = now_ms();
    if (trace) fprintf(stderr, "[trace] backbone: %u chunks, %zu records; kernels + copies %.3f ms\n", chunks, recs.size(), tb1 - tb0);
    std::vector<BbSeg> segs;
    bb_sort_records(recs);
    bb_sweep(ivs, recs, segs, islands);
    const double tb2 = now_ms();
    BbQueries Q; const uint32_t *qcnt = nullptr;
    bb_query_slots(ivs, segs, islands, (size_t)1 << 20, Q);
    if (const int rc = bb_rank_queries(c, A, Q.qcol, &qcnt)) return rc;
    const double tb3 = now_ms();
    if (trace) fprintf(stderr, "[trace] backbone: sort + sweep %.3f ms (%zu segments), %zu rank queries %.3f ms\n", tb2 - tb1, segs.size(), Q.qcol.size(), tb3 - tb2);
    bb_tables(A.N, ivs, segs, islands, Q, A.left, A.right, A.reverse, tile_cnt.data(), tile_cnt.size() / (size_t)A.N, qcnt, B);
    B.valid = true;
    if (trace) fprintf(stderr, "[trace] backbone: coordinates + tables %.3f ms\n", now_ms() - tb3);
    return MAUVE_OK;
}

}  // namespace

extern "C" {

int mauve_backbone(mauve_ctx *c, int64_t island_gap_size, int64_t *n_seg, int64_t *n_islands)
{
    if (!c || !n_seg || !n_islands) return MAUVE_ERR_ARG;
    if (island_gap_size < 0 || island_gap_size > 0x7fffffff) { c->err = "backbone: island_gap_size out of range"; return MAUVE_ERR_ARG; }
    AlnView A;       // the genomes are not read: a host-side result whose genomes were replaced is taken
    if (const int rc = aln_from_context(c, "backbone", false, c->bb_cols, &A)) return rc;
    if (A.n_iv == 0) { c->bb = BackboneResult(); c->bb.N = c->nseq; c->bb.valid = true; *n_seg = *n_islands = 0; return MAUVE_OK; }   // nothing was aligned
    if (const int rc = backbone_run(c, A, island_gap_size)) return rc;
    *n_seg = (int64_t)c->bb.seg_iv.size(); *n_islands = (int64_t)c->bb.islands.size() / 8;
    return MAUVE_OK;
}

int mauve_backbone_alignment(mauve_ctx *c, int nseq, int64_t n_iv, const int64_t *left, const int64_t *right, const int8_t *reverse,
                             const int64_t *col_off, const uint32_t *cols, int64_t island_gap_size, int64_t *n_seg, int64_t *n_islands)
{
    if (!c || !n_seg || !n_islands || nseq < 1 || nseq > MAUVE_MAX_SEQ || n_iv < 0 || (n_iv && (!left || !right || !reverse || !col_off || !cols))) return MAUVE_ERR_ARG;
    c->bb = BackboneResult(); c->bb.N = nseq;
    *n_seg = *n_islands = 0;
    if (n_iv == 0) { c->bb.valid = true; return MAUVE_OK; }
    AlnView A;
    if (const int rc = aln_from_arrays(c, "backbone", nseq, n_iv, left, right, reverse, col_off, cols, &A)) return rc;
    if (const int rc = backbone_run(c, A, island_gap_size)) return rc;
    *n_seg = (int64_t)c->bb.seg_iv.size(); *n_islands = (int64_t)c->bb.islands.size() / 8;
    return MAUVE_OK;
}

int mauve_backbone_fetch(mauve_ctx *c, int64_t *seg_iv, int64_t *seg_col, int64_t *seg_len, uint32_t *seg_mask, int64_t *seg_left,
                         int64_t *seg_right, int64_t *islands)
{
    if (!c) return MAUVE_ERR_ARG;
    const BackboneResult &B = c->bb;
    if (!B.valid) { c->err = "backbone_fetch: no backbone computed"; return MAUVE_ERR_STATE; }
    if (seg_iv) std::copy(B.seg_iv.begin(), B.seg_iv.end(), seg_iv);
    if (seg_col) std::copy(B.seg_col.begin(), B.seg_col.end(), seg_col);
    if (seg_len) std::copy(B.seg_len.begin(), B.seg_len.end(), seg_len);
    if (seg_mask) std::copy(B.seg_mask.begin(), B.seg_mask.end(), seg_mask);
    if (seg_left) std::copy(B.seg_left.begin(), B.seg_left.end(), seg_left);
    if (seg_right) std::copy(B.seg_right.begin(), B.seg_right.end(), seg_right);
    if (islands) std::copy(B.islands.begin(), B.islands.end(), islands);
    return MAUVE_OK;
}

}  // extern "C"
