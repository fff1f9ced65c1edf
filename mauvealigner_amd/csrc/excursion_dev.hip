// excursion_dev.hip -- excursions of the column scores: the state machine of getLocalRecordHeights (evd.cpp:12-66,
// multiEVD.cpp:29-79) along the columns of chosen ranges, for chosen genome pairs (pair streams) or genome groups (core streams).  It reads
// the coordinate index in force (S14) and the resident genomes; a cell is the S15 cell, the letter codes and the run rule are those of S16.
// With v = -s the walk is x_c = max(0, x_{c-1} + v_c): a column acts on x as x -> max(B, x + A) with (A, B) = (v, 0), such maps compose, and a
// column outside the stream is the identity (0, -inf).  So no thread walks a stream:
//   ex_front     (extract_cells.hpp) the ranges checked; a chunk is EXC_UNITS 64-column words of one range, counted from the range's first
//                word: chunks per range (ExcChunks), scanned.  An element is one (set, chunk), stored set-major: for one set the elements
//                are its streams one after another, each starting at its range's first chunk (the head).
//   exc_walk<0>  a workgroup per chunk (grid-stride).  Phase 1, a wave per word and a lane per column: the bit-sliced letter masks of the
//                genomes some set names, to LDS.  Phase 2, a wave per set: per word the lane's value (pairs: the run-opening columns from the
//                carry-chain add ps_run_mask, the state in front of the chunk from ps_look_back), a wave scan of the composed maps, the
//                words chained -> the chunk's map.
//   exc_scan     segmented scan of the maps along every set (tile aggregates, then every workgroup composes the tiles before it): the x
//                at every chunk's entry.
//   exc_walk<1>  the same walk with the entry x: the chunk's emission count, the maximum of x behind its last emission (of all its
//                columns when it has none), and the stream's x at the end of a range's last chunk.
//   exc_scan     counts summed and the maximum carried along every set -- it restarts at a chunk with an emission -> every chunk's
//                first output slot in its stream and the height carried into it; the streams' counts and tail heights.
//   vscan        the streams' counts -> stream_off, the one figure read back.
//   exc_walk<2>  the walk a third time: a segmented maximum scan over the lanes gives every emission its height, a ballot its slot.
// The column values are recomputed in each walk rather than kept: a kept value is 8 bytes per column and set, the index words and genome
// bases they are made from a fraction of that.  Records are placed by scanned offsets: two calls return identical bytes.
#include "common.hpp"
#include "extract_cells.hpp"
#include <algorithm>
#include <cstring>
#include <vector>

namespace {

constexpr int EXC_UNITS = 8;                       // words per chunk: MAUVE_EXCURSION_CHUNK = 512 columns from the range's first word on
constexpr int EXC_MAX_GROUPS = 2048;               // workgroups of exc_walk at the most
constexpr int EXC_MAX_SETS = 1024;
constexpr int64_t EXC_MAX_STREAMS = (int64_t)1 << 24;
constexpr int64_t EXC_NEG = -((int64_t)1 << 62);   // the B of the identity map
static_assert(EXC_UNITS * 64 == MAUVE_EXCURSION_CHUNK, "chunk size");

// chunks of a range
struct ExcChunks {
    const int64_t *gs, *cl;
    static ExcChunks of(const int64_t *gs, const int64_t *cl) { return ExcChunks{gs, cl}; }
    __device__ int64_t value(uint32_t r) const
    {
        const int64_t n = cl[r];
        return n ? (((gs[r] + n - 1) >> 6) - (gs[r] >> 6) + EXC_UNITS) / EXC_UNITS : 0;
    }
};
struct ExcArray { const int64_t *p; __device__ int64_t value(uint32_t i) const { return p[i]; } };

// the sets of a call: ordered pairs (a, b) or genome masks; need: the genomes any of them names
struct ExcSets { int S, pairs; const int32_t *a, *b; const uint32_t *mask; int32_t m[4][4], gap_open, gap_extend; uint32_t need; };

// the per-element arrays [S][n_chunks] and the result
struct ExcData {
    int64_t n_chunks;
    int64_t *A, *B;                                // the chunk's map; later: emissions of the stream before the chunk, the height carried into it
    int64_t *X, *CN, *PO;                          // x at the chunk's entry; its emissions; the maximum of x behind the last one
    int64_t *cnt, *tail;                           // per stream: emissions; (x, h) at its end
    const int64_t *stream_off;
    int64_t *height, *end_col, n_exc;
};

__device__ __forceinline__ int64_t exc_wave_max(int64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (int64_t)__shfl_xor((long long)v, o));
    return v;
}
__device__ __forceinline__ int64_t exc_up(int64_t v, int o) { return (int64_t)__shfl_up((long long)v, o); }

__device__ __forceinline__ int exc_code(const uint64_t *L, int lane)
{
    int c = -1;
#pragma unroll
    for (int l = 0; l < 5; l++) if (L[l] >> lane & 1) c = l;
    return c < 4 ? c : 0;                          // N scores as A (the caller has seen a residue)
}

// MODE 0: the chunks' maps.  1: counts and maxima from the entry x.  2: the records.
template <int MODE>
__global__ void __launch_bounds__(256) exc_walk(CoordDev D, ExGenomes G, int64_t R, const int64_t *__restrict__ r_iv, const int64_t *__restrict__ gstart,
                                                const int64_t *__restrict__ clen, const int64_t *__restrict__ chunk_off, ExcSets Z, ExcData W,
                                                uint32_t *__restrict__ flag)
{
    __shared__ uint64_t s_L[EXC_UNITS][MAUVE_MAX_SEQ][5];      // the letter masks of the chunk
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, N = D.N;
    uint32_t bad = 0;
    for (int64_t ch = blockIdx.x; ch < W.n_chunks; ch += gridDim.x) {
        const int64_t r = ex_range_of(chunk_off, R, ch), i = r_iv ? r_iv[r] : r, gs = gstart[r], n = clen[r];
        const int64_t u0 = (ch - chunk_off[r]) * EXC_UNITS, units = ((gs + n - 1) >> 6) - (gs >> 6) + 1, aw0 = (gs >> 6) + u0;
        const int nu = (int)min((int64_t)EXC_UNITS, units - u0);
        const bool iv_ok = i >= 0 && i < D.n_iv;               // (ex_ranges refused the call otherwise)
        const bool last = ch + 1 == chunk_off[r + 1];
        if (!iv_ok) bad |= CO_BAD_INDEX;
        // phase 1
        for (int j = wave; j < nu; j += 4) {
            const int64_t x = (aw0 + j) * 64 + lane;
            const bool valid = iv_ok && x >= gs && x < gs + n;
            for (int g = 0; g < N; g++) {
                if (!(Z.need >> g & 1)) continue;
                int code = -1;
                if (valid) { const char c = ex_cell(D, G, i, x, g, &code, &bad); if (c == 'N') code = 4; }
                uint64_t mine = 0;
#pragma unroll
                for (int l = 0; l < 5; l++) { const uint64_t m = __ballot(code == l); if (lane == l) mine = m; }
                if (lane < 5) s_L[j][g][lane] = mine;
            }
        }
        __syncthreads();
        // phase 2
        for (int k = wave; k < Z.S && iv_ok; k += 4) {
            const size_t el = (size_t)k * (size_t)W.n_chunks + (size_t)ch;
            const int a = Z.pairs ? Z.a[k] : 0, b = Z.pairs ? Z.b[k] : 0;
            const uint32_t gm = Z.pairs ? 0u : Z.mask[k];
            uint32_t ca = 0, cb = 0;
            bool known = u0 == 0;                              // the range's first word: no run open
            int64_t cA = 0, cB = EXC_NEG;                      // MODE 0: the map of the words so far
            int64_t xw = MODE ? W.X[el] : 0;                   // MODE 1, 2: x in front of the word
            int64_t post = 0, cnt = 0;                         // MODE 1
            int64_t hc = MODE == 2 ? W.B[el] : 0;              // MODE 2: the maximum since the last emission, in front of the word
            int64_t slot = MODE == 2 ? W.stream_off[(size_t)r * Z.S + k] + W.A[el] : 0;
            for (int j = 0; j < nu; j++) {
                // the lane's column: in the stream? its value v = -s
                bool in = false;
                int64_t v = 0;
                if (Z.pairs) {
                    const uint64_t *La = s_L[j][a], *Lb = s_L[j][b];
                    const uint64_t Pa = La[0] | La[1] | La[2] | La[3] | La[4], Pb = Lb[0] | Lb[1] | Lb[2] | Lb[3] | Lb[4];
                    const uint64_t Y = Pa | Pb, oa = Pa & ~Pb, ob = Pb & ~Pa;
                    if (!known && Y) { ps_look_back(D, i, a, b, gs, aw0 + j, ca, cb); known = true; }
                    const uint64_t open = ps_run_mask(oa, Y, ca) | ps_run_mask(ob, Y, cb);
                    in = Y >> lane & 1;
                    if (Pa & Pb & (1ull << lane)) v = -(int64_t)Z.m[exc_code(La, lane)][exc_code(Lb, lane)];
                    else if (in) v = -(int64_t)(open >> lane & 1 ? Z.gap_open : Z.gap_extend);
                } else {
                    uint64_t all = ~0ull;
                    for (int g = 0; g < N; g++)
                        if (gm >> g & 1) { const uint64_t *L = s_L[j][g]; all &= L[0] | L[1] | L[2] | L[3] | L[4]; }
                    in = all >> lane & 1;
                    if (in) {
                        int32_t seen[4] = {0, 0, 0, 0};
                        int64_t s = 0;
                        for (int g = 0; g < N; g++) {
                            if (!(gm >> g & 1)) continue;
                            const int y = exc_code(s_L[j][g], lane);
#pragma unroll
                            for (int x = 0; x < 4; x++) { s += (int64_t)seen[x] * Z.m[x][y]; seen[x] += x == y; }
                        }
                        v = -s;
                    }
                }
                // the composed map of the lanes up to this one
                int64_t A = in ? v : 0, B = in ? 0 : EXC_NEG;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int64_t tA = exc_up(A, o), tB = exc_up(B, o);
                    if (lane >= o) { B = max(B, tB + A); A += tA; }
                }
                if (MODE == 0) {
                    const int64_t wA = (int64_t)__shfl((long long)A, 63), wB = (int64_t)__shfl((long long)B, 63);
                    cB = max(wB, cB + wA); cA += wA;
                    continue;
                }
                const int64_t x = max(B, xw + A);
                int64_t xp = exc_up(x, 1);
                if (lane == 0) xp = xw;
                const bool e = in && xp > 0 && xp + v < 0;
                const uint64_t E = __ballot(e);
                xw = (int64_t)__shfl((long long)x, 63);
                if (MODE == 1) {
                    if (!E) post = max(post, exc_wave_max(x));
                    else { const int le = 63 - __clzll((long long)E); post = exc_wave_max(lane >= le ? x : 0); cnt += __popcll(E); }
                } else {
                    // the maximum of x from the last emission at or before the lane on (from the word's start when there is none)
                    int64_t mx = x;
                    int fl = e;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const int64_t t = exc_up(mx, o);
                        const int tf = __shfl_up(fl, o);
                        if (lane >= o) { if (!fl) mx = max(mx, t); fl |= tf; }
                    }
                    int64_t hb = exc_up(mx, 1);
                    int fb = __shfl_up(fl, 1);
                    if (lane == 0) { hb = 0; fb = 0; }
                    if (e) {
                        const int64_t o = slot + __popcll(E & co_below(lane));
                        if (o >= 0 && o < W.n_exc) { W.height[o] = fb ? hb : max(hb, hc); W.end_col[o] = (aw0 + j) * 64 + lane - D.col_off[i]; }
                        else bad |= CO_BAD_INDEX;
                    }
                    const int64_t m63 = (int64_t)__shfl((long long)mx, 63);
                    hc = E ? m63 : max(hc, m63);
                    slot += __popcll(E);
                }
            }
            if (lane == 0) {
                if (MODE == 0) { W.A[el] = cA; W.B[el] = cB; }
                if (MODE == 1) { W.CN[el] = cnt; W.PO[el] = post; if (last) W.tail[2 * ((size_t)r * Z.S + k)] = xw; }
            }
        }
        __syncthreads();
    }
    if (bad) atomicOr(flag, bad);
}

// ---- segmented scans along the sets: an element (a, b, f), f bit 0: the first chunk of a range (head), bit 1: a cut ----
struct ExcTrip { int64_t a, b; int32_t f; };
// the maps: (A, B) after (A', B') is (A + A', max(B', B + A'))
struct ExcOpMap {
    __device__ static ExcTrip id() { return ExcTrip{0, EXC_NEG, 0}; }
    __device__ static ExcTrip comb(const ExcTrip &l, const ExcTrip &r) { return r.f & 1 ? r : ExcTrip{l.a + r.a, max(r.b, l.b + r.a), l.f}; }
};
// a: the emissions summed; b: the maximum, which restarts at an element with an emission (bit 1)
struct ExcOpCnt {
    __device__ static ExcTrip id() { return ExcTrip{0, 0, 0}; }
    __device__ static ExcTrip comb(const ExcTrip &l, const ExcTrip &r) { return r.f & 1 ? r : ExcTrip{l.a + r.a, r.f & 2 ? r.b : max(l.b, r.b), l.f | r.f}; }
};
struct ExcIoMap {
    ExcData W; const int64_t *chunk_off; int64_t R; int S;
    __device__ ExcTrip load(int k, int64_t i) const
    {
        const size_t el = (size_t)k * W.n_chunks + i;
        return ExcTrip{W.A[el], W.B[el], i == chunk_off[ex_range_of(chunk_off, R, i)]};
    }
    __device__ void store(int k, int64_t i, const ExcTrip &before, const ExcTrip &me) const
    {
        W.X[(size_t)k * W.n_chunks + i] = me.f & 1 ? 0 : max(before.b, before.a);        // the maps before it, applied to 0
    }
};
struct ExcIoCnt {
    ExcData W; const int64_t *chunk_off; int64_t R; int S;
    __device__ ExcTrip load(int k, int64_t i) const
    {
        const size_t el = (size_t)k * W.n_chunks + i;
        const int64_t n = W.CN[el];
        return ExcTrip{n, W.PO[el], (i == chunk_off[ex_range_of(chunk_off, R, i)] ? 1 : 0) | (n > 0 ? 2 : 0)};
    }
    __device__ void store(int k, int64_t i, const ExcTrip &before, const ExcTrip &me) const
    {
        const size_t el = (size_t)k * W.n_chunks + i;
        const int64_t nb = me.f & 1 ? 0 : before.a, hi = me.f & 1 ? 0 : before.b;
        W.A[el] = nb; W.B[el] = hi;
        const int64_t r = ex_range_of(chunk_off, R, i);
        if (i + 1 == chunk_off[r + 1]) {
            const size_t st = (size_t)r * S + k;
            W.cnt[st] = nb + me.a;
            W.tail[2 * st + 1] = me.f & 2 ? me.b : max(hi, me.b);
        }
    }
};

// exclusive scan of one element per thread over the workgroup, in thread order; *total: all of them
template <class Op>
__device__ __forceinline__ ExcTrip exc_block_scan(const ExcTrip &v, ExcTrip *total, ExcTrip *lds /*[4]*/)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    ExcTrip inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const ExcTrip t{exc_up(inc.a, o), exc_up(inc.b, o), __shfl_up(inc.f, o)};
        if (lane >= o) inc = Op::comb(t, inc);
    }
    ExcTrip up{exc_up(inc.a, 1), exc_up(inc.b, 1), __shfl_up(inc.f, 1)};
    if (lane == 0) up = Op::id();
    __syncthreads();                         // lds may still be read from an earlier call
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    ExcTrip wbase = Op::id(), tot = Op::id();
#pragma unroll
    for (int w = 0; w < 4; w++) { const ExcTrip c = lds[w]; if (w < wave) wbase = Op::comb(wbase, c); tot = Op::comb(tot, c); }
    *total = tot;
    return Op::comb(wbase, up);
}

// grid (tiles, sets): the tile's aggregate
template <class Op, class Io>
__global__ void __launch_bounds__(256) exc_scan_tiles(Io io, ExcTrip *__restrict__ agg)
{
    __shared__ ExcTrip lds[4];
    const int k = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * devscan::TILE + threadIdx.x * 4;
    ExcTrip t = Op::id();
#pragma unroll
    for (int q = 0; q < 4; q++) if (i0 + q < io.W.n_chunks) t = Op::comb(t, io.load(k, i0 + q));
    ExcTrip tot;
    (void)exc_block_scan<Op>(t, &tot, lds);
    if (threadIdx.x == 0) agg[(size_t)k * gridDim.x + blockIdx.x] = tot;
}
// ... and every workgroup composes the aggregates of the tiles before it for itself, then scans its own elements
template <class Op, class Io>
__global__ void __launch_bounds__(256) exc_scan_write(Io io, const ExcTrip *__restrict__ agg)
{
    __shared__ ExcTrip lds[4];
    const int k = blockIdx.y;
    const uint32_t nb = blockIdx.x, per = (nb + 255) / 256;
    ExcTrip mine = Op::id();
    for (uint32_t t = threadIdx.x * per; t < min(nb, (threadIdx.x + 1) * per); t++) mine = Op::comb(mine, agg[(size_t)k * gridDim.x + t]);
    ExcTrip before;
    (void)exc_block_scan<Op>(mine, &before, lds);
    const int64_t i0 = (int64_t)blockIdx.x * devscan::TILE + threadIdx.x * 4;
    ExcTrip e[4], t = Op::id();
#pragma unroll
    for (int q = 0; q < 4; q++) { e[q] = i0 + q < io.W.n_chunks ? io.load(k, i0 + q) : Op::id(); t = Op::comb(t, e[q]); }
    ExcTrip dummy;
    ExcTrip run = Op::comb(before, exc_block_scan<Op>(t, &dummy, lds));
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if (i0 + q >= io.W.n_chunks) break;
        io.store(k, i0 + q, run, e[q]);
        run = Op::comb(run, e[q]);
    }
}

template <class Op, class Io>
void exc_scan(mauve_ctx *c, const Io &io, ExcTrip *agg)
{
    const dim3 grid((uint32_t)((io.W.n_chunks + devscan::TILE - 1) / devscan::TILE), (uint32_t)io.S);
    hipLaunchKernelGGL((exc_scan_tiles<Op, Io>), grid, dim3(256), 0, c->stream, io, agg);
    hipLaunchKernelGGL((exc_scan_write<Op, Io>), grid, dim3(256), 0, c->stream, io, (const ExcTrip *)agg);
}

// both entry points behind their set lists.  sets: pairs: the a of every pair, then the b; else the masks
int exc_run(mauve_ctx *c, const char *who, const mauve_scoring *sc, bool pairs, const std::vector<int32_t> &sets, uint32_t need, int64_t n_range,
            const int64_t *range_iv, const int64_t *range_col, const int64_t *range_len, int64_t *n_exc)
{
    c->exc.valid = false;
    mauve_scoring dflt;
    if (!sc) { mauve_default_scoring(&dflt); sc = &dflt; }
    const int S = (int)(pairs ? sets.size() / 2 : sets.size());
    // the stream limit comes before any device work; range arguments that ex_front will refuse are left to it: that refusal comes first
    const int64_t R = range_iv ? n_range : c->co.n_iv;
    const bool r_ok = R >= 0 && R < ((int64_t)1 << 31) && !(range_iv && R && (!range_col || !range_len));
    if (r_ok && R * (int64_t)S > EXC_MAX_STREAMS) { c->err = std::string(who) + ": more than 2^24 streams"; return MAUVE_ERR_LIMIT; }
    ExFront F;                                               // the set lists travel behind the ranges
    if (const int rf = ex_front<ExcChunks>(c, who, c->exc_work, n_range, range_iv, range_col, range_len, sets.data(), sets.size() * 4, &F)) return rf;
    const int64_t n_chunks = F.total, n_stream = R * (int64_t)S;
    if (n_chunks * (int64_t)S >= ((int64_t)1 << 31)) { c->err = std::string(who) + ": the ranges hold 2^40 columns or more over all sets"; return MAUVE_ERR_LIMIT; }
    const size_t n_el = (size_t)n_chunks * (size_t)S, tiles = (size_t)((n_chunks + devscan::TILE - 1) / devscan::TILE);
    const uint32_t tilesS = (uint32_t)((n_stream + devscan::TILE - 1) / devscan::TILE);
    // scratch: five element arrays | the tile aggregates | the streams' counts | their tile sums.  meta: stream_off | tail
    const size_t t_agg = 5 * up64(n_el * 8), t_cnt = t_agg + up64(tiles * S * sizeof(ExcTrip)), t_bs = t_cnt + up64((size_t)n_stream * 8 + 8),
                 t_total = t_bs + up64((size_t)tilesS * 8 + 8);
    HIPCHK(c, c->exc_tmp.ensure(t_total));
    const size_t m_tail = up64((size_t)(n_stream + 1) * 8);
    HIPCHK(c, c->exc_meta.ensure(m_tail + up64((size_t)n_stream * 16 + 8)));
    char *tb = c->exc_tmp.as<char>(), *mb = c->exc_meta.as<char>();
    ExcData W; memset(&W, 0, sizeof W);
    W.n_chunks = n_chunks;
    W.A = reinterpret_cast<int64_t *>(tb); W.B = reinterpret_cast<int64_t *>(tb + up64(n_el * 8)); W.X = reinterpret_cast<int64_t *>(tb + 2 * up64(n_el * 8));
    W.CN = reinterpret_cast<int64_t *>(tb + 3 * up64(n_el * 8)); W.PO = reinterpret_cast<int64_t *>(tb + 4 * up64(n_el * 8));
    ExcTrip *agg = reinterpret_cast<ExcTrip *>(tb + t_agg);
    W.cnt = reinterpret_cast<int64_t *>(tb + t_cnt);
    int64_t *bsum = reinterpret_cast<int64_t *>(tb + t_bs), *stream_off = reinterpret_cast<int64_t *>(mb);
    W.stream_off = stream_off; W.tail = reinterpret_cast<int64_t *>(mb + m_tail);
    HIPCHK(c, hipMemsetAsync(W.cnt, 0, (size_t)n_stream * 8 + 8, c->stream));
    HIPCHK(c, hipMemsetAsync(W.tail, 0, (size_t)n_stream * 16 + 8, c->stream));
    ExcSets Z; memset(&Z, 0, sizeof Z);
    Z.S = S; Z.pairs = pairs; Z.need = need; Z.gap_open = sc->gap_open; Z.gap_extend = sc->gap_extend;
    for (int x = 0; x < 4; x++) for (int y = 0; y < 4; y++) Z.m[x][y] = sc->matrix[x][y];
    const int32_t *d_sets = reinterpret_cast<const int32_t *>(F.tail);
    if (pairs) { Z.a = d_sets; Z.b = d_sets + S; } else Z.mask = reinterpret_cast<const uint32_t *>(d_sets);
    const bool work = n_chunks > 0 && S > 0;
    const dim3 grid((uint32_t)std::min<int64_t>(n_chunks, EXC_MAX_GROUPS));
    const CoordDev &D = *c->co.dev;
    if (work) {
        const int64_t cols = n_chunks * MAUVE_EXCURSION_CHUNK;      // (the timers' unit: columns of chunks, whole)
        { KernelTimer t(c, MAUVE_K_EXC_MAPS, cols);
          hipLaunchKernelGGL(exc_walk<0>, grid, dim3(256), 0, c->stream, D, F.G, F.R, F.d_iv, F.gstart, F.clen, F.off, Z, W, F.flag); }
        { KernelTimer t(c, MAUVE_K_EXC_SCAN, (int64_t)n_el);
          exc_scan<ExcOpMap>(c, ExcIoMap{W, F.off, F.R, S}, agg); }
        { KernelTimer t(c, MAUVE_K_EXC_COUNT, cols);
          hipLaunchKernelGGL(exc_walk<1>, grid, dim3(256), 0, c->stream, D, F.G, F.R, F.d_iv, F.gstart, F.clen, F.off, Z, W, F.flag); }
        { KernelTimer t(c, MAUVE_K_EXC_SCAN, (int64_t)n_el);
          exc_scan<ExcOpCnt>(c, ExcIoCnt{W, F.off, F.R, S}, agg); }
    }
    if (n_stream) {
        KernelTimer t(c, MAUVE_K_EXC_SCAN, n_stream);
        const ExcArray in{W.cnt};
        hipLaunchKernelGGL((devscan::vscan_partial<int64_t, ExcArray>), dim3(tilesS), dim3(256), 0, c->stream, in, (uint32_t)n_stream, bsum);
        hipLaunchKernelGGL((devscan::vscan_write<int64_t, ExcArray>), dim3(tilesS), dim3(256), 0, c->stream, in, (uint32_t)n_stream, bsum, stream_off, (int64_t *)nullptr);
    } else HIPCHK(c, hipMemsetAsync(stream_off, 0, 8, c->stream));
    HIPCHK(c, hipGetLastError());
    char *hb = c->pin_stage.as<char>();                      // (ex_front left it at least 256 bytes long)
    HIPCHK(c, hipMemcpyAsync(hb, F.flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hb + 64, stream_off + n_stream, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (const int rf = co_flag_result(c, *reinterpret_cast<const uint32_t *>(hb), who, EX_OUTSIDE)) return rf;
    const int64_t total = *reinterpret_cast<const int64_t *>(hb + 64);
    HIPCHK(c, c->exc_rec.ensure(2 * up64((size_t)total * 8) + 64));
    W.height = c->exc_rec.as<int64_t>(); W.end_col = reinterpret_cast<int64_t *>(c->exc_rec.as<char>() + up64((size_t)total * 8)); W.n_exc = total;
    if (work && total) {
        { KernelTimer t(c, MAUVE_K_EXC_WRITE, n_chunks * MAUVE_EXCURSION_CHUNK);
          hipLaunchKernelGGL(exc_walk<2>, grid, dim3(256), 0, c->stream, D, F.G, F.R, F.d_iv, F.gstart, F.clen, F.off, Z, W, F.flag); }
        HIPCHK(c, hipGetLastError());
        if (const int rf = co_flag_read(c, F.flag, who, EX_OUTSIDE)) return rf;
    }
    c->exc.valid = true; c->exc.genome_gen = c->genome_gen; c->exc.n_stream = n_stream; c->exc.n_exc = total;
    if (n_exc) *n_exc = total;
    return MAUVE_OK;
}

}  // namespace

extern "C" {

int mauve_excursions_pairs(mauve_ctx *c, const mauve_scoring *sc, int64_t n_pair, const int32_t *pair_a, const int32_t *pair_b, int64_t n_range,
                           const int64_t *range_iv, const int64_t *range_col, const int64_t *range_len, int64_t *n_exc)
{
    if (!c) return MAUVE_ERR_ARG;
    c->exc.valid = false;
    if (const int rs = ex_check_state(c, "excursions_pairs")) return rs;
    const int N = c->nseq;
    std::vector<int32_t> sets;                               // the a of every pair, then the b
    uint32_t need = 0;
    if (!pair_a) {
        for (int a = 0; a < N; a++) for (int b = a + 1; b < N; b++) sets.push_back(a);
        for (int a = 0; a < N; a++) for (int b = a + 1; b < N; b++) sets.push_back(b);
    } else {
        if (n_pair < 1 || n_pair > EXC_MAX_SETS || !pair_b) { c->err = "excursions_pairs: n_pair outside [1, 1024] or pair_b missing"; return MAUVE_ERR_ARG; }
        for (int64_t k = 0; k < n_pair; k++) {
            const int32_t a = pair_a[k], b = pair_b[k];
            if (a < 0 || a >= N || b < 0 || b >= N || a == b) { c->err = "excursions_pairs: pair " + std::to_string(k) + " holds an id outside [0, nseq) or one genome twice"; return MAUVE_ERR_ARG; }
        }
        sets.assign(pair_a, pair_a + n_pair); sets.insert(sets.end(), pair_b, pair_b + n_pair);
    }
    for (const int32_t g : sets) need |= 1u << g;
    return exc_run(c, "excursions_pairs", sc, true, sets, need, n_range, range_iv, range_col, range_len, n_exc);
}

int mauve_excursions_core(mauve_ctx *c, const mauve_scoring *sc, int64_t n_group, const uint32_t *group_mask, int64_t n_range, const int64_t *range_iv,
                          const int64_t *range_col, const int64_t *range_len, int64_t *n_exc)
{
    if (!c) return MAUVE_ERR_ARG;
    c->exc.valid = false;
    if (const int rs = ex_check_state(c, "excursions_core")) return rs;
    const int N = c->nseq;
    const uint32_t all = N >= 32 ? 0xffffffffu : (1u << N) - 1;
    std::vector<int32_t> sets;
    uint32_t need = 0;
    if (!group_mask) {
        if (N < 2) { c->err = "excursions_core: a group needs at least two genomes"; return MAUVE_ERR_ARG; }
        sets.push_back((int32_t)all);
    } else {
        if (n_group < 1 || n_group > EXC_MAX_SETS) { c->err = "excursions_core: n_group outside [1, 1024]"; return MAUVE_ERR_ARG; }
        for (int64_t k = 0; k < n_group; k++) {
            const uint32_t m = group_mask[k];
            if ((m & ~all) || __builtin_popcount(m) < 2) { c->err = "excursions_core: group " + std::to_string(k) + " holds fewer than two genomes or a bit at or above nseq"; return MAUVE_ERR_ARG; }
            sets.push_back((int32_t)m);
        }
    }
    for (const int32_t m : sets) need |= (uint32_t)m;
    return exc_run(c, "excursions_core", sc, false, sets, need, n_range, range_iv, range_col, range_len, n_exc);
}

int mauve_excursions_fetch(mauve_ctx *c, int64_t *height, int64_t *end_col, int64_t *stream_off, int64_t *tail)
{
    if (!c) return MAUVE_ERR_ARG;
    const mauve_ctx::Excursions &X = c->exc;
    if (!X.valid || !c->co.valid || X.genome_gen != c->genome_gen) {
        c->err = "excursions_fetch: no result in this context (mauve_excursions_pairs or mauve_excursions_core first; an index call or a genome upload ends it)";
        return MAUVE_ERR_STATE;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nb = (size_t)X.n_exc * 8, m_tail = up64((size_t)(X.n_stream + 1) * 8);
    const char *rb = c->exc_rec.as<char>(), *mb = c->exc_meta.as<char>();
    if (height) if (const int rc = copy_to_caller(c, c->pin_stage, height, rb, nb)) return rc;
    if (end_col) if (const int rc = copy_to_caller(c, c->pin_stage, end_col, rb + up64(nb), nb)) return rc;
    if (stream_off) if (const int rc = copy_to_caller(c, c->pin_stage, stream_off, mb, (size_t)(X.n_stream + 1) * 8)) return rc;
    if (tail) if (const int rc = copy_to_caller(c, c->pin_stage, tail, mb + m_tail, (size_t)X.n_stream * 16)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MAUVE_OK;
}

void mauve_excursion_thresholds(const int64_t *height, int64_t n, int64_t threshold[4], int64_t above[4])
{
    static const double frac[4] = {.95, .99, .999, .9999};
    for (int q = 0; q < 4; q++) threshold[q] = above[q] = 0;
    if (n <= 0) return;
    std::vector<int64_t> h(height, height + n);
    std::sort(h.begin(), h.end());
    for (int q = 0; q < 4; q++) {
        const size_t idx = std::min((size_t)((size_t)n * frac[q]), (size_t)n - 1);           // (evd.cpp:109-116: a size_t times a double)
        threshold[q] = h[idx]; above[q] = n - (int64_t)idx;
    }
}

}  // extern "C"
