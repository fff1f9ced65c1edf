// pairstat_dev.hip -- pairwise column statistics of the alignment: for chosen genome pairs and chosen column ranges, what the
// two rows show against each other -- a 5 x 5 letter table, one-sided columns, gap runs, empty columns.  The stage stands in for the host walks
// of IdentityMatrix (mauveAligner.cpp:784-800, calculateBackboneCoverage.cpp:106-127), BackboneIdentityMatrix (pairCompare.cpp:57-60,77,
// calculateBackboneCoverage2.cpp:98-121), the pairwise loop of gappiness.cpp:33-50 and computeSPScore (multiEVD.cpp:41-46, repeatoire.cpp:2527).
// It reads the coordinate index in force (S14) and the resident genomes; a cell is the S15 cell (extract_cells.hpp).
//   ex_front    (extract_cells.hpp) the ranges against their intervals, the interval ends against the resident genomes; a unit of work is
//               one range x one 64-column word of the index that overlaps it: units per range (PsUnits), scanned
//   ps_count    a workgroup takes a span of consecutive chunks of PS_UNITS units.  Phase 1, a wave per unit and a lane per column: the cell of
//               every genome, five ballots per genome = the bit-sliced letter masks, to LDS.  Phase 2, a thread per pair (strided over the
//               workgroup above 256 pairs) walks the chunk's units: popcounts of mask intersections into 30 counters in registers; the gap
//               runs come out of one 64-bit add per word (ps_runs).  The counters leave with 64-bit integer atomics at the span's end, and
//               in per-range mode whenever the range changes.
// A span that starts inside a range does not know whether a run is open there.  The pair finds out when it meets its first occupied column:
// it looks back through the index's presence words to its previous occupied column of the same range (ps_look_back).  The words passed over
// are empty for the pair, so the spans they belong to look back at nothing: every word is looked back at by at most one span.
// All counts are integers and no result depends on the tiling.
#include "common.hpp"
#include "extract_cells.hpp"
#include <algorithm>
#include <cstring>
#include <vector>

namespace {

constexpr int PS_UNITS = 16;                      // units per chunk: 1024 columns of one range that starts on a word boundary
constexpr int PS_MAX_SPANS = 1024;                // workgroups of ps_count at the most
constexpr int PS_MAX_PAIRS = 1024;
constexpr int64_t PS_MAX_RECORDS = (int64_t)1 << 24;
constexpr int PS_W = MAUVE_PAIR_STATS_WORDS;

// the 64-column words of the index a range overlaps
struct PsUnits {
    const int64_t *gs, *cl;
    static PsUnits of(const int64_t *gs, const int64_t *cl) { return PsUnits{gs, cl}; }
    __device__ int64_t value(uint32_t r) const { const int64_t n = cl[r]; return n ? ((gs[r] + n - 1) >> 6) - (gs[r] >> 6) + 1 : 0; }
};

__device__ __forceinline__ void ps_flush(unsigned long long *__restrict__ rec, uint32_t (&cnt)[30])
{
#pragma unroll
    for (int k = 0; k < 30; k++) { if (cnt[k]) atomicAdd(&rec[k], (unsigned long long)cnt[k]); cnt[k] = 0; }
}

// workgroup = the chunks [blockIdx.x * cps, ... + cps) of the unit list
__global__ void __launch_bounds__(256) ps_count(CoordDev D, ExGenomes G, int64_t R, const int64_t *__restrict__ r_iv, const int64_t *__restrict__ gstart,
                                                const int64_t *__restrict__ clen, const int64_t *__restrict__ unit_off, int64_t n_units, int64_t cps,
                                                int P, const int32_t *__restrict__ pair_a, const int32_t *__restrict__ pair_b, int per_range,
                                                unsigned long long *__restrict__ out, uint32_t *__restrict__ flag)
{
    __shared__ uint64_t s_L[PS_UNITS][MAUVE_MAX_SEQ][5];       // the letter masks of the chunk
    __shared__ uint64_t s_v[PS_UNITS];                         // the range's part of the word
    __shared__ int64_t s_aw[PS_UNITS], s_gs[PS_UNITS], s_iv[PS_UNITS], s_r[PS_UNITS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, N = D.N;
    const int64_t n_chunks = (n_units + PS_UNITS - 1) / PS_UNITS;
    const int64_t c0 = (int64_t)blockIdx.x * cps, c1 = min(c0 + cps, n_chunks);
    const bool carried = P <= 256;                             // a thread has one pair: its counters and run state live across the span's chunks
    uint32_t cnt[30], ca = 0, cb = 0, bad = 0;
    int64_t cur = -1;
    bool known = false;
#pragma unroll
    for (int k = 0; k < 30; k++) cnt[k] = 0;
    for (int64_t c = c0; c < c1; c++) {
        const int64_t u0 = c * PS_UNITS;
        const int nu = (int)min((int64_t)PS_UNITS, n_units - u0);
        // phase 1
        for (int j = wave; j < nu; j += 4) {
            const int64_t u = u0 + j, r = ex_range_of(unit_off, R, u), i = r_iv ? r_iv[r] : r;
            const int64_t gs = gstart[r], aw = (gs >> 6) + (u - unit_off[r]), x = aw * 64 + lane;
            const bool iv_ok = i >= 0 && i < D.n_iv;           // (ex_ranges refused the call otherwise)
            const bool valid = iv_ok && x >= gs && x < gs + clen[r];
            if (!iv_ok) bad |= CO_BAD_INDEX;
            const uint64_t V = __ballot(valid);
            if (lane == 0) { s_v[j] = V; s_aw[j] = aw; s_gs[j] = gs; s_iv[j] = i; s_r[j] = r; }
            for (int g = 0; g < N; g++) {
                int code = -1;
                if (valid) { const char ch = ex_cell(D, G, i, x, g, &code, &bad); if (ch == 'N') code = 4; }
                uint64_t mine = 0;
#pragma unroll
                for (int l = 0; l < 5; l++) { const uint64_t m = __ballot(code == l); if (lane == l) mine = m; }
                if (lane < 5) s_L[j][g][lane] = mine;
            }
        }
        __syncthreads();
        // phase 2
        for (int p = threadIdx.x; p < P; p += 256) {
            if (!carried || c == c0) { cur = -1; ca = cb = 0; known = false; }
            const int a = pair_a[p], b = pair_b[p];
            for (int j = 0; j < nu; j++) {
                const int64_t r = s_r[j];
                if (r != cur) {
                    if (per_range && cur >= 0) ps_flush(out + ((size_t)cur * (size_t)P + (size_t)p) * PS_W, cnt);
                    cur = r; ca = cb = 0;
                    known = s_aw[j] == (s_gs[j] >> 6);          // the range's first word: no run open
                }
                uint64_t La[5], Lb[5];
#pragma unroll
                for (int l = 0; l < 5; l++) { La[l] = s_L[j][a][l]; Lb[l] = s_L[j][b][l]; }
                const uint64_t Pa = La[0] | La[1] | La[2] | La[3] | La[4], Pb = Lb[0] | Lb[1] | Lb[2] | Lb[3] | Lb[4];
                const uint64_t Y = Pa | Pb, oa = Pa & ~Pb, ob = Pb & ~Pa;
                if (!known && Y) { ps_look_back(D, s_iv[j], a, b, s_gs[j], s_aw[j], ca, cb); known = true; }
#pragma unroll
                for (int x = 0; x < 5; x++)
#pragma unroll
                    for (int y = 0; y < 5; y++) cnt[5 * x + y] += (uint32_t)__popcll(La[x] & Lb[y]);
                cnt[25] += (uint32_t)__popcll(oa); cnt[26] += (uint32_t)__popcll(ob);
                cnt[27] += ps_runs(oa, Y, ca); cnt[28] += ps_runs(ob, Y, cb);
                cnt[29] += (uint32_t)__popcll(s_v[j] & ~Y);
            }
            if ((!carried || c == c1 - 1) && cur >= 0) ps_flush(out + ((size_t)(per_range ? cur : 0) * (size_t)P + (size_t)p) * PS_W, cnt);
        }
        __syncthreads();
    }
    if (bad) atomicOr(flag, bad);
}

}  // namespace

extern "C" {

int mauve_pair_stats(mauve_ctx *c, int64_t n_pair, const int32_t *pair_a, const int32_t *pair_b, int64_t n_range, const int64_t *range_iv,
                     const int64_t *range_col, const int64_t *range_len, int per_range, int64_t *stats)
{
    if (!c) return MAUVE_ERR_ARG;
    if (const int rs = ex_check_state(c, "pair_stats")) return rs;
    const int N = c->nseq;
    std::vector<int32_t> pairs;                              // the a of every pair, then the b
    if (!pair_a) {
        for (int a = 0; a < N; a++) for (int b = a + 1; b < N; b++) pairs.push_back(a);
        for (int a = 0; a < N; a++) for (int b = a + 1; b < N; b++) pairs.push_back(b);
    } else {
        if (n_pair < 1 || n_pair > PS_MAX_PAIRS || !pair_b) { c->err = "pair_stats: n_pair outside [1, 1024] or pair_b missing"; return MAUVE_ERR_ARG; }
        for (int64_t k = 0; k < n_pair; k++) {
            const int32_t a = pair_a[k], b = pair_b[k];
            if (a < 0 || a >= N || b < 0 || b >= N || a == b) { c->err = "pair_stats: pair " + std::to_string(k) + " holds an id outside [0, nseq) or one genome twice"; return MAUVE_ERR_ARG; }
        }
        pairs.assign(pair_a, pair_a + n_pair); pairs.insert(pairs.end(), pair_b, pair_b + n_pair);
    }
    const int P = (int)(pairs.size() / 2);
    // the record checks come before any device work; range arguments that ex_front will refuse are left to it: that refusal comes first
    const int64_t R = range_iv ? n_range : c->co.n_iv;
    const bool r_ok = R >= 0 && R < ((int64_t)1 << 31) && !(range_iv && R && (!range_col || !range_len));
    const int64_t n_rec = per_range && r_ok ? R * (int64_t)P : (int64_t)P;
    if (r_ok && n_rec > PS_MAX_RECORDS) { c->err = "pair_stats: more than 2^24 records"; return MAUVE_ERR_LIMIT; }
    if (r_ok && n_rec && !stats) { c->err = "pair_stats: stats is NULL"; return MAUVE_ERR_ARG; }
    ExFront F;                                               // the pair lists travel behind the ranges
    if (const int rf = ex_front<PsUnits>(c, "pair_stats", c->ps_work, n_range, range_iv, range_col, range_len, pairs.data(), pairs.size() * 4, &F)) return rf;
    const int64_t n_units = F.total;
    if (n_units >= ((int64_t)1 << 28)) { c->err = "pair_stats: the ranges hold 2^34 columns or more"; return MAUVE_ERR_LIMIT; }
    HIPCHK(c, c->ps_out.ensure((size_t)n_rec * PS_W * 8 + 64));
    unsigned long long *out = c->ps_out.as<unsigned long long>();
    if (n_rec) HIPCHK(c, hipMemsetAsync(out, 0, (size_t)n_rec * PS_W * 8, c->stream));
    if (n_units && P) {
        const int64_t n_chunks = (n_units + PS_UNITS - 1) / PS_UNITS, cps = (n_chunks + PS_MAX_SPANS - 1) / PS_MAX_SPANS, spans = (n_chunks + cps - 1) / cps;
        const int32_t *d_pairs = reinterpret_cast<const int32_t *>(F.tail);
        hipLaunchKernelGGL(ps_count, dim3((uint32_t)spans), dim3(256), 0, c->stream, *c->co.dev, F.G, R, F.d_iv, F.gstart, F.clen, F.off, n_units, cps, P, d_pairs, d_pairs + P,
                           per_range != 0, out, F.flag);
        HIPCHK(c, hipGetLastError());
        if (const int rf = co_flag_read(c, F.flag, "pair_stats", EX_OUTSIDE)) return rf;
    }
    if (const int rc = copy_to_caller(c, c->pin_stage, stats, out, (size_t)n_rec * PS_W * 8)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MAUVE_OK;
}

void mauve_pair_stats_identity(const int64_t *stats, int64_t n_rec, double *identity)
{
    for (int64_t k = 0; k < n_rec; k++) {
        const int64_t *s = stats + k * PS_W;
        int64_t both = 0;
        for (int q = 0; q < 25; q++) both += s[q];
        identity[k] = both > 0 ? (double)(s[0] + s[6] + s[12] + s[18] + s[24]) / (double)both : 0.0;
    }
}

void mauve_pair_stats_sp_score(const int64_t *stats, int64_t n_rec, const mauve_scoring *sc, int64_t *score)
{
    for (int64_t k = 0; k < n_rec; k++) {
        const int64_t *s = stats + k * PS_W;
        int64_t v = 0;
        for (int x = 0; x < 5; x++) for (int y = 0; y < 5; y++) v += s[5 * x + y] * (int64_t)sc->matrix[x < 4 ? x : 0][y < 4 ? y : 0];
        const int64_t runs = s[27] + s[28];
        score[k] = v + (int64_t)sc->gap_open * runs + (int64_t)sc->gap_extend * (s[25] + s[26] - runs);
    }
}

}  // extern "C"
