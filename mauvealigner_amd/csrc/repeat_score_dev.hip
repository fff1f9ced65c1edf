// repeat_score_dev.hip -- a repeat map scored against a correct alignment of the copies of its repeats: the three figures of
// the reference's scoreProcrastAlignment (scoreProcrastAlignment.cpp:120-364, compareAlignmentsAceD) from the truth index of S17 (co_truth, its
// rows the copy slots of a repeat family) and a list of ungapped multi-component matches in the layout of mauve_repeat_fetch -- a caller's
// list, or the result of the last mauve_repeat_matches where it lies (rm_res).  No genome data is read.
//   rs_order    (resident form only) a thread per record: its place inside its group of equal start 0 by the fetch's rule, counted against
//               the group's other records (the groups are rare and short); then the scan of the multiplicities in that order (dev_scan.hpp)
//               and  rs_gather, which moves the starts: the list as mauve_repeat_fetch would hand it out, without leaving the device
//   rs_extents  a thread per component: its record by a search of start_off, its extent [|start|, |start| + length - 1], the entries checked
//   fo_keys, the project's sort, vmax over FoHi (interval_join.hpp, dev_scan.hpp): S21's join -- the extents sorted by their left end with
//               the prefix maximum of the right ends, all under genome 0
//   rs_count    a wave per 64-column word of T, a lane per column, tiled as sc_count is.  The lane keeps the genome position of every row at
//               its column in LDS (0: gapped or absent) and the rows' reverse flags in a register.  For every row i with a residue it stabs
//               the extents at q_i once -- the upper bound among the left ends, then backward while the prefix maximum reaches q_i -- and for
//               every covering (record, c1) reads the record's <= 32 components from the CSR and tests them against q_j of every row j > i
//               that has a residue: orientation, then the column.  Pairs found go into two bit masks over j; a ballot and a popcount per
//               (i, j) and figure go into an LDS table [N][N][4] of 32-bit counters, which leaves with one 64-bit atomic per non-zero
//               counter at the workgroup's end.  Hit bits are set with atomicOr, and only where the word read does not have them yet.
//               The walk is divergent and latency-bound: every lane follows its own chain of dependent loads and the wave waits for the
//               longest; one extent that spans many short ones makes every query under it walk back over them (as in S21).
//   rs_totals   the population counts of the two hit tables, the sums of mult and of m (m - 1) / 2, the column sums of the pair table
// Every index formed into T, the sorted table or the CSR is checked before it becomes a load (CO_BAD_INDEX); no workgroup waits for another.
// All counts are integers and every update commutes: two calls return identical bytes.
#include "common.hpp"
#include "coord_index.hpp"
#include "dev_scan.hpp"
#include "interval_join.hpp"
#include <algorithm>
#include <cstring>

namespace {

constexpr int RS_W = 4;                           // words per row pair: possible, truepos, exact, 0
constexpr int RS_MAX_GROUPS = 4096;               // workgroups of rs_count at the most
constexpr int RS_MAX_MULT = MAUVE_REPEAT_MAX_MULT;
static_assert(RS_MAX_MULT <= 32 && MAUVE_MAX_SEQ <= 32, "components and rows are bits of 32-bit words");

// the list on the device: the CSR, and the extents sorted by their left end (keys: the left end under genome 0; vals: the component's
// place in starts; pmax: the running maximum of the right ends; hi, rec: per component, unsorted)
struct RsMap {
    const int64_t *len, *mult, *off, *starts;
    const unsigned long long *keys, *pmax; const uint32_t *vals, *rec; const int64_t *hi;
    int64_t n, M;
};

__device__ __forceinline__ int64_t rs_abs(int64_t s) { return s < 0 ? -s : s; }

// the fetch's order inside a group of equal start 0: multiplicity, the signed starts, length (repeat_dev.hip, repeat_fetch)
__device__ bool rs_less(const int64_t *len, const int64_t *mult, const int64_t *off, const int64_t *starts, int64_t x, int64_t y)
{
    if (mult[x] != mult[y]) return mult[x] < mult[y];
    const int64_t *sx = starts + off[x], *sy = starts + off[y];
    for (int64_t k = 0; k < mult[x]; k++) if (sx[k] != sy[k]) return sx[k] < sy[k];
    return len[x] < len[y];
}

__device__ __forceinline__ bool rs_rec_ok(const int64_t *mult, const int64_t *off, int64_t r, int64_t ns)
{
    const int64_t o = off[r], m = mult[r];
    return o >= 0 && m >= 2 && m <= RS_MAX_MULT && o + m <= ns;
}

__global__ void __launch_bounds__(256) rs_order(int64_t n, int64_t ns, const int64_t *__restrict__ len, const int64_t *__restrict__ mult, const int64_t *__restrict__ off,
                                                const int64_t *__restrict__ starts, uint32_t *__restrict__ dest, int64_t *__restrict__ nlen, int64_t *__restrict__ nmult,
                                                uint32_t *__restrict__ flag)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    int64_t d = r; bool ok = rs_rec_ok(mult, off, r, ns);
    if (ok) {
        const int64_t s0 = starts[off[r]];
        int64_t a = r, b = r + 1;
        while (ok && a > 0) { if (!rs_rec_ok(mult, off, a - 1, ns)) ok = false; else if (starts[off[a - 1]] == s0) a--; else break; }
        while (ok && b < n) { if (!rs_rec_ok(mult, off, b, ns)) ok = false; else if (starts[off[b]] == s0) b++; else break; }
        if (ok) {
            int64_t rank = 0;
            for (int64_t g = a; g < b; g++)
                if (g != r && (rs_less(len, mult, off, starts, g, r) || (g < r && !rs_less(len, mult, off, starts, r, g)))) rank++;
            d = a + rank;
        }
    }
    dest[r] = (uint32_t)d; nlen[d] = len[r]; nmult[d] = ok ? mult[r] : 0;
    if (!ok) atomicOr(flag, CO_BAD_INDEX);
}

struct RsMult { const int64_t *m; __device__ int64_t value(uint32_t i) const { return m[i]; } };

__global__ void __launch_bounds__(256) rs_gather(int64_t n, int64_t ns, const int64_t *__restrict__ mult, const int64_t *__restrict__ off, const int64_t *__restrict__ starts,
                                                 const uint32_t *__restrict__ dest, const int64_t *__restrict__ noff, int64_t *__restrict__ nstarts, uint32_t *__restrict__ flag)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int64_t d = dest[r];
    if (d < 0 || d >= n || !rs_rec_ok(mult, off, r, ns) || noff[d] < 0 || noff[d] + mult[r] > ns) { atomicOr(flag, CO_BAD_INDEX); return; }
    for (int64_t c = 0; c < mult[r]; c++) nstarts[noff[d] + c] = starts[off[r] + c];
}

// component t of the list: its record and its extent as an entry of the join's table (genome 0)
__global__ void __launch_bounds__(256) rs_extents(int64_t n, int64_t M, const int64_t *__restrict__ len, const int64_t *__restrict__ off, const int64_t *__restrict__ starts,
                                                  int32_t *__restrict__ seq, int64_t *__restrict__ lo, int64_t *__restrict__ hi, uint32_t *__restrict__ rec, uint32_t *__restrict__ flag)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= M) return;
    int64_t a = 0, e = n;                                      // the last record whose components start at or before t
    while (e - a > 1) { const int64_t mid = (a + e) >> 1; if (off[mid] <= t) a = mid; else e = mid; }
    const int64_t o = off[a], m = off[a + 1] - o, l = len[a], s = starts[t];
    int64_t x = 0, y = 0; uint32_t bad = 0;                    // (an entry fo_keys refuses: lo < 1)
    if (t < o || t - o >= m || m < 2 || m > RS_MAX_MULT || l < 1 || s == 0) bad = CO_BAD_ARG;
    else if (rs_abs(s) >= FM_MAX_POS || l >= FM_MAX_POS) { x = 1; y = FM_MAX_POS; }      // fo_keys raises FM_LIMIT
    else { x = rs_abs(s); y = x + l - 1; }
    seq[t] = 0; lo[t] = x; hi[t] = y; rec[t] = (uint32_t)a;
    if (bad) atomicOr(flag, bad);
}

// LDS: the table [N * N * 4] of counters, then the rows' genome positions [4 waves][N][64 lanes] (0: no residue of that row in the lane's column)
__global__ void __launch_bounds__(256) rs_count(CoordDev T, RsMap C, const int64_t *__restrict__ row_off, int64_t n_cols, int64_t n_words, int64_t wpg,
                                                unsigned long long *__restrict__ pairs, uint32_t *comp_hit, uint32_t *pair_hit, uint32_t *__restrict__ flag)
{
    extern __shared__ uint32_t s_mem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, N = T.N;
    const int n_cnt = N * N * RS_W;
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
        const bool ok = valid && x / CO_BLOCK < T.nb1;
        if (valid && !ok) bad |= CO_BAD_INDEX;
        uint32_t rev = 0;                                      // bit g: row g is reversed in the lane's interval
        for (int g = 0; g < N; g++) {
            uint32_t p = 0;
            if (ok) {
                CoordIv I; bool present; int64_t k;
                if (co_column(T, a, x, g, &I, &present, &k) && present) {
                    const int64_t q = co_residue(I, k);
                    if (k < 0 || q < I.left || q > I.right) bad |= CO_BAD_INDEX;
                    else if (q + row_off[g] >= FM_MAX_POS) bad |= FM_LIMIT;
                    else { p = (uint32_t)(q + row_off[g]); rev |= (uint32_t)(I.col0_rev & 1) << g; }
                }
            }
            s_pos[g * 64 + lane] = p;                          // (a lane reads back only what it wrote itself)
        }
        for (int i = 0; i + 1 < N; i++) {
            const int64_t qi = s_pos[i * 64 + lane];
            if (!__ballot(qi != 0)) continue;
            uint32_t have = 0, tp = 0, ex = 0;                 // bits j > i: the truth pair exists, is supported, is supported exactly
            if (qi) for (int j = i + 1; j < N; j++) if (s_pos[j * 64 + lane]) have |= 1u << j;
            if (have && C.M) {
                int64_t lb = 0, ub = C.M;                      // the first extent that starts behind q_i
                while (lb < ub) { const int64_t mid = (lb + ub) >> 1; if ((int64_t)(C.keys[mid] & FO_POS) <= qi) lb = mid + 1; else ub = mid; }
                for (int64_t s = lb; s > 0;) {
                    --s;
                    if ((int64_t)(C.pmax[s] & FO_POS) < qi) break;       // no extent at or before s reaches q_i
                    const int64_t t = C.vals[s];
                    if (t >= C.M) { bad |= CO_BAD_INDEX; continue; }
                    const int64_t lo1 = (int64_t)(C.keys[s] & FO_POS), hi1 = C.hi[t];
                    if (hi1 < qi) continue;
                    const int64_t r = C.rec[t];
                    if (r >= C.n) { bad |= CO_BAD_INDEX; continue; }
                    const int64_t o = C.off[r], m = C.off[r + 1] - o, c1 = t - o;
                    if (o < 0 || m < 2 || m > RS_MAX_MULT || o + m > C.M || c1 < 0 || c1 >= m) { bad |= CO_BAD_INDEX; continue; }
                    const int64_t l = C.len[r], st1 = C.starts[t];
                    if (rs_abs(st1) != lo1 || lo1 + l - 1 != hi1) { bad |= CO_BAD_INDEX; continue; }
                    const bool neg1 = st1 < 0;
                    const int64_t col1 = neg1 ? hi1 - qi : qi - lo1;
                    uint32_t hit = 0;
                    for (int c2 = 0; c2 < (int)m; c2++) {
                        if (c2 == (int)c1) continue;
                        const int64_t st2 = C.starts[o + c2], l2 = rs_abs(st2), r2 = l2 + l - 1;
                        const bool neg2 = st2 < 0;
                        for (uint32_t hb = have; hb; hb &= hb - 1) {
                            const int j = __ffs(hb) - 1;
                            const int64_t qj = s_pos[j * 64 + lane];
                            if (qj < l2 || qj > r2) continue;
                            if ((neg1 == neg2) != ((((rev >> i) ^ (rev >> j)) & 1u) == 0)) continue;        // the chain holds the pair, the strand is wrong
                            tp |= 1u << j;
                            if ((neg2 ? r2 - qj : qj - l2) == col1) ex |= 1u << j;
                            hit |= 1u << c2;
                            const int ca = min((int)c1, c2), cb = max((int)c1, c2);
                            if (!(pair_hit[o + ca] >> cb & 1u)) atomicOr(&pair_hit[o + ca], 1u << cb);
                        }
                    }
                    if (hit) { hit |= 1u << c1; if ((comp_hit[r] & hit) != hit) atomicOr(&comp_hit[r], hit); }
                }
            }
            for (int j = i + 1; j < N; j++) {
                const uint64_t m0 = __ballot(have >> j & 1u);
                if (!m0) continue;
                const uint64_t m1 = __ballot(tp >> j & 1u), m2 = __ballot(ex >> j & 1u);
                if (lane < 3) {                                // (the popcount of a ballot is one scalar instruction)
                    const uint32_t v = (uint32_t)__popcll(lane == 0 ? m0 : lane == 1 ? m1 : m2);
                    if (v) atomicAdd(&s_tab[(i * N + j) * RS_W + lane], v);
                }
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < n_cnt; t += 256) {
        const uint32_t v = s_tab[t];
        if (v) atomicAdd(&pairs[t], (unsigned long long)v);
    }
    if (bad) atomicOr(flag, bad);
}

// tot: sp_possible, sp_truepos, sp_exact, components, components_hit, component_pairs, component_pairs_hit, 0
__global__ void __launch_bounds__(256) rs_totals(int64_t n, int64_t M, int n_pair_words, const int64_t *__restrict__ mult, const uint32_t *__restrict__ comp_hit,
                                                 const uint32_t *__restrict__ pair_hit, const unsigned long long *__restrict__ pairs, unsigned long long *__restrict__ tot)
{
    __shared__ unsigned long long s_tot[8];
    if (threadIdx.x < 8) s_tot[threadIdx.x] = 0;
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n) {
        const unsigned long long m = (unsigned long long)mult[t];
        atomicAdd(&s_tot[3], m); atomicAdd(&s_tot[5], m * (m - 1) / 2);
        if (const uint32_t h = comp_hit[t]) atomicAdd(&s_tot[4], (unsigned long long)__popc(h));
    }
    if (t < M) if (const uint32_t h = pair_hit[t]) atomicAdd(&s_tot[6], (unsigned long long)__popc(h));
    if (t < n_pair_words && (t & 3) < 3) if (const unsigned long long v = pairs[t]) atomicAdd(&s_tot[t & 3], v);
    __syncthreads();
    if (threadIdx.x < 7 && s_tot[threadIdx.x]) atomicAdd(&tot[threadIdx.x], s_tot[threadIdx.x]);
}

const char *const RS_OUTSIDE = "a record of the list lies outside its domain (mult outside [2, 32], length < 1 or a zero start)";

// the caller's list judged on the host, where it lies: the refusals name the record
int rs_check_list(mauve_ctx *c, int64_t n, const int64_t *length, const int64_t *mult, const int64_t *start_off, const int64_t *starts)
{
    int64_t acc = 0;
    bool limit = false;
    for (int64_t r = 0; r < n; r++) {
        const auto who = [r] { return "repeat_score: record " + std::to_string(r); };       // (made for a refusal only: the loop runs over every start)
        if (mult[r] < 2 || mult[r] > RS_MAX_MULT) { c->err = who() + " has multiplicity " + std::to_string(mult[r]) + " outside [2, 32]"; return MAUVE_ERR_ARG; }
        if (start_off[r] != acc) { c->err = who() + ": start_off is not the prefix sum of mult"; return MAUVE_ERR_ARG; }
        if (length[r] < 1) { c->err = who() + " has a length below 1"; return MAUVE_ERR_ARG; }
        for (int64_t k = 0; k < mult[r]; k++) {
            const int64_t s = starts[acc + k];
            if (s == 0) { c->err = who() + " has a zero start (component " + std::to_string(k) + ")"; return MAUVE_ERR_ARG; }
            if (s <= -FM_MAX_POS || s >= FM_MAX_POS || length[r] >= FM_MAX_POS || (s < 0 ? -s : s) + length[r] - 1 >= FM_MAX_POS) limit = true;
        }
        acc += mult[r];
    }
    if (n && start_off[n] != acc) { c->err = "repeat_score: record " + std::to_string(n - 1) + ": start_off is not the prefix sum of mult (its last entry)"; return MAUVE_ERR_ARG; }
    if (limit) { c->err = "repeat_score: a position of 2^31 or more"; return MAUVE_ERR_LIMIT; }
    return MAUVE_OK;
}

}  // namespace

extern "C" int mauve_repeat_score(mauve_ctx *c, int64_t n, const int64_t *length, const int64_t *mult, const int64_t *start_off, const int64_t *starts,
                                  const int64_t *row_offset, mauve_repeat_score_totals *totals, int64_t *pair_records, uint32_t *comp_hit, uint32_t *pair_hit)
{
    if (!c) return MAUVE_ERR_ARG;
    if (!totals) { c->err = "repeat_score: totals is NULL"; return MAUVE_ERR_ARG; }
    const bool resident = length == nullptr;
    if (resident && (mult || start_off || starts)) { c->err = "repeat_score: length is NULL (the resident result) but other arrays of a list are given"; return MAUVE_ERR_ARG; }
    const mauve_ctx::CoordIndex &XT = c->co_truth;
    if (!XT.valid) { c->err = "repeat_score: no correct alignment in this context (mauve_score_truth first)"; return MAUVE_ERR_STATE; }
    int64_t M = 0;
    if (resident) {
        if (!c->rm.valid || c->rm.genome_gen != c->genome_gen) { c->err = "repeat_score: no repeat result in force (mauve_repeat_matches first; a genome upload ends it)"; return MAUVE_ERR_STATE; }
        n = c->rm.n; M = c->rm.ns;
    } else {
        if (n < 0 || (n && (!mult || !start_off || !starts))) { c->err = "repeat_score: missing arrays of the list"; return MAUVE_ERR_ARG; }
        if (n > FM_MAX_N) { c->err = "repeat_score: more than 2^24 records"; return MAUVE_ERR_LIMIT; }
        if (const int rc = rs_check_list(c, n, length, mult, start_off, starts)) return rc;
        M = n ? start_off[n] : 0;
    }
    const int N = XT.N;
    int64_t h_off[MAUVE_MAX_SEQ] = {0};
    for (int g = 0; row_offset && g < N; g++) {
        if (row_offset[g] < 0) { c->err = "repeat_score: row_offset of row " + std::to_string(g) + " is negative"; return MAUVE_ERR_ARG; }
        if (row_offset[g] >= FM_MAX_POS) { c->err = "repeat_score: a position of 2^31 or more (row_offset of row " + std::to_string(g) + ")"; return MAUVE_ERR_LIMIT; }
        h_off[g] = row_offset[g];
    }
    const size_t nr = (size_t)n, nc = (size_t)M, pw = (size_t)N * N * RS_W;
    const uint32_t tiles = (uint32_t)((nc + devscan::TILE - 1) / devscan::TILE), rtiles = (uint32_t)((nr + devscan::TILE - 1) / devscan::TILE);
    // work area: flag | totals | row offsets | pair table | comp_hit | pair_hit  (zeroed, in one piece)  | length | mult | start_off | starts |
    // seq, lo, hi, rec of the extents | keys x 2 | values x 2 | prefix maxima | tile maxima | the resident form's places and tile sums
    const size_t w_tot = 64, w_ro = w_tot + 64, w_pairs = w_ro + up64(MAUVE_MAX_SEQ * 8), w_ch = w_pairs + up64(pw * 8), w_ph = w_ch + up64(nr * 4), w_zero = w_ph + up64(nc * 4),
                 w_len = w_zero, w_mult = w_len + up64(nr * 8), w_off = w_mult + up64(nr * 8), w_st = w_off + up64((nr + 1) * 8), w_seq = w_st + up64(nc * 8),
                 w_lo = w_seq + up64(nc * 4), w_hi = w_lo + up64(nc * 8), w_rec = w_hi + up64(nc * 8), w_k1 = w_rec + up64(nc * 4), w_k2 = w_k1 + up64(nc * 8),
                 w_v1 = w_k2 + up64(nc * 8), w_v2 = w_v1 + up64(nc * 4), w_pm = w_v2 + up64(nc * 4), w_bm = w_pm + up64(nc * 8), w_dest = w_bm + up64((size_t)tiles * 8),
                 w_bs = w_dest + up64(nr * 4), w_total = w_bs + up64((size_t)rtiles * 8);
    const bool direct = resident || n == 0 || (host_pointer_is_pinned(length) && host_pointer_is_pinned(mult) && host_pointer_is_pinned(start_off) && host_pointer_is_pinned(starts));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->rs_work.ensure(w_total));
    HIPCHK(c, c->pin_stage.ensure(256 + up64(MAUVE_MAX_SEQ * 8) + (direct ? 0 : 2 * up64(nr * 8) + up64((nr + 1) * 8) + up64(nc * 8))));
    char *wk = c->rs_work.as<char>();
    uint32_t *flag = reinterpret_cast<uint32_t *>(wk), *d_ch = reinterpret_cast<uint32_t *>(wk + w_ch), *d_ph = reinterpret_cast<uint32_t *>(wk + w_ph);
    unsigned long long *d_tot = reinterpret_cast<unsigned long long *>(wk + w_tot), *d_pairs = reinterpret_cast<unsigned long long *>(wk + w_pairs);
    int64_t *d_len = reinterpret_cast<int64_t *>(wk + w_len), *d_mult = reinterpret_cast<int64_t *>(wk + w_mult), *d_off = reinterpret_cast<int64_t *>(wk + w_off),
            *d_st = reinterpret_cast<int64_t *>(wk + w_st), *d_hi = reinterpret_cast<int64_t *>(wk + w_hi);
    HIPCHK(c, hipMemsetAsync(wk, 0, w_zero, c->stream));
    size_t used = 256;
    if (const int r0 = fm_put(c, wk + w_ro, h_off, MAUVE_MAX_SEQ * 8, false, &used)) return r0;
    if (resident && n) {
        const int64_t *s_len = c->rm_res.as<int64_t>(), *s_mult = s_len + n, *s_off = s_mult + n, *s_st = s_off + n + 1;
        uint32_t *dest = reinterpret_cast<uint32_t *>(wk + w_dest);
        int64_t *bs = reinterpret_cast<int64_t *>(wk + w_bs);
        hipLaunchKernelGGL(rs_order, dim3((uint32_t)((nr + 255) / 256)), dim3(256), 0, c->stream, n, M, s_len, s_mult, s_off, s_st, dest, d_len, d_mult, flag);
        const RsMult in{d_mult};
        hipLaunchKernelGGL((devscan::vscan_partial<int64_t, RsMult>), dim3(rtiles), dim3(256), 0, c->stream, in, (uint32_t)nr, bs);
        hipLaunchKernelGGL((devscan::vscan_write<int64_t, RsMult>), dim3(rtiles), dim3(256), 0, c->stream, in, (uint32_t)nr, bs, d_off, (int64_t *)nullptr);
        hipLaunchKernelGGL(rs_gather, dim3((uint32_t)((nr + 255) / 256)), dim3(256), 0, c->stream, n, M, s_mult, s_off, s_st, dest, d_off, d_st, flag);
        HIPCHK(c, hipGetLastError());
    } else if (n) {
        if (const int r1 = fm_put(c, d_len, length, nr * 8, direct, &used)) return r1;
        if (const int r2 = fm_put(c, d_mult, mult, nr * 8, direct, &used)) return r2;
        if (const int r3 = fm_put(c, d_off, start_off, (nr + 1) * 8, direct, &used)) return r3;
        if (const int r4 = fm_put(c, d_st, starts, nc * 8, direct, &used)) return r4;
    }
    RsMap Cm{d_len, d_mult, d_off, d_st, nullptr, nullptr, nullptr, reinterpret_cast<const uint32_t *>(wk + w_rec), d_hi, n, M};
    if (M) {
        unsigned long long *keys = reinterpret_cast<unsigned long long *>(wk + w_k1), *pmax = reinterpret_cast<unsigned long long *>(wk + w_pm);
        uint32_t *vals = reinterpret_cast<uint32_t *>(wk + w_v1);
        hipLaunchKernelGGL(rs_extents, dim3((uint32_t)((nc + 255) / 256)), dim3(256), 0, c->stream, n, M, d_len, d_off, d_st, reinterpret_cast<int32_t *>(wk + w_seq),
                           reinterpret_cast<int64_t *>(wk + w_lo), d_hi, reinterpret_cast<uint32_t *>(wk + w_rec), flag);
        hipLaunchKernelGGL(fo_keys, dim3((uint32_t)((nc + 255) / 256)), dim3(256), 0, c->stream, M, reinterpret_cast<const int32_t *>(wk + w_seq),
                           reinterpret_cast<const int64_t *>(wk + w_lo), d_hi, keys, vals, flag);
        HIPCHK(c, hipGetLastError());
        uint64_t *k = reinterpret_cast<uint64_t *>(keys);
        if (const int rs = sort_pairs_u64(c, (uint32_t)nc, 31, &k, &vals, reinterpret_cast<uint64_t *>(wk + w_k2), reinterpret_cast<uint32_t *>(wk + w_v2), MAUVE_K_MISC)) return rs;
        keys = reinterpret_cast<unsigned long long *>(k);
        const FoHi in{keys, vals, d_hi};
        unsigned long long *bm = reinterpret_cast<unsigned long long *>(wk + w_bm);
        hipLaunchKernelGGL((devscan::vmax_partial<unsigned long long, FoHi>), dim3(tiles), dim3(256), 0, c->stream, in, (uint32_t)nc, bm);
        hipLaunchKernelGGL((devscan::vmax_write<unsigned long long, FoHi>), dim3(tiles), dim3(256), 0, c->stream, in, (uint32_t)nc, bm, pmax);
        Cm.keys = keys; Cm.pmax = pmax; Cm.vals = vals;
    }
    const int64_t n_cols = XT.n_cols, n_words = (n_cols + 63) / 64;
    if (n_words) {
        // a counter gains at most one per column: a workgroup's span stays below 2^32 columns
        const int64_t wpg = std::max<int64_t>(4, (n_words + RS_MAX_GROUPS - 1) / RS_MAX_GROUPS), groups = (n_words + wpg - 1) / wpg;
        if (wpg >= ((int64_t)1 << 26)) { c->err = "repeat_score: the correct alignment is too long"; return MAUVE_ERR_LIMIT; }
        const size_t lds = (pw + (size_t)4 * N * 64) * 4;
        hipLaunchKernelGGL(rs_count, dim3((uint32_t)groups), dim3(256), lds, c->stream, *XT.dev, Cm, reinterpret_cast<const int64_t *>(wk + w_ro), n_cols, n_words, wpg, d_pairs,
                           d_ch, d_ph, flag);
    }
    const size_t most = std::max(std::max(nr, nc), pw);
    hipLaunchKernelGGL(rs_totals, dim3((uint32_t)((most + 255) / 256)), dim3(256), 0, c->stream, n, M, (int)pw, d_mult, d_ch, d_ph, d_pairs, d_tot);
    HIPCHK(c, hipGetLastError());
    // the one round trip: the flag and the totals (behind the list's upload on the same stream, so the staging is free again)
    char *hb = c->pin_stage.as<char>();
    HIPCHK(c, hipMemcpyAsync(hb, wk, 128, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (const int rf = fm_flag_result(c, *reinterpret_cast<const uint32_t *>(hb), "repeat_score", RS_OUTSIDE)) return rf;
    memcpy(totals, hb + 64, sizeof *totals);
    if (pair_records) if (const int r5 = copy_to_caller(c, c->pin_stage, pair_records, d_pairs, pw * 8)) return r5;
    if (comp_hit && n) if (const int r6 = copy_to_caller(c, c->pin_stage, comp_hit, d_ch, nr * 4)) return r6;
    if (pair_hit && M) if (const int r7 = copy_to_caller(c, c->pin_stage, pair_hit, d_ph, nc * 4)) return r7;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MAUVE_OK;
}
