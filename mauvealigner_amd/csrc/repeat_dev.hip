// repeat_dev.hip -- extended repeat matches of ONE genome: the repeat map behind mauveAligner --repeats
// (mauveAligner.cpp:480-483, RepeatHash::FindMatches), the single-genome counterpart of the ungapped extension of S4.
//   rm_extract : the genome's windows -> (canonical masked mer, global window index | strand); an invalid window (contig join,
//                ambiguous base) gets the all-ones key
//   (radix_sort.hip: stable sort by the mer -- a family is a run of the list, its windows in ascending position)
//   rm_table   : per window the family size, saturated at 255, and the strand flag; the family heads with a multiplicity in range
//   (dev_scan.hpp: the heads compacted in list order, with the offsets of their starts)
//   rm_extend  : one wave per head walks the family's diagonal, 64 offsets a round (seed_dev.hpp: the walk of mum_extend)
//   (dev_scan.hpp / radix_sort.hip: the slots of dropped heads removed, the records sorted by start 0, the CSR offsets)
//   rm_write   : the records in that order
// Every launch is sized by a count the host has read; the kernels use plain loads, stores and LDS.
#include "common.hpp"
#include "dev_scan.hpp"
#include "radix_sort.hpp"
#include "seed_dev.hpp"

static_assert(MAUVE_REPEAT_MAX_MULT == MAUVE_MAX_SEQ, "a family's components fill the ExtComp table of the walk (ext_mismatch: MAUVE_MAX_SEQ entries)");
static_assert(MAUVE_REPEAT_MAX_MULT < 255, "rm_table's count saturates at 255: a candidate's multiplicity must be exact");

template <typename KeyT, typename ValT>
__global__ void __launch_bounds__(256) rm_extract(const uint64_t *__restrict__ G, const uint64_t *__restrict__ VM, const uint64_t *__restrict__ CM,
                                                  SeedShape sh, uint32_t nw, uint32_t gpos0, KeyT *__restrict__ keys, ValT *__restrict__ vals)
{
    const SeedRuns<false> runs(sh);
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < nw; p += gridDim.x * 256u) {
        const MerKey m = mer_at<false>(G, p, runs);
        keys[p] = window_blocked(VM, CM, p, sh.span) ? (KeyT)~0ULL : (KeyT)m.key;      // (no canonical mer is all ones: min(F, R) is never all T)
        vals[p] = win_make<ValT>(gpos0 + p, m.strand);
    }
}

// wtab[w]: bits 0-7 the size of window w's family, saturated at 255 (0: invalid window), bit 8 its strand flag.  emit[i]: the multiplicity
// of the family whose head is list entry i when it is a hit (lo_m <= m <= hi_m), else 0.
constexpr uint32_t RM_STRAND = 0x100u;
template <typename KeyT, typename ValT>
__global__ void __launch_bounds__(256) rm_table(const KeyT *__restrict__ keys, const ValT *__restrict__ vals, uint32_t n, uint32_t gpos0,
                                                uint32_t lo_m, uint32_t hi_m, uint16_t *__restrict__ wtab, uint32_t *__restrict__ emit)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const KeyT k = keys[i];
        const ValT v = vals[i];
        const uint32_t w = win_idx(v) - gpos0;
        if (k == (KeyT)~0ULL) { wtab[w] = 0; emit[i] = 0; continue; }
        uint32_t back = 0, fwd = 1;                            // the walks stop at the saturation count
        for (uint32_t j = i; j > 0 && back < 254u && keys[j - 1] == k; j--) back++;
        for (uint32_t j = i + 1; j < n && back + fwd < 255u && keys[j] == k; j++) fwd++;
        const uint32_t c = back + fwd;
        wtab[w] = (uint16_t)(c | (win_strand(v) ? RM_STRAND : 0u));
        emit[i] = (back == 0 && c >= lo_m && c <= hi_m) ? c : 0u;
    }
}

struct RmEmit { const uint32_t *e; __device__ uint32_t value(uint32_t i) const { return e[i]; } };
// the hits in list order: head entry, multiplicity, offset of its starts; tot[0] hits, tot[1] their starts
struct RmCand {
    const uint32_t *em, *soff; uint32_t n, cap; uint32_t *cand, *cmult, *coff, *tot;
    __device__ uint32_t domain(int) const { return n; }
    __device__ bool flag(uint32_t i, int) const { return em[i] != 0; }
    __device__ void each(uint32_t, uint32_t, bool, int) const {}
    __device__ void emit(uint32_t i, uint32_t r, int) const { if (r < cap) { cand[r] = i; cmult[r] = em[i]; coff[r] = soff[i]; } }
    __device__ void total(uint32_t hits, int) const { tot[0] = hits; tot[1] = soff[n]; }
};
// the slots the extension kept (length != 0): sort key = start 0 (0-based; component 0 is forward), value = slot; tot[2] records
struct RmKeep {
    const int32_t *rlen, *rstart; const uint32_t *coff; uint32_t ncand; uint32_t *skey, *sval, *tot;
    __device__ uint32_t domain(int) const { return ncand; }
    __device__ bool flag(uint32_t ci, int) const { return rlen[ci] != 0; }
    __device__ void each(uint32_t, uint32_t, bool, int) const {}
    __device__ void emit(uint32_t ci, uint32_t r, int) const { skey[r] = (uint32_t)(rstart[coff[ci]] - 1); sval[r] = ci; }
    __device__ void total(uint32_t recs, int) const { tot[2] = recs; }
};
struct RmMultOf { const uint32_t *cmult, *sval; __device__ int64_t value(uint32_t s) const { return cmult[sval[s]]; } };

// One wave per hit.  The family's m windows, entries i0 .. i0 + m - 1 of the sorted list, are the components: ascending
// position, component c reverse iff its strand flag differs from component 0's.  The walk is mum_extend's; what differs is the range of
// admissible offsets -- beside the genome's ends, the offsets at which two components that walk towards each other have not yet met or
// passed (the position order of the windows stays that of k = 0) -- and the test for another hit of the diagonal met on the left:
// the window of component 0 at that offset belongs to a family of exactly m windows (then: the diagonal's windows there) whose strand
// relations are the diagonal's (they differ only for a mer that is its own reverse complement: all flags 0; one reversed component decides).
// rlen[ci] = 0: dropped, another hit of the diagonal emits the cluster.  rounds[ci]: 64-offset rounds this hit took.
template <typename ValT>
__global__ void __launch_bounds__(256) rm_extend(const uint64_t *__restrict__ G, const uint64_t *__restrict__ VM, const uint64_t *__restrict__ CM,
                                                 SeedShape sh, uint32_t nw, uint32_t gpos0, const ValT *__restrict__ vals,
                                                 const uint16_t *__restrict__ wtab, const uint32_t *__restrict__ cand,
                                                 const uint32_t *__restrict__ cmult, const uint32_t *__restrict__ coff, uint32_t ncand,
                                                 int32_t *__restrict__ rlen, int32_t *__restrict__ rstart, uint32_t *__restrict__ rounds)
{
    __shared__ ExtComp s_comp[4][MAUVE_REPEAT_MAX_MULT];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t wave_global = (blockIdx.x * 256u + threadIdx.x) >> 6, nwaves = gridDim.x * 4u;
    ExtComp *comp = s_comp[wv];
    const bool masks = VM || CM;
    for (uint32_t ci = wave_global; ci < ncand; ci += nwaves) {
        const uint32_t i0 = cand[ci];
        const int m = (int)min(cmult[ci], (uint32_t)MAUVE_REPEAT_MAX_MULT);
        const uint32_t s0 = win_strand(vals[i0]);
        if (lane < m) {
            const ValT v = vals[i0 + lane];
            ExtComp C;
            C.G = G; C.VM = VM; C.CM = CM;
            C.pos = (int64_t)(win_idx(v) - gpos0);
            C.rev = win_strand(v) ^ s0; C.g = (uint32_t)lane; C.pad = 0;
            C.lo = 0; C.hi = (int64_t)nw - 1;
            C.maxw = (uint32_t)(((uint64_t)nw + (uint32_t)sh.span - 1 + 31) / 32 + 2);       // mauve_packed_words - 1
            comp[lane] = C;
        }
        __threadfence_block();          // the table is read by every lane of this wave
        // admissible offsets: every window inside the genome, and no two neighbours that walk towards each other meet (neighbours in
        // position order suffice: between a forward component and a reverse one behind it lies a neighbouring pair of that kind, no further apart)
        int64_t kmin = INT64_MIN, kmax = INT64_MAX;
        for (int c = 0; c < m; c++) {
            const ExtComp &C = comp[c];
            kmin = max(kmin, C.rev ? C.pos - C.hi : C.lo - C.pos); kmax = min(kmax, C.rev ? C.pos - C.lo : C.hi - C.pos);
            if (c + 1 < m && comp[c + 1].rev != C.rev) {
                const int64_t d = comp[c + 1].pos - C.pos;     // > 0; the sign of d - 2k (forward first) / d + 2k (reverse first) must stay
                if (C.rev) kmin = max(kmin, -((d - 1) >> 1)); else kmax = min(kmax, (d - 1) >> 1);
            }
        }
        const uint32_t revset = (uint32_t)__ballot(lane < m && comp[min(lane, m - 1)].rev != 0u);
        const int rev_at = revset ? __ffs(revset) - 1 : -1;                                    // a component on the other strand, if there is one
        const int64_t p0 = comp[0].pos, prv = comp[max(rev_at, 0)].pos;
        uint32_t nround = 0;
        // the first round of either walk: offsets -64 .. -1 and 1 .. 64, fetched together
        uint64_t M2[2][4];
        { const int64_t jj[2] = {-64, 1}; ext_mismatch<2>(comp, m, sh.span, jj, lane, M2); }
        // ---- left walk: offsets cur-1 .. cur-64 per round ----
        int64_t cur = 0;
        bool leftmost = true;
        for (bool done = false; !done;) {
            const int64_t k = cur - 1 - lane;
            const int64_t hq = p0 + k;
            const uint32_t tw = (hq >= 0 && hq < (int64_t)nw) ? wtab[hq] : 0u;
            nround++;
            uint64_t M1[1][4];
            if (cur != 0) { const int64_t jj[1] = {cur - 64}; ext_mismatch<1>(comp, m, sh.span, jj, lane, M1); }
            else { for (int q = 0; q < 4; q++) M1[0][q] = M2[0][q]; }
            bool a = k >= kmin && k <= kmax && ext_window_clean(M1[0], 63 - lane, sh);
            if (masks) a = a && !ext_blocked(comp, m, sh.span, k);
            const bool hh = a && (tw & 255u) == (uint32_t)m;
            const uint64_t A = __ballot(a), H = __ballot(hh);
            const int p = walk_round(A, sh.span, done);                          // offsets consumed in this round
            uint64_t Hv = H & (p >= 64 ? ~0ULL : ((1ULL << p) - 1ULL));
            if (Hv && rev_at >= 0) {
                bool met = false;
                for (; Hv && !met; Hv &= Hv - 1) {
                    const int64_t kk = cur - (int64_t)__ffsll((unsigned long long)Hv);       // an admissible offset: both windows inside the genome
                    met = ((wtab[p0 + kk] ^ wtab[prv - kk]) & RM_STRAND) != 0u;
                }
                Hv = met;
            }
            if (Hv) { leftmost = false; done = true; }
            cur -= p;
            if (p == 0) done = true;                   // (p == 0 only happens with done set; keeps cur != 0 a valid "not the first round" test)
        }
        if (!leftmost) {
            if (lane == 0) { rlen[ci] = 0; rounds[ci] = nround; }
            __threadfence_block(); continue;
        }
        const int64_t klo = cur;
        // ---- right walk ----
        cur = 0;
        for (bool done = false; !done;) {
            const int64_t k = cur + 1 + lane;
            nround++;
            uint64_t M1[1][4];
            if (cur != 0) { const int64_t jj[1] = {cur + 1}; ext_mismatch<1>(comp, m, sh.span, jj, lane, M1); }
            else { for (int q = 0; q < 4; q++) M1[0][q] = M2[1][q]; }
            bool a = k >= kmin && k <= kmax && ext_window_clean(M1[0], lane, sh);
            if (masks) a = a && !ext_blocked(comp, m, sh.span, k);
            const uint64_t A = __ballot(a);
            const int p = walk_round(A, sh.span, done);
            cur += p;
        }
        const int64_t khi = cur;
        if (lane == 0) { rlen[ci] = (int32_t)(khi - klo) + sh.span; rounds[ci] = nround; }
        if (lane < m) {
            const ExtComp &C = comp[lane];
            rstart[(size_t)coff[ci] + lane] = C.rev ? (int32_t)(-(C.pos - khi + 1)) : (int32_t)(C.pos + klo + 1);
        }
        __threadfence_block();          // the next candidate overwrites the table
    }
}

// record s of the result = slot sval[s]: length, multiplicity, its starts behind start_off[s]
__global__ void __launch_bounds__(256) rm_write(const uint32_t *__restrict__ sval, uint32_t nrec, const int32_t *__restrict__ rlen,
                                                const int32_t *__restrict__ rstart, const uint32_t *__restrict__ cmult,
                                                const uint32_t *__restrict__ coff, const int64_t *__restrict__ start_off,
                                                int64_t *__restrict__ length, int64_t *__restrict__ mult, int64_t *__restrict__ starts)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= nrec) return;
    const uint32_t ci = sval[s], m = cmult[ci];
    length[s] = rlen[ci]; mult[s] = m;
    const int32_t *src = rstart + coff[ci];
    int64_t *dst = starts + start_off[s];
    for (uint32_t c = 0; c < m; c++) dst[c] = src[c];
}

namespace {
struct RmPass {
    mauve_ctx *c; SeedShape sh; uint32_t nw, gpos0; const uint64_t *G, *VM, *CM; uint32_t lo_m, hi_m;
};

template <typename KeyT, typename ValT>
int rm_pass(const RmPass &P)
{
    using namespace devscan;
    mauve_ctx *c = P.c; const uint32_t n = P.nw;
    double t0 = now_ms();
    HIPCHK(c, c->keysA.ensure((size_t)n * sizeof(KeyT))); HIPCHK(c, c->keysB.ensure((size_t)n * sizeof(KeyT)));
    HIPCHK(c, c->valsA.ensure((size_t)n * sizeof(ValT))); HIPCHK(c, c->valsB.ensure((size_t)n * sizeof(ValT)));
    KeyT *keys = c->keysA.as<KeyT>(); ValT *vals = c->valsA.as<ValT>();
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)n + 255) / 256, (uint64_t)c->cus * 16);
    { KernelTimer t(c, MAUVE_K_EXTRACT, n);
      hipLaunchKernelGGL((rm_extract<KeyT, ValT>), dim3(grid), dim3(256), 0, c->stream, P.G, P.VM, P.CM, P.sh, n, P.gpos0, keys, vals); }
    HIPCHK(c, hipGetLastError());
    // the mer bits, or the whole key when there are invalid windows: their all-ones keys end the list
    const int key_bits = (P.VM || P.CM) ? (int)sizeof(KeyT) * 8 : 2 * P.sh.weight;
    if (int rc = sort_pairs<KeyT, ValT>(c, n, key_bits, &keys, &vals, c->keysB.as<KeyT>(), c->valsB.as<ValT>(), false)) return rc;
    seed_trace(c, "repeat map: sort", t0);

    // work area: wtab[n] u16 | emit[n] | soff[n + 1] | cand, cmult, coff [cap] | bsum[nb] | bcnt[nb] | tot[4]
    const uint32_t nb = (n + TILE - 1) / TILE, cap = n / 2 + 1;
    const size_t o_emit = up64((size_t)n * 2), o_soff = o_emit + up64((size_t)n * 4), o_cand = o_soff + up64(((size_t)n + 1) * 4),
                 o_cmult = o_cand + up64((size_t)cap * 4), o_coff = o_cmult + up64((size_t)cap * 4), o_bsum = o_coff + up64((size_t)cap * 4),
                 o_bcnt = o_bsum + up64((size_t)nb * 4), o_tot = o_bcnt + up64((size_t)nb * 4);
    HIPCHK(c, c->rm_work.ensure(o_tot + 64));
    char *W = c->rm_work.as<char>();
    uint16_t *wtab = reinterpret_cast<uint16_t *>(W);
    uint32_t *emit = reinterpret_cast<uint32_t *>(W + o_emit), *soff = reinterpret_cast<uint32_t *>(W + o_soff),
             *cand = reinterpret_cast<uint32_t *>(W + o_cand), *cmult = reinterpret_cast<uint32_t *>(W + o_cmult),
             *coff = reinterpret_cast<uint32_t *>(W + o_coff), *bsum = reinterpret_cast<uint32_t *>(W + o_bsum),
             *bcnt = reinterpret_cast<uint32_t *>(W + o_bcnt), *tot = reinterpret_cast<uint32_t *>(W + o_tot);
    HIPCHK(c, hipMemsetAsync(tot, 0, 64, c->stream));
    hipLaunchKernelGGL((rm_table<KeyT, ValT>), dim3(grid), dim3(256), 0, c->stream, keys, vals, n, P.gpos0, P.lo_m, P.hi_m, wtab, emit);
    hipLaunchKernelGGL((vscan_partial<uint32_t, RmEmit>), dim3(nb), dim3(256), 0, c->stream, RmEmit{emit}, n, bsum);
    hipLaunchKernelGGL((vscan_write<uint32_t, RmEmit>), dim3(nb), dim3(256), 0, c->stream, RmEmit{emit}, n, bsum, soff, (uint32_t *)nullptr);
    const RmCand rc_{emit, soff, n, cap, cand, cmult, coff, tot};
    hipLaunchKernelGGL((cmp_count<RmCand>), dim3(nb), dim3(256), 0, c->stream, rc_, bcnt);
    hipLaunchKernelGGL((cmp_write<RmCand>), dim3(nb), dim3(256), 0, c->stream, rc_, bcnt);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, c->pin_stage.ensure(64));
    uint32_t *ht = c->pin_stage.as<uint32_t>();
    HIPCHK(c, hipMemcpyAsync(ht, tot, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint32_t ncand = std::min(ht[0], cap), nst = ht[1];
    seed_trace(c, "repeat map: families", t0);
    c->rm.n = 0; c->rm.ns = 0;
    if (ncand == 0) { HIPCHK(c, c->rm_res.ensure(64)); HIPCHK(c, hipMemsetAsync(c->rm_res.p, 0, 8, c->stream)); return MAUVE_OK; }

    // extension: slot records (int32) in the seed pass's record buffers, the rounds behind the lengths
    HIPCHK(c, c->mlen.ensure((size_t)ncand * 8)); HIPCHK(c, c->mstart.ensure((size_t)nst * 4));
    int32_t *rlen = c->mlen.as<int32_t>(), *rstart = c->mstart.as<int32_t>();
    uint32_t *rounds = c->mlen.as<uint32_t>() + ncand;
    { KernelTimer t(c, MAUVE_K_EXTEND, ncand);
      const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)ncand + 3) / 4, (uint64_t)c->cus * 32);
      hipLaunchKernelGGL((rm_extend<ValT>), dim3(blocks), dim3(256), 0, c->stream, P.G, P.VM, P.CM, P.sh, n, P.gpos0, vals, wtab, cand, cmult, coff,
                         ncand, rlen, rstart, rounds); }
    HIPCHK(c, hipGetLastError());
    // the kept slots, keyed by start 0
    const uint32_t nbc = (ncand + TILE - 1) / TILE;        // (<= nb: bcnt holds them)
    HIPCHK(c, c->canon_k1.ensure((size_t)ncand * 4 + 64)); HIPCHK(c, c->canon_k2.ensure((size_t)ncand * 4 + 64));
    HIPCHK(c, c->canon_v1.ensure((size_t)ncand * 4 + 64)); HIPCHK(c, c->canon_v2.ensure((size_t)ncand * 4 + 64));
    uint32_t *skey = c->canon_k1.as<uint32_t>(), *sval = c->canon_v1.as<uint32_t>();
    const RmKeep rk{rlen, rstart, coff, ncand, skey, sval, tot};
    hipLaunchKernelGGL((cmp_count<RmKeep>), dim3(nbc), dim3(256), 0, c->stream, rk, bcnt);
    hipLaunchKernelGGL((cmp_write<RmKeep>), dim3(nbc), dim3(256), 0, c->stream, rk, bcnt);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(ht, tot, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint32_t nrec = std::min(ht[2], ncand);
    seed_trace(c, "repeat map: extension", t0);
    if (switches().trace) {
        std::vector<uint32_t> hr(ncand);
        HIPCHK(c, hipMemcpy(hr.data(), rounds, (size_t)ncand * 4, hipMemcpyDeviceToHost));
        uint64_t sum = 0; uint32_t mx = 0;
        for (uint32_t r : hr) { sum += r; mx = std::max(mx, r); }
        fprintf(stderr, "[trace] repeat map: %u windows, %u hits, %u records, %llu rounds, most rounds of one hit %u\n", n, ncand, nrec, (unsigned long long)sum, mx);
    }
    if (nrec == 0) { HIPCHK(c, c->rm_res.ensure(64)); HIPCHK(c, hipMemsetAsync(c->rm_res.p, 0, 8, c->stream)); return MAUVE_OK; }
    // canonical order: stable sort on start 0 (ties are finished by the fetch), then the CSR
    int kb = 1; while (kb < 32 && ((uint64_t)n >> kb)) kb++;
    if (int rc = sort_pairs<uint32_t, uint32_t>(c, nrec, kb, &skey, &sval, c->canon_k2.as<uint32_t>(), c->canon_v2.as<uint32_t>(), false, MAUVE_K_CANON)) return rc;
    HIPCHK(c, c->rm_res.ensure(((size_t)nrec * 3 + 1 + nst) * 8 + 64));
    int64_t *d_len = c->rm_res.as<int64_t>(), *d_mult = d_len + nrec, *d_off = d_mult + nrec, *d_starts = d_off + nrec + 1;
    const uint32_t nbr = (nrec + TILE - 1) / TILE;
    int64_t *bsum64 = reinterpret_cast<int64_t *>(W + o_soff);        // (soff has served; nbr <= nb / 2 + 1 int64 fit n + 1 words)
    hipLaunchKernelGGL((vscan_partial<int64_t, RmMultOf>), dim3(nbr), dim3(256), 0, c->stream, RmMultOf{cmult, sval}, nrec, bsum64);
    hipLaunchKernelGGL((vscan_write<int64_t, RmMultOf>), dim3(nbr), dim3(256), 0, c->stream, RmMultOf{cmult, sval}, nrec, bsum64, d_off, (int64_t *)nullptr);
    hipLaunchKernelGGL(rm_write, dim3((nrec + 255) / 256), dim3(256), 0, c->stream, sval, nrec, rlen, rstart, cmult, coff, d_off, d_len, d_mult, d_starts);
    HIPCHK(c, hipGetLastError());
    int64_t *h64 = c->pin_stage.as<int64_t>();
    HIPCHK(c, hipMemcpyAsync(h64, d_off + nrec, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->rm.n = nrec; c->rm.ns = h64[0];
    seed_trace(c, "repeat map: order", t0);
    return MAUVE_OK;
}
}  // namespace

int repeat_matches(mauve_ctx *c, int seq, uint64_t pattern, int64_t min_multi, int64_t max_multi)
{
    const GenomeSet gs = main_genome_set(c);
    RmPass P; P.c = c;
    if (!make_seed_shape(pattern, &P.sh)) { c->err = "seed pattern must be palindromic, span <= 49, weight <= 31"; return MAUVE_ERR_ARG; }
    if (max_multi > MAUVE_REPEAT_MAX_MULT || max_multi < 2) { c->err = "repeat_matches: max_multi outside [2, MAUVE_REPEAT_MAX_MULT = 32]"; return MAUVE_ERR_ARG; }
    if (gs.nseq < 1) { c->err = "no genomes set"; return MAUVE_ERR_STATE; }
    if (seq < 0 || seq >= gs.nseq) { c->err = "sequence index out of range"; return MAUVE_ERR_ARG; }
    if (int rc = refuse_past_2g(c, "repeat_matches")) return rc;
    c->rm.valid = false;
    // the global window numbering of the seed pass (its sort values; MAUVE_WIDE_INDEX widens them here as there)
    int64_t total = 0, before = 0;
    for (int g = 0; g < gs.nseq; g++) { const int64_t w = std::max<int64_t>(0, gs.lens[(size_t)g] - P.sh.span + 1); if (g < seq) before += w; total += w; }
    const int64_t nw = std::max<int64_t>(0, gs.lens[(size_t)seq] - P.sh.span + 1);
    P.nw = (uint32_t)nw; P.gpos0 = (uint32_t)before;
    P.G = gs.buf->as<uint64_t>() + gs.word_off[(size_t)seq];
    P.VM = gs.vmask ? gs.vmask->as<uint64_t>() + gs.mask_off[(size_t)seq] : nullptr;
    P.CM = gs.cmask ? gs.cmask->as<uint64_t>() + gs.mask_off[(size_t)seq] : nullptr;
    P.lo_m = (uint32_t)std::min<int64_t>(std::max<int64_t>(2, min_multi), 256); P.hi_m = (uint32_t)max_multi;
    c->rm.n = 0; c->rm.ns = 0;
    if (nw > 0) {
        const bool wide = seedpass_wide(total);
        int rc;
        if (2 * P.sh.weight <= 32) rc = wide ? rm_pass<uint32_t, uint64_t>(P) : rm_pass<uint32_t, uint32_t>(P);
        else rc = wide ? rm_pass<uint64_t, uint64_t>(P) : rm_pass<uint64_t, uint32_t>(P);
        if (rc) return rc;
    }
    c->rm.valid = true; c->rm.genome_gen = c->genome_gen;
    return MAUVE_OK;
}

// The records come off the device ordered by start 0; the rest of the canonical order (multiplicity, the signed starts, length) is made
// here inside the groups of equal start 0, which are rare and short.
int repeat_fetch(mauve_ctx *c, int64_t *length, int64_t *mult, int64_t *start_off, int64_t *starts)
{
    if (!c->rm.valid || c->rm.genome_gen != c->genome_gen) { c->err = "repeat_fetch: no repeat result in force (mauve_repeat_matches first; a genome upload ends it)"; return MAUVE_ERR_STATE; }
    const size_t n = (size_t)c->rm.n, ns = (size_t)c->rm.ns;
    if (!start_off || (n && (!length || !mult)) || (ns && !starts)) { c->err = "repeat_fetch: null output"; return MAUVE_ERR_ARG; }
    if (n == 0) { start_off[0] = 0; return MAUVE_OK; }
    const int64_t *d_len = c->rm_res.as<int64_t>(), *d_mult = d_len + n, *d_off = d_mult + n, *d_starts = d_off + n + 1;
    if (int rc = copy_to_caller(c, c->pin_stage, length, d_len, n * 8)) return rc;
    if (int rc = copy_to_caller(c, c->pin_stage, mult, d_mult, n * 8)) return rc;
    if (int rc = copy_to_caller(c, c->pin_stage, start_off, d_off, (n + 1) * 8)) return rc;
    if (int rc = copy_to_caller(c, c->pin_stage, starts, d_starts, ns * 8)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<size_t> idx; std::vector<int64_t> tl, tm, ts;
    for (size_t a = 0; a < n;) {
        size_t b = a + 1;
        while (b < n && starts[start_off[b]] == starts[start_off[a]]) b++;
        if (b - a > 1) {
            idx.resize(b - a);
            for (size_t i = 0; i < b - a; i++) idx[i] = a + i;
            std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) {
                if (mult[x] != mult[y]) return mult[x] < mult[y];
                const int64_t *sx = starts + start_off[x], *sy = starts + start_off[y];
                for (int64_t k = 0; k < mult[x]; k++) if (sx[k] != sy[k]) return sx[k] < sy[k];
                return length[x] < length[y];
            });
            tl.clear(); tm.clear(); ts.clear();
            for (size_t i : idx) { tl.push_back(length[i]); tm.push_back(mult[i]); ts.insert(ts.end(), starts + start_off[i], starts + start_off[i + 1]); }
            int64_t o = start_off[a];
            std::copy(ts.begin(), ts.end(), starts + o);
            for (size_t i = 0; i < b - a; i++) { length[a + i] = tl[i]; mult[a + i] = tm[i]; start_off[a + i] = o; o += tm[i]; }
        }
        a = b;
    }
    return MAUVE_OK;
}
