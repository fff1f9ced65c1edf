// seed_finish.hip -- the end of a seed pass, from the point where the candidates' records are in ctx->mlen / mstart: nothing here
// depends on the key or index width of the pass (seed_pass.hip), so it is compiled once.
//   pair_length_sums, bp_*      : the guide tree's view of the pairwise matches (sums of lengths, breakpoint estimate)
//   canon_keys, canon_gather    : the canonical order of large candidate sets on the device; small sets are sorted on the host
#include "common.hpp"
#include <algorithm>
#include <cstring>
#include <cstdlib>

// ------------------------------------------------------------------------------------------------
// canonical order on the device (large candidate sets): key = first component << pos_bits | |its start| per candidate
// (pos_bits = bits of the longest genome: fewer radix passes than a fixed 32)
// (dropped candidates get first component = nseq and sort behind everything), the radix sort of radix_sort.hip on
// (key, candidate index), then a gather of the surviving records as int64 in sorted order.
// ------------------------------------------------------------------------------------------------
// guide tree (progressive.cpp): all it needs of the pairwise matches is the sum of their lengths per genome pair -- no
// canonical order, no copy of the (hundreds of thousands of) records.  Block-level sums in LDS, then one atomic per pair.
__global__ void __launch_bounds__(256) pair_length_sums(const int32_t *__restrict__ mlen, const int32_t *__restrict__ mstart, uint32_t ncand,
                                                        int nseq, unsigned long long *__restrict__ sums)
{
    __shared__ unsigned long long s[MAUVE_MAX_SEQ * MAUVE_MAX_SEQ];
    for (int i = threadIdx.x; i < nseq * nseq; i += 256) s[i] = 0;
    __syncthreads();
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < ncand; i += gridDim.x * 256u) {
        const int32_t len = mlen[i];
        if (len == 0) continue;
        int a = -1, b = -1;
        for (int g = 0; g < nseq; g++) if (mstart[(size_t)i * nseq + g]) { if (a < 0) a = g; else if (b < 0) b = g; }
        if (b >= 0) atomicAdd(&s[a * nseq + b], (unsigned long long)len);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nseq * nseq; i += 256) if (s[i]) atomicAdd(&sums[i], s[i]);
}

// ---- pairwise breakpoint estimate (progressive.cpp scales node weights by it) ----
// Of every genome pair's matches (length >= min_len): order by position in the lower genome, rank by position in the higher one,
// and count the adjacencies that are not conserved.  Small kernels around three stable radix sorts of (pair, position) keys: by the
// higher genome first (position, strand), so that the order along the lower genome breaks its ties that way, then the ranks.
__device__ __forceinline__ bool bp_pair_of(const int32_t *__restrict__ st, int nseq, int *a, int *b)
{
    int x = -1, y = -1;
    for (int g = 0; g < nseq; g++) if (st[g]) { if (x < 0) x = g; else if (y < 0) y = g; }
    *a = x; *b = y;
    return y >= 0;
}
// which = 1: key by the higher genome (position, strand bit); 0: by the lower genome.  order == nullptr: record j itself (first sort:
// records that do not count get the pair id nseq * nseq, behind every pair).  vals: the record index (keep_record) or j.
__global__ void __launch_bounds__(256) bp_keys(const int32_t *__restrict__ mlen, const int32_t *__restrict__ mstart, const uint32_t *__restrict__ order, uint32_t n, int nseq,
                                               int pos_bits, int32_t min_len, int which, int keep_record, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                               uint32_t *__restrict__ n_valid)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    bool valid = false;
    if (j < n) {
        const uint32_t i = order ? order[j] : j;
        uint64_t key = (uint64_t)(nseq * nseq) << (pos_bits + 1);
        const int32_t len = mlen[i];
        int a, b;
        if (len != 0 && len >= min_len && bp_pair_of(mstart + (size_t)i * nseq, nseq, &a, &b)) {
            const int32_t sx = mstart[(size_t)i * nseq + (which ? b : a)];
            key = ((uint64_t)(a * nseq + b) << (pos_bits + 1)) | ((uint64_t)(sx < 0 ? -sx : sx) << 1) | (uint64_t)(sx < 0);
            valid = true;
        }
        keys[j] = key; vals[j] = keep_record ? i : j;
    }
    if (n_valid) { const uint64_t bal = __ballot(valid); if ((threadIdx.x & 63) == 0 && bal) atomicAdd(n_valid, (uint32_t)__popcll(bal)); }
}
__global__ void __launch_bounds__(256) bp_rank(const uint32_t *__restrict__ order_b, uint32_t nv, uint32_t *__restrict__ rank)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t < nv) rank[order_b[t]] = t;
}
__global__ void __launch_bounds__(256) bp_count(const uint64_t *__restrict__ keys_a, const uint32_t *__restrict__ order_a, const uint32_t *__restrict__ rank,
                                                const int32_t *__restrict__ mstart, uint32_t nv, int nseq, int pos_bits, unsigned long long *__restrict__ out)
{
    __shared__ uint32_t s[MAUVE_MAX_SEQ * MAUVE_MAX_SEQ];
    for (int i = threadIdx.x; i < nseq * nseq; i += 256) s[i] = 0;
    __syncthreads();
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j + 1 < nv; j += gridDim.x * 256u) {
        const uint32_t pair = (uint32_t)(keys_a[j] >> (pos_bits + 1));
        if ((uint32_t)(keys_a[j + 1] >> (pos_bits + 1)) != pair) continue;
        const uint32_t b = pair % (uint32_t)nseq;
        const int32_t s0 = mstart[(size_t)order_a[j] * nseq + b], s1 = mstart[(size_t)order_a[j + 1] * nseq + b];
        const uint32_t r0 = rank[j], r1 = rank[j + 1];
        const bool conserved = (s0 > 0 && s1 > 0 && r1 == r0 + 1) || (s0 < 0 && s1 < 0 && r1 + 1 == r0);
        if (!conserved) atomicAdd(&s[pair], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nseq * nseq; i += 256) if (s[i]) atomicAdd(&out[i], (unsigned long long)s[i]);
}

__global__ void __launch_bounds__(256) canon_keys(const int32_t *__restrict__ mlen, const int32_t *__restrict__ mstart, uint32_t ncand,
                                                  int nseq, int pos_bits, int inval, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                  uint32_t *__restrict__ n_valid)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool valid = false;
    if (i < ncand) {
        uint64_t key = (uint64_t)inval << pos_bits;                 // dropped candidates: behind every match
        if (mlen[i] != 0) {
            const int32_t *s = mstart + (size_t)i * nseq;
            int f = 0; while (f < nseq && s[f] == 0) f++;
            const uint32_t a = f < nseq ? (uint32_t)(s[f] < 0 ? -s[f] : s[f]) : 0u;
            key = ((uint64_t)f << pos_bits) | a;
            valid = true;
        }
        keys[i] = key; vals[i] = i;
    }
    const uint64_t b = __ballot(valid);
    if (b && (threadIdx.x & 63) == (uint32_t)(__ffsll((unsigned long long)b) - 1)) atomicAdd(n_valid, (uint32_t)__popcll(b));
}

// The number of surviving records is still on the device (*n_valid): the launch covers all candidates, the output is
// out[0 .. nm) lengths followed by nm * nseq starts.  Two neighbours with the same key (first component, start) are a
// tie the key alone does not order: *ties is raised and the host finishes the order (rare).
__global__ void __launch_bounds__(256) canon_gather(const int32_t *__restrict__ mlen, const int32_t *__restrict__ mstart,
                                                    const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                    const uint32_t *__restrict__ n_valid, int nseq, int64_t *__restrict__ out,
                                                    uint32_t *__restrict__ ties)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nm = *n_valid;
    if (r >= nm) return;
    int64_t *out_len = out, *out_start = out + nm;
    if (r > 0 && keys[r] == keys[r - 1]) atomicOr(ties, 1u);
    const uint32_t src = vals[r];
    out_len[r] = mlen[src];
    for (int g = 0; g < nseq; g++) out_start[(size_t)r * nseq + g] = mstart[(size_t)src * nseq + g];
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// bits of a position in the longest genome
static int pos_bits_of(const GenomeSet &gs)
{
    int64_t maxlen = 1; for (int g = 0; g < gs.nseq; g++) maxlen = std::max<int64_t>(maxlen, gs.lens[(size_t)g]);
    int pos_bits = 1; while (pos_bits < 32 && (1LL << pos_bits) <= maxlen) pos_bits++;
    return pos_bits;
}

// (key, candidate index) sort buffers.  (Own buffers: over several finder passes the candidates can outnumber the windows, so
// the sorted-mer buffers are not guaranteed to be big enough.)
static int ensure_canon_buffers(mauve_ctx *ctx, uint32_t ncand)
{
    HIPCHK(ctx, ctx->canon_k1.ensure((size_t)ncand * 8 + 64)); HIPCHK(ctx, ctx->canon_k2.ensure((size_t)ncand * 8 + 64));
    HIPCHK(ctx, ctx->canon_v1.ensure((size_t)ncand * 4 + 64)); HIPCHK(ctx, ctx->canon_v2.ensure((size_t)ncand * 4 + 64));
    return MAUVE_OK;
}

// an [N][N] table of 64-bit sums from the device into `out`
static int fetch_pair_table(mauve_ctx *ctx, const unsigned long long *d, int N, std::vector<int64_t> &out)
{
    HIPCHK(ctx, ctx->pin_seed.ensure(64 + (size_t)N * N * 8));
    HIPCHK(ctx, hipMemcpyAsync(ctx->pin_seed.as<char>() + 64, d, (size_t)N * N * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(out.data(), ctx->pin_seed.as<char>() + 64, (size_t)N * N * 8);
    return MAUVE_OK;
}

// the guide tree's view of the pairwise matches
static int pair_sums(mauve_ctx *ctx, int N, uint32_t ncand)
{
    ctx->pair_sums.assign((size_t)N * N, 0);
    if (!ncand) return MAUVE_OK;
    HIPCHK(ctx, ctx->run_sum.ensure((size_t)N * N * 8 + 64));
    unsigned long long *d = ctx->run_sum.as<unsigned long long>();
    HIPCHK(ctx, hipMemsetAsync(d, 0, (size_t)N * N * 8, ctx->stream));
    hipLaunchKernelGGL(pair_length_sums, dim3(std::min<uint32_t>((ncand + 255) / 256, 1024)), dim3(256), 0, ctx->stream, ctx->mlen.as<int32_t>(),
                       ctx->mstart.as<int32_t>(), ncand, N, d);
    HIPCHK(ctx, hipGetLastError());
    return fetch_pair_table(ctx, d, N, ctx->pair_sums);
}

// broken adjacencies per pair, from the same records
static int pair_breakpoints(mauve_ctx *ctx, const GenomeSet &gs, uint32_t ncand)
{
    const int N = gs.nseq;
    ctx->pair_bp.assign((size_t)N * N, 0);
    if (ncand < 2) return MAUVE_OK;
    if (int rc = ensure_canon_buffers(ctx, ncand)) return rc;
    HIPCHK(ctx, ctx->bp_work.ensure((size_t)ncand * 8 * 2 + (size_t)ncand * 4 * 3 + (size_t)N * N * 8 + 256));
    uint64_t *ck = ctx->canon_k1.as<uint64_t>(), *ck2 = ctx->canon_k2.as<uint64_t>();
    uint32_t *cv = ctx->canon_v1.as<uint32_t>(), *cv2 = ctx->canon_v2.as<uint32_t>();
    uint64_t *bk = ctx->bp_work.as<uint64_t>(), *bk2 = bk + ncand;
    uint32_t *bv = reinterpret_cast<uint32_t *>(bk2 + ncand), *bv2 = bv + ncand, *rank = bv2 + ncand;
    unsigned long long *dbp = reinterpret_cast<unsigned long long *>(ctx->bp_work.as<char>() + (((size_t)ncand * 28 + 63) & ~(size_t)63));
    const int32_t *mlen = ctx->mlen.as<int32_t>(), *mstart = ctx->mstart.as<int32_t>();
    HIPCHK(ctx, hipMemsetAsync(ctx->counters.p, 0, 64, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(dbp, 0, (size_t)N * N * 8, ctx->stream));
    const int pos_bits = pos_bits_of(gs);
    int pid_bits = 1; while ((1 << pid_bits) <= N * N) pid_bits++;
    const int32_t min_len = (int32_t)std::min<int64_t>(ctx->bp_min_len, INT32_MAX);
    const int kb = pos_bits + 1 + pid_bits;
    // 1. by the higher genome (position, strand): only to break the ties of the next order
    hipLaunchKernelGGL(bp_keys, dim3((ncand + 255) / 256), dim3(256), 0, ctx->stream, mlen, mstart, (const uint32_t *)nullptr, ncand, N,
                       pos_bits, min_len, 1, 1, ck, cv, ctx->counters.as<uint32_t>() + 3);
    HIPCHK(ctx, hipGetLastError());
    if (int rc = sort_pairs_u64(ctx, ncand, kb, &ck, &cv, ck2, cv2, MAUVE_K_CANON)) return rc;
    const uint32_t *cw;
    if (int rc = seed_counters(ctx, 16, &cw)) return rc;
    const uint32_t nv = cw[3];
    if (nv < 2) return MAUVE_OK;
    // 2. along the lower genome: record indices in that order (stable: ties stay in the order of 1.)
    hipLaunchKernelGGL(bp_keys, dim3((nv + 255) / 256), dim3(256), 0, ctx->stream, mlen, mstart, cv, nv, N, pos_bits, min_len, 0, 1,
                       bk, bv, (uint32_t *)nullptr);
    HIPCHK(ctx, hipGetLastError());
    uint64_t *ak = bk; uint32_t *av = bv;
    if (int rc = sort_pairs_u64(ctx, nv, kb, &ak, &av, bk2, bv2, MAUVE_K_CANON)) return rc;
    // 3. ranks along the higher genome (ties in the order of 2.); the canonical-sort buffers are free again
    uint64_t *sk = ctx->canon_k1.as<uint64_t>(); uint32_t *sv = ctx->canon_v1.as<uint32_t>();
    hipLaunchKernelGGL(bp_keys, dim3((nv + 255) / 256), dim3(256), 0, ctx->stream, mlen, mstart, av, nv, N, pos_bits, min_len, 1, 0,
                       sk, sv, (uint32_t *)nullptr);
    HIPCHK(ctx, hipGetLastError());
    if (int rc = sort_pairs_u64(ctx, nv, kb, &sk, &sv, ctx->canon_k2.as<uint64_t>(), ctx->canon_v2.as<uint32_t>(), MAUVE_K_CANON)) return rc;
    // (ak / av: the order along the lower genome, for the count)
    hipLaunchKernelGGL(bp_rank, dim3((nv + 255) / 256), dim3(256), 0, ctx->stream, sv, nv, rank);
    hipLaunchKernelGGL(bp_count, dim3(std::min<uint32_t>((nv + 255) / 256, 1024)), dim3(256), 0, ctx->stream, ak, av, rank, mstart, nv, N, pos_bits, dbp);
    HIPCHK(ctx, hipGetLastError());
    return fetch_pair_table(ctx, dbp, N, ctx->pair_bp);
}

// The rest of the canonical comparator behind (first component, |start|): component mask, starts, length.
// Both routes finish their rare equal-key groups with it (int64 records from the device, int32 records on the host).
template <typename T>
static bool tie_less(const T *a, T la, const T *b, T lb, int N)
{
    uint32_t ma = 0, mb = 0;
    for (int g = 0; g < N; g++) { if (a[g]) ma |= 1u << g; if (b[g]) mb |= 1u << g; }
    if (ma != mb) return ma < mb;
    for (int g = 0; g < N; g++) if (a[g] != b[g]) return a[g] < b[g];
    return la < lb;
}

// device route, after the copy-out: equal (first component, start) groups are ordered by the rest of the comparator (rare).
// Returns whether there was such a group.
static bool canon_repair_ties(mauve_ctx *ctx, int N, uint32_t nm)
{
    auto k1of = [&](uint32_t r) {
        const int64_t *st = &ctx->match_start[(size_t)r * N];
        int f = 0; while (f < N && st[f] == 0) f++;
        return ((uint64_t)f << 32) | (uint64_t)(f < N ? std::llabs(st[f]) : 0);
    };
    bool ties = false;
    uint64_t prev = k1of(0);
    for (uint32_t i = 0; i < nm;) {
        uint32_t j = i + 1; uint64_t kj = 0;
        while (j < nm && (kj = k1of(j)) == prev) j++;
        if (j - i > 1) {
            ties = true;
            const std::vector<int64_t> gl(&ctx->match_len[i], &ctx->match_len[i] + (j - i)), gs(&ctx->match_start[(size_t)i * N], &ctx->match_start[(size_t)i * N] + (size_t)(j - i) * N);
            std::vector<uint32_t> o(j - i);
            for (uint32_t r = 0; r < j - i; r++) o[r] = r;
            std::sort(o.begin(), o.end(), [&](uint32_t x, uint32_t y) { return tie_less(&gs[(size_t)x * N], gl[x], &gs[(size_t)y * N], gl[y], N); });
            for (uint32_t r = 0; r < j - i; r++) {
                ctx->match_len[i + r] = gl[o[r]];
                std::copy(&gs[(size_t)o[r] * N], &gs[(size_t)o[r] * N] + N, &ctx->match_start[(size_t)(i + r) * N]);
            }
        }
        prev = kj; i = j;
    }
    return ties;
}

// the nm records of ctx->sorted_rec into ctx->match_len / match_start
// (through page-locked staging: a pageable destination of tens of MB copies at a fraction of the link rate)
static int sorted_rec_to_host(mauve_ctx *ctx, size_t nm, int N)
{
    const size_t rbytes = nm * (1 + (size_t)N) * 8;
    HIPCHK(ctx, ctx->pin_seed.ensure(64 + rbytes));
    char *pin = ctx->pin_seed.as<char>() + 64;
    HIPCHK(ctx, hipMemcpyAsync(pin, ctx->sorted_rec.p, rbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->match_len.resize(nm); ctx->match_start.resize(nm * N);
    memcpy(ctx->match_len.data(), pin, nm * 8);
    memcpy(ctx->match_start.data(), pin + nm * 8, nm * N * 8);
    return MAUVE_OK;
}

// host copy of a match list the seed pass left on the device only (canon_device with lazy_matches_ok)
int seed_matches_to_host(mauve_ctx *ctx)
{
    if (!ctx->matches_pending) return MAUVE_OK;
    if (int rc = sorted_rec_to_host(ctx, (size_t)ctx->n_matches, ctx->match_nseq)) return rc;
    ctx->matches_pending = false;
    return MAUVE_OK;
}

// large sets: sort on the device, gather, copy out in order
static int canon_device(mauve_ctx *ctx, const GenomeSet &gs, const SeedRequest &rq, uint32_t ncand, double &trace_t0)
{
    const int N = gs.nseq;
    if (int rc = ensure_canon_buffers(ctx, ncand)) return rc;
    uint64_t *ck = ctx->canon_k1.as<uint64_t>(), *ck2 = ctx->canon_k2.as<uint64_t>();
    uint32_t *cv = ctx->canon_v1.as<uint32_t>(), *cv2 = ctx->canon_v2.as<uint32_t>();
    HIPCHK(ctx, hipMemsetAsync(ctx->counters.p, 0, 64, ctx->stream));
    const int pos_bits = pos_bits_of(gs);
    // the bits above the position hold the first component (0 .. N-1; N = dropped).  An N-way search (mask = every genome) only
    // has matches that start in genome 0: one bit tells them from the dropped ones, which at bacterial sizes saves a sort pass
    const bool nway_only = rq.mask != 0 && (uint32_t)rq.mask == full_mask(N) && rq.mode != MAUVE_MODE_PAIRWISE;
    int fbits = 1; if (!nway_only) while ((1 << fbits) <= N) fbits++;
    { KernelTimer t(ctx, MAUVE_K_CANON, ncand);
      hipLaunchKernelGGL(canon_keys, dim3((ncand + 255) / 256), dim3(256), 0, ctx->stream, ctx->mlen.as<int32_t>(),
                         ctx->mstart.as<int32_t>(), ncand, N, pos_bits, nway_only ? 1 : N, ck, cv, ctx->counters.as<uint32_t>() + 3); }
    HIPCHK(ctx, hipGetLastError());
    if (int rc = sort_pairs_u64(ctx, ncand, pos_bits + fbits, &ck, &cv, ck2, cv2, MAUVE_K_CANON)) return rc;
    HIPCHK(ctx, ctx->sorted_rec.ensure((size_t)ncand * (1 + N) * 8 + 64));
    hipLaunchKernelGGL(canon_gather, dim3((ncand + 255) / 256), dim3(256), 0, ctx->stream, ctx->mlen.as<int32_t>(),
                       ctx->mstart.as<int32_t>(), ck, cv, ctx->counters.as<uint32_t>() + 3, N, ctx->sorted_rec.as<int64_t>(),
                       ctx->counters.as<uint32_t>() + 4);
    HIPCHK(ctx, hipGetLastError());
    const uint32_t *cw;
    if (int rc = seed_counters(ctx, 32, &cw)) return rc;
    const uint32_t nm = cw[3];
    const bool dev_ties = cw[4] != 0;
    if (ctx->lazy_matches_ok && nm && !dev_ties) {
        // the caller keeps working on the device copy (sorted_rec); the host copy is made when somebody asks for it
        ctx->match_len.clear(); ctx->match_start.clear();
        ctx->matches_pending = true; ctx->match_nseq = N;
        ctx->n_matches = nm; ctx->dev_rec_n = (int64_t)nm;
        if (rq.n_matches) *rq.n_matches = nm;
        seed_trace(ctx, "canonical sort (device, list stays)", trace_t0);
        return MAUVE_OK;
    }
    ctx->match_len.resize(nm); ctx->match_start.resize((size_t)nm * N);
    ctx->n_matches = nm;
    if (nm) {
        if (int rc = sorted_rec_to_host(ctx, nm, N)) return rc;
        if (canon_repair_ties(ctx, N, nm)) {
            // the host finished the order inside the tie groups: the device copy follows (the chaining stages read it)
            char *pin = ctx->pin_seed.as<char>() + 64;
            memcpy(pin, ctx->match_len.data(), (size_t)nm * 8);
            memcpy(pin + (size_t)nm * 8, ctx->match_start.data(), (size_t)nm * N * 8);
            HIPCHK(ctx, hipMemcpyAsync(ctx->sorted_rec.p, pin, (size_t)nm * (1 + N) * 8, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
    }
    ctx->dev_rec_n = (int64_t)nm;                          // sorted_rec holds the list in canonical order
    if (rq.n_matches) *rq.n_matches = nm;
    seed_trace(ctx, "canonical sort (device)", trace_t0);
    return MAUVE_OK;
}

// small sets: records to the host (page-locked staging), host sort
static int canon_host(mauve_ctx *ctx, int N, const SeedRequest &rq, uint32_t ncand, bool on_host, double &trace_t0)
{
    std::vector<int32_t> &hl = ctx->sdh.hl, &hs = ctx->sdh.hs;
    if (!on_host) {
        hl.resize(ncand); hs.resize((size_t)ncand * N);
        const size_t lbytes = ((size_t)ncand * 4 + 63) & ~(size_t)63, sbytes = (size_t)ncand * 4 * N;
        HIPCHK(ctx, ctx->pin_seed.ensure(64 + lbytes + sbytes));
        char *pin = ctx->pin_seed.as<char>() + 64;
        HIPCHK(ctx, hipMemcpyAsync(pin, ctx->mlen.p, (size_t)ncand * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(pin + lbytes, ctx->mstart.p, sbytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        memcpy(hl.data(), pin, (size_t)ncand * 4);
        memcpy(hs.data(), pin + lbytes, sbytes);
        seed_trace(ctx, "records copy", trace_t0);
    }
    std::vector<uint32_t> &order = ctx->sdh.order; order.clear(); order.reserve(ncand);
    std::vector<uint64_t> &k1 = ctx->sdh.k1; k1.resize(ncand);   // (first component, |start|) packed for a fast first-level compare
    for (uint32_t i = 0; i < ncand; i++) {
        if (hl[i] == 0) continue;
        order.push_back(i);
        const int32_t *s = &hs[(size_t)i * N];
        int f = 0; while (f < N && s[f] == 0) f++;
        uint64_t a = f < N ? (uint64_t)std::abs((int64_t)s[f]) : 0;
        k1[i] = ((uint64_t)f << 40) | a;
    }
    const uint32_t nm = (uint32_t)order.size();
    {   // LSD radix sort of the record indices by k1 (first component << 40 | start): 4 passes of 12 bits,
        // then the rare equal-k1 groups are ordered with the full comparator
        std::vector<uint32_t> &tmp = ctx->sdh.tmp; tmp.resize(nm);
        uint32_t *src = order.data(), *dst = tmp.data();
        for (int pass = 0; pass < 4; pass++) {
            const int sh = 12 * pass;
            uint32_t cnt[4097] = {0};
            for (uint32_t i = 0; i < nm; i++) cnt[(((k1[src[i]] & 0xffffffffULL) | ((k1[src[i]] >> 40) << 32)) >> sh & 4095) + 1]++;
            for (int b = 0; b < 4096; b++) cnt[b + 1] += cnt[b];
            for (uint32_t i = 0; i < nm; i++) dst[cnt[((k1[src[i]] & 0xffffffffULL) | ((k1[src[i]] >> 40) << 32)) >> sh & 4095]++] = src[i];
            std::swap(src, dst);
        }
        if (src != order.data()) std::copy(src, src + nm, order.data());
        auto full_less = [&](uint32_t x, uint32_t y) { return tie_less(&hs[(size_t)x * N], hl[x], &hs[(size_t)y * N], hl[y], N); };
        for (uint32_t i = 0; i < nm;) {
            uint32_t j = i + 1;
            while (j < nm && k1[order[j]] == k1[order[i]]) j++;
            if (j - i > 1) std::sort(order.begin() + i, order.begin() + j, full_less);
            i = j;
        }
    }
    ctx->match_len.resize(nm); ctx->match_start.resize((size_t)nm * N);
    for (uint32_t i = 0; i < nm; i++) {
        uint32_t o = order[i];
        ctx->match_len[i] = hl[o];
        for (int g = 0; g < N; g++) ctx->match_start[(size_t)i * N + g] = hs[(size_t)o * N + g];
    }
    ctx->n_matches = nm;
    if (rq.n_matches) *rq.n_matches = nm;
    seed_trace(ctx, "canonical sort", trace_t0);
    return MAUVE_OK;
}

int seed_finish(mauve_ctx *ctx, const GenomeSet &gs, const SeedRequest &rq, uint32_t ncand, bool on_host, double &trace_t0)
{
    if (ctx->pair_sums_only) {
        if (int rc = pair_sums(ctx, gs.nseq, ncand)) return rc;
        seed_trace(ctx, "pair length sums", trace_t0);
        if (ctx->bp_min_len < 0) return MAUVE_OK;
        if (int rc = pair_breakpoints(ctx, gs, ncand)) return rc;
        seed_trace(ctx, "pair breakpoints", trace_t0);
        return MAUVE_OK;
    }
    if (ncand == 0) return MAUVE_OK;
    // ---- canonical order (first component, |start|, mask, starts, length) ----
    if (ncand >= (uint32_t)switches().canon_device_min) return canon_device(ctx, gs, rq, ncand, trace_t0);
    return canon_host(ctx, gs.nseq, rq, ncand, on_host, trace_t0);
}
