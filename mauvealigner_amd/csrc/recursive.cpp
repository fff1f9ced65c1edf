// recursive.cpp -- recursive anchoring of long inter-anchor gaps (Aligner::align's recursion on gaps longer
// than min_recursive_gap_length, mauveAligner.cpp:127,670-672,899; default 200).  Frozen spec: DESIGN.md S8.
//
// MI355X-first shape: instead of one small seed search per gap, every gap of a recursion level that
// wants the same seed weight is searched in ONE batched seed pass.  The gap sub-sequences (in LCB
// orientation) are concatenated per genome into a virtual genome set; the kernels run in segmented mode
// (seed_pass.hip): keys carry the gap id, windows may not straddle gaps, extension stops at gap ends.
// The per-gap chaining that follows (forward-only filter, overlap elimination, collinear LCB) runs on the
// device for large batches and gap by gap on the host for small ones.
//
// recursive_anchoring is the level loop over the stages of a batch (rec_deal .. rec_exchange); whichever way a batch
// is chained, it leaves one list of survivors (RecSurvivors) for one consumer (rec_emit).  Pure steps: recursion_host.hpp.
#include "common.hpp"
#include "recursion_host.hpp"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>

namespace {

// Virtual genomes of one recursion batch, built on the device from the resident packed genomes: thread (g, j)
// writes packed word j of virtual genome g -- 32 bases, each looked up through the segment table (which gap it
// belongs to) and the gap's source range; reverse gaps are read backwards and complemented.  Pad words are zero.
struct RecGatherArgs {
    uint64_t src_word_off[MAUVE_MAX_SEQ];   // genome g's words inside the resident genome buffer
    uint64_t dst_word_off[MAUVE_MAX_SEQ];   // virtual genome g's words inside rec_genomes
    uint64_t dst_words[MAUVE_MAX_SEQ];      // including the 3 pad words
};

__global__ void __launch_bounds__(256) rec_gather(const uint64_t *__restrict__ genomes, uint64_t *__restrict__ out, RecGatherArgs ga,
                                                  const uint32_t *__restrict__ seg, const int64_t *__restrict__ glo0,
                                                  const uint8_t *__restrict__ grev, uint32_t K)
{
    const int g = blockIdx.y;
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= ga.dst_words[g]) return;
    const uint32_t *sg = seg + (size_t)g * (K + 1);
    const uint32_t tot = sg[K];
    const uint64_t base0 = j * 32;
    uint64_t word = 0;
    if (base0 < tot) {
        // last k with sg[k] <= base0: the (non-empty) gap that holds base0
        uint32_t lo = 0, hi = K;
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (sg[mid] <= base0) lo = mid; else hi = mid; }
        uint32_t k = lo;
        const uint64_t *G = genomes + ga.src_word_off[g];
        for (int b = 0; b < 32; b++) {
            const uint64_t p = base0 + b;
            if (p >= tot) break;
            while (p >= sg[k + 1]) k++;                       // steps over empty gaps as well
            const int64_t off = (int64_t)(p - sg[k]), len = (int64_t)(sg[k + 1] - sg[k]), s0 = glo0[(size_t)g * K + k];
            const bool rev = grev[(size_t)g * K + k] != 0;
            const int64_t src = rev ? s0 + len - 1 - off : s0 + off;
            uint64_t code = (G[src >> 5] >> (2 * (src & 31))) & 3ULL;
            if (rev) code = 3ULL - code;
            word |= code << (2 * b);
        }
    }
    out[ga.dst_word_off[g] + j] = word;
}

// The unusable-base and contig-start bitmaps of the virtual genomes (only when the resident genomes carry them,
// mauve_set_genomes_contigs): thread (g, j) builds word j -- 64 virtual bases -- of both.  A contig boundary lies
// between a base and its predecessor, so on a reverse gap it moves to the other side of the base pair.
__global__ void __launch_bounds__(256) rec_gather_mask(const uint64_t *__restrict__ inv, const uint64_t *__restrict__ cm, uint64_t *__restrict__ vinv,
                                                       uint64_t *__restrict__ vcm, RecGatherArgs ga /* src = base mask words, dst = virtual mask words */,
                                                       const uint32_t *__restrict__ seg, const int64_t *__restrict__ glo0,
                                                       const uint8_t *__restrict__ grev, uint32_t K)
{
    const int g = blockIdx.y;
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= ga.dst_words[g]) return;
    const uint32_t *sg = seg + (size_t)g * (K + 1);
    const uint32_t tot = sg[K];
    const uint64_t base0 = j * 64;
    uint64_t wi = 0, wc = 0;
    if (base0 < tot) {
        uint32_t lo = 0, hi = K;
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (sg[mid] <= base0) lo = mid; else hi = mid; }
        uint32_t k = lo;
        const uint64_t *I = inv ? inv + ga.src_word_off[g] : nullptr, *C = cm ? cm + ga.src_word_off[g] : nullptr;
        for (int b = 0; b < 64; b++) {
            const uint64_t p = base0 + b;
            if (p >= tot) break;
            while (p >= sg[k + 1]) k++;
            const int64_t off = (int64_t)(p - sg[k]), len = (int64_t)(sg[k + 1] - sg[k]), s0 = glo0[(size_t)g * K + k];
            const bool rev = grev[(size_t)g * K + k] != 0;
            const int64_t src = rev ? s0 + len - 1 - off : s0 + off;
            if (I && (I[src >> 6] >> (src & 63) & 1)) wi |= 1ULL << b;
            if (C && off > 0) {                                   // a boundary before the gap's first base is the gap's own edge
                const int64_t cb = rev ? src + 1 : src;           // the source base whose bit says "a contig starts here"
                if (C[cb >> 6] >> (cb & 63) & 1) wc |= 1ULL << b;
            }
        }
    }
    if (vinv) vinv[ga.dst_word_off[g] + j] = wi;
    if (vcm) vcm[ga.dst_word_off[g] + j] = wc;
}

// A gap waiting for a recursive search: flat record [lcb, prev_w, a(1+N), b(1+N)] in `work`.
struct WorkList {
    int N; std::vector<int64_t> d;
    explicit WorkList(int n) : N(n) {}
    size_t rec() const { return 2 + 2 * (size_t)(1 + N); }
    size_t size() const { return d.size() / rec(); }
    void push(int64_t lcb, int prev_w, const int64_t *a, const int64_t *b)
    {
        d.push_back(lcb); d.push_back(prev_w); d.insert(d.end(), a, a + 1 + N); d.insert(d.end(), b, b + 1 + N);
    }
    int64_t lcb(size_t i) const { return d[i * rec()]; }
    int prev_w(size_t i) const { return (int)d[i * rec() + 1]; }
    const int64_t *a(size_t i) const { return &d[i * rec() + 2]; }
    const int64_t *b(size_t i) const { return &d[i * rec() + 2 + 1 + N]; }
};

// which seed weight a gap wants at this level (0 = none), DESIGN.md S8
inline int gap_weight(int N, const int64_t *a, const int64_t *b, int prev_w, int64_t min_gap)
{
    int64_t mx = 0, mn = -1, sum = 0;
    for (int g = 0; g < N; g++) {
        int64_t lo, ln; gap_of(a, b, g, lo, ln);
        mx = std::max(mx, ln); mn = mn < 0 ? ln : std::min(mn, ln); sum += ln;
    }
    if (mx <= min_gap) return 0;
    int w = mauve_default_seed_weight(sum / N);
    if (w > prev_w - 2) w = prev_w - 2;
    if (w < 5) return 0;
    if (mn < mauve_seed_length(mauve_get_seed(w, 0))) return 0;
    return w;
}

// the gaps of the chains that the first level looks at
void rec_work_list(mauve_ctx *c, const mauve_params *p, int w0, const std::vector<MatchVec> &chains, WorkList &work)
{
    // c->rec_flags (one byte per anchor in chain order, from the device: the gap behind it is longer than min_recursive_gap on some side):
    // consumed once; without it every gap is tested
    std::vector<uint8_t> flags; flags.swap(c->rec_flags);
    size_t total = 0; for (const MatchVec &ch : chains) total += ch.size();
    const bool use_flags = !flags.empty() && flags.size() == total;
    size_t off = 0;
    for (size_t l = 0; l < chains.size(); l++) {
        const size_t n = chains[l].size();
        for (size_t i = 0; i + 1 < n; i++)
            if ((!use_flags || flags[off + i]) && gap_weight(work.N, chains[l].rec(i), chains[l].rec(i + 1), w0, p->min_recursive_gap))
                work.push((int64_t)l, w0, chains[l].rec(i), chains[l].rec(i + 1));
        off += n;
    }
}

// One level of the recursion: the gaps it searches, the gaps the next level will look at, the new anchors of every LCB.
struct RecLevel {
    const WorkList &work; WorkList &next; std::vector<MatchVec> &found;
    // what the new anchors of gap wi (gl: real coordinates, genome-0 order), found with seed weight w, mean for the next level
    void apply(size_t wi, int w, const MatchVec &gl) const
    {
        const int64_t lcb = work.lcb(wi);
        for (size_t q = 0; q <= gl.size(); q++)
            next.push(lcb, w, q == 0 ? work.a(wi) : gl.rec(q - 1), q == gl.size() ? work.b(wi) : gl.rec(q));
        for (size_t q = 0; q < gl.size(); q++) found[(size_t)lcb].push(gl.rec(q));
    }
};

// The gaps of a level that want seed weight w, searched in one seed pass.  Several contexts, one alignment (mauve_set_shard): the
// gaps of the batch are LPT-dealt by their size, this rank searches and chains its share, and what every gap yields -- its new
// anchors -- is exchanged (rec_exchange), so that every rank goes on with the same work list.
struct RecBatch {
    int N, w;
    const std::vector<size_t> &all;                             // the whole batch: indices into the level's work list
    bool sharded = false;
    std::vector<size_t> mine; std::vector<uint32_t> pos_of;     // sharded: this rank's gaps; pos_of[k]: their places in `all` (the order results are applied in)
    uint32_t K = 0;                                             // this rank's gaps
    // gap k in genome g: where it starts in virtual genome g (seg[g * (K + 1) + k]; [.. + K]: the total), its real left end, 0-based,
    // its length and its strand ([g * K + k])
    std::vector<uint32_t> seg; std::vector<int64_t> glo0, glen; std::vector<uint8_t> grev;
    GenomeSet vs;                                               // the virtual genomes: per genome, the gap sub-sequences in LCB orientation, concatenated
    RecBatch(int n, int weight, const std::vector<size_t> &ids_all) : N(n), w(weight), all(ids_all) {}
    const std::vector<size_t> &ids() const { return sharded ? mine : all; }
};

// times and route of one batch, for its trace lines
struct RecTrace { double t_batch = 0, t_chain = 0, t_elim = 0, t_lcb = 0; const char *route = "host"; };

void rec_deal(const mauve_ctx *c, const WorkList &work, RecBatch &B)
{
    B.sharded = c->shard_on && B.all.size() >= (size_t)(2 * c->shard_world);
    if (B.sharded) {
        std::vector<int64_t> cost(B.all.size(), 0);
        for (size_t q = 0; q < B.all.size(); q++)
            for (int g = 0; g < B.N; g++) { int64_t lo, ln; gap_of(work.a(B.all[q]), work.b(B.all[q]), g, lo, ln); cost[q] += ln; }
        std::vector<int> owner; shard_lpt(cost, c->shard_world, owner);
        for (size_t q = 0; q < B.all.size(); q++) if (owner[q] == c->shard_rank) { B.mine.push_back(B.all[q]); B.pos_of.push_back((uint32_t)q); }
    }
    B.K = (uint32_t)B.ids().size();
}

// the tables of the batch and the layout of its virtual genomes (ga: for rec_gather)
int rec_batch_tables(mauve_ctx *c, const WorkList &work, const int *gmap, RecBatch &B, RecGatherArgs &ga)
{
    const int N = B.N; const uint32_t K = B.K;
    const std::vector<size_t> &ids = B.ids();
    GenomeSet &vs = B.vs; vs.buf = &c->rec_genomes; vs.nseq = N; vs.lens.assign(N, 0); vs.word_off.assign(N, 0);
    B.seg.resize((size_t)N * (K + 1)); B.glo0.resize((size_t)N * K); B.glen.resize((size_t)N * K); B.grev.resize((size_t)N * K);
    memset(&ga, 0, sizeof ga);
    size_t words = 0;
    for (int g = 0; g < N; g++) {
        int64_t tot = 0;
        for (uint32_t k = 0; k < K; k++) {
            int64_t lo; gap_of(work.a(ids[k]), work.b(ids[k]), g, lo, B.glen[(size_t)g * K + k]);
            B.glo0[(size_t)g * K + k] = lo - 1;
            B.seg[(size_t)g * (K + 1) + k] = (uint32_t)tot; tot += B.glen[(size_t)g * K + k];
            B.grev[(size_t)g * K + k] = work.a(ids[k])[1 + g] > 0 ? 0 : 1;
        }
        B.seg[(size_t)g * (K + 1) + K] = (uint32_t)tot;
        if (tot >= (1LL << 31)) { c->err = "recursive anchoring: gap set too large"; return MAUVE_ERR_LIMIT; }
        vs.lens[g] = tot;
        const size_t nw = mauve_packed_words(tot);
        vs.word_off[g] = words;
        ga.src_word_off[g] = c->word_off[gmap ? gmap[g] : g]; ga.dst_word_off[g] = words; ga.dst_words[g] = nw;
        words += nw;
    }
    return MAUVE_OK;
}

// the gaps inherit the ambiguity / contig bitmaps of the resident genomes (dseg, dlo0, drev: the batch's tables on the device)
int rec_batch_gather_masks(mauve_ctx *c, const int *gmap, RecBatch &B, const uint32_t *dseg, const int64_t *dlo0, const uint8_t *drev)
{
    const int N = B.N;
    GenomeSet &vs = B.vs;
    RecGatherArgs gm; memset(&gm, 0, sizeof gm);
    vs.mask_off.assign((size_t)N, 0);
    size_t mwords = 0; uint64_t max_mw = 0;
    for (int g = 0; g < N; g++) {
        const size_t nw = (size_t)((vs.lens[(size_t)g] + 63) / 64) + 2;
        vs.mask_off[(size_t)g] = mwords; gm.src_word_off[g] = c->base_mask_off[(size_t)(gmap ? gmap[g] : g)]; gm.dst_word_off[g] = mwords; gm.dst_words[g] = nw;
        max_mw = std::max<uint64_t>(max_mw, nw); mwords += nw;
    }
    HIPCHK(c, c->rec_vinv.ensure(mwords * 8)); HIPCHK(c, c->rec_vcm.ensure(mwords * 8));
    hipLaunchKernelGGL(rec_gather_mask, dim3((uint32_t)((max_mw + 255) / 256), (uint32_t)N), dim3(256), 0, c->stream,
                       c->has_invalid ? c->base_invalid.as<uint64_t>() : nullptr, c->has_contigs ? c->contig_mask.as<uint64_t>() : nullptr,
                       c->has_invalid ? c->rec_vinv.as<uint64_t>() : nullptr, c->has_contigs ? c->rec_vcm.as<uint64_t>() : nullptr, gm, dseg, dlo0, drev, B.K);
    HIPCHK(c, hipGetLastError());
    if (c->has_invalid) vs.vmask = &c->rec_vinv;
    if (c->has_contigs) vs.cmask = &c->rec_vcm;
    return MAUVE_OK;
}

// the tables to the device, the virtual genomes made from them
int rec_batch_gather(mauve_ctx *c, const int *gmap, RecBatch &B, const RecGatherArgs &ga)
{
    const int N = B.N;
    size_t words = 0; uint64_t max_words = 0;
    for (int g = 0; g < N; g++) { words += ga.dst_words[g]; max_words = std::max(max_words, ga.dst_words[g]); }
    HIPCHK(c, c->rec_genomes.ensure((words + 4) * sizeof(uint64_t)));
    // one side buffer: segment table, then the 0-based gap starts, then the strand flags
    const size_t seg_bytes = (B.seg.size() * sizeof(uint32_t) + 7) & ~(size_t)7, glo_bytes = B.glo0.size() * sizeof(int64_t);
    HIPCHK(c, c->rec_seg.ensure(seg_bytes + glo_bytes + B.grev.size() + 8));
    char *side = c->rec_seg.as<char>();
    const uint32_t *dseg = (const uint32_t *)side; const int64_t *dlo0 = (const int64_t *)(side + seg_bytes); const uint8_t *drev = (const uint8_t *)(side + seg_bytes + glo_bytes);
    HIPCHK(c, hipMemcpyAsync(side, B.seg.data(), B.seg.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(side + seg_bytes, B.glo0.data(), glo_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(side + seg_bytes + glo_bytes, B.grev.data(), B.grev.size(), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(rec_gather, dim3((uint32_t)((max_words + 255) / 256), (uint32_t)N), dim3(256), 0, c->stream,
                       c->genomes.as<uint64_t>(), c->rec_genomes.as<uint64_t>(), ga, dseg, dlo0, drev, B.K);
    HIPCHK(c, hipGetLastError());
    if (c->has_invalid || c->has_contigs) { const int rc = rec_batch_gather_masks(c, gmap, B, dseg, dlo0, drev); if (rc) return rc; }
    HIPCHK(c, hipStreamSynchronize(c->stream));    // the copies have read the host tables
    return MAUVE_OK;
}

// Routes 1 and 2: all gaps at once on the device.  chain_device_gaps_compact sends only the survivors back; a batch beyond its
// limits (MAUVE_ERR_LIMIT), or every batch under MAUVE_GAP_CHAIN_ALL_BACK, takes chain_device_gaps, which copies every record
// and the graph back and applies the collinear rule on the host.  MAUVE_ERR_LIMIT: beyond that one's limits too.
int rec_chain_device(mauve_ctx *c, const RecBatch &B, bool all_back, RecSurvivors &S, RecTrace &T)
{
    const int N = B.N; const uint32_t K = B.K;
    int64_t maxlen = 1; for (int g = 0; g < N; g++) maxlen = std::max(maxlen, B.vs.lens[(size_t)g]);
    uint32_t ns = 0;
    const char *route = "device, survivors only";
    int rc = all_back ? MAUVE_ERR_LIMIT : chain_device_gaps_compact(c, N, maxlen, c->rec_seg.as<uint32_t>(), K, &S.len, &S.st, &S.gap, &ns);
    if (rc == MAUVE_ERR_LIMIT) { route = "device"; rc = chain_device_gaps(c, N, maxlen, c->rec_seg.as<uint32_t>(), K, &S.len, &S.st, &S.gap, &ns); }
    if (rc) return rc;
    T.route = route; S.n = ns;
    return MAUVE_OK;
}

// the all-forward matches of the host's list from record i on that start in gap k, 1-based inside the gap -> loc; the index behind them
int64_t rec_gap_matches(const mauve_ctx *c, const RecBatch &B, int64_t i, int64_t nm, uint32_t k, MatchVec &loc)
{
    const int N = B.N; const uint32_t K = B.K;
    loc.d.clear();
    for (; i < nm && (uint32_t)(c->match_start[(size_t)i * N] - 1) < B.seg[k + 1]; i++) {
        bool fwd = true;
        int64_t rec[1 + MAUVE_MAX_SEQ]; rec[0] = c->match_len[(size_t)i];
        for (int g = 0; g < N; g++) {
            const int64_t s = c->match_start[(size_t)i * N + g];
            if (s <= 0) { fwd = false; break; }
            rec[1 + g] = s - B.seg[(size_t)g * (K + 1) + k];
        }
        if (fwd) loc.push(rec);
    }
    return i;
}

// Route 3: the host's copy of the list (canonical order, genome 0 always forward: gap by gap) chained gap by gap
void rec_chain_host(const mauve_ctx *c, const RecBatch &B, int64_t nm, RecSurvivors &S, RecTrace &T)
{
    const int N = B.N; const uint32_t K = B.K;
    const uint32_t *seg0 = B.seg.data();
    MatchVec loc(N);                     // reused from gap to gap (thousands of gaps per batch)
    ChainOrders orders;
    std::vector<int64_t> ml;
    const bool trace = switches().trace;
    for (int64_t i = 0; i < nm;) {
        const uint32_t k = (uint32_t)(std::upper_bound(seg0, seg0 + K + 1, (uint32_t)(c->match_start[(size_t)i * N] - 1)) - seg0) - 1;
        i = rec_gap_matches(c, B, i, nm, k, loc);
        if (loc.empty()) continue;
        const double te0 = trace ? now_ms() : 0;
        host_eliminate_overlaps(loc, &orders);
        const double te1 = trace ? now_ms() : 0;
        int64_t nl = 0;
        host_lcb_chain(loc, 0, true, ml, nl, &orders);
        if (trace) { T.t_elim += te1 - te0; T.t_lcb += now_ms() - te1; }
        for (size_t q = 0; q < loc.size(); q++) {
            if (ml[q] < 0) continue;
            int32_t st[MAUVE_MAX_SEQ];                           // back into the virtual genomes
            for (int g = 0; g < N; g++) st[g] = (int32_t)(loc.st(q)[g] + B.seg[(size_t)g * (K + 1) + k]);
            S.push(k, (int32_t)loc.len(q), st, N);
        }
    }
    S.view_own();
}

// The batched seed pass over the virtual genomes and the per-gap chaining of its N-way forward matches -> S.  Large batches are
// chained on the device (rec_chain_device).  Small batches (host-sorted lists: dev_rec_n != nm) and batches with an overlap cluster
// or a gap sub-graph beyond the device kernels' limits are chained on the host, which is the only route that reads the host copy of
// the list.  (A list with ties in its canonical order is repaired by the seed pass before dev_rec_n is set, so it takes the device
// route like any other.)
int rec_batch_chain(mauve_ctx *c, const RecBatch &B, int level, RecSurvivors &S, RecTrace &T)
{
    const bool host_gaps = switches().host_gap_chain, old_gaps = switches().gap_chain_all_back;      // A/B switches
    int64_t nm = 0;
    c->lazy_matches_ok = !host_gaps && !old_gaps;     // a large batch is chained where its list is: no host copy of it
    int rc = seedpass_run(c, B.vs, mauve_get_seed(B.w, 0), MAUVE_MODE_MEM, full_mask(B.N), 1, c->rec_seg.as<uint32_t>(), B.K, &nm);
    c->lazy_matches_ok = false;
    if (rc) return rc;
    if (switches().trace) fprintf(stderr, "[trace] recursion level %d weight %d: %u gaps, %lld bases, %lld matches, %.3f ms\n", level, B.w, B.K,
                         (long long)B.vs.lens[0], (long long)nm, now_ms() - T.t_batch);
    T.t_chain = now_ms();
    if (!host_gaps && nm > 0 && c->dev_rec_n == nm) {
        rc = rec_chain_device(c, B, old_gaps, S, T);
        if (rc != MAUVE_ERR_LIMIT) return rc;
    }
    rc = seed_matches_to_host(c);
    if (rc) return rc;
    rec_chain_host(c, B, nm, S, T);
    return MAUVE_OK;
}

// The survivors gap by gap: to real coordinates, into genome-0 order, and then applied to the level or, in a sharded batch,
// appended to the rank's message.  (A gap without survivors is not in the list: it emits nothing.)
void rec_emit(const RecBatch &B, const RecSurvivors &S, const RecLevel &L, std::vector<int64_t> &shard_msg)
{
    const int N = B.N; const uint32_t K = B.K;
    MatchVec glob(N);                    // reused from gap to gap
    for (size_t q = 0; q < S.n;) {
        const uint32_t k = S.gap[q];
        size_t e = q + 1;
        while (e < S.n && S.gap[e] == k) e++;
        glob.d.resize((e - q) * (1 + (size_t)N));
        for (int64_t *o = glob.d.data(); q < e; q++) {
            const int64_t len = S.len[q];
            *o++ = len;
            for (int g = 0; g < N; g++) {
                const int64_t s = (int64_t)S.st[q * N + g] - B.seg[(size_t)g * (K + 1) + k];          // 1-based inside the gap
                *o++ = rec_real_start(B.glo0[(size_t)g * K + k] + 1, B.glen[(size_t)g * K + k], B.grev[(size_t)g * K + k] != 0, s, len);
            }
        }
        glob.sort_by_start0();
        if (B.sharded) shard_msg_append(shard_msg, B.pos_of[k], glob);
        else L.apply(B.ids()[k], B.w, glob);
    }
}

// rc_local: what this rank's share of the batch came to.  A rank that failed still takes part in the exchange -- its message is the
// marker [-1, status] -- so that the others do not wait in the collective for ever; every rank then returns an error.
int rec_exchange(mauve_ctx *c, const RecBatch &B, int rc_local, std::vector<int64_t> &shard_msg, const RecLevel &L)
{
    if (!B.sharded) return rc_local;
    std::vector<std::pair<const char *, size_t>> parts;
    const std::string err_local = c->err;
    if (rc_local) shard_msg_fail(shard_msg, rc_local);
    const int rcx = shard_allgather(c, shard_msg.data(), shard_msg.size() * 8, parts);
    if (rcx) return rcx;
    if (rc_local) { c->err = err_local; return rc_local; }
    // every rank's gaps, applied in the order of the whole batch
    std::vector<std::pair<uint32_t, const int64_t *>> got;
    if (int rc = shard_msg_parse(parts, B.N, B.all.size(), got, c->err)) return rc;
    MatchVec gl(B.N);
    for (const auto &gq : got) {
        gl.d.assign(gq.second + 2, gq.second + 2 + gq.second[1] * (1 + B.N));
        L.apply(B.all[gq.first], B.w, gl);
    }
    return MAUVE_OK;
}

// the new anchors into their chains
void rec_merge_found(std::vector<MatchVec> &chains, std::vector<MatchVec> &found)
{
    for (size_t l = 0; l < chains.size(); l++) {
        if (found[l].empty()) continue;
        found[l].sort_by_start0();
        merge_sorted_anchors(chains[l], found[l]);
    }
}

}  // namespace

int recursive_anchoring(mauve_ctx *c, const mauve_params *p, int w0, std::vector<MatchVec> &chains, int N, const int *gmap)
{
    const double t_stage0 = now_ms();
    WorkList work(N);
    rec_work_list(c, p, w0, chains, work);
    std::vector<MatchVec> found(chains.size(), MatchVec(N));
    if (switches().trace) fprintf(stderr, "[trace] recursion: work list of %zu gaps built in %.3f ms\n", work.size(), now_ms() - t_stage0);

    for (int level = 1; work.size(); level++) {
        std::map<int, std::vector<size_t>> classes;     // seed weight -> gaps of this level
        for (size_t i = 0; i < work.size(); i++) {
            int w = gap_weight(N, work.a(i), work.b(i), work.prev_w(i), p->min_recursive_gap);
            if (w) classes[w].push_back(i);
        }
        WorkList next(N);
        next.d.reserve(work.d.size() + work.d.size() / 2);
        const RecLevel L{work, next, found};
        for (const auto &cls : classes) {
            RecBatch B(N, cls.first, cls.second);
            rec_deal(c, work, B);
            RecTrace T; T.t_batch = T.t_chain = now_ms();
            RecSurvivors S;
            std::vector<int64_t> shard_msg;              // what this rank's gaps yielded, for the other ranks (recursion_host.hpp)
            RecGatherArgs ga;
            int rc = MAUVE_OK;                           // (a rank without a gap of this class still takes part in the exchange)
            if (B.K) rc = rec_batch_tables(c, work, gmap, B, ga);
            if (B.K && !rc) rc = rec_batch_gather(c, gmap, B, ga);
            if (B.K && !rc) rc = rec_batch_chain(c, B, level, S, T);
            if (!rc) rec_emit(B, S, L, shard_msg);
            rc = rec_exchange(c, B, rc, shard_msg, L);
            if (rc) return rc;
            if (switches().trace) fprintf(stderr, "[trace]   per-gap chaining %.3f ms (%s; eliminate %.3f, lcb %.3f)\n", now_ms() - T.t_chain, T.route, T.t_elim, T.t_lcb);
        }
        work.d.swap(next.d);
    }
    const double tm0 = now_ms();
    rec_merge_found(chains, found);
    if (switches().trace) fprintf(stderr, "[trace] recursion: merge into chains %.3f ms, whole stage %.3f ms\n", now_ms() - tm0, now_ms() - t_stage0);
    return MAUVE_OK;
}
