// progressive.cpp -- guide tree and guide-tree recursive anchoring behind mauve_progressive_align():
// the stand-in for ProgressiveAligner::align(seq_table, interval_list) [EXT] (progressiveMauve.cpp:575-710) and
// for the distance matrix / guide tree of mauveAligner.cpp:616-623.  Frozen spec: DESIGN.md S9.
//
//   1. pairwise matches of every genome pair (PairwiseMatchFinder rule, one sorted mer list on the device),
//      similarity = matched bases / shorter genome, integer distance in ppm, UPGMA with integer averaging;
//   2. the root of the tree aligns what all genomes share (the Aligner::align path); every internal node below
//      aligns, among its own genomes only, the bases no ancestor has placed.  Placed bases are a 1-bit-per-base
//      mask on the device: windows touching them are invalid for seeding and extension (seed_pass.hip), chains
//      are cut where the stretch between two anchors touches a placed base or is too long for the gapped
//      aligner, so those bases flow down to the subtree that shares them;
//   3. what is left at the leaves becomes single-genome intervals.
// Every node is one pass of the same device pipeline (seed pass, batched recursive anchoring, batched DP).
//
// A node (prog_node) is a list of stages that hand each other one NodeWork record:
//   node_search       seed weight and pattern for what is left of the node's genomes, placed-base mask, the search
//   node_min_weight   minimum LCB weights of the node, scaled by the distances between its subtrees (S11b, S11c)
//   node_chain        overlap elimination and LCBs: on the device at the root, else host_chain_lcbs
//   node_pieces       the chains, cut where a stretch between two anchors touches a placed base
//   (recursive_anchoring, recursive.cpp)
//   node_split_long   pieces cut again where a stretch is too long for the gapped aligner or only a subset's
//   host_gap_table    the interval table (host_chain.hpp)
//   node_dp_plain / node_refine   gapped alignment of the intervals; with refinement also of their rotations (S13)
//   node_blocks       the node's blocks into the result, their bases out of the pools
#include "common.hpp"
#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <map>

namespace {

// The bases of one genome that no block has taken yet: an ordered map start -> end of free stretches (1-based,
// inclusive, disjoint).  Blocks are carved out one by one; a position is identified by the start of the stretch it lies
// in (0 = placed already).
struct FreePool {
    std::map<int64_t, int64_t> free_;
    void reset(int64_t len) { free_.clear(); if (len >= 1) free_[1] = len; }
    bool whole(int64_t len) const { return free_.size() == 1 && free_.begin()->first == 1 && free_.begin()->second == len; }
    int64_t bases() const { int64_t t = 0; for (const auto &kv : free_) t += kv.second - kv.first + 1; return t; }
    int64_t stretch_of(int64_t pos) const
    {
        auto it = free_.upper_bound(pos);
        if (it == free_.begin()) return 0;
        --it;
        return pos <= it->second ? it->first : 0;
    }
    void carve(int64_t l, int64_t h)              // free minus [l, h]
    {
        if (h < l) return;
        auto it = free_.upper_bound(l);
        if (it != free_.begin()) --it;
        while (it != free_.end() && it->first <= h) {
            const int64_t a = it->first, e = it->second;
            if (e < l) { ++it; continue; }
            it = free_.erase(it);
            if (a < l) free_[a] = l - 1;
            if (e > h) { free_[h + 1] = e; break; }
        }
    }
};

struct Prog {
    mauve_ctx *c; const mauve_params *p; int N;
    std::vector<int32_t> left, right;
    std::vector<int64_t> dist;         // [N*N] ppm, filled when the node weights are scaled
    std::vector<int64_t> bpd;          // [N*N] ppm breakpoint distance, filled when bp_dist_scale_ppm is set as well
    std::vector<FreePool> rest;        // per genome: bases not placed in any block yet
    AlignResult *R;
    int64_t n_gap_dp = 0, n_cells = 0, n_anchor = 0, n_multi = 0;
    double t_seed = 0, t_chain = 0, t_rec = 0, t_dp = 0, t_blocks = 0;      // stage times summed over the nodes (mauve_last_stage_times)
};

// what the stages of one node hand each other
struct NodeWork {
    int node = 0, n = 0, w = 0; uint64_t pat = 0; uint32_t full = 0;
    std::vector<int> gm;                       // the node's n genomes: global ids, ascending
    int64_t rest_len = 0;                      // their bases no block has taken yet
    GenomeSet gs;
    int64_t nm = 0; MatchVec m;                // the search's matches; after the chain: overlap-free
    int64_t lcbw = 0, minw_sp = 0;             // minimum LCB weight: length-weighted, score-weighted (lcb_scoring = SP only)
    std::vector<int64_t> match_lcb; int64_t nl = 0;
    std::vector<MatchVec> pieces;              // the node's blocks-to-be: chains, cut
    std::vector<GapRef> gaps; std::vector<DpSeqDesc> desc; int64_t n_dp = 0, code_total = 0;     // (GapRef::lcb: index into pieces; descriptors carry GLOBAL genome ids)
    uint32_t *dcols = nullptr; std::vector<int64_t> dcol_off, dscore; int64_t cells = 0;         // DP outputs (dcols: c->pin_dcols)
    double tn0 = 0, tn1 = 0, tn2 = 0, tn3 = 0; // stage clocks: search from, chain from, recursion from, DP from
};

int leaves_of(const Prog &P, int node, std::vector<int> &out)
{
    if (P.left[node] < 0) { out.push_back(node); return 1; }
    return leaves_of(P, P.left[node], out) + leaves_of(P, P.right[node], out);
}

// upload the placed-base bitmap of the node's genomes (bit set = placed)
int upload_mask(Prog &P, const std::vector<int> &gm, GenomeSet &gs)
{
    mauve_ctx *c = P.c;
    gs.mask_off.assign(gm.size(), 0);
    size_t words = 0;
    for (size_t j = 0; j < gm.size(); j++) { gs.mask_off[j] = words; words += (size_t)((c->lens[gm[j]] + 63) / 64) + 2; }
    std::vector<uint64_t> bits(words, ~0ULL);
    for (size_t j = 0; j < gm.size(); j++)
        for (const auto &fr : P.rest[gm[j]].free_) clear_bits(bits.data() + gs.mask_off[j], fr.first, fr.second);
    // ambiguous bases stay unusable at every node; contig joins likewise (mauve_set_genomes_contigs)
    if (c->has_invalid)
        for (size_t j = 0; j < gm.size(); j++) {
            const size_t w = (size_t)((c->lens[gm[j]] + 63) / 64);
            for (size_t k = 0; k < w; k++) bits[gs.mask_off[j] + k] |= c->h_invalid[c->base_mask_off[(size_t)gm[j]] + k];
        }
    HIPCHK(c, c->placed_mask.ensure(words * 8));
    HIPCHK(c, hipMemcpyAsync(c->placed_mask.p, bits.data(), words * 8, hipMemcpyHostToDevice, c->stream));
    if (c->has_contigs) {
        std::vector<uint64_t> cm(words, 0);
        for (size_t j = 0; j < gm.size(); j++) {
            const size_t w = (size_t)((c->lens[gm[j]] + 63) / 64);
            for (size_t k = 0; k < w; k++) cm[gs.mask_off[j] + k] = c->h_contig[c->base_mask_off[(size_t)gm[j]] + k];
        }
        HIPCHK(c, c->node_cmask.ensure(words * 8));
        HIPCHK(c, hipMemcpy(c->node_cmask.p, cm.data(), words * 8, hipMemcpyHostToDevice));
        gs.cmask = &c->node_cmask;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    gs.vmask = &c->placed_mask;
    return MAUVE_OK;
}

// seed of the node from what is left of its genomes, their placed-base mask, the search (tn0 .. tn1)
int node_search(Prog &P, NodeWork &W)
{
    mauve_ctx *c = P.c; const mauve_params *p = P.p;
    leaves_of(P, W.node, W.gm);
    std::sort(W.gm.begin(), W.gm.end());
    const std::vector<int> &gm = W.gm;
    const int n = W.n = (int)gm.size();
    for (int j = 0; j < n; j++) W.rest_len += P.rest[gm[j]].bases();
    int rc = resolve_seed(c, p, W.rest_len / n, "progressive_align", &W.w, &W.pat);
    if (rc) return rc;
    W.full = full_mask(n);

    GenomeSet &gs = W.gs; gs.buf = &c->genomes; gs.nseq = n;
    for (int j = 0; j < n; j++) { gs.lens.push_back(c->lens[gm[j]]); gs.word_off.push_back(c->word_off[gm[j]]); }
    bool any_placed = false;
    for (int j = 0; j < n; j++) if (!P.rest[gm[j]].whole(c->lens[gm[j]])) any_placed = true;
    if (any_placed) { rc = upload_mask(P, gm, gs); if (rc) return rc; }

    W.tn0 = now_ms();
    W.m = MatchVec(n);
    if (p->seed_family) {                                    // the node searches with the whole seed family
        rc = seed_family_matches(c, gs, W.w, p->mode, W.full, W.m);
        if (rc) return rc;
        W.nm = (int64_t)W.m.size();
    } else {
        rc = seedpass_run(c, gs, W.pat, p->mode, W.full, 1, nullptr, 0, &W.nm);
        if (rc) return rc;
        seed_matches_to_vec(c, n, W.nm, W.m);
    }
    W.tn1 = now_ms();
    return MAUVE_OK;
}

// the node's minimum LCB weights: a given threshold is for all N genomes and is scaled by the node's share of them (of the
// pairs, for sum-of-pairs scores); both shrink with the distance between the node's two subtrees
void node_min_weight(const Prog &P, NodeWork &W)
{
    const mauve_params *p = P.p;
    const int64_t n = W.n, N = P.N;
    W.lcbw = p->lcb_weight >= 0 ? p->lcb_weight * n / N : (int64_t)3 * W.w * n;
    if (p->lcb_scoring == MAUVE_LCB_SCORE_SP)
        W.minw_sp = p->lcb_weight >= 0 ? p->lcb_weight * (n * (n - 1) / 2) / (N * (N - 1) / 2) : sp_default_min_weight(W.w, W.n, &p->scoring);
    if (!p->weight_scaling || P.dist.empty()) return;
    // the node's minimum weight shrinks with the conservation distance between its two subtrees
    std::vector<int> la, lb;
    leaves_of(P, P.left[W.node], la); leaves_of(P, P.right[W.node], lb);
    const int64_t pairs = (int64_t)la.size() * (int64_t)lb.size();
    int64_t sum = 0;
    for (int a : la) for (int b : lb) sum += P.dist[(size_t)a * P.N + b];
    int64_t factor_ppm = std::max<int64_t>(0, 1000000 - (int64_t)p->conservation_scale_ppm * (sum / pairs) / 1000000);
    if (!P.bpd.empty()) {                                     // the breakpoint-distance factor multiplies in
        int64_t bsum = 0;
        for (int a : la) for (int b : lb) bsum += P.bpd[(size_t)a * P.N + b];
        const int64_t f2 = std::max<int64_t>(0, 1000000 - (int64_t)p->bp_dist_scale_ppm * (bsum / pairs) / 1000000);
        factor_ppm = factor_ppm * f2 / 1000000;
    }
    W.lcbw = std::max(W.lcbw * factor_ppm / 1000000, p->min_scaled_penalty);
    if (p->lcb_scoring == MAUVE_LCB_SCORE_SP) W.minw_sp = std::max(W.minw_sp * factor_ppm / 1000000, p->min_scaled_penalty);
}

// The root's list (all genomes, tens of thousands of matches) is still in HBM in canonical order: overlap elimination and LCBs on the
// device (chain_dev.hip), cropped records and labels back -- what mauve_align does.  Nodes below the root have short lists (and a
// genome subset: the device chain takes its position width from the context's genomes), score-weighted LCBs need the matches' scores,
// a list the device chain declines comes back as MAUVE_ERR_LIMIT: the host chain for those.  MAUVE_HOST_CHAIN: A/B switch.
int node_chain(Prog &P, NodeWork &W)
{
    mauve_ctx *c = P.c; const mauve_params *p = P.p;
    const int n = W.n;
    MatchVec &m = W.m;
    const bool sp = p->lcb_scoring == MAUVE_LCB_SCORE_SP;    // the matches' scores are summed on the device too (ch_sp_scores, on the cropped records)
    int rc = MAUVE_ERR_LIMIT;
    if (!switches().host_chain && !p->seed_family && n == P.N && W.nm > 0 && c->dev_rec_n == W.nm && (!sp || n <= 16)) {
        rc = chain_device(c, n, sp ? W.minw_sp : W.lcbw, p->collinear != 0, m, W.match_lcb, W.nl, sp ? &p->scoring : nullptr);
        if (rc && rc != MAUVE_ERR_LIMIT) return rc;
    }
    if (rc) { rc = host_chain_lcbs(c, p, m, W.gm.data(), W.lcbw, W.minw_sp, W.match_lcb, W.nl, nullptr, true); if (rc) return rc; }
    if (switches().trace) {
        int64_t surv = 0; for (size_t i = 0; i < m.size(); i++) if (W.match_lcb[i] >= 0) surv++;
        fprintf(stderr, "[trace] node %d (n=%d, w=%d): %lld n-way matches, %zu after overlap elimination, %lld lcbs, %lld anchors\n", W.node, n, W.w,
                (long long)W.nm, m.size(), (long long)W.nl, (long long)surv);
    }
    return MAUVE_OK;
}

// chains, cut wherever the stretch between two consecutive anchors touches an already placed base
void node_pieces(const Prog &P, NodeWork &W)
{
    const MatchVec &m = W.m;
    int64_t cur_lcb = -1;
    for (size_t i = 0; i < m.size(); i++) {
        const int64_t l = W.match_lcb[i]; if (l < 0) continue;
        bool newp = l != cur_lcb;
        if (!newp) {
            const MatchVec &last = W.pieces.back();
            const int64_t *a = last.st(last.size() - 1);
            for (int j = 0; j < W.n && !newp; j++) {
                const FreePool &fp = P.rest[W.gm[j]];
                if (fp.stretch_of(std::llabs(a[j])) != fp.stretch_of(std::llabs(m.st(i)[j]))) newp = true;
            }
        }
        if (newp) { W.pieces.emplace_back(W.n); cur_lcb = l; }
        W.pieces.back().push(m.rec(i));
    }
}

// a stretch shared by >= 2 genomes that is too long for the gapped aligner, or that only a proper subset of
// this node's genomes has (and that is long enough to be anchored), ends the block: its bases stay in the
// pool for the subtree that shares them
void node_split_long(const Prog &P, NodeWork &W)
{
    const mauve_params *p = P.p; const int n = W.n;
    std::vector<MatchVec> np2;
    for (const MatchVec &pc : W.pieces)
        for (size_t i = 0; i < pc.size(); i++) {
            bool split = i == 0;
            if (!split) {
                int64_t mx = 0; int nonempty = 0, big = 0;
                for (int j = 0; j < n; j++) { int64_t lo, ln; gap_of(pc.rec(i - 1), pc.rec(i), j, lo, ln); mx = std::max(mx, ln); nonempty += ln > 0; big += ln > p->min_recursive_gap; }
                split = nonempty >= 2 && (mx > p->max_gapped_len || (big >= 2 && big < n));
            }
            if (split) np2.emplace_back(n);
            np2.back().push(pc.rec(i));
        }
    W.pieces.swap(np2);
}

int node_dp_plain(Prog &P, NodeWork &W)          // (several contexts: the node's intervals are dealt out)
{
    return dp_batch_run_desc(P.c, W.n, W.n_dp, W.desc.data(), &P.p->scoring, W.dcols, W.dcol_off.data(), W.dscore.data(), &W.cells, true, nullptr);
}

// DESIGN.md S13 (setRefinement): every interval of k >= 3 sequences is also aligned in the rotated orders r = 1 .. min(rounds, k-1) and keeps the
// alignment whose sum-of-pairs score (dp_sp_scores) is highest, lowest rotation on ties.  A candidate's slots hold the rotated sequences, so its
// column bits are slots of the rotation.  The candidates do not depend on the first alignment, only the choice does: ONE batch holds the
// intervals and all their candidates (one sizing pass, one launch with more to balance), the columns stay on the device, the scores come back,
// and only the winners' columns are compacted and copied out (dp_fetch_picked) -- at C4's root 57 k candidates of 29 k intervals, 1 k of them win.
// Several contexts (mauve_set_shard) keep the two exchanged batches.
struct Cand { int64_t iv; int r, k; uint8_t nz[MAUVE_MAX_SEQ]; };
struct RefineWork {
    std::vector<Cand> cands;
    std::vector<int32_t> cbase;                // first candidate of every interval (n_dp + 1 entries)
    bool rot_dev = false;                      // the rotated descriptor rows are made on the device
    int64_t ccodes = 0, replaced = 0;          // bases of all candidates; intervals that keep a candidate
    std::vector<int64_t> aoff, ascore, asp;    // of the batch entries: the intervals, then the candidates
    std::vector<uint32_t> ccols;               // the candidates' columns (the exchanged form only)
};

// the candidates of every interval; their descriptor rows behind the intervals' in c->prog_desc unless the device makes them
// (sized once and filled in place: 86 000 descriptor rows at C4's root; push_back by push_back this took 3 ms.  A batch large enough for the
// device front gets only the intervals and the index of every interval's first candidate: the rotated rows are made on the device.)
void refine_candidates(Prog &P, NodeWork &W, RefineWork &F)
{
    mauve_ctx *c = P.c; const mauve_params *p = P.p;
    const int n = W.n; const int64_t n_dp = W.n_dp;
    const std::vector<DpSeqDesc> &desc = W.desc;
    std::vector<DpSeqDesc> &all = c->prog_desc;
    F.cbase.assign((size_t)n_dp + 1, 0);
    int64_t nc0 = 0;
    for (int64_t iv = 0; iv < n_dp; iv++) {
        int k = 0; for (int j = 0; j < n; j++) k += desc[(size_t)(iv * n + j)].len != 0;
        F.cbase[(size_t)iv] = (int32_t)nc0;
        if (k >= 3) nc0 += std::min(p->refine_rounds, k - 1);
    }
    F.cbase[(size_t)n_dp] = (int32_t)nc0;
    F.rot_dev = !c->shard_on && nc0 > 0 && nc0 < (1LL << 30) && dp_desc_rotations_on_device(n_dp + nc0);
    if (!F.rot_dev) { all.resize((size_t)(n_dp + nc0) * n); std::copy(desc.begin(), desc.end(), all.begin()); }
    F.cands.resize((size_t)nc0);
    DpSeqDesc none; none.genome = W.gm[0]; none.rev = 0; none.lo0 = 0; none.len = 0;
    int64_t q0 = 0;
    for (int64_t iv = 0; iv < n_dp; iv++) {
        Cand cd; cd.iv = iv; cd.k = 0;
        int64_t tot = 0;
        const DpSeqDesc *di = &desc[(size_t)(iv * n)];
        for (int j = 0; j < n; j++) if (di[j].len) { cd.nz[cd.k++] = (uint8_t)j; tot += di[j].len; }
        if (cd.k < 3) continue;
        for (int r = 1; r <= p->refine_rounds && r < cd.k; r++, q0++) {
            cd.r = r; F.cands[(size_t)q0] = cd;
            if (!F.rot_dev) {
                DpSeqDesc *o = &all[(size_t)(n_dp + q0) * n];
                for (int j = 0; j < n; j++) o[j] = j < cd.k ? di[cd.nz[(j + r) % cd.k]] : none;
            }
            F.ccodes += tot;
        }
    }
}

// every interval keeps the batch entry with the highest sum-of-pairs score; the winners' columns into dcols (one batch: compacted on the
// device and fetched; exchanged form: spliced on the host), rotations' column bits back to the node's slots
int refine_pick(Prog &P, NodeWork &W, RefineWork &F)
{
    mauve_ctx *c = P.c;
    const int64_t n_dp = W.n_dp, nc = (int64_t)F.cands.size();
    uint32_t *dcols = W.dcols; std::vector<int64_t> &dcol_off = W.dcol_off;
    const std::vector<int64_t> &aoff = F.aoff, &asp = F.asp;
    std::vector<int64_t> pick((size_t)n_dp), dsp((size_t)n_dp + 1, 0);      // the batch entry whose alignment the interval keeps, and its score
    for (int64_t iv = 0; iv < n_dp; iv++) { pick[(size_t)iv] = iv; dsp[(size_t)iv] = asp[(size_t)iv]; }
    for (int64_t q = 0; q < nc; q++) {                     // candidates of an interval are consecutive, rotations ascending
        const int64_t iv = F.cands[(size_t)q].iv;
        if (asp[(size_t)(n_dp + q)] > dsp[(size_t)iv]) { dsp[(size_t)iv] = asp[(size_t)(n_dp + q)]; F.replaced += pick[(size_t)iv] == iv; pick[(size_t)iv] = n_dp + q; }
    }
    if (!c->shard_on) {
        const int rc = dp_fetch_picked(c, n_dp, pick.data(), aoff.data(), dcols, dcol_off.data());
        if (rc) return rc;
    } else {
        // (the originals are in dcols already; winners' columns are spliced in below)
        std::copy(aoff.begin(), aoff.begin() + n_dp + 1, dcol_off.begin());
        if (F.replaced) {
            std::vector<uint32_t> ncols; ncols.reserve((size_t)dcol_off[(size_t)n_dp]);
            std::vector<int64_t> noff((size_t)n_dp + 1, 0);
            for (int64_t iv = 0; iv < n_dp; iv++) {
                noff[(size_t)iv] = (int64_t)ncols.size();
                const int64_t q = pick[(size_t)iv];
                if (q == iv) ncols.insert(ncols.end(), dcols + dcol_off[(size_t)iv], dcols + dcol_off[(size_t)iv + 1]);
                else ncols.insert(ncols.end(), F.ccols.data() + (aoff[(size_t)q] - aoff[(size_t)n_dp]), F.ccols.data() + (aoff[(size_t)q + 1] - aoff[(size_t)n_dp]));
            }
            noff[(size_t)n_dp] = (int64_t)ncols.size();
            if ((int64_t)ncols.size() > W.code_total) { c->err = "refinement: more columns than bases"; return MAUVE_ERR_STATE; }
            memcpy(dcols, ncols.data(), ncols.size() * sizeof(uint32_t));
            dcol_off.swap(noff);
        }
    }
    if (dcol_off[(size_t)n_dp] > W.code_total) { c->err = "refinement: more columns than bases"; return MAUVE_ERR_STATE; }
    // winners that are rotations: their column bits are slots of the rotation -> the node's slots
    for (int64_t iv = 0; iv < n_dp; iv++) {
        const int64_t q = pick[(size_t)iv];
        W.dscore[(size_t)iv] = F.ascore[(size_t)q];
        if (q == iv) continue;
        const Cand &cd = F.cands[(size_t)(q - n_dp)];
        uint32_t map[MAUVE_MAX_SEQ];
        for (int j = 0; j < cd.k; j++) map[j] = 1u << cd.nz[(j + cd.r) % cd.k];
        for (int64_t k = dcol_off[(size_t)iv]; k < dcol_off[(size_t)iv + 1]; k++) {
            const uint32_t mc = dcols[(size_t)k]; uint32_t o = 0;
            for (int j = 0; j < cd.k; j++) if (mc >> j & 1u) o |= map[j];
            dcols[(size_t)k] = o;
        }
    }
    return MAUVE_OK;
}

// candidates, the batch (one with device rotations, one with host rows, or -- several contexts -- the two exchanged ones), pick + fetch + remap
int node_refine(Prog &P, NodeWork &W)
{
    mauve_ctx *c = P.c; const mauve_params *p = P.p;
    const int n = W.n; const int64_t n_dp = W.n_dp;
    const double tr0 = now_ms();
    RefineWork F;
    refine_candidates(P, W, F);
    const int64_t nc = (int64_t)F.cands.size(), na = n_dp + nc;
    const std::vector<DpSeqDesc> &all = c->prog_desc;
    const double tr1 = now_ms();
    F.aoff.assign((size_t)na + 1, 0); F.ascore.assign((size_t)na + 1, 0); F.asp.assign((size_t)na + 1, 0);
    int rc;
    if (!c->shard_on && F.rot_dev)
        rc = dp_batch_run_desc_rot(c, n, n_dp, W.desc.data(), F.cbase.data(), na, &p->scoring, F.aoff.data(), F.ascore.data(), &W.cells, F.asp.data());
    else if (!c->shard_on)
        rc = dp_batch_run_desc(c, n, na, all.data(), &p->scoring, nullptr, F.aoff.data(), F.ascore.data(), &W.cells, false, F.asp.data());
    else {
        rc = dp_batch_run_desc(c, n, n_dp, all.data(), &p->scoring, W.dcols, F.aoff.data(), F.ascore.data(), &W.cells, true, F.asp.data());
        if (rc) return rc;
        if (nc) {
            F.ccols.resize((size_t)F.ccodes + 1);
            std::vector<int64_t> coff((size_t)nc + 1, 0);
            int64_t cells2 = 0;
            rc = dp_batch_run_desc(c, n, nc, all.data() + (size_t)n_dp * n, &p->scoring, F.ccols.data(), coff.data(), F.ascore.data() + n_dp, &cells2, true, F.asp.data() + n_dp);
            if (rc) return rc;
            W.cells += cells2;
            for (int64_t q = 0; q <= nc; q++) F.aoff[(size_t)(n_dp + q)] = F.aoff[(size_t)n_dp] + coff[(size_t)q];
        }
    }
    if (rc) return rc;
    const double tr2 = now_ms();
    rc = refine_pick(P, W, F);
    if (rc) return rc;
    if (switches().trace) fprintf(stderr, "[trace] node %d: refinement: %lld candidate alignments of %lld intervals, %lld replaced; candidates %.3f ms, batch %.3f, pick + fetch + remap %.3f\n", W.node,
                         (long long)nc, (long long)n_dp, (long long)F.replaced, tr1 - tr0, tr2 - tr1, now_ms() - tr2);
    return MAUVE_OK;
}

// the node's pieces as blocks of the result: anchors, DP columns (local genome bits -> global ones) or, where no DP ran, the
// stretches genome by genome; the blocks' extents leave the pools
void node_blocks(Prog &P, NodeWork &W)
{
    AlignResult &R = *P.R;
    const std::vector<int> &gm = W.gm; const int n = W.n, N = P.N;
    uint32_t gfull = 0; for (int j = 0; j < n; j++) gfull |= 1u << gm[j];
    // local genome bits -> global ones, a byte at a time
    bool same_bits = true; for (int j = 0; j < n; j++) same_bits = same_bits && gm[j] == j;
    std::vector<std::array<uint32_t, 256>> lut(4);
    if (!same_bits)
        for (int by = 0; by < 4; by++)
            for (int v = 0; v < 256; v++) {
                uint32_t o = 0;
                for (int bit = 0; bit < 8; bit++) { const int j = by * 8 + bit; if ((v >> bit & 1) && j < n) o |= 1u << gm[j]; }
                lut[(size_t)by][(size_t)v] = o;
            }
    std::vector<std::vector<std::pair<int64_t, int64_t>>> placed((size_t)n);
    size_t gi = 0;
    for (size_t q = 0; q < W.pieces.size(); q++) {
        const MatchVec &ch = W.pieces[q];
        R.col_off.push_back((int64_t)R.cols.size());
        R.dp_score.push_back(0);
        P.n_anchor += (int64_t)ch.size(); P.n_multi++;
        for (size_t i = 0; i < ch.size(); i++) {
            R.cols.insert(R.cols.end(), (size_t)ch.len(i), gfull);
            if (gi >= W.gaps.size() || W.gaps[gi].lcb != (int64_t)q || W.gaps[gi].idx != (int64_t)i) continue;
            const GapRef &gr = W.gaps[gi++];
            if (gr.dp) {
                const uint32_t *src = W.dcols + W.dcol_off[(size_t)gr.dp_slot], *end = W.dcols + W.dcol_off[(size_t)gr.dp_slot + 1];
                if (same_bits) R.cols.insert(R.cols.end(), src, end);               // (the root, and any node of genomes 0 .. n-1)
                else {
                    const size_t at = R.cols.size();
                    R.cols.resize(at + (size_t)(end - src));
                    uint32_t *dst = R.cols.data() + at;
                    for (; src < end; src++) { const uint32_t m = *src; *dst++ = lut[0][m & 255] | lut[1][m >> 8 & 255] | lut[2][m >> 16 & 255] | lut[3][m >> 24]; }
                }
                R.dp_score.back() += W.dscore[(size_t)gr.dp_slot];
            } else
                for (int j = 0; j < n; j++) { int64_t lo, ln; gap_of(ch.rec(i), ch.rec(i + 1), j, lo, ln); R.cols.insert(R.cols.end(), (size_t)ln, 1u << gm[j]); }
        }
        const size_t base = R.iv_left.size();
        R.iv_left.resize(base + N, 0); R.iv_right.resize(base + N, 0); R.iv_reverse.resize(base + N, 0);
        for (int j = 0; j < n; j++) {
            int64_t le, re; bool rv;
            chain_extent(ch, j, le, re, rv);
            R.iv_left[base + gm[j]] = le; R.iv_right[base + gm[j]] = re; R.iv_reverse[base + gm[j]] = rv;
            placed[(size_t)j].push_back({le, re});
        }
    }
    for (int j = 0; j < n; j++) for (const auto &pl : placed[(size_t)j]) P.rest[gm[j]].carve(pl.first, pl.second);
}

int prog_node(Prog &P, int node)
{
    if (P.left[node] < 0) return MAUVE_OK;
    mauve_ctx *c = P.c; const mauve_params *p = P.p;
    NodeWork W; W.node = node;
    int rc = node_search(P, W);
    if (rc) return rc;
    node_min_weight(P, W);
    rc = node_chain(P, W);
    if (rc) return rc;
    node_pieces(P, W);
    W.tn2 = now_ms();
    if (p->recursive) { rc = recursive_anchoring(c, p, W.w, W.pieces, W.n, W.gm.data()); if (rc) return rc; }
    W.tn3 = now_ms();
    if (p->gapped) node_split_long(P, W);
    // ---- gapped alignment of the inter-anchor intervals of this node ----
    host_gap_table(W.pieces, W.n, W.gm.data(), p->gapped, p->max_gapped_len, W.gaps, W.desc, W.n_dp, W.code_total);
    HIPCHK(c, c->pin_dcols.ensure(((size_t)W.code_total + 1) * sizeof(uint32_t)));
    W.dcols = c->pin_dcols.as<uint32_t>();
    W.dcol_off.assign((size_t)W.n_dp + 1, 0); W.dscore.assign((size_t)W.n_dp + 1, 0);
    c->dp_band_from = INT64_MAX;            // the progressive path splits long intervals instead
    rc = p->refine_rounds > 0 && W.n >= 3 && W.n_dp > 0 ? node_refine(P, W) : node_dp_plain(P, W);
    if (rc) return rc;
    P.n_gap_dp += W.n_dp; P.n_cells += W.cells;
    { const double tn4 = now_ms(); P.t_seed += W.tn1 - W.tn0; P.t_chain += W.tn2 - W.tn1; P.t_rec += W.tn3 - W.tn2; P.t_dp += tn4 - W.tn3; }
    if (switches().trace) {
        int64_t big = 0; for (const DpSeqDesc &d : W.desc) big = std::max(big, d.len);
        fprintf(stderr, "[trace] node %d (n=%d, pool %lld): seed %.1f ms (%lld mums), chain %.1f, recursion %.1f, dp %.1f ms (%lld intervals, %lld cells, longest side %lld)\n",
                node, W.n, (long long)W.rest_len, W.tn1 - W.tn0, (long long)W.nm, W.tn2 - W.tn1, W.tn3 - W.tn2, now_ms() - W.tn3, (long long)W.n_dp, (long long)W.cells, (long long)big);
    }
    const double tb0 = now_ms();
    node_blocks(P, W);
    P.t_blocks += now_ms() - tb0;
    if (switches().trace) fprintf(stderr, "[trace] node %d: blocks %.1f ms\n", node, now_ms() - tb0);
    rc = prog_node(P, P.left[node]);
    if (rc) return rc;
    return prog_node(P, P.right[node]);
}

}  // namespace

extern "C" {

static int guide_tree_core(mauve_ctx *c, uint64_t pattern, int64_t *dist, int32_t *left, int32_t *right, int64_t bp_min_len, int64_t *bp);

// guide tree only (distance matrix in ppm, UPGMA merge order); dist may be NULL
int mauve_guide_tree(mauve_ctx *c, uint64_t pattern, int64_t *dist, int32_t *left, int32_t *right)
{
    if (!c) return MAUVE_ERR_ARG;
    { const int rg = refuse_past_2g(c, "guide_tree"); if (rg) return rg; }
    return guide_tree_core(c, pattern, dist, left, right, -1, nullptr);
}

// the pairwise breakpoint estimate on its own (symmetric counts, bp[nseq*nseq])
int mauve_breakpoint_counts(mauve_ctx *c, uint64_t pattern, int64_t min_len, int64_t *bp)
{
    if (!c || !bp) return MAUVE_ERR_ARG;
    { const int rg = refuse_past_2g(c, "breakpoint_counts"); if (rg) return rg; }
    if (min_len < 0) { c->err = "breakpoint_counts: min_len must not be negative"; return MAUVE_ERR_ARG; }
    if (c->nseq < 2) { c->err = "breakpoint_counts: at least two genomes required"; return MAUVE_ERR_STATE; }
    std::vector<int32_t> l((size_t)(2 * c->nseq - 1)), r((size_t)(2 * c->nseq - 1));
    return guide_tree_core(c, pattern, nullptr, l.data(), r.data(), min_len, bp);
}

static int guide_tree_core(mauve_ctx *c, uint64_t pattern, int64_t *dist, int32_t *left, int32_t *right, int64_t bp_min_len, int64_t *bp)
{
    if (!c || !left || !right) return MAUVE_ERR_ARG;
    if (c->nseq < 2) { c->err = "guide_tree: at least two genomes required"; return MAUVE_ERR_STATE; }
    HIPCHK(c, hipSetDevice(c->device));
    { int rcm = materialize_tables(c); if (rcm) return rcm; }           // a resident result keeps its tables in buffers the passes below reuse
    const int N = c->nseq, M = 2 * N - 1;
    int64_t nm = 0;
    // similarity = sum of the pairwise match lengths per genome pair: summed on the device, the matches themselves stay there
    c->pair_sums_only = true; c->bp_min_len = bp ? bp_min_len : -1;
    int rc = seedpass_run(c, main_genome_set(c), pattern, MAUVE_MODE_PAIRWISE, 0, 1, nullptr, 0, &nm);
    c->pair_sums_only = false; c->bp_min_len = -1;
    if (rc) return rc;
    std::vector<int64_t> S((size_t)N * N, 0);
    if (c->shard_on) {
        // every rank ran the finder passes of its share of the genome pairs (seed_pass.hip): the sums of the others arrive here
        const size_t nn = (size_t)N * N;
        std::vector<int64_t> mine(2 * nn, 0);                 // length sums, then breakpoints
        if (c->pair_sums.size() == nn) std::copy(c->pair_sums.begin(), c->pair_sums.end(), mine.begin());
        if (bp && c->pair_bp.size() == nn) std::copy(c->pair_bp.begin(), c->pair_bp.end(), mine.begin() + (ptrdiff_t)nn);
        std::vector<std::pair<const char *, size_t>> parts;
        rc = shard_allgather(c, mine.data(), mine.size() * 8, parts);
        if (rc) return rc;
        c->pair_sums.assign(nn, 0); c->pair_bp.assign(nn, 0);
        for (const auto &pt : parts) {
            if (pt.second != mine.size() * 8) { c->err = "guide_tree: ranks disagree about the genome set"; return MAUVE_ERR_STATE; }
            const int64_t *v = reinterpret_cast<const int64_t *>(pt.first);
            for (size_t k = 0; k < nn; k++) { c->pair_sums[k] += v[k]; c->pair_bp[k] += v[nn + k]; }
        }
    }
    if (bp) {
        std::fill(bp, bp + (size_t)N * N, 0);
        if (c->pair_bp.size() == (size_t)N * N)
            for (int a = 0; a < N; a++) for (int b = a + 1; b < N; b++) bp[(size_t)a * N + b] = bp[(size_t)b * N + a] = c->pair_bp[(size_t)a * N + b];
    }
    if (c->pair_sums.size() == (size_t)N * N)
        for (int a = 0; a < N; a++) for (int b = a + 1; b < N; b++) { S[(size_t)a * N + b] = S[(size_t)b * N + a] = c->pair_sums[(size_t)a * N + b]; }
    std::vector<int64_t> D((size_t)M * M, 0), size((size_t)M, 0);
    std::vector<char> active((size_t)M, 0);
    for (int i = 0; i < N; i++) for (int j = 0; j < N; j++) {
        const int64_t mn = std::min(c->lens[i], c->lens[j]); int64_t d = 1000000;
        if (i == j) d = 0;
        else if (mn > 0) d = 1000000 - std::min<int64_t>(1000000, S[(size_t)i * N + j] * 1000000 / mn);
        D[(size_t)i * M + j] = d; if (dist) dist[(size_t)i * N + j] = d;
    }
    for (int i = 0; i < N; i++) { active[i] = 1; size[i] = 1; left[i] = right[i] = -1; }
    for (int k = N; k < M; k++) {
        int ba = -1, bb = -1; int64_t bd = 0;
        for (int a = 0; a < k; a++) if (active[a]) for (int b = a + 1; b < k; b++) if (active[b])
            if (ba < 0 || D[(size_t)a * M + b] < bd) { ba = a; bb = b; bd = D[(size_t)a * M + b]; }
        left[k] = ba; right[k] = bb; size[k] = size[ba] + size[bb];
        for (int x = 0; x < k; x++) if (active[x] && x != ba && x != bb)
            D[(size_t)k * M + x] = D[(size_t)x * M + k] = (size[ba] * D[(size_t)ba * M + x] + size[bb] * D[(size_t)bb * M + x]) / size[k];
        active[ba] = active[bb] = 0; active[k] = 1;
    }
    return MAUVE_OK;
}

static int progressive_core(mauve_ctx *c, const mauve_params *p, mauve_align_sizes *sizes, const int32_t *given_left,
                            const int32_t *given_right, int32_t *tree_left, int32_t *tree_right, int64_t *dist);

int mauve_progressive_align(mauve_ctx *c, const mauve_params *p, mauve_align_sizes *sizes, int32_t *tree_left,
                            int32_t *tree_right, int64_t *dist)
{
    if (!c) return MAUVE_ERR_ARG;
    { const int rg = refuse_past_2g(c, "progressive_align"); if (rg) return rg; }
    if (p) { const int rs = refuse_scoring_params(c, p, "progressive_align"); if (rs) return rs; }
    return progressive_core(c, p, sizes, nullptr, nullptr, tree_left, tree_right, dist);
}

// the caller's guide tree instead of the UPGMA one: leaves 0..N-1 childless, every internal node N..2N-2 with two
// distinct children of smaller id, every node but the root 2N-2 used exactly once
int mauve_progressive_align_tree(mauve_ctx *c, const mauve_params *p, mauve_align_sizes *sizes, const int32_t *tree_left,
                                 const int32_t *tree_right)
{
    if (!c || !tree_left || !tree_right) return MAUVE_ERR_ARG;
    { const int rg = refuse_past_2g(c, "progressive_align_tree"); if (rg) return rg; }
    if (p) { const int rs = refuse_scoring_params(c, p, "progressive_align_tree"); if (rs) return rs; }
    const int N = c->nseq, M = 2 * N - 1;
    if (N < 2) { c->err = "progressive_align: at least two genomes required"; return MAUVE_ERR_STATE; }
    std::vector<char> used((size_t)M, 0);
    for (int k = 0; k < M; k++) {
        const int a = tree_left[k], b = tree_right[k];
        if (k < N) { if (a != -1 || b != -1) { c->err = "progressive_align_tree: a leaf has children"; return MAUVE_ERR_ARG; } continue; }
        if (a < 0 || b < 0 || a >= k || b >= k || a == b || used[(size_t)a] || used[(size_t)b]) {
            c->err = "progressive_align_tree: not a binary tree in merge order"; return MAUVE_ERR_ARG;
        }
        used[(size_t)a] = used[(size_t)b] = 1;
    }
    return progressive_core(c, p, sizes, tree_left, tree_right, nullptr, nullptr, nullptr);
}

}  // extern "C"

static int progressive_core(mauve_ctx *c, const mauve_params *p, mauve_align_sizes *sizes, const int32_t *given_left,
                            const int32_t *given_right, int32_t *tree_left, int32_t *tree_right, int64_t *dist)
{
    if (!c || !p || !sizes) return MAUVE_ERR_ARG;
    if (c->nseq < 2) { c->err = "progressive_align: at least two genomes required"; return MAUVE_ERR_STATE; }
    if (p->lcb_scoring != MAUVE_LCB_SCORE_LENGTH && p->lcb_scoring != MAUVE_LCB_SCORE_SP) { c->err = "progressive_align: unknown lcb_scoring"; return MAUVE_ERR_ARG; }
    if (p->seed_family && p->seed_pattern) { c->err = "progressive_align: seed_family takes its patterns from the weight, not from seed_pattern"; return MAUVE_ERR_ARG; }
    HIPCHK(c, hipSetDevice(c->device));
    c->rec_flags.clear();                 // (an earlier call that ended before its recursion may have left its flags behind)
    const double t0 = now_ms();
    const int N = c->nseq;
    int64_t sum = 0; for (int g = 0; g < N; g++) sum += c->lens[g];
    int w; uint64_t pat;
    { const int rs = resolve_seed(c, p, sum / N, "progressive_align", &w, &pat); if (rs) return rs; }
    RepeatScope rp_scope(c);                         // whole-genome multiplicities of the root pattern, once for every node
    { const int rr = repeat_begin(c, p, w, pat); if (rr) return rr; }
    Prog P; P.c = c; P.p = p; P.N = N;
    P.left.assign((size_t)(2 * N - 1), -1); P.right.assign((size_t)(2 * N - 1), -1);
    int rc = 0;
    if (given_left) { std::copy(given_left, given_left + (2 * N - 1), P.left.begin()); std::copy(given_right, given_right + (2 * N - 1), P.right.begin()); }
    const bool need_bp = p->weight_scaling && p->bp_dist_scale_ppm > 0;
    const int64_t bp_min = p->bp_dist_min_score >= 0 ? p->bp_dist_min_score : 2 * (int64_t)w;
    if (need_bp) P.bpd.assign((size_t)N * N, 0);
    bool have_bp = false;
    if (!given_left) { rc = guide_tree_core(c, pat, dist, P.left.data(), P.right.data(), bp_min, need_bp ? P.bpd.data() : nullptr); have_bp = need_bp; }
    if (rc) return rc;
    if (p->weight_scaling) {                // the distances come from the pairwise matches even when the tree is the caller's
        P.dist.assign((size_t)N * N, 0);
        if (given_left || !dist) {
            std::vector<int32_t> tl((size_t)(2 * N - 1)), tr((size_t)(2 * N - 1));
            rc = guide_tree_core(c, pat, P.dist.data(), tl.data(), tr.data(), bp_min, need_bp && !have_bp ? P.bpd.data() : nullptr);
            if (rc) return rc;
        } else std::copy(dist, dist + (size_t)N * N, P.dist.begin());
        if (need_bp) {                      // relative to the most rearranged pair
            int64_t mx = 0; for (int64_t v : P.bpd) mx = std::max(mx, v);
            for (int64_t &v : P.bpd) v = mx ? v * 1000000 / mx : 0;
        }
    }
    const bool trace = switches().trace;
    const double tg1 = now_ms();
    if (trace) fprintf(stderr, "[trace] progressive: guide tree %.1f ms\n", tg1 - t0);
    if (tree_left) std::copy(P.left.begin(), P.left.end(), tree_left);
    if (tree_right) std::copy(P.right.begin(), P.right.end(), tree_right);
    AlignResult &R = c->res;
    result_reset(R);
    R.cols.clear(); R.cols_fill = 0; R.cols_dirty.clear();           // mauve_align's prefilled-buffer invariant no longer holds
    P.R = &R;
    P.rest.assign((size_t)N, FreePool());
    for (int g = 0; g < N; g++) P.rest[(size_t)g].reset(c->lens[g]);
    rc = prog_node(P, 2 * N - 2);
    if (rc) return rc;
    const double tg2 = now_ms();
    if (trace) fprintf(stderr, "[trace] progressive: nodes %.1f ms\n", tg2 - tg1);
    const int64_t n_multi = P.n_multi;
    if (p->add_unaligned)
        for (int g = 0; g < N; g++)
            for (const auto &fr : P.rest[(size_t)g].free_) {
                const int64_t lo = fr.first, hi = fr.second;
                R.col_off.push_back((int64_t)R.cols.size());
                R.cols.insert(R.cols.end(), (size_t)(hi - lo + 1), 1u << g);
                for (int h = 0; h < N; h++) { R.iv_left.push_back(h == g ? lo : 0); R.iv_right.push_back(h == g ? hi : 0); R.iv_reverse.push_back(0); }
                R.dp_score.push_back(0);
            }
    R.col_off.push_back((int64_t)R.cols.size());
    // the multi-genome blocks double as the "LCB" table of the result (signed ends, weight unused)
    R.lcb_left.assign((size_t)n_multi * N, 0); R.lcb_right.assign((size_t)n_multi * N, 0); R.lcb_weight.assign((size_t)n_multi, 0);
    for (int64_t b = 0; b < n_multi; b++) for (int g = 0; g < N; g++) {
        const int64_t le = R.iv_left[(size_t)b * N + g], re = R.iv_right[(size_t)b * N + g];
        const bool rv = R.iv_reverse[(size_t)b * N + g] != 0;
        R.lcb_left[(size_t)b * N + g] = rv ? -le : le; R.lcb_right[(size_t)b * N + g] = rv ? -re : re;
    }
    R.sz.n_mums = 0; R.sz.n_lcb = n_multi; R.sz.n_anchor = 0; R.sz.n_iv = (int64_t)R.dp_score.size();
    R.n_cols = R.cols.size();
    R.sz.n_cols = (int64_t)R.cols.size(); R.sz.n_gap_dp = P.n_gap_dp; R.sz.n_dp_cells = P.n_cells;
    *sizes = R.sz;
    memset(&c->stage, 0, sizeof c->stage);
    c->stage.tree_ms = tg1 - t0; c->stage.seed_ms = P.t_seed; c->stage.chain_ms = P.t_chain; c->stage.recurse_ms = P.t_rec; c->stage.dp_ms = P.t_dp;
    c->stage.assemble_ms = P.t_blocks + (now_ms() - tg2);
    c->stage.total_ms = now_ms() - t0;
    return MAUVE_OK;
}
