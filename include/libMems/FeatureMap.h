// libMems/FeatureMap.h -- annotated ranges mapped through an alignment, and the feature of every sequence that is their counterpart, made
// on the device.  Four of libMems' tools are built around one walk (getOrthologList.cpp:137-313,
// randomGeneSample.cpp:118-157, bbBreakOnGenes.cpp:140-160, scoreProcrastAlignment.cpp:285-305): find the intervals a gene intersects,
// clip the gene to each, CompactGappedAlignment::SeqPosToColumn on both ends, copyRange, LeftEnd / RightEnd of every row, and look up the
// features that intersect that extent.  SeqPosToColumn, copyRange, LeftEnd and RightEnd stay as they are (CompactGappedAlignment.h) and are
// the brute-force check.  HipFeatureMap answers for a whole gene table in one call (mauve_map_ranges) on a HipCoordinateIndex, joins
// extents against feature tables (mauve_range_overlaps), and composes getOrthologList's row for a batch of genes.
#ifndef MAUVE_HIP_FEATUREMAP_H
#define MAUVE_HIP_FEATUREMAP_H

#include "PairStatistics.h"

namespace mems {

// bases [lo, hi] (1-based) of sequence seq: a gene, a feature
struct AnnotatedRange { uint seq; int64_t lo, hi; };
// mauve_map_ranges_fetch: query q owns the pieces piece_off[q] .. piece_off[q + 1]; the per-row arrays are [piece * SeqCount() + g].
// (block, col, len) of a piece is a ColumnRange of the indexed list
struct RangePieces {
    std::vector<int64_t> piece_off, covered, best, piece_query, piece_block, piece_col, piece_len, clip_lo, clip_hi, n_res, ext_left, ext_right;
    size_t PieceCount() const { return piece_block.size(); }
    bool Rearranged(size_t q) const { return piece_off[q + 1] - piece_off[q] > 1; }       // what getOrthologList marks with '*'
};
// mauve_range_overlaps, per query: the features sharing a base with it, the index of the one sharing the most (-1: none), that many bases
struct RangeOverlaps { std::vector<int64_t> n_hit, best, overlap; };
// getOrthologList's row of one gene: the interval of its best piece (-1: the gene lies in no interval), per sequence the counterpart
// feature (index in the feature table, -1: none) and the bases they share, the mean pairwise identity of the piece, the '*' flag
struct OrthologRow { int64_t block; std::vector<int64_t> ortholog, overlap; double identity; bool rearranged; };

class HipFeatureMap {
public:
    explicit HipFeatureMap(const HipCoordinateIndex &ix) : ix_(&ix) {}

    void MapRanges(const std::vector<AnnotatedRange> &genes, RangePieces &out) const
    {
        HipContext &hc = ix_->context();
        const size_t n = genes.size(), N = ix_->SeqCount();
        std::vector<int32_t> seq(n + 1);
        std::vector<int64_t> lo(n + 1), hi(n + 1);
        for (size_t q = 0; q < n; q++) { seq[q] = (int32_t)genes[q].seq; lo[q] = genes[q].lo; hi[q] = genes[q].hi; }
        mauve_range_map_sizes sz;
        hc.check(mauve_map_ranges(hc.get(), (int64_t)n, seq.data(), lo.data(), hi.data(), &sz), "mauve_map_ranges");
        const size_t P = (size_t)sz.n_piece;
        out.piece_off.assign(n + 1, 0); out.covered.assign(n, 0); out.best.assign(n, -1);
        for (std::vector<int64_t> *v : {&out.piece_query, &out.piece_block, &out.piece_col, &out.piece_len, &out.clip_lo, &out.clip_hi}) v->assign(P, 0);
        for (std::vector<int64_t> *v : {&out.n_res, &out.ext_left, &out.ext_right}) v->assign(P * N, 0);
        hc.check(mauve_map_ranges_fetch(hc.get(), out.piece_off.data(), out.covered.data(), out.best.data(), out.piece_query.data(), out.piece_block.data(), out.piece_col.data(),
                                        out.piece_len.data(), out.clip_lo.data(), out.clip_hi.data(), out.n_res.data(), out.ext_left.data(), out.ext_right.data()),
                 "mauve_map_ranges_fetch");
    }
    // queries as (sequence, lo, hi) arrays, ends signed as the extents of RangePieces are, (0, 0) = nothing
    void Overlaps(const std::vector<AnnotatedRange> &features, const std::vector<int32_t> &q_seq, const std::vector<int64_t> &q_lo, const std::vector<int64_t> &q_hi,
                  RangeOverlaps &out) const
    {
        if (q_seq.size() != q_lo.size() || q_seq.size() != q_hi.size()) throw genome::gnException("HipFeatureMap::Overlaps: the query arrays differ in length");
        HipContext &hc = ix_->context();
        const size_t m = features.size(), n = q_seq.size();
        std::vector<int32_t> seq(m + 1);
        std::vector<int64_t> lo(m + 1), hi(m + 1);
        for (size_t t = 0; t < m; t++) { seq[t] = (int32_t)features[t].seq; lo[t] = features[t].lo; hi[t] = features[t].hi; }
        out.n_hit.assign(n, 0); out.best.assign(n, -1); out.overlap.assign(n, 0);
        if (!n) return;
        hc.check(mauve_range_overlaps(hc.get(), (int64_t)m, seq.data(), lo.data(), hi.data(), (int64_t)n, q_seq.data(), q_lo.data(), q_hi.data(), out.n_hit.data(),
                                      out.best.data(), out.overlap.data()), "mauve_range_overlaps");
    }
    // the genes mapped, each gene's best piece taken, its extents joined against the features of all sequences (one table), the identity
    // of the piece's columns from mauve_pair_stats with the pieces as ranges: the mean, over the pairs a < b in which both sequences have
    // a residue in some column of the piece, of identical columns / such columns; 0.0 without such a pair.  The sequences must be
    // resident on the index's context (as for HipPairStatistics)
    std::vector<OrthologRow> OrthologRows(const std::vector<AnnotatedRange> &genes, const std::vector<AnnotatedRange> &features) const
    {
        const size_t n = genes.size(), N = ix_->SeqCount(), P = N * (N - 1) / 2;
        RangePieces m;
        MapRanges(genes, m);
        std::vector<OrthologRow> rows(n);
        std::vector<size_t> have;
        std::vector<int32_t> q_seq;
        std::vector<int64_t> q_lo, q_hi;
        std::vector<ColumnRange> ranges;
        for (size_t q = 0; q < n; q++) {
            rows[q].block = -1; rows[q].ortholog.assign(N, -1); rows[q].overlap.assign(N, 0); rows[q].identity = 0.0; rows[q].rearranged = m.Rearranged(q);
            if (m.best[q] < 0) continue;
            const size_t b = (size_t)m.best[q];
            have.push_back(q);
            rows[q].block = m.piece_block[b];
            ranges.push_back(ColumnRange{m.piece_block[b], m.piece_col[b], m.piece_len[b]});
            for (size_t g = 0; g < N; g++) { q_seq.push_back((int32_t)g); q_lo.push_back(m.ext_left[b * N + g]); q_hi.push_back(m.ext_right[b * N + g]); }
        }
        if (have.empty()) return rows;
        RangeOverlaps ov;
        Overlaps(features, q_seq, q_lo, q_hi, ov);
        const HipPairStatistics::Records st = HipPairStatistics(*ix_).Count(nullptr, &ranges, true);
        std::vector<double> id(have.size() * P + 1, 0.0);
        mauve_pair_stats_identity(st.data(), (int64_t)(have.size() * P), id.data());
        for (size_t k = 0; k < have.size(); k++) {
            OrthologRow &r = rows[have[k]];
            for (size_t g = 0; g < N; g++) { r.ortholog[g] = ov.best[k * N + g]; r.overlap[g] = ov.overlap[k * N + g]; }
            double total = 0.0; size_t count = 0;
            for (size_t p = 0; p < P; p++) {
                const int64_t *s = &st[(k * P + p) * MAUVE_PAIR_STATS_WORDS];
                int64_t both = 0;
                for (int w = 0; w < 25; w++) both += s[w];
                if (both > 0) { total += id[k * P + p]; count++; }
            }
            r.identity = count ? total / (double)count : 0.0;
        }
        return rows;
    }
private:
    const HipCoordinateIndex *ix_;
};

}  // namespace mems
#endif
