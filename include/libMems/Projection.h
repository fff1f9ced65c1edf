// libMems/Projection.h -- an alignment projected onto a subset of its sequences, what becomes collinear coalesced into new LCBs, made on
// the device.  libMems' projectIntervalList (alignmentProjector.cpp:58-77, multiEVD.cpp:142-172, bbBreakOnGenes.cpp:54) and
// the loop projectAndStrip writes out by hand (projectAndStrip.cpp:75-122) keep the intervals in which every chosen sequence is present,
// invert those whose first chosen sequence is reversed, and chain what is left into LCBs, interval by interval on the host.  The host
// projectIntervalList stays (ProgressiveAligner.h) and is the brute-force check.  HipProjection does it for a whole IntervalList in one
// call (mauve_project) on a HipCoordinateIndex of that list, and can make the result the index in force (mauve_project_index) without
// a column crossing the host link: the coordinate, extraction, statistics and excursion classes then work on the projection unchanged.
#ifndef MAUVE_HIP_PROJECTION_H
#define MAUVE_HIP_PROJECTION_H

#include "CoordinateIndex.h"

namespace mems {

// where the projection came from: output interval o is made of the source intervals pieces[piece_off[o] .. piece_off[o + 1]) in column
// order, flipped[] tells which were inverted; source_col[] is every output column's column in the whole column array of the source
// (the intervals of the list one after another), -1 for a filler column
struct ProjectionSource { std::vector<int64_t> piece_off, pieces, source_col; std::vector<int8_t> flipped; };

class HipProjection {
public:
    // the projection of the index's alignment onto `projection` (distinct sequence ids, the first one sets the order and the strands);
    // drop_empty: columns in which no projected sequence has a residue are left out
    HipProjection(const HipCoordinateIndex &ix, const std::vector<uint> &projection, bool drop_empty = true) : ix_(&ix), proj_(projection)
    {
        HipContext &hc = ix.context();
        mauve_project_params p;
        mauve_default_project_params((int)ix.SeqCount(), &p);
        if (projection.size() > MAUVE_MAX_SEQ) throw genome::gnException("HipProjection: projection longer than the sequence limit");
        p.n_proj = (int32_t)projection.size();
        for (size_t k = 0; k < projection.size(); k++) p.proj[k] = (int32_t)projection[k];
        p.drop_empty = drop_empty ? 1 : 0;
        hc.check(mauve_project(hc.get(), &p, &sz_), "mauve_project");
        mine_ = ++latest();
    }
    size_t IntervalCount() const { return (size_t)sz_.n_iv; }
    size_t ColumnCount() const { return (size_t)sz_.n_cols; }
    size_t FillerColumns() const { return (size_t)sz_.n_fill; }

    // the projection as an interval list.  compact = false: over all sequences of the source, the others absent (the form that can be
    // indexed in the source's place); compact = true: over the projected sequences alone, in projection order (alignmentProjector's
    // output).  seq_table / seq_filename are the caller's to fill.
    void GetIntervals(IntervalList &out, bool compact = false, ProjectionSource *where = nullptr) const
    {
        still_mine();
        HipContext &hc = ix_->context();
        const size_t K = (size_t)sz_.n_iv, W = compact ? proj_.size() : ix_->SeqCount(), C = (size_t)sz_.n_cols;
        std::vector<int64_t> left(K * W + 1), right(K * W + 1), col_off(K + 1);
        std::vector<int8_t> rev(K * W + 1);
        std::vector<uint32_t> cols(C + 1);
        ProjectionSource w;
        w.piece_off.assign(K + 1, 0); w.pieces.assign((size_t)sz_.n_src, 0); w.flipped.assign((size_t)sz_.n_src, 0); w.source_col.assign(where ? C : 0, 0);
        hc.check(mauve_project_fetch(hc.get(), compact ? 1 : 0, left.data(), right.data(), rev.data(), col_off.data(), cols.data(), w.piece_off.data(),
                                     w.pieces.empty() ? nullptr : w.pieces.data(), w.flipped.empty() ? nullptr : w.flipped.data(), w.source_col.empty() ? nullptr : w.source_col.data()),
                 "mauve_project_fetch");
        out.clear();
        for (size_t i = 0; i < K; i++) {
            std::vector<int64> l(left.begin() + i * W, left.begin() + (i + 1) * W), r(right.begin() + i * W, right.begin() + (i + 1) * W);
            std::vector<char> rv(rev.begin() + i * W, rev.begin() + (i + 1) * W);
            out.push_back(Interval(l, r, rv, std::vector<uint32_t>(cols.begin() + col_off[i], cols.begin() + col_off[i + 1])));
        }
        if (where) { where->piece_off.swap(w.piece_off); where->pieces.swap(w.pieces); where->flipped.swap(w.flipped); where->source_col.swap(w.source_col); }
    }
    // the projection becomes the index in force on the context (the HipCoordinateIndex it was made from keeps answering: the sequence
    // count is the same); the sequences must be resident and no older than that index
    void MakeIndex() const { still_mine(); ix_->context().check(mauve_project_index(ix_->context().get()), "mauve_project_index"); }
private:
    // A context holds one projection, the last one made, and mauve_project_fetch writes that one: the arrays here are sized by this
    // object's, so a later HipProjection (multiEVD makes one per discarded genome) ends this one -- it throws instead of writing past its
    // vectors.  (A mauve_project call made beside this class is not seen: do not mix the two on one context.)
    static uint64_t &latest() { static uint64_t n = 0; return n; }
    void still_mine() const
    {
        if (mine_ != latest()) throw genome::gnException("HipProjection: a later projection replaced this one on the context (fetch or index a projection before the next is made)");
    }
    uint64_t mine_;
    const HipCoordinateIndex *ix_;
    std::vector<uint> proj_;
    mauve_project_sizes sz_;
};

}  // namespace mems
#endif
