// libMems/AlignmentExtractor.h -- the letters of chosen alignment columns in chosen sequences, made on the device.
// libMems tools that project an alignment onto a subset of its sequences, keep its gap-free columns or cut windows out of it
// (stripGapColumns.cpp:32-64, projectAndStrip.cpp:75-101, stripSubsetLCBs.cpp:125-142, createBackboneMFA.cpp:28-37,
// alignmentProjector.cpp:58-77) ask every interval for its GetAlignment strings and pick letters out of them on the host.
// Interval::GetAlignment stays as it is (Interval.h).  HipAlignmentExtractor answers the same question for a whole IntervalList in one
// selection and one fetch (mauve_extract_select / mauve_extract_fetch), on a HipCoordinateIndex of that list and the sequences
// resident on the index's context: upload them (MatchList::upload, or mauve_set_genomes*) BEFORE the index is built -- an index older
// than the resident sequences is refused.
#ifndef MAUVE_HIP_ALIGNMENTEXTRACTOR_H
#define MAUVE_HIP_ALIGNMENTEXTRACTOR_H

#include "CoordinateIndex.h"

namespace mems {

// which rows, which columns: projection = the sequences to write, in that order (empty: all of them); a column is taken only if every
// sequence of the require mask has a residue in it, with drop_empty only if one of the projection has, with polymorphic only if the
// projection's A/C/G/T cells show two different letters
struct ExtractParams {
    std::vector<uint> projection;
    uint32_t require = 0;
    bool drop_empty = false, polymorphic = false;
};
// columns [col, col + len) of interval `block` of the list
struct ColumnRange { int64_t block, col, len; };
// where the selected columns came from: (blocks[j], cols[j]) is column j of the rows (the form HipCoordinateIndex::GetColumns takes),
// range_off[r] .. range_off[r + 1] the slice of range r
struct ExtractedColumns { std::vector<int64_t> blocks, cols, range_off; };

class HipAlignmentExtractor {
public:
    explicit HipAlignmentExtractor(const HipCoordinateIndex &ix) : ix_(&ix) {}

    // rows[k] = the letters of sequence projection[k] in the selected columns, '-' where it is absent or gapped; ranges == nullptr: every
    // interval whole, in list order
    std::vector<std::string> Extract(const ExtractParams &p, const std::vector<ColumnRange> *ranges = nullptr, ExtractedColumns *where = nullptr) const
    {
        HipContext &hc = ix_->context();
        mauve_extract_params q;
        mauve_default_extract_params((int)ix_->SeqCount(), &q);
        if (!p.projection.empty()) {
            if (p.projection.size() > MAUVE_MAX_SEQ) throw genome::gnException("HipAlignmentExtractor: projection longer than the sequence limit");
            q.n_keep = (int32_t)p.projection.size();
            for (size_t k = 0; k < p.projection.size(); k++) q.keep[k] = (int32_t)p.projection[k];
        }
        q.require = p.require; q.drop_empty = p.drop_empty; q.polymorphic = p.polymorphic;
        int64_t n_sel = 0, n_range = 0;
        if (ranges) {
            std::vector<int64_t> b(ranges->size() + 1), c(ranges->size() + 1), l(ranges->size() + 1);
            for (size_t r = 0; r < ranges->size(); r++) { b[r] = (*ranges)[r].block; c[r] = (*ranges)[r].col; l[r] = (*ranges)[r].len; }
            n_range = (int64_t)ranges->size();
            hc.check(mauve_extract_select(hc.get(), &q, n_range, b.data(), c.data(), l.data(), &n_sel), "mauve_extract_select");
        } else {
            hc.check(mauve_extract_select(hc.get(), &q, 0, nullptr, nullptr, nullptr, &n_sel), "mauve_extract_select");
            hc.check(mauve_coord_index_size(hc.get(), nullptr, &n_range, nullptr), "mauve_coord_index_size");
        }
        std::vector<std::string> rows((size_t)q.n_keep);
        std::vector<char> flat((size_t)q.n_keep * (size_t)n_sel + 1);
        ExtractedColumns w;
        w.blocks.assign((size_t)n_sel, 0); w.cols.assign((size_t)n_sel, 0); w.range_off.assign((size_t)n_range + 1, 0);
        hc.check(mauve_extract_fetch(hc.get(), flat.data(), n_sel, w.blocks.data(), w.cols.data(), w.range_off.data()), "mauve_extract_fetch");
        for (size_t k = 0; k < rows.size(); k++) rows[k].assign(flat.data() + k * (size_t)n_sel, (size_t)n_sel);
        if (where) where->blocks.swap(w.blocks), where->cols.swap(w.cols), where->range_off.swap(w.range_off);
        return rows;
    }
    // stripGapColumns applied to the projection (stripGapColumns.cpp:32-64, projectAndStrip.cpp:75-101): the columns in which every
    // sequence of the projection has a residue
    std::vector<std::string> StripGapColumns(const std::vector<uint> &projection, const std::vector<ColumnRange> *ranges = nullptr, ExtractedColumns *where = nullptr) const
    {
        ExtractParams p;
        p.projection = projection;
        if (projection.empty()) p.require = ix_->SeqCount() >= 32 ? ~0u : (1u << ix_->SeqCount()) - 1u;
        for (uint g : projection) { if (g >= 32) throw genome::gnException("HipAlignmentExtractor::StripGapColumns: sequence index out of range"); p.require |= 1u << g; }
        return Extract(p, ranges, where);
    }
private:
    const HipCoordinateIndex *ix_;
};

}  // namespace mems
#endif
