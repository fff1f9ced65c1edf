// libMems/CoordinateIndex.h -- coordinate translation through an alignment, batched on the device.
// libMems answers "where is this base in the other genomes?" one question at a time, with a walk over the columns of the
// interval: Interval::GetColumn (coordinateTranslate.cpp:36-46) and CompactGappedAlignment::SeqPosToColumn
// (getOrthologList.cpp:219-220, bbBreakOnGenes.cpp:154-155, randomGeneSample.cpp:139-140, scoreProcrastAlignment.cpp:293-303).
// Those two stay as they are (Interval.h, CompactGappedAlignment.h).  HipCoordinateIndex builds a rank/select index of a whole
// IntervalList once (mauve_coord_index_alignment), or of the alignment the context holds (mauve_coord_index), and answers
// batches; a gene table or a variant list is one call.
// The index lives in the context: one at a time, the next HipCoordinateIndex on the same context replaces it.  It is a snapshot --
// searches and alignments that run on the context afterwards leave it as it is, and it does not follow later changes to the list.
#ifndef MAUVE_HIP_COORDINATEINDEX_H
#define MAUVE_HIP_COORDINATEINDEX_H

#include "IntervalList.h"

namespace mems {

// an IntervalList in the arrays of mauve_align_fetch, as the entry points that take a caller's alignment want it (cols is never empty)
struct HipIntervalArrays {
    size_t K;
    uint N;
    std::vector<int64_t> left, right, col_off;
    std::vector<int8_t> rev;
    std::vector<uint32_t> cols;
    HipIntervalArrays(const IntervalList &il, const char *who) : K(il.size()), N((uint)il.seq_table.size())
    {
        for (const Interval &iv : il) N = std::max(N, iv.SeqCount());
        if (N == 0) throw genome::gnException(std::string(who) + ": the interval list names no sequence");
        left.assign(K * N, 0); right.assign(K * N, 0); col_off.assign(K + 1, 0); rev.assign(K * N, 0);
        for (size_t i = 0; i < K; i++) {
            const Interval &iv = il[i];
            for (uint g = 0; g < iv.SeqCount(); g++) {
                left[i * N + g] = (int64_t)iv.LeftEnd(g); right[i * N + g] = iv.LeftEnd(g) ? (int64_t)iv.RightEnd(g) : 0;
                rev[i * N + g] = iv.LeftEnd(g) && iv.Orientation(g) == AbstractMatch::reverse;
            }
            cols.insert(cols.end(), iv.Columns().begin(), iv.Columns().end());
            col_off[i + 1] = (int64_t)cols.size();
        }
        if (cols.empty()) cols.push_back(0);
    }
};

class HipCoordinateIndex {
public:
    // the index of a caller's alignment: every base of a sequence may lie in at most one interval of the list (else gnException)
    explicit HipCoordinateIndex(const IntervalList &il, HipContext &hc = HipContext::global()) : hc_(&hc)
    {
        const HipIntervalArrays a(il, "HipCoordinateIndex");
        hc.check(mauve_coord_index_alignment(hc.get(), (int)a.N, (int64_t)a.K, a.left.data(), a.right.data(), a.rev.data(), a.col_off.data(), a.cols.data()), "mauve_coord_index_alignment");
        n_ = a.N;
    }
    // the index of the alignment the context holds (after Aligner::align / ProgressiveAligner::align); the sequence count is the alignment's
    explicit HipCoordinateIndex(HipContext &hc) : hc_(&hc), n_(0)
    {
        hc.check(mauve_coord_index(hc.get()), "mauve_coord_index");
        int n = 0;
        hc.check(mauve_coord_index_size(hc.get(), &n, nullptr, nullptr), "mauve_coord_index_size");
        n_ = (uint)n;
    }

    uint SeqCount() const { return n_; }
    HipContext &context() const { return *hc_; }          // the context the index lives in (AlignmentExtractor.h works on it)

    // Interval::GetColumn for a batch: query q asks for column cols[q] of interval blocks[q].  pos[q * SeqCount() + g] is the signed
    // position of sequence g's residue there (negative = reverse strand), 0 where g is absent or gapped; defined[q]: bit g set = a
    // residue of g is in the column.  nearest: a gapped sequence gets the residue before the column, else its first one, as
    // coordinateTranslate promises ("the nearest aligned position"); its bit stays clear.
    void GetColumns(const std::vector<int64_t> &blocks, const std::vector<int64_t> &cols, std::vector<int64_t> &pos, std::vector<uint32_t> &defined, bool nearest = false) const
    {
        still_mine();
        if (blocks.size() != cols.size()) throw genome::gnException("HipCoordinateIndex::GetColumns: blocks and cols differ in length");
        pos.assign(blocks.size() * n_, 0); defined.assign(blocks.size(), 0);
        hc_->check(mauve_column_positions(hc_->get(), (int64_t)blocks.size(), blocks.data(), cols.data(), nearest ? 1 : 0, pos.data(), defined.data()), "mauve_column_positions");
    }
    // CompactGappedAlignment::SeqPosToColumn for a batch, over the whole list: base positions[q] (1-based) of sequence seqs[q] lies in
    // column cols[q] of interval blocks[q]; -1 / -1 where no interval of the list holds the base (libMems throws there)
    void SeqPosToColumn(const std::vector<int32_t> &seqs, const std::vector<int64_t> &positions, std::vector<int64_t> &blocks, std::vector<int64_t> &cols) const
    {
        if (seqs.size() != positions.size()) throw genome::gnException("HipCoordinateIndex::SeqPosToColumn: seqs and positions differ in length");
        still_mine();
        blocks.assign(seqs.size(), -1); cols.assign(seqs.size(), -1);
        hc_->check(mauve_seqpos_to_column(hc_->get(), (int64_t)seqs.size(), seqs.data(), positions.data(), blocks.data(), cols.data()), "mauve_seqpos_to_column");
    }
    // the two in turn (coordinateTranslate's whole job): out[q * SeqCount() + g] = where base positions[q] of seqs[q] is in sequence g
    void Translate(const std::vector<int32_t> &seqs, const std::vector<int64_t> &positions, std::vector<int64_t> &out, std::vector<uint32_t> &defined, std::vector<int64_t> &blocks,
                   bool nearest = false) const
    {
        if (seqs.size() != positions.size()) throw genome::gnException("HipCoordinateIndex::Translate: seqs and positions differ in length");
        still_mine();
        out.assign(seqs.size() * n_, 0); defined.assign(seqs.size(), 0); blocks.assign(seqs.size(), -1);
        hc_->check(mauve_translate_positions(hc_->get(), (int64_t)seqs.size(), seqs.data(), positions.data(), nearest ? 1 : 0, out.data(), defined.data(), blocks.data()),
                   "mauve_translate_positions");
    }
private:
    // the answer arrays are sized by this object's sequence count: the index in force must still have it (another HipCoordinateIndex on
    // the same context replaces the index)
    void still_mine() const
    {
        int n = 0;
        hc_->check(mauve_coord_index_size(hc_->get(), &n, nullptr, nullptr), "mauve_coord_index_size");
        if ((uint)n != n_) throw genome::gnException("HipCoordinateIndex: the context's index was replaced by one over another number of sequences");
    }
    HipContext *hc_;
    uint n_;
};

}  // namespace mems
#endif
