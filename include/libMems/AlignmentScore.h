// libMems/AlignmentScore.h -- an alignment scored against a correct one on the device.
// The reference answers "is this alignment right?" with a tool of its own, scoreAlignment <correct alignment> <calculated alignment>
// (scoreAlignment.cpp:99-457): for every base of the correct alignment and every other sequence it asks the calculated alignment what
// it aligned there, one column walk per question.  HipAlignmentScore keeps the correct IntervalList as a second coordinate index in the
// context (mauve_score_truth) and scores any number of calculated lists against it, one HipCoordinateIndex and one count
// (mauve_score_alignment) each.  No sequence data is needed.
#ifndef MAUVE_HIP_ALIGNMENTSCORE_H
#define MAUVE_HIP_ALIGNMENTSCORE_H

#include <ostream>
#include "CoordinateIndex.h"

namespace mems {

class HipAlignmentScore {
public:
    // one record of MAUVE_SCORE_WORDS counters per ordered sequence pair, row-major (i, j):
    // tp, fp_base, fp_gap, fn_unaligned, fn_base, tn, 0, 0
    typedef std::vector<int64_t> RecordList;
    // hc == nullptr: the global context, taken when the first device call needs it (records made elsewhere can be kept without a device: Assign)
    explicit HipAlignmentScore(HipContext *hc = nullptr) : hc_(hc), n_(0), correct_n_(0) {}

    // the correct alignment: stays in the context until the next SetCorrect, whatever else runs there
    void SetCorrect(const IntervalList &correct)
    {
        const HipIntervalArrays a(correct, "HipAlignmentScore::SetCorrect");
        HipContext &hc = context();
        hc.check(mauve_score_truth(hc.get(), (int)a.N, (int64_t)a.K, a.left.data(), a.right.data(), a.rev.data(), a.col_off.data(), a.cols.data()), "mauve_score_truth");
        correct_n_ = a.N;
    }
    // score one calculated alignment (it becomes the context's coordinate index); the totals of the tool
    const mauve_score_totals &Score(const IntervalList &calculated)
    {
        if (!correct_n_) throw genome::gnException("HipAlignmentScore::Score: no correct alignment (SetCorrect first)");
        HipContext &hc = context();
        const HipCoordinateIndex ix(calculated, hc);
        RecordList rec((size_t)correct_n_ * correct_n_ * MAUVE_SCORE_WORDS, 0);
        hc.check(mauve_score_alignment(hc.get(), rec.data()), "mauve_score_alignment");
        Assign(rec, correct_n_);
        return totals_;
    }
    // records made elsewhere (e.g. by mauve_score_alignment on an index of the context's own alignment)
    void Assign(const RecordList &records, uint seq_count)
    {
        if (records.size() != (size_t)seq_count * seq_count * MAUVE_SCORE_WORDS)
            throw genome::gnException("HipAlignmentScore::Assign: " + std::to_string(records.size()) + " counters are not seq_count * seq_count records");
        records_ = records; n_ = seq_count;
        mauve_score_totals_from(records_.data(), (int)n_, &totals_);
    }
    uint SeqCount() const { return n_; }
    const RecordList &Records() const { return records_; }
    // the record of the ordered pair (i, j): what the correct alignment and the calculated one say about the bases of i against j
    const int64_t *Record(uint i, uint j) const
    {
        if (i >= n_ || j >= n_) throw genome::gnException("HipAlignmentScore::Record: sequence index out of range");
        return records_.data() + ((size_t)i * n_ + j) * MAUVE_SCORE_WORDS;
    }
    // bases of sequence i in the correct alignment (every record of a row sums to it); 0 for a single sequence
    int64_t BaseCount(uint i) const
    {
        if (n_ < 2) return 0;
        const int64_t *r = Record(i, i == 0 ? 1 : 0);
        return r[0] + r[1] + r[2] + r[3] + r[4] + r[5];
    }
    const mauve_score_totals &Totals() const { return totals_; }
private:
    HipContext &context() { if (!hc_) hc_ = &HipContext::global(); return *hc_; }
    HipContext *hc_;
    uint n_, correct_n_;
    RecordList records_;
    mauve_score_totals totals_ = {0, 0, 0, 0, 0, 0};
};

// the first five lines of the tool's report (scoreAlignment.cpp:450-454), in its format (a stream's default: six significant digits)
inline void printScoreAlignment(std::ostream &os, const mauve_score_totals &t)
{
    os << "Sensitivity: TP / TP + FN = " << (double)(t.tp) / (double)(t.tp + t.fn) << std::endl;
    os << "Specificity: TN / TN + FP = " << (double)(t.tn) / (double)(t.tn + t.fp) << std::endl;
    os << "TP + TN / total = " << (double)(t.tp + t.tn) / (double)(t.total) << std::endl;
    os << "FP + FN / total = " << (double)(t.fp + t.fn) / (double)(t.total) << std::endl;
    os << "unaligned error = " << (double)t.unaligned_fn / (double)t.total << std::endl;
}

}  // namespace mems
#endif
