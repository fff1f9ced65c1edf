// libMems/RepeatScore.h -- a repeat map scored against a correct alignment of the copies of its repeats, on the device.
// The reference answers "how much of the repeats did the map find?" with a tool of its own, scoreProcrastAlignment <correct alignment>
// <calculated matches> (scoreProcrastAlignment.cpp:120-364, compareAlignmentsAceD): a vector of (match, component) per base of the
// concatenated sequence and two set intersections per pair of the correct alignment.  HipRepeatScore keeps the correct IntervalList -- its
// rows the copies of a repeat -- as the context's second coordinate index (mauve_score_truth) and scores a MatchList of ungapped
// multi-component matches of one sequence, or the repeat map the context still holds (RepeatHash with SetExtension(true)), in one call
// (mauve_repeat_score).  No sequence data is needed.
#ifndef MAUVE_HIP_REPEATSCORE_H
#define MAUVE_HIP_REPEATSCORE_H

#include <ostream>
#include "CoordinateIndex.h"
#include "MatchList.h"

namespace mems {

class HipRepeatScore {
public:
    // hc == nullptr: the global context, taken when the first device call needs it (results made elsewhere can be kept without a device: Assign)
    explicit HipRepeatScore(HipContext *hc = nullptr) : hc_(hc), rows_(0) {}

    // the correct alignment; row_offset: the bases of the concatenated sequence in front of every row's origin (the tool's concat_coords,
    // :131-136), empty = the rows carry the sequence's own coordinates.  It stays in the context until the next SetCorrect
    void SetCorrect(const IntervalList &correct, const std::vector<int64_t> &row_offset = std::vector<int64_t>())
    {
        const HipIntervalArrays a(correct, "HipRepeatScore::SetCorrect");
        if (!row_offset.empty() && row_offset.size() != a.N) throw genome::gnException("HipRepeatScore::SetCorrect: row_offset needs one entry per row");
        HipContext &hc = context();
        hc.check(mauve_score_truth(hc.get(), (int)a.N, (int64_t)a.K, a.left.data(), a.right.data(), a.rev.data(), a.col_off.data(), a.cols.data()), "mauve_score_truth");
        rows_ = a.N; row_offset_ = row_offset;
    }
    // score a list of ungapped matches, every component a copy in the one sequence (Start < 0: reverse strand)
    const mauve_repeat_score_totals &Score(const MatchList &calculated)
    {
        std::vector<int64_t> len, mult, off(1, 0), st;
        for (const Match *m : calculated) {
            len.push_back((int64_t)m->Length()); mult.push_back((int64_t)m->SeqCount());
            for (uint k = 0; k < m->SeqCount(); k++) st.push_back((int64_t)m->Start(k));
            off.push_back((int64_t)st.size());
        }
        if (st.empty()) st.push_back(0);
        if (len.empty()) { len.push_back(0); mult.push_back(0); }
        return run((int64_t)calculated.size(), len.data(), mult.data(), off.data(), st.data(), off);
    }
    // score the repeat map the context holds, where it lies; `list` is the same map as the finder handed it out (for the tables' shape only)
    const mauve_repeat_score_totals &ScoreResident(const MatchList &list)
    {
        std::vector<int64_t> off(1, 0);
        for (const Match *m : list) off.push_back(off.back() + (int64_t)m->SeqCount());
        return run(0, nullptr, nullptr, nullptr, nullptr, off);
    }
    // a result made elsewhere (e.g. by mauve_repeat_score directly): start_off gives the tables their shape
    void Assign(const mauve_repeat_score_totals &totals, uint rows, const std::vector<int64_t> &pair_records, const std::vector<int64_t> &start_off,
                const std::vector<uint32_t> &comp_hit, const std::vector<uint32_t> &pair_hit)
    {
        if (pair_records.size() != (size_t)rows * rows * 4) throw genome::gnException("HipRepeatScore::Assign: " + std::to_string(pair_records.size()) + " counters are not rows * rows records of 4");
        if (start_off.empty() || comp_hit.size() + 1 != start_off.size() || pair_hit.size() != (size_t)start_off.back())
            throw genome::gnException("HipRepeatScore::Assign: the hit tables do not have the shape of start_off");
        totals_ = totals; rows_ = rows; pairs_ = pair_records; off_ = start_off; comp_hit_ = comp_hit; pair_hit_ = pair_hit;
    }
    uint RowCount() const { return rows_; }
    size_t MatchCount() const { return off_.empty() ? 0 : off_.size() - 1; }
    const mauve_repeat_score_totals &Totals() const { return totals_; }
    // possible, truepos, exact, 0 of the rows i < j of the correct alignment
    const int64_t *PairRecord(uint i, uint j) const
    {
        if (i >= rows_ || j >= rows_ || pairs_.empty()) throw genome::gnException("HipRepeatScore::PairRecord: row index out of range");
        return pairs_.data() + ((size_t)i * rows_ + j) * 4;
    }
    uint Multiplicity(size_t r) const { check_match(r); return (uint)(off_[r + 1] - off_[r]); }
    // component c of match r aligned a pair of the correct alignment to another component (component_hits, :318-321)
    bool ComponentHit(size_t r, uint c) const { check_match(r); return c < Multiplicity(r) && (comp_hit_[r] >> c & 1u); }
    // components c1 and c2 of match r aligned a pair of the correct alignment (pairwise_component_hits, :323-335)
    bool PairHit(size_t r, uint c1, uint c2) const
    {
        check_match(r);
        if (c1 > c2) std::swap(c1, c2);
        return c1 != c2 && c2 < Multiplicity(r) && (pair_hit_[(size_t)off_[r] + c1] >> c2 & 1u);
    }
    // SP sensitivity, exact SP sensitivity, match component PPV, pairwise match component PPV (0 / 0 = 0)
    void Figures(double out[4]) const { mauve_repeat_score_ppv(&totals_, out); }
private:
    HipContext &context() { if (!hc_) hc_ = &HipContext::global(); return *hc_; }
    void check_match(size_t r) const { if (r >= MatchCount()) throw genome::gnException("HipRepeatScore: match index out of range"); }
    const mauve_repeat_score_totals &run(int64_t n, const int64_t *len, const int64_t *mult, const int64_t *off, const int64_t *st, const std::vector<int64_t> &shape)
    {
        if (!rows_) throw genome::gnException("HipRepeatScore::Score: no correct alignment (SetCorrect first)");
        HipContext &hc = context();
        std::vector<int64_t> pairs((size_t)rows_ * rows_ * 4, 0);
        std::vector<uint32_t> ch(shape.size() - 1, 0), ph((size_t)shape.back(), 0);
        mauve_repeat_score_totals t;
        hc.check(mauve_repeat_score(hc.get(), n, len, mult, off, st, row_offset_.empty() ? nullptr : row_offset_.data(), &t, pairs.data(), ch.empty() ? nullptr : ch.data(),
                                    ph.empty() ? nullptr : ph.data()), "mauve_repeat_score");
        Assign(t, rows_, pairs, shape, ch, ph);
        return totals_;
    }
    HipContext *hc_;
    uint rows_;
    std::vector<int64_t> row_offset_, pairs_, off_;
    std::vector<uint32_t> comp_hit_, pair_hit_;
    mauve_repeat_score_totals totals_ = {0, 0, 0, 0, 0, 0, 0, 0};
};

// the five lines of the tool's report (scoreProcrastAlignment.cpp:346-363), in its format (a stream's default: six significant digits)
inline void printScoreProcrast(std::ostream &os, const mauve_repeat_score_totals &t)
{
    os << "sp_truepos " << t.sp_truepos << std::endl;
    os << "sp_possible " << t.sp_possible << std::endl;
    os << "SP sensitivity: " << ((double)t.sp_truepos) / ((double)t.sp_possible) << std::endl;
    os << "Match component PPV: " << (double)t.components_hit / (double)t.components << std::endl;
    os << "Pairwise match component PPV: " << (double)t.component_pairs_hit / (double)t.component_pairs << std::endl;
}

}  // namespace mems
#endif
