// libMems/Excursions.h -- the excursions of the column scores of a finished alignment, walked on the device.
// evd and multiEVD (evd.cpp:12-66, multiEVD.cpp:29-79, getLocalRecordHeights) run a state machine along the columns of every interval:
// a running sum of the negated column scores, clamped at zero; every excursion above zero records its highest value when it ends, and the
// sorted heights give the thresholds libMems' backbone detection is calibrated with.  The host pieces of that loop -- INVALID_SCORE,
// computeMatchScores, computeGapScores -- are in Islands.h.  HipExcursions answers for a whole IntervalList in one call
// (mauve_excursions_pairs / mauve_excursions_core) on a HipCoordinateIndex of that list and the sequences resident on the index's
// context: upload them BEFORE the index is built, as for HipAlignmentExtractor.  multiEVD's coalescing of the projected intervals into
// new LCBs (projectIntervalList) is not part of it: every range is a stream of its own.
#ifndef MAUVE_HIP_EXCURSIONS_H
#define MAUVE_HIP_EXCURSIONS_H

#include "AlignmentExtractor.h"
#include "PairwiseScoringScheme.h"

namespace mems {

class HipExcursions {
public:
    // the records of every stream one after another (stream = range * sets + set): stream s owns [stream_off[s], stream_off[s + 1])
    struct Result {
        std::vector<int64_t> height, end_col;            // end_col: the column inside the range's interval
        std::vector<int64_t> stream_off;                 // [streams + 1]
        std::vector<int64_t> tail;                       // [streams][2]: the running sum and the height at the stream's end
    };
    explicit HipExcursions(const HipCoordinateIndex &ix) : ix_(&ix) {}

    // getLocalRecordHeights of evd.cpp for the pairs (nullptr: every pair a < b, row-major in the upper triangle) over the ranges
    // (nullptr: every interval whole)
    Result Pairs(const PairwiseScoringScheme &pss, const std::vector<std::pair<uint, uint>> *pairs = nullptr, const std::vector<ColumnRange> *ranges = nullptr) const
    {
        HipContext &hc = ix_->context();
        const size_t N = ix_->SeqCount();
        const size_t P = pairs ? pairs->size() : N * (N - 1) / 2;
        std::vector<int32_t> a(P + 1), b(P + 1);             // never empty: a null pair list means "all pairs" to the library, an empty one is refused
        if (pairs) for (size_t k = 0; k < P; k++) { a[k] = (int32_t)(*pairs)[k].first; b[k] = (int32_t)(*pairs)[k].second; }
        Ranges R(hc, ranges);
        const mauve_scoring sc = scoring(pss);
        int64_t n = 0;
        hc.check(mauve_excursions_pairs(hc.get(), &sc, (int64_t)P, pairs ? a.data() : nullptr, pairs ? b.data() : nullptr, R.n, ranges ? R.iv.data() : nullptr,
                                        R.col.data(), R.len.data(), &n), "mauve_excursions_pairs");
        return fetch(n, R.count * (int64_t)P);
    }
    // ... of multiEVD.cpp: the columns in which every sequence of a group has a base (nullptr: one group of all sequences), scored by
    // the sum over the group's pairs
    Result Core(const PairwiseScoringScheme &pss, const std::vector<uint32_t> *groups = nullptr, const std::vector<ColumnRange> *ranges = nullptr) const
    {
        HipContext &hc = ix_->context();
        const size_t G = groups ? groups->size() : 1;
        std::vector<uint32_t> m(G + 1, 0);
        if (groups) for (size_t k = 0; k < G; k++) m[k] = (*groups)[k];
        Ranges R(hc, ranges);
        const mauve_scoring sc = scoring(pss);
        int64_t n = 0;
        hc.check(mauve_excursions_core(hc.get(), &sc, (int64_t)G, groups ? m.data() : nullptr, R.n, ranges ? R.iv.data() : nullptr, R.col.data(), R.len.data(), &n),
                 "mauve_excursions_core");
        return fetch(n, R.count * (int64_t)G);
    }
    // the four thresholds evd prints (95%, 99%, 99.9%, 99.99% of the sorted heights) and the numbers of heights at or above them
    static void Thresholds(const std::vector<int64_t> &height, int64_t threshold[4], int64_t above[4])
    {
        mauve_excursion_thresholds(height.data(), (int64_t)height.size(), threshold, above);
    }
private:
    struct Ranges {
        int64_t n = 0, count = 0;
        std::vector<int64_t> iv, col, len;
        Ranges(HipContext &hc, const std::vector<ColumnRange> *ranges) : iv(1), col(1), len(1)
        {
            if (!ranges) { hc.check(mauve_coord_index_size(hc.get(), nullptr, &count, nullptr), "mauve_coord_index_size"); return; }
            n = count = (int64_t)ranges->size();
            iv.resize(ranges->size() + 1); col.resize(ranges->size() + 1); len.resize(ranges->size() + 1);
            for (size_t r = 0; r < ranges->size(); r++) { iv[r] = (*ranges)[r].block; col[r] = (*ranges)[r].col; len[r] = (*ranges)[r].len; }
        }
    };
    static mauve_scoring scoring(const PairwiseScoringScheme &pss)
    {
        mauve_scoring sc;
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) sc.matrix[i][j] = pss.matrix[i][j];
        sc.gap_open = pss.gap_open; sc.gap_extend = pss.gap_extend;
        return sc;
    }
    Result fetch(int64_t n_exc, int64_t n_stream) const
    {
        HipContext &hc = ix_->context();
        Result r;
        r.height.assign((size_t)n_exc + 1, 0); r.end_col.assign((size_t)n_exc + 1, 0);
        r.stream_off.assign((size_t)n_stream + 1, 0); r.tail.assign((size_t)n_stream * 2 + 1, 0);
        hc.check(mauve_excursions_fetch(hc.get(), r.height.data(), r.end_col.data(), r.stream_off.data(), r.tail.data()), "mauve_excursions_fetch");
        r.height.pop_back(); r.end_col.pop_back(); r.tail.pop_back();
        return r;
    }
    const HipCoordinateIndex *ix_;
};

}  // namespace mems
#endif
