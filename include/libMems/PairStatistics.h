// libMems/PairStatistics.h -- what two sequences of an alignment show against each other, counted on the device.
// libMems asks how similar the sequences of a finished alignment are with host walks over GetAlignment strings: IdentityMatrix behind
// --lcb-stats (mauveAligner.cpp:784-800, calculateBackboneCoverage.cpp:106-127), BackboneIdentityMatrix (pairCompare.cpp:57-60,77,
// calculateBackboneCoverage2.cpp:98-121), the pairwise loop of gappiness.cpp:33-50 and computeSPScore (multiEVD.cpp:41-46,
// repeatoire.cpp:2527).  mems::IdentityMatrix (DistanceMatrix.h) and mems::computeSPScore (PairwiseScoringScheme.h) stay as they are.
// HipPairStatistics answers for a whole IntervalList in one call (mauve_pair_stats) on a HipCoordinateIndex of that list and the
// sequences resident on the index's context: upload them BEFORE the index is built, as for HipAlignmentExtractor.
#ifndef MAUVE_HIP_PAIRSTATISTICS_H
#define MAUVE_HIP_PAIRSTATISTICS_H

#include "AlignmentExtractor.h"
#include "NumericMatrix.h"
#include "PairwiseScoringScheme.h"

namespace mems {

class HipPairStatistics {
public:
    // one record of MAUVE_PAIR_STATS_WORDS counters per ordered pair, with per_range one per range and pair (range-major)
    typedef std::vector<int64_t> Records;
    explicit HipPairStatistics(const HipCoordinateIndex &ix) : ix_(&ix) {}

    // pairs == nullptr: every pair a < b, row-major in the upper triangle; ranges == nullptr: every interval whole
    Records Count(const std::vector<std::pair<uint, uint>> *pairs = nullptr, const std::vector<ColumnRange> *ranges = nullptr, bool per_range = false) const
    {
        HipContext &hc = ix_->context();
        const size_t N = ix_->SeqCount();
        const size_t P = pairs ? pairs->size() : N * (N - 1) / 2;
        std::vector<int32_t> a(P + 1), b(P + 1);             // never empty: a null pair list means "all pairs" to the library, an empty one is refused
        if (pairs) for (size_t k = 0; k < P; k++) { a[k] = (int32_t)(*pairs)[k].first; b[k] = (int32_t)(*pairs)[k].second; }
        int64_t n_range = 0;
        std::vector<int64_t> iv(1), col(1), len(1);
        if (ranges) {
            n_range = (int64_t)ranges->size();
            iv.resize(ranges->size() + 1); col.resize(ranges->size() + 1); len.resize(ranges->size() + 1);
            for (size_t r = 0; r < ranges->size(); r++) { iv[r] = (*ranges)[r].block; col[r] = (*ranges)[r].col; len[r] = (*ranges)[r].len; }
        } else if (per_range) hc.check(mauve_coord_index_size(hc.get(), nullptr, &n_range, nullptr), "mauve_coord_index_size");
        Records st((per_range ? (size_t)n_range : 1) * P * MAUVE_PAIR_STATS_WORDS + 1, 0);
        hc.check(mauve_pair_stats(hc.get(), (int64_t)P, pairs ? a.data() : nullptr, pairs ? b.data() : nullptr, n_range, ranges ? iv.data() : nullptr,
                                  col.data(), len.data(), per_range ? 1 : 0, st.data()), "mauve_pair_stats");
        st.pop_back();
        return st;
    }
    // mems::IdentityMatrix(iv_list, identity) of the indexed list: identical columns / columns where both have a base, diagonal 1.0
    void IdentityMatrix(NumericMatrix<double> &identity) const { identity_of(nullptr, identity); }
    // ... over backbone segments (or any ranges) only
    void BackboneIdentityMatrix(const std::vector<ColumnRange> &segments, NumericMatrix<double> &identity) const { identity_of(&segments, identity); }
    // computeSPScore's total, summed over the ranges (nullptr: over every interval's rows); a gap run does not cross a range boundary
    int64_t SumOfPairsScore(const PairwiseScoringScheme &pss, const std::vector<ColumnRange> *ranges = nullptr) const
    {
        const Records st = Count(nullptr, ranges, false);
        mauve_scoring sc;
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) sc.matrix[i][j] = pss.matrix[i][j];
        sc.gap_open = pss.gap_open; sc.gap_extend = pss.gap_extend;
        const size_t P = st.size() / MAUVE_PAIR_STATS_WORDS;
        std::vector<int64_t> score(P + 1, 0);
        mauve_pair_stats_sp_score(st.data(), (int64_t)P, &sc, score.data());
        int64_t total = 0;
        for (size_t p = 0; p < P; p++) total += score[p];
        return total;
    }
private:
    void identity_of(const std::vector<ColumnRange> *ranges, NumericMatrix<double> &identity) const
    {
        const uint N = ix_->SeqCount();
        const Records st = Count(nullptr, ranges, false);
        std::vector<double> id(st.size() / MAUVE_PAIR_STATS_WORDS + 1, 0.0);
        mauve_pair_stats_identity(st.data(), (int64_t)(st.size() / MAUVE_PAIR_STATS_WORDS), id.data());
        identity.init(N, N);
        size_t p = 0;
        for (uint i = 0; i < N; i++) {
            identity(i, i) = 1.0;
            for (uint j = i + 1; j < N; j++, p++) identity(i, j) = identity(j, i) = id[p];
        }
    }
    const HipCoordinateIndex *ix_;
};

}  // namespace mems
#endif
