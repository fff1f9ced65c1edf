// The host pieces of evd's loop in the mirror (usage: excursion_host_test alignment.xmfa genomes.mfa; no device):
// computeMatchScores plus computeGapScores of libMems/Islands.h on two Interval::GetAlignment rows must equal computeSPScore of those two
// rows column by column, with INVALID_SCORE exactly where both rows have a gap, under the default scheme and an asymmetric one.  The
// tool's loop over those scores, written out here, is then counted and printed for the caller to compare with its pinned totals, and
// its heights go through mauve_excursion_thresholds against the index arithmetic of evd.cpp:108-126.
#include <algorithm>
#include <cstdio>
#include <fstream>
#include "libMems/Islands.h"
#include "libMems/MatchList.h"

using namespace mems;

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "excursion_host_test: %s failed at line %d\n", #c, __LINE__); return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: excursion_host_test alignment.xmfa genomes.mfa\n"); return 2; }
    try {
        IntervalList il;
        std::ifstream in(argv[1]);
        REQUIRE(in.good());
        il.ReadStandardAlignment(in);
        REQUIRE(il.size() > 0);
        LoadMFASequences(il, argv[2], nullptr);
        const uint N = (uint)il.seq_table.size();
        REQUIRE(N >= 2);
        const score_t skew[4][4] = {{5, -1, -2, -3}, {-4, 6, -5, -6}, {-7, -8, 7, -9}, {-10, -11, -12, 8}};
        const PairwiseScoringScheme schemes[2] = {PairwiseScoringScheme(), PairwiseScoringScheme(skew, -17, -3)};
        std::vector<int64_t> heights;
        size_t invalid = 0, gap_columns = 0;
        for (size_t i = 0; i < il.size(); i++) {
            std::vector<std::string> rows;
            il[i].GetAlignment(rows, il.seq_table);
            rows.resize(N, std::string((size_t)il[i].AlignmentLength(), '-'));
            for (uint x = 0; x < N; x++)
                for (uint y = x + 1; y < N; y++)
                    for (int s = 0; s < 2; s++) {
                        const PairwiseScoringScheme &pss = schemes[s];
                        std::vector<score_t> scores;
                        computeMatchScores(rows[x], rows[y], pss, scores);
                        computeGapScores(rows[x], rows[y], pss, scores);
                        REQUIRE(scores.size() == rows[x].size());
                        std::vector<std::string> two{rows[x], rows[y]};
                        std::vector<score_t> per_col; score_t total = 0;
                        computeSPScore(two, pss, per_col, total);
                        REQUIRE(per_col.size() == scores.size());
                        for (size_t c = 0; c < scores.size(); c++) {
                            const bool both_gap = rows[x][c] == '-' && rows[y][c] == '-';
                            REQUIRE((scores[c] == INVALID_SCORE) == both_gap);
                            if (both_gap) { REQUIRE(per_col[c] == 0); invalid += s == 0; continue; }
                            REQUIRE(scores[c] == per_col[c]);
                            if (s == 0 && (rows[x][c] == '-' || rows[y][c] == '-')) gap_columns++;
                        }
                        if (s) continue;
                        // evd.cpp:33-62 on the default scheme, in 64 bits
                        int64_t sum = 0, record = 0;
                        for (size_t c = 0; c < scores.size(); c++) {
                            if (scores[c] == INVALID_SCORE) continue;
                            const int64_t v = -(int64_t)scores[c];
                            if (sum > 0 && sum + v < 0) { sum = 0; heights.push_back(record); record = 0; }
                            else if (sum == 0 && v > 0) { sum += v; record = std::max(record, sum); }
                            else if (sum > 0) { sum += v; record = std::max(record, sum); }
                        }
                    }
        }
        REQUIRE(gap_columns > 0);
        int64_t thr[4], above[4];
        mauve_excursion_thresholds(heights.data(), (int64_t)heights.size(), thr, above);
        std::vector<int64_t> sorted(heights);
        std::sort(sorted.begin(), sorted.end());
        const double frac[4] = {.95, .99, .999, .9999};
        for (int q = 0; q < 4 && !sorted.empty(); q++) {
            size_t idx = sorted.size() * frac[q];
            idx = std::min(idx, sorted.size() - 1);
            REQUIRE(thr[q] == sorted[idx] && above[q] == (int64_t)(sorted.size() - idx));
        }
        printf("%zu intervals, %u sequences, %zu columns without the pair\nexcursions %zu\nOK\n", il.size(), N, invalid, heights.size());
    } catch (const genome::gnException &e) {
        fprintf(stderr, "excursion_host_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
