// The host helpers of the pairwise column statistics against the host functions they restate (usage:
// pairstats_host_test alignment.xmfa genomes.mfa; no device): counters made by a plain loop over the Interval::GetAlignment rows of
// every interval go through mauve_pair_stats_sp_score and must equal computeSPScore of those two rows, under the default scheme and an
// asymmetric one; summed over the intervals they go through mauve_pair_stats_identity and must equal mems::IdentityMatrix.
#include <cstdio>
#include <fstream>
#include "libMems/DistanceMatrix.h"
#include "libMems/MatchList.h"
#include "libMems/PairwiseScoringScheme.h"

using namespace mems;

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "pairstats_host_test: %s failed at line %d\n", #c, __LINE__); return 1; } } while (0)

static int code5(char ch) { switch (ch) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return 4; } }

// the S16 record of rows x and y, column by column
static void count_pair(const std::string &x, const std::string &y, int64_t *s)
{
    int open = 0;                                              // 1: an only_a run, 2: an only_b run
    for (size_t c = 0; c < x.size(); c++) {
        const bool gx = x[c] == '-', gy = y[c] == '-';
        if (gx && gy) { s[29]++; continue; }
        if (!gx && !gy) { s[5 * code5(x[c]) + code5(y[c])]++; open = 0; continue; }
        const int side = gy ? 1 : 2;
        s[gy ? 25 : 26]++;
        if (open != side) s[gy ? 27 : 28]++;
        open = side;
    }
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: pairstats_host_test alignment.xmfa genomes.mfa\n"); return 2; }
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
        const size_t P = (size_t)N * (N - 1) / 2;
        std::vector<int64_t> total(P * MAUVE_PAIR_STATS_WORDS, 0);
        size_t gap_columns = 0;
        for (size_t i = 0; i < il.size(); i++) {
            std::vector<std::string> rows;
            il[i].GetAlignment(rows, il.seq_table);
            rows.resize(N, std::string((size_t)il[i].AlignmentLength(), '-'));
            size_t p = 0;
            for (uint x = 0; x < N; x++)
                for (uint y = x + 1; y < N; y++, p++) {
                    int64_t s[MAUVE_PAIR_STATS_WORDS] = {0};
                    count_pair(rows[x], rows[y], s);
                    int64_t sum = 0;
                    for (int k = 0; k < 27; k++) sum += s[k];
                    REQUIRE(sum + s[29] == (int64_t)rows[x].size());
                    gap_columns += (size_t)(s[25] + s[26]);
                    for (const PairwiseScoringScheme &pss : schemes) {
                        mauve_scoring sc;
                        for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) sc.matrix[a][b] = pss.matrix[a][b];
                        sc.gap_open = pss.gap_open; sc.gap_extend = pss.gap_extend;
                        int64_t got = 0;
                        mauve_pair_stats_sp_score(s, 1, &sc, &got);
                        std::vector<std::string> two{rows[x], rows[y]};
                        std::vector<score_t> per_col; score_t want = 0;
                        computeSPScore(two, pss, per_col, want);
                        REQUIRE(got == (int64_t)want);
                    }
                    for (int k = 0; k < MAUVE_PAIR_STATS_WORDS; k++) total[p * MAUVE_PAIR_STATS_WORDS + k] += s[k];
                }
        }
        REQUIRE(gap_columns > 0);
        std::vector<double> id(P, -1.0);
        mauve_pair_stats_identity(total.data(), (int64_t)P, id.data());
        NumericMatrix<double> want;
        IdentityMatrix(il, want);
        size_t p = 0;
        for (uint x = 0; x < N; x++) for (uint y = x + 1; y < N; y++, p++) { REQUIRE(id[p] == want(x, y) && id[p] == want(y, x)); REQUIRE(id[p] > 0.5 && id[p] < 1.0); }
        printf("%zu intervals, %u sequences, %zu one-sided columns\nOK\n", il.size(), N, gap_columns);
    } catch (const genome::gnException &e) {
        fprintf(stderr, "pairstats_host_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
