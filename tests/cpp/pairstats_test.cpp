// HipPairStatistics against the host functions it stands in for (usage: pairstats_test alignment.xmfa genomes.mfa): an IntervalList read
// from an XMFA, with its sequences from a multi-FastA, goes through the device stage.  IdentityMatrix must equal mems::IdentityMatrix --
// the counts are integers and the division is the same, so the comparison is == -- and SumOfPairsScore must equal computeSPScore's
// total over every interval's rows; the backbone form over halves of the intervals equals the host count on those halves.
#include <cstdio>
#include <fstream>
#include "libMems/DistanceMatrix.h"
#include "libMems/PairStatistics.h"

using namespace mems;

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "pairstats_test: %s failed at line %d\n", #c, __LINE__); return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: pairstats_test alignment.xmfa genomes.mfa\n"); return 2; }
    try {
        IntervalList il;
        std::ifstream in(argv[1]);
        REQUIRE(in.good());
        il.ReadStandardAlignment(in);
        REQUIRE(il.size() > 0);
        LoadMFASequences(il, argv[2], nullptr);
        const uint N = (uint)il.seq_table.size();
        REQUIRE(N >= 2);
        HipContext &hc = HipContext::global();
        { MatchList ml; ml.seq_table = il.seq_table; ml.upload(hc); ml.seq_table.clear(); }      // the sequences first, then the index
        HipCoordinateIndex ix(il, hc);
        HipPairStatistics ps(ix);
        NumericMatrix<double> got, want;
        ps.IdentityMatrix(got);
        IdentityMatrix(il, want);
        for (uint i = 0; i < N; i++) for (uint j = 0; j < N; j++) REQUIRE(got(i, j) == want(i, j));
        REQUIRE(got(0, 1) > 0.5 && got(0, 1) < 1.0);
        // the sum-of-pairs score under the default scheme and an asymmetric one
        const score_t skew[4][4] = {{5, -1, -2, -3}, {-4, 6, -5, -6}, {-7, -8, 7, -9}, {-10, -11, -12, 8}};
        const PairwiseScoringScheme schemes[2] = {PairwiseScoringScheme(), PairwiseScoringScheme(skew, -17, -3)};
        for (const PairwiseScoringScheme &pss : schemes) {
            int64_t host = 0;
            for (size_t i = 0; i < il.size(); i++) {
                std::vector<std::string> rows;
                il[i].GetAlignment(rows, il.seq_table);
                std::vector<score_t> per_col; score_t s = 0;
                computeSPScore(rows, pss, per_col, s);
                host += s;
            }
            REQUIRE(ps.SumOfPairsScore(pss) == host && host != 0);
        }
        // ranges: the second half of every interval -- the identity of those columns alone
        std::vector<ColumnRange> halves;
        std::vector<double> same(N * N, 0), both(N * N, 0);
        for (size_t i = 0; i < il.size(); i++) {
            const int64_t n = (int64_t)il[i].AlignmentLength();
            halves.push_back(ColumnRange{(int64_t)i, n / 2, n - n / 2});
            std::vector<std::string> rows;
            il[i].GetAlignment(rows, il.seq_table);
            for (uint x = 0; x < N && x < rows.size(); x++)
                for (uint y = 0; y < N && y < rows.size(); y++)
                    for (int64_t c = n / 2; c < n; c++) {
                        if (rows[x][(size_t)c] == '-' || rows[y][(size_t)c] == '-') continue;
                        both[x * N + y] += 1; same[x * N + y] += rows[x][(size_t)c] == rows[y][(size_t)c];
                    }
        }
        ps.BackboneIdentityMatrix(halves, got);
        for (uint i = 0; i < N; i++) for (uint j = 0; j < N; j++) REQUIRE(got(i, j) == (i == j ? 1.0 : (both[i * N + j] > 0 ? same[i * N + j] / both[i * N + j] : 0.0)));
        // the records themselves: per range, one per pair; they sum to the totals
        const HipPairStatistics::Records per = ps.Count(nullptr, &halves, true), tot = ps.Count(nullptr, &halves, false);
        const size_t P = (size_t)N * (N - 1) / 2, W = MAUVE_PAIR_STATS_WORDS;
        REQUIRE(per.size() == halves.size() * P * W && tot.size() == P * W);
        for (size_t k = 0; k < P * W; k++) { int64_t s = 0; for (size_t r = 0; r < halves.size(); r++) s += per[r * P * W + k]; REQUIRE(s == tot[k]); }
        // a range outside the list is an error, not an answer
        bool threw = false;
        std::vector<ColumnRange> bad(1, ColumnRange{(int64_t)il.size(), 0, 1});
        try { ps.Count(nullptr, &bad, false); } catch (const genome::gnException &) { threw = true; }
        REQUIRE(threw);
        // so is an empty pair list: it does not mean "all pairs", and the record buffer it would get holds none
        threw = false;
        const std::vector<std::pair<uint, uint>> nobody;
        try { ps.Count(&nobody, nullptr, false); } catch (const genome::gnException &) { threw = true; }
        REQUIRE(threw);
        const std::vector<std::pair<uint, uint>> one(1, std::make_pair(1u, 0u));
        REQUIRE(ps.Count(&one, nullptr, false).size() == W);
        printf("%zu intervals, %u sequences, identity(0,1) = %.6f\nOK\n", il.size(), N, want(0, 1));
    } catch (const genome::gnException &e) {
        fprintf(stderr, "pairstats_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
