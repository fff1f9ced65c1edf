// HipExcursions against the host loop it stands in for (usage: excursion_test alignment.xmfa genomes.mfa [--time]): an IntervalList read
// from an XMFA, with its sequences from a multi-FastA, goes through the device stage.  Pairs must equal getLocalRecordHeights of evd.cpp
// -- written out here over Interval::GetAlignment rows, single-threaded, with computeMatchScores / computeGapScores of the mirror -- record
// by record, with the column each excursion ended in and the state at every stream's end; Core must equal the same loop over the columns
// in which every sequence has a base, scored by computeSPScore; the second halves of the intervals as ranges; the thresholds.
// --time prints what the host loop and the device call took.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include "libMems/Excursions.h"
#include "libMems/Islands.h"

using namespace mems;

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "excursion_test: %s failed at line %d\n", #c, __LINE__); return 1; } } while (0)

// the tool's loop (evd.cpp:38-62) over the scores of the columns [c0, c1), in 64 bits; the records, then the state at the end
static void walk(const std::vector<score_t> &scores, size_t c0, size_t c1, HipExcursions::Result &out)
{
    int64_t sum = 0, record = 0;
    for (size_t c = c0; c < c1; c++) {
        if (scores[c] == INVALID_SCORE) continue;
        const int64_t v = -(int64_t)scores[c];
        if (sum > 0 && sum + v < 0) { sum = 0; out.height.push_back(record); out.end_col.push_back((int64_t)c); record = 0; }
        else if (sum == 0 && v > 0) { sum += v; record = std::max(record, sum); }
        else if (sum > 0) { sum += v; record = std::max(record, sum); }
    }
    out.stream_off.push_back((int64_t)out.height.size());
    out.tail.push_back(sum); out.tail.push_back(record);
}

static bool same(const HipExcursions::Result &a, const HipExcursions::Result &b)
{
    return a.height == b.height && a.end_col == b.end_col && a.stream_off == b.stream_off && a.tail == b.tail;
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: excursion_test alignment.xmfa genomes.mfa [--time]\n"); return 2; }
    const bool timing = argc > 3 && !strcmp(argv[3], "--time");
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
        HipExcursions ex(ix);
        const score_t skew[4][4] = {{5, -1, -2, -3}, {-4, 6, -5, -6}, {-7, -8, 7, -9}, {-10, -11, -12, 8}};
        const PairwiseScoringScheme schemes[2] = {PairwiseScoringScheme(), PairwiseScoringScheme(skew, -17, -3)};
        std::vector<ColumnRange> halves;
        for (size_t i = 0; i < il.size(); i++) { const int64_t n = (int64_t)il[i].AlignmentLength(); halves.push_back(ColumnRange{(int64_t)i, n / 2, n - n / 2}); }
        std::vector<std::vector<std::string>> rows(il.size());
        for (size_t i = 0; i < il.size(); i++) { il[i].GetAlignment(rows[i], il.seq_table); rows[i].resize(N, std::string((size_t)il[i].AlignmentLength(), '-')); }
        size_t n_default = 0;
        for (int s = 0; s < 2; s++) {
            const PairwiseScoringScheme &pss = schemes[s];
            for (int half = 0; half < 2; half++) {
                HipExcursions::Result host, core;
                host.stream_off.push_back(0); core.stream_off.push_back(0);
                const auto t0 = std::chrono::steady_clock::now();
                for (size_t i = 0; i < il.size(); i++) {
                    const size_t n = rows[i][0].size(), c0 = half ? n / 2 : 0;
                    for (uint x = 0; x < N; x++)
                        for (uint y = x + 1; y < N; y++) {
                            std::vector<score_t> scores;
                            if (half) {                       // a range starts with no run open: the scores of its own columns
                                const std::string rx = rows[i][x].substr(c0), ry = rows[i][y].substr(c0);
                                std::vector<score_t> part;
                                computeMatchScores(rx, ry, pss, part);
                                computeGapScores(rx, ry, pss, part);
                                scores.assign(c0, INVALID_SCORE);
                                scores.insert(scores.end(), part.begin(), part.end());
                            } else {
                                computeMatchScores(rows[i][x], rows[i][y], pss, scores);
                                computeGapScores(rows[i][x], rows[i][y], pss, scores);
                            }
                            walk(scores, c0, n, host);
                        }
                }
                const auto t1 = std::chrono::steady_clock::now();
                for (size_t i = 0; i < il.size(); i++) {
                    // multiEVD.cpp:38-46: the columns every sequence has a base in, the column's sum-of-pairs score
                    const size_t n = rows[i][0].size(), c0 = half ? n / 2 : 0;
                    std::vector<score_t> per_col; score_t total = 0;
                    computeSPScore(rows[i], pss, per_col, total);
                    for (size_t c = 0; c < n; c++)
                        for (uint g = 0; g < N; g++) if (rows[i][g][c] == '-') per_col[c] = INVALID_SCORE;
                    walk(per_col, c0, n, core);
                }
                const auto t2 = std::chrono::steady_clock::now();
                const HipExcursions::Result dev = ex.Pairs(pss, nullptr, half ? &halves : nullptr);
                const auto t3 = std::chrono::steady_clock::now();
                REQUIRE(same(dev, host));
                REQUIRE(same(ex.Core(pss, nullptr, half ? &halves : nullptr), core));
                if (!s && !half) n_default = host.height.size();
                if (timing && !s && !half) {
                    const auto ms = [](std::chrono::steady_clock::duration d) { return std::chrono::duration<double, std::milli>(d).count(); };
                    printf("host loop, all pairs: %.3f ms; device call and fetch: %.3f ms\n", ms(t1 - t0), ms(t3 - t2));
                }
                if (!s && !half) {
                    int64_t thr[4], above[4];
                    HipExcursions::Thresholds(dev.height, thr, above);
                    std::vector<int64_t> sorted(dev.height);
                    std::sort(sorted.begin(), sorted.end());
                    REQUIRE(!sorted.empty());
                    const double frac[4] = {.95, .99, .999, .9999};
                    for (int q = 0; q < 4; q++) {
                        const size_t idx = std::min((size_t)(sorted.size() * frac[q]), sorted.size() - 1);
                        REQUIRE(thr[q] == sorted[idx] && above[q] == (int64_t)(sorted.size() - idx));
                    }
                }
            }
        }
        // a chosen pair list with a reversed pair; groups
        const std::vector<std::pair<uint, uint>> chosen{{N - 1, 0}, {0, N - 1}};
        const HipExcursions::Result two = ex.Pairs(schemes[0], &chosen);
        REQUIRE(two.stream_off.size() == il.size() * 2 + 1 && two.height.size() % 2 == 0);
        const std::vector<uint32_t> groups{3u, (1u << N) - 1u};
        REQUIRE(ex.Core(schemes[0], &groups).stream_off.size() == il.size() * 2 + 1);
        // a range outside the list and an empty pair list are errors, not answers
        bool threw = false;
        std::vector<ColumnRange> bad(1, ColumnRange{(int64_t)il.size(), 0, 1});
        try { ex.Pairs(schemes[0], nullptr, &bad); } catch (const genome::gnException &) { threw = true; }
        REQUIRE(threw);
        threw = false;
        const std::vector<std::pair<uint, uint>> nobody;
        try { ex.Pairs(schemes[0], &nobody); } catch (const genome::gnException &) { threw = true; }
        REQUIRE(threw);
        printf("%zu intervals, %u sequences, %zu excursions\nOK\n", il.size(), N, n_default);
    } catch (const genome::gnException &e) {
        fprintf(stderr, "excursion_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
