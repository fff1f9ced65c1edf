// The host side of the alignment score, no device: HipAlignmentScore's record bookkeeping on hand-written records,
// mauve_score_totals_from on the same records, printScoreAlignment against a literal.  Built together with
// mauvealigner_amd/csrc/score_host.cpp under -fsanitize=address,undefined and run directly.
#include <cstdio>
#include <sstream>
#include "libMems/mems_hip.h"

using namespace mems;

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "score_host_test: %s failed at line %d\n", #c, __LINE__); return 1; } } while (0)

int main()
{
    // three sequences; record (i, j) = tp, fp_base, fp_gap, fn_unaligned, fn_base, tn, 0, 0; every row sums to the sequence's bases
    const int64_t hand[3][3][MAUVE_SCORE_WORDS] = {
        {{0, 0, 0, 0, 0, 0, 0, 0}, {90, 3, 2, 1, 1, 3, 0, 0}, {80, 5, 4, 6, 2, 3, 0, 0}},
        {{90, 3, 1, 2, 4, 10, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}, {70, 7, 8, 9, 6, 10, 0, 0}},
        {{80, 5, 0, 10, 12, 13, 0, 0}, {70, 7, 11, 6, 5, 21, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}}};
    HipAlignmentScore::RecordList rec(&hand[0][0][0], &hand[0][0][0] + 3 * 3 * MAUVE_SCORE_WORDS);
    mauve_score_totals t;
    mauve_score_totals_from(rec.data(), 3, &t);
    REQUIRE(t.tp == 90 + 80 + 70);                                        // i < j only
    REQUIRE(t.fp == (3 + 2) + (5 + 4) + (7 + 8));
    REQUIRE(t.unaligned_fn == 1 + 6 + 9);
    REQUIRE(t.fn == t.unaligned_fn + (1 + 2 + 4 + 6 + 12 + 5));           // fn_base from both sides
    REQUIRE(t.tn == 3 + 3 + 10 + 10 + 13 + 21);
    REQUIRE(t.total == t.tp + t.tn + t.fp + t.fn);
    mauve_score_totals z;
    mauve_score_totals_from(rec.data(), 0, &z);
    REQUIRE(z.total == 0 && z.tp == 0);
    mauve_score_totals_from(rec.data() + MAUVE_SCORE_WORDS, 1, &z);        // one sequence: its diagonal record is not read as a pair
    REQUIRE(z.total == 0);

    HipAlignmentScore sc;                                                 // (the bookkeeping below never asks for a context)
    REQUIRE(sc.SeqCount() == 0 && sc.Records().empty() && sc.Totals().total == 0 && sc.BaseCount(0) == 0);
    sc.Assign(rec, 3);
    REQUIRE(sc.SeqCount() == 3 && sc.Records() == rec);
    REQUIRE(sc.Record(1, 2)[0] == 70 && sc.Record(2, 0)[5] == 13 && sc.Record(0, 1) == sc.Records().data() + MAUVE_SCORE_WORDS);
    REQUIRE(sc.BaseCount(0) == 100 && sc.BaseCount(1) == 110 && sc.BaseCount(2) == 120);
    const mauve_score_totals &u = sc.Totals();
    REQUIRE(u.tp == t.tp && u.tn == t.tn && u.fp == t.fp && u.fn == t.fn && u.total == t.total && u.unaligned_fn == t.unaligned_fn);
    bool threw = false;
    try { sc.Assign(HipAlignmentScore::RecordList(3 * 3 * MAUVE_SCORE_WORDS - 1, 0), 3); } catch (const genome::gnException &) { threw = true; }
    REQUIRE(threw && sc.SeqCount() == 3);
    threw = false;
    try { sc.Record(3, 0); } catch (const genome::gnException &) { threw = true; }
    REQUIRE(threw);

    const mauve_score_totals lit = {3, 1, 1, 1, 6, 1};
    std::ostringstream os;
    printScoreAlignment(os, lit);
    REQUIRE(os.str() == "Sensitivity: TP / TP + FN = 0.75\nSpecificity: TN / TN + FP = 0.5\nTP + TN / total = 0.666667\nFP + FN / total = 0.333333\nunaligned error = 0.166667\n");
    std::ostringstream os2;
    printScoreAlignment(os2, t);
    char want[256];
    snprintf(want, sizeof want, "Sensitivity: TP / TP + FN = %g\nSpecificity: TN / TN + FP = %g\nTP + TN / total = %g\nFP + FN / total = %g\nunaligned error = %g\n",
             (double)t.tp / (double)(t.tp + t.fn), (double)t.tn / (double)(t.tn + t.fp), (double)(t.tp + t.tn) / (double)t.total, (double)(t.fp + t.fn) / (double)t.total,
             (double)t.unaligned_fn / (double)t.total);
    REQUIRE(os2.str() == want);
    printf("OK\n");
    return 0;
}
