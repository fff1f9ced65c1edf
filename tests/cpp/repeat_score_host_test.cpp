// The host side of the repeat-map score, no device: HipRepeatScore's bookkeeping on a hand-written result,
// mauve_repeat_score_ppv on the same totals, printScoreProcrast against a literal.  Built together with
// mauvealigner_amd/csrc/repeat_score_host.cpp under -fsanitize=address,undefined and run directly.
#include <cstdio>
#include <sstream>
#include "libMems/mems_hip.h"

using namespace mems;

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "repeat_score_host_test: %s failed at line %d\n", #c, __LINE__); return 1; } } while (0)

int main()
{
    // three rows, two matches of 3 and 2 components: match 0 aligned rows through its components (0, 1) and (0, 2), match 1 nothing
    const mauve_repeat_score_totals t = {40, 30, 20, 5, 3, 4, 2, 0};
    std::vector<int64_t> pairs(3 * 3 * 4, 0);
    const int64_t p01[4] = {20, 20, 15, 0}, p02[4] = {10, 10, 5, 0}, p12[4] = {10, 0, 0, 0};
    std::copy(p01, p01 + 4, pairs.begin() + (0 * 3 + 1) * 4);
    std::copy(p02, p02 + 4, pairs.begin() + (0 * 3 + 2) * 4);
    std::copy(p12, p12 + 4, pairs.begin() + (1 * 3 + 2) * 4);
    const std::vector<int64_t> off = {0, 3, 5};
    const std::vector<uint32_t> ch = {7u, 0u}, ph = {6u, 0u, 0u, 0u, 0u};

    double f[4];
    mauve_repeat_score_ppv(&t, f);
    REQUIRE(f[0] == 30.0 / 40.0 && f[1] == 20.0 / 40.0 && f[2] == 3.0 / 5.0 && f[3] == 2.0 / 4.0);
    const mauve_repeat_score_totals z = {0, 0, 0, 0, 0, 0, 0, 0};
    mauve_repeat_score_ppv(&z, f);
    REQUIRE(f[0] == 0.0 && f[1] == 0.0 && f[2] == 0.0 && f[3] == 0.0);             // 0 / 0 is 0
    const mauve_repeat_score_totals h = {0, 0, 0, 7, 0, 9, 0, 0};                  // a map scored against a truth without columns
    mauve_repeat_score_ppv(&h, f);
    REQUIRE(f[0] == 0.0 && f[2] == 0.0 && f[3] == 0.0);

    HipRepeatScore sc;                                                             // (the bookkeeping below never asks for a context)
    REQUIRE(sc.RowCount() == 0 && sc.MatchCount() == 0 && sc.Totals().sp_possible == 0);
    sc.Assign(t, 3, pairs, off, ch, ph);
    REQUIRE(sc.RowCount() == 3 && sc.MatchCount() == 2 && sc.Multiplicity(0) == 3 && sc.Multiplicity(1) == 2);
    REQUIRE(sc.PairRecord(0, 1)[0] == 20 && sc.PairRecord(0, 2)[2] == 5 && sc.PairRecord(1, 2)[1] == 0 && sc.PairRecord(1, 0)[0] == 0);
    REQUIRE(sc.ComponentHit(0, 0) && sc.ComponentHit(0, 1) && sc.ComponentHit(0, 2) && !sc.ComponentHit(0, 3) && !sc.ComponentHit(1, 0) && !sc.ComponentHit(1, 1));
    REQUIRE(sc.PairHit(0, 0, 1) && sc.PairHit(0, 1, 0) && sc.PairHit(0, 2, 0) && !sc.PairHit(0, 1, 2) && !sc.PairHit(0, 1, 1) && !sc.PairHit(1, 0, 1) && !sc.PairHit(0, 0, 3));
    sc.Figures(f);
    REQUIRE(f[0] == 0.75 && f[1] == 0.5 && f[2] == 0.6 && f[3] == 0.5);
    const mauve_repeat_score_totals &u = sc.Totals();
    REQUIRE(u.sp_truepos == 30 && u.components_hit == 3 && u.component_pairs_hit == 2 && u.reserved == 0);
    bool threw = false;
    try { sc.Assign(t, 3, std::vector<int64_t>(3 * 3 * 4 - 1, 0), off, ch, ph); } catch (const genome::gnException &) { threw = true; }
    REQUIRE(threw && sc.MatchCount() == 2);
    threw = false;
    try { sc.Assign(t, 3, pairs, off, ch, std::vector<uint32_t>(4, 0)); } catch (const genome::gnException &) { threw = true; }
    REQUIRE(threw);
    threw = false;
    try { sc.PairRecord(3, 0); } catch (const genome::gnException &) { threw = true; }
    REQUIRE(threw);
    threw = false;
    try { sc.ComponentHit(2, 0); } catch (const genome::gnException &) { threw = true; }
    REQUIRE(threw);

    const mauve_repeat_score_totals lit = {4, 3, 2, 8, 6, 6, 2, 0};
    std::ostringstream os;
    printScoreProcrast(os, lit);
    REQUIRE(os.str() == "sp_truepos 3\nsp_possible 4\nSP sensitivity: 0.75\nMatch component PPV: 0.75\nPairwise match component PPV: 0.333333\n");
    printf("OK\n");
    return 0;
}
