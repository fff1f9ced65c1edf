// The repeat-map score of the mirror on the device: one family of three copies, the middle one reversed, scored
//  1. from a MatchList with the rows in the sequence's own coordinates,
//  2. in the tool's concatenated form (rows as contigs, row_offset = concat_coords),
//  3. against a match on the wrong strand, and against an empty list.
#include <cassert>
#include <iostream>
#include <sstream>
#include "libMems/mems_hip.h"
using namespace mems;

static Interval family(int64 s0, int64 s1, int64 s2)
{
    const std::vector<int64> left = {s0, s1, s2}, right = {s0 + 9, s1 + 9, s2 + 9};
    return Interval(left, right, std::vector<char>{0, 1, 0}, std::vector<uint32_t>(10, 7u));
}

int main()
{
    try {
        HipRepeatScore sc;
        Match m(3); m.SetLength(10); m.SetStart(0, 101); m.SetStart(1, -201); m.SetStart(2, 301);
        MatchList ml; ml.push_back(&m);
        for (int form = 0; form < 2; form++) {
            IntervalList truth;
            truth.push_back(form ? family(101, 1, 1) : family(101, 201, 301));
            sc.SetCorrect(truth, form ? std::vector<int64_t>{0, 200, 300} : std::vector<int64_t>());
            const mauve_repeat_score_totals &t = sc.Score(ml);
            assert(t.sp_possible == 30 && t.sp_truepos == 30 && t.sp_exact == 30 && t.components == 3 && t.components_hit == 3 && t.component_pairs == 3 && t.component_pairs_hit == 3);
            assert(sc.RowCount() == 3 && sc.MatchCount() == 1 && sc.PairRecord(0, 2)[0] == 10 && sc.PairRecord(1, 2)[2] == 10);
            assert(sc.ComponentHit(0, 1) && sc.PairHit(0, 2, 1));
            std::ostringstream os;
            printScoreProcrast(os, t);
            assert(os.str() == "sp_truepos 30\nsp_possible 30\nSP sensitivity: 1\nMatch component PPV: 1\nPairwise match component PPV: 1\n");
        }
        Match w(2); w.SetLength(10); w.SetStart(0, 101); w.SetStart(1, 201);            // row 1 is reversed in the truth: the strand is wrong
        MatchList wl; wl.push_back(&w);
        const mauve_repeat_score_totals &t = sc.Score(wl);
        assert(t.sp_possible == 30 && t.sp_truepos == 0 && t.components == 2 && t.components_hit == 0 && !sc.PairHit(0, 0, 1));
        MatchList none;
        const mauve_repeat_score_totals &e = sc.Score(none);
        assert(e.sp_possible == 30 && e.sp_truepos == 0 && e.components == 0 && sc.MatchCount() == 0);
        ml.clear(); wl.clear();
        std::cout << "OK" << std::endl;
        return 0;
    } catch (const std::exception &e) {
        std::cerr << "repeat_score_test: " << e.what() << std::endl;
        return 1;
    }
}
