// The repeat finder of the mirror on the device (usage: repeat_map_test a.fa):
//  1. a default RepeatHash gives the rows of mauve_seed_match_enumerate: seed-length matches, as before;
//  2. with SetExtension(true) its rows are those of mauve_repeat_matches / mauve_repeat_fetch: fewer, longer
//     matches, in the order of the fetch; an upper multiplicity above MAUVE_REPEAT_MAX_MULT is clamped to it.
#include <cassert>
#include <iostream>
#include <set>
#include <sstream>
#include "libMems/mems_hip.h"
using namespace mems;

static std::string row(const Match *m) { std::ostringstream os; os << *m; return os.str(); }

int main(int argc, char **argv)
{
    try {
        assert(argc == 2);
        MatchList one;
        genome::gnSequence *s = new genome::gnSequence(); s->LoadSource(argv[1]); one.seq_table.push_back(s); one.seq_filename.push_back(argv[1]);
        one.CreateMemorySMLs(11, nullptr, 0);
        const uint64_t pat = (uint64_t)one.sml_table[0]->Seed();
        const int span = (int)one.sml_table[0]->SeedLength();
        HipContext &hc = HipContext::global();
        // 1. the default: one seed-length match per repeated mer
        MatchList def = one; { RepeatHash rh; rh.FindMatches(def); }
        int64_t n = 0, ns = 0;
        hc.check(mauve_seed_match_enumerate(hc.get(), 0, pat, 2, 1000, 0, &n, &ns, nullptr, nullptr, nullptr), "enumerate");
        std::vector<int64_t> mult((size_t)n), off((size_t)n + 1), st((size_t)ns);
        hc.check(mauve_seed_match_enumerate(hc.get(), 0, pat, 2, 1000, 0, &n, &ns, mult.data(), off.data(), st.data()), "enumerate");
        assert(n > 50 && def.size() == (size_t)n);
        std::multiset<std::string> a, b;
        for (size_t i = 0; i < def.size(); i++) {
            a.insert(row(def[i]));
            Match m((uint)mult[i]); m.SetLength((gnSeqI)span);
            for (int64_t k = 0; k < mult[i]; k++) m.SetStart((uint)k, st[(size_t)(off[i] + k)]);
            b.insert(row(&m));
        }
        assert(a == b);
        // 2. extended
        MatchList ext = one; { RepeatHash rh; rh.SetExtension(true); rh.FindMatches(ext); }
        hc.check(mauve_repeat_matches(hc.get(), 0, pat, 2, MAUVE_REPEAT_MAX_MULT, &n, &ns), "repeat_matches");
        std::vector<int64_t> len((size_t)n); mult.assign((size_t)n, 0); off.assign((size_t)n + 1, 0); st.assign((size_t)ns, 0);
        hc.check(mauve_repeat_fetch(hc.get(), len.data(), mult.data(), off.data(), st.data()), "repeat_fetch");
        assert(n > 0 && ext.size() == (size_t)n && ext.size() < def.size());
        bool longer = false;
        for (size_t i = 0; i < ext.size(); i++) {
            Match m((uint)mult[i]); m.SetLength((gnSeqI)len[i]);
            for (int64_t k = 0; k < mult[i]; k++) m.SetStart((uint)k, st[(size_t)(off[i] + k)]);
            assert(row(ext[i]) == row(&m));
            assert(len[i] >= span && ext[i]->Length() == (gnSeqI)len[i]);
            longer = longer || len[i] > 3 * span;
        }
        assert(longer);
        // a wider multiplicity range than the device takes is clamped, not refused
        MatchList cl = one; { RepeatHash rh; rh.SetExtension(true); rh.SetMultiplicityRange(2, 5000); rh.FindMatches(cl); }
        assert(cl.size() == ext.size());
        std::cout << "OK" << std::endl;
        return 0;
    } catch (const std::exception &e) {
        std::cerr << "repeat_map_test: " << e.what() << std::endl;
        return 1;
    }
}
