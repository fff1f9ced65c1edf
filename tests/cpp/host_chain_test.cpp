// Host-only check of the pure host-chain steps (csrc/host_chain.hpp): hand cases with the expected numbers written
// out.  Built and run by tests/test_compat_headers.py with plain g++.
#include "host_chain.hpp"
#include <cstdio>

static int bad = 0;
#define CHECK(x) do { if (!(x)) { printf("line %d: %s\n", __LINE__, #x); bad++; } } while (0)

static MatchVec chain_of(int N, std::initializer_list<std::vector<int64_t>> recs)
{
    MatchVec ch(N);
    for (const auto &r : recs) ch.push(r.data());
    return ch;
}

static void test_gap_of()
{
    int64_t lo, ln, lo2, ln2; bool rv;
    {   // forward pair: a at 100..109 / 200..209, b at 120.. / 230..
        const int64_t a[] = {10, 100, 200}, b[] = {5, 120, 230};
        gap_of(a, b, 0, lo, ln, rv); CHECK(lo == 110 && ln == 10 && !rv);
        gap_of(a, b, 1, lo, ln, rv); CHECK(lo == 210 && ln == 20 && !rv);
        gap_of(a, b, 1, lo2, ln2); CHECK(lo2 == 210 && ln2 == 20);
    }
    {   // reverse pair in genome 1: a at 500..509, b (right of a in genome 0) at 470..474 -- the stretch is 475..499, lo comes from b
        const int64_t a[] = {10, 100, -500}, b[] = {5, 120, -470};
        gap_of(a, b, 1, lo, ln, rv); CHECK(lo == 475 && ln == 25 && rv);
        gap_of(a, b, 1, lo2, ln2); CHECK(lo2 == 475 && ln2 == 25);
        gap_of(a, b, 0, lo, ln, rv); CHECK(lo == 110 && ln == 10 && !rv);
    }
    {   // touching in genome 0 (b starts right behind a), 5 bases apart in genome 1
        const int64_t a[] = {10, 100, 200}, b[] = {5, 110, 215};
        gap_of(a, b, 0, lo, ln, rv); CHECK(lo == 110 && ln == 0 && !rv);
        gap_of(a, b, 1, lo, ln, rv); CHECK(lo == 210 && ln == 5);
    }
    {   // overlapping by 5 in genome 0, by 3 in the reverse genome 1: clamped to 0
        const int64_t a[] = {10, 100, -500}, b[] = {5, 105, -498};
        gap_of(a, b, 0, lo, ln, rv); CHECK(lo == 110 && ln == 0 && !rv);
        gap_of(a, b, 1, lo, ln, rv); CHECK(lo == 503 && ln == 0 && rv);
        gap_of(a, b, 1, lo2, ln2); CHECK(lo2 == 503 && ln2 == 0);
    }
}

static void test_chain_extent()
{
    int64_t le, re; bool rv;
    const MatchVec fwd = chain_of(2, {{10, 100, 200}, {5, 120, 230}, {7, 140, 260}});
    chain_extent(fwd, 0, le, re, rv); CHECK(le == 100 && re == 146 && !rv);
    chain_extent(fwd, 1, le, re, rv); CHECK(le == 200 && re == 266 && !rv);
    // genome 1 reverse: the first anchor is the rightmost there (500..509), the last the leftmost (440..446)
    const MatchVec rev = chain_of(2, {{10, 100, -500}, {5, 120, -470}, {7, 140, -440}});
    chain_extent(rev, 0, le, re, rv); CHECK(le == 100 && re == 146 && !rv);
    chain_extent(rev, 1, le, re, rv); CHECK(le == 440 && re == 509 && rv);
    const MatchVec one = chain_of(2, {{10, 100, -500}});
    chain_extent(one, 0, le, re, rv); CHECK(le == 100 && re == 109 && !rv);
    chain_extent(one, 1, le, re, rv); CHECK(le == 500 && re == 509 && rv);
}

static void test_canon_less()
{
    const auto less = canon_less(2);
    // in canonical order: |start 0| first (9 before 10 whatever the sign), then the signed starts, then the length
    const int64_t r[][3] = {{5, -9, 100}, {5, -10, 3}, {5, 10, -4}, {4, 10, 3}, {5, 10, 3}, {5, 10, 4}, {1, 11, 1}};
    const int n = 7;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) CHECK(less(r[i], r[j]) == (i < j));
    const int64_t same[3] = {5, 10, 3};
    CHECK(!less(r[4], same) && !less(same, r[4]));             // equal records: neither way
    std::vector<const int64_t *> v = {r[6], r[2], r[5], r[0], r[4], r[3], r[1]};
    std::sort(v.begin(), v.end(), less);
    for (int i = 0; i < n; i++) CHECK(v[(size_t)i] == r[i]);
    // canon_sort: a shuffled list into that order (equal records stay, next to each other), a sorted one untouched
    MatchVec m = chain_of(2, {{1, 11, 1}, {5, 10, 3}, {5, -9, 100}, {5, 10, 3}, {4, 10, 3}});
    canon_sort(m);
    CHECK(m.d == std::vector<int64_t>({5, -9, 100, 4, 10, 3, 5, 10, 3, 5, 10, 3, 1, 11, 1}));
    canon_sort(m);
    CHECK(m.size() == 5 && m.d == std::vector<int64_t>({5, -9, 100, 4, 10, 3, 5, 10, 3, 5, 10, 3, 1, 11, 1}));
    // three genomes: the third start decides when the first two agree
    const int64_t x[] = {5, 10, 3, -7}, y[] = {5, 10, 3, 2};
    CHECK(canon_less(3)(x, y) && !canon_less(3)(y, x) && !canon_less(2)(x, y));
}

static void test_clear_bits()
{
    const uint64_t ones = ~0ULL;
    {   // bases 3..6 = bits 2..5 of word 0
        uint64_t M[4] = {ones, ones, ones, ones};
        clear_bits(M, 3, 6);
        CHECK(M[0] == 0xffffffffffffffc3ULL && M[1] == ones && M[2] == ones && M[3] == ones);
    }
    {   // bases 61..64: ends exactly on the word boundary
        uint64_t M[4] = {ones, ones, ones, ones};
        clear_bits(M, 61, 64);
        CHECK(M[0] == 0x0fffffffffffffffULL && M[1] == ones && M[2] == ones && M[3] == ones);
    }
    {   // bases 65..128: exactly one whole word, shift 0
        uint64_t M[4] = {ones, ones, ones, ones};
        clear_bits(M, 65, 128);
        CHECK(M[0] == ones && M[1] == 0 && M[2] == ones && M[3] == ones);
    }
    {   // bases 60..135: bits 59..63 of word 0, all of word 1, bits 0..6 of word 2
        uint64_t M[4] = {ones, ones, ones, ones};
        clear_bits(M, 60, 135);
        CHECK(M[0] == 0x07ffffffffffffffULL && M[1] == 0 && M[2] == 0xffffffffffffff80ULL && M[3] == ones);
    }
    {   // a single base, and an empty range
        uint64_t M[2] = {ones, ones};
        clear_bits(M, 64, 64); CHECK(M[0] == 0x7fffffffffffffffULL && M[1] == ones);
        clear_bits(M, 70, 69); CHECK(M[0] == 0x7fffffffffffffffULL && M[1] == ones);
    }
}

static void test_full_mask()
{
    CHECK(full_mask(1) == 1u && full_mask(31) == 0x7fffffffu && full_mask(32) == 0xffffffffu);
}

static bool same_gap(const GapRef &g, int64_t lcb, int64_t idx, bool dp, int64_t slot, int64_t tot)
{
    return g.lcb == lcb && g.idx == idx && g.dp == dp && g.dp_slot == slot && g.tot == tot;
}
static bool same_row(const DpSeqDesc &d, int genome, int rev, int64_t lo0, int64_t len)
{
    return d.genome == genome && d.rev == rev && d.lo0 == lo0 && d.len == len;
}

static void test_host_gap_table()
{
    // chain 0, all forward; the stretches behind its anchors:
    //   0: none in any genome                               -> skipped
    //   1: 5 bases (220..224) of genome 1 only              -> no DP, tot 5
    //   2: 10 bases each (130.., 235.., 330..)              -> DP
    //   3: 100 / 5 / 5 bases (150.., 255.., 350..)          -> over the limit of 50: no DP, tot 110
    // chain 1, genome 2 reverse: 10 (1020..) / 5 (2020..) / 10 (3090..3099, reverse) -> DP
    std::vector<MatchVec> chains;
    chains.push_back(chain_of(3, {{10, 100, 200, 300}, {10, 110, 210, 310}, {10, 120, 225, 320}, {10, 140, 245, 340}, {10, 250, 260, 355}}));
    chains.push_back(chain_of(3, {{20, 1000, 2000, -3100}, {20, 1030, 2025, -3070}}));
    {
        std::vector<GapRef> gaps; std::vector<DpSeqDesc> desc; int64_t n_dp = 0, codes = 0;
        host_gap_table(chains, 3, nullptr, 1, 50, gaps, desc, n_dp, codes);
        CHECK(gaps.size() == 4 && desc.size() == 6 && n_dp == 2 && codes == 55);
        CHECK(same_gap(gaps[0], 0, 1, false, -1, 5) && same_gap(gaps[1], 0, 2, true, 0, 30));
        CHECK(same_gap(gaps[2], 0, 3, false, -1, 110) && same_gap(gaps[3], 1, 0, true, 1, 25));
        CHECK(same_row(desc[0], 0, 0, 129, 10) && same_row(desc[1], 1, 0, 234, 10) && same_row(desc[2], 2, 0, 329, 10));
        CHECK(same_row(desc[3], 0, 0, 1019, 10) && same_row(desc[4], 1, 0, 2019, 5) && same_row(desc[5], 2, 1, 3089, 10));
    }
    {   // the limit is inclusive: 10 takes both 10-base intervals, 9 takes neither
        std::vector<GapRef> gaps; std::vector<DpSeqDesc> desc; int64_t n_dp = 0, codes = 0;
        host_gap_table(chains, 3, nullptr, 1, 10, gaps, desc, n_dp, codes);
        CHECK(gaps.size() == 4 && n_dp == 2 && codes == 55);
        gaps.clear(); desc.clear(); n_dp = codes = 0;
        host_gap_table(chains, 3, nullptr, 1, 9, gaps, desc, n_dp, codes);
        CHECK(gaps.size() == 4 && n_dp == 0 && codes == 0 && desc.empty());
    }
    {   // gapped alignment off: the same stretches, no DP anywhere
        std::vector<GapRef> gaps; std::vector<DpSeqDesc> desc; int64_t n_dp = 0, codes = 0;
        host_gap_table(chains, 3, nullptr, 0, 50, gaps, desc, n_dp, codes);
        CHECK(gaps.size() == 4 && desc.empty() && n_dp == 0 && codes == 0);
        CHECK(same_gap(gaps[0], 0, 1, false, -1, 5) && same_gap(gaps[1], 0, 2, false, -1, 30));
        CHECK(same_gap(gaps[2], 0, 3, false, -1, 110) && same_gap(gaps[3], 1, 0, false, -1, 25));
    }
    {   // a node of genomes 4, 0, 2 appending behind what the caller's vectors hold
        const int gmap[3] = {4, 0, 2};
        std::vector<GapRef> gaps(1, GapRef{77, 78, true, 79, 80});
        std::vector<DpSeqDesc> desc(1, DpSeqDesc{9, 1, 11, 12});
        int64_t n_dp = 7, codes = 100;
        host_gap_table(chains, 3, gmap, 1, 50, gaps, desc, n_dp, codes);
        CHECK(gaps.size() == 5 && desc.size() == 7 && n_dp == 9 && codes == 155);
        CHECK(same_gap(gaps[0], 77, 78, true, 79, 80) && same_row(desc[0], 9, 1, 11, 12));
        CHECK(same_gap(gaps[2], 0, 2, true, 7, 30) && same_gap(gaps[4], 1, 0, true, 8, 25));
        CHECK(same_row(desc[1], 4, 0, 129, 10) && same_row(desc[2], 0, 0, 234, 10) && same_row(desc[3], 2, 0, 329, 10));
        CHECK(same_row(desc[4], 4, 0, 1019, 10) && same_row(desc[5], 0, 0, 2019, 5) && same_row(desc[6], 2, 1, 3089, 10));
    }
}

int main()
{
    test_gap_of();
    test_chain_extent();
    test_canon_less();
    test_clear_bits();
    test_full_mask();
    test_host_gap_table();
    printf(bad ? "FAIL %d\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
