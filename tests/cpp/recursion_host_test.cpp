// Host-only check of the pure steps of the recursive anchoring's host side (csrc/recursion_host.hpp): hand cases with
// the expected numbers written out.  Built and run by tests/test_compat_headers.py with plain g++.
#include "recursion_host.hpp"
#include <cstdio>

static int bad = 0;
#define CHECK(x) do { if (!(x)) { printf("line %d: %s\n", __LINE__, #x); bad++; } } while (0)

typedef std::vector<int64_t> Words;
typedef std::vector<std::pair<const char *, size_t>> Parts;
typedef std::vector<std::pair<uint32_t, const int64_t *>> Got;

static MatchVec list_of(int N, std::initializer_list<Words> recs)
{
    MatchVec m(N);
    for (const auto &r : recs) m.push(r.data());
    return m;
}
static std::pair<const char *, size_t> part_of(const Words &w) { return {reinterpret_cast<const char *>(w.data()), w.size() * 8}; }

static void test_real_start()
{
    // forward gap 110..119: local 3..6 is 112..115
    CHECK(rec_real_start(110, 10, false, 3, 4) == 112);
    // reverse gap 475..499: local 3..6 is mirrored to 494..497
    CHECK(rec_real_start(475, 25, true, 3, 4) == -494);
    // a record that fills the whole gap
    CHECK(rec_real_start(110, 10, false, 1, 10) == 110);
    CHECK(rec_real_start(475, 25, true, 1, 25) == -475);
    // s = 1: the gap's first bases -- its last ones (496..499) on the reverse strand; and the other end
    CHECK(rec_real_start(110, 10, false, 1, 4) == 110);
    CHECK(rec_real_start(475, 25, true, 1, 4) == -496);
    CHECK(rec_real_start(110, 10, false, 7, 4) == 116);
    CHECK(rec_real_start(475, 25, true, 22, 4) == -475);
    // one base in a gap of one base
    CHECK(rec_real_start(7, 1, false, 1, 1) == 7 && rec_real_start(7, 1, true, 1, 1) == -7);
}

static void test_message()
{
    const int N = 2;
    Got got; std::string err;
    // rank 0 has the gaps at places 3 (two anchors) and 0 (one) of a batch of 4, rank 1 the gap at place 2, rank 2 nothing
    Words m0, m1, m2;
    shard_msg_append(m0, 3, list_of(N, {{10, 100, -200}, {11, 120, -180}}));
    shard_msg_append(m0, 0, list_of(N, {{12, 5, 6}}));
    shard_msg_append(m1, 2, list_of(N, {{13, 50, 60}}));
    CHECK(m0 == Words({3, 2, 10, 100, -200, 11, 120, -180, 0, 1, 12, 5, 6}));
    CHECK(m1 == Words({2, 1, 13, 50, 60}) && m2.empty());
    {
        const Parts parts = {part_of(m0), part_of(m1), part_of(m2)};
        CHECK(shard_msg_parse(parts, N, 4, got, err) == MAUVE_OK && err.empty());
        CHECK(got.size() == 3 && got[0].first == 0 && got[1].first == 2 && got[2].first == 3);     // batch order, whoever sent them
        CHECK(got[0].second == m0.data() + 8 && got[1].second == m1.data() && got[2].second == m0.data());
        CHECK(got[0].second[1] == 1 && got[0].second[2] == 12 && got[2].second[1] == 2 && got[2].second[5] == 11);
    }
    {   // only empty parts: nothing to apply
        const Parts parts = {part_of(m2), part_of(m2)};
        CHECK(shard_msg_parse(parts, N, 4, got, err) == MAUVE_OK && got.empty() && err.empty());
    }
    {   // rank 1 failed with status 7: its marker, whatever the others sent
        Words f = {99, 99, 99}; shard_msg_fail(f, 7);
        CHECK(f == Words({-1, 7}));
        const Parts parts = {part_of(m0), part_of(f)};
        CHECK(shard_msg_parse(parts, N, 4, got, err) == MAUVE_ERR_STATE && err == "recursion shard: rank 1 failed (status 7)");
    }
    {   // 20 bytes: two and a half words
        const Parts parts = {part_of(m1), {reinterpret_cast<const char *>(m1.data()), 20}};
        err.clear();
        CHECK(shard_msg_parse(parts, N, 4, got, err) == MAUVE_ERR_STATE && err == "recursion shard: a rank's part is not a whole number of words");
    }
    {   // two records announced, one there; a part of one word; a negative count
        const Words cut = {1, 2, 13, 50, 60}, one = {1}, neg = {1, -3, 13, 50, 60};
        for (const Words *w : {&cut, &one, &neg}) {
            const Parts parts = {part_of(*w)};
            err.clear();
            CHECK(shard_msg_parse(parts, N, 4, got, err) == MAUVE_ERR_STATE && err == "recursion shard: a rank's part ends inside a record");
        }
        // exactly as many as announced is fine
        const Words fit = {1, 2, 13, 50, 60, 14, 70, 80};
        const Parts parts = {part_of(fit)};
        err.clear();
        CHECK(shard_msg_parse(parts, N, 4, got, err) == MAUVE_OK && got.size() == 1 && err.empty());
    }
    {   // place 4 in a batch of 4 gaps; place 3 is the last one there is
        Words m4; shard_msg_append(m4, 4, list_of(N, {{13, 50, 60}}));
        const Parts parts = {part_of(m1), part_of(m4)};
        err.clear();
        CHECK(shard_msg_parse(parts, N, 4, got, err) == MAUVE_ERR_STATE && err == "recursion shard: ranks disagree about the work list");
        err.clear();
        CHECK(shard_msg_parse(parts, N, 5, got, err) == MAUVE_OK && got.size() == 2 && got[1].first == 4 && err.empty());
    }
}

static void test_merge()
{
    {   // new anchors before, between and after the old ones
        MatchVec ch = list_of(2, {{10, 100, 200}, {10, 300, 400}, {10, 500, 600}});
        merge_sorted_anchors(ch, list_of(2, {{5, 50, 150}, {5, 200, 350}, {6, 220, 370}, {5, 400, 450}, {5, 700, 800}}));
        CHECK(ch.d == Words({5, 50, 150, 10, 100, 200, 5, 200, 350, 6, 220, 370, 10, 300, 400, 5, 400, 450, 10, 500, 600, 5, 700, 800}));
    }
    {   // into a chain of one anchor: one before, one after; and only before / only after
        MatchVec ch = list_of(2, {{10, 300, 400}});
        merge_sorted_anchors(ch, list_of(2, {{5, 100, 150}, {5, 500, 650}}));
        CHECK(ch.d == Words({5, 100, 150, 10, 300, 400, 5, 500, 650}));
        MatchVec c1 = list_of(2, {{10, 300, 400}}), c2 = c1;
        merge_sorted_anchors(c1, list_of(2, {{5, 100, 150}}));
        merge_sorted_anchors(c2, list_of(2, {{5, 500, 650}}));
        CHECK(c1.d == Words({5, 100, 150, 10, 300, 400}) && c2.d == Words({10, 300, 400, 5, 500, 650}));
    }
    {   // three genomes, genome 1 reverse (its starts DEscend along the chain): the order is by |start 0| alone
        MatchVec ch = list_of(3, {{10, 100, -900, 50}, {10, 300, -700, 250}});
        merge_sorted_anchors(ch, list_of(3, {{5, 200, -800, 150}, {5, 400, -600, 350}}));
        CHECK(ch.d == Words({10, 100, -900, 50, 5, 200, -800, 150, 10, 300, -700, 250, 5, 400, -600, 350}));
        // ... and by its absolute value
        MatchVec neg = list_of(2, {{10, -100, 5}, {10, -300, 7}});
        merge_sorted_anchors(neg, list_of(2, {{5, -200, 6}}));
        CHECK(neg.d == Words({10, -100, 5, 5, -200, 6, 10, -300, 7}));
    }
    {   // nothing to add: the chain stays as it is
        MatchVec ch = list_of(2, {{10, 100, 200}, {10, 300, 400}});
        const int64_t *where = ch.d.data();
        merge_sorted_anchors(ch, MatchVec(2));
        CHECK(ch.d == Words({10, 100, 200, 10, 300, 400}) && ch.d.data() == where);
        MatchVec none(2);
        merge_sorted_anchors(none, MatchVec(2));
        CHECK(none.empty());
    }
}

static void test_survivors()
{
    // the host route's list: appended to, then seen through the same view as a device route's block
    RecSurvivors S;
    CHECK(S.n == 0);
    const int32_t a[] = {3, 4}, b[] = {5, 6};
    S.push(0, 10, a, 2); S.push(2, 11, b, 2);
    S.view_own();
    CHECK(S.n == 2 && S.gap[0] == 0 && S.gap[1] == 2 && S.len[0] == 10 && S.len[1] == 11);
    CHECK(S.st[0] == 3 && S.st[1] == 4 && S.st[2] == 5 && S.st[3] == 6);
}

int main()
{
    test_real_start();
    test_message();
    test_merge();
    test_survivors();
    printf(bad ? "FAIL %d\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
