// recursion_host.hpp -- the pure steps of the recursive anchoring's host side (recursive.cpp): the map from a record
// inside a gap to real coordinates, the message the ranks of a sharded batch exchange, and the merge of the new
// anchors into their chain.
//
// Host only, no HIP include (like host_chain.hpp): tests/cpp/recursion_host_test.cpp compiles it with plain g++.
#pragma once
#include <string>
#include <utility>

#include "host_chain.hpp"

// What chaining a recursion batch leaves, whichever way it was chained: the n surviving matches in list order, gap by
// gap.  gap[q]: the gap (index within this rank's batch) of record q, len[q] its length, st[q * N + g] its start in the
// batch's virtual genome g (1-based; behind the gap's segment start).  A view: of the page-locked block a device route
// filled (no copy of a large batch's survivors), or of the vectors the host route appended to.
struct RecSurvivors {
    size_t n = 0;
    const uint32_t *gap = nullptr; const int32_t *len = nullptr, *st = nullptr;
    std::vector<uint32_t> own_gap; std::vector<int32_t> own_len, own_st;
    void push(uint32_t k, int32_t l, const int32_t *starts, int N) { own_gap.push_back(k); own_len.push_back(l); own_st.insert(own_st.end(), starts, starts + N); }
    void view_own() { n = own_gap.size(); gap = own_gap.data(); len = own_len.data(); st = own_st.data(); }
};

// signed real start of a record of length len at s (1-based inside the gap) in a gap with real left end lo and length ln;
// rev: the genome runs backwards through the gap, so the record is mirrored inside it
inline int64_t rec_real_start(int64_t lo, int64_t ln, bool rev, int64_t s, int64_t len)
{
    return rev ? -((lo + ln - 1) - (s - 1) - len + 1) : lo + s - 1;
}

// ---- the message of one rank of a sharded batch: per gap with new anchors [place in the batch, n, n records]; a rank
// ---- that failed sends the marker [-1, status] instead, so that the others do not wait in the collective for ever
inline void shard_msg_append(std::vector<int64_t> &msg, uint32_t place, const MatchVec &gl)
{
    msg.push_back((int64_t)place); msg.push_back((int64_t)gl.size());
    msg.insert(msg.end(), gl.d.begin(), gl.d.end());
}
inline void shard_msg_fail(std::vector<int64_t> &msg, int status) { msg.assign(2, 0); msg[0] = -1; msg[1] = status; }

// every rank's part (N-way records) -> the gaps of the whole batch of `batch` gaps in batch order: (place, its [place, n, records]).
// MAUVE_ERR_STATE with the reason in err when a part is malformed, a rank failed or a place lies outside the batch.
inline int shard_msg_parse(const std::vector<std::pair<const char *, size_t>> &parts, int N, size_t batch,
                           std::vector<std::pair<uint32_t, const int64_t *>> &got, std::string &err)
{
    got.clear();
    for (size_t r = 0; r < parts.size(); r++) {
        const int64_t *v = reinterpret_cast<const int64_t *>(parts[r].first), *e = v + parts[r].second / 8;
        if (parts[r].second % 8) { err = "recursion shard: a rank's part is not a whole number of words"; return MAUVE_ERR_STATE; }
        if (e - v >= 2 && v[0] == -1) { err = "recursion shard: rank " + std::to_string(r) + " failed (status " + std::to_string(v[1]) + ")"; return MAUVE_ERR_STATE; }
        while (v < e) {
            if (e - v < 2 || v[0] < 0 || v[1] < 0 || v[1] > (e - v - 2) / (1 + N)) { err = "recursion shard: a rank's part ends inside a record"; return MAUVE_ERR_STATE; }
            got.push_back({(uint32_t)v[0], v}); v += 2 + v[1] * (1 + N);
        }
    }
    std::sort(got.begin(), got.end(), [](const std::pair<uint32_t, const int64_t *> &x, const std::pair<uint32_t, const int64_t *> &y) { return x.first < y.first; });
    if (!got.empty() && got.back().first >= batch) { err = "recursion shard: ranks disagree about the work list"; return MAUVE_ERR_STATE; }
    return MAUVE_OK;
}

// The new anchors of a chain (add: in genome-0 order) into it: the chain is in genome-0 order already, so the two lists are
// merged -- distinct starts in genome 0, as anchors of one chain never overlap.  In place, from the back: the chain's buffer
// keeps its capacity from call to call, so no fresh 10 MB vector (and its page faults) per alignment; every record moves once.
inline void merge_sorted_anchors(MatchVec &chain, const MatchVec &add)
{
    const size_t R1 = (size_t)(1 + chain.N), na = chain.size(), nb = add.size();
    chain.d.resize((na + nb) * R1);
    const int64_t *B = add.d.data();
    int64_t *D = chain.d.data();
    size_t a = na, b = nb, o = na + nb;
    while (b > 0) {
        if (a > 0 && std::llabs(D[(a - 1) * R1 + 1]) > std::llabs(B[(b - 1) * R1 + 1])) { a--; o--; std::copy(D + a * R1, D + (a + 1) * R1, D + o * R1); }
        else { b--; o--; std::copy(B + b * R1, B + (b + 1) * R1, D + o * R1); }
    }                                                          // (what is left of the chain is in place already)
}
