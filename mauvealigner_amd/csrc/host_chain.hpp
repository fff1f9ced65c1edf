// host_chain.hpp -- the pure steps of the host orchestration between the seed pass and the DP stage: the match
// list type, the stretch between two anchors of a chain, the extent of a chain, the canonical order of N-way
// records, the word-wise clearing of a base mask and the interval table of a set of chains.  One copy each, for
// the align path (pipeline.cpp), the progressive path (progressive.cpp), the recursion (recursive.cpp) and the
// device LCB extension's host half (extend_dev.hip).
//
// Host only, no HIP include (like workers.hpp): tests/cpp/host_chain_test.cpp compiles it with plain g++.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/mauve_hip.h"

// N-way match list in flat records of (1 + N) int64: length, signed 1-based starts (libMems Match layout).
struct MatchVec {
    int N = 0;
    std::vector<int64_t> d;
    explicit MatchVec(int n = 0) : N(n) {}
    size_t size() const { return d.size() / (size_t)(1 + N); }
    bool empty() const { return d.empty(); }
    int64_t &len(size_t i) { return d[i * (1 + N)]; }
    int64_t len(size_t i) const { return d[i * (1 + N)]; }
    int64_t *st(size_t i) { return &d[i * (1 + N) + 1]; }
    const int64_t *st(size_t i) const { return &d[i * (1 + N) + 1]; }
    const int64_t *rec(size_t i) const { return &d[i * (1 + N)]; }
    void push(const int64_t *r) { d.insert(d.end(), r, r + 1 + N); }
    void push(int64_t l, const int64_t *starts) { d.push_back(l); d.insert(d.end(), starts, starts + N); }
    void resize(size_t n) { d.resize(n * (1 + N)); }
    void move(size_t dst, size_t src) { if (dst != src) std::copy(d.begin() + src * (1 + N), d.begin() + (src + 1) * (1 + N), d.begin() + dst * (1 + N)); }
    void reserve(size_t n) { d.reserve(n * (1 + N)); }
    void sort_by_start0();             // chain_host.cpp
};
struct DpSeqDesc { int32_t genome; int32_t rev; int64_t lo0; int64_t len; };   // lo0: 0-based left end in the genome

// one non-empty stretch between anchor idx and idx + 1 of chain lcb: aligned by the DP (slot dp_slot of the descriptor
// table) or, if not, tot bases laid out genome by genome
struct GapRef { int64_t lcb, idx; bool dp; int64_t dp_slot; int64_t tot; };

// every genome of an n-way column
inline uint32_t full_mask(int n) { return n >= 32 ? 0xffffffffu : ((1u << n) - 1); }

// inter-anchor interval of genome g between anchors a (left in genome-0 order) and b, LCB orientation: 1-based left
// end lo, length len (0 where the anchors touch or overlap), rev = the genome runs backwards through the chain
inline void gap_of(const int64_t *a, const int64_t *b, int g, int64_t &lo, int64_t &len, bool &rev)
{
    const int64_t sa = a[1 + g], sb = b[1 + g];
    int64_t hi;
    if (sa > 0) { lo = sa + a[0]; hi = sb - 1; rev = false; }
    else { lo = -sb + b[0]; hi = -sa - 1; rev = true; }
    len = hi - lo + 1; if (len < 0) len = 0;
}
inline void gap_of(const int64_t *a, const int64_t *b, int g, int64_t &lo, int64_t &len) { bool rev; gap_of(a, b, g, lo, len, rev); }

// extent of a non-empty chain in genome g: the anchors are ordered, so the ends come from the first and the last one
inline void chain_extent(const MatchVec &ch, int g, int64_t &le, int64_t &re, bool &rev)
{
    const size_t last = ch.size() - 1;
    const int64_t s0 = ch.st(0)[g], s1 = ch.st(last)[g];
    if (s0 > 0) { le = s0; re = s1 + ch.len(last) - 1; }
    else { le = -s1; re = -s0 + ch.len(0) - 1; }
    rev = s0 < 0;
}

// canonical order of N-way records: |start 0|, signed starts, length
inline auto canon_less(int N)
{
    return [N](const int64_t *a, const int64_t *b) {
        const int64_t sa = std::llabs(a[1]), sb = std::llabs(b[1]);
        if (sa != sb) return sa < sb;
        for (int g = 0; g < N; g++) if (a[1 + g] != b[1 + g]) return a[1 + g] < b[1 + g];
        return a[0] < b[0];
    };
}
// a list into that order (records that compare equal are equal: the result does not depend on the sort)
inline void canon_sort(MatchVec &m)
{
    std::vector<size_t> idx(m.size());
    for (size_t i = 0; i < idx.size(); i++) idx[i] = i;
    auto by = [&m, less = canon_less(m.N)](size_t x, size_t y) { return less(m.rec(x), m.rec(y)); };
    if (std::is_sorted(idx.begin(), idx.end(), by)) return;
    std::stable_sort(idx.begin(), idx.end(), by);
    MatchVec t(m.N); t.reserve(m.size());
    for (size_t i : idx) t.push(m.rec(i));
    m.d.swap(t.d);
}

// clear the bits of the bases lo .. hi (1-based, inclusive) of a 1-bit-per-base mask, word-wise
inline void clear_bits(uint64_t *M, int64_t lo, int64_t hi)
{
    for (int64_t b = lo - 1; b < hi;) {
        const int64_t w = b >> 6, e = std::min<int64_t>(hi, (w + 1) << 6);
        const int n = (int)(e - b), sh = (int)(b & 63);
        M[w] &= ~((n == 64 ? ~0ULL : ((1ULL << n) - 1ULL)) << sh);
        b = e;
    }
}

// The interval table of a set of chains: every non-empty stretch between two consecutive anchors becomes a GapRef, and one
// that at least two of the n genomes have and whose longest side is within len_limit (gapped alignment on) gets a DP slot
// and n descriptor rows (gmap: the genomes of the chains' components, nullptr = 0 .. n-1).  Appends to gaps and desc and
// counts on in n_dp and code_total: the caller's vectors keep their capacity.
inline void host_gap_table(const std::vector<MatchVec> &chains, int n, const int *gmap, int gapped, int64_t len_limit,
                           std::vector<GapRef> &gaps, std::vector<DpSeqDesc> &desc, int64_t &n_dp, int64_t &code_total)
{
    for (size_t l = 0; l < chains.size(); l++) {
        const MatchVec &ch = chains[l];
        for (size_t i = 0; i + 1 < ch.size(); i++) {
            int64_t tot = 0, mx = 0; int nonempty = 0;
            int64_t lo[MAUVE_MAX_SEQ], ln[MAUVE_MAX_SEQ]; bool rv[MAUVE_MAX_SEQ];
            for (int g = 0; g < n; g++) { gap_of(ch.rec(i), ch.rec(i + 1), g, lo[g], ln[g], rv[g]); tot += ln[g]; mx = std::max(mx, ln[g]); nonempty += ln[g] > 0; }
            if (tot == 0) continue;
            GapRef gr{(int64_t)l, (int64_t)i, false, -1, tot};
            if (gapped && nonempty >= 2 && mx <= len_limit) {
                gr.dp = true; gr.dp_slot = n_dp++;
                for (int g = 0; g < n; g++) desc.push_back(DpSeqDesc{gmap ? gmap[g] : g, rv[g], lo[g] - 1, ln[g]});
                code_total += tot;
            }
            gaps.push_back(gr);
        }
    }
}
