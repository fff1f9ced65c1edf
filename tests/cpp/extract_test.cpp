// HipAlignmentExtractor against the host loops it stands in for (usage: extract_test alignment.xmfa genomes.mfa):
// an IntervalList read from an XMFA, with its sequences from a multi-FastA, goes through the device stage; the unconditioned rows are
// compared with Interval::GetAlignment of every interval, StripGapColumns with the stripGapColumns loop written out here
// (stripGapColumns.cpp:32-64: keep the columns without a gap), on all sequences and on a projection, whole and in ranges.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include "libMems/AlignmentExtractor.h"

using namespace mems;

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "extract_test: %s failed at line %d\n", #c, __LINE__); return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: extract_test alignment.xmfa genomes.mfa\n"); return 2; }
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
        REQUIRE(ix.SeqCount() == N);
        HipAlignmentExtractor ex(ix);
        // the host's answer: every interval's GetAlignment strings one behind the other (an absent sequence: all gaps)
        std::vector<std::string> host(N);
        std::vector<int64_t> start(il.size() + 1, 0);
        for (size_t i = 0; i < il.size(); i++) {
            std::vector<std::string> rows;
            il[i].GetAlignment(rows, il.seq_table);
            const size_t n = (size_t)il[i].AlignmentLength();
            for (uint g = 0; g < N; g++) host[g] += g < rows.size() ? rows[g] : std::string(n, '-');
            start[i + 1] = start[i] + (int64_t)n;
        }
        ExtractedColumns w;
        std::vector<std::string> all = ex.Extract(ExtractParams(), nullptr, &w);
        REQUIRE(all == host);
        REQUIRE(w.range_off == start && w.blocks.size() == host[0].size());
        for (size_t j = 0; j < w.blocks.size(); j++) REQUIRE(start[(size_t)w.blocks[j]] + w.cols[j] == (int64_t)j);
        // stripGapColumns on all sequences and on a projection (last sequence first): the columns without a gap, in order
        std::vector<std::vector<uint>> projections;
        projections.push_back(std::vector<uint>());
        projections.push_back(std::vector<uint>{N - 1, 0});
        size_t reverse_cells = 0;
        for (const std::vector<uint> &proj : projections) {
            std::vector<uint> rows_of = proj;
            if (rows_of.empty()) for (uint g = 0; g < N; g++) rows_of.push_back(g);
            std::vector<std::string> want(rows_of.size());
            std::vector<int64_t> want_col;
            for (size_t c = 0; c < host[0].size(); c++) {
                bool gap = false;
                for (uint g : rows_of) gap = gap || host[g][c] == '-';
                if (gap) continue;
                for (size_t k = 0; k < rows_of.size(); k++) want[k].push_back(host[rows_of[k]][c]);
                want_col.push_back((int64_t)c);
            }
            REQUIRE(!want[0].empty() && want[0].size() < host[0].size());
            std::vector<std::string> got = ex.StripGapColumns(proj, nullptr, &w);
            REQUIRE(got == want);
            for (size_t j = 0; j < want_col.size(); j++) REQUIRE(start[(size_t)w.blocks[j]] + w.cols[j] == want_col[j]);
            // ... and the positions of those columns are one GetColumns away: on the reverse strand the letter is the complement
            std::vector<int64_t> pos; std::vector<uint32_t> defined;
            ix.GetColumns(w.blocks, w.cols, pos, defined);
            for (size_t j = 0; j < want_col.size(); j++)
                for (size_t k = 0; k < rows_of.size(); k++) {
                    const int64_t p = pos[j * N + rows_of[k]];
                    REQUIRE(p != 0);
                    REQUIRE(got[k][j] == Interval::base_char(il.seq_table[rows_of[k]]->str()[(size_t)(p < 0 ? -p : p) - 1], p < 0));
                    reverse_cells += p < 0;
                }
        }
        REQUIRE(reverse_cells > 0);
        // ranges: the second half of every interval, then the first interval once more
        std::vector<ColumnRange> ranges;
        for (size_t i = 0; i < il.size(); i++) { const int64_t n = (int64_t)il[i].AlignmentLength(); ranges.push_back(ColumnRange{(int64_t)i, n / 2, n - n / 2}); }
        ranges.push_back(ColumnRange{0, 0, (int64_t)il[0].AlignmentLength()});
        std::vector<std::string> part = ex.Extract(ExtractParams(), &ranges, &w);
        std::vector<std::string> want(N);
        for (const ColumnRange &r : ranges) for (uint g = 0; g < N; g++) want[g] += host[g].substr((size_t)(start[(size_t)r.block] + r.col), (size_t)r.len);
        REQUIRE(part == want && w.range_off.size() == ranges.size() + 1 && w.range_off.back() == (int64_t)want[0].size());
        // a range outside the list is an error, not an answer
        bool threw = false;
        std::vector<ColumnRange> bad(1, ColumnRange{(int64_t)il.size(), 0, 1});
        try { ex.Extract(ExtractParams(), &bad); } catch (const genome::gnException &) { threw = true; }
        REQUIRE(threw);
        printf("%zu columns, %u sequences, %zu reverse-strand cells checked\nOK\n", host[0].size(), N, reverse_cells);
    } catch (const genome::gnException &e) {
        fprintf(stderr, "extract_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
