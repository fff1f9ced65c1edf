// HipCoordinateIndex against the host column walks it stands in for (usage: coord_test alignment.xmfa):
// an IntervalList read from an XMFA goes through the device index, and every answer -- every column of every interval through
// GetColumns, every residue through SeqPosToColumn and Translate -- is compared with Interval::GetColumn and
// CompactGappedAlignment::SeqPosToColumn.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include "libMems/CoordinateIndex.h"
#include "libMems/CompactGappedAlignment.h"

using namespace mems;

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "coord_test: %s failed at line %d\n", #c, __LINE__); return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: coord_test alignment.xmfa\n"); return 2; }
    try {
        IntervalList il;
        std::ifstream in(argv[1]);
        REQUIRE(in.good());
        il.ReadStandardAlignment(in);
        REQUIRE(il.size() > 0);
        HipCoordinateIndex ix(il);
        const uint N = ix.SeqCount();
        // rule 1: every column of every interval
        std::vector<int64_t> blocks, cols, pos, near_pos; std::vector<uint32_t> defined, near_defined;
        for (size_t i = 0; i < il.size(); i++) for (gnSeqI c = 0; c < il[i].AlignmentLength(); c++) { blocks.push_back((int64_t)i); cols.push_back((int64_t)c); }
        ix.GetColumns(blocks, cols, pos, defined);
        ix.GetColumns(blocks, cols, near_pos, near_defined, true);
        REQUIRE(pos.size() == blocks.size() * N && defined.size() == blocks.size() && near_defined == defined);
        // ... and what the host says about them; the residues found are the questions of rules 2 and 3
        std::vector<int32_t> seqs; std::vector<int64_t> positions, want_block, want_col; std::vector<size_t> want_row;
        std::vector<gnSeqI> hp; std::vector<bool> hc;
        size_t q = 0, reverse_residues = 0, gapped = 0;
        for (size_t i = 0; i < il.size(); i++) {
            const Interval &iv = il[i];
            std::vector<int64_t> last(N, 0);                     // the residue last seen in this interval, signed
            for (gnSeqI c = 0; c < iv.AlignmentLength(); c++, q++) {
                iv.GetColumn(c, hp, hc);
                uint32_t mask = 0;
                for (uint g = 0; g < N; g++) {
                    const bool here = g < hc.size() && hc[g];
                    const int64_t want = here ? (iv.Orientation(g) == AbstractMatch::reverse ? -(int64_t)hp[g] : (int64_t)hp[g]) : 0;
                    REQUIRE(pos[q * N + g] == want);
                    if (here) {
                        mask |= 1u << g; last[g] = want;
                        reverse_residues += want < 0;
                        seqs.push_back((int32_t)g); positions.push_back((int64_t)hp[g]); want_block.push_back((int64_t)i); want_col.push_back((int64_t)c); want_row.push_back(q);
                        REQUIRE(near_pos[q * N + g] == want);
                    } else if (g < iv.SeqCount() && iv.LeftEnd(g)) {
                        gapped++;
                        const int64_t first = iv.Orientation(g) == AbstractMatch::reverse ? -(int64_t)iv.RightEnd(g) : (int64_t)iv.LeftEnd(g);
                        REQUIRE(near_pos[q * N + g] == (last[g] ? last[g] : first));
                    } else REQUIRE(near_pos[q * N + g] == 0);
                }
                REQUIRE(defined[q] == mask);
            }
        }
        REQUIRE(gapped > 0);
        // rule 2 against CompactGappedAlignment::SeqPosToColumn, rule 3 against the rows above
        std::vector<int64_t> got_block, got_col, out, out_block; std::vector<uint32_t> out_defined;
        ix.SeqPosToColumn(seqs, positions, got_block, got_col);
        ix.Translate(seqs, positions, out, out_defined, out_block);
        REQUIRE(got_block == want_block && got_col == want_col && out_block == want_block);
        size_t k = 0;
        for (size_t i = 0; i < il.size(); i++) {
            const CompactGappedAlignment<> cga(il[i]);
            for (; k < seqs.size() && want_block[k] == (int64_t)i; k++) {
                REQUIRE((int64_t)cga.SeqPosToColumn((uint)seqs[k], (gnSeqI)positions[k]) == got_col[k]);
                for (uint g = 0; g < N; g++) REQUIRE(out[k * N + g] == pos[want_row[k] * N + g]);
                REQUIRE(out_defined[k] == defined[want_row[k]]);
            }
        }
        REQUIRE(k == seqs.size());
        // a base no interval holds: -1 / -1, zeros
        int64_t top = 0;
        for (const Interval &iv : il) top = std::max<int64_t>(top, (int64_t)iv.RightEnd(0));
        std::vector<int32_t> s1(1, 0); std::vector<int64_t> p1(1, top + 1);
        ix.SeqPosToColumn(s1, p1, got_block, got_col);
        ix.Translate(s1, p1, out, out_defined, out_block, true);
        REQUIRE(got_block[0] == -1 && got_col[0] == -1 && out_block[0] == -1 && out_defined[0] == 0);
        for (uint g = 0; g < N; g++) REQUIRE(out[g] == 0);
        // a question outside the list is an error, not an answer
        bool threw = false;
        try { std::vector<int64_t> b1(1, (int64_t)il.size()), c1(1, 0); ix.GetColumns(b1, c1, pos, defined); } catch (const genome::gnException &) { threw = true; }
        REQUIRE(threw);
        printf("%zu columns, %zu residues (%zu on the reverse strand), %zu gapped entries\nOK\n", blocks.size(), seqs.size(), reverse_residues, gapped);
    } catch (const genome::gnException &e) {
        fprintf(stderr, "coord_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
