// The host projectIntervalList of the mirror (libMems/ProgressiveAligner.h, rules 1 to 3 of DESIGN.md S19), and HipProjection
// (libMems/Projection.h) against it.
// usage: project_test alignment.xmfa [--device genomes.mfa] id id ...
// Host part (no device): the IntervalList read from the XMFA goes through projectIntervalList; per LCB one line
//   lcb <n> : <source interval><+|-> ... | <signed left end>:<signed right end> per projected sequence
// (- = the interval was inverted) for the caller to compare with the restatement's groups.
// With --device the sequences are uploaded, the list indexed and projected on the device: the same groups, the same ends and strands, and the
// same columns, filler included, as an Interval made of the host's adapters; then the projection becomes the
// index in force and answers a column query with the positions of the source.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include "libMems/ProgressiveAligner.h"
#include "libMems/Projection.h"

using namespace mems;

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "project_test: %s failed at line %d\n", #c, __LINE__); return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: project_test alignment.xmfa [--device genomes.mfa] id id ...\n"); return 2; }
    try {
        IntervalList il;
        std::ifstream in(argv[1]);
        REQUIRE(in.good());
        il.ReadStandardAlignment(in);
        int a = 2;
        const char *mfa = nullptr;
        if (!strcmp(argv[a], "--device")) { REQUIRE(argc > a + 2); mfa = argv[a + 1]; a += 2; }
        std::vector<uint> projection;
        for (; a < argc; a++) projection.push_back((uint)atoi(argv[a]));
        REQUIRE(!projection.empty());
        const uint P = (uint)projection.size();

        std::vector<std::vector<MatchProjectionAdapter *>> lcbs;
        std::vector<LCB> adjs;
        projectIntervalList(il, projection, lcbs, adjs);
        REQUIRE(adjs.size() == lcbs.size());
        // which interval of the list an adapter came from: the one with its ends in the first projected sequence
        std::vector<std::vector<int64_t>> piece(lcbs.size());
        std::vector<std::vector<int8_t>> flip(lcbs.size());
        for (size_t l = 0; l < lcbs.size(); l++) {
            printf("lcb %zu :", l);
            for (const MatchProjectionAdapter *m : lcbs[l]) {
                REQUIRE(m->SeqCount() == P && m->Orientation(0) == AbstractMatch::forward);
                int64_t src = -1;
                for (size_t i = 0; i < il.size(); i++)
                    if (projection[0] < il[i].SeqCount() && il[i].LeftEnd(projection[0]) == m->LeftEnd(0) && il[i].RightEnd(projection[0]) == m->RightEnd(0)) src = (int64_t)i;
                REQUIRE(src >= 0);
                const bool inverted = il[(size_t)src].Orientation(projection[0]) == AbstractMatch::reverse;
                for (uint k = 0; k < P; k++) REQUIRE((m->Start(k) < 0) == ((il[(size_t)src].Start(projection[k]) < 0) != inverted));
                piece[l].push_back(src); flip[l].push_back(inverted);
                printf(" %lld%c", (long long)src, inverted ? '-' : '+');
            }
            printf(" |");
            for (uint k = 0; k < P; k++) printf(" %lld:%lld", (long long)adjs[l].left_end[k], (long long)adjs[l].right_end[k]);
            printf("\n");
        }
        if (mfa) {
            LoadMFASequences(il, mfa, nullptr);
            const uint N = (uint)il.seq_table.size();
            HipContext &hc = HipContext::global();
            { MatchList ml; ml.seq_table = il.seq_table; ml.upload(hc); ml.seq_table.clear(); }      // the sequences first, then the index
            HipCoordinateIndex ix(il, hc);
            std::vector<int64_t> start(il.size() + 1, 0);
            for (size_t i = 0; i < il.size(); i++) start[i + 1] = start[i] + (int64_t)il[i].AlignmentLength();
            // the source's answer for every column, before the index is replaced
            std::vector<int64_t> qb, qc, spos; std::vector<uint32_t> sdef;
            for (size_t i = 0; i < il.size(); i++) for (int64_t c = 0; c < (int64_t)il[i].AlignmentLength(); c++) { qb.push_back((int64_t)i); qc.push_back(c); }
            ix.GetColumns(qb, qc, spos, sdef);
            HipProjection pj(ix, projection, false);
            REQUIRE(pj.IntervalCount() == lcbs.size());
            IntervalList wide, compact;
            ProjectionSource w;
            pj.GetIntervals(wide, false, &w);
            pj.GetIntervals(compact, true);
            REQUIRE(wide.size() == lcbs.size() && compact.size() == lcbs.size() && w.piece_off.size() == lcbs.size() + 1);
            size_t col0 = 0, n_flipped = 0, n_filler = 0;
            for (size_t l = 0; l < lcbs.size(); l++) {
                REQUIRE((size_t)(w.piece_off[l + 1] - w.piece_off[l]) == piece[l].size());
                for (size_t q = 0; q < piece[l].size(); q++) {
                    REQUIRE(w.pieces[(size_t)w.piece_off[l] + q] == piece[l][q] && w.flipped[(size_t)w.piece_off[l] + q] == flip[l][q]);
                    n_flipped += flip[l][q];
                }
                REQUIRE(compact[l].SeqCount() == P && wide[l].SeqCount() == N);
                for (uint k = 0; k < P; k++) {
                    REQUIRE(compact[l].Start(k) == adjs[l].left_end[k]);
                    REQUIRE((int64)compact[l].RightEnd(k) == std::llabs(adjs[l].right_end[k]));
                    REQUIRE(wide[l].Start(projection[k]) == compact[l].Start(k) && wide[l].RightEnd(projection[k]) == compact[l].RightEnd(k));
                }
                for (uint g = 0; g < N; g++) if (std::find(projection.begin(), projection.end(), g) == projection.end()) REQUIRE(wide[l].Start(g) == NO_MATCH);
                // the host's adapters as one block (Interval::SetMatches lays the bases between them out as rule 4 does): the device's columns
                Interval host;
                host.SetMatches(lcbs[l]);
                const std::vector<uint32_t> &cc = compact[l].Columns();
                for (size_t c = 0; c < cc.size(); c++) n_filler += w.source_col[col0 + c] < 0;
                REQUIRE(cc == host.Columns());
                for (uint k = 0; k < P; k++) REQUIRE(host.Start(k) == compact[l].Start(k) && host.RightEnd(k) == compact[l].RightEnd(k));
                REQUIRE(wide[l].Columns().size() == cc.size());
                col0 += cc.size();
            }
            REQUIRE(col0 == pj.ColumnCount() && n_filler == pj.FillerColumns());
            // the projection as the index in force: a column that came from the source keeps its positions, negated in an inverted piece
            pj.MakeIndex();
            std::vector<int64_t> pb, pc, ppos; std::vector<uint32_t> pdef;
            for (size_t l = 0; l < wide.size(); l++) for (int64_t c = 0; c < (int64_t)wide[l].AlignmentLength(); c++) { pb.push_back((int64_t)l); pc.push_back(c); }
            ix.GetColumns(pb, pc, ppos, pdef);
            std::vector<char> inv(il.size(), 0);
            for (size_t q = 0; q < w.pieces.size(); q++) inv[(size_t)w.pieces[q]] = w.flipped[q];
            size_t checked = 0;
            for (size_t c = 0; c < pb.size(); c++) {
                const int64_t x = w.source_col[c];
                if (x < 0) continue;
                const size_t i = (size_t)(std::upper_bound(start.begin(), start.end(), x) - start.begin()) - 1;
                for (uint k = 0; k < P; k++) { const uint g = projection[k]; REQUIRE(ppos[c * N + g] == (inv[i] ? -spos[(size_t)x * N + g] : spos[(size_t)x * N + g])); checked++; }
            }
            // a later projection on the context ends this one: it says so instead of fetching the other's arrays into its own sizes
            HipCoordinateIndex ix2(il, hc);
            HipProjection later(ix2, std::vector<uint>(1, projection[0]));
            bool threw = false;
            try { pj.GetIntervals(wide); } catch (const genome::gnException &) { threw = true; }
            REQUIRE(threw);
            IntervalList one;
            later.GetIntervals(one);
            REQUIRE(one.size() == 1 && later.IntervalCount() == 1);
            printf("%zu intervals, %zu columns, %zu filler columns, %zu inverted pieces, %zu positions checked\n", wide.size(), col0, n_filler, n_flipped, checked);
        }
        for (auto &l : lcbs) for (MatchProjectionAdapter *m : l) m->Free();       // (the device part handed them to Intervals)
        printf("OK\n");
    } catch (const genome::gnException &e) {
        fprintf(stderr, "project_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
