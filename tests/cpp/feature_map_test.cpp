// The host walk that DESIGN.md S21 stands in for, on the mirror's classes (libMems/CompactGappedAlignment.h), and HipFeatureMap
// (libMems/FeatureMap.h).
// usage: feature_map_test alignment.xmfa ranges.txt                                  (host only)
//        feature_map_test alignment.xmfa --device genomes.mfa genes.txt features.txt
// ranges.txt, genes.txt, features.txt: one "seq lo hi" per line.
// Host part (no device): for every range the intervals it intersects, by left end in its sequence, the range clipped to each,
// CompactGappedAlignment::SeqPosToColumn on both ends (swapped on the reverse strand, getOrthologList.cpp:221-222), copyRange, and
// Length / LeftEnd / RightEnd of every row of the copy; per piece one line
//   piece <range> <interval> <clip_lo> <clip_hi> <col> <len> | <residues>:<signed left end>:<signed right end> per sequence
// for the caller to compare with the restatement's pieces.
// With --device the sequences are uploaded, the list indexed and HipFeatureMap::OrthologRows run on the genes against the features; per gene
//   row <gene> <interval> <rearranged> <identity as a hex float> | <feature>:<shared bases> per sequence
// and the device's pieces of the genes are compared with the host walk here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include "libMems/CompactGappedAlignment.h"
#include "libMems/FeatureMap.h"

using namespace mems;

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "feature_map_test: %s failed at line %d\n", #c, __LINE__); return 1; } } while (0)

struct HostPiece { int64_t query, block, clip_lo, clip_hi, col, len; std::vector<int64_t> n_res, ext_left, ext_right; };

static bool read_ranges(const char *path, std::vector<AnnotatedRange> &out)
{
    std::ifstream in(path);
    if (!in.good()) return false;
    long long s, lo, hi;
    while (in >> s >> lo >> hi) out.push_back(AnnotatedRange{(uint)s, (int64_t)lo, (int64_t)hi});
    return true;
}

static void host_walk(const IntervalList &il, uint N, const std::vector<AnnotatedRange> &ranges, std::vector<HostPiece> &pieces)
{
    for (size_t q = 0; q < ranges.size(); q++) {
        const uint s = ranges[q].seq;
        std::vector<std::pair<int64_t, size_t>> hit;                       // (left end, interval)
        for (size_t i = 0; i < il.size(); i++) {
            if (s >= il[i].SeqCount() || il[i].Start(s) == NO_MATCH) continue;
            if ((int64_t)il[i].LeftEnd(s) <= ranges[q].hi && (int64_t)il[i].RightEnd(s) >= ranges[q].lo) hit.push_back(std::make_pair((int64_t)il[i].LeftEnd(s), i));
        }
        std::sort(hit.begin(), hit.end());
        for (const auto &h : hit) {
            const Interval &iv = il[h.second];
            const CompactGappedAlignment<> cga(iv);
            HostPiece p;
            p.query = (int64_t)q; p.block = (int64_t)h.second;
            p.clip_lo = std::max<int64_t>(ranges[q].lo, (int64_t)iv.LeftEnd(s)); p.clip_hi = std::min<int64_t>(ranges[q].hi, (int64_t)iv.RightEnd(s));
            gnSeqI lcol = cga.SeqPosToColumn(s, (gnSeqI)p.clip_lo), rcol = cga.SeqPosToColumn(s, (gnSeqI)p.clip_hi);
            if (iv.Orientation(s) == AbstractMatch::reverse) std::swap(lcol, rcol);
            p.col = (int64_t)lcol; p.len = (int64_t)(rcol - lcol + 1);
            CompactGappedAlignment<> part;
            cga.copyRange(part, lcol, rcol - lcol + 1);
            for (uint g = 0; g < N; g++) {
                const bool some = g < part.SeqCount() && part.Start(g) != NO_MATCH;
                const int64_t sign = some && part.Orientation(g) == AbstractMatch::reverse ? -1 : 1;
                p.n_res.push_back(some ? (int64_t)part.Length(g) : 0);
                p.ext_left.push_back(some ? sign * (int64_t)part.LeftEnd(g) : 0);
                p.ext_right.push_back(some ? sign * (int64_t)part.RightEnd(g) : 0);
            }
            pieces.push_back(p);
        }
    }
}

int main(int argc, char **argv)
{
    if (argc != 3 && !(argc == 6 && !strcmp(argv[2], "--device"))) { fprintf(stderr, "usage: feature_map_test alignment.xmfa (ranges.txt | --device genomes.mfa genes.txt features.txt)\n"); return 2; }
    try {
        IntervalList il;
        std::ifstream in(argv[1]);
        REQUIRE(in.good());
        il.ReadStandardAlignment(in);
        uint N = 0;
        for (const Interval &iv : il) N = std::max(N, iv.SeqCount());
        const bool device = argc == 6;
        std::vector<AnnotatedRange> ranges, features;
        REQUIRE(read_ranges(argv[device ? 4 : 2], ranges));
        std::vector<HostPiece> pieces;
        host_walk(il, N, ranges, pieces);
        if (!device) {
            for (const HostPiece &p : pieces) {
                printf("piece %lld %lld %lld %lld %lld %lld |", (long long)p.query, (long long)p.block, (long long)p.clip_lo, (long long)p.clip_hi, (long long)p.col, (long long)p.len);
                for (uint g = 0; g < N; g++) printf(" %lld:%lld:%lld", (long long)p.n_res[g], (long long)p.ext_left[g], (long long)p.ext_right[g]);
                printf("\n");
            }
        } else {
            REQUIRE(read_ranges(argv[5], features));
            LoadMFASequences(il, argv[3], nullptr);
            REQUIRE((uint)il.seq_table.size() == N);
            HipContext &hc = HipContext::global();
            { MatchList ml; ml.seq_table = il.seq_table; ml.upload(hc); ml.seq_table.clear(); }      // the sequences first, then the index
            HipCoordinateIndex ix(il, hc);
            HipFeatureMap fm(ix);
            RangePieces m;
            fm.MapRanges(ranges, m);
            REQUIRE(m.PieceCount() == pieces.size() && m.piece_off.size() == ranges.size() + 1);
            for (size_t p = 0; p < pieces.size(); p++) {
                const HostPiece &h = pieces[p];
                REQUIRE(m.piece_query[p] == h.query && m.piece_block[p] == h.block && m.clip_lo[p] == h.clip_lo && m.clip_hi[p] == h.clip_hi && m.piece_col[p] == h.col && m.piece_len[p] == h.len);
                for (uint g = 0; g < N; g++) REQUIRE(m.n_res[p * N + g] == h.n_res[g] && m.ext_left[p * N + g] == h.ext_left[g] && m.ext_right[p * N + g] == h.ext_right[g]);
            }
            const std::vector<OrthologRow> rows = fm.OrthologRows(ranges, features);
            REQUIRE(rows.size() == ranges.size());
            for (size_t q = 0; q < rows.size(); q++) {
                printf("row %zu %lld %d %a |", q, (long long)rows[q].block, rows[q].rearranged ? 1 : 0, rows[q].identity);
                for (uint g = 0; g < N; g++) printf(" %lld:%lld", (long long)rows[q].ortholog[g], (long long)rows[q].overlap[g]);
                printf("\n");
            }
            printf("%zu genes, %zu pieces equal to the host walk\n", ranges.size(), pieces.size());
        }
        printf("OK\n");
    } catch (const genome::gnException &e) {
        fprintf(stderr, "feature_map_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
