// HipAlignmentText against the host writer it stands in for (usage: text_mirror_test alignment.xmfa genomes.mfa [contig_len]):
// an IntervalList read from an XMFA, with its sequences from a multi-FastA, goes through the device stage; the XMFA text must be the bytes of
// IntervalList::WriteStandardAlignment, block_off must cut it at the "=" lines, and the MAF text must carry one "a" block per interval and
// one "s" line per row.  With contig_len the sequences are cut into contigs of that length: a whole interval then crosses a join and is
// refused, and the ranges of ContigRanges() write it.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include "libMems/AlignmentText.h"

using namespace mems;

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "text_mirror_test: %s failed at line %d\n", #c, __LINE__); return 1; } } while (0)

static size_t count_lines(const std::string &s, const std::string &prefix)
{
    size_t n = 0;
    std::istringstream is(s);
    std::string line;
    while (std::getline(is, line)) n += line.compare(0, prefix.size(), prefix) == 0 && (prefix.size() > 1 || line.size() == 1);
    return n;
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: text_mirror_test alignment.xmfa genomes.mfa [contig_len]\n"); return 2; }
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
        HipAlignmentText tx(ix, il);
        std::ostringstream host, dev, maf;
        il.WriteStandardAlignment(host);
        std::vector<int64_t> boff;
        tx.WriteStandardAlignment(dev, nullptr, &boff);
        REQUIRE(dev.str() == host.str());
        REQUIRE(boff.size() == il.size() + 1 && boff.back() == (int64_t)host.str().size());
        for (size_t i = 1; i < boff.size(); i++) REQUIRE(boff[i] > boff[i - 1] && host.str().compare((size_t)boff[i] - 2, 2, "=\n") == 0);
        size_t rows = 0;
        for (const Interval &iv : il) for (uint g = 0; g < N && g < iv.SeqCount(); g++) rows += iv.LeftEnd(g) != 0;
        tx.WriteMAF(maf);
        REQUIRE(maf.str().compare(0, 41, "##maf version=1 program=progressiveMauve\n") == 0);
        REQUIRE(count_lines(maf.str(), "a") == il.size() && count_lines(maf.str(), "s ") == rows);
        size_t split_rows = 0;
        if (argc > 3) {
            const int64_t clen = atoll(argv[3]);
            REQUIRE(clen > 0);
            for (uint g = 0; g < N; g++) {
                std::vector<int64_t> starts;
                for (int64_t s = 0; s < (int64_t)il.seq_table[g]->length(); s += clen) starts.push_back(s);
                il.seq_table[g]->setContigStarts(starts);
            }
            bool threw = false;
            std::ostringstream none;
            try { tx.WriteMAF(none); } catch (const genome::gnException &) { threw = true; }
            REQUIRE(threw);
            const std::vector<ColumnRange> ranges = tx.ContigRanges();
            REQUIRE(ranges.size() > il.size());
            std::ostringstream cut;
            tx.WriteMAF(cut, &ranges, &boff);
            REQUIRE(boff.size() == ranges.size() + 1 && boff.back() == (int64_t)cut.str().size());
            split_rows = count_lines(cut.str(), "s ");
            REQUIRE(split_rows > rows);
            // every row lies inside a contig of that length
            std::istringstream is(cut.str());
            std::string line;
            while (std::getline(is, line)) {
                if (line.compare(0, 2, "s ") != 0) continue;
                std::istringstream f(line.substr(2));
                std::string src, strand; int64_t start, size, total;
                f >> src >> start >> size >> strand >> total;
                REQUIRE(start >= 0 && size > 0 && start + size <= total && total <= clen);
            }
        }
        printf("%zu bytes of XMFA, %zu rows, %zu rows after the split\nOK\n", host.str().size(), rows, split_rows);
    } catch (const genome::gnException &e) {
        fprintf(stderr, "text_mirror_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
