// libMems/AlignmentText.h -- the XMFA or MAF text of an alignment, written on the device.
// IntervalList::WriteStandardAlignment (mauveAligner.cpp:746-760) and xmfa2maf (xmfa2maf.cpp:46-82) ask every interval for its
// GetAlignment strings and print them on one host thread.  Both stay as they are (IntervalList.h).  HipAlignmentText has the device lay
// out and fill the same text for a whole IntervalList (mauve_alignment_text), on a HipCoordinateIndex of that list and the sequences
// resident on the index's context, and streams it into an ostream in slices (mauve_alignment_text_fetch): upload the sequences
// (MatchList::upload, or mauve_set_genomes*) BEFORE the index is built -- an index older than the resident sequences is refused.
#ifndef MAUVE_HIP_ALIGNMENTTEXT_H
#define MAUVE_HIP_ALIGNMENTTEXT_H

#include <ostream>
#include "AlignmentExtractor.h"

namespace mems {

class HipAlignmentText {
public:
    // il: the list the index was built from (its seq_filename / defline_name give the names, its seq_table the contigs)
    HipAlignmentText(const HipCoordinateIndex &ix, const IntervalList &il) : ix_(&ix), il_(&il) {}

    // IntervalList::WriteStandardAlignment: every interval whole, or the ranges given (a block each); 80 letters per line
    void WriteStandardAlignment(std::ostream &os, const std::vector<ColumnRange> *ranges = nullptr, std::vector<int64_t> *block_off = nullptr) const
    {
        Names nm(*il_, ix_->SeqCount());
        mauve_text_params p;
        mauve_default_text_params(MAUVE_TEXT_XMFA, &p);
        make(p, nm.file.data(), nm.defline.data(), nullptr, nullptr, nullptr, ranges);
        stream(os, ranges, block_off);
    }
    // xmfa2maf's text (xmfa2maf.cpp:46-82) with the contigs of the list's seq_table.  The tool's applyBreakpoints pass is not part of the
    // call: a row across a contig join is refused (gnException); pass ContigRanges() to write a multi-contig alignment
    void WriteMAF(std::ostream &os, const std::vector<ColumnRange> *ranges = nullptr, std::vector<int64_t> *block_off = nullptr) const
    {
        const uint N = ix_->SeqCount();
        Names nm(*il_, N);
        std::vector<int64_t> n_contigs(N, 1), starts;
        std::vector<std::string> cname;
        for (uint g = 0; g < N; g++) {
            if (g < il_->seq_table.size() && il_->seq_table[g]) {
                const genome::gnSequence &s = *il_->seq_table[g];
                n_contigs[g] = (int64_t)s.contigListSize();
                for (uint32 k = 0; k < s.contigListSize(); k++) { starts.push_back(s.contigStarts()[k]); cname.push_back(s.contigName(k)); }
            } else { starts.push_back(0); cname.push_back(std::string()); }
        }
        std::vector<const char *> cn(cname.size());
        for (size_t k = 0; k < cname.size(); k++) cn[k] = cname[k].c_str();
        mauve_text_params p;
        mauve_default_text_params(MAUVE_TEXT_MAF, &p);
        make(p, nm.file.data(), nullptr, n_contigs.data(), starts.data(), cn.data(), ranges);
        stream(os, ranges, block_off);
    }
    // the ranges that split every interval at the columns of the contig starts inside it (mauve_seqpos_to_column), in list order: what
    // WriteMAF takes for an alignment whose rows run over contig joins
    std::vector<ColumnRange> ContigRanges() const
    {
        std::vector<int32_t> seqs; std::vector<int64_t> pos;
        for (uint g = 0; g < ix_->SeqCount() && g < il_->seq_table.size(); g++) {
            if (!il_->seq_table[g]) continue;
            const std::vector<int64_t> &cs = il_->seq_table[g]->contigStarts();
            for (size_t k = 1; k < cs.size(); k++) {
                // a join lies between base cs[k] and base cs[k] + 1 (1-based): the cut is in front of the later of their two columns
                seqs.push_back((int32_t)g); pos.push_back(cs[k]);
                seqs.push_back((int32_t)g); pos.push_back(cs[k] + 1);
            }
        }
        std::vector<int64_t> blocks, cols;
        ix_->SeqPosToColumn(seqs, pos, blocks, cols);
        std::vector<std::vector<int64_t>> cuts(il_->size());
        for (size_t q = 0; q + 1 < blocks.size(); q += 2)
            if (blocks[q] >= 0 && blocks[q] == blocks[q + 1]) cuts[(size_t)blocks[q]].push_back(std::max(cols[q], cols[q + 1]));
        std::vector<ColumnRange> out;
        for (size_t i = 0; i < il_->size(); i++) {
            std::vector<int64_t> &c = cuts[i];
            std::sort(c.begin(), c.end());
            c.erase(std::unique(c.begin(), c.end()), c.end());
            int64_t at = 0;
            const int64_t n = (int64_t)(*il_)[i].AlignmentLength();
            for (int64_t x : c) { if (x > at) out.push_back(ColumnRange{(int64_t)i, at, x - at}); at = std::max(at, x); }
            out.push_back(ColumnRange{(int64_t)i, at, n - at});
        }
        return out;
    }
private:
    struct Names {
        std::vector<std::string> f, d;
        std::vector<const char *> file, defline;
        Names(const IntervalList &il, uint N) : f(N), d(N), file(N), defline(N)
        {
            for (uint g = 0; g < N; g++) {
                f[g] = g < il.seq_filename.size() ? il.seq_filename[g] : std::string();
                d[g] = g < il.defline_name.size() && !il.defline_name[g].empty() ? il.defline_name[g] : f[g];
            }
            for (uint g = 0; g < N; g++) { file[g] = f[g].c_str(); defline[g] = d[g].c_str(); }
        }
    };
    void make(const mauve_text_params &p, const char *const *names, const char *const *deflines, const int64_t *n_contigs, const int64_t *starts,
              const char *const *contig_names, const std::vector<ColumnRange> *ranges) const
    {
        HipContext &hc = ix_->context();
        n_bytes_ = 0;
        if (ranges) {
            std::vector<int64_t> b(ranges->size() + 1), c(ranges->size() + 1), l(ranges->size() + 1);
            for (size_t r = 0; r < ranges->size(); r++) { b[r] = (*ranges)[r].block; c[r] = (*ranges)[r].col; l[r] = (*ranges)[r].len; }
            hc.check(mauve_alignment_text(hc.get(), &p, names, deflines, n_contigs, starts, contig_names, (int64_t)ranges->size(), b.data(), c.data(), l.data(), &n_bytes_, nullptr),
                     "mauve_alignment_text");
        } else
            hc.check(mauve_alignment_text(hc.get(), &p, names, deflines, n_contigs, starts, contig_names, 0, nullptr, nullptr, nullptr, &n_bytes_, nullptr), "mauve_alignment_text");
    }
    // the text in force into os, 8 MiB at a time
    void stream(std::ostream &os, const std::vector<ColumnRange> *ranges, std::vector<int64_t> *block_off) const
    {
        HipContext &hc = ix_->context();
        if (block_off) {
            int64_t n_range = ranges ? (int64_t)ranges->size() : 0;
            if (!ranges) hc.check(mauve_coord_index_size(hc.get(), nullptr, &n_range, nullptr), "mauve_coord_index_size");
            block_off->assign((size_t)n_range + 1, 0);
            hc.check(mauve_alignment_text_fetch(hc.get(), 0, 0, nullptr, block_off->data()), "mauve_alignment_text_fetch");
        }
        const int64_t piece = (int64_t)8 << 20;
        std::vector<char> buf((size_t)std::min(piece, std::max<int64_t>(n_bytes_, 1)));
        for (int64_t o = 0; o < n_bytes_; o += piece) {
            const int64_t n = std::min(piece, n_bytes_ - o);
            hc.check(mauve_alignment_text_fetch(hc.get(), o, n, buf.data(), nullptr), "mauve_alignment_text_fetch");
            os.write(buf.data(), (std::streamsize)n);
        }
    }
    const HipCoordinateIndex *ix_;
    const IntervalList *il_;
    mutable int64_t n_bytes_ = 0;
};

}  // namespace mems
#endif
