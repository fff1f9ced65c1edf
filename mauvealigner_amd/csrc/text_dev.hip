// text_dev.hip -- the alignment as XMFA or MAF text: lay the text out, fill it, hand out slices.  The stage stands in for
// IntervalList::WriteStandardAlignment (mauveAligner.cpp:746-760, per-LCB files :764-781) and for the writing half of xmfa2maf
// (xmfa2maf.cpp:46-82), which walk every column of every row on one host thread.  It reads the coordinate index in force (S14,
// coord_index.hpp) and the resident genomes; a cell is the S15 cell (extract_cells.hpp), the letter mauve_write_xmfa prints.
// A block is a column range; it owns N + 2 slots of the text: what stands in front of its rows (MAF "a\n"), one slot per genome (the row's
// header and body, empty when the genome has no residue in the range), what stands behind them (XMFA "=\n", MAF "\n").
//   tx_rows     a thread per (range, genome): the ranks in front of the range's first column and behind its last one give the row's extent;
//               MAF: the contig that holds it (a row across a join is reported); the bytes of its header and of its body
//   tx_blocks   a thread per range: does it have a row (a block without one is left out whole), the count of those that have
//   scan        of the slot bytes (dev_scan.hpp): slot offsets, the total
//   tx_head     a thread per slot: the row headers, decimal numbers written here, the block marks; block_off
//   tx_body     a thread per 16 aligned bytes of the text: the parts of row bodies in them -- one rank at the first column, the presence
//               bits of the one or two 64-column words, the bases of the one or two packed words -- a whole piece leaves as one store
// Every index formed from caller data is checked before it is used (ex_front); the kernels report through the flag word of coord_index.hpp
// and two words behind it (the first row across a contig join, the blocks with rows).
#include "common.hpp"
#include "extract_cells.hpp"
#include <algorithm>
#include <cstring>

namespace {

struct ExLen { const int64_t *v; static ExLen of(const int64_t *, const int64_t *cl) { return ExLen{cl}; } __device__ int64_t value(uint32_t i) const { return v[i]; } };

// a row of a block: its extent, the name it prints (genome, or contig of the whole table), header bytes, header + body bytes (0: no row)
struct alignas(32) TxRow { int64_t lo, hi, bytes; int32_t hlen, name; };

// the tables of a call (device pointers into the work area) and its format
struct TxTab {
    const int32_t *name_off;                      // [n_name + 1] into name_chr
    const char *name_chr;
    const int64_t *cstart;                        // MAF: 0-based contig starts, genome after genome
    int32_t coff[MAUVE_MAX_SEQ + 1];              // MAF: first contig of genome g in cstart / the names
    int maf;
    int64_t wrap, H;                              // XMFA: letters per line; the bytes of the text's header
};

__device__ __forceinline__ int tx_digits(int64_t v) { int d = 1; while (v >= 10) { v /= 10; d++; } return d; }
// v in decimal at p, d = tx_digits(v)
__device__ __forceinline__ char *tx_put(char *p, int64_t v, int d) { for (int k = d - 1; k >= 0; k--) { p[k] = (char)('0' + v % 10); v /= 10; } return p + d; }

// MAF: the numbers of a row in contig m of its genome (contig [cs, ce) 0-based)
__device__ __forceinline__ void tx_maf(const TxRow &w, bool rev, int64_t cs, int64_t ce, int64_t *start, int64_t *size, int64_t *src)
{
    const int64_t lo_local = w.lo - cs;
    *size = w.hi - w.lo + 1; *src = ce - cs;
    *start = rev ? *src - lo_local - *size + 1 : lo_local - 1;
}

__global__ void __launch_bounds__(256) tx_rows(CoordDev D, ExGenomes G, TxTab T, int64_t R, const int64_t *__restrict__ r_iv, const int64_t *__restrict__ gstart,
                                               const int64_t *__restrict__ clen, TxRow *__restrict__ rows, uint32_t *__restrict__ flag)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= R * D.N) return;
    const int64_t r = t / D.N; const int g = (int)(t - r * D.N);
    const int64_t i = r_iv ? r_iv[r] : r, x = gstart[r], l = clen[r];
    TxRow o; o.lo = o.hi = o.bytes = 0; o.hlen = 0; o.name = g;
    CoordIv I; bool pr; int64_t k0 = 0, k1 = 0;
    if (l > 0 && co_column(D, i, x, g, &I, &pr, &k0)) {
        (void)co_column(D, i, x + l, g, &I, &pr, &k1);          // (x + l <= n_cols: the index keeps the block that holds column n_cols)
        if (k1 > k0) {
            const bool rev = I.col0_rev & 1;
            o.lo = rev ? I.right - k1 + 1 : I.left + k0; o.hi = rev ? I.right - k0 : I.left + k1 - 1;
            if (k0 < 0 || o.lo < 1 || o.hi > G.len[g]) atomicOr(flag, CO_BAD_INDEX);
            else if (!T.maf) {
                o.hlen = 8 + tx_digits(g + 1) + tx_digits(o.lo) + tx_digits(o.hi) + (T.name_off[g + 1] - T.name_off[g]);
                o.bytes = o.hlen + l + (l + T.wrap - 1) / T.wrap;
            } else {
                int32_t a = T.coff[g], e = T.coff[g + 1];
                while (e - a > 1) { const int32_t mid = (a + e) >> 1; if (T.cstart[mid] <= o.lo - 1) a = mid; else e = mid; }
                const int64_t cs = T.cstart[a], ce = a + 1 < T.coff[g + 1] ? T.cstart[a + 1] : G.len[g];
                if (o.hi > ce) atomicMax(flag + 2, 0xFFFFFFFFu - (uint32_t)t);       // the first row across a join, for the message
                else {
                    int64_t start, size, src;
                    tx_maf(o, rev, cs, ce, &start, &size, &src);
                    o.name = a;
                    o.hlen = 8 + (T.name_off[a + 1] - T.name_off[a]) + tx_digits(start) + tx_digits(size) + tx_digits(src);
                    o.bytes = o.hlen + l + 1;
                }
            }
        }
    }
    rows[t] = o;
}

__global__ void __launch_bounds__(256) tx_blocks(int N, int64_t R, const TxRow *__restrict__ rows, uint32_t *__restrict__ has, uint32_t *__restrict__ flag)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool h = false;
    if (r < R) {
        for (int g = 0; g < N; g++) h |= rows[r * N + g].bytes != 0;
        has[r] = h;
    }
    const uint64_t B = __ballot(h);
    if ((threadIdx.x & 63) == 0 && B) atomicAdd(flag + 4, (uint32_t)__popcll(B));
}

// the bytes of slot i (block i / (N + 2))
struct TxSlot {
    const TxRow *rows; const uint32_t *has; uint32_t N; int pre, suf;
    __device__ int64_t value(uint32_t i) const
    {
        const uint32_t r = i / (N + 2), s = i - r * (N + 2);
        if (s == 0) return has[r] ? pre : 0;
        if (s == N + 1) return has[r] ? suf : 0;
        return rows[(size_t)r * N + (s - 1)].bytes;
    }
};

__global__ void __launch_bounds__(256) tx_head(CoordDev D, ExGenomes G, TxTab T, int64_t R, int64_t n_slot, const int64_t *__restrict__ r_iv, const TxRow *__restrict__ rows,
                                               const uint32_t *__restrict__ has, const int64_t *__restrict__ slot_off, char *__restrict__ text, int64_t *__restrict__ boff)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t S = (uint32_t)D.N + 2;
    if (t <= R) boff[t] = T.H + slot_off[t * S];
    if (t >= n_slot) return;
    const uint32_t r = (uint32_t)t / S, s = (uint32_t)t - r * S;
    char *p = text + T.H + slot_off[t];
    if (s == 0 || s == S - 1) {
        if (!has[r]) return;
        if (T.maf) { if (s == 0) { p[0] = 'a'; p[1] = '\n'; } else p[0] = '\n'; }
        else if (s) { p[0] = '='; p[1] = '\n'; }
        return;
    }
    const int g = (int)s - 1;
    const TxRow w = rows[(size_t)r * D.N + g];
    if (!w.bytes) return;
    const int64_t i = r_iv ? r_iv[r] : r;
    const bool rev = D.ivt[(size_t)i * D.N + g].col0_rev & 1;
    const char *nm = T.name_chr + T.name_off[w.name]; const int nl = T.name_off[w.name + 1] - T.name_off[w.name];
    if (!T.maf) {
        *p++ = '>'; *p++ = ' ';
        p = tx_put(p, g + 1, tx_digits(g + 1)); *p++ = ':';
        p = tx_put(p, w.lo, tx_digits(w.lo)); *p++ = '-';
        p = tx_put(p, w.hi, tx_digits(w.hi)); *p++ = ' ';
        *p++ = rev ? '-' : '+'; *p++ = ' ';
        for (int k = 0; k < nl; k++) *p++ = nm[k];
        *p++ = '\n';
    } else {
        const int64_t cs = T.cstart[w.name], ce = w.name + 1 < T.coff[g + 1] ? T.cstart[w.name + 1] : G.len[g];
        int64_t start, size, src;
        tx_maf(w, rev, cs, ce, &start, &size, &src);
        *p++ = 's'; *p++ = ' ';
        for (int k = 0; k < nl; k++) *p++ = nm[k];
        *p++ = ' '; p = tx_put(p, start, tx_digits(start));
        *p++ = ' '; p = tx_put(p, size, tx_digits(size));
        *p++ = ' '; *p++ = rev ? '-' : '+';
        *p++ = ' '; p = tx_put(p, src, tx_digits(src));
        *p++ = ' ';
    }
}

// the last slot that starts at or before text byte P (slots in front of it that are empty share a start); a: a slot known to
__device__ __forceinline__ int64_t tx_slot_of(const int64_t *__restrict__ slot_off, int64_t a, int64_t n_slot, int64_t P)
{
    int64_t e = n_slot;
    while (e - a > 1) { const int64_t mid = (a + e) >> 1; if (slot_off[mid] <= P) a = mid; else e = mid; }
    return a;
}

// thread = the 16 text bytes [16 t, 16 t + 16); a wave = 1024 consecutive bytes
__global__ void __launch_bounds__(256) tx_body(CoordDev D, ExGenomes G, TxTab T, int64_t n_slot, int64_t n_bytes, const int64_t *__restrict__ r_iv,
                                               const int64_t *__restrict__ gstart, const int64_t *__restrict__ clen, const TxRow *__restrict__ rows,
                                               const int64_t *__restrict__ slot_off, char *__restrict__ text, uint32_t *__restrict__ flag)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t P0 = t * 16 - T.H, Pw = (t & ~(int64_t)63) * 16 - T.H;           // relative to the first slot, as slot_off is
    if (P0 + T.H >= n_bytes) return;
    const uint32_t S = (uint32_t)D.N + 2;
    // piece -> slot: once for the wave where it stays inside one slot
    int64_t s = tx_slot_of(slot_off, 0, n_slot, Pw);
    if (slot_off[s + 1] < Pw + 1024) s = tx_slot_of(slot_off, s, n_slot, P0);
    uint32_t bad = 0;
    for (; s < n_slot && slot_off[s] < P0 + 16; s++) {
        const uint32_t r = (uint32_t)s / S, sl = (uint32_t)s - r * S;
        if (sl == 0 || sl == S - 1) continue;
        const int g = (int)sl - 1;
        const TxRow w = rows[(size_t)r * D.N + g];
        if (!w.bytes) continue;
        const int64_t body0 = slot_off[s] + w.hlen, body1 = slot_off[s] + w.bytes;
        const int64_t a = body0 > P0 ? body0 : P0, b = body1 < P0 + 16 ? body1 : P0 + 16;
        if (a >= b) continue;
        const int ia = (int)(a - P0), ib = (int)(b - P0);
        const int64_t l = clen[r], W = T.maf ? l : T.wrap, q0 = a - body0;
        const int64_t line = q0 / (W + 1);
        int64_t rem = q0 - line * (W + 1), j = line * W + rem;                      // j: the next column at or behind byte q0 (rem == W: a newline first)
        // the presence bits of up to 16 columns from j on, the rank in front of the first
        const int n = (int)(l - j < 16 ? l - j : 16);
        uint32_t pm = 0, codes = 0, am = 0; int cnt = 0; bool rev = false;
        if (n > 0) {
            const int64_t i = r_iv ? r_iv[r] : r, x0 = gstart[r] + j, blk = x0 / CO_BLOCK;
            const int off = (int)(x0 - blk * CO_BLOCK), wi = off >> 6, bit = off & 63;
            const CoordIv I = D.ivt[(size_t)i * D.N + g];
            const CoordRec rec = D.rec[(size_t)blk * D.N + g];
            bool pr;
            const int64_t k = co_rank(rec, off, &pr) - I.base;
            uint64_t cur = 0, nxt = 0;
#pragma unroll
            for (int q = 0; q < CO_WORDS; q++) { if (q == wi) cur = rec.w[q]; if (q == wi + 1) nxt = rec.w[q]; }
            uint64_t m = cur >> bit;
            if (n > 64 - bit) {                                                     // (then bit > 48; the columns exist, so does the next record)
                if (wi == CO_WORDS - 1) nxt = D.rec[(size_t)(blk + 1) * D.N + g].w[0];
                m |= nxt << (64 - bit);
            }
            pm = (uint32_t)m & (0xFFFFu >> (16 - n));
            cnt = __popc(pm);
            rev = I.col0_rev & 1;
            // residue k sits at left + k, at right - k on the reverse strand: cnt consecutive bases, the lowest at 0-based ql
            const int64_t ql = rev ? I.right - k - cnt : I.left + k - 1;
            if (cnt && (k < 0 || ql < 0 || ql + cnt > G.len[g])) { bad |= CO_BAD_INDEX; pm = 0; cnt = 0; }
            if (cnt) {
                const uint64_t *gw = G.words + G.word_off[g] + (uint64_t)(ql >> 5);
                const int sh = 2 * (int)(ql & 31);
                uint64_t c2 = gw[0] >> sh;
                if ((int)(ql & 31) + cnt > 32) c2 |= gw[1] << (64 - sh);
                codes = (uint32_t)c2;
                if (G.inv) {
                    const uint64_t *iw = G.inv + G.mask_off[g] + (uint64_t)(ql >> 6);
                    const int sa = (int)(ql & 63);
                    uint64_t a2 = iw[0] >> sa;
                    if (sa + cnt > 64) a2 |= iw[1] << (64 - sa);
                    am = (uint32_t)a2;
                }
            }
        }
        uint32_t v[4] = {0, 0, 0, 0};
        int seen = 0;
#pragma unroll
        for (int by = 0; by < 16; by++) {
            if (by < ia || by >= ib) continue;
            char ch;
            if (rem == W || j == l) { ch = '\n'; rem = 0; }
            else {
                ch = '-';
                if (pm & 1) {
                    const int idx = rev ? cnt - 1 - seen : seen;
                    const int code = (int)(codes >> (2 * idx) & 3);
                    ch = (char)(0x54474341u >> (8 * (rev ? 3 - code : code)));      // "ACGT"
                    if (am >> idx & 1) ch = 'N';
                    seen++;
                }
                pm >>= 1; j++; rem++;
            }
            v[by >> 2] |= (uint32_t)(uint8_t)ch << (8 * (by & 3));
        }
        char *dst = text + T.H + P0;
        if (ia == 0 && ib == 16) *reinterpret_cast<uint4 *>(dst) = make_uint4(v[0], v[1], v[2], v[3]);
        else {
#pragma unroll
            for (int by = 0; by < 16; by++) if (by >= ia && by < ib) dst[by] = (char)(v[by >> 2] >> (8 * (by & 3)));
        }
    }
    if (bad) atomicOr(flag, bad);
}

const char *tx_str(const char *const *a, int g) { return a && a[g] ? a[g] : ""; }

}  // namespace

extern "C" {

void mauve_default_text_params(int format, mauve_text_params *p)
{
    if (!p) return;
    p->format = format; p->wrap = format == MAUVE_TEXT_MAF ? 0 : 80;
}

int mauve_alignment_text(mauve_ctx *c, const mauve_text_params *p, const char *const *names, const char *const *deflines, const int64_t *n_contigs,
                         const int64_t *contig_starts, const char *const *contig_names, int64_t n_range, const int64_t *range_iv, const int64_t *range_col,
                         const int64_t *range_len, int64_t *n_bytes, int64_t *n_blocks)
{
    if (!c) return MAUVE_ERR_ARG;
    c->tx.valid = false;
    if (const int rs = ex_check_state(c, "alignment_text")) return rs;
    if (!p || (p->format != MAUVE_TEXT_XMFA && p->format != MAUVE_TEXT_MAF)) { c->err = "alignment_text: format must be MAUVE_TEXT_XMFA or MAUVE_TEXT_MAF"; return MAUVE_ERR_ARG; }
    const bool maf = p->format == MAUVE_TEXT_MAF;
    if (!maf && p->wrap < 1) { c->err = "alignment_text: wrap must be at least 1 for XMFA"; return MAUVE_ERR_ARG; }
    if (maf && p->wrap != 0) { c->err = "alignment_text: wrap must be 0 for MAF (a row is one line)"; return MAUVE_ERR_ARG; }
    if (!maf && (n_contigs || contig_starts || contig_names)) { c->err = "alignment_text: a contig table goes with MAF only"; return MAUVE_ERR_ARG; }
    if (maf && (!n_contigs != !contig_starts || (contig_names && !n_contigs))) { c->err = "alignment_text: n_contigs and contig_starts go together, contig_names with them"; return MAUVE_ERR_ARG; }
    const int N = c->nseq;
    // the text's header, the names the rows print, the contig table: one block behind the ranges
    std::string head, chr;
    std::vector<int32_t> name_off(1, 0);
    std::vector<int64_t> cstart;
    TxTab T; memset(&T, 0, sizeof T);
    T.maf = maf; T.wrap = maf ? 0 : p->wrap;
    if (!maf) {
        head = "#FormatVersion Mauve1\n";
        for (int g = 0; g < N; g++) {
            const std::string n1 = std::to_string(g + 1);
            head += "#Sequence" + n1 + "File\t" + tx_str(names, g) + "\n#Sequence" + n1 + "Entry\t" + n1 + "\n#Sequence" + n1 + "Format\tFastA\n";
            chr += tx_str(deflines ? deflines : names, g);
            name_off.push_back((int32_t)chr.size());
        }
    } else {
        head = "##maf version=1 program=progressiveMauve\n";
        int64_t at = 0;
        for (int g = 0; g < N; g++) {
            const int64_t nc = n_contigs ? n_contigs[g] : 1;
            if (nc < 1 || at + nc > ((int64_t)1 << 24)) { c->err = "alignment_text: genome " + std::to_string(g) + " has no contig, or the table holds more than 2^24"; return nc < 1 ? MAUVE_ERR_ARG : MAUVE_ERR_LIMIT; }
            T.coff[g] = (int32_t)at;
            for (int64_t k = 0; k < nc; k++) {
                const int64_t s = n_contigs ? contig_starts[at + k] : 0;
                if (k == 0 ? s != 0 : (s <= cstart.back() || s >= c->lens[(size_t)g])) {
                    c->err = "alignment_text: the contig starts of genome " + std::to_string(g) + " do not ascend from 0 inside the genome"; return MAUVE_ERR_ARG;
                }
                cstart.push_back(s);
                chr += tx_str(names, g);
                if (contig_names) { chr += '.'; chr += tx_str(contig_names, (int)(at + k)); }
                name_off.push_back((int32_t)chr.size());
            }
            at += nc;
        }
        T.coff[N] = (int32_t)at;
    }
    if (chr.size() >= ((size_t)1 << 30)) { c->err = "alignment_text: the names hold 2^30 bytes or more"; return MAUVE_ERR_LIMIT; }
    T.H = (int64_t)head.size();
    const size_t t_cs = 0, t_no = t_cs + up64(cstart.size() * 8), t_ch = t_no + up64(name_off.size() * 4), t_hd = t_ch + up64(chr.size()), t_total = t_hd + up64(head.size());
    std::vector<char> tail(t_total, 0);
    if (!cstart.empty()) memcpy(tail.data() + t_cs, cstart.data(), cstart.size() * 8);
    memcpy(tail.data() + t_no, name_off.data(), name_off.size() * 4);
    if (!chr.empty()) memcpy(tail.data() + t_ch, chr.data(), chr.size());
    memcpy(tail.data() + t_hd, head.data(), head.size());
    ExFront F;
    if (const int rf = ex_front<ExLen>(c, "alignment_text", c->tx_work, n_range, range_iv, range_col, range_len, tail.data(), t_total, &F)) return rf;
    const int64_t R = F.R, S = N + 2, n_slot = R * S;
    if (n_slot >= ((int64_t)1 << 31)) { c->err = "alignment_text: ranges x (genomes + 2) reach 2^31"; return MAUVE_ERR_LIMIT; }
    T.cstart = reinterpret_cast<const int64_t *>(F.tail + t_cs); T.name_off = reinterpret_cast<const int32_t *>(F.tail + t_no); T.name_chr = F.tail + t_ch;
    const CoordDev &D = *c->co.dev;
    const size_t nR = (size_t)R, nS = (size_t)n_slot;
    // rows | has | slot_off | tile sums
    const uint32_t tiles = (uint32_t)((nS + devscan::TILE - 1) / devscan::TILE);
    const size_t a_has = up64(nR * (size_t)N * sizeof(TxRow)), a_off = a_has + up64(nR * 4), a_bs = a_off + up64((nS + 1) * 8), a_total = a_bs + up64((size_t)tiles * 8 + 8);
    HIPCHK(c, c->tx_rows.ensure(a_total));
    HIPCHK(c, c->tx_boff.ensure((nR + 1) * 8));
    char *ab = c->tx_rows.as<char>();
    TxRow *rows = reinterpret_cast<TxRow *>(ab);
    uint32_t *has = reinterpret_cast<uint32_t *>(ab + a_has);
    int64_t *slot_off = reinterpret_cast<int64_t *>(ab + a_off), *bsum = reinterpret_cast<int64_t *>(ab + a_bs);
    char *hb = c->pin_stage.as<char>();                      // (ex_front left it at least 256 bytes long)
    int64_t total = 0, nblk = 0;
    if (R) {
        hipLaunchKernelGGL(tx_rows, dim3((uint32_t)((nR * (size_t)N + 255) / 256)), dim3(256), 0, c->stream, D, F.G, T, R, F.d_iv, F.gstart, F.clen, rows, F.flag);
        hipLaunchKernelGGL(tx_blocks, dim3((uint32_t)((nR + 255) / 256)), dim3(256), 0, c->stream, N, R, rows, has, F.flag);
        const TxSlot in{rows, has, (uint32_t)N, maf ? 2 : 0, maf ? 1 : 2};
        hipLaunchKernelGGL((devscan::vscan_partial<int64_t, TxSlot>), dim3(tiles), dim3(256), 0, c->stream, in, (uint32_t)n_slot, bsum);
        hipLaunchKernelGGL((devscan::vscan_write<int64_t, TxSlot>), dim3(tiles), dim3(256), 0, c->stream, in, (uint32_t)n_slot, bsum, slot_off, (int64_t *)nullptr);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(hb, F.flag, 32, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(hb + 64, slot_off + n_slot, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const uint32_t *fw = reinterpret_cast<const uint32_t *>(hb);
        if (const int rf = co_flag_result(c, fw[0], "alignment_text", EX_OUTSIDE)) return rf;
        if (fw[2]) {
            const int64_t t = (int64_t)(0xFFFFFFFFu - fw[2]);
            c->err = "alignment_text: range " + std::to_string(t / N) + ", genome " + std::to_string(t % N) + ": the row crosses a contig join (MAF rows lie in one contig: split the range at the join)";
            return MAUVE_ERR_ARG;
        }
        total = *reinterpret_cast<const int64_t *>(hb + 64); nblk = fw[4];
    } else HIPCHK(c, hipMemsetAsync(slot_off, 0, 8, c->stream));
    const int64_t nb = T.H + total;
    HIPCHK(c, c->tx_text.ensure((size_t)nb + 16));
    char *text = c->tx_text.as<char>();
    HIPCHK(c, hipMemcpyAsync(text, F.tail + t_hd, head.size(), hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL(tx_head, dim3((uint32_t)((std::max(nS, nR + 1) + 255) / 256)), dim3(256), 0, c->stream, D, F.G, T, R, n_slot, F.d_iv, rows, has, slot_off, text, c->tx_boff.as<int64_t>());
    if (total)
        hipLaunchKernelGGL(tx_body, dim3((uint32_t)(((nb + 15) / 16 + 255) / 256)), dim3(256), 0, c->stream, D, F.G, T, n_slot, nb, F.d_iv, F.gstart, F.clen, rows, slot_off, text, F.flag);
    HIPCHK(c, hipGetLastError());
    if (const int rf = co_flag_read(c, F.flag, "alignment_text", EX_OUTSIDE)) return rf;
    c->tx.valid = true; c->tx.genome_gen = c->genome_gen; c->tx.n_bytes = nb; c->tx.n_range = R; c->tx.n_blocks = nblk;
    if (n_bytes) *n_bytes = nb;
    if (n_blocks) *n_blocks = nblk;
    return MAUVE_OK;
}

int mauve_alignment_text_fetch(mauve_ctx *c, int64_t offset, int64_t len, char *buf, int64_t *block_off)
{
    if (!c) return MAUVE_ERR_ARG;
    const mauve_ctx::AlignText &X = c->tx;
    if (!X.valid || X.genome_gen != c->genome_gen) { c->err = "alignment_text_fetch: no text in force (mauve_alignment_text first; an index call or a genome upload ends it)"; return MAUVE_ERR_STATE; }
    if (const int rs = ex_check_state(c, "alignment_text_fetch")) return rs;
    if (offset < 0 || len < 0 || offset > X.n_bytes || len > X.n_bytes - offset) { c->err = "alignment_text_fetch: the slice lies outside the text of " + std::to_string(X.n_bytes) + " bytes"; return MAUVE_ERR_ARG; }
    if (len && !buf) { c->err = "alignment_text_fetch: no buffer for the slice"; return MAUVE_ERR_ARG; }
    HIPCHK(c, hipSetDevice(c->device));
    if (len) if (const int rc = copy_to_caller(c, c->pin_stage, buf, c->tx_text.as<char>() + offset, (size_t)len)) return rc;
    if (block_off) if (const int rc = copy_to_caller(c, c->pin_stage, block_off, c->tx_boff.p, ((size_t)X.n_range + 1) * 8)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MAUVE_OK;
}

}  // extern "C"
