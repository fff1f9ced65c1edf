// common.hpp -- internal declarations shared by the translation units of libmauve_hip.so.
// Product code: must never include anything from oracle/.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include <functional>
#include "switches.hpp"
#include "workers.hpp"
#include "host_chain.hpp"
#include "backbone_host.hpp"
#include <chrono>
#include <algorithm>
#include <cstring>

#include "../../include/mauve_hip.h"

#define HIPCHK(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e__ = (call);                                                                  \
        if (e__ != hipSuccess) {                                                                  \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__) + " (" __FILE__ ":" + \
                         std::to_string(__LINE__) + ")";                                          \
            return MAUVE_ERR_HIP;                                                                 \
        }                                                                                         \
    } while (0)

inline size_t up64(size_t x) { return (x + 63) & ~(size_t)63; }       // the next multiple of 64: parts of a work area start on one

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = bytes + bytes / 8 + 4096;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    // grow keeping the first `used` bytes (the stream is drained first: work queued on it may still read the old block)
    hipError_t ensure_keep(size_t bytes, size_t used, hipStream_t stream)
    {
        if (bytes <= cap) return hipSuccess;
        void *np = nullptr;
        const size_t want = bytes + bytes / 2 + 4096;
        hipError_t e = hipMalloc(&np, want);
        if (e != hipSuccess) return e;
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) { (void)hipFree(np); return e; }
        if (p && used && (e = hipMemcpy(np, p, used, hipMemcpyDeviceToDevice)) != hipSuccess) { (void)hipFree(np); return e; }
        if (p) (void)hipFree(p);
        p = np; cap = want;
        return hipSuccess;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// Page-locked host buffer: the destination of the larger device-to-host copies (a pageable destination goes
// through the runtime's staging buffers at a fraction of the link rate).  Grows, never shrinks; owned by the ctx.
struct PinnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipHostFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = bytes + bytes / 8 + 4096;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// Seed pattern decomposed into runs of contiguous care positions (kernel argument, by value).
// K' ("digit-reversed forward mer"): care offset t_j contributes code << 2j, so that
//   reverse-complement mer = ~K' (masked) and forward mer = digit_reverse(K').
// Run i (care offsets t0 .. t0 + len - 1, the digits j .. j + len - 1 of K') lies 2 * (t0 - j) bits above its place in K': K' is the OR over
// the runs of (window >> shift) under the run's mask in place.  The tables are whole 32-bit words, so that the scalar unit loads them once per
// kernel (seed_dev.hpp: SeedRuns; byte-wide members cost a vector load each, gfx950 has no scalar byte load); entries behind nruns are zero
// and contribute nothing.
constexpr int SEED_RUN_GROUP = 4;                                  // the run loops leave after a whole group of runs
constexpr int SEED_RUNS_NARROW = 16;                               // a span of 32 holds no more runs
constexpr int SEED_RUNS_MAX = ((MAUVE_MAX_SEED_SPAN + 1) / 2 + SEED_RUN_GROUP - 1) / SEED_RUN_GROUP * SEED_RUN_GROUP;
struct SeedShape {
    int span, weight, nruns;
    uint64_t keymask;          // (1 << 2*weight) - 1
    uint32_t run_shift[SEED_RUNS_NARROW];   // one-word windows (seed_narrow): shift, and
    uint32_t run_mask[SEED_RUNS_NARROW];    // ... the mask in place; both zero for any other seed
    uint32_t run_wide[SEED_RUNS_MAX];       // every seed: shift | bit offset in K' << 8 | 2 * run length << 16 (the 64-bit mask is made from the two)
    uint64_t care_lo, care_hi; // 2-bit-expanded care mask of the window (offset t -> bits 2t, 2t+1)
};

// The genomes as the kernels see them: one packed buffer, windows numbered globally.
struct GenomeTab {
    int nseq;
    uint32_t gpos_off[MAUVE_MAX_SEQ + 1];   // first global window index of genome g
    uint32_t nwin[MAUVE_MAX_SEQ];           // valid window starts of genome g
    uint64_t word_off[MAUVE_MAX_SEQ];       // first 64-bit word of genome g in the packed buffer
    uint64_t mask_off[MAUVE_MAX_SEQ];       // first 64-bit word of genome g in the placed-base bitmap (S9), if any
};

// A set of packed genomes resident on the device (the main genomes, or the gap sub-sequences of one
// recursive-anchoring level).
struct GenomeSet {
    DevBuf *buf = nullptr;
    int nseq = 0;
    std::vector<int64_t> lens;
    std::vector<uint64_t> word_off;
    // guide-tree recursive anchoring: 1 bit per base, set = already placed by an ancestor node;
    // windows touching a set bit are invalid for seeding and extension.  nullptr = no mask.
    DevBuf *vmask = nullptr;
    // contig starts (mauve_set_genomes_contigs): 1 bit per base, set = a contig begins here; a window may not run
    // across such a base.  Same word layout as vmask (mask_off).  nullptr = single-contig sequences.
    DevBuf *cmask = nullptr;
    std::vector<uint64_t> mask_off;
};

// seed hits handed in by a host-side finder: n records of (1 + nseq) words {component set, value of every genome}
struct HostHits { uint32_t n; const uint32_t *rec; };

// SeedMatchEnumerator on the device: rule in, CSR result out (mult / start_off / starts may be null: counts only)
struct EnumRequest { int64_t min_multi, max_multi; int direct_only; int64_t n, ns; int64_t *mult, *start_off, *starts; };

// What one seed pass is asked to do; the entry points of seed_pass.hip fill it.
struct SeedRequest {
    int mode = MAUVE_MODE_MEM;
    uint64_t mask = 0;
    int extend = 0;
    int only_seq = -1;                           // >= 0: the sorted mer list of that genome alone (the two exports)
    const uint32_t *seg = nullptr;               // segmented set (recursive anchoring): device array [nseq][nseg + 1] of segment starts
    uint32_t nseg = 0;
    const HostHits *hits = nullptr;              // mauve_extend_hits: the hits come from the host, no sort, no join
    EnumRequest *enumerate = nullptr;            // mauve_seed_match_enumerate: rule in, CSR result out
    std::vector<uint64_t> *out_keys = nullptr;   // sorted-mer-list export
    std::vector<uint32_t> *out_vals = nullptr;
    int64_t *n_matches = nullptr;
};

struct AlignResult {
    mauve_align_sizes sz{};
    std::vector<int64_t> mum_length, mum_start;
    std::vector<int64_t> lcb_left, lcb_right, lcb_weight;
    std::vector<int64_t> anchor_length, anchor_start, anchor_lcb;
    std::vector<int64_t> iv_left, iv_right;
    std::vector<int8_t> iv_reverse;
    std::vector<int64_t> col_off;
    std::vector<uint32_t> cols;        // capacity buffer: the first n_cols entries are the result (see pipeline.cpp)
    size_t n_cols = 0;
    uint32_t cols_fill = 0;            // value every word outside cols_dirty holds (0 = no such invariant)
    std::vector<std::pair<size_t, size_t>> cols_dirty;   // (offset, length) ranges holding gap columns
    std::vector<int64_t> dp_score;
    // device-assembled result (assemble_dev.hip): the columns (res_cols), the anchor table and maybe the match list are still in HBM
    bool stale = false;                     // the genomes were replaced after this result was made: a fetch is refused (mauve_set_genomes)
    bool genomes_replaced = false;          // ... also set when the result was wholly on the host already: it can still be fetched, but the calls that read
                                            // bases against it (mauve_apply_homology, mauve_write_xmfa) are refused -- they would pair the new genomes with the old alignment
    bool dev_pending = false;               // anchor table / match list still on the device
    bool cols_pending = false;              // columns only in res_cols (cols_ext not set)
    size_t dev_na = 0, dev_nm = 0;          // anchors; matches still on the device (0: mum_* are filled)
    const int32_t *dev_alen = nullptr, *dev_ast = nullptr, *dev_alcb = nullptr;     // ... where the anchors are (chain_order_device's arrays)
    const uint32_t *cols_ext = nullptr;      // the columns in page-locked staging after materialize_result (else: cols)
    // bulk tables that travelled while the pass ran (mauve_align_prefetch): the caller's buffers they are in, nullptr = not delivered; a fetch
    // that names the same buffers skips that table's copies (fetch_compact_direct), any fetch uses them up
    const int32_t *del_mum_length = nullptr, *del_mum_start = nullptr, *del_alen = nullptr, *del_ast = nullptr, *del_alcb = nullptr;
    const uint32_t *cols_data() const { return cols_ext ? cols_ext : cols.data(); }
};

// state of an alignment between its begin and finish phases (pipeline.cpp)
struct AlignState {
    typedef ::GapRef GapRef;
    struct Item { int64_t lcb; uint32_t idx; int64_t col0; int64_t gap; };
    bool open = false;
    bool anchor_table_done = false;     // anchor_length/start/lcb already filled (in the DP kernel's shadow)
    bool dev_tail = false;              // the chains stayed on the device: DP front end and assembly run there (mauve_align)
    const int32_t *dv_len = nullptr, *dv_st = nullptr, *dv_lcb = nullptr;   // ... where: anchors in chain order (chain_order_device, or the extended list)
    bool lw_from_host = false;          // the LCB weights of the result are those align_begin left in R.lcb_weight (device extension)
    int64_t mums_kept = -1;             // >= 0: the main pass's match list (that many records) sits in ctx->sorted_rec_keep while the recursion's passes use sorted_rec
    mauve_params p{};
    int N = 0; uint32_t full = 0;
    int64_t sum = 0, nm = 0, nl = 0, n_dp = 0, code_total = 0, n_anchor = 0, anchor_cols = 0;
    double t0 = 0, t_dp0 = 0;
    std::vector<MatchVec> chains;
    std::vector<GapRef> gaps;
    std::vector<DpSeqDesc> desc;
    std::vector<int64_t> dcol_off, dscore;       // DP columns of mauve_align land in ctx->pin_dcols
    // scratch of the host stages; like everything above it keeps its capacity from call to call -- a fresh
    // megabyte-sized vector per stage and call costs more in page faults than the stage itself
    MatchVec m;
    std::vector<int64_t> match_lcb;
    std::vector<int64_t> match_weight;  // sum-of-pairs scores of the matches (lcb_scoring = SP), else empty
    std::vector<Item> items;
    void count_anchors() { for (const MatchVec &ch : chains) { n_anchor += (int64_t)ch.size(); for (size_t i = 0; i < ch.size(); i++) anchor_cols += ch.len(i); } }
    // start a new alignment: scalars to zero, vectors emptied but not released
    void reset()
    {
        open = false; anchor_table_done = false; dev_tail = false; dv_len = dv_st = dv_lcb = nullptr; lw_from_host = false; mums_kept = -1; p = mauve_params(); N = 0; full = 0;
        sum = nm = nl = n_dp = code_total = n_anchor = anchor_cols = 0; t0 = t_dp0 = 0;
        gaps.clear(); desc.clear(); dcol_off.clear(); dscore.clear();
        match_lcb.clear(); match_weight.clear(); items.clear();
    }
};

struct CoordDev;                         // coord_dev.hip
struct mauve_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;           // the one-wave DP launch runs here when there are workgroup launches (those go first, on `stream`)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // third queue (with `stream` and `stream2`; the runtime opens four by default): copies that run beside the pass (the bulk tables of mauve_align_prefetch).  It starts behind ev_io_fork, recorded on `stream`,
    // and `stream` waits on ev_io_done before the pass's last synchronisation: when an entry point returns, nothing is in flight here.
    hipStream_t stream_io = nullptr;
    hipEvent_t ev_io_fork = nullptr, ev_io_done = nullptr;
    struct TablePrefetch {
        int32_t *mum_length = nullptr, *mum_start = nullptr, *anchor_length = nullptr, *anchor_start = nullptr, *anchor_lcb = nullptr;
        int64_t mum_cap = 0, anchor_cap = 0;           // records
        bool armed = false;                             // registered, the next mauve_align takes it
        bool live = false;                              // ... which is running
        bool inflight = false;                          // copies queued on stream_io that `stream` has not waited for yet
        bool got_mums = false, got_anchors = false;     // what they deliver
    } pf;
    DevBuf pf_mums;                      // the match list narrowed to int32 on its way out (as_wide belongs to the fetch)
    std::string err;
    char devname[256] = {0};
    int cus = 256;                       // compute units of the device (launches sized to a whole number of waves per SIMD)

    // genomes
    int nseq = 0;
    std::vector<int64_t> lens;
    std::vector<uint64_t> word_off;      // per genome, in 64-bit words
    std::vector<const uint64_t *> host_packed;   // host copy of every genome's packed words (XMFA text), inside pin_genomes
    PinnedBuf pin_genomes;
    PinnedBuf pin_tail;                  // direct upload from page-locked caller memory: the fixed-up tail words of every genome
    bool host_copy_valid = false;         // host_packed / pin_genomes hold the genomes (else: fetched back on demand, host_genomes)
    size_t total_words = 0;
    DevBuf genomes;
    // ambiguous bases and contig starts of the resident genomes (mauve_set_genomes_contigs): device bitmaps in the
    // layout of GenomeSet::vmask / cmask, their host copies (masks of the guide-tree nodes and of the LCB extension
    // are built on top of the first; the XMFA writer prints N where it is set)
    DevBuf base_invalid, contig_mask, node_cmask;
    bool has_invalid = false, has_contigs = false;
    std::vector<uint64_t> h_invalid, h_contig, base_mask_off;

    // seed-pass workspace
    DevBuf keysA, keysB, valsA, valsB, hist, totals, posmask, hit_mask, hit_pos, hit_seg, cand, mlen, mstart, counters;
    DevBuf sorted_rec;                   // canonical order on the device: gathered (length, starts) records as int64
    DevBuf canon_k1, canon_k2, canon_v1, canon_v2;   // ... and its (key, candidate index) sort buffers
    DevBuf join_bound;                   // join_hash: first bucket boundary at or after every chunk edge
    DevBuf join_ovf;                     // join_hash: [count, pad, (lo, hi) ...] ranges handed back to the full sort + serial join
    DevBuf ch_len, ch_st, ch_crop, ch_ent, ch_ord, ch_rank, ch_node, ch_graph, ch_cnt;   // device chain (chain_dev.hip)
    DevBuf gap_work;                     // recursion batches: collinear rule and survivor compaction on the device (chain_device_gaps_compact)
    DevBuf ch_big;                       // working arrays of overlap clusters beyond the per-thread limit (recursion batches)
    DevBuf ch_anch, ch_lw;               // the chains in chain order and the LCB weights (chain_order_device)
    DevBuf ch_anch2, ext_work, sorted_rec_keep;   // device-resident LCB extension (extend_dev.hip): the extended anchor list, its work area, the main pass's match list set aside
    PinnedBuf pin_ext;
    DevBuf ch_mw;                        // sum-of-pairs scores of the chain's cropped records (score-weighted LCBs on the device chain)
    DevBuf as_wide;                      // the anchor table widened to int64 for a direct fetch (compact fetch: the match list narrowed to int32)
    DevBuf res_narrow;                   // the columns narrowed to 8 / 16 bits for a compact fetch
    DevBuf hom_cols;                     // homology pass (homology_dev.hip): the re-split columns, swapped with res_cols when done
    DevBuf as_work, as_isl, res_cols;    // device assembly (assemble_dev.hip): work area, islands, result columns
    PinnedBuf pin_tab;                   // anchor table and match list of a device-assembled result on their way to the host
    PinnedBuf pin_asm, pin_cols;         // ... its per-LCB rows coming back; the columns and anchors on their way to a fetch
    PinnedBuf pin_chain;
    PinnedBuf pin_mask;                  // LCB extension: the valid-piece bitmap on its way to placed_mask
    BackboneResult bb;                   // backbone / islands of the last alignment (backbone_dev.hip; the struct: backbone_host.hpp)
    PinnedBuf pin_bb;                    // rank queries and their answers
    DevBuf bb_cols, bb_work, bb_query;   // a caller's / a host-assembled column array; interval table + records; rank queries
    size_t bb_rec_cap = 0;
    // coordinate translation (coord_dev.hip): the rank/select index is a snapshot with buffers of its own -- it reads neither the
    // genomes nor res_cols once built, so later passes leave it alone; replaced by the next mauve_coord_index*, freed with the context
    struct CoordIndex { bool valid = false; int N = 0; int64_t n_iv = 0, n_cols = 0; uint64_t genome_gen = 0; struct ::CoordDev *dev = nullptr; } co;     // dev: the kernels' view of the index, owned by coord_dev.hip (coord_index_release)
    DevBuf co_index, co_q;               // the index; one chunk of queries and their answers
    // the staging of the stages that query the index (S14 to S17): queries, ranges and pairs on their way in, the error flag and counts coming
    // back, pageable results on their way out (copy_to_caller).  The stages do not run concurrently on a context and keep nothing here between
    // calls; the one thing that outlives a call, the selection of S15, is device memory (ex_sel below)
    PinnedBuf pin_stage;
    // scoring against a correct alignment (score_dev.hip): a second index, of the correct alignment, read-only beside the one in
    // force; replaced by the next mauve_score_truth, untouched by mauve_coord_index*, alignments and genome uploads
    CoordIndex co_truth;
    DevBuf co_truth_index, sc_out;       // that index; the error flag and the records
    // column extraction (extract_dev.hip): the selection a fetch turns into letters -- the selected columns as (interval, column)
    // in ex_sel, with the request; it belongs to the index and the genomes it was made on (an index call clears `valid`, genome_gen tells an upload)
    struct ExtractSel {
        bool valid = false; uint64_t genome_gen = 0;
        int64_t n_sel = 0, n_range = 0;
        int n_keep = 0; int32_t keep[MAUVE_MAX_SEQ] = {0};
    } ex;
    // alignment text (text_dev.hip): the XMFA or MAF text of the last mauve_alignment_text stays on the device for its fetches, with
    // block_off [n_range + 1]; it belongs to the index and the genomes it was made on (an index call clears `valid`, genome_gen tells an upload)
    struct AlignText { bool valid = false; uint64_t genome_gen = 0; int64_t n_bytes = 0, n_range = 0, n_blocks = 0; } tx;
    DevBuf tx_work, tx_rows, tx_text, tx_boff;  // the flag words, ranges and tables; row records, slot bytes and their scan; the text; block_off
    DevBuf ex_work, ex_bits, ex_sel, ex_mat;   // the flag word, ranges and their scan; selection words and their scan; sel_iv | sel_col | range_off; the matrix (padded pitch)
    // pairwise column statistics (pairstat_dev.hip): no state between calls, work buffers apart from the selection's
    DevBuf ps_work, ps_out;              // the flag word, ranges, their units' scan, the pair lists; the records
    // excursions of the column scores (excursion_dev.hip): the result of the last call stays for its fetches; it belongs to the
    // index and the genomes it was made on (an index call clears `valid`, genome_gen tells an upload)
    struct Excursions { bool valid = false; uint64_t genome_gen = 0; int64_t n_stream = 0, n_exc = 0; } exc;
    DevBuf exc_work, exc_tmp, exc_meta, exc_rec;   // the flag word, ranges, their chunks' scan, the sets; per-chunk arrays; stream_off | tail; height | end_col
    // projection onto a genome subset (project_dev.hip): the result of the last call -- columns and the work area their source columns are made from on the
    // device, the interval tables and the provenance on the host -- stays for its fetches and for mauve_project_index; genome_gen is that of
    // the index it was made from
    struct Projection {
        bool valid = false; uint64_t genome_gen = 0;
        int N = 0, n_proj = 0, drop_empty = 1; int32_t proj[MAUVE_MAX_SEQ] = {0};
        int64_t n_iv = 0, n_cols = 0, n_fill = 0, n_piece = 0, n_unit = 0;      // n_piece, n_unit: the shape of the work area pj_work keeps
        bool have_src = false;               // pj_src holds the source columns (made by the first fetch that asks for them)
        std::vector<int64_t> left, right, col_off, src_off, src_iv;
        std::vector<int8_t> reverse, src_flip;
    } pj;
    // annotated ranges mapped through the alignment (feature_dev.hip): the pieces of the last mauve_map_ranges stay on the device
    // for their fetches -- int64 piece_off[n + 1] | covered[n] | best[n] | six arrays [n_piece] | three [n_piece * N] (FmLayout) -- and belong to the
    // index they were made on (an index call clears `valid`).  The overlap join keeps nothing between calls
    struct RangeMap { bool valid = false; int N = 0; int64_t n_query = 0, n_piece = 0; } fm;
    DevBuf fm_work, fm_res, fo_work;           // the flag word, queries, first pieces, counts and their scan; the result; the join's table, its sort buffers, queries and answers
    DevBuf pj_work, pj_cols, pj_src, pj_out;   // the flag word, pieces, unit counts, their scan and kept words (stays with the result); the columns; their source columns, once asked for; the compact form of a fetch
    DevBuf run_sum;                      // pairwise finder: run list (start, length, exactly-once genome set)
    DevBuf rec_vinv, rec_vcm;            // ... and their ambiguity / contig bitmaps, when the resident genomes have them
    DevBuf rec_genomes, rec_seg;         // recursive anchoring: gap sub-sequences + segment table
    DevBuf placed_mask;                  // guide-tree recursive anchoring: placed-base bitmap
    // last match list (canonical order, host) + nseq it refers to
    std::vector<int64_t> match_len, match_start;
    int64_t n_matches = 0;
    int64_t dev_rec_n = -1;              // >= 0: sorted_rec holds that many records (int64 length[n], start[n*nseq]) in canonical order

    // DP workspace
    DevBuf dp_desc, dp_list, dp_codes, dp_off, dp_prof_cnt, dp_prof_mask, dp_prof2_cnt, dp_prof2_mask, dp_tb, dp_meta, dp_score,
        dp_cols, dp_rows, dp_sp, dp_pick, dp_wflags;

    // the seed pass may leave its match list on the device only (sorted_rec) when the caller says so: mauve_align's device tail
    bool pair_sums_only = false;          // seed pass for the guide tree: per-pair length sums instead of the match list
    std::vector<int64_t> pair_sums;
    int64_t bp_min_len = -1;              // >= 0 with pair_sums_only: also count the broken adjacencies of every pair's matches of at least this length
    std::vector<int64_t> pair_bp;         // [N*N], upper triangle (a < b)
    DevBuf bp_work;
    std::vector<uint8_t> rec_flags;       // one byte per anchor in chain order (LCB by LCB): the gap behind it is a candidate of the recursion; empty = not known (recursive.cpp tests every gap)
    bool lazy_matches_ok = false, matches_pending = false;
    int match_nseq = 0;
    // where dp_run_from_anchors left its device-side results (valid until the next DP launch)
    struct DpFrontOut { const int32_t *alen, *ast, *alcb, *gapcode; const int64_t *col_off, *score; const uint32_t *cols; int64_t n_dp, n_cols; } dpf_out{};
    std::vector<DpSeqDesc> prog_desc;      // progressive.cpp: the descriptors of a node's intervals and of their refinement candidates (kept: no fresh pages per node)
    const int64_t *dp_last_col_off = nullptr; int64_t dp_last_n = 0;     // column offsets (device) and size of the batch dp_core ran last: dp_fetch_picked
    int64_t dp_band_from = INT64_MAX;     // intervals whose longest sequence exceeds this run the banded DP (dp_batch.hip)
    DevBuf dpf_anch, dpf_work, dpf_tot;   // device front end of the DP stage (dp_run_from_anchors)

    // profiling
    bool prof = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double k_ms[MAUVE_K_COUNT] = {0};
    int64_t k_launch[MAUVE_K_COUNT] = {0};
    int64_t k_units[MAUVE_K_COUNT] = {0};

    PinnedBuf pin_anch;                  // anchors in chain order on their way to the device, and the gap codes coming back
    PinnedBuf pin_dcols;                 // DP columns of the whole-call path (mauve_align, mauve_progressive_align)
    PinnedBuf pin_meta;                  // per-interval DP results (length, score, cells)
    PinnedBuf pin_dp_in;                 // DP inputs on their way to the device: offset tables, interval list, descriptors
    PinnedBuf pin_seed;                  // seed pass: counter readback (first 64 B) and the candidates' match records
    // host scratch of dp_core, kept across calls (see AlignState)
    struct DpHost {
        std::vector<int64_t> tb_off, rows_off, est, need, nmax, lst, lst2, seq_off, tb_list;
        std::vector<uint8_t> is_big, cls;
    } dph;
    // host scratch of the seed pass (match records before the canonical sort)
    struct SeedHost {
        std::vector<int32_t> hl, hs;
        std::vector<uint32_t> order, tmp;
        std::vector<uint64_t> k1;
    } sdh;

    // host work that does not depend on the seed pass, run by the seed pass right before its first wait on the
    // stream (extract, sort, join and run detection are in flight by then); one shot
    std::function<void()> shadow;

    SpinPool *pool = nullptr;            // host helpers, armed for the duration of an align call (workers.hpp)

    // one alignment spread over several contexts (mauve_set_shard): this rank, their number, the caller's all-gather
    int shard_rank = 0, shard_world = 1; mauve_allgather_fn shard_fn = nullptr; void *shard_user = nullptr;
    bool shard_on = false;                // the independent units inside the calls are dealt out and exchanged (world > 1; a one-rank RCCL communicator with MAUVE_SHARD_SINGLE: the same code, one part)
    void *shard_comm = nullptr;           // ncclComm_t of mauve_set_shard_rccl: the library runs the all-gathers itself, on its stream, through device buffers
    DevBuf shard_dev;                     // device side of an RCCL exchange: [my size | all sizes | my payload | all payloads]
    PinnedBuf shard_pin;                  // ... and its page-locked host side
    mauve_shard_stats shard_stat = {0, 0, 0, 0.0};

    // repeat penalty: the caller's mode, the mode in force for the alignment call under way (read by the sum-of-pairs
    // scoring launches), and the base multiplicities of the resident genomes for one seed pattern, cached by (genome generation, pattern)
    int repeat_mode = MAUVE_REPEAT_PENALTY_OFF, rp_now = MAUVE_REPEAT_PENALTY_OFF;
    uint64_t genome_gen = 0;             // bumped by every mauve_set_genomes
    uint64_t rp_gen = 0, rp_pat = 0;     // what rp_mult holds (rp_gen 0: nothing)
    DevBuf rp_wcnt, rp_mult;             // per window: its genome's count of the canonical mer (0 = invalid window); per base: the multiplicity
    std::vector<uint64_t> rp_off;        // byte offset of every genome in rp_mult (16-byte aligned)
    // repeat matches of one genome (repeat_dev.hip): the result of the last mauve_repeat_matches stays on the device for
    // mauve_repeat_fetch -- int64 length[n] | mult[n] | start_off[n + 1] | starts[ns], ordered by start 0 -- in a buffer no other call
    // writes; it belongs to the genomes it was made on (genome_gen tells an upload)
    struct RepeatMap { bool valid = false; uint64_t genome_gen = 0; int64_t n = 0, ns = 0; } rm;
    DevBuf rm_work, rm_res;              // the window table, candidate lists and scans; the result
    // a repeat map scored against a correct repeat alignment (repeat_score_dev.hip): no state between calls, buffers of its own
    DevBuf rs_work;                      // the flag word, totals, pair table and hit tables; the list; its extents, their sort buffers and prefix maxima

    AlignResult res;
    AlignState ast;
    mauve_stage_times stage{};
};

// base multiplicities of the resident genomes as a kernel argument: genome g's at p + off[g] (sp_score_matches, ch_sp_scores)
struct SpMult { const uint8_t *p; uint64_t off[MAUVE_MAX_SEQ]; };
// one pair of a sum-of-pairs column: substitution score s, base multiplicities mx, my of the two positions
template <int MODE>
__device__ __forceinline__ int64_t sp_pair(int32_t s, uint32_t mx, uint32_t my)
{
    if (MODE == MAUVE_REPEAT_PENALTY_OFF || s <= 0) return s;
    const int64_t r = (int64_t)(mx > my ? mx : my);
    return MODE == MAUVE_REPEAT_PENALTY_NEGATIVE ? (int64_t)s * (2 - r) / r : (int64_t)s / r;
}

// the repeat penalty of one alignment call: in force from repeat_begin to the end of the scope
struct RepeatScope {
    mauve_ctx *c;
    explicit RepeatScope(mauve_ctx *ctx) : c(ctx) { c->rp_now = MAUVE_REPEAT_PENALTY_OFF; }
    ~RepeatScope() { c->rp_now = MAUVE_REPEAT_PENALTY_OFF; }
};

// RAII-less helper: time one kernel launch on ctx->stream when profiling is on.
struct KernelTimer {
    mauve_ctx *c; int id; int64_t units;
    KernelTimer(mauve_ctx *ctx, int kid, int64_t u) : c(ctx), id(kid), units(u)
    {
        if (c->prof) (void)hipEventRecord(c->ev0, c->stream);
    }
    ~KernelTimer()
    {
        if (!c->prof) return;
        (void)hipEventRecord(c->ev1, c->stream);
        (void)hipEventSynchronize(c->ev1);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
        c->k_ms[id] += ms; c->k_launch[id] += 1; c->k_units[id] += units;
    }
};

static inline double now_ms()
{
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// ---- internal entry points between translation units ----
// the contributions of all ranks to one exchange: parts[r] = (pointer, bytes), valid until the next exchange (api.cpp)
int rec_gap_flags_device(mauve_ctx *c, const int32_t *alen, const int32_t *ast, const int32_t *alcb, int64_t na, int N, int64_t min_gap, uint8_t *d_flag);
int shard_allgather(mauve_ctx *c, const void *send, size_t bytes, std::vector<std::pair<const char *, size_t>> &parts);
// deterministic LPT packing of `cost` into the ranks (ties: lower index first, lower rank first): owner[i] = rank of unit i
void shard_lpt(const std::vector<int64_t> &cost, int world, std::vector<int> &owner);
bool make_seed_shape(uint64_t pattern, SeedShape *out);
GenomeSet main_genome_set(mauve_ctx *ctx);
bool seedpass_wide(int64_t total_windows);
// genome sets of 2^31 bases or more: the seed-pass entry points take them; the alignment path behind them refuses them
// (MAUVE_ERR_LIMIT, `what` named) until it is verified at that size
int refuse_scoring(mauve_ctx *c, const mauve_scoring *sc, const char *what);   // an entry beyond +-MAUVE_SCORING_MAX: MAUVE_ERR_ARG
int refuse_scoring_batch(mauve_ctx *c, const mauve_scoring *sc, int nseq, int64_t n_iv, const int64_t *seq_off, const char *what);   // ... or a scheme that does not fit the 32-bit DP at these intervals' lengths
int refuse_scoring_params(mauve_ctx *c, const mauve_params *p, const char *what);                                                    // ... or at the lengths the parameters admit
int refuse_past_2g(mauve_ctx *c, const char *what);      // 64-bit window indices for a pass of this many windows
int seedpass_run(mauve_ctx *ctx, const GenomeSet &gs, uint64_t pattern, int mode, uint64_t mask, int extend,
                 const uint32_t *seg_dev, uint32_t nseg, int64_t *n_matches);
int seedpass_enumerate(mauve_ctx *ctx, const GenomeSet &gs, int seq, uint64_t pattern, EnumRequest &q);
int seedpass_from_hits(mauve_ctx *ctx, const GenomeSet &gs, uint64_t pattern, const HostHits &hits, int extend, int64_t *n_matches);
int seedpass_sorted_list(mauve_ctx *ctx, const GenomeSet &gs, int seq, uint64_t pattern, std::vector<uint64_t> *keys,
                         std::vector<uint32_t> *vals, int *weight);

int sort_pairs_u32(mauve_ctx *ctx, uint32_t n, int key_bits, uint32_t **keys_io, uint32_t **vals_io, uint32_t *keys_alt, uint32_t *vals_alt,
                   int timer_id);
int sort_pairs_u32_batch(mauve_ctx *ctx, uint32_t S, uint32_t n, size_t seg_stride, int key_bits, uint32_t **keys_io, uint32_t **vals_io,
                         uint32_t *keys_alt, uint32_t *vals_alt, int timer_id);
int sort_pairs_u64(mauve_ctx *ctx, uint32_t n, int key_bits, uint64_t **keys_io, uint32_t **vals_io, uint64_t *keys_alt, uint32_t *vals_alt,
                   int timer_id);
// The two translation units of the seed pass: seed_pass.hip (everything that depends on the key and index widths) hands over to
// seed_finish.hip once the ncand candidate records of all finder passes are in ctx->mlen / mstart (on_host: in ctx->sdh.hl / hs
// already): the guide tree's per-pair sums (ctx->pair_sums_only) or the match list in canonical order.
int seed_finish(mauve_ctx *ctx, const GenomeSet &gs, const SeedRequest &rq, uint32_t ncand, bool on_host, double &trace_t0);
inline void seed_trace(mauve_ctx *ctx, const char *label, double &t0)
{
    if (!switches().trace) return;
    (void)hipStreamSynchronize(ctx->stream);
    const double t = now_ms();
    fprintf(stderr, "[trace] %-22s +%.3f ms\n", label, t - t0);
    t0 = t;
}
// The first `bytes` of the seed pass's counter block, in page-locked memory once the stream has drained.  (pin_seed also carries
// slice tables and records behind its first 64 bytes: whoever reuses it has synchronised first.)
inline int seed_counters(mauve_ctx *ctx, size_t bytes, const uint32_t **words)
{
    HIPCHK(ctx, ctx->pin_seed.ensure(64));
    HIPCHK(ctx, hipMemcpyAsync(ctx->pin_seed.p, ctx->counters.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *words = ctx->pin_seed.as<uint32_t>();
    return MAUVE_OK;
}
// device chain (chain_dev.hip): EliminateOverlaps + LCBs of the N-way list the seed pass left in ctx->sorted_rec
int chain_device(mauve_ctx *c, int N, int64_t min_weight, bool collinear, MatchVec &m, std::vector<int64_t> &match_lcb, int64_t &n_lcb, const mauve_scoring *sp_scoring = nullptr);
struct ChainGraphHost { uint32_t na, K; int64_t *weight; uint32_t *orient; int32_t *prev, *next; int32_t *final_stage; int32_t *final_dev; };
int chain_device_graph(mauve_ctx *c, int N, int64_t maxlen, const uint32_t *seg0, uint32_t nseg, ChainGraphHost *G, bool graph_to_host = true, const mauve_scoring *sp_scoring = nullptr);
int chain_device_gaps_compact(mauve_ctx *c, int N, int64_t maxlen, const uint32_t *seg0_dev, uint32_t nseg, const int32_t **hl_out, const int32_t **hs_out,
                              const uint32_t **hgap_out, uint32_t *ns_out);
int chain_device_core(mauve_ctx *c, int N, int64_t min_weight, bool collinear, int64_t &n_lcb, const mauve_scoring *sp_scoring = nullptr);
int chain_device_gaps(mauve_ctx *c, int N, int64_t maxlen, const uint32_t *seg0_dev, uint32_t nseg, const int32_t **hl_out, const int32_t **hs_out,
                      const uint32_t **hgap_out, uint32_t *ns_out);
// recursive anchoring of the long gaps of `chains` (N genomes; gmap: their resident genomes, nullptr = 0 .. N-1), recursive.cpp
int recursive_anchoring(mauve_ctx *c, const mauve_params *p, int w0, std::vector<MatchVec> &chains, int N, const int *gmap);
int chain_device_copy_back(mauve_ctx *c, int N, MatchVec &m, std::vector<int64_t> &match_lcb);
int chain_order_device(mauve_ctx *c, int N, int64_t nl, int64_t min_gap, int64_t *na_out, int64_t *n_rec_out);
int extend_lcbs_device(mauve_ctx *c, const mauve_params *p, int w, int64_t lcbw, int N, const int32_t **alen_io, const int32_t **ast_io,
                       const int32_t **alcb_io, int64_t *na_io, int64_t *nl_io, int64_t *n_rec_io, std::vector<int64_t> &lcb_weight);

// host chaining (chain_host.cpp)
struct ChainOrders { std::vector<std::vector<uint32_t>> ord; bool sparse = false; };   // per genome: match indices in left-end order;
                                                                                        // sparse: the list still holds dead records (not named here)
void host_eliminate_overlaps(MatchVec &m, ChainOrders *orders = nullptr, bool compact = true);
int seed_family_matches(mauve_ctx *c, const GenomeSet &gs, int w, int mode, uint64_t mask, MatchVec &out);    // pipeline.cpp
void host_merge_matches(MatchVec &kept, const MatchVec &add);        // seed families: kept + what of add no kept match contains
void host_left_orders(const MatchVec &m, ChainOrders &orders);       // per-genome left-end order of an overlap-free list
void host_lcb_chain(const MatchVec &m, int64_t min_weight, bool collinear, std::vector<int64_t> &match_lcb, int64_t &n_lcb,
                    const ChainOrders *orders = nullptr, const int64_t *match_weight = nullptr);
// extant sum-of-pairs scores of the matches of m (n components; gmap: their genomes, nullptr = 0..n-1), assemble_dev.hip
// (c->rp_now != OFF: penalized by the multiplicities in c->rp_mult)
int match_sp_scores(mauve_ctx *c, const MatchVec &m, const int *gmap, const mauve_scoring *sc, std::vector<int64_t> &out);
// base multiplicities of the resident genomes for `pattern` into c->rp_mult (seed_pass.hip; cached)
int repeat_multiplicity(mauve_ctx *c, uint64_t pattern);
// the repeat map of resident genome `seq` (repeat_dev.hip) into c->rm / c->rm_res; the fetch finishes the canonical order
int repeat_matches(mauve_ctx *c, int seq, uint64_t pattern, int64_t min_multi, int64_t max_multi);
int repeat_fetch(mauve_ctx *c, int64_t *length, int64_t *mult, int64_t *start_off, int64_t *starts);
// the root seed pattern of a call (seed families: the first of the family) -> multiplicities, c->rp_now = the context's mode; only
// under sum-of-pairs LCB scoring (pipeline.cpp)
int repeat_begin(mauve_ctx *c, const mauve_params *p, int w, uint64_t pat);
int64_t sp_default_min_weight(int w, int n, const mauve_scoring *sc);
// the steps the align path and the progressive path share (chain_host.cpp; the pure ones: host_chain.hpp)
// seed weight and pattern of a call over genomes of average length avg_len; pat == nullptr: the weight alone, which never fails
int resolve_seed(mauve_ctx *c, const mauve_params *p, int64_t avg_len, const char *who, int *w, uint64_t *pat);
void seed_matches_to_vec(const mauve_ctx *c, int n, int64_t nm, MatchVec &m);      // the seed pass's host list (match_len / match_start) as records
// host chain of a list: overlap elimination, sum-of-pairs scores when p->lcb_scoring asks for them (minimum weight minw_sp, the scores
// left in *match_weight when given), LCBs; lcbw: the minimum weight of length-weighted LCBs; *t_elim: when the elimination was done
int host_chain_lcbs(mauve_ctx *c, const mauve_params *p, MatchVec &m, const int *gmap, int64_t lcbw, int64_t minw_sp, std::vector<int64_t> &match_lcb,
                    int64_t &nl, std::vector<int64_t> *match_weight, bool compact, double *t_elim = nullptr);
void result_reset(AlignResult &R);       // a new result: tables emptied, the column buffer and its fill state kept
void restore_cols(AlignResult &R, uint32_t full, SpinPool *pool = nullptr);        // the gap ranges of the last result back to `full`

void lcb_greedy(int N, int32_t K, int64_t *weight, const uint32_t *orient_bits, int32_t *prevv, int32_t *nextv, int64_t min_weight,
                bool collinear, std::vector<int64_t> &final_id, int64_t &n_lcb);

// DP (dp_batch.hip)
int dp_batch_run_desc(mauve_ctx *ctx, int nseq, int64_t n_iv, const DpSeqDesc *desc, const mauve_scoring *sc,
                      uint32_t *cols, int64_t *col_off, int64_t *score, int64_t *cells, bool may_shard = false, int64_t *sp = nullptr);
// the same with the rows behind n_orig made on the device as rotations of the first n_orig (cbase: first candidate of every interval, n_orig + 1 entries);
// only when dp_desc_rotations_on_device(n_total)
bool dp_desc_rotations_on_device(int64_t n_total);
int dp_batch_run_desc_rot(mauve_ctx *ctx, int nseq, int64_t n_orig, const DpSeqDesc *desc, const int32_t *cbase, int64_t n_total, const mauve_scoring *sc,
                          int64_t *col_off, int64_t *score, int64_t *cells, int64_t *sp);
// gapped-alignment eligibility of an inter-anchor interval by its longest sequence: full DP up to max_gapped_len, banded
// DP above it up to max_banded_len
inline int64_t dp_len_limit(const mauve_params *p) { return p->max_banded_len > p->max_gapped_len ? p->max_banded_len : p->max_gapped_len; }
inline int64_t dp_band_from_of(const mauve_params *p) { return p->max_banded_len > p->max_gapped_len ? p->max_gapped_len : INT64_MAX; }
int dp_run_from_anchors(mauve_ctx *ctx, int N, int64_t na, const int32_t *h_len, const int32_t *h_st, const int32_t *h_lcb, int gapped,
                        int64_t max_gapped_len, const mauve_scoring *scoring, int32_t *gapcode, int64_t *n_dp_out, int64_t *code_total_out,
                        PinnedBuf *dcols, std::vector<int64_t> &dcol_off, std::vector<int64_t> &dscore, int64_t *cells, int stay = 0);
int assemble_device(mauve_ctx *c, int64_t na, int64_t cells, mauve_align_sizes *sizes, bool host_chains = false);
// An alignment as the stages behind it take it (backbone S12, homology pass S12b, coordinate index S14): the interval table on the host
// ([n_iv][N] ends and strands, n_iv + 1 column offsets), the columns on the device.  The two makers and the checks are in aln_view.hip
struct AlnView { int N; int64_t n_iv; const int64_t *left, *right; const int8_t *reverse; const int64_t *col_off; const uint32_t *d_cols; };
// the result of this context: refused when it is stale (refuse_replaced: also when the genomes were replaced under a host-side result) or when there is
// none; the columns where the assembly stage left them, else uploaded to upload_to.  An empty alignment comes back with N = nseq and no columns
int aln_from_context(mauve_ctx *c, const char *who, bool refuse_replaced, DevBuf &upload_to, AlnView *out);
// a caller's arrays: pointer checks, col_off ascends from 0, the columns to bb_cols (waited for: they are the caller's memory), check_columns
int aln_from_arrays(mauve_ctx *c, const char *who, int nseq, int64_t n_iv, const int64_t *left, const int64_t *right, const int8_t *reverse, const int64_t *col_off,
                    const uint32_t *cols, AlnView *out);
// the kernels turn column offsets into block and tile indices: they ascend from 0 (checked before anything is sized by them)
int coord_check_offsets(mauve_ctx *c, const char *who, int64_t n_iv, const int64_t *col_off);
// a caller's columns against its interval table: right - left + 1 residues of every present genome, none of an absent one, no bit at or above nseq
int check_columns(mauve_ctx *c, const char *who, const AlnView &A);
void coord_index_release(mauve_ctx *c);  // coord_dev.hip: the host side of the coordinate indices (their device buffers go with the context's DevBufs)
// coord_dev.hip: the index of a caller's alignment into the slot X / index (mauve_coord_index_alignment: co / co_index; mauve_score_truth: co_truth / co_truth_index)
int coord_index_arrays(mauve_ctx *c, const char *who, mauve_ctx::CoordIndex &X, DevBuf &index, int nseq, int64_t n_iv, const int64_t *left, const int64_t *right,
                       const int8_t *reverse, const int64_t *col_off, const uint32_t *cols);
int materialize_result(mauve_ctx *c);
int materialize_tables(mauve_ctx *c);
int fetch_columns(mauve_ctx *c, uint32_t *dst);
bool fetch_compact_direct(mauve_ctx *c, int col_bytes, int32_t *mum_length, int32_t *mum_start, int32_t *anchor_length, int32_t *anchor_start, int32_t *anchor_lcb,
                          void *cols, bool *tables_done, bool *cols_done, int *rc_out);
// device tail of mauve_align: the two bulk tables start for the buffers mauve_align_prefetch named (assemble_dev.hip)
int prefetch_tables_enqueue(mauve_ctx *c, int N, int64_t na, const int32_t *alen, const int32_t *ast, const int32_t *alcb);
bool fetch_tables_direct(mauve_ctx *c, int64_t *mum_length, int64_t *mum_start, int64_t *anchor_length, int64_t *anchor_start, int64_t *anchor_lcb, int *rc_out);
// coord_dev.hip: the index in force from device columns and a host interval table (mauve_project_index)
int coord_index_device(mauve_ctx *c, const char *who, const AlnView &A);
bool host_pointer_is_pinned(const void *p);
// device -> caller on the context's stream: a page-locked destination directly (queued: the caller synchronises), a pageable one through `pin`
// in pieces of 64 MiB, each waited for
inline int copy_to_caller(mauve_ctx *c, PinnedBuf &pin, void *dst, const void *src, size_t bytes)
{
    if (!bytes) return MAUVE_OK;
    if (host_pointer_is_pinned(dst)) { HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream)); return MAUVE_OK; }
    const size_t piece = (size_t)64 << 20;
    HIPCHK(c, pin.ensure(std::min(bytes, piece)));
    for (size_t o = 0; o < bytes; o += piece) {
        const size_t n = std::min(piece, bytes - o);
        HIPCHK(c, hipMemcpyAsync(pin.p, static_cast<const char *>(src) + o, n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        memcpy(static_cast<char *>(dst) + o, pin.p, n);
    }
    return MAUVE_OK;
}
int host_genomes(mauve_ctx *c);
int seed_matches_to_host(mauve_ctx *ctx);
int dp_fetch_picked(mauve_ctx *ctx, int64_t n_pick, const int64_t *pick, const int64_t *col_off, uint32_t *out, int64_t *out_off);
int dp_batch_run(mauve_ctx *ctx, int nseq, int64_t n_iv, const uint8_t *codes, const int64_t *seq_off,
                 const mauve_scoring *sc, uint32_t *cols, int64_t *col_off, int64_t *score, int64_t *cells);
