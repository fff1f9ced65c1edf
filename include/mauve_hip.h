/*
 * mauve_hip.h -- C-ABI of the MI355X-native mauveAligner hot path (libmauve_hip.so).
 *
 * This is the drop-in boundary.  The reference has no C plugin ABI: its seams are the
 * C++ virtual interfaces of libMems.  Each entry point below names the libMems interface it stands
 * behind, cited by the in-tree call site that pins its contract (file:line relative to the
 * reference tree).  The C++ adapters in include/libMems/ (namespace mems) call these and nothing
 * else; INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions: plain pointers and sizes, caller-owned output buffers (two-phase count / fill),
 * every call returns an int status (0 = MAUVE_OK) and never throws; mauve_last_error() gives the
 * text.  A context is thread-compatible (one thread at a time); there are no hidden globals.
 * Coordinates follow libMems: signed 1-based starts, negative = reverse strand, 0 = NO_MATCH
 * (SeedMatchEnumerator.h:83,127-141; sortContigs.cpp:46).
 * Environment: the MAUVE_* switches are read once, when the process creates its first context; INTEGRATION.md,
 * "Environment switches", lists them and says which few are part of the supported interface.
 */
#ifndef MAUVE_HIP_H
#define MAUVE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAUVE_OK 0
#define MAUVE_ERR_ARG (-1)        /* bad argument */
#define MAUVE_ERR_HIP (-2)        /* HIP runtime failure (text in mauve_last_error) */
#define MAUVE_ERR_NOGPU (-3)      /* no usable device: the product has no CPU fallback */
#define MAUVE_ERR_LIMIT (-4)      /* input exceeds a documented limit */
#define MAUVE_ERR_STATE (-5)      /* call order violated (e.g. no genomes set) */

#define MAUVE_MAX_SEQ 32
/* genome set limits (MAUVE_ERR_LIMIT, checked by mauve_set_genomes*): every genome holds fewer than 2^31 bases (match and anchor starts
   stay int32 on the device), and the genomes together fewer than 2^32 - 2^20 (every window count, rounded up to whole tiles, stays
   32-bit).  A seed pass over 2^31 windows or more carries 64-bit window indices.  On a set of 2^31 bases or more in
   total only the seed-pass entry points run (mauve_seed_mums, mauve_extend_hits, mauve_sorted_mer_list, mauve_seed_match_enumerate,
   mauve_seed_multiplicity); the alignment entry points return MAUVE_ERR_LIMIT (not yet verified at that size). */
#define MAUVE_MAX_GENOME_LEN (1LL << 31)
#define MAUVE_MAX_TOTAL_LEN ((1LL << 32) - (1LL << 20))
#define MAUVE_MAX_SEED_SPAN 49
#define MAUVE_CODING_SEED 3                /* mauveAligner.cpp:266-279 */
#define MAUVE_SOLID_SEED 0x7fffffff        /* repeatoire.cpp:1847 (SOLID_SEED == INT_MAX) */

/* seed-hit rule = which MatchFinder subclass's EnumerateMatches is in force */
#define MAUVE_MODE_MEM 0      /* mems::MemHash / MaskedMemHash (mauveAligner.cpp:523-531) */
#define MAUVE_MODE_UNIQUE 1   /* UniqueMatchFinder::EnumerateMatches (UniqueMatchFinder.cpp:36-60) */
#define MAUVE_MODE_PAIRWISE 2 /* mems::PairwiseMatchFinder (progressiveMauve.cpp:496-501): MemHash on every genome
                                pair separately; matches have exactly two components; mask is ignored */

#define MAUVE_LCB_SCORE_LENGTH 0
#define MAUVE_LCB_SCORE_SP 1

/* repeat penalty on sum-of-pairs anchor scores (progressiveMauve --repeat-penalty, progressiveMauve.cpp:295,606-609; the libMems
   global penalize_repeats; frozen form DESIGN.md S11d) */
#define MAUVE_REPEAT_PENALTY_OFF 0
#define MAUVE_REPEAT_PENALTY_NEGATIVE 1
#define MAUVE_REPEAT_PENALTY_ZERO 2

typedef struct mauve_ctx mauve_ctx;

/* The domain of a scoring scheme.
   (1) Every entry -- gap_open, gap_extend and the 16 of the matrix -- lies within +-MAUVE_SCORING_MAX, and gap_open <= 0: every state of the
       DP may follow every state, so a rewarded gap opening could be collected in every column.  (gap_extend may be positive.)
   (2) The gapped DP runs in int32 with -2^29 as minus infinity; its first boundary row is analytic and not clamped and
       aligned columns add up without an upper clamp, so a scheme must also fit the lengths it is used on.  Every progressive step is a DP
       of its own that starts at 0.  For an interval of k sequences with L bases together, the longest of n:
           2 k |gap_open| + (L + k n) |gap_extend| + k max|matrix|   <  MAUVE_DP_SCORE_MAX    (the all-gap path bounds every cell from below)
           k n max(matrix, 0) + (L + k n) max(gap_extend, 0)         <  MAUVE_DP_SCORE_MAX    (n aligned columns of k rows, and gap columns that
                                                                                               face L + k n residues at most, bound it from above)
       Inside this the result is the frozen definition bit for bit; outside it a sum could wrap, and the call is refused instead.
   mauve_dp_batch[_banded] check (1) and, interval by interval, (2).  mauve_align*, mauve_progressive_align* check (1) and, when `gapped` is set,
   (2) for the largest interval the parameters admit: k = the resident genomes, n = max(max_gapped_len, max_banded_len), L = k n.  For the
   default scheme the second line decides: n <= 5 368 709 / k, that is max_banded_len up to 2 684 354 for two genomes, 671 088 for eight, 167 772
   for 32 (the default lengths need 8e7 of the 5.4e8 at 32 genomes).  mauve_match_sp_scores[_repeat] add in 64 bits and check (1) only.  A refusal
   is MAUVE_ERR_ARG and the message names the limit. */
#define MAUVE_SCORING_MAX (1 << 20)
#define MAUVE_DP_SCORE_MAX (1 << 29)

typedef struct {
    int32_t gap_open;             /* PairwiseScoringScheme.gap_open  (progressiveMauve.cpp:666-687) */
    int32_t gap_extend;           /* PairwiseScoringScheme.gap_extend */
    int32_t matrix[4][4];         /* score_t matrix[4][4], A,C,G,T (readSubstitutionMatrix, :684) */
} mauve_scoring;

typedef struct {
    uint64_t seed_pattern;        /* 0 -> getSeed(weight, rank) */
    int32_t seed_weight;          /* 0 -> getDefaultSeedWeight(avg length)  (mauveAligner.cpp:92,650) */
    int32_t seed_rank;            /* mauveAligner.cpp:93 */
    int32_t mode;                 /* MAUVE_MODE_* */
    int64_t lcb_weight;           /* -1 -> 3*weight*N (mauveAligner.cpp:648-653); total, i.e. already *N */
    int32_t collinear;            /* mauveAligner.cpp:665-666 */
    int32_t recursive;            /* mauveAligner.cpp:94 */
    int32_t gapped;               /* mauveAligner.cpp:96 */
    int32_t add_unaligned;        /* mauveAligner.cpp:748 addUnalignedIntervals */
    int32_t extend_lcbs;          /* lcb_extension, mauveAligner.cpp:95: default 1, as there (frozen form DESIGN.md S10; not applied to score-weighted LCBs) */
    int32_t max_extension_iters;  /* Aligner::SetMaxExtensionIterations, default 4 (mauveAligner.cpp:687-690) */
    int64_t min_recursive_gap;    /* Aligner::SetMinRecursionGapLength, default 200 (:670-672,899) */
    int64_t max_gapped_len;       /* Aligner::SetMaxGappedAlignmentLength (:674-676), default 10000 */
    mauve_scoring scoring;
    int64_t max_banded_len;       /* no reference counterpart (its aligner leaves intervals above max_gapped_len unaligned): intervals
                                     whose longest sequence is in (max_gapped_len, max_banded_len] are aligned by the banded DP
                                     (DESIGN.md S7b); default 0 = off */
    int32_t lcb_scoring;          /* ProgressiveAligner::setLcbScoringScheme (progressiveMauve.cpp:611-625): MAUVE_LCB_SCORE_LENGTH
                                     (0, default: weight = sum of length * n, the Aligner::align rule) or MAUVE_LCB_SCORE_SP (1: extant
                                     sum-of-pairs score of the anchors); lcb_weight is then a score */
    int32_t weight_scaling;   /* progressive path: scale every node's minimum LCB weight by the conservation distance of its two
                                 subtrees (ProgressiveAligner::setUseLcbWeightScaling, progressiveMauve.cpp:626-627); default 0 */
    int32_t conservation_scale_ppm;   /* setConservationDistanceScale in parts per million (:633-637; call-site default 0.5 = 500000) */
    int32_t seed_family;      /* search with the family of three seeds of the weight instead of one (progressiveMauve.cpp:502-546 --seed-family;
                                 ProgressiveAligner::setUseSeedFamilies :604-605); default 0 */
    int64_t min_scaled_penalty;       /* setMinimumBreakpointPenalty (:649-652): floor of the scaled weight; default 0 */
    int32_t refine_rounds;    /* progressive path, ProgressiveAligner::setRefinement (progressiveMauve.cpp:578-579): every gapped interval of >= 3
                                 sequences is also aligned in up to this many rotated orders and the alignment with the best sum-of-pairs score
                                 is kept (frozen form DESIGN.md S13); default 0 = off, the mirror's ProgressiveAligner starts with 2 */
    int32_t bp_dist_scale_ppm;/* setBreakpointDistanceScale in parts per million (--max-breakpoint-distance-scale, :628-632; call-site default
                                 0.5): with weight_scaling, a node's minimum weight also shrinks with the breakpoint distance between its two
                                 subtrees (frozen form DESIGN.md S11c); default 0 */
    int64_t bp_dist_min_score;/* setBpDistEstimateMinScore (:638-642): pairwise matches shorter than this do not count towards the breakpoint
                                 estimate; -1 (default) = 2 x seed weight */
} mauve_params;

/* sizes of the result of mauve_align(), for the caller to allocate the fill buffers */
typedef struct {
    int64_t n_mums;               /* N-way multi-MUMs found by the seed pass */
    int64_t n_lcb;
    int64_t n_anchor;             /* anchors after overlap elimination + recursive anchoring */
    int64_t n_iv;                 /* intervals: LCBs first, then unaligned single-genome islands */
    int64_t n_cols;               /* total alignment columns over all intervals */
    int64_t n_gap_dp;             /* inter-anchor intervals aligned by DP */
    int64_t n_dp_cells;           /* DP cells evaluated */
} mauve_align_sizes;

/* ---- context ----------------------------------------------------------------------------------- */
int mauve_ctx_create(int device, mauve_ctx **out);
void mauve_ctx_destroy(mauve_ctx *ctx);
const char *mauve_last_error(const mauve_ctx *ctx);       /* ctx may be NULL: last create error */
int mauve_device_name(const mauve_ctx *ctx, char *buf, size_t buflen);
int mauve_synchronize(mauve_ctx *ctx);
/* Page-locked host memory for the caller's bulk buffers (no reference counterpart: libMems keeps everything in pageable
   std::vectors).  Optional: every entry point takes any host pointer.  mauve_set_genomes uploads packed genomes that
   live in such a buffer straight from it, and mauve_align_fetch copies the column array straight into one (one DMA,
   no staging copy); pageable buffers go through the context's page-locked staging as before. */
int mauve_host_alloc(size_t bytes, void **out);
void mauve_host_free(void *p);

/* ---- seeds (host-side helpers; libMems free functions getSeed/getSeedLength/getDefaultSeedWeight,
        progressiveMauve.cpp:217,511-517; MatchList::GetDefaultMerSize, mauveAligner.cpp:651) ------ */
uint64_t mauve_get_seed(int weight, int rank);
int mauve_seed_length(uint64_t pattern);
int mauve_seed_weight(uint64_t pattern);
int mauve_default_seed_weight(int64_t avg_len);
void mauve_default_scoring(mauve_scoring *s);              /* hoxd_matrix, -400, -30 */
void mauve_default_params(mauve_params *p);                /* mauveAligner's call site (mauveAligner.cpp:92-99) */
/* progressiveMauve's call site: what a ProgressiveAligner does when main() sets nothing -- ExtantSumOfPairsScoring
   (progressiveMauve.cpp:624-625), LCB weight scaling on with conservation and breakpoint distance scales 0.5 (:285-287,626-637),
   refinement on (:578-579): lcb_scoring = SP, weight_scaling = 1, both *_scale_ppm = 500000, refine_rounds = 2. */
void mauve_default_progressive_params(mauve_params *p);
/* 2-bit packing used at the boundary: base i -> 64-bit word i/32, bits 2*(i%32); A,C,G,T=0..3,
   anything else -> 0.  words must hold mauve_packed_words(len) entries. */
size_t mauve_packed_words(int64_t len);
void mauve_pack_ascii(const char *ascii, int64_t len, uint64_t *words);
void mauve_pack_codes(const uint8_t *codes, int64_t len, uint64_t *words);

/* ---- genomes: gnSequence table of a MatchList (MatchList.seq_table; mauveAligner.cpp:453-465).
        Uploads the packed genomes; they stay resident in HBM until the next call / destroy. ------- */
int mauve_set_genomes(mauve_ctx *ctx, int nseq, const uint64_t *const *packed, const int64_t *lens);

/* The same for sequences that are concatenations of contigs and / or hold ambiguous bases (a multi-record FastA
   loaded as one gnSequence, mauveAligner.cpp:453-465; the contig-start table RepeatHashCat keeps for concatenated
   input, RepeatHashCat.h:19-20 `concat_contig_start`).  n_contigs[g] 0-based ascending starts per genome (the first
   is 0), concatenated in contig_starts; invalid[g]: bitmap of the bases that are not A, C, G, T (bit i of word i/64;
   mauve_ambiguity_bitmap builds it; the array or any entry may be NULL).  No seed window touches an ambiguous base
   or runs across a contig join: matches never cover an ambiguous base, and a match continues over a join only where
   windows on its two sides abut on one diagonal in every genome.  The packed genomes carry A at ambiguous bases
   (the gapped alignment sees A); mauve_write_xmfa prints N there. */
int mauve_set_genomes_contigs(mauve_ctx *ctx, int nseq, const uint64_t *const *packed, const int64_t *lens,
                              const int64_t *n_contigs, const int64_t *contig_starts, const uint64_t *const *invalid);
void mauve_ambiguity_bitmap(const char *ascii, int64_t len, uint64_t *bits);      /* bits: len/64 + 1 words */

/* ---- sorted mer list: MatchList::CreateMemorySMLs / DNAFileSML for one genome
        (mauveAligner.cpp:456,465; SortedMerList::GetMer semantics SeedMatchEnumerator.h:133).
        mer_out: mer left-aligned in 64 bits | strand flag in bit 0; pos_out: 0-based positions;
        both must hold len-span+1 entries.  Returns the entry count in *n_out. ------------------- */
int mauve_sorted_mer_list(mauve_ctx *ctx, int seq, uint64_t pattern, uint64_t *mer_out,
                          int64_t *pos_out, int64_t *n_out);

/* ---- multi-MUMs: MatchFinder::FindMatches(MatchList&) = AddSequence* + CreateMatches + GetMatchList
        (progressiveMauve.cpp:490-501; mauveAligner.cpp:577-589).  mask != 0 keeps only matches
        whose component set equals mask (MaskedMemHash::SetMask, mauveAligner.cpp:525-531);
        extend = 0 returns seed-length matches (SeedMatchEnumerator.h:71-123).  The result stays on
        the device; *n_matches receives the count.  mauve_get_matches copies it out in canonical
        order: length[n], start[n*nseq]. ---------------------------------------------------------- */
int mauve_seed_mums(mauve_ctx *ctx, uint64_t pattern, int mode, uint64_t mask, int extend,
                    int64_t *n_matches);
int mauve_get_matches(mauve_ctx *ctx, int64_t *length, int64_t *start);
/* ---- MemHash::HashMatch for seed hits a host-side finder enumerated itself: the host callback path of a MatchFinder
        subclass that overrides EnumerateMatches(IdmerList&) and calls HashMatch per hit (UniqueMatchFinder.cpp:36-60;
        the virtuals UniqueMatchFinder.h:31, SeedMatchEnumerator.h:38-39).  Hit h has the genomes of mask[h]; genome g's
        window starts at 0-based base pos[h*nseq+g] and strand[h*nseq+g] is the strand flag of its stored mer (bit 0 of
        SortedMerList::GetMer, SeedMatchEnumerator.h:133).  The hits are extended (extend != 0) and put in canonical
        order exactly like the hits of mauve_seed_mums; fetch with mauve_get_matches. ----------------------------- */
int mauve_extend_hits(mauve_ctx *ctx, uint64_t pattern, int64_t n_hits, const uint32_t *mask, const int64_t *pos,
                      const uint8_t *strand, int extend, int64_t *n_matches);

/* ---- SeedMatchEnumerator::FindMatches (SeedMatchEnumerator.h:19-33): single genome `seq`, every
        mer with min_multi..max_multi occurrences becomes one match (CSR output).  Two-phase: call
        with starts == NULL to get *n_out and *n_starts, then again with buffers. ----------------- */
int mauve_seed_match_enumerate(mauve_ctx *ctx, int seq, uint64_t pattern, int64_t min_multi,
                               int64_t max_multi, int direct_only, int64_t *n_out, int64_t *n_starts,
                               int64_t *mult, int64_t *start_off, int64_t *starts);

/* ---- repeat map of one genome: RepeatHash::FindMatches (mauveAligner.cpp:480-483, mauveAligner --repeats; frozen form DESIGN.md
        S20).  The copies of a mer inside resident genome `seq` -- a family of m valid windows, max(2, min_multi) <= m <= max_multi
        <= MAUVE_REPEAT_MAX_MULT -- are extended along their diagonal into maximal ungapped repeat matches, each emitted once.
        mauve_repeat_matches leaves the result on the device and returns the counts; mauve_repeat_fetch copies it out in canonical
        order as a CSR: length[n], mult[n], start_off[n + 1], starts[n_starts] (signed 1-based starts of a match's components in
        ascending position; component 0 is positive).  The result stays until the next mauve_repeat_matches or genome upload;
        like mauve_seed_match_enumerate the call reuses the seed pass's workspace (a device-resident alignment result is brought
        to the host first); the match list of an earlier mauve_seed_mums stays fetchable.
        MAUVE_ERR_ARG: null pointers, a bad pattern, seq out of range, max_multi > MAUVE_REPEAT_MAX_MULT or < 2; MAUVE_ERR_STATE: no
        genomes set, a fetch with no repeat result in force; MAUVE_ERR_LIMIT: the genomes hold 2^31 bases or more together. ---- */
#define MAUVE_REPEAT_MAX_MULT MAUVE_MAX_SEQ
int mauve_repeat_matches(mauve_ctx *ctx, int seq, uint64_t pattern, int64_t min_multi, int64_t max_multi,
                         int64_t *n_matches, int64_t *n_starts);
int mauve_repeat_fetch(mauve_ctx *ctx, int64_t *length, int64_t *mult, int64_t *start_off, int64_t *starts);

/* ---- chaining: MultiplicityFilter + EliminateOverlaps + Aligner::align's LCB stage
        (IdentifyBreakpoints / ComputeLCBs_v2 / greedy breakpoint elimination /
        computeLCBAdjacencies_v2; mauveAligner.cpp:596,600,698; toGrimmFormat.cpp:51-79).
        Host-side (sequential by nature); inputs/outputs are host arrays. ------ */
int mauve_eliminate_overlaps(int nseq, int64_t *n_inout, int64_t *length, int64_t *start);
/* one finder fed by the searches of several seeds (progressiveMauve.cpp:502-546: umf.FindMatches per seed of the family,
   longest first, then umf.GetMatchList): list a, then the matches of b that no match of a contains (same components,
   strands and diagonal), in canonical order.  Two-phase like the other list calls: with len_out == NULL
   *n_out receives the size; with buffers, *n_out is their capacity on entry. */
int mauve_merge_matches(int nseq, int64_t n_a, const int64_t *len_a, const int64_t *start_a, int64_t n_b, const int64_t *len_b,
                        const int64_t *start_b, int64_t *n_out, int64_t *len_out, int64_t *start_out);
int mauve_lcb_chain(int nseq, int64_t n, const int64_t *length, const int64_t *start,
                    int64_t min_weight, int collinear, int64_t *match_lcb, int64_t *n_lcb_out,
                    int64_t *left_end, int64_t *right_end, int64_t *weight, int64_t *left_adj,
                    int64_t *right_adj);   /* per-LCB arrays sized for n entries * nseq */

/* ---- gapped DP: the GappedAligner seam (Aligner::SetGappedAligner, mauveAligner.cpp:674;
        MuscleInterface::Align, MatchRecord.h:311; CallMuscleFast, repeatoire.cpp:1262).
        Batch of n_iv intervals; interval i has nseq sequences given as 0..3 codes, concatenated in
        `codes` with offsets seq_off[i*nseq+g] .. seq_off[i*nseq+g+1].  Output: presence-mask
        columns (bit g = sequence g has a residue), col_off[n_iv+1], per-interval score.
        cols must hold seq_off[n_iv*nseq] entries. ------------------------------------------------ */
int mauve_dp_batch(mauve_ctx *ctx, int nseq, int64_t n_iv, const uint8_t *codes,
                   const int64_t *seq_off, const mauve_scoring *sc, uint32_t *cols,
                   int64_t *col_off, int64_t *score);
/* The same seam for long intervals (GappedAligner::SetMaxAlignmentLength, GappedAligner.h: the reference's aligners
   refuse what is longer; this one bands it): an interval whose longest sequence is above band_from runs every
   progressive step inside the band |j - floor(i*n/m)| <= 128 + |n-m| + (m+n)/64; the others in full. */
int mauve_dp_batch_banded(mauve_ctx *ctx, int nseq, int64_t n_iv, const uint8_t *codes,
                          const int64_t *seq_off, const mauve_scoring *sc, int64_t band_from,
                          uint32_t *cols, int64_t *col_off, int64_t *score);

/* ---- extant sum-of-pairs score of ungapped matches: the anchor score behind ProgressiveAligner::setLcbScoringScheme(
        ExtantSumOfPairsScoring) (progressiveMauve.cpp:611-625; libMems-internal, frozen form DESIGN.md S11): for every column of a
        match and every pair of its components, the substitution score of the two bases.  length[n], start[n*nseq] signed
        1-based on the resident genomes, scores[n] out. ---- */
int mauve_match_sp_scores(mauve_ctx *ctx, int64_t n, const int64_t *length, const int64_t *start, const mauve_scoring *sc,
                          int64_t *scores);

/* ---- repeat penalty: the libMems global penalize_repeats that progressiveMauve sets from --repeat-penalty=<negative|zero>
        (progressiveMauve.cpp:295,606-609; libMems-internal, frozen form DESIGN.md S11d).  The mode is held by the context (it
        survives mauve_set_genomes*) and applies wherever sum-of-pairs LCB scoring is in force (lcb_scoring = MAUVE_LCB_SCORE_SP in
        mauve_align, mauve_align_matches, mauve_align_begin* and at every node of mauve_progressive_align*): a positive pair score S
        of a column becomes S*(2-r)/r (NEGATIVE) or S/r (ZERO), r = the larger base multiplicity of the two positions.  Default
        MAUVE_REPEAT_PENALTY_OFF: every result as without this call.  An unknown mode is MAUVE_ERR_ARG. ---- */
int mauve_set_repeat_penalty(mauve_ctx *ctx, int mode);
/* Base multiplicity of one resident genome (the repeat count RepeatHash-style k-mer counting gives a position; S11d): for every
   0-based position p the minimum, over the valid windows of `pattern` covering p, of the number of valid windows of the genome with
   the same canonical mer (both strands), saturated at 255; 1 where no valid window covers p.  mult: lens[seq] bytes.  Arguments
   and errors as mauve_sorted_mer_list. */
int mauve_seed_multiplicity(mauve_ctx *ctx, int seq, uint64_t pattern, uint8_t *mult);
/* mauve_match_sp_scores with the repeat penalty of `mode` (multiplicities of `pattern`, S11d); mode MAUVE_REPEAT_PENALTY_OFF
   returns exactly mauve_match_sp_scores.  The context's own mode is neither read nor changed. */
int mauve_match_sp_scores_repeat(mauve_ctx *ctx, uint64_t pattern, int mode, int64_t n, const int64_t *length, const int64_t *start,
                                 const mauve_scoring *sc, int64_t *scores);

/* ---- whole path: doAlignment's hot section (mauveAligner.cpp:523-531,585,629-698,746-760):
        multi-MUMs -> N-way filter -> overlap elimination -> LCBs -> recursive anchoring -> gapped
        alignment of every inter-anchor interval -> interval table.  Results are held by the context
        until the next call; fetch them with mauve_align_fetch.  Any fetch pointer may be NULL. ---- */
int mauve_align(mauve_ctx *ctx, const mauve_params *p, mauve_align_sizes *sizes);
/* The same with the match list the caller holds (Aligner::align(MatchList&, ...), mauveAligner.cpp:698: the list may come
   from a file, mauveAligner.cpp:484-503, or from a finder of the caller's own): no seed pass; the N-way matches of the
   list (all nseq starts non-zero; the others are ignored) are put in canonical order, overlap-eliminated and chained.
   length[n], start[n*nseq] signed 1-based. */
int mauve_align_matches(mauve_ctx *ctx, const mauve_params *p, int64_t n, const int64_t *length, const int64_t *start,
                        mauve_align_sizes *sizes);
/* The same resumed from LCBs the caller holds (an IntervalList read back from the .mln file of an earlier run, mauveAligner.cpp:
   705-722 --lcb-input; the matches of one LCB given to Aligner::align again, :723-744 --realign-lcb): anchor i has length[i],
   start[i*nseq + g] (signed 1-based, a component in every genome, forward in genome 0) and belongs to LCB lcb[i] (ids 0 .. n_lcb-1).
   The anchors of an LCB must form one collinear, overlap-free chain.  No seed pass, no overlap / breakpoint elimination, no LCB
   extension: recursive anchoring (p->recursive) and the gapped alignment of every inter-anchor interval (p->gapped) run as in
   mauve_align; n_mums of the result is 0. */
int mauve_align_lcbs(mauve_ctx *ctx, const mauve_params *p, int64_t n, const int64_t *length, const int64_t *start, const int64_t *lcb,
                     mauve_align_sizes *sizes);
int mauve_align_fetch(mauve_ctx *ctx,
                      int64_t *mum_length, int64_t *mum_start,            /* [n_mums], [n_mums*nseq] */
                      int64_t *lcb_left, int64_t *lcb_right, int64_t *lcb_weight, /* [n_lcb*nseq] x2, [n_lcb] */
                      int64_t *anchor_length, int64_t *anchor_start, int64_t *anchor_lcb,
                      int64_t *iv_left, int64_t *iv_right, int8_t *iv_reverse,   /* [n_iv*nseq] */
                      int64_t *col_off, uint32_t *cols, int64_t *dp_score);     /* [n_iv+1],[n_cols],[n_iv] */
/* The same result in the narrowest types that hold it (no reference counterpart: libMems hands out objects; this is what a caller that
   wants the arrays moves).  cols: col_bytes bytes per column (1: up to 8 genomes, 2: up to 16, 4: any; MAUVE_ERR_ARG when a column does not
   fit); match and anchor tables as int32 (every genome holds fewer than 2^31 bases, MAUVE_MAX_GENOME_LEN, so every start and length fits); the small per-LCB and
   per-interval tables as in mauve_align_fetch.  From page-locked buffers (mauve_host_alloc) the bulk arrays are narrowed on the device and
   copied once; any pointer may be NULL.  mauve_align_fetch is unchanged. */
int mauve_align_fetch_compact(mauve_ctx *ctx, int col_bytes,
                              int32_t *mum_length, int32_t *mum_start,
                              int64_t *lcb_left, int64_t *lcb_right, int64_t *lcb_weight,
                              int32_t *anchor_length, int32_t *anchor_start, int32_t *anchor_lcb,
                              int64_t *iv_left, int64_t *iv_right, int8_t *iv_reverse,
                              int64_t *col_off, void *cols, int64_t *dp_score);
/* Optional, before mauve_align: where that call may leave the two bulk tables of its result, in the types of mauve_align_fetch_compact, while
   it is still running (no reference counterpart).  The match list and the anchor table are final long before the pass ends -- the gapped
   alignment and the assembly follow -- so their copies run beside that work on a queue of their own instead of behind it in the fetch.
   All five pointers are page-locked (mauve_host_alloc); mum_cap and anchor_cap are the capacities in records (mum_length[mum_cap],
   mum_start[mum_cap * nseq], anchor_length[anchor_cap], anchor_start[anchor_cap * nseq], anchor_lcb[anchor_cap]).  One shot: it holds for
   the next mauve_align only, whatever path that call takes.  A table whose pointers are NULL or pageable, whose capacity is too small for
   the result, or that the call's path does not keep on the device (host chains, recursion into gaps, score-weighted LCBs) is simply not sent:
   nothing fails, and mauve_align_fetch_compact copies it as it always did.  A table that was sent is in place when mauve_align returns; a
   following mauve_align_fetch_compact that passes the same pointers skips its copy (any other pointer gets a copy from the device as before).
   The buffers must not be written or freed between this call and that fetch, or the next call on the context if no fetch follows. */
int mauve_align_prefetch(mauve_ctx *ctx, int32_t *mum_length, int32_t *mum_start, int64_t mum_cap,
                         int32_t *anchor_length, int32_t *anchor_start, int32_t *anchor_lcb, int64_t anchor_cap);
/* ---- the same path in three phases, for sharding the gapped alignment of ONE alignment over several GPUs
        (mauveAligner.cpp:130-131 --realign-lcb "for parallelization of LCB alignment").  Every rank
        calls mauve_align_begin (deterministic: identical anchors and interval table everywhere), aligns its
        share of the n_dp intervals with mauve_align_dp (indices into the interval table; outputs compact, in
        idx order: cols needs sum of max_cols over idx, col_off n+1, score n), exchanges the columns (one
        all_gather, mauvealigner_amd/parallel.py) and calls mauve_align_finish with the columns of ALL
        intervals in table order.  mauve_align_dp_cost gives per-interval DP cells (for LPT packing) and the
        column capacity each interval needs. ------------------------------------------------------------- */
int mauve_align_begin(mauve_ctx *ctx, const mauve_params *p, int64_t *n_dp, int64_t *n_codes);
int mauve_align_begin_matches(mauve_ctx *ctx, const mauve_params *p, int64_t n, const int64_t *length, const int64_t *start,
                              int64_t *n_dp, int64_t *n_codes);            /* mauve_align_begin on the caller's match list */
int mauve_align_dp_cost(mauve_ctx *ctx, int64_t *cost, int64_t *max_cols);
/* the two anchors that flank every DP interval, records of (1 + nseq): length, signed starts -- what a GappedAligner
   other than the built-in one is called with (GappedAligner::Align(cr, left match, right match, seq_table),
   MatchRecord.h:311): left[n_dp*(1+nseq)], right[n_dp*(1+nseq)] */
int mauve_align_dp_anchors(mauve_ctx *ctx, int64_t *left, int64_t *right);
int mauve_align_dp(mauve_ctx *ctx, const int64_t *idx, int64_t n, uint32_t *cols, int64_t *col_off,
                   int64_t *score, int64_t *cells);
int mauve_align_finish(mauve_ctx *ctx, const uint32_t *cols, const int64_t *col_off, const int64_t *score,
                       int64_t cells, mauve_align_sizes *sizes);
/* ---- the same work spread over several contexts, one per GPU, without splitting the call: every rank holds the same genomes and
        makes the SAME calls (mauve_align, mauve_progressive_align, mauve_guide_tree); inside them the independent units SURVEY.md 8e
        names -- the pairwise finder passes of the guide tree (progressiveMauve.cpp:490-501), the gaps of every recursion level
        (mauveAligner.cpp:130-131: "for parallelization of LCB alignment"), the gapped-alignment intervals of a guide-tree node --
        are LPT-partitioned over the ranks, each rank works on its share, and the (small) results are exchanged through the
        caller's all-gather, so that every rank ends with the whole result, bit-identical to a single context's.  The seed pass
        over the whole genomes and the breakpoint elimination are not partitioned (every rank runs them).
        allgather(user, send, send_bytes, &recv, recv_bytes[world]): blocking; on return *recv points to the contributions of all
        ranks one behind the other in rank order (valid until the next call), recv_bytes[r] their sizes; returns 0 on success.
        world <= 1 or fn == NULL switches the sharding off. ---- */
typedef int (*mauve_allgather_fn)(void *user, const void *send, int64_t send_bytes, const void **recv, int64_t *recv_bytes);
int mauve_set_shard(mauve_ctx *ctx, int rank, int world, mauve_allgather_fn fn, void *user);
/* The same with RCCL inside the library: nccl_comm is the caller's ncclComm_t (one rank per GPU, created with ncclCommInitRank on the context's
   device).  Every exchange is one ncclAllGather of the ranks' sizes and one of the padded payloads, issued by the library on its own stream
   between device buffers; nothing goes through a callback.  RCCL is resolved at this call from what the process has loaded (the librccl the
   caller's communicator comes from; librccl.so.1 is opened if none is), so the library itself does not link it.  world == 1 switches the
   sharding off like mauve_set_shard (with MAUVE_SHARD_SINGLE set the one rank still runs every exchange: a single-GPU rehearsal of the path).
   mauve_shard_get_stats: exchanges, bytes sent and received, and milliseconds spent in them since the collective was set. */
int mauve_set_shard_rccl(mauve_ctx *ctx, int rank, int world, void *nccl_comm);
typedef struct { int64_t exchanges, bytes_sent, bytes_received; double ms; } mauve_shard_stats;
int mauve_shard_get_stats(mauve_ctx *ctx, mauve_shard_stats *out);

/* ---- progressiveMauve path: guide tree + ProgressiveAligner::align(seq_table, interval_list)
        (progressiveMauve.cpp:575-710; distance matrix / guide tree mauveAligner.cpp:616-623).  Frozen replacement
        ("guide-tree recursive anchoring"): UPGMA over pairwise-match coverage; the root aligns
        what all genomes share, every node below aligns -- among its own genomes -- the bases no ancestor has
        placed.  tree_left/right: [2*nseq-1] child ids (-1 for leaves, internal ids nseq.. in merge order);
        dist: [nseq*nseq] distances in parts per million; any of them may be NULL.  The result is fetched with
        mauve_align_fetch / mauve_write_xmfa: intervals with >= 2 genomes first (n_lcb of them), then the
        single-genome leftovers; absent genomes have left = right = 0. ------------------------------------- */
int mauve_guide_tree(mauve_ctx *ctx, uint64_t pattern, int64_t *dist, int32_t *tree_left, int32_t *tree_right);
/* The pairwise breakpoint estimate behind ProgressiveAligner::setBreakpointDistanceScale / setBpDistEstimateMinScore
   (progressiveMauve.cpp:628-642; the estimate is libMems-internal, frozen form DESIGN.md S11c): for every genome pair, the
   adjacencies between its pairwise matches of length >= min_len (ordered along the lower genome) that are not conserved
   in the other genome.  bp: [nseq*nseq], symmetric, zero diagonal. */
int mauve_breakpoint_counts(mauve_ctx *ctx, uint64_t pattern, int64_t min_len, int64_t *bp);
int mauve_progressive_align(mauve_ctx *ctx, const mauve_params *p, mauve_align_sizes *sizes,
                            int32_t *tree_left, int32_t *tree_right, int64_t *dist);
/* ProgressiveAligner::setInputGuideTreeFileName (progressiveMauve.cpp:689-690): the same alignment along the caller's
   tree instead of the UPGMA one.  tree_left/right: [2*nseq-1] in the form mauve_guide_tree returns -- leaves 0..nseq-1
   with -1, every internal node with two distinct children of smaller id, root last; anything else is MAUVE_ERR_ARG. */
int mauve_progressive_align_tree(mauve_ctx *ctx, const mauve_params *p, mauve_align_sizes *sizes,
                                 const int32_t *tree_left, const int32_t *tree_right);
/* ---- backbone and islands: detectBackbone(iv_list, bb_list, &BigGapsDetector(island_gap_size)) of applyBackbone
        (progressiveMauve.cpp:226-260, --island-gap-size :268) and simpleFindIslands / simpleFindBackbone
        (mauveAligner.cpp:822,844-845).  libMems-internal; frozen form DESIGN.md S12: per genome pair, a run of more
        than island_gap_size columns in which only one of the two has residues is an island; the pair is joined
        outside the gap regions that hold an island or touch an end of the interval; a backbone segment is a connected
        component (>= 2 genomes) of the joined pairs over a maximal run of columns.
        mauve_backbone works on the alignment the context holds (after mauve_align* / mauve_progressive_align*, columns
        still in HBM); mauve_backbone_alignment on the caller's (--apply-backbone, progressiveMauve.cpp:367-385).
        Fetch: seg_iv/seg_col/seg_len[n_seg] (interval, first column in it, columns), seg_mask[n_seg] genomes,
        seg_left/seg_right[n_seg*nseq] signed ends (negative = reverse strand, 0 = not in the segment);
        islands[n_islands*8]: interval, a, b (a < b), the genome that has the residues, first column, last column,
        its signed left and right end.  Order: interval, column, genome set / pair.  Any pointer may be NULL. ---- */
int mauve_backbone(mauve_ctx *ctx, int64_t island_gap_size, int64_t *n_seg, int64_t *n_islands);
int mauve_backbone_alignment(mauve_ctx *ctx, int nseq, int64_t n_iv, const int64_t *left, const int64_t *right,
                             const int8_t *reverse, const int64_t *col_off, const uint32_t *cols,
                             int64_t island_gap_size, int64_t *n_seg, int64_t *n_islands);
/* The homology pass in front of the backbone: detectAndApplyBackbone(iv_list, bb_list, hmm_params) (progressiveMauve.cpp:226-243; its
   HomologyHMM is libMems-internal, frozen form DESIGN.md S12b).  A two-state Viterbi path (homologous / unrelated) per interval and
   genome pair over the resident alignment's columns, in integer log-odds x 1000; residues that are homologous to no other genome of
   their column move to columns of their own.  The context's alignment is rewritten in place (column count and offsets change: *sizes
   receives the new sizes for mauve_align_fetch); n_moved = residues taken out of multi-genome columns.  Call before mauve_backbone. */
typedef struct { int32_t match, mismatch, gap, go_homologous, go_unrelated; } mauve_hmm_params;
/* the call site's knobs (progressiveMauve.cpp:319-322: identity 0.7, pgh 1e-5, pgu 1e-9) as integer scores: match = 1000 ln(id / .25),
   mismatch = 1000 ln((1 - id) / .75), gap = -500, transitions = 1000 ln(p).  identity outside (0.25, 1) or a probability outside (0, 1]
   has no such score: *h then carries positive transition scores, which mauve_apply_homology* refuse with MAUVE_ERR_ARG */
void mauve_hmm_params_from(double identity, double pgh, double pgu, mauve_hmm_params *h);
int mauve_apply_homology(mauve_ctx *ctx, const mauve_hmm_params *h, mauve_align_sizes *sizes, int64_t *n_moved);
/* ... of the caller's alignment (the genomes it refers to are the context's): cols_out holds up to one column per residue, col_off_out [n_iv+1].
   The column array must be consistent with the interval table -- right - left + 1 residues of every present genome, none of an absent one, no bit
   at or above nseq -- or the call returns MAUVE_ERR_ARG (mauve_backbone_alignment checks the same) */
int mauve_apply_homology_alignment(mauve_ctx *ctx, int nseq, int64_t n_iv, const int64_t *left, const int64_t *right, const int8_t *reverse,
                                   const int64_t *col_off, const uint32_t *cols, const mauve_hmm_params *h, int64_t *col_off_out, uint32_t *cols_out,
                                   int64_t *n_moved);
int mauve_backbone_fetch(mauve_ctx *ctx, int64_t *seg_iv, int64_t *seg_col, int64_t *seg_len, uint32_t *seg_mask,
                         int64_t *seg_left, int64_t *seg_right, int64_t *islands);
/* ---- coordinate translation through the alignment: Interval::GetColumn as coordinateTranslate uses it (coordinateTranslate.cpp:36-46)
        and CompactGappedAlignment::SeqPosToColumn (getOrthologList.cpp:219-220, bbBreakOnGenes.cpp:154-155, randomGeneSample.cpp:139-140,
        scoreProcrastAlignment.cpp:293-303), batched on a rank/select index over the columns.  Frozen form DESIGN.md S14: genome g is
        present in interval i iff left[i,g] != 0; its residue with ordinal k in column order sits at left + k, at right - k on the
        reverse strand, and is reported signed (negative = reverse strand).
        Index: mauve_coord_index takes the alignment the context holds (MAUVE_ERR_STATE without one), mauve_coord_index_alignment the
        caller's, in the arrays of mauve_align_fetch; the columns must be consistent with the interval ends (as for
        mauve_backbone_alignment) and every base of a genome may lie in at most one interval, else MAUVE_ERR_ARG (the text names the
        two intervals).  The index is a snapshot with device buffers of its own: later seed passes, alignments and genome uploads
        leave it valid, the next index call replaces it, the context's end frees it.  After mauve_apply_homology it still describes
        the columns it was built from until it is built again.  mauve_coord_index_size tells what the index in force was built from
        (genomes, intervals, columns: the answer arrays are sized by its nseq); any pointer may be NULL.
        Queries (MAUVE_ERR_STATE without an index; n = 0 is MAUVE_OK) are host arrays, page-locked ones (mauve_host_alloc) are copied
        directly; any output pointer may be NULL.
        mauve_column_positions: for (iv[q], col[q]) pos[q*nseq + g] = 0 for an absent genome, the signed position of the residue in
          the column where bit g is set (then bit g of defined[q] too); where g is gapped 0, or with nearest != 0 the residue before
          the column, else the first one after it (the defined bit stays clear).
        mauve_seqpos_to_column: for (seq[q], pos[q]), pos 1-based and unsigned, the interval that covers the base and the column in it
          that holds it; (-1, -1) where no interval does (add_unaligned = 0 leaves bases out: a legal question).
        mauve_translate_positions: the two in turn -- nseq signed positions (entry seq[q] is +-pos[q]), the defined mask, the interval;
          zeros, 0 and -1 where nothing covers the base.
        An interval id outside [0, n_iv), a column outside its interval, seq outside [0, nseq) or pos < 1 makes the whole call return
        MAUVE_ERR_ARG. ---- */
int mauve_coord_index(mauve_ctx *ctx);
int mauve_coord_index_alignment(mauve_ctx *ctx, int nseq, int64_t n_iv, const int64_t *left, const int64_t *right,
                                const int8_t *reverse, const int64_t *col_off, const uint32_t *cols);
int mauve_coord_index_size(mauve_ctx *ctx, int *nseq, int64_t *n_iv, int64_t *n_cols);
int mauve_column_positions(mauve_ctx *ctx, int64_t n, const int64_t *iv, const int64_t *col, int nearest,
                           int64_t *pos /* n*nseq */, uint32_t *defined /* n */);
int mauve_seqpos_to_column(mauve_ctx *ctx, int64_t n, const int32_t *seq, const int64_t *pos,
                           int64_t *iv /* n */, int64_t *col /* n */);
int mauve_translate_positions(mauve_ctx *ctx, int64_t n, const int32_t *seq, const int64_t *pos, int nearest,
                              int64_t *out /* n*nseq */, uint32_t *defined /* n */, int64_t *iv /* n */);
/* ---- alignment columns as a base matrix: the GetAlignment loops of stripGapColumns (stripGapColumns.cpp:32-64), projectAndStrip
        (projectAndStrip.cpp:75-101), stripSubsetLCBs (stripSubsetLCBs.cpp:125-142), createBackboneMFA (createBackboneMFA.cpp:28-37) and
        alignmentProjector (alignmentProjector.cpp:58-77) -- choose columns, choose rows, write the letters -- on the coordinate index in
        force and the resident genomes.  Frozen form DESIGN.md S15.  The cell of a column and a genome is '-' where the genome is absent
        from the interval or gapped in the column, else the base at the signed position of S14 ("ACGT", complemented on the reverse
        strand, N where the ambiguity bitmap is set): the letter mauve_write_xmfa prints there.
        Request: keep[0..n_keep) distinct genome ids = the rows, in that order (the projection list); require: genome mask, a column is
        selected only if all of them have a residue (require = the keep set: the core columns); drop_empty: ... and only if a kept genome
        has one; polymorphic: ... and only if the kept genomes' ACGT cells show two different letters (N and '-' do not count).
        Ranges (range_iv, range_col, range_len)[n_range]: the form of seg_iv / seg_col / seg_len of mauve_backbone_fetch; range_iv == NULL:
        one range per interval, all its columns (n_range is then not read).  Selected columns come in range order, ascending inside a
        range; overlapping ranges repeat columns; empty ranges and n_range = 0 are legal.
        mauve_extract_select makes the selection (*n_sel columns) and keeps it in the context; mauve_extract_fetch writes
        rows[k*row_stride + j] = the cell of keep[k] and selected column j (row_stride >= n_sel; the bytes between n_sel and row_stride
        are not written), sel_iv / sel_col [n_sel] in the form mauve_column_positions takes, range_off [n_range+1] = every range's slice
        of the selection.  Any output pointer may be NULL; page-locked ones (mauve_host_alloc) are copied directly.
        MAUVE_ERR_ARG: an interval id outside [0, n_iv), col < 0, len < 0, col + len past the interval, n_keep outside [1, nseq], a keep
        id outside [0, nseq) or repeated, a require bit at or above nseq, an interval of the index that ends beyond the resident genome.
        MAUVE_ERR_STATE: no index, an index of another nseq than the context's, an index built before the last mauve_set_genomes*;
        a fetch without a selection -- a later mauve_coord_index*, mauve_set_genomes* or select ends the one before. ---- */
typedef struct { int32_t n_keep; int32_t keep[MAUVE_MAX_SEQ]; uint32_t require; int32_t drop_empty; int32_t polymorphic; } mauve_extract_params;
void mauve_default_extract_params(int nseq, mauve_extract_params *p);        /* every genome in order, no condition */
int mauve_extract_select(mauve_ctx *ctx, const mauve_extract_params *p, int64_t n_range, const int64_t *range_iv,
                         const int64_t *range_col, const int64_t *range_len, int64_t *n_sel);
int mauve_extract_fetch(mauve_ctx *ctx, char *rows, int64_t row_stride,       /* rows[k*row_stride + j], row_stride >= n_sel */
                        int64_t *sel_iv, int64_t *sel_col, int64_t *range_off); /* [n_sel], [n_sel], [n_range+1]; any may be NULL */
/* ---- pairwise column statistics of the alignment: IdentityMatrix behind --lcb-stats (mauveAligner.cpp:784-800,
        calculateBackboneCoverage.cpp:106-127), BackboneIdentityMatrix (pairCompare.cpp:57-60,77, calculateBackboneCoverage2.cpp:98-121), the
        pairwise loop of gappiness (gappiness.cpp:33-50) and computeSPScore (multiEVD.cpp:41-46, repeatoire.cpp:2527) -- what two rows show
        against each other, counted on the coordinate index in force and the resident genomes.  Frozen form DESIGN.md S16.  The cell of a
        genome in a column is the S15 cell; letter codes A, C, G, T, N -> 0..4.
        A record is MAUVE_PAIR_STATS_WORDS int64_t for one ordered pair (a, b) over one range, with x the cell of a and y the cell of b:
          [5*code(x) + code(y)], 0..24  columns where both have a residue
          [25] only_a  x is a residue, y is '-'            [26] only_b  x is '-', y is a residue
          [27] runs_a  the columns of [25] whose predecessor is missing or no only_a column; [28] runs_b the same for [26]
          [29] neither both '-'                            [30], [31] 0
        The predecessor is the nearest earlier column of the same range that is not a `neither` column (computeSPScore's run rule: two
        gaps neither score nor interrupt a run, two residues end it, every range starts with no run open).  Slots 0..26 and 29 sum to
        the range's length; the pair (b, a) is the transposed table with 25 <-> 26 and 27 <-> 28.
        Pairs: pair_a == NULL: all nseq(nseq-1)/2 pairs a < b, row-major in the upper triangle (n_pair and pair_b are not read); else
        1 <= n_pair <= 1024 ordered pairs, duplicates allowed.  Ranges: as for mauve_extract_select (range_iv == NULL: one range per
        interval, all its columns; n_range = 0 and empty ranges are legal and give zeros).
        stats: per_range = 0: [n_pair][32], every pair's sum of its per-range records (overlapping ranges count twice, runs do not cross a
        range boundary); per_range != 0: [n_range][n_pair][32].  Page-locked stats (mauve_host_alloc) are copied directly.  All counts are
        integers and independent of any tiling: two calls return identical bytes.  The call neither needs nor disturbs the extract
        selection in force.
        MAUVE_ERR_ARG: n_pair outside [1, 1024], a == b or an id outside [0, nseq), and the range errors of mauve_extract_select;
        MAUVE_ERR_LIMIT: more than 2^24 records; MAUVE_ERR_STATE: as for mauve_extract_select.
        Derived on the host, without a context, for n_rec records:
        mauve_pair_stats_identity: (s[0] + s[6] + s[12] + s[18] + s[24]) / the sum of s[0..24], 0.0 when that sum is 0 (IdentityMatrix's
          rule: N against N counts as equal there too);
        mauve_pair_stats_sp_score: the sum of s[5x+y] * matrix[x'][y'] + gap_open * (s[27] + s[28]) + gap_extend * (s[25] + s[26] - s[27] - s[28]),
          N scoring as A (x' = x < 4 ? x : 0): the pair's share of computeSPScore of the range's rows. ---- */
#define MAUVE_PAIR_STATS_WORDS 32
int mauve_pair_stats(mauve_ctx *ctx, int64_t n_pair, const int32_t *pair_a, const int32_t *pair_b,
                     int64_t n_range, const int64_t *range_iv, const int64_t *range_col, const int64_t *range_len,
                     int per_range, int64_t *stats);
void mauve_pair_stats_identity(const int64_t *stats, int64_t n_rec, double *identity);
void mauve_pair_stats_sp_score(const int64_t *stats, int64_t n_rec, const mauve_scoring *sc, int64_t *score);
/* ---- excursions of the column scores: the state machine of getLocalRecordHeights in evd and multiEVD (evd.cpp:12-66, multiEVD.cpp:29-79),
        whose sorted heights are the thresholds libMems' backbone detection is calibrated with, as a scan on the coordinate index in force
        and the resident genomes.  Frozen form DESIGN.md S18.  The cell of a genome in a column is the S15 cell, the letter codes are those
        of S16, N scores as A; sc == NULL: mauve_default_scoring.  All sums are int64_t.
        A stream is the columns of one range, ascending, that one set keeps, each with a score s:
          pair stream (ordered pair (a, b)): the columns in which a or b has a residue; s = matrix[x'][y'] where both have one, else gap_open
            where the column opens a run by S16's rule (slots 27 / 28: the nearest earlier column of the same range that is not `neither`
            is missing or of another kind), else gap_extend;
          core stream (genome mask m of at least two genomes): the columns in which every genome of m has a residue (S15's require = m); s =
            the sum over the pairs g < h of m of matrix[x'_g][x'_h].  A genome of m that is absent from the interval makes the stream empty.
        The walk: v = -s, x = 0, h = 0; per column the first rule that matches: (1) x > 0 and x + v < 0: the record (h, this column), then
        x = 0, h = 0; (2) x == 0 and v > 0: x = v, h = max(h, x); (3) x > 0: x += v, h = max(h, x); (4) nothing.  Nothing is recorded at the
        stream's end; (x, h) there is the stream's tail.  An excursion that returns to exactly 0 is not ended: its height carries into the
        next rise (the tool's loop).
        Pairs and ranges: as for mauve_pair_stats.  group_mask == NULL: one group of every genome (n_group is not read); else
        1 <= n_group <= 1024 masks.  Streams are numbered range-major: stream = r * n_set + k.
        The first two calls compute everything, keep it in the context and tell the number of records; mauve_excursions_fetch writes
        height[n_exc], end_col[n_exc] (the column inside the range's interval, in the form mauve_column_positions takes), stream_off
        [n_stream + 1] and tail[n_stream][2] = (x, h).  Within a stream the records come in column order.  Any output pointer may be NULL;
        page-locked ones (mauve_host_alloc) are copied directly.  Records are placed by scanned offsets and nothing depends on the tiling:
        two calls return identical bytes.  The calls neither need nor disturb the extract selection in force.
        MAUVE_ERR_ARG: n_pair or n_group outside [1, 1024], a == b or an id outside [0, nseq), a mask of fewer than two genomes or with a
        bit at or above nseq, and the range errors of mauve_extract_select; MAUVE_ERR_LIMIT: more than 2^24 streams, or sets x chunks of 2^31 or more; MAUVE_ERR_STATE: as
        for mauve_extract_select; a fetch without a result -- the next excursions call, mauve_coord_index* or mauve_set_genomes* ends it.
        Work is cut into chunks of MAUVE_EXCURSION_CHUNK columns, counted from the 64-column word of the index that holds a range's first
        column; the figure is public for tests and sizing only, no result depends on it.
        mauve_excursion_thresholds, on the host and without a context: for the fractions .95, .99, .999 and .9999 of the sorted heights
        threshold[q] = the height at index min((size_t)(n * f), n - 1) and above[q] = n minus that index (evd.cpp:108-126, in double);
        zeros for n = 0. ---- */
#define MAUVE_EXCURSION_CHUNK 512
int mauve_excursions_pairs(mauve_ctx *ctx, const mauve_scoring *sc, int64_t n_pair, const int32_t *pair_a, const int32_t *pair_b,
                           int64_t n_range, const int64_t *range_iv, const int64_t *range_col, const int64_t *range_len, int64_t *n_exc);
int mauve_excursions_core(mauve_ctx *ctx, const mauve_scoring *sc, int64_t n_group, const uint32_t *group_mask,
                          int64_t n_range, const int64_t *range_iv, const int64_t *range_col, const int64_t *range_len, int64_t *n_exc);
int mauve_excursions_fetch(mauve_ctx *ctx, int64_t *height, int64_t *end_col, int64_t *stream_off, int64_t *tail /* n_stream*2 */);
void mauve_excursion_thresholds(const int64_t *height, int64_t n, int64_t threshold[4], int64_t above[4]);
/* ---- the alignment projected onto a subset of the genomes, what becomes collinear coalesced into new intervals: libMems'
        projectIntervalList (alignmentProjector.cpp:58-77, multiEVD.cpp:142-172, bbBreakOnGenes.cpp:54) and the loop projectAndStrip writes
        out by hand (projectAndStrip.cpp:75-122), on the coordinate index in force.  Frozen form DESIGN.md S19.  No genome data is read.
        Request: proj[0..n_proj) distinct genome ids, 1 <= n_proj <= nseq of the index (P = their set); drop_empty.
        (1) An interval is kept iff every genome of P is present in it; the others are dropped.  (2) A kept interval whose row proj[0] is
        reversed is flipped: its columns are taken in descending order and the strand of every row of P is toggled, the ends stay, so by
        S14's rule every column keeps its positions with the sign changed.  (3) The kept intervals are ordered by their left end in
        proj[0]; two consecutive ones A, B are collinear iff for every other g of P they have the same strand in g (after 2) and, among
        the kept intervals ordered by left end in g, B follows A directly (forward) or precedes it directly (reversed): the match_lcb
        labels of mauve_lcb_chain(n_proj, K, 1..., the signed left ends in proj order, 0, 0).  An output interval is a maximal collinear
        run; with n_proj = 1 everything kept is one run.  (4) Between two consecutive pieces A, B of a run, for k = 0..n_proj-1 in that
        order, genome proj[k] receives one run of d filler columns with its bit alone, d = its bases strictly between A and B (contig
        tables are not consulted): the output interval's ends are the least left and the greatest right end of its pieces and its columns
        hold right - left + 1 residues of every genome of P.  (5) The output keeps the wide form: bit g of a column is bit g of the source
        column for g in P, else 0; genomes outside P are absent from every output interval (left = right = 0).  With drop_empty the source
        columns in which no genome of P has a residue are left out, else they stay as zero masks.  The projection is thus an alignment of
        the same nseq: it can become the index in force and S14 to S18 run on it unchanged.  (6) Provenance: output interval o is made of
        the source intervals src_iv[src_off[o] .. src_off[o+1]) in column order, src_flip[] tells which were flipped; src_col[] is every
        output column's source column in the whole column array of the index, -1 for a filler column.
        mauve_project computes the projection into device buffers of the context and keeps the small tables on the host; *sz (may be NULL):
        output intervals, columns, source pieces (entries of src_iv), filler columns.  No kept interval, or an index of no intervals:
        n_iv = 0, MAUVE_OK.
        mauve_project_fetch writes it in the arrays of mauve_align_fetch: left / right / reverse [n_iv * nseq], col_off [n_iv + 1], cols
        [n_cols], and src_off [n_iv + 1], src_iv / src_flip [n_src], src_col [n_cols].  With compact != 0 left / right / reverse are
        [n_iv * n_proj] in proj order and bit k of a column is genome proj[k] (alignmentProjector's output).  Any pointer may be NULL;
        page-locked destinations (mauve_host_alloc) are copied directly.  Nothing depends on the tiling: two calls return identical bytes.
        mauve_project_index makes the projection the index in force without a column crossing the host link; it ends the extract selection
        and the excursion result, as mauve_coord_index does; the projection stays fetchable.
        MAUVE_ERR_ARG: n_proj outside [1, nseq], an id outside [0, nseq) or repeated.  MAUVE_ERR_STATE: no index; a fetch or
        mauve_project_index without a projection; mauve_project_index when the projection is of another nseq than the context's or the
        genomes were replaced after its index was built.  A call refused for these reasons leaves the index usable; once
        mauve_project_index has begun the build, a failure of the build itself (MAUVE_ERR_LIMIT: the projection is too large for an index;
        MAUVE_ERR_HIP) leaves the context without an index, as a failed mauve_coord_index* does.  A later mauve_project ends the earlier
        projection whether it succeeds or not.  src_col is made by the first fetch that asks for it (from what the projection left on the
        device: the index may have been replaced since); a caller who never asks never pays for it. ---- */
typedef struct { int32_t n_proj; int32_t proj[MAUVE_MAX_SEQ]; int32_t drop_empty; } mauve_project_params;
typedef struct { int64_t n_iv, n_cols, n_src, n_fill; } mauve_project_sizes;
void mauve_default_project_params(int nseq, mauve_project_params *p);   /* every genome in order, drop_empty = 1 */
int mauve_project(mauve_ctx *ctx, const mauve_project_params *p, mauve_project_sizes *sz);
int mauve_project_fetch(mauve_ctx *ctx, int compact, int64_t *left, int64_t *right, int8_t *reverse, int64_t *col_off,
                        uint32_t *cols, int64_t *src_off, int64_t *src_iv, int8_t *src_flip, int64_t *src_col);
int mauve_project_index(mauve_ctx *ctx);
/* ---- annotated ranges mapped through the alignment, and the interval-overlap join behind them: the walk of getOrthologList
        (getOrthologList.cpp:137-313), randomGeneSample (randomGeneSample.cpp:118-157), bbBreakOnGenes (bbBreakOnGenes.cpp:140-160) and
        scoreProcrastAlignment (scoreProcrastAlignment.cpp:285-305) -- the intervals a range intersects, the range clipped to each,
        SeqPosToColumn on both ends, copyRange, LeftEnd / RightEnd of every row, the feature of every genome with the largest overlap --
        on the coordinate index in force.  Frozen form DESIGN.md S21.  No genome data is read.
        A query is (seq, lo, hi): positions 1-based and unsigned, 1 <= lo <= hi; hi may lie past the genome's end (the index does not know
        genome lengths) and is clipped.
        (a) The pieces of query q are the intervals of the index in which seq is present and whose [left, right] in seq shares a base with
        [lo, hi], in ascending order of their left end in seq.  A piece holds piece_query, piece_iv; clip_lo = max(lo, left), clip_hi =
        min(hi, right); piece_col, piece_len: the columns of clip_lo and clip_hi by S14's rule, relative to the interval -- piece_col the
        smaller of the two (on a reverse row they swap), piece_len their distance plus 1: a range in the form mauve_extract_select,
        mauve_pair_stats and mauve_excursions_* take.  For every genome g of the index n_res[p*nseq + g] = the residues of row g in those
        columns, ext_left / ext_right [p*nseq + g] = the smallest and the greatest position among them, both negative where the row is
        reversed in the interval (S14's sign); all three 0 where g is absent from the interval or has only gaps in the range.  For g = seq
        n_res = clip_hi - clip_lo + 1 and the extent is the clip.
        (b) Per query: piece_off [n + 1]; covered[q] = the sum of the clipped lengths; best[q] = the index, in the piece arrays, of the
        piece with the greatest clipped length, among equals the one with the greater interval id (the tool sorts (size, interval) pairs
        and takes the last, :200-206), -1 without pieces.  A query with more than one piece is what the tool flags as rearranged.
        mauve_map_ranges computes everything into device buffers of the context and tells the sizes (*sz may be NULL);
        mauve_map_ranges_fetch writes it; any output pointer may be NULL, page-locked ones (mauve_host_alloc) are copied directly, and
        so are page-locked query arrays.  The result stays until the next mauve_map_ranges, mauve_coord_index* or mauve_project_index ends
        it; it neither needs nor disturbs the extract selection, the excursion result or the projection.  Two calls return identical bytes.
        (c) mauve_range_overlaps is independent of any index and of the genomes: a table of m ranges (tab_seq, tab_lo, tab_hi) in any
        order -- entries may nest, overlap and repeat -- and n queries (q_seq, q_lo, q_hi), which may be signed: their absolute values
        are used and (0, 0) means "nothing", so a row of extents from (a) goes in as it is.  n_hit[q] = the table entries of the same
        genome that share at least one base with the query; best[q] = the table index of the entry sharing the most bases, among equals
        the greater table index (getOrthologList.cpp:250-273); overlap[q] = that number of bases; (0, -1, 0) for no hit.  The tool measures
        the overlap inside n-way backbone segments; this rule measures plain shared bases.  A table entry that spans its genome makes every
        query of that genome visit the genome's whole slice of the table: pass CDS-like features, as the tool does, not `source` features.
        MAUVE_ERR_ARG, for the whole call: seq outside [0, nseq), lo < 1, lo > hi; a table entry with lo < 1 or lo > hi; a table or
        query genome id of (c) outside [0, MAUVE_MAX_SEQ); a query of (c) with exactly one end 0, with ends of different sign, or with
        |lo| > |hi|.  MAUVE_ERR_LIMIT: a position of 2^31 or more, more than 2^24 queries or table entries, 2^31 pieces or more.
        MAUVE_ERR_STATE: no index (the first call), no result (the second).  n = 0 and m = 0 are MAUVE_OK.  A refused mauve_map_ranges
        leaves the index and every other result usable. ---- */
typedef struct { int64_t n_query, n_piece; } mauve_range_map_sizes;
int mauve_map_ranges(mauve_ctx *ctx, int64_t n, const int32_t *seq, const int64_t *lo, const int64_t *hi, mauve_range_map_sizes *sz);
int mauve_map_ranges_fetch(mauve_ctx *ctx, int64_t *piece_off /* n+1 */, int64_t *covered /* n */, int64_t *best /* n */,
                           int64_t *piece_query, int64_t *piece_iv, int64_t *piece_col, int64_t *piece_len, int64_t *clip_lo,
                           int64_t *clip_hi /* n_piece each */, int64_t *n_res, int64_t *ext_left, int64_t *ext_right /* n_piece*nseq each */);
int mauve_range_overlaps(mauve_ctx *ctx, int64_t m, const int32_t *tab_seq, const int64_t *tab_lo, const int64_t *tab_hi,
                         int64_t n, const int32_t *q_seq, const int64_t *q_lo, const int64_t *q_hi,
                         int64_t *n_hit, int64_t *best, int64_t *overlap /* n each */);
/* ---- an alignment scored against a correct one: scoreAlignment <correct alignment> <calculated alignment> (scoreAlignment.cpp:99-457),
        counted on two coordinate indices.  Frozen form DESIGN.md S17.  T is the correct alignment, loaded by the first call below; C, the
        calculated one, is the coordinate index in force (S14); both are over the same nseq genomes and follow S14's position rule.  No
        genome data is read: neither call needs resident genomes.
        For an ordered pair (i, j), i != j, and a base p of genome i that is a residue in some column of T: T_ij(p) is the position of j's
        residue in that column (none: j gapped there or absent from the interval); P_ij(p) is the position of j's residue in the column of
        C that holds base p of i (none: no interval of C covers p, j is absent from it, or j is gapped there); inside_ij(p): p lies in an
        interval of C in which j is present.  A record is MAUVE_SCORE_WORDS int64_t per ordered pair, every such base in exactly one slot:
          [0] tp            T_ij a base, P_ij the same base      [1] fp_base   T_ij a base, P_ij another base
          [2] fp_gap        T_ij a base, P_ij none, inside_ij    [3] fn_unaligned  T_ij a base, P_ij none, not inside_ij
          [4] fn_base       T_ij none, P_ij a base               [5] tn        both none            [6], [7] 0
        Slots 0..5 of record (i, j) sum to the residues genome i has in T; the diagonal records are zero.  Only positions are compared
        (the tool's test is cor_baseJ == +-calc_baseJ, :424-427).  A base whose intervals in C all lack j counts as fn_unaligned (the
        tool's "bad context" branch, :345-350, would call it FP).
        The first call takes the correct alignment in the arrays of the fetch, with the argument and consistency checks of the index of a
        caller's alignment (MAUVE_ERR_ARG, the text names the interval / the two overlapping intervals); positions of 2^31 or more:
        MAUVE_ERR_LIMIT.  It is a snapshot with device buffers of its own: index calls, alignments and genome uploads leave it as it is
        (one truth scores many calculated alignments), the next such call replaces it, the context's end frees it; it touches neither
        the index in force nor an extract selection.
        The second writes records[nseq * nseq][8], row-major (i, j); page-locked records are copied directly.  MAUVE_ERR_STATE: no
        truth, no index in force, or the two differ in nseq.  A truth without intervals or columns gives zeros.  All counts are integers
        and independent of any tiling: two calls return identical bytes.
        The third, on the host and without a context, gives the tool's totals: TP = the sum over i < j of [0], FP = over i < j of
        [1] + [2], FN = over i < j of [3] plus over all i != j of [4], TN = over all i != j of [5], unaligned_fn = over i < j of [3],
        total = the four. ---- */
#define MAUVE_SCORE_WORDS 8
typedef struct { int64_t tp, tn, fp, fn, total, unaligned_fn; } mauve_score_totals;
int mauve_score_truth(mauve_ctx *ctx, int nseq, int64_t n_iv, const int64_t *left, const int64_t *right, const int8_t *reverse,
                      const int64_t *col_off, const uint32_t *cols);
int mauve_score_alignment(mauve_ctx *ctx, int64_t *records /* nseq*nseq*8 */);
void mauve_score_totals_from(const int64_t *records, int nseq, mauve_score_totals *out);
/* ---- a repeat map scored against a correct alignment of the copies of its repeats: scoreProcrastAlignment <correct alignment>
        <calculated matches> (scoreProcrastAlignment.cpp:120-364, compareAlignmentsAceD), counted on the truth index of S17 and the
        component extents of the map.  Frozen form DESIGN.md S22.  No genome data is read: the call needs no resident genomes.
        T is the alignment loaded by mauve_score_truth, unchanged; here its nseq <= 32 rows are the copy slots of a repeat, an interval is
        one repeat family, and a residue of row r lies at genome position row_offset[r] + its position (row_offset NULL: zeros, the rows
        carry genome coordinates; non-zero: the tool's concat_coords, rows as the contigs of one concatenated sequence).
        C is a list in the layout of mauve_repeat_fetch -- length[n], mult[n], start_off[n + 1], starts[start_off[n]], signed 1-based
        starts, 2 <= mult <= MAUVE_REPEAT_MAX_MULT, ungapped: component c of record r covers [|start|, |start| + length - 1], is reverse
        iff its start is negative, and holds base q in column q - left (forward) or right - q (reverse).  length == NULL (mult, start_off
        and starts NULL too, n ignored) scores the result of the last mauve_repeat_matches where it lies on the device, in the order of
        mauve_repeat_fetch (its finishing of the groups of equal start 0 included); the starts are not brought to the host.
        A truth pair is two rows i < j with residues in one column of T, at genome positions q_i and q_j; same_T: the rows have the same
        reverse flag in that interval.  A triple (r, c1, c2), c1 != c2, supports the pair iff q_i lies in c1, q_j lies in c2 and
        (c1, c2 have the same sign) == same_T; exactly iff in addition q_i and q_j have the same column.  All combinations count (the
        components of a tandem record overlap).  The tool pairs the k-th elements of two set intersections (:256-283), which is arbitrary
        there; for an ungapped match its "an anchor intervenes" test (:291-316) always passes, so its figure is sp_truepos and sp_exact
        is the stricter one.
        totals: sp_possible = the truth pairs; sp_truepos / sp_exact = those with a supporting / an exactly supporting triple; components
        = the sum of mult, component_pairs = the sum of m (m - 1) / 2, components_hit and component_pairs_hit = the set bits of the two
        tables below.  pair_records[nseq * nseq * 4], row-major (i, j), filled for i < j: possible, truepos, exact, 0.  comp_hit[n]: bit c
        of word r is set iff c is c1 or c2 of a supporting triple (:318-321).  pair_hit[start_off[n]]: bit max(c1, c2) of word
        start_off[r] + min(c1, c2) (:323-335).  Any output but totals may be NULL; page-locked ones are copied directly, and so is a
        page-locked list.  All counts are integers and every update commutes: two calls return identical bytes.
        MAUVE_ERR_STATE: no truth; the resident form without a repeat result in force.  MAUVE_ERR_ARG, the text names the record: mult
        outside [2, 32], start_off not the prefix sum of mult, a zero start, length < 1; a negative row_offset.  MAUVE_ERR_LIMIT: a genome
        position of 2^31 or more, offset included; more than 2^24 records.  n = 0 and a truth without columns are MAUVE_OK and give zero
        counts (components is still the sum of mult).  The call leaves the truth, the index in force, the repeat result, the extract
        selection, the range map and the projection as they are.
        The second, on the host and without a context: sensitivity = sp_truepos / sp_possible, exact sensitivity = sp_exact /
        sp_possible, component PPV = components_hit / components, pairwise PPV = component_pairs_hit / component_pairs; 0 / 0 gives 0. ---- */
typedef struct { int64_t sp_possible, sp_truepos, sp_exact, components, components_hit, component_pairs, component_pairs_hit, reserved; } mauve_repeat_score_totals;
int mauve_repeat_score(mauve_ctx *ctx, int64_t n, const int64_t *length, const int64_t *mult, const int64_t *start_off,
                       const int64_t *starts, const int64_t *row_offset, mauve_repeat_score_totals *totals,
                       int64_t *pair_records /* nseq*nseq*4 */, uint32_t *comp_hit /* n */, uint32_t *pair_hit /* start_off[n] */);
void mauve_repeat_score_ppv(const mauve_repeat_score_totals *t, double out[4]);
/* IntervalList::WriteStandardAlignment (mauveAligner.cpp:746-760; format mfa2xmfa.cpp:64-115).
   Two-phase: buf == NULL returns the needed size (including NUL) in *len. */
int mauve_write_xmfa(mauve_ctx *ctx, const char *const *names, char *buf, int64_t *len);
/* ---- the alignment as text, written on the device: IntervalList::WriteStandardAlignment (mauveAligner.cpp:746-760), the per-LCB files
        of --output-alignment (mauveAligner.cpp:764-781) and the writing half of xmfa2maf (xmfa2maf.cpp:46-82), on the coordinate index in
        force and the resident genomes.  Frozen form DESIGN.md S23.  Unlike mauve_write_xmfa it writes whatever the index describes -- the
        context's result, a caller's alignment, a projection made the index in force -- and any column ranges of it.
        Blocks: one per range (range_iv, range_col, range_len)[n_range], the form and the checks of mauve_extract_select; range_iv == NULL:
        one per interval, all its columns.  They are written in the order given; overlapping ranges repeat text.
        Rows: genome g (ascending) has a row in a block iff it has a residue in the range; with k0 / k1 residues of its interval row in
        front of the range's first column / behind its last one, the row covers lo = left + k0 .. hi = left + k1 - 1, on the reverse
        strand hi = right - k0, lo = right - k1 + 1.  The cells are the S15 cells.  A block without a row is left out whole.
        MAUVE_TEXT_XMFA (wrap >= 1, default 80): "#FormatVersion Mauve1", per genome "#Sequence{g+1}File\t{names[g]}",
          "#Sequence{g+1}Entry\t{g+1}", "#Sequence{g+1}Format\tFastA"; per row "> {g+1}:{lo}-{hi} {+|-} {deflines[g]}" and the cells in
          lines of wrap; "=" behind a block's rows.  A NULL name is the empty string, deflines == NULL means names.  On whole intervals
          of the context's result with wrap 80 these are the bytes of mauve_write_xmfa, without its trailing NUL.
        MAUVE_TEXT_MAF (wrap = 0): "##maf version=1 program=progressiveMauve"; per block "a", per row
          "s {src} {start} {size} {strand} {srcSize} {cells}", an empty line.  The contig table has the form of
          mauve_set_genomes_contigs (n_contigs[g] 0-based ascending starts per genome, the first 0, concatenated in contig_starts; NULL:
          every genome is one contig), contig_names flat in the same order or NULL.  src = names[g].contig_name, names[g] without contig
          names; size = hi - lo + 1, srcSize = the contig's length, start = lo - contig start - 1, on the reverse strand srcSize minus the
          local hi.  A row whose ends lie in different contigs makes the call return MAUVE_ERR_ARG (the text names the range and the
          genome; no text is kept): split the ranges at the joins (the applyBreakpoints pass of the tool is not part of the call).
        mauve_alignment_text lays the text out and writes it into a device buffer the context keeps: *n_bytes its length (int64: 2^31
        bytes or more are legal), *n_blocks the blocks written.  mauve_alignment_text_fetch copies the slice [offset, offset + len) of it
        (page-locked destinations directly; buf == NULL with len == 0 is legal) and block_off[n_range + 1] when asked: block r is the
        bytes block_off[r] .. block_off[r + 1], block_off[0] the header's length, block_off[n_range] = n_bytes, equal neighbours for a
        block left out.  Slices stream a large text through a small buffer; block_off cuts per-LCB files.
        MAUVE_ERR_ARG: a bad format, wrap < 1 for XMFA, wrap != 0 or a contig table that does not ascend from 0 inside its genome for
        MAF, a contig table for XMFA, the range errors of mauve_extract_select, a slice outside the text.  MAUVE_ERR_LIMIT: ranges x
        (nseq + 2) of 2^31 or more.  MAUVE_ERR_STATE: as for mauve_extract_select; a fetch without a text -- a later
        mauve_coord_index*, mauve_project_index, mauve_set_genomes* or text call ends the one before. ---- */
#define MAUVE_TEXT_XMFA 0
#define MAUVE_TEXT_MAF 1
typedef struct { int32_t format; int32_t wrap; } mauve_text_params;
void mauve_default_text_params(int format, mauve_text_params *p);             /* wrap 80 for XMFA, 0 for MAF */
int mauve_alignment_text(mauve_ctx *ctx, const mauve_text_params *p, const char *const *names, const char *const *deflines,
                         const int64_t *n_contigs, const int64_t *contig_starts, const char *const *contig_names,
                         int64_t n_range, const int64_t *range_iv, const int64_t *range_col, const int64_t *range_len,
                         int64_t *n_bytes, int64_t *n_blocks);
int mauve_alignment_text_fetch(mauve_ctx *ctx, int64_t offset, int64_t len, char *buf,
                               int64_t *block_off /* n_range+1 or NULL */);

/* ---- measurement -------------------------------------------------------------------------------
   Per-kernel HIP-event timing on the context's stream (bench.py roofline).  Kernel ids: */
#define MAUVE_K_EXTRACT 0
#define MAUVE_K_SORT_HIST 1
#define MAUVE_K_SORT_SCAN 2
#define MAUVE_K_SORT_SCATTER 3
#define MAUVE_K_JOIN 4
#define MAUVE_K_EXTEND 5
#define MAUVE_K_DP 6
#define MAUVE_K_RUNS 7
#define MAUVE_K_CANON 8           /* canonical order on the device: key build, its (small) radix sort, gather */
#define MAUVE_K_MISC 9            /* the small sorts of the device chain and of the DP front end */
#define MAUVE_K_EXC_MAPS 10       /* excursions (S18): the chunks' maps */
#define MAUVE_K_EXC_SCAN 11       /* ... the scans along the streams (two launches each, and the scan of the streams' counts) */
#define MAUVE_K_EXC_COUNT 12      /* ... emission counts and carried maxima */
#define MAUVE_K_EXC_WRITE 13      /* ... the records */
#define MAUVE_K_COUNT 14
int mauve_profile_enable(mauve_ctx *ctx, int on);
int mauve_profile_reset(mauve_ctx *ctx);
int mauve_profile_get(mauve_ctx *ctx, int kernel, double *total_ms, int64_t *launches, int64_t *units);
/* wall-clock of the stages of the last mauve_align / mauve_progressive_align call, milliseconds (progressive: summed over the
   nodes of the guide tree; tree_ms = the pairwise passes and the guide tree in front of them) */
typedef struct {
    double seed_ms, chain_ms, recurse_ms, dp_ms, assemble_ms, total_ms, tree_ms;
} mauve_stage_times;
int mauve_last_stage_times(mauve_ctx *ctx, mauve_stage_times *t);

#ifdef __cplusplus
}
#endif
#endif
