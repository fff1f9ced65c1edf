"""ctypes loader for libmauve_hip.so (the C-ABI declared in include/mauve_hip.h).

Plumbing only: tests, bench.py and __graft_entry__ call the product through this module.  There is no
CPU fallback -- `Context()` raises if the library or a GPU is missing.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmauve_hip.so")

MODE_MEM, MODE_UNIQUE, MODE_PAIRWISE = 0, 1, 2
CODING_SEED, SOLID_SEED = 3, 0x7FFFFFFF
MAX_GENOME_LEN, MAX_TOTAL_LEN = 1 << 31, (1 << 32) - (1 << 20)             # mauve_set_genomes* limits (MAUVE_MAX_GENOME_LEN, MAUVE_MAX_TOTAL_LEN)
REPEAT_PENALTY_OFF, REPEAT_PENALTY_NEGATIVE, REPEAT_PENALTY_ZERO = 0, 1, 2    # DESIGN.md S11d (progressiveMauve --repeat-penalty)
K_EXTRACT, K_SORT_HIST, K_SORT_SCAN, K_SORT_SCATTER, K_JOIN, K_EXTEND, K_DP, K_RUNS = range(8)
KERNEL_NAMES = ["seed_extract", "rs_hist", "rs_rowscan", "rs_scatter", "mum_join", "mum_extend", "dp_step", "mum_runs", "canon_sort", "misc_sort",
                "exc_maps", "exc_scan", "exc_count", "exc_write"]

# every symbol include/mauve_hip.h declares (checked by tests/test_abi.py without a GPU)
EXPORTS = [
    "mauve_ctx_create", "mauve_ctx_destroy", "mauve_last_error", "mauve_device_name", "mauve_synchronize",
    "mauve_host_alloc", "mauve_host_free", "mauve_set_shard", "mauve_set_shard_rccl", "mauve_shard_get_stats",
    "mauve_get_seed", "mauve_seed_length", "mauve_seed_weight", "mauve_default_seed_weight", "mauve_default_scoring",
    "mauve_default_params", "mauve_default_progressive_params", "mauve_packed_words", "mauve_pack_ascii", "mauve_pack_codes", "mauve_set_genomes", "mauve_set_genomes_contigs",
    "mauve_ambiguity_bitmap",
    "mauve_sorted_mer_list", "mauve_seed_mums", "mauve_get_matches", "mauve_extend_hits", "mauve_seed_match_enumerate",
    "mauve_eliminate_overlaps", "mauve_lcb_chain", "mauve_dp_batch", "mauve_dp_batch_banded", "mauve_match_sp_scores", "mauve_align", "mauve_align_fetch", "mauve_align_fetch_compact", "mauve_align_prefetch",
    "mauve_align_matches", "mauve_align_lcbs", "mauve_align_begin", "mauve_align_begin_matches", "mauve_align_dp_anchors", "mauve_align_dp_cost", "mauve_align_dp", "mauve_align_finish",
    "mauve_guide_tree", "mauve_breakpoint_counts", "mauve_hmm_params_from", "mauve_apply_homology", "mauve_apply_homology_alignment", "mauve_progressive_align", "mauve_progressive_align_tree",
    "mauve_backbone", "mauve_backbone_alignment", "mauve_backbone_fetch", "mauve_merge_matches",
    "mauve_write_xmfa", "mauve_profile_enable", "mauve_profile_reset", "mauve_profile_get", "mauve_last_stage_times",
    "mauve_set_repeat_penalty", "mauve_seed_multiplicity", "mauve_match_sp_scores_repeat",
    "mauve_coord_index", "mauve_coord_index_alignment", "mauve_coord_index_size", "mauve_column_positions", "mauve_seqpos_to_column", "mauve_translate_positions",
    "mauve_default_extract_params", "mauve_extract_select", "mauve_extract_fetch",
    "mauve_pair_stats", "mauve_pair_stats_identity", "mauve_pair_stats_sp_score",
    "mauve_score_truth", "mauve_score_alignment", "mauve_score_totals_from",
    "mauve_excursions_pairs", "mauve_excursions_core", "mauve_excursions_fetch", "mauve_excursion_thresholds",
    "mauve_default_project_params", "mauve_project", "mauve_project_fetch", "mauve_project_index",
    "mauve_repeat_matches", "mauve_repeat_fetch",
    "mauve_map_ranges", "mauve_map_ranges_fetch", "mauve_range_overlaps",
    "mauve_repeat_score", "mauve_repeat_score_ppv",
    "mauve_default_text_params", "mauve_alignment_text", "mauve_alignment_text_fetch",
]


class Scoring(C.Structure):
    _fields_ = [("gap_open", C.c_int32), ("gap_extend", C.c_int32), ("matrix", (C.c_int32 * 4) * 4)]


class Params(C.Structure):
    _fields_ = [("seed_pattern", C.c_uint64), ("seed_weight", C.c_int32), ("seed_rank", C.c_int32),
                ("mode", C.c_int32), ("lcb_weight", C.c_int64), ("collinear", C.c_int32),
                ("recursive", C.c_int32), ("gapped", C.c_int32), ("add_unaligned", C.c_int32),
                ("extend_lcbs", C.c_int32), ("max_extension_iters", C.c_int32),
                ("min_recursive_gap", C.c_int64), ("max_gapped_len", C.c_int64), ("scoring", Scoring),
                ("max_banded_len", C.c_int64), ("lcb_scoring", C.c_int32), ("weight_scaling", C.c_int32),
                ("conservation_scale_ppm", C.c_int32), ("seed_family", C.c_int32), ("min_scaled_penalty", C.c_int64),
                ("refine_rounds", C.c_int32), ("bp_dist_scale_ppm", C.c_int32), ("bp_dist_min_score", C.c_int64)]


class HmmParams(C.Structure):
    _fields_ = [("match", C.c_int32), ("mismatch", C.c_int32), ("gap", C.c_int32), ("go_homologous", C.c_int32), ("go_unrelated", C.c_int32)]


class ExtractParams(C.Structure):
    _fields_ = [("n_keep", C.c_int32), ("keep", C.c_int32 * 32), ("require", C.c_uint32), ("drop_empty", C.c_int32), ("polymorphic", C.c_int32)]


class TextParams(C.Structure):
    _fields_ = [("format", C.c_int32), ("wrap", C.c_int32)]


TEXT_XMFA, TEXT_MAF = 0, 1


class ProjectParams(C.Structure):
    _fields_ = [("n_proj", C.c_int32), ("proj", C.c_int32 * 32), ("drop_empty", C.c_int32)]


class ProjectSizes(C.Structure):
    _fields_ = [("n_iv", C.c_int64), ("n_cols", C.c_int64), ("n_src", C.c_int64), ("n_fill", C.c_int64)]


class RangeMapSizes(C.Structure):
    _fields_ = [("n_query", C.c_int64), ("n_piece", C.c_int64)]


class AlignSizes(C.Structure):
    _fields_ = [("n_mums", C.c_int64), ("n_lcb", C.c_int64), ("n_anchor", C.c_int64), ("n_iv", C.c_int64),
                ("n_cols", C.c_int64), ("n_gap_dp", C.c_int64), ("n_dp_cells", C.c_int64)]


class StageTimes(C.Structure):
    _fields_ = [("seed_ms", C.c_double), ("chain_ms", C.c_double), ("recurse_ms", C.c_double),
                ("dp_ms", C.c_double), ("assemble_ms", C.c_double), ("total_ms", C.c_double), ("tree_ms", C.c_double)]


_lib = None


def load():
    """dlopen the product library; raises OSError with a clear message when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError("libmauve_hip.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(make -C mauvealigner_amd/csrc); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    L.mauve_last_error.restype = C.c_char_p
    L.mauve_last_error.argtypes = [C.c_void_p]
    L.mauve_get_seed.restype = C.c_uint64
    L.mauve_get_seed.argtypes = [C.c_int, C.c_int]
    L.mauve_seed_length.argtypes = [C.c_uint64]
    L.mauve_seed_weight.argtypes = [C.c_uint64]
    L.mauve_default_seed_weight.argtypes = [C.c_int64]
    L.mauve_packed_words.restype = C.c_size_t
    L.mauve_packed_words.argtypes = [C.c_int64]
    L.mauve_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.mauve_ctx_destroy.argtypes = [C.c_void_p]
    L.mauve_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    L.mauve_host_free.argtypes = [C.c_void_p]
    L.mauve_host_free.restype = None
    L.mauve_align_prefetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    _lib = L
    return L


def default_project_params(nseq):
    """mauve_default_project_params (host only): every genome in order, drop_empty = 1"""
    p = ProjectParams()
    L = load()
    L.mauve_default_project_params.restype = None
    L.mauve_default_project_params(C.c_int(nseq), C.byref(p))
    return p


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


# int (*mauve_allgather_fn)(void *user, const void *send, int64_t send_bytes, const void **recv, int64_t *recv_bytes)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_int64))


class _PinnedBlock:
    """one mauve_host_alloc allocation, released when the last numpy view of it goes away"""

    def __init__(self, nbytes):
        self.L = load()
        p = C.c_void_p()
        rc = self.L.mauve_host_alloc(C.c_size_t(max(int(nbytes), 64)), C.byref(p))
        if rc or not p.value:
            raise MemoryError("mauve_host_alloc(%d) failed (%d)" % (nbytes, rc))
        self.p = p
        self.buf = (C.c_uint8 * max(int(nbytes), 64)).from_address(p.value)

    def __del__(self):
        try:
            if self.p:
                self.L.mauve_host_free(self.p)
                self.p = None
        except Exception:
            pass


def pinned_empty(shape, dtype):
    """numpy array in page-locked host memory (mauve_host_alloc): what a caller hands to set_genomes / fetch for one-DMA transfers"""
    dt = np.dtype(dtype)
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    n = int(np.prod(shape)) if shape else 1
    blk = _PinnedBlock(n * dt.itemsize)
    a = np.frombuffer(blk.buf, dtype=dt, count=n).reshape(shape)
    blk.buf._mauve_block = blk          # the ctypes buffer is the base of every view: it keeps the allocation alive
    return a


class ResultBuffers:
    """Caller-owned, reusable result arrays for Context.align(..., out=...): page-locked, grown on demand, so that a fetch is
    one DMA per bulk array and no allocation.  The arrays returned by a fetch are views that the next fetch overwrites."""

    def __init__(self):
        self._a = {}

    def get(self, name, shape, dtype):
        shape = (shape,) if np.isscalar(shape) else tuple(shape)
        n = int(np.prod(shape)) if shape else 1
        cur = self._a.get(name)
        if cur is None or cur.size < n or cur.dtype != np.dtype(dtype):
            cur = pinned_empty(max(n + n // 8, 16), dtype)
            self._a[name] = cur
        return cur[:n].reshape(shape)


def get_seed(weight, rank=0):
    return int(load().mauve_get_seed(weight, rank))


def seed_length(p):
    return int(load().mauve_seed_length(C.c_uint64(p)))


def seed_weight(p):
    return int(load().mauve_seed_weight(C.c_uint64(p)))


def default_seed_weight(avg_len):
    return int(load().mauve_default_seed_weight(C.c_int64(int(avg_len))))


def default_params(**kw):
    p = Params()
    load().mauve_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_progressive_params(**kw):
    """the progressiveMauve call site's option set (SP scoring, weight scaling 0.5 / 0.5, refinement on)"""
    p = Params()
    load().mauve_default_progressive_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def merge_matches(len_a, st_a, len_b, st_b):
    """mauve_merge_matches (host entry, no context): a, then the matches of b no match of a contains; canonical order."""
    la = np.ascontiguousarray(len_a, np.int64); sa = np.ascontiguousarray(st_a, np.int64)
    lb = np.ascontiguousarray(len_b, np.int64); sb = np.ascontiguousarray(st_b, np.int64)
    N = sa.shape[1] if sa.ndim == 2 and sa.shape[0] else sb.shape[1]
    cap = C.c_int64(len(la) + len(lb))
    lo = np.zeros(max(cap.value, 1), np.int64); so = np.zeros((max(cap.value, 1), N), np.int64)
    rc = load().mauve_merge_matches(N, C.c_int64(len(la)), _p(la, C.c_int64), _p(sa, C.c_int64), C.c_int64(len(lb)), _p(lb, C.c_int64),
                                    _p(sb, C.c_int64), C.byref(cap), _p(lo, C.c_int64), _p(so, C.c_int64))
    if rc:
        raise RuntimeError("mauve_merge_matches failed (%d)" % rc)
    return lo[:cap.value].copy(), so[:cap.value].copy()


def default_scoring():
    s = Scoring()
    load().mauve_default_scoring(C.byref(s))
    return s


PAIR_STATS_WORDS = 32                 # MAUVE_PAIR_STATS_WORDS: int64 per record


def pair_stats_identity(stats):
    """mauve_pair_stats_identity (host entry, no context): records [..., 32] -> identity [...] (equal letters / columns where both have a residue)"""
    st = np.ascontiguousarray(stats, np.int64)
    if st.ndim < 1 or st.shape[-1] != PAIR_STATS_WORDS:
        raise ValueError("pair_stats_identity: records of %d int64 expected" % PAIR_STATS_WORDS)
    out = np.zeros(st.shape[:-1], np.float64)
    L = load()
    L.mauve_pair_stats_identity.restype = None
    if out.size:
        L.mauve_pair_stats_identity(_p(st, C.c_int64), C.c_int64(out.size), _p(out, C.c_double))
    return out


def pair_stats_sp_score(stats, scoring=None):
    """mauve_pair_stats_sp_score (host entry, no context): records [..., 32] -> the pairs' sum-of-pairs scores [...] under `scoring` (a
    Scoring, None = the default)"""
    st = np.ascontiguousarray(stats, np.int64)
    if st.ndim < 1 or st.shape[-1] != PAIR_STATS_WORDS:
        raise ValueError("pair_stats_sp_score: records of %d int64 expected" % PAIR_STATS_WORDS)
    sc = scoring if scoring is not None else default_scoring()
    out = np.zeros(st.shape[:-1], np.int64)
    L = load()
    L.mauve_pair_stats_sp_score.restype = None
    if out.size:
        L.mauve_pair_stats_sp_score(_p(st, C.c_int64), C.c_int64(out.size), C.byref(sc), _p(out, C.c_int64))
    return out


EXCURSION_CHUNK = 512                 # MAUVE_EXCURSION_CHUNK: columns per chunk of the excursion scan; no result depends on it


def excursion_thresholds(height):
    """mauve_excursion_thresholds (host entry, no context): heights -> (threshold[4], above[4]) for the fractions .95, .99, .999, .9999 of
    the sorted heights, by evd's index arithmetic; zeros for no height"""
    h = np.ascontiguousarray(height, np.int64).reshape(-1)
    thr, above = np.zeros(4, np.int64), np.zeros(4, np.int64)
    L = load()
    L.mauve_excursion_thresholds.restype = None
    L.mauve_excursion_thresholds(_p(h if h.size else np.zeros(1, np.int64), C.c_int64), C.c_int64(h.size), _p(thr, C.c_int64), _p(above, C.c_int64))
    return thr, above


SCORE_WORDS = 8                       # MAUVE_SCORE_WORDS: int64 per ordered genome pair


class ScoreTotals(C.Structure):
    _fields_ = [("tp", C.c_int64), ("tn", C.c_int64), ("fp", C.c_int64), ("fn", C.c_int64), ("total", C.c_int64), ("unaligned_fn", C.c_int64)]


def score_totals(records):
    """mauve_score_totals_from (host entry, no context): records [N, N, 8] of Context.score_alignment -> the totals of scoreAlignment.cpp under
    the keys of accuracy.score_alignment_reference (tp, tn, fp, fn, total, sensitivity, specificity), and unaligned_fn"""
    rec = np.ascontiguousarray(records, np.int64)
    if rec.ndim != 3 or rec.shape[0] != rec.shape[1] or rec.shape[2] != SCORE_WORDS:
        raise ValueError("score_totals: records [N, N, %d] expected" % SCORE_WORDS)
    t = ScoreTotals()
    L = load()
    L.mauve_score_totals_from.restype = None
    L.mauve_score_totals_from(_p(rec if rec.size else np.zeros(1, np.int64), C.c_int64), C.c_int(rec.shape[0]), C.byref(t))
    out = {k: int(getattr(t, k)) for k, _ in ScoreTotals._fields_}
    out["sensitivity"] = out["tp"] / max(out["tp"] + out["fn"], 1)
    out["specificity"] = out["tn"] / max(out["tn"] + out["fp"], 1)
    return out


REPEAT_SCORE_WORDS = 4                # int64 per row pair of mauve_repeat_score's pair_records: possible, truepos, exact, 0


class RepeatScoreTotals(C.Structure):
    _fields_ = [("sp_possible", C.c_int64), ("sp_truepos", C.c_int64), ("sp_exact", C.c_int64), ("components", C.c_int64), ("components_hit", C.c_int64),
                ("component_pairs", C.c_int64), ("component_pairs_hit", C.c_int64), ("reserved", C.c_int64)]


def repeat_score_ppv(totals):
    """mauve_repeat_score_ppv (host entry, no context): the totals of Context.repeat_score (dict or RepeatScoreTotals) -> dict(sensitivity,
    exact_sensitivity, component_ppv, pairwise_ppv), the figures of scoreProcrastAlignment.cpp:346-363; 0 / 0 gives 0"""
    t = totals
    if not isinstance(t, RepeatScoreTotals):
        t = RepeatScoreTotals(*[int(totals.get(k, 0)) for k, _ in RepeatScoreTotals._fields_])
    out = (C.c_double * 4)()
    L = load()
    L.mauve_repeat_score_ppv.restype = None
    L.mauve_repeat_score_ppv.argtypes = [C.POINTER(RepeatScoreTotals), C.POINTER(C.c_double)]
    L.mauve_repeat_score_ppv(C.byref(t), out)
    return dict(zip(("sensitivity", "exact_sensitivity", "component_ppv", "pairwise_ppv"), (float(x) for x in out)))


def pack_codes(codes):
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    L = load()
    words = np.zeros(L.mauve_packed_words(len(codes)), dtype=np.uint64)
    L.mauve_pack_codes(_p(codes, C.c_uint8), C.c_int64(len(codes)), _p(words, C.c_uint64))
    return words


def pack_ascii(text):
    b = text if isinstance(text, (bytes, bytearray)) else text.encode()
    L = load()
    words = np.zeros(L.mauve_packed_words(len(b)), dtype=np.uint64)
    L.mauve_pack_ascii(C.c_char_p(bytes(b)), C.c_int64(len(b)), _p(words, C.c_uint64))
    return words


def eliminate_overlaps(length, start):
    length = np.array(length, dtype=np.int64, copy=True)
    start = np.array(start, dtype=np.int64, copy=True)
    n = C.c_int64(len(length))
    N = start.shape[1]
    rc = load().mauve_eliminate_overlaps(N, C.byref(n), _p(length, C.c_int64), _p(start, C.c_int64))
    if rc:
        raise RuntimeError("mauve_eliminate_overlaps: %d" % rc)
    return length[:n.value].copy(), start[:n.value].copy()


def lcb_chain(length, start, min_weight, collinear=False):
    length = np.ascontiguousarray(length, dtype=np.int64)
    start = np.ascontiguousarray(start, dtype=np.int64)
    n, N = len(length), start.shape[1]
    ml = np.zeros(max(n, 1), np.int64)
    le = np.zeros((max(n, 1), N), np.int64)
    re = np.zeros((max(n, 1), N), np.int64)
    wt = np.zeros(max(n, 1), np.int64)
    la = np.zeros((max(n, 1), N), np.int64)
    ra = np.zeros((max(n, 1), N), np.int64)
    k = C.c_int64()
    rc = load().mauve_lcb_chain(N, C.c_int64(n), _p(length, C.c_int64), _p(start, C.c_int64), C.c_int64(min_weight),
                                int(collinear), _p(ml, C.c_int64), C.byref(k), _p(le, C.c_int64), _p(re, C.c_int64),
                                _p(wt, C.c_int64), _p(la, C.c_int64), _p(ra, C.c_int64))
    if rc:
        raise RuntimeError("mauve_lcb_chain: %d" % rc)
    K = k.value
    return {"n_lcb": K, "match_lcb": ml[:n].copy(), "left_end": le[:K].copy(), "right_end": re[:K].copy(),
            "weight": wt[:K].copy(), "left_adj": la[:K].copy(), "right_adj": ra[:K].copy()}


class Context:
    """One mauve_ctx = one GPU + one stream.  Fails loudly when the extension or the GPU is absent."""

    def __init__(self, device=0):
        self.L = load()
        h = C.c_void_p()
        rc = self.L.mauve_ctx_create(device, C.byref(h))
        if rc:
            raise RuntimeError("mauve_ctx_create failed (%d): %s" % (rc, self.L.mauve_last_error(None).decode()))
        self.h = h
        self.nseq = 0
        self._keep = None

    def close(self):
        if self.h:
            self.L.mauve_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, self.L.mauve_last_error(self.h).decode()))

    def device_name(self):
        buf = C.create_string_buffer(256)
        self.L.mauve_device_name(self.h, buf, 256)
        return buf.value.decode()

    def set_shard(self, rank, world, allgather=None):
        """mauve_set_shard: `allgather(payload: bytes-like) -> list of per-rank bytes-like` is the caller's collective (e.g.
        parallel.make_allgather(dist)); None / world <= 1 switches the sharding off.  The callback object is kept alive here."""
        if allgather is None or world <= 1:
            self._shard_cb = None
            self._chk(self.L.mauve_set_shard(self.h, 0, 1, C.cast(None, ALLGATHER_FN), None), "mauve_set_shard")
            return
        state = {"keep": None}

        def cb(user, send, nbytes, recv_out, sizes_out):
            try:
                mine = (C.c_char * nbytes).from_address(send) if nbytes else b""
                parts = allgather(bytes(mine))
                if len(parts) != world:
                    return 2
                blob = b"".join(bytes(x) for x in parts)
                buf = C.create_string_buffer(blob, max(len(blob), 1))
                state["keep"] = buf                          # valid until the next call
                recv_out[0] = C.cast(buf, C.c_void_p).value
                for r in range(world):
                    sizes_out[r] = len(parts[r])
                return 0
            except Exception as ex:                          # never let an exception cross the C boundary
                state["error"] = repr(ex)
                return 1
        self._shard_cb = ALLGATHER_FN(cb)
        self._shard_state = state
        self._chk(self.L.mauve_set_shard(self.h, int(rank), int(world), self._shard_cb, None), "mauve_set_shard")

    def synchronize(self):
        self._chk(self.L.mauve_synchronize(self.h), "mauve_synchronize")

    def set_genomes(self, codes_list, contig_starts=None, invalid=None):
        """codes_list: list of uint8 arrays of 0..3 codes (packed here with mauve_pack_codes).  contig_starts: per genome
        the 0-based starts of its contigs (first 0); invalid: per genome a boolean array, True = ambiguous base."""
        packed = [pack_codes(c) for c in codes_list]
        n = len(packed)
        arr = (C.POINTER(C.c_uint64) * n)(*[_p(w, C.c_uint64) for w in packed])
        lens = (C.c_int64 * n)(*[len(c) for c in codes_list])
        if contig_starts is None and invalid is None:
            self._chk(self.L.mauve_set_genomes(self.h, n, arr, lens), "mauve_set_genomes")
        else:
            cs = contig_starts or [[0]] * n
            ncont = (C.c_int64 * n)(*[len(x) for x in cs])
            flat = np.array([int(v) for x in cs for v in x] + [0], dtype=np.int64)
            bits = []
            for g in range(n):
                L = len(codes_list[g])
                w = np.zeros(L // 64 + 1, np.uint64)
                if invalid is not None and invalid[g] is not None:
                    b = np.zeros((L // 64 + 1) * 64, np.uint8)
                    b[:L] = np.asarray(invalid[g], dtype=np.uint8)
                    w = np.packbits(b, bitorder="little").view(np.uint64).copy()
                bits.append(w)
            inv = (C.POINTER(C.c_uint64) * n)(*[_p(w, C.c_uint64) for w in bits])
            self._chk(self.L.mauve_set_genomes_contigs(self.h, n, arr, lens, ncont, _p(flat, C.c_int64), inv), "mauve_set_genomes_contigs")
        self.nseq = n
        self.lens = [len(c) for c in codes_list]

    def set_genomes_packed(self, packed, lens, contig_starts=None, invalid_bits=None):
        """genomes already in the boundary's 2-bit packing (pack_codes): the upload alone (arrays from pinned_empty go up
        in one DMA each, without a staging copy).  contig_starts: as in set_genomes; invalid_bits: per genome the ambiguity
        bitmap already packed (uint64, bit i of word i // 64 = base i is ambiguous, at least len // 64 + 1 words: the layout
        of mauve_ambiguity_bitmap) or None -- no per-base array, so genomes of a gigabase cost their 2-bit and 1-bit images only"""
        n = len(packed)
        arr = (C.POINTER(C.c_uint64) * n)(*[_p(w, C.c_uint64) for w in packed])
        ln = (C.c_int64 * n)(*[int(x) for x in lens])
        if contig_starts is None and invalid_bits is None:
            self._chk(self.L.mauve_set_genomes(self.h, n, arr, ln), "mauve_set_genomes")
        else:
            if (contig_starts is not None and len(contig_starts) != n) or (invalid_bits is not None and len(invalid_bits) != n):
                raise ValueError("set_genomes_packed: contig_starts / invalid_bits need one entry per genome (%d)" % n)
            cs = contig_starts or [[0]] * n
            ncont = (C.c_int64 * n)(*[len(x) for x in cs])
            flat = np.array([int(v) for x in cs for v in x] + [0], dtype=np.int64)
            bits = []
            for g in range(n):
                w = None if invalid_bits is None else invalid_bits[g]
                if w is not None:
                    w = np.ascontiguousarray(w, dtype=np.uint64)
                    if len(w) < int(lens[g]) // 64 + 1:
                        raise ValueError("invalid_bits[%d]: %d words, the genome needs %d" % (g, len(w), int(lens[g]) // 64 + 1))
                bits.append(w)
            inv = (C.POINTER(C.c_uint64) * n)(*[_p(w, C.c_uint64) if w is not None else C.POINTER(C.c_uint64)() for w in bits])
            self._chk(self.L.mauve_set_genomes_contigs(self.h, n, arr, ln, ncont, _p(flat, C.c_int64), inv), "mauve_set_genomes_contigs")
        self.nseq = n
        self.lens = [int(x) for x in lens]

    def seed_mums(self, pattern, mode=MODE_MEM, mask=0, extend=True, fetch=True):
        n = C.c_int64()
        self._chk(self.L.mauve_seed_mums(self.h, C.c_uint64(pattern), mode, C.c_uint64(mask), int(bool(extend)),
                                         C.byref(n)), "mauve_seed_mums")
        if not fetch:
            return n.value
        ln = np.zeros(n.value, np.int64)
        st = np.zeros((n.value, self.nseq), np.int64)
        self._chk(self.L.mauve_get_matches(self.h, _p(ln, C.c_int64), _p(st, C.c_int64)), "mauve_get_matches")
        return ln, st

    def extend_hits(self, pattern, mask, pos, strand, extend=True):
        """seed hits enumerated on the host (the MatchFinder callback path) -> extended matches in canonical order"""
        mask = np.ascontiguousarray(mask, dtype=np.uint32)
        pos = np.ascontiguousarray(pos, dtype=np.int64)
        strand = np.ascontiguousarray(strand, dtype=np.uint8)
        n = C.c_int64()
        self._chk(self.L.mauve_extend_hits(self.h, C.c_uint64(pattern), C.c_int64(len(mask)), _p(mask, C.c_uint32), _p(pos, C.c_int64),
                                           _p(strand, C.c_uint8), int(bool(extend)), C.byref(n)), "mauve_extend_hits")
        ln = np.zeros(n.value, np.int64)
        st = np.zeros((n.value, self.nseq), np.int64)
        self._chk(self.L.mauve_get_matches(self.h, _p(ln, C.c_int64), _p(st, C.c_int64)), "mauve_get_matches")
        return ln, st

    def align_matches(self, params, length, start, fetch=True, names=None, want_xmfa=False):
        """Aligner::align on the caller's match list (no seed pass)"""
        p = params or default_params()
        length = np.ascontiguousarray(length, dtype=np.int64)
        start = np.ascontiguousarray(start, dtype=np.int64)
        sz = AlignSizes()
        self._chk(self.L.mauve_align_matches(self.h, C.byref(p), C.c_int64(len(length)), _p(length, C.c_int64), _p(start, C.c_int64),
                                             C.byref(sz)), "mauve_align_matches")
        if not fetch:
            return {k: int(getattr(sz, k)) for k, _ in AlignSizes._fields_}
        return self._fetch(sz, names, want_xmfa)

    def align_lcbs(self, params, length, start, lcb, fetch=True, names=None, want_xmfa=False):
        """Aligner::align resumed from the caller's LCBs (mauve_align_lcbs): recursion + gapped alignment only"""
        p = params or default_params()
        length = np.ascontiguousarray(length, dtype=np.int64)
        start = np.ascontiguousarray(start, dtype=np.int64)
        lcb = np.ascontiguousarray(lcb, dtype=np.int64)
        sz = AlignSizes()
        self._chk(self.L.mauve_align_lcbs(self.h, C.byref(p), C.c_int64(len(length)), _p(length, C.c_int64), _p(start, C.c_int64),
                                          _p(lcb, C.c_int64), C.byref(sz)), "mauve_align_lcbs")
        if not fetch:
            return {k: int(getattr(sz, k)) for k, _ in AlignSizes._fields_}
        return self._fetch(sz, names, want_xmfa)

    def align_dp_anchors(self, n_dp):
        N = self.nseq
        left = np.zeros((max(n_dp, 1), 1 + N), np.int64)
        right = np.zeros((max(n_dp, 1), 1 + N), np.int64)
        self._chk(self.L.mauve_align_dp_anchors(self.h, _p(left, C.c_int64), _p(right, C.c_int64)), "mauve_align_dp_anchors")
        return left[:n_dp], right[:n_dp]

    def sorted_mer_list(self, seq, pattern):
        n = max(0, self.lens[seq] - seed_length(pattern) + 1)
        mer = np.zeros(n, np.uint64)
        pos = np.zeros(n, np.int64)
        k = C.c_int64()
        self._chk(self.L.mauve_sorted_mer_list(self.h, seq, C.c_uint64(pattern), _p(mer, C.c_uint64),
                                               _p(pos, C.c_int64), C.byref(k)), "mauve_sorted_mer_list")
        return mer[:k.value], pos[:k.value]

    def seed_match_enumerate(self, seq, pattern, min_multi=2, max_multi=1000, direct_only=False):
        n, ns = C.c_int64(), C.c_int64()
        args = (self.h, seq, C.c_uint64(pattern), C.c_int64(min_multi), C.c_int64(max_multi), int(direct_only))
        self._chk(self.L.mauve_seed_match_enumerate(*args, C.byref(n), C.byref(ns), None, None, None), "seed_match_enumerate")
        mult = np.zeros(n.value, np.int64)
        off = np.zeros(n.value + 1, np.int64)
        st = np.zeros(ns.value, np.int64)
        self._chk(self.L.mauve_seed_match_enumerate(*args, C.byref(n), C.byref(ns), _p(mult, C.c_int64), _p(off, C.c_int64),
                                                    _p(st, C.c_int64)), "seed_match_enumerate")
        return mult, off, st

    def repeat_matches(self, seq, pattern, min_multi=2, max_multi=32):
        """extended repeat matches of resident genome `seq` (mauve_repeat_matches / mauve_repeat_fetch) ->
        (length, mult, start_off, starts), int64, in canonical order"""
        n, ns = C.c_int64(), C.c_int64()
        self._chk(self.L.mauve_repeat_matches(self.h, int(seq), C.c_uint64(pattern), C.c_int64(min_multi), C.c_int64(max_multi),
                                              C.byref(n), C.byref(ns)), "mauve_repeat_matches")
        self._rm_shape = (n.value, ns.value)
        length = np.zeros(n.value, np.int64)
        mult = np.zeros(n.value, np.int64)
        off = np.zeros(n.value + 1, np.int64)
        st = np.zeros(ns.value, np.int64)
        self._chk(self.L.mauve_repeat_fetch(self.h, _p(length, C.c_int64), _p(mult, C.c_int64), _p(off, C.c_int64), _p(st, C.c_int64)),
                  "mauve_repeat_fetch")
        return length, mult, off, st

    def dp_batch(self, intervals, scoring=None, band_from=None):
        """intervals: list of lists of code arrays (nseq each).  -> (cols list, scores).  band_from: intervals whose
        longest sequence is above it run the banded DP (mauve_dp_batch_banded)."""
        sc = scoring or default_scoring()
        n_iv = len(intervals)
        nseq = len(intervals[0]) if n_iv else 1
        if any(len(iv) != nseq for iv in intervals):
            raise ValueError("dp_batch: every interval must hold the same number of sequences")
        flat, off = [], [0]
        for iv in intervals:
            for s in iv:
                flat.append(np.asarray(s, dtype=np.uint8))
                off.append(off[-1] + len(s))
        codes = np.concatenate(flat) if flat and off[-1] else np.zeros(1, np.uint8)
        off = np.array(off, dtype=np.int64)
        cols = np.zeros(max(int(off[-1]), 1), np.uint32)
        col_off = np.zeros(n_iv + 1, np.int64)
        score = np.zeros(max(n_iv, 1), np.int64)
        if band_from is None:
            self._chk(self.L.mauve_dp_batch(self.h, nseq, C.c_int64(n_iv), _p(codes, C.c_uint8), _p(off, C.c_int64),
                                            C.byref(sc), _p(cols, C.c_uint32), _p(col_off, C.c_int64), _p(score, C.c_int64)),
                      "mauve_dp_batch")
        else:
            self._chk(self.L.mauve_dp_batch_banded(self.h, nseq, C.c_int64(n_iv), _p(codes, C.c_uint8), _p(off, C.c_int64),
                                                   C.byref(sc), C.c_int64(int(band_from)), _p(cols, C.c_uint32),
                                                   _p(col_off, C.c_int64), _p(score, C.c_int64)), "mauve_dp_batch_banded")
        return [cols[col_off[i]:col_off[i + 1]].copy() for i in range(n_iv)], score[:n_iv].copy()

    def match_sp_scores(self, length, start, scoring=None):
        """extant sum-of-pairs scores of ungapped matches on the resident genomes (mauve_match_sp_scores)"""
        sc = scoring or default_scoring()
        length = np.ascontiguousarray(length, dtype=np.int64)
        start = np.ascontiguousarray(start, dtype=np.int64).reshape(len(length), self.nseq)
        out = np.zeros(max(len(length), 1), np.int64)
        self._chk(self.L.mauve_match_sp_scores(self.h, C.c_int64(len(length)), _p(length, C.c_int64), _p(start, C.c_int64),
                                               C.byref(sc), _p(out, C.c_int64)), "mauve_match_sp_scores")
        return out[:len(length)].copy()

    def set_repeat_penalty(self, mode):
        """mauve_set_repeat_penalty: REPEAT_PENALTY_OFF / _NEGATIVE / _ZERO for the sum-of-pairs anchor scores of later calls (S11d)"""
        self._chk(self.L.mauve_set_repeat_penalty(self.h, int(mode)), "mauve_set_repeat_penalty")

    def seed_multiplicity(self, seq, pattern):
        """base multiplicities of resident genome `seq` for `pattern` (mauve_seed_multiplicity): uint8[lens[seq]]"""
        n = self.lens[seq] if 0 <= seq < len(self.lens) else 0      # (an index out of range is the library's to refuse)
        out = np.zeros(max(n, 1), np.uint8)
        self._chk(self.L.mauve_seed_multiplicity(self.h, int(seq), C.c_uint64(pattern), _p(out, C.c_uint8)), "mauve_seed_multiplicity")
        return out[:n].copy()

    def match_sp_scores_repeat(self, pattern, mode, length, start, scoring=None):
        """repeat-penalized sum-of-pairs scores of ungapped matches (mauve_match_sp_scores_repeat; mode 0 = match_sp_scores)"""
        sc = scoring or default_scoring()
        length = np.ascontiguousarray(length, dtype=np.int64)
        start = np.ascontiguousarray(start, dtype=np.int64).reshape(len(length), self.nseq)
        out = np.zeros(max(len(length), 1), np.int64)
        self._chk(self.L.mauve_match_sp_scores_repeat(self.h, C.c_uint64(pattern), int(mode), C.c_int64(len(length)), _p(length, C.c_int64),
                                                      _p(start, C.c_int64), C.byref(sc), _p(out, C.c_int64)), "mauve_match_sp_scores_repeat")
        return out[:len(length)].copy()

    def align(self, params=None, fetch=True, names=None, want_xmfa=False, out=None, compact=False):
        """out: a ResultBuffers the result arrays are fetched into (reused from call to call; views)"""
        p = params or default_params()
        sz = AlignSizes()
        if out is not None and compact and not want_xmfa:
            self._prefetch_tables(out)
        self._chk(self.L.mauve_align(self.h, C.byref(p), C.byref(sz)), "mauve_align")
        res = {k: int(getattr(sz, k)) for k, _ in AlignSizes._fields_}
        if not fetch:
            return res
        return self._fetch(sz, names, want_xmfa, out, compact)

    def _prefetch_tables(self, bufs):
        """mauve_align_prefetch: the match and anchor tables of the coming mauve_align may travel into `bufs` while the pass runs.  Only the
        buffers an earlier fetch left in `bufs` are named (ResultBuffers.get hands out views from the base of a block that moves only when it
        grows, so the fetch that follows passes the same pointers; after a regrow it does not, and the library copies as before)."""
        N = self.nseq
        a = [bufs._a.get("c_" + k) for k in ("mum_length", "mum_start", "anchor_length", "anchor_start", "anchor_lcb")]
        if N < 1 or any(x is None or x.dtype != np.int32 for x in a):
            return
        vp = lambda x: x.ctypes.data
        self._chk(self.L.mauve_align_prefetch(self.h, vp(a[0]), vp(a[1]), min(a[0].size, a[1].size // N), vp(a[2]), vp(a[3]), vp(a[4]),
                                              min(a[2].size, a[3].size // N, a[4].size)), "mauve_align_prefetch")

    def _fetch_compact(self, sz, bufs=None):
        """mauve_align_fetch_compact: columns in 1 / 2 / 4 bytes by the genome count, match and anchor tables as int32"""
        N = self.nseq
        out = {k: int(getattr(sz, k)) for k, _ in AlignSizes._fields_}
        cb = 1 if N <= 8 else (2 if N <= 16 else 4)
        cdt = {1: np.uint8, 2: np.uint16, 4: np.uint32}[cb]
        shapes = {
            "mum_length": (sz.n_mums, np.int32), "mum_start": ((sz.n_mums, N), np.int32),
            "lcb_left": ((sz.n_lcb, N), np.int64), "lcb_right": ((sz.n_lcb, N), np.int64), "lcb_weight": (sz.n_lcb, np.int64),
            "anchor_length": (sz.n_anchor, np.int32), "anchor_start": ((sz.n_anchor, N), np.int32), "anchor_lcb": (sz.n_anchor, np.int32),
            "left": ((sz.n_iv, N), np.int64), "right": ((sz.n_iv, N), np.int64), "reverse": ((sz.n_iv, N), np.int8),
            "col_off": (sz.n_iv + 1, np.int64), "cols": (sz.n_cols, cdt), "dp_score": (sz.n_iv, np.int64),
        }
        a = {k: (np.zeros(sh, dt) if bufs is None else bufs.get("c_" + k, sh, dt)) for k, (sh, dt) in shapes.items()}
        self.L.mauve_align_fetch_compact.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 14
        vp = lambda x: x.ctypes.data_as(C.c_void_p)
        self._chk(self.L.mauve_align_fetch_compact(self.h, cb, vp(a["mum_length"]), vp(a["mum_start"]), vp(a["lcb_left"]), vp(a["lcb_right"]), vp(a["lcb_weight"]),
                                                   vp(a["anchor_length"]), vp(a["anchor_start"]), vp(a["anchor_lcb"]), vp(a["left"]), vp(a["right"]), vp(a["reverse"]),
                                                   vp(a["col_off"]), vp(a["cols"]), vp(a["dp_score"])), "mauve_align_fetch_compact")
        out.update(a)
        out["col_bytes"] = cb
        return out

    def _fetch(self, sz, names=None, want_xmfa=False, bufs=None, compact=False):
        if compact and not want_xmfa:
            return self._fetch_compact(sz, bufs)
        N = self.nseq
        out = {k: int(getattr(sz, k)) for k, _ in AlignSizes._fields_}
        shapes = {
            "mum_length": (sz.n_mums, np.int64), "mum_start": ((sz.n_mums, N), np.int64),
            "lcb_left": ((sz.n_lcb, N), np.int64), "lcb_right": ((sz.n_lcb, N), np.int64),
            "lcb_weight": (sz.n_lcb, np.int64),
            "anchor_length": (sz.n_anchor, np.int64), "anchor_start": ((sz.n_anchor, N), np.int64),
            "anchor_lcb": (sz.n_anchor, np.int64),
            "left": ((sz.n_iv, N), np.int64), "right": ((sz.n_iv, N), np.int64),
            "reverse": ((sz.n_iv, N), np.int8), "col_off": (sz.n_iv + 1, np.int64),
            "cols": (sz.n_cols, np.uint32), "dp_score": (sz.n_iv, np.int64),
        }
        if bufs is None:
            a = {k: np.zeros(sh, dt) for k, (sh, dt) in shapes.items()}
        else:
            a = {k: bufs.get(k, sh, dt) for k, (sh, dt) in shapes.items()}
        self._chk(self.L.mauve_align_fetch(
            self.h, _p(a["mum_length"], C.c_int64), _p(a["mum_start"], C.c_int64), _p(a["lcb_left"], C.c_int64),
            _p(a["lcb_right"], C.c_int64), _p(a["lcb_weight"], C.c_int64), _p(a["anchor_length"], C.c_int64),
            _p(a["anchor_start"], C.c_int64), _p(a["anchor_lcb"], C.c_int64), _p(a["left"], C.c_int64),
            _p(a["right"], C.c_int64), _p(a["reverse"], C.c_int8), _p(a["col_off"], C.c_int64),
            _p(a["cols"], C.c_uint32), _p(a["dp_score"], C.c_int64)), "mauve_align_fetch")
        out.update(a)
        if want_xmfa:
            nm = names or ["seq%d" % i for i in range(N)]
            narr = (C.c_char_p * N)(*[s.encode() for s in nm])
            ln = C.c_int64()
            self._chk(self.L.mauve_write_xmfa(self.h, narr, None, C.byref(ln)), "mauve_write_xmfa")
            buf = C.create_string_buffer(ln.value)
            self._chk(self.L.mauve_write_xmfa(self.h, narr, buf, C.byref(ln)), "mauve_write_xmfa")
            out["xmfa"] = buf.value.decode()
        return out

    # ---- sharded form: begin / dp on a subset / finish (include/mauve_hip.h) ----
    def align_begin(self, params=None):
        p = params or default_params()
        n_dp, n_codes = C.c_int64(), C.c_int64()
        self._chk(self.L.mauve_align_begin(self.h, C.byref(p), C.byref(n_dp), C.byref(n_codes)), "mauve_align_begin")
        cost = np.zeros(max(n_dp.value, 1), np.int64)
        cap = np.zeros(max(n_dp.value, 1), np.int64)
        self._chk(self.L.mauve_align_dp_cost(self.h, _p(cost, C.c_int64), _p(cap, C.c_int64)), "mauve_align_dp_cost")
        return n_dp.value, cost[:n_dp.value], cap[:n_dp.value]

    def align_dp(self, idx, cap):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        n = len(idx)
        cols = np.zeros(max(int(cap[idx].sum()) if n else 0, 1), np.uint32)
        col_off = np.zeros(n + 1, np.int64)
        score = np.zeros(max(n, 1), np.int64)
        cells = C.c_int64()
        self._chk(self.L.mauve_align_dp(self.h, _p(idx, C.c_int64), C.c_int64(n), _p(cols, C.c_uint32), _p(col_off, C.c_int64),
                                        _p(score, C.c_int64), C.byref(cells)), "mauve_align_dp")
        return [cols[col_off[i]:col_off[i + 1]] for i in range(n)], score[:n], cells.value

    def align_finish(self, cols_list, scores, cells, fetch=True, names=None, want_xmfa=False, out=None):
        n = len(cols_list)
        col_off = np.zeros(n + 1, np.int64)
        for i, c in enumerate(cols_list):
            col_off[i + 1] = col_off[i] + len(c)
        flat = np.concatenate(cols_list).astype(np.uint32) if n and col_off[n] else np.zeros(1, np.uint32)
        scores = np.ascontiguousarray(scores, dtype=np.int64) if n else np.zeros(1, np.int64)
        sz = AlignSizes()
        self._chk(self.L.mauve_align_finish(self.h, _p(flat, C.c_uint32), _p(col_off, C.c_int64), _p(scores, C.c_int64),
                                            C.c_int64(cells), C.byref(sz)), "mauve_align_finish")
        if not fetch:
            return {k: int(getattr(sz, k)) for k, _ in AlignSizes._fields_}
        return self._fetch(sz, names, want_xmfa, out)

    def guide_tree(self, pattern):
        N = self.nseq
        dist = np.zeros((N, N), np.int64)
        left = np.zeros(2 * N - 1, np.int32)
        right = np.zeros(2 * N - 1, np.int32)
        self._chk(self.L.mauve_guide_tree(self.h, C.c_uint64(pattern), _p(dist, C.c_int64), _p(left, C.c_int32),
                                          _p(right, C.c_int32)), "mauve_guide_tree")
        return dist, left, right

    def breakpoint_counts(self, pattern, min_len):
        """mauve_breakpoint_counts: broken adjacencies between the pairwise matches (length >= min_len) of every genome pair."""
        N = self.nseq
        bp = np.zeros((N, N), np.int64)
        self.L.mauve_breakpoint_counts.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.POINTER(C.c_int64)]
        self._chk(self.L.mauve_breakpoint_counts(self.h, C.c_uint64(pattern), C.c_int64(min_len), _p(bp, C.c_int64)), "mauve_breakpoint_counts")
        return bp

    def progressive_align(self, params=None, fetch=True, names=None, want_xmfa=False, tree=None, out=None, compact=False):
        """tree=(left, right): align along the caller's guide tree (mauve_progressive_align_tree).  out: ResultBuffers."""
        p = params or default_params()
        N = self.nseq
        sz = AlignSizes()
        dist = np.zeros((N, N), np.int64)
        if tree is None:
            left = np.zeros(2 * N - 1, np.int32)
            right = np.zeros(2 * N - 1, np.int32)
            self._chk(self.L.mauve_progressive_align(self.h, C.byref(p), C.byref(sz), _p(left, C.c_int32), _p(right, C.c_int32),
                                                     _p(dist, C.c_int64)), "mauve_progressive_align")
        else:
            left = np.ascontiguousarray(tree[0], np.int32)
            right = np.ascontiguousarray(tree[1], np.int32)
            if len(left) != 2 * N - 1 or len(right) != 2 * N - 1:
                raise ValueError("guide tree must have 2*nseq-1 nodes")
            self._chk(self.L.mauve_progressive_align_tree(self.h, C.byref(p), C.byref(sz), _p(left, C.c_int32),
                                                          _p(right, C.c_int32)), "mauve_progressive_align_tree")
        res = self._fetch(sz, names, want_xmfa, out, compact) if fetch else {k: int(getattr(sz, k)) for k, _ in AlignSizes._fields_}
        res["tree"] = (left, right)
        res["dist"] = dist
        return res

    def _backbone_fetch(self, n_seg, n_isl):
        N = self._bb_nseq
        out = {"seg_iv": np.zeros(n_seg, np.int64), "seg_col": np.zeros(n_seg, np.int64), "seg_len": np.zeros(n_seg, np.int64),
               "seg_mask": np.zeros(n_seg, np.uint32), "seg_left": np.zeros((n_seg, N), np.int64),
               "seg_right": np.zeros((n_seg, N), np.int64), "islands": np.zeros((n_isl, 8), np.int64)}
        self._chk(self.L.mauve_backbone_fetch(self.h, _p(out["seg_iv"], C.c_int64), _p(out["seg_col"], C.c_int64), _p(out["seg_len"], C.c_int64),
                                              _p(out["seg_mask"], C.c_uint32), _p(out["seg_left"], C.c_int64), _p(out["seg_right"], C.c_int64),
                                              _p(out["islands"], C.c_int64)), "mauve_backbone_fetch")
        return out

    def hmm_params(self, identity=0.7, pgh=1e-5, pgu=1e-9, **kw):
        """mauve_hmm_params_from: the call site's knobs (progressiveMauve.cpp:319-322) as integer scores; kw overrides fields."""
        h = HmmParams()
        self.L.mauve_hmm_params_from.argtypes = [C.c_double, C.c_double, C.c_double, C.POINTER(HmmParams)]
        self.L.mauve_hmm_params_from.restype = None
        self.L.mauve_hmm_params_from(identity, pgh, pgu, C.byref(h))
        for k, v in kw.items():
            setattr(h, k, v)
        return h

    def apply_homology(self, hmm=None, fetch=True, names=None, want_xmfa=False):
        """mauve_apply_homology: un-align what the pair HMM classes as unrelated in the alignment this context holds.
        -> the rewritten result (or its sizes) with 'n_moved'."""
        h = hmm or self.hmm_params()
        sz = AlignSizes()
        moved = C.c_int64(0)
        self.L.mauve_apply_homology.argtypes = [C.c_void_p, C.POINTER(HmmParams), C.POINTER(AlignSizes), C.POINTER(C.c_int64)]
        self._chk(self.L.mauve_apply_homology(self.h, C.byref(h), C.byref(sz), C.byref(moved)), "mauve_apply_homology")
        res = self._fetch(sz, names, want_xmfa) if fetch else {k: int(getattr(sz, k)) for k, _ in AlignSizes._fields_}
        res["n_moved"] = int(moved.value)
        return res

    def backbone(self, island_gap=20, nseq=None):
        """Backbone segments and islands of the alignment this context holds (mauve_backbone)."""
        ns, ni = C.c_int64(0), C.c_int64(0)
        self._chk(self.L.mauve_backbone(self.h, C.c_int64(island_gap), C.byref(ns), C.byref(ni)), "mauve_backbone")
        self._bb_nseq = nseq or self.nseq
        return self._backbone_fetch(ns.value, ni.value)

    def backbone_alignment(self, left, right, reverse, col_off, cols, island_gap=20):
        """... of the caller's alignment (mauve_backbone_alignment): left/right/reverse [n_iv, nseq], col_off [n_iv+1], cols."""
        left = np.ascontiguousarray(left, np.int64)
        right = np.ascontiguousarray(right, np.int64)
        reverse = np.ascontiguousarray(reverse, np.int8)
        col_off = np.ascontiguousarray(col_off, np.int64)
        cols = np.ascontiguousarray(cols, np.uint32)
        n_iv, N = left.shape
        ns, ni = C.c_int64(0), C.c_int64(0)
        self._chk(self.L.mauve_backbone_alignment(self.h, N, C.c_int64(n_iv), _p(left, C.c_int64), _p(right, C.c_int64), _p(reverse, C.c_int8),
                                                  _p(col_off, C.c_int64), _p(cols if len(cols) else np.zeros(1, np.uint32), C.c_uint32),
                                                  C.c_int64(island_gap), C.byref(ns), C.byref(ni)), "mauve_backbone_alignment")
        self._bb_nseq = N
        return self._backbone_fetch(ns.value, ni.value)

    def apply_homology_alignment(self, left, right, reverse, col_off, cols, hmm=None):
        """mauve_apply_homology_alignment: the homology pass on the caller's alignment (its genomes are the context's) -> (col_off, cols, n_moved)"""
        left = np.ascontiguousarray(left, np.int64)
        right = np.ascontiguousarray(right, np.int64)
        reverse = np.ascontiguousarray(reverse, np.int8)
        col_off = np.ascontiguousarray(col_off, np.int64)
        cols = np.ascontiguousarray(cols, np.uint32)
        n_iv, N = left.shape
        h = hmm or self.hmm_params()
        residues = int(np.sum(np.where(left != 0, right - left + 1, 0)))
        ncols = np.zeros(max(residues, len(cols)) + 1, np.uint32)
        noff = np.zeros(n_iv + 1, np.int64)
        moved = C.c_int64(0)
        self.L.mauve_apply_homology_alignment.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int8), C.POINTER(C.c_int64),
                                                          C.POINTER(C.c_uint32), C.POINTER(HmmParams), C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_int64)]
        self._chk(self.L.mauve_apply_homology_alignment(self.h, N, n_iv, _p(left, C.c_int64), _p(right, C.c_int64), _p(reverse, C.c_int8), _p(col_off, C.c_int64),
                                                        _p(cols if len(cols) else np.zeros(1, np.uint32), C.c_uint32), C.byref(h), _p(noff, C.c_int64), _p(ncols, C.c_uint32),
                                                        C.byref(moved)), "mauve_apply_homology_alignment")
        return noff, ncols[:noff[-1]].copy(), int(moved.value)

    # ---- coordinate translation through the alignment ----
    def coord_index(self):
        """mauve_coord_index: the rank/select index of the alignment this context holds (a snapshot: it outlives later passes)"""
        self._chk(self.L.mauve_coord_index(self.h), "mauve_coord_index")

    def coord_index_alignment(self, left, right, reverse, col_off, cols):
        """... of the caller's alignment (mauve_coord_index_alignment): left/right/reverse [n_iv, nseq], col_off [n_iv+1], cols."""
        left = np.ascontiguousarray(left, np.int64)
        right = np.ascontiguousarray(right, np.int64)
        reverse = np.ascontiguousarray(reverse, np.int8)
        col_off = np.ascontiguousarray(col_off, np.int64)
        cols = np.ascontiguousarray(cols, np.uint32)
        n_iv, N = left.shape
        self._chk(self.L.mauve_coord_index_alignment(self.h, N, C.c_int64(n_iv), _p(left, C.c_int64), _p(right, C.c_int64), _p(reverse, C.c_int8),
                                                     _p(col_off, C.c_int64), _p(cols if len(cols) else np.zeros(1, np.uint32), C.c_uint32)),
                  "mauve_coord_index_alignment")

    def coord_index_size(self):
        """mauve_coord_index_size: (nseq, n_iv, n_cols) the index in force was built from; the answer arrays are sized by its nseq"""
        n, k, c = C.c_int(0), C.c_int64(0), C.c_int64(0)
        self._chk(self.L.mauve_coord_index_size(self.h, C.byref(n), C.byref(k), C.byref(c)), "mauve_coord_index_size")
        return n.value, k.value, c.value

    @staticmethod
    def _co_out(out, k, shape, dtype):
        """the k-th result array of a coordinate query: the caller's (out=..., e.g. from pinned_empty) or a fresh one"""
        if out is None:
            return np.zeros(shape, dtype)
        a = out[k]
        if a.dtype != np.dtype(dtype) or a.shape != tuple(shape) or not a.flags.c_contiguous:
            raise ValueError("coordinate query: out[%d] must be a contiguous %s array of shape %s" % (k, np.dtype(dtype).name, tuple(shape)))
        return a

    def column_positions(self, iv, col, nearest=False, out=None):
        """mauve_column_positions: (interval, column) -> (pos[n, nseq] signed, defined[n] genome masks).  Arrays from pinned_empty (queries
        and out=(pos, defined)) are copied without staging."""
        iv = np.ascontiguousarray(iv, np.int64)
        col = np.ascontiguousarray(col, np.int64)
        n, N = len(iv), self.coord_index_size()[0]
        if len(col) != n:
            raise ValueError("column_positions: iv and col differ in length")
        pos = self._co_out(out, 0, (n, N), np.int64)
        dfn = self._co_out(out, 1, (n,), np.uint32)
        self._chk(self.L.mauve_column_positions(self.h, C.c_int64(n), _p(iv, C.c_int64), _p(col, C.c_int64), int(bool(nearest)),
                                                _p(pos, C.c_int64), _p(dfn, C.c_uint32)), "mauve_column_positions")
        return pos, dfn

    def seqpos_to_column(self, seq, pos, out=None):
        """mauve_seqpos_to_column: (genome, 1-based position) -> (interval, column in it); (-1, -1) where no interval covers the base"""
        seq = np.ascontiguousarray(seq, np.int32)
        pos = np.ascontiguousarray(pos, np.int64)
        n = len(seq)
        if len(pos) != n:
            raise ValueError("seqpos_to_column: seq and pos differ in length")
        iv = self._co_out(out, 0, (n,), np.int64)
        col = self._co_out(out, 1, (n,), np.int64)
        self._chk(self.L.mauve_seqpos_to_column(self.h, C.c_int64(n), _p(seq, C.c_int32), _p(pos, C.c_int64), _p(iv, C.c_int64), _p(col, C.c_int64)),
                  "mauve_seqpos_to_column")
        return iv, col

    def translate_positions(self, seq, pos, nearest=False, out=None):
        """mauve_translate_positions: (genome, position) -> (out[n, nseq] signed positions in every genome, defined[n], interval[n])"""
        seq = np.ascontiguousarray(seq, np.int32)
        pos = np.ascontiguousarray(pos, np.int64)
        n, N = len(seq), self.coord_index_size()[0]
        if len(pos) != n:
            raise ValueError("translate_positions: seq and pos differ in length")
        res = self._co_out(out, 0, (n, N), np.int64)
        dfn = self._co_out(out, 1, (n,), np.uint32)
        iv = self._co_out(out, 2, (n,), np.int64)
        self._chk(self.L.mauve_translate_positions(self.h, C.c_int64(n), _p(seq, C.c_int32), _p(pos, C.c_int64), int(bool(nearest)),
                                                   _p(res, C.c_int64), _p(dfn, C.c_uint32), _p(iv, C.c_int64)), "mauve_translate_positions")
        return res, dfn, iv

    def _range_args(self, ranges, who):
        """ranges = (iv, col, len) arrays or None (every interval whole) -> (n_range, the four ctypes range arguments)"""
        if ranges is None:
            return self.coord_index_size()[1], (C.c_int64(0), None, None, None)
        arrs = [np.ascontiguousarray(x, np.int64) for x in ranges]
        n = len(arrs[0])
        if not (n == len(arrs[1]) == len(arrs[2])):
            raise ValueError("%s: the range arrays differ in length" % who)
        if n == 0:                                               # (a pointer the library may look at: it reads none of it)
            arrs = [np.zeros(1, np.int64)] * 3
        return n, (C.c_int64(n),) + tuple(_p(a, C.c_int64) for a in arrs)

    # ---- alignment columns as a base matrix ----
    def extract_select(self, keep=None, require=0, drop_empty=False, polymorphic=False, ranges=None):
        """mauve_extract_select: choose the columns (ranges = (iv, col, len) arrays as backbone()'s seg_iv / seg_col / seg_len, None = every
        interval whole) that satisfy the request, and the rows (keep, None = every genome in order).  -> n_sel"""
        p = ExtractParams()
        self.L.mauve_default_extract_params.restype = None
        self.L.mauve_default_extract_params(C.c_int(self.nseq), C.byref(p))
        if keep is not None:
            keep = [int(g) for g in keep]
            if len(keep) > 32:
                raise ValueError("extract: at most 32 rows")
            p.n_keep = len(keep)
            for k, g in enumerate(keep):
                p.keep[k] = g
        p.require, p.drop_empty, p.polymorphic = int(require), int(bool(drop_empty)), int(bool(polymorphic))
        n = C.c_int64(0)
        n_range, args_r = self._range_args(ranges, "extract")
        self._chk(self.L.mauve_extract_select(self.h, C.byref(p), *args_r, C.byref(n)), "mauve_extract_select")
        self._ex_shape = (p.n_keep, n.value, n_range)
        return n.value

    def extract_fetch(self, out=None, lists=True):
        """mauve_extract_fetch of the selection in force -> (rows uint8 [n_keep, n_sel], sel_iv, sel_col, range_off); out = the four arrays
        (e.g. from pinned_empty: copied without staging), rows may be a view of a wider matrix (its row stride is passed on);
        lists=False: the matrix alone (the three lists are not copied: None)"""
        nk, ns, nr = self._ex_shape
        if out is None:
            rows = np.zeros((nk, ns), np.uint8)
        else:
            rows = out[0]
            if rows.dtype != np.uint8 or rows.shape != (nk, ns) or (ns > 1 and rows.strides[1] != 1) or (nk > 1 and rows.strides[0] < ns):
                raise ValueError("extract: out[0] must be a uint8 array of shape %s with contiguous rows" % ((nk, ns),))
        stride = rows.strides[0] if nk > 1 and ns > 0 else max(ns, 1)
        if not lists:
            self._chk(self.L.mauve_extract_fetch(self.h, C.c_void_p(rows.ctypes.data), C.c_int64(stride), None, None, None), "mauve_extract_fetch")
            return rows, None, None, None
        siv = self._co_out(out, 1, (ns,), np.int64)
        scol = self._co_out(out, 2, (ns,), np.int64)
        roff = self._co_out(out, 3, (nr + 1,), np.int64)
        self._chk(self.L.mauve_extract_fetch(self.h, C.c_void_p(rows.ctypes.data), C.c_int64(stride), _p(siv, C.c_int64), _p(scol, C.c_int64), _p(roff, C.c_int64)),
                  "mauve_extract_fetch")
        return rows, siv, scol, roff

    def extract_columns(self, keep=None, require=0, drop_empty=False, polymorphic=False, ranges=None, out=None):
        """select + fetch: the letters of the chosen columns in the chosen genomes, row-major per genome (the projection / core-column /
        SNP matrix of stripGapColumns, projectAndStrip, alignmentProjector).  require: genome mask (int) or a list of genome ids."""
        if not isinstance(require, (int, np.integer)):
            require = sum(1 << int(g) for g in require)
        self.extract_select(keep, require, drop_empty, polymorphic, ranges)
        return self.extract_fetch(out)

    # ---- the alignment as XMFA / MAF text ----
    @staticmethod
    def _c_strings(items):
        """a list of str / bytes / None -> a char* array (None entries stay NULL); None -> NULL"""
        if items is None:
            return None
        enc = [None if s is None else (s if isinstance(s, bytes) else str(s).encode()) for s in items]
        return (C.c_char_p * max(len(enc), 1))(*enc)

    def alignment_text(self, fmt="xmfa", names=None, deflines=None, contigs=None, contig_names=None, ranges=None, wrap=None):
        """mauve_alignment_text: the text of the index in force (ranges as for extract_select, None = every interval whole) into a device
        buffer the context keeps -> (n_bytes, n_blocks).  fmt "xmfa" (wrap: letters per line, None = 80) or "maf" (contigs: per genome
        the 0-based contig starts, contig_names: per genome the names of its contigs; None = every genome is one contig)."""
        if isinstance(fmt, str):
            if fmt not in ("xmfa", "maf"):
                raise ValueError("alignment_text: fmt is 'xmfa' or 'maf'")
            fmt = TEXT_MAF if fmt == "maf" else TEXT_XMFA
        N = self.nseq
        for what, lst in (("names", names), ("deflines", deflines), ("contigs", contigs), ("contig_names", contig_names)):
            if lst is not None and len(lst) != N:
                raise ValueError("alignment_text: %s must have one entry per genome" % what)
        p = TextParams()
        self.L.mauve_default_text_params.restype = None
        self.L.mauve_default_text_params(C.c_int(int(fmt)), C.byref(p))
        if wrap is not None:
            p.wrap = int(wrap)
        n_c = c_st = None
        if contigs is not None:
            per = [np.ascontiguousarray(x, np.int64).reshape(-1) for x in contigs]
            n_c = np.array([len(x) for x in per], np.int64)
            c_st = np.concatenate(per + [np.zeros(1, np.int64)])
        flat = None
        if contig_names is not None:
            if contigs is None:
                raise ValueError("alignment_text: contig_names go with contigs")
            flat = [s for per_g in contig_names for s in per_g]
            if len(flat) != int(n_c.sum()):
                raise ValueError("alignment_text: contig_names must name every contig")
        n_range, args_r = self._range_args(ranges, "alignment_text")
        nb, nk = C.c_int64(0), C.c_int64(0)
        self._tx_shape = None
        self.L.mauve_alignment_text.argtypes = [C.c_void_p, C.POINTER(TextParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        a_names, a_def, a_cn = self._c_strings(names), self._c_strings(deflines), self._c_strings(flat)
        self._chk(self.L.mauve_alignment_text(self.h, C.byref(p), a_names, a_def, None if n_c is None else n_c.ctypes.data, None if c_st is None else c_st.ctypes.data, a_cn,
                                              *args_r, C.byref(nb), C.byref(nk)), "mauve_alignment_text")
        self._tx_shape = (nb.value, n_range)
        return nb.value, nk.value

    def alignment_text_fetch(self, offset=0, length=None, out=None, want_block_off=False):
        """mauve_alignment_text_fetch: the slice [offset, offset + length) of the text in force (length None = to its end) -> bytes, or with
        out (a uint8 array of at least that length, e.g. from pinned_empty: copied without staging) the view out[:length]; with
        want_block_off -> (slice, block_off int64 [n_range + 1])"""
        if getattr(self, "_tx_shape", None) is None:
            n_bytes, n_range = 0, 0                                  # (the library refuses: no text in force)
        else:
            n_bytes, n_range = self._tx_shape
        if length is None:
            length = max(n_bytes - offset, 0)
        length = int(length)
        if out is None:
            buf = np.empty(max(length, 1), np.uint8)
        else:
            buf = out
            if buf.dtype != np.uint8 or buf.ndim != 1 or not buf.flags.c_contiguous or len(buf) < length:
                raise ValueError("alignment_text_fetch: out must be a contiguous uint8 array of at least %d bytes" % length)
        boff = np.zeros(n_range + 1, np.int64) if want_block_off else None
        self.L.mauve_alignment_text_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        self._chk(self.L.mauve_alignment_text_fetch(self.h, C.c_int64(int(offset)), C.c_int64(length), buf.ctypes.data if length else None,
                                                    boff.ctypes.data if want_block_off else None), "mauve_alignment_text_fetch")
        res = buf[:length] if out is not None else buf[:length].tobytes()
        return (res, boff) if want_block_off else res

    # ---- pairwise column statistics ----
    def pair_stats(self, pairs=None, ranges=None, per_range=False, out=None):
        """mauve_pair_stats: what two rows of the alignment show against each other -> int64 records [n_pair, 32], with per_range
        [n_range, n_pair, 32].  pairs = (a, b) id arrays of ordered pairs (None: all pairs a < b, row-major), ranges as for
        extract_select (None: every interval whole), out = the result array (e.g. from pinned_empty: copied without staging)."""
        N = self.coord_index_size()[0]
        z8, z4 = np.zeros(1, np.int64), np.zeros(1, np.int32)
        if pairs is None:
            n_pair, args_p = N * (N - 1) // 2, (C.c_int64(0), None, None)
        else:
            pa, pb = (np.ascontiguousarray(x, np.int32) for x in pairs)
            if pa.ndim != 1 or pa.shape != pb.shape:
                raise ValueError("pair_stats: the pair arrays differ in length")
            n_pair, args_p = len(pa), (C.c_int64(len(pa)), _p(pa if len(pa) else z4, C.c_int32), _p(pb if len(pa) else z4, C.c_int32))
        n_range, args_r = self._range_args(ranges, "pair_stats")
        shape = (n_range, n_pair, PAIR_STATS_WORDS) if per_range else (n_pair, PAIR_STATS_WORDS)
        if n_pair > 1024 or n_pair * (n_range if per_range else 1) > 1 << 24:
            # the library refuses these before it writes a record: nothing to allocate, and its error comes before any word about `out`
            self._chk(self.L.mauve_pair_stats(self.h, *args_p, *args_r, C.c_int(int(bool(per_range))), _p(z8, C.c_int64)), "mauve_pair_stats")
            raise RuntimeError("mauve_pair_stats accepted a request beyond its limits")
        st = self._co_out((out,), 0, shape, np.int64) if out is not None else np.zeros(shape, np.int64)
        self._chk(self.L.mauve_pair_stats(self.h, *args_p, *args_r, C.c_int(int(bool(per_range))), _p(st if st.size else z8, C.c_int64)), "mauve_pair_stats")
        return st

    # ---- excursions of the column scores ----
    def _excursions(self, fn, name, scoring, args_set, n_set, ranges):
        n_range, args_r = self._range_args(ranges, name)
        n = C.c_int64(0)
        self._exc_shape = None
        self._chk(fn(self.h, C.byref(scoring) if scoring is not None else None, *args_set, *args_r, C.byref(n)), "mauve_" + name)
        self._exc_shape = (n.value, n_range * n_set)
        return n.value

    def excursions_pairs(self, pairs=None, ranges=None, scoring=None):
        """mauve_excursions_pairs: the excursions of the negated column scores of genome pairs -> the number of records, kept in the context
        for excursions_fetch.  pairs, ranges as for pair_stats; scoring: a Scoring (None = the default).  Streams: range-major."""
        N = self.coord_index_size()[0]
        z4 = np.zeros(1, np.int32)
        if pairs is None:
            n_pair, args_p = N * (N - 1) // 2, (C.c_int64(0), None, None)
        else:
            pa, pb = (np.ascontiguousarray(x, np.int32) for x in pairs)
            if pa.ndim != 1 or pa.shape != pb.shape:
                raise ValueError("excursions_pairs: the pair arrays differ in length")
            n_pair, args_p = len(pa), (C.c_int64(len(pa)), _p(pa if len(pa) else z4, C.c_int32), _p(pb if len(pa) else z4, C.c_int32))
        return self._excursions(self.L.mauve_excursions_pairs, "excursions_pairs", scoring, args_p, n_pair, ranges)

    def excursions_core(self, groups=None, ranges=None, scoring=None):
        """mauve_excursions_core: the excursions over the columns in which every genome of a group has a residue; groups: genome masks
        (ints) or lists of genome ids, None = one group of every genome"""
        self.coord_index_size()
        if groups is None:
            n_group, args_g = 1, (C.c_int64(0), None)
        else:
            gm = np.ascontiguousarray([g if isinstance(g, (int, np.integer)) else sum(1 << int(t) for t in g) for g in groups], np.uint32).reshape(-1)
            n_group, args_g = len(gm), (C.c_int64(len(gm)), _p(gm if len(gm) else np.zeros(1, np.uint32), C.c_uint32))
        return self._excursions(self.L.mauve_excursions_core, "excursions_core", scoring, args_g, n_group, ranges)

    def excursions_fetch(self, out=None, want=(True, True, True, True)):
        """mauve_excursions_fetch of the result in force -> (height[n_exc], end_col[n_exc], stream_off[n_stream + 1], tail[n_stream, 2]);
        out = the four arrays (e.g. from pinned_empty: copied without staging); want: which of the four to copy (the others: None)"""
        shape = getattr(self, "_exc_shape", None)
        if shape is None:                                        # no result: the library says so (nothing is written)
            self._chk(self.L.mauve_excursions_fetch(self.h, None, None, None, None), "mauve_excursions_fetch")
            raise RuntimeError("mauve_excursions_fetch ran without a result")
        ne, ns = shape
        shapes = ((ne,), (ne,), (ns + 1,), (ns, 2))
        arrs = [self._co_out(out, q, shapes[q], np.int64) if want[q] else None for q in range(4)]
        self._chk(self.L.mauve_excursions_fetch(self.h, *[_p(a, C.c_int64) if a is not None and a.size else None for a in arrs]), "mauve_excursions_fetch")
        return tuple(arrs)

    # ---- projection onto a genome subset ----
    def project(self, proj=None, drop_empty=True):
        """mauve_project: the index in force projected onto the genomes proj (None = every genome in order), collinear intervals coalesced;
        the result stays in the context for project_fetch / project_index.  -> dict(n_iv, n_cols, n_src, n_fill)"""
        N = self.coord_index_size()[0]
        p = default_project_params(N)
        if proj is not None:
            proj = [int(g) for g in proj]
            if len(proj) > 32:
                raise ValueError("project: at most 32 genomes")
            p.n_proj = len(proj)
            for k, g in enumerate(proj):
                p.proj[k] = g
        p.drop_empty = int(bool(drop_empty))
        sz = ProjectSizes()
        self._pj_shape = None
        self._chk(self.L.mauve_project(self.h, C.byref(p), C.byref(sz)), "mauve_project")
        self._pj_shape = (N, p.n_proj, sz.n_iv, sz.n_cols, sz.n_src)
        return {k: getattr(sz, k) for k, _ in ProjectSizes._fields_}

    PROJECT_ARRAYS = ("left", "right", "reverse", "col_off", "cols", "src_off", "src_iv", "src_flip", "src_col")

    def project_fetch(self, compact=False, out=None, want=None):
        """mauve_project_fetch of the projection in force -> dict of left, right, reverse [n_iv, nseq] (compact: [n_iv, n_proj], bit k of a
        column = genome proj[k]), col_off, cols, src_off, src_iv, src_flip, src_col; out = dict of destination arrays (e.g. from
        pinned_empty: copied without staging); want: the names to copy (None = all; the others are None)"""
        shape = getattr(self, "_pj_shape", None)
        if shape is None:                                        # no result: the library says so (nothing is written)
            self._chk(self.L.mauve_project_fetch(self.h, 0, *([None] * 9)), "mauve_project_fetch")
            raise RuntimeError("mauve_project_fetch ran without a projection")
        N, npj, n_iv, n_cols, n_src = shape
        w = npj if compact else N
        spec = {"left": ((n_iv, w), np.int64), "right": ((n_iv, w), np.int64), "reverse": ((n_iv, w), np.int8), "col_off": ((n_iv + 1,), np.int64),
                "cols": ((n_cols,), np.uint32), "src_off": ((n_iv + 1,), np.int64), "src_iv": ((n_src,), np.int64), "src_flip": ((n_src,), np.int8),
                "src_col": ((n_cols,), np.int64)}
        res, args = {}, []
        for name in self.PROJECT_ARRAYS:
            shp, dt = spec[name]
            if want is not None and name not in want:
                res[name] = None
                args.append(None)
                continue
            a = out[name] if out is not None and name in out else np.zeros(shp, dt)
            if a.dtype != np.dtype(dt) or a.shape != shp or not a.flags.c_contiguous:
                raise ValueError("project_fetch: out[%r] must be a contiguous %s array of shape %s" % (name, np.dtype(dt).name, shp))
            res[name] = a
            args.append(C.c_void_p(a.ctypes.data) if a.size else None)
        self.L.mauve_project_fetch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 9
        self._chk(self.L.mauve_project_fetch(self.h, int(bool(compact)), *args), "mauve_project_fetch")
        return res

    def project_index(self):
        """mauve_project_index: the projection in force becomes the index in force (its columns stay on the device)"""
        self._chk(self.L.mauve_project_index(self.h), "mauve_project_index")

    # ---- annotated ranges mapped through the alignment, the interval-overlap join ----
    def map_ranges(self, seq, lo, hi):
        """mauve_map_ranges: the ranges [lo, hi] (1-based) of the genomes seq cut into their pieces, one per interval of the index in force
        that they intersect; the result stays in the context for map_ranges_fetch.  -> dict(n_query, n_piece)"""
        seq = np.ascontiguousarray(seq, np.int32)
        lo = np.ascontiguousarray(lo, np.int64)
        hi = np.ascontiguousarray(hi, np.int64)
        n = len(seq)
        if seq.ndim != 1 or lo.shape != seq.shape or hi.shape != seq.shape:
            raise ValueError("map_ranges: seq, lo and hi differ in length")
        z8, z4 = np.zeros(1, np.int64), np.zeros(1, np.int32)
        sz = RangeMapSizes()
        self._fm_shape = None
        self._chk(self.L.mauve_map_ranges(self.h, C.c_int64(n), _p(seq if n else z4, C.c_int32), _p(lo if n else z8, C.c_int64), _p(hi if n else z8, C.c_int64), C.byref(sz)),
                  "mauve_map_ranges")
        self._fm_shape = (self.coord_index_size()[0], sz.n_query, sz.n_piece)
        return dict(n_query=sz.n_query, n_piece=sz.n_piece)

    RANGE_MAP_ARRAYS = ("piece_off", "covered", "best", "piece_query", "piece_iv", "piece_col", "piece_len", "clip_lo", "clip_hi", "n_res", "ext_left", "ext_right")

    def map_ranges_fetch(self, out=None, want=None):
        """mauve_map_ranges_fetch of the range map in force -> dict of piece_off [n + 1], covered, best [n], piece_query, piece_iv, piece_col,
        piece_len, clip_lo, clip_hi [n_piece], n_res, ext_left, ext_right [n_piece, nseq]; out = dict of destination arrays (e.g. from
        pinned_empty: copied without staging); want: the names to copy (None = all; the others are None)"""
        shape = getattr(self, "_fm_shape", None)
        self.L.mauve_map_ranges_fetch.argtypes = [C.c_void_p] * 13
        if shape is None:                                        # no result: the library says so (nothing is written)
            self._chk(self.L.mauve_map_ranges_fetch(self.h, *([None] * 12)), "mauve_map_ranges_fetch")
            raise RuntimeError("mauve_map_ranges_fetch ran without a range map")
        N, n, P = shape
        shapes = [(n + 1,), (n,), (n,)] + [(P,)] * 6 + [(P, N)] * 3
        res, args = {}, []
        for name, shp in zip(self.RANGE_MAP_ARRAYS, shapes):
            if want is not None and name not in want:
                res[name] = None
                args.append(None)
                continue
            a = out[name] if out is not None and name in out else np.zeros(shp, np.int64)
            if a.dtype != np.int64 or a.shape != shp or not a.flags.c_contiguous:
                raise ValueError("map_ranges_fetch: out[%r] must be a contiguous int64 array of shape %s" % (name, shp))
            res[name] = a
            args.append(C.c_void_p(a.ctypes.data) if a.size else None)
        self._chk(self.L.mauve_map_ranges_fetch(self.h, *args), "mauve_map_ranges_fetch")
        return res

    def range_overlaps(self, tab, queries, out=None):
        """mauve_range_overlaps: tab = (seq, lo, hi) arrays of annotated ranges in any order, queries = (seq, lo, hi) arrays, signed ends
        allowed and (0, 0) = nothing (a column of map_ranges_fetch's ext_left / ext_right goes in as it is) -> (n_hit, best, overlap) per
        query: the table entries sharing a base with it, the table index of the one sharing the most (ties: the greater index) and that
        number of bases; (0, -1, 0) without a hit.  out = the three result arrays (e.g. from pinned_empty)"""
        ts, qs = np.ascontiguousarray(tab[0], np.int32), np.ascontiguousarray(queries[0], np.int32)
        tl, th, ql, qh = (np.ascontiguousarray(x, np.int64) for x in (tab[1], tab[2], queries[1], queries[2]))
        m, n = len(ts), len(qs)
        if ts.ndim != 1 or tl.shape != ts.shape or th.shape != ts.shape or qs.ndim != 1 or ql.shape != qs.shape or qh.shape != qs.shape:
            raise ValueError("range_overlaps: the arrays of the table or of the queries differ in length")
        z8, z4 = np.zeros(1, np.int64), np.zeros(1, np.int32)
        res = [self._co_out(out, k, (n,), np.int64) for k in range(3)]
        self._chk(self.L.mauve_range_overlaps(self.h, C.c_int64(m), _p(ts if m else z4, C.c_int32), _p(tl if m else z8, C.c_int64), _p(th if m else z8, C.c_int64),
                                              C.c_int64(n), _p(qs if n else z4, C.c_int32), _p(ql if n else z8, C.c_int64), _p(qh if n else z8, C.c_int64),
                                              *[_p(a if n else z8, C.c_int64) for a in res]), "mauve_range_overlaps")
        return tuple(res)

    # ---- an alignment scored against a correct one ----
    def score_truth(self, aln):
        """mauve_score_truth: the correct alignment (dict with left, right, reverse, col_off, cols, e.g. accuracy.truth_alignment or a fetched
        result) into the context's second index slot; it stays through index calls, alignments and genome uploads"""
        left = np.ascontiguousarray(aln["left"], np.int64)
        right = np.ascontiguousarray(aln["right"], np.int64)
        reverse = np.ascontiguousarray(aln["reverse"], np.int8)
        col_off = np.ascontiguousarray(aln["col_off"], np.int64)
        cols = np.ascontiguousarray(aln["cols"], np.uint32)
        if left.ndim != 2 or right.shape != left.shape or reverse.shape != left.shape:
            raise ValueError("score_truth: left, right and reverse must be [n_iv, nseq]")
        n_iv, N = left.shape
        self._chk(self.L.mauve_score_truth(self.h, N, C.c_int64(n_iv), _p(left, C.c_int64), _p(right, C.c_int64), _p(reverse, C.c_int8),
                                           _p(col_off, C.c_int64), _p(cols if len(cols) else np.zeros(1, np.uint32), C.c_uint32)), "mauve_score_truth")
        self._score_n = N

    def score_alignment(self, out=None):
        """mauve_score_alignment: the index in force against the correct alignment -> int64 records [N, N, 8] (tp, fp_base, fp_gap,
        fn_unaligned, fn_base, tn, 0, 0 per ordered pair); out = the result array (e.g. from pinned_empty: copied without staging)"""
        N = getattr(self, "_score_n", 0)
        if N == 0:                                               # no truth: the library says so (nothing is written)
            self._chk(self.L.mauve_score_alignment(self.h, _p(np.zeros(SCORE_WORDS, np.int64), C.c_int64)), "mauve_score_alignment")
            raise RuntimeError("mauve_score_alignment ran without a correct alignment")
        rec = self._co_out((out,), 0, (N, N, SCORE_WORDS), np.int64) if out is not None else np.zeros((N, N, SCORE_WORDS), np.int64)
        self._chk(self.L.mauve_score_alignment(self.h, _p(rec, C.c_int64)), "mauve_score_alignment")
        return rec

    # ---- a repeat map scored against a correct repeat alignment ----
    REPEAT_SCORE_ARRAYS = ("pair_records", "comp_hit", "pair_hit")

    def repeat_score(self, records=None, row_offset=None, want=REPEAT_SCORE_ARRAYS, out=None):
        """mauve_repeat_score: the truth of score_truth, its rows the copy slots of a repeat, against a repeat map.  records = (length, mult,
        start_off, starts) as repeat_matches returns them, or None = the result of the last repeat_matches where it lies on the device.
        row_offset [nseq]: genome bases in front of every row's origin (None: zeros).  -> dict(totals = dict of the 8 counters, pair_records
        [nseq, nseq, 4], comp_hit [n] uint32, pair_hit [n_starts] uint32); want: the tables to copy (the others are None); out = dict of
        destination arrays (e.g. from pinned_empty: copied without staging)"""
        N = getattr(self, "_score_n", 0)
        self.L.mauve_repeat_score.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + [C.POINTER(RepeatScoreTotals)] + [C.c_void_p] * 3
        tot = RepeatScoreTotals()
        ro = None
        if row_offset is not None:
            ro = np.ascontiguousarray(row_offset, np.int64)
            if N and ro.shape != (N,):
                raise ValueError("repeat_score: row_offset must have one entry per row of the truth")
        if records is None:
            n, ns = getattr(self, "_rm_shape", (0, 0))
            lst = [None] * 4
        else:
            length, mult, off, st = (np.ascontiguousarray(a, np.int64) for a in records)
            n = len(length)
            if length.ndim != 1 or mult.shape != (n,) or off.shape != (n + 1,) or st.ndim != 1 or (n and len(st) != int(off[n])):
                raise ValueError("repeat_score: records = (length [n], mult [n], start_off [n + 1], starts [start_off[n]])")
            ns = len(st)
            z = np.zeros(1, np.int64)
            lst = [(a if a.size else z) for a in (length, mult, off, st)]
        shapes = {"pair_records": ((N, N, REPEAT_SCORE_WORDS), np.int64), "comp_hit": ((n,), np.uint32), "pair_hit": ((ns,), np.uint32)}
        res, args = {}, []
        for name in self.REPEAT_SCORE_ARRAYS:
            shp, dt = shapes[name]
            if name not in want or N == 0:
                res[name] = None
                args.append(None)
                continue
            a = out[name] if out is not None and name in out else np.zeros(shp, dt)
            if a.dtype != np.dtype(dt) or a.shape != shp or not a.flags.c_contiguous:
                raise ValueError("repeat_score: out[%r] must be a contiguous %s array of shape %s" % (name, np.dtype(dt).name, shp))
            res[name] = a
            args.append(C.c_void_p(a.ctypes.data) if a.size else None)
        self._chk(self.L.mauve_repeat_score(self.h, C.c_int64(n), *[None if a is None else C.c_void_p(a.ctypes.data) for a in lst],
                                            None if ro is None else C.c_void_p(ro.ctypes.data), C.byref(tot), *args), "mauve_repeat_score")
        res["totals"] = {k: int(getattr(tot, k)) for k, _ in RepeatScoreTotals._fields_}
        return res

    def stage_times(self):
        t = StageTimes()
        self.L.mauve_last_stage_times(self.h, C.byref(t))
        return {k: getattr(t, k) for k, _ in StageTimes._fields_}

    def profile(self, on=True):
        self.L.mauve_profile_enable(self.h, int(on))

    def profile_reset(self):
        self.L.mauve_profile_reset(self.h)

    def profile_get(self):
        out = {}
        for i, nm in enumerate(KERNEL_NAMES):
            ms, ln, un = C.c_double(), C.c_int64(), C.c_int64()
            self.L.mauve_profile_get(self.h, i, C.byref(ms), C.byref(ln), C.byref(un))
            out[nm] = {"ms": ms.value, "launches": ln.value, "units": un.value}
        return out
