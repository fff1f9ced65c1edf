"""The device chain stage (chain_dev.hip: the genomes' orders and overlap clusters made up front, one launch per genome, the LCB
graph by flag compactions, the greedy step on the host over the device-built graph) on the planted lists of tests/chain_cases.py:
tile edges of the 1024-entry tiles, clusters of 47 / 48 / 49 around CH_CL_MAX, workgroups that outgrow the LDS pool of
ch_cluster_pass, ties, LCB graphs with a live greedy step, 5 / 17 / 32 genomes, sort keys of 8 | 9, 16 | 17 and 24 | 25 bits, and
random dense lists of 900 .. 2300 matches with their ties kept, at the density of tests/test_gpu_chain_upfront.py (each is one
cluster: 40 hand-backs) and with the span scaled to the list (chained on the device).  tests/test_chain_cpu.py shows from the reference that every
case is where it was aimed.

Every list goes through ctx.align_matches (recursive=0, gapped=0, extend_lcbs=0) at each of its (lcb_weight, collinear) settings;
anchor_length, anchor_start, anchor_lcb, lcb_weight, lcb_left and lcb_right must be those of the oracle's elimination and LCBs,
and on the small cases those of tests/chain_ref.py directly.  The trace line of chain_device_graph must be there exactly when no
overlap cluster of the list AS GIVEN (chain_ref.input_facts) exceeds the limit: a larger one hands the list to the host chain.

The switches are read once per process, so every variant is a child process of its own (with a time limit; a child that faults,
aborts or runs out of time fails its test and nothing more is started from it): the default, MAUVE_CH_CL_MAX=5,
MAUVE_SMALL_SORT=0 (one tiled sort per genome instead of the batched one) and MAUVE_HOST_CHAIN=1 (the host route on the same
inputs).  One context per child, reused across the cases of its families."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import os, sys, tempfile
import numpy as np
sys.path.insert(0, %(root)r)
from mauvealigner_amd import _lib
from oracle import pyoracle as O
from tests import chain_cases as C, chain_ref as R

LINE = "chain (device): eliminate+nodes+graph"
KEYS = ("anchor_length", "anchor_start", "anchor_lcb", "lcb_weight", "lcb_left", "lcb_right")
limit = min(int(os.environ.get("MAUVE_CH_CL_MAX", C.CL_MAX)), C.CL_MAX)
host_only = "MAUVE_HOST_CHAIN" in os.environ


class Stderr:                                    # what the library writes to stderr during one call
    def __enter__(self):
        sys.stderr.flush()
        self.f = tempfile.TemporaryFile()
        self.old = os.dup(2)
        os.dup2(self.f.fileno(), 2)
        return self
    def __exit__(self, *a):
        os.dup2(self.old, 2); os.close(self.old)
        self.f.seek(0); self.text = self.f.read().decode(errors="replace"); self.f.close()


def chain_of(el, es, lc, N):
    el = np.asarray(el, np.int64); es = np.asarray(es, np.int64).reshape(len(el), N); ml = np.asarray(lc["match_lcb"], np.int64)
    keep = np.flatnonzero(ml >= 0)
    keep = keep[np.argsort(ml[keep], kind="stable")]           # LCB by LCB, genome-0 order inside
    K = int(lc["n_lcb"])
    return {"anchor_length": el[keep], "anchor_start": es[keep], "anchor_lcb": ml[keep],
            "lcb_weight": np.asarray(lc["weight"], np.int64).reshape(K), "lcb_left": np.asarray(lc["left_end"], np.int64).reshape(K, N),
            "lcb_right": np.asarray(lc["right_end"], np.int64).reshape(K, N)}


ctx = _lib.Context(0)
runs = on_device = 0
for fam in sys.argv[1:]:
    for case in C.family(fam):
        N, ln, st = case["N"], np.asarray(case["length"], np.int64), np.asarray(case["start"], np.int64)
        ctx.set_genomes(C.genomes(case))
        facts = R.input_facts(case["length"], case["start"])
        top = max(s for g in range(N) for _, s in facts["clusters"][g])
        device = top <= limit and not host_only
        if not host_only and case["device"] is not None and ("MAUVE_CH_CL_MAX" in os.environ) == (fam == "cluster_cl5"):
            assert device == case["device"], case["name"]      # (what the case was planted for: the limit it names)
        el, es = O.eliminate_overlaps(ln, st)
        ref = R.eliminate_overlaps(case["length"], case["start"]) if case["small"] else None
        for w, col in case["runs"]:
            p = _lib.default_params(recursive=0, gapped=0, extend_lcbs=0, lcb_weight=w, collinear=col)
            with Stderr() as cap:
                r = ctx.align_matches(p, ln, st)
            seen = cap.text.count(LINE)
            assert seen == (1 if device else 0), (case["name"], w, col, "trace lines", seen, "largest cluster", top, cap.text[-600:])
            want = [("oracle", chain_of(el, es, O.compute_lcbs(el, es, w, bool(col)), N))]
            if ref:
                want.append(("reference", chain_of(ref["length"], ref["start"], R.compute_lcbs(ref["length"], ref["start"], w, bool(col)), N)))
            for who, e in want:
                assert r["n_lcb"] == len(e["lcb_weight"]) and r["n_anchor"] == len(e["anchor_length"]), \
                    (case["name"], w, col, who, r["n_lcb"], len(e["lcb_weight"]), r["n_anchor"], len(e["anchor_length"]))
                for k in KEYS:
                    assert np.array_equal(np.asarray(r[k], np.int64).reshape(e[k].shape), e[k]), (case["name"], w, col, who, k)
            runs += 1; on_device += device
ctx.close()
print("runs", runs, "device", on_device, "OK")
"""

GAPPED = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
from mauvealigner_amd import _lib
from tests import chain_cases as C, chain_ref as R
case = C.gapped_case()
ctx = _lib.Context(0)
ctx.set_genomes(C.genomes(case))
p = _lib.default_params(recursive=0, gapped=1, extend_lcbs=0, lcb_weight=0)
r = ctx.align_matches(p, np.asarray(case["length"], np.int64), np.asarray(case["start"], np.int64))
ctx.close()
e = R.chain(case["length"], case["start"], 0)
assert e["elim"]["reordered"]                      # the crops reorder genome 0: the chain order is not the list order
assert r["anchor_length"].tolist() == e["anchor_length"] and r["anchor_start"].tolist() == e["anchor_start"]
assert r["anchor_lcb"].tolist() == e["anchor_lcb"] and r["n_gap_dp"] > 0
np.savez(sys.argv[1], **{k: v for k, v in r.items() if isinstance(v, np.ndarray)})
print("OK")
"""


def _child(script, args, **env):
    full = dict(os.environ, MAUVE_TRACE="1", MAUVE_CANON_DEVICE_MIN="1", **env)
    r = subprocess.run([sys.executable, "-c", script % {"root": ROOT}] + list(args), env=full, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.split(), r.stderr.splitlines()


def _counts(out):
    return int(out[out.index("runs") + 1]), int(out[out.index("device") + 1])


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["tile", "cluster", "cluster_cl5", "pool", "ties", "graph", "wide", "key", "dense", "dense_scaled"])
def test_planted_lists_on_the_device_chain(family):
    """(the worker requires the trace line of every run whose largest cluster, by the reference, is within the limit; the counts
    below say how many those were)"""
    runs, device = _counts(_child(WORKER, [family])[0])
    if family == "dense":
        # 900 matches and more in a span of 200 .. 4000: every list is one cluster, the device hands all 40 back and the host chain
        # takes them -- these runs check the hand-back, nothing on the device; the lists of dense_scaled are the random ones it chains
        assert runs == 40 and device == 0
    elif family == "dense_scaled":
        assert runs == 24 and 2 * device >= runs
    else:
        assert runs > 0 and device > 0
    if family in ("ties", "graph", "wide", "key", "pool"):
        assert device == runs


@pytest.mark.gpu
def test_cluster_limit_of_five():
    """MAUVE_CH_CL_MAX=5: clusters of 5 stay on the device, a cluster of 6 hands the list back; so do the clusters of 47 .. 49, and the
    tie families with more than five matches in a cluster"""
    runs, device = _counts(_child(WORKER, ["cluster_cl5", "cluster", "ties"], MAUVE_CH_CL_MAX="5")[0])
    assert 0 < device < runs


@pytest.mark.gpu
def test_one_tiled_sort_per_genome():
    """MAUVE_SMALL_SORT=0: the orders come from one tiled sort per genome; the sort-key widths on both sides of a pass-count change
    again (where the orders land depends on the parity of the passes), the wide lists, the ties and the tile edges"""
    runs, device = _counts(_child(WORKER, ["key", "wide", "ties", "tile"], MAUVE_SMALL_SORT="0")[0])
    assert device == runs - 1 > 0                       # (all but the long match's list, whose cluster is beyond the limit)


@pytest.mark.gpu
@pytest.mark.parametrize("families", [("tile", "pool"), ("cluster", "cluster_cl5", "ties", "key", "wide"), ("graph", "dense", "dense_scaled")],
                         ids=["tile_pool", "clusters_ties_widths", "graph_dense"])
def test_the_host_route_on_the_same_lists(families):
    runs, device = _counts(_child(WORKER, families, MAUVE_HOST_CHAIN="1")[0])
    assert runs > 0 and device == 0


@pytest.mark.gpu
def test_gapped_alignment_behind_a_reordering_elimination(tmp_path):
    """N = 3 on 5000-base genomes, 300 collinear matches with short gaps behind a family whose crops carry a match past its
    neighbour in genome 0; gapped=1, recursive=0.  The survivors come back from the device in list order and chain_device_copy_back
    puts them into the order along genome 0 that everything behind it reads; every fetched array equals the host chain's, with and
    without MAUVE_HOST_TAIL.  (A caller's list never takes the device tail -- mauve_align_matches does not ask for it -- so co_keys /
    co_gather are not reached from here: tests/test_gpu_align.py::test_chain_order_after_the_elimination stays their cover.  For
    the same reason MAUVE_HOST_TAIL is not consulted on this route today and that child runs the default child's code; it is kept
    so that the comparison is in place the day a caller's list does take the device tail.)"""
    got = {}
    for tag, env in (("default", {}), ("host_tail", {"MAUVE_HOST_TAIL": "1"}), ("host_chain", {"MAUVE_HOST_CHAIN": "1"})):
        path = str(tmp_path / (tag + ".npz"))
        _, err = _child(GAPPED, [path], **env)
        got[tag] = dict(np.load(path))
        on_device = any("chain (device): eliminate+nodes+graph" in l for l in err)
        assert on_device == (tag != "host_chain"), (tag, err[-20:])
    for tag in ("host_tail", "host_chain"):
        assert set(got[tag]) == set(got["default"])
        for k in got["default"]:
            assert np.array_equal(got[tag][k], got["default"][k]), (tag, k)
