"""The recursive anchoring of the product (csrc/recursive.cpp, the segmented instantiations of csrc/seed_pass.hip, the
per-gap chain routes of csrc/chain_dev.hip) on the planted genomes of tests/recursion_cases.py: the four conditions of gap_weight
on their limits, three levels and three weight classes in one level, segment starts and totals on word borders, forward and
reverse gaps, the same stretch in two gaps, a seam and a straddling window, matches cropped at a gap's end, 1 .. 1024 gaps in one
batch, ties and merges of the collinear rule, overlap clusters of 48 | 49, gaps of 512 | 513 nodes and 2560 | 2592 links, 2 .. 32
genomes, ambiguity and contig bitmaps.  tests/test_recursion_cpu.py shows from the reference that every case is where it was aimed.

Every case goes through its entry point (mauve_align, or mauve_align_lcbs from the root LCB table): the match list, anchor_length,
anchor_start, anchor_lcb, lcb_weight and n_lcb must be those of tests/recursion_ref.py and (plain genomes) of the oracle; the gapped
entries are compared with the oracle's whole result, the two progressive entries with the oracle's and with the reference's batches
for the node over genomes {1, 2}.  From the trace: one `recursion level L weight W: K gaps, B bases, M matches`
line per batch, in the reference's order and with its numbers (M: the N-way matches before the forward filter), and the route of
every `per-gap chaining (...)` line as the variant and the case prescribe.  After every case that found anchors the same context
runs the case that finds nothing.

The switches are read once per process, so every variant is a child process of its own (with a time limit; a child that faults,
aborts or runs out of time fails its test and nothing more is started from it).  The references and the oracle's results are
computed once, in the parent, and handed to the children in a file."""
import atexit
import functools
import os
import pickle
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import os, pickle, re, sys, tempfile
import numpy as np
sys.path.insert(0, %(root)r)
from mauvealigner_amd import _lib
from tests import recursion_cases as C
from tests.align_helpers import whole_compare

with open(sys.argv[1], "rb") as f:
    WANT = pickle.load(f)
MODE = sys.argv[2]
BATCH = re.compile(r"recursion level (\d+) weight (\d+): (\d+) gaps, (\d+) bases, (\d+) matches")
ROUTE = re.compile(r"per-gap chaining [-+.0-9e]+ ms \(([^;]+);")
SURV, BACK, HOST = "device, survivors only", "device", "host"


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


def run(ctx, case):
    name, N, w = case["name"], case["N"], WANT[case["name"]]
    ref, orc = w.get("ref"), w.get("oracle")
    p = _lib.default_params(**case["params"])
    gapped = bool(case["params"]["gapped"])
    ctx.set_genomes(case["genomes"], contig_starts=case["contigs"], invalid=case["invalid"])
    if case["entry"] == "progressive":           # the oracle's whole result (tests/test_recursion_cpu.py holds it to the reference), and the
        with Stderr() as cap:                    # batches of the node over genomes {1, 2} as tests/recursion_ref.py has them for the pair
            r = ctx.progressive_align(p, want_xmfa=True, tree=case["tree"])
        whole_compare(r, w["full"], "progressive", N, dist=False)
        got = [tuple(int(x) for x in m) for m in BATCH.findall(cap.text)]
        assert got == [tuple(b[:5]) for b in w["batches"]], (name, "the node over genomes {1, 2} searches its gaps", got, w["batches"])
        return {SURV: 0, BACK: 0, HOST: 0}, True
    with Stderr() as cap:
        try:
            if case["entry"] == "resume":
                r = ctx.align_lcbs(p, ref["root"][0], ref["root"][1], ref["root"][2])
            else:
                r = ctx.align(p, want_xmfa=gapped)
        except Exception as ex:                  # (name the case: the library's message does not)
            raise RuntimeError((name, str(ex))) from None
    t = cap.text
    want = [("reference", ref["anchor_length"], ref["anchor_start"], ref["anchor_lcb"])]
    if orc is not None:
        want.append(("oracle",) + orc[:3])
    for who, al, ast, alcb in want:
        got = (r["anchor_length"].tolist(), r["anchor_start"].tolist(), r["anchor_lcb"].tolist())
        for k, g, e in zip(("anchor_length", "anchor_start", "anchor_lcb"), got, (list(al), [list(x) for x in ast], list(alcb))):
            assert g == e, (name, who, k, len(g), len(e), [x for x in g if x not in e][:4], [x for x in e if x not in g][:4], t[-600:])
    if case["entry"] == "align":
        assert r["mum_length"].tolist() == list(ref["mums"][0]) and r["mum_start"].tolist() == [list(x) for x in ref["mums"][1]], (name, "mums")
        assert r["n_lcb"] == ref["n_lcb"] and r["lcb_weight"].tolist() == list(ref["lcb_weight"]), (name, "lcbs", r["n_lcb"], r["lcb_weight"].tolist())
        if orc is not None:
            assert r["n_lcb"] == orc[3] and r["lcb_weight"].tolist() == orc[4], (name, "oracle", "lcbs")
        if gapped:
            whole_compare(r, w["full"], "align", N)
    elif gapped:
        a = w["full"]["aln"]
        for k in ("left", "right", "reverse", "col_off", "cols", "dp_score"):
            assert np.array_equal(r[k], a[k]), (name, "resume", k)
    # ---- the batches and their routes, from the trace ----
    got = [tuple(int(x) for x in m) for m in BATCH.findall(t)]
    assert got == [tuple(b[:5]) for b in ref["batches"]], (name, "batches", got, ref["batches"])
    routes = ROUTE.findall(t)
    assert len(routes) == len(got), (name, "one route per batch", routes)
    tally = {SURV: 0, BACK: 0, HOST: 0}
    for (lv, wt, K, bases, nm, overlap, cluster, beyond), route in zip(ref["batches"], routes):
        if MODE == "host" or nm == 0:
            exp = (HOST,)
        elif case["contigs"] is not None or case["invalid"] is not None:
            exp = (SURV, BACK, HOST)             # (a masked segmented pass sorts on another route: not prescribed here)
        elif MODE == "allback":
            exp = (BACK,)
        elif MODE == "bigmax" and cluster > 2:
            exp = (HOST,)                        # both device routes decline
        elif MODE == "bigmax" and overlap:
            exp = (SURV, BACK, HOST)             # (a cluster may grow past 2 while the passes crop)
        else:
            exp = (BACK,) if beyond else (SURV,)
        assert route in exp, (name, "route", (lv, wt, K, nm), route, exp)
        if len(exp) == 1:
            tally[route] += 1
    return tally, len(ref["anchor_length"]) > len(ref["root"][0])


ctx = _lib.Context(0)
nothing = next(c for c in C.all_cases() if c["name"] == C.NOTHING)
runs, total = 0, {SURV: 0, BACK: 0, HOST: 0}
for fam in sys.argv[3:]:
    for case in C.family(fam):
        tally, found = run(ctx, case)
        runs += 1
        for k, v in tally.items():
            total[k] += v
        if found:
            run(ctx, nothing)                     # stale state of the batches before must not show
ctx.close()
print("runs", runs, "survivors", total[SURV], "allback", total[BACK], "host", total[HOST], "OK")
"""


def _batches(case, ref):
    """per batch in the order they run: level, weight, gaps, bases of virtual genome 0, N-way matches before the forward filter;
    then what the routes depend on: do forward matches of one gap overlap in some genome, the largest overlap cluster of the batch
    (tests/chain_ref.py: input_facts), and is a gap of the batch beyond the device's greedy step (declared by the case)"""
    from tests import chain_ref as CH, recursion_ref as R
    out = []
    for (lv, w), recs in ref["batches"].items():
        cluster = 1
        for r in recs:
            if len(r["forward"]) > 1:
                facts = CH.input_facts([l for l, _ in r["forward"]], [s for _, s in r["forward"]])
                cluster = max([cluster] + [sz for g in range(case["N"]) for _, sz in facts["clusters"][g]])
        beyond = lv == 1 and bool(case["aim"].get("beyond"))
        out.append((lv, w, len(recs), R.virtual_layout(recs)[0]["total"], sum(len(r["matches"]) for r in recs), cluster > 1, cluster, beyond))
    return out


@functools.lru_cache(maxsize=None)
def _wanted():
    """the reference's and the oracle's results of every case, computed once and written where the children read them"""
    from oracle import pyoracle as O
    from tests import recursion_cases as C
    want = {}
    for case in C.all_cases():
        if case["entry"] == "progressive":
            want[case["name"]] = {"full": O.progressive_align(case["genomes"], O.default_params(**case["params"]), want_xmfa=True, tree=case["tree"]),
                                  "batches": _batches({"N": 2, "aim": {}}, C.pair_reference(case))}
            continue
        ref = C.reference(case)
        orc = full = None
        if case["oracle"]:
            e = O.align(case["genomes"], O.default_params(**case["params"]), want_xmfa=bool(case["params"]["gapped"]))
            a = e["aln"]
            orc = (a["anchor_length"].tolist(), a["anchor_start"].tolist(), a["anchor_lcb"].tolist(), e["lcbs"]["n_lcb"], e["lcbs"]["weight"].tolist())
            if case["params"]["gapped"]:
                full = e
        root = ref["root"]
        want[case["name"]] = {"oracle": orc, "full": full,
                              "ref": {"mums": ref["mums"], "anchor_length": ref["anchor_length"], "anchor_start": ref["anchor_start"], "anchor_lcb": ref["anchor_lcb"],
                                      "n_lcb": ref["n_lcb"], "lcb_weight": ref["lcb_weight"], "batches": _batches(case, ref),
                                      "root": (root["anchor_length"], root["anchor_start"], root["anchor_lcb"])}}
    fd, path = tempfile.mkstemp(suffix=".pkl", prefix="recursion_want_")
    with os.fdopen(fd, "wb") as f:
        pickle.dump(want, f)
    atexit.register(os.unlink, path)
    return path


def _child(mode, families, **env):
    full = dict(os.environ, MAUVE_TRACE="1", **env)
    r = subprocess.run([sys.executable, "-c", WORKER % {"root": ROOT}, _wanted(), mode] + list(families), env=full, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-3000:]
    out = r.stdout.split()
    return tuple(int(out[out.index(k) + 1]) for k in ("runs", "survivors", "allback", "host"))


def _declared(mode, families):
    """(cases, batches that must take the survivors-only route, the all-back route, the host route) of these families in this
    variant, from what tests/recursion_cases.py declares and the reference's batches -- the child's own rule, counted here"""
    from tests import recursion_cases as C
    cases = [c for f in families for c in C.family(f)]
    n = {"s": 0, "b": 0, "h": 0}
    for c in cases:
        if c["entry"] == "progressive":
            continue
        masked = c["contigs"] is not None or c["invalid"] is not None
        for lv, w, K, bases, nm, overlap, cluster, beyond in _batches(c, C.reference(c)):
            if mode == "host" or nm == 0:
                n["h"] += 1
            elif masked:
                pass
            elif mode == "allback":
                n["b"] += 1
            elif mode == "bigmax" and cluster > 2:
                n["h"] += 1
            elif mode == "bigmax" and overlap:
                pass
            else:
                n["b" if beyond else "s"] += 1
    return len(cases), n["s"], n["b"], n["h"]


ALL = ("rule", "levels", "gather", "segments", "count", "chain", "limits", "width", "bitmaps", "entries")


@pytest.mark.gpu
def test_small_lists_take_the_host_route():
    got = _child("host", ALL)
    assert got == _declared("host", ALL) and got[1] == got[2] == 0 and got[3] > 0


@pytest.mark.gpu
def test_the_device_route_sends_survivors_only_and_falls_back_beyond_its_limits():
    """MAUVE_CANON_DEVICE_MIN=1.  The limits cases: all back exactly for 513 nodes, 81 x 32 and 427 x 6 links; 512, 80 and 426 stay"""
    got = _child("survivors", ALL, MAUVE_CANON_DEVICE_MIN="1")
    assert got == _declared("survivors", ALL) and got[2] == 3 and got[1] > 0


@pytest.mark.gpu
def test_the_device_route_through_the_general_segmented_kernels():
    """MAUVE_NO_TINY=1: the SEG instantiations of the hash join, not the one-workgroup pass"""
    got = _child("survivors", ALL, MAUVE_CANON_DEVICE_MIN="1", MAUVE_NO_TINY="1")
    assert got == _declared("survivors", ALL) and got[2] == 3


@pytest.mark.gpu
def test_every_batch_through_the_all_back_route():
    got = _child("allback", ALL, MAUVE_CANON_DEVICE_MIN="1", MAUVE_GAP_CHAIN_ALL_BACK="1")
    assert got == _declared("allback", ALL) and got[1] == 0 and got[2] > 0


@pytest.mark.gpu
def test_the_host_loop_behind_the_device_lists():
    got = _child("host", ALL, MAUVE_CANON_DEVICE_MIN="1", MAUVE_HOST_GAP_CHAIN="1")
    assert got == _declared("host", ALL) and got[1] == got[2] == 0


@pytest.mark.gpu
def test_overlap_clusters_beyond_the_per_thread_limit():
    """MAUVE_CH_CL_MAX=2: ch_cluster_pass_big takes the clusters of the chain and limits families; the routes stay"""
    fam = ("chain", "limits")
    got = _child("survivors", fam, MAUVE_CANON_DEVICE_MIN="1", MAUVE_CH_CL_MAX="2")
    assert got == _declared("survivors", fam) and got[2] == 3


@pytest.mark.gpu
def test_both_device_routes_decline_and_the_host_fetches_the_list():
    """... plus MAUVE_CH_BIG_MAX=2: a cluster of three or more makes both device routes return the limit status; the host route then
    fetches the list the seed pass left on the device (seed_matches_to_host), and nothing changes in the result"""
    fam = ("chain", "limits")
    got = _child("bigmax", fam, MAUVE_CANON_DEVICE_MIN="1", MAUVE_CH_CL_MAX="2", MAUVE_CH_BIG_MAX="2")
    assert got == _declared("bigmax", fam) and got[3] >= 3


@pytest.mark.gpu
def test_the_device_route_with_wide_indices():
    fam = ("gather", "segments", "count")
    got = _child("survivors", fam, MAUVE_CANON_DEVICE_MIN="1", MAUVE_WIDE_INDEX="1")
    assert got == _declared("survivors", fam) and got[1] > 0
