"""The LCB extension of the product (extend_lcbs_device and its kernels in csrc/extend_dev.hip, the host rounds
extend_lcbs of csrc/pipeline.cpp) on the planted genomes of tests/extend_cases.py: pieces of exactly one seed length, separators on
word, wave and block edges, the match the separator has to cut, rounds that keep, drop and renumber, weights on the limit, kept
matches slipped into anchor lists of 255 .. 513, recursion gaps of exactly min_recursive_gap, 2 .. 32 genomes, and the inputs that
must keep the host form.  tests/test_extend_cpu.py shows from the reference that every case is where it was aimed.

Every case goes through ctx.align (recursive = 0, gapped = 0): the fetched match list, anchor_length, anchor_start, anchor_lcb,
lcb_weight and n_lcb must be those of tests/extend_ref.py and (plain genomes) of the oracle; all 19 merge cases and one case of
every other family also run gapped, with the recursion as planted, against the oracle's whole path.  From the trace: the device form's round lines are there exactly when
the variant and the case allow the device form, with the reference's count of new matches per round, its kept / dropped and its
LCB counts; the host rounds' lines likewise; and the anchors stay on the device or come to the host as the reference's count of
recursion gaps says.  After every case that kept something the same context runs one that keeps nothing.

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
from tests import extend_cases as C, extend_ref as R
from tests.align_helpers import whole_compare

with open(sys.argv[1], "rb") as f:
    WANT = pickle.load(f)
env = os.environ
dev_variant = "MAUVE_CANON_DEVICE_MIN" in env and "MAUVE_HOST_EXTEND" not in env
decline = "MAUVE_EXT_DECLINE" in env
DEV_ROUND = re.compile(r"lcb extension \(device\) round (\d+): pieces .* (\d+) new matches")
DEV_UNITS = re.compile(r"lcb extension \(device\) round (\d+): units .* (\d+) -> (\d+) LCBs, (kept|dropped)")
HOST_ROUND = re.compile(r"lcb extension round (\d+): mask .* (\d+) new matches")
STAY, TO_HOST = "LCBs stay there", "extended anchors to the host"


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


def params(case, **kw):
    p = dict(case["params"]); p.update(kw)
    return _lib.default_params(**p)


def run(ctx, case):
    name, N, ref, orc = case["name"], case["N"], WANT[case["name"]]["ref"], WANT[case["name"]]["oracle"]
    ctx.set_genomes(case["genomes"], contig_starts=case["contigs"], invalid=case["invalid"])
    with Stderr() as cap:
        try:
            r = ctx.align(params(case, recursive=0, gapped=0))
        except Exception as ex:                  # (name the case: the library's message does not)
            raise RuntimeError((name, str(ex))) from None
    t = cap.text
    want = [("reference", ref["mums"][0], ref["mums"][1], ref["anchor_length"], ref["anchor_start"], ref["anchor_lcb"], ref["n_lcb"],
             ref["lcb_weight"] if case["params"]["lcb_scoring"] == 0 else None)]
    if orc is not None:
        want.append(("oracle",) + orc)
    for who, ml, ms, al, ast, alcb, nl, lw in want:
        got = (r["mum_length"].tolist(), r["mum_start"].tolist(), r["anchor_length"].tolist(), r["anchor_start"].tolist(), r["anchor_lcb"].tolist(), r["n_lcb"])
        exp = (list(ml), [list(x) for x in ms], list(al), [list(x) for x in ast], list(alcb), nl)
        for k, g, e in zip(("mum_length", "mum_start", "anchor_length", "anchor_start", "anchor_lcb", "n_lcb"), got, exp):
            assert g == e, (name, who, k, g if k == "n_lcb" else len(g), e if k == "n_lcb" else len(e), t[-800:])
        if lw is not None:
            assert r["lcb_weight"].tolist() == list(lw), (name, who, "lcb_weight")
    # ---- the route and the rounds, from the trace ----
    entered = [(q["round"], len(q["new"])) for q in ref["rounds"] if not q["starved"]]
    units = [(q["round"], q["lcb_before"], q["lcb_rechained"], "kept" if q["kept"] else "dropped") for q in ref["rounds"] if q["new"]]
    dev = [(int(a), int(b)) for a, b in DEV_ROUND.findall(t)]
    dun = [(int(a), int(b), int(c), d) for a, b, c, d in DEV_UNITS.findall(t)]
    host = [(int(a), int(b)) for a, b in HOST_ROUND.findall(t)]
    on_device = dev_variant and case["device"]
    if not on_device:
        assert "lcb extension (device)" not in t and host == entered, (name, "host route", dev, host, entered)
    elif decline and units:
        first = units[0][0]
        assert dev == [x for x in entered if x[0] <= first] and dun == [] and host == entered, (name, "declined", dev, dun, host, entered)
        last_dev = max(m.end() for m in DEV_ROUND.finditer(t))
        assert last_dev < HOST_ROUND.search(t).start(), (name, "the host rounds follow the device form's last line")
    else:
        assert "lcb extension (device)" in t and dev == entered and dun == units and host == [], (name, "device route", dev, dun, host, entered, units)
        if len(ref["anchor_length"]) >= 2:
            assert STAY in t and TO_HOST not in t, (name, "recursive = 0: the anchors stay on the device")
    took_device = int("lcb extension (device)" in t and not host)
    # ---- the whole path, with the recursion as planted ----
    if case["full"] and WANT[name]["full"] is not None:
        with Stderr() as cap:
            rf = ctx.align(params(case, gapped=1), want_xmfa=True)
        whole_compare(rf, WANT[name]["full"], "align", N)
        if on_device and not decline:
            gaps = len(R.rec_gaps(ref["anchor_length"], ref["anchor_start"], ref["anchor_lcb"], case["params"]["min_recursive_gap"]))
            leaves = bool(case["params"]["recursive"]) and gaps > 0 or len(ref["anchor_length"]) < 2
            assert (TO_HOST in cap.text) == leaves and (STAY in cap.text) == (not leaves), (name, "tail", gaps, cap.text[-600:])
    return took_device, any(q["kept"] for q in ref["rounds"])


ctx = _lib.Context(0)
nothing = next(c for c in C.all_cases() if c["name"] == "lone_short_n2")       # finds a match, keeps nothing
runs = device = 0
for fam in sys.argv[2:]:
    for case in C.family(fam):
        d, kept = run(ctx, case)
        runs += 1; device += d
        if kept:
            run(ctx, nothing)                     # stale state of the kept round must not show
ctx.close()
print("runs", runs, "device", device, "OK")
"""


@functools.lru_cache(maxsize=None)
def _wanted():
    """the reference's and the oracle's results of every case, computed once and written where the children read them"""
    from oracle import pyoracle as O
    from tests import extend_cases as C
    want = {}
    for case in C.all_cases():
        ref = C.reference(case)
        p = {k: v for k, v in case["params"].items()}
        orc = full = None
        if case["contigs"] is None and case["invalid"] is None:      # (the oracle's whole path takes no ambiguity / contig tables)
            e = O.align(case["genomes"], O.default_params(**dict(p, recursive=0, gapped=0)))
            ml, ms = O.multiplicity_filter(e["mums"][0], e["mums"][1], case["N"])
            a = e["aln"]
            orc = (ml.tolist(), ms.tolist(), a["anchor_length"].tolist(), a["anchor_start"].tolist(), a["anchor_lcb"].tolist(), e["lcbs"]["n_lcb"],
                   e["lcbs"]["weight"].tolist() if p["lcb_scoring"] == 0 else None)
            if case["full"]:
                full = O.align(case["genomes"], O.default_params(**dict(p, gapped=1)), want_xmfa=True)
        want[case["name"]] = {"ref": {k: ref[k] for k in ("mums", "anchor_length", "anchor_start", "anchor_lcb", "n_lcb", "lcb_weight")}, "oracle": orc, "full": full}
        want[case["name"]]["ref"]["rounds"] = [{k: q[k] for k in ("round", "new", "starved", "kept", "lcb_before", "lcb_rechained")} for q in ref["rounds"]]
    fd, path = tempfile.mkstemp(suffix=".pkl", prefix="extension_want_")
    with os.fdopen(fd, "wb") as f:
        pickle.dump(want, f)
    atexit.register(os.unlink, path)
    return path


def _child(families, **env):
    full = dict(os.environ, MAUVE_TRACE="1", **env)
    r = subprocess.run([sys.executable, "-c", WORKER % {"root": ROOT}, _wanted()] + list(families), env=full, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-3000:]
    out = r.stdout.split()
    return int(out[out.index("runs") + 1]), int(out[out.index("device") + 1])


def _declared(families):
    """(cases, cases that may take the device form) of these families, as tests/extend_cases.py declares them"""
    from tests import extend_cases as C
    cases = [c for f in families for c in C.family(f)]
    return len(cases), sum(1 for c in cases if c["device"])


ALL = ("pieces", "rounds", "weights", "merge", "width", "host")


@pytest.mark.gpu
def test_small_lists_take_the_host_chain_and_the_host_rounds():
    runs, device = _child(ALL)
    assert runs == _declared(ALL)[0] and device == 0


@pytest.mark.gpu
def test_the_device_form():
    """MAUVE_CANON_DEVICE_MIN=1: device chain, extend_lcbs_device, device tail"""
    runs, device = _child(ALL, MAUVE_CANON_DEVICE_MIN="1")
    assert (runs, device) == _declared(ALL) and device > 0


@pytest.mark.gpu
def test_the_device_form_through_the_general_seed_route():
    """MAUVE_NO_TINY=1: the virtual genomes go through the hash join, not through the one-workgroup pass"""
    runs, device = _child(ALL, MAUVE_CANON_DEVICE_MIN="1", MAUVE_NO_TINY="1")
    assert (runs, device) == _declared(ALL) and device > 0


@pytest.mark.gpu
def test_the_host_rounds_behind_the_device_chain():
    runs, device = _child(ALL, MAUVE_CANON_DEVICE_MIN="1", MAUVE_HOST_EXTEND="1")
    assert runs == _declared(ALL)[0] and device == 0


@pytest.mark.gpu
def test_the_hand_back():
    """MAUVE_EXT_DECLINE=1: the first device round that finds matches hands the call back, the host rounds follow from round 0; a
    call whose rounds find nothing is finished on the device"""
    from tests import extend_cases as C
    runs, device = _child(ALL, MAUVE_CANON_DEVICE_MIN="1", MAUVE_EXT_DECLINE="1")
    silent = sum(1 for c in C.all_cases() if c["device"] and not any(q["new"] for q in C.reference(c)["rounds"]))
    assert runs == _declared(ALL)[0] and device == silent


@pytest.mark.gpu
def test_the_device_form_with_wide_indices():
    fam = ("pieces", "merge")
    runs, device = _child(fam, MAUVE_CANON_DEVICE_MIN="1", MAUVE_WIDE_INDEX="1")
    assert (runs, device) == _declared(fam) and device > 0
