"""The seed's run table as the extraction kernels hold it: one (shift, mask) pair per run of care positions in scalar
registers, the loop over the runs unrolled over the whole table and left after a group of four, the genome of a window group picked out of
the scalar copy of the genome table.  Checked against tests/seed_ref.py (window_mers, find) on every weight of the seed table (one- and
two-word windows, 32- and 64-bit keys), on a solid seed (one run) and on alternating patterns with as many runs as the table has room for
-- the last group of the one-word table (15 runs), the most a span of 32 holds (16), and a span above 32 with 25 -- through the
single-genome list (seed_extract), the one-workgroup pass (tiny_join), the tiled pass (seed_extract_all, strand bitmap, sort, join_hash)
with genome borders and the end of the buffer inside a thread's four windows, and more than eight genomes (the indexed table)."""
import numpy as np
import pytest

from tests import seed_ref as R

pytestmark = pytest.mark.gpu

TILE, TINY_MAX = 4096, 9216


def alternating(span):
    return int("10" * (span // 2) + "1", 2)


ALT29, ALT31, ALT49 = alternating(29), alternating(31), alternating(49)      # 15, 16 and 25 runs
SOLID = (1 << 11) - 1


def runs_of(pat):
    return len([r for r in bin(pat)[2:].split("0") if r])


def make_case(lens, seed, rate=0.03):
    """substitution-only copies of one ancestor (its first len bases), the middle tenth of genome 1 replaced by its reverse complement"""
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 4, max(lens), dtype=np.uint8)
    gs = []
    for L in lens:
        g = anc[:L].copy()
        hit = np.flatnonzero(rng.random(L) < rate)
        g[hit] = (g[hit] + rng.integers(1, 4, len(hit), dtype=np.uint8)) & 3
        gs.append(g)
    a, b = int(lens[1] * 0.45), int(lens[1] * 0.55)
    gs[1][a:b] = (3 - gs[1][a:b])[::-1]
    return gs


def windows(lens, pat):
    span = len(bin(pat)) - 2
    return sum(max(0, L - span + 1) for L in lens)


@pytest.fixture(scope="module")
def ctx():
    from mauvealigner_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lib():
    from mauvealigner_amd import _lib
    return _lib


# ---- the sorted mer list of one genome: keys and strands of every window ----
@pytest.fixture(scope="module")
def one_genome():
    return make_case((3001, 3001), 7)[1]                   # (with its inverted stretch)


def list_patterns(lib):
    return [(("w%d" % w), lib.get_seed(w, 0)) for w in range(3, 32)] + [("alt29", ALT29), ("alt31", ALT31), ("alt49", ALT49), ("solid", SOLID)]


def test_patterns_are_what_they_claim(lib):
    assert [runs_of(p) for p in (ALT29, ALT31, ALT49, SOLID)] == [15, 16, 25, 1]
    assert len(bin(ALT31)) - 2 == 31 and len(bin(ALT49)) - 2 == 49
    spans = {w: lib.seed_length(lib.get_seed(w, 0)) for w in range(3, 32)}
    assert any(s <= 32 for w, s in spans.items() if w <= 15) and any(s > 32 for s in spans.values())     # one- and two-word windows


@pytest.mark.parametrize("which", range(29 + 4))
def test_sorted_mer_list(ctx, lib, one_genome, which):
    name, pat = list_patterns(lib)[which]
    weight = bin(pat).count("1")
    F, Rv = R.window_mers(one_genome, pat)
    canon, strand = np.minimum(F, Rv), (Rv < F).astype(np.uint64)
    order = np.lexsort((np.arange(len(canon)), canon))
    emer = (canon[order] << np.uint64(64 - 2 * weight)) | strand[order]
    ctx.set_genomes([one_genome])
    mer, pos = ctx.sorted_mer_list(0, pat)
    assert strand.any() and not strand.all(), name
    assert np.array_equal(pos, order) and np.array_equal(mer, emer), name


# ---- seed_mums against find ----
def layout(kind, pat):
    """the genome lengths of a layout; none a multiple of 4 or 32, so groups of four windows straddle the genome ends"""
    if kind == "tiny3":
        lens = [1003, 1777, 2501]
    elif kind == "tiled5":
        lens = [9001, 8999, 9003, 9002, 8997]
        if windows(lens, pat) % 4 == 0:
            lens[-1] -= 2                                   # the last group of four is cut by P
    elif kind == "nine":
        lens = [1501 + 10 * i for i in range(9)]
    else:
        lens = [901 + 6 * i for i in range(9)]              # "nine_tiny"
    assert all(L % 4 and L % 32 for L in lens)
    return lens


MUM_PATTERNS = ["w9", "w15", "w19", "alt29", "alt31", "alt49"]
_cases = {}


def case(lib, kind, name):
    """genomes and the reference of both finders, made once"""
    if (kind, name) not in _cases:
        pat = {"alt29": ALT29, "alt31": ALT31, "alt49": ALT49}.get(name) or lib.get_seed(int(name[1:]), 0)
        lens = layout(kind, pat)
        gs = make_case(lens, 11 + len(lens))
        refs = {}
        for mode in (R.MEM, R.UNIQUE):
            ref = R.find(gs, pat, mode=mode, mask=0, extend=True)
            refs[mode] = (np.array(ref["length"], np.int64), np.array(ref["start"], np.int64).reshape(-1, len(gs)))
        _cases[(kind, name)] = (pat, lens, gs, refs)
    return _cases[(kind, name)]


@pytest.mark.parametrize("name", MUM_PATTERNS)
@pytest.mark.parametrize("kind", ["tiny3", "tiled5", "nine", "nine_tiny"])
def test_seed_mums(ctx, lib, kind, name):
    pat, lens, gs, refs = case(lib, kind, name)
    P = windows(lens, pat)
    if kind in ("tiny3", "nine_tiny"):
        assert P <= TINY_MAX
    else:
        assert P > TINY_MAX and P % TILE != 0
    if kind == "tiled5":
        assert P % 4 != 0
    ctx.set_genomes(gs)
    for mode in (R.MEM, R.UNIQUE):
        eln, est = refs[mode]
        assert len(eln) > 0 and (est < 0).any(), "the reference found no match on the reverse strand"
        ln, st = ctx.seed_mums(pat, mode=mode, mask=0, extend=True)
        assert np.array_equal(ln, eln) and np.array_equal(st, est), (kind, name, mode)
