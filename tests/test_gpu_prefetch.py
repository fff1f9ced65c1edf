"""mauve_align_prefetch: the match list and the anchor table travel into the caller's page-locked buffers while mauve_align is still
running.  Every case is compared bit for bit, on every returned array, with a plain compact fetch of the same alignment into pageable
memory (which goes through the context's host copy: another path altogether); where a table must have been sent, or must not have been,
the buffers are looked at between mauve_align and the fetch."""
import ctypes as C

import numpy as np
import pytest

from mauvealigner_amd import synth

pytestmark = pytest.mark.gpu

TABLES = ("mum_length", "mum_start", "anchor_length", "anchor_start", "anchor_lcb")
ARRAYS = TABLES + ("lcb_left", "lcb_right", "lcb_weight", "left", "right", "reverse", "col_off", "cols", "dp_score")
SENTINEL = -0x5A5A5A5B


@pytest.fixture(scope="module")
def lib():
    from mauvealigner_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def genomes():
    return synth.make_config("C3", scale=0.4)          # 5 x 2 Mbp: the match list is long enough to stay on the device (device tail)


def _same(r, ref):
    for k in ARRAYS:
        assert r[k].dtype == ref[k].dtype and np.array_equal(r[k], ref[k]), k
    for k in ("n_mums", "n_lcb", "n_anchor", "n_iv", "n_cols", "n_gap_dp"):
        assert r[k] == ref[k], k


def _tables(lib, N, nm, na):
    """page-locked buffers of nm match records and na anchor records, filled with a value no table holds"""
    a = {"mum_length": lib.pinned_empty(max(nm, 1), np.int32), "mum_start": lib.pinned_empty(max(nm, 1) * N, np.int32),
         "anchor_length": lib.pinned_empty(max(na, 1), np.int32), "anchor_start": lib.pinned_empty(max(na, 1) * N, np.int32),
         "anchor_lcb": lib.pinned_empty(max(na, 1), np.int32)}
    for v in a.values():
        v[:] = SENTINEL
    return a


def _register(lib, ctx, a, nm, na):
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    ctx.L.mauve_align_prefetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    ctx._chk(ctx.L.mauve_align_prefetch(ctx.h, vp(a["mum_length"]), vp(a["mum_start"]), nm, vp(a["anchor_length"]), vp(a["anchor_start"]),
                                        vp(a["anchor_lcb"]), na), "mauve_align_prefetch")


def _align(lib, ctx, p):
    sz = lib.AlignSizes()
    ctx._chk(ctx.L.mauve_align(ctx.h, C.byref(p), C.byref(sz)), "mauve_align")
    return sz


def _bufs_of(lib, a):
    b = lib.ResultBuffers()
    for k, v in a.items():
        b._a["c_" + k] = v
    return b


def _untouched(a, names):
    return all((a[k] == SENTINEL).all() for k in names)


def _arrived(a, ref, names):
    return all(np.array_equal(a[k][:ref[k].size], ref[k].ravel()) for k in names)


MUMS, ANCH = ("mum_length", "mum_start"), ("anchor_length", "anchor_start", "anchor_lcb")


@pytest.mark.parametrize("dm,da", [(0, 0), (1000, 3000), (-1, 0), (0, -1), (-1, -1)])
def test_capacities(lib, ctx, genomes, dm, da):
    """exact and generous capacities deliver; a capacity one record short leaves that table to the fetch, the other still travels"""
    N = len(genomes)
    ctx.set_genomes(genomes)
    p = lib.default_params(seed_weight=15)
    ref = ctx.align(p, compact=True)
    assert ref["n_mums"] >= 16384, "the workload no longer reaches the device tail: the cases below would test nothing"
    nm, na = ref["n_mums"] + dm, ref["n_anchor"] + da
    a = _tables(lib, N, nm, na)
    _register(lib, ctx, a, nm, na)
    sz = _align(lib, ctx, p)
    assert _arrived(a, ref, MUMS) if dm >= 0 else _untouched(a, MUMS)
    assert _arrived(a, ref, ANCH) if da >= 0 else _untouched(a, ANCH)
    _same(ctx._fetch_compact(sz, _bufs_of(lib, a)), ref)


def test_other_pointers_at_fetch_and_second_fetch(lib, ctx, genomes):
    N = len(genomes)
    ctx.set_genomes(genomes)
    p = lib.default_params(seed_weight=15)
    ref = ctx.align(p, compact=True)
    a = _tables(lib, N, ref["n_mums"], ref["n_anchor"])
    _register(lib, ctx, a, ref["n_mums"], ref["n_anchor"])
    sz = _align(lib, ctx, p)
    other = _tables(lib, N, ref["n_mums"], ref["n_anchor"])
    _same(ctx._fetch_compact(sz, _bufs_of(lib, other)), ref)          # fresh page-locked buffers: copied from the device
    for v in a.values():
        v[:] = SENTINEL                                               # after a fetch the registered buffers are the caller's again
    _same(ctx._fetch_compact(sz, _bufs_of(lib, a)), ref)              # ... and a fetch into them copies
    _same(ctx._fetch_compact(sz), ref)                                # pageable


def test_never_fetched_then_next_alignment(lib, ctx, genomes):
    N = len(genomes)
    ctx.set_genomes(genomes)
    p = lib.default_params(seed_weight=15)
    ref = ctx.align(p, compact=True)
    a = _tables(lib, N, ref["n_mums"], ref["n_anchor"])
    _register(lib, ctx, a, ref["n_mums"], ref["n_anchor"])
    _align(lib, ctx, p)                                               # delivered, never fetched
    g2 = [g[::-1].copy() for g in genomes[:3]]                        # other genomes, another count
    ctx.set_genomes(g2)
    ref2 = ctx.align(p, compact=True)
    bufs = lib.ResultBuffers()
    for _ in range(3):                                                # the binding's own route: registered from the second round on
        ctx.set_genomes(g2)
        _same(ctx.align(p, out=bufs, compact=True), ref2)
    ctx.set_genomes(genomes)
    _same(ctx.align(p, out=bufs, compact=True), ref)                  # buffers registered with the old sizes: too small or not, same result


def test_one_registration_one_alignment(lib, ctx, genomes):
    N = len(genomes)
    ctx.set_genomes(genomes)
    p = lib.default_params(seed_weight=15)
    ref = ctx.align(p, compact=True)
    a = _tables(lib, N, ref["n_mums"], ref["n_anchor"])
    _register(lib, ctx, a, ref["n_mums"], ref["n_anchor"])
    _align(lib, ctx, p)
    assert _arrived(a, ref, TABLES)
    for v in a.values():
        v[:] = SENTINEL
    sz = _align(lib, ctx, p)                                          # the registration is used up
    assert _untouched(a, TABLES)
    _same(ctx._fetch_compact(sz, _bufs_of(lib, a)), ref)


def test_pageable_and_null_buffers_are_not_used(lib, ctx, genomes):
    N = len(genomes)
    ctx.set_genomes(genomes)
    p = lib.default_params(seed_weight=15)
    ref = ctx.align(p, compact=True)
    nm, na = ref["n_mums"], ref["n_anchor"]
    a = _tables(lib, N, nm, na)
    a["mum_start"] = np.full(nm * N, SENTINEL, np.int32)              # pageable: the match list stays behind, the anchors travel
    _register(lib, ctx, a, nm, na)
    sz = _align(lib, ctx, p)
    assert _untouched(a, MUMS) and _arrived(a, ref, ANCH)
    _same(ctx._fetch_compact(sz, _bufs_of(lib, a)), ref)
    ctx.L.mauve_align_prefetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    ctx._chk(ctx.L.mauve_align_prefetch(ctx.h, None, None, 0, None, None, None, 0), "mauve_align_prefetch")
    _same(ctx.align(p, compact=True), ref)


@pytest.mark.parametrize("kw,delivers", [({"extend_lcbs": 0}, True), ({"min_recursive_gap": 30}, False), ({"lcb_scoring": 1}, False)])
def test_other_paths(lib, ctx, genomes, kw, delivers):
    """extension off: the anchors are chain_order_device's own; gaps for the recursion, score-weighted LCBs: the call leaves the device tail and
    sends nothing -- same result either way"""
    N = len(genomes)
    ctx.set_genomes(genomes)
    p = lib.default_params(seed_weight=15, **kw)
    ref = ctx.align(p, compact=True)
    a = _tables(lib, N, ref["n_mums"] + 8, ref["n_anchor"] + 8)
    _register(lib, ctx, a, ref["n_mums"] + 8, ref["n_anchor"] + 8)
    sz = _align(lib, ctx, p)
    assert _arrived(a, ref, TABLES) if delivers else _untouched(a, TABLES)
    _same(ctx._fetch_compact(sz, _bufs_of(lib, a)), ref)


def test_small_genomes_and_backbone_without_fetch(lib, ctx):
    """tens of kilobases: the list is sorted on the host and nothing is sent; and fetch=False followed by the backbone"""
    small = synth.make_config("C3", scale=0.01)
    ctx.set_genomes(small)
    p = lib.default_params(seed_weight=11)
    ref = ctx.align(p, compact=True)
    bufs = lib.ResultBuffers()
    for _ in range(2):
        _same(ctx.align(p, out=bufs, compact=True), ref)
    big = synth.make_config("C3", scale=0.4)
    ctx.set_genomes(big)
    p = lib.default_params(seed_weight=15)
    ref = ctx.align(p, compact=True)
    bref = ctx.backbone(island_gap=20)
    bufs = lib.ResultBuffers()
    _same(ctx.align(p, out=bufs, compact=True), ref)
    ctx.align(p, fetch=False, out=bufs, compact=True)                 # registered and delivered, not fetched
    b = ctx.backbone(island_gap=20)
    for k in bref:
        assert np.array_equal(b[k], bref[k]), k
