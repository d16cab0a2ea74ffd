"""Column-aware dealing of the lane-group column-sweep plans (csrc/sgcn_csplan.cpp, sgcn_tune "cs_deal"): the plan still
encodes the matrix exactly, carries fewer pads and a shorter heaviest tile than the weight-only LPT dealing, keeps the
bins' real nonzeros as balanced, does not depend on the number of building threads, and with the knob at 0 is the plan the
library built before the knob existed (digests recorded from that build in tests/golden/csplan_deal_parent.json)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

from stochastic_gcn_amd import synthetic
from stochastic_gcn_amd._ffi import check, lib
from test_csplan import _build, _skewed_csr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "csplan_deal_parent.json")
PAD = 0x80000000


@pytest.fixture(autouse=True)
def _restore_knob():
    before = lib.sgcn_tune_get(b"cs_deal")
    yield
    check(lib.sgcn_tune(b"cs_deal", before))


def _deal(v):
    check(lib.sgcn_tune(b"cs_deal", v))


def _digest(arrays):
    h = hashlib.sha256()
    for x in arrays:
        x = np.ascontiguousarray(x)
        h.update(("%s%s" % (x.dtype.str, x.shape)).encode())
        h.update(x.tobytes())
    return h.hexdigest()


def _check(a, plan, G, rnd, align, tab=None, sh=0):
    """The plan encodes `a` exactly; returns (steps of the heaviest tile, pad fraction, real nonzeros of the heaviest bin)."""
    a = a.tocsr()
    tp, cr, vo, tr, ts, fx, ns = plan
    nt, ne = tp.shape[0] - 1, cr.shape[0]
    assert tp[0] == 0 and tp[-1] == ne
    assert (np.diff(tp) % 64 == 0).all()                               # whole chunks of 64 entries
    if rnd and nt > rnd // 2:
        assert nt % rnd == 0                                           # whole launches
    u = cr.view(np.uint32)
    real = vo.view(np.uint32) != PAD
    assert real.sum() == a.nnz
    e = np.arange(ne)
    tile = np.repeat(np.arange(nt), np.diff(tp))
    g = (e - tp[tile]) % G
    cols = (u & 0x0FFFFFFF).astype(np.int64)
    assert (cols < max(a.shape[1], 1)).all()                           # pads gather from a column of the matrix too
    rows = tr[tile * 16 * G + g * 16 + (u >> 28).astype(np.int64)]
    assert (rows[real] >= 0).all()
    want = a.copy()
    want.data = np.where(want.data.view(np.uint32) == PAD, np.float32(0.0), want.data)      # (a real -0.0f is stored as +0.0f)
    got = sp.coo_matrix((vo[real], (rows[real], cols[real])), shape=a.shape).tocsr()
    assert abs(got - want).nnz == 0 and got.nnz <= a.nnz
    # every nonzero ONCE: (row, column) pairs of the plan = those of the matrix, as multisets
    key_got = np.sort(rows[real].astype(np.int64) * a.shape[1] + cols[real])
    coo = a.tocoo()
    assert np.array_equal(key_got, np.sort(coo.row.astype(np.int64) * a.shape[1] + coo.col))
    # columns ascend inside a bin
    bin_id = tile * G + g
    o = np.argsort(bin_id[real], kind='stable')
    bs, cs = bin_id[real][o], cols[real][o]
    assert ((np.diff(cs) >= 0) | (np.diff(bs) != 0)).all()
    # a step's applied entries lie within `align` positions of its slowest bin
    if align and ne:
        pos = (tab[cols >> sh] if tab is not None else cols).astype(np.int64)
        p2 = np.where(real, pos, np.iinfo(np.int64).max).reshape(-1, G)
        lo = p2.min(axis=1, keepdims=True)
        assert (np.where(real.reshape(-1, G), p2 - lo, 0) <= align).all()
    # split rows: consecutive slots per row, in row order
    trr, tss = tr.reshape(-1), ts.reshape(-1)
    slot = 0
    for r, first, cnt in fx:
        assert first == slot and sorted(tss[trr == r].tolist()) == list(range(first, first + cnt))
        slot += cnt
    assert slot == ns[0] and ((tss >= 0).sum() == slot)
    per_bin = np.bincount(bin_id[real], minlength=max(nt * G, 1))
    return int(np.diff(tp).max() // G) if nt else 0, 1.0 - a.nnz / max(ne, 1), int(per_bin.max())


@pytest.fixture(scope="module")
def small_reddit():
    return synthetic.reddit_like(n=23296, m=1160000, splits=(15241, 2369, 5533), seed=1, with_features=False)[2].tocsr()


CASE1 = [(2, 256, 224), (4, 128, 224)]


@pytest.fixture(scope="module")
def small_plans(small_reddit):
    """(G, deal) -> plan of the small S-Reddit, built once"""
    before = lib.sgcn_tune_get(b"cs_deal")
    out = {}
    for G, rnd, align in CASE1:
        for deal in (0, 1):
            _deal(deal)
            out[G, deal] = _build(small_reddit, G, 4, rnd=rnd, align=align)
    _deal(before)
    return out


@pytest.mark.parametrize("G,rnd,align", CASE1)
def test_column_aware_dealing_pads_less_and_keeps_the_balance(small_reddit, small_plans, G, rnd, align):
    """(the issue's prototype: G = 2 1,632 -> 1,568 steps, pads 0.0392 -> 0.0227; G = 4 1,664 -> 1,584, 0.0609 -> 0.0306)"""
    s0, p0, b0 = _check(small_reddit, small_plans[G, 0], G, rnd, align)
    s1, p1, b1 = _check(small_reddit, small_plans[G, 1], G, rnd, align)
    print("G=%d  steps of the heaviest tile %d -> %d  pad fraction %.4f -> %.4f  heaviest bin %d -> %d" % (G, s0, s1, p0, p1, b0, b1))
    assert p0 > 0.01                                                   # pads exist: the case proves something
    assert s1 <= s0 - 32
    assert p1 <= 0.7 * p0
    assert b1 <= b0 + 16


@pytest.mark.parametrize("G,rnd,align", CASE1)
def test_plan_does_not_depend_on_threads_and_count_agrees(small_reddit, small_plans, G, rnd, align):
    a = small_reddit
    rowptr, col = np.ascontiguousarray(a.indptr, np.int32), np.ascontiguousarray(a.indices, np.int32)
    for deal in (0, 1):
        _deal(deal)
        ref = small_plans[G, deal]
        for threads in (1, 3, 8):
            got = _build(a, G, threads, rnd=rnd, align=align)
            for x, y in zip(ref, got):
                assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        nt, ne, nf, ns = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        check(lib.sgcn_csplang_count(rowptr.ctypes.data, col.ctypes.data, a.shape[0], 0, rnd, align, G, None, 0,
                                     C.byref(nt), C.byref(ne), C.byref(nf), C.byref(ns)))
        assert (nt.value, ne.value, nf.value, ns.value) == (ref[0].shape[0] - 1, ref[1].shape[0], ref[5].shape[0], int(ref[6][0]))


@pytest.mark.parametrize("G", [2, 4])
def test_histograms_are_taken_in_sweep_positions(G):
    """a skewed matrix with a warp table: a dealing that counted column ids would balance the wrong curve"""
    from stochastic_gcn_amd import ops
    a = _skewed_csr(20000, 30000, 400000, 5)
    tab, sh = ops.ColumnSweepCSR.make_warp(np.ascontiguousarray(a.indices, np.int32), a.shape[1], True)
    rnd, align = 64, 256
    stats = []
    for deal in (0, 1):
        _deal(deal)
        stats.append(_check(a, _build(a, G, 4, rnd=rnd, align=align, warp=tab, shift=sh), G, rnd, align, tab, sh))
    print("G=%d  (steps, pad fraction, heaviest bin): %s -> %s" % (G, stats[0], stats[1]))
    assert stats[0][1] > 0.01
    assert stats[1][1] <= stats[0][1]


def _edge_cases():
    rng = np.random.RandomState(7)
    one_col = sp.csr_matrix((rng.rand(500).astype(np.float32) + 0.1, (np.arange(500), np.full(500, 3))), shape=(500, 40))
    hub = sp.vstack([sp.csr_matrix(np.ones((1, 3000), np.float32)),
                     sp.random(5, 3000, density=0.01, random_state=rng, format='csr', dtype=np.float32)]).tocsr()
    few = sp.random(20, 300, density=0.2, random_state=rng, format='csr', dtype=np.float32)
    return [("empty", sp.csr_matrix((0, 0), dtype=np.float32), 0),
            ("no nonzeros", sp.csr_matrix((40, 30), dtype=np.float32), 0),
            ("one row", sp.csr_matrix(rng.rand(1, 200).astype(np.float32)), 0),
            ("one column", one_col, 0),
            ("hub row with more pieces than bins", hub, 24),           # 125 pieces of 24, 6 rows: 5 tiles of 2 bins
            ("fewer rows than one tile", few, 0)]


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("name,a,T", _edge_cases(), ids=[c[0] for c in _edge_cases()])
def test_edge_cases_build_and_encode(name, a, T, G):
    a = a.tocsr()
    a.sort_indices()
    for deal in (0, 1):
        _deal(deal)
        for rnd, align in ((0, 0), (4, 16)):
            _check(a, _build(a, G, 2, T=T, rnd=rnd, align=align), G, rnd, align)


def _golden_cases(small):
    """name -> (matrix, G, rnd, align, warp table, shift): the plans whose digests the parent build recorded"""
    from stochastic_gcn_amd import ops
    sk = _skewed_csr(20000, 30000, 400000, 5)
    tab, sh = ops.ColumnSweepCSR.make_warp(np.ascontiguousarray(sk.indices, np.int32), sk.shape[1], True)
    return {"small_g2": (small, 2, 256, 224, None, 0), "small_g4": (small, 4, 128, 224, None, 0),
            "skewed_g2_warp": (sk, 2, 64, 256, tab, sh), "skewed_g4_warp": (sk, 4, 64, 256, tab, sh)}


def _golden_digests(small):
    return {k: _digest(_build(a, G, 4, rnd=rnd, align=align, warp=tab, shift=sh))
            for k, (a, G, rnd, align, tab, sh) in _golden_cases(small).items()}


def test_knob_off_is_the_plan_of_the_build_before_the_knob(small_reddit):
    """cs_deal = 0 is the weight-only LPT dealing bit for bit -- against digests taken from the library before it had the
    knob -- and setting the knob to 1 and back leaves no state behind."""
    want = json.load(open(GOLDEN))
    _deal(0)
    first = _golden_digests(small_reddit)
    assert first == want
    _deal(1)
    on = _golden_digests(small_reddit)
    assert all(on[k] != want[k] for k in want)
    _deal(0)
    assert _golden_digests(small_reddit) == want


def test_knob_is_a_switch():
    assert lib.sgcn_tune_get(b"cs_deal") in (0, 1)
    assert lib.sgcn_tune(b"cs_deal", 2) != 0 and lib.sgcn_tune(b"cs_deal", -1) != 0
