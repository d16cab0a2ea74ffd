"""Every sparse product, checked on ALL rows against an independent fp64 reference (tests/sparse_cases.py).

Two checks per path.  On dyadic inputs (values +-2^k, integer operands, power-of-two scales) fp32 arithmetic is exact in
any summation order, so a correct kernel equals the fp64 product bit for bit: a dropped, duplicated, misplaced or
mis-scaled term fails, however long its row.  On real-valued inputs (D^-1 A values, N(0, 1) operands) every element
stays within the rigorous bound of ``sparse_cases.fp64_bound``: a loss of precision fails.  Besides: two calls give the
same bits, the pitch padding of ``out`` and the rows after M (NaN sentinels inside one larger buffer) are never
written, and the operands are not changed."""
import functools
import zlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import sparse_cases as sc
from gpu_checks import Operand, check, f32 as _f32

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 4, 30, 64, 66, 128, 130, 256, 260, 320, 330, 602, 1024)

# patterns x widths, pairwise: every pattern with one or more widths, every width with several patterns
PAIRS = [("empty", 3), ("one_row", 602), ("identity", 1), ("identity", 130), ("permutation", 66), ("star_row", 4),
         ("star_row", 30), ("star_col", 256), ("star_col", 3), ("hot_block", 320), ("row_lengths", 1),
         ("row_lengths", 130), ("row_lengths", 602), ("row_lengths", 1024), ("m15_k17", 64), ("m16_k16", 330),
         ("m17_k15", 128), ("m63_k65", 260), ("m64_k64", 1024), ("m65_k63", 4), ("m4095_k4097", 66),
         ("m4096_k4096", 3), ("m4097_k4095", 330), ("k5", 602), ("row_vector", 260), ("col_vector", 64),
         ("rmat", 128), ("sbm", 256), ("sched_adj", 30), ("sched_fadj", 320), ("range_boundary", 130),
         ("range_empty", 30)]
assert {d for _, d in PAIRS} == set(WIDTHS) and {p for p, _ in PAIRS} == set(sc.CATALOGUE)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _pattern(name):
    return sc.pattern(name)


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def _values(a, rng, exact):
    return sc.dyadic(a, rng) if exact else sc.normalised(a)


def _dense(rng, shape, exact):
    return sc.ints(rng, shape) if exact else rng.standard_normal(shape).astype(np.float32)


def _scales(rng, n, exact):
    return sc.pow2(rng, n) if exact else (rng.rand(n) + 0.5).astype(np.float32)


def _pitch(d, pad, align4):
    return ((d + 3) // 4 * 4 if align4 else d) + pad


def _reference(a, B, exact, **kw):
    if exact:
        return sc.spmm_exact(a, B, **kw), None
    return sc.spmm_f64(a, B, **kw), sc.fp64_bound(a, B, **kw)


# ---- ops.spmm: the row-gather product -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,d", PAIRS)
@pytest.mark.parametrize("plan", ["none", "T", "default"])
def test_spmm_row_gather(dev, name, d, plan):
    from stochastic_gcn_amd import ops
    for exact in (True, False):
        rng = np.random.RandomState(_seed(name, d, plan, exact))
        a = _values(_pattern(name), rng, exact)
        A = ops.DeviceCSR.from_scipy(a, dev, plan_T=sc.T_SPLIT if plan == "T" else 0, with_plan=plan != "none")
        B = Operand(_dense(rng, (a.shape[1], d), exact), dev, d + 3)
        ref, bound = _reference(a, B.view.cpu().numpy(), exact)
        check(lambda out: ops.spmm(A, B.view, out=out), dev, a.shape[0], d, d + 1, ref, bound, operands=[B],
              what="spmm %s d=%d plan=%s exact=%s" % (name, d, plan, exact))


FUSIONS = [dict(gidx=1), dict(rscale=1), dict(cscale=1), dict(beta=0.5), dict(add=1), dict(beta=1.0, add=1),
           dict(gidx=1, rscale=1, cscale=1, beta=0.5, add=1)]


def _fused_operands(rng, a, d, f, exact, dev, pitch):
    M, K = a.shape
    kw, ops_ = {}, []
    nB = K + 37 if f.get("gidx") else K
    B = Operand(_dense(rng, (nB, d), exact), dev, pitch)
    if f.get("gidx"):
        kw["gidx"] = rng.choice(nB, K, replace=False).astype(np.int32)
    if f.get("rscale"):
        kw["rscale"] = _scales(rng, M, exact)
    if f.get("cscale"):
        kw["cscale"] = _scales(rng, K, exact)
    C = None
    if f.get("beta"):
        kw["beta"] = f["beta"]
        C = _dense(rng, (M, d), exact)
        kw["C_in"] = C
    add = None
    if f.get("add"):
        add = Operand(_dense(rng, (M, d), exact), dev, pitch)
        kw["add"], kw["add_rows"] = add.view.cpu().numpy(), max(M - 3, 1)
        ops_.append(add)
    return B, kw, C, add, ops_


@pytest.mark.parametrize("name,d", [("row_lengths", 66), ("sched_adj", 128), ("star_col", 3), ("m4097_k4095", 602)])
@pytest.mark.parametrize("fi", range(len(FUSIONS)))
def test_spmm_row_gather_fusions(dev, name, d, fi):
    from stochastic_gcn_amd import ops
    f = FUSIONS[fi]
    for exact in (True, False):
        rng = np.random.RandomState(_seed(name, d, fi, exact))
        a = _values(_pattern(name), rng, exact)
        A = ops.DeviceCSR.from_scipy(a, dev, plan_T=sc.T_SPLIT)
        B, kw, C, add, extra = _fused_operands(rng, a, d, f, exact, dev, d + 2)
        ref, bound = _reference(a, B.view.cpu().numpy(), exact, **kw)
        t = {k: _f32(kw.get(k), dev) for k in ("gidx", "rscale", "cscale")}

        def call(out):
            return ops.spmm(A, B.view, out=out, beta=kw.get("beta", 0.0), d=d,
                            add=None if add is None else add.view, add_rows=kw.get("add_rows", 0), **t)
        check(call, dev, a.shape[0], d, d + 2, ref, bound, C_in=C, operands=[B] + extra,
              what="spmm fusions %s %s exact=%s" % (name, f, exact))


@pytest.mark.parametrize("name,d", [("sched_adj", 602), ("rmat", 64), ("star_col", 130), ("row_lengths", 3),
                                    ("hot_block", 1024)])
def test_spmm_transpose(dev, name, d):
    """A.transpose (the backward product A^T dC) against the fp64 transpose product"""
    from stochastic_gcn_amd import ops
    for exact in (True, False):
        rng = np.random.RandomState(_seed(name, d, exact))
        a = _values(_pattern(name), rng, exact)
        A = ops.DeviceCSR.from_scipy(a, dev, plan_T=sc.T_SPLIT, with_transpose=True)
        at = a.T.tocsr()
        g = Operand(_dense(rng, (a.shape[0], d), exact), dev, d)
        ref, bound = _reference(at, g.view.cpu().numpy(), exact)
        check(lambda out: ops.spmm(A.transpose, g.view, out=out), dev, at.shape[0], d, d + 4, ref, bound, operands=[g],
              what="spmm A^T %s d=%d exact=%s" % (name, d, exact))


# ---- ops.spmm_cs: the column sweep ------------------------------------------------------------------------------------------
CS_FUSIONS = [{}, dict(rscale=1), dict(cscale=1, beta=0.5), dict(gidx=1), dict(gidx=1, rscale=1, cscale=1, beta=1.0)]


def _cs_plan(ops, a, dev, G, warp, T):
    return ops.ColumnSweepCSR(a, dev, G=G, warp=warp, T=T)


@pytest.mark.parametrize("i", range(len(PAIRS)))
def test_spmm_column_sweep(dev, i):
    """every pattern x width pair with G = 1 / 2 / 4 and warp True / False / 'auto' in turn, a fusion set in turn, at a pace
    and unpaced (pacing is timing only: the same bits)"""
    from stochastic_gcn_amd import ops
    name, d = PAIRS[i]
    G, warp = (1, 2, 4)[i % 3], (True, False, 'auto')[(i // 3) % 3]
    f = CS_FUSIONS[i % len(CS_FUSIONS)]
    T = sc.T_SPLIT if name in ("row_lengths", "one_row", "star_row") else 0
    pitch = _pitch(d, 4 * (i % 2), True)
    for exact in (True, False):
        rng = np.random.RandomState(_seed(name, d, "cs", exact))
        a = _values(_pattern(name), rng, exact)
        A = _cs_plan(ops, a, dev, G, warp, T)
        kw_f = {k: v for k, v in f.items() if k != "add"}
        B, kw, C, _, extra = _fused_operands(rng, a, d, kw_f, exact, dev, pitch)
        ref, bound = _reference(a, B.view.cpu().numpy(), exact, **kw)
        t = {k: _f32(kw.get(k), dev) for k in ("gidx", "rscale", "cscale")}
        outs = []
        for pace in (-1, (150, 300)[i % 2]):
            A.pace[d] = pace
            outs.append(check(lambda out: ops.spmm_cs(A, B.view, out=out, beta=kw.get("beta", 0.0), **t), dev, a.shape[0],
                              d, pitch, ref, bound, C_in=C, operands=[B] + extra,
                              what="spmm_cs %s d=%d G=%d warp=%s %s pace=%d exact=%s" % (name, d, G, warp, f, pace, exact)))
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "the pace changed the bits"


@pytest.mark.parametrize("name,d,G", [("rmat", 256, 1), ("sbm", 602, 2), ("row_lengths", 130, 4), ("star_col", 64, 2)])
def test_spmm_column_sweep_autotuned(dev, name, d, G):
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(_seed(name, d, G))
    a = sc.dyadic(_pattern(name), rng)
    A = ops.ColumnSweepCSR(a, dev, G=G, T=sc.T_SPLIT if name == "row_lengths" else 0)
    B = Operand(sc.ints(rng, (a.shape[1], d)), dev, _pitch(d, 0, True))
    A.autotune(B.view)
    assert d in A.pace
    ref = sc.spmm_exact(a, B.view.cpu().numpy())
    check(lambda out: ops.spmm_cs(A, B.view, out=out), dev, a.shape[0], d, _pitch(d, 4, True), ref, operands=[B],
          what="spmm_cs autotuned %s G=%d pace=%s" % (name, G, A.pace[d]))


@pytest.mark.parametrize("name,d,NR,T", [("range_boundary", 130, 2, 0), ("range_boundary", 3, 2, sc.T_SPLIT),
                                         ("range_empty", 602, 3, 0), ("range_empty", 64, 4, 0), ("row_lengths", 1024, 2, sc.T_SPLIT),
                                         ("hot_block", 260, 4, 0), ("m4097_k4095", 330, 3, 0), ("star_row", 30, 2, 0)])
def test_spmm_column_range_plan(dev, name, d, NR, T):
    from stochastic_gcn_amd import ops
    # (the star row's 100,000 terms leave no head room for the scales' powers of two: its exact case gathers rows only)
    for exact, fi in ((True, 0), (True, 3 if name == "star_row" else 4), (False, 4)):
        rng = np.random.RandomState(_seed(name, d, NR, exact, fi))
        a = _values(_pattern(name), rng, exact)
        A = ops.ColumnSweepCSR(a, dev, T=T, col_ranges=NR)
        assert A.ranged == NR
        cuts = np.asarray(A.range_cuts)
        if name == "range_boundary":           # nonzeros on both sides of the cut
            assert np.isin([cuts[1] - 1, cuts[1]], a.indices).all()
        if name == "range_empty":              # a range without a nonzero
            assert any(not np.any((a.indices >= lo) & (a.indices < hi)) for lo, hi in zip(cuts[:-1], cuts[1:]))
        pitch = _pitch(d, 4, True)
        B, kw, C, _, extra = _fused_operands(rng, a, d, CS_FUSIONS[fi], exact, dev, pitch)
        ref, bound = _reference(a, B.view.cpu().numpy(), exact, **kw)
        t = {k: _f32(kw.get(k), dev) for k in ("gidx", "rscale", "cscale")}
        for pace in (-1, 250):
            A.pace[d] = pace
            check(lambda out: ops.spmm_cs(A, B.view, out=out, beta=kw.get("beta", 0.0), **t), dev, a.shape[0], d, pitch,
                  ref, bound, C_in=C, operands=[B] + extra, what="ranged %s NR=%d pace=%d exact=%s" % (name, NR, pace, exact))


@pytest.mark.parametrize("name,d", [("sbm", 128), ("row_lengths", 66), ("rmat", 30), ("sched_adj", 602)])
def test_spmm_grouped_column_sweep(dev, name, d):
    """col_labels / row_labels plans (columns read through the position map, tiles inside row communities, unpaced)"""
    from stochastic_gcn_amd import ops
    for exact in (True, False):
        rng = np.random.RandomState(_seed(name, d, "grouped", exact))
        a = _values(_pattern(name), rng, exact)
        M, K = a.shape
        if name == "sbm":
            cl = rl = sc.sbm_labels()
        else:
            cl, rl = rng.randint(0, 5, K).astype(np.int32), rng.randint(0, 3, M).astype(np.int32)
        A = ops.ColumnSweepCSR(a, dev, T=48, col_labels=cl, row_labels=rl)
        assert A.grouped
        pitch = _pitch(d, 0, True)
        B, kw, C, _, extra = _fused_operands(rng, a, d, dict(gidx=1, rscale=1, beta=0.5), exact, dev, pitch)
        ref, bound = _reference(a, B.view.cpu().numpy(), exact, **kw)
        t = {k: _f32(kw.get(k), dev) for k in ("gidx", "rscale")}
        check(lambda out: ops.spmm_cs(A, B.view, out=out, beta=0.5, **t), dev, M, d, pitch, ref, bound, C_in=C,
              operands=[B] + extra, what="grouped %s exact=%s" % (name, exact))
        with pytest.raises(ValueError):        # a grouped plan refuses cscale (scale B instead)
            ops.spmm_cs(A, B.view, cscale=torch.ones(K, device=dev))


# ---- ops.spmm_lds: the LDS-staged sweep ---------------------------------------------------------------------------------------
def _lds_values(a, kind, rng):
    a = sc.dyadic(a, rng)
    if kind == "ones":
        a.data[:] = 1.0
    elif kind == "row":
        a = sp.diags(sc.pow2(rng, a.shape[0], -2, 2)).dot((a != 0).astype(np.float32)).tocsr().astype(np.float32)
    elif kind == "col":
        a = (a != 0).astype(np.float32).dot(sp.diags(sc.pow2(rng, a.shape[1], -2, 2))).tocsr().astype(np.float32)
    a.sort_indices()
    return a


LDS_CASES = [("sbm", 256, "ones"), ("sbm", 130, "col"), ("sbm", 602, "gen"), ("hot_block", 128, "row"),
             ("row_lengths", 64, "gen"), ("row_lengths", 4, "ones"), ("identity", 30, "col"), ("star_col", 1024, "row"),
             ("m4097_k4095", 3, "gen"), ("k5", 66, "ones"), ("rmat", 260, "col"), ("one_row", 1, "gen"),
             ("empty", 320, "ones"), ("sched_adj", 330, "row")]


@pytest.mark.parametrize("i", range(len(LDS_CASES)))
def test_spmm_lds(dev, i):
    """unit (ones / row-constant / column-constant values) and general plans, labels, min_reuse 1..3, both rings, split
    rows, the G = 4 residual, rscale and beta; and local_only (the planned nonzeros alone) against A minus the residual"""
    from stochastic_gcn_amd import ops
    name, d, kind = LDS_CASES[i]
    rng = np.random.RandomState(_seed(name, d, kind))
    a = _lds_values(_pattern(name), kind, rng)
    M, K = a.shape
    labels = None
    if name == "sbm":
        labels = sc.sbm_labels()
    elif i % 2:
        labels = (rng.randint(0, 4, M).astype(np.int32), rng.randint(0, 4, K).astype(np.int32))
    host = ops.LdsPlanHost(a, labels=labels, min_reuse=1 + i % 3, T=sc.T_SPLIT if i % 4 == 0 else 0,
                           general=(kind == "gen" and i % 3 != 0), ring_slots=80 if i % 2 else 0)
    A = ops.LdsSweepCSR(a, dev, host=host)
    pitch = _pitch(d, 4 * (i % 2), True)
    B = Operand(sc.ints(rng, (K, d)), dev, pitch)
    rs = sc.pow2(rng, M)
    C = sc.ints(rng, (M, d))
    Bh = B.view.cpu().numpy()
    ref = sc.spmm_exact(a, Bh, rscale=rs, beta=0.5, C_in=C)
    check(lambda out: ops.spmm_lds(A, B.view, out=out, rscale=_f32(rs, dev), beta=0.5), dev, M, d, pitch, ref, C_in=C,
          operands=[B], what="lds %s %s" % (name, kind))
    # the planned part alone: A - residual (the residual holds folded values when the plan folded a column value)
    Bf = Bh * host.col_fold[:, None] if host.col_fold is not None else Bh
    res = host.residual
    local = sc.spmm_exact(a, Bh) - sc.spmm_exact(res.astype(np.float32), Bf)
    check(lambda out: ops.spmm_lds(A, B.view, out=out, local_only=True), dev, M, d, pitch, local, operands=[B],
          what="lds local_only %s %s" % (name, kind))
    # real values: D^-1 A (one value per row: a unit plan), N(0, 1) operand, against the bound
    an = sc.normalised(a)
    An = ops.LdsSweepCSR(an, dev, labels=labels, min_reuse=1 + i % 3)
    Bn = Operand(rng.standard_normal((K, d)).astype(np.float32), dev, pitch)
    ref, bound = _reference(an, Bn.view.cpu().numpy(), False)
    check(lambda out: ops.spmm_lds(An, Bn.view, out=out), dev, M, d, pitch, ref, bound, operands=[Bn],
          what="lds real %s" % name)


def test_lds_for_graph_on_communities(dev):
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(7)
    a = sc.dyadic(_pattern("sbm"), rng)
    A = ops.LdsSweepCSR.for_graph(a, dev)
    assert A is not None and A.host_stats["local_nnz"] > 0.5 * a.nnz
    d = 128
    B = Operand(sc.ints(rng, (a.shape[1], d)), dev, d)
    check(lambda out: ops.spmm_lds(A, B.view, out=out), dev, a.shape[0], d, d + 4, sc.spmm_exact(a, B.view.cpu().numpy()),
          operands=[B], what="lds for_graph")


# ---- the control-variate aggregator -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cvd", [True, False])
@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("split,d", [("none", 30), ("T", 128), ("default", 602), ("T", 1), ("none", 260)])
def test_vr_aggregate(dev, cvd, concat, split, d):
    from stochastic_gcn_amd import ops
    adj0, fadj0, fd = sc.scheduler_batch(seed=4, degree=3)
    n, n0, n1 = 3000, fd['f0'].shape[0], adj0.shape[0]
    width = 2 * d if concat else d
    for exact in (True, False):
        rng = np.random.RandomState(_seed(cvd, concat, split, d, exact))
        adj, fadj = _values(adj0, rng, exact), _values(fadj0, rng, exact)
        h, mu, H = (_dense(rng, s, exact) for s in ((n0, d), (n0, d), (n, d)))
        s = _scales(rng, n1, exact)
        A = ops.DeviceCSR.from_scipy(adj, dev, with_plan=False)
        P = ops.DeviceCSR.from_scipy(fadj, dev, plan_T=8 if split == "T" else 0, with_plan=split != "none")
        if split == "T":
            assert P.plan.nfix > 0
        oh, om, mh, mm, nt = sc.vr_aggregate_f64(adj, fadj, h, mu, H, fd['f0'], fd['ff0'], s, cvd, concat)
        if exact:
            sc.assert_exact(mh, sc.low_exp(adj.data, fadj.data) + min(sc.low_exp(s), 0), "aggregate")
            sc.assert_exact(np.abs(h) + np.abs(mu), 0)
        hb, mb = Operand(h, dev, d), Operand(mu, dev, d)
        Hb = Operand(H, dev, d + 2)
        t = lambda x: _f32(x, dev)      # noqa: E731
        outs = {}
        for form in ("fused", "two_phase"):
            for rep in range(2):
                if form == "fused":
                    r = ops.vr_aggregate(A, P, hb.view, mb.view, Hb.view, t(fd['f0']), t(fd['ff0']), t(s), cvd, concat)
                else:
                    r = ops.vr_aggregate_two_phase(A, P, hb.view, mb.view, Hb.view, t(fd['f0']), t(fd['ff0']), t(s), cvd, concat)
                outs.setdefault(form, []).append(r)
            for x, y in zip(*outs[form]):
                assert (x is None) == (y is None) and (x is None or torch.equal(x.view(torch.int32), y.view(torch.int32)))
            assert hb.unchanged() and mb.unchanged() and Hb.unchanged()
            got = [None if x is None else x.double().cpu().numpy() for x in outs[form][0]]
            for g, ref, mag in ((got[0], oh, mh), (got[1], om, mm)):
                if ref is None:
                    continue
                assert g.shape == (n1, width)
                if exact:
                    bad = g != ref
                    assert not bad.any(), "%s: %d rows differ from the exact aggregate" % (form, int(bad.any(1).sum()))
                else:
                    bad = ~(np.abs(g - ref) <= sc.vr_bound(mag, nt, concat))
                    assert not bad.any(), "%s: %d elements outside the fp64 bound" % (form, int(bad.sum()))
        # the fused pass and the two-phase form give the same bits, with or without a plan for P -- also when h / mu
        # (pitch d) allow narrower vectors than Hbar (pitch d + 2) does: d = 30 without a plan is the regression case of
        # the fused pass cutting a P row into other chunks than _pre did (sgcn_agg.hip p_chunks)
        for x, y in zip(outs["fused"][0], outs["two_phase"][0]):
            assert x is None or torch.equal(x.view(torch.int32), y.view(torch.int32)), "fused and two-phase differ"


# ---- full size: the configuration bench.py times -------------------------------------------------------------------------
def test_full_size_column_sweep_exact_on_every_row(dev):
    """S-Reddit, d = 602 (pitch 608), the lane-group count choose_g picks and the autotuned pace: the forward product and
    the A^T product on all 232,965 rows, bit for bit against the exact product (SciPy's fp32 product is exact on these
    inputs: the precondition is asserted first)"""
    from stochastic_gcn_amd import ops, synthetic
    n, _, full_adj, *_ = synthetic.reddit_like(with_features=False)
    d, ld = 602, 608
    rng = np.random.RandomState(11)
    a = sc.dyadic(full_adj, rng, -1, 1)
    at = a.T.tocsr()
    at.sort_indices()
    G = ops.ColumnSweepCSR.choose_g(d, a.nnz / n, n)
    for m, what in ((a, "A"), (at, "A^T")):
        X = sc.ints(rng, (n, d))
        rowmax = np.asarray(abs(m).sum(axis=1)).ravel() * 8.0        # >= every (|A| |X|)_ik
        sc.assert_exact(rowmax, sc.low_exp(m.data), "full-size " + what)
        Xd = Operand(X, dev, ld)
        P = ops.ColumnSweepCSR(m, dev, G=G)
        P.autotune(Xd.view)
        out = torch.full((n + 2, ld), float("nan"), device=dev)
        ops.spmm_cs(P, Xd.view, out=out[:n, :d])
        assert torch.equal(ops.spmm_cs(P, Xd.view), out[:n, :d]), what + ": two calls differ"
        assert torch.isnan(out[:, d:]).all() and torch.isnan(out[n:]).all() and Xd.unchanged()
        ref = m.dot(X)                                                  # fp32, exact by the precondition
        got = out[:n, :d].cpu().numpy()
        bad = got != ref
        assert not bad.any(), "%s (G=%d, pace %s): %d rows differ from the exact product, first %s" % (
            what, G, P.pace.get(d), int(bad.any(1).sum()), np.nonzero(bad.any(1))[0][:8])


# ---- randomised cases (formerly profiles/cs_fuzz.py and profiles/lds_fuzz.py, run by hand) --------------------------------
@pytest.mark.parametrize("seed", range(24))
def test_column_sweep_fuzz(dev, seed):
    from stochastic_gcn_amd import ops
    c = sc.cs_fuzz_case(seed)
    a, d, rng = c["a"], c["d"], c["rng"]
    M, K = a.shape
    if c["ranges"]:
        A = ops.ColumnSweepCSR(a, dev, T=c["T"], col_ranges=c["ranges"])
        assert A.ranged == c["ranges"]
    else:
        A = ops.ColumnSweepCSR(a, dev, T=c["T"], G=c["G"], warp=c["warp"], **({} if c["G"] == 1 else {"align": c["align"]}))
    A.pace[d] = c["pace"]
    pitch = _pitch(d, c["pad"], True)
    f = dict(gidx=c["gather"], rscale=c["rscale"], cscale=c["cscale"], beta=c["beta"])
    B, kw, C, _, extra = _fused_operands(rng, a, d, f, True, dev, pitch)
    ref = sc.spmm_exact(a, B.view.cpu().numpy(), **kw)
    t = {k: _f32(kw.get(k), dev) for k in ("gidx", "rscale", "cscale")}
    check(lambda out: ops.spmm_cs(A, B.view, out=out, beta=kw.get("beta", 0.0), **t), dev, M, d, pitch, ref, C_in=C,
          operands=[B] + extra, what="cs fuzz %d" % seed)


@pytest.mark.parametrize("seed", range(24))
def test_lds_sweep_fuzz(dev, seed):
    from stochastic_gcn_amd import ops
    c = sc.lds_fuzz_case(seed)
    a, d, rng = c["a"], c["d"], c["rng"]
    M, K = a.shape
    A = ops.LdsSweepCSR(a, dev, labels=c["labels"], min_reuse=c["min_reuse"], T=c["T"], ring_slots=c["ring"], general=c["general"])
    pitch = _pitch(d, c["pad"], True)
    B = Operand(sc.ints(rng, (K, d)), dev, pitch)
    rs = sc.pow2(rng, M) if c["rscale"] else None
    C = sc.ints(rng, (M, d)) if c["beta"] else None
    ref = sc.spmm_exact(a, B.view.cpu().numpy(), rscale=rs, beta=c["beta"], C_in=C)
    check(lambda out: ops.spmm_lds(A, B.view, out=out, rscale=_f32(rs, dev), beta=c["beta"]), dev, M, d, pitch, ref,
          C_in=C, operands=[B], what="lds fuzz %d (%s)" % (seed, c["kind"]))
