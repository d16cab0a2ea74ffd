"""Attention with learned additive scores on the device (ops.gat_scores / ops.spgat / ops.spgat_bwd / ops.gat_scores_bwd),
every row and every cell against tests/spgat_ref.py, on the adversarial patterns of tests/spattn_cases.py (empty rows, hub
rows and hub columns, a single entry, M != K), widths 1 .. 1024 with the head counts that divide them, and the plans none /
default / T = 64 / T = 1.

Scores     exact on dyadic tables in every cell; within (dh + 1) u sum |x a| on real-valued ones.
Uniform    U = V = 0 and a dyadic B: every weight is exactly 1, so C equals fl(sum / n_i) BIT FOR BIT whatever the plan cuts.
Winner     U = 0, V[j, h] = 256 (pi_h(j) + 1) for a seeded permutation per head: exact positive z with gaps >= 256, every losing
           weight underflows to exactly 0 -- C[i] is the BITS of one row of B per head, dB the exact sum of the won gradients,
           dU and dV exactly 0 (t and delta go through the same reduction tree).
Kink       rows of power-of-two degree that hold z < 0, z > 0 and z == 0 exactly (dyadic U and V), and rows whose every z is 0
           (u = -v): everything within the bound, which the derivative 1 at z == 0 would miss (asserted on the reference).
General    normal tables: C, lse, delta, dU, dV and dB within the derived bounds, with and without addend and mask.
Way back   sgcn_gat_scores_bwd_f32 at rows 1 .. 4097: da exact on dyadic inputs and within gamma_rows sum |terms| otherwise;
           dX within two roundings; a null dX writes nothing.
Every backward runs twice: equal bits.  Under keep < 1 the kept set read off the device is the one ops.attn_kept predicts."""
import functools

import numpy as np
import pytest
import torch

import sparse_cases as sc
import spattn_cases as cs
import spattn_drop_cases as dc
import spgat_ref as ref

pytestmark = pytest.mark.gpu
U = ref.U_
SLOPE = 0.2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


def _np(t):
    return t.cpu().numpy()


def _csr(a, dev, plan):
    from stochastic_gcn_amd import ops
    T = {"none": 0, "default": 0, "T": sc.T_SPLIT, "1": 1, "8": 8}[plan]
    return ops.DeviceCSR.from_scipy(a, dev, plan_T=T, with_plan=plan != "none")


def _pair(name, dev, plan):
    a, at = cs.pattern(name)
    return a, _csr(a, dev, plan), _csr(at, dev, plan)


def _pitch(d, odd=False):
    """a multiple of 4 (float4 lanes where the head width allows), or an odd one (scalar lanes)"""
    c4 = (d + 3) // 4 * 4
    return (d + 1 if d % 2 == 0 else d + 2) if odd else c4 + 4


def _padded(x, dev, pitch):
    x = np.asarray(x)
    buf = torch.full((x.shape[0], pitch), float('nan'), dtype=torch.float32, device=dev)
    view = buf[:, :x.shape[1]]
    view.copy_(torch.tensor(x))
    return view


def _blank(rows, d, dev, pitch):
    buf = torch.full((rows, pitch), float('nan'), dtype=torch.float32, device=dev)
    return buf, buf[:, :d]


def _dev(x, dev):
    return torch.tensor(np.ascontiguousarray(x)).to(dev)


def _within(got, want, bound, what):
    got = np.asarray(got, np.float64)
    assert np.all(np.isfinite(got)), what
    err = np.abs(got - want)
    ratio = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    print("%s: worst |error| / bound %.4f" % (what, ratio))
    assert np.all(err <= bound), "%s: worst error / bound %.3f" % (what, ratio)
    return ratio


# (pattern, d, H, plan, odd pitch): d in {1, 4, 5, 64, 132, 602, 1024} x the H that divide d (602 in 2 heads is 301 columns a
# head: scalar lanes, over the width limit -- refused, tested below) x the four plans, thinned
CASES = [
    ("row_lengths", 1, 1, "T", False), ("row_lengths", 4, 1, "none", False), ("row_lengths", 4, 2, "default", True),
    ("row_lengths", 4, 4, "T", False), ("row_lengths", 5, 1, "1", False), ("row_lengths", 5, 1, "T", True),
    ("row_lengths", 64, 1, "T", True), ("row_lengths", 64, 2, "1", False), ("row_lengths", 64, 4, "default", False),
    ("row_lengths", 64, 8, "T", False), ("row_lengths", 132, 1, "default", False), ("row_lengths", 132, 2, "T", False),
    ("row_lengths", 132, 4, "1", False), ("row_lengths", 602, 1, "T", False), ("row_lengths", 1024, 1, "default", False),
    ("row_lengths", 1024, 2, "none", False), ("row_lengths", 1024, 4, "T", False), ("row_lengths", 1024, 8, "1", False),
    ("empty", 4, 4, "default", False), ("one_row", 132, 4, "T", False), ("identity", 1, 1, "none", False),
    ("star_row", 5, 1, "T", False), ("star_col", 64, 8, "T", False), ("hot_block", 64, 2, "1", False),
    ("m63_k65", 64, 4, "T", False), ("m65_k63", 132, 2, "1", False), ("m4097_k4095", 4, 2, "default", False),
    ("row_vector", 602, 1, "default", False), ("col_vector", 4, 1, "T", True),
]
assert {c[1] for c in CASES} == {1, 4, 5, 64, 132, 602, 1024} and {c[3] for c in CASES} == {"none", "default", "T", "1"}


# ---- the scores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,H", [(1, 1), (4, 1), (4, 4), (5, 1), (64, 2), (64, 8), (132, 1), (132, 4), (602, 1), (602, 2), (1024, 1),
                                 (1024, 8)])
def test_scores_exact_on_dyadic_tables_and_within_the_bound(dev, d, H):
    from stochastic_gcn_amd import ops
    rows = 131
    rng = np.random.RandomState(cs.seed("scores", d, H))
    xi, ai = sc.ints(rng, (rows, d)) * np.float32(0.5), sc.ints(rng, (2, d)) * np.float32(0.25)
    want, _ = ref.scores_f64(xi, ai, H)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    for odd in (False, True):
        S = _np(ops.gat_scores(_padded(xi, dev, _pitch(d, odd)), _dev(ai, dev), heads=H))
        assert S.shape == (rows, 2 * H) and np.array_equal(S.astype(np.float64), want)               # every cell
    x, av = rng.standard_normal((rows, d)).astype(np.float32), rng.standard_normal((2, d)).astype(np.float32)
    want, bound = ref.scores_f64(x, av, H)
    S = _np(ops.gat_scores(_padded(x, dev, _pitch(d)), _dev(av, dev), heads=H))
    _within(S, want, bound, "gat_scores d=%d H=%d" % (d, H))
    if d // H <= 64:                                  # (one column per lane: the restatement's products round once, as an fma from +0 does)
        assert ref.same_bits(S, ref.scores_f32_kernel_order(x, av, H))


# ---- the uniform regime ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,d,H,plan,odd", CASES)
def test_uniform_regime_bits(dev, name, d, H, plan, odd):
    from stochastic_gcn_amd import ops
    a, A, _ = _pair(name, dev, plan)
    M, K = a.shape
    if plan == "T" and name == "row_lengths":
        assert A.plan.nfix >= 5
    _, B, C_ref, logn = cs.uniform(name, d)
    if odd and d > 256:
        return
    pitch = _pitch(d, odd)
    Cbuf, Cv = _blank(M, d, dev, pitch)
    z = torch.zeros((max(M, K), 2 * H), dtype=torch.float32, device=dev)
    out, lse = ops.spgat(A, _padded(B, dev, pitch), z[:M, :H], z[:K, H:], slope=SLOPE, out=Cv, heads=H)
    assert out.data_ptr() == Cv.data_ptr() and bool(torch.isnan(Cbuf[:, d:]).all().item())
    assert ref.same_bits(_np(Cv), C_ref)
    lse = _np(lse).astype(np.float64)
    empty = np.diff(a.indptr) == 0
    assert lse.shape == (M, H) and np.all(lse[empty] == -np.inf)
    assert np.all(np.abs(lse[~empty] - logn[~empty, None]) <= 2 * U * np.maximum(1.0, logn[~empty, None]))
    out2, none = ops.spgat(A, _padded(B, dev, pitch), z[:M, :H], z[:K, H:], slope=SLOPE, heads=H, want_lse=False)
    assert none is None and ref.same_bits(_np(out2), C_ref)


# ---- the winner regime -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def winner(name, d, H):
    a, _ = cs.pattern(name)
    M, K = a.shape
    dh = d // H
    rng = np.random.RandomState(cs.seed(name, d, H, "gat winner"))
    B = (sc.ints(rng, (K, d)) * np.float32(0.25)).astype(np.float32)
    G = sc.ints(rng, (M, d), -2, 2)
    add = sc.ints(rng, (K, d), -4, 4)
    V = np.stack([256.0 * (rng.permutation(K) + 1.0) for _ in range(H)], axis=1).astype(np.float32)
    Ut = np.zeros((M, H), np.float32)
    indptr, cols = a.indptr.astype(np.int64), a.indices.astype(np.int64)
    C, lse, dB = np.zeros((M, d), np.float32), np.full((M, H), -np.inf, np.float32), np.zeros((K, d), np.float64)
    for h in range(H):
        pos = cs._seg_argmax(V[cols, h].astype(np.float64), indptr)
        has = pos >= 0
        jstar = np.where(has, cols[np.maximum(pos, 0)] if cols.size else 0, -1)
        sl = slice(h * dh, (h + 1) * dh)
        C[has, sl] = B[jstar[has], sl]
        lse[has, h] = V[jstar[has], h]
        np.add.at(dB[:, sl], jstar[has], G[has, sl].astype(np.float64))
    assert float(np.max(np.abs(dB))) < 2.0 ** 20 if dB.size else True
    return Ut, V, B, G, add, C, lse, dB.astype(np.float32)


@pytest.mark.parametrize("name,d,H,plan,odd", CASES)
def test_winner_regime_bits(dev, name, d, H, plan, odd):
    from stochastic_gcn_amd import ops
    a, A, At = _pair(name, dev, plan)
    M, K = a.shape
    if odd and d > 256:
        return
    Ut, V, B, G, add, C_ref, lse_ref, dB_ref = winner(name, d, H)
    pitch = _pitch(d, odd)
    Bv, Gv = _padded(B, dev, pitch), _padded(G, dev, pitch)
    Ud, Vd = _dev(Ut, dev), _dev(V, dev)
    out, lse = ops.spgat(A, Bv, Ud, Vd, slope=SLOPE, heads=H)
    assert ref.same_bits(_np(out), C_ref) and ref.same_bits(_np(lse), lse_ref)
    runs = [ops.spgat_bwd(A, At, Bv, Ud, Vd, Gv, out, lse, slope=SLOPE, heads=H) for _ in range(2)]
    dB, dU, dV, delta = (_np(t) for t in runs[0])
    assert ref.same_bits(dB, dB_ref)
    assert not dU.any() and not dV.any() and dU.shape == (M, H) and dV.shape == (K, H)           # exactly 0
    assert all(ref.same_bits(_np(x), _np(y)) for x, y in zip(*runs))
    dBa = _np(ops.spgat_bwd(A, At, Bv, Ud, Vd, Gv, out, lse, slope=SLOPE, heads=H, add=_padded(add, dev, pitch), add_rows=K)[0])
    assert ref.same_bits(dBa, dB_ref + add)


# ---- the kink ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,H,plan,slope", [("mixed", 1, "none", 0.2), ("mixed", 2, "8", 0.2), ("mixed", 4, "default", 0.25),
                                               ("zero", 1, "none", 0.5), ("zero", 2, "8", 0.25), ("zero", 4, "8", 0.5)])
def test_kink(dev, kind, H, plan, slope):
    """Dyadic scores on rows of power-of-two degree (1 .. 64).  ``mixed``: U[i] in {-1, 0, 1, 2} / 2 and V[j] in {-2, .., 1} / 2,
    so rows hold z < 0, z > 0 and z == 0 exactly.  ``zero``: u = -v everywhere (U = 3, V = -3), every z is 0 exactly, every s is
    0, the forward is the uniform regime (C exact, small-integer B) and every dz = slope e.  The backward recomputes
    p = exp(s - lse) from the ROUNDED lse, so p is 1 / n only to within rounding: dU, dV, dB and delta are held to the derived
    bound, not to the bit -- and the derivative 1 at z == 0 in place of the slope lies OUTSIDE that bound (asserted on the
    reference, which makes the bound check on dV the check of the kink)."""
    from stochastic_gcn_amd import ops
    a, at = dc.readout_pattern("square")
    A, At = _csr(a, dev, plan), _csr(at, dev, plan)
    M, K = a.shape
    dh = 8
    d = dh * H
    rng = np.random.RandomState(cs.seed("kink", kind, H))
    if kind == "mixed":
        Ut = (rng.randint(-1, 3, (M, H)) * 0.5).astype(np.float32)
        V = (rng.randint(-2, 2, (K, H)) * 0.5).astype(np.float32)
        B, G = rng.standard_normal((K, d)).astype(np.float32), rng.standard_normal((M, d)).astype(np.float32)
    else:
        Ut, V = np.full((M, H), 3.0, np.float32), np.full((K, H), -3.0, np.float32)
        B, G = sc.ints(rng, (K, d), -2, 2), sc.ints(rng, (M, d), -2, 2)
    r = ref.backward_f64(a, Ut, V, B, G, slope, H)
    f = r['fwd']
    rows, cols = f.rows, f.cols
    if kind == "mixed":
        z = f.z[0]
        mixed = [i for i in range(M) if (z[rows == i] < 0).any() and (z[rows == i] > 0).any() and (z[rows == i] == 0).any()]
        assert len(mixed) >= M // 8
    else:
        assert all(not zz.any() for zz in f.z) and not r['dU'].any() and np.abs(r['dV']).max() > 0
    for h in range(H):                                      # the derivative 1 at z == 0: outside the bound
        sl = slice(h * dh, (h + 1) * dh)
        t = np.einsum('ek,ek->e', G[rows][:, sl].astype(np.float64), B[cols][:, sl].astype(np.float64))
        e = f.p[h] * (t - r['delta'][rows, h])
        dV1 = np.bincount(cols, weights=e * np.where(f.z[h] >= 0, 1.0, slope), minlength=K)
        assert np.any(np.abs(dV1 - r['dV'][:, h]) > r['bound_dV'][:, h])
    Bv, Gv, Ud, Vd = _dev(B, dev), _dev(G, dev), _dev(Ut, dev), _dev(V, dev)
    out, lse = ops.spgat(A, Bv, Ud, Vd, slope=slope, heads=H)
    what = "kink %s H=%d plan=%s" % (kind, H, plan)
    if kind == "zero":
        assert np.array_equal(_np(out).astype(np.float64), f.C)            # (exact sums of small integers / a power of two)
    _within(_np(out), f.C, f.bound_C, what + " C")
    _within(_np(lse), f.lse, f.bound_lse, what + " lse")
    runs = [ops.spgat_bwd(A, At, Bv, Ud, Vd, Gv, out, lse, slope=slope, heads=H) for _ in range(2)]
    assert all(ref.same_bits(_np(x), _np(y)) for x, y in zip(*runs))
    for k, got in zip(('dB', 'dU', 'dV', 'delta'), runs[0]):
        _within(_np(got), r[k], r['bound_' + k], what + " " + k)


# ---- the general regime ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def general(name, d, H, keep):
    a, _ = cs.pattern(name)
    M, K = a.shape
    rng = np.random.RandomState(cs.seed(name, d, H, "gat general"))
    Ut, V = (1.5 * rng.standard_normal((M, H))).astype(np.float32), (1.5 * rng.standard_normal((K, H))).astype(np.float32)
    B, G, add = (rng.standard_normal(s).astype(np.float32) for s in ((K, d), (M, d), (K, d)))
    key = cs.seed(name, d, H, "key")
    mk = None
    if keep < 1.0:
        from stochastic_gcn_amd import ops
        rows = np.repeat(np.arange(M), np.diff(a.indptr))
        mk = np.stack([ops.attn_kept(rows, a.indices.astype(np.int64), h, key, keep) for h in range(H)], axis=1) \
            * np.float32(np.float32(1.0) / np.float32(keep))
    return Ut, V, B, G, add, key, mk


WORST = {}


@pytest.mark.parametrize("name,d,H,plan,odd", CASES)
def test_general_regime_within_the_bounds(dev, name, d, H, plan, odd):
    from stochastic_gcn_amd import ops
    a, A, At = _pair(name, dev, plan)
    M, K = a.shape
    if odd and d > 256:
        return
    keep = 0.8 if (d + H) % 3 == 0 else 1.0
    with_add = (d + H) % 2 == 0
    Ut, V, B, G, add, key, mk = general(name, d, H, keep)
    r = ref.backward_f64(a, Ut, V, B, G, SLOPE, H, mk, add=add if with_add else None, add_rows=K if with_add else 0)
    f = r['fwd']
    pitch = _pitch(d, odd)
    Bv, Gv, Ud, Vd = _padded(B, dev, pitch), _padded(G, dev, pitch), _dev(Ut, dev), _dev(V, dev)
    what = "spgat %s d=%d H=%d plan=%s keep=%g" % (name, d, H, plan, keep)
    kw = dict(slope=SLOPE, heads=H, keep=keep, key=key)
    Cbuf, Cv = _blank(M, d, dev, pitch)
    out, lse = ops.spgat(A, Bv, Ud, Vd, out=Cv, **kw)
    assert bool(torch.isnan(Cbuf[:, d:]).all().item())
    ratios = dict(C=_within(_np(out), f.C, f.bound_C, what + " C"))
    empty = np.diff(a.indptr) == 0
    l = _np(lse).astype(np.float64)
    assert np.all(l[empty] == -np.inf)
    ratios['lse'] = _within(l[~empty], f.lse[~empty], f.bound_lse[~empty], what + " lse")
    addv = _padded(add, dev, pitch) if with_add else None
    runs = [ops.spgat_bwd(A, At, Bv, Ud, Vd, Gv, out, lse, add=addv, add_rows=K if with_add else 0, **kw) for _ in range(2)]
    assert all(ref.same_bits(_np(x), _np(y)) for x, y in zip(*runs)), what
    for k, got in zip(('dB', 'dU', 'dV', 'delta'), runs[0]):
        ratios[k] = _within(_np(got), r[k], r['bound_' + k], what + " " + k)
    for k, v in ratios.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print("worst ratios so far:", {k: round(v, 4) for k, v in WORST.items()})


# ---- the way back through the scores -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1000, 4097])
@pytest.mark.parametrize("d,H", [(5, 1), (132, 4), (602, 2)])
def test_scores_backward(dev, rows, d, H):
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(cs.seed("scores_bwd", rows, d, H))
    ru = rows if rows % 2 else max(rows - 3, 0)                       # (fewer dU rows than dV rows in half the cases)
    # dyadic: small integers, every product and every sum exact in fp32
    xi, ai = sc.ints(rng, (rows, d), -2, 2), sc.ints(rng, (2, d), -2, 2)
    dUi, dVi, dx0 = sc.ints(rng, (ru, H), -2, 2), sc.ints(rng, (rows, H), -2, 2), sc.ints(rng, (rows, d), -4, 4)
    want = ref.scores_bwd_f64(xi, ai, dUi, dVi, H, dx0)
    assert np.abs(want['da']).max() < 2 ** 20
    pitch = _pitch(d, odd=True)
    dxbuf, dxv = _blank(rows, d, dev, pitch)
    dxv.copy_(_dev(dx0, dev))
    xv = _padded(xi, dev, pitch)
    before = xv.clone()
    da = _np(ops.gat_scores_bwd(xv, _dev(ai, dev), _dev(dUi, dev), _dev(dVi, dev), dx=dxv, heads=H))
    assert np.array_equal(da.astype(np.float64), want['da']) and np.array_equal(_np(dxv).astype(np.float64), want['dx'])
    assert bool(torch.isnan(dxbuf[:, d:]).all().item())
    # a null dX writes nothing but da
    da0 = _np(ops.gat_scores_bwd(xv, _dev(ai, dev), _dev(dUi, dev), _dev(dVi, dev), heads=H))
    assert ref.same_bits(da0, da) and torch.equal(xv, before)
    # real-valued
    x, av = rng.standard_normal((rows, d)).astype(np.float32), rng.standard_normal((2, d)).astype(np.float32)
    dU, dV = rng.standard_normal((ru, H)).astype(np.float32), rng.standard_normal((rows, H)).astype(np.float32)
    dx0 = rng.standard_normal((rows, d)).astype(np.float32)
    want = ref.scores_bwd_f64(x, av, dU, dV, H, dx0)
    outs = []
    for _ in range(2):
        dxv = _dev(dx0, dev)
        outs.append((_np(ops.gat_scores_bwd(_dev(x, dev), _dev(av, dev), _dev(dU, dev), _dev(dV, dev), dx=dxv, heads=H)), _np(dxv)))
    assert ref.same_bits(outs[0][0], outs[1][0]) and ref.same_bits(outs[0][1], outs[1][1])
    _within(outs[0][0], want['da'], want['bound_da'], "da rows=%d d=%d" % (rows, d))
    _within(outs[0][1], want['dx'], want['bound_dx'], "dX rows=%d d=%d" % (rows, d))


# ---- the mask, the limits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,plan", [(1, "none"), (4, "8")])
def test_kept_set_is_the_one_attn_kept_predicts(dev, H, plan):
    """U = V = 0 and an indicator B: every element of C is mk_ijh / n_i exactly (tests/spattn_drop_cases.py's readout)"""
    from stochastic_gcn_amd import ops
    a, _ = dc.readout_pattern("rect")
    M, K = a.shape
    A = _csr(a, dev, plan)
    _, B, C_ref, kept = dc.readout_tables("rect", H)
    z = torch.zeros((K, 2 * H), dtype=torch.float32, device=dev)
    out, _ = ops.spgat(A, _dev(B, dev), z[:M, :H], z[:, H:], slope=SLOPE, heads=H, keep=dc.READOUT_KEEP, key=dc.READOUT_KEY)
    C = _np(out)
    rows, cols = np.repeat(np.arange(M), np.diff(a.indptr)), a.indices.astype(np.int64)
    got = np.stack([C[rows, h * dc.DH + cols % dc.DH] != 0 for h in range(H)], axis=1)
    want = np.stack([ops.attn_kept(rows, cols, h, dc.READOUT_KEY, dc.READOUT_KEEP) for h in range(H)], axis=1)
    assert np.array_equal(got, want) and np.array_equal(want, kept) and ref.same_bits(C, C_ref)


@pytest.mark.parametrize("d,H,pitch", [(602, 2, 604), (1028, 1, 1028), (514, 1, 514), (260, 1, 261), (520, 8, 520)])
def test_widths_over_the_limit_are_refused_with_nothing_written(dev, d, H, pitch):
    from stochastic_gcn_amd import ops
    a, A, At = _pair("m63_k65", dev, "default")
    M, K = a.shape
    Bv, Gv = _padded(np.zeros((K, d), np.float32), dev, pitch), _padded(np.zeros((M, d), np.float32), dev, pitch)
    t = torch.zeros((K, H), dtype=torch.float32, device=dev)
    Cbuf, Cv = _blank(M, d, dev, pitch)
    with pytest.raises(RuntimeError, match="over the limit of"):
        ops.spgat(A, Bv, t, t, out=Cv, heads=H)
    assert bool(torch.isnan(Cbuf).all().item())
    with pytest.raises(RuntimeError, match="over the limit of"):
        ops.spgat_bwd(A, At, Bv, t, t, Gv, Gv, torch.zeros((M, H), device=dev), heads=H)
