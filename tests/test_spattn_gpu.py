"""Softmax dot-product attention over a CSR pattern on the device (ops.spattn / ops.spattn_bwd), every row and every cell
against tests/spattn_ref.py, on the inputs of tests/spattn_cases.py.

Uniform regime (scale = 0, dyadic B): every score is 0, m = 0, every weight exp(0) = 1, l = n_i and the accumulator an
exact sum in any order -- so C equals fl(sum / n_i), include/sgcn.h's true division applied to the exact sum, BIT FOR BIT,
whatever the plan cuts; lse stays within 2 u max(1, log n_i) of log n_i (l is exact, the logarithm rounded once).
Winner-take-all regime (Q[i] = e_0, B[j, 0] = 256 pi(j), scale = 1): scores are exact and distinct with gaps >= 256, every
losing weight underflows to exactly 0, so C[i] is the BITS of B[j*], j* the stored neighbour with the largest pi, and lse
the winner's score; backward with small-integer G: e_ij = 0 exactly, dB[j] equals the sum of G[i] over the rows whose winner
is j bit for bit, dQ equals the addend or +0.0.
General regime (normal tables, scale 1 / sqrt(d) and 1, Q separate and Q = B[:M] on square patterns): every element of C,
lse, dQ, dB and the fused dx lies within the reference's derived bound, with and without addends.
All of it under every plan (none, the default T, T_SPLIT = 64, T = 1: split rows, two-slot rows, many-slot rows) and three
pitches per width (scalar, 2-wide and 4-wide lanes; above 256 columns those whose vector width still holds the row -- the
others are refused, which is tested too); operands sit in pitched buffers whose pad columns hold NaN, results are
prefilled with NaN and their pad columns must come back untouched.  The backward is run twice: bitwise equal."""
import numpy as np
import pytest
import torch

import sparse_cases as sc
import spattn_cases as cs
import spattn_ref as ref

pytestmark = pytest.mark.gpu
U = ref.U


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


def _pitches(d):
    """odd (scalar lanes), a multiple of 2 only, a multiple of 4 (float4 lanes)"""
    c4 = (d + 3) // 4 * 4
    return (d + 1 if d % 2 == 0 else d + 2, c4 + 2, c4 + 4)


def _served(d, pitch):
    """whether one lane group holds d columns at the vector width this pitch allows (d <= 256 * VW); the pitches that do not
    are the refusals of test_widths_over_the_limit_are_refused"""
    return d <= 256 * (4 if pitch % 4 == 0 else 2 if pitch % 2 == 0 else 1)


def _served_pitches(d):
    return [p for p in _pitches(d) if _served(d, p)]


def _padded(x, dev, pitch):
    """x in the first columns of a pitched buffer whose pad columns hold NaN"""
    x = np.asarray(x)
    buf = torch.full((x.shape[0], pitch), float('nan'), dtype=torch.float32, device=dev)
    view = buf[:, :x.shape[1]]
    view.copy_(torch.tensor(x))
    return view


def _blank(rows, d, dev, pitch):
    buf = torch.full((rows, pitch), float('nan'), dtype=torch.float32, device=dev)
    return buf, buf[:, :d]


def _pad_untouched(buf, d):
    return bool(torch.isnan(buf[:, d:]).all().item())


def _csr(a, dev, plan):
    from stochastic_gcn_amd import ops
    T = {"none": 0, "default": 0, "T": sc.T_SPLIT, "1": 1}[plan]
    return ops.DeviceCSR.from_scipy(a, dev, plan_T=T, with_plan=plan != "none")


def _pair(name, dev, plan):
    a, at = cs.pattern(name)
    return a, _csr(a, dev, plan), _csr(at, dev, plan)


def _np(t):
    return t.cpu().numpy()


def _within(got, want, bound, what):
    got = np.asarray(got, np.float64)
    assert np.all(np.isfinite(got)), what
    err = np.abs(got - want)
    ratio = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    assert np.all(err <= bound), "%s: worst error / bound %.3f" % (what, ratio)
    return ratio


@pytest.mark.parametrize("name,d,plan", list(cs.cases()))
def test_uniform_regime_bits(dev, name, d, plan):
    from stochastic_gcn_amd import ops
    a, A, _ = _pair(name, dev, plan)
    M = a.shape[0]
    if plan == "T" and name == "row_lengths":
        assert A.plan.nfix >= 5                     # T + 1, 2 T, 4 T + 1, 9 T + 3, T + 1: two-slot and many-slot rows
    Q, B, C_ref, logn = cs.uniform(name, d)
    empty = np.diff(a.indptr) == 0
    for pitch in _served_pitches(d):
        what = "spattn uniform %s d=%d plan=%s pitch=%d" % (name, d, plan, pitch)
        Qv, Bv = _padded(Q, dev, pitch), _padded(B, dev, pitch + 4)
        Cbuf, Cv = _blank(M, d, dev, pitch)
        out, lse = ops.spattn(A, Bv, q=Qv, scale=0.0, out=Cv)
        assert out.data_ptr() == Cv.data_ptr() and _pad_untouched(Cbuf, d), what
        assert ref.same_bits(_np(Cv), C_ref), what
        lse = _np(lse).astype(np.float64)
        assert np.all(lse[empty] == -np.inf), what
        assert np.all(np.abs(lse[~empty] - logn[~empty]) <= 2 * U * np.maximum(1.0, logn[~empty])), what
        # an evaluation: no lse asked for, the same values
        C2buf, C2v = _blank(M, d, dev, pitch)
        out2, none = ops.spattn(A, Bv, q=Qv, scale=0.0, out=C2v, want_lse=False)
        assert none is None and ref.same_bits(_np(C2v), C_ref) and _pad_untouched(C2buf, d), what


@pytest.mark.parametrize("name,d,plan", list(cs.cases()))
def test_winner_take_all_bits(dev, name, d, plan):
    from stochastic_gcn_amd import ops
    a, A, At = _pair(name, dev, plan)
    M, K = a.shape
    Q, B, G, add, C_ref, lse_ref, dB_ref = cs.winner(name, d)
    for pitch in _served_pitches(d):
        what = "spattn winner %s d=%d plan=%s pitch=%d" % (name, d, plan, pitch)
        Qv, Bv, Gv, addv = _padded(Q, dev, pitch), _padded(B, dev, pitch + 4), _padded(G, dev, pitch), _padded(add, dev, pitch + 8)
        Cbuf, Cv = _blank(M, d, dev, pitch)
        out, lse = ops.spattn(A, Bv, q=Qv, scale=1.0, out=Cv)
        assert _pad_untouched(Cbuf, d), what
        assert ref.same_bits(_np(Cv), C_ref), what
        assert ref.same_bits(_np(lse), lse_ref), what
        for add_rows in (0, M, M // 2):
            dq, dx = ops.spattn_bwd(A, At, Bv, Qv, Gv, Cv, lse, 1.0, add=addv if add_rows else None, add_rows=add_rows)
            dq_ref = np.zeros((M, d), np.float32)
            dq_ref[:add_rows] = add[:add_rows]
            assert ref.same_bits(_np(dq), dq_ref), "%s add_rows=%d: dQ" % (what, add_rows)
            assert ref.same_bits(_np(dx), dB_ref), "%s add_rows=%d: dB" % (what, add_rows)


@pytest.mark.parametrize("name,d,plan", list(cs.cases()))
def test_general_regime_within_the_bound(dev, name, d, plan, capsys):
    from stochastic_gcn_amd import ops
    a, A, At = _pair(name, dev, plan)
    M, K = a.shape
    Q, B, G, add = cs.general(name, d)
    empty = np.diff(a.indptr) == 0
    worst = {}

    def note(key, ratio):
        worst[key] = max(worst.get(key, 0.0), ratio)
    for scale, alias in cs.general_variants(name, d):
        for pitch in _served_pitches(d):
            what = "spattn general %s d=%d plan=%s scale=%.4g alias=%s pitch=%d" % (name, d, plan, scale, alias, pitch)
            Bv, Gv, addv = _padded(B, dev, pitch + 4), _padded(G, dev, pitch), _padded(add, dev, pitch + 8)
            Qv = None if alias else _padded(Q, dev, pitch)
            Cbuf, Cv = _blank(M, d, dev, pitch)
            out, lse = ops.spattn(A, Bv, q=Qv, scale=scale, out=Cv)
            f = cs.general_ref(name, d, scale, alias, False)['fwd']
            assert _pad_untouched(Cbuf, d), what
            C, l = _np(Cv), _np(lse).astype(np.float64)
            note('C', _within(C, f.C, f.bound_C, what + ": C"))
            assert np.all(l[empty] == -np.inf) and ref.same_bits(C[empty], np.zeros((int(empty.sum()), d), np.float32)), what
            note('lse', _within(l[~empty], f.lse[~empty], f.bound_lse[~empty], what + ": lse"))
            for with_add in (False, True):
                r = cs.general_ref(name, d, scale, alias, with_add)
                kw = dict(add=addv, add_rows=M) if with_add else {}
                dq, dx = ops.spattn_bwd(A, At, Bv, Qv, Gv, Cv, lse, scale, **kw)
                dq2, dx2 = ops.spattn_bwd(A, At, Bv, Qv, Gv, Cv, lse, scale, **kw)
                assert ref.same_bits(_np(dx), _np(dx2)), what + ": the backward is not reproducible"
                if alias:
                    assert dq is None and dq2 is None
                    note('dx', _within(_np(dx), r['dx'], r['bound_dx'], what + ": fused dx, add=%s" % with_add))
                else:
                    assert ref.same_bits(_np(dq), _np(dq2)), what + ": the backward is not reproducible"
                    note('dQ', _within(_np(dq), r['dQ'], r['bound_dQ'], what + ": dQ, add=%s" % with_add))
                    note('dB', _within(_np(dx), r['dB'], r['bound_dB'], what + ": dB, add=%s" % with_add))
    with capsys.disabled():
        print("\n[spattn] %s d=%d plan=%s: worst |error| / bound %s" % (
            name, d, plan, ", ".join("%s %.4f" % kv for kv in sorted(worst.items()))))
    # the allocating form, q = None taken as x[:M]
    if M <= K and _served(d, d):                 # (a contiguous table: its pitch is d itself)
        out, lse = ops.spattn(A, torch.tensor(B).to(dev), scale=0.5)
        assert tuple(out.shape) == (M, d) and tuple(lse.shape) == (M,) and lse.dtype == torch.float32


def test_every_width_is_served_at_some_pitch_and_every_vector_width_is_exercised():
    assert all(_served_pitches(d) for d in cs.WIDTHS)
    assert all(len(_served_pitches(d)) == 3 for d in cs.WIDTHS if d <= 256)
    assert [len(_served_pitches(d)) for d in (257, 602, 1024)] == [2, 1, 1]


@pytest.mark.parametrize("d,pitch,limit", [(1025, 1028, 1024), (513, 514, 512), (257, 257, 256), (257, 259, 256), (602, 606, 512),
                                           (602, 603, 256), (1024, 1026, 512), (1024, 1025, 256)])
def test_widths_over_the_limit_are_refused(dev, d, pitch, limit):
    """one lane group holds the whole row: d <= 256 * VW, VW the widest vector the pitches allow -- refused with the limit
    in the message, nothing written"""
    from stochastic_gcn_amd import _ffi, ops
    a, A, At = _pair("m63_k65", dev, "default")
    M, K = a.shape
    mk = lambda rows: torch.zeros((rows, pitch), dtype=torch.float32, device=dev)[:, :d]
    Cbuf, Cv = _blank(M, d, dev, pitch)
    with pytest.raises(_ffi.SgcnError, match=r"over the limit of %d columns" % limit):
        ops.spattn(A, mk(K), q=mk(M), scale=1.0, out=Cv)
    assert bool(torch.isnan(Cbuf).all().item())
    with pytest.raises(_ffi.SgcnError, match=r"over the limit of"):
        ops.spattn_bwd(A, At, mk(K), mk(M), mk(M), mk(M), torch.zeros(M, device=dev), 1.0)
    # one column less, or a wider vector, is served
    if d == 513:
        out, _ = ops.spattn(A, torch.zeros((K, 516), device=dev)[:, :d], q=torch.zeros((M, 516), device=dev)[:, :d], scale=1.0)
        assert tuple(out.shape) == (M, d)
