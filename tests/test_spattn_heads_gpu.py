"""Multi-head softmax dot-product attention on the device (ops.spattn / ops.spattn_bwd with ``heads``), every row and every
cell against tests/spattn_heads_ref.py, on the inputs of tests/spattn_heads_cases.py, with the harness of
tests/test_spattn_gpu.py: pitched operands whose pad columns hold NaN, results prefilled with NaN, pads untouched.

Uniform regime: every weight of every head is exactly 1, so C equals fl(sum / n) BIT FOR BIT whatever the heads and the
plan; lse[:, h] stays within 2 u max(1, log n) of log n in every head, -inf on empty rows.
Winner-take-all regime, a different permutation per head: head h's slice of C is the bits of the row of B that wins under
pi_h (a different row per head -- a mixed-up head, a reduction that leaks across sub-groups, a wrong lse column fail in
bits); lse is the winners' scores; dQ equals the addend or +0.0 (delta goes through the loop's own reduction tree, so
e = 0 exactly); dB equals the exact per-head sum of the G slices of the rows whose head-h winner is j.
General regime: every element of C, lse, dQ, dB and the fused dx within the per-head derived bound, with and without
addends; the backward run twice gives equal bits.
heads = 1 is the single-head kernel: the same bits as the calls without ``heads`` and as the single-head exports.
Widths the head-aware vector width cannot hold, and a d the heads do not divide, are refused with nothing written.

Measured on an MI355X, worst |error| / bound over all general cases: see DESIGN.md section 3.7 (multi-head)."""
import ctypes

import numpy as np
import pytest
import torch

import sparse_cases as sc
import spattn_cases as cs1
import spattn_heads_cases as cs
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


def _served_pitches(d, H):
    """the pitches at which one lane group holds d columns: d <= 256 * VW, VW what the pitch allows AND divides d / H"""
    return [p for p in _pitches(d) if d <= 256 * cs.head_vw(d, H, 4 if p % 4 == 0 else 2 if p % 2 == 0 else 1)]


def _padded(x, dev, pitch):
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


def test_every_pair_is_served_and_every_vector_width_is_exercised():
    assert all(_served_pitches(d, H) for d, H in cs.HD)
    vws = {(d, H): max(cs.head_vw(d, H, 4 if p % 4 == 0 else 2 if p % 2 == 0 else 1) for p in _served_pitches(d, H)) for d, H in cs.HD}
    assert vws[(24, 4)] == 2 and vws[(130, 2)] == 1 and vws[(8, 2)] == 4 and vws[(40, 8)] == 1 and vws[(1024, 8)] == 4


@pytest.mark.parametrize("name,d,H,plan", list(cs.cases()))
def test_uniform_regime_bits(dev, name, d, H, plan):
    from stochastic_gcn_amd import ops
    a, A, _ = _pair(name, dev, plan)
    M = a.shape[0]
    if plan == "T" and name == "row_lengths":
        assert A.plan.nfix >= 5                     # two-slot and many-slot rows
    Q, B, C_ref, logn = cs.uniform(name, d)
    empty = np.diff(a.indptr) == 0
    for pitch in _served_pitches(d, H):
        what = "spattn uniform %s d=%d H=%d plan=%s pitch=%d" % (name, d, H, plan, pitch)
        Qv, Bv = _padded(Q, dev, pitch), _padded(B, dev, pitch + 4)
        Cbuf, Cv = _blank(M, d, dev, pitch)
        out, lse = ops.spattn(A, Bv, q=Qv, scale=0.0, out=Cv, heads=H)
        assert out.data_ptr() == Cv.data_ptr() and _pad_untouched(Cbuf, d), what
        assert ref.same_bits(_np(Cv), C_ref), what
        assert tuple(lse.shape) == (M, H), what
        lse = _np(lse).astype(np.float64)
        assert np.all(lse[empty] == -np.inf), what
        for h in range(H):
            assert np.all(np.abs(lse[~empty, h] - logn[~empty]) <= 2 * U * np.maximum(1.0, logn[~empty])), what
        C2buf, C2v = _blank(M, d, dev, pitch)
        out2, none = ops.spattn(A, Bv, q=Qv, scale=0.0, out=C2v, want_lse=False, heads=H)
        assert none is None and ref.same_bits(_np(C2v), C_ref) and _pad_untouched(C2buf, d), what


@pytest.mark.parametrize("name,d,H,plan", list(cs.cases()))
def test_winner_take_all_bits(dev, name, d, H, plan):
    from stochastic_gcn_amd import ops
    a, A, At = _pair(name, dev, plan)
    M, K = a.shape
    Q, B, G, add, C_ref, lse_ref, dB_ref = cs.winner(name, d, H)
    for pitch in _served_pitches(d, H):
        what = "spattn winner %s d=%d H=%d plan=%s pitch=%d" % (name, d, H, plan, pitch)
        Qv, Bv, Gv, addv = _padded(Q, dev, pitch), _padded(B, dev, pitch + 4), _padded(G, dev, pitch), _padded(add, dev, pitch + 8)
        Cbuf, Cv = _blank(M, d, dev, pitch)
        out, lse = ops.spattn(A, Bv, q=Qv, scale=1.0, out=Cv, heads=H)
        assert _pad_untouched(Cbuf, d), what
        assert ref.same_bits(_np(Cv), C_ref), what
        assert ref.same_bits(_np(lse), lse_ref), what
        for add_rows in (0, M, M // 2):
            dq, dx = ops.spattn_bwd(A, At, Bv, Qv, Gv, Cv, lse, 1.0, add=addv if add_rows else None, add_rows=add_rows, heads=H)
            dq_ref = np.zeros((M, d), np.float32)
            dq_ref[:add_rows] = add[:add_rows]
            assert ref.same_bits(_np(dq), dq_ref), "%s add_rows=%d: dQ" % (what, add_rows)
            assert ref.same_bits(_np(dx), dB_ref), "%s add_rows=%d: dB" % (what, add_rows)


@pytest.mark.parametrize("name,d,H,plan", list(cs.cases()))
def test_general_regime_within_the_bound(dev, name, d, H, plan, capsys):
    from stochastic_gcn_amd import ops
    a, A, At = _pair(name, dev, plan)
    M, K = a.shape
    Q, B, G, add = cs.general(name, d, H)
    empty = np.diff(a.indptr) == 0
    worst = {}

    def note(key, ratio):
        worst[key] = max(worst.get(key, 0.0), ratio)
    for scale, alias in cs.general_variants(name, d, H):
        for pitch in _served_pitches(d, H):
            what = "spattn general %s d=%d H=%d plan=%s scale=%.4g alias=%s pitch=%d" % (name, d, H, plan, scale, alias, pitch)
            Bv, Gv, addv = _padded(B, dev, pitch + 4), _padded(G, dev, pitch), _padded(add, dev, pitch + 8)
            Qv = None if alias else _padded(Q, dev, pitch)
            Cbuf, Cv = _blank(M, d, dev, pitch)
            out, lse = ops.spattn(A, Bv, q=Qv, scale=scale, out=Cv, heads=H)
            f = cs.general_ref(name, d, H, scale, alias, False)['fwd']
            assert _pad_untouched(Cbuf, d), what
            C, l = _np(Cv), _np(lse).astype(np.float64)
            assert l.shape == (M, H), what
            note('C', _within(C, f.C, f.bound_C, what + ": C"))
            assert np.all(l[empty] == -np.inf) and ref.same_bits(C[empty], np.zeros((int(empty.sum()), d), np.float32)), what
            note('lse', _within(l[~empty], f.lse[~empty], f.bound_lse[~empty], what + ": lse"))
            for with_add in (False, True):
                r = cs.general_ref(name, d, H, scale, alias, with_add)
                kw = dict(add=addv, add_rows=M) if with_add else {}
                dq, dx = ops.spattn_bwd(A, At, Bv, Qv, Gv, Cv, lse, scale, heads=H, **kw)
                dq2, dx2 = ops.spattn_bwd(A, At, Bv, Qv, Gv, Cv, lse, scale, heads=H, **kw)
                assert ref.same_bits(_np(dx), _np(dx2)), what + ": the backward is not reproducible"
                if alias:
                    assert dq is None and dq2 is None
                    note('dx', _within(_np(dx), r['dx'], r['bound_dx'], what + ": fused dx, add=%s" % with_add))
                else:
                    assert ref.same_bits(_np(dq), _np(dq2)), what + ": the backward is not reproducible"
                    note('dQ', _within(_np(dq), r['dQ'], r['bound_dQ'], what + ": dQ, add=%s" % with_add))
                    note('dB', _within(_np(dx), r['dB'], r['bound_dB'], what + ": dB, add=%s" % with_add))
    with capsys.disabled():
        print("\n[spattn heads] %s d=%d H=%d plan=%s: worst |error| / bound %s" % (
            name, d, H, plan, ", ".join("%s %.4f" % kv for kv in sorted(worst.items()))))
    # the allocating form, q = None taken as x[:M]
    if M <= K:
        out, lse = ops.spattn(A, torch.tensor(B).to(dev), scale=0.5, heads=H)
        assert tuple(out.shape) == (M, d) and tuple(lse.shape) == (M, H) and lse.dtype == torch.float32


# ---- heads = 1 is the old kernel ----------------------------------------------------------------------------------------
def _plan_ref(csr, width):
    return ctypes.byref(csr.plan.struct(width)) if csr.plan is not None else None


@pytest.mark.parametrize("d", [33, 128])
@pytest.mark.parametrize("plan", ["none", "T"])
def test_one_head_is_the_single_head_kernel(dev, d, plan):
    from stochastic_gcn_amd import _ffi, ops
    from stochastic_gcn_amd.ops import _stream
    lib = _ffi.lib
    a, A, At = _pair("row_lengths", dev, plan)
    M, K = a.shape
    Q, B, G, add = cs1.general("row_lengths", d)
    scale = float(d) ** -0.5
    Qv, Bv, Gv, addv = (torch.tensor(x).to(dev) for x in (Q, B, G, add))
    out0, lse0 = ops.spattn(A, Bv, q=Qv, scale=scale)
    out1, lse1 = ops.spattn(A, Bv, q=Qv, scale=scale, heads=1)
    assert tuple(lse1.shape) == (M,)
    assert ref.same_bits(_np(out0), _np(out1)) and ref.same_bits(_np(lse0), _np(lse1))
    dq0, dx0 = ops.spattn_bwd(A, At, Bv, Qv, Gv, out0, lse0, scale, add=addv, add_rows=M)
    dq1, dx1 = ops.spattn_bwd(A, At, Bv, Qv, Gv, out0, lse0, scale, add=addv, add_rows=M, heads=1)
    assert ref.same_bits(_np(dq0), _np(dq1)) and ref.same_bits(_np(dx0), _np(dx1))

    # the exports themselves: sgcn_spattn_csr_* against sgcn_spattn_mh_csr_* with heads = 1
    def fwd(mh):
        C, lse = torch.full((M, d), float('nan'), device=dev), torch.full((M,), float('nan'), device=dev)
        head = (A.rowptr.data_ptr(), A.col.data_ptr(), M, K, d) + ((1,) if mh else ())
        fn = lib.sgcn_spattn_mh_csr_f32 if mh else lib.sgcn_spattn_csr_f32
        assert fn(*head, Qv.data_ptr(), d, Bv.data_ptr(), d, scale, C.data_ptr(), d, lse.data_ptr(), _plan_ref(A, d + 4), _stream()) == 0
        return C, lse

    def bwd(mh, C, lse):
        delta, dQ, dB = (torch.full(s, float('nan'), device=dev) for s in ((M,), (M, d), (K, d)))
        one = (1,) if mh else ()
        fq = lib.sgcn_spattn_mh_csr_bwd_q_f32 if mh else lib.sgcn_spattn_csr_bwd_q_f32
        fkv = lib.sgcn_spattn_mh_csr_bwd_kv_f32 if mh else lib.sgcn_spattn_csr_bwd_kv_f32
        assert fq(A.rowptr.data_ptr(), A.col.data_ptr(), M, K, d, *one, Qv.data_ptr(), d, Bv.data_ptr(), d, scale, Gv.data_ptr(), d,
                  C.data_ptr(), d, lse.data_ptr(), delta.data_ptr(), dQ.data_ptr(), d, addv.data_ptr(), d, M,
                  _plan_ref(A, d), _stream()) == 0
        assert fkv(At.rowptr.data_ptr(), At.col.data_ptr(), K, M, d, *one, Qv.data_ptr(), d, Bv.data_ptr(), d, scale, Gv.data_ptr(), d,
                   lse.data_ptr(), delta.data_ptr(), dB.data_ptr(), d, None, 0, 0, _plan_ref(At, d), _stream()) == 0
        return delta, dQ, dB
    C_old, lse_old = fwd(False)
    C_new, lse_new = fwd(True)
    assert ref.same_bits(_np(C_old), _np(C_new)) and ref.same_bits(_np(lse_old), _np(lse_new))
    assert ref.same_bits(_np(C_old), _np(out0)) and ref.same_bits(_np(lse_old), _np(lse0))
    for x, y in zip(bwd(False, C_old, lse_old), bwd(True, C_old, lse_old)):
        assert ref.same_bits(_np(x), _np(y))


# ---- refusals on the device path ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,H", [(520, 8), (516, 4)])
def test_widths_the_head_width_cannot_hold_are_refused(dev, d, H):
    """dh = 65 / 129 is odd, so VW = 1 whatever the 16-byte pitch allows, and d > 256: refused with the limit, nothing written"""
    from stochastic_gcn_amd import _ffi, ops
    a, A, At = _pair("m63_k65", dev, "default")
    M, K = a.shape
    pitch = d + 4
    assert pitch % 4 == 0
    mk = lambda rows: torch.zeros((rows, pitch), dtype=torch.float32, device=dev)[:, :d]
    Cbuf, Cv = _blank(M, d, dev, pitch)
    with pytest.raises(_ffi.SgcnError, match=r"over the limit of 256 columns at vector width 1.*must also divide d / heads = %d" % (d // H)):
        ops.spattn(A, mk(K), q=mk(M), scale=1.0, out=Cv, heads=H)
    assert bool(torch.isnan(Cbuf).all().item())
    with pytest.raises(_ffi.SgcnError, match=r"over the limit of 256 columns"):
        ops.spattn_bwd(A, At, mk(K), mk(M), mk(M), mk(M), torch.zeros((M, H), device=dev), 1.0, heads=H)
    # the same width in two heads of an even width is served
    if d == 520:
        out, lse = ops.spattn(A, mk(K), q=mk(M), scale=1.0, heads=2)
        assert tuple(out.shape) == (M, d) and tuple(lse.shape) == (M, 2)


def test_heads_that_do_not_divide_the_width_are_refused(dev):
    from stochastic_gcn_amd import _ffi, ops
    from stochastic_gcn_amd.ops import _stream
    a, A, At = _pair("m63_k65", dev, "none")
    M, K = a.shape
    x, q = torch.zeros((K, 12), device=dev), torch.zeros((M, 12), device=dev)
    with pytest.raises(ValueError, match="not a multiple of heads = 8"):
        ops.spattn(A, x, q=q, scale=1.0, heads=8)
    with pytest.raises(ValueError, match="heads must be one of 1/2/4/8"):
        ops.spattn(A, x, q=q, scale=1.0, heads=3)
    C = torch.full((M, 12), float('nan'), device=dev)
    rc = _ffi.lib.sgcn_spattn_mh_csr_f32(A.rowptr.data_ptr(), A.col.data_ptr(), M, K, 12, 8, q.data_ptr(), 12, x.data_ptr(), 12, 1.0,
                                         C.data_ptr(), 12, None, None, _stream())
    assert rc == -1 and b"d = 12 is not a multiple of heads = 8" in _ffi.lib.sgcn_last_error()
    assert bool(torch.isnan(C).all().item())
