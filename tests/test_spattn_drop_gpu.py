"""Dropout on the attention coefficients on the device (ops.spattn / ops.spattn_bwd with ``keep`` < 1), against
tests/spattn_drop_ref.py on the inputs of tests/spattn_drop_cases.py.

Mask readout: with Q = 0 and B an indicator table every element of C is mk_ijh / n_i exactly, so the kept set is read off the
device for every (i, j, h) and compared with the NumPy mask, bit for bit -- one head and four, with and without split rows, on a
square and on a rectangular pattern.
Real-valued inputs: every element of C, lse, dQ, dB and the fused dx within the derived per-element bound, nothing exempted;
a row whose every coefficient is dropped gives exactly 0 with a finite lse.
Bitwise identities: lse under dropout is the lse without it; keep = 1 through the new exports is the existing exports'
result in every output; two runs with one key agree.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import sparse_cases as sc
import spattn_cases as cs1
import spattn_drop_cases as dc
import spattn_drop_ref as dref

pytestmark = pytest.mark.gpu
U = dref.U


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


def _padded(x, dev, pitch):
    x = np.asarray(x)
    buf = torch.full((x.shape[0], pitch), float('nan'), dtype=torch.float32, device=dev)
    view = buf[:, :x.shape[1]]
    view.copy_(torch.tensor(x))
    return view


def _blank(rows, d, dev, pitch):
    buf = torch.full((rows, pitch), float('nan'), dtype=torch.float32, device=dev)
    return buf, buf[:, :d]


def _csr(a, dev, plan):
    from stochastic_gcn_amd import ops
    T = {"none": 0, "default": 0, "T": sc.T_SPLIT, "8": 8}[plan]
    return ops.DeviceCSR.from_scipy(a, dev, plan_T=T, with_plan=plan != "none")


def _np(t):
    return t.cpu().numpy()


def _within(got, want, bound, what):
    got = np.asarray(got, np.float64)
    assert np.all(np.isfinite(got)), what
    err = np.abs(got - want)
    ratio = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    print("%s: worst |error| / bound %.4f" % (what, ratio))
    assert np.all(err <= bound), "%s: worst error / bound %.3f" % (what, ratio)
    return ratio


# ---- the mask, read off the device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["none", "8"])
@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("name", sorted(dc.READOUT))
def test_exact_mask_readout(dev, name, H, plan):
    from stochastic_gcn_amd import ops
    a, _ = dc.readout_pattern(name)
    M, K = a.shape
    A = _csr(a, dev, plan)
    if plan == "8":
        assert A.plan.nfix >= M // 7 * 3                    # the rows of 16, 32 and 64 entries are split
    Q, B, C_ref, kept = dc.readout_tables(name, H)
    d = H * dc.DH
    out, lse = ops.spattn(A, torch.tensor(B).to(dev), q=torch.tensor(Q).to(dev), scale=1.0, heads=H, keep=dc.READOUT_KEEP,
                          key=dc.READOUT_KEY)
    C = _np(out)
    assert C.shape == (M, d)
    rows = np.repeat(np.arange(M), np.diff(a.indptr))
    cols = a.indices.astype(np.int64)
    got = np.stack([C[rows, h * dc.DH + cols % dc.DH] != 0 for h in range(H)], axis=1)
    print("%s H=%d plan=%s: %d of %d (entry, head) sites kept on the device, %d in the NumPy mask, %d differ"
          % (name, H, plan, got.sum(), got.size, kept.sum(), (got != kept).sum()))
    assert np.array_equal(got, kept)                        # every (i, j, h)
    assert dref.same_bits(C, C_ref)                         # and every element is mk / n_i exactly, 0 off the pattern
    # every weight is 1: lse = log n_i in every head, whatever was dropped
    logn = np.log(np.diff(a.indptr).astype(np.float64))
    l = _np(lse).astype(np.float64).reshape(M, H)
    assert np.all(np.abs(l - logn[:, None]) <= 2 * U * np.maximum(1.0, logn)[:, None])


# ---- real-valued inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,d,H,plan,keep", dc.GENERAL)
def test_real_valued_inputs_within_the_bound(dev, name, d, H, plan, keep):
    from stochastic_gcn_amd import ops
    a, at = dc.pattern(name)
    A, At = _csr(a, dev, plan), _csr(at, dev, plan)
    M, K = a.shape
    if plan == "T":
        assert A.plan.nfix >= 5 and At.plan is not None     # rows split into two and into many slots
    Q, B, G, add = dc.general(name, d)
    key, scale, pitch = dc.key_for(name, H, keep), dc.scale_of(d, H), dc.PITCH[d]
    assert ops.attn_vw(d, _padded(B, dev, pitch), heads=H) == (4 if H == 1 or (d // H) % 4 == 0 else 2 if (d // H) % 2 == 0 else 1)
    empty = np.diff(a.indptr) == 0
    Bv, Gv, addv, Qt = _padded(B, dev, pitch), _padded(G, dev, pitch), _padded(add, dev, pitch), _padded(Q, dev, pitch)
    for alias, with_add in dc.variants(name):
        what = "spattn drop %s d=%d H=%d plan=%s keep=%.1f alias=%s add=%s" % (name, d, H, plan, keep, alias, with_add)
        r = dc.general_ref(name, d, H, keep, alias, with_add)
        f, mk = r['fwd'], r['mk']
        Qv = None if alias else Qt
        Cbuf, Cv = _blank(M, d, dev, pitch)
        out, lse = ops.spattn(A, Bv, q=Qv, scale=scale, out=Cv, heads=H, keep=keep, key=key)
        assert bool(torch.isnan(Cbuf[:, d:]).all().item()), what
        C, l = _np(Cv), _np(lse).astype(np.float64).reshape(M, H)
        _within(C, f.C, f.bound_C, what + ": C")
        assert np.all(l[empty] == -np.inf), what
        _within(l[~empty], f.lse[~empty], f.bound_lse[~empty], what + ": lse")
        # a row whose every coefficient is dropped (one exists: spattn_drop_cases.key_for): exactly 0, a finite lse
        gone, _ = dc._all_dropped(a, mk)
        assert gone.any(), what
        dh = d // H
        for i, h in zip(*np.nonzero(gone)):
            assert not C[i, h * dh:(h + 1) * dh].any() and np.isfinite(l[i, h]), (what, i, h)
        # lse does not see the mask: the bits of the run without dropout (on operands of the same pitch: the vector width,
        # and with it the order of a dot product's additions, follows the pitches)
        _, lse0 = ops.spattn(A, Bv, q=Qv, scale=scale, out=_blank(M, d, dev, pitch)[1], heads=H)
        assert dref.same_bits(_np(lse0), _np(lse)), what + ": lse differs from the run without dropout"
        kw = dict(add=addv, add_rows=M) if with_add else {}
        dq, dx = ops.spattn_bwd(A, At, Bv, Qv, Gv, Cv, lse, scale, heads=H, keep=keep, key=key, **kw)
        dq2, dx2 = ops.spattn_bwd(A, At, Bv, Qv, Gv, Cv, lse, scale, heads=H, keep=keep, key=key, **kw)
        assert dref.same_bits(_np(dx), _np(dx2)), what + ": the backward is not reproducible"
        if alias:
            assert dq is None and dq2 is None
            _within(_np(dx), r['dx'], r['bound_dx'], what + ": fused dx")
        else:
            assert dref.same_bits(_np(dq), _np(dq2)), what + ": the backward is not reproducible"
            _within(_np(dq), r['dQ'], r['bound_dQ'], what + ": dQ")
            _within(_np(dx), r['dB'], r['bound_dB'], what + ": dB")
        # the same key again: the same bits; another key: another mask
        C2buf, C2v = _blank(M, d, dev, pitch)
        ops.spattn(A, Bv, q=Qv, scale=scale, out=C2v, heads=H, keep=keep, key=key)
        assert dref.same_bits(_np(C2v), C), what + ": two runs with one key differ"
        ops.spattn(A, Bv, q=Qv, scale=scale, out=C2v, heads=H, keep=keep, key=key + 1)
        assert not dref.same_bits(_np(C2v), C), what + ": the key is not read"


# ---- keep = 1 through the new exports is the existing exports' result ----------------------------------------------------------
def _plan_ref(csr, width):
    return ctypes.byref(csr.plan.struct(width)) if csr.plan is not None else None


@pytest.mark.parametrize("d,H", [(30, 1), (8, 2), (260, 2)])
@pytest.mark.parametrize("plan", ["none", "T"])
def test_keep_one_is_the_existing_kernels(dev, d, H, plan):
    from stochastic_gcn_amd import _ffi, ops
    from stochastic_gcn_amd.ops import _stream
    lib = _ffi.lib
    a, at = dc.pattern("row_lengths")
    A, At = _csr(a, dev, plan), _csr(at, dev, plan)
    M, K = a.shape
    Q, B, G, add = cs1.general("row_lengths", d)
    scale = dc.scale_of(d, H)
    Qv, Bv, Gv, addv = (torch.tensor(x).to(dev) for x in (Q, B, G, add))
    slot = (d + 3) // 4 * 4

    def fwd(drop):
        C, lse = torch.full((M, d), float('nan'), device=dev), torch.full((M, H), float('nan'), device=dev)
        head = (A.rowptr.data_ptr(), A.col.data_ptr(), M, K, d, H) + ((1.0, 12345) if drop else ())
        fn = lib.sgcn_spattn_drop_csr_f32 if drop else lib.sgcn_spattn_mh_csr_f32
        assert fn(*head, Qv.data_ptr(), d, Bv.data_ptr(), d, scale, C.data_ptr(), d, lse.data_ptr(), _plan_ref(A, slot + 4 * H),
                  _stream()) == 0
        return C, lse

    def bwd(drop, C, lse):
        delta, dQ, dB = (torch.full(s, float('nan'), device=dev) for s in ((M * H,), (M, d), (K, d)))
        extra = (1.0, 12345) if drop else ()
        fq = lib.sgcn_spattn_drop_csr_bwd_q_f32 if drop else lib.sgcn_spattn_mh_csr_bwd_q_f32
        fkv = lib.sgcn_spattn_drop_csr_bwd_kv_f32 if drop else lib.sgcn_spattn_mh_csr_bwd_kv_f32
        assert fq(A.rowptr.data_ptr(), A.col.data_ptr(), M, K, d, H, *extra, Qv.data_ptr(), d, Bv.data_ptr(), d, scale, Gv.data_ptr(),
                  d, C.data_ptr(), d, lse.data_ptr(), delta.data_ptr(), dQ.data_ptr(), d, addv.data_ptr(), d, M,
                  _plan_ref(A, slot), _stream()) == 0
        assert fkv(At.rowptr.data_ptr(), At.col.data_ptr(), K, M, d, H, *extra, Qv.data_ptr(), d, Bv.data_ptr(), d, scale,
                   Gv.data_ptr(), d, lse.data_ptr(), delta.data_ptr(), dB.data_ptr(), d, None, 0, 0, _plan_ref(At, slot),
                   _stream()) == 0
        return delta, dQ, dB
    C_old, lse_old = fwd(False)
    C_new, lse_new = fwd(True)
    assert dref.same_bits(_np(C_old), _np(C_new)) and dref.same_bits(_np(lse_old), _np(lse_new))
    for x, y in zip(bwd(False, C_old, lse_old), bwd(True, C_old, lse_old)):
        assert dref.same_bits(_np(x), _np(y))
    # and through ops: keep = 1.0 is the call without the keyword
    out0, l0 = ops.spattn(A, Bv, q=Qv, scale=scale, heads=H)
    out1, l1 = ops.spattn(A, Bv, q=Qv, scale=scale, heads=H, keep=1.0, key=99)
    assert dref.same_bits(_np(out0), _np(out1)) and dref.same_bits(_np(l0), _np(l1)) and dref.same_bits(_np(out0), _np(C_old))
    g0 = ops.spattn_bwd(A, At, Bv, Qv, Gv, out0, l0, scale, heads=H)
    g1 = ops.spattn_bwd(A, At, Bv, Qv, Gv, out0, l0, scale, heads=H, keep=1.0, key=99)
    assert all(dref.same_bits(_np(x), _np(y)) for x, y in zip(g0, g1))


def test_bad_keep_is_refused_on_the_device_path_with_nothing_written(dev):
    from stochastic_gcn_amd import _ffi
    from stochastic_gcn_amd.ops import _stream
    a, _ = dc.pattern("m64_k64")
    A = _csr(a, dev, "none")
    x = torch.zeros((64, 8), device=dev)
    C = torch.full((64, 8), float('nan'), device=dev)
    for keep in (0.0, 1.5, float('nan')):
        rc = _ffi.lib.sgcn_spattn_drop_csr_f32(A.rowptr.data_ptr(), A.col.data_ptr(), 64, 64, 8, 1, keep, 1, x.data_ptr(), 8,
                                               x.data_ptr(), 8, 1.0, C.data_ptr(), 8, None, None, _stream())
        assert rc == -1 and b"keep must be finite and in (0, 1]" in _ffi.lib.sgcn_last_error()
    assert bool(torch.isnan(C).all().item())
