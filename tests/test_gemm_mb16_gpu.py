"""The bf16-multiply GEMM (sgcn_gemm_mb16_f32 through ops.gemm_bf16), checked on ALL elements of every case of
tests/mb16_cases.py: the three forms, split over K or not, vector or scalar loads on either operand, accumulate, a mask on
the operand or on the output.  Every call goes through gpu_checks.check: twice on a NaN-sentinelled output, the two results
bit-identical, nothing outside the output written, the operands (in NaN-filled buffers, some off alignment) untouched.

1. Exact: bf16-representable small integers, keeps of 0.5 / 0.8 -- equal to dense_cases.gemm_exact bit for bit.
2. Rounding happens inside, to nearest even: operands that are NOT bf16-representable, the expected value the exact
   product of their bf16_ref.round_trip -- bit for bit.
3. Real-valued: within mb16_cases.reference's per-element bound of the fp64 product of the rounded operands; the worst
   observed err / (gamma(n) mag) per form goes to profiles/dense_bf16_numerics.jsonl (fixture numerics_record).
4. The same bits under every split.  5. Empty dimensions and refusals."""
import contextlib
import json
import os
import zlib

import numpy as np
import pytest
import torch

import bf16_ref
import dense_cases as dc
import mb16_cases as mbc
import sparse_cases as sc
from gpu_checks import Operand, Output, check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}          # form -> the worst err / (gamma(n) mag) of the real-valued runs, and the case it came from
SEEN = set()        # the catalogue cases whose real-valued check has passed in this run


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def numerics_record():
    """After the module's tests: the worst observed err / (gamma(n) mag) per form, next to the 2 the bound allows, goes to
    profiles/dense_bf16_numerics.jsonl -- only from a run in which EVERY case's real-valued check has run and passed (a
    selection of tests leaves the record alone).  The kernel is deterministic, so a full run rewrites the same bytes."""
    SEEN.clear()
    WORST.clear()
    yield
    if SEEN != set(range(len(mbc.CASES))):
        return
    lines = [json.dumps(dict(form=f, worst_err_over_gamma_n_mag=round(WORST[f][0], 4), at=WORST[f][1], allowed=2.0,
                             cases=len([c for c in mbc.CASES if c["form"] == f])), sort_keys=True) for f in sorted(mbc.FORMS)]
    with open(os.path.join(ROOT, "profiles", "dense_bf16_numerics.jsonl"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


@contextlib.contextmanager
def knob(value):
    from stochastic_gcn_amd._ffi import lib
    old = int(lib.sgcn_tune_get(b"gemm_mb16_slice_k"))
    assert lib.sgcn_tune(b"gemm_mb16_slice_k", int(value)) == 0
    try:
        yield
    finally:
        lib.sgcn_tune(b"gemm_mb16_slice_k", old)


def _mask(key, shape, keep):
    from oracle import model_np as mnp
    return mnp.hash_mask(key, shape, keep).astype(np.float64)


def _operand(x, dev, vec, way, i=0):
    """x on the device with vector loads possible ('on': pitch width or width + 4) or not ('off': a pitch of width + 1,
    or the base one float past an aligned one); None: an odd pitch"""
    w = x.shape[1]
    if vec == "on":
        return Operand(x, dev, w + 4 * (i % 2))
    if vec == "off":
        return Operand(x, dev, w + 1) if way == "pitch" else Operand(x, dev, (w + 1 + 3) // 4 * 4 + 4, shift=1)
    return Operand(x, dev, w + 3)


def _aligned(t):
    from stochastic_gcn_amd import ops
    p, ld = ops._rows2d(t, "t")
    return p % 16 == 0 and ld % 4 == 0


def inputs(c, kind, tag):
    """(A, B, C_in, masks) of a case as host arrays.  kind: 'exact' (small integers), 'real' (normal draws) or 'round'
    (not bf16-representable: small integers times 1 + delta, and the tie values of bf16_ref.SPECIALS)."""
    ta, tb = mbc.FORMS[c["form"]]
    M, N, K = c["M"], c["N"], c["K"]
    rng = np.random.RandomState(_seed("mb16", tag, kind))
    sa, sb = ((K, M) if ta else (M, K)), ((N, K) if tb else (K, N))
    if kind == "exact":
        r = mbc.int_range(K)
        A, B = sc.ints(rng, sa, -r, r), sc.ints(rng, sb, -r, r)
        C_in = sc.ints(rng, (M, N))
    elif kind == "real":
        A = rng.standard_normal(sa).astype(np.float32)
        B = (rng.standard_normal(sb) / np.sqrt(max(K, 1))).astype(np.float32)
        C_in = rng.standard_normal((M, N)).astype(np.float32)
    else:
        def off_grid(shape):
            v = rng.randint(1, 5, shape) * rng.choice([-1.0, 1.0], shape)
            delta = rng.uniform(2.0 ** -14, 2.0 ** -10, shape) * rng.choice([-1.0, 1.0], shape)
            x = (v.astype(np.float32) * (np.float32(1.0) + delta.astype(np.float32))).astype(np.float32)
            ties = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8)], np.float32)
            assert set(ties[:2]) <= set(bf16_ref.SPECIALS)
            flat = x.reshape(-1)
            pos = rng.choice(flat.size, min(flat.size, 24), replace=False)
            flat[pos] = ties[np.arange(pos.size) % 4]
            return x
        A, B = off_grid(sa), off_grid(sb)
        C_in = sc.ints(rng, (M, N))
        for x in (A, B):       # the point of the test: not one operand element survives a bf16 round trip
            assert not (bf16_ref.round_trip(x) == x).any()
        assert bf16_ref.round_trip(np.float32(1.0 + 2.0 ** -8)) == 1.0                      # ties go to even: down ...
        assert bf16_ref.round_trip(np.float32(1.0 + 3 * 2.0 ** -8)) == 1.0 + 2.0 ** -6      # ... and up
    kw, keys = {}, {}
    if c.get("drop_a"):
        keys["drop_a"] = _seed("drop_a", tag)
        kw.update(mask_a=_mask(keys["drop_a"], A.shape, c["drop_a"]), scale_a=dc.f32_scale(c["drop_a"]))
    if c.get("drop_c"):
        keys["drop_c"] = _seed("drop_c", tag)
        kw.update(mask_c=_mask(keys["drop_c"], (M, N), c["drop_c"]), scale_c=dc.f32_scale(c["drop_c"]))
    return A, B, (C_in if c.get("accumulate") else None), kw, keys


def expected(c, kind, A, B, C_in, kw):
    """(ref, bound, unit): bound None = bit for bit"""
    ta, tb = mbc.FORMS[c["form"]]
    acc = bool(c.get("accumulate"))
    if kind == "exact":
        return dc.gemm_exact(A, B, ta, tb, C_in, acc, **kw), None, None
    if kind == "round":
        Ar, Br = mbc.rounded_operands(A, B, kw.get("mask_a"), kw.get("scale_a", 1.0))
        kc = {k: v for k, v in kw.items() if k.endswith("_c")}
        return dc.gemm_exact(Ar, Br, ta, tb, C_in, acc, **kc), None, None
    return mbc.reference(A, B, ta, tb, C_in, acc, **kw)


def prepare(c, kind, tag):
    """the host side of a run: inputs and reference (computed once where several runs share them)"""
    A, B, C_in, kw, keys = inputs(c, kind, tag)
    return (A, B, C_in, keys) + tuple(expected(c, kind, A, B, C_in, kw))


def _run(dev, c, kind, tag, prepared=None):
    from stochastic_gcn_amd import ops
    ta, tb = mbc.FORMS[c["form"]]
    M, N = c["M"], c["N"]
    A, B, C_in, keys, ref, bound, unit = prepared if prepared is not None else prepare(c, kind, tag)
    Ao = _operand(A, dev, c.get("vec_a", "on"), c.get("off_a"), tag)
    Bo = _operand(B, dev, c.get("vec_b", "on"), c.get("off_b"), tag + 1)
    for side, o in (("a", Ao), ("b", Bo)):
        if c.get("vec_" + side):
            assert _aligned(o.view) == (c["vec_" + side] == "on"), (c, side)
    dk = {k: ops.Drop(c[k], key) for k, key in keys.items()}
    acc = bool(c.get("accumulate"))
    what = "gemm_bf16 %r %s" % (c, kind)
    if bound is not None:          # measure before asserting: the worst error in units of gamma(n) * mag
        o = Output(dev, M, N, N + 3, C_in)
        ops.gemm_bf16(Ao.view, Bo.view, out=o.view, trans_a=ta, trans_b=tb, accumulate=acc, **dk)
        torch.cuda.synchronize()
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.nanmax(np.where(unit > 0, np.abs(o.host() - ref) / unit, 0.0)))
        print("%s: worst err / (gamma(n) mag) = %.4f" % (what, ratio))
        if ratio > WORST.get(c["form"], (-1.0, None))[0]:
            WORST[c["form"]] = (ratio, dict(M=M, N=N, K=c["K"]))
    return check(lambda out: ops.gemm_bf16(Ao.view, Bo.view, out=out, trans_a=ta, trans_b=tb, accumulate=acc, **dk), dev, M, N,
                 N + 3, ref, bound, C_in=C_in, operands=[Ao, Bo], what=what)


# ---- 1 and 3: every plan cell, exact and real-valued ---------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(mbc.CASES)))
def test_gemm_bf16_cell(dev, i):
    c = mbc.CASES[i]
    with knob(c.get("knob", 0)):
        for kind in ("exact", "real"):
            _run(dev, c, kind, i)
    SEEN.add(i)


# ---- 2: the rounding is the kernel's, to nearest even -----------------------------------------------------------------
ROUND_CASES = [dict(form="NN", M=33, N=41, K=40, drop_a=0.8), dict(form="NT", M=33, N=41, K=40, drop_c=0.5, accumulate=True),
               dict(form="TN", M=33, N=41, K=40, drop_a=0.8, accumulate=True), dict(form="NN", M=33, N=41, K=40),
               dict(form="TN", M=41, N=33, K=40, drop_a=0.5, vec_a=None, vec_b=None)]


@pytest.mark.parametrize("i", range(len(ROUND_CASES)))
def test_operands_are_rounded_inside_to_nearest_even(dev, i):
    _run(dev, ROUND_CASES[i], "round", 1000 + i)


# ---- 4: the same bits under every split ----------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(300, 128, 4097), (33, 3, 4096), (44, 33, 70001)])
def test_same_bits_under_every_split(dev, M, N, K):
    """On exact inputs every value of gemm_mb16_slice_k gives the same bits of the weight-gradient form."""
    bits, slices = [], set()
    c = dict(form="TN", M=M, N=N, K=K, accumulate=True, drop_a=0.8)
    prepared = prepare(c, "exact", M + N + K)
    for k in mbc.KNOBS + (128, 4096):
        slices.add(mbc.plan(M, N, K, True, False, slice_k=k)["S"])
        with knob(k):
            out = _run(dev, c, "exact", M + N + K, prepared)
        bits.append(out.view(torch.int32).cpu())
    assert len(slices) >= 3 and 1 in slices, slices
    assert all(torch.equal(b, bits[0]) for b in bits)


# ---- 5: empty dimensions and refusals ------------------------------------------------------------------------------------
def test_empty_dimensions(dev):
    """K = 0: C = 0, or C unchanged with accumulate; M = 0 or N = 0: the output buffer is not touched (as ops.gemm)."""
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(3)
    M, N = 37, 41
    for ta, tb in mbc.FORMS.values():
        A = Operand(np.zeros((0, M)) if ta else np.zeros((M, 0)), dev, M + 1)
        B = Operand(np.zeros((N, 0)) if tb else np.zeros((0, N)), dev, N + 1)
        C_in = sc.ints(rng, (M, N))
        check(lambda out: ops.gemm_bf16(A.view, B.view, out=out, trans_a=ta, trans_b=tb), dev, M, N, N + 2,
              np.zeros((M, N)), what="K = 0")
        check(lambda out: ops.gemm_bf16(A.view, B.view, out=out, trans_a=ta, trans_b=tb, accumulate=True), dev, M, N, N + 2,
              C_in.astype(np.float64), C_in=C_in, what="K = 0, accumulate")
        for m, n in ((0, N), (M, 0)):
            a = Operand(sc.ints(rng, (5, m) if ta else (m, 5)), dev, max(m, 5) + 1)
            b = Operand(sc.ints(rng, (n, 5) if tb else (5, n)), dev, max(n, 5) + 1)
            o = Output(dev, 3, 7, 8, sc.ints(rng, (3, 7)))
            ops.gemm_bf16(a.view, b.view, out=o.buf[:m, :n], trans_a=ta, trans_b=tb, accumulate=bool(m))
            torch.cuda.synchronize()
            assert torch.equal(o.buf.view(torch.int32), o.before), (m, n, ta, tb)


def test_refusals(dev):
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd._ffi import SgcnError, lib
    a, b = torch.ones(8, 8, device=dev), torch.ones(8, 8, device=dev)
    out = torch.full((8, 8), float("nan"), device=dev)
    with pytest.raises(SgcnError, match=r"\(1, 1\)"):
        ops.gemm_bf16(a, b, out=out, trans_a=True, trans_b=True)
    with pytest.raises(ValueError, match="inner dimensions"):
        ops.gemm_bf16(a, torch.ones(7, 8, device=dev))
    with pytest.raises(ValueError, match="accumulate"):
        ops.gemm_bf16(a, b, accumulate=True)
    with pytest.raises(RuntimeError, match="no CPU fallback|HBM"):
        ops.gemm_bf16(a.cpu(), b)
    with pytest.raises(RuntimeError, match="no CPU fallback|HBM"):
        ops.gemm_bf16(a, b, out=out.cpu())
    for args in ((None, b.data_ptr(), out.data_ptr()), (a.data_ptr(), None, out.data_ptr()), (a.data_ptr(), b.data_ptr(), None)):
        assert lib.sgcn_gemm_mb16_f32(0, 0, 8, 8, 8, args[0], 8, args[1], 8, args[2], 8, 0, None, None, None, None) == -1
        assert b"null operand" in lib.sgcn_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())             # nothing was launched
