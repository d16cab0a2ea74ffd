"""Every dense-layer product, checked on ALL elements against an independent fp64 reference (tests/dense_cases.py).

ops.gemm, ops.dense_fwd and ops.dense_bwd run once per cell of their launch plans (K-groups 1 / 2 / 4, split over K or
not, vector or scalar loads, every fused epilogue and its N classes, every input-gradient form of the backward), each
case on two kinds of input.  On small-integer inputs (dropout keeps of 0.5 / 0.8, whose fp32 scales 2 and 1.25 keep the
operands dyadic) fp32 arithmetic is exact in any summation order, so the GEMM products and the plain and ReLU forms equal
the fp64 value bit for bit; the LayerNorm outputs are held to ``dense_cases.ln_fwd_bound`` around ref64's LayerNorm of the
exact pre-activation.  On real-valued inputs every element lies within the bounds derived in dense_cases.  Besides: two
calls give the same bits; the pitch padding and the rows after the output (NaN sentinels) are never written; operands
sit in NaN-filled buffers, some one float off alignment or with an odd pitch, and are not changed; accumulated outputs
(C, dW, d offset, d scale) start from non-zero values."""
import contextlib
import zlib

import numpy as np
import pytest
import torch

import dense_cases as dc
import sparse_cases as sc
from gpu_checks import Operand, Output, check, compare, f32

pytestmark = pytest.mark.gpu

EPS = 1e-9


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


@contextlib.contextmanager
def knob(name, value):
    from stochastic_gcn_amd._ffi import lib
    old = int(lib.sgcn_tune_get(name))
    assert lib.sgcn_tune(name, int(value)) == 0
    try:
        yield
    finally:
        lib.sgcn_tune(name, old)


def _vals(rng, shape, exact, scale=1.0):
    return sc.ints(rng, shape) if exact else (rng.standard_normal(shape) * scale).astype(np.float32)


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


# ---- ops.gemm ---------------------------------------------------------------------------------------------------------------
def _run_gemm(dev, c, exact, tag):
    from stochastic_gcn_amd import ops
    M, N, K, ta, tb = c["M"], c["N"], c["K"], c["ta"], c["tb"]
    rng = np.random.RandomState(_seed("gemm", tag, exact))
    A = _vals(rng, (K, M) if ta else (M, K), exact)
    B = _vals(rng, (N, K) if tb else (K, N), exact, 1.0 / np.sqrt(max(K, 1)))
    Ao = _operand(A, dev, c.get("vec_a"), c.get("off_a"), tag)
    Bo = _operand(B, dev, c.get("vec_b"), c.get("off_b"), tag + 1)
    for side, o in (("a", Ao), ("b", Bo)):
        if c.get("vec_" + side):
            assert _aligned(o.view) == (c["vec_" + side] == "on"), (c, side)
    acc = bool(c.get("accumulate"))
    C_in = _vals(rng, (M, N), exact) if acc else None
    kw, dk = {}, {}
    if c.get("drop_a"):
        key = _seed("drop_a", tag)
        kw.update(mask_a=_mask(key, A.shape, c["drop_a"]), scale_a=dc.f32_scale(c["drop_a"]))
        dk["drop_a"] = ops.Drop(c["drop_a"], key)
    if c.get("drop_c"):
        key = _seed("drop_c", tag)
        kw.update(mask_c=_mask(key, (M, N), c["drop_c"]), scale_c=dc.f32_scale(c["drop_c"]))
        dk["drop_c"] = ops.Drop(c["drop_c"], key)
    if exact:
        ref, bound = dc.gemm_exact(A, B, ta, tb, C_in, acc, **kw), None
    else:
        ref, bound = dc.gemm_f64(A, B, ta, tb, C_in, acc, **kw)[0], dc.gemm_bound(A, B, ta, tb, C_in, acc, **kw)
    return check(lambda out: ops.gemm(Ao.view, Bo.view, out=out, trans_a=ta, trans_b=tb, accumulate=acc, **dk), dev, M, N,
                 N + 3, ref, bound, C_in=C_in, operands=[Ao, Bo], what="gemm %r exact=%s" % (c, exact))


@pytest.mark.parametrize("i", range(len(dc.GEMM_CASES)))
def test_gemm_cell(dev, i):
    c = dc.GEMM_CASES[i]
    with knob(b"gemm_min_steps", c["knob"]):
        for exact in (True, False):
            _run_gemm(dev, c, exact, i)


@pytest.mark.parametrize("M,N,K", [(128, 128, 1280), (96, 40, 1204), (5, 3, 4000), (300, 128, 602), (64, 130, 700)])
def test_gemm_same_bits_under_every_split(dev, M, N, K):
    """On exact inputs every gemm_min_steps value that changes the split or the K-groups gives the same bits."""
    plans = {}
    for ta, tb in ((False, False), (True, False), (False, True)):
        bits = []
        for k in dc.KNOBS:
            p = dc.ops_gemm_plan(M, N, K, ta, tb, min_steps=k)
            if (ta, tb, p["S"], p["KG"]) in plans:
                continue
            plans[(ta, tb, p["S"], p["KG"])] = k
            with knob(b"gemm_min_steps", k):
                out = _run_gemm(dev, dict(M=M, N=N, K=K, ta=ta, tb=tb, accumulate=True), True, M + N + K)
            bits.append(out.view(torch.int32).cpu())
        assert len(bits) >= 2 and all(torch.equal(b, bits[0]) for b in bits), (ta, tb)


def test_gemm_empty_dimensions(dev):
    """K = 0: C = 0, or C unchanged with accumulate; M = 0 or N = 0: the output buffer is not touched."""
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(3)
    M, N = 37, 41
    for ta in (False, True):
        for tb in (False, True):
            A = Operand(np.zeros((0, M)) if ta else np.zeros((M, 0)), dev, M + 1)
            B = Operand(np.zeros((N, 0)) if tb else np.zeros((0, N)), dev, N + 1)
            C_in = sc.ints(rng, (M, N))
            check(lambda out: ops.gemm(A.view, B.view, out=out, trans_a=ta, trans_b=tb), dev, M, N, N + 2,
                  np.zeros((M, N)), what="K = 0")
            check(lambda out: ops.gemm(A.view, B.view, out=out, trans_a=ta, trans_b=tb, accumulate=True), dev, M, N, N + 2,
                  C_in.astype(np.float64), C_in=C_in, what="K = 0, accumulate")
            for m, n in ((0, N), (M, 0)):
                a = Operand(sc.ints(rng, (5, m) if ta else (m, 5)), dev, max(m, 5) + 1)
                b = Operand(sc.ints(rng, (n, 5) if tb else (5, n)), dev, max(n, 5) + 1)
                o = Output(dev, 3, 7, 8, sc.ints(rng, (3, 7)))
                ops.gemm(a.view, b.view, out=o.buf[:m, :n], trans_a=ta, trans_b=tb, accumulate=bool(m))
                torch.cuda.synchronize()
                assert torch.equal(o.buf.view(torch.int32), o.before), (m, n, ta, tb)


# ---- ops.dense_fwd --------------------------------------------------------------------------------------------------------------
def _dense_fwd_into(x, W, off, sc_, relu, x2, drop, y, xhat, rstd):
    """sgcn_dense_fwd_f32 as ops.dense_fwd calls it, into caller-owned outputs (y with its own pitch)"""
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd._ffi import check as ck, lib
    import ctypes as C
    gidx = gidx2 = None
    if isinstance(x2, ops.GatheredRows):
        x2, gidx2 = x2.src, x2.idx
    if isinstance(x, ops.GatheredRows):
        x, gidx = x.src, x.idx
    n1 = int(x.shape[0] if gidx is None else gidx.shape[0])
    K, N = int(x.shape[1]), int(W.shape[1])
    M = n1 + (0 if x2 is None else int(x2.shape[0] if gidx2 is None else gidx2.shape[0]))
    xp, ldx = ops._rows2d(x, "x")
    x2p, ldx2 = ops._rows2d(x2, "x2") if x2 is not None else (None, 0)
    wp, ldw = ops._rows2d(W, "W")
    yp, ldy = ops._rows2d(y, "y")
    dr = C.byref(drop.struct(K, rows=n1)) if drop is not None else None
    need = int(lib.sgcn_gemm_ws_floats(M, N, K)) if N <= 128 else 0
    ws = ops._gemm_ws(need, y.device) if need else None
    ck(lib.sgcn_dense_fwd_f32(M, N, K, xp, ldx, x2p, ldx2, n1, wp, ldw, ops._ptr(off), ops._ptr(sc_), EPS, int(bool(relu)),
                              yp, ldy, ops._ptr(xhat), ops._ptr(rstd), dr, ops._ptr(ws), ops._ptr(gidx), ops._ptr(gidx2),
                              ops._stream()))


def _rows(dev, rng, n, K, gather, exact, special, tag):
    """(device argument, host rows): n rows of width K, plain (padded pitch) or read through an index with repeated
    ids; ``special`` row values are written into the given rows (of the source, when gathered)"""
    from stochastic_gcn_amd import ops
    if gather:
        R = max(n // 2, 1)
        src = _vals(rng, (R, K), exact)
        idx = rng.randint(0, R, n).astype(np.int32)
        if n > 1:
            idx[-1] = idx[0]
        for r, v in special:
            src[idx[r]] = v
        so = Operand(src, dev, K + 1 + tag % 3)
        return ops.GatheredRows(so.view, f32(idx, dev)), src[idx], [so]
    x = _vals(rng, (n, K), exact)
    for r, v in special:
        x[r] = v
    xo = Operand(x, dev, K + (0, 1, 4)[tag % 3])
    return xo.view, x, [xo]


def _run_fwd(dev, c, exact, tag):
    from stochastic_gcn_amd import ops
    M, N, K, epi = c["M"], c["N"], c["K"], c["epi"]
    split, gather, keep = c["split"], c["gather"], c.get("drop")
    norm, relu = epi in ("ln", "ln_relu"), epi in ("relu", "ln_relu")
    n1 = M if split is None else split
    rng = np.random.RandomState(_seed("fwd", tag, exact))
    W = _vals(rng, (K, N), exact, 1.0 / np.sqrt(K))
    W[0] = 2.0                                      # a constant row of W: operand rows below give constant / shifted rows
    special = [(M - 1, np.eye(1, K, 0)[0] * 3), (M - 2, np.eye(1, K, 0)[0] * 1000 + np.eye(1, K, 1)[0])] if M >= 3 else []
    sp1 = [(r, v) for r, v in special if r < n1]
    sp2 = [(r - n1, v) for r, v in special if r >= n1]
    x, xr, ops_ = _rows(dev, rng, n1, K, gather in ("x", "both"), exact, sp1, tag)
    if split is not None:
        x2, x2r, o2 = _rows(dev, rng, M - n1, K, gather in ("x2", "both"), exact, sp2, tag + 1)
        ops_ += o2
    else:
        x2, x2r = None, np.zeros((0, K), np.float32)
    Wo = Operand(W, dev, N + 4 * (tag % 2))
    drop, mask = None, None
    Aeff = np.concatenate([xr, x2r]).astype(np.float64)
    if keep is not None:
        key = _seed("fdrop", tag)
        drop = ops.Drop(keep, key)
        Aeff[:n1] *= _mask(key, (n1, K), keep) * dc.f32_scale(keep)
        mask = np.ones_like(Aeff)                   # (one more rounding for the scaled operand in the bound)
    off = (sc.ints(rng, (1, N), -2, 2) / 4.0 if exact else 0.1 * rng.standard_normal((1, N))).astype(np.float32)
    scl = (1 + sc.ints(rng, (1, N), -2, 2) / 8.0 if exact else 1 + 0.1 * rng.standard_normal((1, N))).astype(np.float32)
    offd, scd = (f32(off, dev), f32(scl, dev)) if norm else (None, None)
    if exact:
        pre, pre_err = dc.gemm_exact(Aeff, W), None
    else:
        pre, pre_err = dc.gemm_f64(Aeff, W)[0], dc.gemm_bound(Aeff, W, mask_a=mask)
    what = "dense_fwd %r exact=%s" % (c, exact)
    res = []
    for _ in range(2):
        y = Output(dev, M, N, N + 3)
        xh = Output(dev, M, N, N) if norm else None
        rs = Output(dev, M, 1, 1) if norm else None
        _dense_fwd_into(x, Wo.view, offd, scd, relu, x2, drop, y.view, xh.view if norm else None,
                        rs.view[:, 0] if norm else None)
        torch.cuda.synchronize()
        for o in (y, xh, rs):
            if o is not None:
                o.written_inside(what)
        res.append((y, xh, rs))
    for a, b in zip(*res):
        if a is not None:
            assert torch.equal(a.bits(), b.bits()), "%s: two calls differ" % what
    for o in ops_ + [Wo]:
        assert o.unchanged(), "%s: an operand was modified" % what
    y, xh, rs = res[0]
    if not norm:
        want = np.maximum(pre, 0) if relu else pre
        compare(y.host(), want, None if exact else pre_err, what)
        return
    y64, h64, r64 = dc.ln_f64(pre, off[0], scl[0], relu, EPS)
    by, bh, br = dc.ln_fwd_bound(pre, off[0], scl[0], EPS, pre_err, sum_exact=exact)
    compare(y.host(), y64, by, what + " y")
    compare(xh.host(), h64, bh, what + " xhat")
    compare(rs.host()[:, 0], r64, br, what + " rstd")


@pytest.mark.parametrize("i", range(len(dc.FWD_CASES)))
def test_dense_fwd_cell(dev, i):
    c = dc.FWD_CASES[i]
    with knob(b"gemm_min_steps", c["knob"]):
        for exact in (True, False):
            _run_fwd(dev, c, exact, i)


def test_dense_fwd_through_ops_equals_the_raw_call(dev):
    """ops.dense_fwd (the product's entry) and the raw call the cell tests make give the same bits"""
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(9)
    x, mu = f32(sc.ints(rng, (300, 96)), dev), f32(sc.ints(rng, (300, 96)), dev)
    W = f32(sc.ints(rng, (96, 100)), dev)
    off, scl = f32(rng.standard_normal((1, 100)).astype(np.float32), dev), f32(np.ones((1, 100), np.float32), dev)
    drop = ops.Drop(0.8, 77)
    y, (xh, rs) = ops.dense_fwd(x, W, off, scl, True, eps=EPS, x2=mu, drop=drop)
    y2, xh2, rs2 = torch.empty_like(y), torch.empty_like(xh), torch.empty_like(rs)
    _dense_fwd_into(x, W, off, scl, True, mu, drop, y2, xh2, rs2)
    assert torch.equal(y, y2) and torch.equal(xh, xh2) and torch.equal(rs, rs2)


# ---- ops.dense_bwd --------------------------------------------------------------------------------------------------------------
def _run_bwd(dev, c, exact, tag):
    """One backward case.  none / ReLU: exact (integers) or real-valued; LayerNorm: integer x, W, dy and a real-valued
    pre-activation, against ref64 autograd within the bounds (d offset exactly: a sum of integers)."""
    from stochastic_gcn_amd import ops
    n, N, K, act = c["n"], c["N"], c["K"], c["act"]
    norm, relu = act in ("ln", "ln_relu"), act in ("relu", "ln_relu")
    rng = np.random.RandomState(_seed("bwd", tag, exact))
    x, xr, opl = _rows(dev, rng, n, K, c["gidx"], exact or norm, [], tag)
    W = _vals(rng, (K, N), exact or norm, 1.0 / np.sqrt(K))
    Wo = Operand(W, dev, N)                                   # contiguous: the row pass needs ldw == N
    dy = _vals(rng, (n, N), exact or norm)
    dyo = Operand(dy, dev, N + 2)
    keep = dc._drop_keep(c["drop"])
    key = _seed("bdrop", tag)
    drop = None if keep is None else ops.Drop(keep, key)
    s = 1.0 if keep is None or keep >= 1 else dc.f32_scale(keep)
    m = np.ones((n, K)) if keep is None or keep >= 1 else _mask(key, (n, K), keep)
    xe = xr.astype(np.float64) * m * s
    dW0, off0, sc0 = sc.ints(rng, (K, N)), sc.ints(rng, (1, N)), sc.ints(rng, (1, N))
    yo, ctx, scd, pre = None, None, None, None
    if norm:
        pre = rng.standard_normal((n, N))
        off = (0.1 * rng.standard_normal((1, N))).astype(np.float32)
        scl = (1 + 0.1 * rng.standard_normal((1, N))).astype(np.float32)
        y64, h64, r64 = dc.ln_f64(pre, off[0], scl[0], relu, EPS)
        yo = Operand(y64.astype(np.float32), dev, N + 1)
        ctx = (f32(h64.astype(np.float32), dev), f32(r64.astype(np.float32), dev))
        scd = f32(scl, dev)
        assert np.array_equal(y64.astype(np.float32) > 0, y64 > 0)
        gm = dy * (y64 > 0) if relu else dy.astype(np.float64)
        g, doff, dsc = dc.ln_bwd_f64(pre, off[0], scl[0], relu, EPS, dy)
        eg = dc.ln_bwd_bound(gm, h64, r64, scl[0])
    elif relu:
        yv = _vals(rng, (n, N), True)
        yo = Operand(yv, dev, N + 1)
        g, eg = dy * (yv > 0), None
    else:
        g, eg = dy.astype(np.float64), None
    mk = dict(mask_c=m, scale_c=s) if keep is not None and keep < 1 else {}
    if eg is None and exact:
        dW_ref, dW_b = dc.gemm_exact(xe, g, ta=True, C_in=dW0, accumulate=True), None
        dx_ref, dx_b = dc.gemm_exact(g, W, tb=True, **mk), None
    else:
        e = np.zeros_like(g) if eg is None else eg
        dW_ref = dc.gemm_f64(xe, g, ta=True, C_in=dW0, accumulate=True)[0]
        dW_b = np.abs(xe).T @ e + dc.gemm_bound(xe, np.abs(g) + e, ta=True, C_in=dW0, accumulate=True,
                                                mask_a=None if keep is None or keep >= 1 else np.ones_like(xe))
        dx_ref = dc.gemm_f64(g, W, tb=True, **mk)[0]
        dx_b = (e @ np.abs(W).T) * (m * s if mk else 1.0) + dc.gemm_bound(np.abs(g) + e, W, tb=True, **mk)
    what = "dense_bwd %r exact=%s" % (c, exact)
    from stochastic_gcn_amd._ffi import lib
    outs = []
    default = int(lib.sgcn_tune_get(b"step_fuse"))
    for fuse in (default, default & ~8, default):
        with knob(b"step_fuse", fuse):
            dWo = Output(dev, K, N, N + 1, dW0)
            doo = Output(dev, 1, N, N + 1, off0) if norm else None
            dso = Output(dev, 1, N, N + 1, sc0) if norm else None
            dx = ops.dense_bwd(dyo.view, yo.view if yo is not None else None, ctx, scd, relu, x, Wo.view, dWo.view,
                               doo.view if norm else None, dso.view if norm else None, need_dx=True, drop=drop)
            torch.cuda.synchronize()
        for o in (dWo, doo, dso):
            if o is not None:
                o.written_inside(what)
        outs.append((dWo, doo, dso, dx))
    for o in opl + [Wo, dyo] + ([yo] if yo is not None else []):
        assert o.unchanged(), "%s: an operand was modified" % what
    for other in outs[1:]:              # the row-pass and MFMA forms of dx, and a repeat: the same bits
        for a, b in zip(outs[0], other):
            if a is not None:
                ta_ = a if isinstance(a, torch.Tensor) else a.buf
                tb_ = b if isinstance(b, torch.Tensor) else b.buf
                assert torch.equal(ta_.view(torch.int32), tb_.view(torch.int32)), "%s: forms or calls differ" % what
    dWo, doo, dso, dx = outs[0]
    compare(dWo.host(), dW_ref, dW_b, what + " dW")
    compare(dx.double().cpu().numpy(), dx_ref, dx_b, what + " dx")
    if norm:
        compare(doo.host()[0], off0[0] + gm.sum(0), None, what + " d offset")
        h32 = h64.astype(np.float32).astype(np.float64)
        b = (np.abs(gm) * sc.U * np.abs(h64)).sum(0) + dc.gamma(n + 2) * ((np.abs(gm) * np.abs(h32)).sum(0) + np.abs(sc0[0]))
        compare(dso.host()[0], sc0[0] + dsc, b, what + " d scale")
        np.testing.assert_allclose(doff, gm.sum(0), rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("i", range(len(dc.BWD_CASES)))
def test_dense_bwd_cell(dev, i):
    c = dc.BWD_CASES[i]
    for exact in ((False,) if c["act"] in ("ln", "ln_relu") else (True, False)):
        _run_bwd(dev, c, exact, i)


# ---- the dense layers of the full-size S-Reddit step -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def reddit_calls():
    """The dense calls of one eager training step of BASELINE config 3 at full size (S-Reddit: 232,965 vertices, 602
    features, hidden 128, batch 512, 41 classes), recorded from the model: shapes, epilogue, stacked / gathered rows and
    dropout of every ops.gemm / dense_fwd / dense_bwd call."""
    import model_cases as mc
    from oracle import model_np as mnp
    from stochastic_gcn_amd import ops, synthetic
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.vrgcn import VRGCN
    n, train_adj, _, _, _, _, labels, tr, _, _ = synthetic.reddit_like(with_features=False)
    feats = np.zeros((n, 602), np.float32)               # values play no part: the calls' shapes are recorded
    fl = mnp.make_flags(normalization='graphsage', weight_decay=0.0, dropout=0.2, layer_norm=True, hidden1=128,
                        num_fc_layers=2, cv=True, cvd=True, degree=1, preprocess=True)
    case = dict(cfg=dict(model='vr', n=n, classes=41, batch=512), flags=fl, adj=train_adj, feats=feats, nbr=feats,
                labels=labels, train=tr.astype(np.int32)[:4096], L_sched=1, ph=mc.placeholders(1, 41))
    FLAGS.reset()
    FLAGS.update(**{k: v for k, v in fl.items() if hasattr(FLAGS, k)})
    FLAGS.update(native_step=False, batch_size=512)
    m = VRGCN(fl['num_layers'], fl['preprocess'], case['ph'], feats, feats, train_adj, fl['cvd'], is_training=True,
              device=torch.device('cuda:0'))
    m.set_params(mc.make_oracle_model(case, seed=3).params)
    sch = mc.make_scheduler(case, 1)
    calls = []

    def keep(d):
        return None if d is None else d.keep

    def rows(x):
        return "none" if x is None else ("gathered" if isinstance(x, ops.GatheredRows) else "plain")
    real = (ops.gemm, ops.dense_fwd, ops.dense_bwd)

    def gemm(A, B, out=None, trans_a=False, trans_b=False, accumulate=False, drop_a=None, drop_c=None):
        M, K = (A.shape[1], A.shape[0]) if trans_a else (A.shape[0], A.shape[1])
        N = B.shape[0] if trans_b else B.shape[1]
        calls.append(("gemm", dict(M=int(M), N=int(N), K=int(K), ta=bool(trans_a), tb=bool(trans_b), accumulate=bool(accumulate),
                                   drop_a=keep(drop_a), drop_c=keep(drop_c))))
        return real[0](A, B, out, trans_a, trans_b, accumulate, drop_a, drop_c)

    def dense_fwd(x, W, offset, scale, relu, eps=1e-9, x2=None, drop=None):
        n1 = int(x.shape[0])
        M = n1 + (0 if x2 is None else int(x2.shape[0]))
        calls.append(("fwd", dict(M=M, N=int(W.shape[1]), K=int(x.shape[1]), knob=0, split=None if x2 is None else n1,
                                  epi=("ln_relu" if relu else "ln") if offset is not None else ("relu" if relu else "plain"),
                                  gather={("plain", "none"): "none", ("gathered", "none"): "x", ("plain", "plain"): "none",
                                          ("gathered", "plain"): "x", ("plain", "gathered"): "x2",
                                          ("gathered", "gathered"): "both"}[(rows(x), rows(x2))], drop=keep(drop))))
        return real[1](x, W, offset, scale, relu, eps, x2, drop)

    def dense_bwd(dy, y, ctx, scale, relu, x, W, dW, doffset=None, dscale=None, need_dx=True, drop=None):
        kp = keep(drop)
        calls.append(("bwd", dict(n=int(dy.shape[0]), N=int(dy.shape[1]), K=int(x.shape[1]), gidx=rows(x) == "gathered",
                                  act=("ln_relu" if relu else "ln") if ctx is not None else ("relu" if relu else "none"),
                                  drop="off" if kp is None else "keep1" if kp >= 1 else "drop", keep=kp)))
        return real[2](dy, y, ctx, scale, relu, x, W, dW, doffset, dscale, need_dx, drop)
    ops.gemm, ops.dense_fwd, ops.dense_bwd = gemm, dense_fwd, dense_bwd
    try:
        pb = sch.minibatch_packed(512, FLAGS.plan_t, None)
        pb.dropout = 0.2
        m.run_one_step(None, pb, sync=True)
    finally:
        ops.gemm, ops.dense_fwd, ops.dense_bwd = real
        FLAGS.reset()
    uniq = []
    for cl in calls:
        if cl not in uniq:
            uniq.append(cl)
    return uniq


def test_full_size_reddit_dense_layers(dev, reddit_calls):
    """Every dense product of the full-size step at its own shape, every element: the first layer cut over K with its
    split-K LayerNorm pass, the 128 -> 128 layer, the output layer and their weight and input gradients."""
    kinds = [k for k, _ in reddit_calls]
    fwd = [c for k, c in reddit_calls if k == "fwd"]
    bwd = [c for k, c in reddit_calls if k == "bwd"]
    assert fwd and bwd, reddit_calls
    assert any(dc.fwd_cell(c)[1] == "splitk" and c["K"] == 1204 for c in fwd), fwd     # the first layer, cut over K
    assert any(c["K"] == 128 and c["N"] == 128 for c in fwd + bwd), fwd + bwd
    assert any(c["N"] == 41 for c in fwd + bwd + [c for k, c in reddit_calls if k == "gemm"]), reddit_calls
    for i, (kind, c) in enumerate(reddit_calls):
        if kind == "gemm":
            if c["drop_a"] is not None and c["drop_a"] not in (0.5, 0.8):
                continue
            _run_gemm(dev, dict(c, drop_a=c["drop_a"], drop_c=c["drop_c"]), True, 1000 + i)
        elif kind == "fwd":
            _run_fwd(dev, c, True, 1000 + i)
            _run_fwd(dev, c, False, 1000 + i)
        else:
            _run_bwd(dev, c, c["act"] in ("none", "relu"), 1000 + i)
    assert len(kinds) >= 4
