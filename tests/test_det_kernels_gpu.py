"""GPU parity tests of the det-dropout kernels (sgcn_det.hip) and of the standalone softmax-CE, LayerNorm and Adam
kernels (sgcn_dense.hip) against the float64 references of tests/ref64.py (backwards by torch.autograd).

Shapes are chosen where these kernels can go wrong: element counts past the 4096-block grid cap (so that the
grid-stride loops take a second pass), rows wider than one wavefront (the lane loops' later trips), more than 64
classes, strided operands, and the numerically delicate ranges of the moment-matching ReLU.  Element-wise errors are
bounded against the magnitudes that enter each result (so cancellation is allowed for, nothing more); selects and
copies are bit-exact."""
import numpy as np
import pytest
import torch

import ref64 as R
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
TOL = 1e-4            # fp32 sums (test_kernels_gpu.py)
ELEM = 1e-6           # element-wise results of a few correctly rounded fp32 operations
NS = [0, 1, 255, 257, (1 << 20) + 37]        # the last is past blocks_for's 4096 x 256 cap
f32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def H(x):
    return x.cpu().numpy()


def within(x, ref, scale, rtol, what):
    """|x - ref| <= rtol * scale element by element (NaN fails)."""
    x, ref, scale = (np.asarray(a, np.float64) for a in (x, ref, scale))
    err = np.abs(x - ref)
    bad = ~(err <= rtol * scale)
    if bad.any():
        i = np.flatnonzero(bad.ravel())[0]
        raise AssertionError("%s: %d of %d elements beyond %.1e; first at %d: got %r, want %r (scale %r)"
                             % (what, bad.sum(), bad.size, rtol, i, x.ravel()[i], ref.ravel()[i], scale.ravel()[i]))


def rowwise_rel(x, ref):
    """max over rows of max|x - ref| / max|ref| in the row."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(x - ref).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1e-30)).max())


def relu_vjp(mu, var, gm, gv):
    """(d_mu, d_var) of the moment-matching ReLU by autograd, and the magnitudes of the two upstream streams' shares
    (the error scale: the kernel adds the two shares, which may cancel)."""
    _, (m1, v1) = R.vjp(R.relu_moments, [mu, var], [gm, None])
    _, (m2, v2) = R.vjp(R.relu_moments, [mu, var], [None, gv])
    return m1 + m2, v1 + v2, np.abs(m1) + np.abs(m2), np.abs(v1) + np.abs(v2)


def bits(x):
    return np.ascontiguousarray(x, dtype=f32).view(np.int32)


# ---- element-wise det ops ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("with_var", [False, True])
def test_det_pre(dev, n, with_var):
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(n + 1)
    mu = (rng.standard_normal(n) * 2).astype(f32)
    var = rng.uniform(0, 2, n).astype(f32) if with_var else None
    keep = 0.7
    out = H(ops.det_pre(T(mu, dev), T(var, dev) if with_var else None, keep))
    ref = R.pre(R.t64(mu), R.t64(var) if with_var else None, keep).numpy()
    assert out.shape == (n,)
    within(out, ref, np.abs(ref), ELEM, "det_pre")


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("want_var", [False, True])
def test_det_pre_bwd_accumulates(dev, n, want_var):
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(n + 2)
    mu, g, d0 = (rng.standard_normal(n).astype(f32) for _ in range(3))
    var = rng.uniform(0, 2, n).astype(f32)
    keep = 0.6
    d_mu = T(d0, dev)
    d_var = ops.det_pre_bwd(T(mu, dev), T(g, dev), keep, d_mu, want_var)
    _, (dm, dv) = R.vjp(lambda m, v: R.pre(m, v, keep), [mu, var], [g])
    within(H(d_mu), d0 + dm, np.abs(d0) + np.abs(dm), ELEM, "d_mu (accumulated)")
    if want_var:
        within(H(d_var), dv, np.abs(dv), ELEM, "d_var")
    else:
        assert d_var is None


@pytest.mark.parametrize("n", NS)
def test_square_and_addmul_accumulates(dev, n):
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(n + 3)
    x, a, b, acc0 = (rng.standard_normal(n).astype(f32) for _ in range(4))
    c = 1.2
    x64 = x.astype(np.float64)
    within(H(ops.square(T(x, dev), c)), f32(c) * x64 * x64, f32(c) * x64 * x64, ELEM, "square")
    acc = T(acc0, dev)
    ops.addmul(acc, T(a, dev), T(b, dev), -0.6)
    inc = float(f32(-0.6)) * a.astype(np.float64) * b
    within(H(acc), acc0 + inc, np.abs(acc0) + np.abs(inc), ELEM, "addmul (accumulated)")


@pytest.mark.parametrize("n", NS)
def test_gauss_sample_is_box_muller_on_the_hash(dev, n):
    """z per element against float64 Box-Muller on the kernel's fp32 uniforms: the fp32 sqrt(-2 log u1) cos(2 pi u2)
    is good to a few ulps of max(1, |z|) (the angle's rounding: 2.4e-7 absolute)."""
    from stochastic_gcn_amd import ops
    key = 0x2545F491 + n
    z = R.gauss_z(key, n)
    zk = H(ops.gauss_sample(T(np.zeros(n, f32), dev), T(np.ones(n, f32), dev), key))      # sqrt(1 + 1e-10) == 1 in fp32
    within(zk, z, np.maximum(1.0, np.abs(z)), 2e-6, "z")
    rng = np.random.RandomState(n + 4)
    mu = rng.standard_normal(n).astype(f32)
    var = rng.uniform(0, 3, n).astype(f32)
    var[::7] = 0                                                                          # sqrt(0 + 1e-10)
    x = H(ops.gauss_sample(T(mu, dev), T(var, dev), key))
    ref = R.sample(R.t64(mu), R.t64(var), R.t64(z)).numpy()
    sd = np.sqrt(var.astype(np.float64) + 1e-10)
    within(x, ref, np.abs(mu) + np.maximum(1.0, np.abs(z)) * sd, 3e-6, "gauss_sample")
    g = rng.standard_normal(n).astype(f32)
    var += f32(1e-3)
    dv = H(ops.gauss_sample_bwd(T(var, dev), T(g, dev), key))
    _, (_, dv_ref) = R.vjp(lambda m, v: R.sample(m, v, R.t64(z)), [mu, var], [g])
    within(dv, dv_ref, np.abs(g) * np.maximum(1.0, np.abs(z)) * 0.5 / np.sqrt(var.astype(np.float64) + 1e-10), 3e-6,
           "gauss_sample_bwd")


def test_gauss_sample_statistics(dev):
    """2^20 samples: moments, Kolmogorov-Smirnov distance to N(0, 1), and no correlation between neighbouring
    indices or between consecutive keys (bounds: ~5 standard errors; the draw is deterministic)."""
    from scipy import stats
    from stochastic_gcn_amd import ops
    n = 1 << 20
    zero, one = T(np.zeros(n, f32), dev), T(np.ones(n, f32), dev)
    z = H(ops.gauss_sample(zero, one, 12345)).astype(np.float64)
    z2 = H(ops.gauss_sample(zero, one, 12346)).astype(np.float64)
    se = 1.0 / np.sqrt(n)
    assert abs(z.mean()) < 5 * se and abs(z.var() - 1.0) < 5 * np.sqrt(2) * se
    assert stats.kstest(z, "norm").statistic < 2.0 * se          # p ~ 1e-3 at 1.95 / sqrt(n)
    assert abs(np.corrcoef(z, z2)[0, 1]) < 5 * se
    assert abs(np.corrcoef(z[:-1], z[1:])[0, 1]) < 5 * se


# ---- ReLU by moment matching ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_det_relu_elementwise(dev, n):
    """Well-conditioned inputs (alpha = -mu / sigma in [-4, 1]) at every grid size; backward against autograd."""
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(n + 5)
    var = np.exp(rng.uniform(-4, 4, n)).astype(f32)
    mu = (-rng.uniform(-4, 1, n) * np.sqrt(var.astype(np.float64))).astype(f32)
    mo, vo = ops.det_relu_fwd(T(mu, dev), T(var, dev))
    (mo_r, vo_r), _ = R.vjp(R.relu_moments, [mu, var], [None, None])
    within(H(mo), mo_r, np.abs(mo_r), 1e-5, "mo")
    within(H(vo), vo_r, np.abs(vo_r), 1e-5, "vo")
    gm, gv = rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)
    dm, dv = ops.det_relu_bwd(T(mu, dev), T(var, dev), T(gm, dev), T(gv, dev))
    dm_r, dv_r, sm, sv = relu_vjp(mu, var, gm, gv)
    within(H(dm), dm_r, sm, TOL, "d_mu")
    within(H(dv), dv_r, sv, TOL, "d_var")


def test_det_relu_sweep(dev):
    """alpha = -mu / sigma over [-8, 40], sigma^2 over [1e-8, 1e4].

    alpha in [-8, 1]: mo and vo to 1e-5 element-wise.  alpha in (1, 2.5]: mo to 1e-5, vo to 1e-4: vo ~ Z sigma^2 q with
    q = 1 + alpha r - r^2 (r = phi / Z), and q loses digits as alpha grows -- at alpha = 2.5, r = 2.82 and q = 0.11, so
    q carries |alpha - 2 r| r / q ~ 80 times the relative error of r (a few fp32 ulps from erfc and exp): ~3e-5.
    Tail (alpha > 2.5, where Z -> 1e-10 takes over): finite, vo > 0, |d mo| <= 1e-5 (|mu| + sigma), and mo >= 1e-10 mu:
    with Z = Phi(-alpha) + 1e-10, mo = sigma (phi - alpha Phi(-alpha)) + 1e-10 mu, which is negative far out (-4e-9 at
    alpha = 40, sigma = 1) in float64 as in the kernel, so mo >= 0 holds only for mu >= 0.
    Backward against autograd at 1e-4 max-norm relative within each (sigma^2, band) group."""
    from stochastic_gcn_amd import ops
    A, S2 = np.meshgrid(np.linspace(-8, 40, 193), np.logspace(-8, 4, 13))
    var = S2.ravel().astype(f32)
    sd = np.sqrt(var.astype(np.float64))
    mu = (-A.ravel() * sd).astype(f32)
    alpha = -mu / sd
    mo, vo = (H(t) for t in ops.det_relu_fwd(T(mu, dev), T(var, dev)))
    (mo_r, vo_r), _ = R.vjp(R.relu_moments, [mu, var], [None, None])
    a, b, tail = alpha <= 1.0, (alpha > 1.0) & (alpha <= 2.5), alpha > 2.5
    within(mo[a | b], mo_r[a | b], np.abs(mo_r[a | b]), 1e-5, "mo (alpha <= 2.5)")
    within(vo[a], vo_r[a], np.abs(vo_r[a]), 1e-5, "vo (alpha <= 1)")
    within(vo[b], vo_r[b], np.abs(vo_r[b]), 1e-4, "vo (1 < alpha <= 2.5)")
    assert np.isfinite(mo[tail]).all() and np.isfinite(vo[tail]).all()
    assert (vo > 0).all() and (mo >= np.minimum(0.0, 1.0001e-10 * mu)).all()
    within(mo[tail], mo_r[tail], np.abs(mu[tail]) + sd[tail], 1e-5, "mo (tail)")
    rng = np.random.RandomState(6)
    gm, gv = rng.standard_normal(mu.size).astype(f32), rng.standard_normal(mu.size).astype(f32)
    dm, dv = (H(t) for t in ops.det_relu_bwd(T(mu, dev), T(var, dev), T(gm, dev), T(gv, dev)))
    _, (dm_r, dv_r) = R.vjp(R.relu_moments, [mu, var], [gm, gv])
    for s2 in np.unique(var):
        for band in (alpha <= 2.5, (alpha > 2.5) & (alpha <= 8), alpha > 8):
            k = band & (var == s2)
            assert onp.rel_err(dm[k], dm_r[k]) <= TOL, ("d_mu", s2)
            assert onp.rel_err(dv[k], dv_r[k]) <= TOL, ("d_var", s2)


def test_det_relu_gate_both_sides(dev):
    """t = var q > 0 (the relu of the variance is open) for an ordinary input; t == 0 where var q underflows.  In fp32
    q >= 0.038 over the whole alpha range, so t <= 0 is reachable only by underflow: var = 2^-149 (denormals are kept)
    at alpha = 0.5 (q = 0.27) gives t = +0, where max(t, 0) + 1e-10 = 1e-10 is also the float64 value.  The open case's backward
    depends on the gated terms (dropping them moves d_mu by 16 % and d_var by 60 %)."""
    from stochastic_gcn_amd import ops
    var = np.array([1.0, 1.4e-45], f32)
    mu = np.array([0.5, -0.5 * np.sqrt(1.4e-45)], f32)
    mo, vo = (H(t) for t in ops.det_relu_fwd(T(mu, dev), T(var, dev)))
    (mo_r, vo_r), _ = R.vjp(R.relu_moments, [mu, var], [None, None])
    assert np.isfinite(mo).all() and np.isfinite(vo).all() and (vo > 0).all()
    within(mo, mo_r, np.abs(mo_r), 1e-5, "mo")
    within(vo, vo_r, np.abs(vo_r), 1e-5, "vo")
    g = np.array([1.0, 1.0], f32)
    dm, dv = (H(t) for t in ops.det_relu_bwd(T(mu, dev), T(var, dev), T(g, dev), T(g, dev)))
    _, (dm_r, dv_r) = R.vjp(R.relu_moments, [mu, var], [g, g])
    within(dm, dm_r, np.abs(dm_r), TOL, "d_mu")
    within(dv, dv_r, np.abs(dv_r), TOL, "d_var")


# ---- LayerNorm on (mu, var): the variance stream ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 5, 1021])
@pytest.mark.parametrize("d", [1, 16, 63, 64, 65, 128, 602, 1204])
def test_det_lnvar(dev, n, d):
    """var2 = var1 s^2 / V with V the row variance (float64 from the same rows; the kernel gets V back from the mean
    stream's rstd), row variances from 1e-6 to 1e2; backward against autograd, d_mu1 and dscale accumulating.

    d == 1: every row is constant (V = 0).  The kernel recovers V as 1 / rstd^2 - eps, which is a few ulps of 1e-10
    from 0 (either sign) or exactly 0, so var2 comes out as +-inf or at least 1e15 var1 s^2 -- recorded here, not
    compared with var1 s^2 / 0."""
    from stochastic_gcn_amd import ops
    eps = 1e-10
    rng = np.random.RandomState(n * 7 + d)
    std = 10.0 ** np.linspace(-3, 1, n)[:, None]
    mu1 = (std * (rng.uniform(-5, 5, (n, 1)) + rng.standard_normal((n, d)))).astype(f32)
    var1 = rng.uniform(0.1, 2.0, (n, d)).astype(f32)
    scale = rng.normal(1.0, 0.5, d).astype(f32)
    _, (xhat, rstd) = ops.ln_act_fwd(T(mu1, dev), T(np.zeros(d, f32), dev), T(scale, dev), False, eps=eps)
    var2 = H(ops.det_lnvar_fwd(T(var1, dev), rstd, T(scale, dev), eps))
    vs2 = var1.astype(np.float64) * scale.astype(np.float64) ** 2
    if d == 1:
        assert not np.isnan(var2).any()
        assert (np.abs(var2) >= 1e15 * vs2).all()
        return
    (ref,), _ = R.vjp(R.ln_var, [mu1, var1, scale], [None])
    within(var2, ref, ref, TOL, "var2")
    g = rng.standard_normal((n, d)).astype(f32)
    _, (dmu_r, dvar_r, dsc_r) = R.vjp(R.ln_var, [mu1, var1, scale], [g])
    mu_pre = (rng.standard_normal((n, d)) * np.abs(dmu_r).max(axis=1, keepdims=True)).astype(f32)
    sc_pre = (rng.standard_normal(d) * np.abs(dsc_r).max()).astype(f32)
    d_mu1, dscale = T(mu_pre, dev), T(sc_pre, dev)
    d_var1 = H(ops.det_lnvar_bwd(T(g, dev), T(var1, dev), xhat, rstd, T(scale, dev), eps, d_mu1, dscale))
    within(d_var1, dvar_r, np.abs(dvar_r), TOL, "d_var1")
    # error scales: the sums over the row (dV) and over the column (dscale) taken of absolute values
    x64, v64, s64 = mu1.astype(np.float64), var1.astype(np.float64), scale.astype(np.float64)
    V = x64.var(axis=1, keepdims=True)
    dv_mag = np.abs(g * v64 * s64 ** 2).sum(axis=1, keepdims=True) / V ** 2
    xc = np.abs(x64 - x64.mean(axis=1, keepdims=True)).max(axis=1, keepdims=True)
    within(H(d_mu1), mu_pre + dmu_r, np.abs(mu_pre) + dv_mag * 2 * xc / d, TOL, "d_mu1 (accumulated)")
    within(H(dscale), sc_pre + dsc_r, np.abs(sc_pre) + np.abs(2 * g * v64 * s64 / V).sum(axis=0), TOL,
           "dscale (accumulated)")


# ---- control-variate aggregator operands ----------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["none", "half", "all"])
def test_det_agg_prep(dev, which):
    """Pitched histories (ldh > d) gathered through an ifield with repeated rows and the last history row, history
    variances with exact zeros; the backward adds a concat aggregator's self half (pitch ldadd > d) to its first
    add_rows rows only."""
    from stochastic_gcn_amd import ops
    n0, d, nh, ldh = 301, 70, 50, 75
    rng = np.random.RandomState(8)
    ifield = rng.randint(0, nh, n0).astype(np.int32)
    ifield[:3] = nh - 1
    ifield[3:6] = 7
    mu = rng.standard_normal((n0, d)).astype(f32)
    var = rng.uniform(0.01, 2.0, (n0, d)).astype(f32)
    Hm = rng.standard_normal((nh, ldh)).astype(f32)
    Hv = rng.uniform(0.0, 2.0, (nh, ldh)).astype(f32)
    Hv[rng.rand(nh, ldh) < 0.2] = 0.0
    Hv[nh - 1, :d:3] = 0.0
    Hm_d, Hv_d = T(Hm, dev)[:, :d], T(Hv, dev)[:, :d]
    dmu, ds2, msig2, ds, sbar = ops.det_agg_prep(T(mu, dev), T(var, dev), Hm_d, Hv_d, T(ifield, dev))
    Hm64, Hv64 = R.t64(Hm[:, :d]), R.t64(Hv[:, :d])
    idx = torch.from_numpy(ifield.astype(np.int64))
    rd, rds2, rms, rds, rsb = (x.numpy() for x in R.agg_prep(R.t64(mu), R.t64(var), Hm64, Hv64, idx))
    hm, sv = Hm[ifield, :d].astype(np.float64), np.sqrt(var.astype(np.float64))
    within(H(dmu), rd, np.abs(mu) + np.abs(hm), ELEM, "delta_mu")
    within(H(sbar), rsb, rsb, ELEM, "sbar")
    within(H(ds), rds, sv + rsb, ELEM, "ds")
    within(H(ds2), rds2, (sv + rsb) ** 2, ELEM, "ds2")
    within(H(msig2), rms, 2 * (sv + rsb) * rsb, ELEM, "msig2")
    assert (H(sbar)[Hv[ifield, :d] == 0] == 0).all()
    add_rows = {"none": 0, "half": n0 // 2, "all": n0}[which]
    g1, g2 = rng.standard_normal((n0, d)).astype(f32), rng.standard_normal((n0, d)).astype(f32)
    wide = rng.standard_normal((n0, 2 * d + 3)).astype(f32)
    d_var = H(ops.det_agg_prep_bwd(T(var, dev), ds, sbar, T(g1, dev), T(g2, dev),
                                   add=T(wide, dev)[:, :d], add_rows=add_rows))
    _, (dv_r,) = R.vjp(lambda v: R.agg_prep(R.t64(mu), v, Hm64, Hv64, idx)[1:3], [var], [g1, g2])
    scale = (2 * (sv + rsb) * np.abs(g1) + 2 * rsb * np.abs(g2)) / (2 * sv)
    dv_r[:add_rows] += wide[:add_rows, :d]
    scale[:add_rows] += np.abs(wide[:add_rows, :d])
    within(d_var, dv_r, scale, ELEM, "d_var")


# ---- relu_eps / gate: selects, bit-exact --------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(1, 1), (37, 70), (2100, 520)])
@pytest.mark.parametrize("eps", [0.0, 1e-10])
def test_relu_eps_into_a_column_block(dev, n, d, eps):
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(n + d)
    raw = rng.standard_normal((n, d + 3)).astype(f32)
    raw[rng.rand(n, d + 3) < 0.1] = 0.0
    raw[rng.rand(n, d + 3) < 0.1] = -0.0
    ov = torch.full((n, 2 * d), -7.25, device=dev)
    out = ops.relu_eps(T(raw, dev)[:, :d], eps, out=ov[:, d:])
    got = H(ov)
    assert out.data_ptr() == ov[:, d:].data_ptr()
    assert (bits(got[:, d:]) == bits(np.maximum(raw[:, :d], f32(0)) + f32(eps))).all()
    assert (got[:, :d] == -7.25).all()


@pytest.mark.parametrize("n,d", [(1, 1), (37, 70), (2100, 520)])
def test_gate_strided(dev, n, d):
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(n * d + 1)
    raw = rng.standard_normal((n, d + 2)).astype(f32)
    raw[rng.rand(n, d + 2) < 0.1] = 0.0
    raw[rng.rand(n, d + 2) < 0.1] = -0.0
    g = rng.standard_normal((n, 2 * d)).astype(f32)
    g[rng.rand(n, 2 * d) < 0.1] = -0.0
    out = H(ops.gate(T(raw, dev)[:, :d], T(g, dev)[:, d:]))
    want = np.where(raw[:, :d] > 0, g[:, d:], f32(0))
    assert out.shape == (n, d) and (bits(out) == bits(want)).all()


# ---- softmax cross-entropy ------------------------------------------------------------------------------------------------
def _ce_inputs(n, c, seed):
    """Logits shifted per row by 0 / +80 / -80, with exact ties of the maximum in some rows; labels one-hot, soft (rows
    not summing to 1), all-zero, or with a tied maximum."""
    rng = np.random.RandomState(seed)
    z = rng.standard_normal((n, c)) * 3 + np.array([0.0, 80.0, -80.0])[np.arange(n) % 3][:, None]
    y = np.zeros((n, c))
    y[np.arange(n), rng.randint(0, c, n)] = 1.0
    for r in range(n):
        kind = r % 5
        if kind == 1:
            y[r] = rng.uniform(0, 1, c) * (rng.rand(c) < 0.5)
        elif kind == 2:
            y[r] = 0.0
        elif kind == 3 and c > 1:
            a, b = sorted(rng.choice(c, 2, replace=False))
            y[r] = 0.0
            y[r, a] = y[r, b] = 0.5
        if r % 4 == 1 and c > 1:
            k = rng.randint(0, c)
            z[r, k] = z[r].max()
        elif r % 4 == 2 and c > 1:
            z[r, c - 1] = z[r].max() + 1.0
            z[r, 0] = z[r, c - 1]
    return z.astype(f32), y.astype(f32)


@pytest.mark.parametrize("n", [1, 3, 5, 1021])
@pytest.mark.parametrize("c", [1, 2, 63, 64, 65, 127, 128, 129, 300, 1000])
def test_softmax_ce_vs_float64(dev, n, c):
    """Loss, accuracy (arg-max ties to the lowest index, as np.argmax), per-row CE, dlogits = (p sum(y) - y) / n,
    the softmax and the evaluation class plane argmax(pred) + 4096 argmax(label), on strided logits.  The +-80 shift
    costs the fp32 log-sum-exp half an ulp of 80 (3.8e-6) in every log p."""
    from stochastic_gcn_amd import ops
    z, y = _ce_inputs(n, c, n * 1000 + c)
    zw = np.zeros((n, c + 5), f32)
    zw[:, 2:2 + c] = z
    stats, dz, pred = ops.softmax_ce(T(zw, dev)[:, 2:2 + c], T(y, dev), want_grad=True, want_pred=True)
    st, dz, pred = H(stats), H(dz), H(pred)
    (ce, p), (dz_r,) = R.vjp(lambda t: R.softmax_ce(t, R.t64(y)), [z], [np.full(n, 1.0 / n), None])
    hit = np.argmax(z, axis=1) == np.argmax(y, axis=1)
    assert abs(st[0] - ce.sum()) <= 1e-5 * max(1.0, np.abs(ce).sum())
    assert abs(st[2] - ce.mean()) <= 1e-5 * max(1.0, np.abs(ce).mean())
    assert st[1] == hit.sum() and abs(st[3] - hit.mean()) <= 1e-6
    within(st[4:4 + n], ce, np.maximum(1.0, np.abs(ce)), 2e-5, "row CE")
    assert (st[4 + n:4 + 2 * n] == hit).all()
    assert onp.rel_err(pred, p) <= 1e-5
    assert onp.rel_err(dz, dz_r) <= 1e-5
    assert (st[4 + 2 * n:4 + 3 * n] == np.argmax(pred, axis=1) + 4096 * np.argmax(y, axis=1)).all()
    s2, dz2, pr2 = ops.softmax_ce(T(zw, dev)[:, 2:2 + c], T(y, dev), want_grad=False, want_pred=False)
    assert dz2 is None and pr2 is None and torch.equal(s2[:4], stats[:4])


def test_softmax_ce_class_plane_limit(dev):
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd._ffi import SgcnError
    z, y = T(np.zeros((2, 4097), f32), dev), T(np.zeros((2, 4097), f32), dev)
    with pytest.raises(SgcnError, match="4096"):
        ops.softmax_ce(z, y, want_pred=True)
    ops.softmax_ce(z, y, want_pred=False)          # the limit is the class plane's only


# ---- standalone LayerNorm + ReLU ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 16, 63, 64, 65, 128, 602, 1204])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("eps", [1e-9, 1e-10])
def test_ln_act_vs_autograd(dev, d, relu, eps):
    """Forward per row at 1e-4 max-norm; dx at 1e-4 of its row's rstd max|dy scale| (the size of the terms it is made
    of: at d = 2, dx is exactly 0); doffset / dscale accumulating into pre-filled buffers, to 1e-4 of the column sums
    of absolute values.  The reference backward takes the ReLU mask from the kernel's y (y > 0, a select), so that a y
    within rounding of 0 cannot flip it."""
    from stochastic_gcn_amd import ops
    n = 133
    rng = np.random.RandomState(d * 4 + relu)
    x = (10.0 ** rng.uniform(-2, 1, (n, 1)) * (rng.uniform(-5, 5, (n, 1)) + rng.standard_normal((n, d)))).astype(f32)
    off = rng.normal(0.2, 0.5, d).astype(f32)
    sc = rng.normal(1.0, 0.5, d).astype(f32)
    y, ctx = ops.ln_act_fwd(T(x, dev), T(off, dev), T(sc, dev), relu, eps=eps)
    yk = H(y)
    (y_r,), _ = R.vjp(lambda a, b, s: R.ln_act(a, b, s, relu, eps), [x, off, sc], [None])
    assert rowwise_rel(yk, y_r) <= TOL
    dy = rng.standard_normal((n, d)).astype(f32)
    gm = dy * (yk > 0) if relu else dy
    _, (dx_r, do_r, ds_r) = R.vjp(lambda a, b, s: R.ln_act(a, b, s, False, eps), [x, off, sc], [gm])
    do0 = (rng.standard_normal(d) * np.abs(do_r).max()).astype(f32)
    ds0 = (rng.standard_normal(d) * np.abs(ds_r).max()).astype(f32)
    doffset, dscale = T(do0, dev), T(ds0, dev)
    dx = ops.ln_act_bwd(T(dy, dev), y, ctx, T(sc, dev), relu, doffset, dscale)
    rstd = H(ctx[1]).astype(np.float64)[:, None]
    within(H(dx), dx_r, rstd * np.abs(gm * sc).max(axis=1, keepdims=True), TOL, "dx")
    xh = np.abs(H(ctx[0]))
    within(H(doffset), do0 + do_r, np.abs(do0) + np.abs(gm).sum(axis=0), TOL, "doffset (accumulated)")
    within(H(dscale), ds0 + ds_r, np.abs(ds0) + np.abs(gm * xh).sum(axis=0), TOL, "dscale (accumulated)")


# ---- Adam ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 256 + 1, 1500000])
def test_adam_step_vs_float64(dev, n):
    """theta, m, v element-wise to 2e-6 of the magnitudes that enter each (|theta| + |step|, |b1 m| + |(1 - b1) g|, v);
    gradients down to 1e-4 so that sqrt(v) is comparable with eps.  The last two sizes are past the 2048-block cap."""
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(n % 1000 + 9)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n)).astype(f32)
    theta = rng.standard_normal(n).astype(f32)
    m = (rng.standard_normal(n) * np.abs(g)).astype(f32)
    v = (rng.uniform(0, 2, n) * g.astype(np.float64) ** 2).astype(f32)
    lr_t, b1, b2, eps = 3e-3, 0.9, 0.999, 1e-8
    td, md, vd = T(theta, dev), T(m, dev), T(v, dev)
    ops.adam_step(td, T(g, dev), md, vd, lr_t, b1, b2, eps)
    th_r, m_r, v_r = R.adam(theta, g, m, v, lr_t, b1, b2, eps)
    b1f = float(f32(b1))
    within(H(md), m_r, b1f * np.abs(m) + (1 - b1f) * np.abs(g), 2e-6, "m")
    within(H(vd), v_r, v_r, 2e-6, "v")
    within(H(td), th_r, np.abs(theta) + np.abs(theta - th_r), 2e-6, "theta")
