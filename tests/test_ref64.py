"""CPU self-check of tests/ref64.py, the float64 references of test_det_kernels_gpu.py: the forwards against
oracle/det_np.py's fp32 restatement in the well-conditioned range, the autograd backwards against det_np's
hand-derived ones, and the softmax-CE / LayerNorm / Adam references against direct float64 restatements.  A
disagreement means ref64 or det_np is wrong, before any kernel is run."""
import math

import numpy as np
import pytest
import torch
from scipy.special import logsumexp

import ref64 as R
from oracle import det_np as dn
from oracle import oracle_np as onp

TOL = 1e-5
f32 = np.float32


def _rng(seed):
    return np.random.RandomState(seed)


@pytest.mark.parametrize("with_var", [False, True])
def test_pre_matches_det_np(with_var):
    rng = _rng(1)
    mu = rng.standard_normal((40, 30)).astype(f32)
    var = rng.uniform(0, 2, (40, 30)).astype(f32) if with_var else None
    g = rng.standard_normal((40, 30)).astype(f32)
    keep = 0.7
    ins = [mu, var] if with_var else [mu]
    (out,), d = R.vjp(lambda m, v=None: R.pre(m, v, keep), ins, [g])
    assert onp.rel_err(dn.pre_fwd(mu, var, keep), out) <= TOL
    d_mu, d_var = dn.pre_bwd(mu, g, keep, with_var)
    assert onp.rel_err(d_mu, d[0]) <= TOL
    if with_var:
        assert onp.rel_err(d_var, d[1]) <= TOL


@pytest.mark.parametrize("d", [7, 64, 130])
def test_layernorm_on_moments_matches_det_np(d):
    rng = _rng(d)
    n = 25
    mu1 = (rng.standard_normal((n, d)) * rng.uniform(0.3, 3, (n, 1))).astype(f32)
    var1 = rng.uniform(0.1, 2, (n, d)).astype(f32)
    off, sc = rng.normal(0, 0.5, (1, d)).astype(f32), rng.normal(1, 0.3, (1, d)).astype(f32)
    gm, gv = rng.standard_normal((n, d)).astype(f32), rng.standard_normal((n, d)).astype(f32)
    mu2, var2, ctx = dn.ln_fwd(mu1, var1, off, sc)
    (mu2_r, var2_r), (dmu, dvar, doff, dsc) = R.vjp(
        lambda m, v, o, s: (R.ln_mean(m, o, s, 1e-10), R.ln_var(m, v, s)), [mu1, var1, off, sc], [gm, gv])
    assert onp.rel_err(mu2, mu2_r) <= TOL and onp.rel_err(var2, var2_r) <= TOL
    d_mu1, d_var1, doffset, dscale = dn.ln_bwd(gm, gv, ctx, sc)
    for got, want in ((d_mu1, dmu), (d_var1, dvar), (doffset, doff), (dscale, dsc)):
        assert onp.rel_err(got, want) <= TOL


def test_relu_moments_match_det_np():
    """alpha = -mu / sigma in [-3, 1] (the fp32 restatement loses digits in q = 1 + alpha r - r^2 further out)."""
    rng = _rng(3)
    n = 4000
    var = np.exp(rng.uniform(-6, 6, n)).astype(f32)
    mu = (-rng.uniform(-3, 1, n) * np.sqrt(var.astype(np.float64))).astype(f32)
    gm, gv = rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)
    mo, vo, ctx = dn.relu_fwd(mu, var)
    (mo_r, vo_r), (dm_r, dv_r) = R.vjp(R.relu_moments, [mu, var], [gm, gv])
    assert np.all(np.abs(mo - mo_r) <= TOL * np.abs(mo_r)) and np.all(np.abs(vo - vo_r) <= TOL * np.abs(vo_r))
    dm, dv = dn.relu_bwd(gm, gv, ctx)
    assert onp.rel_err(dm, dm_r) <= TOL and onp.rel_err(dv, dv_r) <= TOL


def test_gaussian_resampling_matches_det_np():
    key, shape = 0xDEADBEEF, (300, 70)
    n = shape[0] * shape[1]
    z = R.gauss_z(key, n)
    z32 = dn.gauss_noise(key, shape).ravel()
    assert np.all(np.abs(z32 - z) <= 2e-6 * np.maximum(1.0, np.abs(z)))
    rng = _rng(4)
    mu, var = rng.standard_normal(n).astype(f32), rng.uniform(0, 2, n).astype(f32)
    g = rng.standard_normal(n).astype(f32)
    (x,), (dmu, dvar) = R.vjp(lambda m, v: R.sample(m, v, R.t64(z)), [mu, var], [g])
    assert onp.rel_err(dn.sample_fwd(mu, var, z32), x) <= TOL
    g_mu, g_var = dn.sample_bwd(g, var, z32)
    assert onp.rel_err(g_mu, dmu) <= TOL and onp.rel_err(g_var, dvar) <= TOL


def test_gaussian_generator_statistics():
    """The hash generator itself (2^20 draws, two keys): moments, KS distance, no correlation across keys or
    neighbouring indices -- the GPU test asserts the same of the kernel."""
    from scipy import stats
    n = 1 << 20
    z, z2 = R.gauss_z(12345, n), R.gauss_z(12346, n)
    se = 1.0 / math.sqrt(n)
    assert abs(z.mean()) < 5 * se and abs(z.var() - 1.0) < 5 * math.sqrt(2) * se
    assert stats.kstest(z, "norm").statistic < 2.0 * se
    assert abs(np.corrcoef(z, z2)[0, 1]) < 5 * se and abs(np.corrcoef(z[:-1], z[1:])[0, 1]) < 5 * se


def test_agg_prep_backward_is_the_chain_rule():
    rng = _rng(5)
    n0, d, nh = 40, 9, 12
    ifield = rng.randint(0, nh, n0)
    mu, var = rng.standard_normal((n0, d)), rng.uniform(0.01, 2, (n0, d))
    Hm, Hv = rng.standard_normal((nh, d)), rng.uniform(0, 2, (nh, d))
    Hv[0] = 0.0
    g1, g2 = rng.standard_normal((n0, d)), rng.standard_normal((n0, d))
    idx = torch.from_numpy(ifield)
    outs, (dv,) = R.vjp(lambda v: R.agg_prep(R.t64(mu), v, R.t64(Hm), R.t64(Hv), idx)[1:3], [var], [g1, g2])
    sb = np.sqrt(Hv[ifield])
    ds = np.sqrt(var) - sb
    np.testing.assert_allclose(outs[0], ds * ds, rtol=1e-12)
    np.testing.assert_allclose(outs[1], 2 * ds * sb, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(dv, (2 * ds * g1 + 2 * sb * g2) / (2 * np.sqrt(var)), rtol=1e-12)


def test_softmax_ce_reference():
    rng = _rng(6)
    n, c = 30, 130
    z = rng.standard_normal((n, c)) * 3 + 80.0
    y = rng.uniform(0, 1, (n, c)) * (rng.rand(n, c) < 0.3)
    (ce, p), (dz,) = R.vjp(lambda t: R.softmax_ce(t, R.t64(y)), [z], [np.full(n, 1.0 / n), None])
    logp = z - logsumexp(z, axis=1, keepdims=True)
    np.testing.assert_allclose(ce, -(y * logp).sum(axis=1), rtol=1e-12)
    np.testing.assert_allclose(p, np.exp(logp), rtol=1e-12)
    np.testing.assert_allclose(dz, (np.exp(logp) * y.sum(axis=1, keepdims=True) - y) / n, rtol=1e-9, atol=1e-15)


@pytest.mark.parametrize("relu", [False, True])
def test_ln_act_reference(relu):
    """Autograd of the LayerNorm + ReLU forward against the closed-form LayerNorm backward."""
    rng = _rng(7)
    n, d, eps = 20, 33, 1e-9
    x = rng.standard_normal((n, d)) * 2 + 1
    off, sc, dy = rng.standard_normal(d), rng.normal(1, 0.3, d), rng.standard_normal((n, d))
    (y,), (dx, doff, dsc) = R.vjp(lambda a, b, s: R.ln_act(a, b, s, relu, eps), [x, off, sc], [dy])
    mean, var = x.mean(axis=1, keepdims=True), x.var(axis=1, keepdims=True)
    r = 1.0 / np.sqrt(var + eps)
    h = (x - mean) * r
    y_ref = h * sc + off
    g = dy * (y_ref > 0) if relu else dy
    np.testing.assert_allclose(y, np.maximum(y_ref, 0) if relu else y_ref, rtol=1e-12, atol=1e-14)
    t = g * sc
    dx_ref = r * (t - t.mean(axis=1, keepdims=True) - h * (t * h).mean(axis=1, keepdims=True))
    np.testing.assert_allclose(dx, dx_ref, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(doff, g.sum(axis=0), rtol=1e-12)
    np.testing.assert_allclose(dsc, (g * h).sum(axis=0), rtol=1e-9, atol=1e-12)


def test_adam_reference():
    rng = _rng(8)
    theta, g, m = (rng.standard_normal(50).astype(f32) for _ in range(3))
    v = rng.uniform(0, 1, 50).astype(f32)
    th1, m1, v1 = R.adam(theta, g, m, v, 3e-3, 0.9, 0.999, 1e-8)
    for i in range(50):
        b1, b2 = float(f32(0.9)), float(f32(0.999))
        mi = b1 * float(m[i]) + (1 - b1) * float(g[i])
        vi = b2 * float(v[i]) + (1 - b2) * float(g[i]) ** 2
        assert m1[i] == mi and v1[i] == vi
        assert th1[i] == float(theta[i]) - float(f32(3e-3)) * mi / (math.sqrt(vi) + float(f32(1e-8)))
