"""Float64 references of the det-dropout, softmax-CE, LayerNorm and Adam kernels (test-only).

Each forward restates the formula the model states (gcn/layers.py:141-202 for the dropout moments, the LayerNorm on
(mu, var) and the ReLU by moment matching; :320-349 for the control-variate aggregator's element-wise operands;
:425-428 for the Gaussian re-sampling; gcn/models.py for softmax cross-entropy and Adam) in float64 torch on the CPU.
Every backward is torch.autograd of that forward -- never a hand derivation -- so that a derivation error shared by the
kernels and oracle/det_np.py cannot hide.  Inputs are the fp32 arrays the kernels get, widened exactly to float64.
"""
import math

import numpy as np
import torch

from oracle.model_np import _fmix32

f64 = torch.float64
_SQRT2 = math.sqrt(2.0)


def t64(x, grad=False):
    return torch.tensor(np.asarray(x, dtype=np.float64), dtype=f64, requires_grad=grad)


def _np(x):
    return None if x is None else x.detach().numpy()


def vjp(fn, inputs, grads):
    """(outputs, d inputs) of fn at `inputs` (NumPy arrays) for the upstream gradients `grads` (one per output)."""
    xs = [t64(x, True) for x in inputs]
    outs = fn(*xs)
    outs = outs if isinstance(outs, tuple) else (outs,)
    pairs = [(o, t64(g)) for o, g in zip(outs, grads) if g is not None]
    dx = torch.autograd.grad([o for o, _ in pairs], xs, [g for _, g in pairs], allow_unused=True)
    return ([_np(o) for o in outs],
            [np.zeros(x.shape) if d is None else _np(d) for x, d in zip(xs, dx)])


def npdf(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def ncdf(x):
    return 0.5 * torch.special.erfc(-x / _SQRT2)


# ---- dropout moments: x ~ (mu, var), dropout(x) / keep ~ (mu, (var + mu^2) / keep - mu^2); plain input: var = 0 ----
def pre(mu, var, keep):
    mu2 = mu * mu
    return ((0.0 if var is None else var) + mu2) / float(keep) - mu2


# ---- LayerNorm on (mu, var): mean stream tf.nn.batch_normalization(eps), variance stream var * scale^2 / V (no eps) ----
def row_var(mu1):
    """Population variance of every row (tf.nn.moments over axis 1)."""
    mean = mu1.mean(dim=1, keepdim=True)
    return ((mu1 - mean) ** 2).mean(dim=1, keepdim=True)


def ln_var(mu1, var1, scale):
    return var1 * scale * scale / row_var(mu1)


def ln_mean(mu1, offset, scale, eps):
    mean = mu1.mean(dim=1, keepdim=True)
    return (mu1 - mean) / torch.sqrt(row_var(mu1) + eps) * scale + offset


def ln_act(x, offset, scale, relu, eps):
    y = ln_mean(x, offset, scale, eps)
    return torch.relu(y) if relu else y


# ---- ReLU by moment matching of a Gaussian ----------------------------------------------------------------------------
def relu_moments(mu, var):
    sigma = torch.sqrt(var)
    alpha = -mu / sigma
    phi, Phi = npdf(alpha), ncdf(alpha)
    Z = ncdf(-alpha) + 1e-10
    r = phi / Z
    mo = Z * (mu + sigma * r)
    vr = torch.relu(var * (1.0 + alpha * r - r * r)) + 1e-10
    return mo, Z * vr + Z * Phi * mo * mo


# ---- Gaussian re-sampling: x = mu + z sqrt(var + 1e-10), z by Box-Muller on the kernel's counter-based hashes -----------
def gauss_uniforms(key, n):
    """(u1, u2): the fp32 uniforms the kernel feeds to Box-Muller for elements 0..n-1 (oracle.det_np.gauss_noise's
    hash arithmetic, bit for bit), before any transcendental function."""
    M = np.uint64(0xFFFFFFFF)
    idx = np.arange(n, dtype=np.uint64)
    h1 = _fmix32((idx * np.uint64(0x9E3779B1) + np.uint64(key & 0xFFFFFFFF)) & M)
    h2 = _fmix32((((idx * np.uint64(0x85EBCA6B)) & M) + np.uint64(0x165667B1) & M) ^ np.uint64(key & 0xFFFFFFFF))
    s = np.float32(1.0 / 16777216.0)
    u1 = ((h1 >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * s
    u2 = ((h2 >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * s
    return u1, u2


def gauss_z(key, n):
    """N(0, 1) per element in float64 from the kernel's fp32 uniforms."""
    u1, u2 = gauss_uniforms(key, n)
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(2.0 * np.pi * u2.astype(np.float64))


def sample(mu, var, z):
    return mu + z * torch.sqrt(var + 1e-10)


# ---- control-variate aggregator on (mu, var): the element-wise operands of its SpMMs -----------------------------------
def agg_prep(mu, var, Hm, Hv, ifield):
    """(delta_mu, ds2, msig2, ds, sbar) with ds = sqrt(var) - sqrt(Hv[ifield]), msig2 = 2 ds sqrt(Hv[ifield])."""
    sbar = torch.sqrt(Hv[ifield])
    ds = torch.sqrt(var) - sbar
    return mu - Hm[ifield], ds * ds, 2.0 * ds * sbar, ds, sbar


# ---- softmax cross-entropy: mean over rows of -sum_k y_k log softmax(z)_k ------------------------------------------
def softmax_ce(z, y):
    """(per-row CE, softmax probabilities); d(mean CE)/dz by autograd is (p sum(y) - y) / n."""
    logp = torch.log_softmax(z, dim=1)
    return -(y * logp).sum(dim=1), torch.exp(logp)


# ---- Adam (tf.train.AdamOptimizer with the bias correction folded into lr_t) ----------------------------------------
def adam(theta, g, m, v, lr_t, beta1, beta2, eps):
    """One update in float64 of fp32 state; the scalars are taken as the fp32 values the kernel receives."""
    b1, b2, lr, ep = (float(np.float32(x)) for x in (beta1, beta2, lr_t, eps))
    theta, g, m, v = (np.asarray(x, np.float64) for x in (theta, g, m, v))
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    return theta - lr * m1 / (np.sqrt(v1) + ep), m1, v1
