"""NumPy restatement of the weights' moving average that --polyak_decay keeps (include/sgcn.h sgcn_adam_ema_f32; the
operand order of average_model, gcn/models.py:107-108):

    avg <- fl(fl(avg * decay) + fl(theta * one_minus)),   decay = fp32(flag),  one_minus = fl(1.0f - decay)

``ema_f32`` does the three roundings one by one in fp32 (NumPy's fp32 multiply and add are separate, correctly rounded
operations: nothing is contracted into an FMA), which is what the device code is held to bit for bit.  ``ema_f64`` is its
twin in fp64 on the SAME two fp32 factors, rounded nowhere, so the two differ by the three roundings only.  With
a = avg * decay, b = theta * one_minus and M = max(|avg|, |theta|): |a| + |b| <= M (a convex combination), each rounding
errs by at most half an ulp of its own result, i.e. by at most 2^-24 times its magnitude, so the sum of the three is at
most 2^-24 (|a| + |b| + |a + b|) <= 2^-23 M -- ONE fp32 ulp of M, the ulp taken as the format's epsilon times the
magnitude (``ulp_bound``).  The grid spacing at M (np.spacing) is between half of that and all of it, and does NOT bound the
difference: a in M's binade and b in the one below give up to 0.5 + 0.25 + 0.5 spacings (1.06 measured at decay 0.9 on
normal data).  A dyadic decay (0.5) makes both products exact and leaves the sum's rounding: half a spacing."""
import numpy as np


def factors(decay):
    """(decay, one_minus) as fp32 scalars: what the host passes to the kernels"""
    d = np.float32(decay)
    return d, np.float32(np.float32(1.0) - d)


def ema_f32(avg, theta, decay):
    d, om = factors(decay)
    avg, theta = np.asarray(avg, np.float32), np.asarray(theta, np.float32)
    a = (avg * d).astype(np.float32)            # fl(avg * decay)
    b = (theta * om).astype(np.float32)         # fl(theta * one_minus)
    return (a + b).astype(np.float32)           # fl(a + b)


def ema_f64(avg, theta, decay):
    d, om = factors(decay)
    return np.asarray(avg, np.float64) * np.float64(d) + np.asarray(theta, np.float64) * np.float64(om)


def fold(theta0, thetas, decay):
    """the average after each of the recorded weight vectors ``thetas``, starting as a copy of ``theta0``"""
    avg, out = np.asarray(theta0, np.float32).copy(), []
    for t in thetas:
        avg = ema_f32(avg, t, decay)
        out.append(avg)
    return out


def _mag(avg, theta):
    return np.maximum(np.abs(np.asarray(avg, np.float64)), np.abs(np.asarray(theta, np.float64)))


def ulp_bound(avg, theta):
    """one fp32 ulp of max(|avg|, |theta|), element by element: 2^-23 times the magnitude (see the module's docstring)"""
    return _mag(avg, theta) * 2.0 ** -23


def spacing(avg, theta):
    """the fp32 grid spacing at max(|avg|, |theta|)"""
    return np.spacing(_mag(avg, theta).astype(np.float32)).astype(np.float64)
