"""NumPy reference of the bfloat16 history's storage contract (include/sgcn.h, "bfloat16 history"): integer arithmetic
on the fp32 bit patterns only, so it shares nothing with the code under test."""
import numpy as np

# the values the contract names: zeros, infinities, ties to even (down and up), the largest bfloat16 (kept), the first
# fp32 that rounds to inf, subnormals (rounded, not flushed), and a value with all mantissa bits of a bfloat16 set
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.3895314e38, 3.4e38,
                     1e-40, -1e-45, 65280.0], dtype=np.float32)


def round_bits(x):
    """fp32 array -> uint16 bfloat16 bit patterns, round to nearest even; a NaN becomes some NaN."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (u >> 16) | 0x40, r)
    return r.astype(np.uint16).reshape(np.shape(x))


def widen_bits(b):
    """uint16 bfloat16 bit patterns -> the fp32 values they stand for (exact)."""
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).reshape(np.shape(b))


def round_trip(x):
    """what a bfloat16 history hands back for an fp32 row x"""
    return widen_bits(round_bits(x))


def wide_values(n, seed=0):
    """n fp32 values spanning 1e-20 .. 1e20 in magnitude, both signs, followed by SPECIALS"""
    rng = np.random.RandomState(seed)
    v = (10.0 ** rng.uniform(-20, 20, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    return np.concatenate([v, SPECIALS])
