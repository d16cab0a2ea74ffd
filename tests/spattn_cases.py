"""The inputs of tests/test_spattn_gpu.py, built without a device so that tests/test_spattn.py can hold the reference's
bounds to the very same arrays (test-only helper).  Every builder is seeded by its arguments and cached; what it returns is
read-only.

Three regimes (tests/test_spattn_gpu.py says what each one pins):
  uniform   scale = 0 and a dyadic B: every weight is exactly 1, the result is the exact sum divided by the row length
  winner    Q[i] = e_0, B[j, 0] = 256 pi(j) for a seeded permutation pi, scale = 1: exact, distinct scores with gaps >= 256,
            every losing weight underflows to exactly 0 and the row's result is the bits of one row of B
  general   normal Q, B, G; scale 1 / sqrt(d) and 1; Q a table of its own, and Q = B[:M] on the square patterns
"""
import functools
import zlib

import numpy as np

import sparse_cases as sc
import spattn_ref as ref

WIDTHS = (1, 3, 4, 5, 31, 32, 33, 64, 65, 128, 130, 257, 602, 1024)
PLANS = ("none", "default", "T", "1")
# row_lengths (rows around the split threshold, up to 9 T + 3 entries) at every width; every other pattern at two
PAIRS = [("row_lengths", d) for d in WIDTHS] + [
    ("empty", 3), ("empty", 64), ("one_row", 130), ("one_row", 602), ("identity", 1), ("identity", 1024),
    ("permutation", 33), ("permutation", 257), ("star_row", 4), ("star_row", 31), ("star_col", 32), ("star_col", 3),
    ("hot_block", 64), ("hot_block", 5), ("row_vector", 130), ("row_vector", 1), ("col_vector", 65), ("col_vector", 4),
    ("m63_k65", 128), ("m63_k65", 1024), ("m65_k63", 31), ("m65_k63", 257), ("m4097_k4095", 33), ("m4097_k4095", 5),
    ("rmat", 4), ("rmat", 1)]
assert {d for _, d in PAIRS} == set(WIDTHS)
TOO_LARGE_FOR_T1 = ("rmat", "star_row")            # (one slot per stored entry: 2^20 slots; a fix-up walk over 100,000 slots)


def cases():
    for name, d in PAIRS:
        for plan in PLANS:
            if plan == "1" and name in TOO_LARGE_FOR_T1:
                continue
            yield name, d, plan


def seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


@functools.lru_cache(maxsize=None)
def pattern(name):
    from stochastic_gcn_amd import ops
    a = sc.pattern(name)
    return a, ops.transpose_host(a)


def _freeze(*xs):
    for x in xs:
        if isinstance(x, np.ndarray):
            x.setflags(write=False)


def _seg_argmax(v, indptr):
    """per non-empty row the position (into v) of its largest entry; -1 for an empty row"""
    M = indptr.shape[0] - 1
    deg = np.diff(indptr)
    rows = np.repeat(np.arange(M), deg)
    order = np.lexsort((v, rows))                  # by row, then by value: a row's last is its largest
    out = np.full(M, -1, np.int64)
    out[rows[order]] = order                       # (later writes win: the largest)
    return out


@functools.lru_cache(maxsize=None)
def uniform(name, d):
    """(Q, B, C expected in fp32, log n per row): scale = 0, B small integers times a power of two -- every partial sum is
    exact in any order (asserted), so C is fl(sum / n), the header's true division applied to the exact sum."""
    a, _ = pattern(name)
    M, K = a.shape
    rng = np.random.RandomState(seed(name, d, "uniform"))
    B = sc.ints(rng, (K, d)) * np.float32(2.0 ** int(rng.randint(-3, 4)))
    Q = rng.standard_normal((M, d)).astype(np.float32)
    sc.assert_exact(np.abs(a) @ np.abs(B.astype(np.float64)), sc.low_exp(B), "spattn uniform %s d=%d" % (name, d))
    ones = a.copy()
    ones.data[:] = 1.0
    total = np.asarray(ones.astype(np.float64) @ B.astype(np.float64)).astype(np.float32)
    n = np.diff(a.indptr)
    C = np.zeros((M, d), np.float32)
    C[n > 0] = total[n > 0] / n[n > 0].astype(np.float32)[:, None]                # fp32 / fp32, correctly rounded
    with np.errstate(divide='ignore'):
        logn = np.log(n.astype(np.float64))
    _freeze(Q, B, C, logn)
    return Q, B, C, logn


@functools.lru_cache(maxsize=None)
def winner(name, d):
    """(Q, B, G, add, C, lse, dB without the addend): see the module docstring.  G and add are small integers, so the sums
    of G over the rows that share a winner are exact in any order."""
    a, _ = pattern(name)
    M, K = a.shape
    rng = np.random.RandomState(seed(name, d, "winner"))
    pi = rng.permutation(K).astype(np.float64)
    B = (sc.ints(rng, (K, d)) * np.float32(0.25)).astype(np.float32)
    B[:, 0] = (256.0 * pi).astype(np.float32)                         # (a multiple of 256 below 2^25: an fp32 number)
    assert np.array_equal(B[:, 0].astype(np.float64), 256.0 * pi)
    Q = np.zeros((M, d), np.float32)
    Q[:, 0] = 1.0
    G = sc.ints(rng, (M, d), -2, 2)
    add = sc.ints(rng, (M, d), -4, 4)
    indptr, cols = a.indptr.astype(np.int64), a.indices.astype(np.int64)
    pos = _seg_argmax(pi[cols], indptr)
    has = pos >= 0
    jstar = np.where(has, cols[np.maximum(pos, 0)] if cols.size else 0, -1)
    C = np.zeros((M, d), np.float32)
    C[has] = B[jstar[has]]
    lse = np.where(has, B[np.maximum(jstar, 0), 0] if K else 0.0, -np.inf).astype(np.float32)
    dB = np.zeros((K, d), np.float64)
    np.add.at(dB, jstar[has], G[has].astype(np.float64))
    assert float(np.max(np.abs(dB))) < 2.0 ** 24 if dB.size else True
    dB = dB.astype(np.float32)
    _freeze(Q, B, G, add, C, lse, dB)
    return Q, B, G, add, C, lse, dB


def general_variants(name, d):
    """[(scale, alias)]: Q a table of its own at both scales; Q = B[:M] (the model's case) on the square patterns"""
    M, K = pattern(name)[0].shape
    v = [(float(d) ** -0.5, False), (1.0, False)]
    if M == K:
        v.append((float(d) ** -0.5, True))
    return v


@functools.lru_cache(maxsize=None)
def general(name, d):
    """(Q, B, G, add): standard normal tables"""
    a, _ = pattern(name)
    M, K = a.shape
    rng = np.random.RandomState(seed(name, d, "general"))
    out = tuple(rng.standard_normal(s).astype(np.float32) for s in ((M, d), (K, d), (M, d), (M, d)))
    _freeze(*out)
    return out


@functools.lru_cache(maxsize=None)
def general_ref(name, d, scale, alias, with_add):
    """the fp64 reference of one general case: spattn_ref.backward_f64's dict (its 'fwd' holds the forward and its bounds)"""
    a, _ = pattern(name)
    Q, B, G, add = general(name, d)
    M = a.shape[0]
    kw = dict(add=add, add_rows=M) if with_add else {}
    r = ref.backward_f64(a, B[:M] if alias else Q, B, G, scale, fused=alias, **kw)
    _freeze(*r.values())
    return r
