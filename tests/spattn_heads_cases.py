"""The inputs of tests/test_spattn_heads_gpu.py, built without a device so that tests/test_spattn_heads.py can hold the
reference's bounds to the very same arrays (test-only helper; seeded by the arguments and cached like spattn_cases.py, what
a builder returns is read-only).

(d, H) pairs -- the smallest shapes at which each mechanism of the multi-head kernels can go wrong:
    (2, 2), (8, 8)        dh = 1: one lane per head, no reduction at all
    (6, 2), (12, 4)       dh = 3: scalar lanes, a head's sub-group wider than its vectors
    (8, 2)                one float4 per head
    (24, 4)               dh = 6: VW = 2 at best, three vectors per head
    (40, 8)               dh = 5
    (64, 2), (64, 8)      64-wide rows at two head counts
    (128, 4)              the model's width
    (130, 2)              dh = 65: VW = 1, 3 vectors per lane
    (256, 8)              256-wide rows, eight heads
    (1024, 2), (1024, 8)  4 vectors per lane at both ends

Three regimes (tests/test_spattn_heads_gpu.py says what each one pins):
  uniform   scale = 0 and a dyadic B: every weight of every head is exactly 1 -- spattn_cases.uniform as it is (the result
            does not depend on the heads; lse is log n in every head)
  winner    Q[i, h dh] = 1, B[j, h dh] = 256 pi_h(j) with a DIFFERENT seeded permutation per head, scale = 1: head h's slice of
            C is the bits of the row of B that wins under pi_h, a different row per head -- a mixed-up head fails in bits
  general   normal Q, B, G, add; scale 1 / sqrt(dh) and 1; Q a table of its own, and Q = B[:M] on the square patterns
"""
import functools

import numpy as np

import sparse_cases as sc
import spattn_cases as cs
import spattn_heads_ref as href

HD = ((2, 2), (8, 8), (6, 2), (12, 4), (8, 2), (24, 4), (40, 8), (64, 2), (64, 8), (128, 4), (130, 2), (256, 8),
      (1024, 2), (1024, 8))
PLANS = cs.PLANS
# row_lengths at every pair; every other pattern at two small pairs
PAIRS = [("row_lengths", d, H) for d, H in HD] + [
    ("empty", 2, 2), ("empty", 24, 4), ("star_row", 8, 8), ("star_row", 6, 2), ("star_col", 12, 4), ("star_col", 8, 2),
    ("m63_k65", 40, 8), ("m63_k65", 24, 4), ("m65_k63", 6, 2), ("m65_k63", 64, 8), ("m4097_k4095", 8, 2), ("m4097_k4095", 12, 4),
    ("m64_k64", 12, 4), ("m64_k64", 128, 4)]        # (square: the fused form, Q = B[:M], one gradient dx)
assert {(d, H) for _, d, H in PAIRS} == set(HD)

pattern = cs.pattern
seed = cs.seed
_freeze = cs._freeze


def cases():
    for name, d, H in PAIRS:
        for plan in PLANS:
            if plan == "1" and name in cs.TOO_LARGE_FOR_T1:
                continue
            yield name, d, H, plan


def head_vw(d, H, pitch_vw):
    """the kernels' vector width: the widest of what the pitches allow that divides d / H (H > 1)"""
    vw = pitch_vw
    if H > 1:
        while (d // H) % vw:
            vw //= 2
    return vw


def uniform(name, d):
    return cs.uniform(name, d)


@functools.lru_cache(maxsize=None)
def winner(name, d, H):
    """(Q, B, G, add, C, lse (M x H), dB without the addend); G and add are small integers, so the sums of G over the rows that
    share a head's winner are exact in any order."""
    a, _ = pattern(name)
    M, K = a.shape
    dh = d // H
    rng = np.random.RandomState(seed(name, d, H, "winner"))
    B = (sc.ints(rng, (K, d)) * np.float32(0.25)).astype(np.float32)
    Q = np.zeros((M, d), np.float32)
    G = sc.ints(rng, (M, d), -2, 2)
    add = sc.ints(rng, (M, d), -4, 4)
    indptr, cols = a.indptr.astype(np.int64), a.indices.astype(np.int64)
    pis, jstars = [], []
    for h in range(H):
        pi = rng.permutation(K).astype(np.float64)             # (drawn in turn from one stream: different per head)
        B[:, h * dh] = (256.0 * pi).astype(np.float32)         # (a multiple of 256 below 2^25: an fp32 number)
        assert np.array_equal(B[:, h * dh].astype(np.float64), 256.0 * pi)
        Q[:, h * dh] = 1.0
        pos = cs._seg_argmax(pi[cols], indptr)
        jstars.append(np.where(pos >= 0, cols[np.maximum(pos, 0)] if cols.size else 0, -1))
        pis.append(pi)
    if H > 1 and K > 8:
        assert any(not np.array_equal(pis[0], p) for p in pis[1:])
    C = np.zeros((M, d), np.float32)
    lse = np.full((M, H), -np.inf, np.float32)
    dB = np.zeros((K, d), np.float64)
    for h, js in enumerate(jstars):
        has, s = js >= 0, slice(h * dh, (h + 1) * dh)
        C[has, s] = B[js[has], s]
        lse[has, h] = B[js[has], h * dh]
        np.add.at(dB[:, s], js[has], G[has, s].astype(np.float64))
    assert float(np.max(np.abs(dB))) < 2.0 ** 24 if dB.size else True
    dB = dB.astype(np.float32)
    _freeze(Q, B, G, add, C, lse, dB)
    return Q, B, G, add, C, lse, dB


def general_variants(name, d, H):
    """[(scale, alias)]: Q a table of its own at 1 / sqrt(dh) and 1; Q = B[:M] (the model's case) on the square patterns"""
    M, K = pattern(name)[0].shape
    dh = d // H
    v = [(float(dh) ** -0.5, False), (1.0, False)]
    if M == K:
        v.append((float(dh) ** -0.5, True))
    return v


@functools.lru_cache(maxsize=None)
def general(name, d, H):
    """(Q, B, G, add): standard normal tables"""
    a, _ = pattern(name)
    M, K = a.shape
    rng = np.random.RandomState(seed(name, d, H, "general"))
    out = tuple(rng.standard_normal(s).astype(np.float32) for s in ((M, d), (K, d), (M, d), (M, d)))
    _freeze(*out)
    return out


@functools.lru_cache(maxsize=None)
def general_ref(name, d, H, scale, alias, with_add):
    """the fp64 reference of one general case: spattn_heads_ref.backward_f64's dict ('fwd': the forward and its bounds)"""
    a, _ = pattern(name)
    Q, B, G, add = general(name, d, H)
    M = a.shape[0]
    kw = dict(add=add, add_rows=M) if with_add else {}
    r = href.backward_f64(a, B[:M] if alias else Q, B, G, scale, H, fused=alias, **kw)
    _freeze(*[v for v in r.values() if isinstance(v, np.ndarray)])
    return r
