"""Operands of the bf16-table GEMM test (tests/test_gemm_a16_gpu.py; test-only helper): the inputs of a case of
mb16_cases.CASES, an operand placed as the case's load class asks, and the split knob."""
import contextlib
import zlib

import numpy as np

import dense_cases as dc
import mb16_cases as mbc
import sparse_cases as sc
from gpu_checks import Operand


def seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


@contextlib.contextmanager
def knob(value):
    """gemm_mb16_slice_k set to ``value`` inside the block"""
    from stochastic_gcn_amd._ffi import lib
    old = int(lib.sgcn_tune_get(b"gemm_mb16_slice_k"))
    assert lib.sgcn_tune(b"gemm_mb16_slice_k", int(value)) == 0
    try:
        yield
    finally:
        lib.sgcn_tune(b"gemm_mb16_slice_k", old)


def operand(x, dev, vec, way, i=0):
    """x on the device with vector loads possible ('on': pitch width or width + 4) or not ('off': a pitch of width + 1, or
    the base one float past an aligned one); None: an odd pitch"""
    w = x.shape[1]
    if vec == "on":
        return Operand(x, dev, w + 4 * (i % 2))
    if vec == "off":
        return Operand(x, dev, w + 1) if way == "pitch" else Operand(x, dev, (w + 1 + 3) // 4 * 4 + 4, shift=1)
    return Operand(x, dev, w + 3)


def inputs(c, kind, tag):
    """(A, B, C_in or None, reference keywords, dropout keys) of a case as host arrays.  kind: 'exact' (bf16-representable
    small integers, mb16_cases.int_range) or 'real' (normal draws)."""
    from oracle import model_np as mnp
    ta, tb = mbc.FORMS[c["form"]]
    M, N, K = c["M"], c["N"], c["K"]
    rng = np.random.RandomState(seed("a16", tag, kind))
    sa, sb = ((K, M) if ta else (M, K)), ((N, K) if tb else (K, N))
    if kind == "exact":
        r = mbc.int_range(K)
        A, B, C_in = sc.ints(rng, sa, -r, r), sc.ints(rng, sb, -r, r), sc.ints(rng, (M, N))
    else:
        A = rng.standard_normal(sa).astype(np.float32)
        B = (rng.standard_normal(sb) / np.sqrt(max(K, 1))).astype(np.float32)
        C_in = rng.standard_normal((M, N)).astype(np.float32)
    kw, keys = {}, {}
    for side, shape in (("a", A.shape), ("c", (M, N))):
        keep = c.get("drop_" + side)
        if keep:
            keys["drop_" + side] = seed("drop_" + side, tag)
            kw["mask_" + side] = mnp.hash_mask(keys["drop_" + side], shape, keep).astype(np.float64)
            kw["scale_" + side] = dc.f32_scale(keep)
    return A, B, (C_in if c.get("accumulate") else None), kw, keys
