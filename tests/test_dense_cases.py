"""CPU checks of the dense test helpers (tests/dense_cases.py): the restated launch plan agrees with the library's
workspace sizes for every knob value the suite uses, the catalogues reach every reachable plan cell, the exactness
precondition holds where the GPU tests rely on it, and the error bounds accept fp32 results while rejecting real
defects."""
import numpy as np
import pytest

import dense_cases as dc
import sparse_cases as sc

SHAPES = [(M, N, K) for M in (1, 5, 31, 32, 33, 97, 128, 300, 2042, 4097, 9000) for N in (1, 3, 41, 64, 128, 129, 256, 1204)
          for K in (0, 1, 33, 95, 96, 191, 192, 300, 1021, 1204, 4000)]


def test_ws_floats_and_effective_slices_match_the_library():
    """S_split M N == sgcn_gemm_ws_floats(M, N, K) on a grid of shapes for every gemm_min_steps the suite sets, and the
    effective number of slices never exceeds S_split (so the workspace a caller sizes from the library is enough)."""
    from stochastic_gcn_amd._ffi import lib
    old = int(lib.sgcn_tune_get(b"gemm_min_steps"))
    try:
        for knob in dc.KNOBS:
            assert lib.sgcn_tune(b"gemm_min_steps", knob) == 0
            for M, N, K in SHAPES:
                want = int(lib.sgcn_gemm_ws_floats(M, N, K))
                assert dc.ws_floats(M, N, K, knob) == want, (M, N, K, knob)
                p = dc.gemm_plan(M, N, K, ws=True, min_steps=knob)
                if K > 0:
                    assert want == (p["S_split"] * M * N if p["S_split"] > 1 else 0)
                assert p["S"] <= p["S_split"] and (p["S"] - 1) * p["kchunk"] < max(K, 1) <= p["S"] * p["kchunk"]
    finally:
        lib.sgcn_tune(b"gemm_min_steps", old)
    assert int(lib.sgcn_tune_get(b"gemm_min_steps")) == old


def test_default_knobs_never_select_four_k_groups_through_ops_gemm_or_narrow_dense_fwd():
    """The finding the K-groups = 4 cases exist for: with default knobs, ops.gemm (no output mask) and ops.dense_fwd with
    N <= 128 never launch KG = 4 -- small grids are cut over K first.  The plan depends on M and N only through their
    tile counts, so this scan over M <= 9,000 (282 row tiles), N <= 1,204 (10 column tiles) and every K <= 4,000 is
    complete.  If the rule changes, this fails and the catalogues' knob choices want a look."""
    t_m = np.arange(1, 9000 // dc.kTM + 2)[:, None, None]
    t_n = np.arange(1, 1204 // dc.kTN + 2)[None, :, None]
    K = np.arange(0, 4001)[None, None, :]
    s = np.maximum(np.minimum(256 // (t_m * t_n), K // (dc.DEFAULT_MIN_STEPS * dc.kTK)), 1)
    kchunk = -(-(-(-K // s)) // dc.kTK) * dc.kTK
    S = np.where(K > 0, -(-K // np.maximum(kchunk, 1)), 1)
    steps = -(-np.minimum(np.where(K > 0, kchunk, dc.kTK), K) // dc.kTK)
    kg4 = (t_m * t_n * S <= 128) & (steps >= 8)
    assert not kg4.any()
    # the scan agrees with the restated plan on a sample, and the cells exist through the routes that are not covered
    for M, N, k in [(300, 128, 1204), (64, 40, 300), (9000, 1204, 4000), (32, 128, 4000)]:
        assert dc.ops_gemm_plan(M, N, k)["KG"] != 4 and dc.fwd_plan(M, min(N, 128), k)["KG"] != 4
    assert dc.ops_gemm_plan(100, 256, 300, tb=True, drop_c=True)["KG"] == 4          # an output mask: no workspace
    assert dc.fwd_plan(64, 256, 300)["path"] == "kg4"                                  # N > 128: no workspace
    assert dc.ops_gemm_plan(64, 128, 300, min_steps=dc.NO_SPLIT)["KG"] == 4            # the knob


def test_gemm_catalogue_covers_every_reachable_cell():
    reach = dc.gemm_reachable()
    want = {(ta, tb, kg, s, va, vb) for ta in (False, True) for tb in (False, True) for kg in (1, 2, 4)
            for s in (False, True) for va in (False, True) for vb in (False, True)}
    assert reach == want                                   # all 96 are reachable (K-groups 4 only through a knob)
    have = {dc.gemm_cell(c) for c in dc.GEMM_CASES}
    assert reach <= have, sorted(reach - have)
    # vector loads off through the pitch or the base pointer, not only through odd widths, for both operands
    for side in ("a", "b"):
        ways = {c.get("off_" + side) for c in dc.GEMM_CASES if c.get("vec_" + side) == "off"}
        assert {"pitch", "shift"} <= ways
    flags = [c for c in dc.GEMM_CASES if c.get("drop_a")]
    assert {c["ta"] for c in flags} == {False, True} and any(c.get("drop_c") for c in dc.GEMM_CASES)
    assert {(dc.gemm_cell(c)[2], dc.gemm_cell(c)[3]) for c in dc.GEMM_CASES if c.get("accumulate")} == \
        {(kg, s) for kg in (1, 2, 4) for s in (False, True)}


def test_forward_catalogue_covers_every_reachable_cell():
    reach = dc.fwd_reachable()
    want = {(e, p, n) for e in dc.EPIS for p in dc.FWD_PATHS for n in dc.N_CLASSES}
    assert reach == want
    have = {dc.fwd_cell(c) for c in dc.FWD_CASES}
    assert reach <= have, sorted(reach - have)
    assert any(c["N"] > 128 for c in dc.FWD_CASES)
    assert {c["split"] for c in dc.FWD_CASES if c["split"] is not None} >= {0, 37}
    assert any(c["split"] == c["M"] for c in dc.FWD_CASES) and any(c["M"] < 32 for c in dc.FWD_CASES)
    assert {c["gather"] for c in dc.FWD_CASES} == {"none", "x", "x2", "both"}
    for path in dc.FWD_PATHS:          # every path with the fused epilogue at fewer rows than one tile
        assert any(c["M"] < dc.kTM and dc.fwd_cell(c)[1] == path and c["epi"] != "plain" for c in dc.FWD_CASES), path


def test_backward_catalogue_covers_every_reachable_cell():
    reach = dc.bwd_reachable()
    have = {dc.bwd_cell(c) for c in dc.BWD_CASES}
    assert reach <= have, sorted(reach - have)
    dx = {(c[1], c[2]) for c in reach}
    assert dx == {("mfma", 0), ("row_direct", 1), ("row_direct", 2), ("row_lds", 1), ("row_lds", 2)}
    assert {c[0] for c in reach if c[1] != "mfma"} == {"relu", "ln", "ln_relu"}     # the row pass needs an activation
    for act in dc.ACTS:                 # every activation with the weight gradient split and not, dropout off / 1 / < 1
        assert {(c[3], c[4], c[5]) for c in have if c[0] == act} == \
            {(s, d, g) for s in (False, True) for d in dc.DROPS for g in (False, True)}
    assert {c["N"] for c in dc.BWD_CASES} >= {30, 32, 36, 64, 100, 128}
    assert {c["K"] for c in dc.BWD_CASES} >= {24, 64, 200, 256, 300}
    assert {c["n"] for c in dc.BWD_CASES} >= {1, 3, 5}
    assert max(c["n"] for c in dc.BWD_CASES) >= 3000


def test_exact_operands_stay_exact_on_the_largest_catalogue_shapes():
    """sparse_cases' precondition on integer operands at the catalogues' longest K (with a 1.25 dropout scale)"""
    rng = np.random.RandomState(0)
    for M, N, K in [(5, 3, 4000), (96, 40, 1280), (2000, 130, 1204)]:
        A, B, C = sc.ints(rng, (M, K)), sc.ints(rng, (K, N)), sc.ints(rng, (M, N))
        mask = (rng.rand(M, K) < 0.8).astype(np.float64)
        ref = dc.gemm_exact(A, B, C_in=C, accumulate=True, mask_a=mask, scale_a=dc.f32_scale(0.8))
        got = ((A * mask * np.float32(1.25)).astype(np.float32) @ B + C).astype(np.float64)      # fp32, BLAS order
        np.testing.assert_array_equal(got, ref)
    assert dc.f32_scale(0.8) == 1.25 and dc.f32_scale(0.5) == 2.0
    with pytest.raises(AssertionError):
        dc.gemm_exact(np.full((1, 4), 2.0 ** 12 + 1), np.full((4, 1), 2.0 ** 12 + 1))


def _f32_gemm(a, b, order):
    """an fp32 product summed in slices of 32 K-steps in `order` (any order meets the bound)"""
    K = a.shape[1]
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for s in order(list(range(0, K, 32))):
        acc = (acc + (a[:, s:s + 32] @ b[s:s + 32]).astype(np.float32)).astype(np.float32)
    return acc


@pytest.mark.parametrize("K", [1, 33, 300, 1204])
def test_gemm_bound_holds_for_fp32_and_catches_a_dropped_k_step(K):
    rng = np.random.RandomState(K)
    a = rng.standard_normal((40, K)).astype(np.float32)
    b = rng.standard_normal((K, 24)).astype(np.float32)
    ref, _, _ = dc.gemm_f64(a, b)
    bound = dc.gemm_bound(a, b)
    for order in (lambda s: s, lambda s: s[::-1]):
        got = _f32_gemm(a, b, order).astype(np.float64)
        assert np.all(np.abs(got - ref) <= bound)
    if K > 32:
        dropped = _f32_gemm(a[:, :K - 1 - (K - 1) % 32], b[:K - 1 - (K - 1) % 32], lambda s: s).astype(np.float64)
        assert not np.all(np.abs(dropped - ref) <= bound)
    if 1 < K <= 300:              # an fp16 operand path is caught (at long K the worst-case bound is wider than its error)
        half = a.astype(np.float16).astype(np.float64) @ b.astype(np.float16).astype(np.float64)
        assert not np.all(np.abs(half - ref) <= bound)


def _ln_f32(v, offset, scale, eps):
    """the kernel's LayerNorm arithmetic in fp32 (NumPy order)"""
    v = v.astype(np.float32)
    N = v.shape[1]
    mean = (v.sum(1, dtype=np.float32) / np.float32(N)).astype(np.float32)[:, None]
    t = (v - mean).astype(np.float32)
    q = ((t * t).sum(1, dtype=np.float32) / np.float32(N) + np.float32(eps)).astype(np.float32)
    rs = (np.float32(1) / np.sqrt(q)).astype(np.float32)
    h = (t * rs[:, None]).astype(np.float32)
    return (h * scale + offset).astype(np.float32), h, rs


def test_layernorm_bounds_hold_for_fp32_and_grow_with_the_rows_conditioning():
    rng = np.random.RandomState(5)
    N = 100
    v = rng.standard_normal((6, N))
    v[1] += 3e3                           # |mean| >> std
    v[2] = 7.0                            # variance 0
    v[3] *= 1e-3
    off, scale = rng.standard_normal(N).astype(np.float32), (1 + 0.1 * rng.standard_normal(N)).astype(np.float32)
    v32 = v.astype(np.float32)
    y64, h64, r64 = dc.ln_f64(v32, off, scale, False, 1e-9)
    by, bh, br = dc.ln_fwd_bound(v32, off, scale, 1e-9)
    y, h, rs = _ln_f32(v32, off, scale, 1e-9)
    assert np.all(np.abs(y - y64) <= by) and np.all(np.abs(h - h64) <= bh) and np.all(np.abs(rs - r64) <= br)
    assert bh[1].max() > 100 * bh[0].max()                   # the ill-conditioned row gets a looser bound
    assert not np.all(np.abs(h[::-1] - h64) <= bh)           # rows swapped: caught
    w = v32.copy()
    w[:, 7] += np.float32(1e-3)                              # one input moved by 1e-3 (1e-6 in the small row)
    w[3, 7] -= np.float32(1e-3) - np.float32(1e-6)
    y2, _, _ = _ln_f32(w, off, scale, 1e-9)
    for r in (0, 3, 4, 5):
        assert not np.all(np.abs(y2[r] - y64[r]) <= by[r]), r


def test_layernorm_backward_bound_holds_for_fp32():
    rng = np.random.RandomState(6)
    n, N = 50, 36
    v = rng.standard_normal((n, N))
    off, scale = rng.standard_normal(N).astype(np.float32), (1 + 0.1 * rng.standard_normal(N)).astype(np.float32)
    dy = sc.ints(rng, (n, N)).astype(np.float64)
    y64, h64, r64 = dc.ln_f64(v, off, scale, True, 1e-9)
    gm = dy * (y64 > 0)
    g64, doff, dsc = dc.ln_bwd_f64(v, off, scale, True, 1e-9, dy)
    np.testing.assert_allclose(doff, gm.sum(0), rtol=1e-12, atol=1e-12)
    h, r, s = h64.astype(np.float32), r64.astype(np.float32)[:, None], scale[None, :]
    gs = (gm.astype(np.float32) * s).astype(np.float32)
    m1 = (gs.sum(1, dtype=np.float32) / np.float32(N))[:, None]
    m2 = ((gs * h).sum(1, dtype=np.float32) / np.float32(N))[:, None]
    g = (r * (gs - m1 - h * m2)).astype(np.float32)
    bound = dc.ln_bwd_bound(gm, h64, r64, scale)
    assert np.all(np.abs(g - g64) <= bound)
    assert not np.all(np.abs((r * (gs - h * m2)).astype(np.float32) - g64) <= bound)     # a lost mean term: caught
