"""CPU checks of the sparse test helpers (tests/sparse_cases.py): every pattern builds and its exact product is exact,
and the per-element fp64 bound accepts correct fp32 sums in any order while rejecting a dropped term or a bf16 operand."""
import numpy as np
import pytest
import scipy.sparse as sp

import sparse_cases as sc


@pytest.mark.parametrize("name", sorted(sc.CATALOGUE))
def test_catalogue_pattern_builds_and_its_dyadic_product_is_exact(name):
    a = sc.pattern(name)
    assert sp.isspmatrix_csr(a) and a.dtype == np.float32
    assert np.all(np.diff(a.indptr) >= 0) and (a.nnz == 0 or a.indices.max() < a.shape[1])
    rng = np.random.RandomState(1)
    ad = sc.dyadic(a, rng)
    assert np.array_equal(ad.indptr, a.indptr) and np.array_equal(ad.indices, a.indices)
    d = 3
    B = sc.ints(rng, (a.shape[1], d))
    ref = sc.spmm_exact(ad, B)                     # asserts the precondition
    got32 = ad.dot(B)                              # SciPy's fp32 loop, its own order
    assert got32.dtype == np.float32
    np.testing.assert_array_equal(np.asarray(got32, np.float64), ref)
    # ... and with every fusion on (powers of two for the scales and beta, integers for C_in and the addend)
    rs, cs = sc.pow2(rng, a.shape[0]), sc.pow2(rng, a.shape[1])
    C = sc.ints(rng, (a.shape[0], d))
    ref2 = sc.spmm_exact(ad, B, rscale=rs, cscale=cs, beta=0.5, C_in=C, add=C, add_rows=a.shape[0] // 2)
    want = rs[:, None] * np.asarray(ad.dot(B * cs[:, None]), np.float32) + np.float32(0.5) * C
    want[:a.shape[0] // 2] += C[:a.shape[0] // 2]
    np.testing.assert_array_equal(want.astype(np.float64), ref2)


def test_catalogue_covers_the_edges_it_names():
    T = sc.T_SPLIT
    deg = np.diff(sc.pattern("row_lengths").indptr)
    for n in (T - 1, T, T + 1, 2 * T, sc.WAVES_PER_WG * T + 1):
        assert n in deg
    star = sc.pattern("star_row")
    assert star.shape[1] >= 100000 and np.diff(star.indptr).max() == star.shape[1]
    sc_ = sc.pattern("star_col")
    assert np.bincount(sc_.indices).max() == sc_.shape[0]
    assert sc.pattern("row_vector").shape[0] == 1 and sc.pattern("col_vector").shape[1] == 1
    assert sc.pattern("k5").shape[1] < 16
    one = sc.pattern("one_row")
    assert np.count_nonzero(np.diff(one.indptr)) == 1
    rm = sc.pattern("rmat")
    assert rm.shape[0] == 1 << 17
    for deg in (np.diff(rm.indptr), np.bincount(rm.indices, minlength=rm.shape[1])):      # power law on both sides
        assert deg.max() > 50 * max(deg.mean(), 1)


def test_exactness_precondition_fails_loudly():
    a = sp.csr_matrix(np.ones((1, 40), np.float32))
    with pytest.raises(AssertionError):
        sc.spmm_exact(sc.dyadic(a, np.random.RandomState(0), 2, 2), np.full((40, 2), 2.0 ** 22 + 1, np.float32))
    with pytest.raises(AssertionError):           # a value off the grid of the rest: 1 + 2^-30 is not an fp32 sum
        sc.assert_exact(np.array([1.0]), -30)
    assert sc.low_exp(np.array([0.75, 8.0, 0.0])) == -2 and sc.low_exp(np.array([0.0])) == 0
    assert sc.low_exp(np.float32(2.0 ** -130)) == -130


def _real_case(seed, degrees, d=64):
    rng = np.random.RandomState(seed)
    K = 5000
    rows = np.concatenate([np.full(n, i) for i, n in enumerate(degrees)])
    cols = np.concatenate([rng.choice(K, n, replace=False) for n in degrees])
    a = sc.normalised(sc._csr(len(degrees), K, rows, cols))
    B = rng.standard_normal((K, d)).astype(np.float32)
    return a, B, rng


def _sum_f32(terms, order):
    """fp32 sum of a row's terms (n x d) in one of several orders"""
    if order == "forward":
        acc = np.zeros(terms.shape[1], np.float32)
        for t in terms:
            acc = acc + t
        return acc
    if order == "reverse":
        return _sum_f32(terms[::-1], "forward")
    if order == "pairwise":
        x = terms
        while x.shape[0] > 1:
            h = x.shape[0] // 2
            y = x[:h] + x[h:2 * h]
            x = np.concatenate([y, x[2 * h:]]) if x.shape[0] % 2 else y
        return x[0] if x.shape[0] else np.zeros(terms.shape[1], np.float32)
    if order == "pieces":                          # split into pieces of 7, each summed, then an ordered fix-up
        parts = [_sum_f32(terms[i:i + 7], "forward") for i in range(0, terms.shape[0], 7)]
        return _sum_f32(np.array(parts, np.float32).reshape(-1, terms.shape[1]), "forward")
    perm = np.random.RandomState(len(terms)).permutation(terms.shape[0])
    return _sum_f32(terms[perm], "forward")


def _fp32_product(a, B, order, drop=None, Bq=None):
    Bq = B if Bq is None else Bq
    out = np.zeros((a.shape[0], B.shape[1]), np.float32)
    for i in range(a.shape[0]):
        lo, hi = a.indptr[i], a.indptr[i + 1]
        idx = [j for j in range(lo, hi) if j != drop]
        terms = (a.data[idx][:, None] * Bq[a.indices[idx]]).astype(np.float32)
        out[i] = _sum_f32(terms, order)
    return out


@pytest.mark.parametrize("order", ["forward", "reverse", "pairwise", "pieces", "shuffled"])
def test_fp64_bound_accepts_fp32_sums_in_any_order(order):
    a, B, rng = _real_case(0, [1, 2, 7, 64, 65, 300, 1000, 4096])
    rs, cs = rng.rand(a.shape[0]).astype(np.float32) + 0.5, rng.rand(B.shape[0]).astype(np.float32) + 0.5
    C = rng.standard_normal((a.shape[0], B.shape[1])).astype(np.float32)
    ref = sc.spmm_f64(a, B)
    got = _fp32_product(a, B, order)
    assert np.all(np.abs(got - ref) <= sc.fp64_bound(a, B))
    # with the fusions: rs (.) (A (cs (.) B)) + beta C + add, each step rounded in fp32
    ac = a.copy()
    ac.data[:] = (ac.data * cs[ac.indices]).astype(np.float32)
    got2 = (rs[:, None] * _fp32_product(ac, B, order)).astype(np.float32)
    got2 = (got2 + (np.float32(0.3) * C).astype(np.float32)).astype(np.float32)
    got2[:4] = (got2[:4] + C[:4]).astype(np.float32)
    kw = dict(rscale=rs, cscale=cs, beta=0.3, C_in=C, add=C, add_rows=4)
    assert np.all(np.abs(got2 - sc.spmm_f64(a, B, **kw)) <= sc.fp64_bound(a, B, **kw))


@pytest.mark.parametrize("deg", [1, 2, 7, 64, 513, 4096])
def test_fp64_bound_rejects_one_dropped_term(deg):
    a, B, rng = _real_case(deg, [deg, 5])
    bound = sc.fp64_bound(a, B)
    ref = sc.spmm_f64(a, B)
    for drop in rng.choice(deg, min(deg, 5), replace=False):
        got = _fp32_product(a, B, "forward", drop=int(drop))
        assert np.any(np.abs(got[0] - ref[0]) > bound[0]), "dropping term %d of a row of %d passed" % (drop, deg)
        assert np.all(np.abs(got[1] - ref[1]) <= bound[1])


def test_fp64_bound_rejects_a_bf16_operand():
    import torch
    a, B, _ = _real_case(5, [1, 3, 16, 100, 700, 4096])
    Bq = torch.from_numpy(B).to(torch.bfloat16).to(torch.float32).numpy()
    got = _fp32_product(a, B, "forward", Bq=Bq)
    exceeded = np.abs(got - sc.spmm_f64(a, B)) > sc.fp64_bound(a, B)
    assert exceeded.any(axis=1)[:4].all()          # every row of up to 100 terms shows it


def test_vr_aggregate_reference_restates_the_oracle():
    """vr_aggregate_f64 on dyadic inputs equals the fp32 oracle (exact: both are exact), cvd and plain, concatenated or not"""
    from oracle import oracle_np as onp
    adj, fadj, fd = sc.scheduler_batch()
    rng = np.random.RandomState(0)
    adj, fadj = sc.dyadic(adj, rng), sc.dyadic(fadj, rng)
    n0, n = fd['f0'].shape[0], 3000
    h, mu, H = sc.ints(rng, (n0, 6)), sc.ints(rng, (n0, 6)), sc.ints(rng, (n, 6))
    s = sc.pow2(rng, adj.shape[0])
    for cvd in (True, False):
        for concat in (True, False):
            oh, om, mh, mm, nt = sc.vr_aggregate_f64(adj, fadj, h, mu, H, fd['f0'], fd['ff0'], s, cvd, concat)
            sc.assert_exact(mh, sc.low_exp(adj.data, fadj.data) + min(sc.low_exp(s), 0))
            rh, rm, _ = onp.vr_aggregate(adj, fadj, h, mu, H, fd['f0'], fd['ff0'], s, cvd, concat)
            np.testing.assert_array_equal(rh.astype(np.float64), oh)
            if cvd:
                np.testing.assert_array_equal(rm.astype(np.float64), om)


@pytest.mark.parametrize("seed", range(6))
def test_fuzz_case_generators_are_seeded_and_exact(seed):
    for gen in (sc.cs_fuzz_case, sc.lds_fuzz_case):
        c1, c2 = gen(seed), gen(seed)
        a = c1["a"]
        assert (a != c2["a"]).nnz == 0 and c1["d"] == c2["d"]
        assert a.nnz <= sc.MAX_FUZZ_NNZ * 1.1
        B = sc.ints(np.random.RandomState(seed), (a.shape[1], 4))
        np.testing.assert_array_equal(np.asarray(a.dot(B), np.float64), sc.spmm_exact(a, B))
