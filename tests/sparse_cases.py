"""Sparse test cases: sparsity patterns, exact (dyadic) operands and a per-element fp64 error bound (test-only helper).

Patterns.  ``CATALOGUE`` maps a name to a seeded builder that returns a scipy CSR (float32, sorted columns unless the
entry says otherwise).  The values a builder puts in are placeholders: a test gives the pattern its values with
``dyadic`` (exact inputs) or ``normalised`` (D^-1 A, the model's aggregation).

Exact inputs.  Take A's values from +-2^k, k in [-2, 2], every scale (row / column scales, the aggregator's s, beta)
from powers of two, and the dense operands (B, H, h, mu, C_in, the addend) from small integers.  Every product is then
exact, and so is every quotient a planner forms when it moves a power-of-two factor between a row part and a column
part.  Every term of an output element is a multiple of 2^lo, lo being the sum of the lowest set-bit exponents of its
factors (``low_exp``).  A partial sum of such terms is a multiple of 2^lo no larger than the sum of the terms'
magnitudes; if that magnitude stays below 2^(24 + lo), the partial sum is an fp32 number and the addition forming it was
exact -- whatever the summation order, split or tree.  A power-of-two factor moved out of a sum (rscale, a row value
folded into row_fold) scales the magnitude and the grid alike, so the condition is checked once before such a factor
(``inner``) and once after (``total``).  ``assert_exact`` checks it, in fp64, on every element a test compares; a case
that cannot be exact fails loudly instead of passing by luck.  Under it every correct kernel equals the fp64 product
bit for bit, on every row.

Real-valued inputs: see ``fp64_bound``.
"""
import numpy as np
import scipy.sparse as sp

T_SPLIT = 64          # the explicit split threshold of the row-length patterns (plan_T / ColumnSweepCSR T)
WAVES_PER_WG = 4      # waves per workgroup of the fix-up kernels (kBlock / kWave): more pieces take cs_fix_kernel's 2nd path
U = 2.0 ** -24        # unit roundoff of fp32


# ---- patterns ---------------------------------------------------------------------------------------------------------
def _csr(M, K, rows, cols):
    rows = np.asarray(rows, np.int64)
    cols = np.asarray(cols, np.int64)
    a = sp.coo_matrix((np.ones(rows.shape[0], np.float32), (rows, cols)), shape=(M, K)).tocsr()
    a.sum_duplicates()
    a.data[:] = 1.0
    a.sort_indices()
    return a


def _uniform(M, K, per_row, rng):
    """about ``per_row`` distinct random columns in every row"""
    n = int(M * per_row)
    return _csr(M, K, rng.randint(0, M, n), rng.randint(0, K, n)) if M and K else sp.csr_matrix((M, K), dtype=np.float32)


def _stack(*blocks):
    a = sp.vstack(blocks).tocsr().astype(np.float32)
    a.sort_indices()
    return a


def _rows_of_length(K, lengths, rng, filler=3, spacing=5):
    """rows of the given lengths (distinct random columns), each followed by ``spacing`` rows of ~``filler`` nonzeros"""
    rows, cols, r = [], [], 0
    for n in lengths:
        rows.append(np.full(n, r)); cols.append(rng.choice(K, n, replace=False)); r += 1
        for _ in range(spacing):
            k = rng.randint(0, filler + 1)
            rows.append(np.full(k, r)); cols.append(rng.choice(K, k, replace=False)); r += 1
    return _csr(r, K, np.concatenate(rows), np.concatenate(cols))


def p_empty(rng):
    return sp.csr_matrix((50, 70), dtype=np.float32)


def p_one_row(rng):
    """all rows empty but one (a split row: 300 > T_SPLIT)"""
    return _csr(40, 700, np.full(300, 17), rng.choice(700, 300, replace=False))


def p_identity(rng):
    return sp.identity(300, dtype=np.float32, format="csr")


def p_permutation(rng):
    return _csr(257, 257, np.arange(257), rng.permutation(257))


def p_star_row(rng):
    """one row holding all of K = 100,000 columns, among rows of ~3 nonzeros"""
    M, K = 200, 100000
    b = _uniform(M, K, 3, rng)
    star = _csr(1, K, np.zeros(K), np.arange(K))
    return _stack(b[:5], star, b[6:])


def p_star_col(rng):
    """one column present in every row (the warp table's extreme: most of the work at one column id)"""
    M, K = 3000, 500
    a = _uniform(M, K, 2, rng)
    return (a + _csr(M, K, np.arange(M), np.full(M, 7))).tocsr().astype(np.float32)


def p_hot_block(rng):
    """a block of 64 hot columns (every row takes ~30 % of them) among uniform ones"""
    M, K = 2000, 5000
    hot = rng.rand(M, 64) < 0.3
    r, c = np.nonzero(hot)
    return (_uniform(M, K, 4, rng) + _csr(M, K, r, c + 100)).tocsr().astype(np.float32)


def p_row_lengths(rng):
    """rows of length T-1, T, T+1, 2T and WAVES_PER_WG*T + 1 (more pieces than a workgroup has waves)"""
    T = T_SPLIT
    return _rows_of_length(1000, [T - 1, T, T + 1, 2 * T, WAVES_PER_WG * T + 1, 9 * T + 3, T, T + 1], rng)


def _shape(M, K, per_row=3):
    return lambda rng: _uniform(M, K, min(per_row, K), rng)


def p_row_vector(rng):
    """1 x K"""
    return _csr(1, 5000, np.zeros(3000), rng.choice(5000, 3000, replace=False))


def p_col_vector(rng):
    """M x 1"""
    keep = np.nonzero(rng.rand(5000) < 0.7)[0]
    return _csr(5000, 1, keep, np.zeros(keep.shape[0]))


def p_rmat(rng):
    """R-MAT at 2^17 vertices, 2^20 edges (skewed rows AND columns: power-law degree on both sides)"""
    from stochastic_gcn_amd import synthetic
    a = synthetic.rmat_like(1 << 17, 1 << 20, seed=int(rng.randint(1 << 30)))
    a.data[:] = 1.0
    return a.astype(np.float32)


def sbm_labels(n=20000, comm_size=700):
    return (np.arange(n) // comm_size).astype(np.int32)


def p_sbm(rng):
    """planted communities of 700 contiguous vertices (p_in 0.9), Zipf sources"""
    from stochastic_gcn_amd import synthetic
    return synthetic.sbm_zipf_edges(20000, 150000, 0.6, sbm_labels(), 0.9, rng).astype(np.float32)


def p_range_boundary(rng):
    """column-range plans: K = 8192 (one warp bucket per column, so a 2-range cut lands on the median column), nonzeros
    symmetric about K/2, and every row holds columns K/2 - 1, K/2 and K/2 + 1: both sides of the cut carry nonzeros"""
    M, K = 700, 8192
    a = _uniform(M, K // 2, 3, rng)
    r, c = a.nonzero()
    rows = np.concatenate([r, r, np.repeat(np.arange(M), 3)])
    cols = np.concatenate([c, K - 1 - c, np.tile([K // 2 - 1, K // 2, K // 2 + 1], M)])
    return _csr(M, K, rows, cols)


def p_range_empty(rng):
    """column-range plans with a range that holds no nonzero: every nonzero in column 10 or column 5000 (halves of the
    nonzeros), so the cuts of 3 or 4 ranges coincide and a range is empty"""
    M, K = 600, 6000
    r1 = np.nonzero(rng.rand(M) < 0.5)[0]
    r2 = rng.permutation(M)[:r1.shape[0]]
    return _csr(M, K, np.concatenate([r1, r2]), np.concatenate([np.full(r1.shape[0], 10), np.full(r2.shape[0], 5000)]))


def scheduler_batch(seed=3, n=3000, batch=200, degree=2):
    """(adj, fadj, fd) of one minibatch of the product's own sampler: adj / fadj as CSR in the order it stores them"""
    from stochastic_gcn_amd import synthetic
    from stochastic_gcn_amd.scheduler import PyScheduler
    from oracle import oracle_np as onp
    _, train_adj, _, _, _, _, labels, tr, _, _ = synthetic.reddit_like(
        n=n, m=30000, f=4, classes=3, splits=(2000, 300, 700), seed=seed, with_features=False)
    ph = {'adj': ['adj_0'], 'madj': ['madj_0'], 'fadj': ['fadj_0'], 'fields': ['f0', 'f1'],
          'ffields': ['ff0'], 'scales': ['s0'], 'labels': 'labels'}
    sch = PyScheduler(train_adj, labels, 1, [degree], ph, seed, data=tr.copy(), cv=True)
    fd = sch.minibatch(batch)
    return onp.coo_to_csr(fd['adj_0']), onp.coo_to_csr(fd['fadj_0']), fd


def p_sched_adj(rng):
    return scheduler_batch()[0]


def p_sched_fadj(rng):
    return scheduler_batch()[1]


CATALOGUE = {
    "empty": p_empty, "one_row": p_one_row, "identity": p_identity, "permutation": p_permutation,
    "star_row": p_star_row, "star_col": p_star_col, "hot_block": p_hot_block, "row_lengths": p_row_lengths,
    "m15_k17": _shape(15, 17), "m16_k16": _shape(16, 16), "m17_k15": _shape(17, 15),
    "m63_k65": _shape(63, 65), "m64_k64": _shape(64, 64), "m65_k63": _shape(65, 63),
    "m4095_k4097": _shape(4095, 4097, 6), "m4096_k4096": _shape(4096, 4096, 6), "m4097_k4095": _shape(4097, 4095, 6),
    "k5": _shape(300, 5), "row_vector": p_row_vector, "col_vector": p_col_vector,
    "rmat": p_rmat, "sbm": p_sbm, "range_boundary": p_range_boundary, "range_empty": p_range_empty,
    "sched_adj": p_sched_adj, "sched_fadj": p_sched_fadj,
}


def pattern(name, seed=0):
    return CATALOGUE[name](np.random.RandomState(seed))


# ---- values -----------------------------------------------------------------------------------------------------------
def dyadic(a, rng, kmin=-2, kmax=2):
    """``a`` with values +-2^k, k in [kmin, kmax] (the pattern and the stored order kept)"""
    a = a.copy().astype(np.float32)
    a.data[:] = (rng.choice([-1.0, 1.0], a.nnz) * 2.0 ** rng.randint(kmin, kmax + 1, a.nnz)).astype(np.float32)
    return a


def pow2(rng, n, kmin=-1, kmax=1):
    """n signed powers of two (scales)"""
    return (rng.choice([-1.0, 1.0], n) * 2.0 ** rng.randint(kmin, kmax + 1, n)).astype(np.float32)


def ints(rng, shape, lo=-8, hi=8):
    return rng.randint(lo, hi + 1, shape).astype(np.float32)


def normalised(a):
    """D^-1 A on the pattern (row i's values 1 / deg(i), fp32)"""
    a = a.copy().astype(np.float32)
    deg = np.diff(a.indptr)
    a.data[:] = np.repeat((1.0 / np.maximum(deg, 1)).astype(np.float32), deg)
    return a


# ---- exactness ----------------------------------------------------------------------------------------------------------
def low_exp(*xs):
    """the lowest set-bit exponent over the nonzero entries of the arrays (x = odd * 2^e): every entry is a multiple of
    2^low_exp.  0 when there is no nonzero entry (nothing to constrain)."""
    best = None
    for x in xs:
        if x is None:
            continue
        v = np.abs(np.asarray(x, np.float64)).ravel()
        v = v[v != 0]
        if v.size == 0:
            continue
        m, e = np.frexp(v)                              # v = m 2^e, m in [0.5, 1): m 2^53 is an integer
        n = (m * 2.0 ** 53).astype(np.int64)
        tz = np.log2((n & -n).astype(np.float64)).astype(np.int64)
        lo = int(np.min(e - 53 + tz))
        best = lo if best is None else min(best, lo)
    return 0 if best is None else best


def assert_exact(mag, lo, what="product"):
    """The precondition of an exact comparison: every element's sum of term magnitudes ``mag`` (fp64) is below
    2^(24 + lo), the terms lying on the grid 2^lo."""
    m = float(np.max(mag)) if np.size(mag) else 0.0
    assert m < 2.0 ** (24 + lo), "%s cannot be exact in fp32: magnitude %g on the grid 2^%d" % (what, m, lo)
    return m


def _dense(x):
    return None if x is None else np.asarray(x, np.float64)


def spmm_exact(a, B, gidx=None, rscale=None, cscale=None, beta=0.0, C_in=None, add=None, add_rows=0):
    """The exact value of rscale (.) (A (cscale (.) B[gidx])) + beta C_in (+ add on rows < add_rows), in fp64, after
    asserting the exactness precondition on it (module docstring)."""
    a64 = a.astype(np.float64).tocsr()
    Bg = np.asarray(B, np.float64)[np.asarray(gidx)] if gidx is not None else np.asarray(B, np.float64)[:a.shape[1]]
    cs = _dense(cscale)
    x = Bg * cs[:, None] if cs is not None else Bg
    inner = abs(a64).dot(np.abs(x))
    lo_in = low_exp(a.data) + low_exp(Bg) + low_exp(cscale)
    assert_exact(inner, lo_in, "A B (before rscale)")
    ref = a64.dot(x)
    mag, los = inner, [lo_in]
    if rscale is not None:
        rs = _dense(rscale)[:, None]
        ref, mag = ref * rs, mag * np.abs(rs)
        los = [lo_in + low_exp(rscale)]
    if beta != 0.0:
        ref = ref + beta * np.asarray(C_in, np.float64)
        mag = mag + abs(beta) * np.abs(np.asarray(C_in, np.float64))
        los.append(low_exp(np.float64(beta)) + low_exp(C_in))
    if add is not None and add_rows:
        ref = ref.copy()
        ref[:add_rows] += np.asarray(add, np.float64)[:add_rows]
        mag = mag.copy()
        mag[:add_rows] += np.abs(np.asarray(add, np.float64)[:add_rows])
        los.append(low_exp(np.asarray(add)[:add_rows]))
    assert_exact(mag, min(los), "the fused product")
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    return ref


# ---- the per-element bound for real-valued inputs ----------------------------------------------------------------------
EXTRA_ROUNDINGS = 6


def fp64_bound(a, B, gidx=None, rscale=None, cscale=None, beta=0.0, C_in=None, add=None, add_rows=0, extra=0):
    """|fp32 result - exact| <= bound, element by element, for C = rscale (.) (A (cscale (.) B[gidx])) + beta C_in + add.

    Derivation (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Lemma 3.1 and section 4.2).  Write
    gamma_k = k u / (1 - k u), u = 2^-24.  A sum of n terms formed in ANY order -- sequential, a tree, pieces summed
    apart and the pieces summed in a fix-up -- passes every term through at most n - 1 additions, and a product of k
    rounded operations is within a factor (1 + theta_k), |theta_k| <= gamma_k, of the exact one.  A term of row i of the
    product is a_ij cs_j b_jk: at most two rounded products (a_ij cs_j, then times b; one with an FMA), possibly one more
    when a planner factors a_ij into a row part and a column part (the LDS plan's row_fold / col_fold), then rscale (one
    product), then the epilogue: beta C_in (a product and an addition) and the addend (an addition).  So every term and
    every addend passes through at most n_i + 6 rounding steps (EXTRA_ROUNDINGS = 6 >= 2 + 1 + 1 + 2 + 1 - 1):

        |C_ik - fl(C_ik)| <= gamma_{n_i + 6} (|rs_i| (|A| (|cs| |B|))_ik + |beta| |C_in,ik| + |add_ik|)

    The hardware may flush subnormal results to zero: each of those n_i + 6 operations can then lose a value below
    2^-126, scaled at most by |rs_i| afterwards -- an absolute floor of (n_i + 6) max(1, |rs_i|) 2^-126.  ``extra`` adds
    rounding steps for compositions (the aggregator's differences and sums of two products)."""
    a64 = a.astype(np.float64).tocsr()
    Bg = np.asarray(B, np.float64)[np.asarray(gidx)] if gidx is not None else np.asarray(B, np.float64)[:a.shape[1]]
    x = np.abs(Bg)
    if cscale is not None:
        x = x * np.abs(_dense(cscale))[:, None]
    mag = abs(a64).dot(x)
    rs = np.ones((a.shape[0], 1)) if rscale is None else np.abs(_dense(rscale))[:, None]
    mag = mag * rs
    if beta != 0.0:
        mag = mag + abs(beta) * np.abs(np.asarray(C_in, np.float64))
    if add is not None and add_rows:
        mag = mag.copy()
        mag[:add_rows] += np.abs(np.asarray(add, np.float64)[:add_rows])
    n = (np.diff(a.indptr).astype(np.float64) + EXTRA_ROUNDINGS + extra)[:, None]
    gamma = n * U / (1.0 - n * U)
    return gamma * mag + n * np.maximum(1.0, rs) * 2.0 ** -126


def spmm_f64(a, B, gidx=None, rscale=None, cscale=None, beta=0.0, C_in=None, add=None, add_rows=0):
    """The fp64 value of the fused product (no exactness asserted: for real-valued inputs, against ``fp64_bound``)."""
    a64 = a.astype(np.float64).tocsr()
    Bg = np.asarray(B, np.float64)[np.asarray(gidx)] if gidx is not None else np.asarray(B, np.float64)[:a.shape[1]]
    if cscale is not None:
        Bg = Bg * _dense(cscale)[:, None]
    ref = a64.dot(Bg)
    if rscale is not None:
        ref = ref * _dense(rscale)[:, None]
    if beta != 0.0:
        ref = ref + beta * np.asarray(C_in, np.float64)
    if add is not None and add_rows:
        ref[:add_rows] += np.asarray(add, np.float64)[:add_rows]
    return ref


# ---- the control-variate aggregator (oracle/oracle_np.py vr_aggregate, restated in fp64) --------------------------------
def vr_aggregate_f64(adj, fadj, h, mu, Hbar, ifield, ffield, s, cvd, concat_self):
    """(out_h, out_mu, mag_h, mag_mu, nterms): the fp64 outputs, the per-element sums of term magnitudes (for the
    exactness precondition and the bound) and the number of product terms of each output row."""
    A, P = adj.astype(np.float64).tocsr(), fadj.astype(np.float64).tocsr()
    absA, absP = abs(A), abs(P)
    n1 = adj.shape[0]
    H = np.asarray(Hbar, np.float64)
    Hi, Hf = H[np.asarray(ifield)], H[np.asarray(ffield)]
    nterms = (np.diff(adj.indptr) + np.diff(fadj.indptr)).astype(np.float64)
    x = np.asarray(h, np.float64)
    mean, mean_m = P.dot(Hf), absP.dot(np.abs(Hf))
    if cvd:
        m = np.asarray(mu, np.float64)
        sc = np.asarray(s, np.float64)[:, None]
        mu_nbr = A.dot(m - Hi) + mean
        mu_m = absA.dot(np.abs(m) + np.abs(Hi)) + mean_m
        h_nbr = A.dot(x - m) * sc + mu_nbr
        h_m = absA.dot(np.abs(x) + np.abs(m)) * np.abs(sc) + mu_m
        if concat_self:
            return (np.concatenate([x[:n1], h_nbr], 1), np.concatenate([m[:n1], mu_nbr], 1),
                    np.concatenate([np.abs(x[:n1]), h_m], 1), np.concatenate([np.abs(m[:n1]), mu_m], 1), nterms)
        return h_nbr, mu_nbr, h_m, mu_m, nterms
    a_nbr = A.dot(x) - A.dot(Hi) + mean
    a_m = absA.dot(np.abs(x) + np.abs(Hi)) + mean_m
    if concat_self:
        return np.concatenate([x[:n1], a_nbr], 1), None, np.concatenate([np.abs(x[:n1]), a_m], 1), None, nterms
    return a_nbr, None, a_m, None, nterms


def vr_bound(mag, nterms, concat_self, extra=8):
    """fp64_bound's argument for the aggregator: every term of an output row passes through at most (the row's terms in
    A and P) + ``extra`` rounding steps (the differences h - mu and mu - Hbar[ifield], the scale s, the sum of the two
    products, and the products themselves); the copied self half of a concatenated output is exact."""
    n = (nterms + extra)[:, None]
    g = n * U / (1.0 - n * U)
    b = g * mag + n * 2.0 ** -126
    if concat_self:
        d = mag.shape[1] // 2
        b[:, :d] = 0.0
    return b


# ---- randomised cases (formerly run by hand as profiles/cs_fuzz.py and profiles/lds_fuzz.py) --------------------------
# Less than those scripts were run for: the suite runs 24 seeds of each generator (the hand runs were 450 + 360 cases), on
# exact inputs only, and a density draw is thinned to MAX_FUZZ_NNZ nonzeros (the scripts' densest draws reached ~18 M)
# so that the CPU reference stays cheap.  The shapes, plan options and fusions they draw are the scripts' own.
MAX_FUZZ_NNZ = 400000


def _fuzz_matrix(rng, M, K, dens):
    dens = min(dens, MAX_FUZZ_NNZ / max(M * K, 1))
    a = sp.random(M, K, density=dens, format='csr', random_state=rng, dtype=np.float32)
    a.data[:] = 1.0
    return a


def cs_fuzz_case(seed):
    """One randomised column-sweep case: shapes around the bin / tile boundaries, skewed columns, split rows, one / two /
    four lane groups or a column-range plan, gathered operand rows, row / column scales, beta, pitch padding, a pace."""
    rng = np.random.RandomState(seed)
    M = int(rng.choice([1, 15, 16, 17, 63, 64, 65, 700, 4097, 9000]))
    K = int(rng.choice([1, 5, 130, 1000, 5000]))
    a = _fuzz_matrix(rng, M, K, float(rng.choice([0.002, 0.02, 0.1, 0.4])))
    if rng.rand() < 0.4 and a.nnz:            # skewed columns (the clock in work coordinates: a warp table by itself)
        coo = a.tocoo()
        a = _csr(M, K, coo.row, (coo.col.astype(np.int64) ** 2 // max(K, 1)))
    a.sort_indices()
    a = dyadic(a, rng)
    G = int(rng.choice([1, 2, 4]))
    c = dict(a=a, G=G, warp=[True, False, 'auto'][int(rng.randint(3))],
             d=int(rng.choice([4, 30, 64, 66, 128, 130, 320, 602])), pad=int(rng.choice([0, 4])),
             T=int(rng.choice([0, 8, 64])), align=int(rng.choice([0, 64, 2048])) if rng.rand() < 0.7 else 'auto',
             gather=rng.rand() < 0.4, rscale=rng.rand() < 0.5, cscale=rng.rand() < 0.5, beta=float(rng.choice([0.0, 0.5, 1.0])),
             ranges=int(rng.choice([2, 2, 3, 4])) if G == 1 and rng.rand() < 0.5 else 0, pace=int(rng.choice([-1, 100, 300])))
    c["rng"] = rng
    return c


def lds_fuzz_case(seed):
    """One randomised LDS-sweep case: shapes around the tile / wave / ring boundaries, row-constant, column-constant,
    arbitrary and all-ones values, labels, min_reuse, split rows, both rings, row scale, beta, pitch padding."""
    rng = np.random.RandomState(seed)
    M = int(rng.choice([1, 7, 95, 96, 97, 700, 769, 1500, 3000]))
    K = int(rng.choice([1, 5, 130, 129, 1000, 2500]))
    a = _fuzz_matrix(rng, M, K, float(rng.choice([0.002, 0.02, 0.1, 0.4])))
    kind = str(rng.choice(["row", "col", "gen", "ones"]))
    a = dyadic(a, rng)
    if kind == "row":
        a = sp.diags(pow2(rng, M, -2, 2)).dot((a != 0).astype(np.float32)).tocsr().astype(np.float32)
    elif kind == "col":
        a = (a != 0).astype(np.float32).dot(sp.diags(pow2(rng, K, -2, 2))).tocsr().astype(np.float32)
    elif kind == "ones":
        a.data[:] = 1.0
    a.sort_indices()
    c = dict(a=a, kind=kind, d=int(rng.choice([2, 30, 128, 130, 256, 602])), pad=int(rng.choice([0, 4, 8])),
             labels=None if rng.rand() < 0.4 else (rng.randint(0, 4, M).astype(np.int32), rng.randint(0, 4, K).astype(np.int32)),
             min_reuse=int(rng.choice([1, 2, 3])), T=int(rng.choice([0, 8, 64])), ring=int(rng.choice([0, 80])),
             rscale=rng.rand() < 0.5, beta=float(rng.choice([0.0, 0.5, 1.0])), general=bool(kind == "gen" and rng.rand() < 0.5))
    c["rng"] = rng
    return c
