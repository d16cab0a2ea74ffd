"""NumPy reference of the element-wise neighbour maximum (ops.spmax / ops.spmax_bwd, include/sgcn.h sgcn_spmax_csr_f32 and
sgcn_spmax_csr_bwd_f32) -- a test-only helper.

Semantics.  For a CSR pattern ``a`` (the stored VALUES are never read) and a dense table B:
    C[i, c]   = max over the stored entries j of row i, in stored order, of B[j, c]
    arg[i, c] = the column id of the FIRST maximum: the best starts as the first entry and a later entry replaces it only
                when v > best.  That is np.argmax's rule -- it keeps the first of +0.0 / -0.0 and of equal values; +-inf
                are ordinary values; an empty row gives +0.0 and -1.  C holds bits of B.
    dB[j, c]  = the sum over the rows i with arg[i, c] == j of G[i, c], added in ascending i in fp32, starting from +0.0;
                then dB[r] += add[r] for r < add_rows (one more fp32 addition).

``forward`` groups the rows by their length and takes np.argmax over each group's gathered block; ``forward_loops`` states
the rule entry by entry in plain Python, and ``forward_dense`` takes np.argmax / np.max over dense columns (sorted rows
only) -- the two brute-force forms the self-check in tests/test_spmax.py holds ``forward`` to on small matrices.
"""
import numpy as np

U = 2.0 ** -24        # unit roundoff of fp32
_CHUNK = 1 << 22      # gathered elements per block of ``forward``


def forward(a, B):
    """(C, arg): float32 (M, d) holding bits of B, int32 (M, d)."""
    a = a.tocsr()
    B = np.asarray(B, np.float32)
    M, d = a.shape[0], B.shape[1]
    indptr, col = a.indptr.astype(np.int64), a.indices.astype(np.int64)
    C = np.zeros((M, d), np.float32)
    arg = np.full((M, d), -1, np.int32)
    deg = np.diff(indptr)
    cidx = np.arange(d)
    for n in np.unique(deg):
        if n == 0:
            continue
        rows = np.nonzero(deg == n)[0]
        step = max(1, _CHUNK // int(n * d))
        for s in range(0, rows.shape[0], step):
            r = rows[s:s + step]
            cols = col[indptr[r][:, None] + np.arange(n)[None, :]]               # (rows, n) in stored order
            blk = B[cols]                                                        # (rows, n, d)
            k = np.argmax(blk, axis=1)                                           # the first maximum; -0.0 == +0.0
            C[r] = blk[np.arange(r.shape[0])[:, None], k, cidx[None, :]]
            arg[r] = cols[np.arange(r.shape[0])[:, None], k].astype(np.int32)
    return C, arg


def forward_loops(a, B):
    """The rule itself, one comparison at a time (small matrices only)."""
    a = a.tocsr()
    B = np.asarray(B, np.float32)
    M, d = a.shape[0], B.shape[1]
    C = np.zeros((M, d), np.float32)
    arg = np.full((M, d), -1, np.int32)
    for i in range(M):
        cols = a.indices[a.indptr[i]:a.indptr[i + 1]]
        for c in range(d):
            for q, j in enumerate(cols):
                v = B[j, c]
                if q == 0 or v > C[i, c]:
                    C[i, c], arg[i, c] = v, j
    return C, arg


def forward_dense(a, B):
    """np.argmax / np.max over whole dense columns: absent entries are taken out by ranking the values (rank 0 = absent),
    so that -inf stays an ordinary value.  Needs rows stored in ascending column order (then the first maximum in stored
    order is the first in column order); small matrices only."""
    a = a.tocsr()
    assert a.has_sorted_indices
    B = np.asarray(B, np.float32)
    M, K = a.shape
    d = B.shape[1]
    mask = np.zeros((M, K), bool)
    mask[np.repeat(np.arange(M), np.diff(a.indptr)), a.indices] = True
    C = np.zeros((M, d), np.float32)
    arg = np.full((M, d), -1, np.int32)
    for c in range(d):
        # ranks 1.. of the column's values in ascending order, equal values (and -0.0 / +0.0) sharing a rank
        _, inv = np.unique(B[:K, c], return_inverse=True)
        rank = np.where(mask, (inv + 1)[None, :], 0)                              # (M, K)
        k = np.argmax(rank, axis=1)
        has = rank[np.arange(M), k] > 0
        assert np.array_equal(np.max(rank, axis=1) > 0, has)
        C[has, c] = B[k[has], c]
        arg[has, c] = k[has]
    return C, arg


def _targets(arg):
    M, d = arg.shape
    valid = arg >= 0
    flat = arg.astype(np.int64) * d + np.arange(d, dtype=np.int64)[None, :]
    return valid, flat


def backward(a, G, arg, add=None, add_rows=0):
    """dB (K, d) float32 by explicit fp32 sequential addition in ascending i (np.add.at on a float32 array adds element by
    element in index order, each sum rounded to fp32), then the addend."""
    K = a.shape[1]
    G = np.asarray(G, np.float32)
    d = G.shape[1]
    dB = np.zeros(K * d, np.float32)
    valid, flat = _targets(np.asarray(arg))
    np.add.at(dB, flat[valid], G[valid])                  # row-major over (i, c): ascending i for every target
    dB = dB.reshape(K, d)
    if add is not None and add_rows:
        dB[:add_rows] = dB[:add_rows] + np.asarray(add, np.float32)[:add_rows, :d]
    return dB


def backward_loops(a, G, arg, add=None, add_rows=0):
    """The same sum, one fp32 addition at a time (small matrices only)."""
    K, G = a.shape[1], np.asarray(G, np.float32)
    M, d = G.shape
    dB = np.zeros((K, d), np.float32)
    for i in range(M):
        for c in range(d):
            if arg[i, c] >= 0:
                dB[arg[i, c], c] = np.float32(dB[arg[i, c], c] + G[i, c])
    if add is not None and add_rows:
        for r in range(add_rows):
            dB[r] = dB[r] + np.asarray(add, np.float32)[r, :d]
    return dB


def backward_f64(a, G, arg, add=None, add_rows=0):
    """(dB in fp64, the per-element bound).  An element with t terms -- the addend counts as one -- is a sum of t fp32
    numbers taken in SOME order (a segment's partial sums, then the slots): every term passes through at most t - 1
    additions of the sum, one more in the slot pass and one for the addend, so
        |fl(dB) - dB| <= (t + 2) 2^-24 sum |terms|
    (the standard bound for a sum in any order, Higham, Accuracy and Stability of Numerical Algorithms, section 4.2)."""
    K = a.shape[1]
    G = np.asarray(G, np.float64)
    d = G.shape[1]
    valid, flat = _targets(np.asarray(arg))
    idx, g = flat[valid], G[valid]
    dB = np.bincount(idx, weights=g, minlength=K * d).astype(np.float64).reshape(K, d)     # (fp64 sums in index order)
    mag = np.bincount(idx, weights=np.abs(g), minlength=K * d).astype(np.float64).reshape(K, d)
    t = np.bincount(idx, minlength=K * d).astype(np.float64).reshape(K, d)
    if add is not None and add_rows:
        ad = np.asarray(add, np.float64)[:add_rows, :d]
        dB[:add_rows] += ad
        mag[:add_rows] += np.abs(ad)
        t[:add_rows] += 1.0
    return dB, (t + 2.0) * U * mag


def same_bits(x, y):
    """float32 arrays equal bit for bit (+0.0 and -0.0 differ)"""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    return x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32))
