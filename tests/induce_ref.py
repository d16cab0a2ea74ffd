"""Plain-loop restatement of ops.csr_induce (sgcn_induce.hip): the induced block A[S, S] of a CSR with sorted, duplicate-free
rows, the rows' value sums, the 'rows' rescaling in fp64, and the stable transpose.  tests/test_full_batch_parts.py holds
these loops to SciPy's A[S][:, S] and .T.tocsr(); the GPU tests hold the kernels to these loops.  Also the small graphs
both test files share."""
import numpy as np
import scipy.sparse as sp

U = 2.0 ** -24        # unit roundoff of fp32


def block(a, ids):
    """(rowptr, col, val) of A[ids][:, ids]: every selected row's entries whose column is selected, in stored order, the
    column relabelled to its position in ``ids``; val keeps the stored fp32 bits."""
    a = a.tocsr()
    pos = {int(v): k for k, v in enumerate(ids)}
    rowptr, col, val = [0], [], []
    for v in ids:
        for p in range(a.indptr[v], a.indptr[v + 1]):
            k = pos.get(int(a.indices[p]))
            if k is not None:
                col.append(k)
                val.append(a.data[p])
        rowptr.append(len(col))
    return np.array(rowptr, np.int32), np.array(col, np.int32), np.array(val, np.float32)


def row_sums(a, ids):
    """(full, kept) in fp64 and the full rows' lengths: the sums of every selected row's values over all its entries and over
    the kept ones."""
    a = a.tocsr()
    chosen = set(int(v) for v in ids)
    full, kept, length = [], [], []
    for v in ids:
        f = k = 0.0
        for p in range(a.indptr[v], a.indptr[v + 1]):
            f += float(a.data[p])
            if int(a.indices[p]) in chosen:
                k += float(a.data[p])
        full.append(f)
        kept.append(k)
        length.append(int(a.indptr[v + 1] - a.indptr[v]))
    return np.array(full), np.array(kept), np.array(length, np.int64)


def block_rows_f64(a, ids):
    """The block's values under norm='rows' in fp64: row i times full_i / kept_i (1 where kept_i == 0)."""
    rowptr, _, val = block(a, ids)
    full, kept, _ = row_sums(a, ids)
    scale = np.where(kept == 0, 1.0, full / np.where(kept == 0, 1.0, kept))
    return val.astype(np.float64) * np.repeat(scale, np.diff(rowptr))


def transpose(n, rowptr, col):
    """(t_rowptr, t_col, t_src) of the stable transpose of an n x n CSR: the entries of every column in ascending row order
    (the order they are met in), t_src the position each came from."""
    buckets = [[] for _ in range(n)]
    for i in range(n):
        for p in range(rowptr[i], rowptr[i + 1]):
            buckets[col[p]].append((i, p))
    t_rowptr, t_col, t_src = [0], [], []
    for b in buckets:
        t_col.extend(i for i, _ in b)
        t_src.extend(p for _, p in b)
        t_rowptr.append(len(t_col))
    return np.array(t_rowptr, np.int32), np.array(t_col, np.int32), np.array(t_src, np.int64)


# ---- graphs ---------------------------------------------------------------------------------------------------------------
def _sym(n, rows, cols):
    a = sp.coo_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n, n)).tocsr()
    a = (a + a.T).tocsr()
    a.sum_duplicates()
    a.data[:] = 1.0
    a.sort_indices()
    return a.astype(np.float32)


def sbm_graph(n=320, comms=5, p_in=0.12, p_out=0.004, seed=0):
    """an undirected graph of ``comms`` planted communities of contiguous vertices"""
    rng = np.random.RandomState(seed)
    lab = np.arange(n) * comms // n
    p = np.where(lab[:, None] == lab[None, :], p_in, p_out)
    r, c = np.nonzero(np.triu(rng.rand(n, n) < p, 1))
    return _sym(n, r, c)


def flat_graph(n=300, deg=4, seed=1):
    """an undirected graph without communities: ``deg`` uniform random neighbours per vertex"""
    rng = np.random.RandomState(seed)
    r = np.repeat(np.arange(n), deg)
    c = rng.randint(0, n, n * deg)
    keep = r != c
    return _sym(n, r[keep], c[keep])


def positive(a, seed=0):
    """``a`` with strictly positive fp32 values in [0.25, 1.75) (the pattern and the stored order kept)"""
    a = a.copy().astype(np.float32)
    a.data[:] = (0.25 + 1.5 * np.random.RandomState(seed).rand(a.nnz)).astype(np.float32)
    return a


def signed(a, seed=0):
    """``a`` with arbitrary-looking fp32 values of both signs: what a bit-for-bit comparison should see"""
    a = a.copy().astype(np.float32)
    a.data[:] = np.random.RandomState(seed).randn(a.nnz).astype(np.float32)
    return a
