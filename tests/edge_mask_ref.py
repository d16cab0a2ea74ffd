"""The edge mask of --edge_dropout restated in NumPy (test-only helper): the contract of include/sgcn.h (SGCN_EDGE_SITE,
sgcn_edge_revalue_f32) written out on the oracle's own hash (oracle.model_np._fmix32 / dropout_key).  Nothing here imports
the product's ops: what the device and the host decode produce is compared against this file.

    pair(i, j) = fmix32(fmix32(u * 0x9E3779B1 + 0x27D4EB2F) + v * 0x85EBCA77),  u = min(i, j), v = max(i, j)   (mod 2^32)
                 stored as 0xFFFFFFFE if it equals 0xFFFFFFFF;  ALWAYS = 0xFFFFFFFF on the diagonal and on pads
    kept       iff pair == ALWAYS or fmix32(pair + key) < thr,  thr from keep as for every dropout site
    out        = base (bits) if pair == ALWAYS;  base * (1.0f / keep) if kept;  +0.0f otherwise
"""
import numpy as np
import scipy.sparse as sp

from oracle import model_np as mnp

EDGE_SITE = 0x45444745
ALWAYS = 0xFFFFFFFF
PAD_BITS = 0x80000000
_M = np.uint64(0xFFFFFFFF)


def edge_key(seed, step):
    return mnp.dropout_key(seed, EDGE_SITE, step)


def pair_keys(row, col, pad=None):
    """uint32 pair key of every (row, col); ``pad``: entries that are plan pads."""
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    u, v = np.minimum(row, col).astype(np.uint64) & _M, np.maximum(row, col).astype(np.uint64) & _M
    inner = mnp._fmix32((u * np.uint64(0x9E3779B1) + np.uint64(0x27D4EB2F)) & _M)
    h = mnp._fmix32((inner + ((v * np.uint64(0x85EBCA77)) & _M)) & _M)
    h = np.where(h == np.uint64(ALWAYS), np.uint64(ALWAYS - 1), h)
    always = row == col
    if pad is not None:
        always = always | np.asarray(pad, bool)
    return np.where(always, np.uint64(ALWAYS), h).astype(np.uint32)


def threshold(keep):
    t = float(np.float32(keep)) * 4294967296.0
    return 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def kept(pair, key, keep):
    """bool per entry: does the mask of ``key`` keep it?"""
    pair = np.asarray(pair, np.uint32).astype(np.uint64)
    h = mnp._fmix32((pair + np.uint64(int(key) & 0xFFFFFFFF)) & _M)
    return (pair == np.uint64(ALWAYS)) | (h < np.uint64(threshold(keep)))


def revalue(base, pair, key, keep):
    """The re-drawn value array, bit for bit (fp32)."""
    base = np.ascontiguousarray(base, np.float32)
    if np.float32(keep) == np.float32(1.0):
        return base.copy()
    pair = np.asarray(pair, np.uint32)
    k = kept(pair, key, keep)
    scale = np.float32(1.0) / np.float32(keep)
    with np.errstate(invalid='ignore', over='ignore'):
        out = np.where(k, base * scale, np.float32(0.0)).astype(np.float32)
    always = pair == np.uint32(ALWAYS)
    out.view(np.uint32)[always] = base.view(np.uint32)[always]
    return out


def coo_of(a):
    """(row, col) of every stored entry of a CSR, in stored order."""
    a = a.tocsr()
    return np.repeat(np.arange(a.shape[0], dtype=np.int64), np.diff(a.indptr)), a.indices.astype(np.int64)


def masked_matrix(a, key, keep):
    """``a`` under the mask of ``key``: the SAME pattern and stored order, dropped entries kept as explicit +0.0f (so that
    every plan built from it has the layout of the plan of ``a``)."""
    a = a.tocsr()
    row, col = coo_of(a)
    data = revalue(a.data, pair_keys(row, col), key, keep)
    return sp.csr_matrix((data, a.indices.copy(), a.indptr.copy()), shape=a.shape)


def squared(a):
    """``a`` embedded in the top-left corner of a square matrix (the edge mask is defined on a vertex x vertex matrix)."""
    a = a.tocsr()
    n = max(a.shape)
    indptr = np.concatenate([a.indptr, np.full(n - a.shape[0], a.indptr[-1], a.indptr.dtype)])
    out = sp.csr_matrix((a.data.astype(np.float32), a.indices.copy(), indptr), shape=(n, n))
    out.sort_indices()
    return out
