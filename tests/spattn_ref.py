"""NumPy reference of softmax dot-product attention over a CSR pattern (ops.spattn / ops.spattn_bwd, include/sgcn.h
sgcn_spattn_csr_f32, sgcn_spattn_csr_bwd_q_f32 and sgcn_spattn_csr_bwd_kv_f32) -- a test-only helper.

Semantics.  For a CSR pattern ``a`` (M x K, unique column ids per row; the stored VALUES are never read), a query table Q
(M x d), a key / value table B (K x d) and a scalar ``scale``:
    s_ij  = scale * <Q[i], B[j]>                  for j stored in row i
    lse_i = log sum_j exp(s_ij) = m_i + log l_i,  m_i = max_j s_ij,  l_i = sum_j exp(s_ij - m_i)
    p_ij  = exp(s_ij - lse_i),                    C[i] = sum_j p_ij B[j]             (empty row: C = 0, lse = -inf)
and for G = dL/dC, with delta_i = <G[i], C[i]> and e_ij = p_ij (<G[i], B[j]> - delta_i):
    dQ[i] = scale * sum_j e_ij B[j]  (+ add[i] for i < add_rows)
    dB[j] = sum_i ( p_ij G[i] + scale e_ij Q[i] )
    dx    = dB + [dQ ; 0]                         (``fused``: Q is B[:M], one gradient)
``forward`` / ``backward_f64`` evaluate this in fp64 (the fp32 inputs widened) and return, beside the values, a PER-ELEMENT
BOUND on what a correct fp32 evaluation may differ by.  ``forward_loops`` states the definition entry by entry in plain
Python (small matrices); ``forward_online_f32`` / ``backward_f32`` restate the kernels' algorithm in fp32 NumPy, in two
summation orders -- the bound has to accept both and to reject a wrong result (tests/test_spattn.py).

The bounds are derived, not fitted.  u = 2^-24 is the unit roundoff of fp32; n_i is the row's length; every analysis is to
first order, and the result is multiplied by 1 / (1 - x)^2, x the largest first-order relative term of the case (asserted
below 0.25), which covers the products of two such terms.

Forward.
  score    A d-term fp32 dot product in any order (FMA or not) errs by at most (d - 1 + 1) u sum_k |Q_ik B_jk|, its product
           with scale by one more rounding:  es_ij = (d + 2) u |scale| sum_k |Q_ik B_jk|   (one u of slack).
  weight   An entry's effective weight is a product of exponentials whose arguments add up to s_ij - m_i: exp(s_ij - m') for
           the running maximum m' when the entry arrives, then one factor exp(m' - m'') per rise of the maximum (online
           softmax), then exp(m_q - m_i) when a split row's slots meet.  Its relative error is
               W_ij = 2 max_j es_ij            the argument's error: the entry's score and the winner's (every m is a score)
                    + |s_ij - m_i| u           the roundings of the differences (their magnitudes add up to |s_ij - m_i|)
                    + (C_EXP + 1) n_i u        at most n_i exponentials, each within C_EXP u (expf is documented to 1 ulp,
                                               2 u relative: C_EXP = 2), and one rounding per rescaling product.
           The issue's E_i is W_ij / 2 for the row's worst entry; keeping it per entry is tighter where a far-away score
           (large |s - m|, negligible weight) sits in a row.
  sums     acc_c = sum_j w_ij B_jc and l = sum_j w_ij are n_i-term fp32 sums: (n_i + 1) u sum_j |w_ij B_jc| and n_i u l.
           Then one division: u.
  Together, relative to the exact C_ic = acc_c / l:
      bound_C = sum_j p_ij W_ij |B_jc|  +  ( sum_j p_ij W_ij + (2 n_i + 2) u ) sum_j p_ij |B_jc|  +  2 n_i 2^-125 max_j |B_jc|
  -- the last term for the entries whose weight lies below the normal range, p_ij < 2^-126: whatever their RELATIVE error
  (a far-away score's |s_ij - m_i| u need not be small), the computed weight stays below 2^-125 and the entry's
  contribution and its error with it; the smallness of the first-order terms is asserted over the other entries only.
  (In the issue's form, (2 E_i + c (n_i + 4) u) sum_j p_ij |B_jc|, this is c = 2 with the exponentials counted in E.)
  lse = m + log l:  max_j es_ij (m is a score) + sum_j p_ij W_ij + n_i u (l's relative error, absolute in the log)
      + C_LOG u |log l| (a logarithm good to 1 ulp; the kernel's is better) + u (|m| + |lse|) (the addition).

Backward, given a C and an lse that lie within the forward's bounds of the exact ones (the kernels read their own
forward's outputs):
  p~_ij    relative error  P_ij = es_ij + bound_lse_i + |s_ij - lse_i| u + C_EXP u
  t - delta  the cancelling difference: absolute error
           D_ij = (d + 2) u ( sum_k |G_ik B_jk| + sum_k |G_ik C_ik| ) + dC_i + u |t_ij - delta_i|
           dC_i is what the C at hand being off does to delta = <G_i, C_i>.  sum_k |G_ik| bound_C_ik would do, but adds
           the d columns' worst cases as if they were independent; they are not: C~_ik - C_ik = sum_j p_ij w_ij B_jk + r_ik
           with ONE relative weight error w_ij per entry, |w_ij| <= W_ij + sum_j p_ij W_ij (the weight and the normaliser),
           and the sums' and the division's roundings |r_ik| <= (2 n_i + 2) u sum_j p_ij |B_jk|.  Dotted with G_i:
           dC_i = sum_j p_ij (W_ij + Wbar_i) |t_ij| + (2 n_i + 2) u sum_j p_ij sum_k |G_ik B_jk| + sum_k |G_ik| tiny_ik
           -- |t_ij| = |<G_i, B_j>| in place of sum_k |G_ik B_jk|, a factor near sqrt(d) on normal data.
  e~_ij    absolute error  Ee_ij = p_ij ( P_ij |t_ij - delta_i| + D_ij ) + u |e_ij|
  dQ_ic    |scale| ( sum_j Ee_ij |B_jc| + (n_i + 2) u sum_j |e_ij B_jc| ) + u |dQ_ic|     (+ u |dQ_ic + add_ic| with an addend)
  dB_jc    sum_i ( p_ij P_ij |G_ic| + |scale| Ee_ij |Q_ic| + u |scale e_ij Q_ic| )
           + (2 n'_j + 2) u sum_i ( |p_ij G_ic| + |scale e_ij Q_ic| ),   n'_j the entries of column j  (2 terms per entry)
  dx       the two bounds added, + u |dx| for the final addition.
  As in the forward, an entry whose weight p_ij lies below the normal range (< 2^-126) has no small RELATIVE error -- the
  computed weight may be a subnormal or 0 -- but it stays below 2^-125, and so do its terms and their errors: dQ and dB get
  the absolute terms  n_i 2^-125 |scale| max_j |t_ij - delta_i| max_j |B_jc|  and
  n'_j 2^-125 ( max_i |G_ic| + |scale| max |t - delta| max_i |Q_ic| ).
"""
import numpy as np
import scipy.sparse as sp

U = 2.0 ** -24        # unit roundoff of fp32
C_EXP = 2.0           # expf: 1 ulp (HIP's documented maximum) is at most 2 u relative
C_LOG = 2.0           # logf: likewise
_CHUNK = 1 << 22      # gathered elements per block of the entry-wise dot products


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    return x.shape == y.shape and bool(np.array_equal(x.view(np.uint32), y.view(np.uint32)))


def _pattern(a):
    a = a.tocsr()
    indptr, cols = a.indptr.astype(np.int64), a.indices.astype(np.int64)
    deg = np.diff(indptr)
    return indptr, cols, np.repeat(np.arange(a.shape[0], dtype=np.int64), deg), deg


def _edot(X, Y, rows, cols):
    """sum_k X[rows, k] Y[cols, k] per stored entry, in fp64"""
    out = np.empty(rows.shape[0], np.float64)
    step = max(1, _CHUNK // max(int(X.shape[1]), 1))
    for s in range(0, rows.shape[0], step):
        out[s:s + step] = np.einsum('ek,ek->e', X[rows[s:s + step]], Y[cols[s:s + step]])
    return out


def _seg(ufunc, v, indptr, empty):
    """ufunc.reduce over every row's entries; ``empty`` for a row without any"""
    out = np.full(indptr.shape[0] - 1, empty, np.float64)
    ne = np.nonzero(np.diff(indptr) > 0)[0]
    if ne.size:
        out[ne] = ufunc.reduceat(v, indptr[ne])      # (consecutive non-empty rows' starts: the segments are the rows)
    return out


def _csr(v, cols, indptr, shape):
    return sp.csr_matrix((v, cols, indptr), shape=shape)


class Forward(object):
    """C, lse (fp64), bound_C, bound_lse and the per-entry quantities the backward's bound reuses"""


def forward(a, Q, B, scale, values_only=False):
    """``values_only``: the caller reads C and lse, not the bounds (whose first-order analysis is then not asserted to apply)"""
    indptr, cols, rows, deg = _pattern(a)
    Q64, B64 = np.asarray(Q, np.float64), np.asarray(B, np.float64)
    shape, d = a.shape, B64.shape[1]
    scale = float(scale)
    f = Forward()
    f.indptr, f.cols, f.rows, f.deg, f.shape = indptr, cols, rows, deg, shape
    f.s = s = scale * _edot(Q64, B64, rows, cols)
    f.es = es = (d + 2) * U * abs(scale) * _edot(np.abs(Q64), np.abs(B64), rows, cols)
    f.m = m = _seg(np.maximum, s, indptr, -np.inf)
    w = np.exp(s - m[rows])
    l = _seg(np.add, w, indptr, 0.0)
    f.p = p = w / l[rows]
    with np.errstate(divide='ignore'):
        logl = np.log(l)
    f.lse = np.where(deg > 0, m + logl, -np.inf)
    P = _csr(p, cols, indptr, shape)
    f.C = np.asarray(P @ B64)
    # ---- the bound (module docstring) ----
    n = deg.astype(np.float64)
    esmax = _seg(np.maximum, es, indptr, 0.0)
    W = 2 * esmax[rows] + (m[rows] - s) * U + (C_EXP + 1) * n[rows] * U
    Wbar = _seg(np.add, p * W, indptr, 0.0)
    x = float(np.max(np.where(p >= 2.0 ** -126, W + (2 * n[rows] + 2) * U, 0.0))) if rows.size else 0.0
    assert values_only or x < 0.25, "the first-order analysis needs small relative terms, got %g" % x
    f.second = second = 1.0 / (1.0 - min(x, 0.5)) ** 2
    f.W, f.Wbar = W, Wbar
    absB = np.abs(B64)
    tiny = 2 * n[:, None] * 2.0 ** -125 * (absB.max(axis=0)[None, :] if absB.shape[0] else np.zeros((1, d)))
    f.tiny = tiny
    f.bound_C = second * (np.asarray(_csr(p * W, cols, indptr, shape) @ absB)
                          + (Wbar + (2 * n + 2) * U)[:, None] * np.asarray(P @ absB)) + tiny
    fin = np.where(deg > 0, f.lse, 0.0)
    f.bound_lse = np.where(deg > 0, second * (esmax + Wbar + n * U + C_LOG * U * np.abs(np.where(deg > 0, logl, 0.0))
                                              + U * (np.abs(np.where(deg > 0, m, 0.0)) + np.abs(fin))), 0.0)
    return f


def forward_loops(a, Q, B, scale):
    """The definition, entry by entry in fp64 (small matrices only): (C, lse)."""
    a = a.tocsr()
    Q, B = np.asarray(Q, np.float64), np.asarray(B, np.float64)
    M, d = a.shape[0], B.shape[1]
    C, lse = np.zeros((M, d)), np.full(M, -np.inf)
    for i in range(M):
        js = a.indices[a.indptr[i]:a.indptr[i + 1]]
        if js.size == 0:
            continue
        s = [float(scale) * sum(Q[i, k] * B[j, k] for k in range(d)) for j in js]
        tot = sum(np.exp(v - max(s)) for v in s)
        lse[i] = max(s) + np.log(tot)
        for v, j in zip(s, js):
            C[i] += np.exp(v - lse[i]) * B[j]
    return C, lse


def loss_f64(a, Q, B, scale, G):
    """sum(G * C): what the central differences of tests/test_spattn.py differentiate"""
    return float(np.sum(np.asarray(G, np.float64) * forward(a, Q, B, scale).C))


def backward_f64(a, Q, B, G, scale, add=None, add_rows=0, fused=False, values_only=False):
    """dict(dQ, dB, bound_dQ, bound_dB) in fp64, or with ``fused`` (Q is B[:M]) dict(dx, bound_dx); dQ includes the addend."""
    f = forward(a, Q, B, scale, values_only)
    indptr, cols, rows, deg, shape = f.indptr, f.cols, f.rows, f.deg, f.shape
    M, K = shape
    Q64, B64, G64 = np.asarray(Q, np.float64)[:M], np.asarray(B, np.float64), np.asarray(G, np.float64)
    d, scale = B64.shape[1], float(scale)
    absQ, absB, absG = np.abs(Q64), np.abs(B64), np.abs(G64)
    t = _edot(G64, B64, rows, cols)
    delta = np.sum(G64 * f.C, axis=1)
    diff = t - delta[rows]
    e = f.p * diff
    csr = lambda v: _csr(v, cols, indptr, shape)
    dQ = scale * np.asarray(csr(e) @ B64)
    dB = np.asarray(csr(f.p).T.tocsr() @ G64) + scale * np.asarray(csr(e).T.tocsr() @ Q64)
    # ---- the bound (module docstring) ----
    n, nT = deg.astype(np.float64), np.bincount(cols, minlength=K).astype(np.float64)
    lse_rows = np.where(deg > 0, f.lse, 0.0)[rows]
    Pij = f.es + f.bound_lse[rows] + np.abs(f.s - lse_rows) * U + C_EXP * U
    gb = _edot(absG, absB, rows, cols)
    dC = f.second * (_seg(np.add, f.p * (f.W + f.Wbar[rows]) * np.abs(t), indptr, 0.0)
                     + (2 * n + 2) * U * _seg(np.add, f.p * gb, indptr, 0.0)) + np.sum(absG * f.tiny, axis=1)
    Dij = (d + 2) * U * (gb + np.sum(absG * np.abs(f.C), axis=1)[rows]) + dC[rows] + U * np.abs(diff)
    Ee = f.p * (Pij * np.abs(diff) + Dij) + U * np.abs(e)
    bq = abs(scale) * (np.asarray(csr(Ee) @ absB) + ((n + 2) * U)[:, None] * np.asarray(csr(np.abs(e)) @ absB)) + U * np.abs(dQ)
    eT = csr(np.abs(e)).T.tocsr()
    bb = np.asarray(csr(f.p * Pij).T.tocsr() @ absG) + abs(scale) * np.asarray(csr(Ee).T.tocsr() @ absQ) \
        + U * abs(scale) * np.asarray(eT @ absQ) \
        + ((2 * nT + 2) * U)[:, None] * (np.asarray(csr(f.p).T.tocsr() @ absG) + abs(scale) * np.asarray(eT @ absQ))
    dmax = float(np.max(np.abs(diff))) if diff.size else 0.0
    colmax = lambda X: X.max(axis=0)[None, :] if X.shape[0] else np.zeros((1, d))
    bq = bq + n[:, None] * 2.0 ** -125 * abs(scale) * dmax * colmax(absB)
    bb = bb + nT[:, None] * 2.0 ** -125 * (colmax(absG) + abs(scale) * dmax * colmax(absQ))
    if add is not None and add_rows > 0:
        r = int(add_rows)
        dQ[:r] += np.asarray(add, np.float64)[:r]
        bq[:r] += U * np.abs(dQ[:r])
    bq, bb = f.second * bq, f.second * bb
    if not fused:
        return dict(dQ=dQ, dB=dB, bound_dQ=bq, bound_dB=bb, fwd=f)
    assert K >= M
    dx, bx = dB.copy(), bb.copy()
    dx[:M] += dQ
    bx[:M] += bq
    bx += U * np.abs(dx)
    return dict(dx=dx, bound_dx=bx, fwd=f)


# ---- fp32 restatements of the kernels' algorithm (what the bounds must accept) -------------------------------------------
def _pieces(js, reverse, cut):
    js = js[::-1] if reverse else js
    if cut and js.size > 1:
        return [js[:js.size // 2], js[js.size // 2:]]
    return [js]


def forward_online_f32(a, Q, B, scale, reverse=False, cut=False):
    """(C, lse) in fp32 by the online softmax: a running (m, l, acc), rescaled when m rises; ``reverse`` walks every row
    backwards, ``cut`` halves every row into two pieces that are merged as the fix-up merges slots."""
    f32 = np.float32
    a = a.tocsr()
    Q, B, scale = np.asarray(Q, f32), np.asarray(B, f32), f32(scale)
    M, d = a.shape[0], B.shape[1]
    C, lse = np.zeros((M, d), f32), np.full(M, -np.inf, f32)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        for i in range(M):
            js = a.indices[a.indptr[i]:a.indptr[i + 1]]
            if js.size == 0:
                continue
            parts = []
            for piece in _pieces(js, reverse, cut):
                m, l, acc = f32(-np.inf), f32(0), np.zeros(d, f32)
                for j in piece:
                    s = f32(np.dot(Q[i], B[j])) * scale
                    if s > m:
                        alpha = np.exp(f32(m - s))
                        l, acc, m = f32(l * alpha), acc * alpha, s
                    p = np.exp(f32(s - m))
                    l, acc = f32(l + p), acc + p * B[j]
                parts.append((m, l, acc))
            m = max(x[0] for x in parts)
            l, acc = f32(0), np.zeros(d, f32)
            for mq, lq, aq in parts:
                sc = np.exp(f32(mq - m))
                l, acc = f32(l + lq * sc), acc + sc * aq
            C[i], lse[i] = acc / l, f32(m + np.log(l))
    return C, lse


def backward_f32(a, Q, B, G, scale, C, lse, reverse=False, cut=False):
    """(dQ, dB) in fp32 from an fp32 forward's C and lse, p and e recomputed per entry; the sums in the order / pieces of
    ``forward_online_f32``'s arguments (rows of the pattern for dQ, rows of the transposed pattern for dB)."""
    f32 = np.float32
    a = a.tocsr()
    at = a.T.tocsr()
    at.sort_indices()
    Q, B, G, C, lse, scale = (np.asarray(x, f32) for x in (Q, B, G, C, lse, scale))
    M, K, d = a.shape[0], a.shape[1], B.shape[1]
    delta = np.array([f32(np.dot(G[i], C[i])) for i in range(M)], f32)
    dQ, dB = np.zeros((M, d), f32), np.zeros((K, d), f32)

    def pe(i, j):
        p = np.exp(f32(f32(np.dot(Q[i], B[j])) * scale - lse[i]))
        return p, f32(p * f32(f32(np.dot(G[i], B[j])) - delta[i]))
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        for i in range(M):
            tot = np.zeros(d, f32)
            for piece in _pieces(a.indices[a.indptr[i]:a.indptr[i + 1]], reverse, cut):
                acc = np.zeros(d, f32)
                for j in piece:
                    acc = acc + pe(i, j)[1] * B[j]
                tot = tot + acc
            dQ[i] = scale * tot
        for j in range(K):
            tot = np.zeros(d, f32)
            for piece in _pieces(at.indices[at.indptr[j]:at.indptr[j + 1]], reverse, cut):
                acc = np.zeros(d, f32)
                for i in piece:
                    p, e = pe(i, j)
                    acc = acc + p * G[i]
                    acc = acc + f32(scale * e) * Q[i]
                tot = tot + acc
            dB[j] = tot
    return dQ, dB
