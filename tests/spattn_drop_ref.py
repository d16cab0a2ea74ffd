"""NumPy reference of attention with DROPOUT ON THE COEFFICIENTS (ops.spattn / ops.spattn_bwd with ``keep`` < 1;
include/sgcn.h sgcn_spattn_drop_csr_f32, sgcn_spattn_drop_csr_bwd_q_f32, sgcn_spattn_drop_csr_bwd_kv_f32) -- a test-only helper.

The mask, restated on oracle.model_np._fmix32 (nothing of stochastic_gcn_amd is imported here).  All arithmetic mod 2^32,
i the ROW and j the COLUMN of the pattern, h the head:
    pair(i, j)    = fmix32(fmix32(i * 0x9E3779B1 + key) + j * 0x85EBCA77)
    kept(i, j, h) iff fmix32(pair(i, j) + h * 0x27D4EB2F) < thr,   thr = min(floor(fp32(keep) * 2^32), 2^32 - 1)
    mk_ijh        = kept ? fp32(1) / fp32(keep) : 0
    key           = dropout_key(seed, ATTN_SITE + layer index, step)

Definition, per head (heads as in tests/spattn_heads_ref.py; s, m, l, lse and p_ij are those WITHOUT dropout):
    C[i]    = sum_j p_ij mk_ij B[j]
    delta_i = <G[i], C[i]>,   t_ij = <G[i], B[j]>,   e_ij = p_ij (mk_ij t_ij - delta_i)
    dQ[i]   = scale sum_j e_ij B[j] (+ add),   dB[j] = sum_i ( p_ij mk_ij G[i] + scale e_ij Q[i] )
(the gradient of L = sum(G * C) under a fixed mask: dL/ds_ij = p_ij (mk_ij t_ij - sum_k p_ik mk_ik t_ik), and the inner sum is
<G[i], C[i]> with the MASKED C -- ``values`` below evaluates exactly this, tests/test_spattn_drop.py differentiates it).

``forward`` / ``backward_f64`` return, beside the fp64 values, PER-ELEMENT BOUNDS on what a correct fp32 evaluation may differ
by.  They extend the derivation in tests/spattn_ref.py (its notation: u, n_i, es, W, Wbar, P, D, Ee; read that docstring
first); what the mask changes, term by term -- derived, not fitted:
  forward  The weights w_ij, their errors W_ij and the normaliser l (over ALL entries) are untouched, hence lse and bound_lse
           are those of spattn_ref.  The numerator adds fl(w_ij mk_ij) B_jc: ONE MORE ROUNDING per entry, so an entry's term
           carries (W_ij + u) and the magnitude p_ij mk_ij |B_jc|; the n_i-term sums and the division are as before:
               bound_C = sum_j p_ij mk_ij (W_ij + u) |B_jc| + ( Wbar_i + (2 n_i + 2) u ) sum_j p_ij mk_ij |B_jc| + mk tiny_ic
           (tiny: the entries whose weight is below the normal range stay below 2^-125 mk).  The second-order factor is
           1 / (1 - (x + u))^2 with spattn_ref's x.
  backward p~_ij: P_ij as before (p is recomputed from lse; no mask in it).
           fl(mk_ij t~_ij): the dot product's (d + 2) u sum_k |G_ik B_jk| scaled by mk_ij, and one more rounding,
           u |mk_ij t_ij| <= u mk_ij sum_k |G_ik B_jk|:  mk_ij (d + 3) u sum_k |G_ik B_jk|.
           delta~_i = <G_i, C~_i> from the MASKED C~ at hand:  (d + 2) u sum_k |G_ik C_ik| + dC_i with
               dC_i = sum_j p_ij mk_ij (W_ij + u + Wbar_i) |t_ij| + (2 n_i + 2) u sum_j p_ij mk_ij sum_k |G_ik B_jk|
                      + mk sum_k |G_ik| tiny_ik
           D_ij  = mk_ij (d + 3) u sum_k |G_ik B_jk| + (d + 2) u sum_k |G_ik C_ik| + dC_i + u |mk_ij t_ij - delta_i|
           Ee_ij = p_ij ( P_ij |mk_ij t_ij - delta_i| + D_ij ) + u |e_ij|
           dQ_ic: spattn_ref's formula on these e and Ee (a dropped entry still contributes -p_ij delta_i: all n_i terms).
           dB_jc: the first term is fl(p~_ij mk_ij) G_ic -- relative error P_ij + u on p_ij mk_ij |G_ic| -- the rest as before,
                  with |p_ij mk_ij G_ic| in the sums' term.
           The subnormal-weight terms: spattn_ref's, the G term times mk.
"""
import numpy as np

import spattn_heads_ref as href
import spattn_ref as ref
from oracle import model_np as mnp

U = ref.U
ATTN_SITE = 0x4154544E
same_bits = ref.same_bits
_M = np.uint64(0xFFFFFFFF)


# ---- the mask ------------------------------------------------------------------------------------------------------------
def _u32(x):
    return np.asarray(x, dtype=np.int64).astype(np.uint64) & _M


def pair(i, j, key):
    rowh = mnp._fmix32(_u32(i) * np.uint64(0x9E3779B1) + np.uint64(int(key) & 0xFFFFFFFF))
    return mnp._fmix32(rowh + ((_u32(j) * np.uint64(0x85EBCA77)) & _M))


def threshold(keep):
    t = float(np.float32(keep)) * 4294967296.0
    return 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def kept(i, j, h, key, keep):
    """bool array: entry (row i, column j) stays in head h"""
    return mnp._fmix32(pair(i, j, key) + ((_u32(h) * np.uint64(0x27D4EB2F)) & _M)) < np.uint64(threshold(keep))


def mk_value(keep):
    """the fp32 quotient 1 / keep, as a Python float"""
    return float(np.float32(1.0) / np.float32(keep))


def attn_key(seed, layer_index, step):
    return mnp.dropout_key(seed, ATTN_SITE + int(layer_index), step)


def mask(a, heads, key, keep, transposed=False):
    """(nnz, heads) fp64: mk_ijh of every stored entry in CSR order.  ``transposed``: the WRONG mask pair(j, i)."""
    _, cols, rows, _ = ref._pattern(a)
    i, j = (cols, rows) if transposed else (rows, cols)
    if keep >= 1.0:
        return np.ones((rows.shape[0], heads))
    k = np.stack([kept(i, j, h, key, keep) for h in range(heads)], axis=1) if rows.size else np.zeros((0, heads), bool)
    return k * mk_value(keep)


# ---- fp64 values, nothing else (the definition; also the wrong variants the bounds must reject) ------------------------------
def values(a, Q, B, G, scale, heads, mk, norm_over_kept=False, delta_unmasked=False):
    """dict(C, lse (M x H), dQ, dB) in fp64 under the mask ``mk`` (nnz x H).  The two switches state WRONG implementations:
    the softmax normalised over the kept entries only; delta taken from the unmasked output."""
    indptr, cols, rows, deg = ref._pattern(a)
    shape = a.shape
    Q, B, G = (np.asarray(x, np.float64) for x in (Q, B, G))
    M = shape[0]
    out = dict(C=np.zeros((M, B.shape[1])), lse=np.full((M, heads), -np.inf), dQ=np.zeros((M, B.shape[1])), dB=np.zeros_like(B))
    csr = lambda v: ref._csr(v, cols, indptr, shape)     # noqa: E731
    for h, sl in enumerate(href.head_slices(B.shape[1], heads)):
        q, b, g, mkh = Q[:M, sl], B[:, sl], G[:, sl], np.asarray(mk, np.float64)[:, h]
        s = float(scale) * ref._edot(q, b, rows, cols)
        m = ref._seg(np.maximum, s, indptr, -np.inf)
        w = np.exp(s - m[rows])
        l = ref._seg(np.add, w * (mkh > 0) if norm_over_kept else w, indptr, 0.0)
        with np.errstate(divide='ignore', invalid='ignore'):
            p = np.where(l[rows] > 0, w / l[rows], 0.0)
            out['lse'][:, h] = np.where(l > 0, m + np.log(l), -np.inf)
        pm = p * mkh
        C = np.asarray(csr(pm) @ b)
        t = ref._edot(g, b, rows, cols)
        delta = np.sum(g * (np.asarray(csr(p) @ b) if delta_unmasked else C), axis=1)
        e = p * (mkh * t - delta[rows])
        out['C'][:, sl] = C
        out['dQ'][:, sl] = float(scale) * np.asarray(csr(e) @ b)
        out['dB'][:, sl] = np.asarray(csr(pm).T.tocsr() @ g) + float(scale) * np.asarray(csr(e).T.tocsr() @ q)
    return out


def loss_f64(a, Q, B, scale, G, heads, mk):
    return float(np.sum(np.asarray(G, np.float64) * values(a, Q, B, G, scale, heads, mk)['C']))


# ---- fp64 values with bounds ---------------------------------------------------------------------------------------------------
class Forward(object):
    """C (M x d), lse (M x H), bound_C, bound_lse; ``per_head`` the single-head records"""


def _forward1(a, Q, B, scale, mk, values_only):
    f = ref.forward(a, Q, B, scale, values_only)
    B64 = np.asarray(B, np.float64)
    absB = np.abs(B64)
    n = f.deg.astype(np.float64)
    csr = lambda v: ref._csr(v, f.cols, f.indptr, f.shape)     # noqa: E731
    g = Forward()
    g.base, g.mk = f, np.asarray(mk, np.float64)
    g.mkmax = float(max(g.mk.max() if g.mk.size else 1.0, 1.0))
    g.pm = pm = f.p * g.mk
    x = 1.0 - f.second ** -0.5                                  # spattn_ref's largest first-order term
    g.second = 1.0 / (1.0 - min(x + U, 0.5)) ** 2
    g.C = np.asarray(csr(pm) @ B64)
    g.tiny = f.tiny * g.mkmax
    g.bound_C = g.second * (np.asarray(csr(pm * (f.W + U)) @ absB)
                            + (f.Wbar + (2 * n + 2) * U)[:, None] * np.asarray(csr(pm) @ absB)) + g.tiny
    g.lse, g.bound_lse, g.deg = f.lse, f.bound_lse, f.deg
    return g


def _backward1(a, Q, B, G, scale, mk, add, add_rows, fused, values_only):
    g = _forward1(a, Q, B, scale, mk, values_only)
    f = g.base
    indptr, cols, rows, deg, shape = f.indptr, f.cols, f.rows, f.deg, f.shape
    M, K = shape
    Q64, B64, G64 = np.asarray(Q, np.float64)[:M], np.asarray(B, np.float64), np.asarray(G, np.float64)
    d, scale = B64.shape[1], float(scale)
    absQ, absB, absG = np.abs(Q64), np.abs(B64), np.abs(G64)
    csr = lambda v: ref._csr(v, cols, indptr, shape)            # noqa: E731
    mkv, pm = g.mk, g.pm
    t = ref._edot(G64, B64, rows, cols)
    delta = np.sum(G64 * g.C, axis=1)
    diff = mkv * t - delta[rows]
    e = f.p * diff
    dQ = scale * np.asarray(csr(e) @ B64)
    dB = np.asarray(csr(pm).T.tocsr() @ G64) + scale * np.asarray(csr(e).T.tocsr() @ Q64)
    # ---- the bound (module docstring) ----
    n, nT = deg.astype(np.float64), np.bincount(cols, minlength=K).astype(np.float64)
    lse_rows = np.where(deg > 0, f.lse, 0.0)[rows]
    Pij = f.es + f.bound_lse[rows] + np.abs(f.s - lse_rows) * U + ref.C_EXP * U
    gb = ref._edot(absG, absB, rows, cols)
    dC = g.second * (ref._seg(np.add, pm * (f.W + U + f.Wbar[rows]) * np.abs(t), indptr, 0.0)
                     + (2 * n + 2) * U * ref._seg(np.add, pm * gb, indptr, 0.0)) + np.sum(absG * g.tiny, axis=1)
    Dij = mkv * (d + 3) * U * gb + (d + 2) * U * np.sum(absG * np.abs(g.C), axis=1)[rows] + dC[rows] + U * np.abs(diff)
    Ee = f.p * (Pij * np.abs(diff) + Dij) + U * np.abs(e)
    bq = abs(scale) * (np.asarray(csr(Ee) @ absB) + ((n + 2) * U)[:, None] * np.asarray(csr(np.abs(e)) @ absB)) + U * np.abs(dQ)
    eT, pmT = csr(np.abs(e)).T.tocsr(), csr(pm).T.tocsr()
    bb = np.asarray(csr(pm * (Pij + U)).T.tocsr() @ absG) + abs(scale) * np.asarray(csr(Ee).T.tocsr() @ absQ) \
        + U * abs(scale) * np.asarray(eT @ absQ) \
        + ((2 * nT + 2) * U)[:, None] * (np.asarray(pmT @ absG) + abs(scale) * np.asarray(eT @ absQ))
    dmax = float(np.max(np.abs(diff))) if diff.size else 0.0
    colmax = lambda X: X.max(axis=0)[None, :] if X.shape[0] else np.zeros((1, d))      # noqa: E731
    bq = bq + n[:, None] * 2.0 ** -125 * abs(scale) * dmax * colmax(absB)
    bb = bb + nT[:, None] * 2.0 ** -125 * (g.mkmax * colmax(absG) + abs(scale) * dmax * colmax(absQ))
    if add is not None and add_rows > 0:
        r = int(add_rows)
        dQ[:r] += np.asarray(add, np.float64)[:r]
        bq[:r] += U * np.abs(dQ[:r])
    bq, bb = g.second * bq, g.second * bb
    if not fused:
        return dict(dQ=dQ, dB=dB, bound_dQ=bq, bound_dB=bb, fwd=g)
    assert K >= M
    dx, bx = dB.copy(), bb.copy()
    dx[:M] += dQ
    bx[:M] += bq
    bx += U * np.abs(dx)
    return dict(dx=dx, bound_dx=bx, fwd=g)


def _gather(per_head):
    f = Forward()
    f.per_head = per_head
    f.C = np.concatenate([h.C for h in per_head], axis=1)
    f.bound_C = np.concatenate([h.bound_C for h in per_head], axis=1)
    f.lse = np.stack([h.lse for h in per_head], axis=1)
    f.bound_lse = np.stack([h.bound_lse for h in per_head], axis=1)
    f.deg = per_head[0].deg
    return f


def forward(a, Q, B, scale, heads, mk, values_only=False):
    Q, B, mk = np.asarray(Q), np.asarray(B), np.asarray(mk)
    return _gather([_forward1(a, Q[:, s], B[:, s], scale, mk[:, h], values_only)
                    for h, s in enumerate(href.head_slices(B.shape[1], heads))])


def backward_f64(a, Q, B, G, scale, heads, mk, add=None, add_rows=0, fused=False, values_only=False):
    """spattn_heads_ref.backward_f64's dict under the mask ``mk`` (nnz x heads); ``fused``: Q is B[:M], one gradient dx"""
    Q, B, G, mk = np.asarray(Q), np.asarray(B), np.asarray(G), np.asarray(mk)
    M = a.shape[0]
    with_add = add is not None and add_rows > 0
    parts = [_backward1(a, B[:M, s] if fused else Q[:, s], B[:, s], G[:, s], scale, mk[:, h],
                        np.asarray(add)[:, s] if with_add else None, add_rows if with_add else 0, fused, values_only)
             for h, s in enumerate(href.head_slices(B.shape[1], heads))]
    out = {k: np.concatenate([p[k] for p in parts], axis=1) for k in parts[0] if k != 'fwd'}
    out['fwd'] = _gather([p['fwd'] for p in parts])
    return out


# ---- fp32 restatements of the kernels' algorithm (what the bounds must accept) -------------------------------------------------
def _forward_online1(a, Q, B, scale, mk, reverse, cut):
    f32 = np.float32
    a = a.tocsr()
    Q, B, scale, mk = np.asarray(Q, f32), np.asarray(B, f32), f32(scale), np.asarray(mk, f32)
    M, d = a.shape[0], B.shape[1]
    C, lse = np.zeros((M, d), f32), np.full(M, -np.inf, f32)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        for i in range(M):
            es = np.arange(a.indptr[i], a.indptr[i + 1])
            if es.size == 0:
                continue
            parts = []
            for piece in ref._pieces(es, reverse, cut):
                m, l, acc = f32(-np.inf), f32(0), np.zeros(d, f32)
                for e in piece:
                    j = a.indices[e]
                    s = f32(np.dot(Q[i], B[j])) * scale
                    if s > m:
                        alpha = np.exp(f32(m - s))
                        l, acc, m = f32(l * alpha), acc * alpha, s
                    p = np.exp(f32(s - m))
                    l, acc = f32(l + p), acc + f32(p * mk[e]) * B[j]        # l over every entry; the mask on the numerator
                parts.append((m, l, acc))
            m = max(x[0] for x in parts)
            l, acc = f32(0), np.zeros(d, f32)
            for mq, lq, aq in parts:
                sc = np.exp(f32(mq - m))
                l, acc = f32(l + lq * sc), acc + sc * aq
            C[i], lse[i] = acc / l, f32(m + np.log(l))
    return C, lse


def _backward1_f32(a, Q, B, G, scale, C, lse, mk, reverse, cut):
    import scipy.sparse as sp
    f32 = np.float32
    a = a.tocsr()
    nnz = a.indices.shape[0]
    pos = sp.csr_matrix((np.arange(1, nnz + 1, dtype=np.int64), a.indices, a.indptr), shape=a.shape)
    post = pos.T.tocsr()
    post.sort_indices()                                          # row j: the source rows i ascending, data = entry + 1
    Q, B, G, C, lse, scale, mk = (np.asarray(x, f32) for x in (Q, B, G, C, lse, scale, mk))
    M, K, d = a.shape[0], a.shape[1], B.shape[1]
    delta = np.array([f32(np.dot(G[i], C[i])) for i in range(M)], f32)
    dQ, dB = np.zeros((M, d), f32), np.zeros((K, d), f32)

    def pe(i, j, e):
        p = np.exp(f32(f32(np.dot(Q[i], B[j])) * scale - lse[i]))
        tm = f32(mk[e] * f32(np.dot(G[i], B[j])))
        return p, f32(p * f32(tm - delta[i]))
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        for i in range(M):
            tot = np.zeros(d, f32)
            for piece in ref._pieces(np.arange(a.indptr[i], a.indptr[i + 1]), reverse, cut):
                acc = np.zeros(d, f32)
                for e in piece:
                    acc = acc + pe(i, a.indices[e], e)[1] * B[a.indices[e]]
                tot = tot + acc
            dQ[i] = scale * tot
        for j in range(K):
            tot = np.zeros(d, f32)
            for piece in ref._pieces(np.arange(post.indptr[j], post.indptr[j + 1]), reverse, cut):
                acc = np.zeros(d, f32)
                for k in piece:
                    i, e = post.indices[k], int(post.data[k]) - 1
                    p, ev = pe(i, j, e)
                    acc = acc + f32(p * mk[e]) * G[i]
                    acc = acc + f32(scale * ev) * Q[i]
                tot = tot + acc
            dB[j] = tot
    return dQ, dB


def forward_online_f32(a, Q, B, scale, heads, mk, reverse=False, cut=False):
    """(C, lse M x H) in fp32 by the online softmax with the mask on the numerator; orders as spattn_ref.forward_online_f32"""
    Q, B, mk = np.asarray(Q), np.asarray(B), np.asarray(mk)
    parts = [_forward_online1(a, Q[:, s], B[:, s], scale, mk[:, h], reverse, cut)
             for h, s in enumerate(href.head_slices(B.shape[1], heads))]
    return np.concatenate([p[0] for p in parts], axis=1), np.stack([p[1] for p in parts], axis=1)


def backward_f32(a, Q, B, G, scale, C, lse, heads, mk, reverse=False, cut=False):
    Q, B, G, C, lse, mk = (np.asarray(x) for x in (Q, B, G, C, lse, mk))
    parts = [_backward1_f32(a, Q[:, s], B[:, s], G[:, s], scale, C[:, s], lse[:, h], mk[:, h], reverse, cut)
             for h, s in enumerate(href.head_slices(B.shape[1], heads))]
    return np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)
