"""NumPy reference of attention with learned additive scores (GAT) over a CSR pattern (ops.gat_scores / ops.spgat /
ops.spgat_bwd / ops.gat_scores_bwd; include/sgcn.h sgcn_gat_scores_f32, sgcn_spgat_csr_f32, sgcn_spgat_csr_bwd_u_f32,
sgcn_spgat_csr_bwd_v_f32 and sgcn_gat_scores_bwd_f32) -- a test-only helper.

Definition (restated from include/sgcn.h).  H in {1, 2, 4, 8} heads, d % H == 0, dh = d / H, head h the columns
[h dh, (h + 1) dh).  The layer's parameter is a (2, d): a[0] = a_src, a[1] = a_dst, the heads' slices side by side.
    u_i^h = sum_{c in h} x[i, c] a[0, c]        v_j^h = sum_{c in h} x[j, c] a[1, c]
    z_ij  = u_i + v_j   (ONE fp32 addition in the kernels)        s_ij = z_ij > 0 ? z_ij : slope z_ij
    lse_i = log sum_j exp(s_ij) = m_i + log l_i,  p_ij = exp(s_ij - lse_i),  C_i = sum_j mk_ij p_ij B_j
(an empty row: C = 0, lse = -inf; mk_ij = 1, or the coefficient mask of --attn_dropout: 0 or 1 / keep, after the softmax), and for
G = dL/dC:
    delta_i = <G_i, C_i>_h      e_ij = p_ij (mk_ij <G_i, B_j>_h - delta_i)      dz_ij = e_ij (z_ij > 0 ? 1 : slope)
    dU[i, h] = sum_j dz_ij      dV[j, h] = sum_i dz_ij                          dB_j = sum_i mk_ij p_ij G_i
    dX[r, c] += dU[r, h(c)] a[0, c] + dV[r, h(c)] a[1, c]
    da[0, c] = sum_r dU[r, h(c)] x[r, c]        da[1, c] = sum_r dV[r, h(c)] x[r, c]
The derivative of the LeakyReLU at z == 0 is `slope`.

``forward`` / ``backward_f64`` take the score TABLES U (M, H) and V (K, H) as given (fp32 values widened), as the kernels do,
evaluate in fp64 and return, beside the values, a PER-ELEMENT BOUND on what a correct fp32 evaluation may differ by.
``forward_loops`` / ``backward_loops`` state the definition entry by entry in plain Python; ``forward_online_f32`` /
``backward_f32`` restate the kernels' algorithm in fp32 NumPy in two summation orders; ``layer_f64`` is the whole chain from
(x, a) that the central differences of tests/test_spgat.py differentiate.

The bounds are derived the way tests/spattn_ref.py derives its own (u = 2^-24, first-order terms, the result multiplied by
1 / (1 - x)^2 for the largest first-order relative term x of the case, asserted below 0.25).  n_i is the row's length.
  z, s     z is ONE rounding of u_i + v_j: |dz| <= u |z|.  fl(u + v) has the sign of u + v (rounding is monotone, and a sum of
           two fp32 numbers that is not representable is not 0), so the LeakyReLU takes the exact branch; slope * z is one
           more rounding.  |s| <= |z| for a slope in [0, 1]:   es_ij = 2 u |z_ij|.
  weight   as spattn_ref: W_ij = 2 max_j es_ij + |s_ij - m_i| u + (C_EXP + 1) n_i u   (every m is a score; the roundings of
           the differences; at most n_i exponentials within C_EXP u each and one rounding per rescaling product).
  sums     acc_c = sum_j (w_ij mk_ij) B_jc: one rounding for w mk, (n_i + 1) u for the sum; l = sum_j w_ij over ALL entries:
           n_i u; one division: u.
      bound_C   = sum_j mk_ij p_ij W_ij |B_jc| + (Wbar_i + (2 n_i + 3) u) sum_j mk_ij p_ij |B_jc| + 2 n_i 2^-125 mkmax max_j |B_jc|
                  Wbar_i = sum_j p_ij W_ij (the normaliser's relative error; the mask does not touch l)
      bound_lse = max_j es_ij + Wbar_i + n_i u + C_LOG u |log l_i| + u (|m_i| + |lse_i|)
  Backward, from a C and an lse within these bounds of the exact ones (the kernels read their own forward's outputs):
      p~        relative error  P_ij = es_ij + bound_lse_i + |s_ij - lse_i| u + C_EXP u
      delta     bound_delta_i = (dh + 2) u sum_{k in h} |G_ik C_ik| + dC_i, where dC_i is what the C at hand being off does to
                <G_i, C_i>.  As in spattn_ref, not sum_k |G_ik| bound_C_ik (the columns' worst cases are not independent):
                C~_ik - C_ik = sum_j mk_ij p_ij w_ij B_jk + r_ik with ONE relative weight error per entry, |w_ij| <= W_ij + Wbar_i,
                and |r_ik| <= (2 n_i + 3) u sum_j mk_ij p_ij |B_jk|; dotted with G_i,
                dC_i = sum_j mk_ij p_ij (W_ij + Wbar_i) |t_ij| + (2 n_i + 3) u sum_j mk_ij p_ij sum_k |G_ik B_jk| + sum_k |G_ik| tiny_ik
      mk t - delta   absolute error  D_ij = mk_ij (dh + 3) u sum_k |G_ik B_jk| + bound_delta_i + u |mk_ij t_ij - delta_i|
      e~        Ee_ij = p_ij (P_ij |mk_ij t_ij - delta_i| + D_ij) + u |e_ij|
      dz~       Ez_ij = Ee_ij f_ij + u |dz_ij|,  f_ij = 1 or slope  (the exact branch, see above)
      dU[i,h]   sum_j Ez_ij + (n_i + 1) u sum_j |dz_ij| + n_i 2^-125 max_j |mk t - delta|     (weights below the normal range)
      dV[j,h]   the same over the column j, n'_j its entries
      dB_jc     sum_i mk_ij p_ij (P_ij + u) |G_ic| + (n'_j + 1) u sum_i mk_ij p_ij |G_ic| + n'_j 2^-125 mkmax max_i |G_ic|
                (+ u |dB_jc + add_jc| with an addend)
  Scores    u_r^h, v_r^h: a dh-term fp32 dot product in any order, (dh + 1) u sum_{c in h} |x[r, c] a[., c]|.
  da        a sum over `rows` terms, each one fused multiply-add, at most 64 of them and ceil(rows / 64) partial sums deep:
            gamma_rows sum_r |dU[r, h] x[r, c]|, gamma_n = n u / (1 - n u).
  dX        two fused multiply-adds: 2 u (|dX0| + |dU a_0| + |dV a_1|).
"""
import numpy as np
import scipy.sparse as sp

U_ = 2.0 ** -24       # unit roundoff of fp32
C_EXP = 2.0
C_LOG = 2.0


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    return x.shape == y.shape and bool(np.array_equal(x.view(np.uint32), y.view(np.uint32)))


def _pattern(a):
    a = a.tocsr()
    indptr, cols = a.indptr.astype(np.int64), a.indices.astype(np.int64)
    deg = np.diff(indptr)
    return indptr, cols, np.repeat(np.arange(a.shape[0], dtype=np.int64), deg), deg


def _seg(ufunc, v, indptr, empty):
    out = np.full(indptr.shape[0] - 1, empty, np.float64)
    ne = np.nonzero(np.diff(indptr) > 0)[0]
    if ne.size:
        out[ne] = ufunc.reduceat(v, indptr[ne])
    return out


def _csr(v, cols, indptr, shape):
    return sp.csr_matrix((v, cols, indptr), shape=shape)


def leaky(z, slope):
    return np.where(z > 0, z, slope * z)


def leaky_d(z, slope):
    return np.where(z > 0, 1.0, slope)          # (at z == 0: slope)


def scores_f64(x, a, heads):
    """(S, bound): S (rows, 2 H) in fp64 from the fp32 inputs widened; bound = (dh + 1) u sum |x a| per cell"""
    x64, a64 = np.asarray(x, np.float64), np.asarray(a, np.float64)
    rows, d = x64.shape
    dh = d // heads
    S = np.concatenate([(x64 * a64[w]).reshape(rows, heads, dh).sum(axis=2) for w in (0, 1)], axis=1)
    bound = np.concatenate([(np.abs(x64) * np.abs(a64[w])).reshape(rows, heads, dh).sum(axis=2) for w in (0, 1)], axis=1)
    return S, (dh + 1) * U_ * bound


def scores_f32_kernel_order(x, a, heads):
    """S in fp32 in the kernel's documented order: lane l of 64 adds columns l, l + 64, .. of the head by fused multiply-add,
    then the butterfly 32 .. 1.  The fma is restated as an fp64 product (exact) and an fp64 sum rounded to fp32: the very bits
    where a lane holds one column (the sum with +0 is exact), and within one extra fp64 rounding of them otherwise."""
    f32 = np.float32
    x, a = np.asarray(x, f32), np.asarray(a, f32)
    rows, d = x.shape
    dh = d // heads
    S = np.zeros((rows, 2 * heads), f32)
    for w in (0, 1):
        for h in range(heads):
            lanes = np.zeros((rows, 64), f32)
            for c in range(dh):
                col = h * dh + c
                lanes[:, c % 64] = (x[:, col].astype(np.float64) * float(a[w, col]) + lanes[:, c % 64].astype(np.float64)).astype(f32)
            o = 32
            while o:
                lanes = lanes + lanes[:, np.arange(64) ^ o]
                o >>= 1
            S[:, w * heads + h] = lanes[:, 0]
    return S


class Forward(object):
    pass


def _mask(mk, nnz, heads):
    """the coefficient mask as an (nnz, H) fp64 array (None: all ones)"""
    if mk is None:
        return np.ones((nnz, heads))
    mk = np.asarray(mk, np.float64)
    return mk.reshape(nnz, heads)


def forward(a, U, V, B, slope, heads=1, mk=None, values_only=False):
    """C (M, d), lse (M, H) in fp64 with their bounds; ``mk`` (nnz, H): the mask's values per stored entry, in CSR order"""
    indptr, cols, rows, deg = _pattern(a)
    shape = a.shape
    M, K = shape
    U64, V64, B64 = np.asarray(U, np.float64)[:M], np.asarray(V, np.float64)[:K], np.asarray(B, np.float64)[:K]
    d = B64.shape[1]
    dh = d // heads
    slope = float(slope)
    mk = _mask(mk, rows.size, heads)
    f = Forward()
    f.indptr, f.cols, f.rows, f.deg, f.shape, f.heads, f.dh, f.mk, f.slope = indptr, cols, rows, deg, shape, heads, dh, mk, slope
    n = deg.astype(np.float64)
    f.C, f.bound_C = np.zeros((M, d)), np.zeros((M, d))
    f.lse, f.bound_lse = np.full((M, heads), -np.inf), np.zeros((M, heads))
    f.z, f.s, f.p, f.es, f.W, f.Wbar = [], [], [], [], [], []
    xs = 0.0
    for h in range(heads):
        sl = slice(h * dh, (h + 1) * dh)
        z = U64[rows, h] + V64[cols, h]
        s = leaky(z, slope)
        es = 2 * U_ * np.abs(z)
        m = _seg(np.maximum, s, indptr, -np.inf)
        w = np.exp(s - m[rows])
        l = _seg(np.add, w, indptr, 0.0)
        p = w / l[rows]
        with np.errstate(divide='ignore'):
            logl = np.log(l)
        f.lse[:, h] = np.where(deg > 0, m + logl, -np.inf)
        pm = p * mk[:, h]
        Bh, absB = B64[:, sl], np.abs(B64[:, sl])
        f.C[:, sl] = np.asarray(_csr(pm, cols, indptr, shape) @ Bh)
        esmax = _seg(np.maximum, es, indptr, 0.0)
        W = 2 * esmax[rows] + (m[rows] - s) * U_ + (C_EXP + 1) * n[rows] * U_
        Wbar = _seg(np.add, p * W, indptr, 0.0)
        if rows.size:
            xs = max(xs, float(np.max(np.where(p >= 2.0 ** -126, W + (2 * n[rows] + 3) * U_, 0.0))))
        mkmax = float(mk.max()) if mk.size else 1.0
        tiny = 2 * n[:, None] * 2.0 ** -125 * mkmax * (absB.max(axis=0)[None, :] if absB.shape[0] else np.zeros((1, dh)))
        f.bound_C[:, sl] = (np.asarray(_csr(pm * W, cols, indptr, shape) @ absB)            # (first order; finished below)
                            + (Wbar + (2 * n + 3) * U_)[:, None] * np.asarray(_csr(pm, cols, indptr, shape) @ absB))
        f._tiny = getattr(f, '_tiny', {})
        f._tiny[h] = tiny
        fin = np.where(deg > 0, f.lse[:, h], 0.0)
        f.bound_lse[:, h] = np.where(deg > 0, esmax + Wbar + n * U_ + C_LOG * U_ * np.abs(np.where(deg > 0, logl, 0.0))
                                     + U_ * (np.abs(np.where(deg > 0, m, 0.0)) + np.abs(fin)), 0.0)
        for lst, v in ((f.z, z), (f.s, s), (f.p, p), (f.es, es), (f.W, W), (f.Wbar, Wbar)):
            lst.append(v)
    assert values_only or xs < 0.25, "the first-order analysis needs small relative terms, got %g" % xs
    f.second = 1.0 / (1.0 - min(xs, 0.5)) ** 2
    for h in range(heads):
        sl = slice(h * dh, (h + 1) * dh)
        f.bound_C[:, sl] = f.second * f.bound_C[:, sl] + f._tiny[h]
    f.bound_lse = f.second * f.bound_lse
    return f


def forward_loops(a, U, V, B, slope, heads=1, mk=None):
    """The definition, entry by entry in fp64 (small matrices only): (C, lse)."""
    a = a.tocsr()
    U, V, B = (np.asarray(t, np.float64) for t in (U, V, B))
    M, d = a.shape[0], B.shape[1]
    dh = d // heads
    mk = _mask(mk, a.nnz, heads)
    C, lse = np.zeros((M, d)), np.full((M, heads), -np.inf)
    for i in range(M):
        lo, hi = a.indptr[i], a.indptr[i + 1]
        if lo == hi:
            continue
        for h in range(heads):
            s = []
            for j in a.indices[lo:hi]:
                z = U[i, h] + V[j, h]
                s.append(z if z > 0 else slope * z)
            tot = sum(np.exp(v - max(s)) for v in s)
            lse[i, h] = max(s) + np.log(tot)
            for e, (v, j) in enumerate(zip(s, a.indices[lo:hi])):
                C[i, h * dh:(h + 1) * dh] += mk[lo + e, h] * np.exp(v - lse[i, h]) * B[j, h * dh:(h + 1) * dh]
    return C, lse


def backward_loops(a, U, V, B, G, slope, heads=1, mk=None):
    """dict(dU, dV, dB, delta) by the definition, entry by entry in fp64"""
    a = a.tocsr()
    U, V, B, G = (np.asarray(t, np.float64) for t in (U, V, B, G))
    M, K = a.shape
    d = B.shape[1]
    dh = d // heads
    mk = _mask(mk, a.nnz, heads)
    C, lse = forward_loops(a, U, V, B, slope, heads, mk)
    dU, dV, dB, delta = np.zeros((M, heads)), np.zeros((K, heads)), np.zeros((K, d)), np.zeros((M, heads))
    for i in range(M):
        for h in range(heads):
            sl = slice(h * dh, (h + 1) * dh)
            delta[i, h] = float(np.dot(G[i, sl], C[i, sl]))
            for e in range(a.indptr[i], a.indptr[i + 1]):
                j = a.indices[e]
                z = U[i, h] + V[j, h]
                p = np.exp((z if z > 0 else slope * z) - lse[i, h])
                ee = p * (mk[e, h] * float(np.dot(G[i, sl], B[j, sl])) - delta[i, h])
                dz = ee * (1.0 if z > 0 else slope)
                dU[i, h] += dz
                dV[j, h] += dz
                dB[j, sl] += mk[e, h] * p * G[i, sl]
    return dict(dU=dU, dV=dV, dB=dB, delta=delta)


def backward_f64(a, U, V, B, G, slope, heads=1, mk=None, add=None, add_rows=0, values_only=False):
    """dict(dU, dV, dB, delta, bound_*) in fp64; dB includes the addend"""
    f = forward(a, U, V, B, slope, heads, mk, values_only)
    indptr, cols, rows, deg, shape, dh = f.indptr, f.cols, f.rows, f.deg, f.shape, f.dh
    M, K = shape
    B64, G64 = np.asarray(B, np.float64)[:K], np.asarray(G, np.float64)
    d = B64.shape[1]
    n, nT = deg.astype(np.float64), np.bincount(cols, minlength=K).astype(np.float64)
    csr = lambda v: _csr(v, cols, indptr, shape)
    out = dict(fwd=f, dU=np.zeros((M, heads)), dV=np.zeros((K, heads)), dB=np.zeros((K, d)), delta=np.zeros((M, heads)),
               bound_dU=np.zeros((M, heads)), bound_dV=np.zeros((K, heads)), bound_dB=np.zeros((K, d)),
               bound_delta=np.zeros((M, heads)))
    mkmax = float(f.mk.max()) if f.mk.size else 1.0
    for h in range(heads):
        sl = slice(h * dh, (h + 1) * dh)
        Bh, Gh, Ch = B64[:, sl], G64[:, sl], f.C[:, sl]
        absB, absG = np.abs(Bh), np.abs(Gh)
        p, z, s, mkh = f.p[h], f.z[h], f.s[h], f.mk[:, h]
        t = np.einsum('ek,ek->e', Gh[rows], Bh[cols]) if rows.size else np.zeros(0)
        gb = np.einsum('ek,ek->e', absG[rows], absB[cols]) if rows.size else np.zeros(0)
        delta = np.sum(Gh * Ch, axis=1)
        pmk = p * mkh
        bdelta = (dh + 2) * U_ * np.sum(absG * np.abs(Ch), axis=1) + np.sum(absG * f._tiny[h], axis=1) \
            + f.second * (_seg(np.add, pmk * (f.W[h] + f.Wbar[h][rows]) * np.abs(t), indptr, 0.0)
                          + (2 * n + 3) * U_ * _seg(np.add, pmk * gb, indptr, 0.0))
        diff = mkh * t - delta[rows]
        e = p * diff
        fac = leaky_d(z, f.slope)
        dz = e * fac
        out['delta'][:, h], out['bound_delta'][:, h] = delta, f.second * bdelta
        out['dU'][:, h] = _seg(np.add, dz, indptr, 0.0)
        out['dV'][:, h] = np.asarray(csr(dz).T.tocsr() @ np.ones(M)) if rows.size else 0.0
        pm = p * mkh
        out['dB'][:, sl] = np.asarray(csr(pm).T.tocsr() @ Gh)
        # ---- the bounds (module docstring) ----
        lse_rows = np.where(deg > 0, f.lse[:, h], 0.0)[rows]
        Pij = f.es[h] + f.bound_lse[rows, h] + np.abs(s - lse_rows) * U_ + C_EXP * U_
        Dij = mkh * (dh + 3) * U_ * gb + bdelta[rows] + U_ * np.abs(diff)
        Ee = p * (Pij * np.abs(diff) + Dij) + U_ * np.abs(e)
        Ez = Ee * fac + U_ * np.abs(dz)
        dmax = float(np.max(np.abs(diff))) if diff.size else 0.0
        out['bound_dU'][:, h] = f.second * (_seg(np.add, Ez, indptr, 0.0) + (n + 1) * U_ * _seg(np.add, np.abs(dz), indptr, 0.0)
                                            + n * 2.0 ** -125 * dmax)
        if rows.size:
            out['bound_dV'][:, h] = f.second * (np.asarray(csr(Ez).T.tocsr() @ np.ones(M))
                                                + (nT + 1) * U_ * np.asarray(csr(np.abs(dz)).T.tocsr() @ np.ones(M))
                                                + nT * 2.0 ** -125 * dmax)
        colmax = absG.max(axis=0)[None, :] if absG.shape[0] else np.zeros((1, dh))
        out['bound_dB'][:, sl] = f.second * (np.asarray(csr(pm * (Pij + U_)).T.tocsr() @ absG)
                                             + ((nT + 1) * U_)[:, None] * np.asarray(csr(pm).T.tocsr() @ absG)
                                             + nT[:, None] * 2.0 ** -125 * mkmax * colmax)
    if add is not None and add_rows > 0:
        r = int(add_rows)
        out['dB'][:r] += np.asarray(add, np.float64)[:r]
        out['bound_dB'][:r] += U_ * np.abs(out['dB'][:r])
    return out


def scores_bwd_f64(x, a, dU, dV, heads, dx0=None):
    """dict(da, bound_da, dx, bound_dx): the way back through the scores in fp64; dU may have fewer rows than dV"""
    x64, a64 = np.asarray(x, np.float64), np.asarray(a, np.float64)
    dU64, dV64 = np.asarray(dU, np.float64), np.asarray(dV, np.float64)
    rows, ru = dV64.shape[0], dU64.shape[0]
    d = x64.shape[1]
    dh = d // heads
    eU = np.zeros((rows, d))
    eU[:ru] = np.repeat(dU64, dh, axis=1)
    eV = np.repeat(dV64, dh, axis=1)
    xr = x64[:rows]
    da = np.stack([np.sum(eU * xr, axis=0), np.sum(eV * xr, axis=0)])
    gam = rows * U_ / (1 - rows * U_) if rows else 0.0
    bda = gam * np.stack([np.sum(np.abs(eU * xr), axis=0), np.sum(np.abs(eV * xr), axis=0)])
    out = dict(da=da, bound_da=bda)
    if dx0 is not None:
        dx0 = np.asarray(dx0, np.float64)[:rows]
        out['dx'] = dx0 + eU * a64[0] + eV * a64[1]
        out['bound_dx'] = 2 * U_ * (np.abs(dx0) + np.abs(eU * a64[0]) + np.abs(eV * a64[1])) * (1 + 4 * U_)
    return out


def layer_f64(a, x, avec, slope, heads, G=None, mk=None):
    """The whole chain in fp64 with B = x and the tables from (x, avec): dict(C, lse, S) and, given G, dX and da too"""
    a = a.tocsr()
    M, K = a.shape
    x64 = np.asarray(x, np.float64)
    S, _ = scores_f64(x64, avec, heads)
    f = forward(a, S[:M, :heads], S[:K, heads:], x64, slope, heads, mk, values_only=True)
    out = dict(C=f.C, lse=f.lse, S=S)
    if G is not None:
        b = backward_f64(a, S[:M, :heads], S[:K, heads:], x64, G, slope, heads, mk, values_only=True)
        dV = np.zeros((x64.shape[0], heads))
        dV[:K] = b['dV']
        dx0 = np.zeros_like(x64)
        dx0[:K] = b['dB']
        sb = scores_bwd_f64(x64, avec, b['dU'], dV, heads, dx0)
        out.update(dX=sb['dx'], da=sb['da'], dU=b['dU'], dV=b['dV'], dB=b['dB'])
    return out


# ---- fp32 restatements of the kernels' algorithm (what the bounds must accept) -------------------------------------------
def _pieces(js, reverse, cut):
    js = js[::-1] if reverse else js
    if cut and js.size > 1:
        return [js[:js.size // 2], js[js.size // 2:]]
    return [js]


def forward_online_f32(a, U, V, B, slope, heads=1, mk=None, reverse=False, cut=False):
    """(C, lse) in fp32 by the online softmax; ``reverse`` walks every row backwards, ``cut`` halves every row into two pieces
    that are merged as the fix-up merges slots"""
    f32 = np.float32
    a = a.tocsr()
    U, V, B, slope = np.asarray(U, f32), np.asarray(V, f32), np.asarray(B, f32), f32(slope)
    M, d = a.shape[0], B.shape[1]
    dh = d // heads
    mk = _mask(mk, a.nnz, heads).astype(f32)
    C, lse = np.zeros((M, d), f32), np.full((M, heads), -np.inf, f32)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        for i in range(M):
            lo, hi = a.indptr[i], a.indptr[i + 1]
            if lo == hi:
                continue
            for h in range(heads):
                sl = slice(h * dh, (h + 1) * dh)
                parts = []
                for piece in _pieces(np.arange(lo, hi), reverse, cut):
                    m, l, acc = f32(-np.inf), f32(0), np.zeros(dh, f32)
                    for e in piece:
                        j = a.indices[e]
                        z = f32(U[i, h] + V[j, h])
                        s = z if z > 0 else f32(slope * z)
                        if s > m:
                            alpha = np.exp(f32(m - s))
                            l, acc, m = f32(l * alpha), acc * alpha, s
                        p = np.exp(f32(s - m))
                        l, acc = f32(l + p), acc + f32(p * mk[e, h]) * B[j, sl]
                    parts.append((m, l, acc))
                m = max(x[0] for x in parts)
                l, acc = f32(0), np.zeros(dh, f32)
                for mq, lq, aq in parts:
                    sc = np.exp(f32(mq - m))
                    l, acc = f32(l + lq * sc), acc + sc * aq
                C[i, sl], lse[i, h] = acc / l, f32(np.float64(m) + np.log(np.float64(l)))
    return C, lse


def backward_f32(a, U, V, B, G, slope, C, lse, heads=1, mk=None, reverse=False, cut=False):
    """dict(dU, dV, dB, delta) in fp32 from an fp32 forward's C and lse, p and e recomputed per entry, the sums in the order /
    pieces of ``forward_online_f32``'s arguments"""
    f32 = np.float32
    a = a.tocsr()
    M, K = a.shape
    U, V, B, G, C, lse, slope = (np.asarray(t, f32) for t in (U, V, B, G, C, lse, slope))
    d = B.shape[1]
    dh = d // heads
    mk = _mask(mk, a.nnz, heads).astype(f32)
    coo_rows = np.repeat(np.arange(M), np.diff(a.indptr))
    order = np.lexsort((coo_rows, a.indices))               # entries by column, rows ascending
    tptr = np.concatenate([[0], np.cumsum(np.bincount(a.indices, minlength=K))])
    dU, dV, dB, delta = np.zeros((M, heads), f32), np.zeros((K, heads), f32), np.zeros((K, d), f32), np.zeros((M, heads), f32)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        for h in range(heads):
            sl = slice(h * dh, (h + 1) * dh)
            for i in range(M):
                delta[i, h] = f32(np.dot(G[i, sl], C[i, sl]))

            def pe(e):
                i, j = coo_rows[e], a.indices[e]
                z = f32(U[i, h] + V[j, h])
                s = z if z > 0 else f32(slope * z)
                p = np.exp(f32(s - lse[i, h]))
                t = f32(np.dot(G[i, sl], B[j, sl]))
                ee = f32(p * f32(f32(mk[e, h] * t) - delta[i, h]))
                return p, f32(ee * (f32(1) if z > 0 else slope))
            for i in range(M):
                tot = f32(0)
                for piece in _pieces(np.arange(a.indptr[i], a.indptr[i + 1]), reverse, cut):
                    acc = f32(0)
                    for e in piece:
                        acc = f32(acc + pe(e)[1])
                    tot = f32(tot + acc)
                dU[i, h] = tot
            for j in range(K):
                tot, totv = np.zeros(dh, f32), f32(0)
                for piece in _pieces(order[tptr[j]:tptr[j + 1]], reverse, cut):
                    acc, accv = np.zeros(dh, f32), f32(0)
                    for e in piece:
                        p, dz = pe(e)
                        acc = acc + f32(p * mk[e, h]) * G[coo_rows[e], sl]
                        accv = f32(accv + dz)
                    tot, totv = tot + acc, f32(totv + accv)
                dB[j, sl], dV[j, h] = tot, totv
    return dict(dU=dU, dV=dV, dB=dB, delta=delta)
