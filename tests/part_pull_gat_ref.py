"""An fp64 NumPy statement of the two-table attention with learned additive scores (sgcn_spgat_pull.hip) and of the estimator
it serves, --full_batch_part_pull_gat -- a test-only helper.

The kernels, for the selected rows ids of the RESIDENT adjacency a (values never read) and per stored entry e of row ids[i]
with c = col[e], m = map[c], per head h:
    B_e = X[m] if m >= 0 else T[c]          v_e = V[m, h] if m >= 0 else VH[c, h]
    z_e = U[i, h] + v_e,  s_e = leaky(z_e),  lse_i = log sum_e exp(s_e),  p_e = exp(s_e - lse_i),  C[i] = sum_e p_e B_e
    delta_i = <G[i], C[i]>_h,   e_e = p_e (<G[i], B_e>_h - delta_i),   dz_e = e_e leaky'(z_e)
    dU[i, h] = sum_e dz_e                                       over ALL stored entries
    dB[j] = sum_i p_ij G[i],   dV[j, h] = sum_i dz_ij           over IN-PART entries only (stored rows and scores are constants)
    dX = dB + dU a[0] + dV a[1] (+ the addend),   da[0] = sum_r dU[r] x[r],   da[1] = sum_r dV[r] x[r]

  operands, forward, backward_tables   by tests/spgat_ref.py on (the pattern a[ids], U, V_m = VH with the rows of S replaced by V,
                                B = part_pull_attn_ref.operands' merged table): its values and its DERIVED bounds; the
                                estimator's dB and dV are the rows ids of the one-table dB and dV (a column inside S collects
                                exactly the in-part entries of the selected rows)
  backward                      the whole layer from (X, a): the scores in fp64, backward_tables, then spgat_ref.scores_bwd_f64
  loops                         the same numbers by another road, entry by entry (tiny graphs), for tests/test_part_pull_gat.py
                                to hold ``backward`` to -- and, under ``mutant``, four wrong estimators the comparison must
                                reject: 'recompute_scores' (stale scores recomputed from T[c] with the current a), 'du_in_part'
                                (dU over in-part entries only), 'da1_stale' (da[1] -- and dX through dV -- with a share of the
                                stale entries), 'push_before_pull' (the score table holds the fresh V before the pull)

The estimator: ``PartPullGatModel`` is part_history_ref.PartHistoryModel with the aggregation restated as that attention, one
score table per aggregation layer (N x heads, fp32, zero at the start, ALWAYS owned) and gat_aggregator_ref's parameters
(agg<l>/attn_vec, glorot from a stream of its own).  The scores a layer computes and pushes are the fp64 scores rounded to
fp32 once.  Push, refresh, bfloat16 rounding of the ROWS on the push, LayerNorm, masks, loss and Adam are inherited."""
import numpy as np

import part_history_ref as pr
import part_pull_attn_ref as ar
import spgat_ref as gr
from gat_aggregator_ref import init_attn_vecs
from oracle import model_np as mnp

f32 = np.float32
MUTANTS = ('recompute_scores', 'du_in_part', 'da1_stale', 'push_before_pull')


# ---- the kernels --------------------------------------------------------------------------------------------------------
def operands(a, ids, X, T, V, VH):
    """(the n x N pattern of the selected rows, the merged row table, the merged destination-score table)"""
    sub, Z = ar.operands(a, ids, X, T)
    return sub, Z, pr.merged(ids, V, VH)


def forward(a, ids, X, T, U, V, VH, slope, heads=1, values_only=False):
    """spgat_ref.Forward on the merged tables: C (n x d), lse (n x heads), bound_C, bound_lse"""
    sub, Z, Vm = operands(a, ids, X, T, V, VH)
    return gr.forward(sub, np.asarray(U, np.float64), Vm, Z, slope, heads, values_only=values_only)


def backward_tables(a, ids, X, T, U, V, VH, G, slope, heads=1, add=None, add_rows=0, values_only=False):
    """dict(delta, dU: n x heads over ALL entries; dB: n x d (the addend included) and dV: n x heads over IN-PART entries; their
    bound_*; fwd) from the score tables as given"""
    ids = np.asarray(ids, dtype=np.int64)
    sub, Z, Vm = operands(a, ids, X, T, V, VH)
    r = gr.backward_f64(sub, np.asarray(U, np.float64), Vm, Z, G, slope, heads, values_only=values_only)
    out = dict(fwd=r['fwd'], delta=r['delta'], bound_delta=r['bound_delta'], dU=r['dU'], bound_dU=r['bound_dU'],
               dB=r['dB'][ids].copy(), bound_dB=r['bound_dB'][ids].copy(), dV=r['dV'][ids].copy(), bound_dV=r['bound_dV'][ids].copy())
    if add is not None and add_rows > 0:
        k = int(add_rows)
        out['dB'][:k] += np.asarray(add, np.float64)[:k]
        out['bound_dB'][:k] += gr.U_ * np.abs(out['dB'][:k])
    return out


def backward(a, ids, X, T, VH, avec, G, slope, heads=1, add=None, add_rows=0, S=None, values_only=True):
    """The whole layer: dict(C, lse, S, dU, dV, dB, dX, da and, with ``values_only=False``, bound_dX / bound_da).  ``S``: the
    fresh score table to use (n x 2 heads; default: the fp64 scores of (X, avec)) -- a device test hands over the table its
    own launch produced, as the kernels take their tables as given."""
    X64 = np.asarray(X, np.float64)
    if S is None:
        S, _ = gr.scores_f64(X64, avec, heads)
    S = np.asarray(S, np.float64)
    U, V = S[:, :heads], S[:, heads:]
    b = backward_tables(a, ids, X, T, U, V, VH, G, slope, heads, add=add, add_rows=add_rows, values_only=values_only)
    sb = gr.scores_bwd_f64(X64, avec, b['dU'], b['dV'], heads, b['dB'])
    out = dict(C=b['fwd'].C, lse=b['fwd'].lse, S=S, dU=b['dU'], dV=b['dV'], dB=b['dB'], dX=sb['dx'], da=sb['da'], fwd=b['fwd'])
    if not values_only:
        # the bounds summed: every term of dX and da with the bound of the factor the pattern kernels produced
        a64 = np.abs(np.asarray(avec, np.float64))
        dh = X64.shape[1] // heads
        eU, eV = np.repeat(b['bound_dU'], dh, axis=1), np.repeat(b['bound_dV'], dh, axis=1)
        out['bound_dX'] = b['bound_dB'] + eU * a64[0] + eV * a64[1] + sb['bound_dx'] + gr.U_ * np.abs(sb['dx'])
        n = X64.shape[0]
        gam = 1.0 + n * gr.U_ / (1 - n * gr.U_)
        out['bound_da'] = sb['bound_da'] + gam * np.stack([np.sum(eU * np.abs(X64), axis=0), np.sum(eV * np.abs(X64), axis=0)])
    return out


def loops(a, ids, X, T, VH, avec, G, slope, heads=1, mutant=None):
    """(C, lse, dU, dX, da) of the whole layer entry by entry in fp64; ``mutant``: one of MUTANTS, or None"""
    assert mutant is None or mutant in MUTANTS
    a = a.tocsr()
    ids = np.asarray(ids, dtype=np.int64)
    X, T, VH, G, avec = (np.asarray(t, np.float64) for t in (X, T, VH, G, avec))
    VH = VH.copy()
    m = pr.position_map(a.shape[0], ids)
    n, d = X.shape
    dh = d // heads
    U = np.stack([[float(np.dot(X[i, h * dh:(h + 1) * dh], avec[0, h * dh:(h + 1) * dh])) for h in range(heads)] for i in range(n)])
    V = np.stack([[float(np.dot(X[i, h * dh:(h + 1) * dh], avec[1, h * dh:(h + 1) * dh])) for h in range(heads)] for i in range(n)])
    if mutant == 'push_before_pull':
        VH[ids] = V
    C, lse = np.zeros((n, d)), np.full((n, heads), -np.inf)
    dU, dV, dB = np.zeros((n, heads)), np.zeros((n, heads)), np.zeros((n, d))
    dVstale = np.zeros((a.shape[0], heads))       # what a wrong estimator would send back through stale scores
    for i, v in enumerate(ids):
        cols = [int(c) for c in a.indices[a.indptr[v]:a.indptr[v + 1]]]
        if not cols:
            continue
        for h in range(heads):
            sl = slice(h * dh, (h + 1) * dh)
            rows = [(X[m[c]] if m[c] >= 0 else T[c])[sl] for c in cols]
            vs = []
            for c in cols:
                if m[c] >= 0:
                    vs.append(V[m[c], h])
                elif mutant == 'recompute_scores':
                    vs.append(float(np.dot(T[c, sl], avec[1, sl])))
                else:
                    vs.append(VH[c, h])
            z = [U[i, h] + v_ for v_ in vs]
            s = [z_ if z_ > 0 else slope * z_ for z_ in z]
            top = max(s)
            lse[i, h] = top + np.log(sum(np.exp(s_ - top) for s_ in s))
            p = [np.exp(s_ - lse[i, h]) for s_ in s]
            for pe, b in zip(p, rows):
                C[i, sl] += pe * b
            delta = float(np.dot(G[i, sl], C[i, sl]))
            for c, pe, b, z_ in zip(cols, p, rows, z):
                dz = pe * (float(np.dot(G[i, sl], b)) - delta) * (1.0 if z_ > 0 else slope)
                inside = m[c] >= 0
                if inside or mutant != 'du_in_part':
                    dU[i, h] += dz
                if inside:
                    dV[m[c], h] += dz
                    dB[m[c], sl] += pe * G[i, sl]
                else:
                    dVstale[c, h] += dz
    dX, da = dB.copy(), np.zeros((2, d))
    for h in range(heads):
        sl = slice(h * dh, (h + 1) * dh)
        dX[:, sl] += dU[:, [h]] * avec[0, sl] + dV[:, [h]] * avec[1, sl]
        da[0, sl] = (dU[:, [h]] * X[:, sl]).sum(axis=0)
        da[1, sl] = (dV[:, [h]] * X[:, sl]).sum(axis=0)
        if mutant == 'da1_stale':
            da[1, sl] += (dVstale[:, [h]] * T[:, sl]).sum(axis=0)
    return C, lse, dU, dX, da


# ---- the estimator ------------------------------------------------------------------------------------------------------
class PartPullGatModel(pr.PartHistoryModel):
    heads, attn_slope = 1, 0.2

    def attach(self, resident, bf16=False):
        super(PartPullGatModel, self).attach(resident, bf16=bf16)
        self.scores = [np.zeros((resident.shape[0], self.heads), f32) for _ in range(self.L)]
        return self

    def _slope(self):
        return float(f32(self.attn_slope))

    def _scores(self, act, l):
        """the layer's fresh score table (n x 2 heads), the fp64 scores rounded to fp32 once"""
        return gr.scores_f64(act, self.params['agg%d/attn_vec' % l], self.heads)[0].astype(f32)

    def _record_z(self, l, f, ids, act, vh):
        """(layer, smallest |z_e|, largest |z_e|, dead) over the stored entries of every head.  A DEAD entry is one whose z
        has no non-zero term at all -- every product x[i, c] a[0, c] of its source score is exactly 0 (a row the ReLU in
        front zeroed across the head) and its destination score likewise, or a stored 0 -- so that z_e is exactly 0 in every
        arithmetic and the LeakyReLU's branch (slope, at z == 0) is determined: dead entries are counted, not held to a
        margin, as gat_aggregator_ref.py leaves them out of its own condition."""
        H = self.heads
        mag = gr.scores_f64(np.abs(act), np.abs(self.params['agg%d/attn_vec' % l]), H)[0]
        m = pr.position_map(self.resident.shape[0], ids)[f.cols]
        small, big, dead = np.inf, 0.0, 0
        for h in range(H):
            vmag = np.where(m >= 0, mag[np.maximum(m, 0), H + h], np.abs(np.asarray(vh, np.float64)[f.cols, h]))
            live = (mag[f.rows, h] + vmag) > 0
            z = np.abs(f.z[h])
            assert not z[~live].any()
            dead += int((~live).sum())
            if live.any():
                small, big = min(small, float(z[live].min())), max(big, float(z.max()))
        self.zmargins.append((l, small, big, dead))

    def push_scores(self, l, ids, S):
        self.scores[l][np.asarray(ids, np.int64)] = S[:, self.heads:]

    def forward_part(self, ids, dropout, masks, stop_at_last_agg=False):
        fl, keep = self.flags, 1.0 - dropout
        concat = fl['normalization'] != 'gcn'
        ids = np.asarray(ids, dtype=np.int64)
        act = self.features[ids]
        tape, acts, self.pushed, self.pushed_scores = [], [], {}, {}
        self.zmargins = []                # _record_z's tuples, one per aggregation layer
        last_agg = max(li for li, s in enumerate(self.specs) if s[0] == 'agg')
        for li, s in enumerate(self.specs):
            kind = s[0]
            if kind == 'dropout':
                m = masks('L%d' % li, act.shape) if dropout > 0 else None
                act = mnp.dropout_fwd(act, keep, m)
                tape.append(('dropout', m, keep))
            elif kind == 'dense':
                _, name, fin, fout, sparse_in, relu, norm = s
                assert not sparse_in
                y = pr._mm(act, self.params[name + '/weights'])
                ctx = None
                if norm:
                    y, ctx = mnp.layer_norm_fwd(y, self.params[name + '/offset'], self.params[name + '/scale'])
                pre = y
                if relu:
                    y = np.maximum(y, 0).astype(f32)
                tape.append(('dense', s, act, ctx, pre))
                act = y
            elif kind == 'agg':
                l = s[1]
                d = act.shape[1]
                assert d % self.heads == 0
                S = self._scores(act, l)
                if stop_at_last_agg and li == last_agg:
                    self.push(l, ids, act)
                    self.push_scores(l, ids, S)
                    self.pushed[l], self.pushed_scores[l] = act, S[:, self.heads:]
                    break
                table = np.array(self.table(l), dtype=f32, copy=True)       # as the forward saw them: the backward re-reads
                vh = self.scores[l].copy()
                f = forward(self.resident, ids, act, table, S[:, :self.heads], S[:, self.heads:], vh, self._slope(), self.heads,
                            values_only=True)
                self._record_z(l, f, ids, act, vh)
                C = f.C.astype(f32)
                self.push(l, ids, act)                    # push after pull: columns in S never read either table
                self.push_scores(l, ids, S)
                self.pushed[l], self.pushed_scores[l] = act, S[:, self.heads:]
                tape.append(('agg', ids, act, table, vh, S, concat, d, l))
                act = np.hstack([act, C]).astype(f32) if concat else C
            else:
                raise NotImplementedError(kind)
            acts.append(act)
        self._tape = tape
        return act, acts

    def backward(self, dout):
        grads = {k: np.zeros_like(v) for k, v in self.params.items()}
        g = dout
        self.gtrace = []
        for rec in reversed(self._tape):
            kind = rec[0]
            if kind == 'dense':
                _, s, xin, ctx, pre = rec
                _, name, fin, fout, sparse_in, relu, norm = s
                if relu:
                    g = (g * self._gate(name, pre)).astype(f32)
                if norm:
                    g, doff, dsc = mnp.layer_norm_bwd(g, ctx, self.params[name + '/scale'])
                    grads[name + '/offset'] += doff
                    grads[name + '/scale'] += dsc
                grads[name + '/weights'] += pr._mm(xin.T, g)
                g = pr._mm(g, self.params[name + '/weights'].T)
            elif kind == 'dropout':
                _, m, keep = rec
                if m is not None:
                    g = (g * (m * f32(1.0 / keep))).astype(f32)
            elif kind == 'agg':
                _, ids, x, table, vh, S, concat, d, l = rec
                kw = dict(add=g[:, :d], add_rows=len(ids)) if concat else {}
                out = backward(self.resident, ids, x, table, vh, self.params['agg%d/attn_vec' % l], g[:, d:] if concat else g,
                               self._slope(), self.heads, S=S, **kw)
                grads['agg%d/attn_vec' % l] += out['da'].astype(f32)
                g = out['dX'].astype(f32)
            self.gtrace.append((kind, g))
        wd = f32(self.flags['weight_decay'])
        for k in self._wd_names():
            grads[k] += wd * self.params[k]
        return grads

    def z_margin(self):
        """the smallest live |z_e| / its layer's largest |z_e| over the last forward (the LeakyReLU's derivative jumps at 0)"""
        return min([np.inf] + [small / big for _, small, big, _ in self.zmargins if big > 0])


def model_class(heads, slope=0.2):
    return type('PartPullGatModel%d' % heads, (PartPullGatModel,), dict(heads=int(heads), attn_slope=float(slope)))


def make_model(case, heads=1, seed=None, params=None, bf16=False, slope=0.2):
    """the PartPullGatModel of a case dict of attn_aggregator_cases.build, attached to its training adjacency"""
    cls = model_class(heads, slope)
    fl = case['flags']
    seed = case['cfg']['init'] if seed is None else seed
    args = (fl, fl['num_layers'], fl['preprocess'], False, False, case['feats'], case['nbr_train'], case['n'], case['classes'])
    if params is None:
        probe = cls(*args, {})
        params = mnp.init_params(probe.specs, seed)
        init_attn_vecs(params, fl, fl['preprocess'], case['feats'].shape[1], probe.L, seed)
    return cls(*args, params).attach(case['train_adj'], bf16=bf16)
