"""An fp64 NumPy statement of the two-table attention (sgcn_spattn_pull.hip) and of the estimator it serves,
--full_batch_part_pull with --aggregator attn -- a test-only helper.

The kernels, for the selected rows ids of the RESIDENT adjacency a (values never read) and per stored entry e of row ids[i]
with c = col[e]:   B_e = X[map[c]] if map[c] >= 0 else H[c]   and per head
    s_e = scale <X[i], B_e>,  lse_i = log sum_e exp(s_e),  p_e = exp(s_e - lse_i),  C[i] = sum_e p_e B_e
    delta_i = <G[i], C[i]>,   e_e = p_e (<G[i], B_e> - delta_i)
    dQ[i] = scale sum_e e_e B_e                                   over ALL stored entries
    dB[j] = sum_i ( p_ij G[i] + scale e_ij X[i] )                 over IN-PART entries only (stored rows are constants)
    dX    = dQ + dB (+ the addend)

  operands, forward, backward   by tests/spattn_heads_ref.py on (the pattern a[ids], Q = X, B = part_history_ref.merged(ids, X,
                                H)): its values and its DERIVED bounds; backward's dX is dQ + dB[ids]
  loops                         the same numbers by another road, entry by entry (tiny graphs), for tests/test_part_pull.py to
                                hold ``backward`` to -- and, under ``mutant``, three wrong kernels the comparison must reject:
                                'softmax_in_part' (the normaliser over in-part entries only: --full_batch_parts without the
                                flag), 'stale_in_part' (stored rows read for in-part columns), 'dq_in_part' (the query's
                                gradient over in-part entries only)

The estimator: ``PartPullAttnModel`` is part_history_ref.PartHistoryModel with the aggregation restated as that attention over
(a[ids], act, merged table) with the layer scale of attn_heads_ref (1 / sqrt(d / heads) as fp32 where --attn_scale is 0); its
backward is dQ + dB[ids], rounded once.  Push, refresh, bfloat16 rounding on the push, LayerNorm, masks, loss and Adam are
inherited, not copied."""
import numpy as np

import part_history_ref as pr
import spattn_heads_ref as href
from attn_aggregator_ref import layer_scale
from oracle import model_np as mnp

f32 = np.float32
MUTANTS = ('softmax_in_part', 'stale_in_part', 'dq_in_part')


# ---- the kernels --------------------------------------------------------------------------------------------------------
def operands(a, ids, X, H):
    """(the n x N pattern of the selected rows, the merged table): what the one-table definition runs on"""
    ids = np.asarray(ids, dtype=np.int64)
    sub = a.tocsr()[ids].tocsr()
    sub.sort_indices()
    return sub, pr.merged(ids, X, H)


def forward(a, ids, X, H, scale, heads=1, values_only=False):
    """spattn_heads_ref.Forward: C (n x d), lse (n x heads), bound_C, bound_lse"""
    sub, Z = operands(a, ids, X, H)
    return href.forward(sub, np.asarray(X, np.float64), Z, scale, heads, values_only=values_only)


def backward(a, ids, X, H, G, scale, heads=1, add=None, add_rows=0, values_only=False):
    """dict(dQ, bound_dQ: n x d, the addend included; dB, bound_dB: N x d over ALL entries, of which only the rows ids are the
    estimator's; dX = dQ + dB[ids]; fwd)"""
    ids = np.asarray(ids, dtype=np.int64)
    sub, Z = operands(a, ids, X, H)
    r = href.backward_f64(sub, np.asarray(X, np.float64), Z, G, scale, heads, add=add, add_rows=add_rows, values_only=values_only)
    r['dX'] = r['dQ'] + r['dB'][ids]
    return r


def loops(a, ids, X, H, G, scale, heads=1, mutant=None):
    """(C, lse, dQ, dX) entry by entry in fp64; ``mutant``: one of MUTANTS, or None for the definition"""
    assert mutant is None or mutant in MUTANTS
    a = a.tocsr()
    ids = np.asarray(ids, dtype=np.int64)
    X, H, G = (np.asarray(t, np.float64) for t in (X, H, G))
    m = pr.position_map(a.shape[0], ids)
    n, d = X.shape
    C, lse, dQ, dB = np.zeros((n, d)), np.full((n, heads), -np.inf), np.zeros((n, d)), np.zeros((n, d))
    for i, v in enumerate(ids):
        cols = [int(c) for c in a.indices[a.indptr[v]:a.indptr[v + 1]]]
        if mutant == 'softmax_in_part':
            cols = [c for c in cols if m[c] >= 0]
        if not cols:
            continue
        for h, sl in enumerate(href.head_slices(d, heads)):
            rows = [(H[c] if (m[c] < 0 or mutant == 'stale_in_part') else X[m[c]])[sl] for c in cols]
            s = [float(scale) * float(np.dot(X[i, sl], b)) for b in rows]
            top = max(s)
            lse[i, h] = top + np.log(sum(np.exp(v_ - top) for v_ in s))
            p = [np.exp(v_ - lse[i, h]) for v_ in s]
            for pe, b in zip(p, rows):
                C[i, sl] += pe * b
            delta = float(np.dot(G[i, sl], C[i, sl]))
            for c, pe, b in zip(cols, p, rows):
                e = pe * (float(np.dot(G[i, sl], b)) - delta)
                inside = m[c] >= 0
                if inside or mutant != 'dq_in_part':
                    dQ[i, sl] += float(scale) * e * b
                if inside:
                    dB[m[c], sl] += pe * G[i, sl] + float(scale) * e * X[i, sl]
    return C, lse, dQ, dQ + dB


# ---- the estimator ------------------------------------------------------------------------------------------------------
class PartPullAttnModel(pr.PartHistoryModel):
    heads, attn_scale = 1, 0.0

    def forward_part(self, ids, dropout, masks, stop_at_last_agg=False):
        fl, keep = self.flags, 1.0 - dropout
        concat = fl['normalization'] != 'gcn'
        ids = np.asarray(ids, dtype=np.int64)
        act = self.features[ids]
        tape, acts, self.pushed = [], [], {}
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
                if stop_at_last_agg and li == last_agg:
                    self.push(l, ids, act)
                    self.pushed[l] = act
                    break
                d = act.shape[1]
                assert d % self.heads == 0
                scale = layer_scale(d // self.heads, self.attn_scale)
                table = np.array(self.table(l), dtype=f32, copy=True)       # as the forward saw it: the backward re-reads it
                C = forward(self.resident, ids, act, table, scale, self.heads).C.astype(f32)
                self.push(l, ids, act)                    # push after pull: columns in S never read the table
                self.pushed[l] = act
                tape.append(('agg', ids, act, table, scale, concat, d))
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
                _, ids, x, table, scale, concat, d = rec
                kw = dict(add=g[:, :d], add_rows=len(ids)) if concat else {}
                g = backward(self.resident, ids, x, table, g[:, d:] if concat else g, scale, self.heads, **kw)['dX'].astype(f32)
            self.gtrace.append((kind, g))
        wd = f32(self.flags['weight_decay'])
        for k in self._wd_names():
            grads[k] += wd * self.params[k]
        return grads


def model_class(heads, attn_scale=0.0):
    return type('PartPullAttnModel%d' % heads, (PartPullAttnModel,), dict(heads=int(heads), attn_scale=float(attn_scale)))


def make_model(case, heads=1, seed=None, params=None, bf16=False):
    """the PartPullAttnModel of a case dict of attn_aggregator_cases.build, attached to its training adjacency"""
    cls = model_class(heads)
    fl = case['flags']
    seed = case['cfg']['init'] if seed is None else seed
    args = (fl, fl['num_layers'], fl['preprocess'], False, False, case['feats'], case['nbr_train'], case['n'], case['classes'])
    if params is None:
        params = mnp.init_params(cls(*args, {}).specs, seed)
    return cls(*args, params).attach(case['train_adj'], bf16=bf16)
