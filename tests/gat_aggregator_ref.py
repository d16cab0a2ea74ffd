"""An independent restatement of a plain layer stack under --aggregator attn --attn_score gat -- a test-only helper.

``GatModel`` is attn_dropout_cases.DropModel (heads, coefficient masks keyed by (seed, layer position, step), fp64-accumulating
dense layers) with its aggregation restated: every aggregation layer owns ``agg<l>/attn_vec`` of shape (2, d), d its own input
width, and computes tests/spgat_ref.py's definition in fp64 from its fp32 input and vectors -- the scores u, v, the LeakyReLU of
their sum at --attn_slope (as the fp32 number the kernel receives), the softmax, the masked weighted sum -- rounded to fp32
once; its backward is spgat_ref.layer_f64's dX (+ the self half under concat) and da, rounded once.  attn_vec is
glorot-initialised from the case's seed, carries no weight decay (oracle.model_np.Model._wd_names names the first DENSE layer) and
goes through the oracle's own Adam with every other parameter.

``forward`` records, beside the ReLU margins of attn_aggregator_ref, what the second well-posedness condition needs
(gat_aggregator_cases): over the stored entries of every aggregation layer and every head, the smallest |z_ij| / ez_ij, where
    ez_ij = (dh + 1) u (sum_{c in h} |x[i,c] a[0,c]| + sum_{c in h} |x[j,c] a[1,c]|) + u |z_ij|
is the derived fp32 error bound of z (two dh-term dot products in any order, one addition; tests/spgat_ref.py)."""
import numpy as np
import scipy.sparse as sp

import spgat_ref
from attn_aggregator_ref import _mm, f32
from attn_dropout_cases import DropModel
from oracle import model_np as mnp
from oracle import oracle_np as onp

U = spgat_ref.U_


def init_attn_vecs(params, flags, preprocess, input_dim, L, seed):
    """agg<l>/attn_vec (2, d) glorot-uniform from a stream of its own (seed + 1000), added to ``params``"""
    rng = np.random.RandomState(seed + 1000)
    for l in range(L):
        d = (flags['hidden1'] if preprocess else input_dim) if l == 0 else flags['hidden1']
        lim = np.sqrt(6.0 / (2 + d))
        params['agg%d/attn_vec' % l] = rng.uniform(-lim, lim, (2, d)).astype(f32)
    return params


class GatModel(DropModel):
    attn_slope = 0.2

    def _slope(self):
        return float(f32(self.attn_slope))

    def forward(self, feed, ph, dropout, masks):
        fl, keep = self.flags, 1.0 - dropout
        concat = fl['normalization'] != 'gcn'
        assert not (self.cv or self.cvd or fl['det_dropout'] or sp.issparse(self.features)), "plain dense-input stacks only"
        act = self.features[feed[ph['fields'][0]]]
        tape, acts = [], []
        self.margins = []                 # (kind, layer, smallest non-zero |input|, largest input magnitude)
        self.zratios = []                 # (layer, smallest |z| / its derived fp32 error bound)
        for li, s in enumerate(self.specs):
            kind = s[0]
            if kind == 'dropout':
                m = masks('L%d' % li, act.shape) if dropout > 0 else None
                act = mnp.dropout_fwd(act, keep, m)
                tape.append(('dropout', m, keep))
            elif kind == 'dense':
                _, name, fin, fout, sparse_in, relu, norm = s
                assert not sparse_in
                y = _mm(act, self.params[name + '/weights'])
                ctx = None
                if norm:
                    y, ctx = mnp.layer_norm_fwd(y, self.params[name + '/offset'], self.params[name + '/scale'])
                pre = y
                if relu:
                    nz = np.abs(pre[pre != 0])
                    self.margins.append(('relu', li, float(nz.min()) if nz.size else np.inf, float(np.abs(pre).max())))
                    y = np.maximum(y, 0).astype(f32)
                tape.append(('dense', s, act, ctx, pre))
                act = y
            elif kind == 'agg':
                adj = onp.coo_to_csr(feed[ph['adj'][s[1]]])
                d, H = act.shape[1], self.heads
                assert adj.shape[0] == adj.shape[1] == act.shape[0] and d % H == 0
                a = self.params['agg%d/attn_vec' % s[1]]
                assert a.shape == (2, d) and a.dtype == f32
                mk = self._mask(adj, li)
                out = spgat_ref.layer_f64(adj, act, a, self._slope(), H, mk=mk)
                C = out['C'].astype(f32)
                # the second condition's figure: |z| against its derived fp32 error bound, per stored entry and head
                S, bS = spgat_ref.scores_f64(act, a, H)
                rows = np.repeat(np.arange(adj.shape[0]), np.diff(adj.indptr))
                z = S[rows, :H] + S[adj.indices, H:]
                ez = bS[rows, :H] + bS[adj.indices, H:] + U * np.abs(z)
                # (ez == 0: every product of both dot products is exactly 0 -- a dead input row --, and z is exactly 0 in fp32 too)
                with np.errstate(divide='ignore', invalid='ignore'):
                    ratio = np.where(ez > 0, np.abs(z) / ez, np.inf)
                self.zratios.append((li, float(np.min(ratio)) if z.size else np.inf))
                tape.append(('agg', adj, act, a, concat, d, mk, s[1]))
                act = np.hstack([act[:adj.shape[0]], C]).astype(f32) if concat else C
            else:
                raise NotImplementedError(kind)
            acts.append(act)
        self._tape = tape
        return act, acts

    def backward(self, dout):
        grads = {k: np.zeros_like(v) for k, v in self.params.items()}
        g = dout
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
                grads[name + '/weights'] += _mm(xin.T, g)
                g = _mm(g, self.params[name + '/weights'].T)
            elif kind == 'dropout':
                _, m, keep = rec
                if m is not None:
                    g = (g * (m * f32(1.0 / keep))).astype(f32)
            elif kind == 'agg':
                _, adj, x, a, concat, d, mk, l = rec
                out = spgat_ref.layer_f64(adj, x, a, self._slope(), self.heads, g[:, d:] if concat else g, mk)
                dX = out['dX']
                if concat:
                    dX = dX + np.asarray(g[:, :d], np.float64)
                grads['agg%d/attn_vec' % l] += out['da'].astype(f32)
                g = dX.astype(f32)
        wd = f32(self.flags['weight_decay'])
        for k in self._wd_names():
            grads[k] += wd * self.params[k]
        return grads
