"""attn_aggregator_ref.AttnModel restated with --attn_heads -- a test-only helper.

Same structure: every aggregation is the MULTI-HEAD attention of tests/spattn_heads_ref.py over the adjacency's stored pattern
with the layer's own input as queries, keys and values; the scale is --attn_scale, 0 meaning 1 / sqrt(d / heads) of the
layer's input width d (as fp32); every matrix product accumulates in fp64 and is rounded to fp32 once; the backward of an
attention layer is spattn_heads_ref.backward_f64's fused gradient, rounded once.  Everything else is the oracle's own."""
import numpy as np
import scipy.sparse as sp

import spattn_heads_ref as href
from attn_aggregator_ref import AttnModel, _mm, f32, layer_scale
from oracle import model_np as mnp
from oracle import oracle_np as onp


class HeadsModel(AttnModel):
    heads = 1

    def forward(self, feed, ph, dropout, masks):
        fl, keep = self.flags, 1.0 - dropout
        concat = fl['normalization'] != 'gcn'
        assert not (self.cv or self.cvd or fl['det_dropout'] or sp.issparse(self.features)), "plain dense-input stacks only"
        act = self.features[feed[ph['fields'][0]]]
        tape, acts = [], []
        self.margins = []                 # (kind, layer, smallest non-zero |input|, largest input magnitude)
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
                d = act.shape[1]
                assert adj.shape[0] == adj.shape[1] == act.shape[0] and d % self.heads == 0
                scale = layer_scale(d // self.heads, self.attn_scale)
                C = href.forward(adj, act, act, scale, self.heads).C.astype(f32)
                tape.append(('agg', adj, act, scale, concat, d))
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
                _, adj, x, scale, concat, d = rec
                if concat:
                    g = href.backward_f64(adj, x, x, g[:, d:], scale, self.heads, add=g[:, :d], add_rows=adj.shape[0],
                                          fused=True)['dx'].astype(f32)
                else:
                    g = href.backward_f64(adj, x, x, g, scale, self.heads, fused=True)['dx'].astype(f32)
        wd = f32(self.flags['weight_decay'])
        for k in self._wd_names():
            grads[k] += wd * self.params[k]
        return grads


def model_class(heads):
    return type('HeadsModel%d' % heads, (HeadsModel,), dict(heads=int(heads)))
