"""The end-to-end cases of --attn_dropout (tests/test_attn_dropout_model_gpu.py) and their reference model -- test-only.

    sage_ln_pp_p2      attn_aggregator_cases' graphsage / LayerNorm / pre-processed stack, one head, --attn_dropout 0.2
    gcn_nopp_h2_p2     its gcn stack without pre-processing (every aggregation is attention), --attn_heads 2, --attn_dropout 0.2

``DropModel`` is attn_heads_ref.HeadsModel with the coefficient mask of tests/spattn_drop_ref.py in every attention layer of a
TRAINING model: the key of the layer at position li of the layer list is attn_key(seed, li, step) -- seed and step are the ones
that key the step's activation dropout -- and keep = 1 - P as the fp32 number the kernel receives.  An evaluation model
(is_training False) never masks.  The forward and the backward are spattn_drop_ref's fp64 evaluation, rounded once.

Well-posedness is the CONDITION of attn_aggregator_cases.py, unchanged and with the mask applied: ``init`` is the first seed
of 3 .. 12 for which, over three reference steps on the CPU, every non-zero |ReLU input| is at least MARGIN = 1e-4 of its
layer's largest.  tests/test_spattn_drop.py asserts that the entries below are the scan's answers."""
import numpy as np
import scipy.sparse as sp

import attn_aggregator_cases as ax
import full_batch_cases as fc
import spattn_drop_ref as dref
from attn_aggregator_ref import _mm, f32, layer_scale
from attn_heads_ref import HeadsModel
from oracle import model_np as mnp
from oracle import oracle_np as onp

MARGIN = ax.MARGIN
SEEDS = ax.SEEDS
P = 0.2

CASES = {
    'sage_ln_pp_p2': dict(base='sage_ln_pp', heads=1, init=3),
    'gcn_nopp_h2_p2': dict(base='gcn_nopp', heads=2, init=3),
}


class DropModel(HeadsModel):
    attn_dropout = 0.0
    drop_seed, drop_step = 1, 0            # the device model's dropout_seed / dropout_step of the step at hand

    def _mask(self, adj, li):
        if not (self.is_training and self.attn_dropout > 0):
            return np.ones((adj.nnz, self.heads))
        return dref.mask(adj, self.heads, dref.attn_key(self.drop_seed, li, self.drop_step), 1.0 - self.attn_dropout)

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
                mk = self._mask(adj, li)
                C = dref.forward(adj, act, act, scale, self.heads, mk, values_only=True).C.astype(f32)
                tape.append(('agg', adj, act, scale, concat, d, mk))
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
                _, adj, x, scale, concat, d, mk = rec
                kw = dict(add=g[:, :d], add_rows=adj.shape[0]) if concat else {}
                g = dref.backward_f64(adj, x, x, g[:, d:] if concat else g, scale, self.heads, mk, fused=True, values_only=True,
                                      **kw)['dx'].astype(f32)
        wd = f32(self.flags['weight_decay'])
        for k in self._wd_names():
            grads[k] += wd * self.params[k]
        return grads


def build(name):
    """attn_aggregator_cases.build's dict for the base stack, with the heads, the probability and this case's seed"""
    c = CASES[name]
    case = ax.build(c['base'])
    case['name'], case['heads'], case['init'], case['attn_dropout'] = name, c['heads'], c['init'], P
    return case


def reference_model(case, nbr, seed=None, params=None, is_training=True, attn_dropout=None):
    cls = type('DropModel%d' % case['heads'], (DropModel,),
               dict(heads=int(case['heads']), attn_dropout=float(case['attn_dropout'] if attn_dropout is None else attn_dropout)))
    fl = case['flags']
    seed = case['init'] if seed is None else seed
    args = (fl, fl['num_layers'], fl['preprocess'], False, False, case['feats'], nbr, case['n'], case['classes'])
    if params is None:
        params = mnp.init_params(cls(*args, {}).specs, seed)
    return cls(*args, params, is_training=is_training)


def reference_step(om, case, feed, rows, dropout, masks, seed, step):
    """One exact training step of the reference, its coefficient masks keyed by (seed, step)."""
    om.drop_seed, om.drop_step = int(seed), int(step)
    return ax.reference_step(om, case, feed, rows, dropout, masks)


def margin(name, init, steps=3):
    """The smallest |non-zero ReLU input| / (its layer's largest input magnitude) over ``steps`` reference steps, the
    coefficient masks applied.  CPU only."""
    case = build(name)
    fl = case['flags']
    om = reference_model(case, case['nbr_train'], seed=init)
    feed, rows = fc.exact_feed(case, case['train_adj'], fl['dropout']), np.sort(case['train'])
    worst = np.inf
    for step in range(steps):
        reference_step(om, case, feed, rows, fl['dropout'], mnp.HashMasks(1, step, 1.0 - fl['dropout']), 1, step)
        for kind, li, small, big in om.margins:
            if np.isfinite(small) and big > 0:
                worst = min(worst, small / big)
    return worst


def scan(name):
    """The first seed of 3 .. 12 whose margin is at least MARGIN, or None."""
    return next((i for i in SEEDS if margin(name, i) >= MARGIN), None)
