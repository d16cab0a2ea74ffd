"""Graphs and option sets of the full-graph tests (tests/test_full_batch_gpu.py), in the style of model_cases.py, and the
exact feed built BY HAND for the NumPy oracle: fields = arange(N), the whole CSR as every layer's adjacency, unit scales."""
import numpy as np

import model_cases as mc
from oracle import model_np as mnp

REDDIT_FLAGS = dict(normalization='graphsage', weight_decay=0.0, dropout=0.2, layer_norm=True, hidden1=32, num_fc_layers=2)

# ``init`` is the seed of the weights.  A ReLU input within fp32 rounding of zero has no determined gate -- summation order
# decides it -- and one gate switches a whole gradient contribution on or off (on the 3,000-vertex graphs: 2e-3 .. 2e-2 of
# the first layer's weight gradient), so that no 1e-4 comparison of gradients between two fp32 implementations is
# well-posed there.  The seeds are therefore chosen WITH THE ORACLE ALONE, before any device is involved: of the seeds
# 3 .. 12, the one whose smallest non-zero |ReLU input| over the three oracle steps is largest (``gate_margin`` below;
# e.g. reddit3k_nopp: 2.3e-7 at seed 3, 2.5e-6 at seed 9).  The tests then hold every gradient and weight to the plain 1e-4.
CASES = {
    # S-Cora at its SURVEY.md 8d size: gcn normalisation, sparse input features, PP
    'cora': dict(init=12, graph='cora', kernels=('rows', 'cs'),
                 flags=dict(normalization='gcn', hidden1=32, preprocess=True, dropout=0.5, weight_decay=5e-4)),
    # S-PubMed at its size
    'pubmed': dict(init=7, graph='pubmed', kernels=('rows', 'cs'),
                   flags=dict(normalization='gcn', hidden1=32, preprocess=True, dropout=0.5, weight_decay=5e-4)),
    # a 3,000-vertex reddit-like graph with the Reddit recipe: graphsage concat, LayerNorm, two FC layers, dropout 0.2
    'reddit3k_pp': dict(init=9, graph='reddit', n=3000, m=40000, f=24, classes=5, splits=(2000, 300, 700), kernels=('rows', 'cs'),
                        flags=dict(REDDIT_FLAGS, preprocess=True)),
    # ... without pre-processing: two aggregations, the first at the feature width
    'reddit3k_nopp': dict(init=9, graph='reddit', n=3000, m=40000, f=24, classes=5, splits=(2000, 300, 700), kernels=('rows', 'cs'),
                          flags=dict(REDDIT_FLAGS, preprocess=False)),
    # ... with a feature width that is not a multiple of 4: the first aggregation's products fall back to the row kernel
    'reddit3k_nopp_odd': dict(init=10, graph='reddit', n=3000, m=40000, f=22, classes=5, splits=(2000, 300, 700), kernels=('cs',),
                              flags=dict(REDDIT_FLAGS, preprocess=False)),
    # multi-label (the ppi loss): sigmoid cross-entropy over 12 independent labels
    'multilabel': dict(init=9, graph='reddit', n=2000, m=24000, f=20, classes=12, splits=(1200, 300, 500), multitask=True,
                       kernels=('rows', 'cs'), flags=dict(REDDIT_FLAGS, preprocess=True, num_fc_layers=1)),
    # planted communities (a graph ops.LdsSweepCSR.for_graph accepts): the LDS-staged sweep, forward and transposed
    'sbm_lds': dict(init=6, graph='sbm', n=9000, m=300000, f=24, classes=9, splits=(6000, 900, 1800), kernels=('lds',),
                    flags=dict(REDDIT_FLAGS, preprocess=True)),
}


def build(name, seed=0):
    """dict(data = the loader's 10-tuple with the PP products filled in, flags, ph, L, multitask, ...)."""
    from stochastic_gcn_amd import synthetic
    c = CASES[name]
    fl = mnp.make_flags(**c['flags'])
    rng = np.random.RandomState(seed)
    if c['graph'] in ('cora', 'pubmed'):
        n, train_adj, full_adj, feats, _, _, labels, tr, va, te = \
            (synthetic.cora_like if c['graph'] == 'cora' else synthetic.pubmed_like)(fl['normalization'], 123)
        nbr_tr = train_adj.dot(feats).tocsr().astype(np.float32)
        nbr_tr.sort_indices()
        nbr_te = nbr_tr
    else:
        gen = synthetic.reddit_sbm if c['graph'] == 'sbm' else synthetic.reddit_like
        n, train_adj, full_adj, _, _, _, labels, tr, va, te = gen(n=c['n'], m=c['m'], f=c['f'], classes=c['classes'],
                                                                  splits=c['splits'], seed=3, with_features=False)
        feats = rng.standard_normal((n, c['f'])).astype(np.float32)
        nbr_tr = train_adj.dot(feats).astype(np.float32)
        nbr_te = full_adj.dot(feats).astype(np.float32)
    multitask = bool(c.get('multitask'))
    if multitask:
        labels = (rng.rand(n, c['classes']) < 0.3).astype(np.float32)
    classes = int(labels.shape[1])
    L = fl['num_layers'] - 1 if fl['preprocess'] else fl['num_layers']
    return dict(name=name, cfg=c, flags=fl, n=n, classes=classes, L=L, multitask=multitask, ph=mc.placeholders(L, classes),
                train_adj=train_adj, full_adj=full_adj, feats=feats, nbr_train=nbr_tr, nbr_test=nbr_te, labels=labels,
                train=np.asarray(tr, np.int32), val=np.asarray(va, np.int32), test=np.asarray(te, np.int32),
                data=(n, train_adj, full_adj, feats, nbr_tr, nbr_te, labels, np.asarray(tr, np.int32),
                      np.asarray(va, np.int32), np.asarray(te, np.int32)))


def exact_feed(case, adj, dropout):
    """The feed of exact propagation over ``adj``, by hand: every field is all N vertices in order, every layer's adjacency
    the whole matrix (row-major COO triple, as the sampler hands it out), unit scales, the whole label table."""
    ph, L, n = case['ph'], case['L'], case['n']
    coo = adj.tocsr().tocoo()
    assert np.all(np.diff(coo.row) >= 0)
    triple = (np.stack([coo.row, coo.col], axis=1).astype(np.int32), coo.data.astype(np.float32), adj.shape)
    feed = {ph['labels']: case['labels'], ph['dropout']: dropout}
    for l in range(L + 1):
        feed[ph['fields'][l]] = np.arange(n, dtype=np.int32)
    for l in range(L):
        feed[ph['adj'][l]] = triple
        feed[ph['scales'][l]] = np.ones(n, np.float32)
    return feed


def oracle_model(case, nbr, params=None, is_training=True, seed=None):
    fl = case['flags']
    seed = case['cfg']['init'] if seed is None else seed
    args = (fl, fl['num_layers'], fl['preprocess'], False, False, case['feats'], nbr, case['n'], case['classes'])
    if params is None:
        params = mnp.init_params(mnp.Model(*args, {}, multitask=case['multitask']).specs, seed)
    return mnp.Model(*args, params, multitask=case['multitask'], is_training=is_training)


def device_model(case, nbr, adj, params, is_training=True, extra_flags=None):
    import torch
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.plaingcn import PlainGCN
    FLAGS.reset()
    FLAGS.update(**{k: v for k, v in case['flags'].items() if hasattr(FLAGS, k)})
    FLAGS.update(**(extra_flags or {}))
    fl = case['flags']
    m = PlainGCN(fl['num_layers'], fl['preprocess'], case['ph'], case['feats'], nbr, adj, False,
                 multitask=case['multitask'], is_training=is_training, device=torch.device('cuda:0'))
    m.set_params(params)
    return m


def gate_margin(name, init):
    """The smallest non-zero |ReLU input| of the oracle over three exact training steps of case ``name`` with the weights
    seeded by ``init`` (an exact zero is a sum of no terms and the same on every implementation).  CPU only; this is the
    scan the ``init`` entries of CASES come from:  max(range(3, 13), key=lambda i: gate_margin(name, i))."""
    case = build(name)
    fl = case['flags']
    om = oracle_model(case, case['nbr_train'], seed=init)
    feed, rows = exact_feed(case, case['train_adj'], fl['dropout']), np.sort(case['train'])
    seen = []

    def scan(layer, pre):
        a = np.abs(pre)
        seen.append(float(a[a > 0].min()))
        return pre > 0
    om.relu_gate_hook = scan
    for step in range(3):
        logits, _ = om.forward(feed, case['ph'], fl['dropout'], mnp.HashMasks(1, step, 1.0 - fl['dropout']))
        dout = np.zeros_like(logits)
        dout[rows] = om.loss_and_grad(logits[rows], case['labels'][rows])[3]
        om.adam_step(om.backward(dout))
    return min(seen)


def first_layer_gate_interval(om, dout, band):
    """(lo, hi, gradient, number of ambiguous gates) of the FIRST dense layer's weight gradient over every assignment of the
    oracle's ambiguous ReLU gates (|pre| < band) -- the criterion of test_model_gpu._gate_interval, which takes one full
    backward pass per gate, restated so that it is affordable at 233 k rows: below an aggregator the backward pass is
    row-local (LayerNorm, dropout and the dense products act on each row alone) and the aggregator spreads a row's gradient
    to its neighbours only, so the contribution c_s of gate s = (layer, row, column) is the backward pass of ONE element
    restricted to the rows it reaches.  As there, the gradient is taken as affine in the gate vector: with g0 = all of S
    off, lo = g0 + sum min(0, c_s), hi = g0 + sum max(0, c_s).  Oracle only; for a stack with dense inputs."""
    tape = om._tape
    grads = om.backward(dout)                                  # the oracle's own gates
    off = lambda pre: (pre > 0) & (np.abs(pre) >= band)        # noqa: E731  (every ambiguous gate off)
    om.gtrace, om.relu_gate_hook = [], (lambda name, pre: off(pre))
    g0 = om.backward(dout)
    trace, om.gtrace, om.relu_gate_hook = om.gtrace, None, None
    T = len(tape)
    g_in = lambda p: dout if p == T - 1 else trace[T - 2 - p][1]          # noqa: E731  (gradient at record p's OUTPUT)
    first = next(i for i, r in enumerate(tape) if r[0] == 'dense')
    name0 = tape[first][1][1] + '/weights'

    def down(p, R, G, gated):
        """dW of the first dense layer from the gradient G at the output of record p, rows R (``gated``: the ReLU of p is
        already applied)."""
        while True:
            rec = tape[p]
            if rec[0] == 'dense':
                _, s, xin, ctx, pre = rec
                _, name, fin, fout, sparse_in, relu, norm = s
                if relu and not gated:
                    G = G * off(pre[R])
                if norm:
                    xhat, rstd = ctx[0][R], ctx[1][R]
                    dxh = G * om.params[name + '/scale']
                    G = rstd * (dxh - dxh.mean(axis=1, keepdims=True) - xhat * (dxh * xhat).mean(axis=1, keepdims=True))
                if p == first:
                    return xin[R].T.astype(np.float64) @ G
                G = G @ om.params[name + '/weights'].T.astype(np.float64)
            elif rec[0] == 'dropout':
                _, m, keep, _ = rec
                if m is not None:
                    G = G * (m[R] * (1.0 / keep))
            elif rec[0] == 'agg':
                _, adj, scale, concat = rec
                assert scale is None
                d = G.shape[1] // 2 if concat else G.shape[1]
                sub = adj[R]
                K = np.unique(np.concatenate([R, sub.indices]))
                dx = sub.T.tocsr()[K].astype(np.float64) @ (G[:, d:] if concat else G)
                if concat:
                    dx[np.searchsorted(K, R)] += G[:, :d]
                R, G = K, dx
            else:
                raise NotImplementedError(rec[0])
            p, gated = p - 1, False

    g0 = g0[name0].astype(np.float64)
    up, dn, n_amb = np.zeros_like(g0), np.zeros_like(g0), 0
    for p, rec in enumerate(tape):
        if rec[0] != 'dense' or not rec[1][5]:
            continue
        pre, gi = rec[4], g_in(p)
        for i, j in np.argwhere(np.abs(pre) < band):
            G = np.zeros((1, pre.shape[1]))
            G[0, j] = gi[i, j]
            c = down(p, np.array([i]), G, True)                # this gate on minus all of S off
            up += np.maximum(c, 0)
            dn += np.minimum(c, 0)
            n_amb += 1
    return g0 + dn, g0 + up, grads[name0], n_amb
