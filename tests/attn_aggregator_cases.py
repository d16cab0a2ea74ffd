"""The tiny graphs of the end-to-end test of --aggregator attn (tests/test_attn_aggregator_gpu.py), in the style of
max_aggregator_cases.py, and the scan their weight seeds come from.

Well-posedness is a CONDITION here, not a measurement.  A ReLU input within rounding of zero has no determined gate
(full_batch_cases.py), and no 1e-4 comparison between two fp32 implementations is well-posed there.  Attention itself is
smooth -- a softmax has no ties to break -- and adds no condition of its own.  So ``init``, the seed of the weights, is
chosen WITH THE REFERENCE ALONE, on the CPU: over the three reference steps every non-zero |ReLU input| must be at least
MARGIN = 1e-4 times that layer's largest input magnitude (the scan of max_aggregator_cases.scan without its gap
condition).  ``scan`` looks through the seeds 3 .. 12:  {name: scan(name)} gives the ``init`` entries below."""
import numpy as np

import full_batch_cases as fc
import model_cases as mc
from oracle import model_np as mnp

MARGIN = 1e-4
SEEDS = range(3, 13)

CASES = {
    # graphsage concat with LayerNorm, pre-processed: one attention layer at the hidden width behind a LayerNorm / ReLU layer
    'sage_ln_pp': dict(init=3, n=96, m=700, f=6, classes=4, splits=(60, 12, 24),
                       flags=dict(normalization='graphsage', layer_norm=True, preprocess=True, hidden1=8, num_fc_layers=1,
                                  dropout=0.2, weight_decay=0.0)),
    # gcn (no concat) without LayerNorm and without pre-processing: every aggregation is attention, the first over the features
    'gcn_nopp': dict(init=3, n=96, m=700, f=6, classes=4, splits=(60, 12, 24),
                     flags=dict(normalization='gcn', layer_norm=False, preprocess=False, hidden1=8, num_fc_layers=1,
                                dropout=0.2, weight_decay=5e-4)),
}


def build(name):
    """The dict full_batch_cases.build gives (what exact_feed and device_model read), for a tiny reddit-like graph."""
    from stochastic_gcn_amd import synthetic
    c = CASES[name]
    fl = mnp.make_flags(**c['flags'])
    n, train_adj, full_adj, _, _, _, labels, tr, va, te = synthetic.reddit_like(
        n=c['n'], m=c['m'], f=c['f'], classes=c['classes'], splits=c['splits'], seed=3, with_features=False)
    assert n <= 500 and fl['hidden1'] == 8
    rng = np.random.RandomState(0)
    feats = rng.standard_normal((n, c['f'])).astype(np.float32)
    nbr_tr = train_adj.dot(feats).astype(np.float32)
    nbr_te = full_adj.dot(feats).astype(np.float32)
    classes = int(labels.shape[1])
    L = fl['num_layers'] - 1 if fl['preprocess'] else fl['num_layers']
    return dict(name=name, cfg=c, flags=fl, n=n, classes=classes, L=L, multitask=False, ph=mc.placeholders(L, classes),
                train_adj=train_adj, full_adj=full_adj, feats=feats, nbr_train=nbr_tr, nbr_test=nbr_te, labels=labels,
                train=np.asarray(tr, np.int32), val=np.asarray(va, np.int32), test=np.asarray(te, np.int32))


def reference_model(case, nbr, seed=None, params=None, is_training=True):
    from attn_aggregator_ref import AttnModel
    fl = case['flags']
    seed = case['cfg']['init'] if seed is None else seed
    args = (fl, fl['num_layers'], fl['preprocess'], False, False, case['feats'], nbr, case['n'], case['classes'])
    if params is None:
        params = mnp.init_params(AttnModel(*args, {}).specs, seed)
    return AttnModel(*args, params, is_training=is_training)


def reference_step(om, case, feed, rows, dropout, masks):
    """One exact training step of the reference with the loss over ``rows``."""
    logits, acts = om.forward(feed, case['ph'], dropout, masks)
    loss, acc, _, dl = om.loss_and_grad(logits[rows], case['labels'][rows])
    dout = np.zeros_like(logits)
    dout[rows] = dl
    grads = om.backward(dout)
    om.adam_step(grads)
    return logits, acts, float(loss), float(acc), grads


def margin(name, init, steps=3):
    """The smallest |non-zero ReLU input| / (its layer's largest input magnitude) over ``steps`` reference steps of case
    ``name`` with the weights seeded by ``init``.  CPU only."""
    case = build(name)
    fl = case['flags']
    om = reference_model(case, case['nbr_train'], seed=init)
    feed, rows = fc.exact_feed(case, case['train_adj'], fl['dropout']), np.sort(case['train'])
    worst = np.inf
    for step in range(steps):
        reference_step(om, case, feed, rows, fl['dropout'], mnp.HashMasks(1, step, 1.0 - fl['dropout']))
        for kind, li, small, big in om.margins:
            if np.isfinite(small) and big > 0:
                worst = min(worst, small / big)
    return worst


def scan(name):
    """The first seed of 3 .. 12 whose margin is at least MARGIN, or None."""
    return next((i for i in SEEDS if margin(name, i) >= MARGIN), None)
