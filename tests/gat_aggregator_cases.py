"""The end-to-end cases of --attn_score gat (tests/test_gat_aggregator_gpu.py) -- test-only.

    sage_ln_pp_gat        attn_aggregator_cases' graphsage / LayerNorm / pre-processed stack, one head
    gcn_nopp_h2_gat       its gcn stack without pre-processing (every aggregation is attention, agg0 the first parametrised
                          layer), --attn_heads 2
    ..._p2                the same two with --attn_dropout 0.2

Well-posedness is a CONDITION, checked with the reference alone on the CPU.  ``init``, the seed of the weights, is the first seed
of 3 .. 12 for which, over three reference steps,
  (1) every non-zero |ReLU input| is at least MARGIN = 1e-4 of its layer's largest (attn_aggregator_cases.py), and
  (2) every stored entry's |z_ij|, in every aggregation layer and head, is at least ZMARGIN = 64 times that entry's derived fp32
      error bound for z (gat_aggregator_ref.py): fp32 rounding cannot flip a LeakyReLU branch, whose two sides differ in slope.
``scan`` gives the entries below; tests/test_gat_aggregator_gpu.py asserts both conditions again on every step it compares."""
import numpy as np

import attn_aggregator_cases as ax
import full_batch_cases as fc
from oracle import model_np as mnp

MARGIN = ax.MARGIN
ZMARGIN = 64.0
SEEDS = ax.SEEDS
SLOPE = 0.2

CASES = {
    'sage_ln_pp_gat': dict(base='sage_ln_pp', heads=1, p=0.0, init=3),
    'gcn_nopp_h2_gat': dict(base='gcn_nopp', heads=2, p=0.0, init=4),
    'sage_ln_pp_gat_p2': dict(base='sage_ln_pp', heads=1, p=0.2, init=3),
    'gcn_nopp_h2_gat_p2': dict(base='gcn_nopp', heads=2, p=0.2, init=4),
}


def build(name):
    c = CASES[name]
    case = ax.build(c['base'])
    case['name'], case['heads'], case['init'], case['attn_dropout'] = name, c['heads'], c['init'], c['p']
    return case


def extra_flags(case):
    fl = dict(aggregator='attn', full_batch=True, test_full_batch=True, attn_score='gat', attn_heads=case['heads'])
    if case['attn_dropout'] > 0:
        fl['attn_dropout'] = case['attn_dropout']
    return fl


def reference_model(case, nbr, seed=None, params=None, is_training=True):
    from gat_aggregator_ref import GatModel, init_attn_vecs
    cls = type('GatModel%d' % case['heads'], (GatModel,),
               dict(heads=int(case['heads']), attn_dropout=float(case['attn_dropout']), attn_slope=SLOPE))
    fl = case['flags']
    seed = case['init'] if seed is None else seed
    args = (fl, fl['num_layers'], fl['preprocess'], False, False, case['feats'], nbr, case['n'], case['classes'])
    if params is None:
        params = mnp.init_params(cls(*args, {}).specs, seed)
        init_attn_vecs(params, fl, fl['preprocess'], case['feats'].shape[1], case['L'], seed)
    return cls(*args, params, is_training=is_training)


def reference_step(om, case, feed, rows, dropout, masks, seed, step):
    om.drop_seed, om.drop_step = int(seed), int(step)
    return ax.reference_step(om, case, feed, rows, dropout, masks)


def margins(name, init, steps=3):
    """(the smallest ReLU margin, the smallest |z| / bound) over ``steps`` reference steps of case ``name`` seeded by ``init``"""
    case = build(name)
    fl = case['flags']
    om = reference_model(case, case['nbr_train'], seed=init)
    feed, rows = fc.exact_feed(case, case['train_adj'], fl['dropout']), np.sort(case['train'])
    worst, zworst = np.inf, np.inf
    for step in range(steps):
        reference_step(om, case, feed, rows, fl['dropout'], mnp.HashMasks(1, step, 1.0 - fl['dropout']), 1, step)
        for kind, li, small, big in om.margins:
            if np.isfinite(small) and big > 0:
                worst = min(worst, small / big)
        zworst = min([zworst] + [r for _, r in om.zratios])
    return worst, zworst


def well_posed(name, init):
    m, z = margins(name, init)
    return m >= MARGIN and z >= ZMARGIN


def scan(name):
    """The first seed of 3 .. 12 that meets both conditions, or None."""
    return next((i for i in SEEDS if well_posed(name, i)), None)
