"""The end-to-end cases of --attn_heads (tests/test_attn_heads_model_gpu.py): the two stacks of attn_aggregator_cases.py with
heads, and the scan their weight seeds come from.

    sage_ln_pp at heads 2 and 8   hidden1 = 8: dh = 4 and dh = 1 on the one attention layer
    gcn_nopp at heads 2           f = 6: dh = 3 on the first layer, 4 on the second

Well-posedness is the CONDITION of attn_aggregator_cases.py, unchanged: ``init`` is the first seed of 3 .. 12 for which, over
three reference steps on the CPU, every non-zero |ReLU input| is at least MARGIN = 1e-4 of its layer's largest.  The scan runs
with the reference alone (tests/attn_heads_ref.py); tests/test_spattn_heads.py asserts that the entries below are its answers."""
import numpy as np

import attn_aggregator_cases as ax
import full_batch_cases as fc
from oracle import model_np as mnp

MARGIN = ax.MARGIN
SEEDS = ax.SEEDS

CASES = {
    'sage_ln_pp_h2': dict(base='sage_ln_pp', heads=2, init=3),
    'sage_ln_pp_h8': dict(base='sage_ln_pp', heads=8, init=3),
    'gcn_nopp_h2': dict(base='gcn_nopp', heads=2, init=3),
}


def build(name):
    """attn_aggregator_cases.build's dict for the base stack, with the heads and this case's seed"""
    c = CASES[name]
    case = ax.build(c['base'])
    case['name'], case['heads'], case['init'] = name, c['heads'], c['init']
    return case


def reference_model(case, nbr, seed=None, params=None, is_training=True):
    from attn_heads_ref import model_class
    cls = model_class(case['heads'])
    fl = case['flags']
    seed = case['init'] if seed is None else seed
    args = (fl, fl['num_layers'], fl['preprocess'], False, False, case['feats'], nbr, case['n'], case['classes'])
    if params is None:
        params = mnp.init_params(cls(*args, {}).specs, seed)
    return cls(*args, params, is_training=is_training)


reference_step = ax.reference_step


def margin(name, init, steps=3):
    """The smallest |non-zero ReLU input| / (its layer's largest input magnitude) over ``steps`` reference steps.  CPU only."""
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
