"""The model cases of the --full_batch_part_pull_max tests (tests/test_part_pull_max_gpu.py): the two 96-vertex graphs of
part_history_cases.py under the schedule of part steps (P = 3, q = 1, three epochs), driven through the reference of
tests/part_pull_max_ref.py, and the scan their weight seeds come from.

Well-posedness is a CONDITION, as in max_aggregator_cases.py: a maximum whose runner-up sits within fp32 rounding of the
winner has no determined argmax -- and here the loser may be a stored row, so the gradient would go to another vertex or
nowhere -- and a ReLU input within rounding of zero has no determined gate.  ``INIT`` is therefore chosen WITH THE REFERENCE
ALONE, on the CPU, before any device is involved: over every reference step of the schedules the tests compare at 1e-4 --
single parts for three epochs; the same with part 2 stripped of its training vertices (the refresh path, one epoch) -- every
non-zero top-two gap of every pull-max layer, taken over ALL stored entries of a selected row, stale ones included, and every
non-zero |ReLU input| must be at least MARGIN = 1e-4 (max_aggregator_cases.MARGIN) times its layer's largest input
magnitude.  Exact ties are fine: both sides resolve them by the same rule.  ``scan(name)`` gives the first seed of 3 .. 12
with that property:  {name: scan(name) for name in INIT};  ``margins(name, seed)`` the figures.

``reaches_both_branches`` is the second condition, on the reference too: in every step after the first epoch every max layer
has at least one element won by a stale row and at least one won by a fresh row -- otherwise the comparison would not
reach the kernel's two tables."""
import numpy as np

import max_aggregator_cases as mx
import part_history_cases as pc
import part_pull_max_ref as xr

MARGIN = mx.MARGIN
SEEDS = range(3, 13)
# margins(name, seed) = (single parts, refresh schedule) at the chosen seeds, both with a fresh and a stale winner in every
# max layer of every step after the first epoch:
#   sage_ln_pp seed 3: 3.7e-4 / 6.2e-4      gcn_nopp seed 3: 2.2e-4 / 2.2e-4
#   (seeds that fail: sage_ln_pp 5 (3.4e-5 on the refresh schedule), 9 (1.7e-5), 11 (8.9e-5); gcn_nopp 4, 6, 7, 8, 9, 11)
INIT = {'sage_ln_pp': 3, 'gcn_nopp': 3}
P, EPOCHS, SEED = pc.P, pc.EPOCHS, pc.SEED

build, schedule, loss_rows, reference_steps = pc.build, pc.schedule, pc.loss_rows, pc.reference_steps


def without_training_vertices_in(case, part):
    """``case`` with the training vertices of ``part`` taken out of the training set: a group over it takes the refresh path"""
    case['train'] = np.setdiff1d(case['train'], part).astype(np.int32)
    return case


def _walk(case, om, sched, epochs):
    """(the worst margin, [(epoch, per-layer (fresh, stale) winners) of every training step]) over the reference's steps"""
    worst, step, won = np.inf, 0, []
    for e in range(epochs):
        groups = sched.epoch(e)
        for r in reference_steps(om, case, groups, first_step=step):
            worst = min(worst, om.margin())
            if r['kind'] == 'step':
                won.append((e, dict(om.winners)))
        step += len(groups)
    return worst, won


def margins(name, init):
    """the smallest relative (non-zero top-two gap or |ReLU input|) of (single parts, the refresh schedule)"""
    case = build(name)
    a, _ = _walk(case, xr.make_model(case, seed=init), schedule(case), EPOCHS)
    case = build(name)
    without_training_vertices_in(case, schedule(case).parts[2])
    b, _ = _walk(case, xr.make_model(case, seed=init), schedule(case), 1)
    return a, b


def reaches_both_branches(name, init):
    """every step after the first epoch: every max layer has a fresh and a stale winner"""
    case = build(name)
    om = xr.make_model(case, seed=init)
    _, won = _walk(case, om, schedule(case), EPOCHS)
    late = [w for e, w in won if e >= 1]
    return len(late) == (EPOCHS - 1) * P and all(len(w) == om.L and all(f > 0 and s > 0 for f, s in w.values()) for w in late)


def scan(name):
    return next((i for i in SEEDS if min(margins(name, i)) >= MARGIN and reaches_both_branches(name, i)), None)
