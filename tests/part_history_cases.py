"""The model cases of the --full_batch_part_history tests (tests/test_part_history_gpu.py): the two tiny graphs of
attn_aggregator_cases.py (96 vertices) under the schedule of part steps, driven through the fp64 reference of
tests/part_history_ref.py, and the scan their weight seeds come from.

Well-posedness is a CONDITION, as in full_batch_cases.py: a ReLU input within rounding of zero has no determined gate, and
no 1e-4 comparison between two fp32 implementations is well-posed there.  ``INIT`` is therefore chosen WITH THE REFERENCE ALONE,
on the CPU, before any device is involved: over every reference step of the schedule the tests run (P = 3, q = 1, three
epochs) every non-zero |ReLU input| must be at least MARGIN = 1e-4 times its layer's largest input magnitude.
``scan(name)`` gives the first seed of 3 .. 12 with that property:  {name: scan(name) for name in INIT}."""
import numpy as np

import attn_aggregator_cases as ax
from oracle import model_np as mnp
import part_history_ref as pr

MARGIN = 1e-4
SEEDS = range(3, 13)
INIT = {'sage_ln_pp': 3, 'gcn_nopp': 4}     # margins 1.5e-3 / 1.6e-4 and 8.4e-4 / 1.4e-4 (gcn_nopp at seed 3: 4.4e-5)
P, EPOCHS, SEED = 3, 3, 1


def build(name):
    case = ax.build(name)
    a = case['train_adj'].tocsr().copy()
    a.sort_indices()
    case['train_adj'] = a
    return case


def schedule(case, parts=P, per_step=1):
    """the PartSchedule the trainer builds for --full_batch_parts parts --full_batch_parts_per_step per_step --seed 1"""
    from stochastic_gcn_amd.full_batch import PartSchedule, partition
    return PartSchedule(partition(case['train_adj'], parts, SEED), per_step, SEED)


def loss_rows(case, ids):
    return np.flatnonzero(np.isin(ids, case['train'])).astype(np.int32)


def reference_steps(om, case, groups, first_step=0, seed=SEED):
    """Runs the reference over the vertex sets ``groups`` in order -- a training step where the set holds a training vertex,
    the forward-only refresh otherwise -- and yields one dict per set: kind, ids, rows, and for a step logits / acts / loss /
    grads.  The dropout masks are the product's hash masks under (seed, step counter)."""
    drop = case['flags']['dropout']
    for k, ids in enumerate(groups):
        masks = mnp.HashMasks(seed, first_step + k, 1.0 - drop)
        rows = loss_rows(case, ids)
        if rows.size == 0:
            _, acts = om.forward_part(ids, drop, masks, stop_at_last_agg=True)
            yield dict(kind='refresh', ids=ids, rows=rows, acts=acts)
        else:
            logits, acts, loss, grads = om.step(ids, rows, case['labels'], drop, masks)
            yield dict(kind='step', ids=ids, rows=rows, logits=logits, acts=acts, loss=loss, grads=grads)


def margin(name, init, per_step=1):
    """the smallest relative |non-zero ReLU input| over the reference's EPOCHS epochs of steps over ``per_step`` parts"""
    case = build(name)
    om = pr.make_model(case, seed=init)
    sched = schedule(case, per_step=per_step)
    worst, step = np.inf, 0
    for e in range(EPOCHS):
        groups = sched.epoch(e)
        for _ in reference_steps(om, case, groups, first_step=step):
            worst = min(worst, om.relu_margin())
        step += len(groups)
    return worst


def scan(name):
    """(both schedules the tests compare at 1e-4: single parts, and the one union of all three)"""
    return next((i for i in SEEDS if min(margin(name, i, 1), margin(name, i, P)) >= MARGIN), None)
