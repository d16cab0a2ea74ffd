"""The model cases of the --full_batch_part_pull tests with --aggregator attn (tests/test_part_pull_attn_gpu.py): the two
96-vertex graphs of attn_aggregator_cases.py under the schedule of part steps, at 1 and 2 heads, driven through the fp64
reference of tests/part_pull_attn_ref.py, and the scan their weight seeds come from.

Well-posedness is a CONDITION, as in part_history_cases.py: a ReLU input within rounding of zero has no determined gate, and
no 1e-4 comparison between two fp32 implementations is well-posed there (attention itself is smooth and adds no condition).
``INIT`` is therefore chosen WITH THE REFERENCE ALONE, on the CPU, before any device is involved: over every reference step of
the schedules the tests run -- P = 3 with q = 1 for three epochs, fp32 and bfloat16 tables; the same with part 2 stripped of
its training vertices (the refresh path, one epoch); q = 3 for three epochs -- every non-zero |ReLU input| must be at least
MARGIN = 1e-4 times its layer's largest input magnitude.  ``scan(name, heads)`` gives the first seed of 3 .. 12 with that
property:  {(name, heads): scan(name, heads) for (name, heads) in INIT};  ``margins(name, heads, seed)`` the figures."""
import numpy as np

import part_history_cases as pc
import part_pull_attn_ref as ar

MARGIN = pc.MARGIN
SEEDS = range(3, 13)
HEADS = (1, 2)
# the margins of the four schedules (single parts fp32 / single parts bf16 / refresh / union) at the chosen seeds, per margins():
#   sage_ln_pp heads 1 seed 3: 4.7e-4 / 4.8e-4 / 1.8e-3 / 5.4e-4      sage_ln_pp heads 2 seed 3: 1.5e-3 / 1.4e-3 / 1.1e-3 / 1.1e-4
#   gcn_nopp   heads 1 seed 3: 6.9e-4 / 6.9e-4 / 5.3e-4 / 1.5e-4      gcn_nopp   heads 2 seed 5: 1.5e-4 / 1.5e-4 / 1.5e-4 / 2.0e-4
#   (gcn_nopp heads 2 at seed 3: 1.5e-5 on the single-part schedule, at seed 4: 6.2e-7)
INIT = {('sage_ln_pp', 1): 3, ('sage_ln_pp', 2): 3, ('gcn_nopp', 1): 3, ('gcn_nopp', 2): 5}
P, EPOCHS, SEED = pc.P, pc.EPOCHS, pc.SEED

build, schedule, loss_rows, reference_steps = pc.build, pc.schedule, pc.loss_rows, pc.reference_steps


def without_training_vertices_in(case, part):
    """``case`` with the training vertices of ``part`` taken out of the training set: a group over it takes the refresh path"""
    case['train'] = np.setdiff1d(case['train'], part).astype(np.int32)
    return case


def _margin(case, om, sched, epochs):
    worst, step = np.inf, 0
    for e in range(epochs):
        groups = sched.epoch(e)
        for _ in reference_steps(om, case, groups, first_step=step):
            worst = min(worst, om.relu_margin())
        step += len(groups)
    return worst


def margins(name, heads, init):
    """the smallest relative |non-zero ReLU input| of (single parts fp32, single parts bf16, the refresh schedule, the union)"""
    out = []
    for bf16 in (False, True):
        case = build(name)
        out.append(_margin(case, ar.make_model(case, heads=heads, seed=init, bf16=bf16), schedule(case), EPOCHS))
    case = build(name)
    without_training_vertices_in(case, schedule(case).parts[2])
    out.append(_margin(case, ar.make_model(case, heads=heads, seed=init), schedule(case), 1))
    case = build(name)
    out.append(_margin(case, ar.make_model(case, heads=heads, seed=init), schedule(case, per_step=P), EPOCHS))
    return tuple(out)


def scan(name, heads):
    return next((i for i in SEEDS if min(margins(name, heads, i)) >= MARGIN), None)
