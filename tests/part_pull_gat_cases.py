"""The model cases of the --full_batch_part_pull_gat tests (tests/test_part_pull_gat_gpu.py): the two 96-vertex graphs of
gat_aggregator_cases.py (attn_aggregator_cases' sage_ln_pp and gcn_nopp) under part_history_cases' schedules of part steps, at
1 and 2 heads, driven through the fp64 reference of tests/part_pull_gat_ref.py, and the scan their weight seeds come from.

Well-posedness is a CONDITION, as in part_pull_attn_cases.py, with one more term: a ReLU input within rounding of zero has no
determined gate, and neither has a LeakyReLU input -- the derivative of the score's LeakyReLU jumps at z = 0, so |z_e| counts
too.  ``INIT`` is chosen WITH THE REFERENCE ALONE, on the CPU, before any device is involved: over every reference step of the
schedules the tests run -- P = 3 with q = 1 for three epochs, fp32 and bfloat16 tables; the same with part 2 stripped of its
training vertices (the refresh path, one epoch); q = 3 for three epochs -- every non-zero |ReLU input| and every |z_e| of every
stored entry and head must be at least MARGIN = 1e-4 times its layer's largest magnitude.  One kind of entry is counted and
not held to the margin: a DEAD one, whose z has no non-zero term at all (a source row the ReLU zeroed across the whole head
meeting a destination score of exactly 0, part_pull_gat_ref.PartPullGatModel._record_z) -- its z is exactly 0 in every arithmetic
and its branch is determined.  gcn_nopp at 2 heads (8 columns per head behind a ReLU) has such entries at every seed: held to
the margin as well, no seed of 3 .. 399 qualifies for it.  ``scan(name, heads)`` gives the first seed of SEEDS with the property
-- the range of part_pull_attn_cases.py, 3 .. 12, widened until every case has one, the margin left alone:  {(name, heads): scan(name, heads) for (name, heads) in INIT};  ``margins(name, heads, seed)``
the figures, (ReLU, z) per schedule."""
import numpy as np

import part_history_cases as pc
import part_pull_attn_cases as ac
import part_pull_gat_ref as gr

MARGIN = pc.MARGIN
SEEDS = range(3, 101)
HEADS = (1, 2)
SLOPE = 0.2
# the margins min(ReLU, z) of the four schedules (single parts fp32 / single parts bf16 / refresh / union) at the chosen seeds,
# per margins():
#   sage_ln_pp heads 1 seed  3: ReLU 3.9e-4 / 3.9e-4 / 1.8e-3 / 5.5e-4      z 1.8e-4 / 1.5e-4 / 4.2e-3 / 8.9e-4
#   sage_ln_pp heads 2 seed  5: ReLU 1.2e-4 / 1.2e-4 / 2.6e-3 / 1.3e-4      z 2.4e-4 / 2.6e-4 / 4.6e-3 / 7.0e-4
#   gcn_nopp   heads 1 seed 14: ReLU 2.0e-4 / 2.0e-4 / 2.0e-3 / 1.9e-4      z 1.1e-4 / 1.0e-4 / 6.7e-4 / 1.6e-4
#   gcn_nopp   heads 2 seed 70: ReLU 1.1e-3 / 1.1e-3 / 1.5e-4 / 6.1e-4      z 1.7e-4 / 1.8e-4 / 2.1e-4 / 1.5e-4
#   (sage_ln_pp heads 2 at seed 3: ReLU 7.9e-6 on the union; gcn_nopp heads 1 at seed 3: ReLU 4.8e-5; heads 2 at seed 3: z 5.8e-6)
INIT = {('sage_ln_pp', 1): 3, ('sage_ln_pp', 2): 5, ('gcn_nopp', 1): 14, ('gcn_nopp', 2): 70}
P, EPOCHS, SEED = pc.P, pc.EPOCHS, pc.SEED

build, schedule, loss_rows, reference_steps = pc.build, pc.schedule, pc.loss_rows, pc.reference_steps
without_training_vertices_in = ac.without_training_vertices_in


def make_model(case, heads, seed=None, bf16=False, params=None):
    return gr.make_model(case, heads=heads, seed=seed, bf16=bf16, params=params, slope=SLOPE)


def _margin(case, om, sched, epochs):
    relu, z, step = np.inf, np.inf, 0
    for e in range(epochs):
        groups = sched.epoch(e)
        for _ in reference_steps(om, case, groups, first_step=step):
            relu, z = min(relu, om.relu_margin()), min(z, om.z_margin())
        step += len(groups)
    return relu, z


def margins(name, heads, init):
    """(smallest relative |non-zero ReLU input|, smallest relative |z_e|) of (single parts fp32, single parts bf16, the
    refresh schedule, the union)"""
    out = []
    for bf16 in (False, True):
        case = build(name)
        out.append(_margin(case, make_model(case, heads, seed=init, bf16=bf16), schedule(case), EPOCHS))
    case = build(name)
    without_training_vertices_in(case, schedule(case).parts[2])
    out.append(_margin(case, make_model(case, heads, seed=init), schedule(case), 1))
    case = build(name)
    out.append(_margin(case, make_model(case, heads, seed=init), schedule(case, per_step=P), EPOCHS))
    return tuple(out)


def scan(name, heads):
    return next((i for i in SEEDS if min(min(m) for m in margins(name, heads, i)) >= MARGIN), None)
