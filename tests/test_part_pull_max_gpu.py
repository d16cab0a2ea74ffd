"""GPU tests of --full_batch_part_pull_max above the kernel: part steps of --aggregator max whose every aggregation layer takes
the element-wise maximum over every stored neighbour -- fresh rows inside the step's vertex set, stored rows outside -- against
the reference of tests/part_pull_max_ref.py (forward, push, the gradient scattered to in-part winners only), at the project's
plain 1e-4 (max|x - ref| / max|ref|, as tests/test_part_history_gpu.py) on the 96-vertex cases of tests/part_pull_max_cases.py,
whose weight seeds were chosen by the reference alone so that no maximum and no ReLU gate is within rounding of a tie.  A run
with bfloat16 tables is NOT held to the reference: a one-ulp fp32 difference in a pushed value can flip its bfloat16 rounding
(2^-8 relative), and under a maximum that element can be a winner; there the pushed rows must be the rounding of the device's
own layer inputs, and the kernel-level identity of tests/test_spmax_pull_gpu.py carries the bfloat16 kernel.  Every figure is
printed before it is asserted."""
import re

import numpy as np
import pytest
import torch

import part_history_ref as pr
import part_pull_max_cases as mc
import part_pull_max_ref as xr
from oracle import oracle_np as onp
from test_part_pull_attn_gpu import _agg_inputs, _device_step, _np, _run_main, _tables, _trainer

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = torch.device('cuda:0')
CASES = sorted(mc.INIT)


@pytest.fixture(autouse=True)
def _reset_flags():
    from stochastic_gcn_amd.flags import FLAGS
    FLAGS.reset()
    yield
    FLAGS.reset()


def _pair(name, case=None, **flags):
    """(case, reference model, trainer whose training model holds the reference's initial weights)"""
    case = mc.build(name) if case is None else case
    om = xr.make_model(case, seed=mc.INIT[name], bf16=flags.get('history_dtype') == 'bf16')
    tr = _trainer(case, full_batch_part_pull_max=True, aggregator='max', **flags)
    assert tr.part_pull_max and tr.part_history and not tr.part_pull and not tr.part_pull_gat
    tr.train_model.set_params({k: v.copy() for k, v in om.params.items()})
    assert len(tr.train_model.layers) == len(om.specs)
    return case, om, tr


def _step(tr, ids):
    kind, outs = _device_step(tr, ids)
    return kind, outs


def _compare_step(name, where, dm, om, r, outs, ids, worst):
    """every activation, the loss, every gradient, weight and owned table of one step against the reference's"""
    d_acts, dg, dp = [_np(a) for a in dm.activations[1:]], dm.get_grads(), dm.get_params()
    assert len(d_acts) == len(r['acts'])
    for li, (da, oa) in enumerate(zip(d_acts, r['acts'])):
        err = onp.rel_err(da, oa)
        worst['act'] = max(worst['act'], err)
        print("    %s layer %d: rel_err %.3e" % (where, li, err))
        assert da.shape == oa.shape and np.isfinite(da).all() and err <= TOL, (name, where, 'layer', li, err)
    loss = float(outs[1])
    worst['loss'] = max(worst['loss'], abs(loss - r['loss']) / abs(r['loss']))
    print("    %s |S| %d: loss %.7f (reference %.7f)" % (where, len(ids), loss, r['loss']))
    assert abs(loss - r['loss']) <= TOL * abs(r['loss'])
    for key, g in r['grads'].items():
        err = onp.rel_err(dg[key], g)
        worst['grad'] = max(worst['grad'], err)
        print("    %s grad %s: rel_err %.3e" % (where, key, err))
        assert np.isfinite(dg[key]).all() and err <= TOL, (name, where, 'grad', key, err)
    for key, v in om.params.items():
        err = onp.rel_err(dp[key], v)
        worst['param'] = max(worst['param'], err)
        assert err <= TOL, (name, where, 'param', key, err)
    inputs = _agg_inputs(dm)
    tables = dm.part_history[0]
    for l, (got, want) in enumerate(zip(_tables(dm), om.tables)):
        if want is None:
            assert got is None and tables[l] is dm.features_dev
            continue
        err = onp.rel_err(got, want)
        worst['table'] = max(worst['table'], err)
        print("    %s table %d: rel_err %.3e" % (where, l, err))
        assert err <= TOL, (name, where, 'table', l, err)
        assert got[ids].tobytes() == inputs[l].tobytes(), "the pushed rows are not the layer's input"


# ---- 1. single-part steps against the reference, fp32 tables --------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_single_part_steps_match_the_reference(name):
    """P = 3, q = 1, three epochs: every activation, loss, gradient, weight and owned table after every step within 1e-4 of the
    reference; the rows a layer pushed are its input bit for bit; after the first epoch every max layer of every step has
    winners from both tables (on the reference AND in the device's own arg)"""
    case, om, tr = _pair(name, full_batch_parts=3, full_batch_parts_per_step=1)
    dm = tr.train_model
    sched = mc.schedule(case)
    assert all(np.array_equal(a, b) for a, b in zip(sched.parts, tr.part_ids))
    tables, owned = dm.part_history
    assert len(tables) == dm.L and [not o for o in owned] == [t is None for t in om.tables]
    assert all(t.dtype == torch.float32 and float(t.abs().sum()) == 0 for t, o in zip(tables, owned) if o)
    from stochastic_gcn_amd.layers import PlainAggregator
    aggs = [layer for layer in dm.layers if isinstance(layer, PlainAggregator)]
    worst = dict(act=0.0, grad=0.0, param=0.0, table=0.0, loss=0.0)
    for e in range(mc.EPOCHS):
        groups = sched.epoch(e)
        assert all(np.array_equal(a, b) for a, b in zip(groups, tr.part_schedule.epoch(e)))
        ref = mc.reference_steps(om, case, groups, first_step=dm.dropout_step, seed=dm.dropout_seed)
        for k, ids in enumerate(groups):
            kind, outs = _step(tr, ids)
            r = next(ref)
            assert kind == r['kind'] == 'step' and 0 < len(ids) < case['n']
            _compare_step(name, "epoch %d step %d" % (e, k), dm, om, r, outs, ids, worst)
            won = [(int((layer._arg >= 0).sum()), int((layer._arg <= -2).sum())) for layer in aggs]
            print("    epoch %d step %d: (fresh, stale) winners per max layer: device %s, reference %s"
                  % (e, k, won, [om.winners[l] for l in sorted(om.winners)]))
            assert won == [om.winners[l] for l in sorted(om.winners)]
            if e >= 1:
                assert all(f > 0 and s > 0 for f, s in won)
    assert all(np.abs(t).sum() > 0 for t in _tables(dm) if t is not None)
    assert np.array_equal(_np(dm.features_dev), np.asarray(om.features, np.float32))             # never written
    print("%s: worst rel err  activations %.1e  loss %.1e  grads %.1e  params %.1e  tables %.1e"
          % (name, worst['act'], worst['loss'], worst['grad'], worst['param'], worst['table']))
    assert dm.adam_t == 3 * mc.EPOCHS


# ---- 2. a group without a training vertex takes the refresh path ----------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_a_group_without_training_vertices_is_refreshed(name):
    case = mc.build(name)
    parts = mc.schedule(case).parts
    mc.without_training_vertices_in(case, parts[2])
    case, om, tr = _pair(name, case=case, full_batch_parts=3, full_batch_parts_per_step=1)
    dm = tr.train_model
    groups = tr.part_schedule.epoch(0)
    ref = mc.reference_steps(om, case, groups, first_step=dm.dropout_step, seed=dm.dropout_seed)
    kinds, worst = [], dict(act=0.0, grad=0.0, param=0.0, table=0.0, loss=0.0)
    for k, ids in enumerate(groups):
        before = dm.get_params()
        kind, outs = _step(tr, ids)
        r = next(ref)
        kinds.append(kind)
        assert kind == r['kind']
        if kind == 'step':
            _compare_step(name, "step %d" % k, dm, om, r, outs, ids, worst)
            continue
        after = dm.get_params()
        assert all(before[key].tobytes() == after[key].tobytes() for key in before), "a refresh changed the weights"
        assert np.array_equal(np.sort(ids), np.sort(parts[2]))
        for l, (got, want) in enumerate(zip(_tables(dm), om.tables)):
            if want is not None:
                err = onp.rel_err(got, want)
                print("    refresh: table %d rel_err %.3e" % (l, err))
                assert np.abs(got[ids]).sum() > 0 and err <= TOL, (kind, l)
    assert sorted(kinds) == ['refresh', 'step', 'step'] and dm.adam_t == 2
    tr.train_epoch()                       # the trainer's own loop counts it (epoch 0 of ITS schedule, again)
    print("%s: kinds %s, last_epoch %s" % (name, kinds, {k: tr.last_epoch[k] for k in ('steps', 'skipped', 'refreshed')}))
    assert (tr.last_epoch['steps'], tr.last_epoch['skipped'], tr.last_epoch['refreshed']) == (2, 0, 1)


# ---- 3. q = P: S = everything, whatever the tables hold ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ['fp32', 'bf16'])
@pytest.mark.parametrize("name", CASES)
def test_the_union_of_all_parts_is_full_batch_on_every_logit(name, dtype):
    """P = q = 3 with the owned tables pre-filled with +inf -- a value that would win every maximum it entered: no out-of-part
    entry exists, so no table is read, and three steps give the logits, losses and weights of --full_batch --aggregator max
    --full_batch_kernel rows, bit for bit"""
    case = mc.build(name)
    ta = _trainer(case, full_batch_kernel='rows', aggregator='max')
    start = {k: v.copy() for k, v in ta.train_model.get_params().items()}
    logits_a, losses_a = [], []
    for _ in range(mc.EPOCHS):
        ta.train_epoch()
        logits_a.append(_np(ta.train_model.activations[-1]))
        losses_a.append(np.float32(ta.avg_loss.mean()))
    after_a = ta.train_model.get_params()
    tb = _trainer(case, full_batch_part_pull_max=True, aggregator='max', full_batch_parts=3, full_batch_parts_per_step=3,
                  history_dtype=dtype)
    tb.train_model.set_params({k: v.copy() for k, v in start.items()})
    tables, owned = tb.train_model.part_history
    assert any(owned) and tb.part_history_bf16 == (dtype == 'bf16')
    for t, o in zip(tables, owned):
        if o:
            assert t.dtype == (torch.bfloat16 if dtype == 'bf16' else torch.float32)
            t.fill_(float('inf'))
    for e in range(mc.EPOCHS):
        tb.train_epoch()
        assert tb.last_epoch['steps'] == 1 and tb.last_epoch['skipped'] == 0
        got = _np(tb.train_model.activations[-1])
        loss = np.float32(tb.avg_loss.mean())
        print("%s %s epoch %d: loss %.7f (full batch %.7f), logits differ in %d of %d elements"
              % (name, dtype, e, loss, losses_a[e], int(np.sum(got.view(np.uint32) != logits_a[e].view(np.uint32))), got.size))
        assert np.isfinite(got).all() and got.shape == (case['n'], case['classes'])
        assert got.tobytes() == logits_a[e].tobytes() and loss.tobytes() == losses_a[e].tobytes()
    after_b = tb.train_model.get_params()
    assert all(after_a[k].tobytes() == after_b[k].tobytes() for k in after_a)
    assert all(np.isfinite(t).all() for t in _tables(tb.train_model) if t is not None)           # every row was pushed


# ---- 4. bfloat16 tables -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_bf16_tables_hold_the_rounding_of_the_devices_own_inputs(name):
    """P = 3, q = 1, three epochs under --history_dtype bf16: after every step the rows a layer pushed are the round-to-nearest-
    even bfloat16 image of the DEVICE's own layer input, bit for bit; everything stays finite; a second run gives the same
    bits"""
    runs = []
    for rep in range(2):
        case, om, tr = _pair(name, full_batch_parts=3, full_batch_parts_per_step=1, history_dtype='bf16')
        dm = tr.train_model
        tables, owned = dm.part_history
        assert all(t.dtype == torch.bfloat16 for t, o in zip(tables, owned) if o)
        losses = []
        for e in range(mc.EPOCHS):
            for k, ids in enumerate(tr.part_schedule.epoch(e)):
                kind, outs = _step(tr, ids)
                assert kind == 'step' and np.isfinite(float(outs[1]))
                losses.append(np.float32(float(outs[1])).tobytes())
                inputs = _agg_inputs(dm)
                for l, got in enumerate(_tables(dm)):
                    if got is not None:
                        want = pr.widen_bf16(pr.round_bf16(inputs[l]))
                        assert np.isfinite(got).all() and got[ids].tobytes() == want.tobytes(), (e, k, l)
                assert all(np.isfinite(_np(a)).all() for a in dm.activations[1:])
        params = dm.get_params()
        assert all(np.isfinite(v).all() for v in params.values())
        runs.append((losses, {k: v.tobytes() for k, v in params.items()}, [t.tobytes() for t in _tables(dm) if t is not None]))
    print("%s: %d steps, last loss bits %s / %s" % (name, len(runs[0][0]), runs[0][0][-1].hex(), runs[1][0][-1].hex()))
    assert runs[0] == runs[1]


# ---- 5. without the flag nothing changes ------------------------------------------------------------------------------------
def test_without_the_flag_the_two_table_launch_is_never_made(monkeypatch):
    """--full_batch_parts --aggregator max without the flag: an InducedMatrix, ops.spmax_pull never called, no table allocated;
    and where no out-of-part entry exists (q = P, values kept) the flag's run gives that run's bits -- the new launch and
    the block's one-table maximum meet"""
    from stochastic_gcn_amd import ops
    case = mc.build('sage_ln_pp')
    calls = []
    real = ops.spmax_pull
    monkeypatch.setattr(ops, 'spmax_pull', lambda *a, **k: calls.append(1) or real(*a, **k))
    runs = {}
    for flag in (False, True):
        tr = _trainer(case, aggregator='max', full_batch_parts=3, full_batch_parts_per_step=3, full_batch_part_norm='keep',
                      **(dict(full_batch_part_pull_max=True) if flag else {}))
        batch = tr.part_batch(tr.part_schedule.epoch(0)[0])
        assert type(batch.matrix).__name__ == ('PulledMatrix' if flag else 'InducedMatrix')
        assert tr.part_history is flag and (tr.train_model.part_history is not None) == flag
        before = len(calls)
        losses = []
        for _ in range(2):
            tr.train_epoch()
            losses.append(np.float32(tr.avg_loss.mean()).tobytes())
        made = len(calls) - before
        print("flag %s: %d two-table launches, loss bits %s" % (flag, made, [l.hex() for l in losses]))
        assert (made > 0) == flag
        runs[flag] = (losses, {k: v.tobytes() for k, v in tr.train_model.get_params().items()})
    assert runs[False] == runs[True]


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------
def test_train_main_end_to_end(tmp_path, monkeypatch):
    """s-cora, 2 epochs, P = 4, q = 2, --aggregator max with the flag: the log line names it, every table ends finite and
    filled"""
    monkeypatch.chdir(tmp_path)
    argv = ['--dataset', 's-cora', '--full_batch', '--test_full_batch', '--epochs', '2', '--full_batch_parts', '4',
            '--full_batch_parts_per_step', '2', '--full_batch_part_pull_max', '--aggregator', 'max']
    tr, out = _run_main(monkeypatch, argv)
    setup = [l for l in out.splitlines() if l.startswith("[sgcn] --full_batch_parts 4:")]
    assert len(setup) == 1 and "(values: history)" in setup[0]
    line = [l for l in out.splitlines() if l.startswith("[sgcn] --full_batch_part_pull_max: a step takes the maximum over every stored "
                                                        "entry of its rows")]
    assert len(line) == 1 and " fp32: " in line[0] and "MiB" in line[0]
    assert "a group without a training vertex runs the forward only and pushes its rows" in line[0]
    assert not [l for l in out.splitlines() if l.startswith("[sgcn] --full_batch_part_history:")]
    print(line[0])
    walls = [l for l in out.splitlines() if l.startswith("[sgcn] epoch train wall")]
    ep = [l for l in out.splitlines() if l.startswith("Epoch:")]
    assert len(ep) == len(walls) and len(ep) >= 2
    mask = np.zeros(tr.num_data, dtype=bool)
    mask[tr.train_d] = True
    want = [sum(int(mask[u].any()) for u in tr.part_schedule.epoch(e)) for e in range(len(ep))]
    got = [int(re.search(r" over (\d+) steps ", l).group(1)) for l in walls]
    print("steps per epoch %s (groups with a training vertex: %s); last epoch %s" % (got, want, tr.last_epoch))
    assert got == want
    assert tr.last_epoch['skipped'] == 0 and tr.last_epoch['steps'] + tr.last_epoch['refreshed'] == 2
    for l in ep:
        tok = l.split()
        assert np.isfinite(float(tok[3])) and np.isfinite(float(tok[7]))
    m = re.search(r"Test set results: cost= (\d+\.\d{5})", out)
    assert m and np.isfinite(float(m.group(1)))
    tables, owned = tr.train_model.part_history
    assert tr.part_pull_max and all(t.dtype == torch.float32 for t, o in zip(tables, owned) if o)
    assert all(bool(torch.isfinite(t).all()) and float(t.abs().sum()) > 0 for t, o in zip(tables, owned) if o)
