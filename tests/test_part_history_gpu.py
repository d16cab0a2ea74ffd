"""GPU tests of --full_batch_part_history above the kernel: part steps that read stored rows for their out-of-part neighbours
against the fp64 reference of tests/part_history_ref.py (forward, push, backward through A[S, S] only), at the project's plain
1e-4 (max|x - ref| / max|ref|, as tests/test_full_batch_gpu.py) on the 96-vertex cases of tests/part_history_cases.py, whose
weight seeds were chosen by the reference alone.  Every figure is printed before it is asserted."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

import part_history_cases as pc
import part_history_ref as pr
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = torch.device('cuda:0')
NAMES = sorted(pc.INIT)


@pytest.fixture(autouse=True)
def _reset_flags():
    from stochastic_gcn_amd.flags import FLAGS
    FLAGS.reset()
    yield
    FLAGS.reset()


def _np(x):
    if hasattr(x, 'materialize'):
        x = x.materialize()
    return x.detach().cpu().numpy()


def _trainer(case, **flags):
    from stochastic_gcn_amd import train
    from stochastic_gcn_amd.flags import FLAGS
    FLAGS.reset()
    FLAGS.update(**{k: v for k, v in case['flags'].items() if hasattr(FLAGS, k)})
    FLAGS.update(full_batch=True, test_full_batch=True, **flags)
    data = (case['n'], case['train_adj'], case['full_adj'], case['feats'], case['nbr_train'], case['nbr_test'], case['labels'],
            case['train'], case['val'], case['test'])
    return train.Trainer(data=data, verbose=False)


def _pair(name, **flags):
    """(case, reference model, trainer whose training model holds the reference's initial weights)"""
    case = pc.build(name)
    om = pr.make_model(case, seed=pc.INIT[name], bf16=flags.get('history_dtype') == 'bf16')
    tr = _trainer(case, full_batch_part_history=True, **flags)
    tr.train_model.set_params({k: v.copy() for k, v in om.params.items()})
    assert len(tr.train_model.layers) == len(om.specs)
    return case, om, tr


def _device_step(tr, ids):
    """what Trainer.train_epoch_parts does with one group; returns (kind, outs)"""
    from stochastic_gcn_amd.flags import FLAGS
    batch = tr.part_batch(ids)
    batch.dropout = FLAGS.dropout
    if batch.rows is None:
        tr.train_model.refresh_part_history(batch)
        return 'refresh', None
    return 'step', tr.train_model.run_one_step(None, batch, sync=False)


def _tables(model):
    """the model's owned tables widened to fp32 on the host (None for a layer that reads the feature table)"""
    from stochastic_gcn_amd import ops
    tables, owned = model.part_history
    return [ops.history_widen(t).cpu().numpy() if own else None for t, own in zip(tables, owned)]


def _agg_inputs(model):
    """the device input of every aggregation layer of the last forward, in layer order"""
    from stochastic_gcn_amd.layers import PlainAggregator
    return [_np(model.activations[i]) for i, layer in enumerate(model.layers[:len(model.activations) - 1])
            if isinstance(layer, PlainAggregator)]


# ---- 1. single-part steps against the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_single_part_steps_match_the_reference(name):
    """P = 3, q = 1, three epochs, fp32 history: every activation, gradient, weight and history table after every step within
    1e-4 of the reference; the rows a layer pushed are its input bit for bit"""
    case, om, tr = _pair(name, full_batch_parts=3, full_batch_parts_per_step=1)
    dm = tr.train_model
    sched = pc.schedule(case)
    assert all(np.array_equal(a, b) for a, b in zip(sched.parts, tr.part_ids))
    tables, owned = dm.part_history
    assert len(tables) == dm.L and [not o for o in owned] == [t is None for t in om.tables]
    assert all(float(t.abs().sum()) == 0 for t, o in zip(tables, owned) if o) and dm._history == []
    worst = dict(act=0.0, grad=0.0, param=0.0, table=0.0, loss=0.0)
    for e in range(pc.EPOCHS):
        groups = sched.epoch(e)
        assert all(np.array_equal(a, b) for a, b in zip(groups, tr.part_schedule.epoch(e)))
        ref = pc.reference_steps(om, case, groups, first_step=dm.dropout_step, seed=dm.dropout_seed)
        for k, ids in enumerate(groups):
            kind, outs = _device_step(tr, ids)
            r = next(ref)
            assert kind == r['kind'] == 'step'
            d_acts, dg, dp = [_np(a) for a in dm.activations[1:]], dm.get_grads(), dm.get_params()
            assert len(d_acts) == len(r['acts'])
            for li, (da, oa) in enumerate(zip(d_acts, r['acts'])):
                err = onp.rel_err(da, oa)
                worst['act'] = max(worst['act'], err)
                assert da.shape == oa.shape and err <= TOL, (name, e, k, 'layer', li, err)
            loss = float(outs[1])
            worst['loss'] = max(worst['loss'], abs(loss - r['loss']) / abs(r['loss']))
            assert abs(loss - r['loss']) <= TOL * abs(r['loss'])
            for key, g in r['grads'].items():
                err = onp.rel_err(dg[key], g)
                worst['grad'] = max(worst['grad'], err)
                assert err <= TOL, (name, e, k, 'grad', key, err)
            for key, v in om.params.items():
                err = onp.rel_err(dp[key], v)
                worst['param'] = max(worst['param'], err)
                assert err <= TOL, (name, e, k, 'param', key, err)
            inputs = _agg_inputs(dm)
            for l, (got, want) in enumerate(zip(_tables(dm), om.tables)):
                if want is None:
                    assert got is None and tables[l] is dm.features_dev
                    continue
                err = onp.rel_err(got, want)
                worst['table'] = max(worst['table'], err)
                assert err <= TOL, (name, e, k, 'table', l, err)
                assert got[ids].tobytes() == inputs[l].tobytes(), "the pushed rows are not the layer's input"
            print("%s epoch %d step %d: |S| %d, loss %.7f (reference %.7f)" % (name, e, k, len(ids), loss, r['loss']))
    rest = np.setdiff1d(np.arange(case['n']), np.concatenate(sched.epoch(0)))
    assert rest.size == 0 and all(np.abs(t).sum() > 0 for t in _tables(dm) if t is not None)
    assert np.array_equal(_np(dm.features_dev), np.asarray(om.features, np.float32))             # never written
    print("%s: worst rel err  activations %.1e  loss %.1e  grads %.1e  params %.1e  tables %.1e"
          % (name, worst['act'], worst['loss'], worst['grad'], worst['param'], worst['table']))
    assert dm.adam_t == 3 * pc.EPOCHS


# ---- 2. P = q: an exact full-graph step, whatever the tables hold -----------------------------------------------------------
@pytest.mark.parametrize("dtype", ['fp32', 'bf16'])
@pytest.mark.parametrize("name", NAMES)
def test_the_union_of_all_parts_is_a_full_batch_step(name, dtype):
    """P = q = 3 with the tables pre-filled with NaN: no out-of-part entry exists, so three steps are finite and within 1e-4
    of three --full_batch --full_batch_kernel rows steps -- under a bfloat16 history too (the fresh operand is never rounded)"""
    case = pc.build(name)
    start = pr.make_model(case, seed=pc.INIT[name]).params
    ta = _trainer(case, full_batch_kernel='rows')
    ta.train_model.set_params({k: v.copy() for k, v in start.items()})
    losses_a = []
    for _ in range(3):
        ta.train_epoch()
        losses_a.append(float(ta.avg_loss.mean()))
    after_a = ta.train_model.get_params()
    tb = _trainer(case, full_batch_parts=3, full_batch_parts_per_step=3, full_batch_part_history=True, history_dtype=dtype)
    tb.train_model.set_params({k: v.copy() for k, v in start.items()})
    tables, owned = tb.train_model.part_history
    assert any(owned) and all(t.dtype == (torch.bfloat16 if dtype == 'bf16' else torch.float32) for t, o in zip(tables, owned) if o)
    for t, o in zip(tables, owned):
        if o:
            t.fill_(float('nan'))
    losses_b = []
    for _ in range(3):
        tb.train_epoch()
        losses_b.append(float(tb.avg_loss.mean()))
        assert tb.last_epoch['steps'] == 1 and tb.last_epoch['skipped'] == 0 and tb.last_epoch['refreshed'] == 0
    after_b = tb.train_model.get_params()
    print("%s %s: losses %s (full batch) %s (all parts, NaN tables)" % (name, dtype, losses_a, losses_b))
    assert all(np.isfinite(l) for l in losses_b)
    assert all(abs(a - b) <= TOL * abs(a) for a, b in zip(losses_a, losses_b))
    for k in after_a:
        err = onp.rel_err(after_b[k], after_a[k])
        print("    %s rel_err %.3e" % (k, err))
        assert np.isfinite(after_b[k]).all() and err <= TOL, (k, err)
    assert all(np.isfinite(t).all() for t in _tables(tb.train_model) if t is not None)          # every row was pushed


# ---- 3. exact tables give exact logits -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_exact_tables_give_the_full_graph_logits(name):
    """dropout 0, the tables hand-filled with the reference's exact activations under the current weights: a q < P step's
    logits on S are the full-graph logits' rows S within 1e-4"""
    from stochastic_gcn_amd import ops
    case, om, tr = _pair(name, full_batch_parts=3, full_batch_parts_per_step=1, dropout=0.0)
    dm = tr.train_model
    everything = np.arange(case['n'])
    full_logits, _ = om.forward_part(everything, 0.0, None)              # S = everything: exact, and it pushes exact rows
    tables, owned = dm.part_history
    for l, (t, o) in enumerate(zip(tables, owned)):
        if o:
            ops.history_assign(t, torch.from_numpy(om.tables[l]).to(DEV))
    for ids in tr.part_schedule.epoch(0):
        batch = tr.part_batch(ids)
        assert 0 < len(ids) < case['n']
        dm.dropout = 0.0
        logits = _np(dm.forward(dm.get_data(batch)))
        err = onp.rel_err(logits, full_logits[ids])
        dropped = pr.make_model(case, params=om.params)                  # zero tables: what ignoring the neighbours costs
        far = onp.rel_err(dropped.forward_part(ids, 0.0, None)[0], full_logits[ids])
        print("%s |S| %d: logits rel_err %.3e (with zero tables the reference is off by %.3e)" % (name, len(ids), err, far))
        assert err <= TOL and far > 100 * TOL


# ---- 4. a group without a training vertex is refreshed ---------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_a_group_without_training_vertices_is_refreshed(name):
    case = pc.build(name)
    parts = pc.schedule(case).parts
    case['train'] = np.setdiff1d(case['train'], parts[2]).astype(np.int32)        # part 2 holds no training vertex
    om = pr.make_model(case, seed=pc.INIT[name])
    tr = _trainer(case, full_batch_parts=3, full_batch_parts_per_step=1, full_batch_part_history=True)
    dm = tr.train_model
    dm.set_params({k: v.copy() for k, v in om.params.items()})
    groups = tr.part_schedule.epoch(0)
    ref = pc.reference_steps(om, case, groups, first_step=dm.dropout_step, seed=dm.dropout_seed)
    kinds = []
    for ids in groups:
        before = dm.get_params()
        kind, _ = _device_step(tr, ids)
        r = next(ref)
        kinds.append(kind)
        assert kind == r['kind']
        if kind == 'refresh':
            after = dm.get_params()
            assert all(before[k].tobytes() == after[k].tobytes() for k in before), "a refresh changed the weights"
            assert np.array_equal(np.sort(ids), np.sort(parts[2]))
        for l, (got, want) in enumerate(zip(_tables(dm), om.tables)):
            if want is not None:
                assert np.abs(got[ids]).sum() > 0 and onp.rel_err(got, want) <= TOL, (kind, l)
    assert sorted(kinds) == ['refresh', 'step', 'step'] and dm.adam_t == 2
    tr.train_epoch()                       # the trainer's own loop counts it (epoch 0 of ITS schedule, again)
    print("%s: kinds %s, last_epoch %s" % (name, kinds, {k: tr.last_epoch[k] for k in ('steps', 'skipped', 'refreshed')}))
    assert (tr.last_epoch['steps'], tr.last_epoch['skipped'], tr.last_epoch['refreshed']) == (2, 0, 1)
    assert all(np.abs(t[parts[2]]).sum() > 0 for t in _tables(dm) if t is not None)
    # without the flag the same group is skipped, as before
    t0 = _trainer(case, full_batch_parts=3, full_batch_parts_per_step=1)
    t0.train_epoch()
    assert (t0.last_epoch['steps'], t0.last_epoch['skipped']) == (2, 1) and 'refreshed' not in t0.last_epoch
    assert t0.train_model.part_history is None


# ---- 5. the flag off changes nothing ---------------------------------------------------------------------------------------
def test_flag_off_runs_give_equal_bits():
    case = pc.build('sage_ln_pp')
    runs = []
    for extra in ({}, {}, dict(full_batch_part_history=False)):
        tr = _trainer(case, full_batch_parts=3, full_batch_parts_per_step=2, **extra)
        assert tr.part_history is False and tr.train_model.part_history is None
        losses = []
        for _ in range(2):
            tr.train_epoch()
            losses.append(np.float32(tr.avg_loss.mean()).tobytes())
        batch = tr.part_batch(tr.part_schedule.epoch(0)[0])
        assert type(batch.matrix).__name__ == 'InducedMatrix'
        runs.append((losses, {k: v.tobytes() for k, v in tr.train_model.get_params().items()}))
    assert runs[0] == runs[1] == runs[2]


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------
def _run_main(monkeypatch, argv):
    from stochastic_gcn_amd import train
    made = []
    real = train.Trainer

    class Keep(real):
        def __init__(self, *a, **k):
            made.append(self)
            super(Keep, self).__init__(*a, **k)
    monkeypatch.setattr(train, "Trainer", Keep)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train.main(argv)
    monkeypatch.setattr(train, "Trainer", real)
    return made[0], buf.getvalue()


@pytest.mark.parametrize("dtype", ['fp32', 'bf16'])
def test_train_main_end_to_end(tmp_path, monkeypatch, dtype):
    """s-cora, 3 epochs (the loop runs epochs + 2 = 5), P = 4, q = 2: a group that holds no training vertex (s-cora's 140 fall
    138 / 0 / 0 / 2 into the parts) is refreshed, not skipped"""
    monkeypatch.chdir(tmp_path)
    argv = ['--dataset', 's-cora', '--full_batch', '--test_full_batch', '--epochs', '3', '--full_batch_parts', '4',
            '--full_batch_parts_per_step', '2', '--full_batch_part_history', '--history_dtype', dtype]
    tr, out = _run_main(monkeypatch, argv)
    setup = [l for l in out.splitlines() if l.startswith("[sgcn] --full_batch_parts 4:")]
    assert len(setup) == 1 and "(values: history)" in setup[0]
    hist = [l for l in out.splitlines() if l.startswith("[sgcn] --full_batch_part_history:")]
    assert len(hist) == 1 and (" %s: " % dtype) in hist[0] and "MiB" in hist[0]
    print(hist[0])
    walls = [l for l in out.splitlines() if l.startswith("[sgcn] epoch train wall")]
    ep = [l for l in out.splitlines() if l.startswith("Epoch:")]
    assert len(ep) == len(walls) == 5
    mask = np.zeros(tr.num_data, dtype=bool)
    mask[tr.train_d] = True
    want = [sum(int(mask[u].any()) for u in tr.part_schedule.epoch(e)) for e in range(5)]
    got = [int(re.search(r" over (\d+) steps ", l).group(1)) for l in walls]
    print("steps per epoch %s (groups with a training vertex: %s); last epoch %s" % (got, want, tr.last_epoch))
    assert got == want and 1 in got
    assert tr.last_epoch['skipped'] == 0 and tr.last_epoch['steps'] + tr.last_epoch['refreshed'] == 2
    assert tr.train_model.adam_t == sum(want)
    for line in ep:
        tok = line.split()
        assert np.isfinite(float(tok[3])) and np.isfinite(float(tok[7]))
    m = re.search(r"Test set results: cost= (\d+\.\d{5})", out)
    assert m and np.isfinite(float(m.group(1)))
    tables, owned = tr.train_model.part_history
    assert all(t.dtype == (torch.bfloat16 if dtype == 'bf16' else torch.float32) for t, o in zip(tables, owned) if o)
    assert all(bool(torch.isfinite(t.float()).all()) and float(t.float().abs().sum()) > 0 for t, o in zip(tables, owned) if o)
