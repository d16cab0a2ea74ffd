"""GPU tests of --full_batch_part_pull above the kernels: part steps of --aggregator attn that attend over every stored
neighbour -- fresh rows inside the step's vertex set, stored rows outside -- against the fp64 reference of
tests/part_pull_attn_ref.py (forward, push, dQ over all entries + dB through A[S, S] only), at the project's plain 1e-4
(max|x - ref| / max|ref|, as tests/test_part_history_gpu.py) on the 96-vertex cases of tests/part_pull_attn_cases.py at 1 and 2
heads, whose weight seeds were chosen by the reference alone.  With --aggregator sum the flag must be --full_batch_part_history
bit for bit.  Every figure is printed before it is asserted."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

import part_history_ref as pr
import part_pull_attn_cases as pc
import part_pull_attn_ref as ar
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = torch.device('cuda:0')
CASES = sorted(pc.INIT)


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


def _pair(name, heads, case=None, **flags):
    """(case, reference model, trainer whose training model holds the reference's initial weights)"""
    case = pc.build(name) if case is None else case
    om = ar.make_model(case, heads=heads, seed=pc.INIT[(name, heads)], bf16=flags.get('history_dtype') == 'bf16')
    tr = _trainer(case, full_batch_part_pull=True, aggregator='attn', attn_heads=heads, **flags)
    assert tr.part_pull and tr.part_history
    tr.train_model.set_params({k: v.copy() for k, v in om.params.items()})
    assert len(tr.train_model.layers) == len(om.specs)
    return case, om, tr


def _device_step(tr, ids):
    """what Trainer.train_epoch_parts does with one group; returns (kind, outs)"""
    from stochastic_gcn_amd.flags import FLAGS
    batch = tr.part_batch(ids)
    assert type(batch.matrix).__name__ == 'PulledMatrix'
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


def _compare_step(name, where, dm, om, r, outs, ids, worst, bf16):
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
        pushed = pr.widen_bf16(pr.round_bf16(inputs[l])) if bf16 else inputs[l]
        assert got[ids].tobytes() == pushed.tobytes(), "the pushed rows are not the layer's input"


# ---- 1. single-part steps against the reference, fp32 and bfloat16 tables ------------------------------------------------------
@pytest.mark.parametrize("name,heads,dtype", [c + ('fp32',) for c in CASES] + [('sage_ln_pp', 2, 'bf16'), ('gcn_nopp', 1, 'bf16')])
def test_single_part_steps_match_the_reference(name, heads, dtype):
    """P = 3, q = 1, three epochs: every activation, loss, gradient, weight and owned table after every step within 1e-4 of the
    reference; the rows a layer pushed are its input bit for bit (rounded to bfloat16 under --history_dtype bf16, as the
    reference rounds on its push)"""
    case, om, tr = _pair(name, heads, full_batch_parts=3, full_batch_parts_per_step=1, history_dtype=dtype)
    dm = tr.train_model
    sched = pc.schedule(case)
    assert all(np.array_equal(a, b) for a, b in zip(sched.parts, tr.part_ids))
    tables, owned = dm.part_history
    assert len(tables) == dm.L and [not o for o in owned] == [t is None for t in om.tables]
    assert all(t.dtype == (torch.bfloat16 if dtype == 'bf16' else torch.float32) for t, o in zip(tables, owned) if o)
    assert all(float(t.float().abs().sum()) == 0 for t, o in zip(tables, owned) if o)
    worst = dict(act=0.0, grad=0.0, param=0.0, table=0.0, loss=0.0)
    for e in range(pc.EPOCHS):
        groups = sched.epoch(e)
        assert all(np.array_equal(a, b) for a, b in zip(groups, tr.part_schedule.epoch(e)))
        ref = pc.reference_steps(om, case, groups, first_step=dm.dropout_step, seed=dm.dropout_seed)
        for k, ids in enumerate(groups):
            kind, outs = _device_step(tr, ids)
            r = next(ref)
            assert kind == r['kind'] == 'step' and 0 < len(ids) < case['n']
            _compare_step(name, "epoch %d step %d" % (e, k), dm, om, r, outs, ids, worst, dtype == 'bf16')
    assert all(np.abs(t).sum() > 0 for t in _tables(dm) if t is not None)
    assert np.array_equal(_np(dm.features_dev), np.asarray(om.features, np.float32))             # never written
    print("%s heads %d %s: worst rel err  activations %.1e  loss %.1e  grads %.1e  params %.1e  tables %.1e"
          % (name, heads, dtype, worst['act'], worst['loss'], worst['grad'], worst['param'], worst['table']))
    assert dm.adam_t == 3 * pc.EPOCHS


def test_the_stored_rows_matter():
    """the reference with its tables emptied before a late step is far from the device: the comparison above sees the estimator"""
    name, heads = 'sage_ln_pp', 2
    case, om, tr = _pair(name, heads, full_batch_parts=3, full_batch_parts_per_step=1)
    dm = tr.train_model
    groups = pc.schedule(case).epoch(0)
    ref = pc.reference_steps(om, case, groups, first_step=dm.dropout_step, seed=dm.dropout_seed)
    for ids in groups[:2]:
        _device_step(tr, ids)
        next(ref)
    blind = ar.make_model(case, heads=heads, params={k: v.copy() for k, v in om.params.items()})       # zero tables
    b = next(pc.reference_steps(blind, case, groups[2:], first_step=dm.dropout_step, seed=dm.dropout_seed))
    kind, outs = _device_step(tr, groups[2])
    r = next(ref)
    assert kind == r['kind'] == b['kind'] == 'step'
    got = _np(dm.activations[-1])
    near, far = onp.rel_err(got, r['logits']), onp.rel_err(got, b['logits'])
    print("logits of step 3: rel_err %.3e to the reference, %.3e to the reference with zero tables" % (near, far))
    assert near <= TOL and far > 100 * TOL


# ---- 2. a group without a training vertex takes the refresh path ----------------------------------------------------------------
@pytest.mark.parametrize("name,heads", CASES)
def test_a_group_without_training_vertices_is_refreshed(name, heads):
    case = pc.build(name)
    parts = pc.schedule(case).parts
    pc.without_training_vertices_in(case, parts[2])
    case, om, tr = _pair(name, heads, case=case, full_batch_parts=3, full_batch_parts_per_step=1)
    dm = tr.train_model
    groups = tr.part_schedule.epoch(0)
    ref = pc.reference_steps(om, case, groups, first_step=dm.dropout_step, seed=dm.dropout_seed)
    kinds, worst = [], dict(act=0.0, grad=0.0, param=0.0, table=0.0, loss=0.0)
    for k, ids in enumerate(groups):
        before = dm.get_params()
        kind, outs = _device_step(tr, ids)
        r = next(ref)
        kinds.append(kind)
        assert kind == r['kind']
        if kind == 'step':
            _compare_step(name, "step %d" % k, dm, om, r, outs, ids, worst, False)
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
    print("%s heads %d: kinds %s, last_epoch %s" % (name, heads, kinds, {k: tr.last_epoch[k] for k in ('steps', 'skipped', 'refreshed')}))
    assert (tr.last_epoch['steps'], tr.last_epoch['skipped'], tr.last_epoch['refreshed']) == (2, 0, 1)


# ---- 3. q = P: S = everything, whatever the tables hold -----------------------------------------------------------------------
@pytest.mark.parametrize("name,heads", CASES)
def test_the_union_of_all_parts_never_reads_the_tables(name, heads):
    """P = q = 3 with the owned tables pre-filled with NaN: no out-of-part entry exists, so three steps are finite and within
    1e-4 of the reference (whose tables do not matter either)"""
    case, om, tr = _pair(name, heads, full_batch_parts=3, full_batch_parts_per_step=3)
    dm = tr.train_model
    tables, owned = dm.part_history
    assert any(owned)
    for t, o in zip(tables, owned):
        if o:
            t.fill_(float('nan'))
    for l, t in enumerate(om.tables):
        if t is not None:
            t.fill(np.nan)
    sched = pc.schedule(case, per_step=pc.P)
    worst = dict(act=0.0, grad=0.0, param=0.0, table=0.0, loss=0.0)
    for e in range(pc.EPOCHS):
        groups = sched.epoch(e)
        assert len(groups) == 1 and len(groups[0]) == case['n']
        ref = pc.reference_steps(om, case, groups, first_step=dm.dropout_step, seed=dm.dropout_seed)
        kind, outs = _device_step(tr, groups[0])
        _compare_step(name, "epoch %d" % e, dm, om, next(ref), outs, groups[0], worst, False)
    assert all(np.isfinite(t).all() for t in _tables(dm) if t is not None)          # every row was pushed
    print("%s heads %d: worst rel err  activations %.1e  loss %.1e  grads %.1e  params %.1e"
          % (name, heads, worst['act'], worst['loss'], worst['grad'], worst['param']))


# ---- 4. with the sum aggregator the flag is --full_batch_part_history ------------------------------------------------------------
@pytest.mark.parametrize("dtype", ['fp32', 'bf16'])
def test_the_sum_aggregator_gives_the_bits_of_part_history(dtype):
    import part_history_cases as hc
    case = hc.build('sage_ln_pp')
    runs = []
    for flags in (dict(full_batch_part_history=True), dict(full_batch_part_pull=True),
                  dict(full_batch_part_history=True, full_batch_part_pull=True)):
        tr = _trainer(case, full_batch_parts=3, full_batch_parts_per_step=1, history_dtype=dtype, **flags)
        assert tr.part_history is True and tr.part_history_bf16 == (dtype == 'bf16')
        tr.train_epoch()
        batch = tr.part_batch(tr.part_schedule.epoch(0)[0])
        assert type(batch.matrix).__name__ == 'PulledMatrix' and batch.matrix.describe(8)['kernel'] == "sgcn::spmm_pull_kernel"
        runs.append((np.float32(tr.avg_loss.mean()).tobytes(), {k: v.tobytes() for k, v in tr.train_model.get_params().items()},
                     [t.tobytes() for t in _tables(tr.train_model) if t is not None], tr.last_epoch['steps']))
    print("loss bits %s" % [r[0].hex() for r in runs])
    assert runs[0] == runs[1] == runs[2] and runs[0][3] == 3


# ---- 5. end to end -------------------------------------------------------------------------------------------------------
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


def test_train_main_end_to_end(tmp_path, monkeypatch):
    """s-cora, 2 epochs, P = 4, q = 2, --aggregator attn with 2 heads and bfloat16 tables: the log line names the aggregator, a
    group without a training vertex is refreshed, every table ends finite and filled"""
    monkeypatch.chdir(tmp_path)
    argv = ['--dataset', 's-cora', '--full_batch', '--test_full_batch', '--epochs', '2', '--full_batch_parts', '4',
            '--full_batch_parts_per_step', '2', '--full_batch_part_pull', '--aggregator', 'attn', '--attn_heads', '2',
            '--history_dtype', 'bf16']
    tr, out = _run_main(monkeypatch, argv)
    setup = [l for l in out.splitlines() if l.startswith("[sgcn] --full_batch_parts 4:")]
    assert len(setup) == 1 and "(values: history)" in setup[0]
    line = [l for l in out.splitlines() if l.startswith("[sgcn] --full_batch_part_pull (--aggregator attn): a step attends over")]
    assert len(line) == 1 and " bf16: " in line[0] and "MiB" in line[0]
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
    assert all(t.dtype == torch.bfloat16 for t, o in zip(tables, owned) if o)
    assert all(bool(torch.isfinite(t.float()).all()) and float(t.float().abs().sum()) > 0 for t, o in zip(tables, owned) if o)
