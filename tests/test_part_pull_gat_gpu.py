"""GPU tests of --full_batch_part_pull_gat above the kernels: part steps of --aggregator attn --attn_score gat that attend over
every stored neighbour -- fresh rows and scores inside the step's vertex set, stored rows and stored destination scores
outside -- against the fp64 reference of tests/part_pull_gat_ref.py (forward, both pushes, dU over all entries, dB and dV
through A[S, S] only, attn_vec's gradient), at the project's plain 1e-4 (max|x - ref| / max|ref|, as
tests/test_part_pull_attn_gpu.py) on the 96-vertex cases of tests/part_pull_gat_cases.py at 1 and 2 heads, whose weight seeds
were chosen by the reference alone.  Every figure is printed before it is asserted."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

import part_pull_gat_cases as gc
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = torch.device('cuda:0')
CASES = sorted(gc.INIT)


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
    # (attn_vec is as wide as its layer's input: the evaluation model shares the training model's variables, so it must
    # pre-process exactly where the training model does)
    FLAGS.update(full_batch=True, test_full_batch=True, aggregator='attn', attn_score='gat', attn_slope=gc.SLOPE,
                 test_preprocess=bool(case['flags']['preprocess']), **flags)
    data = (case['n'], case['train_adj'], case['full_adj'], case['feats'], case['nbr_train'], case['nbr_test'], case['labels'],
            case['train'], case['val'], case['test'])
    return train.Trainer(data=data, verbose=False)


def _pair(name, heads, case=None, **flags):
    """(case, reference model, trainer whose training model holds the reference's initial weights)"""
    case = gc.build(name) if case is None else case
    om = gc.make_model(case, heads, seed=gc.INIT[(name, heads)], bf16=flags.get('history_dtype') == 'bf16')
    tr = _trainer(case, full_batch_part_pull_gat=True, attn_heads=heads, **flags)
    assert tr.part_pull_gat and tr.part_history and not tr.part_pull
    tr.train_model.set_params({k: v.copy() for k, v in om.params.items()})
    assert len(tr.train_model.layers) == len(om.specs)
    return case, om, tr


def _device_step(tr, ids):
    """what Trainer.train_epoch_parts does with one group; returns (kind, outs)"""
    from stochastic_gcn_amd.flags import FLAGS
    batch = tr.part_batch(ids)
    assert type(batch.matrix).__name__ == 'PulledMatrix'
    assert all(a is b for a, b in zip(batch.matrix.scores, tr.train_model.part_scores)) and len(batch.matrix.scores) == tr.train_model.L
    batch.dropout = FLAGS.dropout
    if batch.rows is None:
        tr.train_model.refresh_part_history(batch)
        return 'refresh', None
    return 'step', tr.train_model.run_one_step(None, batch, sync=False)


def _tables(model):
    """the model's owned row tables widened to fp32 on the host (None for a layer that reads the feature table)"""
    from stochastic_gcn_amd import ops
    tables, owned = model.part_history
    return [ops.history_widen(t).cpu().numpy() if own else None for t, own in zip(tables, owned)]


def _compare_tables(name, where, dm, om, worst, ids=None):
    for l, (got, want) in enumerate(zip(_tables(dm), om.tables)):
        if want is None:
            assert got is None and dm.part_history[0][l] is dm.features_dev
            continue
        err = onp.rel_err(got, want)
        worst['table'] = max(worst['table'], err)
        print("    %s row table %d: rel_err %.3e" % (where, l, err))
        assert err <= TOL, (name, where, 'table', l, err)
    assert len(dm.part_scores) == len(om.scores) == dm.L
    for l, (t, want) in enumerate(zip(dm.part_scores, om.scores)):
        got = _np(t)
        err = onp.rel_err(got, want)
        worst['score'] = max(worst['score'], err)
        print("    %s score table %d: rel_err %.3e" % (where, l, err))
        assert t.dtype == torch.float32 and got.shape == want.shape and err <= TOL, (name, where, 'score table', l, err)
        if ids is not None:
            assert np.abs(got[ids]).sum() > 0


def _compare_step(name, where, dm, om, r, outs, ids, worst):
    """every activation, the loss, every gradient (attn_vec's among them), weight, row table and score table of one step"""
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
    assert sorted(dg) == sorted(r['grads']) and any(k.endswith('attn_vec') for k in dg)
    for key, g in r['grads'].items():
        err = onp.rel_err(dg[key], g)
        worst['grad'] = max(worst['grad'], err)
        print("    %s grad %s: rel_err %.3e" % (where, key, err))
        assert np.isfinite(dg[key]).all() and err <= TOL, (name, where, 'grad', key, err)
    for key, v in om.params.items():
        err = onp.rel_err(dp[key], v)
        worst['param'] = max(worst['param'], err)
        assert err <= TOL, (name, where, 'param', key, err)
    _compare_tables(name, where, dm, om, worst, ids)


def _worst():
    return dict(act=0.0, grad=0.0, param=0.0, table=0.0, score=0.0, loss=0.0)


# ---- 1. single-part steps against the reference, fp32 and bfloat16 tables ------------------------------------------------------
@pytest.mark.parametrize("dtype", ['fp32', 'bf16'])
@pytest.mark.parametrize("name,heads", CASES)
def test_single_part_steps_match_the_reference(name, heads, dtype):
    """P = 3, q = 1, three epochs: every activation, loss, gradient, weight, row table and score table after every step within
    1e-4 of the reference (rows rounded to bfloat16 on the push under --history_dtype bf16; the score tables stay fp32)"""
    case, om, tr = _pair(name, heads, full_batch_parts=3, full_batch_parts_per_step=1, history_dtype=dtype)
    dm = tr.train_model
    sched = gc.schedule(case)
    assert all(np.array_equal(a, b) for a, b in zip(sched.parts, tr.part_ids))
    tables, owned = dm.part_history
    assert len(tables) == dm.L and [not o for o in owned] == [t is None for t in om.tables]
    assert all(t.dtype == (torch.bfloat16 if dtype == 'bf16' else torch.float32) for t, o in zip(tables, owned) if o)
    assert all(tuple(t.shape) == (case['n'], heads) and float(t.abs().sum()) == 0 for t in dm.part_scores)
    worst = _worst()
    for e in range(gc.EPOCHS):
        groups = sched.epoch(e)
        assert all(np.array_equal(a, b) for a, b in zip(groups, tr.part_schedule.epoch(e)))
        ref = gc.reference_steps(om, case, groups, first_step=dm.dropout_step, seed=dm.dropout_seed)
        for k, ids in enumerate(groups):
            kind, outs = _device_step(tr, ids)
            r = next(ref)
            assert kind == r['kind'] == 'step' and 0 < len(ids) < case['n']
            assert om.relu_margin() >= gc.MARGIN and om.z_margin() >= gc.MARGIN          # the condition, on the step compared
            _compare_step(name, "epoch %d step %d" % (e, k), dm, om, r, outs, ids, worst)
    assert np.array_equal(_np(dm.features_dev), np.asarray(om.features, np.float32))             # never written
    print("%s heads %d %s: worst rel err  activations %.1e  loss %.1e  grads %.1e  params %.1e  row tables %.1e  score tables %.1e"
          % (name, heads, dtype, worst['act'], worst['loss'], worst['grad'], worst['param'], worst['table'], worst['score']))
    assert dm.adam_t == 3 * gc.EPOCHS


def test_the_stored_scores_matter():
    """the reference with its SCORE tables emptied (its row tables kept) before a late step is far from the device: the
    comparison above sees the stored scores, not the rows alone"""
    name, heads = 'sage_ln_pp', 1
    case, om, tr = _pair(name, heads, full_batch_parts=3, full_batch_parts_per_step=1)
    dm = tr.train_model
    groups = gc.schedule(case).epoch(0)
    ref = gc.reference_steps(om, case, groups, first_step=dm.dropout_step, seed=dm.dropout_seed)
    for ids in groups[:2]:
        _device_step(tr, ids)
        next(ref)
    blind = gc.make_model(case, heads, params={k: v.copy() for k, v in om.params.items()})
    blind.tables = [None if t is None else t.copy() for t in om.tables]                       # zero score tables only
    b = next(gc.reference_steps(blind, case, groups[2:], first_step=dm.dropout_step, seed=dm.dropout_seed))
    kind, outs = _device_step(tr, groups[2])
    r = next(ref)
    assert kind == r['kind'] == b['kind'] == 'step'
    got = _np(dm.activations[-1])
    near, far = onp.rel_err(got, r['logits']), onp.rel_err(got, b['logits'])
    print("logits of step 3: rel_err %.3e to the reference, %.3e to the reference with zero score tables" % (near, far))
    assert near <= TOL and far > 10 * TOL


# ---- 2. a group without a training vertex takes the refresh path ----------------------------------------------------------------
@pytest.mark.parametrize("name,heads", CASES)
def test_a_group_without_training_vertices_is_refreshed(name, heads):
    """it pushes rows and scores of every aggregation layer and takes no Adam step"""
    case = gc.build(name)
    parts = gc.schedule(case).parts
    gc.without_training_vertices_in(case, parts[2])
    case, om, tr = _pair(name, heads, case=case, full_batch_parts=3, full_batch_parts_per_step=1)
    dm = tr.train_model
    groups = tr.part_schedule.epoch(0)
    ref = gc.reference_steps(om, case, groups, first_step=dm.dropout_step, seed=dm.dropout_seed)
    kinds, worst = [], _worst()
    for k, ids in enumerate(groups):
        before, t0 = dm.get_params(), dm.adam_t
        kind, outs = _device_step(tr, ids)
        r = next(ref)
        kinds.append(kind)
        assert kind == r['kind']
        if kind == 'step':
            _compare_step(name, "step %d" % k, dm, om, r, outs, ids, worst)
            continue
        after = dm.get_params()
        assert all(before[key].tobytes() == after[key].tobytes() for key in before) and dm.adam_t == t0, "a refresh stepped"
        assert np.array_equal(np.sort(ids), np.sort(parts[2]))
        _compare_tables(name, "refresh", dm, om, worst, ids)
        for l, t in enumerate(_tables(dm)):
            if t is not None:
                assert np.abs(t[ids]).sum() > 0
    assert sorted(kinds) == ['refresh', 'step', 'step'] and dm.adam_t == 2
    tr.train_epoch()                       # the trainer's own loop counts it (epoch 0 of ITS schedule, again)
    print("%s heads %d: kinds %s, last_epoch %s" % (name, heads, kinds, {k: tr.last_epoch[k] for k in ('steps', 'skipped', 'refreshed')}))
    assert (tr.last_epoch['steps'], tr.last_epoch['skipped'], tr.last_epoch['refreshed']) == (2, 0, 1)


# ---- 3. q = P: every neighbour is fresh ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,heads", CASES)
def test_the_union_of_all_parts_has_the_bits_of_plain_part_steps(name, heads):
    """P = q = 3 with every owned table pre-filled with NaN: no out-of-part entry exists, no table is read, and each of three
    steps has the bits -- loss, every gradient, every weight -- of the same step under plain --full_batch_parts
    --full_batch_part_norm keep, whose block is the whole matrix; and it is within 1e-4 of the reference"""
    case, om, tr = _pair(name, heads, full_batch_parts=3, full_batch_parts_per_step=3)
    plain = _trainer(gc.build(name), full_batch_parts=3, full_batch_parts_per_step=3, full_batch_part_norm='keep', attn_heads=heads)
    assert not plain.part_history and plain.train_model.part_scores is None and plain.train_model.part_history is None
    plain.train_model.set_params({k: v.copy() for k, v in om.params.items()})
    dm, pm = tr.train_model, plain.train_model
    tables, owned = dm.part_history
    for t, o in zip(tables, owned):
        if o:
            t.fill_(float('nan'))
    for t in dm.part_scores:
        t.fill_(float('nan'))
    sched = gc.schedule(case, per_step=gc.P)
    worst = _worst()
    for e in range(gc.EPOCHS):
        groups = sched.epoch(e)
        assert len(groups) == 1 and len(groups[0]) == case['n']
        ref = gc.reference_steps(om, case, groups, first_step=dm.dropout_step, seed=dm.dropout_seed)
        kind, outs = _device_step(tr, groups[0])
        pb = plain.part_batch(groups[0])
        assert type(pb.matrix).__name__ == 'InducedMatrix'
        pb.dropout = case['flags']['dropout']
        pouts = pm.run_one_step(None, pb, sync=False)
        assert np.float32(float(outs[1])).tobytes() == np.float32(float(pouts[1])).tobytes(), "loss bits differ from plain part steps"
        g1, g2, p1, p2 = dm.get_grads(), pm.get_grads(), dm.get_params(), pm.get_params()
        for key in g1:
            assert g1[key].tobytes() == g2[key].tobytes(), ("grad bits", key)
            assert p1[key].tobytes() == p2[key].tobytes(), ("param bits", key)
        _compare_step(name, "epoch %d" % e, dm, om, next(ref), outs, groups[0], worst)
    assert all(np.isfinite(t).all() for t in _tables(dm) if t is not None)          # every row was pushed
    assert all(bool(torch.isfinite(t).all()) for t in dm.part_scores)               # every score was pushed
    print("%s heads %d: worst rel err  activations %.1e  loss %.1e  grads %.1e  params %.1e"
          % (name, heads, worst['act'], worst['loss'], worst['grad'], worst['param']))


def test_with_the_flag_off_nothing_is_allocated():
    case = gc.build('sage_ln_pp')
    tr = _trainer(case, full_batch_parts=3, attn_heads=2)
    assert not tr.part_pull_gat and not tr.part_history
    assert tr.train_model.part_scores is None and tr.train_model.part_history is None
    assert type(tr.part_batch(tr.part_schedule.epoch(0)[0]).matrix).__name__ == 'InducedMatrix'


# ---- 4. end to end -------------------------------------------------------------------------------------------------------
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
    """s-cora, 2 epochs, P = 4, q = 2, 2 heads, bfloat16 row tables: the set-up line appears once, losses are finite, the
    full-graph one-table evaluation runs, every table ends finite and filled"""
    monkeypatch.chdir(tmp_path)
    argv = ['--dataset', 's-cora', '--full_batch', '--test_full_batch', '--epochs', '2', '--full_batch_parts', '4',
            '--full_batch_parts_per_step', '2', '--full_batch_part_pull_gat', '--aggregator', 'attn', '--attn_score', 'gat',
            '--attn_heads', '2', '--history_dtype', 'bf16']
    tr, out = _run_main(monkeypatch, argv)
    setup = [l for l in out.splitlines() if l.startswith("[sgcn] --full_batch_parts 4:")]
    assert len(setup) == 1 and "(values: history)" in setup[0]
    line = [l for l in out.splitlines() if l.startswith("[sgcn] --full_batch_part_pull_gat: a step attends over")]
    assert len(line) == 1 and " bf16: " in line[0] and "MiB" in line[0] and "score table(s) of %d x 2 fp32" % tr.num_data in line[0]
    assert not [l for l in out.splitlines() if l.startswith("[sgcn] --full_batch_part_history:")
                or l.startswith("[sgcn] --full_batch_part_pull ")]
    print(line[0])
    walls = [l for l in out.splitlines() if l.startswith("[sgcn] epoch train wall")]
    ep = [l for l in out.splitlines() if l.startswith("Epoch:")]
    assert len(ep) == len(walls) and len(ep) >= 2
    assert tr.last_epoch['skipped'] == 0 and tr.last_epoch['steps'] + tr.last_epoch['refreshed'] == 2
    for l in ep:
        tok = l.split()
        assert np.isfinite(float(tok[3])) and np.isfinite(float(tok[7]))
    m = re.search(r"Test set results: cost= (\d+\.\d{5})", out)
    assert m and np.isfinite(float(m.group(1)))
    tables, owned = tr.train_model.part_history
    assert all(t.dtype == torch.bfloat16 for t, o in zip(tables, owned) if o)
    assert all(bool(torch.isfinite(t.float()).all()) and float(t.float().abs().sum()) > 0 for t, o in zip(tables, owned) if o)
    scores = tr.train_model.part_scores
    assert len(scores) == tr.train_model.L and all(t.dtype == torch.float32 and tuple(t.shape) == (tr.num_data, 2) for t in scores)
    assert all(bool(torch.isfinite(t).all()) and float(t.abs().sum()) > 0 for t in scores)
