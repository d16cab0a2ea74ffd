"""GPU tests of --attn_score gat in the model: three unsynchronised training steps of two tiny stacks (and of both with
--attn_dropout 0.2) against an independent fp64-accumulating restatement (tests/gat_aggregator_ref.py; the cases and the two
conditions that make the comparison well-posed: tests/gat_aggregator_cases.py) at the project's plain 1e-4 -- activations,
every gradient including agg*/attn_vec, the weights after each Adam step; an evaluation model that keeps no lse; checkpoints,
the Polyak average and weight decay with a parametrised aggregator; --attn_score dot as the run without the flag, bit for bit;
two gat runs with identical weights; and train.main end to end.  Every figure is printed before it is asserted."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

import attn_aggregator_cases as ax
import full_batch_cases as fc
import gat_aggregator_cases as gc
import spgat_ref as ref
from oracle import model_np as mnp
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
TOL = 1e-4                 # the project's standing tolerance for model steps
DEV = torch.device('cuda:0')
ATTN = dict(aggregator='attn', full_batch=True, test_full_batch=True)


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


def _static_batch(case, adj, model, rows):
    from stochastic_gcn_amd.full_batch import StaticBatch, model_matrix
    mat = model_matrix(adj, DEV, model, 3)
    return mat, StaticBatch(mat, case['labels'], np.sort(rows), model.L, DEV)


def _device_steps(case, params, extra, steps=3):
    """the weights after ``steps`` training steps of a fresh device model"""
    adj, rows = case['train_adj'], np.sort(case['train'])
    dm = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in params.items()}, extra_flags=extra)
    _, sb = _static_batch(case, adj, dm, rows)
    sb.dropout = case['flags']['dropout']
    for _ in range(steps):
        dm.run_one_step(None, sb)
    return dm, dm.get_params()


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_three_steps_match_the_reference(name):
    case = gc.build(name)
    fl = case['flags']
    adj, rows = case['train_adj'], np.sort(case['train'])
    om = gc.reference_model(case, case['nbr_train'])
    dm = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in om.params.items()}, extra_flags=gc.extra_flags(case))
    assert len(dm.layers) == len(om.specs) and set(dm.get_params()) == set(om.params)
    assert sum(k.endswith('/attn_vec') for k in om.params) == case['L']
    if not fl['preprocess']:
        # agg0 is the first parametrised layer and forms no dX; weight decay covers dense0/weights alone
        assert dm.layers[dm._first_param].name == 'agg0' and dm.layers[dm._first_param].need_dx is False
        lo, hi = dm._wd_range
        span = {n: (off, off + cnt) for n, _, _, off, cnt in dm._layout}
        assert (lo, hi) == span['dense0/weights'] and fl['weight_decay'] > 0
    mat, sb = _static_batch(case, adj, dm, rows)
    sb.dropout = fl['dropout']
    feed = fc.exact_feed(case, adj, fl['dropout'])
    worst = dict(act=0.0, grad=0.0, param=0.0, loss=0.0, vec=0.0)
    for step in range(3):
        masks = mnp.HashMasks(dm.dropout_seed, dm.dropout_step, 1.0 - fl['dropout'])
        assert (dm.dropout_seed, dm.dropout_step) == (1, step)                 # what gat_aggregator_cases.margins replayed
        outs = dm.run_one_step(None, sb)
        d_acts, dg, dp = [_np(a) for a in dm.activations[1:]], dm.get_grads(), dm.get_params()
        logits, o_acts, o_loss, o_acc, o_grads = gc.reference_step(om, case, feed, rows, fl['dropout'], masks, 1, step)
        for kind, li, small, big in om.margins:
            print("%s step %d %s layer %d: smallest non-zero margin %.3e of largest input %.3e" % (name, step, kind, li, small, big))
            assert not np.isfinite(small) or small >= gc.MARGIN * big
        for li, ratio in om.zratios:
            print("%s step %d aggregation layer %d: smallest |z| / its fp32 error bound %.1f" % (name, step, li, ratio))
            assert ratio >= gc.ZMARGIN                                            # no LeakyReLU branch within rounding
        assert len(d_acts) == len(o_acts) and masks.calls > 0
        for li, (da, oa) in enumerate(zip(d_acts, o_acts)):
            e = onp.rel_err(da, oa)
            worst['act'] = max(worst['act'], e)
            print("%s step %d layer %d rel_err %.3e" % (name, step, li, e))
            assert da.shape == oa.shape and e <= TOL, (name, step, li, e)
        print("%s step %d loss %.7f (reference %.7f)  acc %.6f (%.6f)" % (name, step, outs[1], o_loss, outs[2], o_acc))
        worst['loss'] = max(worst['loss'], abs(outs[1] - o_loss) / max(abs(o_loss), 1e-30))
        assert abs(outs[1] - o_loss) <= TOL * abs(o_loss) and abs(outs[2] - o_acc) <= 1e-6
        for k, g in o_grads.items():
            e = onp.rel_err(dg[k], g)
            worst['vec' if k.endswith('attn_vec') else 'grad'] = max(worst['vec' if k.endswith('attn_vec') else 'grad'], e)
            print("%s step %d grad %s rel_err %.3e  (largest |g| %.3e)" % (name, step, k, e, float(np.abs(g).max())))
            assert e <= TOL, (name, step, 'grad', k, e)
            if k.endswith('attn_vec'):
                assert np.abs(g).max() > 0
        for k, v in om.params.items():
            e = onp.rel_err(dp[k], v)
            worst['param'] = max(worst['param'], e)
            print("%s step %d param %s rel_err %.3e" % (name, step, k, e))
            assert e <= TOL, (name, step, 'param', k, e)
    assert all(a._attn and a._gat_on and a._lse is not None and a._S is not None for a in dm.aggregators)
    print("%s: worst rel err  activations %.1e  loss %.1e  grads %.1e  attn_vec grads %.1e  params %.1e"
          % (name, worst['act'], worst['loss'], worst['grad'], worst['vec'], worst['param']))


@pytest.mark.parametrize("name", ['sage_ln_pp_gat', 'gcn_nopp_h2_gat_p2'])
def test_evaluation_model_keeps_no_lse_and_agrees(name):
    """the same weights on the same adjacency: the evaluation model's logits are the training model's forward at dropout 0 and
    without coefficient dropout (an evaluation never masks)"""
    case = gc.build(name)
    adj, rows = case['train_adj'], np.sort(case['train'])
    params = gc.reference_model(case, case['nbr_train']).params
    extra = gc.extra_flags(case)
    tm = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in params.items()}, is_training=False, extra_flags=extra)
    _, sbt = _static_batch(case, adj, tm, rows)
    outs = tm.run_one_step(None, sbt)
    assert np.isfinite(outs[0])
    assert all(a._gat_on and a._lse is None and a._x is None and a._S is None for a in tm.aggregators)
    ev = _np(tm.activations[-1])
    dm = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in params.items()},
                         extra_flags=dict(extra, attn_dropout=0.0))
    _, sb = _static_batch(case, adj, dm, rows)
    sb.dropout = 0.0
    dm.run_one_step(None, sb)
    trn = _np(dm.activations[-1])
    assert ev.shape == trn.shape and ref.same_bits(ev, trn)
    om = gc.reference_model(case, case['nbr_train'], params={k: v.copy() for k, v in params.items()}, is_training=False)
    logits, _ = om.forward(fc.exact_feed(case, adj, 0.0), case['ph'], 0.0, None)
    e = onp.rel_err(ev, logits)
    print("%s evaluation logits rel_err %.3e" % (name, e))
    assert e <= TOL


def test_checkpoint_round_trip_carries_attn_vec(tmp_path):
    case = gc.build('gcn_nopp_h2_gat')
    params = gc.reference_model(case, case['nbr_train']).params
    extra = gc.extra_flags(case)
    dm, after = _device_steps(case, params, extra, steps=2)
    path = dm.save(path=str(tmp_path / "gat.ckpt.npz"))
    z = np.load(path)
    assert {"var/agg0/attn_vec", "var/agg1/attn_vec"} <= set(z.files) and ref.same_bits(z["var/agg0/attn_vec"], after['agg0/attn_vec'])
    fresh = fc.device_model(case, case['nbr_train'], case['train_adj'], {k: np.zeros_like(v) for k, v in params.items()}, extra_flags=extra)
    fresh.load(path=path)
    got = fresh.get_params()
    assert all(ref.same_bits(got[k], after[k]) for k in after) and np.abs(after['agg1/attn_vec'] - params['agg1/attn_vec']).max() > 0


def test_polyak_evaluation_reads_the_averaged_attn_vec():
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.models import make_template
    from stochastic_gcn_amd.plaingcn import PlainGCN
    case = gc.build('gcn_nopp_h2_gat')
    fl = case['flags']
    params = gc.reference_model(case, case['nbr_train']).params
    FLAGS.reset()
    FLAGS.update(**{k: v for k, v in fl.items() if hasattr(FLAGS, k)})
    FLAGS.update(**gc.extra_flags(case), polyak_decay=0.9)
    create = make_template('model', lambda is_training, _store=None: PlainGCN(
        fl['num_layers'], fl['preprocess'], case['ph'], case['feats'], case['nbr_train'], case['train_adj'], False, multitask=False,
        is_training=is_training, device=DEV, _store=_store))
    tm, em = create(True), create(False)
    tm.set_params({k: v.copy() for k, v in params.items()})
    tm.reset_average()
    _, sb = _static_batch(case, case['train_adj'], tm, np.sort(case['train']))
    sb.dropout = fl['dropout']
    from stochastic_gcn_amd import ops
    st = tm._store
    raw, avg = dict(tm._named_views(st.theta)), dict(tm._named_views(st.average))
    keys = ['agg%d/attn_vec' % l for l in range(len(em.aggregators))]
    dec, om = (np.float32(v) for v in ops.polyak_factors(0.9))
    want = {k: params[k].copy() for k in keys}
    for _ in range(3):
        tm.run_one_step(None, sb)
        for k in keys:                     # avg <- fl(fl(avg * decay) + fl(theta_new * fl(1 - decay))), restated in fp32
            want[k] = (want[k] * dec).astype(np.float32) + (_np(raw[k]) * om).astype(np.float32)
    for l, agg in enumerate(em.aggregators):
        k = keys[l]
        assert agg.vars['attn_vec'].data_ptr() == avg[k].data_ptr() != raw[k].data_ptr()       # the evaluation model's view
        assert tm.aggregators[l].vars['attn_vec'].data_ptr() == raw[k].data_ptr()
        assert not torch.equal(avg[k], raw[k]) and np.abs(_np(raw[k]) - params[k]).max() > 0
        assert ref.same_bits(_np(avg[k]), want[k])
    _, sbe = _static_batch(case, case['train_adj'], em, np.sort(case['train']))
    assert np.isfinite(em.run_one_step(None, sbe)[0])


@pytest.mark.parametrize("base", sorted(ax.CASES))
def test_dot_is_the_run_without_the_flag_bit_for_bit(base):
    case = ax.build(base)
    params = ax.reference_model(case, case['nbr_train']).params
    _, off = _device_steps(case, params, dict(ATTN, attn_heads=2, attn_dropout=0.2))
    dm, dot = _device_steps(case, params, dict(ATTN, attn_heads=2, attn_dropout=0.2, attn_score='dot'))
    assert set(off) == set(dot) and all(ref.same_bits(off[k], dot[k]) for k in off)
    assert not any(k.endswith('attn_vec') for k in dot) and all(not a._gat_on for a in dm.aggregators)


@pytest.mark.parametrize("name", ['sage_ln_pp_gat_p2', 'gcn_nopp_h2_gat_p2'])
def test_two_runs_give_identical_weights(name):
    case = gc.build(name)
    params = gc.reference_model(case, case['nbr_train']).params
    _, a = _device_steps(case, params, gc.extra_flags(case))
    _, b = _device_steps(case, params, gc.extra_flags(case))
    assert all(ref.same_bits(a[k], b[k]) for k in a) and any(not ref.same_bits(a[k], params[k]) for k in a if k.endswith('attn_vec'))


def test_train_main_end_to_end(tmp_path, monkeypatch):
    from stochastic_gcn_amd import train
    monkeypatch.chdir(tmp_path)
    made = []
    real = train.Trainer

    class Keep(real):
        def __init__(self, *a, **k):
            made.append(self)
            super(Keep, self).__init__(*a, **k)
    monkeypatch.setattr(train, "Trainer", Keep)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train.main(['--dataset', 's-cora', '--full_batch', '--test_full_batch', '--aggregator', 'attn', '--attn_score', 'gat',
                    '--attn_heads', '4', '--epochs', '2'])
    out = buf.getvalue()
    tr = made[0]
    assert tr.attn_aggregator is True and tr.attn_gat is True and tr.attn_slope == 0.2 and tr.attn_heads == 4
    assert all(a._gat_on and a._lse is not None and tuple(a._lse.shape)[1] == 4 for a in tr.train_model.aggregators)
    assert all(a._gat_on and a._lse is None for a in tr.test_model.aggregators)
    names = [n for n, _ in tr.train_model._store.layout]
    assert sum(n.endswith('/attn_vec') for n in names) == len(tr.train_model.aggregators)
    ep = [l for l in out.splitlines() if l.startswith("Epoch:")]
    assert len(ep) == 4                   # the reference's exit is `epoch > FLAGS.epochs`: epochs + 2
    for line in ep:
        tok = line.split()
        assert tok[0] == "Epoch:" and tok[2] == "train_loss=" and tok[6] == "val_loss="
        assert np.isfinite(float(tok[3])) and np.isfinite(float(tok[7]))
    print("train loss per epoch:", [float(l.split()[3]) for l in ep])
    m = re.search(r"Test set results: cost= (\d+\.\d{5})", out)
    assert m and np.isfinite(float(m.group(1)))
