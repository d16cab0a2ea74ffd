"""GPU tests of --attn_heads in the model: three unsynchronised training steps of the stacks of tests/attn_heads_cases.py against
the fp64-accumulating restatement with heads (tests/attn_heads_ref.py), an evaluation model that allocates no lse and
reproduces the training model's forward at dropout 0, the refusal of a width the heads do not divide, and train.main end to
end at four heads.  Every figure is printed before it is asserted."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

import attn_heads_cases as hx
import full_batch_cases as fc
import spattn_ref as ref
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


def _flags(case):
    return dict(ATTN, attn_heads=case['heads'])


@pytest.mark.parametrize("name", sorted(hx.CASES))
def test_three_steps_match_the_reference(name):
    case = hx.build(name)
    fl, H = case['flags'], case['heads']
    adj, rows = case['train_adj'], np.sort(case['train'])
    om = hx.reference_model(case, case['nbr_train'])
    dm = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in om.params.items()}, extra_flags=_flags(case))
    assert len(dm.layers) == len(om.specs)
    mat, sb = _static_batch(case, adj, dm, rows)
    sb.dropout = fl['dropout']
    feed = fc.exact_feed(case, adj, fl['dropout'])
    worst = dict(act=0.0, grad=0.0, param=0.0, loss=0.0)
    for step in range(3):
        masks = mnp.HashMasks(dm.dropout_seed, dm.dropout_step, 1.0 - fl['dropout'])
        assert (dm.dropout_seed, dm.dropout_step) == (1, step)                 # what attn_heads_cases.margin replayed
        outs = dm.run_one_step(None, sb)
        d_acts, dg, dp = [_np(a) for a in dm.activations[1:]], dm.get_grads(), dm.get_params()
        logits, o_acts, o_loss, o_acc, o_grads = hx.reference_step(om, case, feed, rows, fl['dropout'], masks)
        for kind, li, small, big in om.margins:
            print("%s step %d %s layer %d: smallest non-zero margin %.3e of largest input %.3e" % (name, step, kind, li, small, big))
            assert not np.isfinite(small) or small >= hx.MARGIN * big             # the condition the seed was chosen under
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
            worst['grad'] = max(worst['grad'], e)
            print("%s step %d grad %s rel_err %.3e" % (name, step, k, e))
            assert e <= TOL, (name, step, 'grad', k, e)
        for k, v in om.params.items():
            e = onp.rel_err(dp[k], v)
            worst['param'] = max(worst['param'], e)
            print("%s step %d param %s rel_err %.3e" % (name, step, k, e))
            assert e <= TOL, (name, step, 'param', k, e)
    n = case['n']
    assert all(a._attn and a._heads == H and tuple(a._lse.shape) == (n, H) and a._out is not None for a in dm.aggregators)
    print("%s: worst rel err  activations %.1e  loss %.1e  grads %.1e  params %.1e"
          % (name, worst['act'], worst['loss'], worst['grad'], worst['param']))


@pytest.mark.parametrize("name", sorted(hx.CASES))
def test_evaluation_model_allocates_no_lse_and_agrees(name):
    """the same weights on the same adjacency: the evaluation model's logits are the training model's forward at dropout 0"""
    case = hx.build(name)
    adj, rows = case['train_adj'], np.sort(case['train'])
    params = hx.reference_model(case, case['nbr_train']).params
    tm = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in params.items()}, is_training=False,
                         extra_flags=_flags(case))
    _, sbt = _static_batch(case, adj, tm, rows)
    outs = tm.run_one_step(None, sbt)
    assert np.isfinite(outs[0])
    assert all(a._attn and a._lse is None and a._x is None for a in tm.aggregators)           # nothing kept for a backward
    ev = _np(tm.activations[-1])
    dm = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in params.items()}, extra_flags=_flags(case))
    _, sb = _static_batch(case, adj, dm, rows)
    sb.dropout = 0.0
    dm.run_one_step(None, sb)
    assert all(a._lse is not None for a in dm.aggregators)
    trn = _np(dm.activations[-1])
    assert ev.shape == trn.shape and ref.same_bits(ev, trn)
    om = hx.reference_model(case, case['nbr_train'], params={k: v.copy() for k, v in params.items()})
    logits, _ = om.forward(fc.exact_feed(case, adj, 0.0), case['ph'], 0.0, None)
    e = onp.rel_err(ev, logits)
    print("%s evaluation logits rel_err %.3e" % (name, e))
    assert e <= TOL


def test_a_width_the_heads_do_not_divide_is_refused():
    """hidden1 = 8 under four heads is fine, the 6-wide feature layer of gcn_nopp is not: refused with the layer and the width"""
    case = hx.build('gcn_nopp_h2')
    adj, rows = case['train_adj'], np.sort(case['train'])
    params = hx.reference_model(case, case['nbr_train']).params
    dm = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in params.items()},
                         extra_flags=dict(ATTN, attn_heads=4))
    _, sb = _static_batch(case, adj, dm, rows)
    with pytest.raises(ValueError, match=r"--attn_heads 4 does not divide the input width of \S+ \(6 columns\)") as ei:
        dm.run_one_step(None, sb)
    assert dm.aggregators[0].name in str(ei.value)


def test_trainer_refuses_a_hidden_width_the_heads_do_not_divide(tmp_path, monkeypatch):
    """as soon as the widths are known: after the data is loaded, before a model exists"""
    from stochastic_gcn_amd import train
    monkeypatch.chdir(tmp_path)
    built = []
    monkeypatch.setattr(train, "make_template", lambda *a, **k: built.append(a) or (lambda *a, **k: None))
    with pytest.raises(ValueError, match=r"--attn_heads 4 does not divide the input width of .*--hidden1\) \(30 columns\)"):
        with contextlib.redirect_stdout(io.StringIO()):
            train.main(['--dataset', 's-cora', '--full_batch', '--test_full_batch', '--aggregator', 'attn', '--attn_heads', '4',
                        '--hidden1', '30', '--epochs', '1'])
    assert built == []


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
        train.main(['--dataset', 's-cora', '--full_batch', '--test_full_batch', '--aggregator', 'attn', '--attn_heads', '4',
                    '--epochs', '2'])
    out = buf.getvalue()
    tr = made[0]
    assert tr.attn_aggregator is True and tr.attn_heads == 4
    N = tr.num_data
    assert tr.train_model.aggregators and all(a._attn and a._heads == 4 and tuple(a._lse.shape) == (N, 4)
                                              and a._x.shape[1] == 32 for a in tr.train_model.aggregators)
    assert all(a._attn and a._lse is None for a in tr.test_model.aggregators)
    ep = [l for l in out.splitlines() if l.startswith("Epoch:")]
    assert len(ep) == 4                   # the reference's exit is `epoch > FLAGS.epochs`: epochs + 2
    for line in ep:
        tok = line.split()
        assert np.isfinite(float(tok[3])) and np.isfinite(float(tok[7]))
    print("train loss per epoch:", [float(l.split()[3]) for l in ep])
    m = re.search(r"Test set results: cost= (\d+\.\d{5})", out)
    assert m and np.isfinite(float(m.group(1)))
