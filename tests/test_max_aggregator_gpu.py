"""GPU tests of --aggregator max in the model: the wiring of layers.PlainAggregator at a realistic small size (every max
aggregator's captured input, output, ids and gradients against tests/spmax_ref.py), three unsynchronised training steps of
two tiny stacks against an independent fp64-accumulating restatement (tests/max_aggregator_ref.py; the cases and the
condition that makes the comparison well-posed: tests/max_aggregator_cases.py), --aggregator sum against the run without
the flag, and train.main end to end.  Every figure is printed before it is asserted."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

import full_batch_cases as fc
import max_aggregator_cases as mx
import spmax_ref as ref
from oracle import model_np as mnp
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = torch.device('cuda:0')
MAX = dict(aggregator='max', full_batch=True, test_full_batch=True)


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


@contextlib.contextmanager
def _captured():
    """Every PlainAggregator call inside: (layer, input, output, ids or None) per forward, (layer, g, dx) per backward."""
    from stochastic_gcn_amd import layers
    fwd, bwd = [], []
    real_f, real_b = layers.PlainAggregator.forward, layers.PlainAggregator.backward

    def forward(self, x):
        out = real_f(self, x)
        arg = getattr(self, '_arg', None)
        fwd.append((self, _np(layers.dense_of(x)), _np(out), None if arg is None else _np(arg)))
        return out

    def backward(self, g):
        dx = real_b(self, g)
        bwd.append((self, _np(g), _np(dx)))
        return dx
    layers.PlainAggregator.forward, layers.PlainAggregator.backward = forward, backward
    try:
        yield fwd, bwd
    finally:
        layers.PlainAggregator.forward, layers.PlainAggregator.backward = real_f, real_b


# ---- wiring at a realistic small size ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ['reddit3k_pp', 'reddit3k_nopp'])
def test_wiring_one_step_and_one_evaluation(name):
    case = fc.build(name)
    fl = case['flags']
    assert fl['normalization'] == 'graphsage'                   # concat: the self half and the addend are in play
    params = fc.oracle_model(case, case['nbr_train']).params
    # one training step
    adj, n = case['train_adj'].tocsr(), case['n']
    dm = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in params.items()}, extra_flags=MAX)
    mat, sb = _static_batch(case, adj, dm, case['train'])
    assert mat.kernel == 'rows' and mat._plan is None            # no sweep plan for products that never run
    sb.dropout = fl['dropout']
    with _captured() as (fwd, bwd):
        outs = dm.run_one_step(None, sb)
    assert np.isfinite(outs[1]) and len(fwd) == dm.L and 1 <= len(bwd) <= dm.L
    for agg, x, out, arg in fwd:
        d = x.shape[1]
        C, a_ref = ref.forward(adj, x)
        assert out.shape == (n, 2 * d) and arg is not None and arg.dtype == np.int32
        assert ref.same_bits(out[:, :d], x[:n]), "self half, layer %d" % agg.l
        assert ref.same_bits(out[:, d:], C) and np.array_equal(arg, a_ref), "maximum / ids, layer %d" % agg.l
        print("%s train: layer %d maximum over %d columns: values and ids bit for bit" % (name, agg.l, d))
    by_layer = {agg.l: arg for agg, _, _, arg in fwd}
    for agg, g, dx in bwd:
        d = g.shape[1] // 2
        d64, bound = ref.backward_f64(adj, g[:, d:], by_layer[agg.l], add=g[:, :d], add_rows=n)
        err = np.abs(dx.astype(np.float64) - d64)
        ratio = float(np.max(err / np.maximum(bound, 1e-300)))
        print("%s train: layer %d outgoing gradient: worst |error| / bound %.4f" % (name, agg.l, ratio))
        assert dx.shape == (n, d) and np.all(err <= bound), (name, agg.l, ratio)
        # the addend alone: a vertex nobody's maximum chose receives exactly its self half
        ids = by_layer[agg.l].astype(np.int64)
        t = np.bincount((ids * d + np.arange(d)[None, :])[ids >= 0], minlength=n * d).reshape(n, d)
        assert (t == 0).any() and np.array_equal(dx[t == 0], g[:, :d][t == 0])
    # one evaluation: the same values, no ids allocated
    full = case['full_adj'].tocsr()
    tm = fc.device_model(case, case['nbr_test'], full, {k: v.copy() for k, v in params.items()}, is_training=False,
                         extra_flags=MAX)
    _, sbt = _static_batch(case, full, tm, case['val'])
    with _captured() as (fwd, bwd):
        outs = tm.run_one_step(None, sbt)
    assert np.isfinite(outs[0]) and len(fwd) == tm.L and bwd == []
    for agg, x, out, arg in fwd:
        d = x.shape[1]
        assert arg is None and agg._arg is None                                   # the evaluation model allocates no ids
        assert ref.same_bits(out[:, :d], x[:n]) and ref.same_bits(out[:, d:], ref.forward(full, x)[0])
        print("%s evaluation: layer %d maximum over %d columns: values bit for bit, no ids" % (name, agg.l, d))


# ---- end to end against an independent reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mx.CASES))
def test_three_steps_match_the_reference(name):
    case = mx.build(name)
    fl = case['flags']
    adj, rows = case['train_adj'], np.sort(case['train'])
    om = mx.reference_model(case, case['nbr_train'])
    dm = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in om.params.items()}, extra_flags=MAX)
    assert len(dm.layers) == len(om.specs)
    _, sb = _static_batch(case, adj, dm, rows)
    sb.dropout = fl['dropout']
    feed = fc.exact_feed(case, adj, fl['dropout'])
    worst = dict(act=0.0, grad=0.0, param=0.0, loss=0.0)
    for step in range(3):
        masks = mnp.HashMasks(dm.dropout_seed, dm.dropout_step, 1.0 - fl['dropout'])
        assert (dm.dropout_seed, dm.dropout_step) == (1, step)                 # what max_aggregator_cases.margin replayed
        outs = dm.run_one_step(None, sb)
        d_acts, dg, dp = [_np(a) for a in dm.activations[1:]], dm.get_grads(), dm.get_params()
        logits, o_acts, o_loss, o_acc, o_grads = mx.reference_step(om, case, feed, rows, fl['dropout'], masks)
        for kind, li, small, big in om.margins:
            print("%s step %d %s layer %d: smallest non-zero margin %.3e of largest input %.3e" % (name, step, kind, li, small, big))
            assert not np.isfinite(small) or small >= mx.MARGIN * big             # the condition the seed was chosen under
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
    print("%s: worst rel err  activations %.1e  loss %.1e  grads %.1e  params %.1e"
          % (name, worst['act'], worst['loss'], worst['grad'], worst['param']))


# ---- --aggregator sum is the run without the flag ----------------------------------------------------------------------------
def test_aggregator_sum_is_bit_for_bit_the_run_without_the_flag():
    from stochastic_gcn_amd import ops
    case = fc.build('reddit3k_pp')
    adj, rows = case['train_adj'], np.sort(case['train'])
    params = fc.oracle_model(case, case['nbr_train']).params
    res = []
    for extra in (None, dict(aggregator='sum')):
        dm = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in params.items()}, extra_flags=extra)
        from stochastic_gcn_amd.full_batch import StaticBatch, model_matrix
        mat = model_matrix(adj, DEV, dm, 3, kernel='rows')
        sb = StaticBatch(mat, case['labels'], rows, dm.L, DEV)
        sb.dropout = case['flags']['dropout']
        calls = []
        real = ops.spmax
        ops.spmax = lambda *a, **k: calls.append(1) or real(*a, **k)
        try:
            outs = dm.run_one_step(None, sb)
        finally:
            ops.spmax = real
        assert calls == [] and mat.rows_csr.plan.ws_ids is None                   # nothing of the maximum runs or is allocated
        assert all(getattr(a, '_arg', None) is None for a in dm.aggregators)
        res.append((outs[1], outs[2], dm.get_grads(), dm.get_params(), [_np(a) for a in dm.activations[1:]]))
    (l0, a0, g0, p0, x0), (l1, a1, g1, p1, x1) = res
    assert l0 == l1 and a0 == a1
    assert all(ref.same_bits(g0[k], g1[k]) for k in g0) and all(ref.same_bits(p0[k], p1[k]) for k in p0)
    assert all(ref.same_bits(u, v) for u, v in zip(x0, x1))


# ---- train.main ------------------------------------------------------------------------------------------------------------
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
        train.main(['--dataset', 's-cora', '--scale', '0.25', '--full_batch', '--test_full_batch', '--aggregator', 'max',
                    '--epochs', '2'])
    out = buf.getvalue()
    tr = made[0]
    assert tr.max_aggregator is True and tr.train_sch is None and tr.eval_sch is None
    assert all(m.kernel == 'rows' and m._plan is None for _, m in tr.static_matrices)
    assert all(a._max and a._arg is not None for a in tr.train_model.aggregators)
    assert all(a._max and a._arg is None for a in tr.test_model.aggregators)
    ep = [l for l in out.splitlines() if l.startswith("Epoch:")]
    assert len(ep) == 4                   # the reference's exit is `epoch > FLAGS.epochs`: epochs + 2
    for line in ep:
        tok = line.split()
        assert tok[0] == "Epoch:" and tok[2] == "train_loss=" and tok[4] == "train_acc=" and tok[6] == "val_loss="
        assert tok[8] == "val_acc=" and "time=" in tok and "ttime=" in tok
        assert np.isfinite(float(tok[3])) and np.isfinite(float(tok[7]))
    print("train loss per epoch:", [float(l.split()[3]) for l in ep])
    assert "over 1 steps" in out
    m = re.search(r"Test set results: cost= (\d+\.\d{5}) accuracy= (\d+\.\d{5}) mi F1=(\d+\.\d{5}) ma F1=(\d+\.\d{5})", out)
    assert m and np.isfinite(float(m.group(1)))
