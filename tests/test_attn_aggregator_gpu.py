"""GPU tests of --aggregator attn in the model: three unsynchronised training steps of two tiny stacks against an independent
fp64-accumulating restatement (tests/attn_aggregator_ref.py; the cases and the condition that makes the comparison
well-posed: tests/attn_aggregator_cases.py), an evaluation model that allocates no lse and reproduces the training model's
forward at dropout 0, and train.main end to end.  Every figure is printed before it is asserted."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

import attn_aggregator_cases as ax
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


@pytest.mark.parametrize("name", sorted(ax.CASES))
def test_three_steps_match_the_reference(name):
    case = ax.build(name)
    fl = case['flags']
    adj, rows = case['train_adj'], np.sort(case['train'])
    om = ax.reference_model(case, case['nbr_train'])
    dm = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in om.params.items()}, extra_flags=ATTN)
    assert len(dm.layers) == len(om.specs)
    mat, sb = _static_batch(case, adj, dm, rows)
    assert mat.kernel == 'rows' and mat._plan is None            # no sweep plan for products that never run
    sb.dropout = fl['dropout']
    feed = fc.exact_feed(case, adj, fl['dropout'])
    worst = dict(act=0.0, grad=0.0, param=0.0, loss=0.0)
    for step in range(3):
        masks = mnp.HashMasks(dm.dropout_seed, dm.dropout_step, 1.0 - fl['dropout'])
        assert (dm.dropout_seed, dm.dropout_step) == (1, step)                 # what attn_aggregator_cases.margin replayed
        outs = dm.run_one_step(None, sb)
        d_acts, dg, dp = [_np(a) for a in dm.activations[1:]], dm.get_grads(), dm.get_params()
        logits, o_acts, o_loss, o_acc, o_grads = ax.reference_step(om, case, feed, rows, fl['dropout'], masks)
        for kind, li, small, big in om.margins:
            print("%s step %d %s layer %d: smallest non-zero margin %.3e of largest input %.3e" % (name, step, kind, li, small, big))
            assert not np.isfinite(small) or small >= ax.MARGIN * big             # the condition the seed was chosen under
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
    assert all(a._attn and a._lse is not None and a._out is not None for a in dm.aggregators)
    print("%s: worst rel err  activations %.1e  loss %.1e  grads %.1e  params %.1e"
          % (name, worst['act'], worst['loss'], worst['grad'], worst['param']))


@pytest.mark.parametrize("name", sorted(ax.CASES))
def test_evaluation_model_allocates_no_lse_and_agrees(name):
    """the same weights on the same adjacency: the evaluation model's logits are the training model's forward at dropout 0"""
    case = ax.build(name)
    adj, rows = case['train_adj'], np.sort(case['train'])
    params = ax.reference_model(case, case['nbr_train']).params
    tm = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in params.items()}, is_training=False,
                         extra_flags=ATTN)
    _, sbt = _static_batch(case, adj, tm, rows)
    outs = tm.run_one_step(None, sbt)
    assert np.isfinite(outs[0])
    assert all(a._attn and a._lse is None and a._x is None for a in tm.aggregators)           # nothing kept for a backward
    ev = _np(tm.activations[-1])
    dm = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in params.items()}, extra_flags=ATTN)
    _, sb = _static_batch(case, adj, dm, rows)
    sb.dropout = 0.0
    dm.run_one_step(None, sb)
    assert all(a._lse is not None for a in dm.aggregators)
    trn = _np(dm.activations[-1])
    assert ev.shape == trn.shape and ref.same_bits(ev, trn)
    # and both are the reference's forward
    om = ax.reference_model(case, case['nbr_train'], params={k: v.copy() for k, v in params.items()})
    logits, _ = om.forward(fc.exact_feed(case, adj, 0.0), case['ph'], 0.0, None)
    e = onp.rel_err(ev, logits)
    print("%s evaluation logits rel_err %.3e" % (name, e))
    assert e <= TOL


def test_sampled_adjacency_is_refused():
    from stochastic_gcn_amd import layers, ops
    from stochastic_gcn_amd.flags import FLAGS
    import scipy.sparse as sp
    FLAGS.update(**ATTN)

    class Cur(object):
        adj = [ops.DeviceCSR.from_scipy(sp.identity(4, format='csr', dtype=np.float32), DEV)]

    class Model(object):
        cur, is_training = Cur(), True
    agg = layers.PlainAggregator(Model(), 0, name='agg0')
    with pytest.raises(RuntimeError, match="--aggregator attn runs on a full-graph matrix only"):
        agg.forward(torch.zeros(4, 8, device=DEV))


def test_wide_misaligned_operands_are_staged():
    """602-wide features on a pitch of 602 floats (VW = 2: over 512 columns) and a concat output view at a column offset
    of 602: StaticMatrix stages them into aligned scratch tables, allocated once per role and width"""
    from stochastic_gcn_amd import full_batch, ops
    import sparse_cases as sc
    a = sc.pattern("m64_k64")
    m = full_batch.StaticMatrix(a, DEV, 'rows')
    rng = np.random.RandomState(2)
    d = 602
    x = rng.standard_normal((64, d)).astype(np.float32)
    g = rng.standard_normal((64, 2 * d)).astype(np.float32)
    xt, gt = torch.tensor(x).to(DEV), torch.tensor(g).to(DEV)
    assert ops.attn_vw(d, xt) == 2
    scale = d ** -0.5
    out = torch.full((64, 2 * d), float('nan'), device=DEV)
    res, lse = m.attn_product(xt, scale, out=out[:, d:])
    assert res.data_ptr() == out[:, d:].data_ptr() and bool(torch.isnan(out[:, :d]).all().item())
    r = ref.backward_f64(a, x, x, g[:, d:], scale, add=g[:, :d], add_rows=64, fused=True)
    f = r['fwd']
    some = np.diff(a.indptr) > 0
    assert np.all(np.abs(_np(out[:, d:]) - f.C) <= f.bound_C)
    assert np.all(np.abs(_np(lse)[some] - f.lse[some]) <= f.bound_lse[some]) and np.all(_np(lse)[~some] == -np.inf)
    tables = dict(m._scratch)
    dx = m.attn_backward(xt, gt[:, d:], out[:, d:], lse, scale, add=gt[:, :d], add_rows=64)
    assert np.all(np.abs(_np(dx) - r['dx']) <= r['bound_dx'])
    m.attn_product(xt, scale, out=out[:, d:])
    assert all(m._scratch[k] is v for k, v in tables.items())                   # reused, not allocated again


@pytest.mark.parametrize("kind", ["attn", "gat"])
def test_staged_operands_give_the_bits_of_aligned_ones(kind):
    """d = 258 on a pitch of 259 floats (VW = 1: 258 > 256 columns, the smallest width that is staged at all) against the same
    values on a pitch of 260 (VW = 4, served as it is): x, out, g, out_fwd and add all go through StaticMatrix's staging
    helpers, the results of both score kinds are those of the aligned tables to the bit, and a second call allocates nothing"""
    from stochastic_gcn_amd import full_batch, ops
    import sparse_cases as sc
    a = sc.pattern("row_lengths")
    M, K = a.shape
    d, slope = 258, 0.2
    rng = np.random.RandomState(5)
    host = dict(x=rng.standard_normal((K, d)), g=rng.standard_normal((M, d)), add=rng.standard_normal((M, d)))
    av = torch.tensor((rng.standard_normal((2, d)) * d ** -0.5).astype(np.float32)).to(DEV)

    def view(v, pitch):
        t = torch.full((v.shape[0], pitch), float('nan'), device=DEV)
        t[:, :d] = torch.tensor(v.astype(np.float32)).to(DEV)
        return t[:, :d]

    def run(pitch):
        m = full_batch.StaticMatrix(a, DEV, 'rows')
        x, g, add = (view(host[k], pitch) for k in ('x', 'g', 'add'))
        buf = torch.full((M, pitch), float('nan'), device=DEV)
        out = buf[:, :d]
        got, tables = [], None
        for _ in range(2):
            if kind == "attn":
                res, lse = m.attn_product(x, d ** -0.5, out=out)
                back = (m.attn_backward(x, g, out, lse, d ** -0.5, add=add, add_rows=M),)
                fwd = (res, lse)
            else:
                res, lse, S = m.gat_product(x, av, slope, out=out)
                back = m.gat_backward(x, av, S, g, out, lse, slope, add=add, add_rows=M)
                fwd = (res, lse, S)
            assert res.data_ptr() == out.data_ptr() and bool(torch.isnan(buf[:, d:]).all().item())
            got.append([_np(t) for t in fwd + tuple(back)])
            if tables is None:
                tables = dict(m._scratch)
        assert sorted(m._scratch) == sorted(tables) and all(m._scratch[k] is v for k, v in tables.items())
        assert all(ref.same_bits(p, q) for p, q in zip(*got))
        return x, got[0], tables

    x259, staged, tables = run(259)
    x260, aligned, none = run(260)
    assert ops.attn_vw(d, x259) == 1 and ops.attn_vw(d, x260) == 4
    assert sorted(k[1] for k in tables) == ['add', 'g', 'out', 'out_fwd', 'x'] and none == {}
    assert len(staged) == len(aligned) == (3 if kind == "attn" else 5)
    for i, (p, q) in enumerate(zip(staged, aligned)):
        assert p.shape == q.shape and ref.same_bits(p, q), (kind, i)


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
        train.main(['--dataset', 's-cora', '--full_batch', '--test_full_batch', '--aggregator', 'attn', '--epochs', '2'])
    out = buf.getvalue()
    tr = made[0]
    assert tr.attn_aggregator is True and tr.attn_scale == 0.0 and tr.max_aggregator is False
    assert tr.train_sch is None and tr.eval_sch is None
    assert all(m.kernel == 'rows' and m._plan is None for _, m in tr.static_matrices)
    assert all(a._attn and a._lse is not None for a in tr.train_model.aggregators)
    assert all(a._attn and a._lse is None for a in tr.test_model.aggregators)
    ep = [l for l in out.splitlines() if l.startswith("Epoch:")]
    assert len(ep) == 4                   # the reference's exit is `epoch > FLAGS.epochs`: epochs + 2
    for line in ep:
        tok = line.split()
        assert tok[0] == "Epoch:" and tok[2] == "train_loss=" and tok[6] == "val_loss="
        assert np.isfinite(float(tok[3])) and np.isfinite(float(tok[7]))
    print("train loss per epoch:", [float(l.split()[3]) for l in ep])
    m = re.search(r"Test set results: cost= (\d+\.\d{5})", out)
    assert m and np.isfinite(float(m.group(1)))
