"""GPU tests of exact full-graph training and evaluation (--full_batch / --test_full_batch, stochastic_gcn_amd/full_batch.py).

Against the oracle: the exact feed is built by hand (full_batch_cases.exact_feed) and drives oracle/model_np.Model --
forward over all N rows, the loss on the gathered subset rows, dlogits scattered into zeros, backward, Adam -- for three
steps with the product's hash masks replayed.  The gate is the project's own (as test_model_gpu.py):
max|x - ref| / max(|ref|, tiny) <= 1e-4 on every layer output, the logits, the loss, the gradients and the weights
after each step, three unsynchronised steps, nothing re-based.  (The weights' seeds are chosen with the oracle alone so that
it has no ReLU input within fp32 rounding of zero: full_batch_cases.CASES.)  Against the code that exists: the same mathematics through the sampler (--nocv --degree 10000, one
batch of all train ids).  Every figure is printed before it is asserted."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

import full_batch_cases as fc
from oracle import model_np as mnp
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = torch.device('cuda:0')


def _np(x):
    if isinstance(x, tuple):
        return tuple(_np(t) for t in x)
    if hasattr(x, 'csr'):
        return None
    if hasattr(x, 'materialize'):
        x = x.materialize()
    return x.detach().cpu().numpy()


def _static_batch(case, adj, model, rows, kernel, products=3):
    from stochastic_gcn_amd.full_batch import StaticBatch, model_matrix
    mat = model_matrix(adj, DEV, model, products, kernel=kernel)
    assert mat.kernel == kernel
    return StaticBatch(mat, case['labels'], np.sort(rows), model.L, DEV)


def _oracle_step(om, case, feed, rows, dropout, masks):
    """One exact step of the oracle with the loss over ``rows``: nothing the device computed enters."""
    logits, acts = om.forward(feed, case['ph'], dropout, masks)
    loss, acc, _, dl = om.loss_and_grad(logits[rows], case['labels'][rows])
    dout = np.zeros_like(logits)
    dout[rows] = dl
    grads = om.backward(dout)
    om.adam_step(grads)
    return logits, acts, float(loss), float(acc), grads


KERNEL_CASES = [(n, k) for n in sorted(fc.CASES) for k in fc.CASES[n]['kernels']]


@pytest.mark.parametrize("name,kernel", KERNEL_CASES)
def test_full_batch_steps_match_oracle(name, kernel):
    from stochastic_gcn_amd import ops
    case = fc.build(name)
    fl = case['flags']
    adj, rows = case['train_adj'], np.sort(case['train'])
    om = fc.oracle_model(case, case['nbr_train'])
    dm = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in om.params.items()})
    assert len(dm.layers) == len(om.specs)
    sb = _static_batch(case, adj, dm, rows, kernel)
    if kernel == 'lds':
        assert ops.LdsSweepCSR.for_graph(adj, DEV) is not None, "the planner must accept this graph"
    sb.dropout = fl['dropout']
    feed = fc.exact_feed(case, adj, fl['dropout'])
    worst = dict(act=0.0, grad=0.0, param=0.0, loss=0.0)
    for step in range(3):
        masks = mnp.HashMasks(dm.dropout_seed, dm.dropout_step, 1.0 - fl['dropout'])
        outs = dm.run_one_step(None, sb)
        d_acts, dg, dp = [_np(a) for a in dm.activations[1:]], dm.get_grads(), dm.get_params()
        logits, o_acts, o_loss, o_acc, o_grads = _oracle_step(om, case, feed, rows, fl['dropout'], masks)
        assert fl['dropout'] == 0 or masks.calls > 0
        assert len(d_acts) == len(o_acts)
        for li, (da, oa) in enumerate(zip(d_acts, o_acts)):
            if da is None or hasattr(oa, 'tocsr'):
                continue
            e = onp.rel_err(da, oa)
            worst['act'] = max(worst['act'], e)
            print("%s/%s step %d layer %d rel_err %.3e" % (name, kernel, step, li, e))
            assert da.shape == oa.shape and e <= TOL, (name, kernel, step, li, e)
        e = onp.rel_err(d_acts[-1], logits)
        print("%s/%s step %d logits rel_err %.3e  loss %.7f (oracle %.7f)  acc %.6f (%.6f)"
              % (name, kernel, step, e, outs[1], o_loss, outs[2], o_acc))
        assert e <= TOL
        worst['loss'] = max(worst['loss'], abs(outs[1] - o_loss) / max(abs(o_loss), 1e-30))
        assert abs(outs[1] - o_loss) <= TOL * abs(o_loss), (outs[1], o_loss)
        assert abs(outs[2] - o_acc) <= 1e-6
        for k, g in o_grads.items():
            e = onp.rel_err(dg[k], g)
            worst['grad'] = max(worst['grad'], e)
            print("%s/%s step %d grad %s rel_err %.3e" % (name, kernel, step, k, e))
            assert e <= TOL, (name, kernel, step, 'grad', k, e)
        for k, v in om.params.items():
            e = onp.rel_err(dp[k], v)
            worst['param'] = max(worst['param'], e)
            print("%s/%s step %d param %s rel_err %.3e" % (name, kernel, step, k, e))
            assert e <= TOL, (name, kernel, step, 'param', k, e)
    # the epoch counters count nnz and N per layer
    dm.init_counts()
    dm.run_one_step(None, sb)
    assert list(dm.adj_sizes) == [adj.nnz] * dm.L and list(dm.field_sizes) == [case['n']] * (dm.L + 1)
    assert dm.amt_data == adj.nnz * dm.L and list(dm.fadj_sizes) == [0] * dm.L and (dm.L == 0 or dm.g_ops > 0) and dm.nn_ops > 0
    print("%s/%s: worst rel err  activations %.1e  loss %.1e  grads %.1e  params %.1e"
          % (name, kernel, worst['act'], worst['loss'], worst['grad'], worst['param']))


def test_unaligned_width_runs_on_the_row_kernel():
    """reddit3k_nopp_odd under cs: the first aggregation (22 columns) falls back product by product; the second (32) sweeps."""
    from stochastic_gcn_amd import ops
    case = fc.build('reddit3k_nopp_odd')
    om = fc.oracle_model(case, case['nbr_train'])
    dm = fc.device_model(case, case['nbr_train'], case['train_adj'], om.params)
    sb = _static_batch(case, case['train_adj'], dm, case['train'], 'cs')
    calls = []
    real_rows, real_cs = ops.spmm, ops.spmm_cs
    try:
        ops.spmm = lambda A, B, **kw: calls.append(('rows', int(B.shape[1]))) or real_rows(A, B, **kw)
        ops.spmm_cs = lambda A, B, **kw: (None if A._tuning else calls.append(('cs', int(B.shape[1])))) or real_cs(A, B, **kw)
        dm.run_one_step(None, sb)
    finally:
        ops.spmm, ops.spmm_cs = real_rows, real_cs
    assert sorted(set(calls)) == [('cs', 32), ('rows', 22)], calls
    # the first aggregation has no backward (nothing in front of it has parameters); the second runs forward and backward
    assert calls.count(('rows', 22)) == 1 and calls.count(('cs', 32)) == 2


def test_multiply_takes_a_width_off_the_vector_size_on_a_padded_pitch_on_every_kernel():
    """StaticMatrix.multiply (what train.pp_products calls) makes no alignment decision: 130 columns -- two 128-column
    passes, no multiple of 4 -- as a view of a 132-float pitch run on the kernel that was asked for.  1,000 vertices in 8
    planted communities (p_in 0.95, ~20 k nonzeros): no multiple of the LDS sweep's 768-row tile or the sweep's 16-row bins.
    Against SciPy in float64 with the bound of the pp tests (tests/test_train_gpu.py): max|got - ref| <= 1e-4 max|ref|."""
    from stochastic_gcn_amd import synthetic
    from stochastic_gcn_amd.full_batch import StaticMatrix
    a = synthetic.reddit_sbm(n=1000, m=10000, classes=8, splits=(600, 100, 300), p_in=0.95, seed=3)[2]
    assert a.shape == (1000, 1000) and 15000 <= a.nnz <= 21000
    X = np.random.RandomState(0).standard_normal((1000, 130)).astype(np.float32)
    ref = a.astype(np.float64).dot(X.astype(np.float64))
    x = torch.zeros((1000, 132), dtype=torch.float32, device=DEV)[:, :130]
    x.copy_(torch.from_numpy(X))
    assert x.stride(0) == 132
    for kernel in ('rows', 'cs', 'lds'):
        m = StaticMatrix(a, DEV, kernel, 3, 130)
        assert m.kernel == kernel and m.kernel_for(x) == 'rows'          # (product would fall back; multiply does not)
        got = m.multiply(x)
        assert tuple(got.shape) == (1000, 130)
        err = np.abs(got.cpu().numpy() - ref).max()
        print("multiply on %s: max err %.3e, bound %.3e" % (kernel, err, 1e-4 * np.abs(ref).max()))
        assert err <= 1e-4 * np.abs(ref).max(), kernel
        if kernel == 'cs':
            assert 130 in m._plan.pace                                    # tuned by the first product ...
            assert torch.equal(m.multiply(x), got)                        # ... and the second one is the same product
        assert m.describe(130)['products'] == 3


@pytest.mark.parametrize("name", ['cora', 'pubmed', 'reddit3k_pp', 'reddit3k_nopp', 'multilabel'])
def test_full_batch_matches_the_sampled_exact_route(name):
    """The parent's way to the same mathematics: --nocv --degree 10000 with ONE batch of all train ids, through the sampler
    and the minibatch kernels.  Loss, accuracy and the weights after three steps agree within 1e-4 (the vertex order
    differs, so the sums do too: not bit-identical).  Dropout is off in this comparison: the masks are a hash of the
    element index, and the two routes number the rows differently."""
    from stochastic_gcn_amd.scheduler import PyScheduler
    case = fc.build(name)
    adj, rows, L, ph = case['train_adj'], np.sort(case['train']), case['L'], case['ph']
    params = fc.oracle_model(case, case['nbr_train']).params
    off = dict(dropout=0.0)
    full = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in params.items()}, extra_flags=off)
    sb = _static_batch(case, adj, full, rows, 'cs')
    res_full = [full.run_one_step(None, sb)[1:] for _ in range(3)]
    p_full = full.get_params()
    samp = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in params.items()}, extra_flags=off)
    sch = PyScheduler(adj, case['labels'], L, [10000] * L, ph, 1, data=case['train'].copy(), cv=False)
    res_samp = []
    for _ in range(3):
        sch.start = 0
        feed = sch.minibatch(len(rows))
        assert feed[ph['fields'][-1]].shape[0] == len(rows)
        feed[ph['dropout']] = 0.0
        res_samp.append(samp.run_one_step(None, feed)[1:])
    p_samp = samp.get_params()
    for step, ((lf, af), (ls, as_)) in enumerate(zip(res_full, res_samp)):
        print("%s step %d: loss %.7f vs %.7f  acc %.6f vs %.6f" % (name, step, lf, ls, af, as_))
        assert abs(lf - ls) <= TOL * abs(ls) and abs(af - as_) <= TOL
    for k in p_samp:
        e = onp.rel_err(p_full[k], p_samp[k])
        print("%s weights %s rel_err %.3e" % (name, k, e))
        assert e <= TOL, (name, k, e)


def _trainer(case, **flags):
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.train import Trainer
    FLAGS.reset()
    FLAGS.update(dataset='ppi' if case['multitask'] else 's-reddit', seed=1, prefetch=0,
                 test_preprocess=case['flags']['preprocess'],
                 **{k: v for k, v in case['flags'].items() if hasattr(FLAGS, k)})
    FLAGS.update(**flags)
    with contextlib.redirect_stdout(io.StringIO()):
        return Trainer(data=case['data'], verbose=False)


@pytest.mark.parametrize("name", ['cora', 'reddit3k_pp', 'reddit3k_nopp', 'multilabel'])
def test_exact_evaluation_matches_oracle_and_its_own_f1(name):
    from stochastic_gcn_amd.utils import calc_f1, f1_from_classes
    case = fc.build(name)
    tr = _trainer(case, test_full_batch=True, full_batch_kernel='cs')
    assert tr.eval_sch is None and tr.eval_slots == [] and tr.train_sch is not None
    loss, acc, micro, macro, _ = tr.evaluate(tr.val_d)
    d_logits = tr.test_model.outputs.cpu().numpy()
    assert d_logits.shape == (case['n'], case['classes'])
    om = fc.oracle_model(case, case['nbr_test'], params=tr.test_model.get_params(), is_training=False)
    feed = fc.exact_feed(case, case['full_adj'], 0.0)
    o_logits, _ = om.forward(feed, case['ph'], 0.0, lambda *a: None)
    rows = np.sort(case['val'])
    o_loss, o_acc, _, _ = om.loss_and_grad(o_logits[rows], case['labels'][rows])
    e = onp.rel_err(d_logits, o_logits)
    print("%s: exact logits rel_err %.3e  loss %.7f (oracle %.7f)  acc %.6f (%.6f)" % (name, e, loss, o_loss, acc, o_acc))
    assert e <= TOL and abs(loss - float(o_loss)) <= TOL * abs(float(o_loss)) and abs(acc - float(o_acc)) <= 1e-6
    if case['multitask']:
        p = 1.0 / (1.0 + np.exp(-d_logits[rows].astype(np.float64)))
        want = calc_f1(p.astype(np.float32), case['labels'][rows], True)
        assert abs(micro - want[0]) <= 1e-6 and abs(macro - want[1]) <= 1e-6
    else:
        want = f1_from_classes(case['labels'][rows].argmax(1), d_logits[rows].argmax(1))
        assert (micro, macro) == tuple(want)
    # validation and test after the same epoch share ONE forward: the logits are cached per weight version
    fwd = []
    real = tr.test_model.forward
    tr.test_model.forward = lambda cur: fwd.append(1) or real(cur)
    again = tr.evaluate(tr.val_d)
    t_loss = tr.evaluate(tr.test_d)[0]
    assert fwd == [] and again[:4] == (loss, acc, micro, macro) and t_loss != loss
    tr.test_model.theta.mul_(1.0)                    # an in-place write of the weights: a new version
    tr.evaluate(tr.val_d)
    assert fwd == [1]


def test_cv_trained_model_scores_the_same_exactly_and_by_exact_batches(tmp_path):
    """A model trained three epochs with --cv --cvd evaluates under --test_full_batch and under --notest_cv --test_degree
    10000 batches to the same loss within 1e-4; the weights travel through a checkpoint (weights only)."""
    case = fc.build('reddit3k_pp')
    common = dict(cv=True, cvd=True, degree=1, batch_size=256, test_batch_size=256)
    a = _trainer(case, test_full_batch=True, **common)
    assert a.train_sch is not None and a.full_batch is False
    for _ in range(3):
        a.train_epoch()
    exact = a.evaluate(a.val_d)
    path = a.train_model.save(path=str(tmp_path / "cv.ckpt.npz"))
    b = _trainer(case, test_cv=False, test_degree=10000, **common)
    b.train_model.load(path=path)
    batched = b.evaluate(b.val_d)
    c = _trainer(case, test_full_batch=True, full_batch_kernel='rows', **common)
    c.train_model.load(path=path)
    exact_rows = c.evaluate(c.val_d)
    print("exact %r\nrows  %r\nbatched %r" % (exact[:4], exact_rows[:4], batched[:4]))
    for other in (batched, exact_rows):
        assert abs(exact[0] - other[0]) <= TOL * abs(other[0])
        assert abs(exact[1] - other[1]) <= 2.0 / len(a.val_d)            # a tie of two logits may fall either way


def test_train_main_end_to_end(tmp_path, monkeypatch):
    from stochastic_gcn_amd import train
    from stochastic_gcn_amd.flags import FLAGS
    monkeypatch.chdir(tmp_path)
    made = []
    real = train.Trainer

    class Keep(real):
        def __init__(self, *a, **k):
            made.append(self)
            super(Keep, self).__init__(*a, **k)
    monkeypatch.setattr(train, "Trainer", Keep)
    FLAGS.reset()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train.main(['--dataset', 's-cora', '--full_batch', '--test_full_batch', '--epochs', '5'])
    out = buf.getvalue()
    tr = made[0]
    assert tr.train_sch is None and tr.eval_sch is None and tr.slots == [] and tr.eval_slots == []      # no sampler, no staging
    assert getattr(tr.train_model, '_programs', None) in (None, {})                                      # no step program
    ep = [l for l in out.splitlines() if l.startswith("Epoch:")]
    assert len(ep) == 7                   # the reference's exit is `epoch > FLAGS.epochs`: epochs + 2
    tok = ep[0].split()
    assert tok[0] == "Epoch:" and tok[2] == "train_loss=" and tok[4] == "train_acc=" and tok[6] == "val_loss="
    assert tok[8] == "val_acc=" and "time=" in tok and "ttime=" in tok and "(sch" in tok and "data" in tok
    assert re.search(r"TF time = .*, g time = .*, G GFLOPS = .*, NN GFLOPS = .*, field sizes = \[2708\. 2708\.\], adj sizes = ", out)
    assert "over 1 steps" in out
    losses = [float(l.split()[3]) for l in ep]
    print("train loss per epoch:", losses)
    assert losses[4] < losses[0]
    m = re.search(r"Test set results: cost= (\d+\.\d{5}) accuracy= (\d+\.\d{5}) mi F1=(\d+\.\d{5}) ma F1=(\d+\.\d{5})", out)
    assert m
    res = tr.evaluate(tr.test_d)
    assert tuple("%.5f" % v for v in res[:4]) == m.groups()
    # checkpoint (weights only): save -> clobber -> load -> identical evaluation
    path = tr.train_model.save(path=str(tmp_path / "fb.ckpt.npz"))
    tr.train_model.theta.zero_()
    assert tr.evaluate(tr.test_d)[:4] != res[:4]
    tr.test_model.load(path=path)
    assert tr.evaluate(tr.test_d)[:4] == res[:4]


def _sample_rows(adj, ids, n, seed=11, k=2000, heavy=32):
    """A seeded sample of rows that always includes the heaviest rows and the first and last id of the loss subset."""
    deg = np.diff(adj.indptr)
    heaviest = np.argsort(deg)[-heavy:]
    rng = np.random.RandomState(seed)
    return np.unique(np.concatenate([rng.choice(n, k, replace=False), heaviest, [ids.min(), ids.max()]])).astype(np.int64)


def test_full_size_reddit_full_batch_step_and_evaluation_match_oracle():
    """The S-Reddit README recipe without --cv at FULL size (N = 232,965, 602 features, 10.1 M training / 23.2 M full
    nonzeros): one --full_batch training step (column sweep) and one --test_full_batch evaluation against the NumPy oracle
    on the hand-built exact feed, with the checker and gate of test_model_gpu.test_full_size_reddit_cvd_pp_steps_match_oracle
    (rel_err <= 1e-4 per layer) on a seeded sample of rows that includes the heaviest rows and the first and last train id;
    the loss at 1e-4.  Nothing computed on the device is fed to the oracle.

    The first-layer weight gradient of the training step -- through the product by A^T on the sweep kernel, the LayerNorm
    backward and the split-K weight-gradient reduction at 233 k rows -- is held to that test's gradient criterion: inside
    the oracle's gradient INTERVAL over its ambiguous ReLU gates (|pre| < 3e-5; thousands at 90 M ReLU inputs), within 1e-4
    of the gradient's max-norm.  The interval is full_batch_cases.first_layer_gate_interval: the same enumeration, each
    gate's contribution taken on the rows it reaches instead of by a full backward pass (tests/test_full_batch.py holds the
    two forms together on a small graph)."""
    from stochastic_gcn_amd import synthetic
    from stochastic_gcn_amd.full_batch import StaticBatch, StaticMatrix
    n, train_adj, full_adj, _, _, _, labels, tr, va, _ = synthetic.reddit_like(with_features=False)
    feats = np.random.RandomState(0).standard_normal((n, 602)).astype(np.float32)
    fl = mnp.make_flags(normalization='graphsage', weight_decay=0.0, dropout=0.2, layer_norm=True, hidden1=128,
                        num_fc_layers=2, cv=False, cvd=False, preprocess=True)
    import model_cases as mc
    case = dict(flags=fl, ph=mc.placeholders(1, 41), L=1, n=n, classes=41, multitask=False, feats=feats, labels=labels)
    for what, adj, ids, training in (("train step", train_adj, np.sort(tr), True), ("evaluation", full_adj, np.sort(va), False)):
        nbr = adj.dot(feats).astype(np.float32)                       # the PP product, SciPy (gcn/utils.py:321-322)
        om = fc.oracle_model(case, nbr, is_training=training, seed=1)
        dm = fc.device_model(case, nbr, adj, {k: v.copy() for k, v in om.params.items()}, is_training=training)
        sb = StaticBatch(StaticMatrix(adj, DEV, 'cs', 30, 128), labels, ids, 1, DEV)
        drop = 0.2 if training else 0.0
        sb.dropout = drop
        step_id, seed = dm.dropout_step, dm.dropout_seed
        outs = dm.run_one_step(None, sb)
        d_loss = outs[1] if training else outs[0]
        rows = _sample_rows(adj, ids, n)
        assert {int(ids[0]), int(ids[-1])} <= set(rows.tolist())
        pick = torch.from_numpy(rows).to(DEV)
        d_acts = [a[pick].cpu().numpy() for a in (_materialized(x) for x in dm.activations[1:])]
        d_gw = dm.get_grads()['dense0/weights'] if training else None
        del dm, sb
        torch.cuda.empty_cache()
        masks = mnp.HashMasks(seed, step_id, 1.0 - drop) if training else (lambda *a: None)
        feed = fc.exact_feed(case, adj, drop)
        logits, o_acts = om.forward(feed, case['ph'], drop, masks)
        o_loss = float(om.loss_and_grad(logits[ids], labels[ids])[0])
        worst = 0.0
        assert len(d_acts) == len(o_acts)
        for li, (da, oa) in enumerate(zip(d_acts, o_acts)):
            e = onp.rel_err(da, oa[rows])
            worst = max(worst, e)
            print("full size %s: layer %d rel_err %.3e on %d sampled rows" % (what, li, e, len(rows)))
            assert e <= TOL, (what, li, e)
        print("full size %s: loss %.7f (oracle %.7f), worst activation rel_err %.2e" % (what, d_loss, o_loss, worst))
        assert abs(d_loss - o_loss) <= 1e-4 * max(1.0, abs(o_loss))
        if training:
            from test_model_gpu import BAND, GRAD_TOL
            dout = np.zeros_like(logits)
            dout[ids] = om.loss_and_grad(logits[ids], labels[ids])[3]
            lo, hi, g, n_amb = fc.first_layer_gate_interval(om, dout, BAND)
            gmax = np.abs(g).max()
            excess = max(float((lo - d_gw).max()), float((d_gw - hi).max()), 0.0) / gmax
            print("full size %s: dense0/weights gradient rel_err %.3e against the oracle's own gates; %d ambiguous gates, "
                  "interval width %.3e of the max-norm; outside the interval by %.3e"
                  % (what, onp.rel_err(d_gw, g), n_amb, float((hi - lo).max() / gmax), excess))
            tol = GRAD_TOL * gmax
            assert np.all(d_gw >= lo - tol) and np.all(d_gw <= hi + tol), excess
            del dout, lo, hi
        del om, logits, o_acts, feed


def _materialized(x):
    return x.materialize() if hasattr(x, 'materialize') else x
