"""The --gradvar bias / variance study (Trainer.GradientVariance, gcn/train.py:241-276) on the GPU: its returned values
against a NumPy fp64 restatement of the reference's formulas over the very draws it saw, the command line end to end
(the reference's seven lines in its order and wording, then the test line), and what the study is for -- the
control variate's sampled predictions scatter far less than plain neighbour sampling's, and the every-neighbour
estimator does not scatter at all without dropout (scripts/run-experiments.py:24-32, VarNSPP / VarCV)."""
import contextlib
import io
import math
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _data():
    from stochastic_gcn_amd import synthetic
    return synthetic.reddit_like(n=6000, m=60000, f=32, classes=6, splits=(3600, 800, 1600), seed=5,
                                 with_features=True, planted=True)


def _train(flags, epochs):
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.train import Trainer
    FLAGS.reset()
    base = dict(dataset='s-reddit', normalization='graphsage', weight_decay=0.0, dropout=0.1, layer_norm=True,
                hidden1=64, num_fc_layers=1, batch_size=256, test_batch_size=512, learning_rate=0.01, seed=1,
                prefetch=2, gradvar=True, test_degree=10000)
    base.update(flags)
    FLAGS.update(**base)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        tr = Trainer(data=_data(), verbose=False)
        for _ in range(epochs):
            tr.train_epoch()
    return tr


def _restate(rec):
    """gcn/train.py:256-275 over host copies of the draws: np.mean / np.std of the stacked lists, as gcn/stats.py."""
    fp, fg = (np.stack([r[i] for r in rec['full']]) for i in (0, 1))
    pp, pg = (np.stack([r[i] for r in rec['part']]) for i in (0, 1))
    full_preds_m = np.mean(np.abs(fp.mean(axis=0)))
    full_grads_m = np.mean(np.abs(fg.mean(axis=0)))
    return full_preds_m, full_grads_m, dict(
        full_pred_stdev=np.mean(fp.std(axis=0)) / full_preds_m,
        full_grad_stdev=np.mean(fg.std(axis=0)) / full_grads_m,
        part_pred_bias=np.mean(np.abs(pp.mean(axis=0) - fp.mean(axis=0))) / full_preds_m,
        part_pred_stdev=np.mean(pp.std(axis=0)) / full_preds_m,
        part_grad_bias=np.mean(np.abs(fg.mean(axis=0) - pg.mean(axis=0))) / full_grads_m,
        part_grad_stdev=np.mean(pg.std(axis=0)) / full_grads_m,
        full_grads_m=full_grads_m,
        part_grad_std_mean=np.mean(pg.std(axis=0)),
        part_grad_mean_abs=np.mean(np.abs(pg.mean(axis=0))))


def test_study_matches_its_host_restatement():
    import torch
    from stochastic_gcn_amd.flags import FLAGS
    tr = _train(dict(cv=True, degree=1), 3)
    FLAGS.update(gradvar_draws=32)
    rec = {'full': [], 'part': []}
    first = tr.train_model.named_vars()[0][1]

    def observer(kind, pred, grad):
        assert isinstance(pred, torch.Tensor) and pred.is_cuda and grad.is_cuda
        assert grad.shape == first.shape
        rec[kind].append((pred.cpu().numpy().astype(np.float64), grad.cpu().numpy().astype(np.float64)))

    res = tr.GradientVariance(observer=observer)
    assert len(rec['full']) == 32 and len(rec['part']) == 32
    full_preds_m, full_grads_m, want = _restate(rec)
    assert set(res) == set(want) and len(res) == 9
    print({k: (res[k], float(want[k])) for k in want})
    for k, w in want.items():
        # every value to 1e-9 of its normaliser: the normalised ones absolutely, the raw gradient means of full_grads_m
        unit = full_grads_m if k in ('full_grads_m', 'part_grad_std_mean', 'part_grad_mean_abs') else 1.0
        assert math.isfinite(res[k]) and abs(res[k] - w) <= 1e-9 * unit, (k, res[k], w)
    assert res['full_pred_stdev'] > 0 and res['part_pred_stdev'] > res['full_pred_stdev']    # dropout 0.1: both scatter
    # the observer's copies are the draws themselves: get_pred_and_grad (host form) of a fresh draw has the same shapes
    feed = tr.eval_sch.batch(tr.train_d[:FLAGS.batch_size])
    feed[tr.placeholders['dropout']] = FLAGS.dropout
    pred, grad = tr.test_model.get_pred_and_grad(tr.sess, feed)
    assert pred.shape == rec['full'][0][0].shape and grad[0].shape == rec['full'][0][1].shape


LINES = ('Full pred stdev = ', 'Full grad stdev = ', 'Part pred bias = ', 'Part pred stdev = ', 'Part grad bias = ',
         'Part grad stdev = ')


def test_command_line_prints_the_reference_lines(tmp_path, monkeypatch, capsys):
    from stochastic_gcn_amd import train
    monkeypatch.chdir(tmp_path)
    common = ['--dataset', 's-cora', '--epochs', '1', '--early_stopping', '100', '--batch_size', '64',
              '--test_batch_size', '256', '--hidden1', '16', '--seed', '3']
    train.main(common + ['--degree', '2'])
    assert (tmp_path / 'tmp' / 'model.ckpt.npz').exists()
    capsys.readouterr()
    train.main(common + ['--load', '--gradvar', '--test_degree=10000', '--degree=1', '--gradvar_draws', '16'])
    out = capsys.readouterr().out.splitlines()
    at = []
    for label in LINES:
        idx = [i for i, l in enumerate(out) if l.startswith(label)]
        assert len(idx) == 1, (label, out)
        at.append(idx[0])
        assert math.isfinite(float(out[idx[0]][len(label):]))
    assert at == sorted(at) and at == list(range(at[0], at[0] + 6)), out     # the reference's order, back to back
    last = out[at[-1] + 1].split()
    assert len(last) == 3 and all(math.isfinite(float(v)) for v in last), out[at[-1] + 1]
    test_lines = [i for i, l in enumerate(out) if l.startswith('Test set results:')]
    assert test_lines and test_lines[0] > at[-1] + 1
    assert re.match(r"Test set results: cost= \d+\.\d{5} accuracy= \d+\.\d{5} mi F1=", out[test_lines[0]])
    assert not any('not part of this package' in l for l in out)


def test_control_variate_scatters_less_than_neighbour_sampling(tmp_path, monkeypatch):
    """The recipes of scripts/run-experiments.py:24-32 on one checkpoint: VarTrainCV (--dropout 0 --cv --degree=1)
    trains and saves; VarNSPP (--load --gradvar --dropout 0 --degree=1) and VarCV (the same + --cv) restore it and
    run the study.  On the same weights the control variate's sampled predictions scatter less than half as much
    as plain neighbour sampling's, its gradients less; the every-neighbour estimator does not scatter."""
    from stochastic_gcn_amd.flags import FLAGS
    monkeypatch.chdir(tmp_path)
    tr = _train(dict(dropout=0.0, degree=1, cv=True, gradvar=False), 20)
    tr.train_model.save()
    res = {}
    for name, flags in (("ns", dict(cv=False)), ("cv", dict(cv=True))):
        tr = _train(dict(dropout=0.0, degree=1, load=True, **flags), 0)
        tr.SGDTrain()                                   # --load: the weights, and the histories under --gradvar
        FLAGS.update(gradvar_draws=100)
        res[name] = tr.GradientVariance()
    print({k: {n: v for n, v in r.items() if 'stdev' in n or 'bias' in n} for k, r in res.items()})
    for r in res.values():
        assert r['full_pred_stdev'] <= 1e-5 and all(math.isfinite(v) for v in r.values())
    assert abs(res['cv']['full_grads_m'] - res['ns']['full_grads_m']) <= 1e-6 * res['ns']['full_grads_m']   # one model
    assert res['cv']['part_pred_stdev'] < 0.5 * res['ns']['part_pred_stdev']
    assert res['cv']['part_grad_stdev'] < res['ns']['part_grad_stdev']
