"""--polyak_decay on the device, above the kernel (tests/test_adam_ema_gpu.py holds sgcn_adam_ema_f32 itself).

The parked forms: in a compiled step the optimizer's launch also runs the grouped weight-gradient reductions (split-K tiles,
LayerNorm parameter partials), each of which applies the update to the element it has just reduced, and walks the rest of the
buffer -- every parameter element must get the average's update exactly once.  Three steps of the smallest CVD+PP case with
LayerNorm, four ways (default program, --nogroup_dw, --nolean_sync, eager layers): everything bit-identical, and the
average equal to the NumPy restatement (tests/ema_ref.py) folded over the recorded weights.

The wiring: models that only evaluate read the average, training and its exact twin the raw weights; an evaluation's logits
equal the NumPy oracle's on the averaged weights read back (the project's 1e-4) and are far from the oracle's on the raw
ones (the gap was sized with the oracle alone, before any device run: 0.77 of max|logit| after three steps at decay 0.9 on
reddit_cvd_pp with the weights of seed 3, 1.2 on reddit3k_pp full-batch); checkpoints; train.main end to end."""
import contextlib
import io

import numpy as np
import pytest
import torch

import ema_ref
import full_batch_cases as fc
import model_cases as mc
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TOL = 1e-4
DECAY = 0.9
CASE = 'reddit_cvd_pp'        # the smallest CVD+PP case with LayerNorm: split-K weight gradients and LayerNorm partials
STEPS = 3


def _set_flags(case, **extra):
    from stochastic_gcn_amd.flags import FLAGS
    FLAGS.reset()
    FLAGS.update(**{k: v for k, v in case['flags'].items() if hasattr(FLAGS, k)})
    FLAGS.update(batch_size=case['cfg']['batch'], **extra)


def _train_model(case, params):
    from stochastic_gcn_amd.vrgcn import VRGCN
    fl = case['flags']
    m = VRGCN(fl['num_layers'], fl['preprocess'], case['ph'], case['feats'], case['nbr'], case['adj'], fl['cvd'],
              is_training=True, device=DEV)
    m.set_params({k: v.copy() for k, v in params.items()})
    m.reset_average()                      # (the average starts from the weights the first step starts from)
    return m


def _steps(case, params, **flags):
    """STEPS packed training steps; after each one the weights, moments, average, history and loss statistics"""
    from stochastic_gcn_amd.flags import FLAGS
    _set_flags(case, **flags)
    m = _train_model(case, params)
    sch = mc.make_scheduler(case, 1)
    rec = []
    for _ in range(STEPS):
        pb = sch.minibatch_packed(case['cfg']['batch'], FLAGS.plan_t, None)
        pb.dropout = case['flags']['dropout']
        out = m.run_one_step(None, pb, sync=False)
        torch.cuda.synchronize()
        rec.append(dict(theta=m.theta.clone(), m=m.adam_m.clone(), v=m.adam_v.clone(),
                        avg=None if m.average is None else m.average.clone(),
                        hist=[h.clone() for hs in m.history for h in hs], loss=out[1].clone(), acc=out[2].clone()))
    return m, rec


def _same(a, b, what, keys=('theta', 'm', 'v', 'avg', 'loss', 'acc')):
    for step, (x, y) in enumerate(zip(a, b)):
        for k in keys:
            assert torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)), "%s: step %d: %s differs" % (what, step, k)
        assert len(x['hist']) == len(y['hist']) > 0 and all(torch.equal(p, q) for p, q in zip(x['hist'], y['hist'])), \
            "%s: step %d: the history differs" % (what, step)


def _codes(prog):
    return [o for o, _ in prog.ops_fb + prog.ops_opt + prog.ops_hist]


@pytest.fixture(scope="module")
def parked():
    """the four runs with the flag and the default run without it (computed once, left unchanged)"""
    case = mc.build_case(CASE)
    params = mc.make_oracle_model(case, seed=3).params
    runs = {}
    for name, flags in (('default', {}), ('nogroup_dw', dict(group_dw=False)), ('nolean_sync', dict(lean_sync=False)),
                        ('eager', dict(native_step=False))):
        runs[name] = _steps(case, params, polyak_decay=DECAY, **flags)
    runs['off'] = _steps(case, params)
    from stochastic_gcn_amd.flags import FLAGS
    FLAGS.reset()
    return case, params, runs


def test_the_four_step_forms_agree_bit_for_bit(parked):
    case, params, runs = parked
    for name in ('default', 'nogroup_dw', 'nolean_sync'):
        progs = list(getattr(runs[name][0], '_programs', {}).values())
        assert progs and all(p is not None for p in progs), getattr(runs[name][0], '_program_note', 'no program')
    assert not getattr(runs['eager'][0], '_programs', {})
    for name in ('nogroup_dw', 'nolean_sync', 'eager'):
        _same(runs['default'][1], runs[name][1], name)
    assert float(runs['default'][1][-1]['hist'][0].abs().sum()) > 0


@pytest.mark.parametrize("name", ['default', 'nogroup_dw', 'nolean_sync', 'eager'])
def test_every_element_is_averaged_exactly_once(parked, name):
    """A reduction and a gap walker both touching an element would average it twice, neither would leave it behind: either
    shows as a difference from the restatement folded over the recorded weights."""
    case, params, runs = parked
    m, rec = runs[name]
    theta0 = np.zeros(m.theta.numel(), np.float32)
    for (pname, shape, _, off, n) in m._layout:
        theta0[off:off + n] = params[pname].reshape(-1)
    want = ema_ref.fold(theta0, [r['theta'].cpu().numpy() for r in rec], DECAY)
    moved = 0
    for step, (r, w) in enumerate(zip(rec, want)):
        got = r['avg'].cpu().numpy()
        bad = got.view(np.int32) != w.view(np.int32)
        assert not bad.any(), "%s step %d: %d of %d elements of the average differ (first at %s)" % (
            name, step, int(bad.sum()), bad.size, np.nonzero(bad)[0][:8])
        moved = int((got != theta0).sum())
    pad = m.theta.numel() - sum(n for *_, n in m._layout)
    assert moved >= 0.9 * (m.theta.numel() - pad)          # (the weights did move, and the average with them)
    assert not np.array_equal(rec[-1]['avg'].cpu().numpy(), rec[-1]['theta'].cpu().numpy())


def test_the_program_gains_no_op(parked):
    from stochastic_gcn_amd.step_program import OP
    case, params, runs = parked
    on, off = (next(iter(runs[k][0]._programs.values())) for k in ('default', 'off'))
    c_on, c_off = _codes(on), _codes(off)
    assert c_off.count(OP['ADAM']) == 1 and OP['ADAM_EMA'] not in c_off
    assert c_on == [OP['ADAM_EMA'] if c == OP['ADAM'] else c for c in c_off] and on.n_all == off.n_all
    a_on = next(a for o, a in on.ops_opt if o == OP['ADAM_EMA'])
    a_off = next(a for o, a in off.ops_opt if o == OP['ADAM'])
    assert len(a_on) == len(a_off) + 3 and a_on[4][2] == runs['default'][0].average.data_ptr()
    d, om = ema_ref.factors(DECAY)
    assert [a_on[-2][2], a_on[-1][2]] == [int(d.view(np.uint32)), int(om.view(np.uint32))]
    # the neighbours of the optimizer are what they were: the grouped reductions in front, the history scatters behind
    assert on.ops_fb[-1][0] == OP['DW_FLUSH'] and all(o == OP['SCATTER_ROWS'] for o, _ in on.ops_hist) and on.ops_hist


def test_without_the_flag_nothing_changes(parked):
    """No buffer, the op ADAM, and the weights, moments, history and statistics of the run with the flag (whose theta / m / v
    are sgcn_adam_f32's bit for bit: tests/test_adam_ema_gpu.py) -- the average rides along and feeds nothing back."""
    case, params, runs = parked
    m, rec = runs['off']
    assert m.average is None and m._store.average is None and all(r['avg'] is None for r in rec)
    _same(runs['default'][1], rec, 'flag off', keys=('theta', 'm', 'v', 'loss', 'acc'))


def _template(case, cls_args=()):
    from stochastic_gcn_amd.models import make_template
    from stochastic_gcn_amd.vrgcn import VRGCN
    fl, ph = case['flags'], case['ph']

    def model_func(is_training, _store=None):
        return VRGCN(fl['num_layers'], True, ph, case['feats'], case['nbr'], case['adj'], True, is_training=is_training,
                     device=DEV, _store=_store)
    create = make_template('model', model_func)
    return create(True), create(False)


def _train_packed(case, train_m, steps):
    from stochastic_gcn_amd.flags import FLAGS
    sch = mc.make_scheduler(case, 1)
    for _ in range(steps):
        pb = sch.minibatch_packed(case['cfg']['batch'], FLAGS.plan_t, None)
        pb.dropout = case['flags']['dropout']
        train_m.run_one_step(None, pb, sync=False)
    torch.cuda.synchronize()


def test_evaluation_models_read_the_average_and_training_the_raw_weights():
    from stochastic_gcn_amd.exact_history import ExactTwin
    from stochastic_gcn_amd.flags import FLAGS
    case = mc.build_case(CASE)
    fl, c, ph = case['flags'], case['cfg'], case['ph']
    _set_flags(case, polyak_decay=DECAY)
    try:
        train_m, test_m = _template(case)
        st = train_m._store
        assert st.average is not None and st.average.data_ptr() != st.theta.data_ptr() and st is test_m._store
        assert test_m.theta.data_ptr() == st.average.data_ptr() != train_m.theta.data_ptr() == st.theta.data_ptr()
        assert train_m.average is st.average and test_m.average is None          # (only the training model's optimizer moves it)
        assert torch.equal(st.average, st.theta)
        assert ExactTwin(test_m).theta.data_ptr() == st.average.data_ptr()
        assert ExactTwin(train_m).theta.data_ptr() == st.theta.data_ptr()
        params = mc.make_oracle_model(case, seed=3).params
        train_m.set_params({k: v.copy() for k, v in params.items()})
        train_m.reset_average()
        _train_packed(case, train_m, STEPS)
        assert next(iter(train_m._programs.values())) is not None
        raw, avg = train_m.get_params(), test_m.get_params()
        assert all(np.array_equal(avg[k].reshape(-1), st.average[off:off + n].cpu().numpy())
                   for k, _, _, off, n in test_m._layout)
        # one evaluation batch, layer by layer, against the oracle on the averaged and on the raw weights
        feed = mc.make_scheduler(case, 1).minibatch(c['batch'])
        before = (st.theta.clone(), st.average.clone())
        loss, acc, pred = test_m.run_one_step(None, feed)
        logits = test_m.outputs.cpu().numpy()
        assert torch.equal(before[0], st.theta) and torch.equal(before[1], st.average)       # evaluation writes neither
        o = {}
        for which, p in (('avg', avg), ('raw', raw)):
            om = mc.make_oracle_model(case, params={k: v.copy() for k, v in p.items()}, is_training=False)
            o_loss, _, o_pred, o_acts, _ = om.run_one_step(feed, ph, 0.0, lambda *a: None)
            o[which] = (onp.rel_err(logits, o_acts[-1]), float(o_loss), onp.rel_err(pred, o_pred))
        print("logits vs the oracle: on the averaged weights %.3e, on the raw weights %.3e; loss %.7f (oracle %.7f / %.7f)"
              % (o['avg'][0], o['raw'][0], loss, o['avg'][1], o['raw'][1]))
        assert o['avg'][0] <= TOL and o['avg'][2] <= TOL and abs(loss - o['avg'][1]) <= TOL
        assert o['raw'][0] > 10 * TOL
        # the compiled evaluation step reads the same buffer: its program baked the average's address in
        test_m2 = _template(case)[1]
        test_m2.theta.copy_(st.average)
        pb = mc.make_scheduler(case, 1).minibatch_packed(c['batch'], FLAGS.plan_t, None)
        l2, a2, p2 = test_m2.run_one_step(None, pb, sync=True)
        assert next(iter(test_m2._programs.values())) is not None
        assert onp.rel_err(p2, pred) <= TOL and abs(l2 - loss) <= TOL
    finally:
        FLAGS.reset()


def test_without_the_flag_the_models_share_one_buffer():
    from stochastic_gcn_amd.flags import FLAGS
    case = mc.build_case(CASE)
    _set_flags(case)
    try:
        train_m, test_m = _template(case)
        assert test_m.theta is train_m.theta and train_m._store.average is None and train_m.average is None
        train_m.reset_average("never printed")                                       # a no-op without the flag
    finally:
        FLAGS.reset()


def _trainer(case, **flags):
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.train import Trainer
    FLAGS.reset()
    FLAGS.update(dataset='s-reddit', seed=1, prefetch=0, test_preprocess=case['flags']['preprocess'],
                 **{k: v for k, v in case['flags'].items() if hasattr(FLAGS, k)})
    FLAGS.update(**flags)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        tr = Trainer(data=case['data'], verbose=True)
    return tr, buf.getvalue()


def test_full_batch_route_trains_raw_and_scores_the_average():
    """--full_batch --test_full_batch: eager Adam (ops.adam_ema_step) and one exact forward of the test model per evaluation"""
    from stochastic_gcn_amd.flags import FLAGS
    case = fc.build('reddit3k_pp')
    try:
        tr, out = _trainer(case, full_batch=True, test_full_batch=True, full_batch_kernel='cs', polyak_decay=DECAY)
        assert "[sgcn] --polyak_decay 0.9" in out and "moving average" in out
        st = tr.train_model._store
        assert tr.test_model.theta.data_ptr() == st.average.data_ptr() != tr.train_model.theta.data_ptr()
        theta0 = st.theta.cpu().numpy()
        assert torch.equal(st.average, st.theta)
        thetas = []
        for _ in range(STEPS):
            tr.train_epoch()
            thetas.append(st.theta.cpu().numpy())
        assert tr.train_model.adam_t == STEPS and not getattr(tr.train_model, '_programs', None)
        assert np.array_equal(st.average.cpu().numpy().view(np.int32), ema_ref.fold(theta0, thetas, DECAY)[-1].view(np.int32))
        loss, acc, _, _, _ = tr.evaluate(tr.val_d)
        logits = tr.test_model.outputs.cpu().numpy()
        feed, rows = fc.exact_feed(case, case['full_adj'], 0.0), np.sort(case['val'])
        o = {}
        for which, p in (('avg', tr.test_model.get_params()), ('raw', tr.train_model.get_params())):
            om = fc.oracle_model(case, case['nbr_test'], params=p, is_training=False)
            o_logits, _ = om.forward(feed, case['ph'], 0.0, lambda *a: None)
            o[which] = (onp.rel_err(logits, o_logits), float(om.loss_and_grad(o_logits[rows], case['labels'][rows])[0]))
        print("full-batch logits vs the oracle: averaged weights %.3e, raw weights %.3e; loss %.7f (oracle %.7f / %.7f)"
              % (o['avg'][0], o['raw'][0], loss, o['avg'][1], o['raw'][1]))
        assert o['avg'][0] <= TOL and abs(loss - o['avg'][1]) <= TOL * abs(o['avg'][1])
        assert o['raw'][0] > 10 * TOL
        # a further step moves the average: the cached logits of the evaluation are not reused
        tr.train_epoch()
        assert tr.evaluate(tr.val_d)[0] != loss
    finally:
        FLAGS.reset()


def test_checkpoints_carry_the_average(tmp_path, capsys):
    from stochastic_gcn_amd.flags import FLAGS
    case = mc.build_case(CASE)
    params = mc.make_oracle_model(case, seed=3).params
    try:
        _set_flags(case, polyak_decay=DECAY)
        a = _train_model(case, params)
        _train_packed(case, a, 2)
        assert not torch.equal(a.average, a.theta)
        with_avg = a.save(path=str(tmp_path / "avg.ckpt.npz"))
        z = np.load(with_avg)
        names = [n for n, *_ in a._layout]
        assert all("var/" + n in z.files and "avg/" + n in z.files for n in names)
        b = _train_model(case, mc.make_oracle_model(case, seed=4).params)
        capsys.readouterr()
        b.load(path=with_avg)
        assert "no averaged weights" not in capsys.readouterr().out
        assert torch.equal(b.theta, a.theta) and torch.equal(b.average, a.average)
        # without the flag: the weights only, the file's avg/* keys ignored; and the file it writes is as ever
        _set_flags(case)
        c = _train_model(case, mc.make_oracle_model(case, seed=4).params)
        c.load(path=with_avg)
        assert c.average is None and torch.equal(c.theta, a.theta)
        plain = c.save(path=str(tmp_path / "plain.ckpt.npz"))
        zp = np.load(plain)
        assert not [k for k in zp.files if k.startswith("avg/")] and sorted(zp.files) == sorted(k for k in z.files if not k.startswith("avg/"))
        assert all(np.array_equal(zp[k], z[k]) for k in zp.files if k.startswith("var/"))     # (the history is each model's own)
        # a file without averages, with the flag: the average starts from the loaded weights, and says so
        _set_flags(case, polyak_decay=DECAY)
        d = _train_model(case, mc.make_oracle_model(case, seed=4).params)
        capsys.readouterr()
        d.load(path=plain)
        said = capsys.readouterr().out
        assert torch.equal(d.theta, a.theta) and torch.equal(d.average, d.theta)
        assert len([l for l in said.splitlines() if "no averaged weights" in l]) == 1
    finally:
        FLAGS.reset()


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
    try:
        with contextlib.redirect_stdout(buf):
            train.main(['--dataset', 's-cora', '--polyak_decay', '0.9', '--epochs', '0'])
        out = buf.getvalue()
    finally:
        FLAGS.reset()
    tr = made[0]
    st = tr.train_model._store
    assert tr.test_model.theta.data_ptr() == st.average.data_ptr() != st.theta.data_ptr()
    assert tr.train_model.adam_t > 0 and not torch.equal(st.average, st.theta)
    assert len([l for l in out.splitlines() if l.startswith("[sgcn] --polyak_decay 0.9")]) == 1
    ep = [l for l in out.splitlines() if l.startswith("Epoch:")]
    assert len(ep) == 2                   # the reference's exit is `epoch > FLAGS.epochs`: epochs + 2
    for line in ep:
        tok = line.split()
        assert tok[0] == "Epoch:" and tok[2] == "train_loss=" and tok[4] == "train_acc=" and tok[6] == "val_loss="
        assert tok[8] == "val_acc=" and "time=" in tok and "ttime=" in tok and "(sch" in tok and "data" in tok
        assert np.isfinite(float(tok[7]))
    assert "Test set results:" in out and "Optimization Finished!" in out
    z = np.load(str(tmp_path / "tmp" / (tr.train_model.name + ".ckpt.npz")))
    assert any(k.startswith("avg/") for k in z.files)
