"""The exact control-variate history on the GPU (exact_history.py; --history_init / --history_refresh / --history_error).

1. the exact pass against the NumPy oracle (a plain model on the hand-built exact feed), and what an assign leaves in an
   fp32 / a bfloat16 history;
2. the fresh-history identity (SURVEY 8c ii): with H = the exact activations, A (mu - H[ifield]) = 0 and ONE sampled
   control-variate forward gives the exact logits on the batch rows -- eager and as a step program; with the zero history
   it is off by O(1).  The oracle alone gives 1.0e-7 .. 1.6e-7 and 0.57 .. 3.0 on these cases; the gate is the project's 1e-4;
3. the reported staleness: 1.0 under zeros, 0.0 after an fp32 init, <= 2^-8 after a bfloat16 one, > 0 after a training step,
   0.0 again after a refresh;
4. the defaults change nothing, and neither does constructing a twin or measuring with it;
5. train.main end to end.
"""
import contextlib
import io
import math
import re

import numpy as np
import pytest
import torch

import bf16_ref
import model_cases as mc
from oracle import model_np as mnp, oracle_np as onp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-4
NAMES = ['reddit_cvd_pp', 'reddit_cv_pp', 'cvd_pp_L3', 'cv_nopp_L2', 'pubmed_cvd_pp', 'reddit_cvd_pp_wide']
KERNELS = ['rows', 'cs']


@pytest.fixture(autouse=True)
def _flags():
    from stochastic_gcn_amd.flags import FLAGS
    yield
    FLAGS.reset()


# ---- the reference: computed once per case, shared, never written to -------------------------------------------------------
_REF = {}


def _exact_feed(case):
    """full_batch_cases.exact_feed for a model_cases case: every field all N vertices in order, the whole matrix as every
    layer's adjacency, unit scales."""
    ph, L, n = case['ph'], case['L_sched'], case['cfg']['n']
    coo = case['adj'].tocsr().tocoo()
    assert np.all(np.diff(coo.row) >= 0)
    triple = (np.stack([coo.row, coo.col], axis=1).astype(np.int32), coo.data.astype(np.float32), case['adj'].shape)
    feed = {ph['labels']: case['labels'], ph['dropout']: 0.0}
    for l in range(L + 1):
        feed[ph['fields'][l]] = np.arange(n, dtype=np.int32)
    for l in range(L):
        feed[ph['adj'][l]] = triple
        feed[ph['scales'][l]] = np.ones(n, np.float32)
    return feed


def _ref(name):
    """(case, params, the oracle's aggregator inputs, its exact logits) -- weights seed 3, dropout 0."""
    if name not in _REF:
        case = mc.build_case(name)
        fl, c = case['flags'], case['cfg']
        params = mc.make_oracle_model(case, seed=3).params
        plain = mnp.Model(fl, fl['num_layers'], fl['preprocess'], False, False, case['feats'], case['nbr'], c['n'],
                          c['classes'], {k: v.copy() for k, v in params.items()}, is_training=False)
        logits, acts = plain.forward(_exact_feed(case), case['ph'], 0.0, None)
        inputs = []
        for i, s in enumerate(plain.specs):
            if s[0] == 'agg':
                x = acts[i - 1] if i else plain.features
                assert not isinstance(x, tuple)
                inputs.append(np.asarray(x, dtype=np.float32))
        assert len(inputs) == case['L_sched']
        for a in inputs + [logits]:
            a.setflags(write=False)
        _REF[name] = (case, params, inputs, logits)
    return _REF[name]


def _owner(case, params, is_training=True, **extra):
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.vrgcn import VRGCN
    FLAGS.reset()
    FLAGS.update(**{k: v for k, v in case['flags'].items() if hasattr(FLAGS, k)})
    FLAGS.update(**extra)
    fl = case['flags']
    with contextlib.redirect_stdout(io.StringIO()):
        m = VRGCN(fl['num_layers'], fl['preprocess'], case['ph'], case['feats'], case['nbr'], case['adj'], fl['cvd'],
                  is_training=is_training, device=DEV)
    m.set_params({k: v.copy() for k, v in params.items()})
    return m


def _exact(owner, case, kernel):
    from stochastic_gcn_amd.exact_history import ExactHistory, make_matrix
    return ExactHistory(owner, make_matrix(case['adj'], DEV, owner, 1, kernel=kernel))


def _hist(owner):
    from stochastic_gcn_amd import ops
    return [ops.history_widen(hs[0]).cpu().numpy() for hs in owner.history]


# ---- 1. the exact pass --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", NAMES)
def test_exact_pass_matches_the_oracle_and_fills_the_history(name, kernel):
    case, params, o_inputs, o_logits = _ref(name)
    owner = _owner(case, params)
    ex = _exact(owner, case, kernel)
    assert ex.twin.theta is owner.theta and ex.twin.features_dev is owner.features_dev      # live weights, ONE feature table
    assert not ex.twin._history and len(ex.twin.agg_index) == owner.L
    acts = ex.forward(full=True)
    assert len(acts) == len(o_inputs) == len(owner.history)
    for l, (a, o) in enumerate(zip(acts, o_inputs)):
        e = onp.rel_err(a.cpu().numpy(), o)
        print("%s %s: layer %d input %r rel err %.2e" % (name, kernel, l, tuple(a.shape), e))
        assert tuple(a.shape) == o.shape == tuple(owner.history[l][0].shape) and e <= TOL, (name, l, e)
    e = onp.rel_err(ex.twin.outputs.cpu().numpy(), o_logits)
    print("%s %s: exact logits rel err %.2e" % (name, kernel, e))
    assert e <= TOL
    # a pass that stops at the last aggregator's input gives the same inputs, bit for bit
    kept = [a.clone() for a in acts]
    again = ex.forward()
    assert len(ex.twin.activations) == ex.twin.agg_index[-1] + 1
    assert all(torch.equal(a, b) for a, b in zip(again, kept))
    # fp32 history: the device activations, bit for bit, in the SAME tables
    ptrs = [hs[0].data_ptr() for hs in owner.history]
    assert all(float(hs[0].abs().max()) == 0.0 for hs in owner.history)
    ex.assign(again)
    assert [hs[0].data_ptr() for hs in owner.history] == ptrs
    assert all(torch.equal(hs[0], a) for hs, a in zip(owner.history, kept))
    # bfloat16 history: round to nearest even of them, bit for bit
    owner16 = _owner(case, params, history_dtype='bf16')
    assert all(hs[0].dtype == torch.bfloat16 for hs in owner16.history)
    ex16 = _exact(owner16, case, kernel)
    acts16 = ex16.forward()
    assert all(torch.equal(a, b) for a, b in zip(acts16, kept))
    ex16.assign(acts16)
    for h, a in zip(_hist(owner16), kept):
        want = bf16_ref.round_trip(a.cpu().numpy())
        assert h.tobytes() == want.tobytes()


# ---- 2. the fresh-history identity ------------------------------------------------------------------------------------
def _sampled_logits(owner, case, native_step):
    """One sampled control-variate step at dropout 0 on the first batch of the product's scheduler (seed 1): (logits on the
    batch rows, the batch's vertex ids, the packed batch, the path taken)."""
    from stochastic_gcn_amd.flags import FLAGS
    FLAGS.update(native_step=native_step)
    sch = mc.make_scheduler(case, 1)
    pb = sch.minibatch_packed(case['cfg']['batch'], FLAGS.plan_t, None)
    pb.dropout = 0.0
    rows = np.array(pb.field(owner.L), copy=True)
    prog = owner._program(pb, 0.0)
    owner.outputs = None
    owner.run_one_step(None, pb)
    if owner.outputs is None:                  # the step ran as a program: the logits are an activation of its arena
        assert prog is not None
        logits = prog.tensor_of(prog.logits, len(rows)).cpu().numpy()
    else:                                      # layer by layer (no program for this stack, or the batch did not fit it)
        logits = owner.outputs.cpu().numpy()
    assert logits.shape[0] == len(rows)
    return logits, rows, pb, prog


@pytest.mark.parametrize("native_step", [False, True])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", NAMES)
def test_fresh_history_identity(name, kernel, native_step):
    from stochastic_gcn_amd.flags import FLAGS
    case, params, _, o_logits = _ref(name)
    scale = float(np.abs(o_logits).max())
    # the untouched zero history: the same batch is off by O(1)
    stale, rows0, _, _ = _sampled_logits(_owner(case, params), case, native_step)
    off = float(np.abs(stale - o_logits[rows0]).max()) / scale
    # the history filled by one exact pass
    owner = _owner(case, params, native_step=native_step)
    ex = _exact(owner, case, kernel)
    sch = mc.make_scheduler(case, 1)
    probe = sch.minibatch_packed(case['cfg']['batch'], FLAGS.plan_t, None)
    before = owner._program(probe, 0.0)                  # compiled against the zero history's addresses
    ex.assign(ex.forward())
    fresh, rows, pb, prog = _sampled_logits(owner, case, native_step)
    assert prog is before and len(getattr(owner, '_programs', {})) <= 1        # the assign was in place: the cached program
    assert native_step or prog is None
    assert np.array_equal(rows, rows0)
    err = float(np.abs(fresh - o_logits[rows]).max()) / scale
    print("%s %s %s: sampled CV logits vs exact: fresh history %.2e, zero history %.2e of max|exact| = %.3f (%d rows)"
          % (name, kernel, "program" if prog is not None else "eager", err, off, scale, len(rows)))
    assert err <= TOL, (name, err)
    assert off > 0.1, (name, off)


@pytest.mark.parametrize("native_step", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_fresh_bf16_history_teacher_forced(name, native_step):
    """--history_dtype bf16: the device history is read back widened and GIVEN to the oracle's control-variate model, so that
    a bfloat16 rounding tie cannot decide the comparison; the device forward is held to that oracle."""
    from stochastic_gcn_amd.flags import FLAGS
    case, params, _, o_logits = _ref(name)
    owner = _owner(case, params, history_dtype='bf16', native_step=native_step)
    ex = _exact(owner, case, 'rows')
    ex.assign(ex.forward())
    om = mc.make_oracle_model(case, params={k: v.copy() for k, v in params.items()})
    om.history = _hist(owner)
    feed = mc.make_scheduler(case, 1).minibatch(case['cfg']['batch'])
    want, _ = om.forward(feed, case['ph'], 0.0, None)
    got, rows, _, prog = _sampled_logits(owner, case, native_step)
    assert np.array_equal(rows, feed[case['ph']['fields'][owner.L]])
    e = onp.rel_err(got, want)
    print("%s %s: bf16 history, device vs teacher-forced oracle %.2e (vs exact logits %.2e)"
          % (name, "program" if prog is not None else "eager", e, onp.rel_err(got, o_logits[rows])))
    assert e <= TOL


# ---- 3. the staleness ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", NAMES)
def test_reported_staleness(name, kernel):
    from stochastic_gcn_amd.flags import FLAGS
    case, params, _, _ = _ref(name)
    owner = _owner(case, params)
    assert FLAGS.learning_rate > 0
    ex = _exact(owner, case, kernel)
    r = ex.run(measure=True)                                              # zeros, before the first step
    assert [l['rel_err'] for l in r['layers']] == [1.0] * owner.L and not r['refreshed']
    assert all(l['rows_off'] > 0 and l['max_err'] > 0 for l in r['layers'])
    r = ex.run(measure=True, assign=True)                                 # measured first, then assigned
    assert [l['rel_err'] for l in r['layers']] == [1.0] * owner.L and r['refreshed']
    r = ex.run(measure=True)
    assert [(l['rel_err'], l['max_err'], l['rows_off']) for l in r['layers']] == [(0.0, 0.0, 0)] * owner.L
    # one training step moves the weights: the twin reads them live, so every layer behind a weight is stale again
    sch = mc.make_scheduler(case, 1)
    pb = sch.minibatch_packed(case['cfg']['batch'], FLAGS.plan_t, None)
    pb.dropout = case['flags']['dropout']
    owner.run_one_step(None, pb)
    r = ex.run(measure=True)
    for l, e in enumerate(r['layers']):
        print("%s %s: layer %d after one step: rel_err %.3e max_err %.3e rows_off %d" % (name, kernel, l, e['rel_err'],
                                                                                         e['max_err'], e['rows_off']))
        if l == 0 and not owner.preprocess:           # the raw feature table: no weight in front of it
            assert e['rel_err'] == 0.0
        else:
            assert 0.0 < e['rel_err'] < 1.0 and e['rows_off'] > 0
    r = ex.run(measure=True, assign=True)
    r = ex.run(measure=True)
    assert [(l['rel_err'], l['max_err'], l['rows_off']) for l in r['layers']] == [(0.0, 0.0, 0)] * owner.L
    assert ex.passes == 6


@pytest.mark.parametrize("name", NAMES)
def test_staleness_of_a_fresh_bf16_history(name):
    case, params, _, _ = _ref(name)
    owner = _owner(case, params, history_dtype='bf16')
    ex = _exact(owner, case, 'rows')
    assert [l['rel_err'] for l in ex.run(measure=True, assign=True)['layers']] == [1.0] * owner.L
    r = ex.run(measure=True)
    for l, e in enumerate(r['layers']):
        print("%s: layer %d fresh bf16 history rel_err %.3e (2^-8 = %.3e)" % (name, l, e['rel_err'], 2.0 ** -8))
        # round to nearest: 2^-9 relative per element; the norm ratio cannot exceed the worst element's
        assert 0.0 < e['rel_err'] <= 2.0 ** -8


# ---- 4. the defaults change nothing ---------------------------------------------------------------------------------------
def _trainer(case, **flags):
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.train import Trainer
    c = case['cfg']
    rest = np.setdiff1d(np.arange(c['n'], dtype=np.int32), case['train'])
    data = (c['n'], case['adj'], case['adj'], case['feats'], case['nbr'], case['nbr'], case['labels'], case['train'].copy(),       # (the sampler shuffles its ids in place)
            rest[:100].astype(np.int32), rest[100:200].astype(np.int32))
    FLAGS.reset()
    FLAGS.update(**{k: v for k, v in case['flags'].items() if hasattr(FLAGS, k)})
    FLAGS.update(dataset='s-reddit', seed=1, prefetch=0, batch_size=c['batch'], test_batch_size=c['batch'], max_steps=3,
                 test_degree=case['flags']['degree'])
    FLAGS.update(**flags)
    with contextlib.redirect_stdout(io.StringIO()):
        return Trainer(data=data, verbose=False)


def _three_steps(tr):
    tr.train_epoch()
    torch.cuda.synchronize()
    assert tr.last_epoch['steps'] == 3
    return tr.train_model.theta.cpu().numpy().copy(), _hist(tr.train_model)


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and len(a[1]) == len(b[1]) and all(x.tobytes() == y.tobytes()
                                                                               for x, y in zip(a[1], b[1]))


def test_defaults_change_nothing():
    case = mc.build_case('reddit_cvd_pp')
    tr = _trainer(case)                                                   # the flags absent; no twin exists yet
    assert tr.exact_train is None and tr.exact_test is None and tr.history_pass(0) is None
    base = _three_steps(tr)
    assert np.abs(base[1][0]).max() > 0
    tr = _trainer(case, history_init='zeros', history_refresh=0)          # the defaults spelled out
    assert tr.exact_train is None and tr.exact_test is None and tr.history_pass(0) is None
    assert _same(_three_steps(tr), base)
    tr = _trainer(case, history_error=True)                               # a twin and its matrix are built, and measure
    assert tr.exact_train is not None and tr.exact_test is None
    rec = tr.history_pass(0)
    assert [l['rel_err'] for l in rec['layers']] == [1.0] and not rec['refreshed'] and rec['epoch'] == 1
    assert _same(_three_steps(tr), base)
    tr = _trainer(case, history_init='exact', test_cv=True, test_cvd=True)  # ... while an exact init does change the run
    assert tr.exact_train is not None and tr.exact_test is not None
    assert tr.exact_test.matrix is tr.exact_train.matrix                  # (one adjacency object here: one matrix)
    rec = tr.history_pass(0)
    assert rec['refreshed'] and rec['layers'] is None
    assert float(tr.test_model.history[0][0].abs().max()) > 0
    assert torch.equal(tr.test_model.history[0][0], tr.train_model.history[0][0])      # same weights, adjacency, features
    assert not _same(_three_steps(tr), base)


# ---- 5. train.main end to end ---------------------------------------------------------------------------------------------
ARGS = ['--dataset', 's-cora', '--cv', '--cvd', '--epochs', '2']
HIST = ['--history_init', 'exact', '--history_refresh', '1', '--history_error']


def _main(argv):
    from stochastic_gcn_amd import train
    from stochastic_gcn_amd.flags import FLAGS
    FLAGS.reset()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train.main(argv)
    return buf.getvalue().splitlines()


def _check_log(lines, epochs=4):
    ep = [l.split() for l in lines if l.startswith("Epoch:")]
    assert len(ep) == epochs                                  # the reference's exit is `epoch > FLAGS.epochs`: epochs + 2
    for t in ep:                                              # the token positions scripts/analyze-time.py reads
        assert [t[i] for i in (0, 2, 4, 6, 8, 14, 16)] == ["Epoch:", "train_loss=", "train_acc=", "val_loss=", "val_acc=",
                                                           "time=", "ttime="]
        assert all(math.isfinite(float(t[i])) for i in (3, 5, 7, 9, 15, 17))
    hist = [l for l in lines if l.startswith("[sgcn] history:")]
    pat = re.compile(r"\[sgcn\] history: epoch (\d{4}) layer 0 rel_err=(\S+) max_err=(\S+) rows_off=(\d+) \| refreshed \| pass \S+ s$")
    got = [pat.match(l) for l in hist]
    assert len(hist) == epochs and all(got), hist             # one per epoch and per layer (one aggregation layer here)
    assert [int(m.group(1)) for m in got] == list(range(1, epochs + 1))
    rel = [float(m.group(2)) for m in got]
    assert rel[0] == 1.0 and all(0.0 < r < 1.0 for r in rel[1:])        # zeros before epoch 1; one epoch of drift after it
    # (the history line of an epoch comes before its Epoch: line)
    order = [l.split()[0] + l.split()[1] for l in lines if l.startswith("Epoch:") or l.startswith("[sgcn] history:")]
    assert order == ["[sgcn]history:", "Epoch:0001", "[sgcn]history:", "Epoch:0002", "[sgcn]history:", "Epoch:0003",
                     "[sgcn]history:", "Epoch:0004"]
    return rel


def test_train_main_end_to_end(tmp_path, monkeypatch):
    from stochastic_gcn_amd import exact_history, ops
    monkeypatch.chdir(tmp_path)
    rel = _check_log(_main(ARGS + HIST))
    print("staleness before epochs 1..4:", rel)
    z = np.load(str(tmp_path / "tmp" / "model.ckpt.npz"))
    assert "history/0" in z.files and np.isfinite(z["history/0"]).all() and np.abs(z["history/0"]).max() > 0
    lines = _main(ARGS + ['--load'])                          # the checkpoint loads back (--load refuses the history flags)
    assert any(l.startswith("Model restored from file") for l in lines) and any(l.startswith("Test set results:") for l in lines)
    # --test_full_batch --dense_dtype bf16 beside it: the evaluation multiplies in bfloat16, the history passes never do
    calls, inside = [], [0]
    real_gemm, real_run = ops.gemm_bf16, exact_history.ExactHistory.run

    def gemm_bf16(*a, **k):
        calls.append(inside[0])
        return real_gemm(*a, **k)

    def run(self, *a, **k):
        inside[0] += 1
        try:
            return real_run(self, *a, **k)
        finally:
            inside[0] -= 1
    monkeypatch.setattr(ops, "gemm_bf16", gemm_bf16)
    monkeypatch.setattr(exact_history.ExactHistory, "run", run)
    _check_log(_main(ARGS + HIST + ['--test_full_batch', '--dense_dtype', 'bf16']))
    assert len(calls) > 0 and not any(calls)
