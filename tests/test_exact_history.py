"""CPU tests of the exact control-variate history (--history_init / --history_refresh / --history_error): flags, refusals,
the refresh schedule, the pass count handed to the kernel choice, and the three additive exports.  Nothing here touches a
device."""
import ctypes
import os
import re

import pytest
import torch

from stochastic_gcn_amd import _ffi
from stochastic_gcn_amd.flags import FLAGS, _Flags, check_exact_history

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sgcn_hist_error_f32", "sgcn_hist_error_h16", "sgcn_hist_error_ws_doubles")
A = 4096       # a non-null address that is never dereferenced: the calls below fail validation first


@pytest.fixture(autouse=True)
def _reset_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


# ---- flags ------------------------------------------------------------------------------------------------------------
def test_defaults_and_parsing():
    f = _Flags()
    assert (f.history_init, f.history_refresh, f.history_error) == ('zeros', 0, False)
    f.parse([])
    assert (f.history_init, f.history_refresh, f.history_error) == ('zeros', 0, False)
    assert check_exact_history(f) == (False, 0, False)
    f.parse(['--cv', '--history_init', 'exact', '--history_refresh', '3', '--history_error'])
    assert (f.history_init, f.history_refresh, f.history_error) == ('exact', 3, True)
    assert check_exact_history(f) == (True, 3, True)
    f.parse(['--history_init=zeros', '--nohistory_error', '--history_refresh=0'])
    assert (f.history_init, f.history_refresh, f.history_error) == ('zeros', 0, False)
    with pytest.raises(SystemExit):
        f.parse(['--history_init', 'ones'])
    assert {'history_init', 'history_refresh', 'history_error'} <= set(f.as_dict())


# ---- refusals ---------------------------------------------------------------------------------------------------------
ON = [dict(history_init='exact'), dict(history_refresh=2), dict(history_error=True)]


def test_init_exact_needs_a_history_owner():
    FLAGS.update(history_init='exact')
    with pytest.raises(ValueError, match="--history_init exact needs --cv or --test_cv"):
        check_exact_history()
    FLAGS.update(test_cv=True)
    assert check_exact_history() == (True, 0, False)              # the test model alone owns one
    FLAGS.update(test_cv=False, cv=True)
    assert check_exact_history() == (True, 0, False)


@pytest.mark.parametrize("flag,name", [(dict(history_refresh=2), "--history_refresh"), (dict(history_error=True), "--history_error")])
def test_refresh_and_error_need_cv(flag, name):
    FLAGS.update(test_cv=True, **flag)                            # (a test-model history does not make them meaningful)
    with pytest.raises(ValueError, match="%s needs --cv" % name):
        check_exact_history()
    FLAGS.update(cv=True)
    check_exact_history()


def test_negative_refresh():
    FLAGS.update(cv=True, history_refresh=-1)
    with pytest.raises(ValueError, match="--history_refresh must be >= 0"):
        check_exact_history()


def test_unknown_init():
    FLAGS.update(cv=True, history_init='ones')
    with pytest.raises(ValueError, match="--history_init must be one of zeros/exact"):
        check_exact_history()


@pytest.mark.parametrize("on", ON)
@pytest.mark.parametrize("other", ['det_dropout', 'gradvar', 'load'])
def test_refused_with(on, other):
    FLAGS.update(cv=True, test_cv=True, **on)
    check_exact_history()
    FLAGS.update(**{other: True})
    with pytest.raises(ValueError, match="is not supported with --%s" % other):
        check_exact_history()


@pytest.mark.parametrize("on", ON)
def test_refused_on_several_ranks(on):
    FLAGS.update(cv=True, **on)
    check_exact_history(world=1)
    with pytest.raises(ValueError, match="2 ranks"):
        check_exact_history(world=2)
    FLAGS.reset()
    FLAGS.update(cv=True)
    assert check_exact_history(world=2) == (False, 0, False)      # (the flags absent: nothing to refuse)


def test_history_dtype_bf16_is_accepted():
    FLAGS.update(cv=True, cvd=True, history_dtype='bf16', history_init='exact', history_refresh=1, history_error=True)
    assert check_exact_history() == (True, 1, True)


@pytest.mark.parametrize("flags,msg", [
    (dict(history_init='exact'), "--history_init exact needs --cv or --test_cv"),
    (dict(history_error=True), "--history_error needs --cv"),
    (dict(cv=True, history_refresh=-2), "--history_refresh must be >= 0"),
    (dict(cv=True, history_refresh=1, det_dropout=True), "--history_refresh is not supported with --det_dropout"),
    (dict(cv=True, history_init='exact', gradvar=True), "--history_init exact is not supported with --gradvar"),
    (dict(cv=True, history_error=True, load=True), "--history_error is not supported with --load"),
])
def test_trainer_refuses_before_a_device_is_touched(monkeypatch, flags, msg):
    from stochastic_gcn_amd import train
    touched = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: touched.append("is_available") or False)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: touched.append("set_device"))
    monkeypatch.setattr(train, "load_data", lambda *a, **k: touched.append("load_data"))
    FLAGS.update(**flags)
    with pytest.raises(ValueError, match=msg):
        train.Trainer(verbose=False)
    assert touched == []


def test_trainer_refuses_several_ranks(monkeypatch):
    from stochastic_gcn_amd import train
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("device touched"))
    FLAGS.update(cv=True, history_init='exact')
    with pytest.raises(ValueError, match="2 ranks"):
        train.Trainer(verbose=False)


# ---- the schedule -----------------------------------------------------------------------------------------------------
def test_refresh_schedule():
    from stochastic_gcn_amd.exact_history import refresh_due
    assert [e for e in range(10) if refresh_due(e, 0)] == []
    assert [e for e in range(6) if refresh_due(e, 1)] == [1, 2, 3, 4, 5]          # (0-based: before the log's epochs 2, 3, ...)
    assert [e for e in range(10) if refresh_due(e, 3)] == [3, 6, 9]                # before the log's epochs 4, 7, 10 = K+1, 2K+1, ...
    assert not any(refresh_due(0, k) for k in (0, 1, 3, 100))                      # epoch 0 is filled through --history_init only


def test_history_pass_runs_one_pass_per_epoch_and_measures_before_it_assigns():
    """Trainer.history_pass on a recording stand-in: which epochs run a pass, with which of (measure, assign)."""
    from stochastic_gcn_amd import train

    class Ex(object):
        def __init__(self):
            self.calls = []

        def run(self, measure=False, assign=False):
            self.calls.append((measure, assign))
            return dict(layers=[dict(rel_err=0.5, max_err=1.0, rows_off=3)] if measure else None, refreshed=assign, pass_s=0.0)

    class M(object):
        L = 1

    def trainer(init, refresh, error, test=False):
        tr = train.Trainer.__new__(train.Trainer)
        tr.history_init_exact, tr.history_refresh, tr.history_error = init, refresh, error
        tr.exact_train, tr.exact_test, tr.train_model, tr.lines = Ex(), (Ex() if test else None), M(), []
        tr.log = lambda *a: tr.lines.append(" ".join(str(x) for x in a))
        return tr

    tr = trainer(True, 2, False, test=True)
    recs = [tr.history_pass(e) for e in range(5)]
    assert tr.exact_train.calls == [(False, True)] * 3 and [r is not None for r in recs] == [True, False, True, False, True]
    assert tr.exact_test.calls == [(False, True)]                               # the test model: once, before epoch 0
    assert recs[2]['epoch'] == 3 and recs[2]['refreshed'] and recs[2]['layers'] is None
    tr = trainer(False, 0, True)
    recs = [tr.history_pass(e) for e in range(3)]
    assert tr.exact_train.calls == [(True, False)] * 3 and all(not r['refreshed'] for r in recs)
    assert len(tr.lines) == 3 and all(re.match(r"\[sgcn\] history: epoch 000\d layer 0 rel_err=5\.0+e-01 max_err=1\.0+e\+00 "
                                                r"rows_off=3 \| pass ", l) for l in tr.lines)
    tr = trainer(True, 1, True)                                                 # both fall on every epoch: ONE pass each
    [tr.history_pass(e) for e in range(3)]
    assert tr.exact_train.calls == [(True, True)] * 3 and all(" | refreshed | pass " in l for l in tr.lines)
    tr = trainer(False, 0, False)
    tr.exact_train = None                                                       # the defaults: nothing is built, nothing runs
    assert [tr.history_pass(e) for e in range(3)] == [None] * 3 and tr.lines == []


# ---- the pass count ---------------------------------------------------------------------------------------------------
def test_pass_count_per_flag_set():
    from stochastic_gcn_amd.exact_history import history_passes
    FLAGS.update(epochs=10)
    assert history_passes('train') == 0 and history_passes('test') == 0
    FLAGS.update(history_init='exact')
    assert history_passes('train') == 1 and history_passes('test') == 1
    FLAGS.update(history_refresh=3)
    assert history_passes('train') == 1 + 12 // 3 and history_passes('test') == 1
    FLAGS.update(history_refresh=5, history_init='zeros')
    assert history_passes('train') == 12 // 5 and history_passes('test') == 0
    FLAGS.update(history_error=True)                                            # a pass before every one of epochs + 2 epochs
    assert history_passes('train') == 12
    FLAGS.update(history_init='exact', history_refresh=0)
    assert history_passes('train') == 13 and history_passes('test') == 1


def test_matrix_gets_the_products_of_the_passes(monkeypatch):
    """make_matrix: fp32 operand, the kernel of --full_batch_kernel, passes x (L - 1) products -- a pass stops at the last
    aggregator's input."""
    from stochastic_gcn_amd import exact_history, full_batch
    made = []

    class Rec(object):
        def __init__(self, a, device, kernel, products, d, cache_path, bf16=None):
            made.append((kernel, products, d, cache_path, bf16))
    monkeypatch.setattr(full_batch, "StaticMatrix", Rec)            # (full_batch.model_matrix constructs it)

    class M(object):
        def __init__(self, L, agg0):
            self.L, self.agg0_dim = L, agg0
    FLAGS.update(hidden1=48, full_batch_kernel='cs', full_batch_dtype='bf16', test_full_batch=True)
    exact_history.make_matrix("adj", "dev", M(1, 48), 7, "p.npz")
    assert made[-1] == ('cs', 0, 48, "p.npz", False)
    FLAGS.update(full_batch_kernel='auto')
    exact_history.make_matrix("adj", "dev", M(2, 602), 7)
    assert made[-1] == ('auto', 7, 602, None, False)
    exact_history.make_matrix("adj", "dev", M(3, 20), 4)
    assert made[-1] == ('auto', 8, 48, None, False)


# ---- the exports ------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_binding_and_library():
    src = open(os.path.join(ROOT, "include", "sgcn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sgcn_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for s in NEW:
        assert s in declared and s in _ffi.SIGNATURES and hasattr(lib, s), s
    assert _ffi.lib.sgcn_abi_version() == _ffi.ABI_VERSION == 16
    assert _ffi.lib.sgcn_hist_error_ws_doubles() == 4 * 1024
    assert _ffi.SIGNATURES["sgcn_hist_error_f32"] == _ffi.SIGNATURES["sgcn_hist_error_h16"]


@pytest.mark.parametrize("fn", ["sgcn_hist_error_f32", "sgcn_hist_error_h16"])
def test_argument_checks_run_before_any_hip_call(fn):
    f = getattr(_ffi.lib, fn)

    def fails(rc, text):
        assert rc == -1 and text in _ffi.lib.sgcn_last_error(), _ffi.lib.sgcn_last_error()
    fails(f(A, 8, A, 8, -1, 8, A, A, None), b"negative size")
    fails(f(A, 8, A, 8, 4, -1, A, A, None), b"negative size")
    fails(f(A, 8, A, 8, 4, 8, None, A, None), b"out4")
    fails(f(None, 8, A, 8, 4, 8, A, A, None), b"null operand")
    fails(f(A, 8, None, 8, 4, 8, A, A, None), b"null operand")
    fails(f(A, 8, A, 8, 4, 8, A, None, None), b"null operand")
    fails(f(A, 7, A, 8, 4, 8, A, A, None), b"leading dimension too small")
    fails(f(A + 2, 8, A, 8, 4, 8, A, A, None), b"not aligned")


def test_h16_storage_contract():
    f = _ffi.lib.sgcn_hist_error_h16
    assert f(A, 8, A, 12, 4, 8, A, A, None) == -1 and b"ldh % 8 == 0" in _ffi.lib.sgcn_last_error()
    assert f(A, 8, A + 8, 8, 4, 8, A, A, None) == -1 and b"16-byte aligned" in _ffi.lib.sgcn_last_error()
    assert f(A, 3, A, 0, 4, 3, A, A, None) == -1 and b"leading dimension too small" in _ffi.lib.sgcn_last_error()


def test_history_error_refuses_host_tensors_and_shape_mismatch():
    from stochastic_gcn_amd import ops
    with pytest.raises(RuntimeError, match="HBM"):
        ops.history_error(torch.zeros(4, 8), torch.zeros(4, 8))
