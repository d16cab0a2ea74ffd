"""CPU tests of the full-graph modes (--full_batch / --test_full_batch / --full_batch_kernel): flags, refusals, the static
batch, the product count handed to static_kernel_for, and the two additive exports.  Nothing here touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from stochastic_gcn_amd import _ffi
from stochastic_gcn_amd.flags import FLAGS, _Flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sgcn_softmax_ce_rows_f32", "sgcn_sigmoid_ce_rows_f32")


@pytest.fixture(autouse=True)
def _reset_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


# ---- flags ------------------------------------------------------------------------------------------------------------
def test_flag_defaults_and_parsing():
    f = _Flags()
    assert f.full_batch is False and f.test_full_batch is False and f.full_batch_kernel == 'auto'
    f.parse(['--full_batch', '--test_full_batch', '--full_batch_kernel', 'cs'])
    assert f.full_batch is True and f.test_full_batch is True and f.full_batch_kernel == 'cs'
    f.parse(['--full_batch', '--nofull_batch', '--test_full_batch=False'])
    assert f.full_batch is False and f.test_full_batch is False
    f.parse(['--full_batch=False', '--test_full_batch=True', '--full_batch_kernel=lds'])
    assert f.full_batch is False and f.test_full_batch is True and f.full_batch_kernel == 'lds'
    f.parse(['--notest_full_batch', '--full_batch=true'])
    assert f.full_batch is True and f.test_full_batch is False
    for k in ('auto', 'rows', 'cs', 'lds'):
        assert f.parse(['--full_batch_kernel', k]).full_batch_kernel == k
    with pytest.raises(SystemExit):
        f.parse(['--full_batch_kernel', 'dense'])
    assert {'full_batch', 'test_full_batch', 'full_batch_kernel'} <= set(f.as_dict())


# ---- refusals ---------------------------------------------------------------------------------------------------------
TRAIN_REFUSED = ['cv', 'cvd', 'importance', 'det_dropout', 'gradvar']
TEST_REFUSED = ['test_cv', 'test_cvd', 'test_importance', 'det_dropout', 'gradvar']


@pytest.mark.parametrize("other", TRAIN_REFUSED)
def test_full_batch_refuses(other):
    from stochastic_gcn_amd.full_batch import check_full_batch
    FLAGS.update(full_batch=True, **{other: True})
    with pytest.raises(ValueError, match="--full_batch is not supported with --%s" % other):
        check_full_batch()


@pytest.mark.parametrize("other", TEST_REFUSED)
def test_test_full_batch_refuses(other):
    from stochastic_gcn_amd.full_batch import check_full_batch
    FLAGS.update(test_full_batch=True, **{other: True})
    with pytest.raises(ValueError, match="--test_full_batch is not supported with --%s" % other):
        check_full_batch()


def test_full_batch_refuses_several_ranks_and_bad_kernel():
    from stochastic_gcn_amd.full_batch import check_full_batch
    FLAGS.update(full_batch=True)
    assert check_full_batch(world=1) == (True, False)
    with pytest.raises(ValueError, match="2 ranks"):
        check_full_batch(world=2)
    FLAGS.update(full_batch=False, test_full_batch=True)
    assert check_full_batch(world=2) == (False, True)            # evaluation is the same on every rank
    FLAGS.update(full_batch_kernel='dense')
    with pytest.raises(ValueError, match="--full_batch_kernel must be one of auto/rows/cs/lds"):
        check_full_batch()


def test_independent_pairs_are_accepted():
    """--test_full_batch scores a --cv --cvd model; --full_batch evaluates by --test_cv batches; --history_dtype has
    nothing to act on in a model without history and is ignored there."""
    from stochastic_gcn_amd.full_batch import check_full_batch
    FLAGS.update(cv=True, cvd=True, test_full_batch=True)
    assert check_full_batch() == (False, True)
    FLAGS.reset()
    FLAGS.update(full_batch=True, test_cv=True, history_dtype='bf16')
    assert check_full_batch() == (True, False)


@pytest.mark.parametrize("flags,msg", [
    (dict(full_batch=True, cv=True), "--full_batch is not supported with --cv"),
    (dict(full_batch=True, det_dropout=True), "--full_batch is not supported with --det_dropout"),
    (dict(test_full_batch=True, test_cv=True), "--test_full_batch is not supported with --test_cv"),
])
def test_trainer_refuses_before_a_device_is_touched(monkeypatch, flags, msg):
    """The Trainer raises the refusal ahead of its first look at the GPU and ahead of loading anything."""
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
    FLAGS.update(full_batch=True)
    with pytest.raises(ValueError, match="2 ranks"):
        train.Trainer(verbose=False)


# ---- the static batch -------------------------------------------------------------------------------------------------
class _FakeMatrix(object):
    bf16 = False

    def __init__(self, n, nnz):
        self.shape, self.nnz, self.device = (n, n), nnz, torch.device("cpu")


def test_static_batch_shapes():
    from stochastic_gcn_amd.full_batch import StaticBatch
    N, C, L = 11, 3, 2
    labels = np.eye(C, dtype=np.float32)[np.arange(N) % C]
    A = _FakeMatrix(N, 40)
    sb = StaticBatch(A, labels, np.array([1, 4, 9]), L, torch.device("cpu"))
    assert len(sb.fields) == L + 1 and len(sb.scales) == L and len(sb.adj) == L
    for f in sb.fields:
        assert f.dtype == torch.int32 and torch.equal(f, torch.arange(N, dtype=torch.int32))
    for s in sb.scales:
        assert s.dtype == torch.float32 and torch.equal(s, torch.ones(N))
    assert all(a is A for a in sb.adj)                           # ONE shared matrix object
    assert tuple(sb.labels.shape) == (N, C) and sb.labels.dtype == torch.float32
    assert sb.rows.dtype == torch.int32 and sb.rows.tolist() == [1, 4, 9]
    assert sb.sizes == dict(adj=[40, 40], fadj=[0, 0], fields=[N, N, N])       # the epoch counters count nnz and N per layer
    cur = sb.cur("inputs")
    assert cur.inputs == "inputs" and cur.rows is sb.rows and cur.adj[0] is A and cur.labels is sb.labels
    assert np.array_equal(cur.host_fields[0], np.arange(N))
    other = sb.with_rows(np.array([0, 10]))
    assert other.rows.tolist() == [0, 10] and sb.rows.tolist() == [1, 4, 9] and other.labels is sb.labels
    assert other.adj[0] is A


@pytest.mark.parametrize("rows", [[4, 1, 9], [1, 1, 4], [1, 4, 11], [-1, 3], []])
def test_static_batch_rows_must_be_sorted_unique_in_range(rows):
    from stochastic_gcn_amd.full_batch import StaticBatch
    labels = np.zeros((11, 3), np.float32)
    with pytest.raises(ValueError, match="loss rows"):
        StaticBatch(_FakeMatrix(11, 40), labels, np.array(rows, dtype=np.int64), 1, torch.device("cpu"))
    sb = StaticBatch(_FakeMatrix(11, 40), labels, np.array([0, 10]), 1, torch.device("cpu"))
    with pytest.raises(ValueError, match="loss rows"):
        sb.with_rows(np.array(rows, dtype=np.int64))


def test_static_batch_checks_the_label_table():
    from stochastic_gcn_amd.full_batch import StaticBatch
    with pytest.raises(ValueError, match="labels has 10 rows"):
        StaticBatch(_FakeMatrix(11, 40), np.zeros((10, 3), np.float32), np.array([0]), 1, torch.device("cpu"))


# ---- the kernel choice ------------------------------------------------------------------------------------------------
def _ring(n):
    i = np.arange(n)
    return sp.csr_matrix((np.ones(2 * n, np.float32), (np.r_[i, i], np.r_[(i + 1) % n, (i + 3) % n])), shape=(n, n))


def test_auto_asks_static_kernel_for_with_the_product_count(monkeypatch):
    """auto = static_kernel_for(nnz, d, products), products = the number of times that plan will run: the epochs for a
    training matrix (SGDTrain runs epochs + 2 of them), one evaluation per epoch and the test for full_adj."""
    from stochastic_gcn_amd import full_batch, train
    from stochastic_gcn_amd.full_batch import StaticMatrix
    seen = []
    monkeypatch.setattr(full_batch, "static_kernel_for", lambda nnz, d, products: seen.append((nnz, d, products)) or 'rows')
    FLAGS.update(epochs=37)
    assert train.full_batch_products('train') == 39 and train.full_batch_products('full') == 40
    a = _ring(50)
    m = StaticMatrix(a, torch.device("cpu"), 'auto', train.full_batch_products('train'), 128)
    assert m.kernel == 'rows' and seen == [(100, 128, 39)]
    assert m.shape == (50, 50) and m.nnz == 100
    t = m.transpose                                              # the transposed plan: the same count, asked or inherited
    assert t.kernel == 'rows' and t.shape == (50, 50) and t.transpose is m
    assert (t.a != a.T.tocsr()).nnz == 0
    m2 = StaticMatrix(a, torch.device("cpu"), 'auto', train.full_batch_products('full'), 64)
    assert seen[-1] == (100, 64, 40) and m2.kernel == 'rows'
    n = len(seen)
    assert StaticMatrix(a, torch.device("cpu"), 'rows', 5, 64).kernel == 'rows' and len(seen) == n     # forced: not asked


def test_trainer_hands_the_counts_over(monkeypatch):
    """Trainer._static_batch: the training matrix with the epochs, full_adj with the evaluations, the operand type of
    --full_batch_dtype as an ordinary keyword."""
    from stochastic_gcn_amd import full_batch, train
    made, operand = [], []

    class Rec(object):
        def __init__(self, a, device, kernel, products, d, cache_path, bf16):
            made.append((a.shape, kernel, products, d, cache_path))
            operand.append(bf16)
            self.shape, self.nnz, self.device, self.bf16 = a.shape, a.nnz, device, bf16
    monkeypatch.setattr(full_batch, "StaticMatrix", Rec)            # (full_batch.model_matrix constructs it)
    FLAGS.update(epochs=12, hidden1=48, full_batch_kernel='auto')

    class M(object):
        L, agg0_dim = 2, 48
    tr = train.Trainer.__new__(train.Trainer)
    tr.device, tr.labels = torch.device("cpu"), np.zeros((50, 3), np.float32)
    tr.static_matrices, tr._labels_dev = [], None
    sb = tr._static_batch(_ring(50), 'train', None, M(), np.array([7, 3, 5]))
    assert made[-1] == ((50, 50), 'auto', 14, 48, None) and sb.rows.tolist() == [3, 5, 7] and sb.L == 2
    assert operand[-1] is False
    tr._static_batch(_ring(50), 'full', "x.npz", M(), np.array([1]))
    assert made[-1] == ((50, 50), 'auto', 15, 48, "x.npz")
    assert isinstance(sb, full_batch.StaticBatch)
    FLAGS.update(full_batch_dtype='bf16', full_batch=True)
    tr._static_batch(_ring(50), 'train', None, M(), np.array([1]))
    assert made[-1] == ((50, 50), 'auto', 14, 48, None) and operand[-1] is True
    assert [m for _, m in tr.static_matrices] and all(isinstance(m, Rec) for _, m in tr.static_matrices)


def test_unaligned_width_falls_back_to_the_row_kernel():
    """A width that is not a multiple of 4 floats (or a misaligned view) takes the row kernel for that product; the
    decision needs no device."""
    from stochastic_gcn_amd.full_batch import StaticMatrix
    m = StaticMatrix.__new__(StaticMatrix)
    m.kernel = 'cs'
    assert m.kernel_for(torch.zeros(8, 16)) == 'cs'
    assert m.kernel_for(torch.zeros(8, 7)) == 'rows'
    assert m.kernel_for(torch.zeros(8, 16), out=torch.zeros(8, 32)[:, 16:]) == 'cs'
    assert m.kernel_for(torch.zeros(8, 16), out=torch.zeros(8, 34)[:, 18:]) == 'rows'
    assert m.kernel_for(torch.zeros(8, 20)[:, 2:18]) == 'rows'
    m.kernel = 'rows'
    assert m.kernel_for(torch.zeros(8, 16)) == 'rows'


# ---- one path for every static-graph product ---------------------------------------------------------------------------
class _FakeClock(object):
    def __init__(self):
        self.pace = {}


class _FakePlan(object):
    """What StaticMatrix asks of a ColumnSweepCSR, recorded."""

    def __init__(self, log):
        self.log, self._clock = log, _FakeClock()

    def clock(self, bf16=False):
        return self._clock

    def autotune(self, x, d=None):
        self.log.append(('autotune', tuple(x.shape), d))
        self._clock.pace[d] = 250

    def store_if_cached(self):
        self.log.append(('store_if_cached',))

    def variant(self, d, bf16=False):
        return "fake sweep d=%d" % d


@pytest.fixture
def recorded(monkeypatch):
    """Recorders in place of everything StaticMatrix builds or launches: ``log`` lists the calls in order."""
    from stochastic_gcn_amd import ops
    log = []

    def product(name):
        def run(A, x, out=None, beta=0.0, d=None, **kw):
            log.append((name, tuple(x.shape), tuple(x.stride()), d, beta))
            return torch.zeros((A.shape[0], x.shape[1]))
        return run

    class Csr(object):
        def __init__(self, a):
            self.shape = a.shape
    monkeypatch.setattr(ops.DeviceCSR, "from_scipy", staticmethod(lambda a, device: log.append(('from_scipy',)) or Csr(a)))

    def cached(a, device, path=None, G=1):
        log.append(('cached', path, G))
        plan = _FakePlan(log)
        plan.shape = a.shape
        return plan, False
    monkeypatch.setattr(ops.ColumnSweepCSR, "cached", staticmethod(cached))
    monkeypatch.setattr(ops.LdsSweepCSR, "for_graph", staticmethod(lambda a, device: log.append(('for_graph',))))
    monkeypatch.setattr(ops, "spmm", product('spmm'))
    monkeypatch.setattr(ops, "spmm_cs", product('spmm_cs'))
    monkeypatch.setattr(ops, "spmm_lds", product('spmm_lds'))
    return log


def _pp(log, monkeypatch, verdict, **kw):
    from stochastic_gcn_amd import full_batch, train
    asked = []
    monkeypatch.setattr(full_batch, "static_kernel_for", lambda nnz, d, products: asked.append((nnz, d, products)) or verdict)
    a, X = _ring(50), torch.arange(300, dtype=torch.float32).reshape(50, 6)
    tf, ff = train.pp_products(a, a, X, torch.device("cpu"), **kw)
    assert tuple(tf.shape) == tuple(ff.shape) == (50, 6) and tf.is_contiguous()
    return asked


def test_pp_products_run_once_ask_the_cost_model_and_take_the_rows_kernel(recorded, monkeypatch):
    asked = _pp(recorded, monkeypatch, 'rows', products=1)
    assert asked == [(100, 6, 1)] * 2
    assert [c[0] for c in recorded] == ['from_scipy', 'spmm', 'from_scipy', 'spmm']


def test_pp_products_sweep_an_unaligned_width_on_a_padded_pitch(recorded, monkeypatch):
    """Width 6 is no multiple of 4: pp_products pads the pitch once and the sweep -- not the row kernel that
    StaticMatrix.product would fall back to -- takes the view."""
    from stochastic_gcn_amd import ops
    stats = []
    _pp(recorded, monkeypatch, 'cs', products=200, cache=("t.npz", "f.npz"), stats=stats)
    G = ops.ColumnSweepCSR.choose_g(6, 100 / 50, 50)
    assert [c for c in recorded if c[0] == 'cached'] == [('cached', "t.npz", G), ('cached', "f.npz", G)]
    products = [c for c in recorded if c[0].startswith('spmm')]
    assert [c[0] for c in products] == ['spmm_cs', 'spmm_cs']
    for _, shape, stride, d, beta in products:
        assert shape == (50, 6) and stride[0] % 4 == 0 and stride[1] == 1 and d == 6 and beta == 0.0
    for c in recorded:
        if c[0] == 'autotune':
            assert c[1] == (50, 6) and c[2] == 6
    assert not any(c[0] in ('for_graph', 'from_scipy') for c in recorded)          # a cache path: the LDS planner is not asked
    assert len(stats) == 2
    for rec in stats:
        assert set(rec) == {'plan_from_cache', 'pace', 'kernel', 'products'}
        assert rec == dict(plan_from_cache=False, pace=250, kernel="fake sweep d=6", products=200)


def test_multiply_tunes_a_width_once(recorded):
    from stochastic_gcn_amd.full_batch import StaticMatrix
    m = StaticMatrix(_ring(50), torch.device("cpu"), 'cs', 5, 8, "p.npz")
    x = torch.zeros(50, 8)
    m.multiply(x)
    first = [c[0] for c in recorded]
    assert first == ['cached', 'autotune', 'store_if_cached', 'spmm_cs']
    m.multiply(x)
    assert [c[0] for c in recorded[len(first):]] == ['spmm_cs']                    # no autotune, no store
    m.multiply(torch.zeros(50, 12))                                                 # another width: its own tune
    assert [c[0] for c in recorded[len(first) + 1:]] == ['autotune', 'store_if_cached', 'spmm_cs']
    with pytest.raises(ValueError, match="not on 'lds'"):
        m.multiply(x, kernel='lds')
    assert m.describe(8) == dict(plan_from_cache=False, pace=250, kernel="fake sweep d=8", products=5)


def test_forward_only_static_batch():
    from stochastic_gcn_amd.full_batch import StaticBatch
    N, L = 11, 2
    A, dev = _FakeMatrix(N, 40), torch.device("cpu")
    full = StaticBatch(A, np.zeros((N, 3), np.float32), np.array([1, 4]), L, dev)
    fwd = StaticBatch(A, None, None, L, dev)
    assert fwd.labels is None and fwd.rows is None and fwd.host_rows is None
    assert (fwd.N, fwd.L, fwd.dropout, fwd.sizes) == (full.N, full.L, full.dropout, full.sizes)
    assert len(fwd.fields) == L + 1 and len(fwd.scales) == L
    assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(fwd.fields + fwd.scales, full.fields + full.scales))
    assert fwd.adj == full.adj == [A] * L and np.array_equal(fwd.host_field, full.host_field)
    cur = fwd.cur("inputs")
    assert cur.labels is None and cur.rows is None and cur.adj[0] is A
    with pytest.raises(ValueError, match="forward-only"):
        fwd.with_rows(np.array([0]))
    with pytest.raises(ValueError, match="label table"):
        StaticBatch(A, None, np.array([0]), L, dev)


def test_full_batch_does_not_import_train():
    import subprocess
    import sys
    code = ("import sys; import stochastic_gcn_amd.full_batch; "
            "sys.exit(1 if 'stochastic_gcn_amd.train' in sys.modules else 0)")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


# ---- the exports ------------------------------------------------------------------------------------------------------
def test_new_exports_agree_in_header_library_and_ctypes_table():
    src = open(os.path.join(ROOT, "include", "sgcn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    plain = {"sgcn_softmax_ce_rows_f32": "sgcn_softmax_ce_f32", "sgcn_sigmoid_ce_rows_f32": "sgcn_sigmoid_ce_f32"}
    for s in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, src)
        assert m, "%s is not declared in include/sgcn.h" % s
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == 15
        assert hasattr(lib, s), "libsgcn.so does not export %s" % s
        restype, argtypes = _ffi.SIGNATURES[s]
        assert restype is ctypes.c_int and len(argtypes) == 15
        # the plain entry point's operands with (N, c, rows, n) in place of (n, c)
        p = list(_ffi.SIGNATURES[plain[s]][1])
        assert argtypes == p[:4] + [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32] + p[6:]
        for a, t in zip(args, argtypes):
            want = ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_int32 if a.startswith("int32_t") else ctypes.c_void_p
            assert t is want, (s, a, t)
    assert _ffi.lib.sgcn_abi_version() == _ffi.ABI_VERSION == 16           # additive: the version stays


@pytest.mark.parametrize("name", NEW)
def test_new_exports_validate_before_any_hip_call(name):
    fn = getattr(_ffi.lib, name)
    one = ctypes.c_void_p(16)           # never dereferenced: validation comes first
    ok = dict(z=one, ldz=5, y=one, ldl=5, N=9, c=5, rows=one, n=4, dz=one, lddz=5, p=one, ldp=5, st=one, rs=one)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return fn(a['z'], a['ldz'], a['y'], a['ldl'], a['N'], a['c'], a['rows'], a['n'], a['dz'], a['lddz'], a['p'], a['ldp'],
                  a['st'], a['rs'], None)
    for bad in (dict(n=0), dict(n=10), dict(rows=None), dict(ldz=4), dict(ldl=4), dict(lddz=4), dict(ldp=4), dict(N=0),
                dict(z=None), dict(rs=None)):
        assert call(**bad) == -1, bad
        assert b"ce_rows" in _ffi.lib.sgcn_last_error()


def test_ops_losses_take_rows_and_refuse_cpu_tensors():
    import inspect
    from stochastic_gcn_amd import ops
    for f in (ops.softmax_ce, ops.sigmoid_ce):
        assert inspect.signature(f).parameters['rows'].default is None
        with pytest.raises(RuntimeError, match="HBM"):
            f(torch.zeros(4, 3), torch.zeros(4, 3), rows=torch.zeros(2, dtype=torch.int32))
    assert ops.check_loss_rows([0, 2, 3], 4).dtype == np.int32
    with pytest.raises(ValueError):
        ops.check_loss_rows([2, 0], 4)


def test_row_restricted_gate_interval_is_the_full_enumeration():
    """full_batch_cases.first_layer_gate_interval (what the full-size GPU test holds the first layer's weight gradient to)
    against test_model_gpu._gate_interval, one full oracle backward pass per ambiguous gate, on 3,000 and 9,000 vertices:
    the same interval up to fp32 summation noise, with and without pre-processing.  Oracle only."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import full_batch_cases as fc
    from oracle import model_np as mnp
    from test_model_gpu import BAND, _gate_interval
    for name in ('reddit3k_pp', 'reddit3k_nopp', 'sbm_lds'):
        case = fc.build(name)
        fl = case['flags']
        om = fc.oracle_model(case, case['nbr_train'], seed=3)
        feed, rows = fc.exact_feed(case, case['train_adj'], fl['dropout']), np.sort(case['train'])
        logits, _ = om.forward(feed, case['ph'], fl['dropout'], mnp.HashMasks(1, 0, 1.0 - fl['dropout']))
        dout = np.zeros_like(logits)
        dout[rows] = om.loss_and_grad(logits[rows], case['labels'][rows])[3]
        lo, hi, k = _gate_interval(om, dout)
        lo2, hi2, g, k2 = fc.first_layer_gate_interval(om, dout, BAND)
        gmax = np.abs(g).max()
        assert k == k2 and k >= 3
        assert np.abs(hi['dense0/weights'] - lo['dense0/weights']).max() > 1e-3 * gmax          # the interval is not trivial
        assert np.abs(lo2 - lo['dense0/weights']).max() <= 5e-6 * gmax and np.abs(hi2 - hi['dense0/weights']).max() <= 5e-6 * gmax
        assert np.array_equal(g, om.backward(dout)['dense0/weights'])
