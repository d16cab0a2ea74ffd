"""CPU tests of --aggregator max: the NumPy reference of the element-wise neighbour maximum against two brute-force forms,
the flag and its refusals, and the two exports' argument checks.  Nothing here touches a device."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import sparse_cases as sc
import spmax_ref as ref
from stochastic_gcn_amd import _ffi, ops
from stochastic_gcn_amd.flags import _DEFS, FLAGS, _Flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _reset_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


# ---- the reference against brute force ------------------------------------------------------------------------------------
def _small_patterns():
    rng = np.random.RandomState(11)
    out = {name: sc.pattern(name) for name in ("m15_k17", "m16_k16", "m17_k15", "k5")}
    a = sc.pattern("m63_k65").tolil()
    a[3, :] = 0                                  # empty rows among the others
    a[40, :] = 0
    out["with_empty_rows"] = a.tocsr()
    out["empty"] = sp.csr_matrix((6, 9), dtype=np.float32)
    out["dense_block"] = sp.csr_matrix(np.ones((7, 12), np.float32))
    out["one_row"] = sc._csr(5, 40, np.full(30, 2), rng.choice(40, 30, replace=False))
    return out


def _tables(K, d, rng):
    t = {
        "normal": rng.standard_normal((K, d)).astype(np.float32),
        "ties": rng.randint(-2, 3, (K, d)).astype(np.float32),
        "constant": np.full((K, d), 1.5, np.float32),
        "all_negative": -np.abs(rng.standard_normal((K, d))).astype(np.float32) - 1.0,
    }
    z = np.zeros((K, d), np.float32)
    z[::2] = -0.0                                # -0.0 before +0.0 ...
    t["neg_zero_first"] = z.copy()
    t["pos_zero_first"] = -z                      # ... and the reverse
    mixed = rng.randint(-1, 2, (K, d)).astype(np.float32) * rng.choice([0.0, -0.0, 1.0], (K, d)).astype(np.float32)
    t["mixed_zeros"] = mixed
    inf = rng.standard_normal((K, d)).astype(np.float32)
    inf[:, 0] = -np.inf                          # a column that is -inf everywhere
    inf[rng.rand(K) < 0.3, d - 1] = -np.inf      # and one that is -inf here and there
    inf[rng.rand(K) < 0.1, d // 2] = np.inf
    t["inf"] = inf
    return t


@pytest.mark.parametrize("name", sorted(_small_patterns()))
def test_reference_forward_against_brute_force(name):
    a = _small_patterns()[name]
    rng = np.random.RandomState(3)
    for kind, B in _tables(a.shape[1], 5, rng).items():
        C, arg = ref.forward(a, B)
        C1, arg1 = ref.forward_loops(a, B)
        C2, arg2 = ref.forward_dense(a, B)
        assert ref.same_bits(C, C1) and np.array_equal(arg, arg1), (name, kind)
        assert ref.same_bits(C, C2) and np.array_equal(arg, arg2), (name, kind)
        deg = np.diff(a.indptr)
        assert np.all(arg[deg == 0] == -1) and np.all(C[deg == 0].view(np.int32) == 0)           # +0.0, not -0.0
        rows = np.nonzero(deg)[0]
        for i in rows:                                                                            # np.max, and C holds bits of B
            cols = a.indices[a.indptr[i]:a.indptr[i + 1]]
            assert np.array_equal(C[i], B[cols].max(axis=0))
            assert ref.same_bits(C[i], B[arg[i], np.arange(B.shape[1])])
            assert np.all(np.isin(arg[i], cols))


def test_reference_tie_rule_by_hand():
    a = sp.csr_matrix((np.ones(4, np.float32), np.array([1, 2, 4, 5]), np.array([0, 4, 4])), shape=(2, 6))
    B = np.zeros((6, 4), np.float32)
    B[:, 0] = [9, -0.0, 0.0, 9, 0.0, -0.0]        # -0.0 first: it stays, no later zero is greater
    B[:, 1] = [9, 0.0, -0.0, 9, -0.0, 0.0]        # +0.0 first
    B[:, 2] = [9, -np.inf, -np.inf, 9, -np.inf, -np.inf]
    B[:, 3] = [9, -3, -1, 9, -1, -2]              # all negative, the maximum twice: the first of them
    C, arg = ref.forward(a, B)
    assert arg[0].tolist() == [1, 1, 1, 2] and arg[1].tolist() == [-1] * 4
    assert C[0].view(np.int32).tolist() == np.array([-0.0, 0.0, -np.inf, -1], np.float32).view(np.int32).tolist()
    assert C[1].view(np.int32).tolist() == [0, 0, 0, 0]
    # stored order, not column order, decides: the same row stored as 5, 4, 2, 1
    b = sp.csr_matrix((np.ones(4, np.float32), np.array([5, 4, 2, 1]), np.array([0, 4, 4])), shape=(2, 6))
    C, arg = ref.forward(b, B)
    assert arg[0].tolist() == [5, 5, 5, 4]
    assert C[0].view(np.int32).tolist() == np.array([-0.0, 0.0, -np.inf, -1], np.float32).view(np.int32).tolist()


@pytest.mark.parametrize("name", ["m15_k17", "m17_k15", "k5", "with_empty_rows", "dense_block", "empty"])
def test_reference_backward_against_loops(name):
    a = _small_patterns()[name]
    rng = np.random.RandomState(4)
    M, K = a.shape
    d = 3
    _, arg = ref.forward(a, rng.randint(-2, 3, (K, d)).astype(np.float32))
    G = rng.standard_normal((M, d)).astype(np.float32)
    add = rng.standard_normal((K, d + 2)).astype(np.float32)
    for kw in (dict(), dict(add=add, add_rows=K), dict(add=add, add_rows=K // 2)):
        dB = ref.backward(a, G, arg, **kw)
        assert ref.same_bits(dB, ref.backward_loops(a, G, arg, **kw))
        d64, bound = ref.backward_f64(a, G, arg, **kw)
        assert np.all(np.abs(dB.astype(np.float64) - d64) <= bound)
    # every gradient element lands exactly once: the column sums agree (integers: exact)
    Gi = sc.ints(rng, (M, d))
    dB = ref.backward(a, Gi, arg)
    assert np.array_equal(dB.sum(axis=0), (Gi * (arg >= 0)).sum(axis=0))


# ---- the flag ------------------------------------------------------------------------------------------------------------
def test_flag_default_and_choices():
    from stochastic_gcn_amd.full_batch import check_aggregator
    f = _Flags()
    assert f.aggregator == 'sum' and 'aggregator' in f.as_dict()
    assert check_aggregator(f) is False
    f.parse(['--full_batch', '--test_full_batch', '--aggregator', 'max'])
    assert f.aggregator == 'max' and check_aggregator(f) is True
    assert _Flags().parse(['--aggregator', 'sum']).aggregator == 'sum'
    with pytest.raises(SystemExit):
        _Flags().parse(['--aggregator', 'mean'])
    FLAGS.update(aggregator='mean')
    with pytest.raises(ValueError, match="--aggregator must be one of sum/max"):
        check_aggregator()
    FLAGS.update(aggregator='sum', full_batch_dtype='bf16', edge_dropout=0.3)           # sum: nothing to refuse
    assert check_aggregator() is False
    help_ = {name: h for name, _, _, h in _DEFS}['aggregator']
    assert '--preprocess' in help_ and 'weighted sum' in help_


BOTH = dict(full_batch=True, test_full_batch=True, aggregator='max')
REFUSALS = [
    (dict(aggregator='max'), "--aggregator max needs --full_batch and --test_full_batch"),
    (dict(aggregator='max', full_batch=True), "--aggregator max needs --full_batch and --test_full_batch"),
    (dict(aggregator='max', test_full_batch=True), "--aggregator max needs --full_batch and --test_full_batch"),
    (dict(BOTH, full_batch_dtype='bf16'), "--aggregator max is not supported with --full_batch_dtype bf16"),
    (dict(BOTH, dense_dtype='bf16', feature_dtype='bf16'), "--aggregator max is not supported with --feature_dtype bf16"),
    (dict(BOTH, edge_dropout=0.2), "--aggregator max is not supported with --edge_dropout"),
]


@pytest.mark.parametrize("flags,msg", REFUSALS)
def test_refusals(flags, msg):
    from stochastic_gcn_amd.full_batch import check_aggregator
    FLAGS.update(**flags)
    with pytest.raises(ValueError, match=msg):
        check_aggregator()


@pytest.mark.parametrize("flags,msg", REFUSALS + [
    (dict(BOTH, cv=True), "--full_batch is not supported with --cv"),                   # the refusals --full_batch makes stay
    (dict(BOTH, det_dropout=True), "--full_batch is not supported with --det_dropout"),
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


def test_accepted_combination_reaches_the_device_check(monkeypatch):
    from stochastic_gcn_amd import train
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    FLAGS.update(**BOTH)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        train.Trainer(verbose=False)


def test_model_matrix_builds_no_sweep_plan_under_max(monkeypatch):
    """A model whose aggregations are all maxima reads the row CSR only: 'rows' whatever --full_batch_kernel says."""
    from stochastic_gcn_amd import full_batch

    class Model(object):
        L, agg0_dim = 2, 64
    a = sc.pattern("m64_k64")
    FLAGS.update(**BOTH, full_batch_kernel='cs')
    m = full_batch.model_matrix(a, torch.device("cpu"), Model(), products=1000)
    assert m.kernel == 'rows' and m._plan is None
    FLAGS.update(aggregator='sum', full_batch_kernel='rows')
    assert full_batch.model_matrix(a, torch.device("cpu"), Model(), products=1000).kernel == 'rows'


# ---- the end-to-end cases of tests/test_max_aggregator_gpu.py are well-posed (decided here, without a device) ------------------
@pytest.mark.parametrize("name", ["sage_ln_pp", "gcn_nopp"])
def test_end_to_end_cases_are_well_posed(name):
    import max_aggregator_cases as mx
    c = mx.CASES[name]
    m = mx.margin(name, c['init'])
    print("%s: init %d, smallest non-zero gap or |ReLU input| / largest input %.3e (needs >= %.0e)" % (name, c['init'], m, mx.MARGIN))
    assert m >= mx.MARGIN
    assert c['init'] in mx.SEEDS and c['n'] <= 500 and c['flags']['hidden1'] == 8


def test_top_two_gap_by_hand():
    from max_aggregator_ref import top_two_gap
    a = sp.csr_matrix(np.array([[1, 1, 1, 0], [0, 1, 0, 0], [0, 0, 0, 0], [1, 0, 0, 1]], np.float32))
    B = np.array([[1.0, 5.0], [3.0, 5.0], [2.5, -1.0], [1.0, 4.0]], np.float32)
    # row 0: column 0 has 3 over 2.5 (gap 0.5), column 1 a tie (gap 0: not counted); row 3: a tie, and 5 over 4 (gap 1)
    assert top_two_gap(a, B) == 0.5
    assert top_two_gap(sp.identity(4, format='csr', dtype=np.float32), B) == np.inf


# ---- the exports ---------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "sgcn.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, nargs in (("sgcn_spmax_csr_f32", 14), ("sgcn_spmax_csr_bwd_f32", 16)):
        assert "int %s(" % name in src
        assert hasattr(lib, name) and name in _ffi.SIGNATURES
        assert len(_ffi.SIGNATURES[name][1]) == nargs
    assert "NaN-free" in src
    assert _ffi.lib.sgcn_abi_version() == _ffi.ABI_VERSION == 16          # additive exports


def _plan(nfix, nslots, ws, ws_elems, seg=4096, nseg=8, fix=8192):
    return _ffi.Plan(seg, nseg, fix if nfix else None, nfix, nslots, ws, ws_elems)


def test_forward_validates_before_any_device_call():
    lib, A = _ffi.lib, 4096          # (non-null addresses that are never dereferenced: every call fails validation first)
    err = lib.sgcn_last_error

    def fwd(rowptr=A, col=2 * A, M=8, K=8, d=8, B=3 * A, ldb=8, C=4 * A, ldc=8, arg=5 * A, ldarg=8, plan=None, ids=None):
        return lib.sgcn_spmax_csr_f32(rowptr, col, M, K, d, B, ldb, C, ldc, arg, ldarg, plan, ids, None)
    for kw in (dict(rowptr=None), dict(B=None), dict(C=None)):
        assert fwd(**kw) == -1 and b"null operand" in err()
    for d in (0, -3):
        assert fwd(d=d) == -1 and b"d must be positive" in err()
    for kw in (dict(ldb=7), dict(ldc=7), dict(ldarg=7)):
        assert fwd(**kw) == -1 and b"leading dimension smaller than d" in err()
    assert fwd(M=-1) == -1 and b"negative size" in err()
    p = _plan(2, 6, 6 * A, 6 * 8)
    assert fwd(plan=ctypes.byref(p), ids=None) == -1 and b"needs dev_ws_arg" in err()               # split rows, no id slots
    p = _plan(2, 6, None, 0)
    assert fwd(plan=ctypes.byref(p), ids=7 * A) == -1 and b"needs dev_fix/dev_ws" in err()
    p = _plan(2, 6, 6 * A, 6 * 8 - 1)
    assert fwd(plan=ctypes.byref(p), ids=7 * A) == -1 and b"workspace too small" in err()
    p = _plan(2, 6, 6 * A, 6 * 8)
    assert fwd(d=9, ldb=9, ldc=9, ldarg=9, plan=ctypes.byref(p), ids=7 * A) == -1 and b"workspace too small" in err()   # ldw = 12
    p = _plan(0, 0, None, 0, nseg=7)
    assert fwd(plan=ctypes.byref(p)) == -1 and b"malformed plan" in err()
    assert fwd(M=0, rowptr=A) == 0                                                                   # no rows: nothing to do


def test_backward_validates_before_any_device_call():
    lib, A = _ffi.lib, 4096
    err = lib.sgcn_last_error

    def bwd(rowptr=A, row=2 * A, K=8, M=8, d=8, G=3 * A, ldg=8, arg=4 * A, ldarg=8, dB=5 * A, lddb=8, add=None, ldadd=0,
            add_rows=0, plan=None):
        return lib.sgcn_spmax_csr_bwd_f32(rowptr, row, K, M, d, G, ldg, arg, ldarg, dB, lddb, add, ldadd, add_rows, plan, None)
    for kw in (dict(rowptr=None), dict(G=None), dict(arg=None), dict(dB=None)):
        assert bwd(**kw) == -1 and b"null operand" in err()
    for d in (0, -1):
        assert bwd(d=d) == -1 and b"d must be positive" in err()
    for kw in (dict(ldg=7), dict(ldarg=7), dict(lddb=7)):
        assert bwd(**kw) == -1 and b"leading dimension smaller than d" in err()
    assert bwd(add=6 * A, ldadd=7, add_rows=4) == -1 and b"bad addend" in err()
    assert bwd(add=6 * A, ldadd=8, add_rows=9) == -1 and b"bad addend" in err()
    p = _plan(1, 3, None, 0)
    assert bwd(plan=ctypes.byref(p)) == -1 and b"needs dev_fix/dev_ws" in err()
    p = _plan(1, 3, 6 * A, 3 * 8 - 1)
    assert bwd(plan=ctypes.byref(p)) == -1 and b"workspace too small" in err()
    assert bwd(K=0) == 0


def test_ops_refuse_cpu_tensors_and_duplicate_columns():
    a = sp.identity(4, format='csr', dtype=np.float32)
    A = ops.DeviceCSR.from_scipy(a, torch.device("cpu"), with_plan=False)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.spmax(A, torch.zeros(4, 8))
    with pytest.raises(RuntimeError, match="HBM"):
        ops.spmax_bwd(A, torch.zeros(4, 8), torch.zeros(4, 8, dtype=torch.int32))
    # a row that stores column 2 twice (scipy keeps duplicates until asked to sum them), sorted and unsorted
    for cols in ([0, 2, 2, 3, 1], [2, 0, 2, 3, 1]):
        dup = ops.DeviceCSR.from_arrays((2, 4), [0, 3, 5], cols, np.ones(5, np.float32), torch.device("cpu"), with_plan=False)
        with pytest.raises(ValueError, match="unique column ids"):
            ops.spmax(dup, torch.zeros(4, 8))
    # the same ids in different rows, and rows stored in descending order, are fine: the tensor check is what refuses
    ok = ops.DeviceCSR.from_arrays((2, 4), [0, 3, 5], [3, 2, 0, 2, 0], np.ones(5, np.float32), torch.device("cpu"), with_plan=False)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.spmax(ok, torch.zeros(4, 8))
    assert ok._unique_cols                                   # checked once per matrix
