"""CPU tests of --full_batch_part_history (part steps that read stored rows for their out-of-part neighbours): the flag, its
refusals before a device is touched, the fp64 reference of the two-table product (tests/part_history_ref.py) against a dense
evaluation and against two mutants, and the argument checks of the two exports through the raw C-ABI.  Nothing here touches
a device."""
import os

import numpy as np
import pytest
import torch

import induce_ref as ir
import part_history_ref as pr
from stochastic_gcn_amd import _ffi
from stochastic_gcn_amd.flags import _DEFS, FLAGS, _Flags

NEW = ("sgcn_spmm_pull_f32", "sgcn_spmm_pull_h16")
ON = dict(full_batch=True, full_batch_parts=4, full_batch_part_history=True)


@pytest.fixture(autouse=True)
def _reset_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


# ---- the flag -----------------------------------------------------------------------------------------------------------
def test_flag_defaults_and_parsing():
    from stochastic_gcn_amd.full_batch import check_part_history
    f = _Flags()
    assert f.full_batch_part_history is False and 'full_batch_part_history' in f.as_dict()
    name, typ, default, text = next(d[:4] for d in _DEFS if d[0] == 'full_batch_part_history')
    assert (typ, default) == (bool, False)
    for word in ('GNNAutoScale', '--history_dtype', '--aggregator max / attn', '--reverse', '--full_batch_dtype bf16',
                 '--full_batch_parts > 0'):
        assert word in text, word                                  # the estimator, the refusals, the role of --history_dtype
    assert check_part_history(f) == (False, False)                 # off: nothing else is looked at
    argv = ['--full_batch', '--full_batch_parts', '8', '--full_batch_part_history']
    f.parse(argv)
    assert check_part_history(f) == (True, False)
    f.parse(argv + ['--history_dtype', 'bf16'])
    assert check_part_history(f) == (True, True)
    f.parse(argv + ['--history_dtype', 'bf16', '--nofull_batch_part_history'])
    assert check_part_history(f) == (False, False)
    # what it does not interfere with
    FLAGS.update(full_batch_parts_per_step=4, full_batch_part_norm='keep', test_full_batch=True, dense_dtype='bf16', **ON)
    assert check_part_history() == (True, False)


@pytest.mark.parametrize("flags,msg", [
    (dict(full_batch_part_history=True), r"--full_batch_part_history needs --full_batch_parts > 0"),
    (dict(full_batch=True, full_batch_part_history=True), r"--full_batch_part_history needs --full_batch_parts > 0"),
    (dict(ON, aggregator='max', test_full_batch=True), r"--full_batch_part_history is not supported with --aggregator max"),
    (dict(ON, aggregator='attn', test_full_batch=True), r"--full_batch_part_history is not supported with --aggregator attn"),
    (dict(ON, reverse=True), r"--full_batch_part_history is not supported with --reverse"),
    (dict(ON, full_batch_dtype='bf16'), r"--full_batch_part_history is not supported with --full_batch_dtype bf16"),
])
def test_refusals(flags, msg):
    from stochastic_gcn_amd.full_batch import check_part_history
    FLAGS.update(**flags)
    with pytest.raises(ValueError, match=msg):
        check_part_history()


@pytest.mark.parametrize("flags,msg", [
    (dict(full_batch=True, full_batch_part_history=True), "--full_batch_part_history needs --full_batch_parts > 0"),
    (dict(ON, aggregator='max', test_full_batch=True), "--full_batch_part_history is not supported with --aggregator max"),
    (dict(ON, reverse=True), "--full_batch_part_history is not supported with --reverse"),
    (dict(ON, full_batch_dtype='bf16'), "--full_batch_part_history is not supported with --full_batch_dtype bf16"),
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


def test_check_full_batch_parts_keeps_its_answers():
    from stochastic_gcn_amd.full_batch import check_full_batch_parts
    assert check_full_batch_parts(_Flags()) == (0, 1, 'rows')
    for norm in ('rows', 'keep'):
        FLAGS.reset()
        FLAGS.update(full_batch_part_norm=norm, full_batch_parts_per_step=2, **ON)
        assert check_full_batch_parts() == (4, 2, norm)                       # the history flag changes nothing here
        assert check_full_batch_parts(num_vertices=4) == (4, 2, norm)
    FLAGS.reset()
    FLAGS.update(full_batch_part_history=True, full_batch_parts=4)
    with pytest.raises(ValueError, match="--full_batch_parts needs --full_batch: its steps are exact steps"):
        check_full_batch_parts()


# ---- the reference ------------------------------------------------------------------------------------------------------
def _subsets(N, rng):
    return {'all': np.arange(N), 'one': np.array([N // 3]), 'every_other': np.arange(0, N, 2),
            'third': np.sort(rng.choice(N, max(N // 3, 1), replace=False))}


@pytest.mark.parametrize("graph", ['sbm', 'flat'])
@pytest.mark.parametrize("d", [1, 5])
def test_reference_is_the_dense_evaluation_and_rejects_the_mutants(graph, d):
    a = ir.signed({'sbm': ir.sbm_graph, 'flat': ir.flat_graph}[graph](), seed=5)
    N = a.shape[0]
    rng = np.random.RandomState(3)
    H = rng.randn(N, d)
    for sname, ids in _subsets(N, np.random.RandomState(2)).items():
        X = rng.randn(len(ids), d)
        got, want = pr.pull(a, ids, X, H), pr.pull_dense(a, ids, X, H)
        scale = max(float(pr.pull_magnitude(a, ids, X, H).max()), 1.0)
        err = float(np.abs(got - want).max())
        print("%s / %s / d=%d: |entry-wise - dense| = %.3e (magnitude %.3e)" % (graph, sname, d, err, scale))
        assert got.shape == (len(ids), d) and err <= 1e-12 * scale
        rows, col, _ = pr._entries(a, ids)
        inside = pr.position_map(N, ids)[col] >= 0
        for mname, mutant in pr.MUTANTS.items():
            wrong = float(np.abs(mutant(a, ids, X, H) - want).max())
            differs = bool(inside.any()) if mname == 'stale_in_part' else bool((~inside).any())
            print("    mutant %s: off by %.3e (%s)" % (mname, wrong, "must differ" if differs else "no such entry"))
            assert (wrong > 1e-3 * scale) == differs
    # no out-of-part entry under S = everything, none in-part off the diagonal under S = one vertex
    assert np.array_equal(pr.position_map(5, [1, 3]), [-1, 0, -1, 1, -1])


def test_reference_backward_is_the_block_only():
    """d(sum(G . pull)) / dX = A[S, S]^T G by central differences of the fp64 forward: stored rows carry no gradient"""
    a = ir.signed(ir.flat_graph(60, 4, seed=2), seed=1)
    rng = np.random.RandomState(0)
    ids = np.sort(rng.choice(60, 25, replace=False))
    X, H, G = rng.randn(25, 3), rng.randn(60, 3), rng.randn(25, 3)
    want = pr.block(a, ids).T.astype(np.float64) @ G
    got = np.zeros_like(X)
    for i in range(25):
        for k in range(3):
            e = np.zeros_like(X)
            e[i, k] = 1e-3
            got[i, k] = ((pr.pull(a, ids, X + e, H) - pr.pull(a, ids, X - e, H)) * G).sum() / 2e-3
    assert np.allclose(got, want, rtol=1e-8, atol=1e-8)


def test_bf16_round_and_widen():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.1415927, 0.0, 65504.0], dtype=np.float32)
    t = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(pr.round_bf16(x), t)
    assert np.array_equal(pr.widen_bf16(t), torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy())


# ---- the exports --------------------------------------------------------------------------------------------------------
def test_exports_are_declared_and_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sgcn.h")).read()
    for s in NEW:
        assert s in _ffi.SIGNATURES and hasattr(_ffi.lib, s) and (s + "(") in header
        assert len(_ffi.SIGNATURES[s][1]) == 15
    assert _ffi.lib.sgcn_abi_version() == 16 == _ffi.ABI_VERSION          # additive exports: the ABI version stays


def _err():
    return _ffi.lib.sgcn_last_error() or b""


@pytest.mark.parametrize("name", NEW)
def test_argument_checks(name):
    """every refusal comes before any HIP call: the addresses are never dereferenced"""
    fn = getattr(_ffi.lib, name)
    p = 4096                                  # a 16-byte aligned address nobody reads

    def call(rowptr=p, col=p, val=p, ids=p, n=3, N=10, map_=p, d=4, X=p, ldx=8, H=p, ldh=8, C=p, ldc=8):
        return fn(rowptr, col, val, ids, n, N, map_, d, X, ldx, H, ldh, C, ldc, None)
    assert call(n=-1) == -1 and b"negative size" in _err()
    assert call(n=0, N=-1) == -1 and b"negative size" in _err()
    assert call(n=11) == -1 and b"11 rows cannot be unique in [0, 10)" in _err()
    for d in (0, -4):
        assert call(d=d) == -1 and b"d must be positive" in _err()
    for pitch in ('ldx', 'ldh', 'ldc'):
        assert call(**{pitch: 3}) == -1 and b"leading dimension smaller than d" in _err()
    for operand in ('rowptr', 'col', 'val', 'ids', 'map_', 'X', 'H', 'C'):
        assert call(**{operand: None}) == -1 and b"null operand" in _err(), operand
    assert fn(None, None, None, None, 0, 10, None, 4, None, 8, None, 8, None, 8, None) == 0        # n == 0: no launch
    assert fn(None, None, None, None, 0, 0, None, 1, None, 1, None, 8, None, 1, None) == 0
    if name.endswith("_h16"):
        assert call(ldh=12, d=4) == -1 and b"ldh % 8 == 0" in _err()
        assert call(H=p + 8) == -1 and b"16-byte aligned" in _err()


def test_ops_checks_on_the_host():
    from stochastic_gcn_amd import ops
    import scipy.sparse as sp
    a = sp.identity(4, format='csr', dtype=np.float32)
    cpu = torch.device("cpu")
    A = ops.DeviceCSR.from_scipy(a, cpu, with_plan=False)
    ids, vmap = torch.arange(2, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="must live in HBM"):
        ops.spmm_pull(A, ids, vmap, torch.zeros(2, 3), torch.zeros(4, 3))
    R = ops.DeviceCSR.from_scipy(sp.csr_matrix(np.ones((2, 4), np.float32)), cpu, with_plan=False)
    with pytest.raises(ValueError, match="square"):
        ops.spmm_pull(R, ids, vmap, torch.zeros(2, 3), torch.zeros(4, 3))


def test_pulled_matrix_needs_the_map():
    from stochastic_gcn_amd.full_batch import PulledMatrix

    class Block(object):
        transpose = object()
    with pytest.raises(ValueError, match="position map"):
        PulledMatrix(Block(), None, None, [], [])
