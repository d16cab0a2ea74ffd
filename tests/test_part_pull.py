"""CPU tests of --full_batch_part_pull (part steps of the sum AND the attention aggregator that read stored rows for their
out-of-part neighbours): the flag, its refusals before a device is touched, the fp64 reference of the two-table attention
(tests/part_pull_attn_ref.py) against an entry-by-entry evaluation and three mutants, and the argument checks of the four
exports through the raw C-ABI.  Nothing here touches a device."""
import os

import numpy as np
import pytest
import torch

import induce_ref as ir
import part_history_ref as pr
import part_pull_attn_ref as ar
from stochastic_gcn_amd import _ffi
from stochastic_gcn_amd.flags import _DEFS, FLAGS, _Flags

FWD = ("sgcn_spattn_pull_f32", "sgcn_spattn_pull_h16")
BWD = ("sgcn_spattn_pull_bwd_q_f32", "sgcn_spattn_pull_bwd_q_h16")
ON = dict(full_batch=True, test_full_batch=True, full_batch_parts=4, full_batch_part_pull=True)
ATTN = dict(ON, aggregator='attn')


@pytest.fixture(autouse=True)
def _reset_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


# ---- the flag -----------------------------------------------------------------------------------------------------------
def test_flag_defaults_and_parsing():
    from stochastic_gcn_amd.full_batch import check_part_history, check_part_pull
    f = _Flags()
    assert f.full_batch_part_pull is False and 'full_batch_part_pull' in f.as_dict()
    name, typ, default, text = next(d[:4] for d in _DEFS if d[0] == 'full_batch_part_pull')
    assert (typ, default) == (bool, False)
    for word in ('--aggregator sum', '--full_batch_part_history exactly', '--aggregator attn', 'EVERY stored neighbour',
                 '--history_dtype bf16', '--full_batch_parts > 0', '--aggregator max', '--attn_score gat', '--attn_dropout',
                 '--reverse', '--full_batch_dtype bf16'):
        assert word in text, word
    assert check_part_pull(f) == (False, False)                    # off: nothing else is looked at
    argv = ['--full_batch', '--test_full_batch', '--full_batch_parts', '8', '--full_batch_part_pull']
    f.parse(argv)
    assert check_part_pull(f) == (True, False) and check_part_history(f) == (False, False)
    f.parse(argv + ['--aggregator', 'attn', '--attn_heads', '4'])
    assert check_part_pull(f) == (True, False)
    f.parse(argv + ['--aggregator', 'attn', '--history_dtype', 'bf16'])
    assert check_part_pull(f) == (True, True)
    f.parse(argv + ['--history_dtype', 'bf16', '--nofull_batch_part_pull'])
    assert check_part_pull(f) == (False, False)
    # both flags with the sum aggregator are allowed; what it does not interfere with
    FLAGS.update(full_batch_parts_per_step=4, full_batch_part_norm='keep', dense_dtype='bf16', full_batch_part_history=True, **ON)
    assert check_part_pull() == (True, False) and check_part_history() == (True, False)
    FLAGS.reset()
    FLAGS.update(attn_heads=2, attn_scale=0.5, **ATTN)
    assert check_part_pull() == (True, False)


REFUSALS = [
    (dict(full_batch_part_pull=True), "--full_batch_part_pull needs --full_batch_parts > 0"),
    (dict(full_batch=True, full_batch_part_pull=True), "--full_batch_part_pull needs --full_batch_parts > 0"),
    (dict(ON, aggregator='max'), "--full_batch_part_pull is not supported with --aggregator max.*a two-table maximum is a follow-up"),
    (dict(ATTN, attn_score='gat'), "--full_batch_part_pull is not supported with --attn_score gat.*stale scores"),
    (dict(ATTN, attn_dropout=0.1), "--full_batch_part_pull is not supported with --attn_dropout > 0.*mask of out-of-part "
                                   "entries is not defined"),
    (dict(ON, reverse=True), "--full_batch_part_pull is not supported with --reverse"),
    (dict(ATTN, reverse=True), "--full_batch_part_pull is not supported with --reverse"),
    (dict(ON, full_batch_dtype='bf16'), "--full_batch_part_pull is not supported with --full_batch_dtype bf16"),
]


@pytest.mark.parametrize("flags,msg", REFUSALS)
def test_refusals(flags, msg):
    from stochastic_gcn_amd.full_batch import check_part_pull
    FLAGS.update(**flags)
    with pytest.raises(ValueError, match=msg):
        check_part_pull()


@pytest.mark.parametrize("flags,msg", REFUSALS[1:])
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


def test_the_old_flag_speaks_first_and_keeps_its_words(monkeypatch):
    """both flags on: check_part_history refuses attention with its own message, in the trainer too"""
    from stochastic_gcn_amd import train
    from stochastic_gcn_amd.full_batch import check_part_history
    FLAGS.update(full_batch_part_history=True, **ATTN)
    with pytest.raises(ValueError, match="--full_batch_part_history is not supported with --aggregator attn: the maximum and "
                                         "the attention kernels gather from one table; a two-table form is a follow-up"):
        check_part_history()
    touched = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: touched.append("is_available") or False)
    monkeypatch.setattr(train, "load_data", lambda *a, **k: touched.append("load_data"))
    with pytest.raises(ValueError, match="--full_batch_part_history is not supported with --aggregator attn"):
        train.Trainer(verbose=False)
    assert touched == []


def test_an_accepted_configuration_reaches_the_device_check(monkeypatch):
    """--aggregator attn under the new flag passes every flag check: the trainer stops at the missing device, not before"""
    from stochastic_gcn_amd import train
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(train, "load_data", lambda *a, **k: pytest.fail("data loaded without a device"))
    FLAGS.update(attn_heads=2, **ATTN)
    with pytest.raises(RuntimeError, match="training needs an MI355X"):
        train.Trainer(verbose=False)


# ---- the reference ------------------------------------------------------------------------------------------------------
def _tiny():
    a = ir.signed(ir.flat_graph(40, 4, seed=2), seed=1)
    a.sort_indices()
    return a


@pytest.mark.parametrize("heads,d", [(1, 3), (2, 4)])
def test_reference_is_the_entrywise_evaluation_and_rejects_the_mutants(heads, d):
    a = _tiny()
    N = a.shape[0]
    rng = np.random.RandomState(3)
    H = rng.randn(N, d)
    subsets = {'all': np.arange(N), 'one': np.array([N // 3]), 'every_other': np.arange(0, N, 2),
               'third': np.sort(rng.choice(N, N // 3, replace=False))}
    scale = 0.7
    for sname, ids in subsets.items():
        n = len(ids)
        X, G, add = rng.randn(n, d), rng.randn(n, d), rng.randn(n, d)
        f = ar.forward(a, ids, X, H, scale, heads)
        b = ar.backward(a, ids, X, H, G, scale, heads)
        C, lse, dQ, dX = ar.loops(a, ids, X, H, G, scale, heads)
        errs = [float(np.abs(x - y).max()) for x, y in ((f.C, C), (f.lse, lse), (b['dQ'], dQ), (b['dX'], dX))]
        print("%s / heads %d: |reference - entry-wise|  C %.2e  lse %.2e  dQ %.2e  dX %.2e" % ((sname, heads) + tuple(errs)))
        assert f.C.shape == (n, d) and f.lse.shape == (n, heads) and max(errs) <= 1e-12
        with_add = ar.backward(a, ids, X, H, G, scale, heads, add=add, add_rows=n)
        assert np.allclose(with_add['dX'], dX + add, rtol=0, atol=1e-12)
        rows, col, _ = pr._entries(a, ids)
        inside = pr.position_map(N, ids)[col] >= 0
        # a cut row: one with entries on both sides; a mutant must differ exactly where its kind of entry exists
        differs = dict(softmax_in_part=bool((~inside).any()), stale_in_part=bool(inside.any()),
                       dq_in_part=bool((~inside).any()))
        for mname in ar.MUTANTS:
            mC, mlse, mdQ, mdX = ar.loops(a, ids, X, H, G, scale, heads, mutant=mname)
            off = max(float(np.abs(mC - C).max()), float(np.abs(mdX - dX).max()))
            print("    mutant %s: off by %.3e (%s)" % (mname, off, "must differ" if differs[mname] else "no such entry"))
            assert (off > 1e-3) == differs[mname]
            if mname == 'dq_in_part':
                assert np.array_equal(mC, C) and np.array_equal(mlse, lse)           # its forward is right
    assert not (pr.position_map(N, subsets['all']) < 0).any()


def test_reference_backward_is_the_derivative_of_its_forward():
    """d(sum(G . C)) / dX by central differences of the fp64 forward: queries over every entry, keys / values in-part only"""
    a = _tiny()
    rng = np.random.RandomState(0)
    ids = np.sort(rng.choice(40, 17, replace=False))
    d, heads, scale = 4, 2, 0.5
    X, H, G = rng.randn(17, d), rng.randn(40, d), rng.randn(17, d)
    want = ar.backward(a, ids, X, H, G, scale, heads)['dX']
    got = np.zeros_like(X)
    for i in range(17):
        for k in range(d):
            e = np.zeros_like(X)
            e[i, k] = 1e-5
            got[i, k] = ((ar.forward(a, ids, X + e, H, scale, heads).C - ar.forward(a, ids, X - e, H, scale, heads).C) * G).sum() / 2e-5
    err = float(np.abs(got - want).max())
    print("central differences against the reference's dX: %.3e" % err)
    assert err <= 1e-8 * max(1.0, float(np.abs(want).max()))


def test_model_reference_steps_and_pushes():
    """the fp64 model: a step pushes its aggregation inputs, the refresh stops at the last aggregation, heads change numbers"""
    import attn_aggregator_cases as ax
    from oracle import model_np as mnp
    case = ax.build('sage_ln_pp')
    a = case['train_adj'].tocsr().copy()
    a.sort_indices()
    case['train_adj'] = a
    ids = np.arange(0, case['n'], 2)
    rows = np.flatnonzero(np.isin(ids, case['train'])).astype(np.int32)
    out = {}
    for heads in (1, 2):
        om = ar.make_model(case, heads=heads, seed=3)
        logits, acts, loss, grads = om.step(ids, rows, case['labels'], 0.2, mnp.HashMasks(1, 0, 0.8))
        assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads.values())
        for l, t in enumerate(om.tables):
            if t is not None:
                assert np.array_equal(t[ids], om.pushed[l]) and not t[np.setdiff1d(np.arange(case['n']), ids)].any()
        out[heads] = logits
    assert np.abs(out[1] - out[2]).max() > 1e-6


# ---- the exports --------------------------------------------------------------------------------------------------------
def test_exports_are_declared_and_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sgcn.h")).read()
    for names, nargs in ((FWD, 17), (BWD, 25)):
        for s in names:
            assert s in _ffi.SIGNATURES and hasattr(_ffi.lib, s) and (s + "(") in header
            assert len(_ffi.SIGNATURES[s][1]) == nargs
    assert _ffi.lib.sgcn_abi_version() == 16 == _ffi.ABI_VERSION          # additive exports: the ABI version stays


def _err():
    return _ffi.lib.sgcn_last_error() or b""


P_ = 4096                                  # a 16-byte aligned address nobody reads


def _caller(name):
    fn = getattr(_ffi.lib, name)
    if name in FWD:
        def call(rowptr=P_, col=P_, ids=P_, n=3, N=10, map_=P_, d=4, heads=1, X=P_, ldx=8, H=P_, ldh=8, scale=1.0, C=P_, ldc=8,
                 lse=P_):
            return fn(rowptr, col, ids, n, N, map_, d, heads, X, ldx, H, ldh, scale, C, ldc, lse, None)
        return call, ('ldx', 'ldh', 'ldc'), ('rowptr', 'col', 'ids', 'map_', 'X', 'H', 'C')

    def call(rowptr=P_, col=P_, ids=P_, n=3, N=10, map_=P_, d=4, heads=1, X=P_, ldx=8, H=P_, ldh=8, scale=1.0, G=P_, ldg=8,
             C=P_, ldc=8, lse=P_, delta=P_, dQ=P_, lddq=8, add=None, ldadd=0, add_rows=0):
        return fn(rowptr, col, ids, n, N, map_, d, heads, X, ldx, H, ldh, scale, G, ldg, C, ldc, lse, delta, dQ, lddq, add, ldadd,
                  add_rows, None)
    return call, ('ldx', 'ldh', 'ldg', 'ldc', 'lddq'), ('rowptr', 'col', 'ids', 'map_', 'X', 'H', 'G', 'C', 'lse', 'delta', 'dQ')


@pytest.mark.parametrize("name", FWD + BWD)
def test_argument_checks(name):
    """every refusal comes before any HIP call: the addresses are never dereferenced"""
    call, pitches, operands = _caller(name)
    assert call(n=-1) == -1 and b"negative size" in _err()
    assert call(n=0, N=-1) == -1 and b"negative size" in _err()
    assert call(n=11) == -1 and b"11 rows cannot be unique in [0, 10)" in _err()
    for d in (0, -4):
        assert call(d=d) == -1 and b"d must be positive" in _err()
    h16 = name.endswith("_h16")

    def at(v):                                # every pitch at v (a bfloat16 table's stays a multiple of 8)
        return {p: ((v + 7) // 8 * 8 if h16 and p == 'ldh' else v) for p in pitches}
    for heads in (0, 3, 16):
        assert call(heads=heads, d=48, **at(48)) == -1 and b"heads must be one of 1/2/4/8" in _err()
    assert call(heads=4, d=6) == -1 and b"is not a multiple of heads" in _err()
    for pitch in pitches:
        assert call(**{pitch: 3}) == -1 and b"leading dimension smaller than d" in _err()
    for operand in operands:
        assert call(**{operand: None}) == -1 and b"null operand" in _err(), operand
    for scale in (float('nan'), float('inf'), -float('inf')):
        assert call(scale=scale) == -1 and b"scale must be finite" in _err()
    # the width limit d <= 256 * VW: 1032 columns at VW = 4; 520 on an odd pitch (VW = 1); heads whose width VW must divide
    assert call(d=1032, **at(1032)) == -1 and b"is over the limit of 1024 columns at vector width 4" in _err()
    assert call(d=520, heads=8, **at(521)) == -1 and b"is over the limit of 256 columns at vector width 1" in _err()
    assert call(d=520, heads=8, **at(520)) == -1 and b"vector width 1" in _err()                # 65 per head: VW = 1
    if name in BWD:
        assert call(add=P_, ldadd=3, add_rows=2) == -1 and b"bad addend" in _err()
        assert call(add=P_, ldadd=8, add_rows=4) == -1 and b"bad addend" in _err()
    if name.endswith("_h16"):
        assert call(ldh=12, d=4) == -1 and b"ldh % 8 == 0" in _err()
        assert call(H=P_ + 8) == -1 and b"16-byte aligned" in _err()
    # n == 0: no launch, whatever the pointers
    zero = dict(rowptr=None, col=None, ids=None, n=0, map_=None, X=None, H=None, C=None)
    assert call(**zero) == 0
    assert call(N=0, **zero) == 0
