"""CPU tests of --full_batch_part_pull_max (part steps of the maximum aggregator that read stored rows for their out-of-part
neighbours): the flag, its help words and its refusals before a device is touched; that the three older part-flag checks
still speak as before; the exact reference of the two-table maximum (tests/part_pull_max_ref.py) against the entry-by-entry
definition, a dense evaluation and three mutants; the argument checks of the two exports through the raw C-ABI; and the
launches an aggregation layer makes over a PulledMatrix with the switch on and off (the recorders of
tests/test_aggregator_wiring.py).  Nothing here touches a device."""
import inspect
import os
import types

import numpy as np
import pytest
import torch

import induce_ref as ir
import part_history_ref as pr
import part_pull_max_ref as xr
import spmax_ref
import test_aggregator_wiring as w
from stochastic_gcn_amd import _ffi, full_batch, ops
from stochastic_gcn_amd.flags import _DEFS, FLAGS, _Flags

EXPORTS = ("sgcn_spmax_pull_f32", "sgcn_spmax_pull_h16")
ON = dict(full_batch=True, test_full_batch=True, full_batch_parts=4, full_batch_part_pull_max=True)
MAX = dict(ON, aggregator='max')
SPMAX_PULL = inspect.signature(ops.spmax_pull)           # (the real wrapper's: taken before any test replaces it)


@pytest.fixture(autouse=True)
def _reset_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


# ---- the flag -----------------------------------------------------------------------------------------------------------
def test_flag_defaults_and_parsing():
    from stochastic_gcn_amd.full_batch import check_part_history, check_part_pull, check_part_pull_gat, check_part_pull_max
    f = _Flags()
    assert f.full_batch_part_pull_max is False and 'full_batch_part_pull_max' in f.as_dict()
    name, typ, default, text = next(d[:4] for d in _DEFS if d[0] == 'full_batch_part_pull_max')
    assert (typ, default) == (bool, False)
    for word in ('--aggregator max', 'element-wise maximum', 'EVERY stored neighbour', 'first maximum', 'whichever table',
                 'gradient of an element goes to its winner', 'constant of the step', 'stale row sends nothing',
                 'without a training vertex runs the forward only', '--history_dtype bf16 halves the tables',
                 '--full_batch_parts > 0', '--reverse', '--full_batch_dtype bf16', '--full_batch_part_history',
                 '--full_batch_part_pull or', '--full_batch_part_pull_gat'):
        assert word in text, word
    assert check_part_pull_max(f) == (False, False)                # off: nothing else is looked at
    argv = ['--full_batch', '--test_full_batch', '--full_batch_parts', '8', '--full_batch_part_pull_max', '--aggregator', 'max']
    f.parse(argv)
    assert check_part_pull_max(f) == (True, False)
    assert check_part_history(f) == check_part_pull(f) == check_part_pull_gat(f) == (False, False)
    f.parse(argv + ['--history_dtype', 'bf16'])
    assert check_part_pull_max(f) == (True, True)
    f.parse(argv + ['--history_dtype', 'bf16', '--nofull_batch_part_pull_max'])
    assert check_part_pull_max(f) == (False, False)
    # what it does not interfere with
    FLAGS.update(full_batch_parts_per_step=4, full_batch_part_norm='keep', dense_dtype='bf16', **MAX)
    assert check_part_pull_max() == (True, False)


TOGETHER = "--full_batch_part_pull_max is not supported together with --%s: not together with"
REFUSALS = [
    (dict(full_batch_part_pull_max=True), "--full_batch_part_pull_max needs --full_batch_parts > 0"),
    (dict(full_batch=True, full_batch_part_pull_max=True, aggregator='max'), "--full_batch_part_pull_max needs --full_batch_parts > 0"),
    (dict(ON), r"--full_batch_part_pull_max needs --aggregator max \(got sum\)"),
    (dict(ON, aggregator='attn'), r"--full_batch_part_pull_max needs --aggregator max \(got attn\)"),
    (dict(MAX, reverse=True), "--full_batch_part_pull_max is not supported with --reverse"),
    (dict(MAX, full_batch_dtype='bf16'), "--full_batch_part_pull_max is not supported with --full_batch_dtype bf16"),
    (dict(MAX, history_dtype='fp16'), "--history_dtype must be one of fp32/bf16, got 'fp16'"),
    (dict(MAX, full_batch_part_history=True), TOGETHER % "full_batch_part_history"),
    (dict(MAX, full_batch_part_pull=True), TOGETHER % "full_batch_part_pull"),
    (dict(MAX, full_batch_part_pull_gat=True), TOGETHER % "full_batch_part_pull_gat"),
]


@pytest.mark.parametrize("flags,msg", REFUSALS)
def test_refusals(flags, msg):
    from stochastic_gcn_amd.full_batch import check_part_pull_max
    FLAGS.update(**flags)
    with pytest.raises(ValueError, match=msg):
        check_part_pull_max()


# (in the trainer the older checks run first: with one of their flags on beside the new one THEY refuse --aggregator max, in
# their own words; what is left for the new check to word is tried here)
@pytest.mark.parametrize("flags,msg", REFUSALS[1:7])
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


OLD = [
    ('check_part_history', dict(MAX, full_batch_part_history=True),
     "--full_batch_part_history is not supported with --aggregator max: the maximum and the attention kernels gather from one "
     "table; a two-table form is a follow-up"),
    ('check_part_pull', dict(MAX, full_batch_part_pull=True),
     "--full_batch_part_pull is not supported with --aggregator max: the maximum kernel gathers from one table; a two-table "
     "maximum is a follow-up"),
    ('check_part_pull_gat', dict(MAX, full_batch_part_pull_gat=True),
     r"--full_batch_part_pull_gat needs --aggregator attn \(got max\): it is the two-table form of the attention with learned "
     "scores; --full_batch_part_pull serves the sum"),
]


@pytest.mark.parametrize("check,flags,msg", OLD)
def test_the_older_checks_speak_as_before_and_first(monkeypatch, check, flags, msg):
    from stochastic_gcn_amd import train
    FLAGS.update(**flags)
    with pytest.raises(ValueError, match=msg):
        getattr(full_batch, check)()
    touched = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: touched.append("is_available") or False)
    monkeypatch.setattr(train, "load_data", lambda *a, **k: touched.append("load_data"))
    with pytest.raises(ValueError, match=msg):
        train.Trainer(verbose=False)
    assert touched == []


def test_the_older_checks_do_not_see_the_new_flag():
    """the new flag alone, accepted: the three older checks answer `off`; without it they answer what they always did"""
    FLAGS.update(**MAX)
    assert full_batch.check_part_pull_max() == (True, False)
    assert [getattr(full_batch, c)() for c, _, _ in OLD] == [(False, False)] * 3
    FLAGS.reset()
    FLAGS.update(full_batch=True, test_full_batch=True, full_batch_parts=4, full_batch_part_history=True, full_batch_part_pull=True)
    assert full_batch.check_part_history() == full_batch.check_part_pull() == (True, False)
    assert full_batch.check_part_pull_max() == (False, False)


def test_an_accepted_configuration_reaches_the_device_check(monkeypatch):
    from stochastic_gcn_amd import train
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(train, "load_data", lambda *a, **k: pytest.fail("data loaded without a device"))
    FLAGS.update(history_dtype='bf16', **MAX)
    with pytest.raises(RuntimeError, match="training needs an MI355X"):
        train.Trainer(verbose=False)


# ---- the reference ------------------------------------------------------------------------------------------------------
def _tiny():
    a = ir.signed(ir.flat_graph(40, 4, seed=2), seed=1).tolil()
    a[5, :] = 0                                    # a row that stores nothing
    a = a.tocsr()
    a.eliminate_zeros()
    a.sort_indices()
    return a


def _grid(rng, shape):
    """values from a coarse grid with both zeros -- the right half of the columns holds nothing above zero, so that a zero
    wins there: ties across the two tables occur, and ties between -0.0 and +0.0"""
    v = rng.randint(-2, 3, shape).astype(np.float32) / 2.0
    half = shape[1] // 2
    v[:, half:] = np.float32(0.0) - np.abs(v[:, half:])        # (0 - 0 = +0.0: the zeros' signs are drawn below)
    v[(v == 0) & (rng.rand(*shape) < 0.5)] = -0.0
    return v


@pytest.mark.parametrize("d,grid", [(3, False), (4, True)])
def test_reference_is_the_entrywise_definition_and_rejects_the_mutants(d, grid):
    a = _tiny()
    N = a.shape[0]
    rng = np.random.RandomState(3)
    subsets = {'all': np.arange(N), 'one': np.array([N // 3]), 'every_other': np.arange(0, N, 2),
               'third': np.sort(rng.choice(N, N // 3, replace=False))}
    caught = {m: 0 for m in xr.MUTANTS}
    for sname, ids in subsets.items():
        n = len(ids)
        draw = (lambda s: _grid(rng, s)) if grid else (lambda s: rng.randn(*s).astype(np.float32))
        X, H, G, add = draw((n, d)), draw((N, d)), rng.randn(n, d).astype(np.float32), rng.randn(n, d).astype(np.float32)
        C, arg = xr.forward(a, ids, X, H)
        lC, larg = xr.loops(a, ids, X, H)
        assert spmax_ref.same_bits(C, lC) and np.array_equal(arg, larg), sname
        assert np.array_equal(C, xr.dense(a, ids, X, H))                      # (values; +0.0 == -0.0 here)
        # the encoding: a fresh winner is a position in S, a stale one -2 - column, an empty row -1; decode undoes it
        g = xr.decode(arg, ids)
        m = pr.position_map(N, ids)
        empty = np.diff(a.indptr)[ids] == 0
        assert np.all((arg == -1) == empty[:, None]) and np.all(C[empty] == 0) and not np.signbit(C[empty]).any()
        assert np.all(m[g[arg >= 0]] == arg[arg >= 0]) and np.all(m[g[arg <= -2]] < 0) and np.all(g[arg <= -2] == -2 - arg[arg <= -2])
        Z = xr.merged32(ids, X, H)
        won = arg != -1
        assert spmax_ref.same_bits(C[won], Z[g[won], np.nonzero(won)[1]])
        # dX: the scatter to in-part winners only
        dX = xr.backward(n, G, arg)
        want = np.zeros((n, d), np.float64)
        for i in range(n):
            for c in range(d):
                if arg[i, c] >= 0:
                    want[arg[i, c], c] += float(G[i, c])
        f64, bound = xr.backward_f64(n, G, arg)
        assert np.allclose(f64, want, rtol=0, atol=1e-12) and np.all(np.abs(dX - f64) <= bound)
        assert np.array_equal(xr.backward(n, G, arg, add=add, add_rows=n), dX + add)
        rows, col, _ = pr._entries(a, ids)
        inside = m[col] >= 0
        for mname in xr.MUTANTS:
            mC, marg = xr.loops(a, ids, X, H, mutant=mname)
            if mname == 'grad_to_stale':
                assert spmax_ref.same_bits(mC, C)                             # its forward is right
                sent = marg.copy()
                sent[sent >= n] = -1
                off = not np.array_equal(spmax_ref.backward(xr._square(n), G, sent), dX)
                assert off == bool(np.any((arg <= -2) & (-2 - arg < n) & (G != 0)))
            else:
                off = not (spmax_ref.same_bits(mC, C) and np.array_equal(marg, arg))
                if mname == 'drop_out_of_part':
                    assert off == bool((~inside).any())                       # (a dropped entry's word is gone, at least)
            caught[mname] += int(off)
            print("%s d=%d: mutant %s %s" % (sname, d, mname, "differs" if off else "agrees"))
    print("mutants caught on %s of %d vertex sets" % (caught, len(subsets)))
    assert all(v > 0 for v in caught.values()), caught


def test_ties_across_the_tables_and_both_zeros_occur_on_the_grid():
    """the first of equal values wins whichever table it comes from: on the grid some maximum is tied between a fresh and a
    stale entry, with either kind first, and some winner is a -0.0 that a later +0.0 did not replace"""
    a = _tiny()
    N, d = a.shape[0], 6
    rng = np.random.RandomState(5)
    ids = np.arange(0, N, 2)
    X, H = _grid(rng, (len(ids), d)), _grid(rng, (N, d))
    C, arg = xr.forward(a, ids, X, H)
    assert np.array_equal(arg, xr.loops(a, ids, X, H)[1])
    m = pr.position_map(N, ids)
    Z = xr.merged32(ids, X, H)
    tied = dict(fresh_first=0, stale_first=0, neg_zero=0)
    for i, r in enumerate(ids):
        cols = a.indices[a.indptr[r]:a.indptr[r + 1]]
        for c in range(d):
            at = cols[Z[cols, c] == C[i, c]]
            if (m[at] >= 0).any() and (m[at] < 0).any():
                tied['fresh_first' if m[at[0]] >= 0 else 'stale_first'] += 1
                assert xr.decode(arg, ids)[i, c] == at[0]
            if at.size > 1 and C[i, c] == 0 and np.signbit(C[i, c]) and not np.signbit(Z[at[1:], c]).all():
                tied['neg_zero'] += 1
    print(tied)
    assert all(v > 0 for v in tied.values())


def test_the_patterns_of_the_gpu_test_store_no_column_twice():
    """ops.spmax_pull refuses a resident matrix that stores a column twice in a row (ops.check_unique_cols): none of the nine
    patterns does"""
    from test_induce_gpu import PATTERNS
    for name in sorted(PATTERNS):
        a = PATTERNS[name](np.random.RandomState(21)).tocsr()
        a.sort_indices()
        A = ops.DeviceCSR.from_scipy(a, torch.device('cpu'), with_plan=False)
        ops.check_unique_cols(A)
        assert A._unique_cols and a.shape[0] == a.shape[1] <= 400, name


def test_model_reference_steps_pushes_and_records_its_margins():
    import part_pull_max_cases as mc
    from oracle import model_np as mnp
    for name in sorted(mc.INIT):
        case = mc.build(name)
        ids = np.arange(0, case['n'], 2)
        rows = mc.loss_rows(case, ids)
        om = xr.make_model(case, seed=mc.INIT[name])
        logits, acts, loss, grads = om.step(ids, rows, case['labels'], 0.2, mnp.HashMasks(1, 0, 0.8))
        assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads.values())
        kinds = [k for k, _, _, _ in om.margins]
        assert kinds.count('max') == om.L == len(om.winners) and 'relu' in kinds and 0 < om.margin() < np.inf
        for l, t in enumerate(om.tables):
            if t is not None:
                assert np.array_equal(t[ids], om.pushed[l]) and not t[np.setdiff1d(np.arange(case['n']), ids)].any()


def test_the_committed_seeds_are_what_the_scan_gives():
    """well-posedness, established with the reference alone: the margins of both schedules at the committed seeds are at
    least MARGIN, and every step after the first epoch has a fresh and a stale winner in every max layer"""
    import max_aggregator_cases as mx
    import part_pull_max_cases as mc
    assert mc.MARGIN == mx.MARGIN == 1e-4 and (mc.P, mc.EPOCHS) == (3, 3) and list(mc.SEEDS) == list(range(3, 13))
    for name, seed in sorted(mc.INIT.items()):
        m = mc.margins(name, seed)
        both = mc.reaches_both_branches(name, seed)
        print("%s seed %d: margins single parts %.2e, refresh schedule %.2e; both branches reached: %s" % ((name, seed) + m + (both,)))
        assert min(m) >= mc.MARGIN and both and seed in mc.SEEDS


# ---- the exports --------------------------------------------------------------------------------------------------------
def test_exports_are_declared_and_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sgcn.h")).read()
    for s in EXPORTS:
        assert s in _ffi.SIGNATURES and hasattr(_ffi.lib, s) and (s + "(") in header
        assert len(_ffi.SIGNATURES[s][1]) == 16
    assert _ffi.lib.sgcn_abi_version() == 16 == _ffi.ABI_VERSION          # additive exports: the ABI version stays


def _err():
    return _ffi.lib.sgcn_last_error() or b""


P_ = 4096                                  # a 16-byte aligned address nobody reads


@pytest.mark.parametrize("name", EXPORTS)
def test_argument_checks(name):
    """every refusal comes before any HIP call: the addresses are never dereferenced"""
    fn = getattr(_ffi.lib, name)

    def call(rowptr=P_, col=P_, ids=P_, n=3, N=10, map_=P_, d=4, X=P_, ldx=8, H=P_, ldh=8, C=P_, ldc=8, arg=P_, ldarg=8):
        return fn(rowptr, col, ids, n, N, map_, d, X, ldx, H, ldh, C, ldc, arg, ldarg, None)
    assert call(n=-1) == -1 and b"negative size" in _err()
    assert call(n=0, N=-1) == -1 and b"negative size" in _err()
    assert call(n=11) == -1 and b"11 rows cannot be unique in [0, 10)" in _err()
    for d in (0, -4):
        assert call(d=d) == -1 and b"d must be positive" in _err()
    for pitch in ('ldx', 'ldh', 'ldc', 'ldarg'):
        assert call(**{pitch: 3}) == -1 and b"leading dimension smaller than d" in _err(), pitch
    assert call(arg=None, ldarg=0, n=0) == 0                                  # no arg: its pitch is not looked at
    for operand in ('rowptr', 'col', 'ids', 'map_', 'X', 'H', 'C'):
        assert call(**{operand: None}) == -1 and (b"null operand" in _err() or b"null history" in _err()), operand
    if name.endswith("_h16"):
        assert call(ldh=12, d=4) == -1 and b"ldh % 8 == 0" in _err()
        assert call(H=P_ + 8) == -1 and b"16-byte aligned" in _err()
    # n == 0: no launch, whatever the pointers
    zero = dict(rowptr=None, col=None, ids=None, n=0, map_=None, X=None, H=None, C=None, arg=None)
    assert call(**zero) == 0
    assert call(N=0, **zero) == 0


def test_the_wrapper_refuses_cpu_tensors_and_a_doubled_column():
    import scipy.sparse as sp
    a = sp.identity(4, format='csr', dtype=np.float32)
    A = ops.DeviceCSR.from_scipy(a, torch.device('cpu'), with_plan=False)
    ids, vmap = torch.arange(2, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.spmax_pull(A, ids, vmap, torch.zeros(2, 8), torch.zeros(4, 8))
    twice = sp.csr_matrix((np.ones(3, np.float32), np.array([1, 1, 2]), np.array([0, 2, 3, 3, 3])), shape=(4, 4))
    with pytest.raises(ValueError, match="unique column ids within each row"):
        ops.spmax_pull(ops.DeviceCSR.from_scipy(twice, torch.device('cpu'), with_plan=False), ids, vmap, torch.zeros(2, 8),
                       torch.zeros(4, 8))
    assert list(SPMAX_PULL.parameters) == ['A', 'ids_dev', 'map_dev', 'x', 'H', 'out', 'want_arg', 'arg']
    assert SPMAX_PULL.parameters['want_arg'].default is True and SPMAX_PULL.parameters['out'].default is None


# ---- the wiring ---------------------------------------------------------------------------------------------------------
n, N, d = w.n, w.N, w.d


class Recorder(w.Recorder):
    """the recorders of tests/test_aggregator_wiring.py, with a stand-in for ops.spmax_pull"""

    def __init__(self, monkeypatch):
        super(Recorder, self).__init__(monkeypatch)
        monkeypatch.setattr(ops, 'spmax_pull', self._stand_in('spmax_pull', SPMAX_PULL))

    def _spmax_pull(self, A, ids_dev, map_dev, x, H, out, want_arg, arg):
        shape = (ids_dev.shape[0], x.shape[1])
        return self._result('out', out, shape), (self.new('arg', shape, torch.int32) if want_arg else None)


class Rig(w.Rig):
    """one part batch over a PulledMatrix built with ``pull_max``"""

    def __init__(self, monkeypatch, pull_max, L=1, owned=None, training=True, x_dtype=torch.float32):
        self.rec = rec = Recorder(monkeypatch)
        self.x = rec.name('x', torch.randn(n, d).to(x_dtype))
        ids, vmap = rec.name('ids', torch.arange(n, dtype=torch.int32)), rec.name('map', torch.full((N,), -1, dtype=torch.int32))
        block = rec.name('block', w.Block((n, n), vmap))
        rec.name('blockT', block.transpose)
        resident = rec.name('resident', w.Block((N, N), None))
        tables = [rec.new('table%d' % l, (N, d)) for l in range(L)]
        args = (block, resident, ids, tables, owned or [True] * L, torch.device('cpu'))
        self.matrix = full_batch.PulledMatrix(*args) if pull_max is None else full_batch.PulledMatrix(*args, pull_max=pull_max)
        self.batch = full_batch.PartBatch(list(range(n)), ids, self.matrix, None, None, L)
        self.model = types.SimpleNamespace(cur=self.batch.cur(self.x), is_training=training, agg0_dim=d, dropout_seed=w.SEED,
                                           dropout_step=w.STEP)


def want_pull_max(concat, training, l=0, owned=True):
    g, add = w.grad(concat)
    fwd = [('spmax_pull', dict(A='resident', ids_dev=w.IDS, map_dev=w.MAP, x=w.X, H=w.TAB(l), **w.nbr_out(concat),
                               **({} if training else dict(want_arg=False))))]
    fwd += [('scatter_rows', dict(H=w.TAB(l), idx=w.IDS, src=w.X))] if owned else []
    return fwd, [('spmax_bwd', dict(At='blockT', g=g, arg=w.ARG, **add))]


@pytest.mark.parametrize("training", w.BOTH)
@pytest.mark.parametrize("concat", w.BOTH)
def test_pull_max_on(monkeypatch, concat, training):
    """one spmax_pull on resident / ids / map / x / table l into the concat view, then one scatter_rows; the backward is ONE
    spmax_bwd over the block's transpose with the pull's arg and the self half as its addend: no new backward launch"""
    w.flags('max', concat)
    rig = Rig(monkeypatch, True, training=training)
    assert rig.matrix.pull_max is True
    layer = rig.layer()
    w.run(rig, layer, concat, *want_pull_max(concat, training))
    assert layer._max and (layer._arg is not None) == training


@pytest.mark.parametrize("pull_max", [None, False])
@pytest.mark.parametrize("training", w.BOTH)
@pytest.mark.parametrize("concat", w.BOTH)
def test_pull_max_off_is_todays_launches(monkeypatch, concat, training, pull_max):
    """the switch defaults to off: the block's one-table maximum, nothing read, nothing pushed"""
    w.flags('max', concat)
    rig = Rig(monkeypatch, pull_max, training=training)
    assert rig.matrix.pull_max is False
    w.run(rig, rig.layer(), concat, *w.want_max(concat, training))


@pytest.mark.parametrize("concat", w.BOTH)
def test_an_unowned_table_is_read_and_never_written(monkeypatch, concat):
    w.flags('max', concat)
    rig = Rig(monkeypatch, True, owned=[False])
    want = want_pull_max(concat, True, owned=False)
    w.run(rig, rig.layer(), concat, *want)
    assert [name for name, _ in want[0]] == ['spmax_pull']


def test_two_layers_read_their_own_tables(monkeypatch):
    w.flags('max', True)
    rig = Rig(monkeypatch, True, L=2, owned=[False, True])
    for l, owned in ((0, False), (1, True)):
        w.run(rig, rig.layer(l), True, *want_pull_max(True, True, l=l, owned=owned))


def test_a_bfloat16_operand_is_refused_before_any_launch(monkeypatch):
    w.flags('max', False)
    rig = Rig(monkeypatch, True)
    with pytest.raises(ValueError, match="the two-table element-wise maximum has no bfloat16-operand form"):
        rig.matrix.pull_max_product(rig.x.to(torch.bfloat16), 0)
    with pytest.raises(ValueError, match="the two-table element-wise maximum has no bfloat16-operand form"):
        rig.matrix.layer(0).max_product(rig.x.to(torch.bfloat16))
    assert rig.rec.take() == []


def test_the_trainer_hands_the_switch_to_the_matrix():
    """train.Trainer.part_batch passes pull_max=self.part_pull_max (read from the source: building a trainer needs a device)"""
    from stochastic_gcn_amd import train
    src = inspect.getsource(train.Trainer.part_batch)
    assert "pull_max=self.part_pull_max" in src
    assert "check_part_pull_max()" in inspect.getsource(train.Trainer.__init__)
