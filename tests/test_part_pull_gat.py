"""CPU tests of --full_batch_part_pull_gat (part steps of --aggregator attn --attn_score gat that read stored rows AND stored
destination scores for their out-of-part neighbours): the flag, its refusals before a device is touched, the fp64 reference
of the two-table attention (tests/part_pull_gat_ref.py) against an entry-by-entry evaluation and four mutants, central
differences of the fp64 layer, and the argument checks of the four exports through the raw C-ABI.  Nothing here touches a
device."""
import os

import numpy as np
import pytest
import torch

import induce_ref as ir
import part_history_ref as pr
import part_pull_gat_ref as gr
import spgat_ref
from stochastic_gcn_amd import _ffi
from stochastic_gcn_amd.flags import _DEFS, FLAGS, _Flags

FWD = ("sgcn_spgat_pull_f32", "sgcn_spgat_pull_h16")
BWD = ("sgcn_spgat_pull_bwd_u_f32", "sgcn_spgat_pull_bwd_u_h16")
ON = dict(full_batch=True, test_full_batch=True, full_batch_parts=4, full_batch_part_pull_gat=True, aggregator='attn',
          attn_score='gat')


@pytest.fixture(autouse=True)
def _reset_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


# ---- 1. the flag --------------------------------------------------------------------------------------------------------
def test_flag_defaults_and_parsing():
    from stochastic_gcn_amd.full_batch import check_part_history, check_part_pull, check_part_pull_gat
    f = _Flags()
    assert f.full_batch_part_pull_gat is False and 'full_batch_part_pull_gat' in f.as_dict()
    name, typ, default, text = next(d[:4] for d in _DEFS if d[0] == 'full_batch_part_pull_gat')
    assert (typ, default) == (bool, False)
    for word in ('--attn_score gat', 'stored scores', 'in-part entries only', '--history_dtype bf16', '--attn_dropout',
                 '--reverse', '--full_batch_dtype bf16'):
        assert word in text, word
    assert check_part_pull_gat(f) == (False, False)                # off: nothing else is looked at
    argv = ['--full_batch', '--test_full_batch', '--full_batch_parts', '8', '--full_batch_part_pull_gat', '--aggregator', 'attn',
            '--attn_score', 'gat']
    f.parse(argv)
    assert check_part_pull_gat(f) == (True, False)
    assert check_part_pull(f) == (False, False) and check_part_history(f) == (False, False)
    f.parse(argv + ['--attn_heads', '4', '--attn_slope', '0.1'])
    assert check_part_pull_gat(f) == (True, False)
    f.parse(argv + ['--history_dtype', 'bf16'])
    assert check_part_pull_gat(f) == (True, True)                  # bf16 is reported
    f.parse(argv + ['--history_dtype', 'bf16', '--nofull_batch_part_pull_gat'])
    assert check_part_pull_gat(f) == (False, False)
    # what it does not interfere with
    FLAGS.update(full_batch_parts_per_step=4, full_batch_part_norm='keep', dense_dtype='bf16', attn_heads=2, **ON)
    assert check_part_pull_gat() == (True, False)


# ---- 2. the refusals ----------------------------------------------------------------------------------------------------
REFUSALS = [
    (dict(full_batch_part_pull_gat=True), "--full_batch_part_pull_gat needs --full_batch_parts > 0"),
    (dict(full_batch=True, full_batch_part_pull_gat=True, aggregator='attn', attn_score='gat'),
     "--full_batch_part_pull_gat needs --full_batch_parts > 0"),
    (dict(ON, aggregator='sum', attn_score='dot'), r"--full_batch_part_pull_gat needs --aggregator attn \(got sum\)"),
    (dict(ON, aggregator='max', attn_score='dot'), r"--full_batch_part_pull_gat needs --aggregator attn \(got max\)"),
    (dict(ON, attn_score='dot'), "--full_batch_part_pull_gat needs --attn_score gat"),
    (dict(ON, attn_dropout=0.1), "--full_batch_part_pull_gat is not supported with --attn_dropout > 0.*mask of out-of-part "
                                 "entries is not defined"),
    (dict(ON, reverse=True), "--full_batch_part_pull_gat is not supported with --reverse"),
    (dict(ON, full_batch_dtype='bf16'), "--full_batch_part_pull_gat is not supported with --full_batch_dtype bf16"),
    (dict(ON, history_dtype='fp16'), "--history_dtype must be one of"),
]


@pytest.mark.parametrize("flags,msg", REFUSALS)
def test_refusals(flags, msg):
    from stochastic_gcn_amd.full_batch import check_part_pull_gat
    FLAGS.update(**flags)
    with pytest.raises(ValueError, match=msg):
        check_part_pull_gat()


def _untouched(monkeypatch):
    from stochastic_gcn_amd import train
    touched = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: touched.append("is_available") or False)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: touched.append("set_device"))
    monkeypatch.setattr(train, "load_data", lambda *a, **k: touched.append("load_data"))
    return train, touched


@pytest.mark.parametrize("flags,msg", REFUSALS)
def test_trainer_refuses_before_a_device_is_touched(monkeypatch, flags, msg):
    """in every case this check is the first of the trainer's to speak, with its own words"""
    train, touched = _untouched(monkeypatch)
    FLAGS.update(**flags)
    with pytest.raises(ValueError, match=msg):
        train.Trainer(verbose=False)
    assert touched == []


def test_the_older_flags_speak_first_and_keep_their_words(monkeypatch):
    """with --full_batch_part_pull also on the old message about --attn_score gat is the one raised, in the trainer too; with
    --full_batch_part_history, that flag's message about --aggregator attn"""
    train, touched = _untouched(monkeypatch)
    from stochastic_gcn_amd.full_batch import check_part_history, check_part_pull
    FLAGS.update(full_batch_part_pull=True, **ON)
    old = ("--full_batch_part_pull is not supported with --attn_score gat: its score table would need stale scores for the "
           "out-of-part neighbours; a two-table form is a follow-up")
    with pytest.raises(ValueError, match=old):
        check_part_pull()
    with pytest.raises(ValueError, match=old):
        train.Trainer(verbose=False)
    FLAGS.reset()
    FLAGS.update(full_batch_part_history=True, **ON)
    with pytest.raises(ValueError, match="--full_batch_part_history is not supported with --aggregator attn"):
        check_part_history()
    with pytest.raises(ValueError, match="--full_batch_part_history is not supported with --aggregator attn"):
        train.Trainer(verbose=False)
    assert touched == []


def test_an_accepted_configuration_reaches_the_device_check(monkeypatch):
    from stochastic_gcn_amd import train
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(train, "load_data", lambda *a, **k: pytest.fail("data loaded without a device"))
    FLAGS.update(attn_heads=2, history_dtype='bf16', **ON)
    with pytest.raises(RuntimeError, match="training needs an MI355X"):
        train.Trainer(verbose=False)


# ---- 3. the reference ---------------------------------------------------------------------------------------------------
def _tiny():
    a = ir.signed(ir.flat_graph(40, 4, seed=2), seed=1)
    a.sort_indices()
    return a


@pytest.mark.parametrize("heads,d", [(1, 3), (2, 4)])
def test_reference_is_the_entrywise_evaluation_and_rejects_the_mutants(heads, d):
    a = _tiny()
    N = a.shape[0]
    rng = np.random.RandomState(3)
    T, VH, avec = rng.randn(N, d), rng.randn(N, heads), rng.randn(2, d)
    subsets = {'all': np.arange(N), 'one': np.array([N // 3]), 'every_other': np.arange(0, N, 2),
               'third': np.sort(rng.choice(N, N // 3, replace=False))}
    slope = 0.2
    for sname, ids in subsets.items():
        n = len(ids)
        X, G, add = rng.randn(n, d), rng.randn(n, d), rng.randn(n, d)
        b = gr.backward(a, ids, X, T, VH, avec, G, slope, heads)
        C, lse, dU, dX, da = gr.loops(a, ids, X, T, VH, avec, G, slope, heads)
        errs = [float(np.abs(x - y).max()) for x, y in ((b['C'], C), (b['lse'], lse), (b['dU'], dU), (b['dX'], dX), (b['da'], da))]
        print("%s / heads %d: |reference - entry-wise|  C %.2e  lse %.2e  dU %.2e  dX %.2e  da %.2e" % ((sname, heads) + tuple(errs)))
        assert b['C'].shape == (n, d) and b['lse'].shape == (n, heads) and max(errs) <= 1e-12
        # ``forward`` alone, from the tables
        f = gr.forward(a, ids, X, T, b['S'][:, :heads], b['S'][:, heads:], VH, slope, heads)
        assert np.array_equal(f.C, b['C']) and np.array_equal(f.lse, b['lse'])
        with_add = gr.backward(a, ids, X, T, VH, avec, G, slope, heads, add=add, add_rows=n)
        assert np.allclose(with_add['dX'], dX + add, rtol=0, atol=1e-12) and np.array_equal(with_add['da'], b['da'])
        rows, col, _ = pr._entries(a, ids)
        outside = bool((pr.position_map(N, ids)[col] < 0).any())
        # a mutant must differ exactly where its kind of entry exists.  Scores pushed BEFORE the pull write VH[ids] only, and
        # columns inside S never read the table: that mutant has no entry to differ on -- which is why the push may come
        # either side of the pull -- and must give the definition's numbers on every vertex set
        differs = dict(recompute_scores=outside, du_in_part=outside, da1_stale=outside, push_before_pull=False)
        for mname in gr.MUTANTS:
            m = gr.loops(a, ids, X, T, VH, avec, G, slope, heads, mutant=mname)
            off = max(float(np.abs(x - y).max()) for x, y in zip(m, (C, lse, dU, dX, da)))
            print("    mutant %s: off by %.3e (%s)" % (mname, off, "must differ" if differs[mname] else "no such entry"))
            if sname == 'one' and mname in ('du_in_part', 'da1_stale'):
                # (one selected row: sum_e e_e = 0 by construction, so where every z_e lies on one side of the LeakyReLU's
                # kink the row's dz_e sum to rounding and there is no gradient for these two to misplace; not asserted)
                continue
            assert (off > 1e-3) == differs[mname], mname
            if not differs[mname]:
                assert off == 0.0
            if mname in ('du_in_part', 'da1_stale'):
                assert np.array_equal(m[0], C) and np.array_equal(m[1], lse)         # their forward is right
            if mname == 'da1_stale':
                assert np.array_equal(m[4][0], da[0]) and (not outside or np.abs(m[4][1] - da[1]).max() > 1e-3)
            if mname == 'du_in_part' and outside:
                assert np.abs(m[4][0] - da[0]).max() > 1e-3 and np.array_equal(m[4][1], da[1])
    assert not (pr.position_map(N, subsets['all']) < 0).any()


def test_a_stale_score_table_that_mirrors_the_fresh_scores_is_what_the_mutant_reads():
    """the mutant 'recompute_scores' IS the definition where VH happens to hold T a[1]: the comparison above separates the
    two only because the stored scores are another step's"""
    a = _tiny()
    rng = np.random.RandomState(5)
    d, heads = 4, 2
    T, avec = rng.randn(40, d), rng.randn(2, d)
    ids = np.arange(0, 40, 2)
    X, G = rng.randn(20, d), rng.randn(20, d)
    VH = spgat_ref.scores_f64(T, avec, heads)[0][:, heads:]
    want = gr.loops(a, ids, X, T, VH, avec, G, 0.2, heads)
    got = gr.loops(a, ids, X, T, rng.randn(40, heads), avec, G, 0.2, heads, mutant='recompute_scores')
    assert max(float(np.abs(x - y).max()) for x, y in zip(got, want)) <= 1e-12


# ---- 4. central differences ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,slope", [(2, 0.2), (1, 0.0), (2, 1.0)])
def test_reference_backward_is_the_derivative_of_its_forward(heads, slope):
    """d(sum(G . C)) / dX and / da by central differences of the fp64 layer with both tables held constant"""
    a = _tiny()
    rng = np.random.RandomState(0)
    ids = np.sort(rng.choice(40, 17, replace=False))
    d = 4
    X, T, VH, G, avec = rng.randn(17, d), rng.randn(40, d), rng.randn(40, heads), rng.randn(17, d), rng.randn(2, d)
    want = gr.backward(a, ids, X, T, VH, avec, G, slope, heads)
    z = np.abs(np.concatenate(want['fwd'].z))
    assert z.min() > 1e-3, "an entry sits on the LeakyReLU's kink: central differences are not defined there"

    def value(X_, a_):
        return float((gr.backward(a, ids, X_, T, VH, a_, G, slope, heads)['C'] * G).sum())
    h = 1e-6
    dX = np.zeros_like(X)
    for i in range(17):
        for k in range(d):
            e = np.zeros_like(X)
            e[i, k] = h
            dX[i, k] = (value(X + e, avec) - value(X - e, avec)) / (2 * h)
    da = np.zeros_like(avec)
    for w in (0, 1):
        for k in range(d):
            e = np.zeros_like(avec)
            e[w, k] = h
            da[w, k] = (value(X, avec + e) - value(X, avec - e)) / (2 * h)
    ex, ea = float(np.abs(dX - want['dX']).max()), float(np.abs(da - want['da']).max())
    print("heads %d slope %g: central differences against the reference  dX %.3e  da %.3e" % (heads, slope, ex, ea))
    assert ex <= 1e-7 * max(1.0, float(np.abs(want['dX']).max()))
    assert ea <= 1e-7 * max(1.0, float(np.abs(want['da']).max()))


def test_model_reference_steps_and_pushes():
    """the fp64 model: a step pushes its aggregation inputs and destination scores, the refresh stops at the last aggregation
    and pushes both, heads change numbers, attn_vec has a gradient"""
    import part_pull_gat_cases as gc
    from oracle import model_np as mnp
    case = gc.build('sage_ln_pp')
    ids = np.arange(0, case['n'], 2)
    rest = np.setdiff1d(np.arange(case['n']), ids)
    rows = np.flatnonzero(np.isin(ids, case['train'])).astype(np.int32)
    out = {}
    for heads in (1, 2):
        om = gc.make_model(case, heads, seed=3)
        assert len(om.scores) == om.L and all(s.shape == (case['n'], heads) and not s.any() for s in om.scores)
        logits, acts, loss, grads = om.step(ids, rows, case['labels'], 0.2, mnp.HashMasks(1, 0, 0.8))
        assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads.values())
        assert all(np.abs(grads['agg%d/attn_vec' % l]).max() > 0 for l in range(om.L))
        for l in range(om.L):
            if om.tables[l] is not None:
                assert np.array_equal(om.tables[l][ids], om.pushed[l]) and not om.tables[l][rest].any()
            assert np.array_equal(om.scores[l][ids], om.pushed_scores[l]) and not om.scores[l][rest].any()
            assert np.abs(om.scores[l][ids]).max() > 0
        before = {k: v.copy() for k, v in om.params.items()}
        om.forward_part(rest, 0.2, mnp.HashMasks(1, 1, 0.8), stop_at_last_agg=True)
        assert all(np.abs(s[rest]).max() > 0 for s in om.scores) and sorted(om.pushed_scores) == list(range(om.L))
        assert all(np.array_equal(before[k], om.params[k]) for k in before)
        out[heads] = logits
    assert np.abs(out[1] - out[2]).max() > 1e-6


def test_the_chosen_seeds_meet_the_margin():
    """the condition of part_pull_gat_cases.py, re-evaluated by the reference for one case (the scan itself is in that file)"""
    import part_pull_gat_cases as gc
    name, heads = 'gcn_nopp', 2
    m = gc.margins(name, heads, gc.INIT[(name, heads)])
    print("%s heads %d seed %d: (ReLU, z) margins %s" % (name, heads, gc.INIT[(name, heads)], m))
    assert min(min(x) for x in m) >= gc.MARGIN


# ---- 5. the exports -----------------------------------------------------------------------------------------------------
def test_exports_are_declared_and_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sgcn.h")).read()
    for names, nargs in ((FWD, 23), (BWD, 27)):
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
        def call(rowptr=P_, col=P_, ids=P_, n=3, N=10, map_=P_, d=4, heads=1, X=P_, ldx=8, H=P_, ldh=8, U=P_, ldu=1, V=P_, ldv=1,
                 VH=P_, ldvh=1, slope=0.2, C=P_, ldc=8, lse=P_):
            return fn(rowptr, col, ids, n, N, map_, d, heads, X, ldx, H, ldh, U, ldu, V, ldv, VH, ldvh, slope, C, ldc, lse, None)
        return call, ('ldx', 'ldh', 'ldc'), ('rowptr', 'col', 'ids', 'map_', 'X', 'H', 'U', 'V', 'VH', 'C')

    def call(rowptr=P_, col=P_, ids=P_, n=3, N=10, map_=P_, d=4, heads=1, X=P_, ldx=8, H=P_, ldh=8, U=P_, ldu=1, V=P_, ldv=1,
             VH=P_, ldvh=1, slope=0.2, G=P_, ldg=8, C=P_, ldc=8, lse=P_, delta=P_, dU=P_):
        return fn(rowptr, col, ids, n, N, map_, d, heads, X, ldx, H, ldh, U, ldu, V, ldv, VH, ldvh, slope, G, ldg, C, ldc, lse,
                  delta, dU, None)
    return call, ('ldx', 'ldh', 'ldg', 'ldc'), ('rowptr', 'col', 'ids', 'map_', 'X', 'H', 'U', 'V', 'VH', 'G', 'C', 'lse', 'delta',
                                                 'dU')


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
    for pitch in ('ldu', 'ldv', 'ldvh'):      # the score tables' pitches: below heads
        assert call(heads=2, **{pitch: 1}, **{p: 2 for p in ('ldu', 'ldv', 'ldvh') if p != pitch}) == -1
        assert b"score table pitch smaller than heads" in _err(), pitch
        assert call(**{pitch: 0}) == -1 and b"score table pitch smaller than heads" in _err()
    for operand in operands:
        assert call(**{operand: None}) == -1 and b"null operand" in _err(), operand
    for slope in (-0.1, 1.5, float('nan'), float('inf'), -float('inf')):
        assert call(slope=slope) == -1 and b"slope must lie in [0, 1]" in _err(), slope
    # the width limit d <= 256 * VW: 1032 columns at VW = 4; 520 on an odd pitch (VW = 1); heads whose width VW must divide
    assert call(d=1032, **at(1032)) == -1 and b"is over the limit of 1024 columns at vector width 4" in _err()
    assert call(d=520, heads=8, ldu=8, ldv=8, ldvh=8, **at(521)) == -1 and b"is over the limit of 256 columns at vector width 1" in _err()
    assert call(d=520, heads=8, ldu=8, ldv=8, ldvh=8, **at(520)) == -1 and b"vector width 1" in _err()   # 65 per head: VW = 1
    if h16:
        assert call(ldh=12, d=4) == -1 and b"ldh % 8 == 0" in _err()
        assert call(H=P_ + 8) == -1 and b"16-byte aligned" in _err()
    # n == 0: no launch, whatever the pointers
    zero = dict(rowptr=None, col=None, ids=None, n=0, map_=None, X=None, H=None, U=None, V=None, VH=None, C=None)
    assert call(**zero) == 0
    assert call(N=0, **zero) == 0
