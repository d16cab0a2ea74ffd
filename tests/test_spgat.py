"""--attn_score gat without a device: the reference of tests/spgat_ref.py against the definition stated entry by entry and
against central differences, its derived bounds against two fp32 restatements of the kernels' algorithm (accepted) and
against three wrong results (rejected), the flags and their refusals, the exports' argument checks, and the parameter
layout with the flag off."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import spgat_ref as ref
from stochastic_gcn_amd import _ffi, ops
from stochastic_gcn_amd.flags import _DEFS, FLAGS, _Flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


def small(seed, M=7, K=9, d=8, heads=2, keep=1.0, dens=0.45):
    """a tiny case: a pattern with an empty row and a single-entry row, normal x-like tables, scores of both signs"""
    rng = np.random.RandomState(seed)
    pat = (rng.uniform(size=(M, K)) < dens).astype(np.float32)
    pat[1, :] = 0
    pat[2, :] = 0
    pat[2, K - 1] = 1
    pat[0, :] = 1                                          # a full row
    a = sp.csr_matrix(pat)
    a.sort_indices()
    U = (1.5 * rng.standard_normal((M, heads))).astype(np.float32)
    V = (1.5 * rng.standard_normal((K, heads))).astype(np.float32)
    B = rng.standard_normal((K, d)).astype(np.float32)
    G = rng.standard_normal((M, d)).astype(np.float32)
    mk = None
    if keep < 1.0:
        mk = (rng.uniform(size=(a.nnz, heads)) < keep) * np.float32(1.0 / keep)
    return a, U, V, B, G, mk


CASES = [(1, 8, 1, 1.0), (2, 8, 2, 1.0), (3, 8, 4, 0.7), (4, 5, 1, 0.7), (5, 6, 2, 1.0)]
SLOPE = 0.2


@pytest.mark.parametrize("seed,d,H,keep", CASES)
def test_reference_is_the_definition(seed, d, H, keep):
    a, U, V, B, G, mk = small(seed, d=d, heads=H, keep=keep)
    f = ref.forward(a, U, V, B, SLOPE, H, mk)
    C, lse = ref.forward_loops(a, U, V, B, SLOPE, H, mk)
    np.testing.assert_allclose(f.C, C, rtol=1e-13, atol=1e-14)
    assert np.array_equal(np.isinf(f.lse), np.isinf(lse)) and np.all(f.lse[1] == -np.inf) and np.all(f.C[1] == 0)
    np.testing.assert_allclose(f.lse[np.isfinite(lse)], lse[np.isfinite(lse)], rtol=1e-13)
    b, bl = ref.backward_f64(a, U, V, B, G, SLOPE, H, mk), ref.backward_loops(a, U, V, B, G, SLOPE, H, mk)
    for k in ('dU', 'dV', 'dB', 'delta'):
        np.testing.assert_allclose(b[k], bl[k], rtol=1e-12, atol=1e-13, err_msg=k)
    # the scores: u and v are per-head dot products with a[0] and a[1]
    rng = np.random.RandomState(seed)
    x, av = rng.standard_normal((9, d)).astype(np.float32), rng.standard_normal((2, d)).astype(np.float32)
    S, _ = ref.scores_f64(x, av, H)
    dh = d // H
    for r in range(9):
        for h in range(H):
            assert abs(S[r, h] - sum(float(x[r, c]) * float(av[0, c]) for c in range(h * dh, (h + 1) * dh))) < 1e-13
            assert abs(S[r, H + h] - sum(float(x[r, c]) * float(av[1, c]) for c in range(h * dh, (h + 1) * dh))) < 1e-13


def test_kink_takes_the_slope_at_zero():
    """z == 0 exactly: s = 0 and dz = slope * e"""
    a = sp.csr_matrix(np.ones((1, 2), np.float32))
    U, V = np.array([[1.0]], np.float32), np.array([[-1.0], [0.5]], np.float32)
    B, G = np.array([[1.0], [3.0]], np.float32), np.array([[1.0]], np.float32)
    b = ref.backward_f64(a, U, V, B, G, 0.25)
    f = b['fwd']
    assert f.z[0][0] == 0.0 and f.s[0][0] == 0.0
    p = np.exp(np.array([0.0, 1.5])) / np.sum(np.exp(np.array([0.0, 1.5])))
    delta = p[0] * 1.0 + p[1] * 3.0
    e = p * (np.array([1.0, 3.0]) - delta)
    np.testing.assert_allclose(b['dV'][:, 0], e * np.array([0.25, 1.0]), rtol=1e-14)
    np.testing.assert_allclose(b['dU'][0, 0], e[0] * 0.25 + e[1], rtol=1e-14)


@pytest.mark.parametrize("seed,d,H,keep", CASES)
def test_reference_backward_against_central_differences(seed, d, H, keep):
    a, U, V, B, G, mk = small(seed, d=d, heads=H, keep=keep)
    U, V, B = (t.astype(np.float64) for t in (U, V, B))
    # (move every |z| away from the kink by more than the step)
    eps = 1e-6
    z = np.abs(U[:, None, :] + V[None, :, :])
    assert z.min() > 1e-3
    b = ref.backward_f64(a, U, V, B, G, SLOPE, H, mk)
    loss = lambda U_, V_, B_: float(np.sum(G * ref.forward(a, U_, V_, B_, SLOPE, H, mk, values_only=True).C))
    for name, idx in (('dU', 0), ('dV', 1), ('dB', 2)):
        T = (U, V, B)[idx]
        num = np.zeros_like(T)
        for i in np.ndindex(*T.shape):
            hi, lo = [t.copy() for t in (U, V, B)], [t.copy() for t in (U, V, B)]
            hi[idx][i] += eps
            lo[idx][i] -= eps
            num[i] = (loss(*hi) - loss(*lo)) / (2 * eps)
        np.testing.assert_allclose(b[name], num, rtol=2e-6, atol=2e-8, err_msg=name)


@pytest.mark.parametrize("seed,d,H,keep", [(11, 8, 2, 1.0), (12, 6, 1, 0.7), (13, 8, 4, 1.0)])
def test_layer_gradients_against_central_differences(seed, d, H, keep):
    """da and dX through the whole chain: scores from (x, a), B = x"""
    rng = np.random.RandomState(seed)
    n = 8
    pat = (rng.uniform(size=(n, n)) < 0.5).astype(np.float32)
    np.fill_diagonal(pat, 1)
    a = sp.csr_matrix(pat)
    a.sort_indices()
    x, av, G = rng.standard_normal((n, d)), rng.standard_normal((2, d)), rng.standard_normal((n, d))
    mk = (rng.uniform(size=(a.nnz, H)) < keep) / keep if keep < 1 else None
    out = ref.layer_f64(a, x, av, SLOPE, H, G, mk)
    S = out['S']
    assert np.abs(S[:, None, :H] + S[None, :, H:]).min() > 1e-4
    eps = 1e-6
    loss = lambda x_, a_: float(np.sum(G * ref.layer_f64(a, x_, a_, SLOPE, H, mk=mk)['C']))
    for name, idx in (('dX', 0), ('da', 1)):
        T = (x, av)[idx]
        num = np.zeros_like(T)
        for i in np.ndindex(*T.shape):
            hi, lo = [x.copy(), av.copy()], [x.copy(), av.copy()]
            hi[idx][i] += eps
            lo[idx][i] -= eps
            num[i] = (loss(*hi) - loss(*lo)) / (2 * eps)
        np.testing.assert_allclose(out[name], num, rtol=5e-6, atol=5e-8, err_msg=name)


def _inside(got, want, bound):
    return bool(np.all(np.abs(np.asarray(got, np.float64) - want) <= bound))


@pytest.mark.parametrize("seed,d,H,keep", CASES)
@pytest.mark.parametrize("reverse,cut", [(False, False), (True, True)])
def test_bounds_accept_fp32_restatements_in_two_orders(seed, d, H, keep, reverse, cut):
    a, U, V, B, G, mk = small(seed, M=12, K=14, d=d, heads=H, keep=keep, dens=0.6)
    b = ref.backward_f64(a, U, V, B, G, SLOPE, H, mk)
    f = b['fwd']
    C, lse = ref.forward_online_f32(a, U, V, B, SLOPE, H, mk, reverse=reverse, cut=cut)
    assert _inside(C, f.C, f.bound_C)
    fin = np.isfinite(f.lse)
    assert np.array_equal(fin, np.isfinite(lse)) and _inside(lse[fin], f.lse[fin], f.bound_lse[fin])
    g = ref.backward_f32(a, U, V, B, G, SLOPE, C, lse, H, mk, reverse=reverse, cut=cut)
    for k in ('dU', 'dV', 'dB', 'delta'):
        assert _inside(g[k], b[k], b['bound_' + k]), k
        # (a bound that accepts anything would accept these too; what it rejects: test_bounds_reject_wrong_results)
        assert float(np.max(b['bound_' + k])) < 1e-3, k


def test_scores_bound_accepts_the_kernel_order_and_dyadic_tables_are_exact():
    rng = np.random.RandomState(3)
    for d, H in ((5, 1), (132, 4), (64, 8), (602, 2)):
        x, av = rng.standard_normal((9, d)).astype(np.float32), rng.standard_normal((2, d)).astype(np.float32)
        S, bound = ref.scores_f64(x, av, H)
        assert _inside(ref.scores_f32_kernel_order(x, av, H), S, bound)
        xi = rng.randint(-4, 5, (9, d)).astype(np.float32) * np.float32(0.5)
        ai = rng.randint(-4, 5, (2, d)).astype(np.float32) * np.float32(0.25)
        assert np.array_equal(ref.scores_f32_kernel_order(xi, ai, H).astype(np.float64), ref.scores_f64(xi, ai, H)[0])


@pytest.mark.parametrize("seed,d,H,keep", CASES[:3])
def test_bounds_reject_wrong_results(seed, d, H, keep):
    """one entry left out; the slope replaced by 1; a_src and a_dst swapped -- each lands outside the bounds somewhere in
    C and in every gradient.  The inputs: scores of both signs and of order 1 (a slope that matters), a_src != a_dst, rows with
    several entries of comparable weight (an entry that matters)."""
    rng = np.random.RandomState(seed)
    n = 10
    pat = (rng.uniform(size=(n, n)) < 0.6).astype(np.float32)
    np.fill_diagonal(pat, 1)
    a = sp.csr_matrix(pat)
    a.sort_indices()
    x = rng.standard_normal((n, d)).astype(np.float32)
    av = rng.standard_normal((2, d)).astype(np.float32)
    G = rng.standard_normal((n, d)).astype(np.float32)
    mk = (rng.uniform(size=(a.nnz, H)) < keep) * np.float32(1.0 / keep) if keep < 1 else None
    S = ref.scores_f64(x, av, H)[0].astype(np.float32)
    Uu, Vv = S[:, :H], S[:, H:]
    right = ref.backward_f64(a, Uu, Vv, x, G, SLOPE, H, mk)
    # (1) the first entry of the longest row left out
    i = int(np.argmax(np.diff(a.indptr)))
    e0 = a.indptr[i]
    less = a.copy().tolil()
    less[i, a.indices[e0]] = 0
    less = less.tocsr()
    less.eliminate_zeros()
    less.sort_indices()
    mk_less = None if mk is None else np.delete(mk, e0, axis=0)
    wrong = [ref.backward_f64(less, Uu, Vv, x, G, SLOPE, H, mk_less),
             ref.backward_f64(a, Uu, Vv, x, G, 1.0, H, mk),                                     # (2) no LeakyReLU
             ref.backward_f64(a, S[:, H:], S[:, :H], x, G, SLOPE, H, mk)]                       # (3) a_src <-> a_dst
    for w in wrong:
        assert not _inside(w['fwd'].C, right['fwd'].C, right['fwd'].bound_C)
        for k in ('dU', 'dV', 'dB'):
            assert not _inside(w[k], right[k], right['bound_' + k]), k


def test_scores_bwd_reference():
    rng = np.random.RandomState(5)
    d, H, rows, ru = 12, 4, 70, 65
    x, av = rng.standard_normal((rows, d)), rng.standard_normal((2, d))
    dU, dV, dx0 = rng.standard_normal((ru, H)), rng.standard_normal((rows, H)), rng.standard_normal((rows, d))
    out = ref.scores_bwd_f64(x, av, dU, dV, H, dx0)
    dh = d // H
    for c in (0, 5, 11):
        h = c // dh
        assert abs(out['da'][0, c] - sum(dU[r, h] * x[r, c] for r in range(ru))) < 1e-12
        assert abs(out['da'][1, c] - sum(dV[r, h] * x[r, c] for r in range(rows))) < 1e-12
        assert abs(out['dx'][3, c] - (dx0[3, c] + dU[3, h] * av[0, c] + dV[3, h] * av[1, c])) < 1e-13
        assert abs(out['dx'][68, c] - (dx0[68, c] + dV[68, h] * av[1, c])) < 1e-13          # (no dU row there)


# ---- the flags ----------------------------------------------------------------------------------------------------------------
BOTH = dict(full_batch=True, test_full_batch=True, aggregator='attn')


def test_flag_default_parsing_and_help():
    from stochastic_gcn_amd.full_batch import check_attention, check_attn_score
    f = _Flags()
    assert f.attn_score == 'dot' and f.attn_slope == 0.2 and check_attn_score(f) == (False, 0.2)
    f.parse(['--full_batch', '--test_full_batch', '--aggregator', 'attn', '--attn_score', 'gat', '--attn_slope', '0.1'])
    assert check_attn_score(f) == (True, 0.1) and check_attention(f) == (True, 0.0)
    for s in (0.0, 0.2, 1.0):
        FLAGS.update(**BOTH, attn_score='gat', attn_slope=s)
        assert check_attn_score() == (True, s)
    FLAGS.reset()
    FLAGS.update(**BOTH)
    assert check_attn_score() == (False, 0.2)
    help_ = {name: h for name, _, _, h in _DEFS}
    assert 'agg0/attn_vec' in help_['attn_score'] and 'get_pred_and_grad' in help_['attn_score']
    assert ('attn_score', str, 'dot') == next(d[:3] for d in _DEFS if d[0] == 'attn_score')
    assert ('attn_slope', float, 0.2) == next(d[:3] for d in _DEFS if d[0] == 'attn_slope')


REFUSALS = [
    (dict(BOTH, attn_score='gatv2'), r"--attn_score must be one of dot/gat, got 'gatv2'"),
    (dict(attn_score='gat'), r"--attn_score gat needs --aggregator attn"),
    (dict(full_batch=True, test_full_batch=True, aggregator='max', attn_score='gat'), r"--attn_score gat needs --aggregator attn"),
    (dict(BOTH, attn_score='gat', attn_scale=0.5), r"--attn_score gat is not supported with --attn_scale"),
    (dict(BOTH, attn_score='gat', attn_slope=-0.1), r"--attn_slope must lie in \[0, 1\], got -0.1"),
    (dict(BOTH, attn_score='gat', attn_slope=1.5), r"--attn_slope must lie in \[0, 1\]"),
    (dict(BOTH, attn_score='gat', attn_slope=float('nan')), r"--attn_slope must lie in \[0, 1\]"),
    (dict(BOTH, attn_slope=0.1), r"--attn_slope needs --attn_score gat"),
    (dict(attn_slope=0.3), r"--attn_slope needs --attn_score gat"),
]


@pytest.mark.parametrize("flags,msg", REFUSALS)
def test_refusals(flags, msg):
    from stochastic_gcn_amd.full_batch import check_attn_score
    FLAGS.update(**flags)
    with pytest.raises(ValueError, match=msg):
        check_attn_score()


@pytest.mark.parametrize("flags,msg", REFUSALS)
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


def test_existing_checks_keep_their_answers():
    from stochastic_gcn_amd import full_batch as fb
    FLAGS.update(**BOTH, attn_score='gat', attn_heads=4, attn_dropout=0.2)
    assert fb.check_aggregator() is False and fb.check_attention() == (True, 0.0)
    assert fb.check_attn_heads() == 4 and fb.check_attn_dropout() == 0.2


@pytest.mark.parametrize("extra", [dict(attn_score='gat'), dict(attn_score='gat', attn_heads=4, attn_slope=0.1), dict(attn_score='dot')])
def test_accepted_combination_reaches_the_device_check(monkeypatch, extra):
    from stochastic_gcn_amd import train
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    FLAGS.update(**BOTH, **extra)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        train.Trainer(verbose=False)


# ---- the parameter layout ----------------------------------------------------------------------------------------------------
def _model(name, **extra):
    import attn_aggregator_cases as ac
    from stochastic_gcn_amd.plaingcn import PlainGCN
    case = ac.build(name)
    fl = case['flags']
    FLAGS.reset()
    FLAGS.update(**{k: v for k, v in fl.items() if hasattr(FLAGS, k)})
    FLAGS.update(**BOTH, **extra)
    return PlainGCN(fl['num_layers'], fl['preprocess'], case['ph'], case['feats'], case['nbr_train'], case['train_adj'], False,
                    multitask=False, is_training=True, device=torch.device('cpu'))


@pytest.mark.parametrize("name", ["sage_ln_pp", "gcn_nopp"])
def test_dot_is_the_run_without_the_flag(name):
    m0, m1 = _model(name), _model(name, attn_score='dot')
    assert m0._store.layout == m1._store.layout and m0._wd_range == m1._wd_range and m0._first_param == m1._first_param
    assert torch.equal(m0.theta, m1.theta)
    assert all(not l.param_shapes() for l in m1.aggregators)


def test_gat_layout_weight_decay_and_first_variable():
    m = _model("gcn_nopp", attn_score='gat', attn_heads=2)
    names = [n for n, _ in m._store.layout]
    assert names == ['agg0/attn_vec', 'dense0/weights', 'agg1/attn_vec', 'dense1/weights']
    assert dict(m._store.layout)['agg0/attn_vec'] == (2, 6) and dict(m._store.layout)['agg1/attn_vec'] == (2, 8)
    # weight decay: dense0/weights alone (6 x 8 floats behind the 12 of agg0/attn_vec); the first parametrised layer is agg0,
    # which needs no input gradient
    assert m._wd_range == (12, 60) and m.layers[m._first_param].name == 'agg0' and m.layers[m._first_param].need_dx is False
    assert m.aggregators[0].wd_vars() == [] and m.aggregators[1].need_dx is True
    a0 = m.aggregators[0].vars['attn_vec']
    lim = float(np.sqrt(6.0 / (2 + 6)))
    assert tuple(a0.shape) == (2, 6) and float(a0.abs().max()) <= lim and float(a0.abs().max()) > 0
    p = _model("sage_ln_pp", attn_score='gat')
    assert [n for n, _ in p._store.layout][:3] == ['dense0/weights', 'dense0/offset', 'dense0/scale']
    assert p._wd_range[0] == 0 and 'agg0/attn_vec' in dict(p._store.layout)


# ---- the exports ---------------------------------------------------------------------------------------------------------
NAMES = (("sgcn_gat_scores_f32", 8), ("sgcn_spgat_csr_f32", 20), ("sgcn_spgat_csr_bwd_u_f32", 24), ("sgcn_spgat_csr_bwd_v_f32", 27),
         ("sgcn_gat_scores_bwd_f32", 15))


def test_symbols_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "sgcn.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, nargs in NAMES:
        assert "int %s(" % name in src
        assert hasattr(lib, name) and name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == nargs
    assert _ffi.lib.sgcn_abi_version() == _ffi.ABI_VERSION == 16          # additive exports


A0 = 4096          # (non-null addresses that are never dereferenced: every call below fails validation first)


def _fwd(rowptr=A0, col=2 * A0, M=8, K=8, d=8, heads=2, keep=1.0, key=1, U=3 * A0, ldu=4, V=10 * A0, ldv=4, B=4 * A0, ldb=8, slope=0.2,
         C=5 * A0, ldc=8, lse=6 * A0, plan=None):
    return _ffi.lib.sgcn_spgat_csr_f32(rowptr, col, M, K, d, heads, keep, key, U, ldu, V, ldv, B, ldb, slope, C, ldc, lse, plan, None)


def _bwd_u(rowptr=A0, col=2 * A0, M=8, K=8, d=8, heads=2, keep=1.0, key=1, U=3 * A0, ldu=4, V=10 * A0, ldv=4, B=4 * A0, ldb=8,
           slope=0.2, G=5 * A0, ldg=8, C=6 * A0, ldc=8, lse=7 * A0, delta=8 * A0, dU=9 * A0, plan=None):
    return _ffi.lib.sgcn_spgat_csr_bwd_u_f32(rowptr, col, M, K, d, heads, keep, key, U, ldu, V, ldv, B, ldb, slope, G, ldg, C, ldc,
                                             lse, delta, dU, plan, None)


def _bwd_v(rowptr=A0, col=2 * A0, M=8, K=8, d=8, heads=2, keep=1.0, key=1, U=3 * A0, ldu=4, V=10 * A0, ldv=4, B=4 * A0, ldb=8,
           slope=0.2, G=5 * A0, ldg=8, lse=7 * A0, delta=8 * A0, dB=9 * A0, lddb=8, dV=11 * A0, add=None, ldadd=0, add_rows=0,
           plan=None):
    return _ffi.lib.sgcn_spgat_csr_bwd_v_f32(rowptr, col, K, M, d, heads, keep, key, U, ldu, V, ldv, B, ldb, slope, G, ldg, lse, delta,
                                             dB, lddb, dV, add, ldadd, add_rows, plan, None)


@pytest.mark.parametrize("fn", [_fwd, _bwd_u, _bwd_v])
def test_pattern_calls_validate_before_any_device_call(fn):
    err = _ffi.lib.sgcn_last_error
    for keep in (0.0, 1.5, float('nan')):
        assert fn(keep=keep) == -1 and b"keep must be finite and in (0, 1]" in err()
    for slope in (-0.1, 1.5, float('nan'), float('inf')):
        assert fn(slope=slope) == -1 and b"slope must lie in [0, 1]" in err()
    for keep in (0.8, 1.0):
        assert fn(keep=keep, heads=3) == -1 and b"heads must be one of 1/2/4/8" in err()
        assert fn(keep=keep, d=6, heads=4) == -1 and b"d = 6 is not a multiple of heads = 4" in err()
        assert fn(keep=keep, rowptr=None) == -1 and b"null operand" in err()
        assert fn(keep=keep, V=None) == -1 and b"null operand" in err()
        assert fn(keep=keep, d=0) == -1 and b"d must be positive" in err()
        assert fn(keep=keep, ldb=7) == -1 and b"leading dimension smaller than d" in err()
        assert fn(keep=keep, ldu=1) == -1 and b"score table pitch smaller than heads" in err()
        p = _ffi.Plan(4096, 8, None, 1, 3, None, 0)
        assert fn(keep=keep, plan=ctypes.byref(p)) == -1 and b"needs dev_fix/dev_ws" in err()
        lds = {k: 520 for k in ("ldb", "ldc", "ldg", "lddb") if k in fn.__code__.co_varnames}
        assert fn(keep=keep, d=520, heads=8, ldu=8, ldv=8, **lds) == -1 and b"over the limit of 256 columns at vector width 1" in err()
        lds = {k: 1028 for k in lds}
        assert fn(keep=keep, d=1028, heads=1, **lds) == -1 and b"over the limit of 1024 columns at vector width 4" in err()
    p = _ffi.Plan(4096, 8, 4096, 1, 3, 4096, 3 * 8 - 1)       # (the smallest slot of the three is 8 floats)
    assert fn(plan=ctypes.byref(p)) == -1 and b"workspace too small" in err()


def test_score_calls_validate_before_any_device_call():
    err = _ffi.lib.sgcn_last_error
    sc = lambda x=A0, ldx=8, rows=4, d=8, heads=2, a=2 * A0, S=3 * A0: _ffi.lib.sgcn_gat_scores_f32(x, ldx, rows, d, heads, a, S, None)
    assert sc(heads=3) == -1 and b"heads must be one of 1/2/4/8" in err()
    assert sc(d=6, heads=4) == -1 and b"not a multiple of heads" in err()
    assert sc(a=None) == -1 and b"null operand" in err()
    assert sc(ldx=7) == -1 and b"leading dimension smaller than d" in err()
    assert sc(rows=-1) == -1 and sc(d=0) == -1
    assert sc(rows=0, x=None, S=None) == 0

    def sb(x=A0, ldx=8, rows=100, rows_u=100, d=8, heads=2, a=2 * A0, dU=3 * A0, dV=4 * A0, dX=None, lddx=0, da=5 * A0, ws=6 * A0,
           ws_elems=2 * 2 * 8):
        return _ffi.lib.sgcn_gat_scores_bwd_f32(x, ldx, rows, rows_u, d, heads, a, dU, dV, dX, lddx, da, ws, ws_elems, None)
    assert sb(rows_u=101) == -1 and b"0 <= rows_u <= rows" in err()
    assert sb(heads=3) == -1 and b"heads must be one of 1/2/4/8" in err()
    assert sb(da=None) == -1 and b"null operand" in err()
    assert sb(dX=7 * A0, lddx=7) == -1 and b"leading dimension smaller than d" in err()
    assert sb(ws_elems=2 * 2 * 8 - 1) == -1 and b"workspace too small" in err()
    assert sb(ws=None) == -1 and b"workspace too small" in err()


def test_ops_refuse_bad_arguments_and_cpu_tensors():
    a = sp.identity(4, format='csr', dtype=np.float32)
    A = ops.DeviceCSR.from_scipy(a, torch.device("cpu"), with_plan=False)
    x, t = torch.zeros(4, 8), torch.zeros(4, 2)
    with pytest.raises(ValueError, match=r"slope must lie in \[0, 1\]"):
        ops.spgat(A, x, t, t, slope=1.5, heads=2)
    with pytest.raises(ValueError, match=r"keep must be finite and in \(0, 1\]"):
        ops.spgat(A, x, t, t, heads=2, keep=0.0)
    with pytest.raises(ValueError, match=r"slope must lie in \[0, 1\]"):
        ops.spgat_bwd(A, A, x, t, t, x, x, t, slope=float('nan'), heads=2)
    for fn in (lambda: ops.spgat(A, x, t, t, heads=2), lambda: ops.gat_scores(x, torch.zeros(2, 8), heads=2),
               lambda: ops.spgat_bwd(A, A, x, t, t, x, x, t, heads=2),
               lambda: ops.gat_scores_bwd(x, torch.zeros(2, 8), t, t, heads=2)):
        with pytest.raises(RuntimeError, match="HBM"):
            fn()


def test_static_matrix_refuses_what_attention_refuses():
    import sparse_cases as sc
    from stochastic_gcn_amd import full_batch
    m = full_batch.StaticMatrix(sc.pattern("m64_k64"), torch.device("cpu"), 'rows')
    x, a = torch.zeros(64, 8), torch.zeros(2, 8)
    with pytest.raises(ValueError, match="attention has no bfloat16-operand form"):
        m.gat_product(x.to(torch.bfloat16), a, 0.2)
    m.edge = full_batch.EdgeMask(0.2)
    with pytest.raises(ValueError, match="attention has no edge-masked form"):
        m.gat_product(x, a, 0.2)
    with pytest.raises(ValueError, match="attention has no edge-masked form"):
        m.gat_backward(x, a, None, x, x, None, 0.2)
