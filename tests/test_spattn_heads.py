"""CPU tests of --attn_heads: the per-head NumPy reference against the single-head definition on slices and central
differences, its bounds against fp32 restatements (accepted) and against the single-head result at the same width
(rejected -- the tests can tell one head from many), the flag and its refusals, the three multi-head exports' argument checks,
the head-aware vector width, and the well-posedness of the end-to-end cases.  Nothing here touches a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import spattn_heads_cases as cs
import spattn_heads_ref as href
import spattn_ref as ref
from stochastic_gcn_amd import _ffi, ops
from stochastic_gcn_amd.flags import _DEFS, FLAGS, _Flags
from test_spattn import _small_patterns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _reset_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


# ---- the reference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(_small_patterns()))
def test_reference_is_the_single_head_definition_on_slices(name):
    a = _small_patterns()[name]
    rng = np.random.RandomState(4)
    M, K = a.shape
    for d, H, scale in ((2, 2, 1.0), (6, 2, 0.4), (12, 4, -1.5), (8, 8, 0.7), (5, 1, 0.3)):
        Q, B = rng.standard_normal((M, d)).astype(np.float32), rng.standard_normal((K, d)).astype(np.float32)
        f = href.forward(a, Q, B, scale, H)
        assert f.C.shape == (M, d) and f.lse.shape == (M, H) and f.bound_C.shape == (M, d) and f.bound_lse.shape == (M, H)
        dh = d // H
        for h in range(H):
            C, lse = ref.forward_loops(a, Q[:, h * dh:(h + 1) * dh], B[:, h * dh:(h + 1) * dh], scale)
            assert np.allclose(f.C[:, h * dh:(h + 1) * dh], C, rtol=1e-13, atol=1e-14)
            assert np.allclose(f.lse[:, h], lse, rtol=1e-13, atol=1e-14)
        C, lse = href.forward_loops(a, Q, B, scale, H)
        assert np.allclose(f.C, C, rtol=1e-13, atol=1e-14) and np.allclose(f.lse, lse, rtol=1e-13, atol=1e-14)
        deg = np.diff(a.indptr)
        assert np.all(f.lse[deg == 0] == -np.inf) and np.all(f.C[deg == 0] == 0)
    # one head is spattn_ref itself
    f1, g1 = href.forward(a, Q, B, 0.3, 1), ref.forward(a, Q, B, 0.3)
    assert np.array_equal(f1.C, g1.C) and np.array_equal(f1.lse[:, 0], g1.lse) and np.array_equal(f1.bound_C, g1.bound_C)


def _central(fn, X, h=1e-6):
    num = np.zeros_like(X)
    for idx in np.ndindex(*X.shape):
        keep = X[idx]
        X[idx] = keep + h
        up = fn()
        X[idx] = keep - h
        down = fn()
        X[idx] = keep
        num[idx] = (up - down) / (2 * h)
    return num


def test_reference_backward_against_central_differences():
    a = _small_patterns()["m15_k17"]
    rng = np.random.RandomState(6)
    M, K, d, H, scale = a.shape[0], a.shape[1], 6, 2, 0.7
    Q, B, G = rng.standard_normal((M, d)), rng.standard_normal((K, d)), rng.standard_normal((M, d))
    r = href.backward_f64(a, Q, B, G, scale, H)
    worst = 0.0
    for X, got in ((Q, r['dQ']), (B, r['dB'])):
        worst = max(worst, float(np.max(np.abs(_central(lambda: href.loss_f64(a, Q, B, scale, G, H), X) - got))))
    print("largest deviation from central differences %.3e" % worst)
    assert worst < 1e-8
    # the fused form on a square pattern, four heads: Q = B[:M], one gradient; the addend lands on dQ's rows
    a = _small_patterns()["m16_k16"]
    d, H = 8, 4
    X, G, add = rng.standard_normal((16, d)), rng.standard_normal((16, d)), rng.standard_normal((16, d))
    r = href.backward_f64(a, X, X, G, scale, H, add=add, add_rows=9, fused=True)
    num = _central(lambda: href.loss_f64(a, X, X, scale, G, H), X)
    num[:9] += add[:9]
    worst = float(np.max(np.abs(num - r['dx'])))
    print("fused: largest deviation from central differences %.3e" % worst)
    assert worst < 1e-8


# ---- the bounds on the GPU test's own inputs ------------------------------------------------------------------------------------
# (the patterns whose every entry a Python loop can visit; the same arrays as tests/test_spattn_heads_gpu.py)
BOUND_CASES = [("row_lengths", 6, 2), ("row_lengths", 8, 8), ("row_lengths", 24, 4), ("row_lengths", 130, 2),
               ("m63_k65", 40, 8), ("m65_k63", 64, 8), ("m64_k64", 12, 4), ("m64_k64", 128, 4)]


@pytest.mark.parametrize("name,d,H", BOUND_CASES)
def test_bounds_accept_fp32_restatements_per_head(name, d, H):
    a, _ = cs.pattern(name)
    M = a.shape[0]
    Q, B, G, add = cs.general(name, d, H)
    empty = np.diff(a.indptr) == 0
    for scale, alias in cs.general_variants(name, d, H):
        q = B[:M] if alias else Q
        r = cs.general_ref(name, d, H, scale, alias, False)
        f = r['fwd']
        for kw in (dict(), dict(reverse=True, cut=True)):
            C, lse = href.forward_online_f32(a, q, B, scale, H, **kw)
            what = "%s d=%d H=%d scale=%.4g alias=%s %s" % (name, d, H, scale, alias, kw)
            assert np.all(np.abs(C - f.C) <= f.bound_C), what
            assert np.all(lse[empty] == -np.inf) and np.all(np.abs(lse[~empty] - f.lse[~empty]) <= f.bound_lse[~empty]), what
            dQ, dB = href.backward_f32(a, q, B, G, scale, C, lse, H, **kw)
            if alias:
                dx = dB.copy()
                dx[:M] = dx[:M] + dQ
                assert np.all(np.abs(dx - r['dx']) <= r['bound_dx']), what
            else:
                assert np.all(np.abs(dQ - r['dQ']) <= r['bound_dQ']), what
                assert np.all(np.abs(dB - r['dB']) <= r['bound_dB']), what


@pytest.mark.parametrize("name,d,H", BOUND_CASES + [("row_lengths", 2, 2), ("row_lengths", 128, 4), ("row_lengths", 1024, 8)])
def test_bounds_reject_the_single_head_result(name, d, H):
    """one softmax over the whole width is not H softmaxes over its slices: a kernel that ignored ``heads`` would be caught, in
    C and in the backward"""
    a, _ = cs.pattern(name)
    Q, B, G, add = cs.general(name, d, H)
    for scale, alias in cs.general_variants(name, d, H):
        if alias:
            continue
        r = cs.general_ref(name, d, H, scale, False, False)
        f = r['fwd']
        one = ref.backward_f64(a, Q, B, G, scale, values_only=True)
        assert np.any(np.abs(one['fwd'].C - f.C) > f.bound_C), (name, d, H, scale)
        assert np.any(np.abs(one['dQ'] - r['dQ']) > r['bound_dQ']) and np.any(np.abs(one['dB'] - r['dB']) > r['bound_dB'])
        # and heads in the wrong order are caught too: the reference with the heads' slices of Q swapped
        if H >= 2:
            dh = d // H
            Qs = Q.copy()
            Qs[:, :dh], Qs[:, dh:2 * dh] = Q[:, dh:2 * dh], Q[:, :dh]
            assert np.any(np.abs(href.forward(a, Qs, B, scale, H, values_only=True).C - f.C) > f.bound_C)


def test_exact_regimes_are_what_they_claim():
    """the winner-take-all inputs against the fp64 reference: the expected bits are the exact results, a different winner per head"""
    for name, d, H in (("row_lengths", 6, 2), ("m63_k65", 40, 8), ("row_lengths", 8, 8)):
        a, _ = cs.pattern(name)
        Q, B, G, add, C, lse, dB = cs.winner(name, d, H)
        r = href.backward_f64(a, Q, B, G, 1.0, H, values_only=True)
        near = lambda x, y: np.allclose(np.where(np.isfinite(y), x, 0), np.where(np.isfinite(y), y, 0), rtol=0, atol=1e-90) \
            and np.array_equal(np.isfinite(x), np.isfinite(y))
        assert near(r['fwd'].C, C.astype(np.float64)) and near(r['fwd'].lse, lse.astype(np.float64))
        assert near(r['dB'], dB.astype(np.float64)) and near(r['dQ'], np.zeros_like(r['dQ']))
        assert lse.shape == (a.shape[0], H)
        some = np.isfinite(lse[:, 0])
        assert any(np.any(lse[some, 0] != lse[some, h]) for h in range(1, H))       # the heads' winners differ


# ---- the flag -----------------------------------------------------------------------------------------------------------------
BOTH = dict(full_batch=True, test_full_batch=True, aggregator='attn')


def test_flag_default_parsing_and_help():
    from stochastic_gcn_amd.full_batch import ATTN_HEADS, check_attention, check_attn_heads
    f = _Flags()
    assert f.attn_heads == 1 and 'attn_heads' in f.as_dict() and check_attn_heads(f) == 1
    f.parse(['--full_batch', '--test_full_batch', '--aggregator', 'attn', '--attn_heads', '4'])
    assert f.attn_heads == 4 and check_attn_heads(f) == 4 and check_attention(f) == (True, 0.0)
    for H in (1, 2, 4, 8):
        FLAGS.update(**BOTH, attn_heads=H)
        assert check_attn_heads() == H
    assert ATTN_HEADS == ops.ATTN_HEADS == (1, 2, 4, 8)
    help_ = {name: h for name, _, _, h in _DEFS}
    assert '1/2/4/8' in help_['attn_heads'] and '1 / sqrt(d / H)' in help_['attn_heads']
    assert ('attn_heads', int, 1) == next(d[:3] for d in _DEFS if d[0] == 'attn_heads')


REFUSALS = [
    (dict(BOTH, attn_heads=3), r"--attn_heads must be one of 1/2/4/8, got 3"),
    (dict(BOTH, attn_heads=0), r"--attn_heads must be one of 1/2/4/8, got 0"),
    (dict(BOTH, attn_heads=16), r"--attn_heads must be one of 1/2/4/8, got 16"),
    (dict(BOTH, attn_heads=-2), r"--attn_heads must be one of 1/2/4/8, got -2"),
    (dict(attn_heads=2), r"--attn_heads needs --aggregator attn"),
    (dict(full_batch=True, test_full_batch=True, aggregator='max', attn_heads=4), r"--attn_heads needs --aggregator attn"),
]


@pytest.mark.parametrize("flags,msg", REFUSALS)
def test_refusals(flags, msg):
    from stochastic_gcn_amd.full_batch import check_attn_heads
    FLAGS.update(**flags)
    with pytest.raises(ValueError, match=msg):
        check_attn_heads()


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


@pytest.mark.parametrize("extra", [dict(attn_heads=1), dict(attn_heads=2), dict(attn_heads=8, attn_scale=0.3)])
def test_accepted_combination_reaches_the_device_check(monkeypatch, extra):
    from stochastic_gcn_amd import train
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    FLAGS.update(**BOTH, **extra)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        train.Trainer(verbose=False)


def test_heads_must_divide_the_width():
    from stochastic_gcn_amd.full_batch import attn_heads_divide
    attn_heads_divide(4, 32, "x")
    with pytest.raises(ValueError, match=r"--attn_heads 4 does not divide the input width of layer one \(30 columns\)"):
        attn_heads_divide(4, 30, "layer one")


def test_vector_width_rule_with_heads():
    t = lambda rows, pitch, d, off=0: torch.zeros(rows * pitch + off)[off:].view(rows, pitch)[:, :d]
    assert ops.attn_vw(24, t(3, 24, 24), heads=4) == 2              # dh = 6
    assert ops.attn_vw(130, t(3, 130, 130), heads=2) == 1           # dh = 65
    assert ops.attn_vw(130, t(3, 132, 130), heads=2) == 1
    assert ops.attn_vw(8, t(3, 8, 8), heads=2) == 4                 # one float4 per head
    assert ops.attn_vw(8, t(3, 8, 8), heads=8) == 1 and ops.attn_vw(8, t(3, 8, 8), heads=4) == 2
    assert ops.attn_vw(8, t(3, 8, 8, off=2), heads=2) == 2          # the pointers still count
    assert ops.attn_vw(24, t(3, 24, 24)) == 4 and ops.attn_vw(24, t(3, 24, 24), heads=1) == 4
    assert all(cs.head_vw(d, H, 4) == ops.attn_vw(d, heads=H) for d, H in cs.HD)
    with pytest.raises(ValueError, match="heads must be one of 1/2/4/8"):
        ops._attn_heads(8, 3)
    with pytest.raises(ValueError, match="not a multiple of heads = 8"):
        ops._attn_heads(12, 8)


def test_static_matrix_keeps_its_refusals_with_heads():
    import sparse_cases as sc
    from stochastic_gcn_amd import full_batch
    a = sc.pattern("m64_k64")
    x = torch.zeros(64, 8)
    m = full_batch.StaticMatrix(a, torch.device("cpu"), 'rows', bf16=True)
    with pytest.raises(ValueError, match="attention has no bfloat16-operand form"):
        m.attn_product(x, 1.0, heads=2)
    with pytest.raises(ValueError, match="attention has no bfloat16-operand form"):
        m.attn_backward(x, x, x, torch.zeros(64, 2), 1.0, heads=2)
    m = full_batch.StaticMatrix(a, torch.device("cpu"), 'rows')
    m.edge = full_batch.EdgeMask(0.2)
    with pytest.raises(ValueError, match="attention has no edge-masked form"):
        m.attn_product(x, 1.0, heads=2)


# ---- the end-to-end cases of tests/test_attn_heads_model_gpu.py are well-posed (decided here, without a device) ----------------
@pytest.mark.parametrize("name", ["sage_ln_pp_h2", "sage_ln_pp_h8", "gcn_nopp_h2"])
def test_end_to_end_cases_are_well_posed(name):
    import attn_heads_cases as hx
    c = hx.CASES[name]
    assert c['init'] == hx.scan(name)                        # the FIRST seed of 3 .. 12 that satisfies the condition
    m = hx.margin(name, c['init'])
    print("%s: init %d, smallest non-zero |ReLU input| / largest input %.3e (needs >= %.0e)" % (name, c['init'], m, hx.MARGIN))
    assert m >= hx.MARGIN == 1e-4
    assert c['init'] in hx.SEEDS and list(hx.SEEDS) == list(range(3, 13))
    case = hx.build(name)
    assert case['flags']['hidden1'] == 8 and 8 % c['heads'] == 0 and (case['flags']['preprocess'] or case['feats'].shape[1] % c['heads'] == 0)


def test_reference_model_scale_is_per_head():
    from attn_aggregator_ref import layer_scale
    import attn_heads_cases as hx
    case = hx.build('sage_ln_pp_h2')
    om = hx.reference_model(case, case['nbr_train'])
    assert om.heads == 2 and layer_scale(8 // 2) == float(np.float32(4 ** -0.5))


# ---- the exports ---------------------------------------------------------------------------------------------------------
NAMES = (("sgcn_spattn_mh_csr_f32", 16), ("sgcn_spattn_mh_csr_bwd_q_f32", 24), ("sgcn_spattn_mh_csr_bwd_kv_f32", 22))


def test_symbols_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "sgcn.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, nargs in NAMES:
        assert "int %s(" % name in src
        assert hasattr(lib, name) and name in _ffi.SIGNATURES
        sig = _ffi.SIGNATURES[name][1]
        assert len(sig) == nargs
        old = _ffi.SIGNATURES[name.replace("_mh_", "_")][1]
        assert sig[:5] == old[:5] and sig[5] is ctypes.c_int32 and sig[6:] == old[5:]      # `heads` directly after d
    version = src[src.index("v16 packed minibatch"):src.index("int sgcn_abi_version")]
    assert all(name in version for name, _ in NAMES)
    assert "4*ceil(d/4) + 4*heads" in src and "4*ceil(d/4) + 4" in src and "[i*heads + h]" in src
    assert _ffi.lib.sgcn_abi_version() == _ffi.ABI_VERSION == 16          # additive exports


def _plan(nfix, nslots, ws, ws_elems, seg=4096, nseg=8, fix=8192):
    return _ffi.Plan(seg, nseg, fix if nfix else None, nfix, nslots, ws, ws_elems)


A0 = 4096          # (non-null addresses that are never dereferenced: every call below fails validation first)


def _fwd(rowptr=A0, col=2 * A0, M=8, K=8, d=8, heads=2, Q=3 * A0, ldq=8, B=4 * A0, ldb=8, scale=1.0, C=5 * A0, ldc=8, lse=6 * A0,
         plan=None):
    return _ffi.lib.sgcn_spattn_mh_csr_f32(rowptr, col, M, K, d, heads, Q, ldq, B, ldb, scale, C, ldc, lse, plan, None)


def _bwd_q(rowptr=A0, col=2 * A0, M=8, K=8, d=8, heads=2, Q=3 * A0, ldq=8, B=4 * A0, ldb=8, scale=1.0, G=5 * A0, ldg=8, C=6 * A0,
           ldc=8, lse=7 * A0, delta=8 * A0, dQ=9 * A0, lddq=8, add=None, ldadd=0, add_rows=0, plan=None):
    return _ffi.lib.sgcn_spattn_mh_csr_bwd_q_f32(rowptr, col, M, K, d, heads, Q, ldq, B, ldb, scale, G, ldg, C, ldc, lse, delta, dQ,
                                                 lddq, add, ldadd, add_rows, plan, None)


def _bwd_kv(rowptr=A0, row=2 * A0, K=8, M=8, d=8, heads=2, Q=3 * A0, ldq=8, B=4 * A0, ldb=8, scale=1.0, G=5 * A0, ldg=8,
            lse=7 * A0, delta=8 * A0, dB=9 * A0, lddb=8, add=None, ldadd=0, add_rows=0, plan=None):
    return _ffi.lib.sgcn_spattn_mh_csr_bwd_kv_f32(rowptr, row, K, M, d, heads, Q, ldq, B, ldb, scale, G, ldg, lse, delta, dB, lddb,
                                                  add, ldadd, add_rows, plan, None)


@pytest.mark.parametrize("fn", [_fwd, _bwd_q, _bwd_kv])
def test_heads_are_validated_before_any_device_call(fn):
    err = _ffi.lib.sgcn_last_error
    for H in (0, -1, 3, 5, 6, 7, 16, 64):
        assert fn(heads=H) == -1 and b"heads must be one of 1/2/4/8" in err()
    ld = {k: 12 for k in ("ldq", "ldb", "ldc", "ldg", "lddq", "lddb") if k in fn.__code__.co_varnames}
    assert fn(d=12, heads=8, **ld) == -1 and b"d = 12 is not a multiple of heads = 8" in err()
    assert fn(d=6, heads=4) == -1 and b"d = 6 is not a multiple of heads = 4" in err()


def test_forward_validates_before_any_device_call():
    err = _ffi.lib.sgcn_last_error
    for kw in (dict(rowptr=None), dict(Q=None), dict(B=None), dict(C=None)):
        assert _fwd(**kw) == -1 and b"null operand" in err()
    for d in (0, -3):
        assert _fwd(d=d) == -1 and b"d must be positive" in err()
    for kw in (dict(ldq=7), dict(ldb=7), dict(ldc=7)):
        assert _fwd(**kw) == -1 and b"leading dimension smaller than d" in err()
    for s in (float('nan'), float('inf'), -float('inf')):
        assert _fwd(scale=s) == -1 and b"scale must be finite" in err()
    assert _fwd(M=-1) == -1 and b"negative size" in err()
    p = _plan(2, 6, None, 0)
    assert _fwd(plan=ctypes.byref(p)) == -1 and b"needs dev_fix/dev_ws" in err()
    # a forward slot: 4 ceil(d / 4) + 4 heads floats -- 16 at (8, 2), 40 at (8, 8), 12 at (8, 1)
    for H, slot in ((2, 16), (8, 40), (1, 12), (4, 24)):
        p = _plan(2, 6, 6 * A0, 6 * slot - 1)
        assert _fwd(heads=H, plan=ctypes.byref(p)) == -1 and b"workspace too small" in err()
        assert ("(%d < %d floats)" % (6 * slot - 1, 6 * slot)).encode() in err()
    p = _plan(0, 0, None, 0, nseg=7)
    assert _fwd(plan=ctypes.byref(p)) == -1 and b"malformed plan" in err()
    # the width limit, 256 * VW with the head-aware VW, named in the message together with the rule
    assert _fwd(d=520, heads=8, ldq=520, ldb=520, ldc=520) == -1 and b"over the limit of 256 columns at vector width 1" in err()
    assert b"VW must also divide d / heads = 65" in err()
    assert _fwd(d=516, heads=4, ldq=516, ldb=516, ldc=516) == -1 and b"over the limit of 256 columns at vector width 1" in err()
    assert b"VW must also divide d / heads = 129" in err()
    assert _fwd(d=1028, heads=2, ldq=1028, ldb=1028, ldc=1028) == -1 and b"over the limit of 512 columns at vector width 2" in err()
    assert _fwd(d=1032, heads=2, ldq=1032, ldb=1032, ldc=1032) == -1 and b"over the limit of 1024 columns at vector width 4" in err()
    assert _fwd(d=516, heads=2, ldq=518, ldb=518, ldc=518) == -1 and b"over the limit of 512 columns at vector width 2" in err()
    assert _fwd(M=0, Q=None) == 0                                                                   # no rows: nothing to do
    assert _fwd(M=0, Q=None, lse=None, heads=8) == 0


def test_backward_validates_before_any_device_call():
    err = _ffi.lib.sgcn_last_error
    for kw in (dict(rowptr=None), dict(Q=None), dict(B=None), dict(G=None), dict(C=None), dict(lse=None), dict(delta=None), dict(dQ=None)):
        assert _bwd_q(**kw) == -1 and b"null operand" in err()
    for kw in (dict(rowptr=None), dict(Q=None), dict(B=None), dict(G=None), dict(lse=None), dict(delta=None), dict(dB=None)):
        assert _bwd_kv(**kw) == -1 and b"null operand" in err()
    for fn, lds in ((_bwd_q, ("ldq", "ldb", "ldg", "ldc", "lddq")), (_bwd_kv, ("ldq", "ldb", "ldg", "lddb"))):
        for d in (0, -1):
            assert fn(d=d) == -1 and b"d must be positive" in err()
        for ld in lds:
            assert fn(**{ld: 7}) == -1 and b"leading dimension smaller than d" in err()
        assert fn(scale=float('nan')) == -1 and b"scale must be finite" in err()
        assert fn(add=6 * A0, ldadd=7, add_rows=4) == -1 and b"bad addend" in err()
        assert fn(add=6 * A0, ldadd=8, add_rows=9) == -1 and b"bad addend" in err()
        p = _plan(1, 3, None, 0)
        assert fn(plan=ctypes.byref(p)) == -1 and b"needs dev_fix/dev_ws" in err()
        for H in (2, 8):                                                      # a backward slot stays 4 ceil(d / 4) floats
            p = _plan(1, 3, 6 * A0, 3 * 8 - 1)
            assert fn(heads=H, plan=ctypes.byref(p)) == -1 and b"workspace too small" in err()
        kw = {ld: 520 for ld in lds}
        assert fn(d=520, heads=8, **kw) == -1 and b"over the limit of 256 columns at vector width 1" in err()
        assert b"VW must also divide d / heads = 65" in err()
    assert _bwd_q(M=0, Q=None, G=None, C=None, lse=None, delta=None) == 0
    assert _bwd_kv(K=0, B=None) == 0


def test_ops_refuse_cpu_tensors_with_heads():
    import scipy.sparse as sp
    a = sp.identity(4, format='csr', dtype=np.float32)
    A = ops.DeviceCSR.from_scipy(a, torch.device("cpu"), with_plan=False)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.spattn(A, torch.zeros(4, 8), scale=1.0, heads=2)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.spattn_bwd(A, A, torch.zeros(4, 8), None, torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4, 2), 1.0, heads=2)
