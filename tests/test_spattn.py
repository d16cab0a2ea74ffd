"""CPU tests of --aggregator attn: the NumPy reference of softmax dot-product attention over a CSR pattern against brute
force and central differences, its error bounds against fp32 restatements (accepted) and wrong results (rejected) on the
GPU test's own inputs, the flags and their refusals, and the three exports' argument checks.  Nothing here touches a
device."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import sparse_cases as sc
import spattn_cases as cs
import spattn_ref as ref
from stochastic_gcn_amd import _ffi, ops
from stochastic_gcn_amd.flags import _DEFS, FLAGS, _Flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _reset_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


# ---- the reference against brute force and central differences ------------------------------------------------------------
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


@pytest.mark.parametrize("name", sorted(_small_patterns()))
def test_reference_forward_against_brute_force(name):
    a = _small_patterns()[name]
    rng = np.random.RandomState(3)
    M, K = a.shape
    for d, scale in ((1, 1.0), (5, 0.4), (5, -1.5), (5, 0.0)):
        Q, B = rng.standard_normal((M, d)).astype(np.float32), rng.standard_normal((K, d)).astype(np.float32)
        f = ref.forward(a, Q, B, scale)
        C, lse = ref.forward_loops(a, Q, B, scale)
        assert np.allclose(f.C, C, rtol=1e-13, atol=1e-14) and np.allclose(f.lse, lse, rtol=1e-13, atol=1e-14)
        deg = np.diff(a.indptr)
        assert np.all(f.lse[deg == 0] == -np.inf) and np.all(f.C[deg == 0] == 0) and np.all(f.bound_C[deg == 0] == 0)
        if f.p.size:                             # the weights of a row sum to one; one neighbour: its row itself
            assert np.allclose(np.add.reduceat(f.p, a.indptr[:-1][deg > 0]), 1.0, rtol=1e-13)
            one = np.nonzero(deg == 1)[0]
            assert np.allclose(f.C[one], B[a.indices[a.indptr[one]]].astype(np.float64), rtol=1e-14, atol=0)


def test_reference_backward_against_central_differences():
    """an unsymmetric pattern, fp64 tables: d sum(G * C) / dQ and / dB by central differences"""
    a = _small_patterns()["m15_k17"]
    rng = np.random.RandomState(5)
    M, K, d, scale, h = a.shape[0], a.shape[1], 3, 0.7, 1e-6
    Q, B, G = rng.standard_normal((M, d)), rng.standard_normal((K, d)), rng.standard_normal((M, d))
    r = ref.backward_f64(a, Q, B, G, scale)
    worst = 0.0
    for X, got in ((Q, r['dQ']), (B, r['dB'])):
        num = np.zeros_like(X)
        for idx in np.ndindex(*X.shape):
            keep = X[idx]
            X[idx] = keep + h
            up = ref.loss_f64(a, Q, B, scale, G)
            X[idx] = keep - h
            down = ref.loss_f64(a, Q, B, scale, G)
            X[idx] = keep
            num[idx] = (up - down) / (2 * h)
        worst = max(worst, float(np.max(np.abs(num - got))))
    print("largest deviation from central differences %.3e" % worst)
    assert worst < 1e-8
    # the fused form on a square pattern: Q = B[:M], one gradient; the addend lands on dQ's rows
    a = _small_patterns()["m16_k16"]
    X, G, add = rng.standard_normal((16, d)), rng.standard_normal((16, d)), rng.standard_normal((16, d))
    r = ref.backward_f64(a, X, X, G, scale, add=add, add_rows=9, fused=True)
    num = np.zeros_like(X)
    for idx in np.ndindex(*X.shape):
        keep = X[idx]
        X[idx] = keep + h
        up = ref.loss_f64(a, X, X, scale, G)
        X[idx] = keep - h
        down = ref.loss_f64(a, X, X, scale, G)
        X[idx] = keep
        num[idx] = (up - down) / (2 * h)
    num[:9] += add[:9]
    assert float(np.max(np.abs(num - r['dx']))) < 1e-8


# ---- the bounds on the GPU test's own inputs: fp32 restatements pass, wrong results do not ----------------------------------
# (the patterns whose every entry a Python loop can visit; the same (Q, B, G, add) arrays as tests/test_spattn_gpu.py)
BOUND_CASES = [("row_lengths", 5), ("row_lengths", 33), ("row_lengths", 130), ("m63_k65", 128), ("m65_k63", 31),
               ("one_row", 130), ("identity", 1), ("permutation", 33)]


@pytest.mark.parametrize("name,d", BOUND_CASES)
def test_bounds_accept_fp32_restatements(name, d):
    a, _ = cs.pattern(name)
    M = a.shape[0]
    Q, B, G, add = cs.general(name, d)
    empty = np.diff(a.indptr) == 0
    for scale, alias in cs.general_variants(name, d):
        q = B[:M] if alias else Q
        r = cs.general_ref(name, d, scale, alias, False)
        f = r['fwd']
        for kw in (dict(), dict(reverse=True, cut=True)):
            C, lse = ref.forward_online_f32(a, q, B, scale, **kw)
            what = "%s d=%d scale=%.4g alias=%s %s" % (name, d, scale, alias, kw)
            assert np.all(np.abs(C - f.C) <= f.bound_C), what
            assert np.all(lse[empty] == -np.inf) and np.all(np.abs(lse[~empty] - f.lse[~empty]) <= f.bound_lse[~empty]), what
            dQ, dB = ref.backward_f32(a, q, B, G, scale, C, lse, **kw)
            if alias:
                dx = dB.copy()
                dx[:M] = dx[:M] + dQ
                assert np.all(np.abs(dx - r['dx']) <= r['bound_dx']), what
            else:
                assert np.all(np.abs(dQ - r['dQ']) <= r['bound_dQ']), what
                assert np.all(np.abs(dB - r['dB']) <= r['bound_dB']), what


@pytest.mark.parametrize("name,d", [("row_lengths", 33), ("row_lengths", 130), ("m63_k65", 128)])
def test_bounds_reject_wrong_results(name, d):
    """the reference with one stored entry of one row left out, and with scale multiplied by 1 + 2^-10: outside the bound,
    in C, lse, dQ and dB alike"""
    a, _ = cs.pattern(name)
    Q, B, G, add = cs.general(name, d)
    for scale, alias in cs.general_variants(name, d):
        if alias:
            continue
        r = cs.general_ref(name, d, scale, False, False)
        f = r['fwd']
        deg = np.diff(a.indptr)
        i = int(np.argmax(deg))                          # the longest row: leaving one entry out changes it least
        # the entry that goes is the row's runner-up by weight: at scale 1 the softmax is nearly saturated and most of a long
        # row's weights lie below fp32 resolution -- leaving such an entry out is no error any bound could see
        row = slice(a.indptr[i], a.indptr[i + 1])
        victim = int(np.argsort(f.p[row])[-2])
        less = a.copy().tolil()
        less[i, a.indices[a.indptr[i] + victim]] = 0
        less = less.tocsr()
        less.eliminate_zeros()
        assert less.nnz == a.nnz - 1
        for wrong in (ref.backward_f64(less, Q, B, G, scale), ref.backward_f64(a, Q, B, G, scale * (1 + 2.0 ** -10))):
            w = wrong['fwd']
            assert np.any(np.abs(w.C - f.C) > f.bound_C), (name, d, scale)
            assert np.any(np.abs(w.lse[deg > 0] - f.lse[deg > 0]) > f.bound_lse[deg > 0]), (name, d, scale)
            assert np.any(np.abs(wrong['dQ'] - r['dQ']) > r['bound_dQ']), (name, d, scale)
            assert np.any(np.abs(wrong['dB'] - r['dB']) > r['bound_dB']), (name, d, scale)


def test_exact_regimes_are_what_they_claim():
    """the uniform and the winner-take-all inputs against the fp64 reference: the expected bits are the exact results"""
    for name, d in (("row_lengths", 5), ("m63_k65", 128), ("one_row", 130)):
        a, _ = cs.pattern(name)
        Q, B, C, logn = cs.uniform(name, d)
        f = ref.forward(a, Q, B, 0.0)
        assert np.all(np.abs(C - f.C) <= ref.U * np.abs(f.C) + 1e-14)         # one rounding: the division (+ fp64's own noise)
        assert np.allclose(f.lse[np.diff(a.indptr) > 0], logn[np.diff(a.indptr) > 0], rtol=1e-15)
        Q, B, G, add, C, lse, dB = cs.winner(name, d)
        r = ref.backward_f64(a, Q, B, G, 1.0, values_only=True)
        # (fp64 keeps exp(-256) = 1e-111 where fp32 has an exact 0: equal up to that)
        near = lambda x, y: np.allclose(np.where(np.isfinite(y), x, 0), np.where(np.isfinite(y), y, 0), rtol=0, atol=1e-90) \
            and np.array_equal(np.isfinite(x), np.isfinite(y))
        assert near(r['fwd'].C, C.astype(np.float64)) and near(r['fwd'].lse, lse.astype(np.float64))
        assert near(r['dB'], dB.astype(np.float64)) and near(r['dQ'], np.zeros_like(r['dQ']))


# ---- the flags -------------------------------------------------------------------------------------------------------------
def test_flag_defaults_and_choices():
    from stochastic_gcn_amd.flags import _CHOICES
    from stochastic_gcn_amd.full_batch import check_aggregator, check_attention
    f = _Flags()
    assert f.aggregator == 'sum' and f.attn_scale == 0.0 and 'attn_scale' in f.as_dict()
    assert _CHOICES['aggregator'] == ('sum', 'max', 'attn')
    assert check_attention(f) == (False, 0.0) and check_aggregator(f) is False
    f.parse(['--full_batch', '--test_full_batch', '--aggregator', 'attn'])
    assert f.aggregator == 'attn' and check_attention(f) == (True, 0.0) and check_aggregator(f) is False
    f.parse(['--full_batch', '--test_full_batch', '--aggregator', 'attn', '--attn_scale', '0.25'])
    assert check_attention(f) == (True, 0.25)
    with pytest.raises(SystemExit):
        _Flags().parse(['--aggregator', 'mean'])
    FLAGS.update(aggregator='mean')
    with pytest.raises(ValueError, match="--aggregator must be one of sum/max/attn"):
        check_attention()
    FLAGS.update(aggregator='max', full_batch=True, test_full_batch=True)      # max: nothing for attention to refuse
    assert check_attention() == (False, 0.0) and check_aggregator() is True
    help_ = {name: h for name, _, _, h in _DEFS}
    assert '--preprocess' in help_['aggregator'] and 'weighted sum' in help_['aggregator'] and 'attn' in help_['aggregator']
    assert '1 / sqrt(d)' in help_['attn_scale']


BOTH = dict(full_batch=True, test_full_batch=True, aggregator='attn')
REFUSALS = [
    (dict(aggregator='attn'), "--aggregator attn needs --full_batch and --test_full_batch"),
    (dict(aggregator='attn', full_batch=True), "--aggregator attn needs --full_batch and --test_full_batch"),
    (dict(aggregator='attn', test_full_batch=True), "--aggregator attn needs --full_batch and --test_full_batch"),
    (dict(BOTH, full_batch_dtype='bf16'), "--aggregator attn is not supported with --full_batch_dtype bf16"),
    (dict(BOTH, dense_dtype='bf16', feature_dtype='bf16'), "--aggregator attn is not supported with --feature_dtype bf16"),
    (dict(BOTH, edge_dropout=0.2), "--aggregator attn is not supported with --edge_dropout"),
    (dict(BOTH, attn_scale=-0.5), "--attn_scale must be finite and >= 0"),
    (dict(BOTH, attn_scale=float('inf')), "--attn_scale must be finite and >= 0"),
    (dict(BOTH, attn_scale=float('nan')), "--attn_scale must be finite and >= 0"),
    (dict(attn_scale=0.5), "--attn_scale needs --aggregator attn"),
    (dict(full_batch=True, test_full_batch=True, aggregator='max', attn_scale=0.5), "--attn_scale needs --aggregator attn"),
]


@pytest.mark.parametrize("flags,msg", REFUSALS)
def test_refusals(flags, msg):
    from stochastic_gcn_amd.full_batch import check_aggregator, check_attention
    FLAGS.update(**flags)
    with pytest.raises(ValueError, match=msg):
        check_attention()
    if flags.get('aggregator') == 'attn':          # check_aggregator validates attn too (and answers `maximum?` otherwise)
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


@pytest.mark.parametrize("extra", [dict(), dict(attn_scale=0.3), dict(dense_dtype='bf16')])
def test_accepted_combination_reaches_the_device_check(monkeypatch, extra):
    from stochastic_gcn_amd import train
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    FLAGS.update(**BOTH, **extra)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        train.Trainer(verbose=False)


def test_model_matrix_builds_no_sweep_plan_under_attn():
    """A model whose aggregations are all attention reads the row CSR only: 'rows' whatever --full_batch_kernel says."""
    from stochastic_gcn_amd import full_batch

    class Model(object):
        L, agg0_dim = 2, 64
    a = sc.pattern("m64_k64")
    FLAGS.update(**BOTH, full_batch_kernel='cs')
    m = full_batch.model_matrix(a, torch.device("cpu"), Model(), products=1000)
    assert m.kernel == 'rows' and m._plan is None


def test_static_matrix_refuses_bf16_and_edge_masks():
    from stochastic_gcn_amd import full_batch
    a = sc.pattern("m64_k64")
    x = torch.zeros(64, 8)
    m = full_batch.StaticMatrix(a, torch.device("cpu"), 'rows', bf16=True)
    with pytest.raises(ValueError, match="attention has no bfloat16-operand form"):
        m.attn_product(x, 1.0)
    with pytest.raises(ValueError, match="attention has no bfloat16-operand form"):
        m.attn_backward(x, x, x, torch.zeros(64), 1.0)
    m = full_batch.StaticMatrix(a, torch.device("cpu"), 'rows')
    with pytest.raises(ValueError, match="attention has no bfloat16-operand form"):
        m.attn_product(x.to(torch.bfloat16), 1.0)
    m.edge = full_batch.EdgeMask(0.2)
    with pytest.raises(ValueError, match="attention has no edge-masked form"):
        m.attn_product(x, 1.0)


def test_vector_width_rule():
    t = lambda rows, pitch, d, off=0: torch.zeros(rows * pitch + off)[off:].view(rows, pitch)[:, :d]
    assert ops.attn_vw(602, t(3, 602, 602)) == 2 and ops.attn_vw(602, t(3, 604, 602)) == 4
    assert ops.attn_vw(602, t(3, 604, 602), t(3, 603, 602)) == 1
    assert ops.attn_vw(8, t(3, 8, 8, off=2)) == 2 and ops.attn_vw(8, t(3, 8, 8, off=1)) == 1
    assert ops.attn_vw(8, t(3, 8, 8), None) == 4
    assert ops.ATTN_MAX_VECTORS == 256


# ---- the end-to-end cases of tests/test_attn_aggregator_gpu.py are well-posed (decided here, without a device) -----------------
@pytest.mark.parametrize("name", ["sage_ln_pp", "gcn_nopp"])
def test_end_to_end_cases_are_well_posed(name):
    import attn_aggregator_cases as ax
    c = ax.CASES[name]
    assert c['init'] == ax.scan(name)                        # the FIRST seed of 3 .. 12 that satisfies the condition
    m = ax.margin(name, c['init'])
    print("%s: init %d, smallest non-zero |ReLU input| / largest input %.3e (needs >= %.0e)" % (name, c['init'], m, ax.MARGIN))
    assert m >= ax.MARGIN
    assert c['init'] in ax.SEEDS and c['n'] <= 500 and c['flags']['hidden1'] == 8


def test_reference_model_scale_is_the_layers():
    from attn_aggregator_ref import layer_scale
    assert layer_scale(8) == float(np.float32(8 ** -0.5)) and layer_scale(602, 0.25) == 0.25


# ---- the exports ---------------------------------------------------------------------------------------------------------
NAMES = (("sgcn_spattn_csr_f32", 15), ("sgcn_spattn_csr_bwd_q_f32", 23), ("sgcn_spattn_csr_bwd_kv_f32", 21))


def test_symbols_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "sgcn.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, nargs in NAMES:
        assert "int %s(" % name in src
        assert hasattr(lib, name) and name in _ffi.SIGNATURES
        assert len(_ffi.SIGNATURES[name][1]) == nargs
    version = src[src.index("v16 packed minibatch"):src.index("int sgcn_abi_version")]
    assert all(name in version for name, _ in NAMES)
    assert "acc / l" in src and "4*ceil(d/4) + 4" in src
    assert _ffi.lib.sgcn_abi_version() == _ffi.ABI_VERSION == 16          # additive exports


def _plan(nfix, nslots, ws, ws_elems, seg=4096, nseg=8, fix=8192):
    return _ffi.Plan(seg, nseg, fix if nfix else None, nfix, nslots, ws, ws_elems)


A0 = 4096          # (non-null addresses that are never dereferenced: every call below fails validation first)


def _fwd(rowptr=A0, col=2 * A0, M=8, K=8, d=8, Q=3 * A0, ldq=8, B=4 * A0, ldb=8, scale=1.0, C=5 * A0, ldc=8, lse=6 * A0, plan=None):
    return _ffi.lib.sgcn_spattn_csr_f32(rowptr, col, M, K, d, Q, ldq, B, ldb, scale, C, ldc, lse, plan, None)


def _bwd_q(rowptr=A0, col=2 * A0, M=8, K=8, d=8, Q=3 * A0, ldq=8, B=4 * A0, ldb=8, scale=1.0, G=5 * A0, ldg=8, C=6 * A0, ldc=8,
           lse=7 * A0, delta=8 * A0, dQ=9 * A0, lddq=8, add=None, ldadd=0, add_rows=0, plan=None):
    return _ffi.lib.sgcn_spattn_csr_bwd_q_f32(rowptr, col, M, K, d, Q, ldq, B, ldb, scale, G, ldg, C, ldc, lse, delta, dQ, lddq,
                                              add, ldadd, add_rows, plan, None)


def _bwd_kv(rowptr=A0, row=2 * A0, K=8, M=8, d=8, Q=3 * A0, ldq=8, B=4 * A0, ldb=8, scale=1.0, G=5 * A0, ldg=8, lse=7 * A0,
            delta=8 * A0, dB=9 * A0, lddb=8, add=None, ldadd=0, add_rows=0, plan=None):
    return _ffi.lib.sgcn_spattn_csr_bwd_kv_f32(rowptr, row, K, M, d, Q, ldq, B, ldb, scale, G, ldg, lse, delta, dB, lddb,
                                               add, ldadd, add_rows, plan, None)


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
    p = _plan(2, 6, 6 * A0, 6 * 12 - 1)                                   # a forward slot: 4 ceil(d / 4) + 4 floats
    assert _fwd(plan=ctypes.byref(p)) == -1 and b"workspace too small" in err()
    p = _plan(2, 6, 6 * A0, 6 * 12)
    assert _fwd(d=9, ldq=9, ldb=9, ldc=9, plan=ctypes.byref(p)) == -1 and b"workspace too small" in err()       # ldw = 16
    p = _plan(0, 0, None, 0, nseg=7)
    assert _fwd(plan=ctypes.byref(p)) == -1 and b"malformed plan" in err()
    # the width limit, 256 * VW, named in the message: VW = 4, 2 and 1 by pitch and by base alignment
    assert _fwd(d=1025, ldq=1028, ldb=1028, ldc=1028) == -1 and b"over the limit of 1024 columns at vector width 4" in err()
    assert _fwd(d=513, ldq=514, ldb=516, ldc=516) == -1 and b"over the limit of 512 columns at vector width 2" in err()
    assert _fwd(d=513, ldq=516, ldb=516, ldc=516, C=5 * A0 + 8) == -1 and b"over the limit of 512 columns" in err()
    assert _fwd(d=257, ldq=257, ldb=260, ldc=260) == -1 and b"over the limit of 256 columns at vector width 1" in err()
    assert _fwd(M=0, Q=None) == 0                                                                   # no rows: nothing to do
    assert _fwd(M=0, Q=None, lse=None) == 0


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
        p = _plan(1, 3, 6 * A0, 3 * 8 - 1)                                # a backward slot: 4 ceil(d / 4) floats
        assert fn(plan=ctypes.byref(p)) == -1 and b"workspace too small" in err()
        kw = {ld: 1028 for ld in lds}
        assert fn(d=1025, **kw) == -1 and b"over the limit of 1024 columns" in err()
    assert _bwd_q(M=0, Q=None, G=None, C=None, lse=None, delta=None) == 0
    assert _bwd_kv(K=0, B=None) == 0


def test_ops_refuse_cpu_tensors_and_duplicate_columns():
    a = sp.identity(4, format='csr', dtype=np.float32)
    A = ops.DeviceCSR.from_scipy(a, torch.device("cpu"), with_plan=False)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.spattn(A, torch.zeros(4, 8), scale=1.0)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.spattn(A, torch.zeros(4, 8), q=torch.zeros(4, 8), scale=1.0)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.spattn_bwd(A, A, torch.zeros(4, 8), None, torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4), 1.0)
    for cols in ([0, 2, 2, 3, 1], [2, 0, 2, 3, 1]):
        dup = ops.DeviceCSR.from_arrays((2, 4), [0, 3, 5], cols, np.ones(5, np.float32), torch.device("cpu"), with_plan=False)
        with pytest.raises(ValueError, match="unique column ids"):
            ops.spattn(dup, torch.zeros(4, 8), scale=1.0)
