"""Dropout on the attention coefficients (--attn_dropout) without a device: the mask's NumPy restatement against
ops.attn_kept and its statistics, the fp64 reference of tests/spattn_drop_ref.py (its values against central differences, its
bounds against fp32 restatements they must accept and wrong results they must reject), the preconditions of the GPU cases, the
flag, and the validation of the three new exports through addresses that are never dereferenced."""
import ctypes
import os

import numpy as np
import pytest
import torch

import spattn_cases as cs1
import spattn_drop_cases as dc
import spattn_drop_ref as dref
from stochastic_gcn_amd import _ffi, ops
from stochastic_gcn_amd.flags import _DEFS, FLAGS, _Flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = dref.U


@pytest.fixture(autouse=True)
def _reset_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


# ---- the mask --------------------------------------------------------------------------------------------------------------
def test_mask_restatement_equals_the_package_mask():
    rng = np.random.RandomState(7)
    n = 200000
    i = rng.randint(0, 2 ** 31 - 1, n)
    j = rng.randint(0, 2 ** 31 - 1, n)
    i[:1000], j[:1000] = rng.randint(0, 300, 1000), rng.randint(0, 300, 1000)        # small ids, and some on the diagonal
    j[:100] = i[:100]
    h = rng.randint(0, 8, n)
    for key, keep in ((0, 0.5), (0xFFFFFFFF, 0.8), (0x12345678, 0.9), (77, 0.999999), (5, 2.0 ** -20)):
        mine = dref.kept(i, j, h, key, keep)
        assert mine.dtype == bool and np.array_equal(mine, ops.attn_kept(i, j, h, key, keep))
    assert bool(ops.attn_kept(3, 4, 0, 9, 0.5)) == bool(dref.kept(3, 4, 0, 9, 0.5))    # scalars too
    for seed, layer, step in ((1, 0, 0), (123, 5, 977), (-7, 2, 2 ** 20), (2 ** 31 + 5, 11, 3)):
        assert ops.attn_key(seed, layer, step) == dref.attn_key(seed, layer, step) == ops.dropout_key(seed, ops.ATTN_SITE + layer, step)
    assert ops.ATTN_SITE == dref.ATTN_SITE == 0x4154544E
    assert "#define SGCN_ATTN_SITE 0x4154544E" in open(os.path.join(ROOT, "include", "sgcn.h")).read()
    # keep = 1 keeps everything but the one hash value 2^32 - 1 (the threshold saturates, as for sgcn_dropout_t)
    assert dref.threshold(1.0) == 0xFFFFFFFF and dref.threshold(0.5) == 2 ** 31 and dref.mk_value(0.5) == 2.0


@pytest.mark.parametrize("keep", [0.5, 0.8, 0.9])
def test_mask_statistics(keep):
    """10^6 sites: the kept fraction within 5 sigma of keep, sigma = sqrt(keep (1 - keep) / n); two masks that should be
    independent agree on keep^2 + (1 - keep)^2 of the sites, within the same 5 sigma"""
    n = 10 ** 6
    rng = np.random.RandomState(11)
    i, j = rng.randint(0, 1 << 20, n), rng.randint(0, 1 << 20, n)
    j = np.where(i == j, j + 1, j)                          # (i, j) against (j, i) needs two different sites
    tol = 5.0 * np.sqrt(keep * (1.0 - keep) / n)
    key = dref.attn_key(1, 3, 0)
    base = dref.kept(i, j, 0, key, keep)
    frac = float(base.mean())
    print("keep %.1f: kept fraction %.6f (tolerance %.6f)" % (keep, frac, tol))
    assert abs(frac - keep) <= tol
    both = keep ** 2 + (1.0 - keep) ** 2
    others = dict(head=dref.kept(i, j, 1, key, keep), step=dref.kept(i, j, 0, dref.attn_key(1, 3, 1), keep),
                  layer=dref.kept(i, j, 0, dref.attn_key(1, 4, 0), keep), transposed=dref.kept(j, i, 0, key, keep))
    for what, other in others.items():
        agree = float((base == other).mean())
        print("keep %.1f: agreement with another %s %.6f (independent: %.6f)" % (keep, what, agree, both))
        assert abs(agree - both) <= tol, what


# ---- the reference -------------------------------------------------------------------------------------------------------------
SMALL = [("m64_k64", 8, 1, 0.5), ("m64_k64", 8, 2, 0.5), ("m63_k65", 6, 2, 0.8), ("row_lengths", 8, 2, 0.8), ("row_lengths", 5, 1, 0.8)]


def _inputs(name, d, H, keep, key=9):
    a, _ = cs1.pattern(name)
    Q, B, G, add = cs1.general(name, d)
    return a, Q, B, G, add, float(np.float32(float(d // H) ** -0.5)), dref.mask(a, H, key, keep)


@pytest.mark.parametrize("name,d,H,keep", SMALL)
def test_reference_values_are_the_definition(name, d, H, keep):
    """backward_f64 / forward (the bounded forms) and ``values`` (the definition in a dozen lines) agree; without a mask both
    are tests/spattn_heads_ref.py; lse does not see the mask"""
    import spattn_heads_ref as href
    a, Q, B, G, add, scale, mk = _inputs(name, d, H, keep)
    assert 0 < (mk > 0).mean() < 1 and set(np.unique(mk)) == {0.0, dref.mk_value(keep)}
    v = dref.values(a, Q, B, G, scale, H, mk)
    r = dref.backward_f64(a, Q, B, G, scale, H, mk)
    for k, w in (('C', r['fwd'].C), ('lse', r['fwd'].lse), ('dQ', r['dQ']), ('dB', r['dB'])):
        assert np.allclose(v[k], w, rtol=1e-13, atol=1e-13), k
    plain = href.backward_f64(a, Q, B, G, scale, H)
    assert np.array_equal(r['fwd'].lse, plain['fwd'].lse) and np.array_equal(r['fwd'].bound_lse, plain['fwd'].bound_lse)
    ones = dref.backward_f64(a, Q, B, G, scale, H, np.ones_like(mk))
    for k in ('dQ', 'dB'):
        assert np.allclose(ones[k], plain[k], rtol=1e-13, atol=1e-13)
        assert np.all(ones['bound_' + k] >= plain['bound_' + k])           # (one more rounding per entry: never tighter)
    assert np.allclose(ones['fwd'].C, plain['fwd'].C, rtol=1e-13, atol=1e-13)


def _central(fn, X, idx, h=1e-5):
    X = np.array(X, np.float64)
    out = []
    for i in idx:
        old = X[i]
        X[i] = old + h
        up = fn(X)
        X[i] = old - h
        dn = fn(X)
        X[i] = old
        out.append((up - dn) / (2 * h))
    return np.array(out)


@pytest.mark.parametrize("name,d,H,keep", [("m64_k64", 4, 1, 0.5), ("m64_k64", 4, 2, 0.8), ("m63_k65", 6, 2, 0.5)])
def test_reference_backward_against_central_differences(name, d, H, keep):
    """L = sum(G * C) under a FIXED mask, differentiated numerically in fp64 (h = 1e-5: truncation ~ h^2 |L'''| ~ 1e-10,
    roundoff ~ 2^-53 |L| / h ~ 1e-10; tolerance 1e-7 (1 + |g|))"""
    a, Q, B, G, add, scale, mk = _inputs(name, d, H, keep)
    Q, B = np.asarray(Q, np.float64), np.asarray(B, np.float64)
    r = dref.backward_f64(a, Q, B, G, scale, H, mk, values_only=True)
    rng = np.random.RandomState(5)
    iq = [(int(rng.randint(Q.shape[0])), int(rng.randint(d))) for _ in range(16)]
    ib = [(int(rng.randint(B.shape[0])), int(rng.randint(d))) for _ in range(16)]
    gq = _central(lambda X: dref.loss_f64(a, X, B, scale, G, H, mk), Q, iq)
    gb = _central(lambda X: dref.loss_f64(a, Q, X, scale, G, H, mk), B, ib)
    wq, wb = np.array([r['dQ'][i] for i in iq]), np.array([r['dB'][i] for i in ib])
    assert np.any(wq != 0) and np.any(wb != 0)
    assert np.all(np.abs(gq - wq) <= 1e-7 * (1 + np.abs(wq))), np.abs(gq - wq).max()
    assert np.all(np.abs(gb - wb) <= 1e-7 * (1 + np.abs(wb))), np.abs(gb - wb).max()
    if a.shape[0] == a.shape[1]:                           # the fused form: Q is B[:M]
        fx = dref.backward_f64(a, B, B, G, scale, H, mk, fused=True, values_only=True)['dx']
        gx = _central(lambda X: dref.loss_f64(a, X, X, scale, G, H, mk), B, ib)
        wx = np.array([fx[i] for i in ib])
        assert np.all(np.abs(gx - wx) <= 1e-7 * (1 + np.abs(wx)))


def _ratio(got, want, bound):
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / np.maximum(bound, 1e-300)))


@pytest.mark.parametrize("name,d,H,keep", SMALL)
def test_bounds_accept_fp32_restatements_in_two_orders(name, d, H, keep):
    a, Q, B, G, add, scale, mk = _inputs(name, d, H, keep)
    r = dref.backward_f64(a, Q, B, G, scale, H, mk)
    f = r['fwd']
    some = f.deg > 0
    for reverse, cut in ((False, False), (True, True)):
        C, lse = dref.forward_online_f32(a, Q, B, scale, H, mk, reverse, cut)
        dQ, dB = dref.backward_f32(a, Q, B, G, scale, C, lse, H, mk, reverse, cut)
        ratios = dict(C=_ratio(C, f.C, f.bound_C), lse=_ratio(lse[some], f.lse[some], f.bound_lse[some]),
                      dQ=_ratio(dQ, r['dQ'], r['bound_dQ']), dB=_ratio(dB, r['dB'], r['bound_dB']))
        print("%s d=%d H=%d reverse=%s cut=%s: worst |error| / bound %s" % (name, d, H, reverse, cut, ratios))
        assert all(v <= 1.0 for v in ratios.values()), ratios
        assert np.all(lse[~some] == -np.inf)
    # the two orders differ somewhere (else the second accepts nothing new), and lse is the unmasked one bit for bit
    C0, lse0 = dref.forward_online_f32(a, Q, B, scale, H, mk)
    C1, lse1 = dref.forward_online_f32(a, Q, B, scale, H, mk, True, True)
    assert not dref.same_bits(C0, C1)
    import spattn_heads_ref as href
    assert dref.same_bits(lse0, href.forward_online_f32(a, Q, B, scale, H)[1])


@pytest.mark.parametrize("name,d,H,keep", SMALL)
def test_bounds_reject_wrong_results(name, d, H, keep):
    a, Q, B, G, add, scale, mk = _inputs(name, d, H, keep)
    r = dref.backward_f64(a, Q, B, G, scale, H, mk)
    f = r['fwd']

    def outside(v, keys=('C', 'dQ', 'dB')):
        want = dict(C=(f.C, f.bound_C), dQ=(r['dQ'], r['bound_dQ']), dB=(r['dB'], r['bound_dB']))
        return {k: bool(np.any(np.abs(v[k] - want[k][0]) > want[k][1])) for k in keys}
    # the right values pass
    assert not any(outside(dref.values(a, Q, B, G, scale, H, mk)).values())
    # the mask evaluated as pair(j, i)
    wrong = dref.mask(a, H, 9, keep, transposed=True)
    assert not np.array_equal(wrong, mk)
    assert all(outside(dref.values(a, Q, B, G, scale, H, wrong)).values())
    # one kept entry dropped: the kept one whose weight is nearest 1/2 (an entry that owns its row alone, p = 1, has
    # dQ = 0 with and without it: nothing to notice there)
    p = np.concatenate([h.base.p[:, None] for h in f.per_head], axis=1)
    e, h = np.unravel_index(int(np.argmax(p * (1 - p) * (mk > 0))), p.shape)
    assert mk[e, h] > 0 and 0.1 < p[e, h] < 0.9
    less = mk.copy()
    less[e, h] = 0.0
    assert all(outside(dref.values(a, Q, B, G, scale, H, less)).values())
    # the 1 / keep factor omitted
    assert all(outside(dref.values(a, Q, B, G, scale, H, (mk > 0).astype(np.float64))).values())
    # the softmax normalised over the kept entries only
    assert all(outside(dref.values(a, Q, B, G, scale, H, mk, norm_over_kept=True)).values())
    # delta taken from the unmasked output: the forward is right, both gradients are not
    got = outside(dref.values(a, Q, B, G, scale, H, mk, delta_unmasked=True))
    assert got == dict(C=False, dQ=True, dB=True)


# ---- the GPU cases' preconditions -------------------------------------------------------------------------------------------------
def test_readout_inputs_are_what_they_claim():
    for name, (M, K) in dc.READOUT.items():
        a, at = dc.readout_pattern(name)
        assert a.shape == (M, K) and (name != "rect" or M < K)
        assert not (M == K and (abs(a - a.T)).nnz == 0)                        # asymmetric
        for i in range(M):
            js = a.indices[a.indptr[i]:a.indptr[i + 1]]
            assert len(set(js % dc.DH)) == js.size and js.size & (js.size - 1) == 0
        for H in (1, 4):
            Q, B, C, k = dc.readout_tables(name, H)
            assert not Q.any() and np.all(B.sum(axis=1) == H) and 0.4 < k.mean() < 0.6
            # every expected element is mk / n exactly: 2 / 2^k
            nz = C[C != 0]
            assert np.all(np.log2(nz) == np.round(np.log2(nz))) and (C != 0).sum() == k.sum()
            if H == 4:
                assert any(not np.array_equal(k[:, 0], k[:, h]) for h in (1, 2, 3))


def test_general_cases_cover_what_they_must():
    ds, Hs = {c[1] for c in dc.GENERAL}, {c[2] for c in dc.GENERAL}
    assert ds == {8, 30, 260, 602} and Hs == {1, 2, 8} and dc.PITCH[602] == 604 and dc.PITCH[30] % 4 == 0 and 30 % 4
    from stochastic_gcn_amd import ops as _ops
    import sparse_cases as sc
    for name, d, H, plan, keep in dc.GENERAL:
        a, _ = dc.pattern(name)
        M, K = a.shape
        assert K >= M and (abs(sp_pad(a) - sp_pad(a).T)).nnz > 0                # asymmetric
        key = dc.key_for(name, H, keep)
        assert key is not None
        mk = dref.mask(a, H, key, keep)
        gone, keptn = dc._all_dropped(a, mk)
        assert gone.any() and (keptn >= 2).any()                                # a row with every entry dropped exists
        assert not np.array_equal(mk, dref.mask(a, H, key, keep, transposed=True))
    a, _ = dc.pattern("row_lengths")
    assert np.diff(a.indptr).max() > 4 * sc.T_SPLIT                             # rows the plan "T" splits into many slots
    assert _ops.ATTN_MAX_VECTORS * 4 >= 602 > _ops.ATTN_MAX_VECTORS * 2


def sp_pad(a):
    """``a`` embedded in a square matrix, so that it can be compared with its transpose"""
    import scipy.sparse as sp
    n = max(a.shape)
    c = a.tocoo()
    return sp.csr_matrix((c.data, (c.row, c.col)), shape=(n, n))


@pytest.mark.parametrize("name", sorted(__import__("attn_dropout_cases").CASES))
def test_end_to_end_cases_are_well_posed(name):
    import attn_dropout_cases as dx
    c = dx.CASES[name]
    assert c['init'] == dx.scan(name)                        # the FIRST seed of 3 .. 12 that satisfies the condition
    m = dx.margin(name, c['init'])
    print("%s: init %d, smallest non-zero |ReLU input| / largest input %.3e (needs >= %.0e)" % (name, c['init'], m, dx.MARGIN))
    assert m >= dx.MARGIN == 1e-4 and dx.P == 0.2
    case = dx.build(name)
    assert case['n'] <= 500 and case['flags']['hidden1'] == 8
    # the masks bite: the masked reference differs from the unmasked one, and an evaluation model never masks
    import full_batch_cases as fc
    feed = fc.exact_feed(case, case['train_adj'], 0.0)
    on = dx.reference_model(case, case['nbr_train']).forward(feed, case['ph'], 0.0, None)[0]
    off = dx.reference_model(case, case['nbr_train'], attn_dropout=0.0).forward(feed, case['ph'], 0.0, None)[0]
    ev = dx.reference_model(case, case['nbr_train'], is_training=False).forward(feed, case['ph'], 0.0, None)[0]
    assert not np.array_equal(on, off) and np.array_equal(ev, off)


# ---- the flag -----------------------------------------------------------------------------------------------------------------
BOTH = dict(full_batch=True, test_full_batch=True, aggregator='attn')


def test_flag_default_parsing_and_help():
    from stochastic_gcn_amd.full_batch import check_attention, check_attn_dropout
    f = _Flags()
    assert f.attn_dropout == 0.0 and 'attn_dropout' in f.as_dict() and check_attn_dropout(f) == 0.0
    f.parse(['--full_batch', '--test_full_batch', '--aggregator', 'attn', '--attn_dropout', '0.2'])
    assert f.attn_dropout == 0.2 and check_attn_dropout(f) == 0.2 and check_attention(f) == (True, 0.0)
    for p in (0.0, 0.2, 0.999):
        FLAGS.update(**BOTH, attn_dropout=p)
        assert check_attn_dropout() == p
    FLAGS.reset()
    assert check_attn_dropout() == 0.0                        # off needs no attention
    help_ = {name: h for name, _, _, h in _DEFS}
    assert '[0, 1)' in help_['attn_dropout'] and 'Evaluation never masks' in help_['attn_dropout']
    assert ('attn_dropout', float, 0.0) == next(d[:3] for d in _DEFS if d[0] == 'attn_dropout')


REFUSALS = [
    (dict(BOTH, attn_dropout=-0.1), r"--attn_dropout must lie in \[0, 1\) \(0 = off\), got -0.1"),
    (dict(BOTH, attn_dropout=1.0), r"--attn_dropout must lie in \[0, 1\)"),
    (dict(BOTH, attn_dropout=1.5), r"--attn_dropout must lie in \[0, 1\)"),
    (dict(BOTH, attn_dropout=float('nan')), r"--attn_dropout must lie in \[0, 1\)"),
    (dict(attn_dropout=0.2), r"--attn_dropout needs --aggregator attn"),
    (dict(full_batch=True, test_full_batch=True, aggregator='max', attn_dropout=0.2), r"--attn_dropout needs --aggregator attn"),
]


@pytest.mark.parametrize("flags,msg", REFUSALS)
def test_refusals(flags, msg):
    from stochastic_gcn_amd.full_batch import check_attn_dropout
    FLAGS.update(**flags)
    with pytest.raises(ValueError, match=msg):
        check_attn_dropout()


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


@pytest.mark.parametrize("extra", [dict(attn_dropout=0.2), dict(attn_dropout=0.5, attn_heads=4), dict(attn_dropout=0.0)])
def test_accepted_combination_reaches_the_device_check(monkeypatch, extra):
    from stochastic_gcn_amd import train
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    FLAGS.update(**BOTH, **extra)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        train.Trainer(verbose=False)


def test_static_matrix_passes_the_keywords_only_when_set(monkeypatch):
    """keep = 1 is the call ops.spattn has always taken; keep < 1 travels with its key; the refusals stay"""
    import sparse_cases as sc
    from stochastic_gcn_amd import full_batch
    a = sc.pattern("m64_k64")
    m = full_batch.StaticMatrix(a, torch.device("cpu"), 'rows')
    seen = []
    monkeypatch.setattr(ops, "spattn", lambda *a, **k: seen.append(k) or (None, None))
    monkeypatch.setattr(ops, "spattn_bwd", lambda *a, **k: seen.append(k) or (None, None))
    x = torch.zeros(64, 8)
    m.attn_product(x, 1.0)
    m.attn_product(x, 1.0, keep=0.8, key=5)
    m.attn_backward(x, x, x, torch.zeros(64), 1.0)
    m.attn_backward(x, x, x, torch.zeros(64), 1.0, keep=0.8, key=5)
    assert ['keep' in k for k in seen] == [False, True, False, True]
    assert all(k['keep'] == 0.8 and k['key'] == 5 for k in seen if 'keep' in k)
    m.edge = full_batch.EdgeMask(0.2)
    with pytest.raises(ValueError, match="attention has no edge-masked form"):
        m.attn_product(x, 1.0, keep=0.8, key=5)
    for bad in (0.0, -1.0, 1.5, float('nan')):
        with pytest.raises(ValueError, match=r"keep must be finite and in \(0, 1\]"):
            ops._attn_keep(bad)


def test_aggregator_draws_one_key_per_step_and_keeps_it_for_the_backward():
    """layers.PlainAggregator on a recording matrix: a training model under --attn_dropout hands forward and backward the
    same (keep, key), the key that of (seed, its own index, step); an evaluation model and P = 0 hand none"""
    from stochastic_gcn_amd import layers
    calls = []

    class Mat(object):
        shape = (4, 4)

        def attn_product(self, x, scale, out=None, want_lse=True, heads=1, **kw):
            calls.append(('fwd', kw))
            return torch.zeros(4, x.shape[1]), (torch.zeros(4) if want_lse else None)

        def attn_backward(self, x, g, out_fwd, lse, scale, add=None, add_rows=0, heads=1, **kw):
            calls.append(('bwd', kw))
            return torch.zeros_like(x)

    class Cur(object):
        adj = [Mat()]

    class Model(object):
        cur, is_training, dropout_seed, dropout_step = Cur(), True, 7, 0
    FLAGS.update(**BOTH, attn_dropout=0.25, normalization='gcn')
    model = Model()
    agg = layers.PlainAggregator(model, 0, name='agg0')
    agg.index = 5
    for step in (0, 1):
        model.dropout_step = step
        agg.forward(torch.zeros(4, 8))
        agg.backward(torch.zeros(4, 8))
    want = [dict(keep=0.75, key=ops.attn_key(7, 5, s)) for s in (0, 0, 1, 1)]
    assert [kw for _, kw in calls] == want and want[0]['key'] != want[2]['key']
    del calls[:]
    model.is_training = False
    agg.forward(torch.zeros(4, 8))
    FLAGS.update(attn_dropout=0.0)
    model.is_training = True
    agg.forward(torch.zeros(4, 8))
    agg.backward(torch.zeros(4, 8))
    assert [kw for _, kw in calls] == [{}, {}, {}]


# ---- the exports ---------------------------------------------------------------------------------------------------------
NAMES = (("sgcn_spattn_drop_csr_f32", 18), ("sgcn_spattn_drop_csr_bwd_q_f32", 26), ("sgcn_spattn_drop_csr_bwd_kv_f32", 24))


def test_symbols_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "sgcn.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, nargs in NAMES:
        assert "int %s(" % name in src
        assert hasattr(lib, name) and name in _ffi.SIGNATURES
        sig = _ffi.SIGNATURES[name][1]
        assert len(sig) == nargs
        old = _ffi.SIGNATURES[name.replace("_drop_", "_mh_")][1]
        assert sig[:6] == old[:6] and sig[6] is ctypes.c_float and sig[7] is ctypes.c_uint32 and sig[8:] == old[6:]
    version = src[src.index("v16 packed minibatch"):src.index("int sgcn_abi_version")]
    assert all(name in version for name, _ in NAMES)
    assert _ffi.lib.sgcn_abi_version() == _ffi.ABI_VERSION == 16          # additive exports


A0 = 4096          # (non-null addresses that are never dereferenced: every call below fails validation first)


def _fwd(rowptr=A0, col=2 * A0, M=8, K=8, d=8, heads=2, keep=0.8, key=1, Q=3 * A0, ldq=8, B=4 * A0, ldb=8, scale=1.0, C=5 * A0,
         ldc=8, lse=6 * A0, plan=None):
    return _ffi.lib.sgcn_spattn_drop_csr_f32(rowptr, col, M, K, d, heads, keep, key, Q, ldq, B, ldb, scale, C, ldc, lse, plan, None)


def _bwd_q(rowptr=A0, col=2 * A0, M=8, K=8, d=8, heads=2, keep=0.8, key=1, Q=3 * A0, ldq=8, B=4 * A0, ldb=8, scale=1.0, G=5 * A0,
           ldg=8, C=6 * A0, ldc=8, lse=7 * A0, delta=8 * A0, dQ=9 * A0, lddq=8, add=None, ldadd=0, add_rows=0, plan=None):
    return _ffi.lib.sgcn_spattn_drop_csr_bwd_q_f32(rowptr, col, M, K, d, heads, keep, key, Q, ldq, B, ldb, scale, G, ldg, C, ldc,
                                                   lse, delta, dQ, lddq, add, ldadd, add_rows, plan, None)


def _bwd_kv(rowptr=A0, row=2 * A0, K=8, M=8, d=8, heads=2, keep=0.8, key=1, Q=3 * A0, ldq=8, B=4 * A0, ldb=8, scale=1.0, G=5 * A0,
            ldg=8, lse=7 * A0, delta=8 * A0, dB=9 * A0, lddb=8, add=None, ldadd=0, add_rows=0, plan=None):
    return _ffi.lib.sgcn_spattn_drop_csr_bwd_kv_f32(rowptr, row, K, M, d, heads, keep, key, Q, ldq, B, ldb, scale, G, ldg, lse, delta,
                                                    dB, lddb, add, ldadd, add_rows, plan, None)


@pytest.mark.parametrize("fn", [_fwd, _bwd_q, _bwd_kv])
def test_keep_is_validated_before_any_device_call(fn):
    err = _ffi.lib.sgcn_last_error
    for keep in (0.0, 1.5, float('nan'), -0.5, float('inf')):
        assert fn(keep=keep) == -1 and b"keep must be finite and in (0, 1]" in err()
    # everything the multi-head calls refuse, at keep < 1 and at keep = 1 alike
    for keep in (0.8, 1.0):
        assert fn(keep=keep, heads=3) == -1 and b"heads must be one of 1/2/4/8" in err()
        assert fn(keep=keep, d=6, heads=4) == -1 and b"d = 6 is not a multiple of heads = 4" in err()
        assert fn(keep=keep, rowptr=None) == -1 and b"null operand" in err()
        assert fn(keep=keep, d=0) == -1 and b"d must be positive" in err()
        assert fn(keep=keep, ldq=7) == -1 and b"leading dimension smaller than d" in err()
        assert fn(keep=keep, scale=float('nan')) == -1 and b"scale must be finite" in err()
        p = _ffi.Plan(4096, 8, None, 1, 3, None, 0)
        assert fn(keep=keep, plan=ctypes.byref(p)) == -1 and b"needs dev_fix/dev_ws" in err()
        lds = {k: 520 for k in ("ldq", "ldb", "ldc", "ldg", "lddq", "lddb") if k in fn.__code__.co_varnames}
        assert fn(keep=keep, d=520, heads=8, **lds) == -1 and b"over the limit of 256 columns at vector width 1" in err()
    assert _fwd(M=0, Q=None) == 0 and _bwd_q(M=0, Q=None, G=None, C=None, lse=None, delta=None) == 0 and _bwd_kv(K=0, B=None) == 0


def test_ops_refuse_bad_keep_and_cpu_tensors():
    import scipy.sparse as sp
    a = sp.identity(4, format='csr', dtype=np.float32)
    A = ops.DeviceCSR.from_scipy(a, torch.device("cpu"), with_plan=False)
    with pytest.raises(ValueError, match=r"keep must be finite and in \(0, 1\]"):
        ops.spattn(A, torch.zeros(4, 8), scale=1.0, keep=0.0)
    with pytest.raises(ValueError, match=r"keep must be finite and in \(0, 1\]"):
        ops.spattn_bwd(A, A, torch.zeros(4, 8), None, torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4), 1.0, keep=float('nan'))
    with pytest.raises(RuntimeError, match="HBM"):
        ops.spattn(A, torch.zeros(4, 8), scale=1.0, heads=2, keep=0.8, key=3)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.spattn_bwd(A, A, torch.zeros(4, 8), None, torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4, 2), 1.0, heads=2,
                       keep=0.8, key=3)
