"""The wiring of --dense_dtype bf16 (layers.Dense on a static batch), on the small cases of tests/full_batch_cases.py.

The calls of ops.gemm_bf16, ops.gemm, ops.dense_fwd, ops.dense_bwd and ops.ln_act_fwd are recorded with their operands.
Under the flag every dense-input Dense layer makes exactly one NN call forward and, backward, one TN call with accumulate
plus one NT call where it needs an input gradient, and no fp32 GEMM call; a sparse-input first layer makes the calls it
makes without the flag.  Teacher-forced numerics: every recorded product lies within mb16_cases.reference's bound of the
fp64 product of ITS OWN recorded operands, rounded as the kernel rounds them, and the layer output behind ln_act_fwd
within dense_cases.ln_fwd_bound with that bound as the pre-activation's error.  Besides: the same step twice gives the same
weights bit for bit; without the flag ops.gemm_bf16 is never called; with --cv --cvd --test_full_batch the sampled
training steps stay fp32 and the exact evaluation takes the new route; train.main runs end to end."""
import contextlib
import io
import math
import re

import numpy as np
import pytest
import torch

import dense_cases as dc
import full_batch_cases as fc
import mb16_cases as mbc
from oracle import model_np as mnp

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NAMES = ('gemm_bf16', 'gemm', 'dense_fwd', 'dense_bwd', 'ln_act_fwd', 'spmm')


def _host(t):
    return None if t is None else t.detach().double().cpu().numpy()


@contextlib.contextmanager
def recording(keep_operands=True):
    """ops' entry points wrapped: rec[name] is the list of calls; a gemm_bf16 call keeps its operands, the old output
    (accumulate) and its result on the host"""
    from stochastic_gcn_amd import ops
    rec = {n: [] for n in NAMES}
    real = {n: getattr(ops, n) for n in NAMES}

    def gemm_bf16(A, B, out=None, trans_a=False, trans_b=False, accumulate=False, drop_a=None, drop_c=None):
        r = dict(ta=bool(trans_a), tb=bool(trans_b), accumulate=bool(accumulate), drop_a=drop_a, drop_c=drop_c,
                 shape_a=tuple(A.shape), shape_b=tuple(B.shape))
        if keep_operands:
            r.update(A=A.detach().cpu().numpy().copy(), B=B.detach().cpu().numpy().copy(),
                     C_in=_host(out) if accumulate else None)
        res = real['gemm_bf16'](A, B, out=out, trans_a=trans_a, trans_b=trans_b, accumulate=accumulate, drop_a=drop_a,
                                drop_c=drop_c)
        r['res_dev'] = res
        if keep_operands:
            r['res'] = _host(res)
        rec['gemm_bf16'].append(r)
        return res

    def ln_act_fwd(x, offset, scale, relu, eps=1e-9):
        y, ctx = real['ln_act_fwd'](x, offset, scale, relu, eps)
        rec['ln_act_fwd'].append(dict(x_dev=x, offset=_host(offset), scale=_host(scale), relu=bool(relu), eps=eps,
                                      y=_host(y) if keep_operands else None))
        return y, ctx

    def plain(name):
        def f(*a, **k):
            rec[name].append((a, k))
            return real[name](*a, **k)
        return f
    try:
        ops.gemm_bf16, ops.ln_act_fwd = gemm_bf16, ln_act_fwd
        for n in ('gemm', 'dense_fwd', 'dense_bwd', 'spmm'):
            setattr(ops, n, plain(n))
        yield rec
    finally:
        for n in NAMES:
            setattr(ops, n, real[n])


def _form(r):
    return "TN" if r['ta'] else "NT" if r['tb'] else "NN"


def _reference(r):
    """(ref, bound) of a recorded gemm_bf16 call from its own operands"""
    kw = {}
    M, N = r['res'].shape
    if r['drop_a'] is not None:
        d = r['drop_a']
        kw.update(mask_a=mnp.hash_mask(d.key, r['A'].shape, d.keep).astype(np.float64), scale_a=dc.f32_scale(d.keep))
    if r['drop_c'] is not None:
        d = r['drop_c']
        kw.update(mask_c=mnp.hash_mask(d.key, (M, N), d.keep).astype(np.float64), scale_c=dc.f32_scale(d.keep))
    ref, bound, _ = mbc.reference(r['A'], r['B'], r['ta'], r['tb'], r['C_in'], r['accumulate'], **kw)
    return ref, bound


def _check_products(rec, what):
    for i, r in enumerate(rec['gemm_bf16']):
        ref, bound = _reference(r)
        err = np.abs(r['res'] - ref)
        print("%s: gemm_bf16 call %d %s %r x %r: worst err / bound %.4f" % (what, i, _form(r), r['shape_a'], r['shape_b'],
                                                                           float(np.max(err / bound))))
        assert (err <= bound).all(), (what, i, _form(r))
        r['ref'], r['bound'] = ref, bound


def _check_layer_outputs(rec, what):
    """every ln_act_fwd behind a recorded NN product: its output against fp64 LayerNorm / ReLU of the fp64 product"""
    seen = 0
    for l in rec['ln_act_fwd']:
        src = [r for r in rec['gemm_bf16'] if r['res_dev'] is l['x_dev']]
        if not src:
            continue
        r = src[0]
        assert _form(r) == "NN"
        v, pre = r['ref'], r['bound']
        if l['offset'] is not None:
            y_ref = dc.ln_f64(v, l['offset'], l['scale'], l['relu'], l['eps'])[0]
            by = dc.ln_fwd_bound(v, l['offset'], l['scale'], l['eps'], pre_err=pre)[0]
        else:
            y_ref, by = (np.maximum(v, 0.0) if l['relu'] else v), pre
        err = np.abs(l['y'] - y_ref)
        finite = np.isfinite(by)
        print("%s: layer output %r: worst err / bound %.4f (%d of %d elements bounded)"
              % (what, l['y'].shape, float(np.max(np.where(finite, err / np.where(finite, by, 1.0), 0.0))), int(finite.sum()), by.size))
        assert (err <= by).all(), what
        seen += 1
    return seen


def _dense_layers(model):
    from stochastic_gcn_amd.layers import Dense
    return [l for l in model.layers if isinstance(l, Dense)]


def _static_batch(case, adj, model, rows, kernel='cs'):
    from stochastic_gcn_amd.full_batch import StaticBatch, model_matrix
    mat = model_matrix(adj, DEV, model, 3, kernel=kernel)
    return StaticBatch(mat, case['labels'], np.sort(rows), model.L, DEV)


def _model(case, bf16, is_training=True):
    om = fc.oracle_model(case, case['nbr_train'])
    dm = fc.device_model(case, case['nbr_train'], case['train_adj'], {k: v.copy() for k, v in om.params.items()},
                         is_training=is_training, extra_flags=dict(dense_dtype='bf16' if bf16 else 'fp32'))
    sb = _static_batch(case, case['train_adj'], dm, case['train'])
    sb.dropout = case['flags']['dropout']
    return dm, sb


def _trainer(case, **flags):
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.train import Trainer
    FLAGS.reset()
    FLAGS.update(dataset='ppi' if case['multitask'] else 's-reddit', seed=1, prefetch=0,
                 test_preprocess=case['flags']['preprocess'],
                 **{k: v for k, v in case['flags'].items() if hasattr(FLAGS, k)})
    FLAGS.update(**flags)
    with contextlib.redirect_stdout(io.StringIO()):
        return Trainer(data=case['data'], verbose=False)


@pytest.fixture(autouse=True)
def _flags():
    from stochastic_gcn_amd.flags import FLAGS
    yield
    FLAGS.reset()


@pytest.mark.parametrize("name", ['reddit3k_pp', 'reddit3k_nopp', 'cora'])
def test_training_step_call_pattern_and_teacher_forced_numerics(name):
    case = fc.build(name)
    dm, sb = _model(case, True)
    with recording() as rec:
        outs = dm.run_one_step(None, sb)
        torch.cuda.synchronize()
    assert math.isfinite(float(outs[1]))
    dense = _dense_layers(dm)
    mine = [l for l in dense if not l.sparse_inputs]
    assert mine and all(l._bf16 for l in mine) and not any(l._bf16 for l in dense if l.sparse_inputs)
    forms = [_form(r) for r in rec['gemm_bf16']]
    nn = [r for r in rec['gemm_bf16'] if _form(r) == "NN"]
    tn = [r for r in rec['gemm_bf16'] if _form(r) == "TN"][::-1]        # the backward runs the layers in reverse
    nt = [r for r in rec['gemm_bf16'] if _form(r) == "NT"][::-1]
    assert len(nn) == len(tn) == len(mine) and len(nt) == len([l for l in mine if l.need_dx])
    assert forms[:len(mine)] == ["NN"] * len(mine)                       # the forward first, layer by layer
    nt_of = iter(nt)
    n = case['n']
    for l, f, w in zip(mine, nn, tn):        # layer by layer: its own shapes, and ONE dropout site in all of its products
        assert f['shape_a'] == (n, l.input_dim) and f['shape_b'] == (l.input_dim, l.output_dim) and not f['accumulate']
        assert w['shape_a'] == (n, l.input_dim) and w['shape_b'] == (n, l.output_dim) and w['accumulate']
        assert w['drop_a'] is f['drop_a'] and f['drop_c'] is None and w['drop_c'] is None
        if l.need_dx:
            x = next(nt_of)
            assert x['shape_a'] == (n, l.output_dim) and x['shape_b'] == (l.input_dim, l.output_dim) and not x['accumulate']
            assert x['drop_c'] is f['drop_a'] and x['drop_a'] is None
    assert rec['gemm'] == [] and rec['dense_fwd'] == [] and rec['dense_bwd'] == []          # no fp32 GEMM call
    if case['flags']['dropout'] > 0:         # dropout reaches the products
        assert any(r['drop_a'] is not None for r in nn)
    if any(l.sparse_inputs for l in dense):
        # a sparse-input first layer makes the calls it makes without the flag: the same step with the flag off records
        # the same spmm calls (operand types and shapes, in order) and the same LayerNorm passes outside the new route
        off, sb_off = _model(case, False)
        with recording(keep_operands=False) as rec_off:
            off.run_one_step(None, sb_off)
            torch.cuda.synchronize()
        sig = lambda r: [(type(a[0]).__name__, tuple(a[0].shape), tuple(a[1].shape), sorted(k)) for a, k in r['spmm']]  # noqa: E731
        assert len(rec['spmm']) >= 2 and sig(rec) == sig(rec_off)
        fed = {id(r['res_dev']) for r in rec['gemm_bf16']}
        ln = lambda r: [(tuple(c['x_dev'].shape), c['relu'], c['offset'] is not None) for c in r['ln_act_fwd']   # noqa: E731
                        if id(c['x_dev']) not in fed]
        assert ln(rec) == ln(rec_off) and len(ln(rec)) >= 1
        assert rec_off['gemm_bf16'] == [] and len(rec_off['dense_fwd']) == len(mine)
    _check_products(rec, name)
    assert _check_layer_outputs(rec, name) == len([l for l in mine if l.norm or l.act])


@pytest.mark.parametrize("name", ['reddit3k_pp', 'cora'])
def test_exact_evaluation_call_pattern_and_numerics(name):
    case = fc.build(name)
    tr = _trainer(case, test_full_batch=True, full_batch_kernel='cs', dense_dtype='bf16')
    with recording() as rec:
        res = tr.evaluate(tr.val_d)
        torch.cuda.synchronize()
    assert all(math.isfinite(v) for v in res[:4])
    mine = [l for l in _dense_layers(tr.test_model) if not l.sparse_inputs]
    assert mine and [_form(r) for r in rec['gemm_bf16']] == ["NN"] * len(mine)
    assert all(r['drop_a'] is None for r in rec['gemm_bf16'])
    assert rec['gemm'] == [] and rec['dense_fwd'] == [] and rec['dense_bwd'] == []
    _check_products(rec, name + " eval")
    _check_layer_outputs(rec, name + " eval")


def test_the_same_step_twice_gives_the_same_weights():
    case = fc.build('reddit3k_nopp')
    bits = []
    for _ in range(2):
        dm, sb = _model(case, True)
        for _ in range(2):
            dm.run_one_step(None, sb)
        torch.cuda.synchronize()
        bits.append(dm.theta.detach().view(torch.int32).cpu().clone())
    assert torch.equal(bits[0], bits[1])
    assert bool(torch.isfinite(bits[0].view(torch.float32)).all())


def test_the_default_route_never_calls_gemm_bf16():
    case = fc.build('reddit3k_pp')
    dm, sb = _model(case, False)
    with recording(keep_operands=False) as rec:
        dm.run_one_step(None, sb)
        torch.cuda.synchronize()
    assert rec['gemm_bf16'] == [] and len(rec['dense_fwd']) > 0 and len(rec['dense_bwd']) > 0
    assert not any(l._bf16 for l in _dense_layers(dm))


def test_mixed_mode_sampled_steps_stay_fp32_and_the_exact_evaluation_takes_the_new_route():
    case = fc.build('reddit3k_pp')
    tr = _trainer(case, cv=True, cvd=True, degree=1, batch_size=256, test_batch_size=256, test_full_batch=True,
                  dense_dtype='bf16')
    assert tr.train_sch is not None and tr.full_batch is False
    with recording(keep_operands=False) as rec:
        tr.train_epoch()
        torch.cuda.synchronize()
    assert rec['gemm_bf16'] == []
    with recording(keep_operands=False) as rec:
        res = tr.evaluate(tr.val_d)
        torch.cuda.synchronize()
    assert len(rec['gemm_bf16']) > 0 and rec['gemm'] == [] and rec['dense_fwd'] == [] and math.isfinite(res[0])
    # ... and a second epoch after it is still fp32 (the flag is read per pass, not latched by the evaluation)
    with recording(keep_operands=False) as rec:
        tr.train_epoch()
        torch.cuda.synchronize()
    assert rec['gemm_bf16'] == []


def test_train_main_end_to_end(tmp_path, monkeypatch):
    from stochastic_gcn_amd import train
    from stochastic_gcn_amd.flags import FLAGS
    monkeypatch.chdir(tmp_path)
    runs = []
    for _ in range(2):
        FLAGS.reset()
        buf = io.StringIO()
        with recording(keep_operands=False) as rec, contextlib.redirect_stdout(buf):
            train.main(['--dataset', 's-cora', '--full_batch', '--test_full_batch', '--dense_dtype', 'bf16', '--epochs', '3'])
        assert len(rec['gemm_bf16']) > 0
        ep = [l.split() for l in buf.getvalue().splitlines() if l.startswith("Epoch:")]
        assert len(ep) == 5                   # the reference's exit is `epoch > FLAGS.epochs`: epochs + 2
        vals = [(float(t[3]), float(t[5]), float(t[7]), float(t[9])) for t in ep]       # train loss / acc, val loss / acc
        assert all(math.isfinite(v) for row in vals for v in row)
        m = re.search(r"Test set results: cost= (\d+\.\d{5}) accuracy= (\d+\.\d{5})", buf.getvalue())
        assert m
        runs.append((vals, m.groups()))
    print("train loss per epoch:", [v[0] for v in runs[0][0]])
    assert runs[0] == runs[1]
