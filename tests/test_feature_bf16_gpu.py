"""--feature_dtype bf16 end to end on the small dense cases of tests/full_batch_cases.py.

1. Three --full_batch steps and a --test_full_batch evaluation with the bfloat16 feature table equal, bit for bit in loss,
   logits and every weight, the same run with --feature_dtype fp32 on features passed through bf16_ref.round_trip first --
   with dropout off and with the recipe's dropout (the masks are a hash of the element index: the same in both runs).
2. Residency: the selected model's table is torch.bfloat16 on the pitch-8 layout and no fp32 tensor of its shape stays
   referenced by the model.
3. Recorded calls: which products receive a bfloat16 A, and that the layer-0 aggregation reads the table itself.
4. Mixed mode --cv --cvd --test_full_batch: the sampled training model is untouched, only the test model's table is bfloat16.
5. train.main end to end."""
import contextlib
import io
import math
import re

import numpy as np
import pytest
import torch

import bf16_ref
import full_batch_cases as fc

pytestmark = pytest.mark.gpu

ON = dict(dense_dtype='bf16', feature_dtype='bf16')
OFF = dict(dense_dtype='bf16', feature_dtype='fp32')


@pytest.fixture(autouse=True)
def _flags():
    from stochastic_gcn_amd.flags import FLAGS
    yield
    FLAGS.reset()


@pytest.fixture(scope="module")
def cases():
    """name -> (the case, the same case with every feature table passed through bf16_ref.round_trip); built once"""
    out = {}
    for name in ('reddit3k_pp', 'reddit3k_nopp'):
        case = fc.build(name)
        d = list(case['data'])
        d[3], d[4], d[5] = (bf16_ref.round_trip(np.asarray(x, np.float32)) for x in d[3:6])
        out[name] = (case, dict(case, data=tuple(d)))
    return out


def _trainer(case, **flags):
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.train import Trainer
    FLAGS.reset()
    FLAGS.update(dataset='s-reddit', seed=1, prefetch=0, test_preprocess=case['flags']['preprocess'],
                 **{k: v for k, v in case['flags'].items() if hasattr(FLAGS, k)})
    FLAGS.update(**flags)
    d = case['data']
    data = d[:7] + tuple(np.array(x) for x in d[7:])          # (a sampler shuffles its id array in place: every trainer its own)
    with contextlib.redirect_stdout(io.StringIO()):
        return Trainer(data=data, verbose=False)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _run(case, **flags):
    """three --full_batch epochs (one step each) and one --test_full_batch evaluation"""
    tr = _trainer(case, full_batch=True, test_full_batch=True, **flags)
    steps = []
    for _ in range(3):
        tr.train_epoch()
        m = tr.train_model
        steps.append(dict(loss=float(tr.avg_loss.window[-1]), logits=m.outputs.detach().cpu().numpy(), grads=m.get_grads(),
                          params=m.get_params()))
    ev = tr.evaluate(tr.val_d)
    torch.cuda.synchronize()
    return steps, tr.test_model.outputs.cpu().numpy(), tuple(ev[:2]), tr


# ---- 1. the same bits as the fp32 table holding the rounded features ---------------------------------------------------------
@pytest.mark.parametrize("name,kernel,dropout", [('reddit3k_pp', 'cs', 0.0), ('reddit3k_pp', 'cs', None),
                                                 ('reddit3k_nopp', 'cs', 0.0), ('reddit3k_nopp', 'cs', None),
                                                 ('reddit3k_nopp', 'rows', None)])
def test_bf16_table_equals_fp32_table_of_round_tripped_features(cases, name, kernel, dropout):
    case, rounded = cases[name]
    extra = dict(full_batch_kernel=kernel, **({} if dropout is None else dict(dropout=dropout)))
    got, got_logits, got_ev, tr = _run(case, **ON, **extra)
    assert tr.train_model.features_dev.dtype == torch.bfloat16 and tr.test_model.features_dev.dtype == torch.bfloat16
    want, want_logits, want_ev, tr32 = _run(rounded, **OFF, **extra)
    assert tr32.train_model.features_dev.dtype == torch.float32 and tr32.test_model.features_dev.dtype == torch.float32
    for step, (g, w) in enumerate(zip(got, want)):
        print("%s/%s dropout %s step %d: loss %r / %r" % (name, kernel, dropout, step, g['loss'], w['loss']))
        assert math.isfinite(g['loss']) and g['loss'] == w['loss'], (step, 'loss')
        assert np.array_equal(_bits(g['logits']), _bits(w['logits'])), (step, 'logits')
        for what in ('grads', 'params'):
            assert sorted(g[what]) == sorted(w[what])
            for k in g[what]:
                assert np.array_equal(_bits(g[what][k]), _bits(w[what][k])), (step, what, k)
    assert np.array_equal(_bits(got_logits), _bits(want_logits)) and got_ev == want_ev
    assert all(math.isfinite(float(v)) for v in got_ev)
    # Against the same run on the UNROUNDED fp32 features.  Under --preprocess with dropout off the only readers of the table
    # are the first layer's two products, which round each element to nearest even in registers: rounding once at set-up
    # gives the same bits as today's run.  With input dropout the factor multiplies the rounded value instead of the fp32
    # one, and under --nopreprocess the fp32 aggregation reads the unrounded table: there the rounding shows.
    plain = _run(case, **OFF, **extra)[0]
    same = all(np.array_equal(_bits(got[2]['params'][k]), _bits(plain[2]['params'][k])) for k in got[2]['params'])
    assert same == (case['flags']['preprocess'] and dropout == 0.0)


# ---- 2. residency -----------------------------------------------------------------------------------------------------------
def _tensors(obj, depth=3, seen=None):
    seen = set() if seen is None else seen
    if id(obj) in seen:
        return
    seen.add(id(obj))
    if isinstance(obj, torch.Tensor):
        yield obj
    elif depth > 0:
        if isinstance(obj, dict):
            items = list(obj.values())
        elif isinstance(obj, (list, tuple, set)):
            items = list(obj)
        else:
            items = list(getattr(obj, '__dict__', {}).values())
        for v in items:
            for t in _tensors(v, depth - 1, seen):
                yield t


@pytest.mark.parametrize("name", ['reddit3k_pp', 'reddit3k_nopp'])
def test_table_residency(cases, name):
    case = cases[name][0]
    tr = _trainer(case, full_batch=True, test_full_batch=True, full_batch_kernel='rows', **ON)
    n, f = case['n'], case['feats'].shape[1]
    width = 2 * f if case['flags']['preprocess'] else f            # hstack(X, A.X) under --preprocess
    srcs = (np.hstack([case['feats'], case['nbr_train']]), np.hstack([case['feats'], case['nbr_test']])) \
        if case['flags']['preprocess'] else (case['feats'], case['feats'])
    for model, src in zip((tr.train_model, tr.test_model), srcs):
        assert model.feature_bf16
        t = model.features_dev
        assert t.dtype == torch.bfloat16 and tuple(t.shape) == (n, width) and model.features is t
        pitch = (width + 7) // 8 * 8
        assert tuple(t.stride()) == (pitch, 1) and t.data_ptr() % 16 == 0
        base = t._base if t._base is not None else t
        assert tuple(base.shape) == (n, pitch) and base.data_ptr() == t.data_ptr()           # the pitch-8 table
        assert bool((base[:, width:].view(torch.int16) == 0).all())                          # zero padding
        # rounded once, to nearest even
        assert np.array_equal(t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16), bf16_ref.round_bits(src))
        left = [x for x in _tensors(model) if x.dtype == torch.float32 and x.dim() == 2 and tuple(x.shape) == (n, width)]
        assert left == [], "an fp32 tensor of the table's shape is still referenced by the model"
    # a step and an evaluation later it is still so (nothing caches a widened copy)
    tr.train_epoch()
    tr.evaluate(tr.val_d)
    for model in (tr.train_model, tr.test_model):
        keep = {id(a) for a in model.activations[1:]}
        left = [x for x in _tensors(model) if x.dtype == torch.float32 and x.dim() == 2 and tuple(x.shape) == (n, width)
                and id(x) not in keep]
        assert left == [] and model.features_dev.dtype == torch.bfloat16


# ---- 3. recorded calls ------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def recording():
    """ops.gemm_bf16, ops.operand_round, ops.spmm and ops.spmm_cs with their operands noted (the calls still run)"""
    from stochastic_gcn_amd import ops
    rec = dict(gemm_bf16=[], operand_round=[], spmm=[])
    real = {k: getattr(ops, k) for k in ('gemm_bf16', 'operand_round', 'spmm', 'spmm_cs')}

    def gemm_bf16(A, B, out=None, trans_a=False, trans_b=False, **kw):
        rec['gemm_bf16'].append(dict(form="NT" if trans_b else "TN" if trans_a else "NN", A=A, B=B, drop_a=kw.get('drop_a')))
        return real['gemm_bf16'](A, B, out=out, trans_a=trans_a, trans_b=trans_b, **kw)

    def operand_round(x, out=None):
        rec['operand_round'].append(tuple(x.shape))
        return real['operand_round'](x, out=out)

    def product(name):
        def run(A, B, *a, **kw):
            rec['spmm'].append(dict(kernel=name, B=B))
            return real[name](A, B, *a, **kw)
        return run
    ops.gemm_bf16, ops.operand_round, ops.spmm, ops.spmm_cs = gemm_bf16, operand_round, product('spmm'), product('spmm_cs')
    try:
        yield rec
    finally:
        for k, v in real.items():
            setattr(ops, k, v)


def _step_and_eval(tr):
    tr.train_epoch()                  # (unrecorded: a sweep tunes its clock on the first product of a width and operand type)
    tr.evaluate(tr.val_d)
    with recording() as rec_train:
        tr.train_epoch()
        torch.cuda.synchronize()
    with recording() as rec_eval:
        tr.evaluate(tr.val_d)
        torch.cuda.synchronize()
    return rec_train, rec_eval


def test_preprocess_only_the_first_layers_two_products_read_the_table(cases):
    case = cases['reddit3k_pp'][0]
    tr = _trainer(case, full_batch=True, test_full_batch=True, full_batch_kernel='rows', **ON)
    rec_train, rec_eval = _step_and_eval(tr)
    for rec, model, forms in ((rec_train, tr.train_model, ["NN", "TN"]), (rec_eval, tr.test_model, ["NN"])):
        tab = model.features_dev
        b16 = [r for r in rec['gemm_bf16'] if r['A'].dtype == torch.bfloat16]
        assert [r['form'] for r in b16] == forms
        assert all(r['A'] is tab for r in b16)                                      # the table itself: no copy of any type
        assert all(r['B'].dtype == torch.float32 for r in rec['gemm_bf16'])
        others = [r for r in rec['gemm_bf16'] if r['A'].dtype != torch.bfloat16]
        assert others and all(r['A'].dtype == torch.float32 for r in others)
        assert not any(r['B'].dtype == torch.bfloat16 for r in rec['spmm'])          # --full_batch_dtype fp32: nothing rounded
        assert rec['operand_round'] == []
    assert rec_train['gemm_bf16'][0]['A'] is tr.train_model.features_dev             # the first product of the forward
    assert rec_train['gemm_bf16'][0]['drop_a'] is not None                           # the recipe's input dropout rides on it
    assert [r for r in rec_train['gemm_bf16'] if r['form'] == "TN"][-1]['A'] is tr.train_model.features_dev


@pytest.mark.parametrize("kernel", ['cs', 'rows'])
def test_nopreprocess_the_first_aggregation_reads_the_table_itself(cases, kernel):
    case = cases['reddit3k_nopp'][0]
    tr = _trainer(case, full_batch=True, test_full_batch=True, full_batch_kernel=kernel, full_batch_dtype='bf16', **ON)
    n, f = case['n'], case['feats'].shape[1]
    rec_train, rec_eval = _step_and_eval(tr)
    for rec, model in ((rec_train, tr.train_model), (rec_eval, tr.test_model)):
        tab = model.features_dev
        assert tab.dtype == torch.bfloat16
        first = rec['spmm'][0]
        assert first['B'] is tab and first['kernel'] == ('spmm_cs' if kernel == 'cs' else 'spmm')
        assert len([r for r in rec['spmm'] if r['B'] is tab]) == 1                    # layer 0, forward; nothing else reads it
        assert (n, f) not in rec['operand_round']                                     # no rounding pass for the table
        assert rec['operand_round'], "the other products still round their fp32 operands (--full_batch_dtype bf16)"
        assert not any(r['A'].dtype == torch.bfloat16 for r in rec['gemm_bf16'])      # the dense layers sit behind the aggregator
    assert tr.train_static.matrix._scratch and f not in tr.train_static.matrix._scratch     # no scratch table of that width


def test_without_the_flag_nothing_receives_a_bf16_a(cases):
    for name in ('reddit3k_pp', 'reddit3k_nopp'):
        tr = _trainer(cases[name][0], full_batch=True, test_full_batch=True, full_batch_kernel='rows', **OFF)
        assert tr.train_model.features_dev.dtype == torch.float32 and tr.test_model.features_dev.dtype == torch.float32
        assert not tr.train_model.feature_bf16 and not tr.test_model.feature_bf16
        for rec in _step_and_eval(tr):
            assert rec['gemm_bf16'] and all(r['A'].dtype == torch.float32 for r in rec['gemm_bf16'])
            assert all(r['B'].dtype == torch.float32 for r in rec['spmm'])


# ---- 4. mixed mode -------------------------------------------------------------------------------------------------------------
def test_mixed_mode_leaves_the_sampled_training_model_alone(cases):
    case = cases['reddit3k_pp'][0]
    mixed = dict(cv=True, cvd=True, degree=1, batch_size=256, test_batch_size=256, max_steps=3, test_full_batch=True)
    weights = []
    for flags in (ON, dict(dense_dtype='bf16')):
        tr = _trainer(case, **mixed, **flags)
        assert tr.train_sch is not None and tr.full_batch is False
        assert tr.train_model.features_dev.dtype == torch.float32 and not tr.train_model.feature_bf16
        want = torch.bfloat16 if flags is ON else torch.float32
        assert tr.test_model.features_dev.dtype == want and tr.test_model.feature_bf16 == (flags is ON)
        tr.train_epoch()                                    # three sampled steps (--max_steps 3)
        torch.cuda.synchronize()
        weights.append(tr.train_model.theta.detach().view(torch.int32).cpu().clone())
        ev = tr.evaluate(tr.val_d)
        assert math.isfinite(float(ev[0]))
    assert torch.equal(weights[0], weights[1])
    assert bool(torch.isfinite(weights[0].view(torch.float32)).all())


def test_a_bf16_table_model_refuses_a_sampled_batch(cases):
    case = cases['reddit3k_pp'][0]
    tr = _trainer(case, full_batch=True, test_full_batch=True, full_batch_kernel='rows', **ON)
    with pytest.raises(ValueError, match="static batches only"):
        tr.train_model.upload({})


# ---- 5. train.main end to end ---------------------------------------------------------------------------------------------
def test_train_main_end_to_end(tmp_path, monkeypatch):
    from stochastic_gcn_amd import train
    from stochastic_gcn_amd.flags import FLAGS
    monkeypatch.chdir(tmp_path)
    FLAGS.reset()
    buf = io.StringIO()
    with recording() as rec, contextlib.redirect_stdout(buf):
        train.main(['--dataset', 's-reddit', '--scale', '0.01', '--normalization', 'graphsage', '--weight_decay', '0',
                    '--dropout', '0.2', '--layer_norm', '--hidden1', '32', '--num_fc_layers', '2', '--epochs', '3',
                    '--full_batch', '--test_full_batch', '--dense_dtype', 'bf16', '--feature_dtype', 'bf16'])
    assert any(r['A'].dtype == torch.bfloat16 for r in rec['gemm_bf16'])
    ep = [l.split() for l in buf.getvalue().splitlines() if l.startswith("Epoch:")]
    assert len(ep) == 5                   # the reference's exit is `epoch > FLAGS.epochs`: epochs + 2
    vals = [(float(t[3]), float(t[5]), float(t[7]), float(t[9])) for t in ep]       # train loss / acc, val loss / acc
    assert all(math.isfinite(v) for row in vals for v in row)
    print("train loss per epoch:", [v[0] for v in vals])
    assert re.search(r"Test set results: cost= (\d+\.\d{5}) accuracy= (\d+\.\d{5})", buf.getvalue())
