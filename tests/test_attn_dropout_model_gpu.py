"""GPU tests of --attn_dropout in the model: three unsynchronised training steps of two tiny stacks (one of them with
--attn_heads 2) against an fp64-accumulating restatement that replays the coefficient masks from their NumPy restatement
(tests/attn_dropout_cases.py; the condition that makes the comparison well-posed is decided on the CPU, in
tests/test_spattn_drop.py), with the tolerance tests/test_attn_aggregator_gpu.py applies; an evaluation that is bit for bit the
evaluation without the flag; two training runs that give the same weights; and --attn_dropout 0 as the run without the flag.
Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import attn_dropout_cases as dx
import full_batch_cases as fc
import spattn_ref as ref
from oracle import model_np as mnp
from oracle import oracle_np as onp
from test_attn_aggregator_gpu import TOL          # the project's standing tolerance for model steps, taken from there

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ATTN = dict(aggregator='attn', full_batch=True, test_full_batch=True)


@pytest.fixture(autouse=True)
def _reset_flags():
    from stochastic_gcn_amd.flags import FLAGS
    FLAGS.reset()
    yield
    FLAGS.reset()


def _np(x):
    if hasattr(x, 'materialize'):
        x = x.materialize()
    return x.detach().cpu().numpy()


def _flags(case, **over):
    fl = dict(ATTN, attn_heads=case['heads'], attn_dropout=case['attn_dropout'])
    fl.update(over)
    return fl


def _static_batch(case, adj, model, rows):
    from stochastic_gcn_amd.full_batch import StaticBatch, model_matrix
    mat = model_matrix(adj, DEV, model, 3)
    return mat, StaticBatch(mat, case['labels'], np.sort(rows), model.L, DEV)


def _train(case, params, steps=3, **over):
    """the device model after ``steps`` training steps from ``params``: (model, its logits of the last step)"""
    adj, rows = case['train_adj'], np.sort(case['train'])
    dm = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in params.items()}, extra_flags=_flags(case, **over))
    _, sb = _static_batch(case, adj, dm, rows)
    sb.dropout = case['flags']['dropout']
    for _ in range(steps):
        dm.run_one_step(None, sb)
    return dm, _np(dm.activations[-1])


@pytest.mark.parametrize("name", sorted(dx.CASES))
def test_three_steps_match_the_reference(name):
    assert TOL == 1e-4
    case = dx.build(name)
    fl = case['flags']
    adj, rows = case['train_adj'], np.sort(case['train'])
    om = dx.reference_model(case, case['nbr_train'])
    dm = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in om.params.items()}, extra_flags=_flags(case))
    assert len(dm.layers) == len(om.specs)                 # no layer was inserted: the activation dropouts keep their keys
    assert [l.index for l in dm.layers] == list(range(len(dm.layers)))
    mat, sb = _static_batch(case, adj, dm, rows)
    sb.dropout = fl['dropout']
    feed = fc.exact_feed(case, adj, fl['dropout'])
    worst = dict(act=0.0, grad=0.0, param=0.0, loss=0.0)
    for step in range(3):
        masks = mnp.HashMasks(dm.dropout_seed, dm.dropout_step, 1.0 - fl['dropout'])
        assert (dm.dropout_seed, dm.dropout_step) == (1, step)                 # what attn_dropout_cases.margin replayed
        outs = dm.run_one_step(None, sb)
        d_acts, dg, dp = [_np(a) for a in dm.activations[1:]], dm.get_grads(), dm.get_params()
        logits, o_acts, o_loss, o_acc, o_grads = dx.reference_step(om, case, feed, rows, fl['dropout'], masks, 1, step)
        for kind, li, small, big in om.margins:
            print("%s step %d %s layer %d: smallest non-zero margin %.3e of largest input %.3e" % (name, step, kind, li, small, big))
            assert not np.isfinite(small) or small >= dx.MARGIN * big             # the condition the seed was chosen under
        assert len(d_acts) == len(o_acts) and masks.calls > 0
        for li, (da, oa) in enumerate(zip(d_acts, o_acts)):
            e = onp.rel_err(da, oa)
            worst['act'] = max(worst['act'], e)
            print("%s step %d layer %d rel_err %.3e" % (name, step, li, e))
            assert da.shape == oa.shape and e <= TOL, (name, step, li, e)
        print("%s step %d loss %.7f (reference %.7f)  acc %.6f (%.6f)" % (name, step, outs[1], o_loss, outs[2], o_acc))
        worst['loss'] = max(worst['loss'], abs(outs[1] - o_loss) / max(abs(o_loss), 1e-30))
        assert abs(outs[1] - o_loss) <= TOL * abs(o_loss) and abs(outs[2] - o_acc) <= 1e-6
        for k, g in o_grads.items():
            e = onp.rel_err(dg[k], g)
            worst['grad'] = max(worst['grad'], e)
            print("%s step %d grad %s rel_err %.3e" % (name, step, k, e))
            assert e <= TOL, (name, step, 'grad', k, e)
        for k, v in om.params.items():
            e = onp.rel_err(dp[k], v)
            worst['param'] = max(worst['param'], e)
            print("%s step %d param %s rel_err %.3e" % (name, step, k, e))
            assert e <= TOL, (name, step, 'param', k, e)
        # every aggregation layer ran under the key of (seed, its own index, this step), forward and backward
        from stochastic_gcn_amd import ops
        for a in dm.aggregators:
            assert a._drop == dict(keep=1.0 - case['attn_dropout'], key=ops.attn_key(1, a.index, step))
    print("%s: worst rel err  activations %.1e  loss %.1e  grads %.1e  params %.1e"
          % (name, worst['act'], worst['loss'], worst['grad'], worst['param']))
    # the comparison is not vacuous: without the masks the reference is somewhere else
    off = dx.reference_model(case, case['nbr_train'], attn_dropout=0.0)
    for step in range(3):
        dx.reference_step(off, case, feed, rows, fl['dropout'], mnp.HashMasks(1, step, 1.0 - fl['dropout']), 1, step)
    far = max(onp.rel_err(off.params[k], v) for k, v in om.params.items())
    print("%s: the unmasked reference's weights differ by %.1e" % (name, far))
    assert far > 10 * TOL


@pytest.mark.parametrize("name", sorted(dx.CASES))
def test_evaluation_is_the_evaluation_without_the_flag(name):
    """the weights after three masked training steps, evaluated with the flag on and off: the same bits, no mask, no lse"""
    case = dx.build(name)
    adj, rows = case['train_adj'], np.sort(case['train'])
    dm, _ = _train(case, dx.reference_model(case, case['nbr_train']).params)
    params = dm.get_params()
    logits = {}
    for p in (case['attn_dropout'], 0.0):
        tm = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in params.items()}, is_training=False,
                             extra_flags=_flags(case, attn_dropout=p))
        _, sbt = _static_batch(case, adj, tm, rows)
        outs = tm.run_one_step(None, sbt)
        assert np.isfinite(outs[0])
        assert all(a._attn and a._lse is None and a._drop == {} for a in tm.aggregators)
        logits[p] = _np(tm.activations[-1])
    assert ref.same_bits(logits[case['attn_dropout']], logits[0.0])
    om = dx.reference_model(case, case['nbr_train'], params={k: v.copy() for k, v in params.items()}, is_training=False)
    want, _ = om.forward(fc.exact_feed(case, adj, 0.0), case['ph'], 0.0, None)
    e = onp.rel_err(logits[0.0], want)
    print("%s evaluation logits rel_err %.3e" % (name, e))
    assert e <= TOL


@pytest.mark.parametrize("name", sorted(dx.CASES))
def test_training_is_reproducible_and_zero_is_off(name):
    case = dx.build(name)
    init = dx.reference_model(case, case['nbr_train']).params
    a, la = _train(case, init)
    b, lb = _train(case, init)
    pa, pb = a.get_params(), b.get_params()
    assert all(ref.same_bits(pa[k], pb[k]) for k in pa) and ref.same_bits(la, lb)       # two runs: identical weights
    # --attn_dropout 0 is the run without the flag, bit for bit -- and not the run with it
    zero, lz = _train(case, init, attn_dropout=0.0)
    fl = dict(ATTN, attn_heads=case['heads'])
    adj, rows = case['train_adj'], np.sort(case['train'])
    plain = fc.device_model(case, case['nbr_train'], adj, {k: v.copy() for k, v in init.items()}, extra_flags=fl)
    _, sb = _static_batch(case, adj, plain, rows)
    sb.dropout = case['flags']['dropout']
    for _ in range(3):
        plain.run_one_step(None, sb)
    pz, pp = zero.get_params(), plain.get_params()
    assert all(ref.same_bits(pz[k], pp[k]) for k in pz) and ref.same_bits(lz, _np(plain.activations[-1]))
    assert all(a_._drop == {} for a_ in zero.aggregators)
    assert any(not ref.same_bits(pa[k], pz[k]) for k in pa)
