"""GPU parity of the whole training step (sampler -> DevFeed -> layers fwd -> loss -> bwd ->
Adam -> history scatter) against the NumPy oracle on the same seeded inputs and dropout masks:
every layer activation, loss, accuracy, all gradients, the updated weights and the updated
history, over 3 consecutive steps (step k reads the history step k-1 wrote).
Tolerance 1e-4 relative (max-norm) on activations (BASELINE.json north_star)."""
import numpy as np
import pytest
import torch

import model_cases as mc
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
TOL = 1e-4          # activations, loss, history (BASELINE.json north_star)
GRAD_TOL = 1e-4     # gradients, max-norm relative per tensor
PARAM_TOL = 5e-4    # Adam-updated weights on well-conditioned entries: lr * g / (|g| + 3e-7) amplifies the
                    # gradient's fp32 summation noise where |g| is small (tests/test_model_golden.py)


def _make_device_model(case, params, is_training=True):
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.vrgcn import VRGCN
    from stochastic_gcn_amd.plaingcn import PlainGCN
    FLAGS.reset()
    FLAGS.update(**{k: v for k, v in case['flags'].items() if hasattr(FLAGS, k)})
    cls = VRGCN if case['cfg']['model'] == 'vr' else PlainGCN
    fl = case['flags']
    m = cls(fl['num_layers'], fl['preprocess'], case['ph'], case['feats'], case['nbr'], case['adj'],
            fl['cvd'], is_training=is_training, device=torch.device('cuda:0'))
    m.set_params(params)
    return m


def _np(x):
    if isinstance(x, tuple):
        return tuple(_np(t) for t in x)
    if hasattr(x, 'csr'):
        return None
    if hasattr(x, 'materialize'):          # layers.Dropped: a pending (fused) dropout
        x = x.materialize()
    return x.detach().cpu().numpy()


def _masks(dmodel, keep):
    """The oracle replays the product's counter-based dropout masks (no hooks, no recording): the
    key of layer i at this step is dropout_key(seed, i, step) on both sides."""
    from oracle import model_np as mnp
    from stochastic_gcn_amd.flags import FLAGS
    return mnp.HashMasks(dmodel.dropout_seed, dmodel.dropout_step, keep)


@pytest.mark.parametrize("name", sorted(mc.CASES) + sorted(mc.DET_CASES))
def test_training_steps_match_oracle(name):
    from stochastic_gcn_amd.scheduler import PyScheduler
    case = mc.build_case(name)
    fl, c, ph = case['flags'], case['cfg'], case['ph']
    omodel = mc.make_oracle_model(case, seed=3)
    dmodel = _make_device_model(case, {k: v.copy() for k, v in omodel.params.items()})
    assert len(dmodel.layers) == len(omodel.specs)          # layer index i keys the same dropout site
    sch = mc.make_scheduler(case, 1)
    worst, well = 0.0, {}
    for step in range(3):
        feed = sch.minibatch(c['batch'])
        feed[ph['dropout']] = fl['dropout']
        masks = _masks(dmodel, 1.0 - fl['dropout'])
        o_loss, o_acc, o_pred, o_acts, o_grads = omodel.run_one_step(feed, ph, fl['dropout'], masks)
        outs = dmodel.run_one_step(None, feed)
        assert fl['dropout'] == 0 or masks.calls > 0
        # activations layer by layer
        d_acts = dmodel.activations[1:]
        assert len(d_acts) == len(o_acts)
        for li, (da, oa) in enumerate(zip(d_acts, o_acts)):
            da = _np(da)
            if da is None or hasattr(oa, 'tocsr'):
                continue
            if isinstance(oa, tuple):
                for dd, oo in zip(da, oa):
                    e = onp.rel_err(dd, oo); worst = max(worst, e)
                    assert e <= TOL, (name, step, li, e)
            else:
                e = onp.rel_err(da, oa); worst = max(worst, e)
                assert e <= TOL, (name, step, li, e)
        assert abs(outs[1] - float(o_loss)) <= 1e-4 * max(1.0, abs(float(o_loss))), (outs[1], o_loss)
        assert abs(outs[2] - float(o_acc)) <= 1e-6
        d_grads = dmodel.get_grads()
        for k, g in o_grads.items():
            e = onp.rel_err(d_grads[k], g)
            assert e <= GRAD_TOL, (name, step, 'grad', k, e)
        # Adam's first steps are sign-like (lr * g / (|g| + 1e-8)): a weight whose gradient is ~1e-8
        # amplifies fp32 summation-order noise, so weights are compared where |g| is above it
        d_params = dmodel.get_params()
        for k, v in omodel.params.items():
            well[k] = well.get(k, True) & (np.abs(o_grads[k]) > 1e-6)
            assert np.mean(well[k]) > 0.5
            assert np.abs(d_params[k] - v)[well[k]].max() <= 5e-4 * np.abs(v).max(), (name, step, 'param', k)
        for l, h in enumerate(omodel.history):
            e = onp.rel_err(dmodel.history[l][0].cpu().numpy(), h)
            assert e <= TOL, (name, step, 'history', l, e)
        for l, h in enumerate(omodel.history_var):          # det-dropout: the variance history (gcn/vrgcn.py:28)
            e = onp.rel_err(dmodel.history[l][1].cpu().numpy(), h)
            assert e <= TOL, (name, step, 'history_var', l, e)
    print("%s: worst activation rel err %.2e" % (name, worst))


def test_det_dropout_packed_batches_take_the_same_path():
    """Packed minibatches -- what the training loop produces -- of a det-dropout model run as a step program since round 6
    (ops GEMM .. GATE, ABI v16; the third adjacency = the sampled pattern with the packed medg weights, its transpose with
    the same weights in transposed order), reference-format feeds run layer by layer with the third adjacency rebuilt on
    the host: the same numbers."""
    from stochastic_gcn_amd.flags import FLAGS
    case = mc.build_case('det_cv_pp_L3')
    fl, c, ph = case['flags'], case['cfg'], case['ph']
    om = mc.make_oracle_model(case, seed=3)
    res = []
    for packed in (False, True):
        dm = _make_device_model(case, {k: v.copy() for k, v in om.params.items()})
        sch = mc.make_scheduler(case, 1)
        losses = []
        for step in range(3):
            if packed:
                pb = sch.minibatch_packed(c['batch'], FLAGS.plan_t, None)
                pb.dropout = fl['dropout']
                out = dm.run_one_step(None, pb)
            else:
                feed = sch.minibatch(c['batch'])
                feed[ph['dropout']] = fl['dropout']
                out = dm.run_one_step(None, feed)
            losses.append(out[1])
        progs = [v for v in (getattr(dm, '_programs', None) or {}).values()]
        assert (progs and all(v is not None and v.det for v in progs)) if (packed and FLAGS.native_step) else not progs
        res.append((losses, dm.get_params(), [h.cpu().numpy() for hs in dm.history for h in hs]))
    # (the two feeds carry different launch plans -- long rows are split differently -- so sums differ in their last bits)
    assert np.allclose(res[0][0], res[1][0], rtol=1e-5)
    for k in res[0][1]:
        assert onp.rel_err(res[0][1][k], res[1][1][k]) < 1e-4, k
    for a, b in zip(res[0][2], res[1][2]):
        assert onp.rel_err(a, b) < 1e-5
    assert len(res[0][2]) == 4 and all(np.abs(h).max() > 0 for h in res[0][2])     # two histories per layer, both written


GOLD = None


def _gold():
    global GOLD
    if GOLD is None:
        import golden_util as gu
        GOLD = gu.load("model_steps.npz")
    return GOLD


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_training_steps_match_independent_golden(name):
    """The HIP training step against golden vectors from an INDEPENDENT fp32 implementation (PyTorch-CPU
    ops + autograd, tests/golden/make_model_golden.py) -- not against this repo's own oracle: logits,
    aggregator outputs, loss, accuracy, every gradient, Adam-updated weights over 3 consecutive
    unsynchronised steps, and the final history."""
    from stochastic_gcn_amd.scheduler import PyScheduler
    from stochastic_gcn_amd.layers import PlainAggregator, VRAggregator
    gold = _gold()
    case = mc.build_case(name)
    fl, c, ph = case['flags'], case['cfg'], case['ph']
    params = mc.make_oracle_model(case, seed=3).params
    dmodel = _make_device_model(case, {k: v.copy() for k, v in params.items()})
    assert dmodel.dropout_seed == 1
    sch = mc.make_scheduler(case, 1)
    agg_index = [i for i, l in enumerate(dmodel.layers) if isinstance(l, (PlainAggregator, VRAggregator))]
    well, worst = {}, dict(act=0.0, grad=0.0, param=0.0)
    for step in range(3):
        feed = sch.minibatch(c['batch'])
        feed[ph['dropout']] = fl['dropout']
        key = "%s/s%d/" % (name, step)
        assert np.array_equal(feed[ph['fields'][0]], gold[key + "field0"])
        outs = dmodel.run_one_step(None, feed)
        acts = dmodel.activations[1:]
        e = onp.rel_err(_np(acts[-1]), gold[key + "logits"]); worst['act'] = max(worst['act'], e)
        assert e <= TOL, (name, step, 'logits', e)
        for l, li in enumerate(agg_index):
            a = _np(acts[li])
            a = a[0] if isinstance(a, tuple) else a
            e = onp.rel_err(a, gold[key + "agg%d" % l]); worst['act'] = max(worst['act'], e)
            assert e <= TOL, (name, step, 'agg', l, e)
        assert abs(outs[1] - float(gold[key + "loss"])) <= 1e-4 * max(1.0, abs(float(gold[key + "loss"])))
        assert abs(outs[2] - float(gold[key + "acc"])) <= 1e-6
        dg = dmodel.get_grads()
        for k in params:
            g = gold[key + "grad/" + k]
            e = onp.rel_err(dg[k], g); worst['grad'] = max(worst['grad'], e)
            assert e <= GRAD_TOL, (name, step, 'grad', k, e)
            well[k] = well.get(k, True) & (np.abs(g) > 1e-6)
        dp = dmodel.get_params()
        for k in params:
            gv = gold[key + "param/" + k]
            e = np.abs(dp[k] - gv)[well[k]].max() / np.abs(gv).max(); worst['param'] = max(worst['param'], e)
            assert e <= PARAM_TOL, (name, step, 'param', k, e)
    for l in range(len(dmodel.history)):
        assert onp.rel_err(dmodel.history[l][0].cpu().numpy(), gold["%s/history%d" % (name, l)]) <= TOL
    print("%s vs independent golden: worst rel err  activations %.1e  grads %.1e  params %.1e"
          % (name, worst['act'], worst['grad'], worst['param']))


@pytest.mark.parametrize("name", sorted(mc.DET_CASES))
def test_det_dropout_training_steps_match_independent_golden(name):
    """--det_dropout on the HIP path (csrc/sgcn_det.hip, layers.DetDropoutFC, the aggregators on (mean, variance)) against the
    INDEPENDENT fp32 golden (PyTorch-CPU ops + autograd of the reference's definitions, tests/golden/model_steps_det.npz) --
    the second implementation VERDICT r3 found missing for this variant: logits, both streams of every aggregator output,
    loss, accuracy, every gradient, the Adam-updated weights over 3 steps, both histories."""
    import os
    from stochastic_gcn_amd.layers import PlainAggregator, VRAggregator
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_steps_det.npz"))
    case = mc.build_case(name)
    fl, c, ph = case['flags'], case['cfg'], case['ph']
    params = mc.make_oracle_model(case, seed=3).params
    dmodel = _make_device_model(case, {k: v.copy() for k, v in params.items()})
    sch = mc.make_scheduler(case, 1)
    agg_index = [i for i, l in enumerate(dmodel.layers) if isinstance(l, (PlainAggregator, VRAggregator))]
    well, worst = {}, dict(act=0.0, grad=0.0, param=0.0)
    for step in range(3):
        feed = sch.minibatch(c['batch'])
        feed[ph['dropout']] = fl['dropout']
        key = "%s/s%d/" % (name, step)
        assert np.array_equal(feed[ph['fields'][0]], gold[key + "field0"])
        outs = dmodel.run_one_step(None, feed)
        acts = dmodel.activations[1:]
        e = onp.rel_err(_np(acts[-1]), gold[key + "logits"]); worst['act'] = max(worst['act'], e)
        assert e <= TOL, (name, step, 'logits', e)
        for l, li in enumerate(agg_index):
            a = _np(acts[li])
            e = onp.rel_err(a[0] if isinstance(a, tuple) else a, gold[key + "agg%d" % l]); worst['act'] = max(worst['act'], e)
            assert e <= TOL, (name, step, 'agg', l, e)
            if isinstance(a, tuple):
                e = onp.rel_err(a[1], gold[key + "aggvar%d" % l]); worst['act'] = max(worst['act'], e)
                assert e <= TOL, (name, step, 'agg variance', l, e)
        assert abs(outs[1] - float(gold[key + "loss"])) <= 1e-4 * max(1.0, abs(float(gold[key + "loss"])))
        assert abs(outs[2] - float(gold[key + "acc"])) <= 1e-6
        dg = dmodel.get_grads()
        for k in params:
            g = gold[key + "grad/" + k]
            e = onp.rel_err(dg[k], g); worst['grad'] = max(worst['grad'], e)
            assert e <= GRAD_TOL, (name, step, 'grad', k, e)
            well[k] = well.get(k, True) & (np.abs(g) > 1e-6)
        dp = dmodel.get_params()
        for k in params:
            gv = gold[key + "param/" + k]
            e = np.abs(dp[k] - gv)[well[k]].max() / np.abs(gv).max(); worst['param'] = max(worst['param'], e)
            assert e <= PARAM_TOL, (name, step, 'param', k, e)
    for l in range(len(dmodel.history)):
        assert onp.rel_err(dmodel.history[l][0].cpu().numpy(), gold["%s/history%d" % (name, l)]) <= TOL
        assert onp.rel_err(dmodel.history[l][1].cpu().numpy(), gold["%s/history_var%d" % (name, l)]) <= TOL
    print("%s vs independent golden: worst rel err  activations %.1e  grads %.1e  params %.1e"
          % (name, worst['act'], worst['grad'], worst['param']))


@pytest.mark.parametrize("which", ["cora", "pubmed"])
def test_planetoid_configs_at_full_size_match_oracle(which):
    """BASELINE configs 1 and 2 at their SURVEY.md 8d sizes (S-Cora: N = 2,708, 1,433 sparse features,
    exact PlainGCN degree 20; S-PubMed: N = 19,717, 500 sparse features, CVD+PP degree 1): sparse first
    layer (K9) with sparse dropout (K12), 3 consecutive unsynchronised steps vs the oracle."""
    case = mc.planetoid_case(which)
    fl, c, ph = case['flags'], case['cfg'], case['ph']
    omodel = mc.make_oracle_model(case, seed=3)
    dmodel = _make_device_model(case, {k: v.copy() for k, v in omodel.params.items()})
    sch = mc.make_scheduler(case, 1)
    well, worst = {}, dict(act=0.0, grad=0.0)
    for step in range(3):
        sch.start = 0                       # one batch = the whole train set, every epoch
        feed = sch.minibatch(1000)
        assert feed[ph['fields'][-1]].shape[0] == c['batch']
        feed[ph['dropout']] = fl['dropout']
        masks = _masks(dmodel, 1.0 - fl['dropout'])
        o_loss, o_acc, _, o_acts, o_grads = omodel.run_one_step(feed, ph, fl['dropout'], masks)
        outs = dmodel.run_one_step(None, feed)
        for da, oa in zip(dmodel.activations[1:], o_acts):
            da = _np(da)
            if da is None or hasattr(oa, 'tocsr'):
                continue
            for dd, oo in (zip(da, oa) if isinstance(oa, tuple) else [(da, oa)]):
                e = onp.rel_err(dd, oo); worst['act'] = max(worst['act'], e)
                assert e <= TOL, (which, step, e)
        assert abs(outs[1] - float(o_loss)) <= 1e-4 * max(1.0, abs(float(o_loss)))
        assert abs(outs[2] - float(o_acc)) <= 1e-6
        dg = dmodel.get_grads()
        for k, g in o_grads.items():
            e = onp.rel_err(dg[k], g); worst['grad'] = max(worst['grad'], e)
            assert e <= GRAD_TOL, (which, step, k, e)
            well[k] = well.get(k, True) & (np.abs(g) > 1e-6)
        dp = dmodel.get_params()
        for k, v in omodel.params.items():
            assert np.abs(dp[k] - v)[well[k]].max() <= PARAM_TOL * np.abs(v).max(), (which, step, k)
        for l, h in enumerate(omodel.history):
            assert onp.rel_err(dmodel.history[l][0].cpu().numpy(), h) <= TOL
    print("S-%s at full size: worst rel err activations %.1e grads %.1e" % (which, worst['act'], worst['grad']))


def test_eval_model_shares_weights_and_keeps_own_history():
    """tf.make_template semantics (gcn/train.py:115-119): the test model reuses the train
    model's weights but owns a separate history; eval = forward + history scatter only."""
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.models import make_template
    from stochastic_gcn_amd.vrgcn import VRGCN
    from stochastic_gcn_amd.scheduler import PyScheduler
    case = mc.build_case('reddit_cvd_pp')
    fl, c, ph = case['flags'], case['cfg'], case['ph']
    FLAGS.reset()
    FLAGS.update(**{k: v for k, v in fl.items() if hasattr(FLAGS, k)})
    dev = torch.device('cuda:0')

    def model_func(nbr, is_training, _store=None):
        return VRGCN(fl['num_layers'], True, ph, case['feats'], nbr, case['adj'], True,
                     is_training=is_training, device=dev, _store=_store)
    create = make_template('model', model_func)
    train_m = create(case['nbr'], True)
    test_m = create(case['nbr'], False)
    assert test_m.theta.data_ptr() == train_m.theta.data_ptr()
    assert test_m.history[0][0].data_ptr() != train_m.history[0][0].data_ptr()
    sch = PyScheduler(case['adj'], case['labels'], 1, [1], ph, 1, data=case['train'].copy(), cv=True)
    feed = sch.minibatch(c['batch'])
    before = train_m.theta.clone()
    loss, acc, pred = test_m.run_one_step(None, feed)
    assert torch.equal(before, train_m.theta)                       # eval never touches weights
    assert pred.shape == (c['batch'], c['classes']) and np.allclose(pred.sum(1), 1, atol=1e-5)
    f0 = feed[ph['fields'][0]]
    assert float(test_m.history[0][0][torch.from_numpy(f0).long().to(dev)].abs().sum()) > 0
    assert float(train_m.history[0][0].abs().sum()) == 0.0
    # oracle agreement for the eval step
    om = mc.make_oracle_model(case, params=train_m.get_params(), is_training=False)
    o_loss, o_acc, o_pred, _, _ = om.run_one_step(feed, ph, 0.0, lambda *a: None)
    assert onp.rel_err(pred, o_pred) <= TOL and abs(loss - float(o_loss)) <= 1e-4


def test_save_load_roundtrip(tmp_path):
    case = mc.build_case('reddit_cvd_pp')
    om = mc.make_oracle_model(case, seed=1)
    m = _make_device_model(case, om.params)
    m.history[0][0].normal_()
    p = m.save(path=str(tmp_path / "m.ckpt.npz"))
    m2 = _make_device_model(case, mc.make_oracle_model(case, seed=2).params)
    m2.load(path=p, load_history=True)
    assert torch.equal(m.theta, m2.theta) and torch.equal(m.history[0][0], m2.history[0][0])


BAND = 3e-5      # |pre-activation| below this: the device's ReLU gate may legitimately differ from the oracle's


def _gate_interval(om, dlogits):
    """Gradient interval of the oracle over every assignment of its AMBIGUOUS ReLU gates.

    A ReLU input within fp32 rounding of 0 has no determined gate -- summation order decides it -- and a
    gate switches a whole gradient contribution on or off.  Nothing is taken from the device: the
    oracle's own pre-activations define the ambiguous set S = {|pre| < BAND}; the gradient is affine in
    the gate vector, grad = g0 + sum_s gate_s * c_s, so with g0 (all of S off) and one backward pass per
    element (c_s) the device's gradient must lie in  [g0 + sum min(0, c_s), g0 + sum max(0, c_s)]
    whatever gates it took.  Returns (lo, hi, |S|)."""
    amb = {}

    def scan(name, pre):
        amb[name] = np.argwhere(np.abs(pre) < BAND)
        return pre > 0
    om.relu_gate_hook = scan
    om.backward(dlogits)
    S = [(n, tuple(ix)) for n, arr in amb.items() for ix in arr]

    def run(on):
        def hook(name, pre):
            g = pre > 0
            for ix in amb[name]:
                g[tuple(ix)] = (name, tuple(ix)) == on
            return g
        om.relu_gate_hook = hook
        return om.backward(dlogits)
    g0 = run(None)
    lo = {k: v.copy() for k, v in g0.items()}
    hi = {k: v.copy() for k, v in g0.items()}
    for s_ in S:
        gs = run(s_)
        for k in g0:
            c = gs[k] - g0[k]
            lo[k] += np.minimum(c, 0)
            hi[k] += np.maximum(c, 0)
    om.relu_gate_hook = None
    return lo, hi, len(S)


def test_full_size_reddit_cvd_pp_steps_match_oracle():
    """BASELINE config 3 at FULL size (S-Reddit: N = 232,965, 602 features, reddit.config flags +
    --cv --cvd --degree=1, batch 512): THREE CONSECUTIVE training steps, device vs NumPy oracle, each
    side on its own weights, Adam moments and history throughout -- the PP product, every layer
    activation, loss, gradients, Adam-updated weights and the 119 MB history.  NOTHING the device
    computed enters the oracle: not its forward pass, not its backward pass, not its weights (round 2
    still took 14 % of the Adam-updated weights from the device).

    Two things are ill-conditioned at this size and are handled explicitly instead of by loose
    tolerances or by steering the oracle:
    (1) with ~330k ReLU inputs per step a few land within fp32 rounding of 0 and their gate switches
        a gradient contribution on or off -- the device's gradient is required to lie in the oracle's
        gradient INTERVAL over all assignments of those gates (_gate_interval);
    (2) Adam's first steps are sign-like (lr * g / (|g| + 3e-7)), so a weight's update is DETERMINED
        at fp32 only where |g| is above its noise floor and where the entry's BUDGET -- Adam's
        sensitivity (|d update / d g| <= lr / (|g| + 3e-7), doubled) times the width of its gate
        interval -- stays small.  Determined weights are compared at PARAM_TOL plus their budget.  The
        undetermined rest -- where two correct fp32 implementations may differ by a fraction of lr --
        is checked against Adam's own bound (|update| <= ~lr per step) and then LEFT ALONE on both
        sides.  What that does to the NEXT step is measured on the oracle alone, with a TWIN: a second
        oracle instance that takes the same steps on its own weights, moments and history, except that
        its gradients carry noise of 1e-5 of each tensor's max-norm before Adam sees them -- the level
        at which the device's gradients agree with the oracle's (measured: 9e-6), i.e. the twin is "an
        implementation that meets the gradient parity claim".  The relative distance D of the twin's
        layer activations from the oracle's is how far two such implementations drift apart through
        Adam's sign-like first steps; steps 2 and 3 compare activations at TOL + 3 D and gradients at
        GRAD_TOL + 3 D (step 1: D = 0, i.e. the plain tolerances).  D is printed and bounded."""
    from stochastic_gcn_amd import synthetic, ops
    from stochastic_gcn_amd.scheduler import PyScheduler
    from oracle import model_np as mnp
    n, train_adj, full_adj, _, _, _, labels, tr, va, te = synthetic.reddit_like(with_features=False)
    rng = np.random.RandomState(0)
    feats = rng.standard_normal((n, 602)).astype(np.float32)
    nbr = train_adj.dot(feats).astype(np.float32)            # PP product, SciPy (gcn/utils.py:321)
    fl = mnp.make_flags(normalization='graphsage', weight_decay=0.0, dropout=0.2, layer_norm=True,
                        hidden1=128, num_fc_layers=2, cv=True, cvd=True, degree=1, preprocess=True)
    ph = mc.placeholders(1, 41)
    case = dict(cfg=dict(model='vr', n=n, classes=41), flags=fl, adj=train_adj, feats=feats, nbr=nbr,
                labels=labels, ph=ph)
    probe = mnp.Model(fl, 2, True, True, True, feats, nbr, n, 41, {})
    om = mnp.Model(fl, 2, True, True, True, feats, nbr, n, 41, mnp.init_params(probe.specs, 1))
    twin = mnp.Model(fl, 2, True, True, True, feats, nbr, n, 41, {k: v.copy() for k, v in om.params.items()})
    dm = _make_device_model(case, {k: v.copy() for k, v in om.params.items()})
    dev = torch.device('cuda:0')
    # the PP product itself at full size: both HIP SpMM kernels vs SciPy
    Xd = torch.zeros((n, 604), device=dev)[:, :602]
    Xd.copy_(torch.from_numpy(feats))
    pp = ops.spmm(ops.DeviceCSR.from_scipy(train_adj, dev), Xd)
    assert onp.rel_err(pp.cpu().numpy(), nbr) <= TOL
    pp = ops.spmm_cs(ops.ColumnSweepCSR(train_adj, dev), Xd)
    assert onp.rel_err(pp.cpu().numpy(), nbr) <= TOL
    del pp, Xd
    sch = PyScheduler(train_adj, labels, 1, [1], ph, 1, data=tr.copy(), cv=True)
    prng = np.random.RandomState(99)
    n_amb, n_und, n_w, worst, drift, drift_g = 0, 0, 0, dict(act=0.0, grad_excess=0.0, param=0.0), [], []
    for step in range(3):
        feed = sch.minibatch(512)
        feed[ph['dropout']] = 0.2
        step_id = dm.dropout_step                            # the dropout keys of THIS step (the device advances its counter)
        mk = lambda: mnp.HashMasks(dm.dropout_seed, step_id, 0.8)          # noqa: E731
        outs = dm.run_one_step(None, feed)
        d_acts, dg = [_np(a) for a in dm.activations[1:]], dm.get_grads()
        masks = mk()
        logits, o_acts = om.forward(feed, ph, 0.2, masks)
        assert masks.calls == 4
        # the twin's step (oracle alone: the device is not consulted), and how far it has drifted
        t_logits, t_acts = twin.forward(feed, ph, 0.2, mk())
        D = 0.0
        for pa, oa in zip(t_acts, o_acts):
            for pp_, oo in (zip(pa, oa) if isinstance(oa, tuple) else [(pa, oa)]):
                D = max(D, onp.rel_err(pp_, oo))
        drift.append(D)
        _, _, _, t_dlogits = twin.loss_and_grad(t_logits, feed[ph['labels']])
        t_grads = twin.backward(t_dlogits)
        o_loss, o_acc, _, dlogits = om.loss_and_grad(logits, feed[ph['labels']])
        lo, hi, k_amb = _gate_interval(om, dlogits)
        n_amb += k_amb
        o_grads = om.backward(dlogits)               # the oracle's own gates
        Dg = max(onp.rel_err(t_grads[k], o_grads[k]) for k in o_grads)          # the twin's gradient drift (0 at step 1)
        drift_g.append(Dg)
        twin.adam_step({k: (g + 1e-5 * np.abs(g).max() * prng.standard_normal(g.shape)).astype(np.float32) for k, g in t_grads.items()})
        twin.update_history(feed, ph)
        om.adam_step(o_grads)
        om.update_history(feed, ph)
        for da, oa in zip(d_acts, o_acts):
            for dd, oo in (zip(da, oa) if isinstance(oa, tuple) else [(da, oa)]):
                e = onp.rel_err(dd, oo); worst['act'] = max(worst['act'], e - 3 * D)
                assert e <= TOL + 3 * D, (step, e, D)
        assert abs(outs[1] - float(o_loss)) <= (1e-4 + 3 * D) * max(1.0, abs(float(o_loss)))
        dp = dm.get_params()
        for k, g in o_grads.items():
            tol = (GRAD_TOL + 3 * Dg) * np.abs(g).max()
            excess = max(float((lo[k] - dg[k]).max()), float((dg[k] - hi[k]).max()), 0.0) / np.abs(g).max()
            worst['grad_excess'] = max(worst['grad_excess'], excess - 3 * Dg)
            assert np.all(dg[k] >= lo[k] - tol) and np.all(dg[k] <= hi[k] + tol), (step, k, excess, Dg)
            v = om.params[k]
            wmax = np.abs(v).max()
            budget = 2.0 * fl['learning_rate'] * (hi[k] - lo[k]) / (np.abs(g) + 3e-7)
            det = (np.abs(g) > 1e-6) & (budget <= 10 * PARAM_TOL * wmax)
            err = np.abs(dp[k] - v)
            if step == 0:        # one Adam step from identical weights: the determined entries must agree
                e = float((err - budget)[det].max(initial=0.0) / wmax); worst['param'] = max(worst['param'], e)
                assert e <= PARAM_TOL, (step, k, e)
                n_und += int((~det).sum()); n_w += det.size
            # every entry: inside Adam's own bound (each side moved it by at most ~lr per step); nothing is copied
            assert err.max(initial=0.0) <= 2.5 * fl['learning_rate'] * (step + 1), (step, k)
        idx = feed[ph['fields'][0]]
        assert onp.rel_err(dm.history[0][0][torch.from_numpy(idx).long().to(dev)].cpu().numpy(),
                           om.history[0][idx]) <= TOL + 3 * D
    assert onp.rel_err(dm.history[0][0].cpu().numpy(), om.history[0]) <= TOL + 3 * max(drift)
    print("full-size parity, 3 unsynchronised steps, nothing fed from the device: %d ambiguous ReLU gates (|pre| < %.0e); "
          "twin drift per step: activations %s gradients %s; worst rel err beyond 3 x drift: activations %.1e  gradient "
          "outside the gate interval %.1e; step-1 determined weights %.1e, %.2f %% of the first weight updates undetermined at "
          "fp32 (left alone on both sides)"
          % (n_amb, BAND, ["%.1e" % d for d in drift], ["%.1e" % d for d in drift_g], worst['act'], worst['grad_excess'],
             worst['param'], 100.0 * n_und / max(n_w, 1)))
    # step 1 is the strict one (no drift yet); the later steps are bounded by what Adam's sign-like first updates do to ANY
    # two implementations that agree on gradients to 1e-5 (the twin): a few per cent by step 3
    assert drift[0] == 0.0 and drift_g[0] == 0.0 and max(drift) <= 0.1 and n_und <= 0.25 * n_w
    # ---- the history path across steps, STRICT: the same three-step run with the learning rate at 0 ----------------
    # (weights stay put on both sides, so nothing is ill-conditioned; the control-variate history is not: step k's
    # aggregator reads the rows steps < k scattered, on each side from its own 119 MB history)
    from stochastic_gcn_amd.flags import FLAGS
    fl0 = dict(fl, learning_rate=0.0)
    om0 = mnp.Model(fl0, 2, True, True, True, feats, nbr, n, 41, mnp.init_params(probe.specs, 1))
    dm0 = _make_device_model(dict(case, flags=fl0), {k: v.copy() for k, v in om0.params.items()})
    assert FLAGS.learning_rate == 0.0
    sch0 = PyScheduler(train_adj, labels, 1, [1], ph, 1, data=tr.copy(), cv=True)
    worst0, touched = 0.0, 0
    for step in range(3):
        feed = sch0.minibatch(512)
        feed[ph['dropout']] = 0.2
        step_id = dm0.dropout_step
        outs = dm0.run_one_step(None, feed)
        d_acts = [_np(a) for a in dm0.activations[1:]]
        o_loss, _, _, o_acts, _ = om0.run_one_step(feed, ph, 0.2, mnp.HashMasks(dm0.dropout_seed, step_id, 0.8))
        for da, oa in zip(d_acts, o_acts):
            for dd, oo in (zip(da, oa) if isinstance(oa, tuple) else [(da, oa)]):
                e = onp.rel_err(dd, oo); worst0 = max(worst0, e)
                assert e <= TOL, ("lr = 0", step, e)
        assert abs(outs[1] - float(o_loss)) <= 1e-4 * max(1.0, abs(float(o_loss)))
        touched += len(feed[ph['fields'][0]])
    for k, v in om0.params.items():
        np.testing.assert_array_equal(dm0.get_params()[k], v)               # (nothing moved)
    assert onp.rel_err(dm0.history[0][0].cpu().numpy(), om0.history[0]) <= TOL and float(np.abs(om0.history[0]).sum()) > 0
    print("full-size history path, 3 unsynchronised steps at learning rate 0 (%d history rows written, read back by later "
          "steps): worst activation rel err %.1e" % (touched, worst0))


@pytest.mark.parametrize("mode,degree", [("NS", 20), ("Exact", 10000)])
def test_full_size_non_pp_two_hops_match_oracle(mode, degree):
    """SURVEY.md 8f f-4 AT SCALE (it existed only as a probe): the full S-Reddit graph (N = 232,965, 602
    features), NO preprocessing, two sampled hops -- neighbour sampling with degree 20 (512 -> ~10 k -> ~106 k vertices,
    ~200 k sampled edges: the true "sampled SpMM" regime of K1) and Exact (degree 10000: the receptive field is most of
    the graph, all 154 k training vertices, 2.9 M edges in the input-side hop) -- PlainGCN, graphsage concat, LayerNorm, dropout 0.2: one training
    step, device vs NumPy oracle.  Forward (every layer activation, loss, accuracy) at 1e-4.  Gradients: with 13-30 M
    ReLU inputs a few hundred land within fp32 rounding of zero and their gates are not determined (the enumeration of
    the batch-512 CVD test would need hundreds of backward passes here), so they are compared at 2e-4 of each tensor's
    max-norm (measured: 6e-6 / 6e-5)."""
    from stochastic_gcn_amd import synthetic
    from stochastic_gcn_amd.scheduler import PyScheduler
    from oracle import model_np as mnp
    n, train_adj, _, _, _, _, labels, tr, _, _ = synthetic.reddit_like(with_features=False)
    rng = np.random.RandomState(0)
    feats = rng.standard_normal((n, 602)).astype(np.float32)
    fl = mnp.make_flags(normalization='graphsage', weight_decay=0.0, dropout=0.2, layer_norm=True, hidden1=128,
                        num_fc_layers=1, cv=False, cvd=False, degree=degree, preprocess=False, num_layers=2)
    ph = mc.placeholders(2, 41)
    case = dict(cfg=dict(model='plain', n=n, classes=41), flags=fl, adj=train_adj, feats=feats, nbr=feats, labels=labels, ph=ph)
    probe = mnp.Model(fl, 2, False, False, False, feats, feats, n, 41, {})
    om = mnp.Model(fl, 2, False, False, False, feats, feats, n, 41, mnp.init_params(probe.specs, 1))
    dm = _make_device_model(case, {k: v.copy() for k, v in om.params.items()})
    sch = PyScheduler(train_adj, labels, 2, [degree, degree], ph, 1, data=tr.copy(), cv=False)
    feed = sch.minibatch(512)
    feed[ph['dropout']] = 0.2
    sizes = [int(feed[ph['fields'][l]].shape[0]) for l in range(3)]
    edges = [int(feed[ph['adj'][l]][1].shape[0]) for l in range(2)]
    assert sizes[2] == 512 and sizes[0] > (100000 if mode == "Exact" else 50000) and edges[0] > (2_000_000 if mode == "Exact" else 150_000)
    masks = _masks(dm, 0.8)
    outs = dm.run_one_step(None, feed)
    d_acts, dg = [_np(a) for a in dm.activations[1:]], dm.get_grads()
    o_loss, o_acc, _, o_acts, o_grads = om.run_one_step(feed, ph, 0.2, masks)
    worst = 0.0
    for da, oa in zip(d_acts, o_acts):
        for dd, oo in (zip(da, oa) if isinstance(oa, tuple) else [(da, oa)]):
            e = onp.rel_err(dd, oo); worst = max(worst, e)
            assert e <= TOL, (mode, e)
    assert abs(outs[1] - float(o_loss)) <= 1e-4 * max(1.0, abs(float(o_loss))) and abs(outs[2] - float(o_acc)) <= 1e-6
    gw = max(onp.rel_err(dg[k], g) for k, g in o_grads.items())
    assert gw <= 2e-4, (mode, gw)
    print("full-size %s, no PP, 2 hops: fields %s, sampled edges %s; worst rel err activations %.1e, gradients %.1e"
          % (mode, sizes, edges, worst, gw))
