"""GPU tests of --edge_dropout: the re-draw kernel against its NumPy restatement bit for bit, the products of every
static-graph kernel on re-drawn values against the same kernel's plan of the HOST-masked matrix bit for bit, full-graph
training steps against the oracle fed the host-masked adjacency of each step, and the isolation of everything that is not
a training step.  The mask is restated in tests/edge_mask_ref.py; every figure is printed before it is asserted."""
import contextlib
import io

import numpy as np
import pytest
import torch

import edge_mask_ref as ref
import full_batch_cases as fc
import gpu_checks
import sparse_cases as sc
from oracle import model_np as mnp
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TOL = 1e-4                       # the gate of tests/test_full_batch_gpu.py
NAN_FILL = 0x7FC0BEEF            # what ``out`` holds before a call


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [0.5, 0.8, 1.0])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 70001])
def test_revalue_kernel_matches_the_restatement_bit_for_bit(n, keep):
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(100 + n)
    key = ref.edge_key(1, n % 7)
    for off in (0, 1):            # 16-byte aligned arrays (four entries per lane) and arrays one element off (one per lane)
        base = rng.standard_normal(n).astype(np.float32)
        pair = rng.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        pair[pair == ref.ALWAYS] = ref.ALWAYS - 1
        always = np.nonzero(rng.rand(n) < 0.2)[0]
        pair[always] = ref.ALWAYS
        base.view(np.uint32)[always[0::3]] = ref.PAD_BITS          # -0.0f pad markers under ALWAYS
        base[always[1::3]] = np.nan                                # NaN under ALWAYS
        if n >= 1:
            pair[0], base.view(np.uint32)[0] = ref.ALWAYS, ref.PAD_BITS
        if n >= 2:
            pair[1], base[1] = ref.ALWAYS, np.nan
        if n >= 3:
            pair[2], base[2] = 12345, -1.5
        assert n < 3 or (base[pair != ref.ALWAYS] < 0).any()
        assert not np.any(base.view(np.uint32)[pair != ref.ALWAYS] == ref.PAD_BITS)
        total = n + off + 1                                        # one guard element behind the n outputs
        bbuf, pbuf = torch.zeros(total, dtype=torch.float32, device=DEV), torch.zeros(total, dtype=torch.int32, device=DEV)
        obuf = _t(np.full(total, NAN_FILL, np.uint32).view(np.float32))
        bd, pd, od = bbuf[off:off + n], pbuf[off:off + n], obuf[off:off + n]
        bd.copy_(_t(base))
        pd.copy_(_t(pair.view(np.int32)))
        assert ops.edge_revalue(bd, pd, key, keep, out=od) is od
        got, want = _bits(obuf), ref.revalue(base, pair, key, keep).view(np.uint32)
        assert np.array_equal(got[off:off + n], want), (n, keep, off, int((got[off:off + n] != want).sum()))
        assert np.all(got[:off] == NAN_FILL) and got[off + n] == NAN_FILL                     # nothing outside [0, n)
        assert not np.any((got[off:off + n] == ref.PAD_BITS) & (base.view(np.uint32) != ref.PAD_BITS))
        assert np.array_equal(_bits(bbuf)[off:off + n], base.view(np.uint32))                 # base untouched
        if n and keep < 1.0:
            dropped = ~ref.kept(pair, key, keep)
            assert np.all(got[off:off + n][dropped] == 0)
            assert n < 1000 or 0 < dropped.sum() < n
    if n:
        with pytest.raises(Exception, match="must not alias"):
            ops.edge_revalue(bd, pd, key, 0.5, out=bd)
        with pytest.raises(Exception, match="keep must lie"):
            ops.edge_revalue(bd, pd, key, 0.0, out=od)


def test_revalue_kernel_past_the_first_grid_stride():
    """The launch is capped at 4,096 workgroups of 256 threads: above 4 x 1,048,576 aligned entries (every re-draw of a full-size
    training adjacency) a thread takes a second float4, and above 1,048,576 entries one element off a second scalar.  One
    size past both, with a tail, against the restatement bit for bit."""
    from stochastic_gcn_amd import ops
    n, keep, key = 4 * 1048576 + 70001, 0.8, ref.edge_key(3, 2)
    rng = np.random.RandomState(11)
    base = rng.standard_normal(n).astype(np.float32)
    pair = rng.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    pair[pair == ref.ALWAYS] = ref.ALWAYS - 1
    always = np.nonzero(rng.rand(n) < 0.1)[0]
    pair[always] = ref.ALWAYS
    base.view(np.uint32)[always[0::2]] = ref.PAD_BITS
    want = ref.revalue(base, pair, key, keep).view(np.uint32)
    for off in (0, 1):
        bbuf, pbuf = torch.zeros(n + off + 1, dtype=torch.float32, device=DEV), torch.zeros(n + off + 1, dtype=torch.int32, device=DEV)
        obuf = _t(np.full(n + off + 1, NAN_FILL, np.uint32).view(np.float32))
        bbuf[off:off + n].copy_(_t(base))
        pbuf[off:off + n].copy_(_t(pair.view(np.int32)))
        ops.edge_revalue(bbuf[off:off + n], pbuf[off:off + n], key, keep, out=obuf[off:off + n])
        got = _bits(obuf)
        assert np.array_equal(got[off:off + n], want), (off, int((got[off:off + n] != want).sum()))
        assert np.all(got[:off] == NAN_FILL) and got[off + n] == NAN_FILL


# ---- products ----------------------------------------------------------------------------------------------------------
PATTERNS = ("empty", "identity", "star_row", "star_col", "row_lengths", "rmat", "hub")
KERNELS = ("rows", "cs1", "cs2", "cs4")
KEY = ref.edge_key(1, 5)
_PATTERNS = {}


def hub_pattern():
    """A symmetric pattern on 300 vertices with self loops and a hub of degree 200 (T = 64 splits its row and, in the
    transpose, its column's row)."""
    rng = np.random.RandomState(4)
    i, j = rng.randint(0, 300, 900), rng.randint(0, 300, 900)
    h = rng.choice(np.arange(1, 300), 200, replace=False)
    rows = np.concatenate([i, j, np.zeros(200, np.int64), h, np.arange(300)])
    cols = np.concatenate([j, i, h, np.zeros(200, np.int64), np.arange(300)])
    return sc._csr(300, 300, rows, cols)


def pattern(name):
    if name not in _PATTERNS:
        _PATTERNS[name] = hub_pattern() if name == "hub" else ref.squared(sc.pattern(name))
    return _PATTERNS[name]


def _plan(a, kernel):
    from stochastic_gcn_amd import ops
    if kernel == "rows":
        return ops.DeviceCSR.from_scipy(a, DEV, plan_T=sc.T_SPLIT)
    return ops.ColumnSweepCSR(a, DEV, G=int(kernel[2:]), T=sc.T_SPLIT)


def _redrawn(plan, key, keep):
    """The plan's value array re-drawn on the device, with the pair keys of the host decode."""
    from stochastic_gcn_amd import ops
    pair = ops.edge_pair_keys(*ops.plan_entries(plan))
    return ops.edge_revalue(plan.val, _t(pair.view(np.int32)), key, keep)


def _multiply(plan, x, values=None):
    """plan . x on the plan's kernel, reading ``values`` instead of the plan's own where given."""
    from stochastic_gcn_amd import ops
    if isinstance(plan, ops.DeviceCSR):
        if values is not None:
            plan = ops.DeviceCSR(plan.shape, plan.rowptr, plan.col, values, plan.plan, host_rowptr=plan.host_rowptr)
        return ops.spmm(plan, x)
    plan.live_val = values
    try:
        return ops.spmm_cs(plan, x)
    finally:
        plan.live_val = None


def _operands(rng, n, d, ints=False):
    """(fp32 operand, the same rounded into a bfloat16 table)"""
    from stochastic_gcn_amd import ops
    x = _t(sc.ints(rng, (n, d)) if ints else rng.standard_normal((n, d)).astype(np.float32))
    return x, ops.operand_round(x, out=ops.history_alloc(n, d, DEV, bf16=True))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", PATTERNS)
def test_products_on_redrawn_values_equal_the_plan_of_the_host_masked_matrix(name, kernel):
    from stochastic_gcn_amd import ops
    keep = 0.8
    a = sc.normalised(pattern(name))
    rng = np.random.RandomState(7)
    for side, m in (("A", a), ("A^T", ops.transpose_host(a))):
        masked = ref.masked_matrix(m, KEY, keep)
        assert masked.nnz == m.nnz and (m.nnz == 0 or name == "identity" or 0 < np.count_nonzero(masked.data) < m.nnz)
        plan, want_plan = _plan(m, kernel), _plan(masked, kernel)
        base_bits = _bits(plan.val).copy()
        vals = _redrawn(plan, KEY, keep)
        # the re-drawn array IS the value array of the same plan type built from the host-masked matrix
        assert np.array_equal(_bits(vals), _bits(want_plan.val)), (name, kernel, side)
        for d in (4, 128, 132):
            for x in _operands(rng, m.shape[1], d):
                got, want = _multiply(plan, x, vals), _multiply(want_plan, x)
                assert _same_bits(got, want), (name, kernel, side, d, x.dtype)
        assert np.array_equal(_bits(plan.val), base_bits)            # the base values were read, never written


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", PATTERNS)
def test_dyadic_products_on_redrawn_values_are_exact(name, kernel):
    """Values +-2^k and keep = 0.5 (a factor of 2): small-integer operands make every sum exact whatever its order, so the
    product on re-drawn values equals the fp64 product of the host-masked matrix bit for bit (sparse_cases.spmm_exact
    asserts the precondition)."""
    from stochastic_gcn_amd import ops
    a = sc.dyadic(pattern(name), np.random.RandomState(3))
    rng = np.random.RandomState(8)
    for side, m in (("A", a), ("A^T", ops.transpose_host(a))):
        masked = ref.masked_matrix(m, KEY, 0.5)
        plan = _plan(m, kernel)
        vals = _redrawn(plan, KEY, 0.5)
        for d in (4, 128, 132):
            x, xb = _operands(rng, m.shape[1], d, ints=True)
            want = sc.spmm_exact(masked, x.cpu().numpy())            # (small integers: the bfloat16 table holds them exactly)
            for op in (x, xb):
                got = _multiply(plan, op, vals).cpu().numpy().astype(np.float64)
                gpu_checks.compare(got, want, what="%s %s %s d=%d %s" % (name, kernel, side, d, op.dtype))


# ---- the static matrix -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("kernel", ["rows", "cs"])
def test_static_matrix_redraws_inside_a_step_and_reads_the_base_values_outside(kernel, bf16):
    """begin_step .. end_step on the hub graph: the products of the matrix and of its lazily built transpose, on the matrix's
    kernel (width 128) and on the row kernel it falls back to (width 22), equal those of an unmasked StaticMatrix of the
    host-masked adjacency; each array is drawn once per step; outside a step the products are those of the adjacency."""
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd.full_batch import StaticMatrix
    p, a = 0.2, sc.normalised(hub_pattern())
    keep = 1.0 - p
    n = a.shape[0]
    rng = np.random.RandomState(9)
    xs = {d: _t(rng.standard_normal((n, d)).astype(np.float32)) for d in (128, 22)}
    adds = {d: _t(rng.standard_normal((n, d)).astype(np.float32)) for d in (128, 22)}
    mat = StaticMatrix(a, DEV, kernel, 3, 128, bf16=bf16, edge_dropout=p)
    plain = StaticMatrix(a, DEV, kernel, 3, 128, bf16=bf16)
    assert mat.kernel == plain.kernel == kernel and plain.edge is None and plain._redrawn == {}
    before = {d: plain.product(xs[d]).clone() for d in xs}
    calls, real = [], ops.edge_revalue
    ops.edge_revalue = lambda *a_, **k: calls.append(1) or real(*a_, **k)
    try:
        assert all(_same_bits(mat.product(xs[d]), before[d]) for d in xs) and calls == []      # no step: the adjacency
        for step in (0, 1):
            key = ref.edge_key(1, step)
            want = StaticMatrix(ref.masked_matrix(a, key, keep), DEV, kernel, 3, 128, bf16=bf16)
            del calls[:]
            mat.begin_step(key)
            assert calls == [1]                                   # the forward's array, ahead of the forward
            for _ in range(2):
                for d in xs:
                    assert _same_bits(mat.product(xs[d]), want.product(xs[d])), (kernel, bf16, step, d)
                    assert _same_bits(mat.transpose.product(xs[d], add=adds[d], add_rows=n),
                                      want.transpose.product(xs[d], add=adds[d], add_rows=n)), (kernel, bf16, step, d, 'T')
            # one draw per value array a product read: the plan's and (cs) the row kernel's CSR, for A and for A^T
            assert len(calls) == (2 if kernel == 'rows' else 4), calls
            mat.end_step()
            assert all(_same_bits(mat.product(xs[d]), before[d]) for d in xs)
            assert _same_bits(mat.transpose.product(xs[128]), plain.transpose.product(xs[128]))
    finally:
        ops.edge_revalue = real
    for m, q in ((mat, plain), (mat.transpose, plain.transpose)):
        assert _same_bits(m.rows_csr.val, q.rows_csr.val)
        if kernel == 'cs':
            assert _same_bits(m._plan.val, q._plan.val) and m._plan.live_val is None


# ---- the model -----------------------------------------------------------------------------------------------------------
P_EDGE = 0.2
# The seeds of the weights, chosen WITH THE ORACLE ALONE as full_batch_cases.CASES' are (a ReLU input within fp32 rounding of
# zero has no determined gate): of the seeds 3 .. 12, the one whose smallest non-zero |ReLU input| over the three oracle
# steps on the host-masked adjacencies is largest (``masked_gate_margin`` below).
MODEL_SEEDS = {'reddit3k_pp': 5, 'multilabel': 8}          # margins 4.1e-6 and 2.4e-5 (seed 1 of the masks)


def _masked_adj(adj, seed, step):
    return ref.masked_matrix(adj, ref.edge_key(seed, step), 1.0 - P_EDGE)


def masked_gate_margin(name, init, seed=1):
    """full_batch_cases.gate_margin with every step's adjacency under the step's edge mask.  CPU only."""
    case = fc.build(name)
    fl = case['flags']
    om = fc.oracle_model(case, case['nbr_train'], seed=init)
    rows, seen = np.sort(case['train']), []

    def scan(layer, pre):
        a = np.abs(pre)
        seen.append(float(a[a > 0].min()))
        return pre > 0
    om.relu_gate_hook = scan
    for step in range(3):
        feed = fc.exact_feed(case, _masked_adj(case['train_adj'], seed, step), fl['dropout'])
        logits, _ = om.forward(feed, case['ph'], fl['dropout'], mnp.HashMasks(seed, step, 1.0 - fl['dropout']))
        dout = np.zeros_like(logits)
        dout[rows] = om.loss_and_grad(logits[rows], case['labels'][rows])[3]
        om.adam_step(om.backward(dout))
    return min(seen)


def _np(x):
    if hasattr(x, 'csr'):
        return None
    if hasattr(x, 'materialize'):
        x = x.materialize()
    return x.detach().cpu().numpy()


def _device(case, params, kernel, extra=None, bf16=False):
    from stochastic_gcn_amd.full_batch import StaticBatch, model_matrix
    dm = fc.device_model(case, case['nbr_train'], case['train_adj'], {k: v.copy() for k, v in params.items()}, extra_flags=extra)
    mat = model_matrix(case['train_adj'], DEV, dm, 3, kernel=kernel, bf16=bf16, edge_dropout=P_EDGE)
    assert mat.kernel == kernel and mat.edge is not None
    sb = StaticBatch(mat, case['labels'], np.sort(case['train']), dm.L, DEV)
    sb.dropout = case['flags']['dropout']
    return dm, sb


@pytest.mark.parametrize("kernel", ["rows", "cs"])
@pytest.mark.parametrize("name", sorted(MODEL_SEEDS))
def test_training_steps_match_the_oracle_on_the_host_masked_adjacency(name, kernel):
    case = fc.build(name)
    fl, adj, rows = case['flags'], case['train_adj'], np.sort(case['train'])
    om = fc.oracle_model(case, case['nbr_train'], seed=MODEL_SEEDS[name])
    start = {k: v.copy() for k, v in om.params.items()}
    dm, sb = _device(case, start, kernel)
    worst = dict(act=0.0, grad=0.0, param=0.0, loss=0.0)
    for step in range(3):
        assert dm.dropout_step == step
        masks = mnp.HashMasks(dm.dropout_seed, dm.dropout_step, 1.0 - fl['dropout'])
        masked = _masked_adj(adj, dm.dropout_seed, dm.dropout_step)
        assert 0.7 * adj.nnz < np.count_nonzero(masked.data) < 0.9 * adj.nnz
        outs = dm.run_one_step(None, sb)
        d_acts, dg, dp = [_np(a) for a in dm.activations[1:]], dm.get_grads(), dm.get_params()
        feed = fc.exact_feed(case, masked, fl['dropout'])
        logits, o_acts = om.forward(feed, case['ph'], fl['dropout'], masks)
        o_loss, o_acc, _, dl = om.loss_and_grad(logits[rows], case['labels'][rows])
        dout = np.zeros_like(logits)
        dout[rows] = dl
        o_grads = om.backward(dout)
        om.adam_step(o_grads)
        assert len(d_acts) == len(o_acts)
        for li, (da, oa) in enumerate(zip(d_acts, o_acts)):
            if da is None or hasattr(oa, 'tocsr'):
                continue
            e = onp.rel_err(da, oa)
            worst['act'] = max(worst['act'], e)
            print("%s/%s step %d layer %d rel_err %.3e" % (name, kernel, step, li, e))
            assert da.shape == oa.shape and e <= TOL, (name, kernel, step, li, e)
        e = abs(outs[1] - float(o_loss)) / max(abs(float(o_loss)), 1e-30)
        worst['loss'] = max(worst['loss'], e)
        print("%s/%s step %d loss %.7f (oracle %.7f) acc %.6f (%.6f)" % (name, kernel, step, outs[1], float(o_loss), outs[2], float(o_acc)))
        assert e <= TOL and abs(outs[2] - float(o_acc)) <= 1e-6
        for k, g in o_grads.items():
            e = onp.rel_err(dg[k], g)
            worst['grad'] = max(worst['grad'], e)
            print("%s/%s step %d grad %s rel_err %.3e" % (name, kernel, step, k, e))
            assert e <= TOL, (name, kernel, step, 'grad', k, e)
        for k, v in om.params.items():
            e = onp.rel_err(dp[k], v)
            worst['param'] = max(worst['param'], e)
            print("%s/%s step %d param %s rel_err %.3e" % (name, kernel, step, k, e))
            assert e <= TOL, (name, kernel, step, 'param', k, e)
    print("%s/%s: worst rel err  activations %.1e  loss %.1e  grads %.1e  params %.1e"
          % (name, kernel, worst['act'], worst['loss'], worst['grad'], worst['param']))
    # the same run again: the same bits
    dm2, sb2 = _device(case, start, kernel)
    for _ in range(3):
        dm2.run_one_step(None, sb2)
    assert _same_bits(dm2.theta, dm.theta)
    # the epoch counters count nnz and N per layer, as without the mask
    dm.init_counts()
    dm.run_one_step(None, sb)
    assert list(dm.adj_sizes) == [adj.nnz] * dm.L and list(dm.field_sizes) == [case['n']] * (dm.L + 1)


@pytest.mark.parametrize("kernel", ["rows", "cs"])
def test_bf16_step_runs_on_the_redrawn_values(kernel):
    """--full_batch_dtype bf16 --dense_dtype bf16: the step runs, its products gather a bfloat16 operand, and the value
    array every one of them read is the step's re-drawn array (the values stay fp32)."""
    from stochastic_gcn_amd import ops
    case = fc.build('reddit3k_pp')
    om = fc.oracle_model(case, case['nbr_train'], seed=MODEL_SEEDS['reddit3k_pp'])
    dm, sb = _device(case, om.params, kernel, extra=dict(full_batch_dtype='bf16', dense_dtype='bf16'), bf16=True)
    dm.run_one_step(None, sb)                           # (tunes the sweep's clock: those products are not the step's)
    key = ref.edge_key(dm.dropout_seed, dm.dropout_step)
    seen, real_rows, real_cs = [], ops.spmm, ops.spmm_cs
    try:
        ops.spmm = lambda A, B, **kw: seen.append((A, A.val.clone(), B.dtype)) or real_rows(A, B, **kw)
        ops.spmm_cs = lambda A, B, **kw: seen.append((A, None if A.live_val is None else A.live_val.clone(), B.dtype)) \
            or real_cs(A, B, **kw)
        outs = dm.run_one_step(None, sb)
    finally:
        ops.spmm, ops.spmm_cs = real_rows, real_cs
    assert np.isfinite(outs[1]) and len(seen) == 2                 # one aggregation: forward by A, backward by A^T
    mat = sb.matrix
    for (A, vals, dtype), m in zip(seen, (mat, mat.transpose)):
        base = m.rows_csr if isinstance(A, ops.DeviceCSR) else m._plan
        assert isinstance(A, ops.DeviceCSR) == (kernel == 'rows')
        assert dtype == torch.bfloat16 and vals is not None and vals.dtype == torch.float32
        pair = ref.pair_keys(*ops.plan_entries(base))
        want = ref.revalue(base.val.cpu().numpy(), pair, key, 1.0 - P_EDGE)
        assert np.array_equal(_bits(vals), want.view(np.uint32))
        assert not np.array_equal(_bits(vals), _bits(base.val))


# ---- isolation -----------------------------------------------------------------------------------------------------------
def test_train_main_leaves_the_adjacency_as_uploaded_and_evaluates_unmasked(tmp_path, monkeypatch):
    from stochastic_gcn_amd import ops, train
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.full_batch import StaticBatch, StaticMatrix
    monkeypatch.chdir(tmp_path)
    made, draws = [], []
    real = train.Trainer

    class Keep(real):
        def __init__(self, *a, **k):
            made.append(self)
            super(Keep, self).__init__(*a, **k)
    monkeypatch.setattr(train, "Trainer", Keep)
    real_draw = ops.edge_revalue
    monkeypatch.setattr(ops, "edge_revalue", lambda *a, **k: draws.append(k['out'].data_ptr()) or real_draw(*a, **k))
    FLAGS.reset()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train.main(['--dataset', 's-cora', '--full_batch', '--test_full_batch', '--full_batch_kernel', 'cs',
                    '--edge_dropout', '0.2', '--epochs', '0'])
    out = buf.getvalue()
    tr = made[0]
    assert len([l for l in out.splitlines() if l.startswith("Epoch:")]) == 2            # epochs + 2
    assert "[sgcn] --edge_dropout 0.2" in out and "keep 0.8" in out
    mat, ev = tr.train_static.matrix, tr.eval_static.matrix
    assert mat.edge is not None and mat.edge.key is None and ev.edge is None and ev._redrawn == {}
    assert len(draws) == 2 * len(set(draws)) >= 4                   # per epoch: the forward's array and the transpose's
    # every base value array is bit-identical to its upload
    fresh = StaticMatrix(mat.a, DEV, 'cs', mat.products, mat.d_hint)
    for m, q in ((mat, fresh), (mat.transpose, fresh.transpose)):
        assert m._plan.G == q._plan.G and _same_bits(m._plan.val, q._plan.val) and m._plan.live_val is None
        assert _same_bits(m.rows_csr.val, _t(m.a.data.astype(np.float32)))
    # ... anything that multiplies by the matrix outside a step sees A
    x = _t(np.random.RandomState(0).standard_normal((mat.shape[1], 32)).astype(np.float32))
    assert _same_bits(mat.product(x), fresh.product(x)) and _same_bits(mat.transpose.product(x), fresh.transpose.product(x))
    # the evaluation logits are those of an unmasked forward with the final weights
    n_draws = len(draws)
    tr.evaluate(tr.val_d)
    logits = tr.test_model.outputs.clone()
    plain = StaticBatch(StaticMatrix(ev.a, DEV, 'cs', 3, ev.d_hint), tr._labels_dev, np.sort(tr.val_d), tr.test_model.L, DEV)
    tr.test_model.run_one_step(None, plain)
    assert _same_bits(tr.test_model.outputs, logits) and len(draws) == n_draws


def _trainer(case, **flags):
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.train import Trainer
    FLAGS.reset()
    FLAGS.update(dataset='s-reddit', seed=1, prefetch=0, test_preprocess=case['flags']['preprocess'],
                 **{k: v for k, v in case['flags'].items() if hasattr(FLAGS, k)})
    FLAGS.update(**flags)
    with contextlib.redirect_stdout(io.StringIO()):
        return Trainer(data=case['data'], verbose=False)


def test_flag_at_zero_is_the_default_run(monkeypatch):
    from stochastic_gcn_amd import ops
    case = fc.build('reddit3k_pp')
    draws = []
    real_draw = ops.edge_revalue
    monkeypatch.setattr(ops, "edge_revalue", lambda *a, **k: draws.append(1) or real_draw(*a, **k))
    thetas = []
    for flags in (dict(), dict(edge_dropout=0.0)):
        tr = _trainer(case, full_batch=True, full_batch_kernel='cs', **flags)
        mat = tr.train_static.matrix
        assert tr.edge_dropout == 0.0 and mat.edge is None and mat._redrawn == {}      # nothing allocated
        for _ in range(2):
            tr.train_epoch()
        assert mat._redrawn == {} and mat.transpose._redrawn == {}
        thetas.append(tr.train_model.theta.clone())
    assert draws == [] and _same_bits(thetas[0], thetas[1])
    # ... and the flag set changes the epoch's weights
    tr = _trainer(case, full_batch=True, full_batch_kernel='cs', edge_dropout=0.2)
    for _ in range(2):
        tr.train_epoch()
    assert len(draws) == 4 and not _same_bits(tr.train_model.theta, thetas[0])
