"""GPU tests of --full_batch_parts above the kernels: every product and backward of an InducedMatrix against the same method of
a StaticMatrix over SciPy's A[S][:, S] on the row kernel, bit for bit; three Cluster-GCN training steps whose union is the
whole graph against three steps of --full_batch --full_batch_kernel rows, bit for bit; and train.main end to end."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

import attn_aggregator_cases as ax
import induce_ref as ir
import sparse_cases as sc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _reset_flags():
    from stochastic_gcn_amd.flags import FLAGS
    FLAGS.reset()
    yield
    FLAGS.reset()


def _same(a, b):
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- matrix level -------------------------------------------------------------------------------------------------------
_PAIR = {}


def _pair(sname):
    """(InducedMatrix over S, StaticMatrix of SciPy's A[S][:, S] on the row kernel, n) on a 200-vertex row-normalised graph;
    built once per subset and shared (nothing below writes to either)."""
    if sname not in _PAIR:
        from stochastic_gcn_amd import ops
        from stochastic_gcn_amd.full_batch import InducedMatrix, StaticMatrix
        a = sc.normalised(ir.flat_graph(200, 5, seed=9))
        a.sort_indices()
        rng = np.random.RandomState(5)
        ids = {'every_other': np.arange(0, 200, 2, dtype=np.int32),
               'third': np.sort(rng.choice(200, 67, replace=False)).astype(np.int32)}[sname]
        # one resident matrix per subset: a block lives in its matrix's buffers until the next csr_induce on that matrix
        A = ops.DeviceCSR.from_scipy(a, DEV, with_plan=False, with_transpose=True)       # (as the trainer keeps it)
        ind = InducedMatrix(ops.csr_induce(A, ids, norm='keep'), DEV)
        sub = a[ids][:, ids].tocsr()
        sub.sort_indices()
        _PAIR[sname] = (ind, StaticMatrix(sub, DEV, 'rows'), len(ids), A)
    return _PAIR[sname][:3]


def _operands(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn((n, d), generator=g).to(DEV) for _ in range(3))


@pytest.mark.parametrize("sname", ['every_other', 'third'])
@pytest.mark.parametrize("d", [8, 20])
def test_sum_products_are_the_static_matrix_bits(sname, d):
    ind, ref, n = _pair(sname)
    assert ind.kernel == ref.kernel == 'rows' and ind.shape == ref.shape == (n, n) and ind.nnz == ref.nnz
    assert ind.transpose.transpose is ind and ind.edge is None and ind.bf16 is False
    x, g, add = _operands(n, d, 1)
    assert _same(ind.product(x), ref.product(x))
    assert _same(ind.multiply(x), ref.multiply(x))
    assert _same(ind.transpose.product(g), ref.transpose.product(g))
    assert _same(ind.transpose.product(g, add=add, add_rows=n), ref.transpose.product(g, add=add, add_rows=n))
    oi, orf = (torch.zeros((n, 2 * d), device=DEV) for _ in range(2))
    ind.product(x, out=oi[:, d:])
    ref.product(x, out=orf[:, d:])
    assert _same(oi, orf) and float(oi[:, d:].abs().sum()) > 0


@pytest.mark.parametrize("sname", ['every_other', 'third'])
@pytest.mark.parametrize("d", [8, 20])
def test_max_products_are_the_static_matrix_bits(sname, d):
    ind, ref, n = _pair(sname)
    x, g, add = _operands(n, d, 2)
    (oi, ai), (orf, ar) = ind.max_product(x), ref.max_product(x)
    assert _same(oi, orf) and _same(ai, ar)
    assert _same(ind.transpose.max_backward(g, ai), ref.transpose.max_backward(g, ar))
    assert _same(ind.transpose.max_backward(g, ai, add=add, add_rows=n), ref.transpose.max_backward(g, ar, add=add, add_rows=n))


@pytest.mark.parametrize("sname", ['every_other', 'third'])
@pytest.mark.parametrize("d", [8, 20])
@pytest.mark.parametrize("keep", [1.0, 0.75])
def test_attn_products_are_the_static_matrix_bits(sname, d, keep):
    ind, ref, n = _pair(sname)
    x, g, add = _operands(n, d, 3)
    kw = dict(heads=2, keep=keep, key=0x1234567)
    scale = float(d // 2) ** -0.5
    (oi, li), (orf, lr) = ind.attn_product(x, scale, **kw), ref.attn_product(x, scale, **kw)
    assert _same(oi, orf) and _same(li, lr) and tuple(li.shape) == (n, 2)
    assert _same(ind.attn_backward(x, g, oi, li, scale, **kw), ref.attn_backward(x, g, orf, lr, scale, **kw))
    assert _same(ind.attn_backward(x, g, oi, li, scale, add=add, add_rows=n, **kw),
                 ref.attn_backward(x, g, orf, lr, scale, add=add, add_rows=n, **kw))


@pytest.mark.parametrize("sname", ['every_other', 'third'])
@pytest.mark.parametrize("d", [8, 20])
def test_gat_products_are_the_static_matrix_bits(sname, d):
    ind, ref, n = _pair(sname)
    x, g, add = _operands(n, d, 4)
    a = torch.randn((2, d), generator=torch.Generator().manual_seed(8)).to(DEV)
    kw = dict(heads=2, keep=0.75, key=77)
    (oi, li, si), (orf, lr, sr) = ind.gat_product(x, a, 0.2, **kw), ref.gat_product(x, a, 0.2, **kw)
    assert _same(oi, orf) and _same(li, lr) and _same(si, sr)
    (dxi, dai), (dxr, dar) = (m.gat_backward(x, a, s, g, o, l, 0.2, add=add, add_rows=n, **kw)
                              for m, s, o, l in ((ind, si, oi, li), (ref, sr, orf, lr)))
    assert _same(dxi, dxr) and _same(dai, dar)
    (_, dai), (_, dar) = (m.gat_backward(x, a, s, g, o, l, 0.2, need_dx=False, **kw)
                          for m, s, o, l in ((ind, si, oi, li), (ref, sr, orf, lr)))
    assert _same(dai, dar)


# ---- step level ---------------------------------------------------------------------------------------------------------
def _trainer(case, **flags):
    from stochastic_gcn_amd import train
    from stochastic_gcn_amd.flags import FLAGS
    FLAGS.reset()
    FLAGS.update(**{k: v for k, v in case['flags'].items() if hasattr(FLAGS, k)})
    FLAGS.update(full_batch=True, test_full_batch=True, **flags)
    data = (case['n'], case['train_adj'], case['full_adj'], case['feats'], case['nbr_train'], case['nbr_test'], case['labels'],
            case['train'], case['val'], case['test'])
    return train.Trainer(data=data, verbose=False)


@pytest.mark.parametrize("agg", ['sum', 'max', 'attn'])
def test_three_steps_over_the_whole_union_are_full_batch_steps(agg):
    """P = 3, q = 3, --full_batch_part_norm rows: the union is every vertex, the block the adjacency itself (full_i / kept_i
    is exactly 1), the gathered rows the tables themselves -- loss and every weight as after --full_batch --full_batch_kernel
    rows, bit for bit"""
    case = ax.build('gcn_nopp')
    extra = dict(aggregator=agg, **(dict(attn_heads=2) if agg == 'attn' else {}))
    ta = _trainer(case, full_batch_kernel='rows', **extra)
    start = {k: v.copy() for k, v in ta.train_model.get_params().items()}
    losses_a = []
    for _ in range(3):
        ta.train_epoch()
        losses_a.append(np.float32(ta.avg_loss.mean()))
    assert ta.last_epoch['steps'] == 1 and ta.train_static.matrix.kernel == 'rows'
    after_a = ta.train_model.get_params()
    tb = _trainer(case, full_batch_parts=3, full_batch_parts_per_step=3, full_batch_part_norm='rows', **extra)
    assert not hasattr(tb, 'train_static') and len(tb.part_ids) == 3 and len(tb.part_schedule) == 1
    tb.train_model.set_params({k: v.copy() for k, v in start.items()})
    losses_b = []
    for _ in range(3):
        tb.train_epoch()
        losses_b.append(np.float32(tb.avg_loss.mean()))
        assert tb.last_epoch['steps'] == 1 and tb.last_epoch['skipped'] == 0
    after_b = tb.train_model.get_params()
    print("%s: losses %s (full batch) %s (one union of three parts)" % (agg, losses_a, losses_b))
    assert all(np.isfinite(l) for l in losses_a)
    assert [l.tobytes() for l in losses_a] == [l.tobytes() for l in losses_b]
    assert set(after_a) == set(after_b) and all(after_a[k].tobytes() == after_b[k].tobytes() for k in after_a)
    assert any(after_a[k].tobytes() != start[k].tobytes() for k in after_a)
    assert tb.train_model.adam_t == 3


def test_part_batch_carries_ids_labels_and_loss_positions():
    case = ax.build('sage_ln_pp')
    tr = _trainer(case, full_batch_parts=3, full_batch_parts_per_step=2)
    ids = tr.part_schedule.epoch(0)[0]
    pb = tr.part_batch(ids)
    n = len(ids)
    assert pb.N == n and pb.matrix.shape == (n, n) and np.array_equal(pb.ids, ids) and np.array_equal(pb.ids_dev.cpu().numpy(), ids)
    assert np.array_equal(pb.labels.cpu().numpy(), np.asarray(case['labels'], np.float32)[ids])
    want = np.flatnonzero(np.isin(ids, case['train']))
    assert np.array_equal(pb.host_rows, want) and np.array_equal(pb.rows.cpu().numpy(), want) and want.size > 0
    a = case['train_adj'].tocsr().copy()
    a.sort_indices()
    blk = ir.block(a, ids)
    assert np.array_equal(pb.matrix.rows_csr.rowptr.cpu().numpy(), blk[0]) and np.array_equal(pb.matrix.rows_csr.col.cpu().numpy(), blk[1])
    # a vertex set without a training vertex gives no batch
    rest = np.setdiff1d(np.arange(case['n']), case['train']).astype(np.int32)
    assert tr.part_batch(rest[:10]) is None


# ---- end to end ---------------------------------------------------------------------------------------------------------
def _run_main(monkeypatch, argv):
    from stochastic_gcn_amd import train
    made = []
    real = train.Trainer

    class Keep(real):
        def __init__(self, *a, **k):
            made.append(self)
            super(Keep, self).__init__(*a, **k)
    monkeypatch.setattr(train, "Trainer", Keep)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train.main(argv)
    monkeypatch.setattr(train, "Trainer", real)
    return made[0], buf.getvalue()


@pytest.mark.parametrize("extra", [[], ['--aggregator', 'attn', '--attn_heads', '2']], ids=['sum', 'attn2'])
def test_train_main_end_to_end(tmp_path, monkeypatch, extra):
    """s-cora, 3 epochs (the loop runs epochs + 2 = 5), P = 4, q = 2: two groups per epoch.  A group takes a step when it holds
    a training vertex and is skipped and counted otherwise, and s-cora's 140 training vertices are its first 140 ids: under
    the partition of seed 1 they fall 138 / 0 / 0 / 2 into the four parts, so whenever the schedule pairs the two parts
    without one (epochs 1, 3 and 4 of the five) that group is skipped.  `Two steps in each epoch` therefore cannot hold on
    this dataset; the test pins every epoch's step count to the number of its groups that hold a training vertex, worked
    out here on the host from the parts and the schedule, and needs both kinds of epoch to occur."""
    monkeypatch.chdir(tmp_path)
    argv = ['--dataset', 's-cora', '--full_batch', '--test_full_batch', '--epochs', '3', '--full_batch_parts', '4',
            '--full_batch_parts_per_step', '2'] + extra
    tr, out = _run_main(monkeypatch, argv)
    setup = [l for l in out.splitlines() if l.startswith("[sgcn] --full_batch_parts 4:")]
    assert len(setup) == 1 and "part sizes min / median / max" in setup[0] and "of the nonzeros lie inside parts" in setup[0]
    print(setup[0])
    ep = [l for l in out.splitlines() if l.startswith("Epoch:")]
    walls = [l for l in out.splitlines() if l.startswith("[sgcn] epoch train wall")]
    assert len(ep) == len(walls) == 5               # the reference's exit is `epoch > FLAGS.epochs`: epochs + 2
    mask = np.zeros(tr.num_data, dtype=bool)
    mask[tr.train_d] = True
    per_part = [int(mask[p].sum()) for p in tr.part_ids]
    want = [sum(int(mask[u].any()) for u in tr.part_schedule.epoch(e)) for e in range(5)]
    got = [int(re.search(r" over (\d+) steps ", l).group(1)) for l in walls]
    print("training vertices per part %s; steps per epoch %s (groups with a training vertex: %s)" % (per_part, got, want))
    assert all(len(tr.part_schedule.epoch(e)) == 2 for e in range(5))
    assert got == want and 2 in got and set(got) <= {1, 2}
    assert tr.last_epoch['steps'] == want[-1] and tr.last_epoch['steps'] + tr.last_epoch['skipped'] == 2
    assert tr.train_model.adam_t == sum(want)
    for line in ep:
        tok = line.split()
        assert np.isfinite(float(tok[3])) and np.isfinite(float(tok[7]))
    print("train loss per epoch:", [float(l.split()[3]) for l in ep])
    m = re.search(r"Test set results: cost= (\d+\.\d{5})", out)
    assert m and np.isfinite(float(m.group(1)))
    first = tr.train_model.get_params()
    tr2, out2 = _run_main(monkeypatch, argv)
    second = tr2.train_model.get_params()
    assert set(first) == set(second) and all(first[k].tobytes() == second[k].tobytes() for k in first)
    assert [l.split()[3] for l in out2.splitlines() if l.startswith("Epoch:")] == [l.split()[3] for l in ep]
