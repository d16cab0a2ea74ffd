"""CPU tests of --full_batch_parts (Cluster-GCN steps on device-cut subgraphs): flags and refusals, the partitioner, the
schedule of the groupings, the plain-loop reference of the induced block (tests/induce_ref.py) against SciPy, and the argument
checks of the three exports through the raw C-ABI.  Nothing here touches a device."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import induce_ref as ir
import sparse_cases as sc
from stochastic_gcn_amd import _ffi
from stochastic_gcn_amd.flags import _DEFS, FLAGS, _Flags

NEW = ("sgcn_induce_map_i32", "sgcn_csr_induce_count", "sgcn_csr_induce_fill")
ON = dict(full_batch=True, full_batch_parts=4)


@pytest.fixture(autouse=True)
def _reset_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


# ---- flags ------------------------------------------------------------------------------------------------------------
def test_flag_defaults_and_parsing():
    from stochastic_gcn_amd.flags import _CHOICES
    from stochastic_gcn_amd.full_batch import check_full_batch_parts
    f = _Flags()
    assert (f.full_batch_parts, f.full_batch_parts_per_step, f.full_batch_part_norm) == (0, 1, 'rows')
    assert {'full_batch_parts', 'full_batch_parts_per_step', 'full_batch_part_norm'} <= set(f.as_dict())
    for name, typ, default in (('full_batch_parts', int, 0), ('full_batch_parts_per_step', int, 1),
                               ('full_batch_part_norm', str, 'rows')):
        assert (name, typ, default) == next(d[:3] for d in _DEFS if d[0] == name)
    assert _CHOICES['full_batch_part_norm'] == ('rows', 'keep')
    assert check_full_batch_parts(f) == (0, 1, 'rows')                       # off: nothing else is looked at
    f.parse(['--full_batch', '--full_batch_parts', '32', '--full_batch_parts_per_step=4', '--full_batch_part_norm', 'keep'])
    assert check_full_batch_parts(f) == (32, 4, 'keep')
    with pytest.raises(SystemExit):
        f.parse(['--full_batch_part_norm', 'cols'])
    # the kernels a part batch can run on, and what it does not interfere with
    for kernel in ('auto', 'rows'):
        FLAGS.reset()
        FLAGS.update(full_batch_kernel=kernel, test_full_batch=True, aggregator='attn', attn_heads=2, full_batch_dtype='fp32', **ON)
        assert check_full_batch_parts() == (4, 1, 'rows')
    FLAGS.reset()
    FLAGS.update(full_batch_dtype='bf16', dense_dtype='bf16', full_batch_parts_per_step=4, **ON)
    assert check_full_batch_parts() == (4, 4, 'rows')


@pytest.mark.parametrize("flags,msg", [
    (dict(full_batch=True, full_batch_parts=-1), r"--full_batch_parts must be >= 0"),
    (dict(full_batch_parts=4), r"--full_batch_parts needs --full_batch"),
    (dict(ON, full_batch_parts_per_step=0), r"--full_batch_parts_per_step must lie in \[1, --full_batch_parts = 4\], got 0"),
    (dict(ON, full_batch_parts_per_step=5), r"--full_batch_parts_per_step must lie in \[1, --full_batch_parts = 4\], got 5"),
    (dict(ON, edge_dropout=0.1), r"--full_batch_parts is not supported with --edge_dropout"),
    (dict(ON, feature_dtype='bf16', dense_dtype='bf16'), r"--full_batch_parts is not supported with --feature_dtype bf16"),
    (dict(ON, full_batch_kernel='cs'), r"--full_batch_parts is not supported with --full_batch_kernel cs"),
    (dict(ON, full_batch_kernel='lds'), r"--full_batch_parts is not supported with --full_batch_kernel lds"),
    (dict(ON, full_batch_part_norm='cols'), r"--full_batch_part_norm must be one of rows/keep"),
])
def test_refusals(flags, msg):
    from stochastic_gcn_amd.full_batch import check_full_batch_parts
    FLAGS.update(**flags)
    with pytest.raises(ValueError, match=msg):
        check_full_batch_parts()


def test_more_parts_than_vertices_is_refused_once_the_graph_is_known():
    from stochastic_gcn_amd.full_batch import check_full_batch_parts
    FLAGS.update(**ON)
    assert check_full_batch_parts(num_vertices=4) == (4, 1, 'rows')
    with pytest.raises(ValueError, match=r"--full_batch_parts 4 is more than the graph's 3 vertices"):
        check_full_batch_parts(num_vertices=3)


@pytest.mark.parametrize("flags,msg", [
    (dict(full_batch_parts=4), "--full_batch_parts needs --full_batch"),
    (dict(ON, edge_dropout=0.1), "--full_batch_parts is not supported with --edge_dropout"),
    (dict(ON, full_batch_kernel='cs'), "--full_batch_parts is not supported with --full_batch_kernel cs"),
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


# ---- the partitioner ----------------------------------------------------------------------------------------------------
GRAPHS = {'sbm': ir.sbm_graph, 'flat': ir.flat_graph}


@pytest.mark.parametrize("graph", sorted(GRAPHS))
@pytest.mark.parametrize("P", [1, 2, 5])
def test_partition_covers_every_vertex_once(graph, P):
    from stochastic_gcn_amd.full_batch import partition
    a = GRAPHS[graph]()
    N = a.shape[0]
    parts = partition(a, P, seed=3)
    assert len(parts) == P and all(p.dtype == np.int32 and p.ndim == 1 and p.size > 0 for p in parts)
    assert all(np.all(np.diff(p) > 0) for p in parts)                        # ascending, unique
    assert np.array_equal(np.sort(np.concatenate(parts)), np.arange(N))      # every vertex in exactly one part
    again = partition(a, P, seed=3)
    assert all(np.array_equal(p, q) for p, q in zip(parts, again))           # deterministic
    sizes = [len(p) for p in parts]
    print("%s P=%d part sizes %s" % (graph, P, sizes))
    assert max(sizes) <= 2 * -(-N // P)          # largest-first packing of pieces of at most ceil(N / P)


def test_partition_keeps_planted_communities_together():
    """on the SBM graph most edges stay inside parts; on the graph without communities a balanced cut cannot do that"""
    from stochastic_gcn_amd.full_batch import part_stats, partition
    a, b = ir.sbm_graph(), ir.flat_graph()
    sa = part_stats(a, partition(a, 5, seed=1), np.arange(0, 300, 3))
    sb = part_stats(b, partition(b, 5, seed=1), np.arange(0, 300, 3))
    print("share of nonzeros inside parts: sbm %.3f, flat %.3f" % (sa['inside'], sb['inside']))
    assert sa['inside'] > sb['inside'] and 0.0 < sb['inside'] < 1.0
    assert sa['sizes'][0] >= 1 and sum(sa['train'][k] >= 0 for k in range(3)) == 3


def test_partition_never_leaves_a_part_empty():
    from stochastic_gcn_amd.full_batch import partition
    a = sp.identity(9, dtype=np.float32, format='csr')             # ceil(9 / 4) = 3: three pieces of one community
    for P in (4, 9):
        parts = partition(a, P, seed=1)
        assert len(parts) == P and all(p.size > 0 for p in parts)
        assert np.array_equal(np.sort(np.concatenate(parts)), np.arange(9))
    for P in (0, 10):
        with pytest.raises(ValueError, match="partition: P must lie in"):
            partition(a, P, seed=1)


# ---- the schedule -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,q", [(5, 1), (5, 2), (5, 5), (4, 2), (1, 1)])
def test_schedule_uses_every_part_once_per_epoch(P, q):
    from stochastic_gcn_amd.full_batch import PartSchedule, partition
    a = ir.sbm_graph()
    parts = partition(a, P, seed=1)
    s = PartSchedule(parts, q, seed=7)
    assert len(s) == -(-P // q)
    seen = []
    for e in range(4):
        groups, unions = s.groups(e), s.epoch(e)
        assert len(groups) == len(unions) == -(-P // q)
        assert sorted(int(j) for g in groups for j in g) == list(range(P))          # every part exactly once
        assert all(len(g) == q for g in groups[:-1]) and 1 <= len(groups[-1]) <= q
        for g, u in zip(groups, unions):
            assert np.all(np.diff(u) > 0) and np.array_equal(u, np.sort(np.concatenate([parts[j] for j in g])))
        assert np.array_equal(np.sort(np.concatenate(unions)), np.arange(a.shape[0]))
        assert all(np.array_equal(x, y) for x, y in zip(unions, s.epoch(e)))        # seeded by (seed, e)
        seen.append(tuple(int(j) for g in groups for j in g))
    if P == 5:
        assert len(set(seen)) > 1                                                   # epochs differ
        other = PartSchedule(parts, q, seed=8)
        assert [tuple(int(j) for g in other.groups(e) for j in g) for e in range(4)] != seen
    with pytest.raises(ValueError, match="q must lie in"):
        PartSchedule(parts, P + 1, seed=7)


# ---- the plain-loop reference against SciPy -----------------------------------------------------------------------------
def _subsets(N, rng):
    return {'all': np.arange(N), 'one': np.array([N // 3]), 'every_other': np.arange(0, N, 2),
            'third': np.sort(rng.choice(N, max(N // 3, 1), replace=False))}


@pytest.mark.parametrize("name", ['sbm', 'flat', 'permutation', 'm64_k64', 'identity'])
def test_reference_is_scipy(name):
    a = GRAPHS[name]() if name in GRAPHS else sc.pattern(name)
    a = ir.signed(a, seed=5)
    a.sort_indices()
    N = a.shape[0]
    for sname, ids in _subsets(N, np.random.RandomState(2)).items():
        want = a[ids][:, ids].tocsr()
        assert want.has_sorted_indices or np.all([np.all(np.diff(want.indices[want.indptr[i]:want.indptr[i + 1]]) > 0)
                                                  for i in range(len(ids))])
        rowptr, col, val = ir.block(a, ids)
        assert np.array_equal(rowptr, want.indptr) and np.array_equal(col, want.indices), (name, sname)
        assert np.array_equal(val.view(np.uint32), want.data.astype(np.float32).view(np.uint32)), (name, sname)
        # the stable transpose is SciPy's .T.tocsr() (rows ascend inside a column), the values the block's own, permuted
        n = len(ids)
        t_rowptr, t_col, t_src = ir.transpose(n, rowptr, col)
        wt = sp.csr_matrix((val, col, rowptr), shape=(n, n)).T.tocsr()
        wt.sort_indices()
        assert np.array_equal(t_rowptr, wt.indptr) and np.array_equal(t_col, wt.indices), (name, sname)
        assert np.array_equal(val[t_src].view(np.uint32), wt.data.view(np.uint32)), (name, sname)
        # the row sums and the 'rows' rescaling: every row keeps its value sum
        full, kept, length = ir.row_sums(a, ids)
        assert np.allclose(full, np.asarray(a[ids].astype(np.float64).sum(axis=1)).ravel(), rtol=1e-12, atol=1e-12)
        assert np.allclose(kept, np.asarray(want.astype(np.float64).sum(axis=1)).ravel(), rtol=1e-12, atol=1e-12)
        assert np.array_equal(length, np.diff(a.indptr)[ids])
    p = ir.positive(a)
    ids = _subsets(N, np.random.RandomState(2))['every_other']
    rowptr, _, _ = ir.block(p, ids)
    scaled = ir.block_rows_f64(p, ids)
    full, kept, _ = ir.row_sums(p, ids)
    sums = np.array([scaled[rowptr[i]:rowptr[i + 1]].sum() for i in range(len(ids))])
    assert np.allclose(sums[kept > 0], full[kept > 0], rtol=1e-12)


# ---- the exports' argument checks, through the raw C-ABI ----------------------------------------------------------------
def test_exports_are_declared_and_bound():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sgcn.h")).read()
    for s in NEW:
        assert s in _ffi.SIGNATURES and hasattr(_ffi.lib, s) and (s + "(") in header
    assert _ffi.lib.sgcn_abi_version() == 16              # additive exports: the ABI version stays


def _err():
    return _ffi.lib.sgcn_last_error() or b""


def test_map_argument_checks():
    lib = _ffi.lib
    assert lib.sgcn_induce_map_i32(None, -1, 10, None, None) == -1 and b"negative size" in _err()
    assert lib.sgcn_induce_map_i32(None, 0, -1, None, None) == -1 and b"negative size" in _err()
    assert lib.sgcn_induce_map_i32(None, 11, 10, None, None) == -1 and b"11 ids cannot be unique in [0, 10)" in _err()
    assert lib.sgcn_induce_map_i32(None, 3, 10, None, None) == -1 and b"null operand" in _err()
    ids = np.arange(3, dtype=np.int32)
    assert lib.sgcn_induce_map_i32(ids.ctypes.data, 3, 10, None, None) == -1 and b"null operand" in _err()
    assert lib.sgcn_induce_map_i32(None, 0, 0, None, None) == 0                      # nothing to do: no HIP call


def test_count_argument_checks():
    lib = _ffi.lib
    assert lib.sgcn_csr_induce_count(None, None, None, None, -1, None, None, None, None, None) == -1 and b"negative size" in _err()
    assert lib.sgcn_csr_induce_count(None, None, None, None, 3, None, None, None, None, None) == -1 and b"null operand" in _err()
    x = np.zeros(8, dtype=np.int32)
    p = x.ctypes.data
    assert lib.sgcn_csr_induce_count(p, p, None, None, 3, p, p, None, None, None) == -1 and b"null operand" in _err()      # ids
    assert lib.sgcn_csr_induce_count(p, p, p, p, 3, p, p, None, None, None) == -1 and b"null operand" in _err()   # values, no sums
    assert lib.sgcn_csr_induce_count(None, None, None, None, 0, None, None, None, None, None) == 0


def test_fill_argument_checks():
    lib = _ffi.lib
    none12 = [None] * 4
    assert lib.sgcn_csr_induce_fill(*none12, -1, None, None, None, None, None, None, 0, 0, None) == -1 and b"negative size" in _err()
    assert lib.sgcn_csr_induce_fill(*none12, 2, None, None, None, None, None, None, 0, -5, None) == -1 and b"negative size" in _err()
    assert lib.sgcn_csr_induce_fill(*none12, 2, None, None, None, None, None, None, 0, 0, None) == -1 and b"null operand" in _err()
    x = np.zeros(8, dtype=np.int32)
    p = x.ctypes.data
    assert lib.sgcn_csr_induce_fill(p, p, p, p, 2, p, p, None, p, None, None, 0, 0, None) == -1 and b"null operand" in _err()    # no o_val
    assert lib.sgcn_csr_induce_fill(p, p, None, p, 2, p, p, p, p, None, None, 0, 0, None) == -1 and b"rscale needs values" in _err()
    assert lib.sgcn_csr_induce_fill(*none12, 0, None, None, None, None, None, None, 0, 0, None) == 0


def test_ops_check_the_vertex_set_on_the_host():
    from stochastic_gcn_amd import ops
    for bad in ([3, 2], [1, 1], [-1, 2], [0, 10], [], [[1, 2]]):
        with pytest.raises(ValueError, match="induced subgraph"):
            ops.check_induce_ids(np.array(bad, dtype=np.int64), 10)
    assert ops.check_induce_ids(np.array([0, 4, 9]), 10).dtype == np.int32
    a = sp.identity(4, format='csr', dtype=np.float32)
    A = ops.DeviceCSR.from_scipy(a, torch.device("cpu"), with_plan=False)
    with pytest.raises(ValueError, match="norm must be one of keep/rows"):
        ops.csr_induce(A, np.arange(2), norm='cols')
    with pytest.raises(ValueError, match="induced subgraph"):
        ops.csr_induce(A, np.array([2, 1]))
