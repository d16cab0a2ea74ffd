"""GPU tests of ops.csr_induce (sgcn_induce.hip): the induced block A[S, S] of a resident CSR cut on the device, against the
plain-loop reference of tests/induce_ref.py (which tests/test_full_batch_parts.py holds to SciPy) -- bit for bit under
norm='keep', within the fp32 bound of its two sums, one division and one product under norm='rows' -- with its stable
transpose, its plans, and the same bits on a second run -- the transposed block both ways: by the device transposition of the
block, and as the same cut of a resident transpose (what the trainer keeps).  N <= 400 throughout; every figure is printed before it is asserted."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import induce_ref as ir
import sparse_cases as sc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
DEFAULT_T = 256            # include/sgcn.h: the split threshold of a plan built with T = 0
WAVE = 64                  # entries a row's wavefront looks at per chunk


def _empty_rows(rng):
    """a third of the rows store nothing (their columns stay in use)"""
    a = ir.flat_graph(300, 5, seed=4).tolil()
    for i in rng.choice(300, 100, replace=False):
        a.rows[i], a.data[i] = [], []
    return a.tocsr()


def _lose_all(rng):
    """even rows store odd columns only: under S = every other vertex they lose every entry; odd rows store both kinds"""
    n = 301
    rows, cols = [], []
    for i in range(n):
        k = rng.randint(1, 7)
        pool = np.arange(1, n, 2) if i % 2 == 0 else np.arange(n)
        rows.append(np.full(k, i)); cols.append(rng.choice(pool, k, replace=False))
    return sc._csr(n, n, np.concatenate(rows), np.concatenate(cols))


def _hub(rng):
    """row 7 stores 330 of 400 columns -- longer than the default T and than 5 chunks of 64 + 1 --, column 11 is stored by 330
    rows (the transposed block's hub), row 8 exactly 64 and row 9 exactly 65 entries (a full chunk, a chunk and one)"""
    n = 400
    assert 330 > DEFAULT_T and 330 > 5 * WAVE + 1
    base = ir.flat_graph(n, 3, seed=6).tocoo()
    rows = [base.row, np.full(330, 7), rng.choice(n, 330, replace=False), np.full(64, 8), np.full(65, 9)]
    cols = [base.col, rng.choice(n, 330, replace=False), np.full(330, 11), rng.choice(n, 64, replace=False),
            rng.choice(n, 65, replace=False)]
    return sc._csr(n, n, np.concatenate(rows), np.concatenate(cols))


PATTERNS = {
    'empty_rows': _empty_rows, 'lose_all': _lose_all, 'hub': _hub,
    'diagonal': lambda rng: sp.identity(257, dtype=np.float32, format='csr'),
    'sbm': lambda rng: ir.sbm_graph(),
    # the adversarial patterns of sparse_cases that are square and small enough
    'permutation': sc.p_permutation, 'identity': sc.p_identity, 'm16_k16': sc.CATALOGUE['m16_k16'],
    'm64_k64': sc.CATALOGUE['m64_k64'],
}


def _subsets(N, rng):
    return {'all': np.arange(N, dtype=np.int32), 'one': np.array([N // 3], dtype=np.int32),
            'every_other': np.arange(0, N, 2, dtype=np.int32),
            'third': np.sort(rng.choice(N, max(N // 3, 1), replace=False)).astype(np.int32)}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _host(block):
    """everything csr_induce returned, on the host (the device buffers are reused by the next call)"""
    t = block.transpose
    return dict(rowptr=block.rowptr.cpu().numpy(), col=block.col.cpu().numpy(), val=block.val.cpu().numpy(),
                coo=block.coo_rows.cpu().numpy(), host_rowptr=block.host_rowptr.copy(),
                t_rowptr=t.rowptr.cpu().numpy(), t_col=t.col.cpu().numpy(), t_val=t.val.cpu().numpy(),
                t_host_rowptr=t.host_rowptr.copy(), seg=block.plan.seg.cpu().numpy(), t_seg=t.plan.seg.cpu().numpy(),
                nfix=(block.plan.nfix, t.plan.nfix), shape=(block.shape, t.shape, block.nnz, t.nnz))


RESIDENT = pytest.mark.parametrize("resident", [False, True], ids=['transposition', 'resident_transpose'])


@RESIDENT
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_keep_is_the_reference_bit_for_bit(name, resident):
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd.scheduler import build_plan
    rng = np.random.RandomState(11)
    a = ir.signed(PATTERNS[name](rng), seed=3)
    a.sort_indices()
    N = a.shape[0]
    assert a.shape[0] == a.shape[1] and N <= 400
    A = ops.DeviceCSR.from_scipy(a, DEV, with_plan=False, with_transpose=resident)
    for sname, ids in _subsets(N, rng).items():
        n = len(ids)
        rowptr, col, val = ir.block(a, ids)
        t_rowptr, t_col, t_src = ir.transpose(n, rowptr, col)
        got = _host(ops.csr_induce(A, ids, norm='keep'))
        lost = int(np.sum((np.diff(a.indptr)[ids] > 0) & (np.diff(rowptr) == 0)))
        print("%s / %s: n %d, kept %d of %d entries, %d rows lose every entry, longest full row %d"
              % (name, sname, n, rowptr[-1], int(np.diff(a.indptr)[ids].sum()), lost, int(np.diff(a.indptr)[ids].max())))
        assert got['shape'] == ((n, n), (n, n), int(rowptr[-1]), int(rowptr[-1]))
        assert np.array_equal(got['rowptr'], rowptr) and np.array_equal(got['host_rowptr'], rowptr)
        assert np.array_equal(got['col'], col) and np.array_equal(_bits(got['val']), _bits(val))
        assert np.array_equal(got['coo'], np.repeat(np.arange(n), np.diff(rowptr)))
        # the transposed block: the stable transpose, its values the block's own, permuted
        assert np.array_equal(got['t_rowptr'], t_rowptr) and np.array_equal(got['t_host_rowptr'], t_rowptr)
        assert np.array_equal(got['t_col'], t_col) and np.array_equal(_bits(got['t_val']), _bits(val[t_src]))
        # the plans: scheduler.build_plan on the row pointer with T = 0, what DeviceCSR.from_scipy makes of the same matrix
        for key, rp in (('seg', rowptr), ('t_seg', t_rowptr)):
            seg, _, _ = build_plan(rp, 0)
            assert np.array_equal(got[key].reshape(seg.shape), seg)
        # a second run gives the same bits
        again = _host(ops.csr_induce(A, ids, norm='keep'))
        assert all(got[k].tobytes() == again[k].tobytes() for k in got if isinstance(got[k], np.ndarray))
    if name == 'lose_all':
        ids = _subsets(N, rng)['every_other']
        assert np.all(np.diff(ir.block(a, ids)[0]) == 0) and a[ids].nnz > 0        # every selected row lost everything
    if name == 'hub':
        full = _host(ops.csr_induce(A, np.arange(N, dtype=np.int32)))
        assert full['nfix'][0] >= 1 and full['nfix'][1] >= 1                        # the hub row and the hub column are split


@RESIDENT
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_rows_keeps_the_value_sums_within_the_fp32_bound(name, resident):
    """strictly positive values: every stored value within (2 len_i + 4) 2^-24, relative, of the fp64 reference -- two fp32 sums
    of at most len_i non-negative terms (len_i - 1 roundings each, in any order), one division, one product; S = all vertices
    gives the input's bits"""
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(12)
    a = ir.positive(PATTERNS[name](rng), seed=4)
    a.sort_indices()
    N = a.shape[0]
    A = ops.DeviceCSR.from_scipy(a, DEV, with_plan=False, with_transpose=resident)
    for sname, ids in _subsets(N, rng).items():
        rowptr, col, val = ir.block(a, ids)
        want = ir.block_rows_f64(a, ids)
        _, _, length = ir.row_sums(a, ids)
        got = _host(ops.csr_induce(A, ids, norm='rows'))
        assert np.array_equal(got['rowptr'], rowptr) and np.array_equal(got['col'], col)
        bound = np.repeat((2.0 * length + 4.0) * ir.U, np.diff(rowptr))
        err = np.abs(got['val'].astype(np.float64) - want) / np.abs(want) if len(want) else np.zeros(0)
        worst = float((err / bound).max()) if len(want) else 0.0
        print("%s / %s: %d values, worst relative error %.3e = %.3f of its bound" % (name, sname, len(want), float(err.max()) if len(want)
                                                                                  else 0.0, worst))
        assert np.all(err <= bound)
        if sname == 'all':
            assert np.array_equal(_bits(got['val']), _bits(a.data))
        else:
            sums = np.array([got['val'][rowptr[i]:rowptr[i + 1]].astype(np.float64).sum() for i in range(len(ids))])
            full, kept, _ = ir.row_sums(a, ids)
            assert np.allclose(sums[kept > 0], full[kept > 0], rtol=1e-4)
        t_rowptr, t_col, t_src = ir.transpose(len(ids), rowptr, col)
        assert np.array_equal(got['t_rowptr'], t_rowptr) and np.array_equal(got['t_col'], t_col)
        assert np.array_equal(_bits(got['t_val']), _bits(got['val'][t_src]))
        again = _host(ops.csr_induce(A, ids, norm='rows'))
        assert np.array_equal(_bits(again['val']), _bits(got['val'])) and np.array_equal(_bits(again['t_val']), _bits(got['t_val']))


def test_buffers_are_reused_and_grow():
    from stochastic_gcn_amd import ops
    a = ir.signed(ir.sbm_graph(), seed=1)
    A = ops.DeviceCSR.from_scipy(a, DEV, with_plan=False)
    N = a.shape[0]
    small = ops.csr_induce(A, np.arange(0, N, 4, dtype=np.int32))
    ptr, b = small.col.data_ptr(), A._induce
    rows, entries = b.rows, b.entries
    big = ops.csr_induce(A, np.arange(N, dtype=np.int32))
    assert A._induce is b and b.rows == N > rows and b.entries == a.nnz > entries
    again = ops.csr_induce(A, np.arange(0, N, 4, dtype=np.int32))
    assert again.col.data_ptr() == big.col.data_ptr() != ptr and (b.rows, b.entries) == (N, a.nnz)
    want = ir.block(a, np.arange(0, N, 4))
    assert np.array_equal(again.col.cpu().numpy(), want[1]) and np.array_equal(_bits(again.val.cpu().numpy()), _bits(want[2]))
