"""GPU tests of ops.spmm_pull (sgcn_spmm_pull.hip): the two-table gather product of --full_batch_part_history against the fp64
statement of tests/part_history_ref.py -- bit for bit on dyadic inputs, within the row kernel's fp64 bound
(sparse_cases.fp64_bound, what tests/test_sparse_exact_gpu.py applies at the same row length) on real-valued ones -- on the
patterns and vertex sets of the induce tests (a 330-entry row: five chunks and a tail at 64 lanes; rows that store nothing;
rows without an in-part entry; S = everything, S = one vertex), at d in {1, 3, 4, 5, 64, 132, 602} and on pitches that force
every vector width.  The bfloat16-history form must give the fp32 form's bits on the widened table at every shape; two runs
give equal bits; stored rows of S and fresh rows outside the map are never read; nothing is written past d.
N <= 400 throughout; every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import induce_ref as ir
import part_history_ref as pr
import sparse_cases as sc
from test_induce_gpu import PATTERNS, _subsets

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
WIDTHS = (1, 3, 4, 5, 64, 132, 602)
# two widths per vertex set, every width used, on every pattern
WIDTHS_OF = {'all': (1, 64), 'one': (3, 602), 'every_other': (4, 132), 'third': (5, 64)}
SENTINEL = -777.0


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _pitched(x, pitch, fill=0.0):
    """the (n, d) array ``x`` as the [:, :d] view of an (n, pitch) fp32 device table"""
    x = np.asarray(x, np.float32)
    t = torch.full((max(x.shape[0], 1), pitch), fill, dtype=torch.float32, device=DEV)[:x.shape[0]]
    t[:, :x.shape[1]] = torch.from_numpy(x).to(DEV)
    return t[:, :x.shape[1]]


def _pitch(d, vw):
    """a row pitch >= d under which the widest vector is ``vw`` (4: 16-byte rows; 2: 8-byte rows; 1: an odd pitch)"""
    if vw == 4:
        return (d + 3) // 4 * 4
    if vw == 2:
        return (d + 1) // 2 * 2 + (2 if ((d + 1) // 2 * 2) % 4 == 0 else 0)
    return d + (1 if d % 2 == 0 else 2)


class Resident(object):
    """a resident DeviceCSR with the map of one vertex set"""

    def __init__(self, a):
        from stochastic_gcn_amd import ops
        self.a, self.N = a, a.shape[0]
        self.A = ops.DeviceCSR.from_scipy(a, DEV, with_plan=False)
        self.map = torch.empty(self.N, dtype=torch.int32, device=DEV)

    def select(self, ids):
        from stochastic_gcn_amd import _ffi, ops
        self.ids = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(DEV)
        _ffi.check(_ffi.lib.sgcn_induce_map_i32(self.ids.data_ptr(), len(ids), self.N, self.map.data_ptr(), ops._stream()))
        assert np.array_equal(self.map.cpu().numpy(), pr.position_map(self.N, ids))
        return self

    def pull(self, x, H, ldc=None):
        """(result, the whole padded output) of one launch into a sentinel-filled table of pitch ldc"""
        from stochastic_gcn_amd import ops
        n, d = int(x.shape[0]), int(x.shape[1])
        full = torch.full((max(n, 1), ldc or d), SENTINEL, dtype=torch.float32, device=DEV)[:n]
        out = ops.spmm_pull(self.A, self.ids, self.map, x, H, out=full[:, :d])
        assert out.data_ptr() == full.data_ptr()
        return out.cpu().numpy(), full.cpu().numpy()


def _h16(H32):
    """(the bfloat16 table of ops.history_alloc's layout holding H32 rounded, the same rows widened into an fp32 table of the
    same element pitch)"""
    from stochastic_gcn_amd import ops
    N, d = H32.shape
    Hb = ops.history_assign(ops.history_alloc(N, d, DEV, bf16=True), torch.from_numpy(np.asarray(H32, np.float32)).to(DEV))
    wide = ops.history_widen(Hb).cpu().numpy()
    assert np.array_equal(_bits(wide), _bits(pr.widen_bf16(pr.round_bf16(H32))))
    return Hb, _pitched(wide, int(Hb.stride(0))), wide


def _both(r, x, H32, ldc=None):
    """the fp32 form on H32, then the bfloat16 form against the fp32 form on the widened table: (fp32 result, its padded
    output); asserts the two forms' bits, two runs' bits and the padding"""
    d = int(x.shape[1])
    got, full = r.pull(x, _pitched(H32, _pitch(d, 4)), ldc)
    again, _ = r.pull(x, _pitched(H32, _pitch(d, 4)), ldc)
    assert np.array_equal(_bits(got), _bits(again)), "two runs differ"
    assert np.all(full[:, d:] == SENTINEL), "written past d"
    Hb, Hw, _ = _h16(H32)
    g16, full16 = r.pull(x, Hb, ldc)
    g32, _ = r.pull(x, Hw, ldc)
    assert np.array_equal(_bits(g16), _bits(g32)), "the bfloat16 form is not the fp32 form on the widened table"
    assert np.all(full16[:, d:] == SENTINEL)
    return got, g16


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_dyadic_inputs_give_the_exact_product(name):
    rng = np.random.RandomState(21)
    a = sc.dyadic(PATTERNS[name](rng), rng)
    a.sort_indices()
    r = Resident(a)
    N = a.shape[0]
    assert N <= 400
    for sname, ids in _subsets(N, rng).items():
        r.select(ids)
        for d in WIDTHS_OF[sname]:
            X, H = sc.ints(rng, (len(ids), d)), sc.ints(rng, (N, d))             # (integers in [-8, 8]: bfloat16 holds them)
            want = pr.pull(a, ids, X, H)
            assert float(pr.pull_magnitude(a, ids, X, H).max(initial=0.0)) < 2.0 ** 20       # exact in fp32 in any order
            got, g16 = _both(r, _pitched(X, _pitch(d, 4)), H, ldc=_pitch(d, 4) + 4)
            lens = np.diff(a.indptr)[ids]
            bad = int(np.sum(got.astype(np.float64) != want)), int(np.sum(g16.astype(np.float64) != want))
            print("%s / %s / d=%d: n %d, longest row %d, empty rows %d, wrong elements f32 %d h16 %d"
                  % (name, sname, d, len(ids), int(lens.max()), int(np.sum(lens == 0)), bad[0], bad[1]))
            assert bad == (0, 0)
            assert np.array_equal(_bits(got), _bits(want.astype(np.float32)))


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_real_inputs_stay_within_the_row_kernels_bound(name):
    rng = np.random.RandomState(22)
    a = ir.signed(PATTERNS[name](rng), seed=7)
    a.sort_indices()
    r = Resident(a)
    N = a.shape[0]
    for sname, ids in _subsets(N, rng).items():
        r.select(ids)
        d = WIDTHS_OF[sname][0] if name != 'hub' else WIDTHS_OF[sname][1]
        X, H = rng.randn(len(ids), d).astype(np.float32), rng.randn(N, d).astype(np.float32)
        got, g16 = _both(r, _pitched(X, _pitch(d, 4)), H)
        sub = a[ids].tocsr()
        for what, g, tab in (('f32', got, H), ('h16', g16, pr.widen_bf16(pr.round_bf16(H)))):
            Z = pr.merged(ids, X, tab)                # the pull IS the plain product of A[ids] with the merged table
            want, bound = pr.pull(a, ids, X, tab), sc.fp64_bound(sub, Z)
            assert np.allclose(want, sc.spmm_f64(sub, Z), rtol=1e-12, atol=1e-12)
            err = np.abs(g.astype(np.float64) - want)
            print("%s / %s / d=%d %s: longest row %d, worst error %.3e = %.3f of its bound"
                  % (name, sname, d, what, int(np.diff(sub.indptr).max()), float(err.max(initial=0.0)),
                     float((err / bound).max(initial=0.0))))
            assert np.all(err <= bound)


@pytest.mark.parametrize("vw", [4, 2, 1])
@pytest.mark.parametrize("d", WIDTHS)
def test_every_width_on_every_vector_width(d, vw):
    """the hub graph (a 330-entry row, a 64- and a 65-entry row) under S = a third: X and C on pitches that allow exactly
    ``vw`` elements per vector, exact on dyadic inputs"""
    rng = np.random.RandomState(23)
    a = sc.dyadic(PATTERNS['hub'](rng), rng)
    a.sort_indices()
    N = a.shape[0]
    ids = _subsets(N, rng)['third']
    ids = np.union1d(ids, [7, 8, 9]).astype(np.int32)                 # the long rows are selected
    r = Resident(a).select(ids)
    X, H = sc.ints(rng, (len(ids), d)), sc.ints(rng, (N, d))
    want = pr.pull(a, ids, X, H)
    ld = _pitch(d, vw)
    assert ld >= d and (ld % 4 == 0 if vw == 4 else ld % 4 == 2 if vw == 2 else ld % 2 == 1)
    got, g16 = _both(r, _pitched(X, ld), H, ldc=ld)
    print("d=%d vw=%d pitch %d: n %d, rows of %s entries" % (d, vw, ld, len(ids), sorted(set(np.diff(a.indptr)[[7, 8, 9]]))))
    assert np.diff(a.indptr)[7] >= 300
    assert np.array_equal(_bits(got), _bits(want.astype(np.float32))) and np.array_equal(_bits(g16), _bits(got))
    # the fp32 history on the same narrow pitch too
    again, full = r.pull(_pitched(X, ld), _pitched(H, ld), ldc=ld)
    assert np.array_equal(_bits(again), _bits(got)) and np.all(full[:, d:] == SENTINEL)


@pytest.mark.parametrize("d", [3, 64])
def test_stored_rows_of_the_vertex_set_are_never_read(d):
    """H[ids] = NaN with X finite: the result is finite and unchanged -- in-part columns never touch H"""
    rng = np.random.RandomState(24)
    a = ir.signed(PATTERNS['sbm'](rng), seed=2)
    N = a.shape[0]
    for sname, ids in _subsets(N, rng).items():
        r = Resident(a).select(ids)
        X, H = rng.randn(len(ids), d).astype(np.float32), rng.randn(N, d).astype(np.float32)
        clean, c16 = _both(r, _pitched(X, _pitch(d, 4)), H)
        H[ids] = np.nan
        got, g16 = _both(r, _pitched(X, _pitch(d, 4)), H)
        print("%s d=%d: finite %s / %s" % (sname, d, bool(np.isfinite(got).all()), bool(np.isfinite(g16).all())))
        assert np.isfinite(got).all() and np.isfinite(g16).all()
        assert np.array_equal(_bits(got), _bits(clean)) and np.array_equal(_bits(g16), _bits(c16))


def test_rows_without_an_in_part_entry_never_read_x():
    """the lose_all pattern under S = every other vertex: no selected row stores a column of S, so no row of X is ever
    addressed -- X = NaN leaves the result finite, and it is the product of the stored rows alone"""
    rng = np.random.RandomState(25)
    a = sc.dyadic(PATTERNS['lose_all'](rng), rng)
    a.sort_indices()
    N = a.shape[0]
    ids = _subsets(N, rng)['every_other']
    assert pr.block(a, ids).nnz == 0 and a[ids].nnz > 0
    r = Resident(a).select(ids)
    for d in (5, 132):
        H = sc.ints(rng, (N, d))
        X = np.full((len(ids), d), np.nan, np.float32)
        got, g16 = _both(r, _pitched(X, _pitch(d, 4)), H)
        want = pr.pull(a, ids, np.zeros_like(X), H)
        assert np.isfinite(got).all() and np.array_equal(_bits(got), _bits(want.astype(np.float32)))
        assert np.array_equal(_bits(g16), _bits(got))


def test_no_rows_is_no_launch():
    from stochastic_gcn_amd import ops
    a = ir.signed(ir.flat_graph(50, 3, seed=1), seed=1)
    r = Resident(a)
    r.ids = torch.empty(0, dtype=torch.int32, device=DEV)
    for H in (torch.zeros((50, 4), device=DEV), ops.history_alloc(50, 4, DEV, bf16=True)):
        out = ops.spmm_pull(r.A, r.ids, r.map, torch.empty((0, 4), device=DEV), H)
        assert tuple(out.shape) == (0, 4)


def test_csr_induce_hands_out_its_map():
    """the block keeps the position map it was cut with (the step does not compute it twice); nothing else of it changes"""
    from stochastic_gcn_amd import ops
    a = ir.signed(ir.sbm_graph(), seed=1)
    A = ops.DeviceCSR.from_scipy(a, DEV, with_plan=False, with_transpose=True)
    ids = np.arange(0, a.shape[0], 3, dtype=np.int32)
    blk = ops.csr_induce(A, ids, norm='keep')
    assert np.array_equal(blk.map.cpu().numpy()[:a.shape[0]], pr.position_map(a.shape[0], ids))
    want = ir.block(a, ids)
    assert np.array_equal(blk.col.cpu().numpy(), want[1]) and np.array_equal(_bits(blk.val.cpu().numpy()), _bits(want[2]))
    x = torch.randn((len(ids), 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    H = torch.randn((a.shape[0], 8), generator=torch.Generator().manual_seed(2)).to(DEV)
    got = ops.spmm_pull(A, torch.from_numpy(ids).to(DEV), blk.map, x, H).cpu().numpy()
    want = pr.pull(a, ids, x.cpu().numpy(), H.cpu().numpy())
    assert np.all(np.abs(got - want) <= sc.fp64_bound(a[ids].tocsr(), pr.merged(ids, x.cpu().numpy(), H.cpu().numpy())))
