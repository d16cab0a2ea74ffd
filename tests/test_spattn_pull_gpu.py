"""GPU tests of ops.spattn_pull / ops.spattn_pull_bwd_q (sgcn_spattn_pull.hip): the two-table attention of
--full_batch_part_pull, on the patterns and vertex sets of the induce tests (a 330-entry row: five chunks and a tail at 64
lanes; 64- and 65-entry rows; rows that store nothing; rows without an in-part entry; S = everything, S = one vertex), at
(d, heads) in {(1,1), (3,1), (5,1), (8,2), (64,4), (64,8), (132,4), (602,1)} and on pitches that force every vector width.

  1. bit identity with the one-table kernels: with Z = H with the rows of S replaced by X (on the device, on H's pitch) and
     A_sub = the rows ids of the adjacency without a plan, the pull launches give the bits of ops.spattn(A_sub, Z, q=X) and of
     the dq of ops.spattn_bwd(A_sub, At_sub, Z, X, ...).  A condition, not a tolerance: both run the same arithmetic, and the
     one-table kernels are held to fp64 by tests/test_spattn*.py.
  2. the fp64 reference of tests/part_pull_attn_ref.py within spattn_ref's DERIVED bounds: C, lse, dQ, and the composed dX of
     PulledMatrix.pull_attn_backward within bound_dQ + bound_dB[ids] + u |dX|.  Nothing is fitted.
  3. the bfloat16 form gives the fp32 form's bits on the widened table, at every shape (inside every launch helper).
  4. hygiene: two runs give equal bits, nothing is written past d, H[ids] = NaN changes nothing, rows without an in-part entry
     read stored rows alone, an empty row gives +0.0 / -inf and its dQ is the addend alone, n == 0 is no launch.
  5. refusals.
N <= 400 throughout; every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import induce_ref as ir
import part_history_ref as pr
import part_pull_attn_ref as ar
import spattn_heads_ref as href
from test_induce_gpu import PATTERNS, _subsets
from test_spmm_pull_gpu import SENTINEL, Resident, _bits, _h16, _pitch, _pitched

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SHAPES = ((1, 1), (3, 1), (5, 1), (8, 2), (64, 4), (64, 8), (132, 4), (602, 1))
# two shapes per vertex set, every shape used, on every pattern
SHAPES_OF = {'all': ((1, 1), (64, 4)), 'one': ((3, 1), (602, 1)), 'every_other': ((8, 2), (132, 4)), 'third': ((5, 1), (64, 8))}
U = href.U


def _scale(d, heads):
    return float(np.float32(float(d // heads) ** -0.5))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)


def _graph(name, seed):
    rng = np.random.RandomState(seed)
    a = ir.signed(PATTERNS[name](rng), seed=7).tocsr()
    a.sort_indices()
    assert a.shape[0] <= 400
    return a, rng


def _hub_exact(seed):
    """the hub pattern with rows 8 and 9 cut to exactly 64 and 65 entries: a full chunk at 64 lanes, a chunk and one"""
    import scipy.sparse as sp
    a, rng = _graph('hub', seed)
    keep = np.ones(a.nnz, dtype=bool)
    for row, k in ((8, 64), (9, 65)):
        keep[a.indptr[row] + k:a.indptr[row + 1]] = False
    rows = np.repeat(np.arange(a.shape[0]), np.diff(a.indptr))[keep]
    a = sp.csr_matrix((a.data[keep], (rows, a.indices[keep])), shape=a.shape)
    a.sort_indices()
    assert list(np.diff(a.indptr)[[8, 9]]) == [64, 65] and np.diff(a.indptr)[7] >= 330
    return a, rng


class Pull(Resident):
    """the resident matrix, one vertex set, and the launches of both kinds into sentinel-filled tables"""

    def select(self, ids):
        from stochastic_gcn_amd import ops
        super(Pull, self).select(ids)
        self.ids_np = np.asarray(ids, np.int64)
        self.sub = self.a[self.ids_np].tocsr()
        self.sub.sort_indices()
        self.A_sub = ops.DeviceCSR.from_scipy(self.sub, DEV, with_plan=False, with_transpose=True)
        return self

    def merged(self, x, H32dev):
        """Z: the fp32 table ``H32dev`` (a pitched view) with the rows of S replaced by x, on the same pitch"""
        pitch = int(H32dev.stride(0)) if H32dev.shape[0] > 1 else int(H32dev.shape[1])
        Z = torch.zeros((H32dev.shape[0], pitch), dtype=torch.float32, device=DEV)[:, :H32dev.shape[1]]
        Z.copy_(H32dev)
        Z[torch.from_numpy(self.ids_np).to(DEV)] = x
        assert H32dev.shape[0] == 1 or Z.stride(0) == H32dev.stride(0)
        return Z

    def fwd(self, x, H, scale, heads, ldc=None):
        """(out, lse) as device tensors, twice (equal bits), into a sentinel table of pitch ldc (nothing past d)"""
        from stochastic_gcn_amd import ops
        n, d = int(x.shape[0]), int(x.shape[1])
        res = []
        for _ in range(2):
            full = torch.full((max(n, 1), ldc or _pitch(d, 4) + 4), SENTINEL, dtype=torch.float32, device=DEV)[:n]
            out, lse = ops.spattn_pull(self.A, self.ids, self.map, x, H, scale, out=full[:, :d], heads=heads)
            assert out.data_ptr() == full.data_ptr() and tuple(lse.shape) == ((n,) if heads == 1 else (n, heads))
            assert bool((full[:, d:] == SENTINEL).all()), "written past d"
            res.append((out, lse))
        assert np.array_equal(_bits(res[0][0].cpu().numpy()), _bits(res[1][0].cpu().numpy())), "two runs differ"
        assert np.array_equal(_bits(res[0][1].cpu().numpy()), _bits(res[1][1].cpu().numpy())), "two runs differ (lse)"
        return res[0]

    def bwd(self, x, H, g, out, lse, scale, heads, add=None, add_rows=0):
        from stochastic_gcn_amd import ops
        res = [ops.spattn_pull_bwd_q(self.A, self.ids, self.map, x, H, g, out, lse, scale, add=add, add_rows=add_rows, heads=heads)
               for _ in range(2)]
        for k in (0, 1):
            assert np.array_equal(_bits(res[0][k].cpu().numpy()), _bits(res[1][k].cpu().numpy())), "two runs differ"
        return res[0]

    def one_table(self, x, Z, g, scale, heads, add=None, add_rows=0, ldc=None):
        """(out, lse, dq) of the one-table kernels without a plan on (A_sub, Z, q = x)"""
        from stochastic_gcn_amd import ops
        n, d = int(x.shape[0]), int(x.shape[1])
        full = torch.full((max(n, 1), ldc or _pitch(d, 4) + 4), SENTINEL, dtype=torch.float32, device=DEV)[:n]
        out, lse = ops.spattn(self.A_sub, Z, q=x, scale=scale, out=full[:, :d], heads=heads)
        dq, _ = ops.spattn_bwd(self.A_sub, self.A_sub.transpose, Z, x, g, out, lse, scale, add=add, add_rows=add_rows, heads=heads)
        return out, lse, dq


def _same(x, y):
    return np.array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy()))


def _all_forms(r, X, H32, G, add, add_rows, scale, heads, ld=None, ldh=None):
    """Runs the fp32 form on H32 and the bfloat16 form on H32 rounded, each against the one-table kernels on its merged table
    (test 1) and the bfloat16 form against the fp32 form on the widened table (test 3).  X, G, add on pitch ``ld`` (default:
    16-byte rows), the fp32 history on ``ldh``.  Returns the fp32 form's (out, lse, dq, delta) and the bfloat16 form's, as
    NumPy arrays, and the widened table."""
    d = X.shape[1]
    ld = ld or _pitch(d, 4)
    x, g = _pitched(X, ld), _pitched(G, ld)
    ad = _pitched(add, ld) if add is not None else None
    Hd = _pitched(H32, ldh or ld)
    ldc = ld + 4                              # (the same alignment class, and room for the sentinel)
    out, lse = r.fwd(x, Hd, scale, heads, ldc=ldc)
    dq, delta = r.bwd(x, Hd, g, out, lse, scale, heads, add=ad, add_rows=add_rows)
    o1, l1, q1 = r.one_table(x, r.merged(x, Hd), g, scale, heads, add=ad, add_rows=add_rows, ldc=ldc)
    assert _same(out, o1), "forward: not the one-table kernel's bits"
    assert _same(lse, l1), "lse: not the one-table kernel's bits"
    assert _same(dq, q1), "bwd_q: not the one-table kernel's bits"
    Hb, Hw, wide = _h16(H32)
    out16, lse16 = r.fwd(x, Hb, scale, heads, ldc=ldc)
    dq16, delta16 = r.bwd(x, Hb, g, out16, lse16, scale, heads, add=ad, add_rows=add_rows)
    outw, lsew = r.fwd(x, Hw, scale, heads, ldc=ldc)
    dqw, deltaw = r.bwd(x, Hw, g, outw, lsew, scale, heads, add=ad, add_rows=add_rows)
    assert _same(out16, outw) and _same(lse16, lsew), "the bfloat16 form is not the fp32 form on the widened table"
    assert _same(dq16, dqw) and _same(delta16, deltaw), "the bfloat16 bwd_q is not the fp32 form on the widened table"
    o2, l2, q2 = r.one_table(x, r.merged(x, Hw), g, scale, heads, add=ad, add_rows=add_rows, ldc=ldc)
    assert _same(out16, o2) and _same(lse16, l2) and _same(dq16, q2), "bfloat16 form: not the one-table kernel's bits"
    f32 = tuple(t.cpu().numpy() for t in (out, lse, dq, delta))
    h16 = tuple(t.cpu().numpy() for t in (out16, lse16, dq16, delta16))
    return f32, h16, wide


def _within(what, got, want, bound):
    got, want = np.asarray(got, np.float64).reshape(np.shape(want)), np.asarray(want, np.float64)
    both_inf = np.isneginf(got) & np.isneginf(want)
    err = np.where(both_inf, 0.0, np.abs(got - np.where(both_inf, 0.0, want)))
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(err > 0, err / bound, 0.0)
    print("        %-6s worst error %.3e = %.3f of its bound" % (what, float(err.max(initial=0.0)), float(frac.max(initial=0.0))))
    assert np.all(err <= bound), what


def _check_fp64(r, a, ids, X, tab, G, add, add_rows, scale, heads, got):
    """test 2 for one launch: ``got`` = (out, lse, dq, delta) against the reference on the table ``tab``"""
    ref = ar.backward(a, ids, X, tab, G, scale, heads, add=add, add_rows=add_rows)
    f = ref['fwd']
    _within('C', got[0], f.C, f.bound_C)
    _within('lse', got[1], f.lse, f.bound_lse)
    _within('dQ', got[2], ref['dQ'], ref['bound_dQ'])
    return ref


# ---- 1 + 3 (+ 2 on the fp32 form): every pattern, every vertex set ---------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_bits_of_the_one_table_kernels_and_the_fp64_reference(name):
    a, rng = _graph(name, 31)
    N = a.shape[0]
    r = Pull(a)
    for sname, ids in _subsets(N, rng).items():
        r.select(ids)
        n = len(ids)
        for d, heads in SHAPES_OF[sname]:
            scale = _scale(d, heads)
            X, H, G, add = (rng.randn(*s).astype(np.float32) for s in ((n, d), (N, d), (n, d), (n, d)))
            add_rows = n if d % 2 else n // 2
            lens = np.diff(a.indptr)[ids]
            inside = pr.position_map(N, ids)[r.sub.indices] >= 0
            print("%s / %s / d=%d heads=%d: n %d, longest row %d, empty rows %d, %d of %d entries in-part"
                  % (name, sname, d, heads, n, int(lens.max()), int(np.sum(lens == 0)), int(inside.sum()), inside.size))
            f32, h16, wide = _all_forms(r, X, H, G, add, add_rows, scale, heads)
            _check_fp64(r, a, ids, X, H, G, add, add_rows, scale, heads, f32)
            if d in (5, 64):
                _check_fp64(r, a, ids, X, wide, G, add, add_rows, scale, heads, h16)


# ---- every (d, heads) on every vector width -------------------------------------------------------------------------------
@pytest.mark.parametrize("vw", [4, 2, 1])
@pytest.mark.parametrize("d,heads", SHAPES)
def test_every_shape_on_every_vector_width(d, heads, vw):
    """the hub graph (a row of 330 and more entries, one of exactly 64 and one of exactly 65) under S = a third plus the long rows: X, G, the addend, C
    and the fp32 history on pitches that allow exactly ``vw`` elements per vector.  602 columns need VW = 4 (d <= 256 * VW):
    on the narrower pitches the launch is refused with the width message"""
    from stochastic_gcn_amd import ops
    a, rng = _hub_exact(33)
    N = a.shape[0]
    ids = np.union1d(_subsets(N, rng)['third'], [7, 8, 9]).astype(np.int32)
    r = Pull(a).select(ids)
    n = len(ids)
    scale = _scale(d, heads)
    X, H, G, add = (rng.randn(*s).astype(np.float32) for s in ((n, d), (N, d), (n, d), (n, d)))
    ld = _pitch(d, vw)
    assert ld >= d and (ld % 4 == 0 if vw == 4 else ld % 4 == 2 if vw == 2 else ld % 2 == 1)
    eff = ops.attn_vw(d, _pitched(X, ld), heads=heads)
    print("d=%d heads=%d vw=%d pitch %d (effective VW %d): n %d, rows of %s entries"
          % (d, heads, vw, ld, eff, n, sorted(set(np.diff(a.indptr)[[7, 8, 9]]))))
    assert eff <= vw
    if d > 256 * eff:
        with pytest.raises(RuntimeError, match=r"spattn_pull: d = %d is over the limit of %d columns at vector width %d" % (d, 256 * eff, eff)):
            ops.spattn_pull(r.A, r.ids, r.map, _pitched(X, ld), _pitched(H, ld), scale, heads=heads, out=_pitched(X, ld).clone())
        return
    f32, h16, wide = _all_forms(r, X, H, G, add, n, scale, heads, ld=ld)
    _check_fp64(r, a, ids, X, H, G, add, n, scale, heads, f32)
    _check_fp64(r, a, ids, X, wide, G, add, n, scale, heads, h16)


# ---- 2. the composed gradient --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("name,sname,d,heads", [('hub', 'third', 64, 4), ('sbm', 'every_other', 8, 2), ('empty_rows', 'third', 5, 1),
                                                ('lose_all', 'every_other', 3, 1), ('sbm', 'all', 132, 4), ('hub', 'one', 602, 1)])
def test_pulled_matrix_backward_is_dq_plus_the_blocks_db(name, sname, d, heads, bf16):
    """PulledMatrix.pull_attn_product / pull_attn_backward over the block ops.csr_induce cut: dX within
    bound_dQ + bound_dB[ids] + u |dX| of dQ + dB[ids], with and without the self half as addend"""
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd.full_batch import PulledMatrix
    a, rng = _graph(name, 35)
    N = a.shape[0]
    ids = _subsets(N, rng)[sname]
    if name == 'hub' and sname == 'third':
        ids = np.union1d(ids, [7, 8, 9]).astype(np.int32)
    n = len(ids)
    A = ops.DeviceCSR.from_scipy(a, DEV, with_plan=False, with_transpose=True)
    ids_dev = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(DEV)
    scale = _scale(d, heads)
    X, H, G, add = (rng.randn(*s).astype(np.float32) for s in ((n, d), (N, d), (n, d), (n, d)))
    ld = _pitch(d, 4)                         # (16-byte rows: 602 columns need VW = 4, and the pull launches do not stage)
    if bf16:
        table = ops.history_assign(ops.history_alloc(N, d, DEV, bf16=True), _dev(H))
        tab = pr.widen_bf16(pr.round_bf16(H))
    else:
        table, tab = _pitched(H, ld), H
    for with_add in (False, True):
        blk = ops.csr_induce(A, ids, ids_dev, norm='keep')
        pm = PulledMatrix(blk, A, ids_dev, [table], [True], DEV)
        x, g = _pitched(X, ld), _pitched(G, ld)
        out, lse = pm.pull_attn_product(x, 0, scale, heads=heads)
        kw = dict(add=_pitched(add, ld), add_rows=n) if with_add else {}
        dx = pm.pull_attn_backward(x, 0, g, out, lse, scale, heads=heads, **kw).cpu().numpy()
        ref = ar.backward(a, ids, X, tab, G, scale, heads, **(dict(add=add, add_rows=n) if with_add else {}))
        bound = ref['bound_dQ'] + ref['bound_dB'][ids] + U * np.abs(ref['dX'])
        print("%s / %s / d=%d heads=%d %s add=%s: n %d" % (name, sname, d, heads, 'bf16' if bf16 else 'fp32', with_add, n))
        _within('C', out.cpu().numpy(), ref['fwd'].C, ref['fwd'].bound_C)
        _within('dX', dx, ref['dX'], bound)
        # push after pull: the table's rows of S change, the backward's result does not (it re-reads rows outside S only)
        pm.push(x, 0)
        again = pm.pull_attn_backward(x, 0, g, out, lse, scale, heads=heads, **kw).cpu().numpy()
        assert np.array_equal(_bits(again), _bits(dx)), "the backward read a pushed row"
        ops.history_assign(table, _dev(H))


# ---- 4. hygiene ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,heads", [(3, 1), (64, 4)])
def test_stored_rows_of_the_vertex_set_are_never_read(d, heads):
    """H[ids] = NaN with X finite: every result is finite and unchanged -- in-part columns never touch H"""
    a, rng = _graph('sbm', 36)
    N = a.shape[0]
    for sname, ids in _subsets(N, rng).items():
        r = Pull(a).select(ids)
        n = len(ids)
        X, H, G, add = (rng.randn(*s).astype(np.float32) for s in ((n, d), (N, d), (n, d), (n, d)))
        clean, clean16, _ = _all_forms(r, X, H, G, add, n, _scale(d, heads), heads)
        H[ids] = np.nan
        got, got16, _ = _all_forms(r, X, H, G, add, n, _scale(d, heads), heads)
        fin = all(np.isfinite(t[np.isfinite(c)]).all() for t, c in zip(got + got16, clean + clean16))
        print("%s d=%d heads=%d: finite %s" % (sname, d, heads, fin))
        for t, c in zip(got + got16, clean + clean16):
            assert np.array_equal(_bits(t), _bits(c)) and not np.isnan(t).any()


@pytest.mark.parametrize("d,heads", [(5, 1), (132, 4)])
def test_rows_without_an_in_part_entry_read_stored_rows_alone(d, heads):
    """the lose_all pattern under S = every other vertex: no selected row stores a column of S, so X is read as the queries
    only (the export has ONE fresh table, queries and in-part keys alike, so the keys cannot be poisoned on their own): the
    result is the attention over the stored rows alone -- the one-table kernel's bits on the UNMERGED table H, and the fp64
    reference with B = H"""
    from stochastic_gcn_amd import ops
    a, rng = _graph('lose_all', 37)
    N = a.shape[0]
    ids = _subsets(N, rng)['every_other']
    assert pr.block(a, ids).nnz == 0 and a[ids].nnz > 0
    r = Pull(a).select(ids)
    n = len(ids)
    scale = _scale(d, heads)
    X, H, G = (rng.randn(*s).astype(np.float32) for s in ((n, d), (N, d), (n, d)))
    ld = _pitch(d, 4)
    x, g, Hd = _pitched(X, ld), _pitched(G, ld), _pitched(H, ld)
    out, lse = r.fwd(x, Hd, scale, heads, ldc=ld)
    dq, delta = r.bwd(x, Hd, g, out, lse, scale, heads)
    o1, l1, q1 = r.one_table(x, Hd, g, scale, heads, ldc=ld)
    assert _same(out, o1) and _same(lse, l1) and _same(dq, q1)
    ref = href.backward_f64(r.sub, X, H, G, scale, heads)
    _within('C', out.cpu().numpy(), ref['fwd'].C, ref['fwd'].bound_C)
    _within('lse', lse.cpu().numpy(), ref['fwd'].lse, ref['fwd'].bound_lse)
    _within('dQ', dq.cpu().numpy(), ref['dQ'], ref['bound_dQ'])
    # and the keys' / values' half has nothing to add: the block is empty, dX is dQ
    A = ops.DeviceCSR.from_scipy(a, DEV, with_plan=False, with_transpose=True)
    blk = ops.csr_induce(A, ids, r.ids, norm='keep')
    from stochastic_gcn_amd.full_batch import PulledMatrix
    pm = PulledMatrix(blk, A, r.ids, [_dev(H)], [True], DEV)
    xc, gc = _dev(X), _dev(G)
    o2, l2 = pm.pull_attn_product(xc, 0, scale, heads=heads)
    dx = pm.pull_attn_backward(xc, 0, gc, o2, l2, scale, heads=heads)
    dq2, _ = ops.spattn_pull_bwd_q(A, r.ids, blk.map, xc, pm.tables[0], gc, o2, l2, scale, heads=heads)
    assert _same(dx, dq2)


@pytest.mark.parametrize("d,heads", [(3, 1), (8, 2), (64, 8)])
def test_an_empty_row_gives_zero_minus_infinity_and_the_addend(d, heads):
    a, rng = _graph('empty_rows', 38)
    N = a.shape[0]
    ids = _subsets(N, rng)['every_other']
    empty = np.flatnonzero(np.diff(a.indptr)[ids] == 0)
    assert 0 < empty.size < len(ids)
    r = Pull(a).select(ids)
    n = len(ids)
    X, H, G, add = (rng.randn(*s).astype(np.float32) for s in ((n, d), (N, d), (n, d), (n, d)))
    (out, lse, dq, delta), (o16, l16, q16, d16), _ = _all_forms(r, X, H, G, add, n, _scale(d, heads), heads)
    print("d=%d heads=%d: %d of %d selected rows store nothing" % (d, heads, empty.size, n))
    for o, l, q, dl in ((out, lse, dq, delta), (o16, l16, q16, d16)):
        assert not _bits(o[empty]).any(), "+0.0"
        assert np.isneginf(l.reshape(n, heads)[empty]).all()
        assert np.array_equal(_bits(q[empty]), _bits(add[empty])), "dQ of an empty row is the addend alone"
        assert not dl.reshape(n, heads)[empty].any()
        assert np.isfinite(l.reshape(n, heads)[np.setdiff1d(np.arange(n), empty)]).all()


def test_no_rows_is_no_launch():
    from stochastic_gcn_amd import ops
    a = ir.signed(ir.flat_graph(50, 3, seed=1), seed=1)
    r = Resident(a)
    r.ids = torch.empty(0, dtype=torch.int32, device=DEV)
    e = torch.empty((0, 4), device=DEV)
    for H in (torch.zeros((50, 4), device=DEV), ops.history_alloc(50, 4, DEV, bf16=True)):
        for heads in (1, 2):
            out, lse = ops.spattn_pull(r.A, r.ids, r.map, e, H, 0.5, heads=heads)
            assert tuple(out.shape) == (0, 4) and tuple(lse.shape) == ((0,) if heads == 1 else (0, 2))
            dq, delta = ops.spattn_pull_bwd_q(r.A, r.ids, r.map, e, H, e, out, lse, 0.5, heads=heads)
            assert tuple(dq.shape) == (0, 4) and delta.numel() == 0
    out, lse = ops.spattn_pull(r.A, r.ids, r.map, e, H, 0.5, want_lse=False)
    assert lse is None


def test_without_lse_the_output_is_the_same():
    from stochastic_gcn_amd import ops
    a, rng = _graph('sbm', 39)
    N = a.shape[0]
    ids = _subsets(N, rng)['third']
    r = Pull(a).select(ids)
    X, H = rng.randn(len(ids), 8).astype(np.float32), rng.randn(N, 8).astype(np.float32)
    for heads in (1, 2):
        a1, l1 = ops.spattn_pull(r.A, r.ids, r.map, _dev(X), _dev(H), 0.4, heads=heads)
        a2, l2 = ops.spattn_pull(r.A, r.ids, r.map, _dev(X), _dev(H), 0.4, heads=heads, want_lse=False)
        assert l2 is None and _same(a1, a2)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def test_a_row_too_wide_for_its_vector_width_is_refused():
    """(520, 8) on a VW = 1 pitch: 520 > 256 columns; the same on 16-byte rows runs (65 per head: VW = 1 again -- refused too)"""
    from stochastic_gcn_amd import ops
    a, rng = _graph('sbm', 40)
    N = a.shape[0]
    ids = _subsets(N, rng)['third']
    r = Pull(a).select(ids)
    n, d, heads = len(ids), 520, 8
    X, H = rng.randn(n, d).astype(np.float32), rng.randn(N, d).astype(np.float32)
    msg = r"%s: d = 520 is over the limit of 256 columns at vector width 1 \(d <= 256 \* VW"
    for ld in (_pitch(d, 1), _pitch(d, 4)):
        x, Hd = _pitched(X, ld), _pitched(H, ld)
        out = torch.full((n, d), SENTINEL, dtype=torch.float32, device=DEV)
        with pytest.raises(RuntimeError, match=msg % "spattn_pull"):
            ops.spattn_pull(r.A, r.ids, r.map, x, Hd, 0.1, out=out, heads=heads)
        assert bool((out == SENTINEL).all()), "a refused call wrote"
        lse = torch.zeros((n, heads), device=DEV)
        with pytest.raises(RuntimeError, match=msg % "spattn_pull_bwd_q"):
            ops.spattn_pull_bwd_q(r.A, r.ids, r.map, x, Hd, x, x, lse, 0.1, heads=heads)
    # 512 columns in 8 heads of 64 on 16-byte rows: VW = 4, 128 vectors -- runs
    X, H = X[:, :512].copy(), H[:, :512].copy()
    out, lse = ops.spattn_pull(r.A, r.ids, r.map, _dev(X), _dev(H), 0.1, heads=8)
    assert bool(torch.isfinite(out).all())


def test_argument_checks_through_the_raw_abi():
    """on real device operands: every refusal leaves the output untouched"""
    from stochastic_gcn_amd import _ffi, ops
    a, rng = _graph('sbm', 41)
    N = a.shape[0]
    ids = _subsets(N, rng)['third']
    r = Pull(a).select(ids)
    n, d = len(ids), 8
    x, H = _dev(rng.randn(n, d)), _dev(rng.randn(N, d))
    Hb = ops.history_alloc(N, d, DEV, bf16=True)
    out = torch.full((n, d), SENTINEL, dtype=torch.float32, device=DEV)
    lse = torch.full((n,), SENTINEL, dtype=torch.float32, device=DEV)
    P = lambda t: t.data_ptr()

    def fwd(fn=_ffi.lib.sgcn_spattn_pull_f32, n_=n, N_=N, d_=d, heads=1, ldx=d, Ht=H, ldh=d, scale=0.5, ldc=d, ids_=r.ids):
        return fn(P(r.A.rowptr), P(r.A.col), P(ids_) if ids_ is not None else None, n_, N_, P(r.map), d_, heads, P(x), ldx, P(Ht),
                  ldh, scale, P(out), ldc, P(lse), ops._stream())

    def err():
        return _ffi.lib.sgcn_last_error() or b""
    assert fwd(n_=-1) == -1 and b"negative size" in err()
    assert fwd(n_=N + 1) == -1 and b"rows cannot be unique" in err()
    assert fwd(d_=0) == -1 and b"d must be positive" in err()
    assert fwd(heads=3) == -1 and b"heads must be one of 1/2/4/8" in err()
    assert fwd(d_=6, heads=4) == -1 and b"not a multiple of heads" in err()
    assert fwd(ldx=d - 1) == -1 and b"leading dimension smaller than d" in err()
    assert fwd(ids_=None) == -1 and b"null operand" in err()
    assert fwd(scale=float('nan')) == -1 and b"scale must be finite" in err()
    h16 = _ffi.lib.sgcn_spattn_pull_h16
    assert fwd(fn=h16, Ht=Hb, ldh=12) == -1 and b"ldh % 8 == 0" in err()
    assert fwd(fn=h16, Ht=Hb[:, 4:], ldh=8) == -1 and b"16-byte aligned" in err()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((lse == SENTINEL).all()), "a refused call wrote"
    assert fwd() == 0 and fwd(fn=h16, Ht=Hb, ldh=int(Hb.stride(0))) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    # the addend of bwd_q
    g, dq, delta = _dev(rng.randn(n, d)), torch.full((n, d), SENTINEL, device=DEV), torch.full((n,), SENTINEL, device=DEV)

    def bwd(ldadd=d, add_rows=n):
        return _ffi.lib.sgcn_spattn_pull_bwd_q_f32(P(r.A.rowptr), P(r.A.col), P(r.ids), n, N, P(r.map), d, 1, P(x), d, P(H), d, 0.5,
                                                   P(g), d, P(out), d, P(lse), P(delta), P(dq), d, P(g), ldadd, add_rows,
                                                   ops._stream())
    assert bwd(ldadd=d - 1) == -1 and b"bad addend" in err()
    assert bwd(add_rows=n + 1) == -1 and b"bad addend" in err()
    torch.cuda.synchronize()
    assert bool((dq == SENTINEL).all()) and bool((delta == SENTINEL).all())
    assert bwd() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dq).all())
