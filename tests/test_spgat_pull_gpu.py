"""GPU tests of ops.spgat_pull / ops.spgat_pull_bwd_u / ops.spgat_pull_bwd_v (sgcn_spgat_pull.hip): the two-table attention
with learned additive scores of --full_batch_part_pull_gat, on the patterns and vertex sets of the induce tests (a 330-entry
row: five chunks and a tail at 64 lanes; 64- and 65-entry rows; rows that store nothing; rows without an in-part entry;
S = everything, S = one vertex), at (d, heads) in {(1,1), (3,1), (5,1), (8,2), (64,4), (64,8), (132,4), (602,1)}, on pitches
that force every vector width, at slopes 0.2, 0 and 1.

  1. bit identity with the one-table kernels, a condition: with Z = T with the rows of S replaced by X, V_m = VH with the rows
     of S replaced by V (on the device) and A_sub = the rows ids of the adjacency without a plan, the pull launches give the
     bits of ops.spgat(A_sub, Z, U, V_m) and of the delta and dU of ops.spgat_bwd.
  2. the fp64 reference of tests/part_pull_gat_ref.py within spgat_ref's DERIVED bounds: C, lse, delta, dU, and the composed dX
     and da of PulledMatrix.pull_gat_backward within the bounds summed term by term (part_pull_gat_ref.backward).  Nothing is
     fitted.
  3. the bfloat16 form gives the fp32 form's bits on the widened table, at every shape (inside every launch helper).
  4. hygiene: two runs give equal bits, nothing is written past d or past heads, NaN in T[ids] and VH[ids] changes nothing, rows
     without an in-part entry read stored rows and scores alone, an empty row gives +0.0 / -inf with dU = 0, n == 0 is no launch.
  5. refusals.
N <= 400 throughout; every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import induce_ref as ir
import part_history_ref as pr
import part_pull_gat_ref as gr
import spgat_ref
from test_induce_gpu import PATTERNS, _subsets
from test_spattn_pull_gpu import _graph, _hub_exact
from test_spmm_pull_gpu import SENTINEL, Resident, _bits, _h16, _pitch, _pitched

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SHAPES = ((1, 1), (3, 1), (5, 1), (8, 2), (64, 4), (64, 8), (132, 4), (602, 1))
# two shapes per vertex set, every shape used, on every pattern
SHAPES_OF = {'all': ((1, 1), (64, 4)), 'one': ((3, 1), (602, 1)), 'every_other': ((8, 2), (132, 4)), 'third': ((5, 1), (64, 8))}
SLOPES = (0.2, 0.0, 1.0)
U_ = spgat_ref.U_


def _slope(d, heads):
    return SLOPES[(d + heads) % 3]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)


def _same(x, y):
    return np.array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy()))


def _tables(rng, n, N, heads):
    """the fresh scores as the two halves of ONE (n, 2 heads) table (pitch 2 heads, as ops.gat_scores returns them) and the
    stored scores on a pitch of heads + 1: (S device, VH device view, U, V, VH as NumPy)"""
    S = rng.randn(n, 2 * heads).astype(np.float32)
    VH = rng.randn(N, heads).astype(np.float32)
    return _dev(S), _pitched(VH, heads + 1), S[:, :heads], S[:, heads:], VH


class GatPull(Resident):
    """the resident matrix, one vertex set, and the launches of both kinds into sentinel-filled tables"""

    def select(self, ids):
        from stochastic_gcn_amd import ops
        super(GatPull, self).select(ids)
        self.ids_np = np.asarray(ids, np.int64)
        self.sub = self.a[self.ids_np].tocsr()
        self.sub.sort_indices()
        self.A_sub = ops.DeviceCSR.from_scipy(self.sub, DEV, with_plan=False, with_transpose=True)
        self.idx = torch.from_numpy(self.ids_np).to(DEV)
        return self

    def merged(self, x, T32dev):
        """Z: the fp32 table ``T32dev`` (a pitched view) with the rows of S replaced by x, on the same pitch"""
        pitch = int(T32dev.stride(0)) if T32dev.shape[0] > 1 else int(T32dev.shape[1])
        Z = torch.zeros((T32dev.shape[0], pitch), dtype=torch.float32, device=DEV)[:, :T32dev.shape[1]]
        Z.copy_(T32dev)
        Z[self.idx] = x
        return Z

    def fwd(self, x, T, S, VH, slope, heads, ldc=None):
        """(out, lse), twice (equal bits), into a sentinel table of pitch ldc (nothing past d)"""
        from stochastic_gcn_amd import ops
        n, d = int(x.shape[0]), int(x.shape[1])
        res = []
        for _ in range(2):
            full = torch.full((max(n, 1), ldc or _pitch(d, 4) + 4), SENTINEL, dtype=torch.float32, device=DEV)[:n]
            out, lse = ops.spgat_pull(self.A, self.ids, self.map, x, T, S[:, :heads], S[:, heads:], VH, slope, out=full[:, :d],
                                      heads=heads)
            assert out.data_ptr() == full.data_ptr() and tuple(lse.shape) == (n, heads)
            assert bool((full[:, d:] == SENTINEL).all()), "written past d"
            res.append((out, lse))
        assert _same(res[0][0], res[1][0]) and _same(res[0][1], res[1][1]), "two runs differ"
        return res[0]

    def bwd(self, x, T, S, VH, g, out, lse, slope, heads):
        from stochastic_gcn_amd import ops
        res = [ops.spgat_pull_bwd_u(self.A, self.ids, self.map, x, T, S[:, :heads], S[:, heads:], VH, g, out, lse, slope, heads=heads)
               for _ in range(2)]
        for k in (0, 1):
            assert tuple(res[0][k].shape) == (int(x.shape[0]), heads) and _same(res[0][k], res[1][k]), "two runs differ"
        return res[0]

    def one_table(self, x, Z, S, Vm, g, slope, heads, ldc=None):
        """(out, lse, dU, delta) of the one-table kernels without a plan on (A_sub, Z, U, V_m)"""
        from stochastic_gcn_amd import ops
        n, d = int(x.shape[0]), int(x.shape[1])
        full = torch.full((max(n, 1), ldc or _pitch(d, 4) + 4), SENTINEL, dtype=torch.float32, device=DEV)[:n]
        out, lse = ops.spgat(self.A_sub, Z, S[:, :heads], Vm, slope=slope, out=full[:, :d], heads=heads)
        _, dU, _, delta = ops.spgat_bwd(self.A_sub, self.A_sub.transpose, Z, S[:, :heads], Vm, g, out, lse, slope=slope, heads=heads)
        return out, lse, dU, delta

    def merged_scores(self, S, VH, heads):
        Vm = VH.clone()
        Vm[self.idx] = S[:, heads:]
        return Vm


def _all_forms(r, X, T32, G, S, VH, slope, heads, ld=None, ldh=None):
    """Runs the fp32 form on T32 and the bfloat16 form on T32 rounded, each against the one-table kernels on its merged tables
    (test 1) and the bfloat16 form against the fp32 form on the widened table (test 3).  X, G on pitch ``ld`` (default: 16-byte
    rows), the fp32 row table on ``ldh``.  Returns the fp32 form's (out, lse, dU, delta) and the bfloat16 form's, as NumPy
    arrays, and the widened table."""
    d = X.shape[1]
    ld = ld or _pitch(d, 4)
    x, g = _pitched(X, ld), _pitched(G, ld)
    Td = _pitched(T32, ldh or ld)
    ldc = ld + 4                              # (the same alignment class, and room for the sentinel)
    Vm = r.merged_scores(S, VH, heads)
    out, lse = r.fwd(x, Td, S, VH, slope, heads, ldc=ldc)
    dU, delta = r.bwd(x, Td, S, VH, g, out, lse, slope, heads)
    o1, l1, u1, d1 = r.one_table(x, r.merged(x, Td), S, Vm, g, slope, heads, ldc=ldc)
    assert _same(out, o1), "forward: not the one-table kernel's bits"
    assert _same(lse, l1), "lse: not the one-table kernel's bits"
    assert _same(delta, d1), "delta: not the one-table kernel's bits"
    assert _same(dU, u1), "dU: not the one-table kernel's bits"
    Tb, Tw, wide = _h16(T32)
    out16, lse16 = r.fwd(x, Tb, S, VH, slope, heads, ldc=ldc)
    dU16, delta16 = r.bwd(x, Tb, S, VH, g, out16, lse16, slope, heads)
    outw, lsew = r.fwd(x, Tw, S, VH, slope, heads, ldc=ldc)
    dUw, deltaw = r.bwd(x, Tw, S, VH, g, outw, lsew, slope, heads)
    assert _same(out16, outw) and _same(lse16, lsew), "the bfloat16 form is not the fp32 form on the widened table"
    assert _same(dU16, dUw) and _same(delta16, deltaw), "the bfloat16 bwd_u is not the fp32 form on the widened table"
    o2, l2, u2, d2 = r.one_table(x, r.merged(x, Tw), S, Vm, g, slope, heads, ldc=ldc)
    assert _same(out16, o2) and _same(lse16, l2) and _same(dU16, u2) and _same(delta16, d2), "bfloat16 form: not the one-table bits"
    f32 = tuple(t.cpu().numpy() for t in (out, lse, dU, delta))
    h16 = tuple(t.cpu().numpy() for t in (out16, lse16, dU16, delta16))
    return f32, h16, wide


def _within(what, got, want, bound):
    got, want = np.asarray(got, np.float64).reshape(np.shape(want)), np.asarray(want, np.float64)
    both_inf = np.isneginf(got) & np.isneginf(want)
    err = np.where(both_inf, 0.0, np.abs(got - np.where(both_inf, 0.0, want)))
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(err > 0, err / bound, 0.0)
    print("        %-6s worst error %.3e = %.3f of its bound" % (what, float(err.max(initial=0.0)), float(frac.max(initial=0.0))))
    assert np.all(err <= bound), what


def _check_fp64(a, ids, X, tab, Un, Vn, VHn, G, slope, heads, got):
    """test 2 for one launch pair: ``got`` = (out, lse, dU, delta) against the reference on the row table ``tab``"""
    ref = gr.backward_tables(a, ids, X, tab, Un, Vn, VHn, G, slope, heads)
    f = ref['fwd']
    _within('C', got[0], f.C, f.bound_C)
    _within('lse', got[1], f.lse, f.bound_lse)
    _within('delta', got[3], ref['delta'], ref['bound_delta'])
    _within('dU', got[2], ref['dU'], ref['bound_dU'])
    return ref


# ---- 1 + 3 (+ 2 on the fp32 form): every pattern, every vertex set ---------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_bits_of_the_one_table_kernels_and_the_fp64_reference(name):
    a, rng = _graph(name, 31)
    N = a.shape[0]
    r = GatPull(a)
    for sname, ids in _subsets(N, rng).items():
        r.select(ids)
        n = len(ids)
        for d, heads in SHAPES_OF[sname]:
            slope = _slope(d, heads)
            X, T, G = (rng.randn(*s).astype(np.float32) for s in ((n, d), (N, d), (n, d)))
            S, VH, Un, Vn, VHn = _tables(rng, n, N, heads)
            lens = np.diff(a.indptr)[ids]
            inside = pr.position_map(N, ids)[r.sub.indices] >= 0
            print("%s / %s / d=%d heads=%d slope=%g: n %d, longest row %d, empty rows %d, %d of %d entries in-part"
                  % (name, sname, d, heads, slope, n, int(lens.max()), int(np.sum(lens == 0)), int(inside.sum()), inside.size))
            f32, h16, wide = _all_forms(r, X, T, G, S, VH, slope, heads)
            _check_fp64(a, ids, X, T, Un, Vn, VHn, G, slope, heads, f32)
            if d in (5, 64):
                _check_fp64(a, ids, X, wide, Un, Vn, VHn, G, slope, heads, h16)


# ---- every (d, heads) on every vector width -------------------------------------------------------------------------------
@pytest.mark.parametrize("vw", [4, 2, 1])
@pytest.mark.parametrize("d,heads", SHAPES)
def test_every_shape_on_every_vector_width(d, heads, vw):
    """the hub graph (a row of 330 and more entries, one of exactly 64 and one of exactly 65) under S = a third plus the long
    rows: X, G, C and the fp32 row table on pitches that allow exactly ``vw`` elements per vector, every slope.  602 columns need
    VW = 4 (d <= 256 * VW): on the narrower pitches the launch is refused with the width message"""
    from stochastic_gcn_amd import ops
    a, rng = _hub_exact(33)
    N = a.shape[0]
    ids = np.union1d(_subsets(N, rng)['third'], [7, 8, 9]).astype(np.int32)
    r = GatPull(a).select(ids)
    n = len(ids)
    X, T, G = (rng.randn(*s).astype(np.float32) for s in ((n, d), (N, d), (n, d)))
    S, VH, Un, Vn, VHn = _tables(rng, n, N, heads)
    ld = _pitch(d, vw)
    eff = ops.attn_vw(d, _pitched(X, ld), heads=heads)
    print("d=%d heads=%d vw=%d pitch %d (effective VW %d): n %d, rows of %s entries"
          % (d, heads, vw, ld, eff, n, sorted(set(np.diff(a.indptr)[[7, 8, 9]]))))
    assert eff <= vw
    if d > 256 * eff:
        with pytest.raises(RuntimeError, match=r"spgat_pull: d = %d is over the limit of %d columns at vector width %d" % (d, 256 * eff, eff)):
            ops.spgat_pull(r.A, r.ids, r.map, _pitched(X, ld), _pitched(T, ld), S[:, :heads], S[:, heads:], VH, 0.2, heads=heads,
                           out=_pitched(X, ld).clone())
        return
    for slope in SLOPES:
        f32, h16, wide = _all_forms(r, X, T, G, S, VH, slope, heads, ld=ld)
        _check_fp64(a, ids, X, T, Un, Vn, VHn, G, slope, heads, f32)
        _check_fp64(a, ids, X, wide, Un, Vn, VHn, G, slope, heads, h16)


# ---- 2. the composed gradient --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("name,sname,d,heads", [('hub', 'third', 64, 4), ('sbm', 'every_other', 8, 2), ('empty_rows', 'third', 5, 1),
                                                ('lose_all', 'every_other', 3, 1), ('sbm', 'all', 132, 4), ('hub', 'one', 602, 1)])
def test_pulled_matrix_backward_composes_the_three_launches(name, sname, d, heads, bf16):
    """PulledMatrix.pull_gat_product / pull_gat_backward over the block ops.csr_induce cut: dX and da within the summed bounds
    of part_pull_gat_ref.backward -- the reference takes the score table the device's own launch produced, as the kernels take
    theirs --, with and without the self half as addend, with and without dX"""
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
    slope = _slope(d, heads)
    X, T, G, add = (rng.randn(*s).astype(np.float32) for s in ((n, d), (N, d), (n, d), (n, d)))
    avec = (rng.randn(2, d) * (2.0 / np.sqrt(d // heads))).astype(np.float32)
    VHn = rng.randn(N, heads).astype(np.float32)
    ld = _pitch(d, 4)                         # (16-byte rows: 602 columns need VW = 4, and the pull launches do not stage)
    if bf16:
        table = ops.history_assign(ops.history_alloc(N, d, DEV, bf16=True), _dev(T))
        tab = pr.widen_bf16(pr.round_bf16(T))
    else:
        table, tab = _pitched(T, ld), T
    for with_add in (False, True):
        blk = ops.csr_induce(A, ids, ids_dev, norm='keep')
        scores = _dev(VHn)
        pm = PulledMatrix(blk, A, ids_dev, [table], [True], DEV, scores=[scores])
        x, g, av = _pitched(X, ld), _pitched(G, ld), _dev(avec)
        out, lse, S = pm.pull_gat_product(x, av, 0, slope, heads=heads)
        assert tuple(S.shape) == (n, 2 * heads) and _same(S, ops.gat_scores(x, av, heads=heads))
        kw = dict(add=_pitched(add, ld), add_rows=n) if with_add else {}
        dx, da = pm.pull_gat_backward(x, av, S, 0, g, out, lse, slope, heads=heads, **kw)
        dx, da = dx.cpu().numpy(), da.cpu().numpy()
        ref = gr.backward(a, ids, X, tab, VHn, avec, G, slope, heads, S=S.cpu().numpy(), values_only=False,
                          **(dict(add=add, add_rows=n) if with_add else {}))
        print("%s / %s / d=%d heads=%d slope=%g %s add=%s: n %d" % (name, sname, d, heads, slope, 'bf16' if bf16 else 'fp32', with_add, n))
        _within('C', out.cpu().numpy(), ref['fwd'].C, ref['fwd'].bound_C)
        _within('dX', dx, ref['dX'], ref['bound_dX'])
        _within('da', da, ref['da'], ref['bound_da'])
        none, da2 = pm.pull_gat_backward(x, av, S, 0, g, out, lse, slope, heads=heads, need_dx=False, **kw)
        assert none is None and np.array_equal(_bits(da2.cpu().numpy()), _bits(da)), "need_dx=False changed da"
        # push after pull: the tables' rows of S change, the backward's result does not (it re-reads rows outside S only)
        pm.push(x, 0)
        pm.push_scores(S, 0)
        got = scores.cpu().numpy()
        assert np.array_equal(_bits(got[ids]), _bits(S[:, heads:].cpu().numpy())), "the pushed scores are not V"
        rest = np.setdiff1d(np.arange(N), ids)
        assert np.array_equal(_bits(got[rest]), _bits(VHn[rest])), "a push wrote outside S"
        dx2, da3 = pm.pull_gat_backward(x, av, S, 0, g, out, lse, slope, heads=heads, **kw)
        assert np.array_equal(_bits(dx2.cpu().numpy()), _bits(dx)) and np.array_equal(_bits(da3.cpu().numpy()), _bits(da)), \
            "the backward read a pushed row or score"
        ops.history_assign(table, _dev(T))


# ---- 4. hygiene ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,heads", [(3, 1), (64, 4)])
def test_stored_rows_and_scores_of_the_vertex_set_are_never_read(d, heads):
    """T[ids] = NaN and VH[ids] = NaN with X, U, V finite: every result is finite and unchanged"""
    a, rng = _graph('sbm', 36)
    N = a.shape[0]
    for sname, ids in _subsets(N, rng).items():
        r = GatPull(a).select(ids)
        n = len(ids)
        X, T, G = (rng.randn(*s).astype(np.float32) for s in ((n, d), (N, d), (n, d)))
        S, VH, Un, Vn, VHn = _tables(rng, n, N, heads)
        clean, clean16, _ = _all_forms(r, X, T, G, S, VH, 0.2, heads)
        T[ids] = np.nan
        VH[r.idx] = float('nan')
        got, got16, _ = _all_forms(r, X, T, G, S, VH, 0.2, heads)
        print("%s d=%d heads=%d: NaN in %d stored rows and scores" % (sname, d, heads, n))
        for t, c in zip(got + got16, clean + clean16):
            assert np.array_equal(_bits(t), _bits(c)) and not np.isnan(t).any()


@pytest.mark.parametrize("d,heads", [(5, 1), (132, 4)])
def test_rows_without_an_in_part_entry_read_stored_rows_and_scores_alone(d, heads):
    """the lose_all pattern under S = every other vertex: no selected row stores a column of S, so X and V are never gathered
    (V = NaN changes nothing): the result is the one-table kernel's bits on the UNMERGED tables, and the fp64 reference's"""
    a, rng = _graph('lose_all', 37)
    N = a.shape[0]
    ids = _subsets(N, rng)['every_other']
    assert pr.block(a, ids).nnz == 0 and a[ids].nnz > 0
    r = GatPull(a).select(ids)
    n = len(ids)
    X, T, G = (rng.randn(*s).astype(np.float32) for s in ((n, d), (N, d), (n, d)))
    S, VH, Un, Vn, VHn = _tables(rng, n, N, heads)
    ld = _pitch(d, 4)
    x, g, Td = _pitched(X, ld), _pitched(G, ld), _pitched(T, ld)
    out, lse = r.fwd(x, Td, S, VH, 0.2, heads, ldc=ld)
    dU, delta = r.bwd(x, Td, S, VH, g, out, lse, 0.2, heads)
    o1, l1, u1, d1 = r.one_table(x, Td, S, VH, g, 0.2, heads, ldc=ld)
    assert _same(out, o1) and _same(lse, l1) and _same(dU, u1) and _same(delta, d1)
    ref = spgat_ref.backward_f64(r.sub, Un, VHn, T, G, 0.2, heads)
    _within('C', out.cpu().numpy(), ref['fwd'].C, ref['fwd'].bound_C)
    _within('lse', lse.cpu().numpy(), ref['fwd'].lse, ref['fwd'].bound_lse)
    _within('dU', dU.cpu().numpy(), ref['dU'], ref['bound_dU'])
    S2 = S.clone()
    S2[:, heads:] = float('nan')
    o2, l2 = r.fwd(x, Td, S2, VH, 0.2, heads, ldc=ld)
    u2, d2 = r.bwd(x, Td, S2, VH, g, o2, l2, 0.2, heads)
    assert _same(o2, out) and _same(l2, lse) and _same(u2, dU) and _same(d2, delta), "a fresh destination score was read"


@pytest.mark.parametrize("d,heads", [(3, 1), (8, 2), (64, 8)])
def test_an_empty_row_gives_zero_minus_infinity_and_no_gradient(d, heads):
    a, rng = _graph('empty_rows', 38)
    N = a.shape[0]
    ids = _subsets(N, rng)['every_other']
    empty = np.flatnonzero(np.diff(a.indptr)[ids] == 0)
    assert 0 < empty.size < len(ids)
    r = GatPull(a).select(ids)
    n = len(ids)
    X, T, G = (rng.randn(*s).astype(np.float32) for s in ((n, d), (N, d), (n, d)))
    S, VH, Un, Vn, VHn = _tables(rng, n, N, heads)
    (out, lse, dU, delta), (o16, l16, u16, d16), _ = _all_forms(r, X, T, G, S, VH, 0.2, heads)
    print("d=%d heads=%d: %d of %d selected rows store nothing" % (d, heads, empty.size, n))
    for o, l, u, dl in ((out, lse, dU, delta), (o16, l16, u16, d16)):
        assert not _bits(o[empty]).any(), "+0.0"
        assert np.isneginf(l[empty]).all()
        assert not u[empty].any() and not dl[empty].any(), "dU = 0 and delta = 0"
        assert np.isfinite(l[np.setdiff1d(np.arange(n), empty)]).all()


def test_nothing_is_written_past_heads():
    """through the raw ABI: lse, delta and dU are n x heads contiguous; the sentinel behind them stays"""
    from stochastic_gcn_amd import _ffi, ops
    a, rng = _graph('sbm', 42)
    N = a.shape[0]
    ids = _subsets(N, rng)['third']
    r = GatPull(a).select(ids)
    n, d, heads = len(ids), 8, 2
    x, T, g = _dev(rng.randn(n, d)), _dev(rng.randn(N, d)), _dev(rng.randn(n, d))
    S, VH, _, _, _ = _tables(rng, n, N, heads)
    P = lambda t: t.data_ptr()
    out = torch.full((n, d), SENTINEL, device=DEV)
    lse, delta, dU = (torch.full((n * heads + 16,), SENTINEL, device=DEV) for _ in range(3))
    common = (P(r.A.rowptr), P(r.A.col), P(r.ids), n, N, P(r.map), d, heads, P(x), d, P(T), d, P(S), 2 * heads, P(S) + 4 * heads,
              2 * heads, P(VH), int(VH.stride(0)), 0.2)
    assert _ffi.lib.sgcn_spgat_pull_f32(*common, P(out), d, P(lse), ops._stream()) == 0
    assert _ffi.lib.sgcn_spgat_pull_bwd_u_f32(*common, P(g), d, P(out), d, P(lse), P(delta), P(dU), ops._stream()) == 0
    torch.cuda.synchronize()
    for t in (lse, delta, dU):
        assert bool((t[n * heads:] == SENTINEL).all()) and bool((t[:n * heads] != SENTINEL).all())
    o2, l2 = ops.spgat_pull(r.A, r.ids, r.map, x, T, S[:, :heads], S[:, heads:], VH, 0.2, heads=heads)
    assert _same(o2, out) and _same(l2.reshape(-1), lse[:n * heads])


def test_no_rows_is_no_launch():
    from stochastic_gcn_amd import ops
    a = ir.signed(ir.flat_graph(50, 3, seed=1), seed=1)
    r = Resident(a)
    r.ids = torch.empty(0, dtype=torch.int32, device=DEV)
    e = torch.empty((0, 4), device=DEV)
    for T in (torch.zeros((50, 4), device=DEV), ops.history_alloc(50, 4, DEV, bf16=True)):
        for heads in (1, 2):
            s, vh = torch.empty((0, heads), device=DEV), torch.zeros((50, heads), device=DEV)
            out, lse = ops.spgat_pull(r.A, r.ids, r.map, e, T, s, s, vh, 0.2, heads=heads)
            assert tuple(out.shape) == (0, 4) and tuple(lse.shape) == (0, heads)
            dU, delta = ops.spgat_pull_bwd_u(r.A, r.ids, r.map, e, T, s, s, vh, e, out, lse, 0.2, heads=heads)
            assert tuple(dU.shape) == (0, heads) and tuple(delta.shape) == (0, heads)
    out, lse = ops.spgat_pull(r.A, r.ids, r.map, e, T, s, s, vh, 0.2, heads=2, want_lse=False)
    assert lse is None


def test_without_lse_the_output_is_the_same():
    from stochastic_gcn_amd import ops
    a, rng = _graph('sbm', 39)
    N = a.shape[0]
    ids = _subsets(N, rng)['third']
    r = GatPull(a).select(ids)
    X, T = rng.randn(len(ids), 8).astype(np.float32), rng.randn(N, 8).astype(np.float32)
    for heads in (1, 2):
        S, VH, _, _, _ = _tables(rng, len(ids), N, heads)
        a1, l1 = ops.spgat_pull(r.A, r.ids, r.map, _dev(X), _dev(T), S[:, :heads], S[:, heads:], VH, 0.2, heads=heads)
        a2, l2 = ops.spgat_pull(r.A, r.ids, r.map, _dev(X), _dev(T), S[:, :heads], S[:, heads:], VH, 0.2, heads=heads, want_lse=False)
        assert l2 is None and _same(a1, a2)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_through_ops():
    from stochastic_gcn_amd import ops
    a, rng = _graph('sbm', 40)
    N = a.shape[0]
    ids = _subsets(N, rng)['third']
    r = GatPull(a).select(ids)
    n, d, heads = len(ids), 520, 8
    X, T = rng.randn(n, d).astype(np.float32), rng.randn(N, d).astype(np.float32)
    S, VH, _, _, _ = _tables(rng, n, N, heads)
    U, V = S[:, :heads], S[:, heads:]
    msg = r"%s: d = 520 is over the limit of 256 columns at vector width 1 \(d <= 256 \* VW"
    for ld in (_pitch(d, 1), _pitch(d, 4)):            # (65 columns per head: VW = 1 on 16-byte rows too)
        x, Td = _pitched(X, ld), _pitched(T, ld)
        out = torch.full((n, d), SENTINEL, dtype=torch.float32, device=DEV)
        with pytest.raises(RuntimeError, match=msg % "spgat_pull"):
            ops.spgat_pull(r.A, r.ids, r.map, x, Td, U, V, VH, 0.2, out=out, heads=heads)
        assert bool((out == SENTINEL).all()), "a refused call wrote"
        lse = torch.zeros((n, heads), device=DEV)
        with pytest.raises(RuntimeError, match=msg % "spgat_pull_bwd_u"):
            ops.spgat_pull_bwd_u(r.A, r.ids, r.map, x, Td, U, V, VH, x, x, lse, 0.2, heads=heads)
    # 512 columns in 8 heads of 64 on 16-byte rows: VW = 4, 128 vectors -- runs
    x, Td = _dev(X[:, :512].copy()), _dev(T[:, :512].copy())
    out, lse = ops.spgat_pull(r.A, r.ids, r.map, x, Td, U, V, VH, 0.2, heads=8)
    assert bool(torch.isfinite(out).all())
    # the operand checks of ops: the slope, the score tables' shapes, the row tables', lse's
    for slope in (-0.1, 1.1, float('nan')):
        with pytest.raises(ValueError, match=r"slope must lie in \[0, 1\]"):
            ops.spgat_pull(r.A, r.ids, r.map, x, Td, U, V, VH, slope, heads=8)
    with pytest.raises(ValueError, match=r"u has shape .* need \(>=%d, 8\)" % n):
        ops.spgat_pull(r.A, r.ids, r.map, x, Td, U[:, :4], V, VH, 0.2, heads=8)
    with pytest.raises(ValueError, match=r"v has shape .* need \(>=%d, 8\)" % n):
        ops.spgat_pull(r.A, r.ids, r.map, x, Td, U, V[:n - 1], VH, 0.2, heads=8)
    with pytest.raises(ValueError, match=r"vh has shape .* need \(>=%d, 8\)" % N):
        ops.spgat_pull(r.A, r.ids, r.map, x, Td, U, V, VH[:N - 1], 0.2, heads=8)
    with pytest.raises(ValueError, match="H has shape"):
        ops.spgat_pull(r.A, r.ids, r.map, x, Td[:N - 1], U, V, VH, 0.2, heads=8)
    with pytest.raises(ValueError, match="x has %d rows" % (n - 1)):
        ops.spgat_pull(r.A, r.ids, r.map, x[:n - 1], Td, U, V, VH, 0.2, heads=8)
    with pytest.raises(ValueError, match="lse must be what spgat_pull returned"):
        ops.spgat_pull_bwd_u(r.A, r.ids, r.map, x, Td, U, V, VH, x, out, lse.reshape(-1), 0.2, heads=8)
    with pytest.raises(ValueError, match="At must be the square transposed block"):
        ops.spgat_pull_bwd_v(r.A_sub.transpose, x, U, V, x, lse, lse, 0.2, heads=8)
    # a PulledMatrix without score tables names the flag
    from stochastic_gcn_amd.full_batch import PulledMatrix
    A = ops.DeviceCSR.from_scipy(a, DEV, with_plan=False, with_transpose=True)
    pm = PulledMatrix(ops.csr_induce(A, ids, r.ids, norm='keep'), A, r.ids, [Td], [True], DEV)
    with pytest.raises(RuntimeError, match="carries no score tables"):
        pm.pull_gat_product(x, _dev(rng.randn(2, 512)), 0, 0.2, heads=8)
    with pytest.raises(ValueError, match="one score table per history table"):
        PulledMatrix(ops.csr_induce(A, ids, r.ids, norm='keep'), A, r.ids, [Td], [True], DEV, scores=[])
