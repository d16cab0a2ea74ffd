"""GPU tests of ops.spmax_pull (sgcn_spmax_pull.hip): the two-table element-wise maximum of --full_batch_part_pull_max.  The
forward has no arithmetic, so every check is BIT FOR BIT: against ops.spmax without a plan on the rows ids of the matrix and
the merged table (H with the rows ids replaced by X) -- values and decoded winners -- and against the exact reference of
tests/part_pull_max_ref.py, on the nine patterns and four vertex sets of tests/test_spmm_pull_gpu.py (a 330-entry row: five
chunks and a tail at 64 lanes; rows that store nothing; rows without an in-part entry; S = everything: rows without an
out-of-part entry; S = one vertex), at d in {1, 3, 4, 5, 64, 132, 602} and on pitches that force every vector width for X, H, C
and arg independently.  Inputs from a coarse grid make ties across the two tables and between -0.0 and +0.0 occur (asserted
on the CPU).  The bfloat16-table form must give the fp32 form's bits and winners on the widened table; two runs give equal
bits; stored rows of S are never read (+inf there changes nothing); nothing is written past column d or past row n;
``want_arg=False`` gives the same values.  The backward is the EXISTING ops.spmax_bwd over the block's transpose with the
pull's arg: bit for bit the reference's scatter on dyadic gradients, within sparse_cases.fp64_bound's row bound on real
ones.  N <= 400 throughout; every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import induce_ref as ir
import part_history_ref as pr
import part_pull_max_ref as xr
import sparse_cases as sc
import spmax_ref
from test_induce_gpu import PATTERNS, _subsets
from test_spmm_pull_gpu import SENTINEL, WIDTHS, WIDTHS_OF, Resident, _bits, _h16, _pitch, _pitched

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ARG_SENTINEL = -777777


def _grid(rng, shape):
    """a coarse grid with both zeros; the right half of the columns holds nothing above zero, so that zeros win there"""
    v = rng.randint(-2, 3, shape).astype(np.float32) / 2.0
    half = shape[1] // 2
    v[:, half:] = np.float32(0.0) - np.abs(v[:, half:])
    v[(v == 0) & (rng.rand(*shape) < 0.5)] = -0.0
    return v


def _pull(r, x, H, ldc=None, ldarg=None, want_arg=True, guard_rows=2):
    """(C, arg, padded C, padded arg) of one launch into sentinel-filled tables of pitch ldc / ldarg with ``guard_rows`` rows
    behind the n the launch may write"""
    from stochastic_gcn_amd import ops
    n, d = int(x.shape[0]), int(x.shape[1])
    full = torch.full((n + guard_rows, ldc or d), SENTINEL, dtype=torch.float32, device=DEV)
    afull = torch.full((n + guard_rows, ldarg or d), ARG_SENTINEL, dtype=torch.int32, device=DEV)
    out, arg = ops.spmax_pull(r.A, r.ids, r.map, x, H, out=full[:n, :d], want_arg=want_arg, arg=afull[:n, :d] if want_arg else None)
    assert out.data_ptr() == full.data_ptr() and (arg is None) == (not want_arg)
    if want_arg:
        assert arg.data_ptr() == afull.data_ptr()
    full, afull = full.cpu().numpy(), afull.cpu().numpy()
    assert np.all(full[:n, d:] == SENTINEL) and np.all(full[n:] == SENTINEL), "C written past column d or past row n"
    assert np.all(afull[:n, d:] == ARG_SENTINEL) and np.all(afull[n:] == ARG_SENTINEL), "arg written past column d or past row n"
    if not want_arg:
        assert np.all(afull == ARG_SENTINEL)
    return full[:n, :d].copy(), (afull[:n, :d].copy() if want_arg else None)


def _one_table(a, ids, Z):
    """(C, arg as global columns) of ops.spmax WITHOUT a plan on the rows ids of ``a`` and the merged table"""
    from stochastic_gcn_amd import ops
    sub = a[np.asarray(ids, np.int64)].tocsr()
    sub.sort_indices()
    S = ops.DeviceCSR.from_scipy(sub, DEV, with_plan=False)
    assert S.plan is None
    C, arg = ops.spmax(S, torch.from_numpy(np.ascontiguousarray(Z, np.float32)).to(DEV))
    return C.cpu().numpy(), arg.cpu().numpy()


def _check(r, a, ids, X, H32, pitches=(4, 4, 4, 4), what=""):
    """one shape, every property of the forward; returns the fp32 form's (C, arg)"""
    n, d = X.shape
    N = a.shape[0]
    px, ph, pc_, pa = (_pitch(d, v) for v in pitches)
    x = _pitched(X, px)
    got, arg = _pull(r, x, _pitched(H32, ph), ldc=pc_, ldarg=pa)
    again, arg2 = _pull(r, x, _pitched(H32, ph), ldc=pc_, ldarg=pa)
    assert np.array_equal(_bits(got), _bits(again)) and np.array_equal(arg, arg2), "two runs differ"
    noarg, _ = _pull(r, x, _pitched(H32, ph), ldc=pc_, want_arg=False)
    assert np.array_equal(_bits(noarg), _bits(got)), "want_arg=False changes C"
    # the one-table kernel on the merged table, and the reference
    Z = xr.merged32(ids, X, H32)
    C1, g1 = _one_table(a, ids, Z)
    wantC, wantarg = xr.forward(a, ids, X, H32)
    bad = (int(np.sum(_bits(got) != _bits(C1))), int(np.sum(xr.decode(arg, ids) != g1)), int(np.sum(_bits(got) != _bits(wantC))),
           int(np.sum(arg != wantarg)))
    lens = np.diff(a.indptr)[ids]
    print("%s d=%d pitches %s: n %d, longest row %d, empty rows %d, fresh / stale winners %d / %d; wrong elements against "
          "spmax: C %d arg %d, against the reference: C %d arg %d"
          % (what, d, (px, ph, pc_, pa), n, int(lens.max(initial=0)), int(np.sum(lens == 0)), int(np.sum(arg >= 0)),
             int(np.sum(arg <= -2)), bad[0], bad[1], bad[2], bad[3]))
    assert bad == (0, 0, 0, 0)
    assert np.array_equal(arg, xr.encode(g1, N, ids))
    # the bfloat16 table: the fp32 form's bits and winners on the widened table
    Hb, Hw, wide = _h16(H32)
    c16, a16 = _pull(r, x, Hb, ldc=pc_, ldarg=pa)
    c32, a32 = _pull(r, x, Hw, ldc=pc_, ldarg=pa)
    assert np.array_equal(_bits(c16), _bits(c32)) and np.array_equal(a16, a32), "the bfloat16 form is not the fp32 form on the widened table"
    w16 = xr.forward(a, ids, X, wide)
    assert np.array_equal(_bits(c16), _bits(w16[0])) and np.array_equal(a16, w16[1])
    return got, arg


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_every_pattern_and_vertex_set_is_spmax_on_the_merged_table(name):
    rng = np.random.RandomState(31)
    a = PATTERNS[name](rng).tocsr()
    a.sort_indices()
    r = Resident(a)
    N = a.shape[0]
    assert N <= 400
    seen = dict(no_in_part=0, no_out_of_part=0, empty=0, both=0)
    for sname, ids in _subsets(N, rng).items():
        r.select(ids)
        m = pr.position_map(N, ids)
        for i in ids:
            cols = a.indices[a.indptr[i]:a.indptr[i + 1]]
            k = 'empty' if cols.size == 0 else 'no_in_part' if (m[cols] < 0).all() else 'no_out_of_part' if (m[cols] >= 0).all() else 'both'
            seen[k] += 1
        for k, d in enumerate(WIDTHS_OF[sname]):
            draw = _grid if k == 0 else (lambda g, s: g.randn(*s).astype(np.float32))
            X, H = draw(rng, (len(ids), d)), draw(rng, (N, d))
            _check(r, a, ids, X, H, what="%s / %s / %s" % (name, sname, "grid" if k == 0 else "real"))
    print("%s: rows by kind %s" % (name, seen))
    if name == 'empty_rows':
        assert seen['empty'] > 0
    if name == 'lose_all':
        assert seen['no_in_part'] > 0
    assert seen['no_out_of_part'] > 0                     # (S = everything)


def test_the_grid_makes_ties_across_the_tables_and_between_the_zeros():
    """asserted on the CPU, on the inputs the device then runs: some maximum is tied between a fresh and a stale entry with
    either kind first, and some winner is a -0.0 in front of a +0.0 (and the other way round)"""
    rng = np.random.RandomState(32)
    a = ir.sbm_graph().tocsr()
    a.sort_indices()
    N, d = a.shape[0], 8
    ids = _subsets(N, rng)['every_other']
    X, H = _grid(rng, (len(ids), d)), _grid(rng, (N, d))
    C, arg = xr.forward(a, ids, X, H)
    m, Z, g = pr.position_map(N, ids), xr.merged32(ids, X, H), xr.decode(arg, ids)
    tied = dict(fresh_first=0, stale_first=0, neg_zero_first=0, pos_zero_first=0)
    for i, row in enumerate(ids):
        cols = a.indices[a.indptr[row]:a.indptr[row + 1]]
        for c in range(d):
            at = cols[Z[cols, c] == C[i, c]]
            if (m[at] >= 0).any() and (m[at] < 0).any():
                tied['fresh_first' if m[at[0]] >= 0 else 'stale_first'] += 1
            if at.size > 1 and C[i, c] == 0 and len(set(np.signbit(Z[at, c]))) == 2:
                tied['neg_zero_first' if np.signbit(C[i, c]) else 'pos_zero_first'] += 1
            if at.size:
                assert g[i, c] == at[0] and np.signbit(C[i, c]) == np.signbit(Z[at[0], c])
    print(tied)
    assert all(v > 0 for v in tied.values())
    _check(Resident(a).select(ids), a, ids, X, H, what="sbm / every_other / grid")


@pytest.mark.parametrize("vw", [4, 2, 1])
@pytest.mark.parametrize("d", WIDTHS)
def test_every_width_on_every_vector_width(d, vw):
    """the hub graph (a row of over 300 entries, two of just over one chunk) under S = a third: the four operands in turn on a pitch that
    allows exactly ``vw`` elements per vector (the others at 4), then all four on it"""
    rng = np.random.RandomState(33)
    a = PATTERNS['hub'](rng).tocsr()
    a.sort_indices()
    N = a.shape[0]
    ids = np.union1d(_subsets(N, rng)['third'], [7, 8, 9]).astype(np.int32)          # the long rows are selected
    assert np.diff(a.indptr)[7] >= 300 and min(np.diff(a.indptr)[[8, 9]]) > 64          # (five chunks and a tail; a chunk and a tail)
    r = Resident(a).select(ids)
    X, H = _grid(rng, (len(ids), d)), _grid(rng, (N, d))
    ld = _pitch(d, vw)
    assert ld >= d and (ld % 4 == 0 if vw == 4 else ld % 4 == 2 if vw == 2 else ld % 2 == 1)
    combos = [(vw, vw, vw, vw)] if vw == 4 else [(vw, 4, 4, 4), (4, vw, 4, 4), (4, 4, vw, 4), (4, 4, 4, vw), (vw, vw, vw, vw)]
    ref = None
    for pitches in combos:
        got = _check(r, a, ids, X, H, pitches=pitches, what="hub vw=%d" % vw)
        assert ref is None or (np.array_equal(_bits(got[0]), _bits(ref[0])) and np.array_equal(got[1], ref[1]))
        ref = got


@pytest.mark.parametrize("d", [3, 64])
def test_stored_rows_of_the_vertex_set_are_never_read(d):
    """+inf in every row of H[ids] with X finite: C stays finite and equals the clean run (a NaN could not tell: it never
    wins a strict comparison)"""
    rng = np.random.RandomState(34)
    a = ir.sbm_graph().tocsr()
    a.sort_indices()
    N = a.shape[0]
    for sname, ids in _subsets(N, rng).items():
        r = Resident(a).select(ids)
        X, H = rng.randn(len(ids), d).astype(np.float32), rng.randn(N, d).astype(np.float32)
        clean = _check(r, a, ids, X, H, what="sbm / %s clean" % sname)
        H[ids] = np.inf
        x = _pitched(X, _pitch(d, 4))
        got, arg = _pull(r, x, _pitched(H, _pitch(d, 4)))
        g16, a16 = _pull(r, x, _h16(H)[0])
        c16, _ = _pull(r, x, _h16(np.where(np.isinf(H), 0, H).astype(np.float32))[0])
        print("%s d=%d: finite %s / %s" % (sname, d, bool(np.isfinite(got).all()), bool(np.isfinite(g16).all())))
        assert np.isfinite(got).all() and np.isfinite(g16).all()
        assert np.array_equal(_bits(got), _bits(clean[0])) and np.array_equal(arg, clean[1])
        assert np.array_equal(_bits(g16), _bits(c16))


def test_rows_without_an_in_part_entry_never_read_x():
    """the lose_all pattern under S = every other vertex: no selected row stores a column of S, so no row of X is addressed --
    X = +inf leaves the result finite, every winner is stale"""
    rng = np.random.RandomState(35)
    a = PATTERNS['lose_all'](rng).tocsr()
    a.sort_indices()
    N = a.shape[0]
    ids = _subsets(N, rng)['every_other']
    assert pr.block(a, ids).nnz == 0 and a[ids].nnz > 0
    r = Resident(a).select(ids)
    for d in (5, 132):
        H = rng.randn(N, d).astype(np.float32)
        X = np.full((len(ids), d), np.inf, np.float32)
        got, arg = _pull(r, _pitched(X, _pitch(d, 4)), _pitched(H, _pitch(d, 4)))
        want = xr.forward(a, ids, np.zeros_like(X), H)
        assert np.isfinite(got).all() and np.array_equal(_bits(got), _bits(want[0])) and np.array_equal(arg, want[1])
        assert not (arg >= 0).any()


def test_no_rows_is_no_launch():
    from stochastic_gcn_amd import ops
    a = ir.signed(ir.flat_graph(50, 3, seed=1), seed=1)
    r = Resident(a)
    r.ids = torch.empty(0, dtype=torch.int32, device=DEV)
    for H in (torch.zeros((50, 4), device=DEV), ops.history_alloc(50, 4, DEV, bf16=True)):
        out, arg = ops.spmax_pull(r.A, r.ids, r.map, torch.empty((0, 4), device=DEV), H)
        assert tuple(out.shape) == (0, 4) and tuple(arg.shape) == (0, 4) and arg.dtype == torch.int32


# ---- the backward is the existing one -------------------------------------------------------------------------------------
def _product_bound(n, G, arg, add=None):
    """sparse_cases.fp64_bound of the backward read as a sparse product, column by column: dX[:, c] = S_c G[:, c] (+ add[:, c])
    with S_c[j, i] = 1 where arg[i, c] == j -- unit values, a row of S_c as long as the number of rows that row j won"""
    import scipy.sparse as sp
    out = np.zeros((n, G.shape[1]), np.float64)
    for c in range(G.shape[1]):
        i = np.flatnonzero(arg[:, c] >= 0)
        S = sp.csr_matrix((np.ones(i.size, np.float32), (arg[i, c], i)), shape=(n, n))
        kw = {} if add is None else dict(add=add[:, c:c + 1], add_rows=n)
        out[:, c] = sc.fp64_bound(S, G[:, c:c + 1], **kw)[:, 0]
    return out


@pytest.mark.parametrize("name", ['hub', 'sbm', 'lose_all', 'empty_rows'])
def test_spmax_bwd_over_the_blocks_transpose_is_the_scatter_to_in_part_winners(name):
    """ops.csr_induce's 'keep' block, its transpose with a plan, the pull's arg: dX bit for bit on dyadic G (with and without
    the self-half addend), within the fp64 bound on real G; a row whose every winner is stale sends nothing"""
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(36)
    a = PATTERNS[name](rng).tocsr()
    a.sort_indices()
    N = a.shape[0]
    A = ops.DeviceCSR.from_scipy(a, DEV, with_plan=False, with_transpose=True)
    for sname in ('every_other', 'third'):
        ids = _subsets(N, rng)[sname]
        n = len(ids)
        for d in (5, 64):
            blk = ops.csr_induce(A, ids, norm='keep')
            ids_dev = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(DEV)
            X, H = _grid(rng, (n, d)), _grid(rng, (N, d))
            if name == 'sbm':
                H = H + np.float32(4.0)               # every row with an out-of-part entry is won by stale rows alone
            C, arg = ops.spmax_pull(A, ids_dev, blk.map, torch.from_numpy(X).to(DEV), torch.from_numpy(H).to(DEV))
            wantC, wantarg = xr.forward(a, ids, X, H)
            arg_h = arg.cpu().numpy()
            assert np.array_equal(_bits(C.cpu().numpy()), _bits(wantC)) and np.array_equal(arg_h, wantarg)
            all_stale = np.flatnonzero((arg_h <= -2).all(axis=1))
            if name == 'sbm' or (name, sname) == ('lose_all', 'every_other'):
                assert all_stale.size > 0
            for kind in ('dyadic', 'real'):
                G = sc.ints(rng, (n, d)).astype(np.float32) if kind == 'dyadic' else rng.randn(n, d).astype(np.float32)
                add = sc.ints(rng, (n, d)).astype(np.float32) if kind == 'dyadic' else rng.randn(n, d).astype(np.float32)
                g_dev, add_dev = torch.from_numpy(G).to(DEV), torch.from_numpy(add).to(DEV)
                dx = ops.spmax_bwd(blk.transpose, g_dev, arg).cpu().numpy()
                dxa = ops.spmax_bwd(blk.transpose, g_dev, arg, add=add_dev, add_rows=n).cpu().numpy()
                f64, bound = xr.backward_f64(n, G, arg_h)
                f64a, bounda = xr.backward_f64(n, G, arg_h, add=add, add_rows=n)
                err, erra = np.abs(dx - f64), np.abs(dxa - f64a)
                print("%s / %s / d=%d %s: fresh / stale winners %d / %d, rows won by stale rows alone %d; worst error %.3e "
                      "(%.3f of its bound), with the addend %.3e" % (name, sname, d, kind, int(np.sum(arg_h >= 0)),
                                                                      int(np.sum(arg_h <= -2)), all_stale.size, float(err.max(initial=0)),
                                                                      float((err / np.maximum(bound, 1e-300)).max(initial=0)),
                                                                      float(erra.max(initial=0))))
                assert np.all(err <= bound) and np.all(erra <= bounda)
                assert np.all(err <= _product_bound(n, G, arg_h)) and np.all(erra <= _product_bound(n, G, arg_h, add))
                if kind == 'dyadic':
                    assert np.array_equal(_bits(dx), _bits(xr.backward(n, G, arg_h)))
                    assert np.array_equal(_bits(dxa), _bits(xr.backward(n, G, arg_h, add=add, add_rows=n)))
                # what a row won by stale rows alone sends: nothing -- the same dX with that row's gradient zeroed
                if all_stale.size:
                    G0 = G.copy()
                    G0[all_stale] = 0
                    dx0 = ops.spmax_bwd(blk.transpose, torch.from_numpy(G0).to(DEV), arg).cpu().numpy()
                    assert np.array_equal(_bits(dx0), _bits(dx))
