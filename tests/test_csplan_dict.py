"""Dictionary plans of the two-group column sweep (csrc/sgcn_csplan.cpp sgcn_csbuild_dict, sgcn_tune "cs_dict"): a tile's
values live in a table of its distinct bit patterns and an entry's column word carries the table index.  Decoded on the
host -- word -> column, local row, table value -- such a plan is the cs_dict = 0 plan of the same matrix entry for entry,
pads included; it falls back, byte for byte, where a tile has too many values or the column leaves too few index bits;
and it does not depend on the number of building threads."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from stochastic_gcn_amd._ffi import check, lib

PAD = 0x80000000
RND, ALIGN = 64, 256


@pytest.fixture(autouse=True)
def _restore_knob():
    before = lib.sgcn_tune_get(b"cs_dict")
    yield
    check(lib.sgcn_tune(b"cs_dict", before))


def build(a, K, threads=4, G=2, T=0, rnd=RND, align=ALIGN, offer=True):
    """sgcn_csplan_build [+ sgcn_csbuild_dict] + the exports: dict(bits, tile_ptr, colrow, val | None, rows, slots, fix, nslots,
    tile_vals | None, tile_nvals | None)"""
    a = a.tocsr()
    rowptr, col = np.ascontiguousarray(a.indptr, np.int32), np.ascontiguousarray(a.indices, np.int32)
    val = np.ascontiguousarray(a.data, np.float32)
    h = C.c_void_p()
    check(lib.sgcn_csplan_build(rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, a.shape[0], G, 16, T, rnd, align, None, None, 0,
                                threads, C.byref(h)))
    try:
        bits = C.c_int32(-1)
        if offer:
            check(lib.sgcn_csbuild_dict(h, K, C.byref(bits)))
        else:
            bits.value = 0
        nt, ne, nf, ns = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        check(lib.sgcn_csbuild_sizes(h, C.byref(nt), C.byref(ne), C.byref(nf), C.byref(ns), None, None))
        tp, cr = np.empty(nt.value + 1, np.int64), np.empty(ne.value, np.int32)
        vo = np.empty(ne.value, np.float32) if bits.value == 0 else None
        tr, ts = np.empty(nt.value * 16 * G, np.int32), np.empty(nt.value * 16 * G, np.int32)
        fx = np.empty((nf.value, 3), np.int32)
        check(lib.sgcn_csbuild_export(h, tp.ctypes.data, cr.ctypes.data, vo.ctypes.data if vo is not None else None, tr.ctypes.data,
                                      ts.ctypes.data, fx.ctypes.data if nf.value else None))
        tv = tn = None
        if bits.value:
            tv, tn = np.empty(nt.value << bits.value, np.float32), np.empty(nt.value, np.int32)
            check(lib.sgcn_csbuild_export_dict(h, tv.ctypes.data, tn.ctypes.data))
        else:
            assert lib.sgcn_csbuild_export_dict(h, None, None) == -1          # not a dictionary plan: nothing to export
    finally:
        lib.sgcn_csbuild_free(h)
    return dict(bits=bits.value, tile_ptr=tp, colrow=cr, val=vo, rows=tr, slots=ts, fix=fx, nslots=ns.value, tile_vals=tv,
                tile_nvals=tn)


def plain(a, K, **kw):
    check(lib.sgcn_tune(b"cs_dict", 0))
    p = build(a, K, **kw)
    check(lib.sgcn_tune(b"cs_dict", 1))
    assert p["bits"] == 0
    return p


def same_bytes(p, q):
    for k in ("tile_ptr", "colrow", "val", "rows", "slots", "fix", "tile_vals", "tile_nvals"):
        x, y = p[k], q[k]
        assert (x is None) == (y is None), k
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k
    assert p["bits"] == q["bits"] and p["nslots"] == q["nslots"]


def want_bits(K):
    return min(10, 28 - int(np.ceil(np.log2(K))) if K > 1 else 28)


def check_decodes_to(d, p, K):
    """dictionary plan ``d`` against the plan with a value array ``p`` of the same matrix: entry for entry"""
    bits = d["bits"]
    assert bits == want_bits(K) and 5 <= bits <= 10
    colbits = 28 - bits
    for k in ("tile_ptr", "rows", "slots", "fix"):
        assert np.array_equal(d[k], p[k]), k
    assert d["nslots"] == p["nslots"] and d["val"] is None
    cr = d["colrow"].view(np.uint32)
    nt = d["tile_ptr"].shape[0] - 1
    tile = np.repeat(np.arange(nt, dtype=np.int64), np.diff(d["tile_ptr"]))
    col, idx, lr = cr & np.uint32((1 << colbits) - 1), (cr >> np.uint32(colbits)) & np.uint32((1 << bits) - 1), cr >> np.uint32(28)
    pcr = p["colrow"].view(np.uint32)
    assert np.array_equal(col, pcr & np.uint32(0x0FFFFFFF)) and np.array_equal(lr, pcr >> np.uint32(28))
    assert col.size == 0 or int(col.max()) < K                                        # what the kernel gathers from
    assert np.array_equal(col | (lr << np.uint32(28)), pcr)                           # the word with its index cleared IS the parent's
    nv = d["tile_nvals"].astype(np.int64)
    assert (idx.astype(np.int64) < nv[tile]).all() and nv.max(initial=0) <= (1 << bits)
    tv = d["tile_vals"].view(np.uint32).reshape(nt, 1 << bits)
    got = tv[tile, idx.astype(np.int64)]
    assert np.array_equal(got, p["val"].view(np.uint32))                              # same value bits, pads included
    # the tables: a tile's distinct patterns, ascending as uint32, zero behind them
    pv = p["val"].view(np.uint32)
    for t in range(nt):
        u = np.unique(pv[d["tile_ptr"][t]:d["tile_ptr"][t + 1]])
        assert nv[t] == u.size and np.array_equal(tv[t, :u.size], u) and not tv[t, u.size:].any()
    return bits


def rownorm(n=3000, k=None, deg=30, seed=1, long_rows=(5, 17, 400), long_cols=()):
    """a row-normalised random graph (one value per row), a few rows -- and, for its transpose, columns -- longer than the
    split threshold (8 x the mean degree)"""
    k = n if k is None else k
    rng = np.random.RandomState(seed)
    rows = np.repeat(np.arange(n), rng.poisson(deg, n).clip(1))
    a = sp.csr_matrix((np.ones(rows.size, np.float32), (rows, rng.randint(0, k, rows.size))), shape=(n, k))
    a = a.tolil()
    for r in long_rows:
        a[r, rng.choice(k, 700, replace=False)] = 1.0
    for c in long_cols:
        a[rng.choice(n, 700, replace=False), c] = 1.0
    a = a.tocsr()
    a.data[:] = 1.0
    a.sort_indices()
    d = np.diff(a.indptr)
    a.data = np.repeat((1.0 / np.maximum(d, 1)).astype(np.float32), d)
    return a


@pytest.fixture(scope="module")
def graph():
    a = rownorm(long_cols=(9, 1234))
    a.data[a.indptr[40] + 2] = -0.0               # a real -0.0f: the pad marker's bits (stored as +0.0f, as without tables)
    assert np.diff(a.indptr).max() > 8 * a.nnz // a.shape[0]
    return a


def test_row_normalised_graph_and_its_transpose_decode_to_the_plain_plan(graph):
    for a in (graph, graph.T.tocsr()):
        a.sort_indices()
        K = a.shape[1]
        p, d = plain(a, K), build(a, K)
        assert p["fix"].shape[0] >= 2 and (p["val"].view(np.uint32) == PAD).any()      # split rows and pads are present
        assert check_decodes_to(d, p, K) == 10
        print("K=%d tiles=%d entries=%d distinct per tile: mean %.1f max %d" % (
            K, d["tile_nvals"].size, d["colrow"].size, d["tile_nvals"].mean(), d["tile_nvals"].max()))


def test_a_real_negative_zero_is_stored_as_the_plain_plan_stores_it(graph):
    K = graph.shape[1]
    p, d = plain(graph, K), build(graph, K)
    r = 40
    tv = d["tile_vals"].view(np.uint32).reshape(-1, 1 << d["bits"])
    cr = d["colrow"].view(np.uint32)
    tile = np.repeat(np.arange(d["tile_ptr"].size - 1), np.diff(d["tile_ptr"]))
    e = np.arange(cr.size) - d["tile_ptr"][:-1][tile]
    row = d["rows"][tile * 32 + (e % 2) * 16 + (cr >> np.uint32(28)).astype(np.int64)]
    vb = tv[tile, ((cr >> np.uint32(18)) & np.uint32(1023)).astype(np.int64)]
    mine = (row == r) & (vb != PAD)
    assert mine.sum() == graph.indptr[r + 1] - graph.indptr[r]                        # -0.0 did not become a pad ...
    assert (vb[mine] == 0).sum() == 1                                                 # ... it is the row's one +0.0f
    assert np.array_equal(vb, p["val"].view(np.uint32))


@pytest.mark.parametrize("K,bits", [((1 << 18) - 3, 10), (1 << 20, 8), ((1 << 20) + 1, 7), (1 << 23, 5)])
def test_the_index_takes_the_bits_the_column_leaves(K, bits):
    """K just below 2^18: ten index bits; at 2^20: eight; 2^23: five, the floor (constant values there: 32 rows of a tile
    with a value each, and the pad marker, would be 33 patterns)"""
    a = rownorm(n=2000, k=K, deg=20, seed=K % 1000, long_rows=(3,))
    if bits == 5:
        a.data[:] = 0.25
    a[0, K - 1] = a.data[0]                                                           # the last column is used
    a = a.tocsr()
    a.sort_indices()
    assert want_bits(K) == bits
    p, d = plain(a, K), build(a, K)
    assert check_decodes_to(d, p, K) == bits
    assert int((d["colrow"].view(np.uint32) & np.uint32((1 << (28 - bits)) - 1)).max()) == K - 1


def test_too_few_index_bits_fall_back_to_the_plain_plan():
    K = (1 << 23) + 1                                                                 # ceil(log2 K) = 24: four bits, below the floor
    a = rownorm(n=2000, k=K, deg=20, seed=4, long_rows=(3,))
    a.data[:] = 0.25
    assert want_bits(K) == 4
    same_bytes(build(a, K), plain(a, K))
    same_bytes(build(a, 1 << 28), plain(a, K))


def test_one_tile_with_one_value_too_many_makes_the_whole_plan_fall_back():
    K = 1 << 20                                                                       # eight index bits: 256 patterns per tile
    a = rownorm(n=2000, k=K, deg=20, seed=9, long_rows=())
    a.data[:] = 0.5
    r = int(np.argmax(np.diff(a.indptr) >= 1))
    a = a.tolil()
    cols = np.arange(255) * 3
    a[r, :] = 0
    a[r, cols] = (1.0 + np.arange(255) / 1024.0).astype(np.float32)                   # 255 patterns + 0.5 of the other rows + the pad marker
    a = a.tocsr()
    a.eliminate_zeros()
    a.sort_indices()
    p = plain(a, K, T=1024)
    tile = np.repeat(np.arange(p["tile_ptr"].size - 1), np.diff(p["tile_ptr"]))
    per_tile = [np.unique(p["val"].view(np.uint32)[tile == t]).size for t in range(p["tile_ptr"].size - 1)]
    assert max(per_tile) == 257 and sorted(per_tile)[-2] <= 2                         # ONE tile is over, by one
    same_bytes(build(a, K, T=1024), p)
    a.data[a.indptr[r]] = a.data[a.indptr[r] + 1]                                     # one pattern fewer: 256, the plan takes tables
    d = build(a, K, T=1024)
    assert d["bits"] == 8 and d["tile_nvals"].max() == 256
    check_decodes_to(d, plain(a, K, T=1024), K)


def test_a_matrix_of_arbitrary_values_keeps_its_value_array():
    """every nonzero its own pattern: the tables would be as long as the entries"""
    a = sp.random(300, 300, density=0.05, format='csr', dtype=np.float32, random_state=np.random.RandomState(3))
    a.sort_indices()
    same_bytes(build(a, 300), plain(a, 300))


def test_the_plan_does_not_depend_on_the_building_threads(graph):
    for a in (graph, graph.T.tocsr()):
        a.sort_indices()
        ref = build(a, a.shape[1], threads=1)
        assert ref["bits"] == 10
        for threads in (3, 8):
            same_bytes(build(a, a.shape[1], threads=threads), ref)


def test_knob_off_other_group_counts_and_bad_arguments(graph):
    K = graph.shape[1]
    same_bytes(plain(graph, K), build(graph, K, offer=False))                         # cs_dict = 0: the build without the call
    for G in (1, 4):                                                                  # only the two-group kernel reads tables
        same_bytes(build(graph, K, G=G, rnd=0 if G == 1 else RND, align=0 if G == 1 else ALIGN),
                   build(graph, K, G=G, rnd=0 if G == 1 else RND, align=0 if G == 1 else ALIGN, offer=False))
    assert lib.sgcn_tune_get(b"cs_dict") == 1
    assert lib.sgcn_tune(b"cs_dict", 2) != 0 and lib.sgcn_tune(b"cs_dict", -1) != 0
    with pytest.raises(RuntimeError, match="column outside"):
        build(graph, K - 1)
    assert lib.sgcn_csbuild_dict(None, 8, None) == -1


# ---- ops.ColumnSweepCSR carries it through -------------------------------------------------------------------------------
def test_column_sweep_csr_carries_the_tables(graph, tmp_path):
    import torch
    from stochastic_gcn_amd import ops
    cpu = torch.device("cpu")
    A = ops.ColumnSweepCSR(graph, cpu, G=2, round_tiles=RND)
    check(lib.sgcn_tune(b"cs_dict", 0))
    P = ops.ColumnSweepCSR(graph, cpu, G=2, round_tiles=RND)
    check(lib.sgcn_tune(b"cs_dict", 1))
    N = ops.ColumnSweepCSR(graph, cpu, G=2, round_tiles=RND, dictionary=False)          # e.g. under an edge mask: values re-drawn
    assert A.dict_bits == 10 and P.dict_bits == N.dict_bits == 0 and A._val is None and N.tile_vals is None
    assert set(vars(A)) == set(vars(P))
    for X in (P, N):
        assert torch.equal(A.tile_ptr, X.tile_ptr) and torch.equal(A.tile_rows, X.tile_rows)
        assert np.array_equal(A.columns_rows(), X.colrow.numpy())
        assert np.array_equal(A.val.numpy().view(np.uint32), X.val.numpy().view(np.uint32))
    for x, y in zip(ops.plan_entries(A), ops.plan_entries(P)):
        assert np.array_equal(x, y)
    st, sp_ = A.struct(64), P.struct(64)
    assert st.dict_bits == 10 and st.dev_val is None and st.dev_tile_vals and st.dev_tile_nvals
    assert sp_.dict_bits == 0 and sp_.dev_val and sp_.dev_tile_vals is None and sp_.dev_tile_nvals is None
    assert "tables of 1024" in A.variant(602) and "tables" not in P.variant(602)
    assert A.variant(602).split("; values")[0] + ")" == P.variant(602)
    A.live_val = P.val                          # a value array handed to a dictionary plan: read on the words without indices
    sl = A.struct(64)
    assert sl.dict_bits == 0 and sl.dev_val == P.val.data_ptr() and sl.dev_tile_vals is None and sl.dev_colrow != st.dev_colrow
    assert torch.equal(A._colrow_plain, P.colrow)
    A.live_val = None
    assert A.struct(64).dict_bits == 10 and A.struct(64).dev_colrow == st.dev_colrow
    # the cache file: a plan with a value array writes what it always wrote; a dictionary plan its tables
    A.pace[64], A.tuned_ms[64] = 250, 1.5
    pa, pp = str(tmp_path / "a.npz"), str(tmp_path / "p.npz")
    A.save(pa, "k")
    P.save(pp, "k")
    za, zp = np.load(pa), np.load(pp)
    assert set(za.files) - set(zp.files) == {"dict_bits", "tile_vals", "tile_nvals"} and za["val"].size == 0
    B = ops.ColumnSweepCSR.load(pa, cpu, "k", g=2)
    assert B is not None and B.dict_bits == 10 and B.pace == {64: 250}
    for k in ("tile_ptr", "colrow", "tile_rows", "tile_slots", "tile_vals", "tile_nvals"):
        assert torch.equal(getattr(A, k), getattr(B, k)), k
    assert B.struct(64).dict_bits == 10 and B.variant(64) == A.variant(64)
    # the cache key says whether the plan was offered to the dictionary
    p1, p2 = str(tmp_path / "c1.npz"), str(tmp_path / "c2.npz")
    X, hit = ops.ColumnSweepCSR.cached(graph, cpu, p1, G=2)
    X.store_if_cached()
    assert not hit and X.dict_bits == 10 and ops.ColumnSweepCSR.cached(graph, cpu, p1, G=2)[1]
    Y, hit = ops.ColumnSweepCSR.cached(graph, cpu, p1, G=2, dictionary=False)
    assert not hit and Y.dict_bits == 0
    Y._cache = (p2, Y._cache[1])
    Y.store_if_cached()
    assert ops.ColumnSweepCSR.cached(graph, cpu, p2, G=2, dictionary=False)[1]
    assert not ops.ColumnSweepCSR.cached(graph, cpu, p2, G=2)[1]


def test_static_matrix_under_an_edge_mask_keeps_the_value_array(graph):
    import torch
    from stochastic_gcn_amd import full_batch
    sq = graph[:, :graph.shape[0]].tocsr()
    m = full_batch.StaticMatrix(sq, torch.device("cpu"), kernel='cs', d=128)
    e = full_batch.StaticMatrix(sq, torch.device("cpu"), kernel='cs', d=128, edge_dropout=0.25)
    assert m._plan.G == 2 and m._plan.dict_bits == 10 and e._plan.dict_bits == 0 and e._plan._val is not None
