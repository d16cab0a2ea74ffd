"""The catalogues of tests/rows_cases.py reach every cell of the launch rules they restate, and the NumPy references the
exact GPU tests (test_rows_exact_gpu.py) compare with are held to what the reference's own C++ produced
(tests/golden/slice.npz), to the library's host pass and to SciPy -- so the GPU tests never compare a kernel with
something only this file vouches for."""
import numpy as np
import pytest
import scipy.sparse as sp

import golden_util as gu
import rows_cases as rc


# ---- the catalogues reach every reachable cell ------------------------------------------------------------------------------
def test_rows_catalogue_reaches_every_cell():
    have = {rc.case_cell(c) for c in rc.ROWS_CASES}
    assert have >= set(rc.rows_reachable()), sorted(set(rc.rows_reachable()) - have)
    # ... and the cells the rules can form at all are there: every vector width with every lane group, ragged where a
    # vector has more than one element, a second trip only with 64 lanes, n below / on / one past a workgroup
    want = {(vw, G, rag, multi, pos) for vw in (1, 2, 4) for G in (8, 16, 32, 64) for rag in ((False,) if vw == 1 else (False, True))
            for multi in ((False, True) if G == 64 else (False,)) for pos in rc.NPOS}
    assert have == want
    assert {c["d"] for c in rc.ROWS_CASES} == set(rc.WIDTHS)
    assert {(c["in_off"], c["out_off"]) for c in rc.ROWS_CASES} == {(a, b) for a in rc.OFFSETS for b in rc.OFFSETS}
    for c in rc.ROWS_CASES:
        assert c["ldi"] >= c["d"] and c["ldo"] >= c["d"] and 0 < c["n"] <= c["N"]
        assert rc.rows_plan(c["d"], c["ldi"], c["ldo"], c["in_off"], c["out_off"])["multi"] == (rc.case_cell(c)[3])


def test_rows_plan_restates_the_launch_rule():
    assert [rc.group_lanes(v) for v in (1, 8, 9, 16, 17, 32, 33, 64, 65, 301)] == [8, 8, 16, 16, 32, 32, 64, 64, 64, 64]
    assert rc.rows_plan(128, 128, 128, 0, 0) == dict(vw=4, nvec=32, G=32, gpb=8, ragged=False, multi=False)
    assert rc.rows_plan(602, 602, 608, 0, 0)["vw"] == 2 and rc.rows_plan(602, 602, 608, 0, 0)["multi"]
    assert rc.rows_plan(128, 128, 128, 1, 0)["vw"] == 1 and rc.rows_plan(128, 128, 128, 2, 0)["vw"] == 2
    assert rc.rows_plan(1204, 1204, 1204, 0, 0) == dict(vw=4, nvec=301, G=64, gpb=4, ragged=False, multi=True)
    assert [rc.n_pos(n, 8) for n in (1, 7, 8, 9, 15, 16, 17)] == ["below", "below", "on", "past", "below", "on", "past"]


def test_park_catalogue_reaches_every_cell():
    have = {rc.park_cell(c["d"], c["ldh"], c["lds"], c["aligned"]) for c in rc.PARK_CASES}
    assert have == set(rc.park_reachable())
    assert have == {("park", False), ("park", True), ("own", "d"), ("own", "ldh"), ("own", "lds"), ("own", "table"), ("own", "source")}
    parked = [c for c in rc.PARK_CASES if rc.park_cell(c["d"], c["ldh"], c["lds"], c["aligned"])[0] == "park"]
    assert {c["d"] for c in parked} == set(rc.PARK_WIDTHS)
    assert {c["d"] for c in rc.PARK_CASES} == set(rc.PARK_WIDTHS + rc.PARK_REFUSED_WIDTHS)
    assert {c["n"] for c in rc.PARK_CASES} == set(rc.PARK_N) and {c["params"] for c in rc.PARK_CASES} == set(rc.ADAM_COUNTS)
    assert rc.park_cell(128, 128, 128, jobs=2) == ("own", "third") and rc.park_cell(128, 128, 128, n=0) == ("own", "n")
    assert [rc.adam_blocks(n) for n in rc.ADAM_COUNTS] == [1, 1, 2, 2048]


def test_transpose_catalogue_reaches_every_cell():
    have = {rc.transpose_cell(*c) for c in rc.TRANSPOSE_CASES}
    assert have == set(rc.transpose_reachable())
    assert have == {(k, lds, full) for k in (1, 2, 3) for lds in (False, True) for full in (False, True)}
    for edge in ((16384, 513), (16385, 513), (300, 511), (300, 512), (300, 513), (255, 1500), (256, 1500), (257, 1500)):
        assert edge in rc.TRANSPOSE_CASES
    assert rc.transpose_plan(16384, 513)["lds_bytes"] == 64 * 1024 and not rc.transpose_plan(16385, 513)["lds"]


def test_transpose_scratch_size_equals_the_library():
    from stochastic_gcn_amd._ffi import lib
    for ncols, nnz in list(rc.TRANSPOSE_CASES) + [(0, 5), (5, 0), (1, 1), (20000, 1 << 20)]:
        assert int(lib.sgcn_csr_transpose_ws_ints(ncols, nnz)) == rc.transpose_plan(ncols, nnz)["ws_ints"], (ncols, nnz)


def test_scale_and_exchange_catalogues():
    assert {rc.scale_cell(c["d"], c["n"]) for c in rc.SCALE_CASES} == set(rc.scale_reachable())
    assert {c["d"] for c in rc.SCALE_CASES} == set(rc.WIDTHS)
    for c in rc.SCALE_CASES:             # the contract of sgcn_scale_rows_f32
        assert c["ldx"] % 4 == 0 and c["ldo"] % 4 == 0 and c["ldx"] >= c["d"] and c["ldo"] >= c["d"]
    ex = rc.EXCHANGE_CASES
    assert {(c["world"], c["d"], c["cap"]) for c in ex} == {(w, d, k) for w in rc.X_WORLDS for d in rc.X_D for k in rc.X_CAP}
    for cap in rc.X_CAP:                 # every block size of a capacity occurs, the full block among them
        assert {s for c in ex if c["cap"] == cap for s in c["sizes"]} == set(rc.x_sizes(cap))
    # the per-rank form's payloads reach every vector width, VW = 4 among them only where d % 4 == 0
    vws = {(c["d"] % 4 == 0, rc.exchange_payload_vw(c["d"], c["ldh"], c["cap"], r)) for c in ex for r in range(c["world"])}
    assert {v for _, v in vws} == {1, 2, 4} and (False, 4) not in vws
    assert rc.exchange_form(2, True) == "rank" and rc.exchange_form(3, True) == "claim" and rc.exchange_form(8, False) == "rank"


def test_inputs_are_distinct_and_ids_unique():
    x = rc.patterns(3000, 129, specials=False)
    assert len(np.unique(rc.bits(x))) == x.size
    y = rc.bits(rc.patterns(40, 12))
    assert np.isnan(y.view(np.float32)).any() and np.isinf(y.view(np.float32)).any() and (y == np.int32(-2 ** 31)).any()
    assert ((y & 0x7f800000) == 0).any()                       # subnormals
    rng = np.random.RandomState(1)
    for N, n in ((2, 2), (500, 123), (9, 9)):
        ids = rc.unique_ids(rng, N, n)
        assert len(set(ids.tolist())) == n and 0 in ids and N - 1 in ids
    ids = rc.unique_ids(rng, 500, 100, pads=30)
    assert (ids == -1).sum() == 30
    with pytest.raises(AssertionError):
        rc.assert_scatter_ids(np.array([3, 5, 3], np.int32), 10)
    big = rc.big_ids(50, "t")
    assert {0, rc.BIG_SPLIT - 1, rc.BIG_SPLIT, rc.BIG_N - 1} <= set(big.tolist()) and rc.BIG_SPLIT == 8388608


# ---- the references against the reference's own outputs, the host pass and SciPy --------------------------------------------
def _golden():
    z = gu.load("slice.npz")
    names = sorted({k.split("/")[1] for k in z.files if k.startswith("slice/")})
    assert len(names) == 5
    return z, names


def test_slice_and_gather_references_reproduce_the_golden_slices():
    z, names = _golden()
    a_d, a_i, a_p = z["a/data"], z["a/indices"], z["a/indptr"]
    for n in names:
        r = z["slice/%s/r" % n]
        o_p, o_d, o_c, o_r = rc.ref_csr_slice(a_d, a_i, a_p, r)
        if ("slice/%s/is_empty_csr" % n) in z.files:
            assert o_p[-1] == 0 and len(o_d) == 0 and tuple(z["slice/%s/is_empty_csr" % n]) == (len(r), int(z["a/shape"][1]))
        else:
            assert gu.bits_equal(np.stack([o_r, o_c], axis=1), z["slice/%s/indices" % n]), n
            assert gu.bits_equal(o_d, z["slice/%s/data" % n]), n
            assert tuple(z["slice/%s/shape" % n]) == (len(r), int(z["a/shape"][1]))
        assert gu.bits_equal(rc.ref_gather(z["dense/a"], r), z["dense/%s/out" % n]), n


def test_row_pointer_reference_equals_the_golden_counts_and_the_host_pass():
    from stochastic_gcn_amd._ffi import check, lib
    z, names = _golden()
    a_p = np.ascontiguousarray(z["a/indptr"], np.int32)
    sels = [np.ascontiguousarray(z["slice/%s/r" % n], np.int32) for n in names]
    for n, r in zip(names, sels):
        o_p = rc.ref_slice_indptr(a_p, r)
        rows = z["slice/%s/indices" % n][:, 0] if ("slice/%s/indices" % n) in z.files else np.zeros(0, np.int32)
        counts = np.bincount(rows, minlength=len(r))
        assert np.array_equal(o_p, np.concatenate([[0], np.cumsum(counts)])), n
    for r in sels + [np.zeros(0, np.int32)]:
        host = np.empty(len(r) + 1, np.int32)
        check(lib.sgcn_csr_slice_indptr(len(r), r.ctypes.data, a_p.ctypes.data, host.ctypes.data))
        assert np.array_equal(host, rc.ref_slice_indptr(a_p, r))
    d, i, p = _slice_matrix()
    for name, r in slice_selections(len(p) - 1, np.diff(p)):
        host = np.empty(len(r) + 1, np.int32)
        check(lib.sgcn_csr_slice_indptr(len(r), r.ctypes.data, p.ctypes.data, host.ctypes.data))
        assert np.array_equal(host, rc.ref_slice_indptr(p, r)), name


def _slice_matrix():
    return rc.csr_with_rows(rc.SLICE_ROW_LENS, rc.SLICE_NCOLS, "slice")


def slice_selections(nrows, lens):
    return rc.slice_selections(nrows, lens)


def test_slice_reference_equals_scipy_row_indexing():
    d, i, p = _slice_matrix()
    A = sp.csr_matrix((np.arange(1, len(d) + 1, dtype=np.float64), i, p), shape=(len(p) - 1, rc.SLICE_NCOLS))
    names = set()
    for name, r in slice_selections(len(p) - 1, np.diff(p)):
        names.add(name)
        o_p, o_d, o_c, o_r = rc.ref_csr_slice(np.arange(1, len(d) + 1, dtype=np.float64), i, p, r)
        S = A[r] if len(r) else sp.csr_matrix((0, rc.SLICE_NCOLS))
        assert np.array_equal(S.indptr, o_p) and np.array_equal(S.indices, o_c) and np.array_equal(S.data, o_d), name
        assert np.array_equal(o_r, np.repeat(np.arange(len(r)), np.diff(o_p)))
    assert {"n1", "n256", "n257", "n65537", "all_empty", "ends_empty", "repeated", "long_next_to_empty"} <= names
    assert {0, 1, 63, 64, 65, 128, 129, 400} <= set(np.diff(p).tolist())


def _transpose_inputs(ncols, nnz, **kw):
    d, i, p = rc.csr_with_nnz(ncols, nnz, (ncols, nnz, sorted(kw.items())), **kw)
    r = np.random.RandomState(rc.seed("perm", ncols, nnz)).permutation(len(p) - 1).astype(np.int32)
    return (d, i, p, r) + rc.ref_csr_slice(d, i, p, r)


def test_transpose_reference_equals_scipy():
    cases = [(c, z, {}) for c, z in rc.TRANSPOSE_CASES] + [(c, z, kw) for c, z, kw in rc.TRANSPOSE_EDGES]
    for ncols, nnz, kw in cases:
        d, i, p, r, o_p, o_d, o_c, o_r = _transpose_inputs(ncols, nnz, **kw)
        assert len(o_c) == nnz
        t_rowptr, t_row, t_src = rc.ref_transpose(ncols, o_c, o_r)
        pos = np.arange(1, nnz + 1, dtype=np.float64)              # the source position of every entry, as its value
        T = sp.csr_matrix((pos, o_c, o_p), shape=(len(r), ncols)).T.tocsr()
        T.sort_indices()
        assert np.array_equal(T.indptr, t_rowptr) and np.array_equal(T.indices, t_row), (ncols, nnz, kw)
        assert np.array_equal(T.data, t_src.astype(np.float64) + 1)
        assert np.array_equal(rc.bits(rc.ref_gather_f32(o_d, t_src)), rc.bits(o_d[(T.data - 1).astype(np.int64)]))
        Tv = sp.csr_matrix((o_d, o_c, o_p), shape=(len(r), ncols)).T.tocsr()       # SciPy moves the fp32 bits untouched
        Tv.sort_indices()
        assert np.array_equal(rc.bits(Tv.data), rc.bits(rc.ref_gather_f32(o_d, t_src)))


def test_scatter_pack_and_apply_references():
    rng = np.random.RandomState(3)
    H = rc.patterns(50, 7, base=1)
    src = rc.patterns(9, 7, base=90000)
    ids = rc.unique_ids(rng, 50, 9, pads=3)
    out = rc.ref_scatter(H, ids, src)
    for m in range(50):
        k = np.nonzero(ids == m)[0]
        assert np.array_equal(rc.bits(out[m]), rc.bits(src[k[0]] if len(k) else H[m]))
    # apply: the higher rank wins, pads skipped, untouched rows kept
    cap, d, world = 4, 3, 3
    blocks = []
    for r, (n, ids) in enumerate([(2, [5, 6]), (4, [6, 7, 8, 9]), (1, [5])]):
        rows = rc.patterns(cap, d, base=1000 * (r + 1), specials=False)
        blocks.append(rc.ref_hist_pack(np.array(ids, np.int32), n, rows, d, cap, fill=-7))
        assert list(blocks[-1][:cap]) == ids + [-1] * (cap - n) and (blocks[-1][cap + n * d:] == -7).all()
    recv = np.concatenate(blocks)
    H = rc.patterns(12, 5, base=7, specials=False)
    out = rc.ref_hist_apply(H, recv, world, cap, d)
    pay = lambda r, i: recv[r * cap * (d + 1) + cap:][i * d:(i + 1) * d]
    assert np.array_equal(rc.bits(out[5, :d]), pay(2, 0)) and np.array_equal(rc.bits(out[6, :d]), pay(1, 0))
    assert np.array_equal(rc.bits(out[9, :d]), pay(1, 3)) and np.array_equal(rc.bits(out[:5]), rc.bits(H[:5]))
    assert np.array_equal(rc.bits(out[:, d:]), rc.bits(H[:, d:])) and np.array_equal(rc.bits(out[10:]), rc.bits(H[10:]))
    x = np.array([[1.5, -0.0, 3.0]], np.float32)
    assert np.array_equal(rc.bits(rc.ref_scale_rows(x, np.array([-1.0], np.float32))), rc.bits(np.array([[-1.5, 0.0, -3.0]], np.float32)))
