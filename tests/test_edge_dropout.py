"""CPU tests of --edge_dropout: the host decode of every plan layout (which original (row, col) a stored entry belongs to, and
so which pair key it carries), the statistics of the mask, the flag and its refusals, and the argument checks of the new
export.  The mask itself is restated in tests/edge_mask_ref.py on the oracle's hash; nothing here touches a device."""
import numpy as np
import pytest
import torch

import edge_mask_ref as ref
import sparse_cases as sc
from stochastic_gcn_amd import _ffi, ops
from stochastic_gcn_amd.flags import FLAGS, _Flags

PATTERNS = ("empty", "identity", "star_row", "star_col", "row_lengths", "rmat")
LAYOUTS = ("csr", "cs1", "cs2", "cs4")


@pytest.fixture(autouse=True)
def _reset_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


# ---- decode ------------------------------------------------------------------------------------------------------------
_MATRICES = {}


def matrix(name):
    """The pattern made square, with distinct-looking non-zero values (built once per name and left unchanged)."""
    if name not in _MATRICES:
        a = ref.squared(sc.pattern(name))
        rng = np.random.RandomState(5)
        a.data[:] = (rng.uniform(0.5, 2.0, a.nnz) * rng.choice([-1.0, 1.0], a.nnz)).astype(np.float32)
        _MATRICES[name] = a
    return _MATRICES[name]


def entries(a, layout):
    """(row, col, pad, stored values) of every stored entry of ``a`` in ``layout``, from the layout's own host records."""
    if layout == "csr":
        return ops.csr_entries(a.indptr, a.indices) + (a.data.astype(np.float32),)
    G = int(layout[2:])
    p = ops.ColumnSweepCSR._plan_one(a, sc.T_SPLIT, 0, None, None, 'auto') if G == 1 else \
        ops.ColumnSweepCSR._plan_groups(a, G, sc.T_SPLIT, 0, 'auto', 'auto')
    assert p["G"] == G
    return ops.cs_entries(p["tile_ptr"], p["colrow"], p["val"], p["tile_rows"], G) + (p["val"],)


def _sorted_triples(row, col, val):
    t = np.stack([np.asarray(row, np.int64), np.asarray(col, np.int64),
                  np.ascontiguousarray(val, np.float32).view(np.uint32).astype(np.int64)], axis=1)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


PADS_SEEN = {}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", PATTERNS)
def test_decode_recovers_the_matrix_and_keys_every_entry(name, layout):
    a = matrix(name)
    row, col, pad, val = entries(a, layout)
    r0, c0 = ref.coo_of(a)
    live = ~pad
    # the decoded non-pad (row, col, base value) multiset is the matrix's COO
    assert np.array_equal(_sorted_triples(row[live], col[live], val[live]), _sorted_triples(r0, c0, a.data))
    if layout in ("csr", "cs1"):
        assert not pad.any()
    else:
        assert np.all(np.ascontiguousarray(val, np.float32).view(np.uint32)[pad] == ref.PAD_BITS)
        PADS_SEEN[layout] = PADS_SEEN.get(layout, 0) + int(pad.sum())
    keys = ops.edge_pair_keys(row, col, pad)
    assert keys.dtype == np.uint32 and np.array_equal(keys, ref.pair_keys(row, col, pad))
    # every pad, and only pads and diagonal entries, carries ALWAYS
    assert np.array_equal(keys == ref.ALWAYS, pad | (row == col))
    if name == "row_lengths" and layout != "csr":
        assert np.diff(a.indptr).max() > sc.T_SPLIT          # (split rows: their virtual rows name one output row)


def test_the_grouped_layouts_were_decoded_with_pads_present():
    """(runs behind the cases above) a G = 2 / 4 plan of these patterns pads its bins: the pad branch was exercised."""
    for layout in ("cs2", "cs4"):
        if layout not in PADS_SEEN:
            for name in PATTERNS:
                PADS_SEEN[layout] = PADS_SEEN.get(layout, 0) + int(entries(matrix(name), layout)[2].sum())
        assert PADS_SEEN[layout] > 0, layout


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", PATTERNS)
def test_the_transpose_carries_the_keys_of_the_swapped_pairs(name, layout):
    a = matrix(name)
    at = ops.transpose_host(a)
    row, col, pad, val = entries(at, layout)
    live = ~pad
    keys = ops.edge_pair_keys(row, col, pad)
    # entry (r, c) of A^T is entry (c, r) of A: the same undirected edge, the same key
    assert np.array_equal(keys[live], ref.pair_keys(col[live], row[live]))
    assert np.array_equal(keys == ref.ALWAYS, pad | (row == col))


def test_plan_entries_refuses_what_it_cannot_decode():
    with pytest.raises(ValueError, match="no decode"):
        ops.plan_entries(object())
    with pytest.raises(ValueError, match="tile pointer"):
        ops.cs_entries(np.array([0, 3]), np.zeros(4, np.int32), np.zeros(4, np.float32), np.zeros(16, np.int32), 1)


# ---- statistics --------------------------------------------------------------------------------------------------------
def _random_graph_pairs():
    """The distinct off-diagonal unordered pairs of a random graph of n = 2,000 vertices and m = 24,000 drawn edges, seed 1:
    RandomState(1), the 24,000 row ends drawn first, then the 24,000 column ends -- 23,842 pairs."""
    rng = np.random.RandomState(1)
    i, j = rng.randint(0, 2000, 24000), rng.randint(0, 2000, 24000)
    u, v = np.minimum(i, j), np.maximum(i, j)
    uv = np.unique(np.stack([u, v], axis=1)[u != v], axis=0)
    return uv[:, 0], uv[:, 1]


@pytest.mark.parametrize("keep", [0.5, 0.8, 0.9])
def test_kept_fraction_per_step_and_pooled(keep):
    u, v = _random_graph_pairs()
    n = u.shape[0]
    assert n == 23842
    pair = ref.pair_keys(u, v)
    assert np.array_equal(pair, ops.edge_pair_keys(u, v))
    assert np.unique(pair).shape[0] == n and not np.any(pair == ref.ALWAYS)          # distinct keys, none reserved
    k32 = float(np.float32(keep))
    sigma = np.sqrt(k32 * (1.0 - k32) / n)
    total, worst = 0, 0.0
    for step in range(64):
        key = ref.edge_key(1, step)
        assert key == ops.edge_key(1, step)
        kept = ref.kept(pair, key, keep)
        frac = kept.mean()
        worst = max(worst, abs(frac - k32) / sigma)
        assert abs(frac - k32) <= 5.0 * sigma, (step, frac)
        total += int(kept.sum())
    pooled = total / (64.0 * n)
    print("keep %.1f: worst step %.2f sigma, pooled %.6f (%.2f sigma)" % (keep, worst, pooled, abs(pooled - k32) / (sigma / 8.0)))
    assert abs(pooled - k32) <= 5.0 * sigma / 8.0


def test_mask_is_symmetric_and_the_diagonal_is_always_kept_with_factor_one():
    u, v = _random_graph_pairs()
    assert np.array_equal(ref.pair_keys(u, v), ref.pair_keys(v, u))
    assert np.array_equal(ops.edge_pair_keys(u, v), ops.edge_pair_keys(v, u))
    key = ref.edge_key(1, 3)
    assert np.array_equal(ref.kept(ref.pair_keys(u, v), key, 0.5), ref.kept(ref.pair_keys(v, u), key, 0.5))
    d = np.arange(2000)
    pd = ref.pair_keys(d, d)
    assert np.all(pd == ref.ALWAYS) and np.array_equal(pd, ops.edge_pair_keys(d, d))
    base = np.random.RandomState(0).standard_normal(2000).astype(np.float32)
    base[:3] = [-0.0, np.nan, 0.0]
    for step in range(8):
        for keep in (0.5, 0.8, 0.9):
            assert ref.kept(pd, ref.edge_key(1, step), keep).all()
            assert np.array_equal(ref.revalue(base, pd, ref.edge_key(1, step), keep).view(np.uint32), base.view(np.uint32))


def test_a_dropped_entry_is_plus_zero_and_a_kept_one_is_one_multiply():
    """The restatement held to the contract's wording (what the device is compared against in the GPU tests), on the keys
    the product's own host code gives the pairs."""
    u, v = _random_graph_pairs()
    pair = ops.edge_pair_keys(u, v)
    assert np.array_equal(pair, ref.pair_keys(u, v))
    base = -np.abs(np.random.RandomState(2).standard_normal(pair.shape[0])).astype(np.float32) - np.float32(0.25)
    key = ref.edge_key(7, 11)
    out = ref.revalue(base, pair, key, 0.8)
    k = ref.kept(pair, key, 0.8)
    assert 0 < k.sum() < k.shape[0]
    assert np.all(out.view(np.uint32)[~k] == 0)                                       # +0.0f, never the pad marker
    assert np.array_equal(out[k], base[k] * (np.float32(1.0) / np.float32(0.8)))
    assert np.array_equal(ref.revalue(base, pair, key, 1.0).view(np.uint32), base.view(np.uint32))
    m = ref.masked_matrix(matrix("row_lengths"), key, 0.5)
    a = matrix("row_lengths")
    assert m.nnz == a.nnz and np.array_equal(m.indices, a.indices) and np.array_equal(m.indptr, a.indptr)
    assert 0 < np.count_nonzero(m.data) < a.nnz


# ---- the flag ----------------------------------------------------------------------------------------------------------
def test_flag_parses_and_zero_is_off():
    from stochastic_gcn_amd.full_batch import check_edge_dropout
    f = _Flags()
    assert f.edge_dropout == 0.0 and 'edge_dropout' in f.as_dict()
    assert f.parse(['--edge_dropout', '0']).edge_dropout == 0.0 and check_edge_dropout(f) == 0.0
    f.parse(['--full_batch', '--edge_dropout', '0.2'])
    assert f.edge_dropout == 0.2 and check_edge_dropout(f) == 0.2
    FLAGS.update(edge_dropout=0.0, gradvar=True, full_batch_kernel='lds')               # off: nothing to refuse
    assert check_edge_dropout() == 0.0


@pytest.mark.parametrize("flags,msg", [
    (dict(full_batch=True, edge_dropout=1.0), r"--edge_dropout must lie in \[0, 1\)"),
    (dict(full_batch=True, edge_dropout=-0.1), r"--edge_dropout must lie in \[0, 1\)"),
    (dict(full_batch=True, edge_dropout=1.5), r"--edge_dropout must lie in \[0, 1\)"),
    (dict(full_batch=True, edge_dropout=float('nan')), r"--edge_dropout must lie in \[0, 1\)"),
    (dict(edge_dropout=0.2), "--edge_dropout needs --full_batch"),
    (dict(test_full_batch=True, edge_dropout=0.2), "--edge_dropout needs --full_batch"),
    (dict(full_batch=True, full_batch_kernel='lds', edge_dropout=0.2), "--edge_dropout is not supported with --full_batch_kernel lds"),
    (dict(full_batch=True, gradvar=True, edge_dropout=0.2), "--edge_dropout is not supported with --gradvar"),
])
def test_refusals(flags, msg):
    from stochastic_gcn_amd.full_batch import check_edge_dropout
    FLAGS.update(**flags)
    with pytest.raises(ValueError, match=msg):
        check_edge_dropout()


@pytest.mark.parametrize("flags,msg", [
    (dict(edge_dropout=0.2), "--edge_dropout needs --full_batch"),
    (dict(full_batch=True, edge_dropout=1.0), "--edge_dropout must lie in"),
    (dict(full_batch=True, full_batch_kernel='lds', edge_dropout=0.2), "--full_batch_kernel lds"),
    (dict(full_batch=True, gradvar=True, edge_dropout=0.2), "--gradvar"),
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


def test_static_matrix_refuses_the_lds_sweep_before_planning():
    from stochastic_gcn_amd.full_batch import StaticMatrix
    with pytest.raises(ValueError, match="no value array to re-draw"):
        StaticMatrix(matrix("identity"), torch.device("cpu"), 'lds', edge_dropout=0.2)


# ---- the export ----------------------------------------------------------------------------------------------------------
def test_edge_revalue_validates_before_any_device_call():
    lib, A = _ffi.lib, 4096          # (non-null addresses that are never dereferenced: every call fails validation first)
    assert lib.sgcn_abi_version() == _ffi.ABI_VERSION == 16          # an additive export
    for keep in (0.0, -0.5, 1.5, float('nan'), float('inf')):
        assert lib.sgcn_edge_revalue_f32(A, 2 * A, 8, 1, keep, 3 * A, None) == -1
        assert b"keep must lie in (0, 1]" in lib.sgcn_last_error()
    assert lib.sgcn_edge_revalue_f32(A, 2 * A, -1, 1, 0.5, 3 * A, None) == -1 and b"negative size" in lib.sgcn_last_error()
    for base, pair, out in ((None, A, A), (A, None, 2 * A), (A, 2 * A, None)):
        assert lib.sgcn_edge_revalue_f32(base, pair, 8, 1, 0.5, out, None) == -1 and b"null operand" in lib.sgcn_last_error()
    assert lib.sgcn_edge_revalue_f32(A + 2, 2 * A, 8, 1, 0.5, 3 * A, None) == -1 and b"not aligned" in lib.sgcn_last_error()
    for out in (A, A + 4, A - 28, 2 * A, 2 * A + 28, 2 * A - 4):                      # over base, over the pair keys
        assert lib.sgcn_edge_revalue_f32(A, 2 * A, 8, 1, 0.5, out, None) == -1 and b"must not alias" in lib.sgcn_last_error()
    assert lib.sgcn_edge_revalue_f32(None, None, 0, 1, 0.5, None, None) == 0           # n == 0: nothing to do
    with pytest.raises(RuntimeError, match="HBM"):
        ops.edge_revalue(torch.zeros(4), torch.zeros(4, dtype=torch.int32), 1, 0.5)
