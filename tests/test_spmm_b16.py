"""Host side of the bfloat16 dense operand of the static-graph products (--full_batch_dtype bf16; include/sgcn.h
"bfloat16 dense operand"): the flag and its refusals, the C-ABI table, the per-type sweep clocks in the plan cache, and
the host logic of ShardedSpMM's bfloat16 all-gather on gloo.  None of this needs a device; the kernels are checked in
test_spmm_b16_gpu.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bf16_ref                                     # noqa: E402
from stochastic_gcn_amd import _ffi                 # noqa: E402
from stochastic_gcn_amd.flags import FLAGS          # noqa: E402

NEW = {"sgcn_spmm_csr_b16": "sgcn_spmm_csr_f32", "sgcn_spmm_csr_add_b16": "sgcn_spmm_csr_add_f32",
       "sgcn_spmm_cs_b16": "sgcn_spmm_cs_f32", "sgcn_spmm_cs_variant_b16": "sgcn_spmm_cs_variant"}


@pytest.fixture(autouse=True)
def _flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


# ---- the flag ---------------------------------------------------------------------------------------------------------
def test_flag_parses_and_defaults_to_fp32():
    assert FLAGS.full_batch_dtype == 'fp32'
    FLAGS.parse(['--full_batch', '--full_batch_dtype', 'bf16'])
    assert FLAGS.full_batch_dtype == 'bf16' and FLAGS.full_batch is True
    FLAGS.reset()
    FLAGS.parse(['--full_batch_dtype', 'fp32'])
    assert FLAGS.full_batch_dtype == 'fp32'
    with pytest.raises(SystemExit):
        FLAGS.parser().parse_args(['--full_batch_dtype', 'fp16'])


def test_check_full_batch_accepts_bf16_with_either_mode():
    from stochastic_gcn_amd.full_batch import check_full_batch, full_batch_bf16
    assert full_batch_bf16() is False
    for kw, want in ((dict(full_batch=True), (True, False)), (dict(test_full_batch=True), (False, True)),
                     (dict(full_batch=True, test_full_batch=True), (True, True))):
        for kernel in ('auto', 'rows', 'cs'):
            FLAGS.reset()
            FLAGS.update(full_batch_dtype='bf16', full_batch_kernel=kernel, **kw)
            assert check_full_batch() == want and full_batch_bf16() is True
    FLAGS.reset()
    assert check_full_batch() == (False, False)                 # the default asks for nothing


def test_check_full_batch_refuses_bf16_without_a_full_graph_mode():
    from stochastic_gcn_amd.full_batch import check_full_batch
    FLAGS.update(full_batch_dtype='bf16')
    with pytest.raises(ValueError) as e:
        check_full_batch()
    assert '--full_batch_dtype bf16' in str(e.value) and '--full_batch' in str(e.value) and 'no other mode' in str(e.value)


@pytest.mark.parametrize("mode", ['full_batch', 'test_full_batch'])
def test_check_full_batch_refuses_bf16_with_the_lds_sweep(mode):
    from stochastic_gcn_amd.full_batch import check_full_batch
    FLAGS.update(full_batch_dtype='bf16', full_batch_kernel='lds', **{mode: True})
    with pytest.raises(ValueError) as e:
        check_full_batch()
    assert '--full_batch_kernel lds' in str(e.value) and 'no bfloat16 form' in str(e.value)
    FLAGS.update(full_batch_dtype='fp32')
    check_full_batch()                                          # the LDS sweep itself stays available


def test_check_full_batch_refuses_an_unknown_dtype():
    from stochastic_gcn_amd.full_batch import check_full_batch
    FLAGS.update(full_batch=True, full_batch_dtype='fp16')
    with pytest.raises(ValueError) as e:
        check_full_batch()
    assert 'fp32/bf16' in str(e.value) and "'fp16'" in str(e.value)


def test_static_matrix_refuses_the_lds_sweep_and_keeps_the_width_fallback():
    from stochastic_gcn_amd.full_batch import StaticMatrix
    a = sp.identity(8, dtype=np.float32, format='csr')
    with pytest.raises(ValueError):
        StaticMatrix(a, torch.device('cpu'), 'lds', bf16=True)
    m = StaticMatrix.__new__(StaticMatrix)
    m.kernel, m.bf16 = 'cs', True
    # the operand is read from the scratch table, which is always aligned: its own alignment decides nothing ...
    assert m.kernel_for(torch.zeros(8, 20)[:, 2:18]) == 'cs'
    # ... the width and the output still do
    assert m.kernel_for(torch.zeros(8, 7)) == 'rows'
    assert m.kernel_for(torch.zeros(8, 16), out=torch.zeros(8, 34)[:, 18:]) == 'rows'
    m.bf16 = False
    assert m.kernel_for(torch.zeros(8, 20)[:, 2:18]) == 'rows'


# ---- the C-ABI --------------------------------------------------------------------------------------------------------
def test_new_entries_in_header_library_and_ctypes_table():
    assert _ffi.ABI_VERSION == 16 and _ffi.lib.sgcn_abi_version() == 16
    src = open(os.path.join(ROOT, "include", "sgcn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for new, old in NEW.items():
        assert new in _ffi.SIGNATURES and hasattr(lib, new)
        m_new = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % new, src)
        m_old = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % old, src)
        assert m_new and m_old, new
        norm = lambda s: re.sub(r"\s+", " ", s).strip()           # noqa: E731
        # the fp32 entry's argument list, the operand a uint16 pointer
        assert norm(m_new.group(1)) == norm(m_old.group(1)).replace("const float* dev_B", "const uint16_t* dev_B"), new
        assert _ffi.SIGNATURES[new][0] is _ffi.SIGNATURES[old][0]
        assert len(_ffi.SIGNATURES[new][1]) == len(_ffi.SIGNATURES[old][1])
        assert all(x is y for x, y in zip(_ffi.SIGNATURES[new][1], _ffi.SIGNATURES[old][1])), new


def test_refusals_need_no_device():
    """The layout checks come first: a table with ldb % 8 != 0, ldb < d or a misaligned base is SGCN_ERR_INVALID with a
    message, before any pointer is read (host memory stands in for the operands)."""
    lib = _ffi.lib
    rowptr = np.zeros(5, np.int32)
    C = np.zeros((4, 16), np.float32)
    B = np.zeros(64 + 8, np.uint16)
    base = B.ctypes.data + (-B.ctypes.data) % 16
    for ldb, ptr, d, frag in ((12, base, 8, b"ldb % 8"), (8, base, 12, b"leading dimension"), (16, base + 2, 8, b"16-byte aligned")):
        rc = lib.sgcn_spmm_csr_b16(rowptr.ctypes.data, None, None, 4, 4, d, ptr, ldb, None, None, None, C.ctypes.data, 16, 0.0,
                                   None, None)
        assert rc != 0 and frag in lib.sgcn_last_error(), (ldb, d, lib.sgcn_last_error())


# ---- the plan cache ---------------------------------------------------------------------------------------------------
def _plan(G=2):
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(3)
    a = sp.random(300, 300, density=0.05, format='csr', dtype=np.float32, random_state=rng)
    a.sort_indices()
    return a, ops.ColumnSweepCSR(a, torch.device('cpu'), G=G)


def test_struct_takes_the_clock_of_the_operand_type():
    a, A = _plan()
    assert A.pace == {} and A.pace_b16 == {} and A.tuned_ms_b16 == {} and A._guard_b16 == {}
    A.pace[64], A.pace_b16[64] = 250, 140
    assert A.struct(64).pace_ns_per_nnz == 250 and A.struct(64, bf16=True).pace_ns_per_nnz == 140
    assert A.struct(128, bf16=True).pace_ns_per_nnz == 0 and A.pace == {64: 250}          # the types never mix
    assert "[bf16 operand]" in A.variant(64, bf16=True) and "bf16" not in A.variant(64)
    assert A.variant(64, bf16=True).replace(" [bf16 operand]", "") == A.variant(64)


@pytest.mark.parametrize("G", [1, 2])
def test_plan_cache_round_trips_bf16_paces_apart_from_the_fp32_ones(tmp_path, G):
    from stochastic_gcn_amd import ops
    a, A = _plan(G)
    key = ops.ColumnSweepCSR.matrix_key(a)
    A.pace[64], A.tuned_ms[64] = 250, 1.5
    A.pace_b16[64], A.tuned_ms_b16[64] = 140, 0.9
    A.pace_b16[128] = -1                                       # unpaced: kept without a time, as for fp32
    A.pace_b16[32] = 99                                        # a pace without its time is not restored (the guard could not watch it)
    path = str(tmp_path / "plan.npz")
    A.save(path, key)
    z = np.load(path)
    assert {"pace", "tuned_ms", "pace_b16", "tuned_ms_b16"} <= set(z.files)
    B = ops.ColumnSweepCSR.load(path, torch.device('cpu'), key, g=G)
    assert B is not None and B.pace == {64: 250} and B.tuned_ms == {64: 1.5}
    assert B.pace_b16 == {64: 140, 128: -1} and B.tuned_ms_b16 == {64: 0.9} and B._guard_b16 == {}
    assert B.struct(64).pace_ns_per_nnz == 250 and B.struct(64, bf16=True).pace_ns_per_nnz == 140


def test_a_cache_with_only_the_parents_keys_loads_with_empty_bf16_state(tmp_path):
    from stochastic_gcn_amd import ops
    a, A = _plan()
    key = ops.ColumnSweepCSR.matrix_key(a)
    A.pace[64], A.tuned_ms[64] = 250, 1.5
    A.pace_b16[64], A.tuned_ms_b16[64] = 140, 0.9
    path = str(tmp_path / "plan.npz")
    A.save(path, key)
    z = dict(np.load(path))
    parent_keys = {"key", "G", "pad_fraction", "R", "shape", "nslots", "round_tiles", "tile_ptr", "colrow", "val", "tile_rows",
                   "tile_slots", "fix", "pace", "tuned_ms", "warp", "warp_shift"}
    assert set(z) - parent_keys == {"pace_b16", "tuned_ms_b16"}              # nothing else is new in the file
    old = str(tmp_path / "old.npz")
    np.savez(old, **{k: v for k, v in z.items() if k in parent_keys})
    B = ops.ColumnSweepCSR.load(old, torch.device('cpu'), key, g=2)
    assert B is not None and B.pace == {64: 250} and B.tuned_ms == {64: 1.5}
    assert B.pace_b16 == {} and B.tuned_ms_b16 == {} and B.struct(64, bf16=True).pace_ns_per_nnz == 0
    # and what the fp32 path reads from a file of this build is what it reads from the parent's
    C = ops.ColumnSweepCSR.load(path, torch.device('cpu'), key, g=2)
    for k in ("tile_ptr", "colrow", "val", "tile_rows", "tile_slots"):
        assert torch.equal(getattr(B, k), getattr(C, k))
    assert (B.pace, B.tuned_ms, B.G, B.shape) == (C.pace, C.tuned_ms, C.G, C.shape)


# ---- the bfloat16 all-gather on gloo ------------------------------------------------------------------------------------
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _matrix(n):
    """a skewed square pattern, so that the load-balanced row blocks are ragged"""
    rng = np.random.RandomState(5)
    deg = np.maximum(1, (rng.pareto(1.2, n) * 3).astype(np.int64)).clip(max=n // 2)
    rows = np.repeat(np.arange(n), deg)
    cols = rng.randint(0, n, rows.shape[0])
    a = sp.csr_matrix((np.ones(rows.shape[0], np.float32), (rows, cols)), shape=(n, n))
    a.sum_duplicates()
    a.sort_indices()
    return a


N_ROWS, WIDTHS = 257, (5, 8, 70)


def _operand(d):
    x = bf16_ref.wide_values(N_ROWS * d - len(bf16_ref.SPECIALS), seed=d).astype(np.float32)
    return np.random.RandomState(d).permutation(x).reshape(N_ROWS, d)


def _gather_worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from stochastic_gcn_amd.parallel import DataParallel, ShardedSpMM
    par = DataParallel(backend="gloo", device=torch.device("cpu"))
    try:
        sh = ShardedSpMM(par, _matrix(N_ROWS), torch.device("cpu"), kernel=None)
        res = dict(lo=np.array([sh.lo]), hi=np.array([sh.hi]), counts=np.array(sh.row_counts))
        for d in WIDTHS:
            X = torch.from_numpy(_operand(d))
            got = sh.allgather_rows(X[sh.lo:sh.hi].contiguous(), bf16=True)
            assert got.dtype == torch.bfloat16 and tuple(got.shape) == (N_ROWS, d)
            res["bits%d" % d] = got.contiguous().view(torch.int16).numpy().view(np.uint16)
            res["pitch%d" % d] = np.array([got.stride(0), got.data_ptr() % 16])
            f = sh.allgather_rows(X[sh.lo:sh.hi].contiguous())                 # the default is unchanged: fp32
            assert f.dtype == torch.float32
            res["f%d" % d] = f.contiguous().numpy()
        np.savez(os.path.join(out_dir, "r%d.npz" % rank), **res)
    finally:
        par.shutdown()


@pytest.mark.parametrize("world", [2, 8])
def test_bf16_allgather_moves_the_rounded_blocks(tmp_path, world):
    """Every rank rounds its own (ragged) block; what arrives on every rank is round_bits of the whole operand at a pitch
    of 8 * ceil(d / 8) elements on a 16-byte aligned base -- also for values that are not finite."""
    mp.spawn(_gather_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r = [np.load(os.path.join(str(tmp_path), "r%d.npz" % k)) for k in range(world)]
    counts = r[0]["counts"]
    assert counts.sum() == N_ROWS and len(set(counts.tolist())) > 1, "the blocks of this matrix must be ragged"
    assert [int(x["lo"][0]) for x in r] == np.concatenate([[0], np.cumsum(counts)[:-1]]).tolist()
    for d in WIDTHS:
        X = _operand(d)
        want = bf16_ref.round_bits(X)
        nan = np.isnan(X)
        for k in range(world):
            got = r[k]["bits%d" % d]
            assert np.array_equal(got[~nan], want[~nan]), (world, d, k)
            assert np.isnan(bf16_ref.widen_bits(got[nan])).all()
            assert r[k]["pitch%d" % d].tolist() == [(d + 7) // 8 * 8, 0]
            assert np.array_equal(r[k]["f%d" % d].view(np.uint32), X.view(np.uint32))


def test_round_rows_on_the_host_is_the_contracts_rounding():
    from stochastic_gcn_amd.parallel import ShardedSpMM
    x = np.concatenate([bf16_ref.wide_values(5000, seed=1), [np.nan, -np.nan]]).astype(np.float32)
    x = x[:x.shape[0] // 7 * 7].reshape(-1, 7)
    out = torch.zeros((x.shape[0], 8), dtype=torch.bfloat16)
    ShardedSpMM.round_rows(torch.from_numpy(x), out[:, :7])
    got = out.view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(x)
    assert np.array_equal(got[:, :7][~nan], bf16_ref.round_bits(x)[~nan]) and (got[:, 7] == 0).all()
    assert np.isnan(bf16_ref.widen_bits(got[:, :7][nan])).all()


def test_single_process_allgather_is_the_rounded_operand():
    from stochastic_gcn_amd.parallel import DataParallel, ShardedSpMM
    par = DataParallel(init=False)
    sh = ShardedSpMM(par, _matrix(N_ROWS), torch.device("cpu"), kernel=None)
    X = _operand(70)
    got = sh.allgather_rows(torch.from_numpy(X), bf16=True)
    assert got.stride(0) == 72 and np.array_equal(got.contiguous().view(torch.int16).numpy().view(np.uint16)[~np.isnan(X)],
                                                  bf16_ref.round_bits(X)[~np.isnan(X)])
