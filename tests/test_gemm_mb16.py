"""Host side of the bf16-multiply GEMM (sgcn_gemm_mb16_f32, ops.gemm_bf16, --dense_dtype bf16): the launch plan restated
in tests/mb16_cases.py against the library's own workspace size, the coverage of the case catalogue, the flag and its
refusals, the C-ABI table, and the refusals the entry point makes before any HIP call.  None of this needs a device; the
kernel is checked in test_gemm_mb16_gpu.py and the layer wiring in test_dense_bf16_gpu.py."""
import contextlib
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mb16_cases as mbc                            # noqa: E402
from stochastic_gcn_amd import _ffi                 # noqa: E402
from stochastic_gcn_amd.flags import FLAGS          # noqa: E402


@pytest.fixture(autouse=True)
def _flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


@contextlib.contextmanager
def knob(value):
    old = int(_ffi.lib.sgcn_tune_get(b"gemm_mb16_slice_k"))
    assert _ffi.lib.sgcn_tune(b"gemm_mb16_slice_k", int(value)) == 0
    try:
        yield
    finally:
        _ffi.lib.sgcn_tune(b"gemm_mb16_slice_k", old)


# ---- the plan ---------------------------------------------------------------------------------------------------------
def test_ws_floats_is_the_librarys_over_shapes_and_knobs():
    assert int(_ffi.lib.sgcn_tune_get(b"gemm_mb16_slice_k")) == 0
    assert _ffi.lib.sgcn_tune(b"gemm_mb16_slice_k", -1) == -1
    sizes = (0, 1, 3, 33, 127, 128, 129, 300, 1204, 5000)
    ks = (0, 1, 33, 63, 64, 127, 128, 602, 1204, 2047, 2048, 4095, 4096, 4097, 70001, 232965)
    for k_ in mbc.KNOBS + (1, 2047, 2049):
        with knob(k_):
            for ta, tb in mbc.FORMS.values():
                for M in sizes:
                    for N in sizes:
                        for K in ks:
                            got = int(_ffi.lib.sgcn_gemm_mb16_ws_floats(int(ta), int(tb), M, N, K))
                            assert got == mbc.ws_floats(ta, tb, M, N, K, k_), (ta, tb, M, N, K, k_)


def test_the_knob_splits_a_few_thousand_k_unevenly_and_the_default_suits_the_full_graph():
    p = mbc.plan(300, 128, 4097, True, False, slice_k=mbc.TN_KNOB)
    assert p["S"] == 4 and p["kchunk"] == 1056 and p["last"] == 929
    p = mbc.plan(41, 130, 70001, True, False, slice_k=mbc.TN_KNOB)
    assert p["S"] == 67 and 0 < p["last"] < p["kchunk"]
    # the weight gradients of the 233 k-row graph: ten tiles -> 51 slices; the forward and the input gradient: never split
    p = mbc.plan(1204, 128, 232965, True, False)
    assert p["grid"][:2] == (10, 1) and p["S"] == 51 and p["kchunk"] >= mbc.DEFAULT_SLICE_K
    assert mbc.plan(232965, 128, 1204)["S"] == 1 and mbc.plan(232965, 1204, 128, False, True)["S"] == 1
    assert mbc.plan(300, 128, 4097, True, False, slice_k=mbc.TN_KNOB, drop_c=True)["S"] == 1       # an output mask: no split


def test_every_reachable_cell_has_a_case():
    cells = mbc.reachable()
    have = {mbc.case_cell(c) for c in mbc.CASES}
    assert cells <= have, sorted(cells - have)
    # both kinds of split and all three forms are reachable, and an output mask is never split
    for form in mbc.FORMS:
        assert {c[1] for c in cells if c[0] == form} == {False, True}
    assert not [c for c in cells if c[1] and c[5] == "c"]
    # vector and scalar loads on either operand, in every form
    for form in mbc.FORMS:
        assert {(c[2], c[3]) for c in cells if c[0] == form} == {(a, b) for a in (False, True) for b in (False, True)}
    # the shape pools are all used
    for key, pool in (("M", mbc.POOL_MN[:8]), ("N", mbc.POOL_MN[:8])):
        assert set(pool) <= {c[key] for c in mbc.CASES}, key
    assert {4097, 70001} <= {c["K"] for c in mbc.CASES if c["form"] == "TN"}
    for c in mbc.CASES:
        if c["form"] == "TN" and c["K"] == 4097 and mbc.case_cell(c)[1]:
            ta, tb = mbc.FORMS["TN"]
            p = mbc.plan(c["M"], c["N"], c["K"], ta, tb, slice_k=c["knob"])
            assert p["S"] >= 3 and p["last"] != p["kchunk"]


def test_exact_operands_satisfy_the_precondition_at_the_longest_k():
    import numpy as np
    import dense_cases as dc
    r = mbc.int_range(70001)
    A, B = np.full((70001, 2), float(r), np.float32), np.full((70001, 2), float(r), np.float32)
    dc.gemm_exact(A, B, True, False, np.full((2, 2), 8.0), True, mask_a=np.ones_like(A, np.float64), scale_a=dc.f32_scale(0.8))


# ---- the flag ---------------------------------------------------------------------------------------------------------
def test_flag_parses_and_defaults_to_fp32():
    from stochastic_gcn_amd.full_batch import dense_bf16
    assert FLAGS.dense_dtype == 'fp32' and dense_bf16() is False
    FLAGS.parse(['--full_batch', '--dense_dtype', 'bf16'])
    assert FLAGS.dense_dtype == 'bf16' and dense_bf16() is True and FLAGS.full_batch_dtype == 'fp32'
    FLAGS.reset()
    with pytest.raises(SystemExit):
        FLAGS.parser().parse_args(['--dense_dtype', 'fp16'])


def test_check_full_batch_accepts_bf16_with_either_mode_and_either_operand_type():
    from stochastic_gcn_amd.full_batch import check_full_batch
    for kw, want in ((dict(full_batch=True), (True, False)), (dict(test_full_batch=True), (False, True)),
                     (dict(cv=True, cvd=True, test_full_batch=True), (False, True))):
        for fbd in ('fp32', 'bf16'):
            FLAGS.reset()
            FLAGS.update(dense_dtype='bf16', full_batch_dtype=fbd, **kw)
            assert check_full_batch() == want


def test_check_full_batch_refuses_bf16_without_a_full_graph_mode():
    from stochastic_gcn_amd.full_batch import check_full_batch
    FLAGS.update(dense_dtype='bf16')
    with pytest.raises(ValueError) as e:
        check_full_batch()
    assert '--dense_dtype bf16' in str(e.value) and '--full_batch' in str(e.value) and '--test_full_batch' in str(e.value)


def test_check_full_batch_refuses_an_unknown_dense_dtype_and_reads_the_flag_with_a_default():
    from stochastic_gcn_amd.full_batch import check_full_batch
    FLAGS.update(full_batch=True, dense_dtype='fp16')
    with pytest.raises(ValueError) as e:
        check_full_batch()
    assert 'fp32/bf16' in str(e.value) and "'fp16'" in str(e.value)

    class Old(object):          # a flag object from before the flag existed
        full_batch, test_full_batch, full_batch_kernel = True, False, 'auto'
        cv = cvd = importance = det_dropout = gradvar = False
    assert check_full_batch(Old()) == (True, False)


# ---- the C-ABI --------------------------------------------------------------------------------------------------------
def test_header_exports_and_ctypes_table_agree():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgcn.h")).read(), flags=re.S)
    for name, twin in (("sgcn_gemm_mb16_f32", "sgcn_gemm_f32"),):
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(_ffi.lib, name)
        assert _ffi.SIGNATURES[name] == _ffi.SIGNATURES[twin]          # the fp32 entry's argument list
    assert re.search(r"\bsgcn_gemm_mb16_ws_floats\s*\(", src)
    res, args = _ffi.SIGNATURES["sgcn_gemm_mb16_ws_floats"]
    assert len(args) == 5 and res is _ffi.SIGNATURES["sgcn_gemm_ws_floats"][0]
    assert _ffi.lib.sgcn_abi_version() == _ffi.ABI_VERSION == 16


def test_entry_refuses_before_any_hip_call():
    lib = _ffi.lib
    assert lib.sgcn_gemm_mb16_f32(1, 1, 4, 4, 4, 16, 4, 16, 4, 16, 4, 0, None, None, None, None) == -1
    assert b"(1, 1)" in lib.sgcn_last_error()
    assert lib.sgcn_gemm_mb16_f32(0, 0, 4, 4, 4, None, 4, None, 4, None, 4, 0, None, None, None, None) == -1
    assert b"null operand" in lib.sgcn_last_error()
    assert lib.sgcn_gemm_mb16_f32(0, 0, -1, 4, 4, None, 4, None, 4, None, 4, 0, None, None, None, None) == -1
    assert lib.sgcn_gemm_mb16_f32(0, 0, 0, 4, 4, None, 4, None, 4, None, 4, 0, None, None, None, None) == 0     # M = 0: nothing to do
    d = _ffi.Dropout(1, 0.5, -1, 5)
    import ctypes
    assert lib.sgcn_gemm_mb16_f32(0, 0, 4, 4, 4, 16, 4, 16, 4, 16, 4, 0, None, ctypes.byref(d), None, None) == -1
    assert b"drop_a width" in lib.sgcn_last_error()


def test_ops_gemm_bf16_refuses_cpu_tensors_and_bad_shapes():
    import torch
    from stochastic_gcn_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback|HBM"):
        ops.gemm_bf16(torch.zeros(4, 8), torch.zeros(8, 4))
