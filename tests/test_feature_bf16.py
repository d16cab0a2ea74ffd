"""CPU tests of --feature_dtype bf16: the flag, its three refusals, the per-model rule as a function of the flags, what
StaticMatrix does with an operand that is bfloat16 already, and the additive export.  Nothing here touches a device."""
import ctypes
import os
import re

import pytest
import torch

from stochastic_gcn_amd import _ffi
from stochastic_gcn_amd.flags import FLAGS, _Flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _reset_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


# ---- the flag ------------------------------------------------------------------------------------------------------------
def test_flag_default_and_parsing():
    f = _Flags()
    assert f.feature_dtype == 'fp32' and 'feature_dtype' in f.as_dict()
    assert f.parse(['--feature_dtype=bf16']).feature_dtype == 'bf16'
    assert f.parse(['--feature_dtype', 'fp32']).feature_dtype == 'fp32'
    with pytest.raises(SystemExit):
        f.parse(['--feature_dtype', 'fp16'])


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refuses_an_unknown_value():
    from stochastic_gcn_amd.full_batch import check_feature_dtype
    FLAGS.update(full_batch=True, dense_dtype='bf16', feature_dtype='fp16')
    with pytest.raises(ValueError, match="--feature_dtype must be one of fp32/bf16, got 'fp16'"):
        check_feature_dtype()


@pytest.mark.parametrize("modes", [dict(full_batch=True), dict(test_full_batch=True), dict(full_batch=True, test_full_batch=True)])
def test_refuses_bf16_without_the_bf16_gemms(modes):
    from stochastic_gcn_amd.full_batch import check_feature_dtype
    FLAGS.update(feature_dtype='bf16', **modes)
    with pytest.raises(ValueError, match="--feature_dtype bf16 needs --dense_dtype bf16: only the bf16-multiply GEMM reads a "
                                         "bfloat16 feature table"):
        check_feature_dtype()


def test_refuses_bf16_without_a_full_graph_mode():
    from stochastic_gcn_amd.full_batch import check_feature_dtype
    f = _Flags()
    f.update(feature_dtype='bf16', dense_dtype='bf16')
    with pytest.raises(ValueError, match="--feature_dtype bf16 needs --full_batch or --test_full_batch"):
        check_feature_dtype(f)


def test_existing_refusals_stay():
    """check_full_batch is not touched: bf16 operands on the LDS sweep stay refused whatever --feature_dtype says."""
    from stochastic_gcn_amd.full_batch import check_full_batch
    FLAGS.update(full_batch=True, dense_dtype='bf16', feature_dtype='bf16', full_batch_dtype='bf16', full_batch_kernel='lds')
    with pytest.raises(ValueError, match="--full_batch_dtype bf16 is not supported with --full_batch_kernel lds"):
        check_full_batch()


def test_trainer_refuses_before_a_device_is_touched(monkeypatch):
    from stochastic_gcn_amd import train
    touched = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: touched.append("is_available") or False)
    monkeypatch.setattr(train, "load_data", lambda *a, **k: touched.append("load_data"))
    FLAGS.update(full_batch=True, feature_dtype='bf16')
    with pytest.raises(ValueError, match="--feature_dtype bf16 needs --dense_dtype bf16"):
        train.Trainer(verbose=False)
    assert touched == []


# ---- the per-model rule -----------------------------------------------------------------------------------------------------
RULE = [
    # flags                                                                   (train table bf16?, test table bf16?)
    (dict(full_batch=True, test_full_batch=True), (True, True)),
    (dict(cv=True, cvd=True, test_full_batch=True), (False, True)),            # the sampled training model keeps fp32
    (dict(full_batch=True), (True, False)),                                     # the sampled evaluation model keeps fp32
    (dict(test_full_batch=True), (False, True)),
    (dict(full_batch=True, test_cv=True), (True, False)),
]


@pytest.mark.parametrize("flags,want", RULE)
def test_rule_is_per_model(flags, want):
    from stochastic_gcn_amd.full_batch import check_feature_dtype, check_full_batch
    FLAGS.update(dense_dtype='bf16', feature_dtype='bf16', **flags)
    check_full_batch()                                  # (an accepted combination of the existing flags)
    assert check_feature_dtype() == want
    FLAGS.update(feature_dtype='fp32')
    assert check_feature_dtype() == (False, False)


@pytest.mark.parametrize("extra", [dict(full_batch_dtype='bf16'), dict(full_batch_kernel='cs'), dict(full_batch_kernel='lds'),
                                   dict(preprocess=False, test_preprocess=False), dict(history_dtype='bf16')])
def test_accepted_combinations(extra):
    from stochastic_gcn_amd.full_batch import check_feature_dtype, check_full_batch
    FLAGS.update(full_batch=True, test_full_batch=True, dense_dtype='bf16', feature_dtype='bf16', **extra)
    assert check_full_batch() == (True, True) and check_feature_dtype() == (True, True)


def test_default_needs_nothing():
    from stochastic_gcn_amd.full_batch import check_feature_dtype
    assert check_feature_dtype() == (False, False)
    FLAGS.update(cv=True, cvd=True)
    assert check_feature_dtype() == (False, False)


# ---- StaticMatrix and an operand that is bfloat16 already ----------------------------------------------------------------------
def _matrix(kernel, bf16, n=12):
    from stochastic_gcn_amd.full_batch import StaticMatrix
    m = StaticMatrix.__new__(StaticMatrix)
    m.kernel, m.bf16, m.shape, m._scratch, m._widened = kernel, bf16, (n, n), {}, {}
    return m


@pytest.fixture
def recorded(monkeypatch):
    """Recorders in place of the two kernels an operand may pass through."""
    from stochastic_gcn_amd import ops
    log = []

    def operand_round(x, out=None):
        log.append(('operand_round', tuple(x.shape), x.dtype))
        return out

    def history_widen(H, out=None):
        log.append(('history_widen', tuple(H.shape), H.dtype, tuple(out.shape), out.dtype, tuple(out.stride())))
        return out
    monkeypatch.setattr(ops, "operand_round", operand_round)
    monkeypatch.setattr(ops, "history_widen", history_widen)
    monkeypatch.setattr(ops, "history_alloc", lambda n, d, dev, bf16=False: torch.zeros((n, (d + 7) // 8 * 8), dtype=torch.bfloat16)[:, :d])
    return log


@pytest.mark.parametrize("kernel", ['rows', 'cs'])
@pytest.mark.parametrize("bf16", [False, True])
def test_operand_hands_a_bf16_table_through(recorded, kernel, bf16):
    m = _matrix(kernel, bf16)
    x = torch.zeros((12, 24), dtype=torch.bfloat16)[:, :20]
    assert m.operand(x) is x
    assert recorded == [] and m._scratch == {} and m._widened == {}
    with pytest.raises(ValueError, match="the operand has 11 rows, the matrix 12 columns"):
        m.operand(x[:11])
    # an fp32 operand is treated as before: rounded under ``bf16``, itself otherwise
    y = torch.zeros((12, 20))
    got = m.operand(y)
    if bf16:
        assert recorded == [('operand_round', (12, 20), torch.float32)] and got is m._scratch[20] and got.dtype == torch.bfloat16
    else:
        assert recorded == [] and got is y


def test_operand_widens_on_an_lds_matrix(recorded, capsys):
    m = _matrix('lds', False)
    x = torch.zeros((12, 24), dtype=torch.bfloat16)[:, :20]
    got = m.operand(x)
    assert capsys.readouterr().out.count("[sgcn] the LDS-staged sweep has no bfloat16-operand form") == 1
    assert recorded == [('history_widen', (12, 20), torch.bfloat16, (12, 20), torch.float32, (20, 1))]
    assert got is m._widened[20] and got.dtype == torch.float32 and m._scratch == {}
    assert m.operand(x) is got and len(recorded) == 2                  # one scratch table per width, reused
    assert m.operand(x, 'lds') is got and len(recorded) == 3
    assert m.operand(x, 'rows') is x and len(recorded) == 3            # a product that fell back to the row kernel reads the table
    assert m.kernel_for(x) == 'lds'
    y = torch.zeros((12, 20))
    assert m.operand(y) is y and len(recorded) == 3
    assert capsys.readouterr().out == ""                               # said once per width, not per product


def test_kernel_for_decides_on_width_and_out_only():
    """A bfloat16 x is a pitch-8 table: as under ``bf16``, its own alignment is not looked at."""
    m = _matrix('cs', False)
    tab = torch.zeros((12, 24), dtype=torch.bfloat16)
    assert m.kernel_for(tab[:, :20]) == 'cs' and m.kernel_for(tab) == 'cs'
    assert m.kernel_for(tab[:, :22]) == 'rows'                                      # a width that is no multiple of 4
    assert m.kernel_for(tab[:, :20], out=torch.zeros(12, 40)[:, 20:]) == 'cs'
    assert m.kernel_for(tab[:, :20], out=torch.zeros(12, 42)[:, 22:]) == 'rows'
    assert m.kernel_for(torch.zeros(12, 24)[:, 2:22]) == 'rows'                     # fp32: as before
    assert _matrix('rows', False).kernel_for(tab[:, :20]) == 'rows'


def test_tuning_is_per_width_and_operand_type():
    from stochastic_gcn_amd.full_batch import StaticMatrix
    log = []

    class Clock(object):
        def __init__(self):
            self.pace = {}

    class Plan(object):
        shape = (12, 12)
        clocks = {False: Clock(), True: Clock()}

        def clock(self, bf16=False):
            return self.clocks[bool(bf16)]

        def autotune(self, x, d=None):
            log.append((d, x.dtype))
            self.clock(x.dtype == torch.bfloat16).pace[d] = 1

        def store_if_cached(self):
            pass
    m = StaticMatrix.__new__(StaticMatrix)
    m.kernel, m._plan, m._tuned = 'cs', Plan(), set()
    a, b = torch.zeros(12, 8), torch.zeros((12, 8), dtype=torch.bfloat16)
    for x in (a, b, a, b):
        m._autotune(x, 8)
    assert log == [(8, torch.float32), (8, torch.bfloat16)]


# ---- ops.gemm_bf16: only A may be a bfloat16 table -------------------------------------------------------------------------
def test_gemm_bf16_refuses_a_bf16_b_or_out():
    from stochastic_gcn_amd import ops
    a, b, o = torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(4, 4)
    with pytest.raises(TypeError, match="B must be torch.float32"):
        ops.gemm_bf16(a, b.to(torch.bfloat16), out=o)
    with pytest.raises(TypeError, match="out must be torch.float32"):
        ops.gemm_bf16(a, b, out=o.to(torch.bfloat16))
    with pytest.raises(RuntimeError, match="no CPU fallback|HBM"):                   # a bfloat16 A gets as far as the device check
        ops.gemm_bf16(a.to(torch.bfloat16), b, out=o)


# ---- the export ------------------------------------------------------------------------------------------------------------
def test_export_agrees_in_header_library_and_ctypes_table():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgcn.h")).read(), flags=re.S)
    decl = {}
    for s in ("sgcn_gemm_mb16_f32", "sgcn_gemm_mb16_a16"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, src)
        assert m, "%s is not declared in include/sgcn.h" % s
        decl[s] = [" ".join(a.split()) for a in m.group(1).split(",")]
    # the f32 entry's argument list with a bfloat16 A
    assert decl["sgcn_gemm_mb16_a16"] == [a.replace("const float* dev_A", "const uint16_t* dev_A") for a in decl["sgcn_gemm_mb16_f32"]]
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), "sgcn_gemm_mb16_a16")
    assert _ffi.SIGNATURES["sgcn_gemm_mb16_a16"] == _ffi.SIGNATURES["sgcn_gemm_mb16_f32"]
    assert _ffi.lib.sgcn_abi_version() == _ffi.ABI_VERSION == 16           # additive: the version stays


def test_export_validates_before_any_hip_call():
    one = ctypes.c_void_p(16)               # never dereferenced: validation comes first
    fn = _ffi.lib.sgcn_gemm_mb16_a16
    assert fn(0, 1, 8, 8, 8, one, 8, one, 8, one, 8, 0, None, None, None, None) == -1
    assert b"NT form" in _ffi.lib.sgcn_last_error() and b"gemm_mb16_a16" in _ffi.lib.sgcn_last_error()
    assert fn(1, 1, 8, 8, 8, one, 8, one, 8, one, 8, 0, None, None, None, None) == -1
    assert b"(1, 1)" in _ffi.lib.sgcn_last_error()
    assert fn(0, 0, 8, 8, 8, None, 8, one, 8, one, 8, 0, None, None, None, None) == -1
    assert b"null operand" in _ffi.lib.sgcn_last_error()
    assert fn(0, 0, 8, 8, 8, ctypes.c_void_p(17), 8, one, 8, one, 8, 0, None, None, None, None) == -1
    assert b"2-byte aligned" in _ffi.lib.sgcn_last_error()
    assert fn(0, 0, 0, 8, 8, None, 8, None, 8, None, 8, 0, None, None, None, None) == 0       # M = 0: nothing to do
