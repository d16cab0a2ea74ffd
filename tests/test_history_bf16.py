"""--history_dtype bf16 without a GPU: the rounding reference against torch, the flag, and the argument checks of the
new entry points (made before any HIP call)."""
import ctypes

import numpy as np
import pytest
import torch

from stochastic_gcn_amd import _ffi
from stochastic_gcn_amd.flags import FLAGS, check_history_dtype

import bf16_ref

lib = _ffi.lib


def test_numpy_rounding_reference_equals_torch_bit_for_bit():
    x = bf16_ref.wide_values(1 << 20)
    assert x.size >= (1 << 20) + len(bf16_ref.SPECIALS)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = bf16_ref.round_bits(x)
    assert np.array_equal(got, want)
    back = bf16_ref.widen_bits(got)
    assert np.array_equal(back, torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy(), equal_nan=True)
    fin = np.isfinite(back) & (np.abs(x) > 1e-30)
    rel = np.abs(back[fin].astype(np.float64) - x[fin]) / np.abs(x[fin].astype(np.float64))
    assert rel.max() <= 2.0 ** -8
    s = dict(zip(range(len(bf16_ref.SPECIALS)), bf16_ref.round_trip(bf16_ref.SPECIALS)))
    assert s[0] == 0 and not np.signbit(s[0]) and s[1] == 0 and np.signbit(s[1])
    assert s[2] == np.inf and s[3] == -np.inf and s[4] == 1.0
    assert s[5] == 1.0                               # a tie: to even = down
    assert s[6] == np.float32(1.0 + 2.0 ** -6)       # a tie: up
    assert s[7] == np.float32(3.3895314e38)          # the largest bfloat16 stays
    assert s[8] == np.inf
    assert bf16_ref.round_bits(np.float32(1e-40)) == 1 and s[9] > 0         # subnormal (0x000116C2): rounded, not flushed
    assert s[10] == 0 and np.signbit(s[10])          # the smallest subnormal rounds to -0
    assert s[11] == 65280.0
    assert np.isnan(bf16_ref.round_trip(np.array([np.nan, -np.nan], np.float32))).all()
    # a NaN whose payload sits in the low 16 bits only must not become inf
    sneaky = np.array([0x7F800001, 0xFF80FFFF, 0x7FFFFFFF], np.uint32).view(np.float32)
    assert np.isnan(bf16_ref.round_trip(sneaky)).all()


def test_flag_default_choices_and_reset():
    FLAGS.reset()
    assert FLAGS.history_dtype == 'fp32'
    try:
        FLAGS.parse(['--history_dtype', 'bf16'])
        assert FLAGS.history_dtype == 'bf16' and check_history_dtype() is True
        FLAGS.reset()
        assert FLAGS.history_dtype == 'fp32' and check_history_dtype() is False
        with pytest.raises(SystemExit):
            FLAGS.parse(['--history_dtype', 'fp16'])
        assert FLAGS.parse([]).history_dtype == 'fp32'
        with pytest.raises(ValueError, match="history_dtype"):
            check_history_dtype('fp16', False)
    finally:
        FLAGS.reset()


def test_bf16_history_with_det_dropout_is_refused_without_a_device():
    FLAGS.reset()
    try:
        with pytest.raises(ValueError) as e:
            check_history_dtype('bf16', True)
        assert '--history_dtype' in str(e.value) and '--det_dropout' in str(e.value)
        FLAGS.update(history_dtype='bf16', det_dropout=True)
        with pytest.raises(ValueError, match="det_dropout"):
            check_history_dtype()
        assert check_history_dtype('fp32', True) is False and check_history_dtype('bf16', False) is True
    finally:
        FLAGS.reset()


# every new export as (name, call(table address, ldh, n, d)): all other pointers are dummies that validation must not
# dereference -- a launch is never reached (n == 0 returns first, everything else is refused)
_X = 0x1000       # a non-null, 16-byte aligned address that is never read


def _agg(H, ldh, n, d):
    return lib.sgcn_vr_aggregate_h16(_X, _X, _X, _X, _X, _X, n, max(n, 0), max(n, 0), d, _X, _X, max(d, 1), H, ldh, _X, _X, _X,
                                     _X, _X, 2 * max(d, 1), 1, 1, None, None)


def _pre(H, ldh, n, d):
    return lib.sgcn_vr_aggregate_pre_h16(_X, _X, _X, n, max(n, 0), d, H, ldh, _X, _X, None, None)


def _post(H, ldh, n, d):
    return lib.sgcn_vr_aggregate_post_h16(_X, _X, _X, n, max(n, 0), d, _X, _X, max(d, 1), H, ldh, _X, _X, _X, _X,
                                          2 * max(d, 1), 1, 1, _X, None)


def _gather(H, ldh, n, d):
    return lib.sgcn_gather_rows_h16(H, ldh, _X, n, d, _X, max(d, 1), None)


def _scatter(H, ldh, n, d):
    return lib.sgcn_scatter_rows_h16(H, ldh, _X, n, d, _X, max(d, 1), None)


def _apply(H, ldh, n, d):
    return lib.sgcn_hist_apply_h16(H, ldh, _X, 2, n, d, None, None)


ENTRY = [("vr_aggregate_h16", _agg), ("vr_aggregate_pre_h16", _pre), ("vr_aggregate_post_h16", _post),
         ("gather_rows_h16", _gather), ("scatter_rows_h16", _scatter), ("hist_apply_h16", _apply)]


@pytest.mark.parametrize("name,call", ENTRY, ids=[e[0] for e in ENTRY])
def test_new_exports_validate_their_arguments_before_any_hip_call(name, call):
    assert lib.sgcn_abi_version() == 16

    def refused(rc):
        msg = (lib.sgcn_last_error() or b"").decode()
        assert rc == -1 and name + ":" in msg, (rc, msg)
    refused(call(None, 48, 4, 41))           # null table
    refused(call(_X, 48, -1, 41))            # negative size
    refused(call(_X, 48, 4, -1))
    refused(call(_X, 40, 4, 41))             # ldh < d
    refused(call(_X, 44, 4, 41))             # ldh % 8 != 0
    refused(call(_X + 8, 48, 4, 41))         # base not 16-byte aligned
    refused(call(_X + 2, 48, 4, 41))
    assert call(_X, 48, 0, 41) == 0          # n == 0: nothing to do
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), "sgcn_" + name)


# the fp32 entry points those mirror, as (message prefix, export, call(table address, ldh, n, d)): the table is checked
# AFTER the early return here, so n == 0 is fine with no table at all
def _agg_f32(H, ldh, n, d):
    return lib.sgcn_vr_aggregate_f32(_X, _X, _X, _X, _X, _X, n, max(n, 0), max(n, 0), d, _X, _X, max(d, 1), H, ldh, _X, _X, _X,
                                     _X, _X, 2 * max(d, 1), 1, 1, None, None)


def _pre_f32(H, ldh, n, d):
    return lib.sgcn_vr_aggregate_pre_f32(_X, _X, _X, n, max(n, 0), d, H, ldh, _X, _X, None, None)


def _post_f32(H, ldh, n, d):
    return lib.sgcn_vr_aggregate_post_f32(_X, _X, _X, n, max(n, 0), d, _X, _X, max(d, 1), H, ldh, _X, _X, _X, _X,
                                          2 * max(d, 1), 1, 1, _X, None)


def _apply_f32(H, ldh, n, d):
    return lib.sgcn_hist_apply_f32(H, ldh, _X, 2, n, d, None, None)


ENTRY_F32 = [("vr_aggregate", "sgcn_vr_aggregate_f32", _agg_f32), ("vr_aggregate_pre", "sgcn_vr_aggregate_pre_f32", _pre_f32),
             ("vr_aggregate_post", "sgcn_vr_aggregate_post_f32", _post_f32), ("hist_apply", "sgcn_hist_apply_f32", _apply_f32)]


@pytest.mark.parametrize("name,export,call", ENTRY_F32, ids=[e[1] for e in ENTRY_F32])
def test_fp32_counterparts_validate_their_arguments_before_any_hip_call(name, export, call):
    def refused(rc):
        msg = (lib.sgcn_last_error() or b"").decode()
        assert rc == -1 and msg.startswith(name + ":"), (rc, msg)
    refused(call(_X, 48, -1, 41))            # negative size
    refused(call(_X, 48, 4, -1))
    refused(call(_X, 40, 4, 41))             # ldh < d
    refused(call(None, 48, 4, 41))           # null table, once there is something to do
    assert call(_X, 48, 0, 41) == 0          # n == 0: nothing to do ...
    assert call(None, 48, 0, 41) == 0        # ... returns before the table is looked at (the bfloat16 forms refuse this)
    assert call(None, 0, 0, 41) == 0
    assert call(None, 48, 4, 0) == 0         # d == 0 likewise
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), export)
