"""CPU test of the row SpMM's refusals of a bad plan (sgcn_spmm_csr_f32 / sgcn_spmm_csr_b16): a hand-made sgcn_plan_t, ordinary
addresses that are never dereferenced, a refusal before any HIP call.  The three checks are the ones every row-segment launch
shares (csrc/sgcn_seg.h); tests/test_spmax.py and tests/test_spattn.py pin them for the other families."""
import ctypes

import pytest

from stochastic_gcn_amd import _ffi

A = 4096          # non-null, 16-byte aligned addresses: every call below fails validation first


def _plan(nfix, nslots, ws, ws_elems, seg=A, nseg=8, fix=2 * A):
    return _ffi.Plan(seg, nseg, fix if nfix else None, nfix, nslots, ws, ws_elems)


@pytest.mark.parametrize("name", ["sgcn_spmm_csr_f32", "sgcn_spmm_csr_b16"])
def test_spmm_refuses_a_bad_plan_before_any_device_call(name):
    fn, err = getattr(_ffi.lib, name), _ffi.lib.sgcn_last_error

    def spmm(plan, d=8, ld=8):
        return fn(3 * A, 4 * A, 5 * A, 8, 8, d, 6 * A, ld, None, None, None, 7 * A, ld, 0.0, ctypes.byref(plan), None)

    # fewer segments than rows; no segment table
    assert spmm(_plan(0, 0, None, 0, nseg=7)) == -1 and err() == b"spmm: malformed plan"
    assert spmm(_plan(0, 0, None, 0, seg=None)) == -1 and err() == b"spmm: malformed plan"
    # split rows without the fix-up's table, without the workspace
    assert spmm(_plan(2, 6, 8 * A, 6 * 8, fix=None)) == -1 and err() == b"spmm: plan with split rows needs dev_fix/dev_ws"
    assert spmm(_plan(2, 6, None, 6 * 8)) == -1 and err() == b"spmm: plan with split rows needs dev_fix/dev_ws"
    # six slots of eight floats do not fit; at d = 9 the slot pitch is 12
    assert spmm(_plan(2, 6, 8 * A, 6 * 8 - 1)) == -1 and err() == b"spmm: workspace too small (47 < 48 floats)"
    assert spmm(_plan(2, 6, 8 * A, 6 * 8), d=9, ld=16) == -1 and err() == b"spmm: workspace too small (48 < 72 floats)"
    # the order: the segment table first, the fix-up's tables second, the room last
    assert spmm(_plan(2, 6, None, 0, nseg=7)) == -1 and err() == b"spmm: malformed plan"
    assert spmm(_plan(2, 6, None, 0)) == -1 and err() == b"spmm: plan with split rows needs dev_fix/dev_ws"
    # the operand checks come before the plan's
    assert fn(None, 4 * A, 5 * A, 8, 8, 8, 6 * A, 8, None, None, None, 7 * A, 8, 0.0,
              ctypes.byref(_plan(0, 0, None, 0, nseg=7)), None) == -1 and err() == b"spmm: null operand"
