"""The --gradvar statistics entry points (sgcn_moments_add_f32, sgcn_moments_summary_f64) validate their arguments
before any HIP call, so the checks run without a GPU; adding them left the ABI version where it was."""
import pytest

from stochastic_gcn_amd import _ffi

lib = _ffi.lib
A = 4096       # a non-null address that is never dereferenced: every call below fails validation first


def _fails(rc, text):
    assert rc == -1
    assert text in lib.sgcn_last_error()


def test_abi_version_unchanged():
    assert lib.sgcn_abi_version() == _ffi.ABI_VERSION == 16


@pytest.mark.parametrize("x,mean,m2", [(None, A, A), (A, None, A), (A, A, None), (None, None, None)])
def test_moments_add_rejects_null_operands(x, mean, m2):
    _fails(lib.sgcn_moments_add_f32(x, 8, 0, mean, m2, None), b"null operand")


def test_moments_add_rejects_negative_size_and_count():
    _fails(lib.sgcn_moments_add_f32(A, -1, 0, A, A, None), b"negative size")
    _fails(lib.sgcn_moments_add_f32(A, 8, -1, A, A, None), b"negative count")
    _fails(lib.sgcn_moments_add_f32(A + 2, 8, 0, A, A, None), b"not aligned")


@pytest.mark.parametrize("mean_a,m2_a,out", [(None, A, A), (A, None, A), (A, A, None)])
def test_moments_summary_rejects_null_operands(mean_a, m2_a, out):
    _fails(lib.sgcn_moments_summary_f64(mean_a, m2_a, 3, None, 8, out, None), b"null operand")


def test_moments_summary_rejects_negative_size_and_empty_count():
    _fails(lib.sgcn_moments_summary_f64(A, A, 3, None, -1, A, None), b"negative size")
    _fails(lib.sgcn_moments_summary_f64(A, A, 0, None, 8, A, None), b"count_a must be positive")
    _fails(lib.sgcn_moments_summary_f64(A, A, -5, A, 8, A, None), b"count_a must be positive")


def test_device_stat_refuses_host_tensors_and_size_changes():
    import torch
    from stochastic_gcn_amd.stats import DeviceStat, summary
    s = DeviceStat()
    with pytest.raises(RuntimeError, match="HBM"):
        s.add(torch.zeros(4))
    with pytest.raises(ValueError, match="no samples"):
        summary(s)
    with pytest.raises(TypeError):
        s.add([1.0, 2.0])
