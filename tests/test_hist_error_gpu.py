"""sgcn_hist_error_f32 / _h16 (ops.history_error) against NumPy fp64: out4 = {sum (x - h)^2, sum x^2, max |x - h|, rows with
any x != h}.

Exact cases: on dyadic inputs (small integers times powers of two, representable in bfloat16) every product and every
partial sum is an exactly representable fp64 number, so all four outputs must equal the reference BIT FOR BIT whatever the
summation order.  Real-valued cases: the two sums are held to the fp64 recursive-summation bound n d 2^-53 Sigma (each
square is one rounded multiply of exact operands on both sides; the reference sums them exactly with math.fsum); the
maximum and the row count are exact."""
import math

import numpy as np
import pytest
import torch

import bf16_ref

pytestmark = pytest.mark.gpu

NS = (0, 1, 63, 64, 65, 257, 4099)
DS = (1, 3, 7, 8, 41, 128, 130, 602)
SHAPES = [(n, d) for n in NS for d in DS] + [(70001, 8)]          # (the last: every wave of the fixed grid takes many rows)
U = 2.0 ** -53


def _dev():
    return torch.device("cuda:0")


def _x_on_device(x, layout):
    """x as a device tensor: contiguous, or a column-offset view of a wider table whose other columns hold NaN."""
    n, d = x.shape
    if layout == 'contiguous':
        return torch.from_numpy(x).to(_dev())
    base = torch.full((n, d + 5), float('nan'), dtype=torch.float32, device=_dev())
    view = base[:, 3:3 + d]
    view.copy_(torch.from_numpy(x).to(_dev()))
    assert view.shape[0] < 2 or view.stride(0) == d + 5
    return view


def _h_on_device(h, dtype):
    """h as an fp32 table, or as a bfloat16 table in the history's storage contract (pitch 8 ceil(d / 8), the pad columns
    holding NaN here: nothing may read them into a sum); h must be representable."""
    n, d = h.shape
    if dtype == 'fp32':
        return torch.from_numpy(h).to(_dev())
    assert np.array_equal(bf16_ref.round_trip(h), h)
    tab = torch.full((n, (d + 7) // 8 * 8), float('nan'), dtype=torch.bfloat16, device=_dev())
    H = tab[:, :d]
    H.copy_(torch.from_numpy(h).to(_dev()).to(torch.bfloat16))
    return H


def _reference(x, h, exact_sums):
    x64, h64 = x.astype(np.float64), h.astype(np.float64)
    e = x64 - h64
    tot = (lambda a: math.fsum(a.ravel().tolist())) if exact_sums else (lambda a: float(a.sum()))
    return np.array([tot(e * e), tot(x64 * x64), np.abs(e).max() if e.size else 0.0,
                     float(np.count_nonzero((x != h).any(axis=1))) if e.size else 0.0], dtype=np.float64)


def _dyadic(rng, shape):
    return (rng.randint(-8, 9, shape) * 2.0 ** rng.randint(-3, 4, shape)).astype(np.float32)


def _run(x, h, dtype, layout):
    from stochastic_gcn_amd import ops
    out = ops.history_error(_x_on_device(x, layout), _h_on_device(h, dtype))
    assert out.dtype == torch.float64 and tuple(out.shape) == (4,)
    return out.cpu().numpy()


@pytest.mark.parametrize("layout", ['contiguous', 'view'])
@pytest.mark.parametrize("dtype", ['fp32', 'bf16'])
def test_dyadic_inputs_bit_for_bit(dtype, layout):
    rng = np.random.RandomState(7)
    for n, d in SHAPES:
        x = _dyadic(rng, (n, d))
        h = x.copy()
        stale = rng.rand(n) < 0.4                              # four rows in ten differ, in a few of their columns
        mask = stale[:, None] & (rng.rand(n, d) < 0.3)
        h[mask] = _dyadic(rng, (n, d))[mask]
        got, ref = _run(x, h, dtype, layout), _reference(x, h, exact_sums=False)
        assert got.tobytes() == ref.tobytes(), (n, d, got, ref)


REAL_SHAPES = [(1, 602), (65, 130), (257, 41), (4099, 128), (70001, 8)]


@pytest.mark.parametrize("dtype", ['fp32', 'bf16'])
def test_real_valued_inputs_within_the_summation_bound(dtype):
    rng = np.random.RandomState(11)
    for n, d in REAL_SHAPES:
        x = rng.standard_normal((n, d)).astype(np.float32)
        if dtype == 'fp32':
            h = (x + 0.1 * rng.standard_normal((n, d))).astype(np.float32)
            h[::3] = x[::3]                                    # a third of the rows are fresh
        else:
            h = bf16_ref.round_trip(x)
        for layout in ('contiguous', 'view'):
            got, ref = _run(x, h, dtype, layout), _reference(x, h, exact_sums=True)
            bound = n * d * U
            print("n=%d d=%d %s %s: |dS|/S = %.3e, %.3e (bound %.3e) max %r rows %r" % (
                n, d, dtype, layout, abs(got[0] - ref[0]) / max(ref[0], 1e-300), abs(got[1] - ref[1]) / ref[1], bound, got[2], got[3]))
            assert abs(got[0] - ref[0]) <= bound * ref[0] and abs(got[1] - ref[1]) <= bound * ref[1], (n, d, got, ref)
            assert got[2] == ref[2] and got[3] == ref[3], (n, d, got, ref)


@pytest.mark.parametrize("dtype", ['fp32', 'bf16'])
def test_same_call_twice_gives_identical_bits(dtype):
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(3)
    x = rng.standard_normal((4099, 130)).astype(np.float32)
    h = bf16_ref.round_trip((x + 0.01 * rng.standard_normal(x.shape)).astype(np.float32))
    X, H = _x_on_device(x, 'contiguous'), _h_on_device(h, dtype)
    a = ops.history_error(X, H).cpu().numpy()
    torch.randn(1 << 20, device=_dev()).sum().item()           # (other work in between)
    b = ops.history_error(X, H).cpu().numpy()
    assert a.tobytes() == b.tobytes() and a[0] > 0


@pytest.mark.parametrize("dtype", ['fp32', 'bf16'])
def test_fresh_history_reports_exact_zeros(dtype):
    rng = np.random.RandomState(5)
    for n, d in ((257, 41), (4099, 128)):
        x = bf16_ref.round_trip(rng.standard_normal((n, d)).astype(np.float32))      # (so that x == widen(h) is possible)
        got, ref = _run(x, x.copy(), dtype, 'view'), _reference(x, x, exact_sums=True)
        assert got[0] == 0.0 and got[2] == 0.0 and got[3] == 0.0, got
        assert abs(got[1] - ref[1]) <= n * d * U * ref[1]


@pytest.mark.parametrize("dtype", ['fp32', 'bf16'])
def test_zero_history_has_relative_error_exactly_one(dtype):
    rng = np.random.RandomState(9)
    for n, d in ((63, 7), (4099, 130)):
        x = rng.standard_normal((n, d)).astype(np.float32)
        x[5] = 0.0                                                                  # an all-zero row is NOT off
        got = _run(x, np.zeros_like(x), dtype, 'contiguous')
        assert got[0].tobytes() == got[1].tobytes() and math.sqrt(got[0] / got[1]) == 1.0
        assert got[2] == np.abs(x).max() and got[3] == n - 1


def test_empty_table_returns_zeros_and_bad_shapes_are_refused():
    from stochastic_gcn_amd import ops
    out = torch.full((4,), 7.0, dtype=torch.float64, device=_dev())
    res = ops.history_error(torch.zeros((0, 16), device=_dev()), torch.zeros((0, 16), device=_dev()), out=out)
    assert res is out and out.cpu().tolist() == [0.0, 0.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="shape"):
        ops.history_error(torch.zeros((4, 16), device=_dev()), torch.zeros((4, 8), device=_dev()))
    with pytest.raises(TypeError):
        ops.history_error(torch.zeros((4, 16), device=_dev()), torch.zeros((4, 16), dtype=torch.float16, device=_dev()))
