"""sgcn_adam_ema_f32 (include/sgcn.h; --polyak_decay) exactly: theta, m and v carry the bits of sgcn_adam_f32, the average
the bits of the NumPy restatement (tests/ema_ref.py: two fp32 multiplies and an fp32 add, each rounded on its own) applied
to the weights read back, over three consecutive steps; nothing outside the n elements moves; what the entry point refuses
writes nothing.  Sizes: rows_cases.ADAM_COUNTS (one lane, either side of a workgroup, one element past the grid cap where
the stride loop wraps) and zero."""
import numpy as np
import pytest
import torch

import ema_ref
import rows_cases as rc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TAIL = 64                               # NaN sentinels behind every buffer
SIZES = (0,) + tuple(rc.ADAM_COUNTS)
DECAYS = (0.5, 0.9, 0.999)
B1, B2, EPS = 0.9, 0.999, 1e-8
SGCN_ERR_INVALID = -1


def _buf(x):
    """x on the device with a tail of NaN sentinels"""
    t = torch.full((x.shape[0] + TAIL,), float('nan'), dtype=torch.float32, device=DEV)
    t[:x.shape[0]] = torch.from_numpy(x).to(DEV)
    return t


def _bits(t):
    return t.view(torch.int32).cpu().numpy()


def _lr(t):
    return 0.01 * np.sqrt(1 - B2 ** t) / (1 - B1 ** t)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def data():
    """per size: start weights / moments and three gradients (shared by the decays, never modified)"""
    out = {}
    for n in SIZES:
        rng = np.random.RandomState(n % 1000 + 7)
        f = lambda s=1.0: (s * rng.standard_normal(n)).astype(np.float32)          # noqa: E731
        out[n] = dict(theta=f(), m=f(0.1), v=np.abs(f(0.01)), grads=[f(), f(0.3), f(3.0)])
    return out


@pytest.mark.parametrize("decay", DECAYS)
@pytest.mark.parametrize("n", SIZES)
def test_three_steps_bit_for_bit(data, n, decay):
    from stochastic_gcn_amd._ffi import lib
    c = data[n]
    d, om = ema_ref.factors(decay)
    th, m, v, avg = _buf(c['theta']), _buf(c['m']), _buf(c['v']), _buf(c['theta'])
    th2, m2, v2 = _buf(c['theta']), _buf(c['m']), _buf(c['v'])
    want_avg, m_ref, v_ref = c['theta'].copy(), c['m'].copy(), c['v'].copy()
    for step, g_host in enumerate(c['grads'], 1):
        g = _buf(g_host)
        g_before = _bits(g)
        lr = float(_lr(step))
        assert lib.sgcn_adam_ema_f32(th.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), avg.data_ptr(), n, lr, B1, B2, EPS,
                                     float(d), float(om), _stream()) == 0
        assert lib.sgcn_adam_f32(th2.data_ptr(), g.data_ptr(), m2.data_ptr(), v2.data_ptr(), n, lr, B1, B2, EPS, _stream()) == 0
        torch.cuda.synchronize()
        for a, b, what in ((th, th2, "theta"), (m, m2, "m"), (v, v2, "v")):
            assert np.array_equal(_bits(a), _bits(b)), "n=%d step %d: %s differs from sgcn_adam_f32 (or its tail moved)" % (n, step, what)
        assert np.array_equal(_bits(g), g_before), "the gradient was written"
        # the moments are products and sums rounded one by one (no FMA): fp32 NumPy gives their bits
        f = np.float32
        m_ref = f(B1) * m_ref + (f(1) - f(B1)) * g_host
        v_ref = f(B2) * v_ref + ((f(1) - f(B2)) * g_host) * g_host
        assert m_ref.dtype == np.float32 and np.array_equal(m[:n].cpu().numpy().view(np.int32), m_ref.view(np.int32))
        assert np.array_equal(v[:n].cpu().numpy().view(np.int32), v_ref.view(np.int32))
        theta_now = th[:n].cpu().numpy()
        if n:
            assert not np.array_equal(theta_now, c['theta'])
        want_avg = ema_ref.ema_f32(want_avg, theta_now, decay)
        got = avg.cpu().numpy()
        assert np.array_equal(got[:n].view(np.int32), want_avg.view(np.int32)), \
            "n=%d decay %g step %d: %d elements of the average differ from the fp32 restatement" % (
                n, decay, step, int((got[:n].view(np.int32) != want_avg.view(np.int32)).sum()))
        for t in (th, m, v, avg):
            assert bool(torch.isnan(t[n:]).all()) and t[n:].numel() == TAIL, "a sentinel behind the buffer was written"
    if n:
        assert not np.array_equal(want_avg, th[:n].cpu().numpy())            # (the average lags the weights: it is not a copy)


def test_refusals_write_nothing(data):
    from stochastic_gcn_amd._ffi import lib
    n = 257
    c = data[n]
    th, g, m, v, avg = _buf(c['theta']), _buf(c['grads'][0]), _buf(c['m']), _buf(c['v']), _buf(c['theta'])
    before = [_bits(t) for t in (th, g, m, v, avg)]
    P = lambda t, off=0: t.data_ptr() + 4 * off                                 # noqa: E731

    def call(avg_ptr, decay, count=n):
        d = np.float32(decay)
        return lib.sgcn_adam_ema_f32(P(th), P(g), P(m), P(v), avg_ptr, count, 0.01, B1, B2, EPS, float(d), float(np.float32(1) - d),
                                     _stream())
    assert call(0, 0.9) == SGCN_ERR_INVALID                                     # no average
    assert call(0, 0.9, count=0) == SGCN_ERR_INVALID
    for other in (th, g, m, v):                                                 # the average IS, or reaches into, an operand
        assert call(P(other), 0.9) == SGCN_ERR_INVALID
        assert call(P(other, n - 1), 0.9) == SGCN_ERR_INVALID
        assert call(P(other, -(n - 1)), 0.9) == SGCN_ERR_INVALID
    for decay in (1.0, 1.5, -0.25, float('nan')):
        assert call(P(avg), decay) == SGCN_ERR_INVALID
    assert call(P(avg), 0.9, count=-1) == SGCN_ERR_INVALID
    torch.cuda.synchronize()
    assert all(np.array_equal(_bits(t), b) for t, b in zip((th, g, m, v, avg), before)), "a refused call wrote something"
    assert call(P(avg), 0.0) == 0                                               # the border that is allowed: the average follows
    torch.cuda.synchronize()
    th1 = th[:n].cpu().numpy()
    assert np.array_equal(avg[:n].cpu().numpy(), ema_ref.ema_f32(c['theta'], th1, 0.0)) and np.array_equal(avg[:n].cpu().numpy(), th1)


def test_ops_wrapper_checks_its_operands(data):
    from stochastic_gcn_amd import ops
    n = 255
    c = data[n]
    t = lambda x: torch.from_numpy(x.copy()).to(DEV)                            # noqa: E731
    th, g, m, v, avg = t(c['theta']), t(c['grads'][0]), t(c['m']), t(c['v']), t(c['theta'])
    ops.adam_ema_step(th, g, m, v, avg, _lr(1), B1, B2, EPS, decay=0.9)
    torch.cuda.synchronize()
    assert np.array_equal(avg.cpu().numpy(), ema_ref.ema_f32(c['theta'], th.cpu().numpy(), 0.9))
    with pytest.raises(ValueError):
        ops.adam_ema_step(th, g, m, v, avg[:-1], _lr(1), B1, B2, EPS, decay=0.9)
    with pytest.raises(TypeError):
        ops.adam_ema_step(th, g, m, v, avg.double(), _lr(1), B1, B2, EPS, decay=0.9)
    with pytest.raises(Exception, match="overlaps"):
        ops.adam_ema_step(th, g, m, v, th, _lr(1), B1, B2, EPS, decay=0.9)
