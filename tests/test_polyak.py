"""--polyak_decay without a device: the flag's refusals, the additive C-ABI (sgcn_adam_ema_f32, SGCN_OP_ADAM_EMA, ABI still
16) and the NumPy restatement of the average (tests/ema_ref.py) against its own fp64 twin."""
import os
import re
import types

import numpy as np
import pytest

import ema_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flags(**kw):
    return types.SimpleNamespace(**dict(dict(polyak_decay=0.0, gradvar=False), **kw))


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.9, 0.99, 0.999, 0.9999999])
def test_check_polyak_accepts(decay):
    from stochastic_gcn_amd.flags import check_polyak
    assert check_polyak(_flags(polyak_decay=decay)) == decay
    assert check_polyak(_flags(polyak_decay=0.0, gradvar=True)) == 0.0          # the study without the average: as ever


@pytest.mark.parametrize("decay", [-0.1, 1.0, 1.5, float('nan'), float('inf'), 1.0 - 1e-9])
def test_check_polyak_refuses_a_decay_outside_the_unit_interval(decay):
    """(1 - 1e-9 is below 1 as a double and IS 1 as the fp32 the kernels take)"""
    from stochastic_gcn_amd.flags import check_polyak
    with pytest.raises(ValueError, match="polyak_decay must lie in"):
        check_polyak(_flags(polyak_decay=decay))


def test_check_polyak_refuses_gradvar():
    from stochastic_gcn_amd.flags import check_polyak
    with pytest.raises(ValueError, match="gradvar"):
        check_polyak(_flags(polyak_decay=0.9, gradvar=True))


def test_flag_defaults_and_parses():
    from stochastic_gcn_amd.flags import FLAGS, check_polyak
    FLAGS.reset()
    assert FLAGS.polyak_decay == 0.0 and check_polyak() == 0.0
    try:
        FLAGS.parse(['--polyak_decay', '0.99'])
        assert check_polyak() == 0.99
        help_ = next(a.help for a in FLAGS.parser()._actions if a.dest == 'polyak_decay' and a.help)
        assert 'moving average' in help_ and 'out of scope' not in help_
    finally:
        FLAGS.reset()


def test_trainer_refuses_before_a_device_is_touched(monkeypatch):
    import torch
    from stochastic_gcn_amd import train
    from stochastic_gcn_amd.flags import FLAGS
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a device was asked for"))
    try:
        for kw in (dict(polyak_decay=1.0), dict(polyak_decay=0.9, gradvar=True)):
            FLAGS.reset()
            FLAGS.update(dataset='s-cora', **kw)
            with pytest.raises(ValueError, match="polyak_decay"):
                train.Trainer(verbose=False)
    finally:
        FLAGS.reset()


def test_the_export_is_declared_bound_and_additive():
    from stochastic_gcn_amd import _ffi
    from stochastic_gcn_amd.step_program import OP
    assert "sgcn_adam_ema_f32" in _ffi.SIGNATURES
    res, args = _ffi.SIGNATURES["sgcn_adam_ema_f32"]
    assert len(args) == 13 and len(_ffi.SIGNATURES["sgcn_adam_f32"][1]) == 10
    assert callable(_ffi.lib.sgcn_adam_ema_f32)
    assert _ffi.lib.sgcn_abi_version() == 16 == _ffi.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "sgcn.h")).read()
    code = int(re.search(r"SGCN_OP_ADAM_EMA\s*=\s*(\d+)", header).group(1))
    assert code == OP['ADAM_EMA'] and list(OP.values()).count(code) == 1
    codes = [int(c) for c in re.findall(r"SGCN_OP_\w+\s*=\s*(\d+)", header)]
    assert code == max(codes) and codes.count(code) == 1                      # the next free code
    assert int(re.search(r"SGCN_OP_ADAM\s*=\s*(\d+)", header).group(1)) == OP['ADAM'] == 6
    assert "gcn/models.py:104-121" in header[header.index("sgcn_adam_ema_f32") - 1500:header.index("sgcn_adam_ema_f32")]


def test_polyak_factors_are_fp32():
    from stochastic_gcn_amd import ops
    for decay in (0.5, 0.9, 0.99, 0.999):
        d, om = ops.polyak_factors(decay)
        rd, rom = ema_ref.factors(decay)
        assert np.float32(d) == rd and np.float32(om) == rom and d == float(rd) and om == float(rom)
        assert rom == np.float32(np.float32(1.0) - np.float32(decay))


@pytest.mark.parametrize("decay", [0.5, 0.9, 0.99, 0.999])
@pytest.mark.parametrize("close", [True, False])
def test_fp32_reference_agrees_with_its_fp64_twin_to_one_ulp(decay, close):
    """The three roundings cost at most one fp32 ulp (2^-23 times the magnitude) of max(|avg|, |theta|): derived in
    ema_ref's docstring, measured here on weights that sit close to their average and on unrelated ones."""
    rng = np.random.RandomState(int(decay * 1000) + close)
    avg = (rng.standard_normal(200000) * np.exp(rng.uniform(-6, 2, 200000))).astype(np.float32)
    theta = (avg * (1 + 0.01 * rng.standard_normal(avg.size))).astype(np.float32) if close else \
        rng.standard_normal(avg.size).astype(np.float32)
    f32, f64 = ema_ref.ema_f32(avg, theta, decay), ema_ref.ema_f64(avg, theta, decay)
    assert f32.dtype == np.float32 and f64.dtype == np.float64
    err = np.abs(f32.astype(np.float64) - f64)
    worst = float((err / ema_ref.ulp_bound(avg, theta)).max())
    print("decay %g: worst %.3f ulp (%.3f grid spacings)" % (decay, worst, float((err / ema_ref.spacing(avg, theta)).max())))
    assert worst <= 1.0
    if decay == 0.5:                      # both products exact: the sum's rounding alone
        assert (err <= 0.5 * ema_ref.spacing(avg, theta)).all()


def test_fold_is_the_recursion_and_decay_zero_copies():
    rng = np.random.RandomState(1)
    t0, ts = rng.standard_normal(50).astype(np.float32), [rng.standard_normal(50).astype(np.float32) for _ in range(3)]
    out = ema_ref.fold(t0, ts, 0.9)
    assert np.array_equal(out[0], ema_ref.ema_f32(t0, ts[0], 0.9)) and np.array_equal(out[2], ema_ref.ema_f32(out[1], ts[2], 0.9))
    assert np.array_equal(ema_ref.ema_f32(t0, ts[0], 0.0), ts[0] + np.float32(0) * t0)
    const = ema_ref.fold(t0, [t0, t0], 0.5)                                   # dyadic: a constant stays put exactly
    assert np.array_equal(const[1], t0)
