"""--history_dtype bf16 on the GPU.  Every comparison is an equality whose reference side is code this feature does not
touch -- the fp32 entry points, the fp32 model, the fp64 aggregate of tests/sparse_cases.py -- plus the integer NumPy
rounding of tests/bf16_ref.py; the bfloat16 code is never compared with itself."""
import contextlib
import io
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import bf16_ref
import model_cases as mc
import sparse_cases as sc
from gpu_checks import Operand, Output

pytestmark = pytest.mark.gpu

WORKERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "history_bf16_workers.py")
SENTINEL = 0x7FC1          # a NaN pattern no rounding produces from the test's values


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


def _pitch(d):
    return (d + 7) // 8 * 8


def _bits(t):
    """uint16 bit patterns of a bfloat16 tensor (any strides)"""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _table(bits, dev, rows=None, fill=0):
    """an N x pitch bfloat16 buffer holding `bits` (uint16, N x d) in its [:, :d] view, `fill` elsewhere"""
    n, d = bits.shape
    buf = torch.full((rows or n, _pitch(d)), fill, dtype=torch.int16, device=dev).view(torch.bfloat16)
    buf[:n, :d].view(torch.int16).copy_(torch.from_numpy(bits.view(np.int16)).to(dev))
    assert buf.data_ptr() % 16 == 0
    return buf, buf[:n, :d]


def _values(rng, shape):
    """N(0, 1) values with the contract's special values and NaNs sprinkled in"""
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    k = min(flat.size, len(bf16_ref.SPECIALS))
    flat[rng.choice(flat.size, k, replace=False)] = bf16_ref.SPECIALS[:k]
    if flat.size > 40:
        flat[rng.choice(flat.size, 3, replace=False)] = np.array([0x7FC00000, 0x7F800001, 0xFFFFFFFF], np.uint32).view(np.float32)
    return x


def _same_bits(got, x):
    """got (uint16) is the rounding of x (fp32): equal bits, NaN for NaN"""
    want = bf16_ref.round_bits(x)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan])
    assert np.isnan(bf16_ref.widen_bits(got[nan])).all()


D_ROWS = [1, 7, 8, 41, 128, 130, 256]


# ---- 1, 2: row scatter / gather -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", D_ROWS)
def test_scatter_rounds_to_nearest_even_and_touches_nothing_else(dev, d):
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(d)
    N, n = 300, 96
    for src_pitch in (d + 3, (d + 3) // 4 * 4, (d + 1) // 2 * 2 + 2):
        idx = rng.choice(N, n, replace=False).astype(np.int32)
        idx[rng.choice(n, 13, replace=False)] = -1
        src = Operand(_values(rng, (n, d)), dev, src_pitch)
        buf, H = _table(np.full((N, d), SENTINEL, np.uint16), dev, fill=np.int16(SENTINEL))
        ops.scatter_rows(H, torch.from_numpy(idx).to(dev), src.view)
        torch.cuda.synchronize()
        got = _bits(buf)
        x = src.view.cpu().numpy()
        keep = np.ones(N, bool)
        keep[idx[idx >= 0]] = False
        assert (got[keep] == SENTINEL).all() and (got[:, d:] == SENTINEL).all()       # rows not addressed, pad columns
        _same_bits(got[idx[idx >= 0], :d], x[idx >= 0])
        assert src.unchanged()
    # a null index: rows 0 .. n-1 in place
    x = _values(rng, (N - 5, d))
    buf, H = _table(np.full((N, d), SENTINEL, np.uint16), dev, fill=np.int16(SENTINEL))
    ops.scatter_rows(H, None, torch.from_numpy(x).to(dev))
    got = _bits(buf)
    _same_bits(got[:N - 5, :d], x)
    assert (got[N - 5:] == SENTINEL).all() and (got[:, d:] == SENTINEL).all()


@pytest.mark.parametrize("d", D_ROWS)
def test_gather_widens_exactly(dev, d):
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(100 + d)
    N, n = 300, 90
    bits = bf16_ref.round_bits(_values(rng, (N, d)))
    buf, H = _table(bits, dev, fill=np.int16(SENTINEL))
    before = _bits(buf)
    idx = rng.choice(N, n).astype(np.int32)                       # repeats allowed
    for out_pitch in (d + 3, (d + 3) // 4 * 4, (d + 1) // 2 * 2 + 2):
        out = Output(dev, n, d, out_pitch)
        ops.gather_rows(H, torch.from_numpy(idx).to(dev), out=out.view)
        torch.cuda.synchronize()
        out.written_inside("gather_rows_h16 d=%d" % d)
        assert np.array_equal(out.view.cpu().numpy().view(np.uint32), bits[idx].astype(np.uint32) << 16)
    whole = ops.gather_rows(H, None)
    assert whole.shape == (N, d) and np.array_equal(whole.cpu().numpy().view(np.uint32), bits.astype(np.uint32) << 16)
    assert np.array_equal(_bits(buf), before)
    assert torch.equal(ops.history_widen(H).view(torch.int32), whole.view(torch.int32))


# ---- 3: the aggregator, bit for bit against the fp32 entry points ---------------------------------------------------------
def _agg_pair(dev, H32, d):
    """(fp32 table with the bfloat16 table's element pitch holding the widened values, bfloat16 table)"""
    bits = bf16_ref.round_bits(H32)
    b16, v16 = _table(bits, dev)
    b32 = torch.zeros((H32.shape[0], _pitch(d)), dtype=torch.float32, device=dev)
    v32 = b32[:, :d]
    v32.copy_(torch.from_numpy(bf16_ref.widen_bits(bits)).to(dev))
    assert b32.data_ptr() % 16 == 0 and v32.stride(0) == v16.stride(0)
    return v32, v16


def _agg_outputs(call, dev, n1, width, cvd):
    pitch = (width + 3) // 4 * 4 + 4          # (pad columns that never limit the vector width: the operands decide it)
    oh, om = Output(dev, n1, width, pitch), Output(dev, n1, width, pitch)
    call(oh.view, om.view if cvd else None)
    torch.cuda.synchronize()
    oh.written_inside()
    om.written_inside()
    return oh.bits(), om.bits()


AGG_D = [8, 41, 64, 128, 130, 256]


# 7 and 25 (beyond the widths the aggregator usually sees): scalar vectors in groups narrower than a wavefront
@pytest.mark.parametrize("d", AGG_D + [7, 25])
@pytest.mark.parametrize("split", ["none", "T"])
@pytest.mark.parametrize("concat", [False, True])
@pytest.mark.parametrize("cvd", [False, True])
def test_aggregator_equals_the_fp32_entry_points_on_the_widened_table(dev, cvd, concat, split, d):
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd._ffi import check, lib
    import ctypes as C
    adj0, fadj0, fd = sc.scheduler_batch(seed=4, degree=3)
    n, n0, n1 = 3000, fd['f0'].shape[0], adj0.shape[0]
    width = 2 * d if concat else d
    rng = np.random.RandomState(1000 * d + 4 * cvd + 2 * concat + (split == "T"))
    adj, fadj = sc.normalised(adj0), sc.normalised(fadj0)
    A = ops.DeviceCSR.from_scipy(adj, dev, with_plan=False)
    P = ops.DeviceCSR.from_scipy(fadj, dev, plan_T=8 if split == "T" else 0, with_plan=split == "T")
    if split == "T":
        assert P.plan.nfix > 0                                    # some rows take the ordered fix-up
    H32, H16 = _agg_pair(dev, rng.standard_normal((n, d)).astype(np.float32), d)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    f0, ff0, s = t(fd['f0']), t(fd['ff0']), t((rng.rand(n1) + 0.5).astype(np.float32))
    st = torch.cuda.current_stream().cuda_stream
    for xpitch in sorted({d, (d + 3) // 4 * 4}):                  # an odd activation pitch narrows the fused call's vectors
        h = Operand(rng.standard_normal((n0, d)).astype(np.float32), dev, xpitch)
        mu = Operand(rng.standard_normal((n0, d)).astype(np.float32), dev, xpitch)

        def fused(H):
            return lambda oh, om: ops.vr_aggregate(A, P, h.view, mu.view if cvd else None, H, f0, ff0, s if cvd else None, cvd,
                                                   concat, out_h=oh, out_mu=om)

        def two_phase(H):
            """_pre + _post into sentinelled outputs (ops.vr_aggregate_two_phase allocates its own)"""
            h16 = H.dtype == torch.bfloat16
            pre = lib.sgcn_vr_aggregate_pre_h16 if h16 else lib.sgcn_vr_aggregate_pre_f32
            post = lib.sgcn_vr_aggregate_post_h16 if h16 else lib.sgcn_vr_aggregate_post_f32

            def call(oh, om):
                accP = torch.full((n1, (d + 3) // 4 * 4), float("nan"), device=dev)
                plan = P.plan.struct(d) if P.plan is not None else None
                check(pre(P.rowptr.data_ptr(), P.col.data_ptr(), P.val.data_ptr(), n1, P.shape[1], d, H.data_ptr(), H.stride(0),
                          ff0.data_ptr(), accP.data_ptr(), C.byref(plan) if plan is not None else None, st))
                check(post(A.rowptr.data_ptr(), A.col.data_ptr(), A.val.data_ptr(), n1, n0, d, h.view.data_ptr(),
                           mu.view.data_ptr() if cvd else None, h.view.stride(0), H.data_ptr(), H.stride(0), f0.data_ptr(),
                           s.data_ptr() if cvd else None, oh.data_ptr(), om.data_ptr() if cvd else None, oh.stride(0),
                           int(cvd), int(concat), accP.data_ptr(), st))
            return call
        want = {"fused": _agg_outputs(fused(H32), dev, n1, width, cvd), "pre + post": _agg_outputs(two_phase(H32), dev, n1, width, cvd)}
        assert not torch.isnan(want["fused"][0].view(torch.float32)[:n1, :width]).any()
        for name, form in (("fused", fused), ("pre + post", two_phase)):
            got = _agg_outputs(form(H16), dev, n1, width, cvd)
            # each form against ITS fp32 entry point(s); and, on the widths the aggregator is specified for, both against
            # the fused fp32 call (at d = 7 and 25 with an odd activation pitch the fp32 forms themselves differ: the fused
            # pass then runs scalar lanes in narrow groups, whose P-sum the compiler contracts, and _pre runs vectors)
            for ref in [name] + (["fused"] if d in AGG_D else []):
                for g, w, which in zip(got, want[ref], ("out_h", "out_mu")):
                    assert torch.equal(g, w), "%s on the bfloat16 table: %s differs from the fp32 %s form (d=%d, pitch %d)" % (
                        name, which, ref, d, xpitch)
        assert h.unchanged() and mu.unchanged()
    # the two-phase wrapper of ops dispatches on the table's dtype as well
    a = ops.vr_aggregate_two_phase(A, P, h.view, mu.view if cvd else None, H16, f0, ff0, s if cvd else None, cvd, concat)
    b = ops.vr_aggregate_two_phase(A, P, h.view, mu.view if cvd else None, H32, f0, ff0, s if cvd else None, cvd, concat)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and (not cvd or torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


# ---- 4: the aggregator against the exact fp64 aggregate -------------------------------------------------------------------
@pytest.mark.parametrize("cvd", [True, False])
@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("split,d", [("none", 30), ("T", 128), ("default", 602), ("T", 1), ("none", 260), ("T", 41)])
def test_aggregator_is_exact_on_dyadic_inputs(dev, cvd, concat, split, d):
    """The form of tests/test_sparse_exact_gpu.py::test_vr_aggregate on a bfloat16 table: nothing here leans on the fp32
    kernel."""
    from stochastic_gcn_amd import ops
    adj0, fadj0, fd = sc.scheduler_batch(seed=4, degree=3)
    n, n0, n1 = 3000, fd['f0'].shape[0], adj0.shape[0]
    width = 2 * d if concat else d
    rng = np.random.RandomState(7 * d + 2 * cvd + concat)
    adj, fadj = sc.dyadic(adj0, rng), sc.dyadic(fadj0, rng)
    h, mu, H = (sc.ints(rng, s) for s in ((n0, d), (n0, d), (n, d)))
    assert np.array_equal(bf16_ref.round_trip(H).view(np.uint32), H.view(np.uint32))          # the table survives storage
    s = sc.pow2(rng, n1)
    A = ops.DeviceCSR.from_scipy(adj, dev, with_plan=False)
    P = ops.DeviceCSR.from_scipy(fadj, dev, plan_T=8 if split == "T" else 0, with_plan=split != "none")
    if split == "T":
        assert P.plan.nfix > 0
    oh, om, mh, mm, nt = sc.vr_aggregate_f64(adj, fadj, h, mu, H, fd['f0'], fd['ff0'], s, cvd, concat)
    sc.assert_exact(mh, sc.low_exp(adj.data, fadj.data) + min(sc.low_exp(s), 0), "aggregate")
    sc.assert_exact(np.abs(h) + np.abs(mu), 0)
    hb, mb = Operand(h, dev, d), Operand(mu, dev, d)
    _, H16 = _table(bf16_ref.round_bits(H), dev)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    for form in (ops.vr_aggregate, ops.vr_aggregate_two_phase):
        r = form(A, P, hb.view, mb.view, H16, t(fd['f0']), t(fd['ff0']), t(s), cvd, concat)
        assert hb.unchanged() and mb.unchanged()
        for g, ref in ((r[0], oh), (r[1], om)):
            if ref is None:
                continue
            g = g.double().cpu().numpy()
            assert g.shape == (n1, width)
            bad = g != ref
            assert not bad.any(), "%s: %d rows differ from the exact aggregate" % (form.__name__, int(bad.any(1).sum()))


# ---- 5: the history exchange's apply ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,sizes", [(3, [64, 17, 0]), (8, [64, 17, 0, 64, 33, 1, 64, 50])])
def test_exchange_apply_rounds_the_fp32_payload_in_rank_order(dev, world, sizes):
    from stochastic_gcn_amd._ffi import check, lib
    rng = np.random.RandomState(0)
    N, d, cap = 500, 37, 64
    start = bf16_ref.round_bits(rng.standard_normal((N, d)).astype(np.float32))
    want = start.copy()
    recv = torch.empty(world * cap * (d + 1), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    for r in range(world):
        n = sizes[r]
        ids = rng.choice(N // 4, n, replace=False).astype(np.int32)              # a quarter of the vertices: ranks collide
        rows = _values(rng, (max(n, 1), 48))                                     # rows with a pitch
        rows[np.isnan(rows)] = 0.5
        send = recv[r * cap * (d + 1):(r + 1) * cap * (d + 1)]
        idt, rt = torch.from_numpy(ids).to(dev), torch.from_numpy(rows).to(dev)
        check(lib.sgcn_hist_pack_f32(idt.data_ptr(), n, rt.data_ptr(), 48, d, cap, send.data_ptr(), st))
        want[ids] = bf16_ref.round_bits(rows[:n, :d])                            # rank order: the higher rank's row stays
    owner = torch.zeros(N, dtype=torch.int32, device=dev)
    for own in (None, owner, owner):
        buf, H = _table(start, dev, fill=np.int16(SENTINEL))
        check(lib.sgcn_hist_apply_h16(H.data_ptr(), H.stride(0), recv.data_ptr(), world, cap, d,
                                      None if own is None else own.data_ptr(), st))
        torch.cuda.synchronize()
        got = _bits(buf)
        assert np.array_equal(got[:, :d], want) and (got[:, d:] == SENTINEL).all()
        assert int(owner.abs().sum()) == 0


# ---- 6, 7: the model against the fp32 model with a rounding hook -------------------------------------------------------
def _round_hook(h, idx, v, fn):
    """what a bfloat16 table would have stored, written into an fp32 one (rounding in NumPy, tests/bf16_ref.py)"""
    x = v.detach().cpu().numpy()
    return fn(h, idx, torch.from_numpy(bf16_ref.round_trip(x)).to(v.device))


def _model(case, params, native, bf16, slot_group=(False, True), is_training=True):
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.vrgcn import VRGCN
    group = slot_group[1]
    FLAGS.reset()
    FLAGS.update(**{k: v for k, v in case['flags'].items() if hasattr(FLAGS, k)})
    FLAGS.update(native_step=native, batch_size=case['cfg']['batch'], test_batch_size=case['cfg']['batch'],
                 test_degree=case['flags']['degree'], group_dw=group, lean_sync=group, agg_overlap=not group,
                 history_dtype='bf16' if bf16 else 'fp32')
    fl = case['flags']
    with contextlib.redirect_stdout(io.StringIO()):
        m = VRGCN(fl['num_layers'], fl['preprocess'], case['ph'], case['feats'], case['nbr'], case['adj'], fl['cvd'],
                  is_training=is_training, device=torch.device('cuda:0'))
    m.set_params({k: v.copy() for k, v in params.items()})
    if not bf16:
        m.history_hook = _round_hook
    return m


def _steps(case, m, steps, slot, training=True):
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.scheduler import StagingSlot
    sch = mc.make_scheduler(case, 1)
    slots = [StagingSlot(pin=True) for _ in range(3)] if slot else None
    outs = []
    for step in range(steps):
        if sch.start >= sch.data.shape[0]:
            sch.start = 0
        pb = sch.minibatch_packed(case['cfg']['batch'], FLAGS.plan_t, slots[step % 3] if slot else None)
        if training:
            pb.dropout = case['flags']['dropout']
            out = m.run_one_step(None, pb, sync=False)
            outs.append((out[1].clone(), out[2].clone()))
        else:
            o = m.run_one_step(None, pb, sync=True)
            outs.append((o[0], o[1], np.array(o[2])))
    torch.cuda.synchronize()
    return outs


def _histories_agree(ref, m):
    """widen(H16) == H32, bit for bit, for every layer; and something was written"""
    from stochastic_gcn_amd import ops
    assert len(ref.history) == len(m.history) > 0
    for hr, hm in zip(ref.history, m.history):
        assert hr[0].dtype == torch.float32 and hm[0].dtype == torch.bfloat16
        assert torch.equal(ops.history_widen(hm[0]).view(torch.int32), hr[0].view(torch.int32))
        wide = (_bits(hm[0]).astype(np.uint32) << 16).view(np.float32)              # ... and by the test's own widening
        assert np.array_equal(wide.view(np.uint32), hr[0].cpu().numpy().view(np.uint32))
    assert any(float(h[0].abs().sum()) > 0 for h in ref.history)


MODEL_CASES = ['reddit_cvd_pp', 'reddit_cv_pp', 'cvd_pp_L3', 'cv_nopp_L2']


@pytest.mark.parametrize("name", MODEL_CASES)
def test_model_equals_the_fp32_model_with_a_rounding_hook(name):
    from stochastic_gcn_amd.step_program import OP
    case = mc.build_case(name)
    params = mc.make_oracle_model(case, seed=3).params
    ref = _model(case, params, False, False)
    lr = _steps(case, ref, 5, False)
    assert not getattr(ref, '_programs', {})
    runs = [("eager", False, (False, True))] + [("program", True, sg) for sg in ((False, True), (True, True), (False, False))]
    for what, native, (slot, group) in runs:
        m = _model(case, params, native, True, (slot, group))
        lm = _steps(case, m, 5, slot)
        tag = "%s %s slot=%s group=%s" % (name, what, slot, group)
        assert torch.equal(ref.theta, m.theta) and torch.equal(ref.adam_m, m.adam_m) and torch.equal(ref.adam_v, m.adam_v), tag
        for (l1, a1), (l2, a2) in zip(lr, lm):
            assert torch.equal(l1, l2) and torch.equal(a1, a2), tag
        assert ref.dropout_step == m.dropout_step == 5 and ref.adam_t == m.adam_t == 5
        _histories_agree(ref, m)
        progs = getattr(m, '_programs', {})
        if not native:
            assert not progs
            continue
        assert progs and all(p is not None for p in progs.values()), getattr(m, '_program_note', 'no program was compiled')
        n_agg = sum(1 for l in m.layers if type(l).__name__ == 'VRAggregator')
        for p in progs.values():
            codes = [o for o, _ in p.ops_fb + p.ops_opt + p.ops_hist]
            assert not any(OP[o] in codes for o in ('VR_AGG', 'VR_AGG_PRE', 'VR_AGG_POST', 'SCATTER_ROWS', 'AUX_SCATTER_ROWS'))
            if group:
                assert codes.count(OP['VR_AGG_H16']) == n_agg and codes.count(OP['SCATTER_ROWS_H16']) == n_agg
            else:                                   # the agg_overlap two-phase form, the scatter on the auxiliary stream
                assert codes.count(OP['VR_AGG_PRE_H16']) == n_agg == codes.count(OP['VR_AGG_POST_H16'])
                assert codes.count(OP['AUX_SCATTER_ROWS_H16']) == n_agg and OP['VR_AGG_H16'] not in codes


def test_evaluation_model_as_a_program_equals_the_hooked_fp32_model():
    """is_training=False with a test history (test_cv): forward, loss, prediction and the test history's scatter over
    three consecutive batches -- the second reads what the first wrote"""
    from stochastic_gcn_amd.step_program import OP
    case = mc.build_case('reddit_cvd_pp')
    params = mc.make_oracle_model(case, seed=3).params
    ref = _model(case, params, False, False, is_training=False)
    o_ref = _steps(case, ref, 3, False, training=False)          # (FLAGS is global: the eager reference runs before m exists)
    assert not getattr(ref, '_programs', {})
    m = _model(case, params, True, True, is_training=False)
    o_m = _steps(case, m, 3, False, training=False)
    progs = list(getattr(m, '_programs', {}).values())
    assert progs and all(p is not None for p in progs), getattr(m, '_program_note', None)
    codes = [o for p in progs for o, _ in p.ops_fb + p.ops_opt + p.ops_hist]
    assert OP['VR_AGG_H16'] in codes and OP['VR_AGG'] not in codes and OP['SCATTER_ROWS'] not in codes
    for (l0, a0, p0), (l1, a1, p1) in zip(o_ref, o_m):
        assert l0 == l1 and a0 == a1 and np.array_equal(p0, p1)
    _histories_agree(ref, m)


# ---- 8: checkpoints ---------------------------------------------------------------------------------------------------------
def test_checkpoints_are_read_across_history_dtypes(tmp_path):
    from stochastic_gcn_amd import ops
    case = mc.build_case('cvd_pp_L3')
    params = mc.make_oracle_model(case, seed=3).params
    a = _model(case, params, True, True)
    _steps(case, a, 3, False)
    assert all(float(ops.history_widen(h[0]).abs().sum()) > 0 for h in a.history)
    path = str(tmp_path / "bf16.ckpt.npz")
    with contextlib.redirect_stdout(io.StringIO()):
        a.save(path=path)
        z = np.load(path)
        b = _model(case, params, False, False)
        b.history_hook = None
        b.load(load_history=True, path=path)
        c = _model(case, params, False, True)
        c.load(load_history=True, path=path)
    for l, (ha, hb, hc) in enumerate(zip(a.history, b.history, c.history)):
        wide = (_bits(ha[0]).astype(np.uint32) << 16).view(np.float32)
        assert z["history/%d" % l].dtype == np.float32 and np.array_equal(z["history/%d" % l].view(np.uint32), wide.view(np.uint32))
        assert np.array_equal(hb[0].cpu().numpy().view(np.uint32), wide.view(np.uint32))       # fp32 model: the widened table
        assert np.array_equal(_bits(hc[0]), _bits(ha[0]))                                       # bf16 model: the table
        assert hc[0].stride(0) % 8 == 0
    assert torch.equal(a.theta, b.theta) and torch.equal(a.theta, c.theta)
    # an fp32 checkpoint read by a bfloat16 model: rounded
    rng = np.random.RandomState(5)
    for h in b.history:
        h[0].copy_(torch.from_numpy(_values(rng, tuple(h[0].shape))).to(h[0].device))
    path32 = str(tmp_path / "fp32.ckpt.npz")
    with contextlib.redirect_stdout(io.StringIO()):
        b.save(path=path32)
        e = _model(case, params, False, True)
        e.load(load_history=True, path=path32)
    for hb, he in zip(b.history, e.history):
        _same_bits(_bits(he[0]), hb[0].cpu().numpy())
        buf = he[0].as_strided((he[0].shape[0], he[0].stride(0)), (he[0].stride(0), 1))
        assert (_bits(buf)[:, he[0].shape[1]:] == 0).all()                                     # pad columns stay zero


# ---- 9: process groups (fresh child processes, each under its own timeout) ------------------------------------------------
def _child(args, timeout):
    import test_parallel_gloo as tg
    port = tg._free_port()
    cmd = [sys.executable] + subprocess._args_from_interpreter_flags() + [WORKERS] + [str(a) if a != "PORT" else str(port) for a in args]
    return subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), timeout, port


def _wait(proc, timeout):
    try:
        out, _ = proc.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        proc.kill()
        proc.communicate()
        pytest.fail("child process exceeded %d s" % timeout)
    assert proc.returncode == 0, out[-4000:]


def test_one_rank_rccl_steps_equal_the_run_without_a_process_group(tmp_path):
    res = {}
    for force, overlap in ((True, True), (True, False), (False, True)):
        out = str(tmp_path / ("rccl%d%d.npz" % (force, overlap)))
        proc, timeout, _ = _child(["rccl", int(force), int(overlap), "PORT", out], 300)
        _wait(proc, timeout)
        res[(force, overlap)] = np.load(out)
    ref = res[(False, True)]
    assert np.abs(bf16_ref.widen_bits(ref["hist"])).sum() > 0
    for mode, r in res.items():
        assert r["used_program"][0] and r["steps"][0] == 3
        np.testing.assert_array_equal(r["theta"], ref["theta"])
        np.testing.assert_array_equal(r["hist"], ref["hist"])


def test_two_rank_gloo_replicas_hold_identical_tables(tmp_path):
    import test_parallel_gloo as tg
    port = tg._free_port()
    outs = [str(tmp_path / ("gloo%d.npz" % r)) for r in range(2)]
    procs = []
    for r in range(2):
        cmd = [sys.executable] + subprocess._args_from_interpreter_flags() + [WORKERS, "gloo", str(r), str(port), outs[r]]
        procs.append(subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    try:
        for p in procs:
            _wait(p, 420)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    r = [np.load(o) for o in outs]
    assert r[0]["steps"][0] == r[1]["steps"][0] == 3 and r[0]["used_program"][0] and r[1]["used_program"][0]
    np.testing.assert_array_equal(r[0]["hist"], r[1]["hist"])
    np.testing.assert_array_equal(r[0]["theta"], r[1]["theta"])
    assert np.abs(bf16_ref.widen_bits(r[0]["hist"])).sum() > 0


# ---- 10: allocation ---------------------------------------------------------------------------------------------------------
def test_a_bf16_model_holds_no_fp32_shadow_of_its_tables():
    import gc
    import scipy.sparse as sp
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.vrgcn import VRGCN
    dev = torch.device('cuda:0')
    n, d, f, classes = 200000, 128, 8, 4
    adj = sp.identity(n, format='csr', dtype=np.float32)
    feats = np.zeros((n, f), np.float32)
    ph = mc.placeholders(2, classes)
    used = {}
    for hd in ('fp32', 'bf16'):
        FLAGS.reset()
        FLAGS.update(normalization='graphsage', hidden1=d, cv=True, cvd=True, degree=1, preprocess=True, num_layers=3,
                     layer_norm=True, history_dtype=hd)
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated(dev)
        with contextlib.redirect_stdout(io.StringIO()) as buf:
            m = VRGCN(3, True, ph, feats, feats, adj, True, is_training=True, device=dev)
        torch.cuda.synchronize()
        used[hd] = torch.cuda.memory_allocated(dev) - base
        assert len(m.history) == 2
        for hs in m.history:
            h = hs[0]
            assert tuple(h.shape) == (n, d)
            if hd == 'bf16':
                assert h.dtype == torch.bfloat16 and h.element_size() == 2 and h.stride(0) % 8 == 0 and h.stride(1) == 1
                assert h.untyped_storage().nbytes() == n * h.stride(0) * 2 and h.data_ptr() % 16 == 0
                assert float(h.float().abs().sum()) == 0.0
            else:
                assert h.dtype == torch.float32
        sizes = [float(x) for x in re.findall(r"History size = (\S+) GB", buf.getvalue())]
        assert sizes == [n * d * (2 if hd == 'bf16' else 4) / 2.0 ** 30] * 2          # the line prints the real bytes
        del m, hs, h
    FLAGS.reset()
    layers = 2
    print("allocated: fp32 %.1f MB, bf16 %.1f MB" % (used['fp32'] / 2 ** 20, used['bf16'] / 2 ** 20))
    assert used['fp32'] - used['bf16'] >= 0.45 * n * d * 4 * layers


# ---- 11: end to end through the command line --------------------------------------------------------------------------
LINES = ('Full pred stdev = ', 'Full grad stdev = ', 'Part pred bias = ', 'Part pred stdev = ', 'Part grad bias = ',
         'Part grad stdev = ')


def test_command_line_trains_saves_and_studies_with_a_bf16_history(tmp_path, monkeypatch, capsys):
    from stochastic_gcn_amd import train
    monkeypatch.chdir(tmp_path)
    common = ['--dataset', 's-cora', '--cv', '--epochs', '1', '--early_stopping', '100', '--batch_size', '64',
              '--test_batch_size', '256', '--hidden1', '16', '--seed', '3']
    size = {}
    for hd in ('fp32', 'bf16'):
        train.main(common + ['--degree', '2', '--history_dtype', hd])
        out = capsys.readouterr().out
        ep = [l for l in out.splitlines() if l.startswith("Epoch:")]
        assert len(ep) >= 2
        for line in ep:
            tok = line.split()
            assert tok[0] == "Epoch:" and tok[2] == "train_loss=" and tok[4] == "train_acc=" and tok[6] == "val_loss="
            assert tok[8] == "val_acc=" and "time=" in tok and "ttime=" in tok and "(sch" in tok and "data" in tok
            assert all(math.isfinite(float(tok[i])) for i in (3, 5, 7, 9))
        assert re.search(r"TF time = .*, g time = .*, G GFLOPS = .*, NN GFLOPS = .*, field sizes = ", out)
        assert re.search(r"Test set results: cost= \d+\.\d{5} accuracy= \d+\.\d{5} mi F1=", out)
        size[hd] = [float(x) for x in re.findall(r"History size = (\S+) GB", out)]
        assert size[hd] and all(s > 0 for s in size[hd])
    assert size['bf16'] == [s / 2 for s in size['fp32']]                  # hidden1 = 16: no pitch padding
    ckpt = np.load(str(tmp_path / 'tmp' / 'model.ckpt.npz'))
    hist = ckpt["history/0"]
    assert hist.dtype == np.float32 and np.abs(hist).sum() > 0
    assert np.array_equal(bf16_ref.round_trip(hist).view(np.uint32), hist.view(np.uint32))      # stored widened: bf16 values
    train.main(common + ['--history_dtype', 'bf16', '--load', '--gradvar', '--test_degree=10000', '--degree=1',
                         '--gradvar_draws', '16'])
    out = capsys.readouterr().out.splitlines()
    at = []
    for label in LINES:
        idx = [i for i, l in enumerate(out) if l.startswith(label)]
        assert len(idx) == 1, (label, out)
        at.append(idx[0])
        assert math.isfinite(float(out[idx[0]][len(label):]))
    assert at == sorted(at) and at == list(range(at[0], at[0] + 6)), out
    assert any(l.startswith('Test set results:') for l in out[at[-1]:])


# ---- 12: the control variate still does its job -------------------------------------------------------------------------
def test_control_variate_on_a_bf16_history_scatters_less_than_neighbour_sampling():
    """The body of tests/test_train_gpu.py::test_control_variate_predictions_scatter_less_than_neighbour_sampling with the
    control-variate leg on a bfloat16 history, under that test's own two inequalities."""
    from stochastic_gcn_amd import synthetic
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.train import Trainer
    data = synthetic.reddit_like(n=6000, m=60000, f=32, classes=6, splits=(3600, 800, 1600), seed=5,
                                 with_features=True, planted=True)
    spread = {}
    for name, flags in (("ns", dict(cv=False, degree=2, test_degree=10000)),
                        ("cv", dict(cv=True, cvd=False, test_cv=False, degree=2, test_degree=10000, history_dtype='bf16'))):
        FLAGS.reset()
        FLAGS.update(dataset='s-reddit', normalization='graphsage', weight_decay=0.0, layer_norm=True, hidden1=64,
                     num_fc_layers=1, batch_size=256, test_batch_size=512, learning_rate=0.01, seed=1, prefetch=2,
                     gradvar=True, dropout=0.0, **flags)
        with contextlib.redirect_stdout(io.StringIO()):
            tr = Trainer(data=data, verbose=False)
            for _ in range(20):
                tr.train_epoch()
        if name == "cv":
            assert tr.train_model.history[0][0].dtype == torch.bfloat16
        ids = np.ascontiguousarray(tr.train_d[:FLAGS.batch_size], dtype=np.int32)

        def draws(sch, model, k):
            out = []
            for _ in range(k):
                feed = sch.batch(ids)
                feed[tr.placeholders['dropout']] = 0.0
                pred, _grad = model.get_pred_and_grad(tr.sess, feed)
                out.append(np.asarray(pred[0] if isinstance(pred, (list, tuple)) else pred, np.float64))
            return np.stack(out)
        exact = draws(tr.eval_sch, tr.test_model, 3)
        assert np.abs(exact - exact[0]).max() <= 1e-5 * np.abs(exact[0]).mean()
        part = draws(tr.train_sch, tr.train_model, 60)
        unit = np.abs(exact[0]).mean()
        spread[name] = (part.std(axis=0).mean() / unit, np.abs(part.mean(axis=0) - exact[0]).mean() / unit)
    FLAGS.reset()
    print(spread)
    assert all(np.isfinite(v) for pair in spread.values() for v in pair)
    assert spread["cv"][0] < 0.5 * spread["ns"][0]
    assert spread["cv"][1] < spread["ns"][1]
