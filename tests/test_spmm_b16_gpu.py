"""The bfloat16 dense operand of the static-graph products on the device (include/sgcn.h "bfloat16 dense operand";
sgcn_spmm_csr_b16 / _csr_add_b16 / sgcn_spmm_cs_b16; --full_batch_dtype bf16; ShardedSpMM's bfloat16 all-gather).

1. The contract: each _b16 entry on round_bits(B) gives, bit for bit on every row, what its _f32 entry gives on a 16-byte
   aligned fp32 table of the same element pitch holding widen_bits(round_bits(B)) -- same plan, gidx, rscale, cscale, beta,
   addend and knobs.  The patterns, widths and kernel rotations are those of tests/test_sparse_exact_gpu.py (its PAIRS,
   FUSIONS, CS_FUSIONS and column-range list are imported, so the two files leave out the same (pattern, kernel) pairs),
   plus every pattern on every column-sweep form.  B holds bf16_ref.wide_values (1e-20 .. 1e20, +-inf, subnormals, ties)
   and NaNs; bit patterns are compared, a NaN matching any NaN; the pad columns of the bfloat16 table hold NaN bits.
2. Independent of the fp32 kernels: on dyadic inputs the _b16 result equals the fp64 product bit for bit; on real-valued
   inputs it lies within sparse_cases.fp64_bound of the fp64 product of the ROUNDED operand.
3. Refusals.  4. Full size.  5. The trainer under --full_batch_dtype bf16.  6. Two ranks.
bf16_ref is integer arithmetic on bit patterns and shares nothing with the code under test."""
import contextlib
import functools
import io
import os
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bf16_ref                                        # noqa: E402
import full_batch_cases as fc                          # noqa: E402
import sparse_cases as sc                              # noqa: E402
import test_parallel_gloo as tg                        # noqa: E402  (free port)
import test_sparse_exact_gpu as base                   # noqa: E402  (the fp32 kernels' case lists)
from gpu_checks import Operand, Output, check, f32 as _f32      # noqa: E402
from oracle import oracle_np as onp                    # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4                                             # tests/test_parallel_gpu.py, tests/test_kernels_gpu.py
NAN16 = 0x7FC1                                         # a bfloat16 NaN (pad columns, rows after the table)
RANGE_CASES = [("range_boundary", 130, 2, 0), ("range_boundary", 3, 2, sc.T_SPLIT), ("range_empty", 602, 3, 0),
               ("range_empty", 64, 4, 0), ("row_lengths", 1024, 2, sc.T_SPLIT), ("hot_block", 260, 4, 0),
               ("m4097_k4095", 330, 3, 0), ("star_row", 30, 2, 0)]          # test_spmm_column_range_plan's list


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _pattern(name):
    return sc.pattern(name)


def _seed(*key):
    return zlib.crc32(repr(("b16",) + key).encode()) & 0x7fffffff


def _pitch16(d, pad=0):
    return (d + 7) // 8 * 8 + 8 * pad


class B16(object):
    """fp32 values ``x`` as a bfloat16 operand: ``view`` is rows x d of a uint16 buffer of pitch ``pitch`` (a multiple of
    8) whose pad columns and extra row hold NaN bits; ``twin`` is the fp32 table of the SAME element pitch, 16-byte
    aligned, that holds the widened values (what the contract compares against); ``rounded`` the widened values on the
    host.  All by bf16_ref's integer arithmetic."""

    def __init__(self, x, dev, pitch):
        rows, d = x.shape
        assert pitch % 8 == 0 and pitch >= d
        bits = bf16_ref.round_bits(x)
        host = np.full((rows + 1, pitch), NAN16, np.uint16)
        host[:rows, :d] = bits
        self.buf = torch.from_numpy(host.view(np.int16)).to(dev)
        self.view = self.buf.view(torch.bfloat16)[:rows, :d]
        self.before = self.buf.clone()
        self.rounded = bf16_ref.widen_bits(bits)
        wide = np.full((rows + 1, pitch), np.nan, np.float32)
        wide[:rows, :d] = self.rounded
        self.twin_buf = torch.from_numpy(wide).to(dev)
        self.twin = self.twin_buf[:rows, :d]
        assert self.view.data_ptr() % 16 == 0 and self.twin.data_ptr() % 16 == 0
        assert self.view.stride(0) == self.twin.stride(0) == pitch

    def unchanged(self):
        return torch.equal(self.buf, self.before)


def _wide(rng, shape, nans=3):
    """bf16_ref.wide_values in random order (magnitudes 1e-20 .. 1e20, both signs, the SPECIALS), and a few NaNs"""
    n = int(np.prod(shape))
    if n <= len(bf16_ref.SPECIALS) + nans:
        return rng.standard_normal(shape).astype(np.float32)
    v = bf16_ref.wide_values(n - len(bf16_ref.SPECIALS) - nans, seed=int(rng.randint(1 << 30)))
    v = np.concatenate([v, np.full(nans, np.nan, np.float32)]).astype(np.float32)
    return rng.permutation(v).reshape(shape)


def contract(call, dev, M, d, pitch, Bop, C_in=None, operands=(), what=""):
    """``call(B, out)`` with the fp32 twin and with the bfloat16 table, each on a fresh NaN-sentinelled output: the two
    buffers agree bit for bit (a NaN matching any NaN), nothing outside the view was written, no operand changed."""
    outs = []
    for operand in (Bop.twin, Bop.view):
        o = Output(dev, M, d, pitch, C_in)
        call(operand, o.view)
        torch.cuda.synchronize()
        o.written_inside(what)
        outs.append(o)
    assert Bop.unchanged() and all(op.unchanged() for op in operands), "%s: an operand was modified" % what
    x, y = outs[0].buf, outs[1].buf
    same = (x.view(torch.int32) == y.view(torch.int32)) | (torch.isnan(x) & torch.isnan(y))
    if not bool(same.all()):
        bad = (~same).any(dim=1).nonzero().flatten()
        raise AssertionError("%s: the bf16 entry differs from the fp32 entry on the widened table in %d elements of %d rows, first %s"
                             % (what, int((~same).sum()), int(bad.numel()), bad[:8].tolist()))
    return outs[1]


def _fused(rng, a, d, f, dev, pitch16, dense):
    """the operands of a fusion set (test_sparse_exact_gpu._fused_operands with a bfloat16 B); ``dense(rng, shape)`` draws"""
    M, K = a.shape
    kw = {}
    nB = K + 37 if f.get("gidx") else K
    B = B16(dense(rng, (nB, d)), dev, pitch16)
    if f.get("gidx"):
        kw["gidx"] = rng.choice(nB, K, replace=False).astype(np.int32)
    if f.get("rscale"):
        kw["rscale"] = f["scales"](rng, M)
    if f.get("cscale"):
        kw["cscale"] = f["scales"](rng, K)
    C = None
    if f.get("beta"):
        kw["beta"] = f["beta"]
        C = f["cin"](rng, (M, d))
        kw["C_in"] = C
    add = None
    if f.get("add"):
        add = Operand(f["cin"](rng, (M, d)), dev, d + 2)
        kw["add"], kw["add_rows"] = add.view.cpu().numpy(), max(M - 3, 1)
    return B, kw, C, add


REAL = dict(scales=lambda rng, n: (rng.rand(n) + 0.5).astype(np.float32),
            cin=lambda rng, s: rng.standard_normal(s).astype(np.float32))
EXACT = dict(scales=lambda rng, n: sc.pow2(rng, n), cin=lambda rng, s: sc.ints(rng, s))


def _dev_kw(kw, dev):
    return {k: _f32(kw.get(k), dev) for k in ("gidx", "rscale", "cscale")}


def _set_pace(A, d, pace):
    A.pace[d] = pace                      # the two operand types keep clocks of their own: the contract runs both on the same
    A.pace_b16[d] = pace


# ==== 1. the contract ======================================================================================================
@pytest.mark.parametrize("name,d", base.PAIRS)
@pytest.mark.parametrize("plan", ["none", "T", "default"])
def test_contract_row_gather(dev, name, d, plan):
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(_seed(name, d, plan))
    a = sc.normalised(_pattern(name))
    A = ops.DeviceCSR.from_scipy(a, dev, plan_T=sc.T_SPLIT if plan == "T" else 0, with_plan=plan != "none")
    for pad, ldc in ((0, d + 1), (1, (d + 3) // 4 * 4 + 4)):           # scalar / narrow lanes and the widest the width allows
        B = B16(_wide(rng, (a.shape[1], d)), dev, _pitch16(d, pad))
        contract(lambda X, out: ops.spmm(A, X, out=out), dev, a.shape[0], d, ldc, B,
                 what="spmm %s d=%d plan=%s ldc=%d" % (name, d, plan, ldc))


@pytest.mark.parametrize("name,d", [("row_lengths", 66), ("sched_adj", 128), ("star_col", 3), ("m4097_k4095", 602)])
@pytest.mark.parametrize("fi", range(len(base.FUSIONS)))
def test_contract_row_gather_fusions(dev, name, d, fi):
    from stochastic_gcn_amd import ops
    f = dict(base.FUSIONS[fi], **REAL)
    rng = np.random.RandomState(_seed(name, d, fi))
    a = sc.normalised(_pattern(name))
    A = ops.DeviceCSR.from_scipy(a, dev, plan_T=sc.T_SPLIT)
    B, kw, C, add = _fused(rng, a, d, f, dev, _pitch16(d, 1), _wide)
    t = _dev_kw(kw, dev)
    contract(lambda X, out: ops.spmm(A, X, out=out, beta=kw.get("beta", 0.0), d=d, add=None if add is None else add.view,
                                     add_rows=kw.get("add_rows", 0), **t),
             dev, a.shape[0], d, d + 2, B, C_in=C, operands=[add] if add is not None else [],
             what="spmm fusions %s %s" % (name, base.FUSIONS[fi]))


def _split_T(name):
    return sc.T_SPLIT if name in ("row_lengths", "one_row", "star_row") else 0


@pytest.mark.parametrize("i", range(len(base.PAIRS)))
def test_contract_column_sweep(dev, i):
    """test_spmm_column_sweep's rotation: every pattern x width pair with G = 1 / 2 / 4, warp True / False / 'auto', a fusion
    set, at a pace and unpaced"""
    from stochastic_gcn_amd import ops
    name, d = base.PAIRS[i]
    G, warp = (1, 2, 4)[i % 3], (True, False, 'auto')[(i // 3) % 3]
    f = dict(base.CS_FUSIONS[i % len(base.CS_FUSIONS)], **REAL)
    pitch = (d + 3) // 4 * 4 + 4 * (i % 2)
    rng = np.random.RandomState(_seed(name, d, "cs"))
    a = sc.normalised(_pattern(name))
    A = ops.ColumnSweepCSR(a, dev, G=G, warp=warp, T=_split_T(name))
    B, kw, C, _ = _fused(rng, a, d, f, dev, _pitch16(d, i % 2), _wide)
    t = _dev_kw(kw, dev)
    for pace in (-1, (150, 300)[i % 2]):
        _set_pace(A, d, pace)
        contract(lambda X, out: ops.spmm_cs(A, X, out=out, beta=kw.get("beta", 0.0), **t), dev, a.shape[0], d, pitch, B,
                 C_in=C, what="spmm_cs %s d=%d G=%d warp=%s pace=%d" % (name, d, G, warp, pace))


# every column-sweep kernel form: (G, d, warp table, cs_g2_wide forced, the fifth plane expected)
FORMS = [(1, 256, False, 0, False), (1, 300, True, 0, True), (1, 602, 'auto', 0, True), (1, 130, True, 0, False),
         (2, 130, True, 0, False), (2, 602, False, 0, False), (2, 260, True, 1, False), (2, 66, False, 1, False),
         (4, 66, False, 0, False), (4, 256, True, 1, False), (4, 330, 'auto', 0, False), (4, 30, False, 1, False)]


@pytest.mark.parametrize("fi", range(len(FORMS)))
@pytest.mark.parametrize("name", sorted(sc.CATALOGUE))
def test_contract_every_pattern_on_every_column_sweep_form(dev, name, fi):
    from stochastic_gcn_amd import _ffi, ops
    G, d, warp, wide, extra = FORMS[fi]
    pi = sorted(sc.CATALOGUE).index(name)
    f = dict(base.CS_FUSIONS[(pi + fi) % len(base.CS_FUSIONS)], **REAL)
    rng = np.random.RandomState(_seed(name, fi))
    a = sc.normalised(_pattern(name))
    A = ops.ColumnSweepCSR(a, dev, G=G, warp=warp, T=_split_T(name))
    kernel = A.variant(d, bf16=True).split(" x ")[0]
    assert ("g2k" in kernel) == (G == 2) and ("g4k" in kernel) == (G == 4) and "[bf16 operand]" in kernel
    if G == 1:
        assert ("true>" in kernel) == extra, kernel
    B, kw, C, _ = _fused(rng, a, d, f, dev, _pitch16(d, (pi + fi) % 2), _wide)
    t = _dev_kw(kw, dev)
    pitch = (d + 3) // 4 * 4 + 4 * (pi % 2)
    _ffi.tune("cs_g2_wide", wide)
    try:
        for pace in (-1, 200):
            _set_pace(A, d, pace)
            contract(lambda X, out: ops.spmm_cs(A, X, out=out, beta=kw.get("beta", 0.0), **t), dev, a.shape[0], d, pitch, B,
                     C_in=C, what="spmm_cs %s form %s pace=%d" % (name, FORMS[fi], pace))
    finally:
        _ffi.tune("cs_g2_wide", 0)


@pytest.mark.parametrize("name,d,NR,T", RANGE_CASES)
def test_contract_column_range_plan(dev, name, d, NR, T):
    from stochastic_gcn_amd import ops
    for fi in (0, 4):
        rng = np.random.RandomState(_seed(name, d, NR, fi))
        a = sc.normalised(_pattern(name))
        A = ops.ColumnSweepCSR(a, dev, T=T, col_ranges=NR)
        assert A.ranged == NR
        B, kw, C, _ = _fused(rng, a, d, dict(base.CS_FUSIONS[fi], **REAL), dev, _pitch16(d, 1), _wide)
        t = _dev_kw(kw, dev)
        pitch = (d + 3) // 4 * 4 + 4
        for pace in (-1, 250):
            _set_pace(A, d, pace)
            contract(lambda X, out: ops.spmm_cs(A, X, out=out, beta=kw.get("beta", 0.0), **t), dev, a.shape[0], d, pitch, B,
                     C_in=C, what="ranged %s NR=%d pace=%d" % (name, NR, pace))


def test_history_table_is_an_operand(dev):
    """a table of ops.history_alloc(bf16=True), filled by the one rounding kernel, is directly usable as B"""
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(5)
    a = sc.normalised(_pattern("rmat"))
    K, d = a.shape[1], 30
    x = rng.standard_normal((K, d)).astype(np.float32)
    H = ops.history_alloc(K, d, dev, bf16=True)
    assert ops.operand_round(torch.from_numpy(x).to(dev), out=H) is H
    assert np.array_equal(H.contiguous().view(torch.int16).cpu().numpy().view(np.uint16), bf16_ref.round_bits(x))
    wide = torch.zeros((K, 32), device=dev)
    wide[:, :d] = torch.from_numpy(bf16_ref.round_trip(x)).to(dev)
    for A, mm in ((ops.DeviceCSR.from_scipy(a, dev), ops.spmm), (ops.ColumnSweepCSR(a, dev, G=2), ops.spmm_cs)):
        out = torch.zeros((a.shape[0], 32), device=dev)[:, :d]
        got = mm(A, H, out=out).contiguous().view(torch.int32).clone()
        want = mm(A, wide[:, :d], out=out).contiguous().view(torch.int32)
        assert torch.equal(got, want)


# ==== 2. independent of the fp32 kernels ====================================================================================
def _independent(a_pat, d, rng_key, dev, make, call, fusion, pitch):
    for exact in (True, False):
        rng = np.random.RandomState(_seed(rng_key, exact))
        a = sc.dyadic(a_pat, rng) if exact else sc.normalised(a_pat)
        A = make(a)
        f = dict(fusion, **(EXACT if exact else REAL))
        dense = (lambda r, s: sc.ints(r, s)) if exact else (lambda r, s: r.standard_normal(s).astype(np.float32))
        B, kw, C, add = _fused(rng, a, d, f, dev, _pitch16(d, 1), dense)
        Bh = B.view.float().cpu().numpy()
        assert np.array_equal(Bh, B.rounded)                                     # (torch's widening is the contract's)
        if exact:
            assert np.array_equal(bf16_ref.round_trip(Bh), Bh)                    # bfloat16 holds these operands exactly
            ref, bound = sc.spmm_exact(a, Bh, **kw), None
        else:
            ref, bound = sc.spmm_f64(a, Bh, **kw), sc.fp64_bound(a, Bh, **kw)     # of the ROUNDED operand
        t = _dev_kw(kw, dev)
        check(lambda out: call(A, B.view, out, kw, t, add), dev, a.shape[0], d, pitch, ref, bound, C_in=C,
              operands=[B] + ([add] if add is not None else []), what="%s exact=%s" % (rng_key, exact))


def _rows_call(d):
    from stochastic_gcn_amd import ops
    return lambda A, X, out, kw, t, add: ops.spmm(A, X, out=out, beta=kw.get("beta", 0.0), d=d,
                                                  add=None if add is None else add.view, add_rows=kw.get("add_rows", 0), **t)


@pytest.mark.parametrize("i", range(len(base.PAIRS)))
def test_independent_row_gather(dev, i):
    """test_spmm_row_gather's pairs, the plan form in turn"""
    from stochastic_gcn_amd import ops
    name, d = base.PAIRS[i]
    plan = ("none", "T", "default")[i % 3]
    _independent(_pattern(name), d, ("rows", name, d, plan), dev,
                 lambda a: ops.DeviceCSR.from_scipy(a, dev, plan_T=sc.T_SPLIT if plan == "T" else 0, with_plan=plan != "none"),
                 _rows_call(d), {}, d + 1 + i % 2)


@pytest.mark.parametrize("name,d", [("row_lengths", 66), ("sched_adj", 128), ("star_col", 3), ("m4097_k4095", 602)])
@pytest.mark.parametrize("fi", range(len(base.FUSIONS)))
def test_independent_row_gather_fusions(dev, name, d, fi):
    """test_spmm_row_gather_fusions' cases"""
    from stochastic_gcn_amd import ops
    _independent(_pattern(name), d, ("rows fused", name, d, fi), dev, lambda a: ops.DeviceCSR.from_scipy(a, dev, plan_T=sc.T_SPLIT),
                 _rows_call(d), base.FUSIONS[fi], d + 2)


@pytest.mark.parametrize("i", range(len(base.PAIRS)))
def test_independent_column_sweep(dev, i):
    from stochastic_gcn_amd import ops
    name, d = base.PAIRS[i]
    G, warp = (1, 2, 4)[i % 3], (True, False, 'auto')[(i // 3) % 3]
    pace = (-1, 150, 300)[i % 3]

    def make(a):
        A = ops.ColumnSweepCSR(a, dev, G=G, warp=warp, T=_split_T(name))
        A.pace_b16[d] = pace
        return A
    _independent(_pattern(name), d, ("cs", name, d, G), dev, make,
                 lambda A, X, out, kw, t, add: ops.spmm_cs(A, X, out=out, beta=kw.get("beta", 0.0), **t),
                 base.CS_FUSIONS[i % len(base.CS_FUSIONS)], (d + 3) // 4 * 4 + 4 * (i % 2))


@pytest.mark.parametrize("name,d,G", [("rmat", 256, 1), ("sbm", 602, 2), ("row_lengths", 130, 4), ("star_col", 64, 2)])
def test_autotune_tunes_the_type_it_is_handed(dev, name, d, G):
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(_seed(name, d, G))
    a = sc.dyadic(_pattern(name), rng)
    A = ops.ColumnSweepCSR(a, dev, G=G, T=sc.T_SPLIT if name == "row_lengths" else 0)
    B = B16(sc.ints(rng, (a.shape[1], d)), dev, _pitch16(d))
    A.autotune(B.view)
    assert d in A.pace_b16 and A.pace == {} and A.tuned_ms == {} and (A.pace_b16[d] <= 0 or d in A.tuned_ms_b16)
    ref = sc.spmm_exact(a, B.rounded)
    check(lambda out: ops.spmm_cs(A, B.view, out=out), dev, a.shape[0], d, (d + 3) // 4 * 4 + 4, ref, operands=[B],
          what="spmm_cs bf16 autotuned %s G=%d pace=%s" % (name, G, A.pace_b16[d]))
    A.autotune(B.twin)
    assert d in A.pace and d in A.pace_b16


# ==== 3. refusals ==========================================================================================================
def test_refusals(dev):
    from stochastic_gcn_amd import _ffi, ops
    a = sc.normalised(_pattern("m64_k64"))
    M, K = a.shape
    R, S = ops.DeviceCSR.from_scipy(a, dev), ops.ColumnSweepCSR(a, dev, G=2)
    out = torch.zeros((M, 8), device=dev)
    bad = [("ldb % 8", torch.zeros((K, 12), dtype=torch.bfloat16, device=dev)[:, :8]),
           ("16-byte aligned", torch.zeros((K, 16), dtype=torch.bfloat16, device=dev)[:, 1:9])]
    for frag, X in bad:
        for mm, A in ((ops.spmm, R), (ops.spmm_cs, S)):
            with pytest.raises(_ffi.SgcnError) as e:
                mm(A, X, out=out)
            assert e.value.code == -1 and frag in str(e.value), str(e.value)           # SGCN_ERR_INVALID
    X = torch.zeros((K, 8), dtype=torch.bfloat16, device=dev)
    out12 = torch.zeros((M, 12), device=dev)
    plan = S.struct(12, bf16=True)
    import ctypes
    rc = _ffi.lib.sgcn_spmm_cs_b16(ctypes.byref(plan), M, K, 12, X.data_ptr(), 8, None, None, None, out12.data_ptr(), 12, 0.0, None)
    assert rc == -1 and b"ldb >= d" in _ffi.lib.sgcn_last_error()
    rc = _ffi.lib.sgcn_spmm_csr_b16(R.rowptr.data_ptr(), R.col.data_ptr(), R.val.data_ptr(), M, K, 12, X.data_ptr(), 8, None, None,
                                    None, out12.data_ptr(), 12, 0.0, None, None)
    assert rc == -1 and _ffi.lib.sgcn_last_error()
    torch.cuda.synchronize()
    assert not out.any() and not out12.any()                                            # nothing was written


# ==== 4. full size ==========================================================================================================
def test_full_size_bf16_plan_and_transpose_vs_oracle_rows(dev):
    """S-Reddit, d = 602, the autotuned bfloat16 plan and its separately planned and tuned transpose against oracle_np.spmm of
    the ROUNDED operand: the row sample (20 heaviest, 20 emptiest, 1,500 seeded) and criterion (rel_err <= 1e-4) of
    test_kernels_gpu.test_two_lane_group_full_size_vs_oracle_rows."""
    from stochastic_gcn_amd import ops, synthetic
    n, _, full_adj, *_ = synthetic.reddit_like(with_features=False)
    d = 602
    G = ops.ColumnSweepCSR.choose_g(d, full_adj.nnz / n, n)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    full_t = full_adj.T.tocsr()
    full_t.sort_indices()
    for m, what, seed in ((full_adj, "A", 1), (full_t, "A^T", 2)):
        A = ops.ColumnSweepCSR(m, dev, G=G)
        X = torch.randn((n, d), device=dev, generator=g)
        Xb = ops.operand_round(X)
        assert Xb.stride(0) == 608 and Xb.dtype == torch.bfloat16
        best = A.autotune(Xb)
        assert d in A.pace_b16 and d not in A.pace and "[bf16 operand]" in A.variant(d, bf16=True)
        c = ops.spmm_cs(A, Xb)
        assert torch.equal(ops.spmm_cs(A, Xb), c), what + ": two calls differ"
        rounded = bf16_ref.round_trip(X.cpu().numpy())
        assert np.array_equal(Xb.float().cpu().numpy(), rounded), "the rounding kernel is not round-to-nearest-even"
        deg = np.diff(m.indptr)
        rows = np.unique(np.concatenate([np.argsort(deg)[-20:], np.argsort(deg)[:20],
                                         np.random.RandomState(seed).choice(n, 1500, replace=False)]))
        sub = m[rows].tocsr()
        ref = onp.spmm(sub.indptr, sub.indices, sub.data, rounded)
        e = onp.rel_err(c[torch.from_numpy(rows).to(dev)].cpu().numpy(), ref)
        print("bf16 full size %s: G=%d  %.3f ms at pace %s  rel_err %.3e on %d rows" % ((what, G) + tuple(best) + (e, len(rows))))
        assert e <= TOL


# ==== 5. the trainer =======================================================================================================
def _trainer(case, **flags):
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.train import Trainer
    FLAGS.reset()
    FLAGS.update(dataset='ppi' if case['multitask'] else 's-reddit', seed=1, prefetch=0,
                 test_preprocess=case['flags']['preprocess'],
                 **{k: v for k, v in case['flags'].items() if hasattr(FLAGS, k)})
    FLAGS.update(**flags)
    with contextlib.redirect_stdout(io.StringIO()):
        return Trainer(data=case['data'], verbose=False)


def _np(x):
    if isinstance(x, tuple):
        return tuple(_np(t) for t in x)
    if hasattr(x, 'csr'):
        return None
    if hasattr(x, 'materialize'):
        x = x.materialize()
    return x.detach().cpu().numpy()


def _run_trainer(case, kernel, bf16):
    """three --full_batch epochs (one step each, nothing re-based in between) and one --test_full_batch evaluation"""
    tr = _trainer(case, full_batch=True, test_full_batch=True, full_batch_kernel=kernel,
                  full_batch_dtype='bf16' if bf16 else 'fp32')
    assert tr.train_static.matrix.bf16 is bf16 and tr.eval_static.matrix.bf16 is bf16 and tr.train_static.matrix.kernel == kernel
    steps = []
    for _ in range(3):
        tr.train_epoch()
        m = tr.train_model
        steps.append(dict(acts=[_np(a) for a in m.activations[1:]], grads=m.get_grads(), params=m.get_params()))
    ev = tr.evaluate(tr.val_d)
    return steps, tr.test_model.outputs.cpu().numpy(), ev[:2], tr


def _bits_equal(x, y):
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    return x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))


TRAINER_CASES = [(n, k) for n in sorted(fc.CASES) for k in fc.CASES[n]['kernels'] if k != 'lds']


@pytest.mark.parametrize("name,kernel", TRAINER_CASES)
def test_trainer_bf16_equals_fp32_on_round_tripped_operands(name, kernel):
    """--full_batch_dtype bf16 against the same run in fp32 whose StaticMatrix.product round-trips its operand on the HOST
    (bf16_ref) in front of the fp32 product: activations, every gradient, the weights after Adam and the evaluation's
    logits are the same bits.  No tolerance: it follows from the kernel contract."""
    from stochastic_gcn_amd.full_batch import StaticMatrix
    case = fc.build(name)
    got, got_logits, got_ev, tr = _run_trainer(case, kernel, True)
    widths = sorted(tr.train_static.matrix._scratch)
    t_widths = sorted(tr.train_static.matrix.transpose._scratch) if tr.train_static.matrix._transpose is not None else []
    assert widths and all(t.dtype == torch.bfloat16 and t.stride(0) % 8 == 0 for t in tr.train_static.matrix._scratch.values())
    print("%s/%s: scratch tables forward %s, transpose %s" % (name, kernel, widths, t_widths))
    real = StaticMatrix.product
    calls = []

    def product(self, x, out=None, add=None, add_rows=0):
        calls.append(int(x.shape[1]))
        n, d = int(x.shape[0]), int(x.shape[1])
        buf = torch.zeros((n, (d + 7) // 8 * 8), device=x.device)           # (the element pitch of the scratch table)
        buf[:, :d] = torch.from_numpy(bf16_ref.round_trip(x.detach().cpu().numpy())).to(x.device)
        return real(self, buf[:, :d], out=out, add=add, add_rows=add_rows)
    StaticMatrix.product = product
    try:
        want, want_logits, want_ev, _ = _run_trainer(case, kernel, False)
    finally:
        StaticMatrix.product = real
    assert calls, "the reference run never multiplied"
    for step, (g, w) in enumerate(zip(got, want)):
        assert len(g['acts']) == len(w['acts'])
        for li, (x, y) in enumerate(zip(g['acts'], w['acts'])):
            assert (x is None) == (y is None) and (x is None or _bits_equal(x, y)), (name, kernel, step, 'activation', li)
        for what in ('grads', 'params'):
            assert sorted(g[what]) == sorted(w[what])
            for k in g[what]:
                assert _bits_equal(g[what][k], w[what][k]), (name, kernel, step, what, k)
    assert _bits_equal(got_logits, want_logits) and got_ev == want_ev
    # ... and the rounding is really there: the plain fp32 run differs
    plain = _run_trainer(case, kernel, False)[0]
    assert not all(_bits_equal(got[2]['params'][k], plain[2]['params'][k]) for k in got[2]['params'])


def test_scratch_table_is_allocated_once_per_width(dev):
    from stochastic_gcn_amd.full_batch import StaticMatrix
    a = sc.normalised(_pattern("rmat"))
    m = StaticMatrix(a, dev, 'cs', 10, 64, bf16=True)
    x = torch.randn((a.shape[1], 64), device=dev)
    y1 = m.product(x).clone()
    tab = m._scratch[64]
    y2 = m.product(x * 2)
    assert m._scratch[64] is tab and sorted(m._scratch) == [64] and torch.equal(y2, 2 * y1)
    m.product(torch.randn((a.shape[1], 32), device=dev))
    assert sorted(m._scratch) == [32, 64] and m.transpose.bf16 and m.transpose._scratch == {}
    assert 64 in m._plan.pace_b16 and m._plan.pace == {}


# ==== 6. two ranks =========================================================================================================
def _worker(rank, world, port, kernel, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SGCN_DIST_BACKEND="gloo")
    from stochastic_gcn_amd import ops, synthetic
    from stochastic_gcn_amd.parallel import DataParallel, ShardedSpMM
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    par = DataParallel(backend="gloo", device=dev)
    try:
        n, d = 3000, 70
        a = synthetic.rmat_like(n, 30 * n, seed=5)          # same matrix on every rank
        rng = np.random.RandomState(1)
        B = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev)
        dC = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev)
        sh = ShardedSpMM(par, a, dev, kernel=kernel)
        c2 = sh.forward_allgather(B[sh.lo:sh.hi].contiguous(), bf16=True)
        db2 = sh.backward_allgather(dC[sh.lo:sh.hi].contiguous(), bf16=True)
        # the resident operand as a bfloat16 table: all rows rounded here
        c1 = sh.forward(ops.operand_round(B))
        db = sh.backward(ops.operand_round(dC))
        gathered = sh.allgather_rows(B[sh.lo:sh.hi].contiguous(), bf16=True)
        np.savez(os.path.join(out_dir, "r%d.npz" % rank), c1=c1.cpu().numpy(), c2=c2.cpu().numpy(),
                 db=db.cpu().numpy(), db2=db2.cpu().numpy(), lo=np.array([sh.lo]), hi=np.array([sh.hi]),
                 gathered=gathered.contiguous().view(torch.int16).cpu().numpy().view(np.uint16),
                 pitch=np.array([gathered.stride(0)]))
    finally:
        par.shutdown()


@pytest.mark.parametrize("kernel", ["cs", "rows"])
def test_sharded_spmm_two_ranks_bf16(tmp_path, kernel):
    import torch.multiprocessing as mp
    from stochastic_gcn_amd import synthetic
    world, port = 2, tg._free_port()
    mp.spawn(_worker, args=(world, port, kernel, str(tmp_path)), nprocs=world, join=True)
    r = [np.load(os.path.join(str(tmp_path), "r%d.npz" % k)) for k in range(world)]
    n, d = 3000, 70
    a = synthetic.rmat_like(n, 30 * n, seed=5)
    rng = np.random.RandomState(1)
    B = bf16_ref.round_trip(rng.standard_normal((n, d)).astype(np.float32))
    dC = bf16_ref.round_trip(rng.standard_normal((n, d)).astype(np.float32))
    want_c, want_db = a.dot(B.astype(np.float64)), a.T.dot(dC.astype(np.float64))          # SciPy on the rounded operand
    assert r[0]["lo"][0] == 0 and r[0]["hi"][0] == r[1]["lo"][0] and r[1]["hi"][0] == n
    for k in range(world):
        assert np.array_equal(r[k]["gathered"], bf16_ref.round_bits(B)) and r[k]["pitch"][0] == 72
    for key, want in (("c1", want_c), ("c2", want_c), ("db", want_db), ("db2", want_db)):
        got = np.concatenate([r[0][key], r[1][key]], axis=0)      # rank order = vertex order
        assert got.shape == want.shape
        e = onp.rel_err(got, want)
        print("two ranks bf16 %s %s rel_err %.3e" % (kernel, key, e))
        assert e <= TOL, key
    for k in range(world):                                         # gathered and resident operands: the same bits
        assert _bits_equal(r[k]["c1"], r[k]["c2"]) and _bits_equal(r[k]["db"], r[k]["db2"])
