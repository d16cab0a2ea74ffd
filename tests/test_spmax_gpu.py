"""The element-wise neighbour maximum on the device (ops.spmax / ops.spmax_bwd), every row and every cell against
tests/spmax_ref.py.

Forward: C and arg equal the reference bit for bit -- there is no arithmetic, so nothing else is acceptable -- on normal
values, heavy ties, constant columns, all-negative tables, mixed signed zeros and -inf columns, with and without the id
output, whatever the plan cuts (none, the default T, T_SPLIT = 64, T = 1: split rows, two-slot rows, many-slot rows) and
whatever vector width the pitches allow.  Backward: on dyadic gradients every partial sum is exact in any order, so dB
equals the reference bit for bit, with and without the addend; on real-valued gradients every element stays within
(t + 2) 2^-24 sum |terms| of the fp64 sum (spmax_ref.backward_f64).  Operands and results sit in pitched buffers whose pad
columns hold NaN / a sentinel and must come back untouched; results are prefilled with NaN / a sentinel."""
import functools
import zlib

import numpy as np
import pytest
import torch

import sparse_cases as sc
import spmax_ref as ref

pytestmark = pytest.mark.gpu

# (at the odd pitch -- scalar lanes -- 200 is 200 vectors: a lane keeps NV = 4; 260 is 260: NV = 3 and two feature slabs)
WIDTHS = (1, 3, 4, 5, 31, 32, 33, 64, 65, 128, 130, 200, 260)
PLANS = ("none", "default", "T", "1")
SENTINEL = -77

# row_lengths (rows around the split threshold, up to 9 T + 3 entries) at every width; every other pattern at two
PAIRS = [("row_lengths", d) for d in WIDTHS] + [
    ("empty", 3), ("empty", 64), ("one_row", 130), ("one_row", 5), ("identity", 1), ("identity", 128),
    ("permutation", 33), ("permutation", 65), ("star_row", 4), ("star_row", 31), ("star_col", 32), ("star_col", 3),
    ("hot_block", 64), ("hot_block", 5), ("row_vector", 130), ("row_vector", 1), ("col_vector", 65), ("col_vector", 4),
    ("m63_k65", 128), ("m65_k63", 31), ("m4097_k4095", 33), ("rmat", 4)]
assert {d for _, d in PAIRS} == set(WIDTHS)
TOO_LARGE_FOR_T1 = ("rmat", "star_row")            # (one slot per stored entry: 2^20 slots; a fix-up walk over 100,000 slots)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


@functools.lru_cache(maxsize=None)
def _pattern(name):
    a = sc.pattern(name)
    from stochastic_gcn_amd import ops
    return a, ops.transpose_host(a)


def _tables(K, d, rng):
    """the dense tables of the forward checks, by kind"""
    t = {"normal": rng.standard_normal((K, d)).astype(np.float32),
         "ties": rng.randint(-2, 3, (K, d)).astype(np.float32),
         "constant": np.tile(rng.standard_normal((1, d)).astype(np.float32), (K, 1)),
         "negative": -np.abs(rng.standard_normal((K, d))).astype(np.float32) - 0.5}
    z = np.where(rng.rand(K, d) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    z[rng.rand(K, d) < 0.2] = -1.0
    t["zeros"] = z
    inf = rng.standard_normal((K, d)).astype(np.float32)
    inf[:, d // 2] = -np.inf
    inf[rng.rand(K) < 0.3, 0] = -np.inf
    t["inf"] = inf
    return t


@functools.lru_cache(maxsize=None)
def _forward_refs(name, d):
    """(table, C, arg) by kind: computed once per (pattern, width), shared by every plan and pitch, never changed"""
    a, _ = _pattern(name)
    out = {}
    for kind, B in _tables(a.shape[1], d, np.random.RandomState(_seed(name, d))).items():
        C, arg = ref.forward(a, B)
        for x in (B, C, arg):
            x.setflags(write=False)
        out[kind] = (B, C, arg)
    return out


def _pitches(d):
    """odd (scalar lanes), a multiple of 2 only, a multiple of 4 (float4 lanes)"""
    c4 = (d + 3) // 4 * 4
    return (d + 1 if d % 2 == 0 else d + 2, c4 + 2, c4 + 4)


def _padded(x, dev, pitch, fill):
    """(buffer, view): x in the first columns of a pitched buffer whose pad columns hold ``fill``"""
    x = np.asarray(x)
    buf = torch.full((x.shape[0], pitch), fill, dtype=torch.int32 if x.dtype == np.int32 else torch.float32, device=dev)
    view = buf[:, :x.shape[1]]
    view.copy_(torch.tensor(x))
    return buf, view


def _blank(rows, d, dev, pitch, dtype):
    fill = float('nan') if dtype == torch.float32 else SENTINEL
    buf = torch.full((rows, pitch), fill, dtype=dtype, device=dev)
    return buf, buf[:, :d]


def _pad_untouched(buf, d):
    pad = buf[:, d:].cpu().numpy()
    return bool(np.all(np.isnan(pad))) if pad.dtype == np.float32 else bool(np.all(pad == SENTINEL))


def _csr(a, dev, plan):
    from stochastic_gcn_amd import ops
    T = {"none": 0, "default": 0, "T": sc.T_SPLIT, "1": 1}[plan]
    return ops.DeviceCSR.from_scipy(a, dev, plan_T=T, with_plan=plan != "none")


def _cases():
    for name, d in PAIRS:
        for plan in PLANS:
            if plan == "1" and name in TOO_LARGE_FOR_T1:
                continue
            yield name, d, plan


@pytest.mark.parametrize("name,d,plan", list(_cases()))
def test_forward_bits(dev, name, d, plan):
    from stochastic_gcn_amd import ops
    a, _ = _pattern(name)
    A = _csr(a, dev, plan)
    M = a.shape[0]
    if plan == "T" and name == "row_lengths":
        assert A.plan.nfix >= 5                     # T + 1, 2 T, 4 T + 1, 9 T + 3, T + 1: two-slot and many-slot rows
    for kind, (B, C_ref, arg_ref) in _forward_refs(name, d).items():
        for pitch in _pitches(d):
            Bbuf, Bv = _padded(B, dev, pitch, float('nan'))
            Cbuf, Cv = _blank(M, d, dev, pitch, torch.float32)
            abuf, av = _blank(M, d, dev, pitch, torch.int32)
            out, arg = ops.spmax(A, Bv, out=Cv, arg=av)
            what = "spmax %s d=%d plan=%s %s pitch=%d" % (name, d, plan, kind, pitch)
            assert out.data_ptr() == Cv.data_ptr() and arg.data_ptr() == av.data_ptr()
            C = Cv.cpu().numpy()
            assert ref.same_bits(C, C_ref), what
            assert np.array_equal(av.cpu().numpy(), arg_ref), what
            assert _pad_untouched(Cbuf, d) and _pad_untouched(abuf, d), what
            assert ref.same_bits(Bv.cpu().numpy(), B), what
            # an evaluation: no ids asked for, the same values
            C2buf, C2v = _blank(M, d, dev, pitch, torch.float32)
            out2, none = ops.spmax(A, Bv, out=C2v, want_arg=False)
            assert none is None and ref.same_bits(C2v.cpu().numpy(), C_ref) and _pad_untouched(C2buf, d), what
    # the allocating form
    B, C_ref, arg_ref = _forward_refs(name, d)["ties"]
    out, arg = ops.spmax(A, torch.tensor(B).to(dev))
    assert ref.same_bits(out.cpu().numpy(), C_ref) and np.array_equal(arg.cpu().numpy(), arg_ref)
    assert arg.dtype == torch.int32 and tuple(arg.shape) == (M, d)



@functools.lru_cache(maxsize=None)
def _backward_refs(name, d):
    """[(kind, arg, exact?, G, add, add_rows, dB in fp32 or None, dB in fp64, bound)]: computed once per (pattern, width),
    shared by every plan and pitch, never changed.  Dyadic gradients: integers in [-8, 8] times a power of two -- every
    partial sum of an element's terms is a multiple of the grid and stays below 2^24 grid steps (asserted), so fp32 addition
    is exact in any order and the sequential fp32 reference IS the fp64 sum."""
    a, _ = _pattern(name)
    M, K = a.shape
    out = []
    for kind in ("normal", "ties"):
        arg = _forward_refs(name, d)[kind][2]
        rng = np.random.RandomState(_seed(name, d, kind, "bwd"))
        scale = np.float32(2.0 ** int(rng.randint(-3, 4)))
        sets = {True: (sc.ints(rng, (M, d)) * scale, sc.ints(rng, (K, d)) * scale),
                False: (rng.standard_normal((M, d)).astype(np.float32), rng.standard_normal((K, d)).astype(np.float32))}
        for add_rows in (None, K, K // 2):
            for exact, (G, add) in sets.items():
                kw = {} if add_rows is None else dict(add=add, add_rows=add_rows)
                d64, bound = ref.backward_f64(a, G, arg, **kw)
                d32 = None
                if exact:
                    mag = ref.backward_f64(a, np.abs(G), arg, **({} if add_rows is None else dict(add=np.abs(add), add_rows=add_rows)))[0]
                    sc.assert_exact(mag, sc.low_exp(G, add if kw else None), "spmax_bwd %s d=%d" % (name, d))
                    d32 = ref.backward(a, G, arg, **kw)
                    assert np.array_equal(d32.astype(np.float64), d64)
                for x in (G, add, d64, bound):
                    x.setflags(write=False)
                out.append((kind, arg, exact, G, add, add_rows, d32, d64, bound))
    return out


@pytest.mark.parametrize("name,d,plan", list(_cases()))
def test_backward_exact_and_bounded(dev, name, d, plan, capsys):
    from stochastic_gcn_amd import ops
    a, at = _pattern(name)
    At = _csr(at, dev, plan)
    M, K = a.shape
    worst = 0.0
    for kind, arg_ref, exact, G, add, add_rows, d32, d64, bound in _backward_refs(name, d):
        for pitch in _pitches(d):
            abuf, av = _padded(arg_ref, dev, pitch, SENTINEL)
            Gbuf, Gv = _padded(G, dev, pitch, float('nan'))
            obuf, ov = _blank(K, d, dev, pitch, torch.float32)
            addv = None
            if add_rows is not None:
                _, addv = _padded(add, dev, pitch + 4, float('nan'))
            out = ops.spmax_bwd(At, Gv, av, out=ov, add=addv, add_rows=add_rows or 0)
            what = "spmax_bwd %s d=%d plan=%s %s pitch=%d add_rows=%s exact=%s" % (name, d, plan, kind, pitch, add_rows, exact)
            assert out.data_ptr() == ov.data_ptr() and _pad_untouched(obuf, d), what
            dB = ov.cpu().numpy()
            if exact:
                assert ref.same_bits(dB, d32), what
            else:
                assert np.all(np.isfinite(dB)), what
                err = np.abs(dB.astype(np.float64) - d64)
                ratio = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
                worst = max(worst, ratio)
                assert np.all(err <= bound), "%s: worst error / bound %.3f" % (what, ratio)
    with capsys.disabled():
        print("\n[spmax_bwd] %s d=%d plan=%s: worst |error| / bound on real-valued gradients %.4f" % (name, d, plan, worst))
    # the allocating form
    kind, arg_ref, exact, G, add, add_rows, d32, d64, bound = _backward_refs(name, d)[0]
    assert exact and add_rows is None
    out = ops.spmax_bwd(At, torch.tensor(G).to(dev), torch.tensor(arg_ref).to(dev))
    assert ref.same_bits(out.cpu().numpy(), d32)
