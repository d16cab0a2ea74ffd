"""The bf16-multiply GEMM on an A that is bfloat16 in memory already (sgcn_gemm_mb16_a16 through ops.gemm_bf16), on the NN
and TN cases of tests/mb16_cases.py -- every reachable plan cell of those two forms: split over K or not, both load classes
on either operand, accumulate, a mask on the operand or on the output.

Contract under test: on a table without subnormal values the result has the BITS of sgcn_gemm_mb16_f32 on the widened
table.  For each case A is the bf16_ref.round_trip of the case's operand, stored in a bfloat16 table of the history's layout
(pitch 8 * ceil(d / 8)) whose padding and spare row hold NaN bits; the fp32 entry runs on the widened copy inside a
NaN-filled buffer.  Both outputs sit in NaN-sentinelled buffers and are compared whole, bit for bit -- so a write outside
the output is seen too -- and on the bf16-representable integer operands the result must also equal the exact product.
No tolerance anywhere."""
import numpy as np
import pytest
import torch

import bf16_ref
import dense_cases as dc
import mb16_cases as mbc
from a16_cases import inputs, knob, operand
from gpu_checks import Operand, Output, compare

pytestmark = pytest.mark.gpu

CASES = [c for c in mbc.CASES if c["form"] in ("NN", "TN")]
NAN16 = 0x7FC5                        # a bfloat16 NaN with a payload


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


class Table(object):
    """fp32 values (bf16-representable) as a bfloat16 table: ``view`` is rows x d at ``shift`` elements into rows of ``pitch``
    elements (default: the history's 8 * ceil(d / 8)); everything around it -- padding and one spare row -- holds NaN bits."""

    def __init__(self, x, dev, pitch=None, shift=0):
        rows, d = x.shape
        pitch = (d + 7) // 8 * 8 if pitch is None else pitch
        assert pitch >= shift + d
        bits = np.full((rows + 1, pitch), NAN16, np.uint16)
        bits[:rows, shift:shift + d] = bf16_ref.round_bits(x)
        assert np.array_equal(bf16_ref.widen_bits(bits[:rows, shift:shift + d]), x), "the operand is not bf16-representable"
        self.buf = torch.from_numpy(bits.view(np.int16)).to(dev)
        self.before = self.buf.clone()
        self.view = self.buf.view(torch.bfloat16)[:rows, shift:shift + d]

    def unchanged(self):
        return torch.equal(self.buf, self.before)


def _both(dev, tab, wide, Bo, ta, M, N, C_in, acc, dk, what):
    """the a16 entry on the table and the f32 entry on the widened copy: two sentinelled outputs, equal in every bit"""
    from stochastic_gcn_amd import ops
    assert tab.view.dtype == torch.bfloat16 and wide.view.dtype == torch.float32
    o16, o32 = Output(dev, M, N, N + 3, C_in), Output(dev, M, N, N + 3, C_in)
    ops.gemm_bf16(tab.view, Bo.view, out=o16.view, trans_a=ta, accumulate=acc, **dk)
    ops.gemm_bf16(wide.view, Bo.view, out=o32.view, trans_a=ta, accumulate=acc, **dk)
    torch.cuda.synchronize()
    o16.written_inside(what)
    assert tab.unchanged() and wide.unchanged() and Bo.unchanged(), "%s: an operand was modified" % what
    diff = int((o16.bits() != o32.bits()).sum())
    print("%s: %d of %d words differ from the fp32-table entry" % (what, diff, o16.buf.numel()))
    assert diff == 0, what
    return o16


@pytest.mark.parametrize("i", range(len(CASES)))
def test_a16_has_the_bits_of_the_f32_entry_on_the_widened_table(dev, i):
    from stochastic_gcn_amd import ops
    c = CASES[i]
    ta, _ = mbc.FORMS[c["form"]]
    M, N, acc = c["M"], c["N"], bool(c.get("accumulate"))
    with knob(c.get("knob", 0)):
        for kind in ("real", "exact"):
            A, B, C_in, kw, keys = inputs(c, kind, i)
            A = bf16_ref.round_trip(A)
            assert not ((A != 0) & (np.abs(A) < 2.0 ** -126)).any()               # no subnormal values: the contract's domain
            tab = Table(A, dev)
            assert tab.view.stride(0) % 8 == 0
            wide = operand(A, dev, c.get("vec_a", "on"), c.get("off_a"), i)
            Bo = operand(B, dev, c.get("vec_b", "on"), c.get("off_b"), i + 1)
            dk = {k: ops.Drop(c[k], key) for k, key in keys.items()}
            what = "gemm_bf16 (bf16 A) %r %s" % (c, kind)
            o = _both(dev, tab, wide, Bo, ta, M, N, C_in, acc, dk, what)
            if kind == "exact":         # bf16-representable integers (mb16_cases.int_range): also the exact product
                compare(o.host(), dc.gemm_exact(A, B, ta, False, C_in, acc, **kw), None, what)


@pytest.mark.parametrize("form,drop", [("NN", None), ("NN", 0.8), ("TN", None), ("TN", 0.5)])
def test_column_offset_view_takes_the_scalar_class(dev, form, drop):
    """A view whose rows start 2-byte- but not 8-byte-aligned (one element into a table of pitch width + 8), its width a
    multiple of 4: only the base keeps it out of the vector class."""
    from stochastic_gcn_amd import ops
    ta, _ = mbc.FORMS[form]
    M, N, K = 132, 33, 40
    rng = np.random.RandomState(11)
    A = bf16_ref.round_trip(rng.standard_normal((K, M) if ta else (M, K)).astype(np.float32))
    B = rng.standard_normal((K, N)).astype(np.float32)
    C_in = rng.standard_normal((M, N)).astype(np.float32)
    tab = Table(A, dev, pitch=A.shape[1] + 8, shift=1)
    assert tab.view.data_ptr() % 8 == 2 and tab.view.stride(0) % 4 == 0 and A.shape[1] % 4 == 0
    wide, Bo = Operand(A, dev, A.shape[1] + 4), Operand(B, dev, N + 1)
    dk = dict(drop_a=ops.Drop(drop, 12345)) if drop else {}
    _both(dev, tab, wide, Bo, ta, M, N, C_in, True, dk, "offset view %s drop %s" % (form, drop))
    # ... and the same values in the aligned table (the vector class) give the same bits
    al = Table(A, dev)
    assert al.view.data_ptr() % 8 == 0
    _both(dev, al, wide, Bo, ta, M, N, C_in, True, dk, "aligned table %s drop %s" % (form, drop))


def test_nt_form_is_refused(dev):
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd._ffi import SgcnError, lib
    a = Table(np.ones((8, 8), np.float32), dev)
    b = torch.ones(8, 8, device=dev)
    out = torch.full((8, 8), float("nan"), device=dev)
    with pytest.raises(SgcnError, match="NT form"):
        ops.gemm_bf16(a.view, b, out=out, trans_b=True)
    assert b"gemm_mb16_a16: the NT form (trans_b) is not provided" in lib.sgcn_last_error()
    with pytest.raises(SgcnError, match=r"\(1, 1\)"):
        ops.gemm_bf16(a.view, b, out=out, trans_a=True, trans_b=True)
    with pytest.raises(TypeError, match="B must be torch.float32"):
        ops.gemm_bf16(b, a.view, out=out)
    with pytest.raises(TypeError, match="out must be torch.float32"):
        ops.gemm_bf16(a.view, b, out=a.view)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and a.unchanged()             # nothing was launched
