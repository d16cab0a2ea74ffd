"""Device-side checking helpers shared by the exact GPU tests (test_sparse_exact_gpu.py, test_dense_exact_gpu.py): operands
and outputs inside NaN-filled buffers, so that a write outside a view or a changed operand is seen, and the comparison
of a result with an exact fp64 value or with a per-element bound.  ``Slab`` (test_rows_exact_gpu.py) is the same idea for
kernels that copy bits or write integers: 32-bit words at any pitch and base offset inside sentinel-filled guards, compared
whole and bit for bit."""
import numpy as np
import torch


class Operand(object):
    """a host array on the device inside a NaN-filled buffer (pitch padding and one row more): ``view`` is what a kernel
    gets; ``unchanged()`` checks afterwards that no bit of the buffer moved.  ``shift``: the view starts that many floats
    into its row (a base pointer off the buffer's alignment)."""

    def __init__(self, x, dev, pitch, shift=0):
        rows, d = x.shape
        self.buf = torch.full((rows + 1, max(pitch, d + shift)), float("nan"), device=dev)
        self.buf[:rows, shift:shift + d] = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        self.view = self.buf[:rows, shift:shift + d]
        self.bits = self.buf.view(torch.int32).clone()

    def unchanged(self):
        return torch.equal(self.buf.view(torch.int32), self.bits)


def f32(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def compare(got, ref, bound=None, what=""):
    """``got`` (fp64 host array) equals ``ref`` bit for bit (bound None) or lies within ``bound`` of it, element by element"""
    if bound is None:
        bad = got != ref
        assert not bad.any(), "%s: %d of %d elements (%d rows, first %s) differ from the exact product" % (
            what, int(bad.sum()), bad.size, int(bad.reshape(bad.shape[0], -1).any(axis=1).sum()),
            np.nonzero(bad.reshape(bad.shape[0], -1).any(axis=1))[0][:8])
    else:
        err = np.abs(got - ref)
        bad = ~(err <= bound)
        assert not bad.any(), "%s: %d elements (rows %s) outside the fp64 bound (worst excess %g)" % (
            what, int(bad.sum()), np.nonzero(bad.reshape(bad.shape[0], -1).any(axis=1))[0][:8],
            float(np.nanmax(np.where(bad, err - bound, 0))))


class Output(object):
    """an output ``rows x d`` (holding ``start``, or NaN) inside a NaN-filled buffer with pitch padding and two rows more;
    ``written_inside()`` checks that nothing outside the view moved"""

    def __init__(self, dev, rows, d, pitch, start=None):
        self.rows, self.d = rows, d
        self.buf = torch.full((rows + 2, max(pitch, d)), float("nan"), device=dev)
        if start is not None:
            self.buf[:rows, :d] = torch.from_numpy(np.ascontiguousarray(start, np.float32)).to(dev)
        self.view = self.buf[:rows, :d]
        self.before = self.buf.view(torch.int32).clone()

    def written_inside(self, what=""):
        after = self.buf.view(torch.int32)
        assert torch.equal(after[:self.rows, self.d:], self.before[:self.rows, self.d:]), \
            "%s: the pitch padding of the output was written" % what
        assert torch.equal(after[self.rows:], self.before[self.rows:]), "%s: rows after the output were written" % what

    def bits(self):
        return self.buf.view(torch.int32).clone()

    def host(self):
        return self.view.double().cpu().numpy()


def check(call, dev, M, d, pitch, ref, bound=None, C_in=None, operands=(), what=""):
    """Run ``call(out)`` twice on a fresh NaN-sentinelled output (holding C_in, when given) and check: the two results are
    bit-identical, the sentinels and the operands are untouched, and the result equals ``ref`` bit for bit (bound None)
    or lies within ``bound`` of it."""
    outs = []
    for _ in range(2):
        o = Output(dev, M, d, pitch, C_in)
        call(o.view)
        torch.cuda.synchronize()
        o.written_inside(what)
        outs.append(o)
    assert torch.equal(outs[0].bits(), outs[1].bits()), "%s: two calls differ" % what
    for op in operands:
        assert op.unchanged(), "%s: an operand was modified" % what
    compare(outs[0].host(), ref, bound, what)
    return outs[0].buf


NAN_BITS = 0x7fc05a5a                               # a NaN with a payload, as an int32
FILL_INT = -7


def _words(x):
    """fp32 or int32 data as int32 words (integers of another width must fit)"""
    x = np.ascontiguousarray(x)
    if x.dtype.kind in "iu" and x.dtype.itemsize != 4:
        assert x.size == 0 or (x.min() >= -2 ** 31 and x.max() < 2 ** 31)
        x = x.astype(np.int32)
    assert x.dtype.itemsize == 4, x.dtype
    return x.view(np.int32)


class Slab(object):
    """``rows x d`` 32-bit words (int32, or the bits of fp32) at a pitch of ``ld`` words, starting ``off`` words past a
    16-byte aligned address, inside a flat buffer filled with a sentinel (a NaN's bits, or -7 for integer outputs): guard
    words in front and behind, the pitch padding, and every row a kernel is not to write.  ``same_as(ref_rows)`` compares
    the WHOLE buffer -- view, padding and guards -- with the start state in which the view holds ``ref_rows``, bit for bit."""

    GUARD = 64

    def __init__(self, dev, rows, d, ld=None, off=0, data=None, fill=NAN_BITS):
        ld = d if ld is None else ld
        assert ld >= d and off >= 0
        self.rows, self.d, self.ld, self.lo = rows, d, ld, self.GUARD + off
        self.start = np.full(self.lo + rows * ld + self.GUARD, fill, np.int32)
        if data is not None:
            self.inside(self.start)[...] = _words(data).reshape(rows, d)
        self.flat = torch.from_numpy(self.start).to(dev)
        assert self.flat.data_ptr() % 16 == 0
        self.ptr = self.flat.data_ptr() + 4 * self.lo

    def inside(self, flat):
        """the rows x d view of a host copy of the buffer"""
        return flat[self.lo:self.lo + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.d]

    def view(self, dtype=torch.float32):
        v = self.flat[self.lo:self.lo + self.rows * self.ld].view(self.rows, self.ld)[:, :self.d]
        return v.view(dtype) if dtype != torch.int32 else v

    def expected(self, ref_rows=None):
        want = self.start.copy()
        if ref_rows is not None:
            self.inside(want)[...] = _words(ref_rows).reshape(self.rows, self.d)
        return want

    def same_as(self, ref_rows=None, what=""):
        got = self.flat.cpu().numpy()
        want = self.expected(ref_rows)
        if not np.array_equal(got, want):
            bad = got != want
            ins = self.inside(bad.copy())
            n_in = int(ins.sum())
            raise AssertionError("%s: %d words differ, %d inside the view (rows %s), %d in padding, guards or rows after it" % (
                what, int(bad.sum()), n_in, np.nonzero(ins.any(axis=1))[0][:8], int(bad.sum()) - n_in))
        return got
