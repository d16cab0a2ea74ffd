"""Device-side checking helpers shared by the exact GPU tests (test_sparse_exact_gpu.py, test_dense_exact_gpu.py): operands
and outputs inside NaN-filled buffers, so that a write outside a view or a changed operand is seen, and the comparison
of a result with an exact fp64 value or with a per-element bound."""
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
