"""The epilogue the two- and four-group column-sweep kernels share (sgcn_spmm_cs.hip cs_epilogue): row ids, slots and row
scales of a tile read once per wave and handed to the bins' lanes, the sixteen rows stored back to back, at the smallest
shapes at which it can go wrong.  (The one-group kernel keeps its own row loop: tests/test_sparse_exact_gpu.py.)

The matrix is 40 x 50 with one row of 40 nonzeros and T = 8: that row becomes five workspace slots plus a fix-up beside
unsplit rows, and the second bin is partly empty (entries without a row).  Widths: a ragged last vector (2, 90, 130), a full
one (4, 128, 324), lanes past d, a second pass (130, 324 for G = 2; 90 .. 324 for G = 4).  Every case
runs unpaced, on integer-valued operands (tests/sparse_cases.py: every fp32 sum is exact), and is compared bit for bit with
the fp64 product; the output lies at a pitch larger than d inside a NaN-filled buffer with rows to spare, and
``gpu_checks.check`` asserts that the sentinels survive and that two calls give the same bits."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import sparse_cases as sc
from gpu_checks import Operand, check, f32

pytestmark = pytest.mark.gpu

M, K, LONG, T = 40, 50, 40, 8
GROUPS = (2, 4)
WIDTHS = (2, 4, 90, 128, 130, 324)
SCALINGS = [(0.0, False), (0.5, False), (0.0, True), (0.5, True)]      # (beta, rscale)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _matrix():
    rng = np.random.RandomState(5)
    rows, cols = [np.full(LONG, 7)], [rng.choice(K, LONG, replace=False)]
    for r in range(M):
        if r != 7 and r % 5 != 3:                # (every fifth row stays empty)
            n = 1 + r % 4
            rows.append(np.full(n, r))
            cols.append(rng.choice(K, n, replace=False))
    a = sp.coo_matrix((np.ones(sum(len(c) for c in cols), np.float32), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(M, K)).tocsr()
    a.sort_indices()
    return sc.dyadic(a, rng)


@functools.lru_cache(maxsize=None)
def _plan(G):
    from stochastic_gcn_amd import ops
    A = ops.ColumnSweepCSR(_matrix(), torch.device("cuda:0"), G=G, T=T)
    assert A.nfix == 1 and A.nslots >= 3, "the long row must become >= 3 workspace slots and a fix-up"
    assert bool((A.tile_rows < 0).any()), "the last tile must hold entries without a row"
    return A


@functools.lru_cache(maxsize=None)
def _operands(d):
    """(B, C_in, rscale) of width d on the host: drawn once and shared by every case of that width"""
    rng = np.random.RandomState(1000 + d)
    return sc.ints(rng, (K, d)), sc.ints(rng, (M, d)), sc.pow2(rng, M)


@functools.lru_cache(maxsize=None)
def _reference(d, beta, scaled):
    B, C, rs = _operands(d)
    return sc.spmm_exact(_matrix(), B, rscale=rs if scaled else None, beta=beta, C_in=C if beta else None)


def _pitch(d):
    return (d + 3) // 4 * 4 + 4


def _run(dev, G, d, B_view, operands, what, bf16=False):
    from stochastic_gcn_amd import ops
    A = _plan(G)
    (A.pace_b16 if bf16 else A.pace)[d] = -1                     # unpaced, no autotune
    _, C, rs = _operands(d)
    for beta, scaled in SCALINGS:
        check(lambda out: ops.spmm_cs(A, B_view, out=out, beta=beta, rscale=f32(rs, dev) if scaled else None), dev, M, d,
              _pitch(d), _reference(d, beta, scaled), C_in=C if beta else None, operands=operands,
              what="%s G=%d d=%d beta=%s rscale=%s" % (what, G, d, beta, scaled))


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("G", GROUPS)
def test_epilogue_fp32(dev, G, d):
    B = Operand(_operands(d)[0], dev, _pitch(d))
    _run(dev, G, d, B.view, [B], "cs epilogue fp32")


@pytest.mark.parametrize("G,d", [(2, 130), (4, 90)])
def test_epilogue_bf16(dev, G, d):
    """the bfloat16 operand's instantiations of the same kernels (integers up to 8 are bfloat16 numbers)"""
    ld = (d + 7) // 8 * 8 + 8
    buf = torch.full((K + 1, ld), float("nan"), dtype=torch.bfloat16, device=dev)
    buf[:K, :d] = torch.from_numpy(_operands(d)[0]).to(dev).to(torch.bfloat16)
    before = buf.view(torch.int16).clone()
    _run(dev, G, d, buf[:K, :d], [], "cs epilogue bf16", bf16=True)
    assert torch.equal(buf.view(torch.int16), before), "the bfloat16 operand was modified"
