"""The column-aware dealing of the lane-group plans (sgcn_tune "cs_deal") on the GPU: the product of a plan dealt by column
spread is BIT-IDENTICAL to the product of the plan dealt by weight alone -- a row's entries stay in one bin, in column order,
pads touch no accumulator, split rows keep their slots and the fix-up its order -- and both are the oracle's on every row."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
TOL = 1e-4
M, K, ROUND, ALIGN = 3000, 2500, 64, 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


@pytest.fixture(scope="module")
def matrix():
    rng = np.random.RandomState(11)
    a = sp.random(M, K, density=0.02, random_state=rng, format='lil', dtype=np.float32)      # ~150 k nonzeros
    a[7, :] = 1.0                                   # an all-ones hub row (split into pieces)
    a[11, :] = 0.0                                  # an empty row
    a = a.tocsr()
    a.eliminate_zeros()
    a.sort_indices()
    a.data[a.indptr[20] + 1] = -0.0                 # a real -0.0f (the pad marker's bits)
    assert a.indptr[12] == a.indptr[11] and a.indptr[8] - a.indptr[7] == K
    return a


@pytest.fixture(scope="module")
def plans(dev, matrix):
    """(G, deal) -> plan, built once"""
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd._ffi import check, lib
    before = lib.sgcn_tune_get(b"cs_deal")
    out = {}
    try:
        for G in (2, 4):
            for deal in (0, 1):
                check(lib.sgcn_tune(b"cs_deal", deal))
                out[G, deal] = ops.ColumnSweepCSR(matrix, dev, G=G, round_tiles=ROUND, align=ALIGN, warp=False)
    finally:
        check(lib.sgcn_tune(b"cs_deal", before))
    return out


@pytest.fixture(scope="module")
def operands(matrix):
    """d -> (B, rscale, C_in, the fp32 oracle products for beta = 0 and for beta = 0.5 with rscale), computed once"""
    out = {}
    for d in (130, 64):
        rng = np.random.RandomState(d)
        pitch = (d + 7) // 4 * 4                    # rows 16-byte aligned, wider than d
        B = rng.standard_normal((K, pitch)).astype(np.float32)
        rs = rng.rand(M).astype(np.float32)
        c0 = rng.standard_normal((M, pitch)).astype(np.float32)
        ref = onp.spmm(matrix.indptr, matrix.indices, matrix.data, B[:, :d])
        ref2 = onp.spmm(matrix.indptr, matrix.indices, matrix.data, B[:, :d], rscale=rs, C_in=c0[:, :d], beta=0.5)
        out[d] = (B, rs, c0, ref, ref2)
    return out


@pytest.mark.parametrize("pace", [-1, 150], ids=["unpaced", "cs_pace=150"])
@pytest.mark.parametrize("d", [130, 64])
@pytest.mark.parametrize("G", [2, 4])
def test_products_of_the_two_dealings_are_bit_identical(dev, matrix, plans, operands, G, d, pace):
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd._ffi import check, lib
    A0, A1 = plans[G, 0], plans[G, 1]
    assert A0.nfix >= 1 and A1.nfix == A0.nfix and A0.pad_fraction > 0.0 and ("g%dk" % G) in A1.variant(d)
    if G == 2:
        assert A1.ntiles > ROUND and A1.ntiles % ROUND == 0            # several launch rounds per pass
    assert not torch.equal(A0.tile_rows, A1.tile_rows)                # (the plans do differ)
    B, rs, c0, ref, ref2 = operands[d]
    Bd = T(B, dev)[:, :d]
    Bh = ops.operand_round(Bd)
    ref_h = onp.spmm(matrix.indptr, matrix.indices, matrix.data, Bh.float().cpu().numpy())
    try:
        for A in (A0, A1):                           # the plan's own clock: unpaced, or unset so that the forced knob holds
            for b16 in (False, True):
                A.clock(b16).pace.pop(d, None)
                if pace < 0:
                    A.clock(b16).pace[d] = -1
        check(lib.sgcn_tune(b"cs_pace", max(pace, 0)))
        got = []
        for A in (A0, A1):
            c = ops.spmm_cs(A, Bd)
            o2 = T(c0, dev)
            ops.spmm_cs(A, Bd, out=o2[:, :d], rscale=T(rs, dev), beta=0.5)
            ch = ops.spmm_cs(A, Bh)
            got.append((c, o2, ch))
        torch.cuda.synchronize()
    finally:
        check(lib.sgcn_tune(b"cs_pace", 0))
    for x, y in zip(got[0], got[1]):
        assert torch.equal(x, y)
        assert np.array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32))
    c, o2, ch = got[1]
    assert onp.rel_err(c.cpu().numpy(), ref) <= TOL
    assert onp.rel_err(o2[:, :d].cpu().numpy(), ref2) <= TOL
    np.testing.assert_array_equal(o2[:, d:].cpu().numpy(), c0[:, d:])          # the pitch padding is never written
    assert onp.rel_err(ch.cpu().numpy(), ref_h) <= TOL
    assert (c[11] == 0).all()                                                  # the empty row
