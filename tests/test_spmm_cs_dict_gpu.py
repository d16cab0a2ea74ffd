"""Dictionary plans (sgcn_tune "cs_dict", sgcn_csbuild_dict) on the GPU: sgcn_spmm_cs_f32 / _b16 on a plan whose values live
in per-tile tables give the bytes they give on the plan with a value array -- the same value bits reach the same FMAs in the
same order -- unpaced and on forced clocks, with beta, rscale, cscale and gidx, with split rows and with a warp table, at
every width class of the two-group kernel (d = 8, 90, 128, 602), and twice in a row.  Before the first product of a plan its
column words are decoded on the host against the plan with a value array: a wrong column mask must fail there, not as a
gather outside the operand."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from test_csplan_dict import rownorm

pytestmark = pytest.mark.gpu
WIDTHS = (8, 90, 128, 602)
PACES = (-1, 150, 300)                         # unpaced; two forced clocks (ns per step of the heaviest tile)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


def _graph():
    a = rownorm(long_cols=(9, 1234))
    a.data[a.indptr[40] + 2] = -0.0             # a real -0.0f
    return a


def _transposed():
    a = _graph().T.tocsr()
    a.sort_indices()
    return a


def _wide(K, const=False):
    a = rownorm(n=2000, k=K, deg=20, seed=K % 1000, long_rows=(3,))
    if const:
        a.data[:] = 0.25
    return a


def _over():
    """one tile with 2^8 + 1 patterns at K = 2^20: the whole plan keeps its value array"""
    K = 1 << 20
    a = rownorm(n=2000, k=K, deg=20, seed=9, long_rows=())
    a.data[:] = 0.5
    r = int(np.argmax(np.diff(a.indptr) >= 1))
    a = a.tolil()
    a[r, :] = 0
    a[r, np.arange(255) * 3] = (1.0 + np.arange(255) / 1024.0).astype(np.float32)
    a = a.tocsr()
    a.eliminate_zeros()
    a.sort_indices()
    return a


def _skewed():
    """an R-MAT-like column law (a third of the nonzeros in the first sixteenth of the ids): the plan gets a warp table"""
    rng = np.random.RandomState(7)
    n, k, nnz = 4000, 30000, 160000
    rows = np.sort(rng.randint(0, n, nnz))
    cols = np.minimum((k * rng.rand(nnz) ** 3).astype(np.int64), k - 1)
    a = sp.csr_matrix((np.ones(nnz, np.float32), (rows, cols)), shape=(n, k))
    a.data[:] = 1.0
    a.sort_indices()
    deg = np.diff(a.indptr)
    a.data = np.repeat((1.0 / np.maximum(deg, 1)).astype(np.float32), deg)
    return a


def _small_reddit(transposed=False):
    from stochastic_gcn_amd import synthetic
    a = synthetic.reddit_like(n=23296, m=1160000, splits=(15241, 2369, 5533), seed=1, with_features=False)[2].tocsr()
    a.sort_indices()
    deg = np.diff(a.indptr)
    a.data = np.repeat((1.0 / np.maximum(deg, 1)).astype(np.float32), deg)          # row-normalised: one value per row
    if transposed:
        a = a.T.tocsr()
        a.sort_indices()
    return a


# name -> (matrix, table index bits the plan must get (0: it keeps its value array), constructor arguments)
CASES = {
    "graph": (_graph, 10, dict(round_tiles=64)),
    "graph^T": (_transposed, 10, dict(round_tiles=64)),
    "K=2^18-3": (lambda: _wide((1 << 18) - 3), 10, dict(round_tiles=64)),
    "K=2^20": (lambda: _wide(1 << 20), 8, dict(round_tiles=64)),
    "K=2^23": (lambda: _wide(1 << 23, const=True), 5, dict(round_tiles=64)),
    "K=2^23+1 falls back": (lambda: _wide((1 << 23) + 1, const=True), 0, dict(round_tiles=64)),
    "one tile over falls back": (_over, 0, dict(round_tiles=64, T=1024)),
    "skewed, warp table": (_skewed, 10, dict(round_tiles=64, warp=True)),
    "small S-Reddit": (_small_reddit, 10, dict(round_tiles=256)),
    "small S-Reddit^T": (lambda: _small_reddit(True), 10, dict(round_tiles=256)),
}


def _plans(a, dev, kw):
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd._ffi import check, lib
    before = lib.sgcn_tune_get(b"cs_dict")
    out = []
    try:
        for knob in (0, 1):
            check(lib.sgcn_tune(b"cs_dict", knob))
            out.append(ops.ColumnSweepCSR(a, dev, G=2, **kw))
    finally:
        check(lib.sgcn_tune(b"cs_dict", before))
    return out


def _host_decode(a, A0, A1, bits):
    """the CPU decode of tests/test_csplan_dict.py on the very plans the products run on"""
    K = a.shape[1]
    assert A0.dict_bits == 0 and A1.dict_bits == bits
    assert torch.equal(A0.tile_ptr, A1.tile_ptr) and torch.equal(A0.tile_rows, A1.tile_rows) and torch.equal(A0.tile_slots, A1.tile_slots)
    cr = A1.colrow.cpu().numpy().view(np.uint32)
    col = cr & np.uint32((1 << (28 - bits)) - 1) if bits else cr & np.uint32(0x0FFFFFFF)
    assert int(col.max()) < K
    assert np.array_equal(A1.columns_rows(), A0.colrow.cpu().numpy())
    assert np.array_equal(A1.val.cpu().numpy().view(np.uint32), A0.val.cpu().numpy().view(np.uint32))
    if bits:
        nv = A1.tile_nvals.cpu().numpy()
        tile = np.repeat(np.arange(A1.ntiles), np.diff(A1.tile_ptr.cpu().numpy()))
        idx = (cr >> np.uint32(28 - bits)) & np.uint32((1 << bits) - 1)
        assert (idx < nv[tile]).all() and 1 <= nv.max() <= (1 << bits) and A1.tile_vals.numel() == A1.ntiles << bits
        assert A1.struct(64).dev_val is None and "tables of %d" % (1 << bits) in A1.variant(64)


@pytest.mark.parametrize("name", list(CASES))
def test_products_on_tables_are_the_products_on_a_value_array(dev, name):
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd._ffi import check, lib
    make, bits, kw = CASES[name]
    a = make()
    M, K = a.shape
    A0, A1 = _plans(a, dev, kw)
    _host_decode(a, A0, A1, bits)                                       # before anything runs on the device
    if "warp" in kw:
        assert A1.warp is not None
    if name in ("graph", "graph^T"):
        assert A1.nfix >= 2 and A1.pad_fraction > 0.0                    # split rows and pads are present
    g = torch.Generator(device=dev).manual_seed(5)
    rs = torch.rand(M, device=dev, generator=g) + 0.5
    cs = torch.rand(K, device=dev, generator=g) + 0.5
    gidx = torch.randperm(K, device=dev, generator=g).to(torch.int32)
    variants = (dict(), dict(rscale=rs, beta=0.5), dict(cscale=cs), dict(gidx=gidx), dict(gidx=gidx, cscale=cs, rscale=rs, beta=-1.25))
    try:
        for d in WIDTHS:
            pitch = (d + 7) // 4 * 4                                    # rows 16-byte aligned, wider than d
            Bf = torch.randn((K, pitch), device=dev, generator=g)[:, :d]
            c0 = torch.randn((M, pitch), device=dev, generator=g)
            for B in (Bf, ops.operand_round(Bf)):                       # sgcn_spmm_cs_f32, sgcn_spmm_cs_b16
                b16 = B.dtype == torch.bfloat16
                for pace in PACES:
                    for A in (A0, A1):                                  # unpaced, or unset so that the forced knob holds
                        A.clock(b16).pace.pop(d, None)
                        if pace < 0:
                            A.clock(b16).pace[d] = -1
                    check(lib.sgcn_tune(b"cs_pace", max(pace, 0)))
                    for v in variants:
                        outs = []
                        for A in (A0, A1, A1):                          # (the third: a rerun)
                            o = c0.clone()
                            ops.spmm_cs(A, B, out=o[:, :d], **v)
                            outs.append(o)
                        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), (name, d, b16, pace, sorted(v))
                        assert torch.equal(outs[1].view(torch.int32), outs[2].view(torch.int32)), (name, d, b16, pace, sorted(v))
                        assert torch.equal(outs[1][:, d:], c0[:, d:])                       # the pitch padding is never written
                        assert not torch.equal(outs[1][:, :d], c0[:, :d])
            del Bf, c0
        torch.cuda.synchronize()
    finally:
        check(lib.sgcn_tune(b"cs_pace", 0))
