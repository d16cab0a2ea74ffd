"""The two ends of a two- / four-group column-sweep launch that are not on its clock (sgcn_spmm_cs.hip): the prologue of the
dictionary kernels, which copies a tile's value table into LDS in four quarters of 256 floats, and the epilogue's stores to
C rows and workspace slots (cs_store: their cache policy is a build-time choice), at the smallest shapes at which either can
go wrong.

The matrix has 4,000 rows over K = 2^17 columns (table index bits: 10), Poisson(24) nonzeros per row and one hub row of
6,000 that is split (T = 512) into workspace slots and a fix-up; launch rounds of 32 tiles (sgcn_tune "cs_round"), so a
product is four rounds.  Every column occurs once, so the tiles' column sets are disjoint and the value of an entry -- a
function of its column alone -- can be chosen per tile: the tiles listed in TARGETS hold exactly 1, 31 - 33, 255 - 257,
511 - 513 and 1,024 table entries (the quarter boundaries of the copy and the full table; the pad marker is an entry like
any other and every tile of this plan has pads, so the smallest table is one value and the marker), which is asserted from
the plan's tile_nvals.  The dense operand repeats a table of PERIOD rows (a prime), so that the fp64 SciPy reference is the
product of the matrix folded onto that table.

Per case (G, d, beta, fused scalings and gather, operand type): (i) the product on the cs_dict = 1 plan is the product on
the cs_dict = 0 plan bit for bit; (ii) both lie within TOL -- the constant of tests/test_kernels_gpu.py and
tests/test_csplan_deal_gpu.py -- of the fp64 product; (iii) C is a column slice of a wider NaN-filled buffer with rows to
spare, and nothing outside it moves; (iv) a second run gives the same bits."""
import contextlib
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gpu_checks import Output
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu

TOL = 1e-4
N, K, DEG, HUB, T, ROUND, PERIOD = 4000, 1 << 17, 24, 6000, 512, 32, 4099
TARGETS = (1, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1024)
WIDTHS = (4, 130, 602)            # one pass; two passes, ragged last vector; five passes, the last 90 columns wide


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _rounds_of_32():
    """launch rounds of ROUND tiles while this module's tests build plans and multiply (the knob is read at both times)"""
    from stochastic_gcn_amd._ffi import check, lib
    before = lib.sgcn_tune_get(b"cs_round")
    check(lib.sgcn_tune(b"cs_round", ROUND))
    yield
    check(lib.sgcn_tune(b"cs_round", before))


@contextlib.contextmanager
def _knobs(cs_dict):
    from stochastic_gcn_amd._ffi import check, lib
    before = lib.sgcn_tune_get(b"cs_dict")
    try:
        check(lib.sgcn_tune(b"cs_dict", cs_dict))
        yield
    finally:
        check(lib.sgcn_tune(b"cs_dict", before))


def _plan(a, device, G, cs_dict):
    from stochastic_gcn_amd import ops
    with _knobs(cs_dict):
        return ops.ColumnSweepCSR(a, device, G=G, T=T)


@functools.lru_cache(maxsize=None)
def _pattern():
    rng = np.random.RandomState(11)
    deg = rng.poisson(DEG, N).clip(1)
    deg[0] = HUB
    cols = rng.permutation(K)[:deg.sum()]               # every column at most once
    a = sp.csr_matrix((np.ones(cols.size, np.float32), (np.repeat(np.arange(N), deg), cols)), shape=(N, K))
    a.sort_indices()
    return a


def _tile_columns(P):
    """(the real columns, whether there are pads) of every tile of a plan with a value array"""
    tp = P.tile_ptr.cpu().numpy()
    word, val = P.colrow.cpu().numpy().view(np.uint32), P.val.cpu().numpy().view(np.uint32)
    out = []
    for t in range(P.ntiles):
        w, v = word[tp[t]:tp[t + 1]], val[tp[t]:tp[t + 1]]
        out.append((np.unique(w[v != 0x80000000] & np.uint32(0x0FFFFFFF)), bool((v == 0x80000000).any())))
    return out


@functools.lru_cache(maxsize=None)
def _matrix():
    """(matrix, {tile of the two-group plan: length its table must have}): value = palette[index(column)].  The pad marker
    is a table entry like any other (sgcn_csplan.cpp make_dict), so a tile with pads gets one real value less."""
    a = _pattern().copy()
    tiles = _tile_columns(_plan(a, torch.device("cpu"), 2, 0))
    by_size = sorted(range(len(tiles)), key=lambda t: (-tiles[t][0].size, t))
    index = np.zeros(K, np.int64)
    want = {}
    for n, t in zip(sorted(TARGETS, reverse=True), by_size):        # the largest count on the tile with the most columns
        cols, pads = tiles[t]
        real = max(n - int(pads), 1)                                # (n = 1 on a padded tile: one real value, a table of two)
        assert cols.size >= real, "tile %d has %d columns for %d values" % (t, cols.size, real)
        index[cols] = np.arange(cols.size) % real
        want[t] = real + int(pads)
    palette = (0.5 + np.arange(1024) / 4096.0).astype(np.float32)   # 1,024 exact, distinct, nonzero values
    a.data = palette[index[a.indices]]
    return a, want


@functools.lru_cache(maxsize=None)
def _plans(G):
    a, want = _matrix()
    dev = torch.device("cuda:0")
    A0, A1 = _plan(a, dev, G, 0), _plan(a, dev, G, 1)
    for A in (A0, A1):
        assert "rounds of %d tiles" % ROUND in A.variant(602) and A.ntiles >= 2 * ROUND, "at least two launch rounds"
        assert A.nfix >= 1 and A.nslots >= 2, "the hub row must become workspace slots and a fix-up"
    assert A0.dict_bits == 0
    if G == 2:
        assert A1.dict_bits == 10
        nv = A1.tile_nvals.cpu().numpy()
        assert torch.equal(A0.tile_rows, A1.tile_rows)
        for t, n in want.items():                       # the case cannot silently miss a quarter boundary
            assert nv[t] == n, "tile %d holds %d values, not %d" % (t, nv[t], n)
        assert set(TARGETS) - {1} <= set(want.values()) and min(want.values()) <= 2
    return A0, A1


@functools.lru_cache(maxsize=None)
def _host(d):
    """host operands of width d: the tables the device operands repeat, C_in, and the fused vectors"""
    rng = np.random.RandomState(2000 + d)
    return dict(Bs=rng.standard_normal((PERIOD, d)).astype(np.float32), Hs=rng.standard_normal((PERIOD, d)).astype(np.float32),
                C=rng.standard_normal((N, d)).astype(np.float32), rs=(rng.rand(N) + 0.5).astype(np.float32),
                cs=(rng.rand(K) + 0.5).astype(np.float32), gidx=rng.permutation(K + 500)[:K].astype(np.int32))


def _round16(x):
    """fp32 -> the bfloat16 the product rounds an operand to -> fp32 (operand_round works on the device)"""
    from stochastic_gcn_amd import ops
    return ops.operand_round(torch.from_numpy(x).to(torch.device("cuda:0"))).float().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _device(d, fused, bf16):
    """the device operand (K or K + 500 rows repeating the table) at a pitch larger than d, rows 16-byte aligned"""
    from stochastic_gcn_amd import ops
    dev = torch.device("cuda:0")
    h = _host(d)
    rows = K + 500 if fused else K
    table = torch.from_numpy(h["Hs"] if fused else h["Bs"]).to(dev)
    pitch = (d + 7) // 8 * 8 + 8
    buf = torch.full((rows, pitch), float("nan"), device=dev)
    buf[:, :d] = table[torch.arange(rows, device=dev) % PERIOD]
    B = buf[:, :d]
    return ops.operand_round(B) if bf16 else B


@functools.lru_cache(maxsize=None)
def _reference(d, beta, fused, bf16):
    """the fp64 SciPy product: the matrix folded onto the operand's table (column c reads table row (gidx[c] or c) % PERIOD)"""
    a, _ = _matrix()
    h = _host(d)
    table = h["Hs"] if fused else h["Bs"]
    if bf16:
        table = _round16(table)
    src = h["gidx"][a.indices].astype(np.int64) if fused else a.indices.astype(np.int64)
    data = a.data.astype(np.float64) * (h["cs"][a.indices].astype(np.float64) if fused else 1.0)
    folded = sp.csr_matrix((data, src % PERIOD, a.indptr), shape=(N, PERIOD))
    ref = folded.dot(table.astype(np.float64))
    if fused:
        ref *= h["rs"].astype(np.float64)[:, None]
    if beta:
        ref += beta * h["C"].astype(np.float64)
    return ref


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "rscale+cscale+gidx"])
@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("G", [2, 4])
def test_boundary(dev, G, d, beta, fused, bf16):
    from stochastic_gcn_amd import ops
    A0, A1 = _plans(G)
    h = _host(d)
    B = _device(d, fused, bf16)
    kw = dict(beta=beta)
    if fused:
        kw.update(rscale=torch.from_numpy(h["rs"]).to(dev), cscale=torch.from_numpy(h["cs"]).to(dev),
                  gidx=torch.from_numpy(h["gidx"]).to(dev))
    ref = _reference(d, beta, fused, bf16)
    what = "G=%d d=%d beta=%s fused=%s bf16=%s" % (G, d, beta, fused, bf16)
    outs = []
    for A in (A0, A1, A1):                               # value array, tables, tables again
        A.clock(bf16).pace[d] = -1                       # unpaced, no autotune
        o = Output(dev, N, d, (d + 3) // 4 * 4 + 4, h["C"] if beta else None)
        ops.spmm_cs(A, B, out=o.view, **kw)
        torch.cuda.synchronize()
        o.written_inside(what)                           # (iii)
        outs.append(o)
    err = [onp.rel_err(o.host(), ref) for o in outs[:2]]
    print("%s: rel_err value array %.3g, tables %.3g" % (what, err[0], err[1]))
    assert torch.equal(outs[0].bits(), outs[1].bits()), "%s: the product on tables differs from the one on a value array" % what   # (i)
    assert torch.equal(outs[1].bits(), outs[2].bits()), "%s: two runs differ" % what                                              # (iv)
    assert max(err) <= TOL, "%s: %s against the fp64 product" % (what, err)                                                      # (ii)
