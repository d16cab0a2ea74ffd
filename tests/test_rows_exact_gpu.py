"""Every kernel that moves rows or builds indices, checked bit for bit against NumPy indexing (tests/rows_cases.py).

sgcn_rows.hip -- rows_kernel (fp32 gather / scatter), csr_slice_kernel, csr_slice_indptr_kernel, the transpose index
(t_hist / t_scan / t_place), gather_f32_kernel, scale_rows_kernel, hist_pack / hist_claim / hist_write -- and the
history-scatter workgroups of the optimizer's launch (sgcn_dense.hip adam_stats_kernel), which only a program in which
SCATTER_ROWS follows ADAM reaches: the programs here are built by hand (tests/step_ops.py) and run through sgcn_step_run.

Every case checks: the result equals the reference bit for bit (compared as int32; no comparison has a tolerance); a
second call gives the same bits; the sentinels (a NaN's bits, or -7 in integer outputs) in the pitch padding, in the guard
words in front of and behind every buffer and in the rows a kernel is not to write are untouched; operands are unchanged.
The references are held to the reference implementation's golden slices, the host pass and SciPy by test_rows_cases.py.
Scatter ids are unique apart from the -1 pads (rows_cases.assert_scatter_ids): a condition on the inputs, not a tolerance."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import rows_cases as rc
import step_ops as so
from gpu_checks import FILL_INT, Slab

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 0.01, 0.9, 0.999, 1e-8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


def _lib():
    from stochastic_gcn_amd._ffi import lib
    return lib


def _OPK():
    from stochastic_gcn_amd.step_program import K, OP
    return OP, K


def ints(dev, x, fill=FILL_INT):
    """an int32 vector on the device inside guards"""
    x = np.ascontiguousarray(x, np.int32)
    return Slab(dev, 1, len(x), data=x, fill=fill)


def sync():
    torch.cuda.synchronize()


def dev_patterns(rows, d, base=0):
    """rows_cases.patterns(..., specials=False) for the given row numbers (an int64 device tensor), as int32 bits"""
    c = torch.arange(d, dtype=torch.int64, device=rows.device)[None, :]
    u = ((base + rows[:, None] * 4099 + c + 1) * 2654435761) & 0xffffffff
    return torch.where(u >= (1 << 31), u - (1 << 32), u).to(torch.int32)


def test_device_patterns_equal_the_host_patterns(dev):
    rows = torch.tensor([0, 1, 77, 1018, 232964], dtype=torch.int64, device=dev)
    want = rc.bits(rc.patterns(232965, 9, base=31, specials=False))[rows.cpu().numpy()]
    assert np.array_equal(dev_patterns(rows, 9, 31).cpu().numpy(), want)


# ---- fp32 gather / scatter: one case per cell of launch_rows ----------------------------------------------------------------
def _gather_ids(rng, N, n):
    ids = rng.randint(0, N, n).astype(np.int32)        # a gather may repeat rows
    ids[n // 2] = 0
    if n > 1:
        ids[n - 1] = N - 1
    if n > 3:
        ids[1] = ids[2]
    return ids


def _run_gather(dev, c, via_ops, tag):
    d, n, N = c["d"], c["n"], c["N"]
    rng = np.random.RandomState(rc.seed("gather", tag))
    data, ids = rc.patterns(N, d, base=tag), _gather_ids(rng, N, n)
    table, idx, out = Slab(dev, N, d, c["ldi"], c["in_off"], data), ints(dev, ids), Slab(dev, n, d, c["ldo"], c["out_off"])
    if via_ops:
        from stochastic_gcn_amd import ops
        ops.gather_rows(table.view(), idx.view(torch.int32)[0], out=out.view())
    else:
        assert _lib().sgcn_gather_rows_f32(table.ptr, c["ldi"], idx.ptr, n, d, out.ptr, c["ldo"], None) == 0
    sync()
    what = "gather %r" % (c,)
    got = out.same_as(rc.ref_gather(data, ids), what)
    table.same_as(data, what + ": table"), idx.same_as(ids, what + ": ids")
    return got


def _run_scatter(dev, c, via_ops, tag):
    d, n, N = c["d"], c["n"], c["N"]
    rng = np.random.RandomState(rc.seed("scatter", tag))
    H0, src = rc.patterns(N, d, base=tag), rc.patterns(n, d, base=7000000 + tag)
    ids = rc.unique_ids(rng, N, n, pads=n // 5)
    H, idx, s = Slab(dev, N, d, c["ldo"], c["out_off"], H0), ints(dev, ids), Slab(dev, n, d, c["ldi"], c["in_off"], src)
    if via_ops:
        from stochastic_gcn_amd import ops
        ops.scatter_rows(H.view(), idx.view(torch.int32)[0], s.view())
    else:
        assert _lib().sgcn_scatter_rows_f32(H.ptr, c["ldo"], idx.ptr, n, d, s.ptr, c["ldi"], None) == 0
    sync()
    what = "scatter %r" % (c,)
    got = H.same_as(rc.ref_scatter(H0, ids, src), what)
    s.same_as(src, what + ": source"), idx.same_as(ids, what + ": ids")
    return got


@pytest.mark.parametrize("i", range(len(rc.ROWS_CASES)))
def test_rows_cell(dev, i):
    """the raw entry points, then the same case through ops.gather_rows / ops.scatter_rows (a strided view carries the pitch
    and the shifted base): both equal the reference, so the two calls give the same bits"""
    c = rc.ROWS_CASES[i]
    for run in (_run_gather, _run_scatter):
        a, b = run(dev, c, False, i), run(dev, c, True, i)
        assert np.array_equal(a, b)


def test_rows_edges_and_refusals(dev):
    lib = _lib()
    N, n, d = 40, 9, 12
    rng = np.random.RandomState(rc.seed("edges"))
    data, src = rc.patterns(N, d), rc.patterns(n, d, base=555)
    for name, ids in (("first_last", np.array([0, N - 1, N - 1, 0, 1, N - 2, 0, 0, N - 1], np.int32)),):
        table, idx, out = Slab(dev, N, d, 16, 0, data), ints(dev, ids), Slab(dev, n, d, 13, 1)
        assert lib.sgcn_gather_rows_f32(table.ptr, 16, idx.ptr, n, d, out.ptr, 13, None) == 0
        sync()
        out.same_as(rc.ref_gather(data, ids), name)
    for name, ids in (("all_pads", np.full(n, -1, np.int32)), ("ends", np.array([N - 1, 0, -1, 5, -1, 7, 8, -1, 1], np.int32))):
        H, idx, s = Slab(dev, N, d, 14, 2, data), ints(dev, rc.assert_scatter_ids(ids, N)), Slab(dev, n, d, 12, 0, src)
        assert lib.sgcn_scatter_rows_f32(H.ptr, 14, idx.ptr, n, d, s.ptr, 12, None) == 0
        sync()
        H.same_as(rc.ref_scatter(data, ids, src), name), s.same_as(src, name)
    # nothing to do, and the refusals: a status, and nothing written
    ids = rc.unique_ids(rng, N, n)
    for name, args, ok in (("n0", dict(n=0), True), ("d0", dict(d=0), True), ("ldi<d", dict(ldi=d - 1), False), ("ldo<d", dict(ldo=d - 1), False),
                           ("null in", dict(inp=None), False), ("null ids", dict(idx=None), False), ("null out", dict(out=None), False),
                           ("n<0", dict(n=-1), False), ("d<0", dict(d=-1), False)):
        for scatter in (False, True):
            table, idx = Slab(dev, N, d, 16, 0, data), ints(dev, ids)
            other = Slab(dev, n, d, 16, 0, src)
            a = dict(inp=table.ptr, ldi=16, idx=idx.ptr, n=n, d=d, out=other.ptr, ldo=16)
            a.update(args)
            if scatter:        # (H, ldh, ids, n, d, src, lds): `inp` is the table here too
                st = lib.sgcn_scatter_rows_f32(a["inp"], a["ldi"], a["idx"], a["n"], a["d"], a["out"], a["ldo"], None)
            else:
                st = lib.sgcn_gather_rows_f32(a["inp"], a["ldi"], a["idx"], a["n"], a["d"], a["out"], a["ldo"], None)
            sync()
            assert (st == 0) == ok, (name, scatter, st)
            table.same_as(data, name), other.same_as(src, name), idx.same_as(ids, name)


# ---- the shipped sizes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1019] + rc.reddit_caps()[1:])
def test_reddit_history_rows(dev, n):
    """the Reddit history (232,965 x 128): n = 1,019 and the row capacities a compiled program sizes its fields for"""
    from stochastic_gcn_amd import ops
    N, d = rc.REDDIT_N, rc.REDDIT_HID
    rng = np.random.RandomState(rc.seed("reddit", n))
    ids = rc.unique_ids(rng, N, n, pads=n // 7)
    idt = torch.from_numpy(ids).to(dev)
    live = torch.from_numpy(ids[ids >= 0].astype(np.int64)).to(dev)
    for _ in range(2):
        H = torch.zeros((N, d), device=dev)
        src = dev_patterns(torch.arange(n, device=dev), d, 17)
        ops.scatter_rows(H, idt, src.view(torch.float32))
        sync()
        want = torch.zeros((N, d), dtype=torch.int32, device=dev)
        want[live] = src[torch.from_numpy(np.nonzero(ids >= 0)[0]).to(dev)]
        assert torch.equal(H.view(torch.int32), want)
        g = ops.gather_rows(H, torch.clamp(idt, min=0))
        sync()
        assert torch.equal(g.view(torch.int32), want[torch.clamp(idt, min=0).long()])
        assert torch.equal(H.view(torch.int32), want)


def test_reddit_feature_gather(dev):
    """the feature gather (232,965 x 1,204 at a pitch of 1,204): element offsets up to 2.8 x 10^8"""
    from stochastic_gcn_amd import ops
    N, d = rc.REDDIT_N, rc.REDDIT_FEAT
    X = torch.empty((N, d), dtype=torch.int32, device=dev)
    for lo in range(0, N, 32768):
        X[lo:lo + 32768] = dev_patterns(torch.arange(lo, min(N, lo + 32768), device=dev), d, 3)
    before = X.clone()
    rng = np.random.RandomState(rc.seed("features"))
    for n in (1019, rc.reddit_caps()[0]):
        ids = rc.unique_ids(rng, N, n)
        idt = torch.from_numpy(ids).to(dev)
        outs = []
        for _ in range(2):
            out = Slab(dev, n, d, d + 4)
            ops.gather_rows(X.view(torch.float32), idt, out=out.view())
            sync()
            outs.append(out.same_as(dev_patterns(idt.long(), d, 3).cpu().numpy(), "features n=%d" % n))
        assert np.array_equal(outs[0], outs[1])
    assert torch.equal(X, before)


@pytest.fixture()
def big_table(dev):
    """config 5's history: 10,000,000 x 256 fp32 zeros (10.2 GB), freed after the case"""
    H = torch.zeros((rc.BIG_N, rc.BIG_D), device=dev)
    box = [H]
    del H
    yield box
    box.clear()
    torch.cuda.empty_cache()


def _rows_with_bits(H):
    """the rows of H that hold any non-zero bit (one device reduction per slab of rows), as a sorted int64 host array"""
    hit = []
    Hi = H.view(torch.int32)
    for lo in range(0, Hi.shape[0], 1 << 21):
        nz = (Hi[lo:lo + (1 << 21)] != 0).any(dim=1)
        hit.append(torch.nonzero(nz)[:, 0] + lo)
    return torch.cat(hit).cpu().numpy()


def _check_big(H, ids, want_bits, what):
    """the rows with any non-zero bit are exactly ``ids`` and hold ``want_bits`` (no source row is all zero)"""
    assert np.array_equal(_rows_with_bits(H), np.sort(ids).astype(np.int64)), what + ": the set of rows written"
    assert torch.equal(H.view(torch.int32)[torch.from_numpy(ids.astype(np.int64)).to(H.device)], want_bits), what


def test_big_table_scatter_and_gather(dev, big_table):
    from stochastic_gcn_amd import ops
    H = big_table[0]
    ids = rc.big_ids(300, "rows")
    n = len(ids)
    src = dev_patterns(torch.arange(n, device=dev), rc.BIG_D, 5)
    assert bool((src != 0).any(dim=1).all())
    padded = np.concatenate([ids[:n // 2], np.full(5, -1, np.int32), ids[n // 2:]]).astype(np.int32)
    srcp = torch.cat([src[:n // 2], torch.full((5, rc.BIG_D), 77, dtype=torch.int32, device=dev), src[n // 2:]])
    for _ in range(2):
        ops.scatter_rows(H, torch.from_numpy(padded).to(dev), srcp.view(torch.float32))
        sync()
        _check_big(H, ids, src, "big scatter")
        got = ops.gather_rows(H, torch.from_numpy(ids).to(dev))
        sync()
        assert torch.equal(got.view(torch.int32), src)
        H.zero_()


def test_big_table_history_apply_claim_form(dev, big_table):
    lib = _lib()
    H = big_table[0]
    world, d, cap = 3, rc.BIG_D, 320
    ids = rc.big_ids(200, "apply")
    rng = np.random.RandomState(rc.seed("big apply"))
    blocks, winner = [], {}
    for r in range(world):
        mine = rng.choice(ids, cap - 8 * r, replace=False).astype(np.int32)        # the ranks collide on most vertices
        if r == world - 1:
            mine[:4] = [0, rc.BIG_SPLIT - 1, rc.BIG_SPLIT, rc.BIG_N - 1]
            mine = np.concatenate([mine[:4], np.setdiff1d(mine[4:], mine[:4])])
        rows = rc.patterns(cap, d, base=100000 * (r + 1), specials=False)
        blocks.append(rc.ref_hist_pack(mine, len(mine), rows, d, cap, fill=FILL_INT))
        for k, v in enumerate(mine):
            winner[int(v)] = rc.bits(rows[k])
    recv_h = np.concatenate(blocks)
    touched = np.array(sorted(winner), np.int32)
    want = torch.from_numpy(np.stack([winner[int(v)] for v in touched])).to(dev)
    assert {0, rc.BIG_SPLIT - 1, rc.BIG_SPLIT, rc.BIG_N - 1} <= set(touched.tolist())
    owner = torch.zeros(rc.BIG_N, dtype=torch.int32, device=dev)
    for _ in range(2):
        recv = ints(dev, recv_h)
        assert lib.sgcn_hist_apply_f32(H.data_ptr(), d, recv.ptr, world, cap, d, owner.data_ptr(), None) == 0
        sync()
        _check_big(H, touched, want, "big apply")
        recv.same_as(recv_h, "big apply: receive buffer")
        assert int((owner != 0).sum()) == 0
        H.zero_()


def test_big_table_history_pack_source_rows(dev, big_table):
    """hist_pack reads row i at rows + i * ld: with a pitch of 639,999,000 floats the fifth row starts 2.56 x 10^9 elements
    (1.02 x 10^10 bytes) into the table and the fourth ends past element 2^31 -- the same arithmetic as a shipped pitch with
    10 M rows, at a block small enough to compare whole"""
    lib = _lib()
    flat = big_table[0].view(-1).view(torch.int32)
    ld, n, cap, d = 639999000, 5, 8, 128
    assert (n - 1) * ld + d <= flat.numel() and (n - 1) * ld > (1 << 31) and 4 * ((n - 1) * ld) > 10 ** 10
    rows = rc.patterns(n, d, base=4242)
    for i in range(n):
        flat[i * ld:i * ld + d] = torch.from_numpy(rc.bits(rows[i])).to(dev)
    ids = np.array([0, rc.BIG_SPLIT - 1, rc.BIG_SPLIT, rc.BIG_N - 1, 12345], np.int32)
    for _ in range(2):
        idx, send = ints(dev, ids), Slab(dev, 1, cap * (d + 1), fill=FILL_INT)
        assert lib.sgcn_hist_pack_f32(idx.ptr, n, flat.data_ptr(), ld, d, cap, send.ptr, None) == 0
        sync()
        send.same_as(rc.ref_hist_pack(ids, n, rows, d, cap, FILL_INT), "big pack")


def test_big_table_parked_scatter(dev, big_table):
    OP, K = _OPK()
    H = big_table[0]
    d = rc.BIG_D
    ids = rc.big_ids(300, "parked")
    n = len(ids)
    src = dev_patterns(torch.arange(n, device=dev), d, 9)
    idt = torch.from_numpy(ids).to(dev)
    assert rc.park_cell(d, d, d) == ("park", True)
    for _ in range(2):
        th, g, m, v, want = _adam_operands(dev, 1000, "big")
        prog = [(OP["ADAM"], _adam_args(th, g, m, v, 1000)),
                (OP["SCATTER_ROWS"], [K(H.data_ptr()), K(d), K(idt.data_ptr()), K(n), K(d), K(src.data_ptr()), K(d)])]
        assert so.run(prog) == 0
        sync()
        _check_adam(th, m, v, want, "big parked")
        _check_big(H, ids, src, "big parked scatter")
        H.zero_()


# ---- the optimizer's parked scatter -----------------------------------------------------------------------------------------
def _adam_operands(dev, n, key):
    """theta, grad, m, v of n parameters and what ops.adam_step makes of clones of them (theta, m, v as int32 bits)"""
    from stochastic_gcn_amd import ops
    rng = np.random.RandomState(rc.seed("adam", n, key))
    t = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev) for _ in range(3)]
    th, g, m = t
    v = torch.from_numpy((rng.standard_normal(n) ** 2).astype(np.float32)).to(dev)
    c = [x.clone() for x in (th, g, m, v)]
    ops.adam_step(c[0], c[1], c[2], c[3], LR, B1, B2, EPS)
    sync()
    return th, g, m, v, [c[0].view(torch.int32), c[2].view(torch.int32), c[3].view(torch.int32), g.clone()]


def _adam_args(th, g, m, v, n):
    _, K = _OPK()
    return [K(th.data_ptr()), K(g.data_ptr()), K(m.data_ptr()), K(v.data_ptr()), K(n), so.F(LR), so.F(B1), so.F(B2), so.F(EPS)]


def _check_adam(th, m, v, want, what, g=None):
    for name, got, w in (("theta", th, want[0]), ("m", m, want[1]), ("v", v, want[2])):
        assert torch.equal(got.view(torch.int32), w), "%s: %s differs from ops.adam_step" % (what, name)
    if g is not None:
        assert torch.equal(g, want[3]), what + ": the gradient was modified"


class _Job(object):
    """one history scatter: a table of N rows, n source rows, ids with pads; ``aligned`` = (table, source) on 16 bytes"""

    def __init__(self, dev, d, ldh, lds, n, key, aligned=(True, True), pads=None, N=None):
        rng = np.random.RandomState(rc.seed("job", key))
        self.d, self.ldh, self.lds, self.n = d, ldh, lds, n
        N = (2 * n + 11) if N is None else N
        self.H0, self.src = rc.patterns(N, d, base=rc.seed(key) % 1000), rc.patterns(max(n, 1), d, base=5000000 + rc.seed(key) % 1000)
        self.ids = rc.unique_ids(rng, N, n, pads=(n // 4 if pads is None else pads)) if n else np.zeros(1, np.int32)
        hoff, soff = (0 if aligned[0] else 1 + rc.seed(key) % 3), (0 if aligned[1] else 3 - rc.seed(key) % 3)
        self.H, self.idx, self.s = Slab(dev, N, d, ldh, hoff, self.H0), ints(dev, self.ids), Slab(dev, max(n, 1), d, lds, soff, self.src)

    def op(self, n=None):
        OP, K = _OPK()
        return (OP["SCATTER_ROWS"], [K(self.H.ptr), K(self.ldh), K(self.idx.ptr), K(self.n) if n is None else n, K(self.d),
                                     K(self.s.ptr), K(self.lds)])

    def direct(self):
        assert _lib().sgcn_scatter_rows_f32(self.H.ptr, self.ldh, self.idx.ptr, self.n, self.d, self.s.ptr, self.lds, None) == 0

    def check(self, what):
        ref = rc.ref_scatter(self.H0, self.ids[:self.n], self.src[:self.n]) if self.n else self.H0
        got = self.H.same_as(ref, what + ": table")
        self.s.same_as(self.src, what + ": source"), self.idx.same_as(self.ids, what + ": ids")
        return got


def _run_park(dev, jobs, params, key, parked=True, slots=(), ns=None):
    """[ADAM, SCATTER_ROWS ...] as one program (parked where scatter_park accepts), or [ADAM] alone and the scatters through
    sgcn_scatter_rows_f32 on fresh copies; returns the tables' bits"""
    OP, _ = _OPK()
    js = [_Job(dev, key=(key, k), **j) for k, j in enumerate(jobs)]
    th, g, m, v, want = _adam_operands(dev, params, key)
    if parked:
        assert so.run([(OP["ADAM"], _adam_args(th, g, m, v, params))] + [j.op(None if ns is None else ns[k]) for k, j in enumerate(js)],
                      slots) == 0
    else:
        assert so.run([(OP["ADAM"], _adam_args(th, g, m, v, params))]) == 0
        for j in js:
            j.direct()
    sync()
    what = "%s %r params=%d" % ("parked" if parked else "unparked", jobs, params)
    _check_adam(th, m, v, want, what, g)
    return [j.check(what) for j in js]


@pytest.mark.parametrize("i", range(len(rc.PARK_CASES)))
def test_park_cell(dev, i):
    """one scatter behind the optimizer per cell of scatter_park, accepted (it rides in the optimizer's launch) and refused
    (a launch of its own): twice as a program, once unparked -- the same bits"""
    c = rc.PARK_CASES[i]
    job = dict(d=c["d"], ldh=c["ldh"], lds=c["lds"], n=c["n"], aligned=c["aligned"])
    a, b = _run_park(dev, [job], c["params"], i), _run_park(dev, [job], c["params"], i)
    u = _run_park(dev, [job], c["params"], i, parked=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], u[0])


PARK_PAIRS = [((128, 1019), (256, 7)), ((4, 8), (600, 9)), ((512, 1), (8, 1019)), ((124, 7), (132, 8)), ((256, 9), (128, 16)),
              ((8, 8), (4, 1)), ((600, 1019), (124, 9))]


@pytest.mark.parametrize("i", range(len(PARK_PAIRS)))
def test_park_two_jobs(dev, i):
    """two scatters in one optimizer launch: different widths, tables, pitches and row counts (n below, on and past the 8
    rows of a workgroup), -1 ids among both"""
    (d1, n1), (d2, n2) = PARK_PAIRS[i]
    jobs = [dict(d=d1, ldh=d1 + 4 * (i % 2), lds=d1, n=n1), dict(d=d2, ldh=d2, lds=d2 + 4 * ((i + 1) % 2), n=n2)]
    for j in jobs:
        assert rc.park_cell(j["d"], j["ldh"], j["lds"])[0] == "park"
    params = rc.ADAM_COUNTS[i % len(rc.ADAM_COUNTS)]
    a, b = _run_park(dev, jobs, params, ("pair", i)), _run_park(dev, jobs, params, ("pair", i))
    u = _run_park(dev, jobs, params, ("pair", i), parked=False)
    assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a, b, u))


def test_park_sequences(dev):
    """an empty scatter in front of a real one; a third scatter (its own launch) that still lands; a refused scatter in front
    of one that could ride (both run as their own launches); row counts read from slots; no ids left but pads"""
    _, K = _OPK()
    full = dict(d=128, ldh=128, lds=132, n=1019)
    seqs = [("empty first", [dict(d=128, ldh=128, lds=128, n=0), full, dict(d=256, ldh=260, lds=256, n=9)], None, ()),
            ("third", [full, dict(d=8, ldh=8, lds=8, n=7), dict(d=132, ldh=136, lds=132, n=17)], None, ()),
            ("third after two of 8", [dict(d=4, ldh=4, lds=4, n=8), dict(d=600, ldh=600, lds=600, n=8), dict(d=128, ldh=128, lds=128, n=8)], None, ()),
            ("refused first", [dict(d=30, ldh=32, lds=32, n=9), full], None, ()),
            ("misaligned second", [full, dict(d=128, ldh=128, lds=128, n=9, aligned=(False, True))], None, ()),
            ("all pads", [dict(d=128, ldh=128, lds=128, n=9, pads=9), dict(d=256, ldh=256, lds=256, n=8, pads=8)], None, ()),
            ("slots", [full, dict(d=256, ldh=256, lds=256, n=9)], [so.S(1, 2, -1), so.S(0, 3, 0)], (3, 510))]
    for name, jobs, ns, slots in seqs:
        if ns is not None:
            assert [2 * slots[1] - 1, 3 * slots[0]] == [j["n"] for j in jobs]
        for params in (257, rc.ADAM_COUNTS[-1]):
            a, b = _run_park(dev, jobs, params, name, slots=slots, ns=ns), _run_park(dev, jobs, params, name, slots=slots, ns=ns)
            u = _run_park(dev, jobs, params, name, parked=False)
            assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a, b, u)), name


# ---- slice and row pointer --------------------------------------------------------------------------------------------------
class _Csr(object):
    def __init__(self, dev, d, i, p):
        self.h = (d, i, p)
        self.d, self.i, self.p = Slab(dev, 1, max(len(d), 1), data=d if len(d) else None), ints(dev, i if len(i) else [0]), ints(dev, p)

    def unchanged(self, what):
        d, i, p = self.h
        if len(d):
            self.d.same_as(d, what + ": values"), self.i.same_as(i, what + ": columns")
        self.p.same_as(p, what + ": row pointer")


def _slice_on_device(dev, A, r, with_rows=True, what=""):
    """row pointer by the device pass, then the copy; everything checked against the reference; returns the output slabs"""
    lib = _lib()
    n = len(r)
    o_p, o_d, o_c, o_r = rc.ref_csr_slice(A.h[0], A.h[1], A.h[2], r)
    nnz = int(o_p[-1])
    rd = ints(dev, r if n else [0])
    P = Slab(dev, 1, n + 1, fill=FILL_INT)
    assert lib.sgcn_csr_slice_indptr_dev(n, rd.ptr, A.p.ptr, P.ptr, None) == 0
    sync()
    P.same_as(o_p, what + ": row pointer")
    D, Cc, R = Slab(dev, 1, max(nnz, 1)), Slab(dev, 1, max(nnz, 1), fill=FILL_INT), Slab(dev, 1, max(nnz, 1), fill=FILL_INT)
    assert lib.sgcn_csr_slice_f32(n, rd.ptr, A.d.ptr, A.i.ptr, A.p.ptr, P.ptr, D.ptr, Cc.ptr, R.ptr if with_rows else None, None) == 0
    sync()
    D.same_as(o_d if nnz else None, what + ": values"), Cc.same_as(o_c if nnz else None, what + ": columns")
    R.same_as(o_r if nnz and with_rows else None, what + ": COO rows")
    P.same_as(o_p, what + ": row pointer after the copy"), rd.same_as(r if n else [0], what + ": selection")
    A.unchanged(what)
    return P, D, Cc, R, (o_p, o_d, o_c, o_r)


def test_slice_and_row_pointer_edges(dev):
    d, i, p = rc.csr_with_rows(rc.SLICE_ROW_LENS, rc.SLICE_NCOLS, "slice")
    A = _Csr(dev, d, i, p)
    for name, r in rc.slice_selections(len(p) - 1, np.diff(p)):
        for with_rows in (True, False):
            outs = [_slice_on_device(dev, A, r, with_rows, "slice %s" % name) for _ in range(2)]
            assert all(np.array_equal(a.flat.cpu().numpy(), b.flat.cpu().numpy()) for a, b in zip(outs[0][:4], outs[1][:4]))
    # n = 0: o_p[0] = 0 and nothing else
    P = Slab(dev, 1, 3, fill=FILL_INT)
    assert _lib().sgcn_csr_slice_indptr_dev(0, None, None, P.ptr, None) == 0
    sync()
    P.same_as(np.array([0, FILL_INT, FILL_INT], np.int32), "row pointer n=0")
    assert _lib().sgcn_csr_slice_f32(0, None, None, None, None, None, None, None, None, None) == 0
    for bad in (dict(n=-1), dict(o_p=None)):
        a = dict(n=2, o_p=P.ptr)
        a.update(bad)
        assert _lib().sgcn_csr_slice_indptr_dev(a["n"], A.p.ptr, A.p.ptr, a["o_p"], None) != 0
    sync()
    P.same_as(np.array([0, FILL_INT, FILL_INT], np.int32), "row pointer refusals")


# ---- the transpose index ----------------------------------------------------------------------------------------------------
def _transpose_case(dev, ncols, nnz, kw, what):
    lib = _lib()
    d, i, p = rc.csr_with_nnz(ncols, nnz, (ncols, nnz, sorted(kw.items())), **kw)
    r = np.random.RandomState(rc.seed("perm", ncols, nnz)).permutation(len(p) - 1).astype(np.int32)
    A = _Csr(dev, d, i, p)
    P, D, Cc, R, (o_p, o_d, o_c, o_r) = _slice_on_device(dev, A, r, True, what)        # coo_rows as csr_slice_kernel writes them
    assert len(o_c) == nnz
    t_rowptr, t_row, t_src = rc.ref_transpose(ncols, o_c, o_r)
    T = sp.csr_matrix((o_d, o_c, o_p), shape=(len(r), ncols)).T.tocsr()
    T.sort_indices()
    assert np.array_equal(T.indptr, t_rowptr) and np.array_equal(T.indices, t_row)
    need = int(lib.sgcn_csr_transpose_ws_ints(ncols, nnz))
    assert need == rc.transpose_plan(ncols, nnz)["ws_ints"]
    outs = []
    for _ in range(2):
        TP, TR, TS = (Slab(dev, 1, k, fill=FILL_INT) for k in (ncols + 1, nnz, nnz))
        ws = Slab(dev, 1, need, fill=FILL_INT)
        assert lib.sgcn_csr_transpose_index(ncols, nnz, Cc.ptr, R.ptr, TP.ptr, TR.ptr, TS.ptr, ws.ptr, None) == 0
        sync()
        TP.same_as(t_rowptr, what + ": t_rowptr"), TR.same_as(t_row, what + ": t_row"), TS.same_as(t_src, what + ": t_src")
        Cc.same_as(o_c, what + ": columns"), R.same_as(o_r, what + ": COO rows")
        ws.same_as(ws.inside(ws.flat.cpu().numpy()).copy(), what + ": the guards of the scratch")
        G = Slab(dev, 1, nnz)
        assert lib.sgcn_gather_f32(D.ptr, TS.ptr, nnz, G.ptr, None) == 0
        sync()
        outs.append(G.same_as(T.data, what + ": values in transposed order"))
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("i", range(len(rc.TRANSPOSE_CASES)))
def test_transpose_cell(dev, i):
    ncols, nnz = rc.TRANSPOSE_CASES[i]
    _transpose_case(dev, ncols, nnz, {}, "transpose %d x nnz %d" % (ncols, nnz))


@pytest.mark.parametrize("i", range(len(rc.TRANSPOSE_EDGES)))
def test_transpose_edges(dev, i):
    """empty columns at both ends; every nonzero in one column (the first, the last, one in the middle)"""
    ncols, nnz, kw = rc.TRANSPOSE_EDGES[i]
    _transpose_case(dev, ncols, nnz, kw, "transpose %d x nnz %d %r" % (ncols, nnz, kw))


def test_transpose_empty_and_refusals(dev):
    lib = _lib()
    TP = Slab(dev, 1, 8, fill=FILL_INT)
    assert lib.sgcn_csr_transpose_index(7, 0, None, None, TP.ptr, None, None, None, None) == 0
    sync()
    TP.same_as(np.zeros(8, np.int32), "nnz = 0")
    TP = Slab(dev, 1, 8, fill=FILL_INT)
    for args in ((-1, 5), (7, -1), (7, 1 << 31)):
        assert lib.sgcn_csr_transpose_index(args[0], args[1], TP.ptr, TP.ptr, TP.ptr, TP.ptr, TP.ptr, TP.ptr, None) != 0
    assert lib.sgcn_csr_transpose_index(7, 3, None, TP.ptr, TP.ptr, TP.ptr, TP.ptr, TP.ptr, None) != 0
    sync()
    TP.same_as(None, "refusals")


# ---- gather_f32 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", rc.GATHER_N)
def test_gather_f32(dev, n):
    lib = _lib()
    rng = np.random.RandomState(rc.seed("gather_f32", n))
    m = 100003
    src_h = rc.patterns(1, m, base=n % 1000).ravel()
    idx_h = rng.randint(0, m, n).astype(np.int32)
    idx_h[0] = m - 1
    idx_h[-1] = 0
    if n > 4:
        idx_h[1:4] = [m - 1, 0, idx_h[4]]
    src, idx = Slab(dev, 1, m, data=src_h), ints(dev, idx_h)
    outs = []
    for _ in range(2):
        out = Slab(dev, 1, n)
        assert lib.sgcn_gather_f32(src.ptr, idx.ptr, n, out.ptr, None) == 0
        sync()
        outs.append(out.same_as(rc.ref_gather_f32(src_h, idx_h), "gather_f32 n=%d" % n))
    assert np.array_equal(outs[0], outs[1])
    src.same_as(src_h, "source"), idx.same_as(idx_h, "indices")
    out = Slab(dev, 1, 4)
    assert lib.sgcn_gather_f32(src.ptr, idx.ptr, 0, out.ptr, None) == 0 and lib.sgcn_gather_f32(src.ptr, idx.ptr, -1, out.ptr, None) != 0
    assert lib.sgcn_gather_f32(None, idx.ptr, 4, out.ptr, None) != 0 and lib.sgcn_gather_f32(src.ptr, None, 4, out.ptr, None) != 0
    sync()
    out.same_as(None, "gather_f32 refusals")


# ---- scale_rows -------------------------------------------------------------------------------------------------------------
def _scales(rng, n):
    """0, -0, -1, powers of two (exact products) and values whose products round"""
    s = rng.standard_normal(n).astype(np.float32)
    fixed = np.array([0.0, -1.0, 2.0, 0.5, -0.0, 1024.0, 1.0 / 3.0, 2.0 ** -20, -3.0, 1.0], np.float32)
    s[:min(n, len(fixed))] = fixed[:n]
    return s


@pytest.mark.parametrize("i", range(len(rc.SCALE_CASES)))
def test_scale_rows(dev, i):
    """out = s (.) x, out of place (both pointers are __restrict__), pitched on both sides.  One fp32 multiply per element:
    NumPy's fp32 product is the same IEEE operation, so the comparison is exact.  The inputs are standard normals
    (|x| >= 2^-40 or so, < 2^3) and scales in [2^-20, 2^10] or 0, so no product is subnormal or overflows and the result
    does not depend on a denormal mode; zero times a negative gives -0 on both sides."""
    lib = _lib()
    c = rc.SCALE_CASES[i]
    n, d = c["n"], c["d"]
    rng = np.random.RandomState(rc.seed("scale", i))
    x_h, s_h = rng.standard_normal((n, d)).astype(np.float32), _scales(rng, n)
    ref = rc.ref_scale_rows(x_h, s_h)
    mag = np.abs(ref[ref != 0])
    assert mag.size == 0 or (mag.min() >= 2.0 ** -100 and mag.max() < 2.0 ** 100)
    x, s = Slab(dev, n, d, c["ldx"], 0, x_h), Slab(dev, 1, n, data=s_h)
    outs = []
    for _ in range(2):
        out = Slab(dev, n, d, c["ldo"])
        assert lib.sgcn_scale_rows_f32(x.ptr, c["ldx"], s.ptr, n, d, out.ptr, c["ldo"], None) == 0
        sync()
        outs.append(out.same_as(ref, "scale_rows %r" % (c,)))
    assert np.array_equal(outs[0], outs[1])
    x.same_as(x_h, "x"), s.same_as(s_h, "s")


def test_scale_rows_refusals(dev):
    lib = _lib()
    n, d = 9, 10
    x_h = np.random.RandomState(2).standard_normal((n, d)).astype(np.float32)
    xo = Slab(dev, n, d, 12, 1, x_h)             # a base 4 bytes off
    x, s, out, oo = Slab(dev, n, d, 12, 0, x_h), Slab(dev, 1, n, data=np.ones(n, np.float32)), Slab(dev, n, d, 12), Slab(dev, n, d, 12, 2)
    call = lambda **k: lib.sgcn_scale_rows_f32(k.get("x", x.ptr), k.get("ldx", 12), k.get("s", s.ptr), k.get("n", n), k.get("d", d),
                                               k.get("out", out.ptr), k.get("ldo", 12), None)
    assert call(n=0) == 0 and call(d=0) == 0
    for bad in (dict(ldx=10), dict(ldo=14), dict(ldx=8), dict(ldo=8), dict(x=xo.ptr), dict(out=oo.ptr), dict(x=None), dict(s=None),
                dict(out=None), dict(n=-1), dict(d=-1)):
        assert call(**bad) != 0, bad
    sync()
    out.same_as(None, "refusals"), oo.same_as(None, "refusals"), x.same_as(x_h, "x")


# ---- the history exchange ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(rc.EXCHANGE_CASES)))
def test_history_exchange(dev, i):
    """pack every rank's block, then apply the gathered buffer: without the owner table (one scatter launch per rank, each
    payload picking its vector width from where cap, d and the rank put it) and with it (the claim form from three ranks
    on; with one or two ranks the per-rank form even so).  The ranks draw their ids from a quarter of the vertices, so they
    collide; the higher rank wins; both forms give the same table and leave the owner table zero."""
    lib = _lib()
    c = rc.EXCHANGE_CASES[i]
    world, d, cap, ldh = c["world"], c["d"], c["cap"], c["ldh"]
    per = cap * (d + 1)
    N = 4 * cap + 12
    rng = np.random.RandomState(rc.seed("exchange", i))
    recv = Slab(dev, 1, world * per, fill=FILL_INT)
    blocks = []
    for r, n in enumerate(c["sizes"]):
        ids = rc.unique_ids(rng, N // 4, n, ends=n > 2)
        rows_h = rc.patterns(max(n, 1), d, base=1000000 * (r + 1) + i)
        ld = d + (r + i) % 3
        idx, rows = ints(dev, ids if n else [0]), Slab(dev, max(n, 1), d, ld, (r + i) % 2, rows_h)
        assert lib.sgcn_hist_pack_f32(idx.ptr, n, rows.ptr, ld, d, cap, recv.ptr + 4 * r * per, None) == 0
        sync()
        blocks.append(rc.ref_hist_pack(ids, n, rows_h, d, cap, FILL_INT))
        rows.same_as(rows_h, "pack: rows"), idx.same_as(ids if n else [0], "pack: ids")
    recv_h = np.concatenate(blocks)
    recv.same_as(recv_h, "pack %r" % (c,))
    H0 = rc.patterns(N, d, base=77 + i)
    want = rc.ref_hist_apply(H0, recv_h, world, cap, d)
    tables = []
    for with_owner in (False, True, True):
        H = Slab(dev, N, d, ldh, 0, H0)
        owner = Slab(dev, 1, N, data=np.zeros(N, np.int32), fill=FILL_INT)
        assert lib.sgcn_hist_apply_f32(H.ptr, ldh, recv.ptr, world, cap, d, owner.ptr if with_owner else None, None) == 0
        sync()
        what = "apply %r (%s form)" % (c, rc.exchange_form(world, with_owner))
        tables.append(H.same_as(want, what))
        owner.same_as(np.zeros(N, np.int32), what + ": owner table")
        recv.same_as(recv_h, what + ": receive buffer")
    assert np.array_equal(tables[0], tables[1]) and np.array_equal(tables[1], tables[2])


def test_history_exchange_refusals(dev):
    lib = _lib()
    send, H = Slab(dev, 1, 64, fill=FILL_INT), Slab(dev, 8, 4, data=rc.patterns(8, 4))
    idx = ints(dev, [1, 2, 3])
    assert lib.sgcn_hist_pack_f32(idx.ptr, 3, H.ptr, 4, 4, 2, send.ptr, None) != 0          # more rows than the capacity
    assert lib.sgcn_hist_pack_f32(idx.ptr, 3, H.ptr, 3, 4, 4, send.ptr, None) != 0          # pitch below the width
    assert lib.sgcn_hist_pack_f32(idx.ptr, 3, H.ptr, 4, 4, 4, None, None) != 0
    assert lib.sgcn_hist_pack_f32(idx.ptr, 0, None, 4, 4, 0, None, None) == 0               # capacity 0: nothing to do
    assert lib.sgcn_hist_apply_f32(H.ptr, 3, send.ptr, 2, 4, 4, None, None) != 0
    assert lib.sgcn_hist_apply_f32(H.ptr, 4, send.ptr, 0, 4, 4, None, None) != 0
    assert lib.sgcn_hist_apply_f32(None, 4, send.ptr, 2, 4, 4, None, None) != 0
    assert lib.sgcn_hist_apply_f32(H.ptr, 4, send.ptr, 2, 0, 4, None, None) == 0
    sync()
    send.same_as(None, "refusals"), H.same_as(rc.patterns(8, 4), "refusals")


# ---- hand-built programs for the other index ops ----------------------------------------------------------------------------
def test_program_csr_slice_and_transpose(dev):
    """CSR_SLICE with the row pointer made on the device (the host never passes the slice's nnz) and the row count read as
    2 * slots[1] - 1; CSR_TRANSPOSE + GATHER_F32 on its outputs; scratch one int too small: a status, nothing launched"""
    OP, K = _OPK()
    d, i, p = rc.csr_with_rows(rc.SLICE_ROW_LENS, rc.SLICE_NCOLS, "slice")
    A = _Csr(dev, d, i, p)
    r = dict(rc.slice_selections(len(p) - 1, np.diff(p)))["n257"]
    n, ncols = len(r), rc.SLICE_NCOLS
    o_p, o_d, o_c, o_r = rc.ref_csr_slice(d, i, p, r)
    nnz = int(o_p[-1])
    t_rowptr, t_row, t_src = rc.ref_transpose(ncols, o_c, o_r)
    need = rc.transpose_plan(ncols, nnz)["ws_ints"]
    slots = (nnz, (n + 1) // 2, need)
    assert 2 * slots[1] - 1 == n
    for ws_cap, ok in ((so.S(2), True), (so.S(2, 1, -1), False)):
        rd, P = ints(dev, r), Slab(dev, 1, n + 1, fill=FILL_INT)
        D, Cc, R = Slab(dev, 1, nnz), Slab(dev, 1, nnz, fill=FILL_INT), Slab(dev, 1, nnz, fill=FILL_INT)
        TP, TR, TS = (Slab(dev, 1, k, fill=FILL_INT) for k in (ncols + 1, nnz, nnz))
        ws, G = Slab(dev, 1, need, fill=FILL_INT), Slab(dev, 1, nnz)
        sl = [(OP["CSR_SLICE"], [so.S(1, 2, -1), K(rd.ptr), K(A.d.ptr), K(A.i.ptr), K(A.p.ptr), K(P.ptr), K(D.ptr), K(Cc.ptr), K(R.ptr)])]
        tr = [(OP["CSR_TRANSPOSE"], [K(ncols), so.S(0), K(Cc.ptr), K(R.ptr), K(TP.ptr), K(TR.ptr), K(TS.ptr), K(ws.ptr), ws_cap]),
              (OP["GATHER_F32"], [K(D.ptr), K(TS.ptr), so.S(0, 2, -nnz), K(G.ptr)])]
        assert so.run(sl, slots) == 0
        assert (so.run(tr, slots) == 0) == ok
        sync()
        P.same_as(o_p, "program: row pointer"), D.same_as(o_d, "program: values"), Cc.same_as(o_c, "program: columns")
        R.same_as(o_r, "program: COO rows"), A.unchanged("program")
        if ok:
            TP.same_as(t_rowptr, "program: t_rowptr"), TR.same_as(t_row, "program: t_row"), TS.same_as(t_src, "program: t_src")
            G.same_as(o_d[t_src], "program: gathered values")
        else:
            for s in (TP, TR, TS, ws, G):
                s.same_as(None, "program: refused transpose")
    assert so.run([(OP["CSR_TRANSPOSE"], [K(ncols), so.S(5)])], slots) != 0        # a slot beyond the table


def test_program_gather_rows_copy2d_and_exchange(dev):
    OP, K = _OPK()
    N, n, d = 600, 123, 37
    rng = np.random.RandomState(rc.seed("program rows"))
    data, ids = rc.patterns(N, d), _gather_ids(rng, N, n)
    slots = (62, 5)
    assert 2 * slots[0] - 1 == n
    for _ in range(2):
        table, idx, out = Slab(dev, N, d, 40, 0, data), ints(dev, ids), Slab(dev, n, d, 38, 2)
        cp = Slab(dev, n, d - 5, 44, 1)
        prog = [(OP["GATHER_ROWS"], [K(table.ptr), K(40), K(idx.ptr), so.S(0, 2, -1), K(d), K(out.ptr), K(38)]),
                (OP["COPY2D"], [K(cp.ptr), K(44), K(table.ptr + 4 * 3), K(40), so.S(0, 2, -1), so.S(1, 6, 2)])]
        assert so.run(prog, slots) == 0
        sync()
        out.same_as(rc.ref_gather(data, ids), "program: GATHER_ROWS"), cp.same_as(data[:n, 3:3 + d - 5], "program: COPY2D")
        table.same_as(data, "program: table")
    # HIST_PACK + HIST_APPLY on the step's own stream (aux = 0), the block's row count 2 * slots[0] - 1
    world, cap = 3, 128
    per = cap * (d + 1)
    own = rc.unique_ids(rng, N // 4, n)
    rows_h = rc.patterns(n, d, base=9)
    others = [rc.ref_hist_pack(rc.unique_ids(rng, N // 4, k), k, rc.patterns(cap, d, base=100 * k), d, cap, FILL_INT) for k in (cap, 17)]
    for with_owner in (False, True):
        recv_h = np.concatenate([others[0], np.full(per, FILL_INT, np.int32), others[1]])
        recv, H = ints(dev, recv_h), Slab(dev, N, d, 40, 0, data)
        idx, rows, owner = ints(dev, own), Slab(dev, n, d, 48, 0, rows_h), Slab(dev, 1, N, data=np.zeros(N, np.int32), fill=FILL_INT)
        prog = [(OP["HIST_PACK"], [K(idx.ptr), so.S(0, 2, -1), K(rows.ptr), K(48), K(d), K(cap), K(recv.ptr + 4 * per), K(0)]),
                (OP["HIST_APPLY"], [K(H.ptr), K(40), K(recv.ptr), so.S(1, 1, -2), K(cap), K(d), K(owner.ptr if with_owner else 0), K(0)])]
        assert so.run(prog, slots) == 0
        sync()
        recv_h[per:2 * per] = rc.ref_hist_pack(own, n, rows_h, d, cap, FILL_INT)
        recv.same_as(recv_h, "program: HIST_PACK")
        H.same_as(rc.ref_hist_apply(data, recv_h, world, cap, d), "program: HIST_APPLY"), owner.same_as(np.zeros(N, np.int32), "owner")
