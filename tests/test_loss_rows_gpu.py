"""GPU tests of the losses over a row subset (sgcn_softmax_ce_rows_f32 / sgcn_sigmoid_ce_rows_f32, csrc/sgcn_dense.hip).

The contract is stated against the existing entry points: with Z = logits[rows], Y = labels[rows], the statistics, the
per-row scratch (class plane included) and the prediction are BIT FOR BIT what sgcn_softmax_ce_f32 / sgcn_sigmoid_ce_f32
give on (Z, Y); dlogits[rows[i]] is their dlogits[i]; every other row of dlogits is +0.0.  All operands are pitched
(pitch > c, offset views), the gradient table is pre-filled with a NaN bit pattern so that a row nobody wrote shows, and
its pad columns must come back untouched.  Loss and gradient are also checked against float64 (tests/ref64.py) with
the bounds of the existing loss tests (test_det_kernels_gpu.py::test_softmax_ce_vs_float64,
test_kernels_gpu.py::test_sigmoid_ce_vs_numpy)."""
import numpy as np
import pytest
import torch

import ref64 as R
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
f32 = np.float32
NAN_BITS = 0x7FC00123
SUBSETS = ["all", "one", "first", "last", "every_other", "random65", "tail_gap"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def subset(kind, N, seed):
    rng = np.random.RandomState(seed)
    if kind == "all":
        r = np.arange(N)
    elif kind == "one":
        r = np.array([N // 2])
    elif kind == "first":
        r = np.array([0])
    elif kind == "last":
        r = np.array([N - 1])
    elif kind == "every_other":
        r = np.arange(0, N, 2)
    elif kind == "random65":
        r = np.flatnonzero(rng.rand(N) < 0.65)
        if r.size == 0:
            r = np.array([rng.randint(0, N)])
    else:   # the subset ends early: 7/8 of the table lies behind the last row, far beyond its workgroup's four rows
        r = np.arange(max(1, N // 8))
    return r.astype(np.int32)


def inputs(N, c, seed, multilabel):
    """Logits shifted per row by 0 / +80 / -80 (softmax) with exact ties of the maximum in some rows; labels one-hot,
    soft, all-zero or tied (softmax), 0/1 per class (sigmoid)."""
    rng = np.random.RandomState(seed)
    z = rng.standard_normal((N, c)) * 3
    if multilabel:
        return z.astype(f32), (rng.rand(N, c) < 0.3).astype(f32)
    z += np.array([0.0, 80.0, -80.0])[np.arange(N) % 3][:, None]
    y = np.zeros((N, c))
    y[np.arange(N), rng.randint(0, c, N)] = 1.0
    soft = np.arange(N) % 5 == 1
    y[soft] = rng.uniform(0, 1, (int(soft.sum()), c)) * (rng.rand(int(soft.sum()), c) < 0.5)
    y[np.arange(N) % 5 == 2] = 0.0
    tie = np.flatnonzero(np.arange(N) % 4 == 1)
    z[tie, rng.randint(0, c, tie.size)] = z[tie].max(axis=1)
    return z.astype(f32), y.astype(f32)


def pitched(a, pad_l, pad_r, dev, fill=0.0):
    """(device buffer, view of it holding `a` with `pad_l` columns in front and `pad_r` behind)"""
    n, c = a.shape
    w = np.full((n, pad_l + c + pad_r), fill, f32)
    w[:, pad_l:pad_l + c] = a
    buf = T(w, dev)
    return buf, buf[:, pad_l:pad_l + c]


def nan_table(n, w, dev):
    return torch.full((n, w), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)


def bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def call_rows(lib, name, z, y, N, c, rows, n, dz, pred, stats):
    """The raw entry point on pitched views (pitch = the row stride of the buffer a view was cut from)."""
    return getattr(lib, name)(z.data_ptr(), z.stride(0), y.data_ptr(), y.stride(0), N, c, rows.data_ptr(), n,
                              0 if dz is None else dz.data_ptr(), 0 if dz is None else dz.stride(0),
                              0 if pred is None else pred.data_ptr(), 0 if pred is None else pred.stride(0),
                              stats.data_ptr(), stats.data_ptr() + 16, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("kind", SUBSETS)
@pytest.mark.parametrize("N", [1, 7, 512, 20001])
@pytest.mark.parametrize("c", [1, 3, 41, 121])
@pytest.mark.parametrize("loss", ["softmax", "sigmoid"])
def test_loss_rows_matches_the_plain_entry_point_on_gathered_rows(dev, loss, c, N, kind):
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd._ffi import lib
    multilabel = loss == "sigmoid"
    seed = 1000 * N + 10 * c + SUBSETS.index(kind)
    rows_h = subset(kind, N, seed)
    n = int(rows_h.size)
    z, y = inputs(N, c, seed, multilabel)
    _, zv = pitched(z, 2, 5, dev)
    _, yv = pitched(y, 1, 3, dev)
    rows = T(rows_h, dev)
    planes = 2 if multilabel else 3
    plain = ops.sigmoid_ce if multilabel else ops.softmax_ce
    name = "sgcn_sigmoid_ce_rows_f32" if multilabel else "sgcn_softmax_ce_rows_f32"
    # the existing entry point on gathered copies
    Z, Y = T(z[rows_h], dev), T(y[rows_h], dev)
    st_ref, G, P = plain(Z, Y, want_grad=True, want_pred=True)
    st_ref_nopred = plain(Z, Y, want_grad=False, want_pred=False)[0]

    for want_grad in (True, False):
        for want_pred in (True, False):
            pl = planes if want_pred else 2
            stats = nan_table(1, 4 + pl * n, dev).view(-1)
            dzbuf = nan_table(N, c + 7, dev) if want_grad else None
            dz = dzbuf[:, 3:3 + c] if want_grad else None
            pbuf = nan_table(n, c + 1, dev) if want_pred else None
            pred = pbuf[:, 1:1 + c] if want_pred else None
            rc = call_rows(lib, name, zv, yv, N, c, rows, n, dz, pred, stats)
            assert rc == 0, lib.sgcn_last_error()
            want_stats = st_ref if want_pred else st_ref_nopred
            assert (bits(stats) == bits(want_stats)).all(), "stats / rowstat differ from the plain entry point"
            if want_pred:
                assert (bits(pred) == bits(P)).all(), "pred differs"
                assert (bits(pbuf[:, :1]) == NAN_BITS).all(), "pred pad columns were written"
            if want_grad:
                got = bits(dz)
                assert (got[rows_h] == bits(G)).all(), "gradient rows differ"
                off = np.ones(N, bool)
                off[rows_h] = False
                assert (got[off] == 0).all(), "an off-subset row of dlogits is not +0.0"
                padbits = bits(dzbuf)
                assert (padbits[:, :3] == NAN_BITS).all() and (padbits[:, 3 + c:] == NAN_BITS).all(), \
                    "dlogits pad columns were written"

    # through ops, contiguous outputs: the same bits, and float64
    st, dz, pred = plain(zv, yv, want_grad=True, want_pred=True, rows=rows)
    assert (bits(st) == bits(st_ref)).all() and (bits(pred) == bits(P)).all() and (bits(dz)[rows_h] == bits(G)).all()
    st, dz = st.cpu().numpy(), dz.cpu().numpy()
    Zh, Yh = z[rows_h], y[rows_h]
    if multilabel:
        def mean_ce(t):
            yy = R.t64(Yh)
            return ((torch.clamp(t, min=0) - t * yy + torch.log1p(torch.exp(-t.abs()))).sum() / (n * c),)
        (ce,), (dz_r,) = R.vjp(mean_ce, [Zh], [np.ones(())])
        print("sigmoid mean CE %.9g vs %.9g" % (st[2], float(ce)))
        assert abs(st[2] - float(ce)) <= 1e-5 * max(1.0, float(ce))
    else:
        (ce, _), (dz_r,) = R.vjp(lambda t: R.softmax_ce(t, R.t64(Yh)), [Zh], [np.full(n, 1.0 / n), None])
        print("softmax mean CE %.9g vs %.9g" % (st[2], ce.mean()))
        assert abs(st[2] - ce.mean()) <= 1e-5 * max(1.0, np.abs(ce).mean())
        assert abs(st[0] - ce.sum()) <= 1e-5 * max(1.0, np.abs(ce).sum())
    full = np.zeros((N, c))
    full[rows_h] = dz_r
    print("dlogits rel_err %.3e" % onp.rel_err(dz, full))
    assert onp.rel_err(dz, full) <= 1e-5


@pytest.mark.parametrize("loss", ["softmax", "sigmoid"])
def test_loss_rows_invalid_arguments_leave_the_outputs_untouched(dev, loss):
    from stochastic_gcn_amd._ffi import lib
    name = "sgcn_sigmoid_ce_rows_f32" if loss == "sigmoid" else "sgcn_softmax_ce_rows_f32"
    N, c, n = 9, 5, 4
    z, y = inputs(N, c, 3, loss == "sigmoid")
    zt, yt, rows = T(z, dev), T(y, dev), T(np.array([1, 2, 5, 8], np.int32), dev)
    st = torch.cuda.current_stream().cuda_stream

    def attempt(**kw):
        a = dict(ldz=c, ldl=c, N=N, n=n, rows=rows.data_ptr(), lddz=c, ldp=c)
        a.update(kw)
        stats, dz, pred = nan_table(1, 4 + 3 * n, dev).view(-1), nan_table(N, c, dev), nan_table(n, c, dev)
        rc = getattr(lib, name)(zt.data_ptr(), a['ldz'], yt.data_ptr(), a['ldl'], a['N'], c, a['rows'], a['n'],
                                dz.data_ptr(), a['lddz'], pred.data_ptr(), a['ldp'], stats.data_ptr(),
                                stats.data_ptr() + 16, st)
        torch.cuda.synchronize()
        untouched = all((bits(t) == NAN_BITS).all() for t in (stats, dz, pred))
        return rc, untouched

    assert attempt() == (0, False)
    for bad in (dict(n=0), dict(n=N + 1), dict(rows=0), dict(ldz=c - 1), dict(ldl=c - 1), dict(lddz=c - 1),
                dict(ldp=c - 1), dict(N=0)):
        rc, untouched = attempt(**bad)
        assert rc == -1 and untouched, bad
        assert b"ce_rows" in lib.sgcn_last_error()


def test_ops_wrapper_checks_the_rows_on_the_host():
    from stochastic_gcn_amd import ops
    assert ops.check_loss_rows(np.array([0, 3, 4]), 5).dtype == np.int32
    for bad in ([3, 1], [1, 1], [0, 5], [-1, 2], []):
        with pytest.raises(ValueError):
            ops.check_loss_rows(np.array(bad, dtype=np.int64), 5)
