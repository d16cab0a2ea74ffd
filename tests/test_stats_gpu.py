"""stats.DeviceStat (sgcn_moments_add_f32) and stats.summary (sgcn_moments_summary_f64) against fp64 NumPy: K draws
streamed into the running statistics agree with np.mean / np.std (ddof 0, as gcn/stats.py's Stat) of the stacked draws,
for views at misaligned offsets into a larger buffer, for data whose stdev is six orders below its mean, and for a
constant input (stdev exactly 0).  The summary is the NumPy three-tuple and bitwise the same on every call."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 65, 154112 + 17)
DRAWS = (1, 2, 37, 1000)


def _draws(kind, K, n, off, seed):
    """K fp32 draws of n elements as views at float offset ``off`` (+ k n) into one device buffer."""
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    buf = torch.zeros(off + K * n + 3, dtype=torch.float32, device=dev)
    if kind == "normal":
        v = torch.randn(K * n, generator=g, device=dev) * 2.0 + 0.5
    elif kind == "cancel":
        v = 1e4 + 1e-2 * torch.randn(K * n, generator=g, device=dev)
    else:
        v = torch.full((K * n,), 0.1, dtype=torch.float32, device=dev)
    buf[off:off + K * n] = v
    return buf[off:off + K * n].view(K, n), [buf[off + k * n:off + (k + 1) * n] for k in range(K)]


def _host_moments(table, chunk=8192):
    """np.mean / np.std (axis 0, float64) of the stacked draws, a block of columns at a time (bounded host memory)."""
    K, n = table.shape
    mean, std = np.empty(n), np.empty(n)
    for c0 in range(0, n, chunk):
        h = table[:, c0:c0 + chunk].cpu().numpy().astype(np.float64)
        mean[c0:c0 + chunk] = np.mean(h, axis=0)
        std[c0:c0 + chunk] = np.std(h, axis=0)
    return mean, std


def _stream(views):
    from stochastic_gcn_amd.stats import DeviceStat
    st = DeviceStat()
    for v in views:
        st.add(v)
    return st


@pytest.mark.parametrize("kind,off", [("normal", 0), ("normal", 1), ("normal", 3), ("cancel", 1), ("cancel", 3),
                                      ("const", 1)])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("K", DRAWS)
def test_device_stat_matches_numpy(K, n, kind, off):
    table, views = _draws(kind, K, n, off, seed=1000 * K + n + off)
    st = _stream(views)
    assert st.count == K
    got_m, got_s = st.mean(), st.std()
    assert got_m.shape == (n,) and got_m.dtype == np.float64
    want_m, want_s = _host_moments(table)
    # the mean to 1e-9 of the draws' magnitude at that element (a mean near 0 has no relative accuracy of its own);
    # the stdev to 1e-9 of itself -- with mean 1e4 and stdev 1e-2, sums of x and x^2 would not get one digit right
    rms = np.sqrt(want_m ** 2 + want_s ** 2)
    assert np.all(np.abs(got_m - want_m) <= 1e-9 * rms), np.max(np.abs(got_m - want_m) / rms)
    assert np.all(np.abs(got_s - want_s) <= 1e-9 * want_s), np.max(np.abs(got_s - want_s) / np.maximum(want_s, 1e-300))
    if kind == "const" or K == 1:
        assert np.all(got_s == 0.0)
        assert np.all(got_m == table[0].cpu().numpy().astype(np.float64))


@pytest.mark.parametrize("n", SIZES)
def test_summary_is_the_numpy_three_tuple_and_bitwise_reproducible(n):
    from stochastic_gcn_amd.stats import summary
    ta, va = _draws("normal", 37, n, 1, seed=7 + n)
    tb, vb = _draws("normal", 5, n, 3, seed=11 + n)
    a, b = _stream(va), _stream(vb)
    m_a, s_a = a.mean().astype(np.float64), a.std()
    m_b = b.mean()
    want = (np.mean(np.abs(m_a)), np.mean(s_a), np.mean(np.abs(m_a - m_b)))
    got = summary(a, b)
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-12 * abs(w), (got, want)
    again = summary(a, b)
    assert [np.float64(x).tobytes() for x in again] == [np.float64(x).tobytes() for x in got]
    alone = summary(a)
    assert alone[2] == 0.0 and alone[0] == got[0] and alone[1] == got[1]


def test_stacked_pairs_and_size_checks():
    """A (mean, variance) pair is accumulated stacked, as np.mean(Stat.vals, axis=0) sees it; a later sample of another
    size is refused."""
    from stochastic_gcn_amd.stats import DeviceStat
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    pairs = [(torch.randn(5, 7, generator=g, device=dev), torch.rand(5, 7, generator=g, device=dev)) for _ in range(9)]
    st = DeviceStat()
    for p in pairs:
        st.add(p)
    host = np.stack([np.stack([x.cpu().numpy(), y.cpu().numpy()]) for x, y in pairs]).astype(np.float64)
    assert st.mean().shape == (2, 5, 7)
    np.testing.assert_allclose(st.mean(), np.mean(host, axis=0), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(st.std(), np.std(host, axis=0), rtol=1e-9, atol=1e-15)
    with pytest.raises(ValueError, match="elements"):
        st.add(torch.zeros(5, 7, device=dev))
    one = DeviceStat()
    one.add(torch.zeros(4, 4, device=dev))
    with pytest.raises(ValueError, match="elements"):
        one.add(torch.zeros(17, device=dev))
