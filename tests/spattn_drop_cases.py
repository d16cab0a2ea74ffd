"""The inputs of tests/test_spattn_drop_gpu.py, built without a device so that tests/test_spattn_drop.py can check their
preconditions (test-only helper; seeded by the arguments and cached, what a builder returns is read-only).  The patterns and
the real-valued tables are those of spattn_cases.py, imported.

Mask readout.  Q = 0, so every score is 0 and every weight exactly 1: C[i] = (1 / n_i) sum_j mk_ij B[j].  Every row's degree is
a power of two (the division is exact), its column ids are distinct mod dh, and B[j] holds a 1 in column h dh + (j mod dh) of
every head h: element [i, h dh + r] of C is mk_ijh / n_i for THE entry j of row i with j mod dh = r, and exactly 0 where the row
has none -- the kept set can be read off the device for every (i, j, h).

Real-valued inputs.  (pattern, d, H, plan, keep):
    row_lengths   48 x 1000, rectangular and asymmetric (a transposed hash reads other bits); under plan "T" its rows of
                  65 .. 579 entries are split; K >= M, so the fused form (Q = B[:M], one gradient dx) runs on it too
    m64_k64       square, about 3 entries per row, asymmetric; at keep = 0.5 whole rows are dropped
    d             8 (one float4 / eight scalar heads), 30 on a pitch of 32 (VW = 4, a ragged last vector), 260 (65 vectors:
                  two per lane), 602 on a pitch of 604 (151 vectors: three per lane)
The key of a case is the first of 1, 2, .. under which some non-empty row loses ALL its entries in some head (and some row
keeps at least two): ``key_for``.  tests/test_spattn_drop.py asserts that one exists for every case.
"""
import functools

import numpy as np
import scipy.sparse as sp

import spattn_cases as cs
import spattn_drop_ref as dref

pattern = cs.pattern
_freeze = cs._freeze

# ---- mask readout ----------------------------------------------------------------------------------------------------------
DH = 64
READOUT_KEEP = 0.5
READOUT_KEY = 0x5EED0001
READOUT = {"square": (256, 256), "rect": (96, 256)}        # M = K = 256; a rectangular M < K


@functools.lru_cache(maxsize=None)
def readout_pattern(name):
    M, K = READOUT[name]
    rng = np.random.RandomState(cs.seed("readout", name))
    rows, cols = [], []
    for i in range(M):
        n = 1 << (i % 7)                                    # 1, 2, .. 64 = DH
        res = rng.choice(DH, n, replace=False)              # distinct mod dh
        rows.append(np.full(n, i))
        cols.append(res + DH * rng.randint(0, K // DH, n))
    a = sp.csr_matrix((np.ones(sum(c.size for c in cols), np.float32), (np.concatenate(rows), np.concatenate(cols))), shape=(M, K))
    a.sort_indices()
    deg = np.diff(a.indptr)
    assert a.nnz == sum(c.size for c in cols) and np.all(deg & (deg - 1) == 0) and deg.max() == DH and deg.min() == 1
    from stochastic_gcn_amd import ops
    return a, ops.transpose_host(a)


@functools.lru_cache(maxsize=None)
def readout_tables(name, H):
    """(Q, B, C expected in fp32, kept (nnz x H) bool)"""
    a, _ = readout_pattern(name)
    M, K = a.shape
    d = H * DH
    B = np.zeros((K, d), np.float32)
    for h in range(H):
        B[np.arange(K), h * DH + np.arange(K) % DH] = 1.0
    Q = np.zeros((M, d), np.float32)
    rows = np.repeat(np.arange(M), np.diff(a.indptr))
    cols = a.indices.astype(np.int64)
    k = np.stack([dref.kept(rows, cols, h, READOUT_KEY, READOUT_KEEP) for h in range(H)], axis=1)
    C = np.zeros((M, d), np.float32)
    n = np.diff(a.indptr).astype(np.float32)
    for h in range(H):
        C[rows, h * DH + cols % DH] = np.where(k[:, h], np.float32(dref.mk_value(READOUT_KEEP)), np.float32(0)) / n[rows]
    _freeze(Q, B, C, k)
    return Q, B, C, k


# ---- real-valued inputs ------------------------------------------------------------------------------------------------------
GENERAL = [("row_lengths", 8, 1, "T", 0.8), ("row_lengths", 8, 2, "T", 0.8), ("row_lengths", 8, 8, "T", 0.8),
           ("row_lengths", 30, 1, "T", 0.8), ("row_lengths", 30, 2, "default", 0.8), ("row_lengths", 260, 1, "T", 0.8),
           ("row_lengths", 260, 2, "T", 0.8), ("row_lengths", 602, 1, "T", 0.8),
           ("m64_k64", 8, 2, "none", 0.5), ("m64_k64", 30, 1, "none", 0.5), ("m64_k64", 260, 2, "default", 0.5)]
PITCH = {8: 8, 30: 32, 260: 260, 602: 604}


def general(name, d):
    return cs.general(name, d)


def _all_dropped(a, mk):
    """bool (M x H): a non-empty row whose every entry is dropped in that head"""
    deg = np.diff(a.indptr)
    rows = np.repeat(np.arange(a.shape[0]), deg)
    keptn = np.zeros((a.shape[0], mk.shape[1]), np.int64)
    np.add.at(keptn, rows, (mk > 0).astype(np.int64))
    return (deg > 0)[:, None] & (keptn == 0), keptn


@functools.lru_cache(maxsize=None)
def key_for(name, H, keep):
    a, _ = pattern(name)
    for key in range(1, 200):
        gone, keptn = _all_dropped(a, dref.mask(a, H, key, keep))
        if gone.any() and (keptn >= 2).any():
            return key
    return None


def variants(name):
    """[(alias, with_add)]: Q a table of its own, and Q = B[:M] (the model's case; K >= M), each with and without an addend"""
    M, K = pattern(name)[0].shape
    assert K >= M
    return [(False, False), (False, True), (True, False), (True, True)]


def scale_of(d, H):
    return float(np.float32(float(d // H) ** -0.5))


@functools.lru_cache(maxsize=None)
def general_ref(name, d, H, keep, alias, with_add):
    """spattn_drop_ref.backward_f64's dict of one case ('fwd': the forward and its bounds; 'mk': the mask)"""
    a, _ = pattern(name)
    Q, B, G, add = general(name, d)
    M = a.shape[0]
    mk = dref.mask(a, H, key_for(name, H, keep), keep)
    kw = dict(add=add, add_rows=M) if with_add else {}
    r = dref.backward_f64(a, B[:M] if alias else Q, B, G, scale_of(d, H), H, mk, fused=alias, **kw)
    r['mk'] = mk
    _freeze(*[v for v in r.values() if isinstance(v, np.ndarray)])
    return r
