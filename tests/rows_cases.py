"""Row, slice, transpose and exchange test cases: the launch rules of sgcn_rows.hip and of the optimizer's parked history
scatter (sgcn_dense.hip) restated, case catalogues that reach every cell of those rules, and NumPy references (test-only
helper; the counterparts are sparse_cases.py and dense_cases.py).  Imports NumPy only.

Cells.  ``rows_cell`` restates ``launch_rows`` (vector width from the two pitches and the two base alignments, lane group,
ragged last vector, more than one trip of a lane, and where the row count sits against the rows of a workgroup),
``park_cell`` the acceptance of ``scatter_park`` and ``transpose_cell`` the chunking and the LDS / global choice of
``sgcn_csr_transpose_index``.  Which cells are reachable is found by scanning pools of shapes; the catalogues hold one case
per reachable cell with the pool values rotated, and the CPU suite (test_rows_cases.py) checks that none is missing.

References.  The kernels copy bits and do integer work, so every reference is NumPy indexing and every comparison is bit
for bit.  Values are distinct bit patterns (``patterns``): a row taken from the wrong place cannot match by accident; a
share of the rows hold NaN payloads, infinities, negative zero and subnormals.  Scatter ids are unique apart from the -1
pads (``assert_scatter_ids``): duplicates inside one scatter are undefined in the reference (tf.scatter_update) and in
the kernel, so no case has them.
"""
import zlib

import numpy as np

kBlock, kWave = 256, 64              # sgcn_host.h
kTChunk, kTLdsCols = 512, 16384      # sgcn_rows.hip: nonzeros per transpose chunk; counters in LDS up to this many columns
kTailRows = kBlock // 32             # sgcn_dense.hip kTailRowsPerBlock: history rows per workgroup of the optimizer's launch
kTailCols = 128                      # ... and the columns one trip of its 32 lanes x float4 covers
kParkJobs = 2                        # scatters that can ride in one optimizer launch
kAdamBlocks = 2048                   # cap of the Adam workgroups (adam_with_stats)
kGatherBlocks = 4096                 # cap of gather_f32_kernel's grid

WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 602, 1204)
OFFSETS = (0, 1, 2)                  # base offsets in floats from a 16-byte aligned address
NPOS = ("below", "on", "past")


def seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def _cdiv(a, b):
    return -(-a // b)


def pitches(d):
    """the pitches a width is tried with: d, d + 1, d + 2, the next multiple of 4, the next multiple of 32"""
    return tuple(sorted({d, d + 1, d + 2, _cdiv(d + 1, 4) * 4, _cdiv(d + 1, 32) * 32}))


# ---- launch_rows ------------------------------------------------------------------------------------------------------------
def group_lanes(nvec):
    """sgcn_seg.h group_lanes"""
    return 8 if nvec <= 8 else 16 if nvec <= 16 else 32 if nvec <= 32 else 64


def rows_plan(d, ldi, ldo, in_off, out_off):
    """launch_rows: ``in_off`` / ``out_off`` are the bases' offsets in floats from a 16-byte aligned address"""
    vw = 1
    if ldi % 4 == 0 and ldo % 4 == 0 and in_off % 4 == 0 and out_off % 4 == 0:
        vw = 4
    elif ldi % 2 == 0 and ldo % 2 == 0 and in_off % 2 == 0 and out_off % 2 == 0:
        vw = 2
    nvec = _cdiv(d, vw)
    G = group_lanes(nvec)
    return dict(vw=vw, nvec=nvec, G=G, gpb=kBlock // G, ragged=d % vw != 0, multi=nvec > G)


def n_at(gpb, pos, k=2):
    """a row count below, on or one past a boundary of ``gpb`` rows per workgroup"""
    return k * gpb + {"below": -1, "on": 0, "past": 1}[pos]


def n_pos(n, gpb):
    return "on" if n % gpb == 0 else "past" if n % gpb == 1 and n > 1 else "below"


def rows_cell(d, ldi, ldo, in_off, out_off, n=None):
    """(vw, G, ragged last vector, a lane makes more than one trip[, n against the rows of a workgroup])"""
    p = rows_plan(d, ldi, ldo, in_off, out_off)
    c = (p["vw"], p["G"], p["ragged"], p["multi"])
    return c if n is None else c + (n_pos(n, p["gpb"]),)


def _rows_pool():
    for d in WIDTHS:
        for ldi in pitches(d):
            for ldo in pitches(d):
                for io in OFFSETS:
                    for oo in OFFSETS:
                        yield d, ldi, ldo, io, oo


def rows_reachable():
    return sorted({rows_cell(*s) + (pos,) for s in _rows_pool() for pos in NPOS})


def rows_cases():
    """one case per reachable cell; among the pool shapes of a cell the one picked rotates with the cell's index"""
    by = {}
    for s in _rows_pool():
        by.setdefault(rows_cell(*s), []).append(s)
    out = []
    for ci, cell in enumerate(sorted(by)):
        for pi, pos in enumerate(NPOS):
            shapes = by[cell]
            d, ldi, ldo, io, oo = shapes[(7 * ci + 3 * pi) * 2654435761 % len(shapes)]
            gpb = kBlock // cell[1]
            n = n_at(gpb, pos, 2 + (ci + pi) % 2)
            out.append(dict(d=d, ldi=ldi, ldo=ldo, in_off=io, out_off=oo, n=n, N=2 * n + 5 + ci % 3))
    for i, d in enumerate(WIDTHS):       # every pool width at least once
        if not any(c["d"] == d for c in out):
            p = pitches(d)
            out.append(dict(d=d, ldi=p[i % len(p)], ldo=p[(i + 2) % len(p)], in_off=i % 3, out_off=(i + 1) % 3, n=123, N=500))
    return out


ROWS_CASES = rows_cases()


def case_cell(c):
    return rows_cell(c["d"], c["ldi"], c["ldo"], c["in_off"], c["out_off"], c["n"])


# ---- scatter_park -----------------------------------------------------------------------------------------------------------
PARK_WIDTHS = (4, 8, 124, 128, 132, 256, 512, 600)
PARK_REFUSED_WIDTHS = (30, 41, 602)
PARK_N = (1, 7, 8, 9, 1019)
ADAM_COUNTS = (1, 255, 257, kAdamBlocks * kBlock + 1)


def park_cell(d, ldh, lds, aligned=(True, True), jobs=0, n=1):
    """scatter_park: ("park", more than one trip over the columns) or ("own", the first test that refuses it).
    ``aligned``: (table, source) base 16-byte aligned; ``jobs``: scatters already parked for this launch."""
    for why, bad in (("third", jobs >= kParkJobs), ("n", n <= 0), ("d0", d <= 0), ("d", d % 4 != 0), ("ldh", ldh % 4 != 0),
                     ("lds", lds % 4 != 0), ("table", not aligned[0]), ("source", not aligned[1])):
        if bad:
            return ("own", why)
    return ("park", d > kTailCols)


def _park_pool():
    for d in PARK_WIDTHS + PARK_REFUSED_WIDTHS:
        for ldh in pitches(d):
            for lds in pitches(d):
                for ah in (True, False):
                    for as_ in (True, False):
                        yield d, ldh, lds, (ah, as_)


def park_reachable():
    """cells of one scatter behind the optimizer (the third scatter and the empty one are cases of their own)"""
    return sorted({park_cell(*s) for s in _park_pool()})


def park_cases():
    """one job per (cell, width that reaches it); n and the optimizer's parameter count rotate through their pools"""
    by = {}
    for s in _park_pool():
        by.setdefault((park_cell(*s), s[0]), []).append(s)
    out = []
    for ci, key in enumerate(sorted(by)):
        shapes = by[key]
        d, ldh, lds, al = shapes[(5 * ci + 1) * 2654435761 % len(shapes)]
        out.append(dict(d=d, ldh=ldh, lds=lds, aligned=al, n=PARK_N[ci % len(PARK_N)], params=ADAM_COUNTS[ci % len(ADAM_COUNTS)]))
    return out


PARK_CASES = park_cases()


def adam_blocks(n):
    return min(_cdiv(n, kBlock), kAdamBlocks)


# ---- sgcn_csr_transpose_index -----------------------------------------------------------------------------------------------
T_NCOLS = (1, 5, 255, 256, 257, 1433, 16384, 16385, 20000)
T_NNZ = (1, 511, 512, 513, 1024, 1500, 1536, 5000)


def transpose_plan(ncols, nnz):
    nchunks = _cdiv(nnz, kTChunk)
    return dict(nchunks=nchunks, lds=ncols <= kTLdsCols, lds_bytes=4 * ncols if ncols <= kTLdsCols else 0,
                span=_cdiv(ncols, kBlock), ws_ints=0 if ncols <= 0 or nnz <= 0 else nchunks * ncols)


def transpose_cell(ncols, nnz):
    """(chunks: 1, 2 or 3 for more; counters in LDS; the last chunk is full)"""
    p = transpose_plan(ncols, nnz)
    return (min(p["nchunks"], 3), p["lds"], nnz % kTChunk == 0)


def transpose_reachable():
    return sorted({transpose_cell(c, z) for c in T_NCOLS for z in T_NNZ})


def transpose_cases():
    by = {}
    for c in T_NCOLS:
        for z in T_NNZ:
            by.setdefault(transpose_cell(c, z), []).append((c, z))
    out = []
    for ci, cell in enumerate(sorted(by)):
        shapes = by[cell]
        out.append(shapes[(3 * ci + 1) * 2654435761 % len(shapes)])
    # the named edges: the LDS / global switch (64 KB of dynamic LDS to the byte at 16,384 columns), the chunk boundary,
    # the spans of the scan (256 threads) at 255 / 256 / 257 columns
    for edge in ((16384, 513), (16385, 513), (16384, 5000), (300, 511), (300, 512), (300, 513), (255, 1500), (256, 1500), (257, 1500)):
        if edge not in out:
            out.append(edge)
    return out


TRANSPOSE_CASES = transpose_cases()


# ---- inputs -----------------------------------------------------------------------------------------------------------------
SPECIALS = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff, 0x00000000],
                    np.uint32)       # quiet / signalling NaNs with payloads, +-inf, -0, the smallest and a large subnormal, +0


def patterns(rows, d, base=0, specials=True):
    """``rows x d`` float32 whose element (r, c) holds the bits of (base + r * 4099 + c + 1) * 2654435761 mod 2^32 -- an odd
    multiplier, so distinct (r, c) inside 2^32 / 4099 rows give distinct bits over all exponents.  Every fifth row
    carries the special values in its first columns."""
    r = np.arange(rows, dtype=np.uint64)[:, None]
    c = np.arange(d, dtype=np.uint64)[None, :]
    u = (((np.uint64(base) + r * np.uint64(4099) + c + np.uint64(1)) * np.uint64(2654435761)) & np.uint64(0xffffffff)).astype(np.uint32)
    if specials and d > 0:
        k = min(d, len(SPECIALS))
        for i in range(2, rows, 5):
            u[i, :k] = np.roll(SPECIALS, i)[:k]
    return u.view(np.float32).reshape(rows, d)


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def assert_scatter_ids(ids, N):
    """the condition every scatter case meets: ids below N, unique apart from the negative pads"""
    ids = np.asarray(ids)
    live = ids[ids >= 0]
    assert ids.dtype == np.int32 and (live < N).all() and len(np.unique(live)) == len(live), "scatter ids must be unique"
    return ids


def unique_ids(rng, N, n, ends=True, pads=0):
    """n unique row ids below N (with 0 and N - 1 among them when ``ends``), ``pads`` of them replaced by -1"""
    assert n <= N
    if ends and n >= 2:
        ids = rng.permutation(np.concatenate([1 + rng.choice(N - 2, n - 2, replace=False), [0, N - 1]])).astype(np.int32)
    else:
        ids = rng.choice(N, n, replace=False).astype(np.int32)
    if pads:
        ids[rng.choice(n, min(pads, n), replace=False)] = -1
    return assert_scatter_ids(ids, N)


# ---- references (NumPy indexing) --------------------------------------------------------------------------------------------
def ref_gather(table, ids):
    return table[np.asarray(ids, np.int64)]


def ref_scatter(H, ids, src):
    """H with H[ids[i]] = src[i] for every ids[i] >= 0 (a copy)"""
    out = H.copy()
    ids = np.asarray(ids, np.int64)
    keep = ids >= 0
    out[ids[keep], :src.shape[1]] = src[:len(ids)][keep]
    return out


def ref_slice_indptr(a_p, r):
    r = np.asarray(r, np.int64)
    o = np.zeros(len(r) + 1, np.int32)
    np.cumsum(np.diff(a_p)[r], out=o[1:])
    return o


def ref_csr_slice(a_d, a_i, a_p, r):
    """(o_p, o_d, o_col, o_row) of the row slice A[r]: the rows' nonzeros in storage order, o_row the slice's own row numbers"""
    r = np.asarray(r, np.int64)
    o_p = ref_slice_indptr(a_p, r)
    lens = np.diff(o_p).astype(np.int64)
    o_row = np.repeat(np.arange(len(r), dtype=np.int32), lens)
    src = np.repeat(np.asarray(a_p, np.int64)[r], lens) + (np.arange(int(o_p[-1]), dtype=np.int64) - np.repeat(o_p[:-1].astype(np.int64), lens))
    return o_p, a_d[src], a_i[src].astype(np.int32), o_row


def ref_transpose(ncols, col, coo_row):
    """(t_rowptr, t_row, t_src): the entries sorted by column, storage order kept inside a column"""
    col = np.asarray(col, np.int64)
    t_src = np.argsort(col, kind="stable").astype(np.int32)
    t_rowptr = np.zeros(ncols + 1, np.int32)
    np.cumsum(np.bincount(col, minlength=ncols), out=t_rowptr[1:])
    return t_rowptr, np.asarray(coo_row, np.int32)[t_src], t_src


def ref_gather_f32(src, idx):
    return src[np.asarray(idx, np.int64)]


def ref_scale_rows(x, s):
    """one fp32 multiply per element"""
    return (s.astype(np.float32)[:, None] * x.astype(np.float32)).astype(np.float32)


def ref_hist_pack(ids, n, rows, d, cap, fill):
    """the send block [cap ids | cap x d row bits] as int32 words; payload rows n .. cap keep ``fill``"""
    out = np.full(cap * (d + 1), fill, np.int32)
    out[:cap] = -1
    out[:n] = ids[:n]
    out[cap:].reshape(cap, d)[:n] = bits(rows[:n, :d])
    return out


def ref_hist_apply(H, recv, world, cap, d):
    """every rank's block scattered in rank order (a copy of H): the higher rank wins"""
    out = H.copy()
    per = cap * (d + 1)
    for r in range(world):
        blk = recv[r * per:(r + 1) * per]
        ids = blk[:cap].astype(np.int64)
        keep = ids >= 0
        out[ids[keep], :d] = blk[cap:].view(np.float32).reshape(cap, d)[keep]
    return out


# ---- matrices ---------------------------------------------------------------------------------------------------------------
def csr_with_rows(lens, ncols, key):
    """a CSR matrix (data, indices, indptr) whose row i has lens[i] nonzeros in ascending distinct columns; the values are
    distinct bit patterns"""
    rng = np.random.RandomState(seed("csr", key))
    indptr = np.zeros(len(lens) + 1, np.int32)
    np.cumsum(lens, out=indptr[1:])
    indices = np.empty(int(indptr[-1]), np.int32)
    for i, k in enumerate(lens):
        assert k <= ncols
        indices[indptr[i]:indptr[i + 1]] = np.sort(rng.choice(ncols, k, replace=False))
    data = patterns(1, int(indptr[-1]), base=seed("val", key) % 100000, specials=False).ravel() if indptr[-1] else np.zeros(0, np.float32)
    return data, indices, indptr


def csr_with_nnz(ncols, nnz, key, lo=0, hi=None, one_column=None):
    """a CSR matrix with exactly ``nnz`` nonzeros: columns in [lo, hi) (empty columns at the ends otherwise), or all in
    ``one_column`` (one nonzero per row, then)"""
    rng = np.random.RandomState(seed("nnz", key))
    hi = ncols if hi is None else hi
    if one_column is not None:
        lens = np.ones(nnz, np.int64)
        d, i, p = csr_with_rows(lens, 1, key)
        return d, np.full(nnz, one_column, np.int32), p
    nrows = max(3, _cdiv(2 * nnz, max(hi - lo, 1)) + 3)
    lin = np.sort(rng.choice(nrows * (hi - lo), nnz, replace=False))
    rows, cols = lin // (hi - lo), (lin % (hi - lo) + lo).astype(np.int32)
    indptr = np.zeros(nrows + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=nrows), out=indptr[1:])
    data = patterns(1, nnz, base=seed("val", key) % 100000, specials=False).ravel()
    return data, cols, indptr


TRANSPOSE_EDGES = ((300, 1500, dict(lo=40, hi=260)), (20000, 1500, dict(lo=9000, hi=9100)),      # empty columns at both ends
                   (300, 1300, dict(one_column=0)), (300, 513, dict(one_column=299)), (20000, 700, dict(one_column=12345)))

SLICE_NCOLS = 500
SLICE_ROW_LENS = tuple([0, 1, 63, 64, 65, 0, 128, 129, 400, 0, 0, 3] + [(7 * k * k + 3 * k) % 11 if k % 4 else 0 for k in range(288)])


def slice_selections(nrows, lens):
    """named row selections of the slice matrix (rows may repeat): the named sizes, empty rows at the end and all over,
    long rows between empty ones"""
    rng = np.random.RandomState(seed("selections"))
    lens = np.asarray(lens)
    empty, short = np.nonzero(lens == 0)[0], np.nonzero(lens <= 10)[0]
    pick = lambda pool, n: pool[rng.randint(0, len(pool), n)]
    row = lambda k: int(np.nonzero(lens == k)[0][0])
    out = [("n1", [row(400)]), ("n1_empty", [row(0)]), ("n255", pick(np.arange(nrows), 255)), ("n256", pick(np.arange(nrows), 256)),
           ("n257", pick(np.arange(nrows), 257)), ("n65537", np.concatenate([pick(short, 65530), [row(400), row(0), row(129), 5, row(65), 0, row(1)]])),
           ("all_empty", pick(empty, 300)), ("ends_empty", np.concatenate([pick(np.arange(nrows), 40), pick(empty, 5)])),
           ("repeated", [row(129), row(129), row(129), 0, row(129), row(1), row(1)]),
           ("long_next_to_empty", [0, row(65), 5, row(128), row(129), 9, row(400), row(63), row(64), 10]),
           ("all_rows", np.arange(nrows)[::-1])]
    return [(name, np.ascontiguousarray(r, np.int32)) for name, r in out]


# ---- the history exchange ---------------------------------------------------------------------------------------------------
X_WORLDS = (1, 2, 3, 8)
X_D = (1, 4, 37, 128, 602)
X_CAP = (1, 5, 64, 1024)


def x_sizes(cap):
    return sorted({0, 1, max(cap - 1, 0), cap})


def exchange_form(world, owner):
    """sgcn_hist_apply_f32: 'claim' (two launches through the owner table) or 'rank' (one scatter launch per rank)"""
    return "claim" if owner and world > 2 else "rank"


def exchange_payload_vw(d, ldh, cap, rank):
    """the vector width launch_rows picks for rank ``rank``'s block in the per-rank form: the payload starts
    rank * cap * (d + 1) + cap words into a 16-byte aligned receive buffer, the table is aligned"""
    return rows_plan(d, d, ldh, (rank * cap * (d + 1) + cap) % 4, 0)["vw"]


def exchange_cases():
    """every world with every d and cap, the block sizes rotating over the ranks; the table's pitch rotates over d, d + 3
    and the next multiple of 4 past d"""
    out = []
    for wi, world in enumerate(X_WORLDS):
        for di, d in enumerate(X_D):
            for ci, cap in enumerate(X_CAP):
                sz = x_sizes(cap)
                sizes = [sz[(r + wi + di + ci) % len(sz)] for r in range(world)]
                if world >= len(sz):
                    assert set(sizes) == set(sz)
                ldh = (d, d + 3, _cdiv(d + 1, 4) * 4)[(wi + di + ci) % 3]
                out.append(dict(world=world, d=d, cap=cap, sizes=sizes, ldh=ldh))
    return out


EXCHANGE_CASES = exchange_cases()

# ---- gather_f32 / scale_rows ------------------------------------------------------------------------------------------------
GATHER_N = (1, 255, 256, 257, kGatherBlocks * kBlock, kGatherBlocks * kBlock + 1, 3 * kGatherBlocks * kBlock + 5)


def scale_cell(d, n):
    """(ragged last vector, n * nvec against the 256 lanes of a workgroup)"""
    nvec = _cdiv(d, 4)
    return (d % 4 != 0, n_pos(n * nvec, kBlock))


def scale_cases():
    """scale_rows takes any width (its contract is on the pitches and bases: multiples of 4 floats, 16-byte aligned), so every
    pool width is a case; the pitches are the next multiple of 4 and 32 (what the product passes), n puts n * nvec below,
    on and one past a workgroup boundary where the width allows"""
    out = []
    for i, d in enumerate(WIDTHS):
        nvec = _cdiv(d, 4)
        for pos in NPOS:
            t = n_at(kBlock, pos, 2)
            n = _cdiv(t, nvec)
            if n * nvec != t:        # not reachable with this width: the nearest n, its own cell
                pos = n_pos(n * nvec, kBlock)
            ldx, ldo = (_cdiv(d, 4) * 4, _cdiv(d + 1, 32) * 32) if i % 2 else (_cdiv(d + 1, 32) * 32, _cdiv(d, 4) * 4 + 4)
            out.append(dict(d=d, n=n, ldx=ldx, ldo=ldo))
    return out


SCALE_CASES = scale_cases()


def scale_reachable():
    return sorted({scale_cell(d, n) for d in WIDTHS for n in range(1, 2 * kBlock + 2)})


# ---- the shipped sizes ------------------------------------------------------------------------------------------------------
REDDIT_N, REDDIT_HID, REDDIT_FEAT = 232965, 128, 1204
BIG_N, BIG_D = 10_000_000, 256       # config 5's history: 10.2 GB of fp32
BIG_SPLIT = (1 << 31) // BIG_D       # the first row whose element offset is 2^31: 8,388,608


def reddit_caps(batch=1000, degree=1, layers=2):
    """the row capacities a compiled program sizes its fields for (step_program.StepProgram: caps[L] = min(N, batch),
    caps[l] = min(N, caps[l + 1] * (1 + degree))) with the Reddit run's batch of 1,000 and one sampled neighbour"""
    caps = [min(REDDIT_N, batch)]
    for _ in range(layers):
        caps.insert(0, min(REDDIT_N, caps[0] * (1 + degree)))
    return caps


def big_ids(n_per_band, key):
    """unique ids of the big table in three bands: element offset below 2^31, above it (byte offset above 2^33), and the
    last rows (byte offset above 10^10); rows 0, 8,388,607, 8,388,608 and 9,999,999 always among them"""
    rng = np.random.RandomState(seed("big", key))
    last_lo = _cdiv(10 ** 10, 4 * BIG_D)
    bands = [rng.choice(BIG_SPLIT, n_per_band, replace=False), BIG_SPLIT + rng.choice(last_lo - BIG_SPLIT, n_per_band, replace=False),
             last_lo + rng.choice(BIG_N - last_lo, n_per_band, replace=False)]
    ids = np.unique(np.concatenate(bands + [np.array([0, BIG_SPLIT - 1, BIG_SPLIT, BIG_N - 1])]))
    assert (ids[ids >= BIG_SPLIT] * BIG_D >= 1 << 31).all() and (ids[ids >= last_lo] * BIG_D * 4 >= 10 ** 10).all()
    return assert_scatter_ids(rng.permutation(ids).astype(np.int32), BIG_N)
