"""Inputs and expected output of tests/host_san/driver.cpp (test-only helper, no device).

The driver is a stand-alone program that links the library's host sources and prints one line per library call,
``name arg=value ... rc=N sum=HEX`` (FNV-1a-64 over the call's output arrays).  This module writes the driver's case files
from ``sparse_cases.CATALOGUE`` (plus four cases of its own) and computes, for every battery and case, the lines the driver
must print: it makes the same calls on the same arrays through the production ``libsgcn.so`` and hashes the outputs the
same way.  The equality ties the driver to the product's call sequences, and catches behaviour that depends on undefined
behaviour or on a race (an -O2 build and an instrumented -O1 build then disagree); that the plans and samples are RIGHT
is the business of test_csplan*.py, test_lds_plan.py, test_sampler.py and test_prefetch.py.

Every function here mirrors the function of the same name in driver.cpp, line for line.
"""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import scipy.sparse as sp

import sparse_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER_DIR = os.path.join(HERE, "host_san")

BATTERIES = ("plan", "csplan", "warp", "transpose", "reorder", "ldsplan", "mult", "sched", "prefetch", "refusals")
THREADED = ("csplan", "warp", "transpose", "ldsplan", "sched", "prefetch")     # run under ThreadSanitizer as well
SQUARE_ONLY = ("reorder", "sched", "prefetch")
TUNE_KEYS = ("cs_deal", "lds_wave_bias", "lds_mix")                            # what the planners read through sgcn_tune_get

CATALOGUE_CASES = ("empty", "one_row", "identity", "permutation", "star_row", "star_col", "hot_block", "row_lengths",
                   "m15_k17", "m16_k16", "m17_k15", "m63_k65", "m65_k63", "m4097_k4095", "k5", "row_vector", "col_vector",
                   "range_empty", "sched_adj", "sched_fadj", "sbm")
OWN_CASES = ("m0", "one_by_one", "multigraph", "isolated")
CASES = CATALOGUE_CASES + OWN_CASES
_KEEP_VALUES = ("identity", "permutation", "sched_adj", "sched_fadj", "sbm")   # the others get dyadic values
_RANDOM_LABELS = ("row_lengths", "m65_k63")                                     # row groups outside the community graph


# ---- cases ------------------------------------------------------------------------------------------------------------
def multigraph():
    """the graph of test_sampler.py::test_vector_and_scalar_full_neighbour_placement_agree: rows of 0 .. 120 neighbours,
    every 16th row with a neighbour repeated inside one 16-entry vector and one repeated across vectors"""
    rng = np.random.RandomState(5)
    n = 400
    rows, cols = [], []
    for r in range(n):
        deg = [0, 1, 3, 15, 16, 17, 40, 120][r % 8]
        c = rng.choice(n, deg, replace=False)
        if r % 16 == 6 and deg >= 3:
            c[2] = c[0]
            c[-1] = c[1]
        rows += [r] * deg
        cols += c.tolist()
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return sp.csr_matrix((rng.rand(len(cols)).astype(np.float32), np.array(cols, np.int32), ptr), shape=(n, n))


def isolated():
    """the graph of test_prefetch.py::test_sampler_error_reaches_the_consumer_through_every_producer_shape: a ring over
    vertices 0 .. 39, vertices 40 .. 63 isolated (a batch of them is an error of the importance sampler)"""
    rows = np.arange(0, 40)
    return sp.csr_matrix((np.ones(40, np.float32), (rows, (rows + 1) % 40)), shape=(64, 64))


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(M, K, rowptr, col, val, row_group, col_pos): the arrays of a case, as the driver's case file holds them"""
    rng = np.random.RandomState(sum(map(ord, name)))
    if name == "m0":
        a = sp.csr_matrix((0, 5), dtype=np.float32)
    elif name == "one_by_one":
        a = sp.csr_matrix(np.ones((1, 1), np.float32))
    elif name == "multigraph":
        a = multigraph()
    elif name == "isolated":
        a = isolated()
    else:
        a = sc.pattern(name).tocsr()
        if name not in _KEEP_VALUES:
            a = sc.dyadic(a, rng)
            if a.shape[0] == a.shape[1]:
                a.data[:] = np.abs(a.data)               # a square case is a graph too: edge weights are positive
    M, K = int(a.shape[0]), int(a.shape[1])
    c = dict(name=name, M=M, K=K, rowptr=np.ascontiguousarray(a.indptr, np.int32), col=np.ascontiguousarray(a.indices, np.int32),
             val=np.ascontiguousarray(a.data, np.float32), row_group=None, col_pos=None)
    labels = None
    if name == "sbm":
        labels = (sc.sbm_labels(), sc.sbm_labels())
    elif name in _RANDOM_LABELS:
        labels = (rng.randint(0, 3, M).astype(np.int32), rng.randint(0, 3, K).astype(np.int32))
    if labels is not None:
        pos2col = np.argsort(labels[1], kind="stable").astype(np.int32)          # ops.LdsPlanHost's sweep positions
        col_pos = np.empty_like(pos2col)
        col_pos[pos2col] = np.arange(K, dtype=np.int32)
        c["row_group"], c["col_pos"] = np.ascontiguousarray(labels[0], np.int32), col_pos
    c["nnz"] = int(c["col"].shape[0])
    assert c["rowptr"].shape[0] == M + 1 and c["rowptr"][0] == 0 and c["rowptr"][-1] == c["nnz"]
    return c


def write_case(name, path):
    c = case(name)
    with open(path, "wb") as f:
        f.write(np.array([c["M"], c["K"], c["nnz"], 1 if c["row_group"] is not None else 0], "<i8").tobytes())
        for k in ("rowptr", "col", "val") + (("row_group", "col_pos") if c["row_group"] is not None else ()):
            f.write(c[k].astype(c[k].dtype.newbyteorder("<")).tobytes())


def applies(battery, name):
    if battery == "refusals":
        return name == "m16_k16"                       # the refusals bring their own arguments
    c = case(name)
    return battery not in SQUARE_ONLY or (c["M"] == c["K"] and c["M"] > 0)


def tune_pairs():
    """the driver's ``key=value`` arguments: the production library's own defaults"""
    from stochastic_gcn_amd._ffi import lib
    return ["%s=%d" % (k, lib.sgcn_tune_get(k.encode())) for k in TUNE_KEYS]


# ---- hashes and buffers --------------------------------------------------------------------------------------------------
_FNV = None
FNV_BASIS = 1469598103934665603


def _fnv():
    """the compiled byte loop (tests/host_san/fnv1a.c), built once per process into a temporary directory"""
    global _FNV
    if _FNV is None:
        d = tempfile.mkdtemp(prefix="sgcn_fnv_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "fnv1a.so")
        subprocess.run(["gcc", "-O2", "-shared", "-fPIC", os.path.join(DRIVER_DIR, "fnv1a.c"), "-o", so], check=True)
        _FNV = C.CDLL(so).fnv1a64
        _FNV.restype = C.c_uint64
        _FNV.argtypes = [C.c_uint64, C.c_void_p, C.c_size_t]
    return _FNV


class Fnv(object):
    def __init__(self):
        self.h = FNV_BASIS

    def add(self, *arrays):
        for a in arrays:
            if a.size:
                self.h = _fnv()(self.h, a.ctypes.data, a.nbytes)
        return self

    def add_ptr(self, address, nbytes):
        if nbytes:
            self.h = _fnv()(self.h, address, nbytes)
        return self

    def hex(self):
        return "%016x" % self.h


NONE = "%016x" % FNV_BASIS           # the sum of a call without output arrays
FILL = 0xA5


def buf(dtype, n):
    """an output array of n elements (>= 1 byte of storage), prefilled like the driver's"""
    n = max(int(n), 0)
    raw = np.full(max(n * np.dtype(dtype).itemsize, 1), FILL, np.uint8)
    a = raw[:n * np.dtype(dtype).itemsize].view(dtype)
    a_base = raw                                         # (the view keeps the storage alive; an empty one still has an address)
    return _Arr(a, a_base)


class _Arr(object):
    """a NumPy array and the address the library gets for it (never NULL, also when empty)"""

    def __init__(self, a, base):
        self.a, self.base = a, base
        self.p = base.ctypes.data

    def untouched(self):
        return bool(np.all(self.base == FILL))


def inp(a):
    """an input array: its address, the address of one spare byte when it is empty"""
    return a.ctypes.data if a.size else _SPARE.ctypes.data


_SPARE = np.zeros(1, np.uint8)
FIX = np.dtype([("row", "<i4"), ("first_slot", "<i4"), ("nslots", "<i4")])
SEG = np.dtype([("row", "<i4"), ("start", "<i4"), ("end", "<i4"), ("slot", "<i4")])


def _lib():
    from stochastic_gcn_amd import _ffi
    return _ffi.lib


class _Env(object):
    """environment variables for the duration of a battery (the library reads them with getenv)"""

    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            _setenv(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            _setenv(k, v)


def _setenv(k, v):
    if v is None:
        os.environ.pop(k, None)
    else:
        os.environ[k] = v


# ---- plan -----------------------------------------------------------------------------------------------------------------
def battery_plan(c, out):
    lib = _lib()
    M = c["M"]
    for T in (0, 1, 64):
        nseg, nfix, nslots = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
        rc = lib.sgcn_plan_count(inp(c["rowptr"]), M, T, C.byref(nseg), C.byref(nfix), C.byref(nslots))
        out.append("plan_count T=%d nseg=%d nfix=%d nslots=%d rc=%d sum=%s" % (T, nseg.value, nfix.value, nslots.value, rc, NONE))
        if rc:
            continue
        seg, fix = buf(SEG, nseg.value), buf(FIX, nfix.value)
        rc = lib.sgcn_plan_fill(inp(c["rowptr"]), M, T, seg.p, fix.p)
        out.append("plan_fill T=%d rc=%d sum=%s" % (T, rc, Fnv().add(seg.a, fix.a).hex()))


# ---- csplan ---------------------------------------------------------------------------------------------------------------
def make_warp(c, max_buckets, out):
    lib = _lib()
    table = buf(np.uint32, max_buckets)
    nb, shift = C.c_int32(0), C.c_int32(0)
    rc = lib.sgcn_cs_warp_table(inp(c["col"]), c["nnz"], c["K"], max_buckets, 1, 0.01, 1, table.p, C.byref(nb), C.byref(shift))
    out.append("cs_warp_table mode=1 max_buckets=%d nbuckets=%d shift=%d rc=%d sum=%s"
               % (max_buckets, nb.value, shift.value, rc, Fnv().add(table.a).hex()))
    return table, nb.value, shift.value


def export_sized(b, rows_per_tile, out):
    lib = _lib()
    nt, ne, nfix, nslots = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    T_used, thr = C.c_int32(-1), C.c_int32(-1)
    rc = lib.sgcn_csbuild_sizes(b, C.byref(nt), C.byref(ne), C.byref(nfix), C.byref(nslots), C.byref(T_used), C.byref(thr))
    out.append("csbuild_sizes ntiles=%d nentries=%d nfix=%d nslots=%d T_used=%d rc=%d sum=%s"
               % (nt.value, ne.value, nfix.value, nslots.value, T_used.value, rc, NONE))
    if rc:
        return
    tile_ptr, colrow, val = buf(np.int64, nt.value + 1), buf(np.int32, ne.value), buf(np.float32, ne.value)
    rows, slots = buf(np.int32, nt.value * rows_per_tile), buf(np.int32, nt.value * rows_per_tile)
    fix = buf(FIX, nfix.value)
    rc = lib.sgcn_csbuild_export(b, tile_ptr.p, colrow.p, val.p, rows.p, slots.p, fix.p)
    out.append("csbuild_export rc=%d sum=%s" % (rc, Fnv().add(tile_ptr.a, colrow.a, val.a, rows.a, slots.a, fix.a).hex()))


def battery_csplan(c, out):
    lib = _lib()
    M, rp, col, val = c["M"], inp(c["rowptr"]), inp(c["col"]), inp(c["val"])
    has_labels = c["row_group"] is not None
    for cfg in range(2):
        R, T = (32, 64) if cfg else (16, 0)
        for rg in range(2 if has_labels else 1):
            grp = inp(c["row_group"]) if rg else None
            nt, nfix, nslots = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
            rc = lib.sgcn_csplan_count(rp, M, R, T, grp, C.byref(nt), C.byref(nfix), C.byref(nslots))
            out.append("csplan_count R=%d T=%d rg=%d ntiles=%d nfix=%d nslots=%d rc=%d sum=%s"
                       % (R, T, rg, nt.value, nfix.value, nslots.value, rc, NONE))
            if rc:
                continue
            tile_ptr, colrow, vo = buf(np.int64, nt.value + 1), buf(np.int32, c["nnz"]), buf(np.float32, c["nnz"])
            rows, slots, fix = buf(np.int32, nt.value * R), buf(np.int32, nt.value * R), buf(FIX, nfix.value)
            rc = lib.sgcn_csplan_fill(rp, col, val, M, R, T, grp, tile_ptr.p, colrow.p, vo.p, rows.p, slots.p, fix.p)
            out.append("csplan_fill R=%d T=%d rg=%d rc=%d sum=%s"
                       % (R, T, rg, rc, Fnv().add(tile_ptr.a, colrow.a, vo.a, rows.a, slots.a, fix.a).hex()))
    table, nb, shift = make_warp(c, 64, out)
    wt = table.p if nb else None
    for G in (2, 4):
        for cfg in range(2):
            T, rt, al = (0, 8, 32) if cfg else (64, 0, 0)
            hw = wt if cfg else None
            nt, ne, nfix, nslots = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
            rc = lib.sgcn_csplang_count(rp, col, M, T, rt, al, G, hw, shift, C.byref(nt), C.byref(ne), C.byref(nfix), C.byref(nslots))
            out.append("csplang_count G=%d T=%d round=%d align=%d warp=%d ntiles=%d nentries=%d nfix=%d nslots=%d rc=%d sum=%s"
                       % (G, T, rt, al, 1 if hw else 0, nt.value, ne.value, nfix.value, nslots.value, rc, NONE))
            if rc:
                continue
            tile_ptr, colrow, vo = buf(np.int64, nt.value + 1), buf(np.int32, ne.value), buf(np.float32, ne.value)
            rows, slots, fix = buf(np.int32, nt.value * 16 * G), buf(np.int32, nt.value * 16 * G), buf(FIX, nfix.value)
            rc = lib.sgcn_csplang_fill(rp, col, val, M, T, rt, al, G, hw, shift, tile_ptr.p, colrow.p, vo.p, rows.p, slots.p, fix.p)
            out.append("csplang_fill G=%d T=%d round=%d align=%d warp=%d rc=%d sum=%s"
                       % (G, T, rt, al, 1 if hw else 0, rc, Fnv().add(tile_ptr.a, colrow.a, vo.a, rows.a, slots.a, fix.a).hex()))
    grid = ((1, 0, 0, 0, 0, 1), (1, 1, 8, 32, 1, 1), (1, 64, 8, 0, 0, 0), (2, 1, 8, 32, 1, 1), (2, 64, 0, 32, 1, 0),
            (4, 0, 0, 0, 0, 1), (4, 64, 8, 32, 1, 0))
    deal0 = lib.sgcn_tune_get(b"cs_deal")
    turn = 0
    try:
        for G, T, rnd, align, warp, deal in grid:
            for rg in range(2 if (G == 1 and has_labels) else 1):
                lib.sgcn_tune(b"cs_deal", deal)
                out.append("tune cs_deal=%d" % deal)
                for nthr in (1, (2, 7, 16, 0)[turn % 4]):
                    b = C.c_void_p()
                    R = (32 if rnd else 16) if G == 1 else 16
                    rc = lib.sgcn_csplan_build(rp, col, val, M, G, R, T, rnd, align, inp(c["row_group"]) if rg else None,
                                               wt if warp else None, shift, nthr, C.byref(b))
                    out.append("csplan_build G=%d R=%d T=%d round=%d align=%d rg=%d warp=%d rc=%d sum=%s"
                               % (G, R, T, rnd, align, rg, 1 if (warp and wt) else 0, rc, NONE))
                    if rc == 0:
                        export_sized(b, R * G, out)
                        lib.sgcn_csbuild_free(b)
                turn += 1
    finally:
        lib.sgcn_tune(b"cs_deal", deal0)


# ---- warp, transpose, reorder -----------------------------------------------------------------------------------------------
def battery_warp(c, out):
    lib = _lib()
    for mode in (0, 1):
        for mb in (1, 64, 4096):
            for nthr in (1, 5):
                table = buf(np.uint32, mb)
                nb, shift = C.c_int32(-1), C.c_int32(-1)
                rc = lib.sgcn_cs_warp_table(inp(c["col"]), c["nnz"], c["K"], mb, mode, 0.01, nthr, table.p, C.byref(nb), C.byref(shift))
                out.append("cs_warp_table mode=%d max_buckets=%d nbuckets=%d shift=%d rc=%d sum=%s"
                           % (mode, mb, nb.value, shift.value, rc, Fnv().add(table.a).hex()))


def battery_transpose(c, out):
    lib = _lib()
    for with_val in (1, 0):
        for nthr in (1, 5):
            trp, tc, tv = buf(np.int32, c["K"] + 1), buf(np.int32, c["nnz"]), buf(np.float32, c["nnz"] if with_val else 0)
            rc = lib.sgcn_csr_transpose_host(inp(c["rowptr"]), inp(c["col"]), inp(c["val"]) if with_val else None, c["M"], c["K"], nthr,
                                             trp.p, tc.p, tv.p if with_val else None)
            out.append("csr_transpose_host values=%d rc=%d sum=%s" % (with_val, rc, Fnv().add(trp.a, tc.a, tv.a).hex()))


def battery_reorder(c, out):
    lib = _lib()
    n = c["M"]
    for max_iters, seed, min_size in ((0, 1, 64), (3, 7, 1)):
        comm = buf(np.int32, n)
        nc = C.c_int32(-1)
        rc = lib.sgcn_reorder_lp(inp(c["rowptr"]), inp(c["col"]), n, max_iters, seed, min_size, comm.p, C.byref(nc))
        out.append("reorder_lp max_iters=%d seed=%d min_size=%d ncomm=%d rc=%d sum=%s"
                   % (max_iters, seed, min_size, nc.value, rc, Fnv().add(comm.a).hex()))


# ---- ldsplan --------------------------------------------------------------------------------------------------------------
def battery_ldsplan(c, out):
    lib = _lib()
    M, K, VW, NW = c["M"], c["K"], 2, 8
    RW = 192 // VW
    for lab in range(2 if c["row_group"] is not None else 1):
        for T in (0, 16):
            for reuse in (1, 2, 3):
                for mode in (0, 1):
                    for ring in (80, 128):
                        h = C.c_void_p()
                        rc = lib.sgcn_ldsplan_create(inp(c["rowptr"]), inp(c["col"]), inp(c["val"]), M, K,
                                                     inp(c["col_pos"]) if lab else None, inp(c["row_group"]) if lab else None,
                                                     VW, T, reuse, mode, ring, C.byref(h))
                        out.append("ldsplan_create labels=%d T=%d min_reuse=%d mode=%d ring_slots=%d rc=%d sum=%s"
                                   % (lab, T, reuse, mode, ring, rc, NONE))
                        if rc:
                            continue
                        sz = buf(np.int64, 19)
                        rc = lib.sgcn_ldsplan_sizes(h, sz.p)
                        out.append("ldsplan_sizes rc=%d sum=%s" % (rc, Fnv().add(sz.a).hex()))
                        nt, nch, nent, nfix, rnnz, S = (int(sz.a[i]) for i in (0, 1, 2, 3, 5, 17))
                        arrs = [buf(np.int32, nt + 1), buf(np.int32, nch * S), buf(np.int32, nch * NW * 32), buf(np.int64, nch * NW + 1),
                                buf(np.uint32, nent + 256), buf(np.float32, nent + 256), buf(np.float32, M),
                                buf(np.int32, nt * NW * RW), buf(np.int32, nt * NW * RW), buf(FIX, nfix),
                                buf(np.int32, M + 1), buf(np.int32, rnnz), buf(np.float32, rnnz)]
                        rc = lib.sgcn_ldsplan_export(h, *[x.p for x in arrs])
                        out.append("ldsplan_export rc=%d sum=%s" % (rc, Fnv().add(*[x.a for x in arrs]).hex()))
                        lib.sgcn_ldsplan_destroy(h)


# ---- mult -----------------------------------------------------------------------------------------------------------------
def battery_mult(c, out):
    from stochastic_gcn_amd import _ffi
    lib = _lib()
    n = min(max(c["M"], 1), 300)
    prob = (((np.arange(n) * 7 + 3) % 11 + 1).astype(np.float32) / np.float32(8.0)).astype(np.float32)
    m = C.c_void_p()
    rc = lib.sgcn_mult_create(inp(prob), n, C.byref(m))
    out.append("mult_create n=%d rc=%d sum=%s" % (n, rc, NONE))
    if rc:
        return
    bit, ln = _ffi.c_f32p(), C.c_int64(-1)
    rc = lib.sgcn_mult_tree(m, C.byref(bit), C.byref(ln))
    f = Fnv()
    if rc == 0:
        f.add_ptr(C.cast(bit, C.c_void_p).value, ln.value * 4)
    out.append("mult_tree len=%d rc=%d sum=%s" % (ln.value, rc, f.hex()))
    for u in (0.0, 0.125, 0.5, 0.875):
        r = C.c_int32(-1)
        rc = lib.sgcn_mult_query_u(m, u, C.byref(r))
        out.append("mult_query_u u=%.3f result=%d rc=%d sum=%s" % (u, r.value, rc, NONE))
    for _ in range(min(n, 5)):
        r = C.c_int32(-1)
        rc = lib.sgcn_mult_query(m, C.byref(r))
        out.append("mult_query result=%d rc=%d sum=%s" % (r.value, rc, NONE))
    lib.sgcn_mult_destroy(m)


# ---- sched ----------------------------------------------------------------------------------------------------------------
L, CLASSES, PLAN_T = 2, 2, 2
DEGREES = np.array([2, 3], np.int32)
ERR_EMPTY_PROB, ERR_NAN = -3, -4


class Graph(object):
    def __init__(self, c):
        self.c, self.n = c, c["M"]
        i = np.arange(self.n)[:, None] + np.arange(CLASSES)[None, :]
        self.labels = np.ascontiguousarray((i % 3).astype(np.float32))
        self.deg = DEGREES.copy()


def batch_ids(n, bs, b):
    return ((b * bs + np.arange(bs, dtype=np.int64)) % n).astype(np.int32)


def new_sampler(c, cv, is_, seed, out):
    lib = _lib()
    s = C.c_void_p()
    rc = lib.sgcn_sched_create(inp(c["val"]), inp(c["col"]), inp(c["rowptr"]), c["M"], c["nnz"], L, cv, is_, C.byref(s))
    out.append("sched_create cv=%d is=%d rc=%d sum=%s" % (cv, is_, rc, NONE))
    if rc:
        return None
    rc = lib.sgcn_sched_seed(s, seed)
    out.append("sched_seed seed=%d rc=%d sum=%s" % (seed, rc, NONE))
    return s


def batch_tail(ni, nf, rc, meta, iaddr, faddr):
    f = Fnv()
    if rc == 0:
        f.add(meta.a).add_ptr(iaddr, ni * 4).add_ptr(faddr, nf * 4)
    return "n_i=%d n_f=%d rc=%d sum=%s" % (ni if rc == 0 else -1, nf if rc == 0 else -1, rc, f.hex())


def sequential(g, s, bs, nb, words, out):
    lib = _lib()
    tails = []
    ml = lib.sgcn_sched_packed_meta_len(L)
    for b in range(nb):
        ids = batch_ids(g.n, bs, b)
        meta = buf(np.int64, ml)
        ni, nf = C.c_int64(-1), C.c_int64(-1)
        rc = lib.sgcn_sched_batch_packed(s, bs, inp(ids), L, inp(g.deg), inp(g.labels), CLASSES, PLAN_T, meta.p, ml, C.byref(ni), C.byref(nf))
        if rc == 0:
            ib, fb = buf(np.int32, max(ni.value, 1)), buf(np.float32, max(nf.value, 1))
            lib.sgcn_sched_packed_copy(s, ib.p, fb.p)
            tails.append(batch_tail(ni.value, nf.value, rc, meta, ib.p, fb.p))
            if words is not None:
                words.append(max(ni.value, 1) + max(nf.value, 1))
        else:
            tails.append(batch_tail(ni.value, nf.value, rc, meta, None, None))
        out.append("sched_batch_packed b=%d " % b + tails[-1])
        if rc:
            break
    return tails


def battery_sched(c, out):
    from stochastic_gcn_amd import _ffi
    lib = _lib()
    g = Graph(c)
    bs, nb = min(g.n, 24), 5
    for novec in (0, 1):
        with _Env(SGCN_NO_AVX512="1" if novec else None):
            out.append("env SGCN_NO_AVX512=%d" % novec)
            for cv in (0, 1):
                for is_ in (0, 1):
                    s = new_sampler(c, cv, is_, 3, out)
                    if s is None:
                        continue
                    ids = batch_ids(g.n, bs, 0)
                    rc = lib.sgcn_sched_start_batch(s, bs, inp(ids))
                    out.append("sched_start_batch n=%d rc=%d sum=%s" % (bs, rc, NONE))
                    for l in range(L):
                        if rc:
                            break
                        rc = lib.sgcn_sched_expand(s, int(DEGREES[L - l - 1]))
                        out.append("sched_expand degree=%d rc=%d sum=%s" % (DEGREES[L - l - 1], rc, NONE))
                        if rc:
                            break
                        for which in range(11):
                            p, ln = _ffi.c_i32p(), C.c_int64(-1)
                            r2 = lib.sgcn_sched_view_i32(s, which, C.byref(p), C.byref(ln))
                            f = Fnv()
                            if r2 == 0:
                                f.add_ptr(C.cast(p, C.c_void_p).value, ln.value * 4)
                            out.append("sched_view_i32 which=%d len=%d rc=%d sum=%s" % (which, ln.value, r2, f.hex()))
                        for which in range(6):
                            p, ln = _ffi.c_f32p(), C.c_int64(-1)
                            r2 = lib.sgcn_sched_view_f32(s, which, C.byref(p), C.byref(ln))
                            f = Fnv()
                            if r2 == 0:
                                f.add_ptr(C.cast(p, C.c_void_p).value, ln.value * 4)
                            out.append("sched_view_f32 which=%d len=%d rc=%d sum=%s" % (which, ln.value, r2, f.hex()))
                    lib.sgcn_sched_destroy(s)
                    scout = new_sampler(c, cv, is_, 5, out)
                    if scout is None:
                        continue
                    words = []
                    want = sequential(g, scout, bs, nb, words, out)
                    lib.sgcn_sched_destroy(scout)
                    s = new_sampler(c, cv, is_, 5, out)
                    if s is None:
                        continue
                    ml = lib.sgcn_sched_packed_meta_len(L)
                    for b in range(len(want)):
                        bi = batch_ids(g.n, bs, b)
                        meta = buf(np.int64, ml)
                        ni, nf = C.c_int64(-1), C.c_int64(-1)
                        known = b < len(words)
                        small = known and bool(b & 1)
                        cap = words[b] - (1 if small else 0) if known else 2
                        stage = buf(np.int32, cap)
                        rc = lib.sgcn_sched_batch_packed_into(s, bs, inp(bi), L, inp(g.deg), inp(g.labels), CLASSES, PLAN_T, meta.p, ml,
                                                              stage.p, cap, C.byref(ni), C.byref(nf))
                        if rc == 1:
                            ib, fb = buf(np.int32, max(ni.value, 1)), buf(np.float32, max(nf.value, 1))
                            lib.sgcn_sched_packed_copy(s, ib.p, fb.p)
                            tail = batch_tail(ni.value, nf.value, 0, meta, ib.p, fb.p)
                        elif rc == 0:
                            tail = batch_tail(ni.value, nf.value, 0, meta, stage.p, stage.p + 4 * max(ni.value, 1))
                        else:
                            tail = batch_tail(ni.value, nf.value, rc, meta, None, None)
                        out.append("sched_batch_packed_into b=%d small=%d ret=%d " % (b, 1 if small else 0, rc) + tail)
                        if rc < 0:
                            break
                    lib.sgcn_sched_destroy(s)


# ---- prefetch -------------------------------------------------------------------------------------------------------------
def epochs(nb):
    # samplers packers lag slots batches take cv is small_slot compare
    return ((1, 0, 0, 3, nb, nb + 1, 1, 0, -1, True), (1, 2, 1, 6, nb, nb + 1, 1, 0, -1, True), (3, 0, 1, 8, nb, nb + 1, 1, 0, -1, False),
            (1, 0, 0, 3, nb, nb + 1, 1, 0, 1, True), (1, 2, 1, 6, nb, nb + 1, 0, 0, 2, True), (1, 0, 1, 4, nb, 4, 1, 0, -1, True),
            (1, 2, 0, 5, nb, 4, 1, 0, -1, True), (3, 0, 0, 7, nb, 4, 0, 0, -1, False), (1, 0, 0, 3, 0, 1, 1, 0, -1, True),
            (1, 2, 0, 5, 0, 1, 1, 0, -1, True), (1, 0, 0, 3, nb, nb + 1, 0, 1, -1, True), (1, 1, 0, 3, nb, nb + 1, 0, 1, -1, True),
            (1, 3, 0, 7, nb, nb + 1, 0, 1, -1, True))


def run_epoch(g, e, bs, out):
    lib = _lib()
    n_samplers, n_packers, lag, n_slots, nb, take, cv, is_, small_slot, compare = e
    out.append("epoch samplers=%d packers=%d lag=%d slots=%d batches=%d take=%d cv=%d is=%d small_slot=%d"
               % (n_samplers, n_packers, lag, n_slots, nb, take, cv, is_, small_slot))
    if compare:
        seq = new_sampler(g.c, cv, is_, 11, out)
        if seq is None:
            return
        sequential(g, seq, bs, nb, None, out)
        lib.sgcn_sched_destroy(seq)
    ss = []
    for k in range(n_samplers):
        s = new_sampler(g.c, cv, is_, 11 + 1000 * k, out)
        if s is None:
            return
        ss.append(s)
    handles = (C.c_void_p * n_samplers)(*[s.value for s in ss])
    ids = np.concatenate([batch_ids(g.n, bs, b) for b in range(nb)]) if nb else np.zeros(0, np.int32)
    off = (np.arange(nb + 1, dtype=np.int64) * bs)
    caps = [2 if i == small_slot else (1 << 20) for i in range(n_slots)]
    slots = [buf(np.int32, cap) for cap in caps]
    ptrs = (C.c_void_p * n_slots)(*[s.p for s in slots])
    caps_c = (C.c_int64 * n_slots)(*caps)
    p = C.c_void_p()
    rc = lib.sgcn_prefetch_start(handles, n_samplers, nb, inp(ids), inp(off), L, inp(g.deg), inp(g.labels), CLASSES, PLAN_T, n_slots,
                                 ptrs, caps_c, lag, n_packers, C.byref(p))
    out.append("prefetch_start rc=%d sum=%s" % (rc, NONE))
    if rc == 0:
        ml = lib.sgcn_sched_packed_meta_len(L)
        pending = []
        for b in range(take):
            while len(pending) > lag:
                r2 = lib.sgcn_prefetch_release(p, pending.pop(0))
                out.append("prefetch_release rc=%d sum=%s" % (r2, NONE))
            slot, ni, nf, spill = C.c_int32(-1), C.c_int64(-1), C.c_int64(-1), C.c_void_p()
            meta = buf(np.int64, ml)
            rc = lib.sgcn_prefetch_next(p, C.byref(slot), meta.p, C.byref(ni), C.byref(nf), C.byref(spill))
            if rc == 1:
                out.append("prefetch_next b=%d end rc=1 sum=%s" % (b, NONE))
                break
            if rc < 0:
                out.append("prefetch_next b=%d " % b + batch_tail(ni.value, nf.value, rc, meta, None, None))
                break
            n1 = max(ni.value, 1)
            w = spill.value if spill.value else slots[slot.value].p
            out.append("prefetch_next b=%d " % b + batch_tail(ni.value, nf.value, 0, meta, w, w + 4 * n1))
            if spill.value:
                r2 = lib.sgcn_prefetch_release(p, slot.value)
                out.append("prefetch_release rc=%d sum=%s" % (r2, NONE))
            else:
                pending.append(slot.value)
        st = (C.c_double * 4)()
        r2 = lib.sgcn_prefetch_stats(p, st)
        out.append("prefetch_stats rc=%d sum=%s" % (r2, NONE))
        lib.sgcn_prefetch_stop(p)
        out.append("prefetch_stop")
    for s in ss:
        lib.sgcn_sched_start_batch(s, bs, inp(batch_ids(g.n, bs, 0)))
        lib.sgcn_sched_destroy(s)


def battery_prefetch(c, out):
    g = Graph(c)
    bs = min(g.n, 16)
    for e in epochs(12):
        run_epoch(g, e, bs, out)


# ---- refusals -------------------------------------------------------------------------------------------------------------
UNSET = 0x5a5a5a5a5a5a5a5a
UNSET32 = 0x5a5a5a5a
_TINY = np.array([0, 1, 2], np.int32)


def refused(what, rc, clean, out):
    lib = _lib()
    msg = lib.sgcn_last_error()
    out.append("refuse %s rc=%d message=%d clean=%d" % (what, rc, 1 if msg else 0, 1 if clean else 0))
    a, b, c = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    ok = lib.sgcn_plan_count(inp(_TINY), 2, 0, C.byref(a), C.byref(b), C.byref(c))
    out.append("plan_count nseg=%d nfix=%d nslots=%d rc=%d" % (a.value, b.value, c.value, ok))


def _handle():
    return C.c_void_p(UNSET)


def _hclean(h):
    return h.value in (None, UNSET)


def battery_refusals(_, out):
    from stochastic_gcn_amd import _ffi
    lib = _lib()
    i32 = lambda *v: np.array(v, np.int32)          # noqa: E731
    rp, bad_rp, col, grp, neg_grp = i32(0, 1, 2), i32(0, 2, 1), i32(0, 1), i32(0, 0), i32(0, -1)
    val = np.array([1.0, 2.0], np.float32)
    warp = np.zeros(4, np.uint32)
    R = lambda what, rc, clean: refused(what, rc, clean, out)          # noqa: E731

    def outs(n=4):
        return [C.c_int64(UNSET) for _ in range(n)]

    def unset(xs):
        return all(x.value == UNSET for x in xs)

    def build(rowptr, colp, M, G, Rr, rg, wp, shift, what, out_handle=True):
        h = _handle()
        rc = lib.sgcn_csplan_build(inp(rowptr), colp, inp(val), M, G, Rr, 0, 0, 0, rg, wp, shift, 1, C.byref(h) if out_handle else None)
        R(what, rc, _hclean(h))

    def lds(rowptr, M, K, pos, rg, VW, ring, what, out_handle=True):
        h = _handle()
        rc = lib.sgcn_ldsplan_create(inp(rowptr), inp(col), inp(val), M, K, pos, rg, VW, 0, 1, 0, ring, C.byref(h) if out_handle else None)
        R(what, rc, _hclean(h))

    # negative M
    x = outs(); rc = lib.sgcn_plan_count(inp(rp), -1, 0, C.byref(x[0]), C.byref(x[1]), C.byref(x[2])); R("plan_count M=-1", rc, unset(x))
    seg, fix = buf(SEG, 2), buf(FIX, 1)
    rc = lib.sgcn_plan_fill(inp(rp), -1, 0, seg.p, fix.p); R("plan_fill M=-1", rc, seg.untouched() and fix.untouched())
    x = outs(); rc = lib.sgcn_csplan_count(inp(rp), -1, 16, 0, None, C.byref(x[0]), C.byref(x[1]), C.byref(x[2])); R("csplan_count M=-1", rc, unset(x))
    x = outs(); rc = lib.sgcn_csplang_count(inp(rp), inp(col), -1, 0, 0, 0, 2, None, 0, *[C.byref(v) for v in x]); R("csplang_count M=-1", rc, unset(x))
    build(rp, inp(col), -1, 1, 16, None, None, 0, "csplan_build M=-1")
    lds(rp, -1, 2, None, None, 2, 0, "ldsplan_create M=-1")
    trp, tc, tv = buf(np.int32, 3), buf(np.int32, 2), buf(np.float32, 2)
    rc = lib.sgcn_csr_transpose_host(inp(rp), inp(col), inp(val), -1, 2, 1, trp.p, tc.p, tv.p)
    R("csr_transpose_host M=-1", rc, trp.untouched() and tc.untouched() and tv.untouched())
    comm, nc = buf(np.int32, 2), C.c_int32(UNSET32)
    rc = lib.sgcn_reorder_lp(inp(rp), inp(col), -1, 0, 1, 1, comm.p, C.byref(nc)); R("reorder_lp n=-1", rc, comm.untouched() and nc.value == UNSET32)
    h = _handle(); rc = lib.sgcn_sched_create(inp(val), inp(col), inp(rp), -1, 2, 1, 0, 0, C.byref(h)); R("sched_create num_data=-1", rc, _hclean(h))

    # a row pointer that goes down
    x = outs(); rc = lib.sgcn_plan_count(inp(bad_rp), 2, 0, C.byref(x[0]), C.byref(x[1]), C.byref(x[2])); R("plan_count rowptr", rc, unset(x))
    seg, fix = buf(SEG, 2), buf(FIX, 1)
    rc = lib.sgcn_plan_fill(inp(bad_rp), 2, 0, seg.p, fix.p); R("plan_fill rowptr", rc, seg.untouched() and fix.untouched())
    x = outs(); rc = lib.sgcn_csplan_count(inp(bad_rp), 2, 16, 0, None, C.byref(x[0]), C.byref(x[1]), C.byref(x[2])); R("csplan_count rowptr", rc, unset(x))
    build(bad_rp, inp(col), 2, 1, 16, None, None, 0, "csplan_build rowptr")
    build(bad_rp, inp(col), 2, 2, 16, None, None, 0, "csplan_build G=2 rowptr")
    lds(bad_rp, 2, 2, None, None, 2, 0, "ldsplan_create rowptr")

    # a column id that does not fit the packed word
    for form in range(4):
        Rr = 32 if form == 1 else 16
        G = 1 if form < 2 else (2 if form == 2 else 4)
        limit = (1 << 27) if Rr == 32 else (1 << 28)
        for over in (1, 0):
            c1 = i32(3, limit if over else limit - 1)
            nt, ne, nf, ns = C.c_int64(-1), C.c_int64(2), C.c_int64(0), C.c_int64(0)
            if G == 1:
                lib.sgcn_csplan_count(inp(rp), 2, Rr, 0, None, C.byref(nt), C.byref(nf), C.byref(ns))
            else:
                lib.sgcn_csplang_count(inp(rp), inp(col) if over else inp(c1), 2, 0, 0, 0, G, None, 0, C.byref(nt), C.byref(ne), C.byref(nf), C.byref(ns))
            tp, cr, vo = buf(np.int64, nt.value + 1), buf(np.int32, ne.value), buf(np.float32, ne.value)
            rows, slots, fx = buf(np.int32, nt.value * Rr * G), buf(np.int32, nt.value * Rr * G), buf(FIX, nf.value)
            if G == 1:
                rc = lib.sgcn_csplan_fill(inp(rp), inp(c1), inp(val), 2, Rr, 0, None, tp.p, cr.p, vo.p, rows.p, slots.p, fx.p)
            else:
                rc = lib.sgcn_csplang_fill(inp(rp), inp(c1), inp(val), 2, 0, 0, 0, G, None, 0, tp.p, cr.p, vo.p, rows.p, slots.p, fx.p)
            what = "%s R=%d G=%d col=2^%d%s" % ("csplan_fill" if G == 1 else "csplang_fill", Rr, G, 27 if Rr == 32 else 28, "" if over else "-1")
            if over:
                R(what, rc, all(b.untouched() for b in (tp, cr, vo, rows, slots)))
            else:
                out.append("accept %s rc=%d sum=%s" % (what, rc, Fnv().add(tp.a, cr.a, vo.a, rows.a, slots.a, fx.a).hex()))

    # a negative group label
    x = outs(); rc = lib.sgcn_csplan_count(inp(rp), 2, 16, 0, inp(neg_grp), C.byref(x[0]), C.byref(x[1]), C.byref(x[2])); R("csplan_count group=-1", rc, unset(x))
    build(rp, inp(col), 2, 1, 16, inp(neg_grp), None, 0, "csplan_build group=-1")
    lds(rp, 2, 2, None, inp(neg_grp), 2, 0, "ldsplan_create group=-1")
    build(rp, inp(col), 2, 2, 16, inp(grp), None, 0, "csplan_build G=2 grouped")

    # warp_shift 28
    x = outs(); rc = lib.sgcn_csplang_count(inp(rp), inp(col), 2, 0, 0, 0, 2, inp(warp), 28, *[C.byref(v) for v in x]); R("csplang_count warp_shift=28", rc, unset(x))
    build(rp, inp(col), 2, 2, 16, None, inp(warp), 28, "csplan_build warp_shift=28")

    # three lane groups
    x = outs(); rc = lib.sgcn_csplang_count(inp(rp), inp(col), 2, 0, 0, 0, 3, None, 0, *[C.byref(v) for v in x]); R("csplang_count ngroups=3", rc, unset(x))
    tp, cr, vo, rows, slots, fx = buf(np.int64, 2), buf(np.int32, 128), buf(np.float32, 128), buf(np.int32, 48), buf(np.int32, 48), buf(FIX, 0)
    rc = lib.sgcn_csplang_fill(inp(rp), inp(col), inp(val), 2, 0, 0, 0, 3, None, 0, tp.p, cr.p, vo.p, rows.p, slots.p, fx.p)
    R("csplang_fill ngroups=3", rc, all(b.untouched() for b in (tp, cr, vo, rows, slots)))
    build(rp, inp(col), 2, 3, 16, None, None, 0, "csplan_build ngroups=3")
    build(rp, inp(col), 2, 1, 33, None, None, 0, "csplan_build R=33")

    # null required pointers
    x = outs(); rc = lib.sgcn_plan_count(None, 2, 0, C.byref(x[0]), C.byref(x[1]), C.byref(x[2])); R("plan_count rowptr=null", rc, unset(x))
    x = outs(); rc = lib.sgcn_plan_count(inp(rp), 2, 0, C.byref(x[0]), None, C.byref(x[2])); R("plan_count nfix=null", rc, unset(x))
    rc = lib.sgcn_plan_fill(inp(rp), 2, 0, None, None); R("plan_fill seg=null", rc, True)
    seg = buf(SEG, 3)
    rc = lib.sgcn_plan_fill(inp(i32(0, 2, 3)), 2, 1, seg.p, None); R("plan_fill fix=null", rc, seg.untouched())
    x = outs(); rc = lib.sgcn_csplan_count(inp(rp), 2, 16, 0, None, None, C.byref(x[1]), C.byref(x[2])); R("csplan_count ntiles=null", rc, unset(x))
    build(rp, inp(col), 2, 1, 16, None, None, 0, "csplan_build out=null", out_handle=False)
    build(rp, None, 2, 1, 16, None, None, 0, "csplan_build col=null")
    x = outs(); rc = lib.sgcn_csbuild_sizes(None, C.byref(x[0]), C.byref(x[1]), C.byref(x[2]), C.byref(x[3]), None, None); R("csbuild_sizes b=null", rc, unset(x))
    rc = lib.sgcn_csbuild_export(None, None, None, None, None, None, None); R("csbuild_export b=null", rc, True)
    h = C.c_void_p()
    lib.sgcn_csplan_build(inp(rp), inp(col), inp(val), 2, 1, 16, 0, 0, 0, None, None, 0, 1, C.byref(h))
    cr, vo = buf(np.int32, 2), buf(np.float32, 2)
    rc = lib.sgcn_csbuild_export(h, None, cr.p, vo.p, None, None, None); R("csbuild_export tile_ptr=null", rc, cr.untouched() and vo.untouched())
    lib.sgcn_csbuild_free(h)
    table, sh = buf(np.uint32, 4), C.c_int32(UNSET32)
    rc = lib.sgcn_cs_warp_table(inp(col), 2, 2, 4, 1, 0.01, 1, table.p, None, C.byref(sh)); R("cs_warp_table nbuckets=null", rc, table.untouched() and sh.value == UNSET32)
    tc, tv = buf(np.int32, 2), buf(np.float32, 2)
    rc = lib.sgcn_csr_transpose_host(inp(rp), inp(col), inp(val), 2, 2, 1, None, tc.p, tv.p); R("csr_transpose_host t_rowptr=null", rc, tc.untouched() and tv.untouched())
    rc = lib.sgcn_sched_create(inp(val), inp(col), inp(rp), 2, 2, 1, 0, 0, None); R("sched_create out=null", rc, True)
    rc = lib.sgcn_mult_create(inp(val), 2, None); R("mult_create out=null", rc, True)
    lds(rp, 2, 2, None, None, 2, 0, "ldsplan_create out=null", out_handle=False)
    sz = buf(np.int64, 19); rc = lib.sgcn_ldsplan_sizes(None, sz.p); R("ldsplan_sizes h=null", rc, sz.untouched())
    lds(rp, 2, 2, None, None, 4, 0, "ldsplan_create VW=4")
    lds(rp, 2, 2, None, None, 2, 96, "ldsplan_create ring_slots=96")
    lds(rp, 2, 2, inp(i32(1, 1)), None, 2, 0, "ldsplan_create col_pos repeated")
    lds(rp, 2, 1, None, None, 2, 0, "ldsplan_create col>=K")

    # max_buckets 0; a column outside [0, K)
    table, nb, sh = buf(np.uint32, 4), C.c_int32(UNSET32), C.c_int32(UNSET32)
    rc = lib.sgcn_cs_warp_table(inp(col), 2, 2, 0, 1, 0.01, 1, table.p, C.byref(nb), C.byref(sh))
    R("cs_warp_table max_buckets=0", rc, table.untouched() and nb.value == UNSET32 and sh.value == UNSET32)
    table, nb, sh = buf(np.uint32, 4), C.c_int32(UNSET32), C.c_int32(UNSET32)
    rc = lib.sgcn_cs_warp_table(inp(col), 2, 1, 4, 1, 0.01, 1, table.p, C.byref(nb), C.byref(sh)); R("cs_warp_table col>=K", rc, table.untouched())
    trp, tc, tv = buf(np.int32, 2), buf(np.int32, 2), buf(np.float32, 2)
    rc = lib.sgcn_csr_transpose_host(inp(rp), inp(col), inp(val), 2, 1, 1, trp.p, tc.p, tv.p)
    R("csr_transpose_host col>=K", rc, trp.untouched() and tc.untouched() and tv.untouched())

    # an empty probability vector
    h = _handle(); rc = lib.sgcn_mult_create(inp(val), 0, C.byref(h)); R("mult_create n=0", rc, _hclean(h))

    # a descriptor table one short
    s = C.c_void_p()
    lib.sgcn_sched_create(inp(val), inp(col), inp(rp), 2, 2, 1, 1, 0, C.byref(s))
    ml = lib.sgcn_sched_packed_meta_len(1)
    meta = buf(np.int64, ml - 1)
    lab = np.arange(4, dtype=np.float32)
    ids, deg = i32(0, 1), i32(1)
    x = outs(2)
    rc = lib.sgcn_sched_batch_packed(s, 2, inp(ids), 1, inp(deg), inp(lab), 2, 0, meta.p, ml - 1, C.byref(x[0]), C.byref(x[1]))
    R("sched_batch_packed meta_cap-1", rc, meta.untouched() and unset(x))
    stage = buf(np.int32, 64)
    x = outs(2)
    rc = lib.sgcn_sched_batch_packed_into(s, 2, inp(ids), 1, inp(deg), inp(lab), 2, 0, meta.p, ml - 1, stage.p, 64, C.byref(x[0]), C.byref(x[1]))
    R("sched_batch_packed_into meta_cap-1", rc, meta.untouched() and stage.untouched() and unset(x))
    p, ln = _ffi.c_i32p(), C.c_int64(UNSET)
    rc = lib.sgcn_sched_view_i32(s, 11, C.byref(p), C.byref(ln)); R("sched_view_i32 which=11", rc, not p and ln.value == UNSET)
    q, ln = _ffi.c_f32p(), C.c_int64(UNSET)
    rc = lib.sgcn_sched_view_f32(s, 6, C.byref(q), C.byref(ln)); R("sched_view_f32 which=6", rc, not q and ln.value == UNSET)
    off, w0, w1 = np.array([0, 2], np.int64), buf(np.int32, 8), buf(np.int32, 8)
    caps, ptrs = (C.c_int64 * 2)(8, 8), (C.c_void_p * 2)(w0.p, w1.p)
    one, two = (C.c_void_p * 1)(s.value), (C.c_void_p * 2)(s.value, s.value)
    h = _handle()
    rc = lib.sgcn_prefetch_start(None, 1, 1, inp(ids), inp(off), 1, inp(deg), inp(lab), 2, 0, 2, ptrs, caps, 0, 0, C.byref(h))
    R("prefetch_start samplers=null", rc, _hclean(h))
    h = _handle()
    rc = lib.sgcn_prefetch_start(one, 1, 1, inp(ids), inp(off), 1, inp(deg), inp(lab), 2, 0, 2, ptrs, caps, 1, 0, C.byref(h))
    R("prefetch_start lag+1>=n_slots", rc, _hclean(h))
    h = _handle()
    rc = lib.sgcn_prefetch_start(two, 2, 1, inp(ids), inp(off), 1, inp(deg), inp(lab), 2, 0, 2, ptrs, caps, 0, 1, C.byref(h))
    R("prefetch_start packers with two samplers", rc, _hclean(h))
    rc = lib.sgcn_prefetch_release(None, 0); R("prefetch_release p=null", rc, True)
    full = buf(np.int64, ml)
    x = outs(2)
    lib.sgcn_sched_batch_packed(s, 2, inp(ids), 1, inp(deg), inp(lab), 2, 0, full.p, ml, C.byref(x[0]), C.byref(x[1]))
    lib.sgcn_sched_destroy(s)


_BATTERY = dict(plan=battery_plan, csplan=battery_csplan, warp=battery_warp, transpose=battery_transpose, reorder=battery_reorder,
                ldsplan=battery_ldsplan, mult=battery_mult, sched=battery_sched, prefetch=battery_prefetch, refusals=battery_refusals)


@functools.lru_cache(maxsize=None)
def expected(battery, name):
    """the lines the driver prints for (battery, case): the same calls through the production library"""
    out = []
    with _Env(SGCN_PLAN_THREADS="8", SGCN_NO_AVX512=None):
        _BATTERY[battery](case(name), out)
    return tuple(out)
