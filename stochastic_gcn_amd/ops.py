"""Device ops of the hot path: thin wrappers that hand raw HBM pointers of PyTorch-ROCm tensors
to the C-ABI of libsgcn.so (include/sgcn.h).  PyTorch is used for device memory and streams
only; every op here is a hand-written HIP kernel and raises if the library is unavailable or
a tensor is not on a GPU (no eager / CPU fallback).

Reference seams replaced:
  spmm            dot(x, y, sparse=True)                    gcn/layers.py:31-37
  vr_aggregate    VRAggregator._call                        gcn/layers.py:298-319,350-362
  gather_rows     history.dense_slice / tf.gather           gcn/_history.pyx:53-62, layers.py:304
  scatter_rows    tf.scatter_update                         gcn/models.py:165
  csr_slice       history.slice                             gcn/_history.pyx:25-51
  dense_fwd / dense_bwd / gemm / dropout   the dense layers around the aggregators (dot + MyLayerNorm
                  + relu + tf.nn.dropout and their autodiff) gcn/layers.py:87-138,365-433
  spmm_cs         the same product as spmm for a STATIC graph (column sweep, ColumnSweepCSR)
  moments_add / moments_summary   Stat.add + np.mean / np.std of the kept draws   gcn/stats.py,
                  gcn/train.py:241-276 (running fp64 statistics on the device, stats.DeviceStat)
  spmax / spmax_bwd   the element-wise neighbour maximum over a CSR pattern and its backward (--aggregator max: GraphSAGE's pooling
                  aggregator without its MLP; no reference counterpart)
  spattn / spattn_bwd   softmax dot-product attention over a CSR pattern and its backward (--aggregator attn: every vertex weighs
                  its neighbours by a softmax over pairwise scores; no reference counterpart); ``keep`` < 1: dropout on the
                  coefficients (--attn_dropout) under the hash mask of attn_key / attn_kept
  csr_induce      the induced subgraph A[S, S] of a resident CSR with its stable transpose and plans, cut on the device
                  (--full_batch_parts: the matrix of a Cluster-GCN step; no reference counterpart)
  history_error   how far a stored history is from the exact activations (no reference counterpart; exact_history.py)
"""
import ctypes as C
import time

import numpy as np
import torch

from . import _ffi
from ._ffi import check, lib
from .scheduler import build_plan


_STREAM_CACHE = None


def _stream():
    """Raw hipStream_t of torch's current stream.  torch.cuda.current_stream() costs ~9 us of
    Python per call (15 calls per training step), so a step brackets its launches with
    pin_stream()/unpin_stream() and the handle is looked up once."""
    if _STREAM_CACHE is not None:
        return _STREAM_CACHE
    return torch.cuda.current_stream().cuda_stream


def pin_stream():
    global _STREAM_CACHE
    _STREAM_CACHE = torch.cuda.current_stream().cuda_stream


def unpin_stream():
    global _STREAM_CACHE
    _STREAM_CACHE = None


def _dev(t, dtype, name):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("%s must live in HBM (got a %s tensor): the SpMM/history path has no "
                           "CPU fallback" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    return t


def _ptr(t):
    return None if t is None else t.data_ptr()


def _rows2d(t, name):
    """(ptr, ld) of a 2-D fp32 tensor whose rows are contiguous (row pitch may exceed width)."""
    _dev(t, torch.float32, name)
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError("%s must be 2-D with unit column stride" % name)
    return t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))


def _hist2d(t, name):
    """(ptr, ld, bf16?) of a table that may be stored as bfloat16 -- a history (--history_dtype bf16) or the dense operand of
    a static-graph product (--full_batch_dtype bf16): fp32, or bfloat16 with ld in elements (the layout include/sgcn.h
    asks for is checked by the library)."""
    if t.dtype == torch.float32:
        return _rows2d(t, name) + (False,)
    if t.dtype != torch.bfloat16:
        raise TypeError("%s must be torch.float32 or torch.bfloat16, got %s" % (name, t.dtype))
    _dev(t, torch.bfloat16, name)
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError("%s must be 2-D with unit column stride" % name)
    return t.data_ptr(), t.stride(0), True


class DevArray(object):
    """A typed window ``base[off : off + n]`` of a 1-D device buffer that is NOT a tensor: the ops
    only need its address and length, and a torch slice costs ~2.5 us of host time -- a packed
    minibatch has ~25 such windows, i.e. a tenth of the launch-bound training step.  ``tensor()``
    materialises the view for the rare consumer that wants one."""
    __slots__ = ("base", "off", "n", "dtype", "_ptr")
    is_cuda = True

    def __init__(self, base, base_ptr, off, n):
        self.base, self.off, self.n, self.dtype = base, off, n, base.dtype
        self._ptr = base_ptr + 4 * off          # int32 / fp32 elements

    def data_ptr(self):
        return self._ptr

    @property
    def shape(self):
        return (self.n,)

    @property
    def device(self):
        return self.base.device

    def numel(self):
        return self.n

    def tensor(self):
        return self.base[self.off:self.off + self.n]


def as_tensor(x):
    return x.tensor() if isinstance(x, DevArray) else x


def _fixup_ws(ws, nslots, d, device):
    """The fix-up workspace of a plan with ``nslots`` partial-sum slots, grown to hold rows of width d (16-byte pitch)."""
    need = nslots * ((d + 3) // 4 * 4)
    if need and (ws is None or ws.numel() < need):
        ws = torch.empty(need, dtype=torch.float32, device=device)
    return ws


def _pitched_out(M, d, device, beta=0.0):
    """A fresh (M, d) fp32 result whose rows sit on a 16-byte pitch (what the sweep kernels store fastest)."""
    if beta != 0.0:
        raise ValueError("beta != 0 needs an existing `out`")
    return torch.empty((M, (d + 3) // 4 * 4), dtype=torch.float32, device=device)[:, :d]


class DevicePlan(object):
    """Device copy of a host work plan + its partial-sum workspace."""

    def __init__(self, seg, fix, nslots, device):
        self.nseg, self.nfix, self.nslots = int(seg.shape[0]), int(fix.shape[0]), int(nslots)
        self.seg = torch.from_numpy(seg).to(device, non_blocking=True)
        self.fix = torch.from_numpy(fix).to(device, non_blocking=True) if self.nfix else None
        self.ws = None
        self.device = device

    ws_ids = None         # (only spmax allocates it)

    def struct(self, d):
        self.ws = _fixup_ws(self.ws, self.nslots, d, self.device)
        return _ffi.Plan(self.seg.data_ptr(), self.nseg, _ptr(self.fix), self.nfix, self.nslots,
                         _ptr(self.ws), 0 if self.ws is None else self.ws.numel())

    def ids(self, d):
        """The int32 twin of the fix-up workspace (sgcn_spmax_csr_f32 dev_ws_arg: the slots' column ids), same geometry."""
        need = self.nslots * ((d + 3) // 4 * 4)
        if need and (self.ws_ids is None or self.ws_ids.numel() < need):
            self.ws_ids = torch.empty(need, dtype=torch.int32, device=self.device)
        return self.ws_ids


class DeviceCSR(object):
    """CSR matrix resident in HBM (int32 rowptr/col, fp32 val) + optional plan / transpose."""

    def __init__(self, shape, rowptr, col, val, plan=None, transpose=None, host_rowptr=None):
        self.shape = (int(shape[0]), int(shape[1]))
        self.rowptr, self.col, self.val = rowptr, col, val
        self.plan, self.transpose, self.host_rowptr = plan, transpose, host_rowptr

    @property
    def nnz(self):
        return int(self.col.shape[0])

    def product(self, x, out=None, add=None, add_rows=0):
        """out = A x (+ add on the first ``add_rows`` rows): what an aggregator calls on its adjacency object (a
        full_batch.StaticMatrix answers the same call with a static-graph kernel)."""
        return spmm(self, x, out=out, add=add, add_rows=add_rows)

    @staticmethod
    def from_arrays(shape, rowptr, col, val, device, plan_T=0, with_plan=True):
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float32)
        plan = None
        if with_plan:
            seg, fix, nslots = build_plan(rowptr, plan_T)
            plan = DevicePlan(seg, fix, nslots, device)
        return DeviceCSR(shape, torch.from_numpy(rowptr).to(device, non_blocking=True),
                         torch.from_numpy(col).to(device, non_blocking=True),
                         torch.from_numpy(val).to(device, non_blocking=True), plan,
                         host_rowptr=rowptr)

    @staticmethod
    def from_scipy(a, device, plan_T=0, with_plan=True, with_transpose=False):
        a = a.tocsr()
        m = DeviceCSR.from_arrays(a.shape, a.indptr, a.indices, a.data, device, plan_T, with_plan)
        if with_transpose:
            at = transpose_host(a)
            m.transpose = DeviceCSR.from_arrays(at.shape, at.indptr, at.indices, at.data, device,
                                                plan_T, with_plan)
        return m

    @staticmethod
    def from_host(h, device, plan_T=0, with_plan=True):
        """From a scheduler.HostCSR bundle (adds the transposed CSR when the sampler built it)."""
        m = DeviceCSR.from_arrays(h.shape, h.rowptr, h.col, h.val, device, plan_T, with_plan)
        if h.t_rowptr is not None:
            m.transpose = DeviceCSR.from_arrays((h.shape[1], h.shape[0]), h.t_rowptr, h.t_col,
                                                h.t_val, device, plan_T, with_plan)
        return m


def spmm(A, B, out=None, gidx=None, rscale=None, cscale=None, beta=0.0, d=None, add=None, add_rows=0):
    """out[M x d] = rscale (.) (A (cscale (.) B[gidx])) + beta * out   (sgcn_spmm_csr_f32);
    with ``add``: out[i] += add[i] for i < add_rows in the same launch (sgcn_spmm_csr_add_f32).  A bfloat16 ``B`` (a table
    of ``history_alloc(..., bf16=True)``'s layout) goes to sgcn_spmm_csr_b16 / _add_b16: half the operand's bytes, the bits
    of the fp32 product of the widened table; ``out`` stays fp32."""
    M, K = A.shape
    bptr, ldb, b16 = _hist2d(B, "B")
    d = int(B.shape[1] if d is None else d)
    if out is None:
        if beta != 0.0:
            raise ValueError("beta != 0 needs an existing `out`")
        out = torch.empty((M, d), dtype=torch.float32, device=B.device)
    cptr, ldc = _rows2d(out, "out")
    if out.shape[0] != M or out.shape[1] < d:
        raise ValueError("out has shape %s, need (%d, >=%d)" % (tuple(out.shape), M, d))
    rows_needed = K if gidx is None else None
    if rows_needed is not None and B.shape[0] < rows_needed:
        raise ValueError("B has %d rows, A has %d columns" % (B.shape[0], K))
    plan = A.plan.struct(d) if A.plan is not None else None
    if add is not None:
        aptr, ldadd = _rows2d(add, "add")
        check((lib.sgcn_spmm_csr_add_b16 if b16 else lib.sgcn_spmm_csr_add_f32)(
            A.rowptr.data_ptr(), _ptr(A.col), _ptr(A.val), M, K, d, bptr, ldb,
            _ptr(_dev(gidx, torch.int32, "gidx")), _ptr(_dev(rscale, torch.float32, "rscale")),
            _ptr(_dev(cscale, torch.float32, "cscale")), cptr, ldc, float(beta),
            C.byref(plan) if plan is not None else None, aptr, ldadd, int(add_rows), _stream()))
        return out
    check((lib.sgcn_spmm_csr_b16 if b16 else lib.sgcn_spmm_csr_f32)(
        A.rowptr.data_ptr(), _ptr(A.col), _ptr(A.val), M, K, d, bptr, ldb,
        _ptr(_dev(gidx, torch.int32, "gidx")), _ptr(_dev(rscale, torch.float32, "rscale")),
        _ptr(_dev(cscale, torch.float32, "cscale")), cptr, ldc, float(beta),
        C.byref(plan) if plan is not None else None, _stream()))
    return out


def check_unique_cols(A):
    """ValueError unless every row of the DeviceCSR ``A`` stores each column id at most once (what spmax's `first maximum`
    and its backward's `arg == j` mean something for).  A host pass over the pattern, made once per matrix."""
    if getattr(A, '_unique_cols', False):
        return
    col = A.col.cpu().numpy().astype(np.int64)
    rowptr = (A.host_rowptr if A.host_rowptr is not None else A.rowptr.cpu().numpy()).astype(np.int64)
    # one key per entry, (row, column) in row-major order: strictly rising as stored when every row is sorted and unique
    key = np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr)) * max(int(A.shape[1]), 1) + col
    if key.size > 1 and not np.all(np.diff(key) > 0):
        key.sort()                                        # (rows stored in another order: look for equal neighbours)
        if np.any(np.diff(key) == 0):
            raise ValueError("spmax needs unique column ids within each row: the %d x %d pattern stores a column twice "
                             "in some row" % A.shape)
    A._unique_cols = True


def spmax(A, x, out=None, want_arg=True, arg=None):
    """(out, arg): out[i, c] = max over the stored entries j of row i of the DeviceCSR ``A`` of x[j, c], arg[i, c] = the
    column id of the first maximum in stored order (int32; -1 and +0.0 on an empty row) -- sgcn_spmax_csr_f32.  The stored
    values are not read.  ``want_arg=False`` (an evaluation): arg is None, nothing is allocated for it; ``arg``: an existing
    (M, >= d) int32 tensor to store the ids into."""
    check_unique_cols(A)
    M, K = A.shape
    bptr, ldb = _rows2d(x, "x")
    d = int(x.shape[1])
    if x.shape[0] < K:
        raise ValueError("x has %d rows, A has %d columns" % (x.shape[0], K))
    if out is None:
        out = torch.empty((M, d), dtype=torch.float32, device=x.device)
    cptr, ldc = _rows2d(out, "out")
    if out.shape[0] != M or out.shape[1] < d:
        raise ValueError("out has shape %s, need (%d, >=%d)" % (tuple(out.shape), M, d))
    ldarg = d
    if not want_arg:
        arg = None
    elif arg is None:
        arg = torch.empty((M, d), dtype=torch.int32, device=x.device)
    else:
        _dev(arg, torch.int32, "arg")
        if arg.dim() != 2 or arg.shape[0] != M or arg.shape[1] < d or (arg.shape[1] > 1 and arg.stride(1) != 1):
            raise ValueError("arg has shape %s, need (%d, >=%d) with unit column stride" % (tuple(arg.shape), M, d))
        ldarg = arg.stride(0) if M > 1 else max(arg.stride(0), arg.shape[1])
    plan = A.plan.struct(d) if A.plan is not None else None
    ids = A.plan.ids(d) if A.plan is not None else None
    check(lib.sgcn_spmax_csr_f32(A.rowptr.data_ptr(), _ptr(A.col), M, K, d, bptr, ldb, cptr, ldc, _ptr(arg), ldarg,
                                 C.byref(plan) if plan is not None else None, _ptr(ids), _stream()))
    return out, arg


def spmax_bwd(At, g, arg, out=None, add=None, add_rows=0):
    """out[j, c] = sum over the rows i with arg[i, c] == j of g[i, c] in ascending i (+ add[j] for j < add_rows, in the same
    launch) -- sgcn_spmax_csr_bwd_f32, a gather over ``At``, the DeviceCSR of the TRANSPOSED pattern (ops.transpose_host:
    source rows ascending).  No atomics: bitwise reproducible."""
    K, M = At.shape
    gptr, ldg = _rows2d(g, "g")
    d = int(g.shape[1])
    _dev(arg, torch.int32, "arg")
    if arg.dim() != 2 or (arg.shape[1] > 1 and arg.stride(1) != 1) or tuple(arg.shape) != (M, d) or g.shape[0] != M:
        raise ValueError("g and arg must be (%d, d) with unit column stride, got %s and %s" % (M, tuple(g.shape), tuple(arg.shape)))
    ldarg = arg.stride(0) if M > 1 else max(arg.stride(0), d)
    if out is None:
        out = torch.empty((K, d), dtype=torch.float32, device=g.device)
    optr, ldo = _rows2d(out, "out")
    if out.shape[0] != K or out.shape[1] < d:
        raise ValueError("out has shape %s, need (%d, >=%d)" % (tuple(out.shape), K, d))
    aptr, ldadd = _rows2d(add, "add") if add is not None else (None, 0)
    plan = At.plan.struct(d) if At.plan is not None else None
    check(lib.sgcn_spmax_csr_bwd_f32(At.rowptr.data_ptr(), _ptr(At.col), K, M, d, gptr, ldg, arg.data_ptr(), ldarg, optr, ldo,
                                     aptr, ldadd, int(add_rows) if add is not None else 0,
                                     C.byref(plan) if plan is not None else None, _stream()))
    return out


ATTN_MAX_VECTORS = 256       # sgcn_spattn.hip: one lane group holds a whole row, 64 lanes x 4 vectors of VW elements


ATTN_HEADS = (1, 2, 4, 8)    # sgcn_spattn_mh_*: a head is an aligned power-of-two range of a group's lanes, the smallest group 8


def attn_vw(d, *tensors, heads=1):
    """The vector width sgcn_spattn_* would pick for width ``d`` and these 2-D operands (include/sgcn.h: the row kernels'
    rule): 4 with 16-byte aligned bases and pitches that are multiples of 4, 2 with 8-byte / multiples of 2, else 1.  The
    kernels hold d <= ATTN_MAX_VECTORS * VW columns.  ``heads`` > 1: a vector never straddles two heads, so the width
    must divide d / heads as well."""
    for vw in (4, 2):
        span = (d + vw - 1) // vw * vw
        ok = heads == 1 or (d // heads) % vw == 0
        for t in tensors:
            if t is None:
                continue
            ld = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])
            if ld % vw or ld < span or t.data_ptr() % (4 * vw):
                ok = False
                break
        if ok:
            return vw
    return 1


def _attn_out(rows, d, device, heads=1):
    """A fresh (rows, d) fp32 result of the attention kernels: contiguous, unless that pitch alone would narrow the vectors
    so far that d no longer fits one lane group -- then on a 16-byte pitch.  (With ``heads`` > 1 the head width d / heads
    caps the vectors as well, whatever the pitch.)"""
    dh = d // heads
    cap = 4 if heads == 1 or dh % 4 == 0 else 2 if dh % 2 == 0 else 1
    if d > ATTN_MAX_VECTORS * min(cap, 4 if d % 4 == 0 else 2 if d % 2 == 0 else 1):
        return _pitched_out(rows, d, device)
    return torch.empty((rows, d), dtype=torch.float32, device=device)


def _attn_heads(d, heads):
    heads = int(heads)
    if heads not in ATTN_HEADS:
        raise ValueError("heads must be one of %s, got %r" % ('/'.join(map(str, ATTN_HEADS)), heads))
    if d % heads:
        raise ValueError("the width %d is not a multiple of heads = %d" % (d, heads))
    return heads


def _attn_keep(keep):
    """``keep`` as a float in (0, 1] (1.0: no dropout on the coefficients)."""
    keep = float(keep)
    if not (0.0 < keep <= 1.0):               # (NaN too)
        raise ValueError("keep must be finite and in (0, 1], got %r" % (keep,))
    return keep


def attn_slot(kind, d, heads=1):
    """Floats per workspace slot of a split row in the attention launches -- the mirror of sgcn_attn_dev.h's fwd_slot, bwd_slot,
    kGatBwdUSlot and gat_bwd_v_slot, what ``DevicePlan.struct`` is sized with.  'fwd' (both score kinds): the row on a 16-byte
    pitch + one vector (m, l, -, -) per head; 'bwd' (dot-product bwd_q / bwd_kv): the row; 'gat_bwd_u': the heads' dU alone;
    'gat_bwd_v': the row + the heads' dV."""
    c4 = (d + 3) // 4 * 4
    return {'fwd': c4 + 4 * heads, 'bwd': c4, 'gat_bwd_u': 8, 'gat_bwd_v': c4 + 8}[kind]


def _attn_operands(A, x, heads, own, out=None, bwd=None, vector_lse=False):
    """The operand checks of spattn, spattn_bwd, spgat and spgat_bwd, in the order they have always run: ``x`` against the K
    columns of ``A`` and ``heads``; ``own(d, heads, (bptr, ldb))``, the caller's own operands (q; the score tables); then the
    forward's ``out`` (allocated when None) or, with ``bwd = (g, out_fwd, lse, add, add_rows)``, the backward's -- lse a
    vector of M floats under ``vector_lse`` at one head, else (M, heads).  Returns d, heads, x's (ptr, pitch), own's result
    and, forward: out, its (ptr, pitch); backward: g's and out_fwd's (ptr, pitch) and (aptr, ldadd, add_rows)."""
    M, K = A.shape
    b = _rows2d(x, "x")
    d = int(x.shape[1])
    heads = _attn_heads(d, heads)
    if x.shape[0] < K:
        raise ValueError("x has %d rows, A has %d columns" % (x.shape[0], K))
    mine = own(d, heads, b)
    if bwd is None:
        if out is None:
            out = _attn_out(M, d, x.device, heads)
        c = _rows2d(out, "out")
        if out.shape[0] != M or out.shape[1] < d:
            raise ValueError("out has shape %s, need (%d, >=%d)" % (tuple(out.shape), M, d))
        return d, heads, b, mine, out, c
    g, out_fwd, lse, add, add_rows = bwd
    gp = _rows2d(g, "g")
    c = _rows2d(out_fwd, "out_fwd")
    if tuple(g.shape) != (M, d) or out_fwd.shape[0] != M or out_fwd.shape[1] < d:
        raise ValueError("g and out_fwd must be (%d, %d), got %s and %s" % (M, d, tuple(g.shape), tuple(out_fwd.shape)))
    _dev(lse, torch.float32, "lse")
    if vector_lse and heads == 1:
        if lse.dim() != 1 or lse.shape[0] != M or not lse.is_contiguous():
            raise ValueError("lse must be a contiguous vector of %d floats" % M)
    elif tuple(lse.shape) != (M, heads) or not lse.is_contiguous():
        raise ValueError("lse must be a contiguous (%d, %d) table of floats" % (M, heads))
    a = _rows2d(add, "add") if add is not None else (None, 0)
    return d, heads, b, mine, gp, c, a + (int(add_rows) if add is not None else 0,)


def _attn_q(q, M, d):
    """(ptr, pitch) of an explicit query table: at least M rows of d floats"""
    qp = _rows2d(q, "q")
    if q.shape[0] < M or q.shape[1] != d:
        raise ValueError("q has shape %s, need (>=%d, %d)" % (tuple(q.shape), M, d))
    return qp


def _byref(plan):
    return C.byref(plan) if plan is not None else None


def spattn(A, x, q=None, scale=1.0, out=None, want_lse=True, heads=1, keep=1.0, key=0):
    """(out, lse): softmax dot-product attention over the stored pattern of the DeviceCSR ``A`` (M x K, unique column ids
    per row; stored values are not read) -- sgcn_spattn_drop_csr_f32.  With s_ij = scale * <q[i], x[j]> over the entries j of
    row i: lse[i] = log sum_j exp(s_ij), out[i] = sum_j exp(s_ij - lse[i]) x[j]; an empty row gives +0.0 and -inf.
    ``q=None`` means x[:M].  ``out`` may be a pitched (M, >= d) view.  ``want_lse=False`` (an evaluation): lse is None,
    nothing is allocated for it.  ``heads`` = H in 1/2/4/8: head h is the columns [h d/H, (h+1) d/H), every head an attention
    of its own over the same pattern, and lse is (M, H) for H > 1.  ``keep`` < 1: dropout on the coefficients -- entry (i, j)
    of head h stays, scaled by 1 / keep, where ``attn_kept(i, j, h, key, keep)``; the softmax and lse are those of keep = 1,
    and keep = 1 makes the library run the kernels without a mask, whatever ``key``."""
    check_unique_cols(A)
    keep = _attn_keep(keep)
    M, K = A.shape

    def queries(d, heads, b):
        if q is not None:
            return _attn_q(q, M, d)
        if x.shape[0] < M:
            raise ValueError("q=None takes x[:%d] as the queries, x has %d rows" % (M, x.shape[0]))
        return b
    d, heads, (bptr, ldb), (qptr, ldq), out, (cptr, ldc) = _attn_operands(A, x, heads, queries, out=out)
    lse = torch.empty((M,) if heads == 1 else (M, heads), dtype=torch.float32, device=x.device) if want_lse else None
    plan = A.plan.struct(attn_slot('fwd', d, heads)) if A.plan is not None else None
    check(lib.sgcn_spattn_drop_csr_f32(A.rowptr.data_ptr(), _ptr(A.col), M, K, d, heads, keep, int(key) & 0xFFFFFFFF, qptr, ldq,
                                       bptr, ldb, float(scale), cptr, ldc, _ptr(lse), _byref(plan), _stream()))
    return out, lse


def spattn_bwd(A, At, x, q, g, out_fwd, lse, scale, add=None, add_rows=0, heads=1, keep=1.0, key=0):
    """(dq, dx), the gradient of ``spattn(A, x, q, scale)`` for g = dL/dout, from the forward's ``out_fwd`` and ``lse`` --
    sgcn_spattn_drop_csr_bwd_q_f32 over ``A``, then sgcn_spattn_drop_csr_bwd_kv_f32 over ``At``, the DeviceCSR of the TRANSPOSED
    pattern (ops.transpose_host: source rows ascending).  Nothing nnz-sized is stored, no atomics: bitwise reproducible.
    With an explicit ``q``: dq (M x d, + add on its first ``add_rows`` rows) and dx = dB (K x d) separately.  With
    ``q=None`` (the queries are x[:M]): (None, dx) with dx = dB + [dQ + add ; 0] -- the first launch's result is the second
    one's addend, so the sum costs no extra pass.  ``heads`` as in ``spattn``, ``lse`` of the shape it returned.  ``keep`` and
    ``key``: the forward's (the launches recompute its mask; ``out_fwd`` is the masked output)."""
    keep = _attn_keep(keep)
    M, K = A.shape
    if tuple(At.shape) != (K, M):
        raise ValueError("At has shape %s, the transpose of %s is needed" % (tuple(At.shape), tuple(A.shape)))

    def queries(d, heads, b):
        if q is not None:
            return _attn_q(q, M, d)
        if x.shape[0] < M or K < M:
            raise ValueError("q=None takes x[:%d] as the queries, x has %d rows and A %d columns" % (M, x.shape[0], K))
        return b
    d, heads, (bptr, ldb), (qptr, ldq), (gptr, ldg), (cptr, ldc), (aptr, ldadd, add_rows) = _attn_operands(
        A, x, heads, queries, bwd=(g, out_fwd, lse, add, add_rows), vector_lse=True)
    delta = torch.empty((M * heads,), dtype=torch.float32, device=x.device)
    dq = _attn_out(M, d, x.device, heads)
    plan = A.plan.struct(attn_slot('bwd', d)) if A.plan is not None else None
    fused = q is None
    key = int(key) & 0xFFFFFFFF
    check(lib.sgcn_spattn_drop_csr_bwd_q_f32(A.rowptr.data_ptr(), _ptr(A.col), M, K, d, heads, keep, key, qptr, ldq, bptr, ldb,
                                             float(scale), gptr, ldg, cptr, ldc, lse.data_ptr(), delta.data_ptr(),
                                             dq.data_ptr(), _rows2d(dq, "dq")[1], aptr, ldadd, add_rows, _byref(plan), _stream()))
    dx = _spattn_bwd_kv(At, d, heads, keep, key, (qptr, ldq), (bptr, ldb), scale, (gptr, ldg), lse, delta, x.device,
                        dq if fused else None)
    return (None if fused else dq), dx


def _spattn_bwd_kv(At, d, heads, keep, key, q, b, scale, g, lse, delta, device, dq):
    """dx (K x d): the keys' / values' half of the attention backward -- sgcn_spattn_drop_csr_bwd_kv_f32 over ``At`` (K x M, the
    TRANSPOSED pattern) with the (ptr, pitch) pairs ``q``, ``b``, ``g`` and the rows' ``lse`` and ``delta``; ``dq`` (M x d, or
    None) is added to its first M rows in the launch's epilogue.  The second half of ``spattn_bwd``, and of
    ``full_batch.PulledMatrix.pull_attn_backward``, whose lse and delta come from the two-table launches."""
    K, M = At.shape
    dx = _attn_out(K, d, device, heads)
    tplan = At.plan.struct(attn_slot('bwd', d)) if At.plan is not None else None
    fused = dq is not None
    check(lib.sgcn_spattn_drop_csr_bwd_kv_f32(At.rowptr.data_ptr(), _ptr(At.col), K, M, d, heads, keep, key, q[0], q[1], b[0],
                                              b[1], float(scale), g[0], g[1], lse.data_ptr(), delta.data_ptr(), dx.data_ptr(),
                                              _rows2d(dx, "dx")[1], dq.data_ptr() if fused else None,
                                              _rows2d(dq, "dq")[1] if fused else 0, M if fused else 0, _byref(tplan), _stream()))
    return dx


GAT_RED_ROWS = 64            # sgcn_gat_scores_bwd_f32: rows per partial sum of da


def _attn_slope(slope):
    """``slope`` as a float in [0, 1] (the LeakyReLU of the learned scores)."""
    slope = float(slope)
    if not (0.0 <= slope <= 1.0):             # (NaN too)
        raise ValueError("slope must lie in [0, 1], got %r" % (slope,))
    return slope


def _gat_vec(a, d):
    _dev(a, torch.float32, "a")
    if tuple(a.shape) != (2, d) or not a.is_contiguous():
        raise ValueError("a must be a contiguous (2, %d) table of floats, got %s" % (d, tuple(a.shape)))
    return a


def _gat_table(t, rows, heads, name):
    """(ptr, pitch) of a score table: at least ``rows`` rows of ``heads`` floats"""
    ptr, ld = _rows2d(t, name)
    if t.shape[0] < rows or t.shape[1] != heads:
        raise ValueError("%s has shape %s, need (>=%d, %d)" % (name, tuple(t.shape), rows, heads))
    return ptr, ld


def gat_scores(x, a, heads=1):
    """S (rows, 2 H): S[r, h] = u_r^h = sum_{c in head h} x[r, c] a[0, c] and S[r, H + h] = v_r^h with a[1] -- the learned
    additive scores' two per-vertex scalars (sgcn_gat_scores_f32; one pass over x, a fixed summation order).  ``S[:, :H]`` and
    ``S[:, H:]`` are the tables U and V of ``spgat``."""
    xptr, ldx = _rows2d(x, "x")
    d = int(x.shape[1])
    heads = _attn_heads(d, heads)
    _gat_vec(a, d)
    rows = int(x.shape[0])
    S = torch.empty((rows, 2 * heads), dtype=torch.float32, device=x.device)
    check(lib.sgcn_gat_scores_f32(xptr, ldx, rows, d, heads, a.data_ptr(), S.data_ptr(), _stream()))
    return S


def spgat(A, x, u, v, slope=0.2, out=None, want_lse=True, heads=1, keep=1.0, key=0):
    """(out, lse): attention with learned additive scores over the stored pattern of the DeviceCSR ``A`` (M x K, unique column
    ids per row) -- sgcn_spgat_csr_f32.  With z_ij = u[i] + v[j] per head and s_ij = z_ij > 0 ? z_ij : slope z_ij:
    lse[i] = log sum_j exp(s_ij), out[i] = sum_j exp(s_ij - lse[i]) x[j]; an empty row gives +0.0 and -inf.  ``u`` (>= M, H)
    and ``v`` (>= K, H) are score tables (views of ``gat_scores``' result serve).  lse is always (M, H).  ``out``, ``want_lse``,
    ``heads``, ``keep`` and ``key`` as in ``spattn``."""
    check_unique_cols(A)
    keep = _attn_keep(keep)
    slope = _attn_slope(slope)
    M, K = A.shape
    d, heads, (bptr, ldb), (uptr, ldu, vptr, ldv), out, (cptr, ldc) = _attn_operands(
        A, x, heads, lambda d, heads, b: _gat_table(u, M, heads, "u") + _gat_table(v, K, heads, "v"), out=out)
    lse = torch.empty((M, heads), dtype=torch.float32, device=x.device) if want_lse else None
    plan = A.plan.struct(attn_slot('fwd', d, heads)) if A.plan is not None else None
    check(lib.sgcn_spgat_csr_f32(A.rowptr.data_ptr(), _ptr(A.col), M, K, d, heads, keep, int(key) & 0xFFFFFFFF, uptr, ldu, vptr,
                                 ldv, bptr, ldb, slope, cptr, ldc, _ptr(lse), _byref(plan), _stream()))
    return out, lse


def spgat_bwd(A, At, x, u, v, g, out_fwd, lse, slope=0.2, add=None, add_rows=0, heads=1, keep=1.0, key=0):
    """(dB, dU, dV, delta), the gradient of ``spgat`` for g = dL/dout from the forward's ``out_fwd`` and ``lse`` --
    sgcn_spgat_csr_bwd_u_f32 over ``A``, then sgcn_spgat_csr_bwd_v_f32 over ``At`` (the TRANSPOSED pattern, source rows
    ascending).  dB (K x d, + add on its first ``add_rows`` rows) is the gradient with respect to ``x`` as the VALUES; dU
    (M, H) and dV (K, H) those of the score tables, which ``gat_scores_bwd`` takes on to x and a.  Nothing nnz-sized is
    stored, no atomics: bitwise reproducible."""
    keep = _attn_keep(keep)
    slope = _attn_slope(slope)
    M, K = A.shape
    if tuple(At.shape) != (K, M):
        raise ValueError("At has shape %s, the transpose of %s is needed" % (tuple(At.shape), tuple(A.shape)))
    d, heads, (bptr, ldb), (uptr, ldu, vptr, ldv), (gptr, ldg), (cptr, ldc), (aptr, ldadd, add_rows) = _attn_operands(
        A, x, heads, lambda d, heads, b: _gat_table(u, M, heads, "u") + _gat_table(v, K, heads, "v"),
        bwd=(g, out_fwd, lse, add, add_rows))
    delta = torch.empty((M, heads), dtype=torch.float32, device=x.device)
    dU = torch.empty((M, heads), dtype=torch.float32, device=x.device)
    dV = torch.empty((K, heads), dtype=torch.float32, device=x.device)
    dB = _attn_out(K, d, x.device, heads)
    plan = A.plan.struct(attn_slot('gat_bwd_u', d)) if A.plan is not None else None
    key = int(key) & 0xFFFFFFFF
    check(lib.sgcn_spgat_csr_bwd_u_f32(A.rowptr.data_ptr(), _ptr(A.col), M, K, d, heads, keep, key, uptr, ldu, vptr, ldv, bptr,
                                       ldb, slope, gptr, ldg, cptr, ldc, lse.data_ptr(), delta.data_ptr(), dU.data_ptr(),
                                       _byref(plan), _stream()))
    tplan = At.plan.struct(attn_slot('gat_bwd_v', d)) if At.plan is not None else None
    check(lib.sgcn_spgat_csr_bwd_v_f32(At.rowptr.data_ptr(), _ptr(At.col), K, M, d, heads, keep, key, uptr, ldu, vptr, ldv, bptr,
                                       ldb, slope, gptr, ldg, lse.data_ptr(), delta.data_ptr(), dB.data_ptr(),
                                       _rows2d(dB, "dB")[1], dV.data_ptr(), aptr, ldadd, add_rows, _byref(tplan), _stream()))
    return dB, dU, dV, delta


def gat_scores_bwd(x, a, dU, dV, dx=None, heads=1):
    """da (2, d): da[0, c] = sum_r dU[r, h(c)] x[r, c] over the rows of ``dU`` and da[1, c] = sum_r dV[r, h(c)] x[r, c] over
    those of ``dV`` (= the first rows of ``x``; dU may have fewer) -- sgcn_gat_scores_bwd_f32, a two-stage reduction whose
    partition depends on the row count alone.  With ``dx`` (rows x d, pitched or not) the launch also ADDS the scores' share of
    the input gradient into it: dx[r, c] += dU[r, h(c)] a[0, c] + dV[r, h(c)] a[1, c]; ``dx=None`` writes nothing but da."""
    xptr, ldx = _rows2d(x, "x")
    d = int(x.shape[1])
    heads = _attn_heads(d, heads)
    _gat_vec(a, d)
    for t, name in ((dU, "dU"), (dV, "dV")):
        _dev(t, torch.float32, name)
        if t.dim() != 2 or t.shape[1] != heads or not t.is_contiguous():
            raise ValueError("%s must be a contiguous (rows, %d) table of floats, got %s" % (name, heads, tuple(t.shape)))
    rows, rows_u = int(dV.shape[0]), int(dU.shape[0])
    if rows_u > rows or x.shape[0] < rows:
        raise ValueError("dU has %d rows, dV %d, x %d: need rows(dU) <= rows(dV) <= rows(x)" % (rows_u, rows, x.shape[0]))
    dxptr, lddx = (None, 0)
    if dx is not None:
        dxptr, lddx = _rows2d(dx, "dx")
        if dx.shape[0] < rows or dx.shape[1] != d:
            raise ValueError("dx has shape %s, need (>=%d, %d)" % (tuple(dx.shape), rows, d))
    da = torch.empty((2, d), dtype=torch.float32, device=x.device)
    nws = (rows + GAT_RED_ROWS - 1) // GAT_RED_ROWS * 2 * d
    ws = torch.empty(max(nws, 1), dtype=torch.float32, device=x.device)
    check(lib.sgcn_gat_scores_bwd_f32(xptr, ldx, rows, rows_u, d, heads, a.data_ptr(), dU.data_ptr(), dV.data_ptr(), dxptr, lddx,
                                      da.data_ptr(), ws.data_ptr(), nws, _stream()))
    return da


def vr_aggregate(A, P, h, mu, Hbar, ifield, ffield, s, cvd, concat_self, out_h=None, out_mu=None):
    """Fused control-variate aggregator forward (sgcn_vr_aggregate_f32; sgcn_vr_aggregate_h16 on a bfloat16 history)."""
    n1, n0 = A.shape
    nf = P.shape[1]
    hptr, ldx = _rows2d(h, "h")
    d = int(h.shape[1])
    width = 2 * d if concat_self else d
    if cvd:
        mptr, ldm = _rows2d(mu, "mu")
        if ldm != ldx or tuple(mu.shape) != tuple(h.shape):
            raise ValueError("h and mu must share shape and row pitch")
    else:
        mptr = None
    Hptr, ldh, h16 = _hist2d(Hbar, "Hbar")
    if out_h is None:
        out_h = torch.empty((n1, width), dtype=torch.float32, device=h.device)
    if cvd and out_mu is None:
        out_mu = torch.empty((n1, width), dtype=torch.float32, device=h.device)
    ohp, ldo = _rows2d(out_h, "out_h")
    omp = None
    if cvd:
        omp, ldo2 = _rows2d(out_mu, "out_mu")
        if ldo2 != ldo:
            raise ValueError("out_h and out_mu must share row pitch")
    plan = P.plan.struct(d) if P.plan is not None else None
    check((lib.sgcn_vr_aggregate_h16 if h16 else lib.sgcn_vr_aggregate_f32)(
        A.rowptr.data_ptr(), _ptr(A.col), _ptr(A.val), P.rowptr.data_ptr(), _ptr(P.col),
        _ptr(P.val), n1, n0, nf, d, hptr, mptr, ldx, Hptr, ldh,
        _ptr(_dev(ifield, torch.int32, "ifield")), _ptr(_dev(ffield, torch.int32, "ffield")),
        _ptr(_dev(s, torch.float32, "s")), ohp, omp, ldo, int(bool(cvd)), int(bool(concat_self)),
        C.byref(plan) if plan is not None else None, _stream()))
    return out_h, out_mu


def vr_aggregate_two_phase(A, P, h, mu, Hbar, ifield, ffield, s, cvd, concat_self, stream_pre=None):
    """The same aggregate as ``vr_aggregate`` through sgcn_vr_aggregate_pre_f32 + _post_f32 (what the step
    program issues, the first phase beside the dense layers): bit-identical to the fused call."""
    n1, n0 = A.shape
    nf = P.shape[1]
    hptr, ldx = _rows2d(h, "h")
    d = int(h.shape[1])
    width = 2 * d if concat_self else d
    Hptr, ldh, h16 = _hist2d(Hbar, "Hbar")
    ldw = (d + 3) // 4 * 4
    accP = torch.empty((n1, ldw), dtype=torch.float32, device=h.device)
    plan = P.plan.struct(d) if P.plan is not None else None
    check((lib.sgcn_vr_aggregate_pre_h16 if h16 else lib.sgcn_vr_aggregate_pre_f32)(P.rowptr.data_ptr(), _ptr(P.col), _ptr(P.val), n1, nf, d, Hptr, ldh,
                                        _ptr(_dev(ffield, torch.int32, "ffield")), accP.data_ptr(),
                                        C.byref(plan) if plan is not None else None, _stream()))
    out_h = torch.empty((n1, width), dtype=torch.float32, device=h.device)
    out_mu = torch.empty((n1, width), dtype=torch.float32, device=h.device) if cvd else None
    check((lib.sgcn_vr_aggregate_post_h16 if h16 else lib.sgcn_vr_aggregate_post_f32)(A.rowptr.data_ptr(), _ptr(A.col), _ptr(A.val), n1, n0, d, hptr,
                                         _rows2d(mu, "mu")[0] if cvd else None, ldx, Hptr, ldh,
                                         _ptr(_dev(ifield, torch.int32, "ifield")), _ptr(_dev(s, torch.float32, "s")),
                                         out_h.data_ptr(), _ptr(out_mu), width, int(bool(cvd)), int(bool(concat_self)),
                                         accP.data_ptr(), _stream()))
    return out_h, out_mu


def gather_rows(inp, idx, out=None, d=None):
    """out[i, :d] = inp[idx[i], :d]   (sgcn_gather_rows_f32).  A bfloat16 ``inp`` (a history table) is widened on the way
    out (sgcn_gather_rows_h16); there ``idx=None`` reads rows 0 .. n-1."""
    iptr, ldi, h16 = _hist2d(inp, "inp")
    if idx is None and not h16:
        raise TypeError("gather_rows: idx=None is for a bfloat16 table")
    _dev(idx, torch.int32, "idx")
    n = int(inp.shape[0] if idx is None else idx.shape[0])
    d = int(inp.shape[1] if d is None else d)
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=inp.device)
    optr, ldo = _rows2d(out, "out")
    check((lib.sgcn_gather_rows_h16 if h16 else lib.sgcn_gather_rows_f32)(iptr, ldi, _ptr(idx), n, d, optr, ldo, _stream()))
    return out


def scatter_rows(H, idx, src, d=None):
    """H[idx[i], :d] = src[i, :d]  (idx unique)   (sgcn_scatter_rows_f32).  A bfloat16 ``H`` (a history table) takes the
    fp32 rows rounded to nearest even (sgcn_scatter_rows_h16); there ``idx=None`` writes rows 0 .. n-1."""
    hptr, ldh, h16 = _hist2d(H, "H")
    if idx is None and not h16:
        raise TypeError("scatter_rows: idx=None is for a bfloat16 table")
    sptr, lds = _rows2d(src, "src")
    _dev(idx, torch.int32, "idx")
    n = int(src.shape[0] if idx is None else idx.shape[0])
    d = int(src.shape[1] if d is None else d)
    check((lib.sgcn_scatter_rows_h16 if h16 else lib.sgcn_scatter_rows_f32)(hptr, ldh, _ptr(idx), n, d, sptr, lds, _stream()))
    return H


def history_alloc(n, d, device, bf16=False):
    """A zeroed ``n x d`` history table.  bfloat16: ``n x pitch`` with pitch = 8 * ceil(d / 8) elements, handed out as its
    ``[:, :d]`` view -- the layout the *_h16 entry points require; the pad columns stay zero."""
    if not bf16:
        return torch.zeros((n, d), dtype=torch.float32, device=device)
    return torch.zeros((n, (d + 7) // 8 * 8), dtype=torch.bfloat16, device=device)[:, :d]


def history_widen(H, out=None):
    """The whole table as fp32 (a copy): exact for a bfloat16 table."""
    if H.dtype == torch.float32:
        return H.clone() if out is None else out.copy_(H)
    return gather_rows(H, None, out=out)


def history_assign(H, src):
    """H[:, :] = src (fp32, same shape), rounded when H is bfloat16."""
    if H.dtype == torch.float32:
        H.copy_(src)
        return H
    if src.shape[0] > 1 and (src.stride(1) != 1):
        src = src.contiguous()
    return scatter_rows(H, None, src)


def operand_round(x, out=None):
    """``x`` (fp32 rows) rounded to nearest even into a bfloat16 operand table for ``spmm`` / ``spmm_cs``
    (sgcn_scatter_rows_h16 with no index: the one rounding kernel).  ``out``: a table of ``history_alloc(n, d, device,
    bf16=True)`` to reuse."""
    if out is None:
        out = history_alloc(int(x.shape[0]), int(x.shape[1]), x.device, bf16=True)
    if tuple(out.shape) != tuple(x.shape):
        raise ValueError("operand_round: out has shape %s, x %s" % (tuple(out.shape), tuple(x.shape)))
    return history_assign(out, x)


def csr_slice(A, rows_host, rows_dev=None, with_coo_rows=False):
    """CSR row slice A[rows] -> DeviceCSR   (sgcn_csr_slice_indptr + sgcn_csr_slice_f32).

    ``A.host_rowptr`` (kept by DeviceCSR.from_*) feeds the host prefix pass, mirroring the
    reference's two-phase c_indptr / c_slice (gcn/history.cpp:50-72)."""
    if A.host_rowptr is None:
        raise ValueError("csr_slice needs A.host_rowptr")
    rows_host = np.ascontiguousarray(rows_host, dtype=np.int32)
    n = int(rows_host.shape[0])
    o_p = np.empty(n + 1, dtype=np.int32)
    check(lib.sgcn_csr_slice_indptr(n, rows_host.ctypes.data, A.host_rowptr.ctypes.data,
                                    o_p.ctypes.data))
    nnz = int(o_p[n])
    dev = A.val.device
    if rows_dev is None:
        rows_dev = torch.from_numpy(rows_host).to(dev, non_blocking=True)
    o_p_dev = torch.from_numpy(o_p).to(dev, non_blocking=True)
    o_d = torch.empty(nnz, dtype=torch.float32, device=dev)
    o_c = torch.empty(nnz, dtype=torch.int32, device=dev)
    o_r = torch.empty(nnz, dtype=torch.int32, device=dev) if with_coo_rows else None
    check(lib.sgcn_csr_slice_f32(n, rows_dev.data_ptr(), A.val.data_ptr(), A.col.data_ptr(),
                                 A.rowptr.data_ptr(), o_p_dev.data_ptr(), o_d.data_ptr(),
                                 o_c.data_ptr(), _ptr(o_r), _stream()))
    out = DeviceCSR((n, A.shape[1]), o_p_dev, o_c, o_d, host_rowptr=o_p)
    out.coo_rows = o_r
    return out


# ---- fused dense-side kernels (sgcn_dense.hip) ---------------------------------------------------
def ln_act_fwd(x, offset, scale, relu, eps=1e-9):
    """y = act(LN(x)*scale + offset) (norm skipped when offset/scale are None).
    Returns (y, ctx) with ctx = (xhat, rstd) or None."""
    xp, ldx = _rows2d(x, "x")
    n, d = int(x.shape[0]), int(x.shape[1])
    y = torch.empty((n, d), dtype=torch.float32, device=x.device)
    norm = offset is not None
    xhat = torch.empty((n, d), dtype=torch.float32, device=x.device) if norm else None
    rstd = torch.empty((n,), dtype=torch.float32, device=x.device) if norm else None
    check(lib.sgcn_ln_act_fwd_f32(xp, ldx, _ptr(offset), _ptr(scale), n, d, float(eps), int(bool(relu)),
                                  y.data_ptr(), d, _ptr(xhat), _ptr(rstd), _stream()))
    return y, ((xhat, rstd) if norm else None)


def ln_act_bwd(dy, y, ctx, scale, relu, doffset=None, dscale=None):
    """dx of ln_act_fwd; accumulates the LN parameter gradients into doffset/dscale."""
    gp, ldg = _rows2d(dy, "dy")
    yp, ldy = _rows2d(y, "y")
    n, d = int(dy.shape[0]), int(dy.shape[1])
    dx = torch.empty((n, d), dtype=torch.float32, device=dy.device)
    norm = ctx is not None
    ws = _gemm_ws(int(lib.sgcn_ln_act_bwd_ws_floats(n, d)), dy.device) if norm else None   # shared scratch
    check(lib.sgcn_ln_act_bwd_f32(gp, ldg, yp, ldy, _ptr(ctx[0]) if norm else None,
                                  _ptr(ctx[1]) if norm else None, _ptr(scale) if norm else None, n, d,
                                  int(bool(relu)), dx.data_ptr(), d, _ptr(doffset), _ptr(dscale),
                                  _ptr(ws), _stream()))
    return dx


def check_loss_rows(rows, N):
    """The host check of a loss subset (the device trusts it): int32 ids in [0, N), ascending and unique."""
    r = np.asarray(rows)
    if r.ndim != 1 or r.size == 0 or not np.issubdtype(r.dtype, np.integer):
        raise ValueError("loss rows must be a non-empty 1-D integer array")
    if int(r[0]) < 0 or int(r[-1]) >= N or (r.size > 1 and not bool(np.all(r[1:] > r[:-1]))):
        raise ValueError("loss rows must be ascending, unique and in [0, %d)" % N)
    return np.ascontiguousarray(r, dtype=np.int32)


def _ce(fn, fn_rows, planes, logits, labels, want_grad, want_pred, rows):
    zp, ldz = _rows2d(logits, "logits")
    lp, ldl = _rows2d(labels, "labels")
    N, c = int(logits.shape[0]), int(logits.shape[1])
    if rows is not None:
        if not isinstance(rows, torch.Tensor):       # host ids: checked here, then uploaded
            rows = torch.from_numpy(check_loss_rows(rows, N)).to(logits.device)
        _dev(rows, torch.int32, "rows")
        if labels.shape[0] != N:
            raise ValueError("with rows, labels is the table of all %d rows (got %d)" % (N, labels.shape[0]))
    n = N if rows is None else int(rows.shape[0])
    # [stats | per-row scratch | with pred: the rows' classes, argmax(pred) + 4096 * argmax(labels)]
    stats = torch.empty(4 + planes * n, dtype=torch.float32, device=logits.device)
    dz = torch.empty((N, c), dtype=torch.float32, device=logits.device) if want_grad else None
    pred = torch.empty((n, c), dtype=torch.float32, device=logits.device) if want_pred else None
    if rows is None:
        check(fn(zp, ldz, lp, ldl, n, c, _ptr(dz), c, _ptr(pred), c, stats.data_ptr(), stats.data_ptr() + 16, _stream()))
    else:
        check(fn_rows(zp, ldz, lp, ldl, N, c, rows.data_ptr(), n, _ptr(dz), c, _ptr(pred), c, stats.data_ptr(),
                      stats.data_ptr() + 16, _stream()))
    return stats, dz, pred


def softmax_ce(logits, labels, want_grad=True, want_pred=False, rows=None):
    """(stats[4] = {sum CE, #correct, mean CE, accuracy}, dlogits or None, pred or None)
    (sgcn_softmax_ce_f32).  ``rows``: the loss over that subset of the rows of N-row tables -- dlogits covers all N rows,
    +0.0 off the subset; pred and the per-row scratch are compact, in subset order (sgcn_softmax_ce_rows_f32).  Host ids
    (a NumPy array or list) are checked by check_loss_rows -- ascending, unique, in [0, N) -- and uploaded.  An int32
    DEVICE tensor is trusted, because reading it back would cost a synchronisation per call: its ids MUST have passed
    check_loss_rows (StaticBatch does that), an id >= N is an out-of-bounds access on the device."""
    return _ce(lib.sgcn_softmax_ce_f32, lib.sgcn_softmax_ce_rows_f32, 3 if want_pred else 2, logits, labels,
               want_grad, want_pred, rows)


def sigmoid_ce(logits, labels, want_grad=True, want_pred=False, rows=None):
    """Multitask (ppi) loss: (stats[4] = {sum CE, #correct elements, mean CE, element accuracy}, dlogits
    or None, pred = sigmoid(logits) or None)   (sgcn_sigmoid_ce_f32; with ``rows`` as softmax_ce:
    sgcn_sigmoid_ce_rows_f32)."""
    return _ce(lib.sgcn_sigmoid_ce_f32, lib.sgcn_sigmoid_ce_rows_f32, 2, logits, labels, want_grad, want_pred, rows)


def l2_penalty(theta, lo, hi, wd, grad=None, loss=None):
    """Weight decay over the flat-buffer range [lo, hi): grad += wd * theta, loss[0] += 0.5 * wd * |theta|^2
    (either may be None)   (sgcn_l2_penalty_f32)."""
    _dev(theta, torch.float32, "theta")
    check(lib.sgcn_l2_penalty_f32(theta.data_ptr(), int(lo), int(hi), float(wd), _ptr(grad), _ptr(loss), _stream()))


def csr_transpose_index(A):
    """(t_rowptr, t_row, t_src) of a row-sliced DeviceCSR with ``coo_rows`` (sgcn_csr_transpose_index):
    the structure of A^T, rows ascending inside every column, + the source position of each entry."""
    if getattr(A, "coo_rows", None) is None:
        raise ValueError("csr_transpose_index needs the COO row ids (csr_slice(..., with_coo_rows=True))")
    dev = A.col.device
    ncols, nnz = int(A.shape[1]), int(A.col.shape[0])
    t_rowptr = torch.empty(ncols + 1, dtype=torch.int32, device=dev)
    t_row = torch.empty(nnz, dtype=torch.int32, device=dev)
    t_src = torch.empty(nnz, dtype=torch.int32, device=dev)
    need = int(lib.sgcn_csr_transpose_ws_ints(ncols, nnz))
    ws = torch.empty(max(need, 1), dtype=torch.int32, device=dev)
    check(lib.sgcn_csr_transpose_index(ncols, nnz, _ptr(A.col), _ptr(A.coo_rows), t_rowptr.data_ptr(),
                                       t_row.data_ptr(), t_src.data_ptr(), ws.data_ptr(), _stream()))
    return t_rowptr, t_row, t_src


def gather_f32(src, idx):
    """out[i] = src[idx[i]]   (sgcn_gather_f32)."""
    _dev(src, torch.float32, "src")
    _dev(idx, torch.int32, "idx")
    out = torch.empty(idx.shape[0], dtype=torch.float32, device=src.device)
    check(lib.sgcn_gather_f32(src.data_ptr(), idx.data_ptr(), int(idx.shape[0]), out.data_ptr(), _stream()))
    return out


# ---- the induced subgraph A[S, S] of a resident CSR (sgcn_induce.hip; --full_batch_parts) -----------------------------------
INDUCE_NORMS = ('keep', 'rows')


def check_induce_ids(ids, N):
    """The host check of a vertex subset (the device trusts it): int32 ids in [0, N), ascending and unique."""
    r = np.asarray(ids)
    if r.ndim != 1 or r.size == 0 or not np.issubdtype(r.dtype, np.integer):
        raise ValueError("the vertices of an induced subgraph must be a non-empty 1-D integer array")
    if int(r[0]) < 0 or int(r[-1]) >= N or (r.size > 1 and not bool(np.all(r[1:] > r[:-1]))):
        raise ValueError("the vertices of an induced subgraph must be ascending, unique and in [0, %d)" % N)
    return np.ascontiguousarray(r, dtype=np.int32)


class _InduceBuffers(object):
    """What csr_induce writes, kept with the resident matrix and reused by every step: the vertex map (N words), the
    per-row arrays (grown to the largest subset seen), the per-entry arrays of the block and of its transpose (grown to the
    largest bound seen), the transposition's workspace, and one pinned host buffer for the two row pointers."""

    def __init__(self, N, device):
        self.device, self.rows, self.entries, self.ws_ints = device, -1, -1, -1
        self.map = torch.empty(max(N, 1), dtype=torch.int32, device=device)

    def fit(self, n, bound, transposition=True):
        dev = self.device
        if n > self.rows:
            self.rows = n
            # (n + 2 words each: the transposition runs over n + 1 columns, the pad column last)
            self.rowptr, self.t_rowptr = (torch.empty(n + 2, dtype=torch.int32, device=dev) for _ in range(2))
            self.full, self.kept, self.rscale = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
            self.host = torch.empty(2 * (n + 1), dtype=torch.int32).pin_memory()
        if bound > self.entries:
            self.entries = bound
            e = max(bound, 1)
            self.col, self.coo, self.t_row, self.t_src = (torch.empty(e, dtype=torch.int32, device=dev) for _ in range(4))
            self.val, self.t_val = (torch.empty(e, dtype=torch.float32, device=dev) for _ in range(2))
        need = int(lib.sgcn_csr_transpose_ws_ints(n + 1, bound)) if transposition else 0
        if need > self.ws_ints:
            self.ws_ints = need
            self.ws = torch.empty(max(need, 1), dtype=torch.int32, device=dev)


def csr_induce(A, ids_host, ids_dev=None, norm='keep', plan_T=0):
    """The induced subgraph A[ids][:, ids] of the resident square DeviceCSR ``A`` as a DeviceCSR with ``.transpose`` set (and
    ``.coo_rows``), cut on the device: sgcn_induce_map_i32, sgcn_csr_induce_count, sgcn_csr_induce_fill, then the stable
    transposition of the block (sgcn_csr_transpose_index on its COO rows, the values following through sgcn_gather_f32).
    Where ``A.transpose`` is resident (DeviceCSR.from_scipy(..., with_transpose=True): rows sorted), the transposed block is
    instead the same cut of that matrix -- two more launches of the induce kernels, an entry scaled by its column's factor --
    which is the stable transpose with the block's own value bits at a thousandth of the transposition's time on a block of
    29,000 columns (profiles/full_batch_parts.jsonl); the trainer keeps the transpose resident for that reason.

    ``ids_host``: ascending, unique, in [0, N) (checked here); ``ids_dev``: the same ids on the device, uploaded if not given.
    ``norm``: 'keep' -- the stored values; with sorted, duplicate-free rows the block then has the row pointer, column ids
    and value bits of SciPy's A[ids][:, ids].  'rows' -- row i is scaled by full_i / kept_i, the sums of its values over
    all its entries and over the kept ones (1 where kept_i == 0), so that a row keeps its value sum: what a row-normalised
    adjacency needs to stay one after inter-part edges are dropped.

    Everything is launched before the host learns the block's size: the per-entry buffers hold ``bound`` elements, the
    selected rows' stored entries (from A.host_rowptr), and fill pads the unused tail with a column behind the last one, which
    the stable transposition sorts behind every real entry.  Both row pointers then reach the host through one pinned buffer
    and ONE synchronisation, and the segment plans come from scheduler.build_plan(rowptr, plan_T) -- the call, with the same
    T, that DeviceCSR.from_scipy makes.  The buffers belong to ``A`` and are reused: a block is valid until the next call."""
    if A.host_rowptr is None:
        raise ValueError("csr_induce needs A.host_rowptr")
    if A.shape[0] != A.shape[1]:
        raise ValueError("csr_induce needs a square (vertex x vertex) matrix")
    if norm not in INDUCE_NORMS:
        raise ValueError("norm must be one of %s, got %r" % ('/'.join(INDUCE_NORMS), norm))
    N, dev = int(A.shape[0]), A.val.device
    ids_host = check_induce_ids(ids_host, N)
    n = int(ids_host.shape[0])
    hp, At = A.host_rowptr, A.transpose
    bound = int((hp[ids_host + 1].astype(np.int64) - hp[ids_host]).sum())
    if At is not None:
        if At.host_rowptr is None or tuple(At.shape) != tuple(A.shape):
            raise ValueError("csr_induce needs the resident transpose with its host_rowptr")
        tp = At.host_rowptr
        bound = max(bound, int((tp[ids_host + 1].astype(np.int64) - tp[ids_host]).sum()))
    if ids_dev is None:
        ids_dev = torch.from_numpy(ids_host).to(dev, non_blocking=True)
    _dev(ids_dev, torch.int32, "ids_dev")
    b = getattr(A, '_induce', None)
    if b is None:
        b = A._induce = _InduceBuffers(N, dev)
    b.fit(n, bound, transposition=At is None)
    st = _stream()
    a_p, a_c, a_v, ids, vmap = A.rowptr.data_ptr(), _ptr(A.col), _ptr(A.val), ids_dev.data_ptr(), b.map.data_ptr()
    check(lib.sgcn_induce_map_i32(ids, n, N, vmap, st))
    check(lib.sgcn_csr_induce_count(a_p, a_c, a_v, ids, n, vmap, b.rowptr.data_ptr(), b.full.data_ptr(), b.kept.data_ptr(), st))
    rscale = None
    if norm == 'rows':
        # n values, between two launches: full / kept is one correctly rounded fp32 division, exactly 1 where nothing was dropped
        rscale = torch.where(b.kept[:n] == 0, torch.ones((), dtype=torch.float32, device=dev), b.full[:n] / b.kept[:n],
                             out=b.rscale[:n])
    check(lib.sgcn_csr_induce_fill(a_p, a_c, a_v, ids, n, vmap, b.rowptr.data_ptr(), _ptr(rscale), b.col.data_ptr(),
                                   b.val.data_ptr(), b.coo.data_ptr(), 0, bound if At is None else 0, st))
    if At is not None:
        # the same cut of the resident transpose: row j of it holds the source rows of column j in ascending order, so its
        # block IS the stable transpose of the block above; an entry's scale is that of its relabelled column (the block's row)
        t_p, t_c, t_v = At.rowptr.data_ptr(), _ptr(At.col), _ptr(At.val)
        check(lib.sgcn_csr_induce_count(t_p, t_c, None, ids, n, vmap, b.t_rowptr.data_ptr(), None, None, st))
        check(lib.sgcn_csr_induce_fill(t_p, t_c, t_v, ids, n, vmap, b.t_rowptr.data_ptr(), _ptr(rscale), b.t_row.data_ptr(),
                                       b.t_val.data_ptr(), None, 1, 0, st))
    else:
        check(lib.sgcn_csr_transpose_index(n + 1, bound, b.col.data_ptr(), b.coo.data_ptr(), b.t_rowptr.data_ptr(),
                                           b.t_row.data_ptr(), b.t_src.data_ptr(), b.ws.data_ptr(), st))
        check(lib.sgcn_gather_f32(b.val.data_ptr(), b.t_src.data_ptr(), bound, b.t_val.data_ptr(), st))
    b.host[:n + 1].copy_(b.rowptr[:n + 1], non_blocking=True)
    b.host[n + 1:2 * (n + 1)].copy_(b.t_rowptr[:n + 1], non_blocking=True)
    torch.cuda.current_stream().synchronize()            # the one synchronisation of a build
    rp, trp = (np.array(h, dtype=np.int32) for h in (b.host[:n + 1].numpy(), b.host[n + 1:2 * (n + 1)].numpy()))
    nnz = int(rp[n])
    if nnz > bound or int(trp[n]) != nnz:
        raise RuntimeError("csr_induce: the block holds %d entries, its transpose %d, the bound is %d" % (nnz, int(trp[n]), bound))

    def csr(rowptr_dev, host_rowptr, col, val):
        seg, fix, nslots = build_plan(host_rowptr, plan_T)
        return DeviceCSR((n, n), rowptr_dev[:n + 1], col[:nnz], val[:nnz], DevicePlan(seg, fix, nslots, dev),
                         host_rowptr=host_rowptr)
    block = csr(b.rowptr, rp, b.col, b.val)
    block.coo_rows = b.coo[:nnz]
    block.transpose = csr(b.t_rowptr, trp, b.t_row, b.t_val)
    block.transpose.transpose = block
    block.map = b.map          # the position map of ``ids`` (N words; valid, like the block, until the next call): ops.spmm_pull
    if getattr(A, '_unique_cols', False):         # (check_unique_cols passed on A: its blocks store no column twice either)
        block._unique_cols = block.transpose._unique_cols = True
    return block


def spmm_pull(A, ids_dev, map_dev, x, H, out=None):
    """out[i] = sum over the stored entries e of row ids[i] of the RESIDENT square DeviceCSR ``A`` of
    val[e] * (x[map[col[e]]] if map[col[e]] >= 0 else H[col[e]])   (sgcn_spmm_pull_f32 / _h16; --full_batch_part_history).

    ``ids_dev``: the n selected vertices on the device, ascending and unique; ``map_dev``: their position map (N words,
    ``csr_induce(...).map``); ``x``: n x d fp32, the rows the step computes; ``H``: N x d, the stored rows of every vertex --
    fp32, or a bfloat16 table of ``history_alloc(..., bf16=True)``'s layout, widened exactly.  ``A`` is read in place: no
    cut, no plan, no synchronisation; one lane group per selected row, however long."""
    N = int(A.shape[0])
    if A.shape[0] != A.shape[1]:
        raise ValueError("spmm_pull needs a square (vertex x vertex) matrix")
    _dev(ids_dev, torch.int32, "ids_dev")
    _dev(map_dev, torch.int32, "map_dev")
    n = int(ids_dev.shape[0])
    xptr, ldx = _rows2d(x, "x")
    hptr, ldh, h16 = _hist2d(H, "H")
    d = int(x.shape[1])
    if int(x.shape[0]) != n:
        raise ValueError("x has %d rows, ids_dev %d entries" % (int(x.shape[0]), n))
    if int(H.shape[0]) < N or int(H.shape[1]) != d:
        raise ValueError("H has shape %s, need (>=%d, %d)" % (tuple(H.shape), N, d))
    if int(map_dev.shape[0]) < N:
        raise ValueError("map_dev has %d words, the matrix %d vertices" % (int(map_dev.shape[0]), N))
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=x.device)
    cptr, ldc = _rows2d(out, "out")
    if out.shape[0] != n or out.shape[1] < d:
        raise ValueError("out has shape %s, need (%d, >=%d)" % (tuple(out.shape), n, d))
    check((lib.sgcn_spmm_pull_h16 if h16 else lib.sgcn_spmm_pull_f32)(
        A.rowptr.data_ptr(), _ptr(A.col), _ptr(A.val), ids_dev.data_ptr(), n, N, map_dev.data_ptr(), d, xptr, ldx, hptr, ldh,
        cptr, ldc, _stream()))
    return out


def _pull_operands(who, A, ids_dev, map_dev, x, H, heads):
    """The checks ``spattn_pull`` and ``spattn_pull_bwd_q`` share -- ``spmm_pull``'s on the matrix, the ids, the map and the
    two tables, then the heads.  Returns n, N, d, heads, x's (ptr, pitch) and H's (ptr, pitch, h16)."""
    check_unique_cols(A)
    N = int(A.shape[0])
    if A.shape[0] != A.shape[1]:
        raise ValueError("%s needs a square (vertex x vertex) matrix" % who)
    _dev(ids_dev, torch.int32, "ids_dev")
    _dev(map_dev, torch.int32, "map_dev")
    n = int(ids_dev.shape[0])
    xp = _rows2d(x, "x")
    hp = _hist2d(H, "H")
    d = int(x.shape[1])
    heads = _attn_heads(d, heads)
    if int(x.shape[0]) != n:
        raise ValueError("x has %d rows, ids_dev %d entries" % (int(x.shape[0]), n))
    if int(H.shape[0]) < N or int(H.shape[1]) != d:
        raise ValueError("H has shape %s, need (>=%d, %d)" % (tuple(H.shape), N, d))
    if int(map_dev.shape[0]) < N:
        raise ValueError("map_dev has %d words, the matrix %d vertices" % (int(map_dev.shape[0]), N))
    return n, N, d, heads, xp, hp


def spmax_pull(A, ids_dev, map_dev, x, H, out=None, want_arg=True, arg=None):
    """(out, arg): the element-wise maximum of the n selected rows ``ids_dev`` of the RESIDENT square DeviceCSR ``A`` over EVERY
    stored entry e of row ids[i] in stored order, the entry's row being x[map[col[e]]] if map[col[e]] >= 0 else H[col[e]]
    (sgcn_spmax_pull_f32 / _h16; --full_batch_part_pull_max).  The first maximum wins under ``spmax``'s rule, whichever table
    it comes from; an empty row gives +0.0.

    arg[i, c] (int32) records the winner for ``spmax_bwd`` over the TRANSPOSED in-part block: >= 0 -- fresh, its POSITION in
    ``ids_dev`` (the block's column); -1 -- empty row; <= -2 -- stale, global column -2 - arg (a constant of the step: no row
    of the block matches it).  ``ids_dev``, ``map_dev``, ``x`` (n x d fp32) and ``H`` (N x d: fp32, or a bfloat16 table of
    ``history_alloc(..., bf16=True)``'s layout, widened exactly) as in ``spmm_pull``; ``out`` (may be a pitched (n, >= d)
    view), ``want_arg`` and ``arg`` as in ``spmax``.  ``A`` is read in place, its values not at all: no cut, no plan, no
    synchronisation; one lane group per selected row, however long.  The result has the bits of ``spmax`` without a plan on
    the rows ``ids`` of ``A`` and the merged table (H with the rows ids replaced by x)."""
    n, N, d, _, (xptr, ldx), (hptr, ldh, h16) = _pull_operands("spmax_pull", A, ids_dev, map_dev, x, H, 1)
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=x.device)
    cptr, ldc = _rows2d(out, "out")
    if out.shape[0] != n or out.shape[1] < d:
        raise ValueError("out has shape %s, need (%d, >=%d)" % (tuple(out.shape), n, d))
    ldarg = d
    if not want_arg:
        arg = None
    elif arg is None:
        arg = torch.empty((n, d), dtype=torch.int32, device=x.device)
    else:
        _dev(arg, torch.int32, "arg")
        if arg.dim() != 2 or arg.shape[0] != n or arg.shape[1] < d or (arg.shape[1] > 1 and arg.stride(1) != 1):
            raise ValueError("arg has shape %s, need (%d, >=%d) with unit column stride" % (tuple(arg.shape), n, d))
        ldarg = arg.stride(0) if n > 1 else max(arg.stride(0), arg.shape[1])
    check((lib.sgcn_spmax_pull_h16 if h16 else lib.sgcn_spmax_pull_f32)(
        A.rowptr.data_ptr(), _ptr(A.col), ids_dev.data_ptr(), n, N, map_dev.data_ptr(), d, xptr, ldx, hptr, ldh, cptr, ldc,
        _ptr(arg), ldarg, _stream()))
    return out, arg


def spattn_pull(A, ids_dev, map_dev, x, H, scale, out=None, want_lse=True, heads=1):
    """(out, lse): softmax dot-product attention of the n selected rows ``ids_dev`` of the RESIDENT square DeviceCSR ``A`` over
    EVERY stored entry e of row ids[i], the entry's key / value row being x[map[col[e]]] if map[col[e]] >= 0 else H[col[e]]
    and the query x[i]   (sgcn_spattn_pull_f32 / _h16; --full_batch_part_pull with --aggregator attn).

    ``ids_dev``, ``map_dev``, ``x`` (n x d fp32, the rows the step computes) and ``H`` (N x d: fp32, or a bfloat16 table of
    ``history_alloc(..., bf16=True)``'s layout, widened exactly) as in ``spmm_pull``; ``scale``, ``out`` (may be a pitched
    (n, >= d) view), ``want_lse`` and ``heads`` as in ``spattn``: lse is (n,) for heads == 1, else (n, heads).  ``A`` is read
    in place: no cut, no plan, no synchronisation; one lane group per selected row, however long.  The result has the bits
    of ``spattn`` without a plan on the rows ``ids`` of ``A`` and the merged table (H with the rows ids replaced by x)."""
    n, N, d, heads, (xptr, ldx), (hptr, ldh, h16) = _pull_operands("spattn_pull", A, ids_dev, map_dev, x, H, heads)
    if out is None:
        out = _attn_out(n, d, x.device, heads)
    cptr, ldc = _rows2d(out, "out")
    if out.shape[0] != n or out.shape[1] < d:
        raise ValueError("out has shape %s, need (%d, >=%d)" % (tuple(out.shape), n, d))
    lse = torch.empty((n,) if heads == 1 else (n, heads), dtype=torch.float32, device=x.device) if want_lse else None
    check((lib.sgcn_spattn_pull_h16 if h16 else lib.sgcn_spattn_pull_f32)(
        A.rowptr.data_ptr(), _ptr(A.col), ids_dev.data_ptr(), n, N, map_dev.data_ptr(), d, heads, xptr, ldx, hptr, ldh,
        float(scale), cptr, ldc, _ptr(lse), _stream()))
    return out, lse


def spattn_pull_bwd_q(A, ids_dev, map_dev, x, H, g, out_fwd, lse, scale, add=None, add_rows=0, heads=1):
    """(dq, delta): the query's half of the gradient of ``spattn_pull`` for g = dL/dout, from the forward's ``out_fwd`` and
    ``lse`` -- sgcn_spattn_pull_bwd_q_f32 / _h16: delta[i, h] = <g[i], out_fwd[i]>_h and dq[i] = scale * sum_e e_e B_e over ALL
    stored entries of row ids[i] (+ add[i] on the first ``add_rows`` rows).  delta is (n * heads,) floats, row-major (n, heads):
    what the keys' / values' half (sgcn_spattn_*_bwd_kv over the transposed induced block) reads.  Stored rows are constants:
    nothing flows into ``H``."""
    n, N, d, heads, (xptr, ldx), (hptr, ldh, h16) = _pull_operands("spattn_pull_bwd_q", A, ids_dev, map_dev, x, H, heads)
    gptr, ldg = _rows2d(g, "g")
    cptr, ldc = _rows2d(out_fwd, "out_fwd")
    if tuple(g.shape) != (n, d) or out_fwd.shape[0] != n or out_fwd.shape[1] < d:
        raise ValueError("g and out_fwd must be (%d, %d), got %s and %s" % (n, d, tuple(g.shape), tuple(out_fwd.shape)))
    _dev(lse, torch.float32, "lse")
    if tuple(lse.shape) != ((n,) if heads == 1 else (n, heads)) or not lse.is_contiguous():
        raise ValueError("lse must be what spattn_pull returned: contiguous, (%d,) at one head, else (%d, %d)" % (n, n, heads))
    aptr, ldadd = _rows2d(add, "add") if add is not None else (None, 0)
    add_rows = int(add_rows) if add is not None else 0
    delta = torch.empty((n * heads,), dtype=torch.float32, device=x.device)
    dq = _attn_out(n, d, x.device, heads)
    check((lib.sgcn_spattn_pull_bwd_q_h16 if h16 else lib.sgcn_spattn_pull_bwd_q_f32)(
        A.rowptr.data_ptr(), _ptr(A.col), ids_dev.data_ptr(), n, N, map_dev.data_ptr(), d, heads, xptr, ldx, hptr, ldh,
        float(scale), gptr, ldg, cptr, ldc, lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), _rows2d(dq, "dq")[1], aptr, ldadd,
        add_rows, _stream()))
    return dq, delta


def spattn_pull_bwd_kv(At, x, g, lse, delta, dq, scale, heads=1):
    """dx = dB + dq: the keys' / values' half of ``spattn_pull``'s gradient, through in-part entries only -- the one-table
    sgcn_spattn_*_bwd_kv over ``At``, the transposed induced block A[S, S]^T (n x n), with queries = keys = ``x`` and the
    ``lse`` / ``delta`` of the two pull launches (the coefficients it recomputes are those of the FULL row); ``dq`` is the
    launch's addend."""
    n = int(At.shape[0])
    if tuple(At.shape) != (n, n) or int(x.shape[0]) != n:
        raise ValueError("At must be the square transposed block over the %d rows of x, got %s" % (int(x.shape[0]), tuple(At.shape)))
    b = _rows2d(x, "x")
    d = int(x.shape[1])
    heads = _attn_heads(d, heads)
    gp = _rows2d(g, "g")
    if tuple(g.shape) != (n, d) or tuple(dq.shape) != (n, d):
        raise ValueError("g and dq must be (%d, %d), got %s and %s" % (n, d, tuple(g.shape), tuple(dq.shape)))
    _dev(lse, torch.float32, "lse")
    _dev(delta, torch.float32, "delta")
    if lse.numel() != n * heads or delta.numel() != n * heads or not lse.is_contiguous() or not delta.is_contiguous():
        raise ValueError("lse and delta must hold %d x %d contiguous floats" % (n, heads))
    return _spattn_bwd_kv(At, d, heads, 1.0, 0, b, b, scale, gp, lse, delta, x.device, dq)


def _gat_pull_operands(who, A, ids_dev, map_dev, x, H, u, v, vh, slope, heads):
    """``_pull_operands``, then the slope and the three score tables: u, v (n, heads) fresh, vh (>= N, heads) stored.  Returns
    what ``_pull_operands`` does, the slope, and the (ptr, pitch) pairs of u, v and vh as one flat tuple."""
    n, N, d, heads, xp, hp = _pull_operands(who, A, ids_dev, map_dev, x, H, heads)
    slope = _attn_slope(slope)
    tabs = _gat_table(u, n, heads, "u") + _gat_table(v, n, heads, "v") + _gat_table(vh, N, heads, "vh")
    return n, N, d, heads, xp, hp, slope, tabs


def spgat_pull(A, ids_dev, map_dev, x, H, u, v, vh, slope, out=None, want_lse=True, heads=1):
    """(out, lse): attention with learned additive scores of the n selected rows ``ids_dev`` of the RESIDENT square DeviceCSR
    ``A`` over EVERY stored entry e of row ids[i]: with c = col[e] and m = map[c], the entry's value row is x[m] if m >= 0 else
    H[c] and its destination score v[m] if m >= 0 else vh[c]; z_e = u[i] + v_e per head, then as ``spgat``
    (sgcn_spgat_pull_f32 / _h16; --full_batch_part_pull_gat).

    ``ids_dev``, ``map_dev``, ``x`` and ``H`` as in ``spattn_pull``; ``u`` and ``v`` (n, H): the fresh score tables (views of
    ``gat_scores(x, a)``'s result serve); ``vh`` (>= N, H) fp32: the stored destination scores, constants.  lse is (n, heads),
    as in ``spgat``.  ``A`` is read in place: no cut, no plan, no synchronisation.  The result has the bits of ``spgat``
    without a plan on the rows ``ids`` of ``A`` and the merged tables."""
    n, N, d, heads, (xptr, ldx), (hptr, ldh, h16), slope, (uptr, ldu, vptr, ldv, vhptr, ldvh) = _gat_pull_operands(
        "spgat_pull", A, ids_dev, map_dev, x, H, u, v, vh, slope, heads)
    if out is None:
        out = _attn_out(n, d, x.device, heads)
    cptr, ldc = _rows2d(out, "out")
    if out.shape[0] != n or out.shape[1] < d:
        raise ValueError("out has shape %s, need (%d, >=%d)" % (tuple(out.shape), n, d))
    lse = torch.empty((n, heads), dtype=torch.float32, device=x.device) if want_lse else None
    check((lib.sgcn_spgat_pull_h16 if h16 else lib.sgcn_spgat_pull_f32)(
        A.rowptr.data_ptr(), _ptr(A.col), ids_dev.data_ptr(), n, N, map_dev.data_ptr(), d, heads, xptr, ldx, hptr, ldh,
        uptr, ldu, vptr, ldv, vhptr, ldvh, slope, cptr, ldc, _ptr(lse), _stream()))
    return out, lse


def spgat_pull_bwd_u(A, ids_dev, map_dev, x, H, u, v, vh, g, out_fwd, lse, slope, heads=1):
    """(dU, delta): the source score's half of the gradient of ``spgat_pull`` for g = dL/dout, from the forward's ``out_fwd``
    and ``lse`` -- sgcn_spgat_pull_bwd_u_f32 / _h16: delta[i, h] = <g[i], out_fwd[i]>_h and dU[i, h] = sum_e dz_e over ALL
    stored entries of row ids[i].  Both are (n, heads): what ``spgat_pull_bwd_v`` and ``gat_scores_bwd`` read.  Stored rows
    and scores are constants: nothing flows into ``H`` or ``vh``."""
    n, N, d, heads, (xptr, ldx), (hptr, ldh, h16), slope, (uptr, ldu, vptr, ldv, vhptr, ldvh) = _gat_pull_operands(
        "spgat_pull_bwd_u", A, ids_dev, map_dev, x, H, u, v, vh, slope, heads)
    gptr, ldg = _rows2d(g, "g")
    cptr, ldc = _rows2d(out_fwd, "out_fwd")
    if tuple(g.shape) != (n, d) or out_fwd.shape[0] != n or out_fwd.shape[1] < d:
        raise ValueError("g and out_fwd must be (%d, %d), got %s and %s" % (n, d, tuple(g.shape), tuple(out_fwd.shape)))
    _dev(lse, torch.float32, "lse")
    if tuple(lse.shape) != (n, heads) or not lse.is_contiguous():
        raise ValueError("lse must be what spgat_pull returned: a contiguous (%d, %d) table of floats" % (n, heads))
    delta = torch.empty((n, heads), dtype=torch.float32, device=x.device)
    dU = torch.empty((n, heads), dtype=torch.float32, device=x.device)
    check((lib.sgcn_spgat_pull_bwd_u_h16 if h16 else lib.sgcn_spgat_pull_bwd_u_f32)(
        A.rowptr.data_ptr(), _ptr(A.col), ids_dev.data_ptr(), n, N, map_dev.data_ptr(), d, heads, xptr, ldx, hptr, ldh,
        uptr, ldu, vptr, ldv, vhptr, ldvh, slope, gptr, ldg, cptr, ldc, lse.data_ptr(), delta.data_ptr(), dU.data_ptr(),
        _stream()))
    return dU, delta


def spgat_pull_bwd_v(At, x, u, v, g, lse, delta, slope, add=None, add_rows=0, heads=1):
    """(dB, dV): the values' and destination scores' half of ``spgat_pull``'s gradient, through in-part entries only -- the
    one-table sgcn_spgat_csr_bwd_v_f32 alone over ``At``, the transposed induced block A[S, S]^T (n x n) with its plan, with
    B = ``x``, the fresh ``u`` / ``v`` and the ``lse`` / ``delta`` of the two pull launches (the coefficients it recomputes are
    those of the FULL row).  ``add`` (its first ``add_rows`` rows) joins dB in the launch's epilogue."""
    n = int(At.shape[0])
    if tuple(At.shape) != (n, n) or int(x.shape[0]) != n:
        raise ValueError("At must be the square transposed block over the %d rows of x, got %s" % (int(x.shape[0]), tuple(At.shape)))
    slope = _attn_slope(slope)
    bptr, ldb = _rows2d(x, "x")
    d = int(x.shape[1])
    heads = _attn_heads(d, heads)
    uptr, ldu = _gat_table(u, n, heads, "u")
    vptr, ldv = _gat_table(v, n, heads, "v")
    gptr, ldg = _rows2d(g, "g")
    if tuple(g.shape) != (n, d):
        raise ValueError("g must be (%d, %d), got %s" % (n, d, tuple(g.shape)))
    for t, name in ((lse, "lse"), (delta, "delta")):
        _dev(t, torch.float32, name)
        if tuple(t.shape) != (n, heads) or not t.is_contiguous():
            raise ValueError("%s must be a contiguous (%d, %d) table of floats" % (name, n, heads))
    aptr, ldadd = _rows2d(add, "add") if add is not None else (None, 0)
    add_rows = int(add_rows) if add is not None else 0
    dV = torch.empty((n, heads), dtype=torch.float32, device=x.device)
    dB = _attn_out(n, d, x.device, heads)
    tplan = At.plan.struct(attn_slot('gat_bwd_v', d)) if At.plan is not None else None
    check(lib.sgcn_spgat_csr_bwd_v_f32(At.rowptr.data_ptr(), _ptr(At.col), n, n, d, heads, 1.0, 0, uptr, ldu, vptr, ldv, bptr,
                                       ldb, slope, gptr, ldg, lse.data_ptr(), delta.data_ptr(), dB.data_ptr(),
                                       _rows2d(dB, "dB")[1], dV.data_ptr(), aptr, ldadd, add_rows, _byref(tplan), _stream()))
    return dB, dV


def adam_step(theta, grad, m, v, lr_t, beta1, beta2, eps=1e-8):
    check(lib.sgcn_adam_f32(theta.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(),
                            int(theta.numel()), float(lr_t), float(beta1), float(beta2), float(eps),
                            _stream()))


def polyak_factors(decay):
    """(decay, one_minus) as sgcn_adam_ema_f32 takes them: fp32(decay) and fl(1.0f - decay), both as Python floats."""
    d = np.float32(decay)
    return float(d), float(np.float32(1.0) - d)


def adam_ema_step(theta, grad, m, v, avg, lr_t, beta1, beta2, eps=1e-8, decay=0.0):
    """adam_step that also moves the weights' average: avg <- fl(fl(avg * decay) + fl(theta_new * fl(1 - decay)))
    (sgcn_adam_ema_f32; --polyak_decay)."""
    n = int(theta.numel())
    for t, name in ((theta, "theta"), (grad, "grad"), (m, "m"), (v, "v"), (avg, "avg")):
        _dev(t, torch.float32, name)
        if not t.is_contiguous() or int(t.numel()) != n:
            raise ValueError("%s must be a contiguous fp32 array of %d elements" % (name, n))
    d, om = polyak_factors(decay)
    check(lib.sgcn_adam_ema_f32(theta.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), avg.data_ptr(), n,
                                float(lr_t), float(beta1), float(beta2), float(eps), d, om, _stream()))


# ---- running statistics of the --gradvar study (sgcn_stats.hip; gcn/stats.py, gcn/train.py:241-276) ----
def moments_add(x, count, mean, m2):
    """Fold the fp32 sample x into the running fp64 (mean, m2) that already hold ``count`` samples (Welford;
    count == 0 initialises them)   (sgcn_moments_add_f32)."""
    xp, n = _flat(x, "x")
    for t, name in ((mean, "mean"), (m2, "m2")):
        _dev(t, torch.float64, name)
        if not t.is_contiguous() or int(t.numel()) != n:
            raise ValueError("%s must be a contiguous fp64 array of %d elements" % (name, n))
    check(lib.sgcn_moments_add_f32(xp, n, int(count), mean.data_ptr(), m2.data_ptr(), _stream()))


def moments_summary(mean_a, m2_a, count_a, mean_b=None, out=None):
    """Device fp64[3] = {mean |mean_a|, mean sqrt(m2_a / count_a), mean |mean_a - mean_b| (0 without mean_b)}
    (sgcn_moments_summary_f64)."""
    n = int(mean_a.numel())
    for t, name in ((mean_a, "mean_a"), (m2_a, "m2_a"), (mean_b, "mean_b")):
        if t is not None:
            _dev(t, torch.float64, name)
            if not t.is_contiguous() or int(t.numel()) != n:
                raise ValueError("%s must be a contiguous fp64 array of %d elements" % (name, n))
    if out is None:
        out = torch.empty(3, dtype=torch.float64, device=mean_a.device)
    check(lib.sgcn_moments_summary_f64(mean_a.data_ptr(), m2_a.data_ptr(), int(count_a), _ptr(mean_b), n,
                                       _dev(out, torch.float64, "out").data_ptr(), _stream()))
    return out


# ---- staleness of a control-variate history (sgcn_stats.hip; --history_error) -----------------------------------------------
_HIST_ERR_WS = {}


def history_error(x, H, out=None):
    """Device fp64[4] = {sum (x - H)^2, sum x^2, max |x - H|, rows with any x != H} of the exact activations ``x`` (fp32 rows,
    a pitched view is fine) against the stored history ``H`` (fp32 or bfloat16, widened exactly): every difference and square
    in fp64, a fixed grid and summation order -- the same bits on every call (sgcn_hist_error_f32 / _h16).  Nothing is
    synchronised; the relative staleness is sqrt(out[0] / out[1]) once the vector is on the host."""
    if x.dim() != 2 or tuple(x.shape) != tuple(H.shape):
        raise ValueError("history_error: x has shape %s, the history %s" % (tuple(x.shape), tuple(H.shape)))
    n, d = int(x.shape[0]), int(x.shape[1])
    if n == 0:          # (the strides of an empty tensor say nothing: the library zeroes out4 without reading a pitch)
        _dev(x, torch.float32, "x")
        if H.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("H must be torch.float32 or torch.bfloat16, got %s" % H.dtype)
        h16 = H.dtype == torch.bfloat16
        xp, ldx, hp, ldh = None, d, None, (d + 7) // 8 * 8
    else:
        xp, ldx = _rows2d(x, "x")
        hp, ldh, h16 = _hist2d(H, "H")
    if not H.is_cuda:
        raise RuntimeError("H must live in HBM (got a %s tensor): the SpMM/history path has no CPU fallback" % (H.device,))
    if out is None:
        out = torch.empty(4, dtype=torch.float64, device=x.device)
    # one workspace per device: the two launches of a call run back to back on the caller's stream
    ws = _HIST_ERR_WS.get(x.device)
    if ws is None:
        ws = _HIST_ERR_WS[x.device] = torch.empty(int(lib.sgcn_hist_error_ws_doubles()), dtype=torch.float64, device=x.device)
    check((lib.sgcn_hist_error_h16 if h16 else lib.sgcn_hist_error_f32)(
        xp, ldx, hp, ldh, n, d, _dev(out, torch.float64, "out").data_ptr(), ws.data_ptr(), _stream()))
    return out


# ---- column-sweep SpMM for static graphs (sgcn_spmm_cs.hip) --------------------------------------
def transpose_host(a, threads=0):
    """A^T of a SciPy CSR as a SciPy CSR with sorted rows, by the library's parallel counting sort
    (sgcn_csr_transpose_host): what the plan of a backward product (the autodiff of gcn/layers.py:31-37) is built from.
    Same arrays as ``a.T.tocsr()`` (rows ascend inside a column), in a fraction of its single-threaded time."""
    import scipy.sparse as sp
    a = a.tocsr()
    M, K = int(a.shape[0]), int(a.shape[1])
    rowptr = np.ascontiguousarray(a.indptr, dtype=np.int32)
    col = np.ascontiguousarray(a.indices, dtype=np.int32)
    val = np.ascontiguousarray(a.data, dtype=np.float32)
    trp = np.empty(K + 1, dtype=np.int32)
    tc = np.empty(col.shape[0], dtype=np.int32)
    tv = np.empty(col.shape[0], dtype=np.float32)
    check(lib.sgcn_csr_transpose_host(rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, M, K, int(threads),
                                      trp.ctypes.data, tc.ctypes.data, tv.ctypes.data))
    t = sp.csr_matrix((tv, tc, trp), shape=(K, M), copy=False)
    t.has_sorted_indices = True
    return t


def reorder_labels(a, max_iters=0, seed=1, min_size=64):
    """Community label per vertex of a square sparse matrix's pattern (sgcn_reorder_lp: seeded
    asynchronous label propagation on the host, graph only).  Returns (comm int32[n], ncomm)."""
    a = a.tocsr()
    if a.shape[0] != a.shape[1]:
        raise ValueError("reorder_labels needs a square (vertex x vertex) matrix")
    rowptr = np.ascontiguousarray(a.indptr, dtype=np.int32)
    col = np.ascontiguousarray(a.indices, dtype=np.int32)
    comm = np.empty(a.shape[0], dtype=np.int32)
    nc = C.c_int32()
    check(lib.sgcn_reorder_lp(rowptr.ctypes.data, col.ctypes.data, int(a.shape[0]), int(max_iters), int(seed),
                              int(min_size), comm.ctypes.data, C.byref(nc)))
    return comm, int(nc.value)


def _cs_round(round_tiles=0):
    """Tiles per launch round of a column-sweep plan: the caller's, else the library's tunable, else 4096."""
    return int(round_tiles or (_ffi.lib.sgcn_tune_get(b"cs_round") or 4096))


def _smallest_t(fits, lo, hi):
    """The smallest split threshold in [lo, hi] whose pieces ``fits`` accepts (monotone in t; ``hi`` when none does)."""
    while lo < hi:
        mid = (lo + hi) // 2
        if fits(mid):
            hi = mid
        else:
            lo = mid + 1
    return lo


class SweepClock(object):
    """The sweep clock of a ColumnSweepCSR for ONE operand type, per width d."""
    # The sweep clock of a plan is tuned per width AND operand type: a bfloat16 operand moves half the bytes per step and holds
    # the lock-step on a different clock.  A plan keeps one record per type (``plan.clock(bf16)``): ``pace`` / ``tuned_ms`` /
    # ``_guard`` of the plan are the fp32 operand's, ``pace_b16`` ... the bfloat16 operand's, and the two never mix -- in
    # struct(), the autotuner, the lost-lock guard and the plan cache.
    __slots__ = ("pace", "tuned_ms", "guard")

    def __init__(self, pace=None, tuned_ms=None):
        self.pace = pace or {}              # d -> ns per step of the heaviest tile (autotuned), -1 = unpaced
        self.tuned_ms = tuned_ms or {}      # d -> the product's time at that pace (what the lost-lock guard compares against)
        self.guard = {}                     # d -> the guard's state (ColumnSweepCSR._guard_before)

    def to_npz(self):
        """The (pace, tuned_ms) arrays of the plan cache."""
        return (np.array([[d, p] for d, p in sorted(self.pace.items())], np.int64).reshape(-1, 2),
                np.array([[d, self.tuned_ms[d]] for d in sorted(self.pace) if d in self.tuned_ms], np.float64).reshape(-1, 2))

    @classmethod
    def from_npz(cls, z, pace_key, tuned_key):
        """A cached pace is only as good as the box and clock it was tuned on: it comes back WITH the time it gave there, so
        the run-time guard (_guard_before / _guard_after) is armed from the first product on; paces stored without that
        time (files of older builds) are dropped and tuned again, unless unpaced.  A file without the keys (a build
        without this operand type) gives an empty clock."""
        tuned = {int(d): float(ms) for d, ms in z[tuned_key]} if tuned_key in z.files else {}
        pace = {int(d): int(p) for d, p in z[pace_key] if int(d) in tuned or int(p) <= 0} if pace_key in z.files else {}
        return cls(pace, {d: ms for d, ms in tuned.items() if d in pace})


class ColumnSweepCSR(object):
    """A static CSR re-laid for the column sweep (include/sgcn.h sgcn_csplan_t): built once on the
    host (full-graph / PP products), then multiplied many times.

    ``col_labels`` / ``row_labels`` (community label per column vertex / per row, e.g. from
    ``reorder_labels``): a locality-preserving plan for graphs that HAVE communities.  Columns are
    renumbered so that a community's vertices are contiguous (the sweep order; B itself is not
    moved -- the kernel reads B rows through the position -> vertex map), tiles are formed inside
    row communities in community order, a launch's consecutive tiles go to the same XCD, and the
    sweep runs unpaced (the waves of an XCD then work on the same few communities' B rows, which is
    what the clock pacing provides on a graph without structure).  Results equal the unlabelled
    plan's up to fp32 summation order."""

    WARP_BUCKETS = 16384      # the warp table's size bound (64 KiB: scalar cache / L2 resident)
    WARP_AUTO_DEV = 0.01      # 'auto': a table is kept when some column's share of the work in front of it is off its
                              # share of the ids by more than this (1 % of the sweep ~ a third of an L2 window)

    def clock(self, bf16=False):
        """The SweepClock of the operand type (fp32, or bfloat16)."""
        return self._clocks[bool(bf16)]

    CLOCK_KEYS = (("pace", "tuned_ms"), ("pace_b16", "tuned_ms_b16"))       # the clocks' keys in the plan cache, by type
    pace = property(lambda self: self._clocks[0].pace)
    tuned_ms = property(lambda self: self._clocks[0].tuned_ms)
    _guard = property(lambda self: self._clocks[0].guard)
    pace_b16 = property(lambda self: self._clocks[1].pace)
    tuned_ms_b16 = property(lambda self: self._clocks[1].tuned_ms)
    _guard_b16 = property(lambda self: self._clocks[1].guard)

    @classmethod
    def make_warp(cls, cols, K, mode='auto'):
        """The sweep clock in work coordinates (include/sgcn.h sgcn_csplan_t.dev_warp): ``(table, shift)`` with
        table[b] = share of the nonzeros in columns < (b << shift), scaled to [0, K) -- or ``(None, 0)`` when the nonzeros
        are spread evenly enough over the column ids for the linear clock (S-Reddit: hubs carry random ids), or
        ``mode`` is False.  R-MAT is the case it exists for: a third of the nonzeros in the first sixteenth of the ids."""
        K = int(K)
        if mode is False or K <= 0 or cols.shape[0] == 0:
            return None, 0
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        table = np.empty(cls.WARP_BUCKETS, dtype=np.uint32)
        nb, shift = C.c_int32(), C.c_int32()
        check(lib.sgcn_cs_warp_table(cols.ctypes.data, cols.shape[0], K, cls.WARP_BUCKETS, 0 if mode == 'auto' else 1,
                                     cls.WARP_AUTO_DEV, 0, table.ctypes.data, C.byref(nb), C.byref(shift)))
        if nb.value == 0:
            return None, 0
        return np.ascontiguousarray(table[:nb.value]), int(shift.value)

    def __init__(self, a, device, R=16, T=0, round_tiles=0, col_labels=None, row_labels=None, G=1, align='auto', warp='auto',
                 col_ranges=0, dictionary=True):
        """G = 2: two 16-row lane groups per wavefront on 128-column passes (sgcn_csplang_*), half the passes of
        the dense operand through every XCD per register byte; ``align``: columns one bin of a wave may run ahead
        of the slowest (the plan pads the bins that are ahead; 'auto': a third of the L2 window, ``auto_align``; with a
        warp table -- ``warp``, ``make_warp`` -- it counts sweep positions).  What ``choose_g(d)`` picks for most widths -- the
        bench and the training path call it: S-Reddit d = 602 3.51 vs 3.67 ms sustained, S-RMAT d = 256 2.61 vs
        2.82 ms.  G = 4 (four groups, 64-column passes, every row of a 233 k-row graph resident in one round): instruction-
        bound on a full graph (3.75 ms on S-Reddit; its gathers alone 3.21: DESIGN.md 3.2), but the better sweep for a SPARSE
        matrix such as the LDS sweep's residual, which is what uses it.
        ``dictionary``: let the library keep the entries' values in per-tile tables where every tile has few distinct ones
        (sgcn_csbuild_dict, sgcn_tune "cs_dict": the library decides, per plan); False for a plan whose value array is
        re-drawn every step (``live_val``; a dictionary plan takes one too, on a second copy of its words)."""
        a = a.tocsr()
        G, labelled = int(G), col_labels is not None or row_labels is not None
        if R != 16:
            raise ValueError("the column-sweep kernels keep 16-row bins (R = 16)")
        if G not in (1, 2, 4):
            raise ValueError("G must be 1, 2 or 4 lane groups per wavefront")
        if col_ranges and int(col_ranges) > 1:
            if G != 1 or labelled:
                raise ValueError("col_ranges needs an unlabelled plan with one lane group per wavefront")
            p = self._plan_ranged(a, int(col_ranges), T, round_tiles)
        elif G != 1:
            if labelled:
                raise ValueError("G = 2 plans are ungrouped and use 16-row bins")
            p = self._plan_groups(a, G, T, round_tiles, align, warp, dictionary)
        else:
            p = self._plan_one(a, T, round_tiles, col_labels, row_labels, warp)
        self._finish(p, device, round_tiles)

    # What a builder (_plan_one / _plan_groups / _plan_ranged) or the cache file (_load) hands to _finish: the host arrays
    # ``tile_ptr, colrow, val, tile_rows, tile_slots, fix``, ``nslots``, ``shape``, ``nnz`` and the entries below, which
    # default to what a plan without them has.  ``host_plan_s``: what the builder spent in the plan builder proper.
    # A dictionary plan (``dict_bits`` > 0) has ``val`` None and the tables ``tile_vals`` [ntiles << dict_bits] / ``tile_nvals``.
    _RECORD = dict(R=16, G=1, T=None, align=None, pad_fraction=0.0, ranged=0, range_cuts=None, grouped=False, pos2col=None,
                   warp=None, warp_shift=0, host_plan_s=None, dict_bits=0, tile_vals=None, tile_nvals=None)

    @staticmethod
    def _record(built, **entries):
        """A plan record from ``_build``'s result; ``entries`` fill (or replace) the rest."""
        tile_ptr, colrow, val, tile_rows, tile_slots, fix, _, _, nslots = built
        p = dict(ColumnSweepCSR._RECORD, tile_ptr=tile_ptr, colrow=colrow, val=val, tile_rows=tile_rows, tile_slots=tile_slots,
                 fix=fix, nslots=nslots)
        p.update(entries)
        return p

    def _finish(self, p, device, round_tiles, clocks=None):
        """Make this object the plan of record ``p`` on ``device``: the one place that assigns a plan's attributes and
        uploads its arrays, so a plan is the same object whether it was built (by any builder) or loaded."""
        t_up = time.perf_counter()
        to = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(device)          # noqa: E731
        self.shape, self.nnz, self.R, self.round_tiles = p["shape"], p["nnz"], p["R"], round_tiles
        self.G, self.T, self.align, self.pad_fraction = p["G"], p["T"], p["align"], p["pad_fraction"]
        self.ranged, self.range_cuts, self.grouped = p["ranged"], p["range_cuts"], p["grouped"]
        self.ntiles, self.nfix, self.nslots = int(p["tile_ptr"].shape[0] - 1), int(p["fix"].shape[0]), int(p["nslots"])
        self._tile_nnz = (np.diff(p["tile_ptr"]) // self.G).astype(np.int64)       # steps per tile (what the pace counts)
        self._hint, self._hint_round = None, None
        self._clocks = clocks or (SweepClock(), SweepClock())                     # (fp32 operand, bfloat16 operand)
        self._tuning, self._cache = False, None                                    # (_cache: where ``cached`` wants it stored)
        self.tile_ptr, self.colrow, self._val = to(p["tile_ptr"]), to(p["colrow"]), to(p["val"])
        # a dictionary plan: no value array (``val`` decodes one on demand), the tiles' tables instead
        self.dict_bits, self.tile_vals, self.tile_nvals = int(p["dict_bits"]), to(p["tile_vals"]), to(p["tile_nvals"])
        self._colrow_plain = None  # (the words without their indices, made when a ``live_val`` is first handed to such a plan)
        self.live_val = None       # a re-drawn value array the products read instead of ``val`` (full_batch.StaticMatrix,
                                   # inside a training step under --edge_dropout); ``val``, the base values, is what is saved
        self.tile_rows, self.tile_slots = to(p["tile_rows"]), to(p["tile_slots"])
        self.fix = to(p["fix"]) if self.nfix else None
        self.ws, self.device = None, device
        self.pos2col = to(p["pos2col"])
        # the clock's coordinates (make_warp; a ranged plan's own table)
        self.warp, self.warp_shift = to(None if p["warp"] is None else p["warp"].view(np.int32)), p["warp_shift"]
        # what the plan cost to set up (the product it serves may run once: gcn/utils.py:321-322); None on a loaded plan
        self.setup_s = None if p["host_plan_s"] is None else {
            "host_plan_s": p["host_plan_s"], "upload_s": time.perf_counter() - t_up, "host_threads": int(lib.sgcn_host_threads())}

    @property
    def val(self):
        """The value of every entry.  A dictionary plan keeps none: it is decoded from the tiles' tables, for the callers
        that inspect a plan (the products never ask)."""
        if self.dict_bits == 0:
            return self._val
        tile = torch.repeat_interleave(torch.arange(self.ntiles, device=self.tile_ptr.device), self.tile_ptr[1:] - self.tile_ptr[:-1])
        idx = (self.colrow.long() >> (28 - self.dict_bits)) & ((1 << self.dict_bits) - 1)
        return self.tile_vals[(tile << self.dict_bits) + idx]

    def columns_rows(self):
        """``colrow`` on the host as a plan with a value array has it: col | local row << 28 (a dictionary plan's index bits
        cleared)."""
        cr = self.colrow.cpu().numpy()
        if self.dict_bits:
            cr = (cr.view(np.uint32) & np.uint32(((1 << (28 - self.dict_bits)) - 1) | 0xF0000000)).view(np.int32)
        return cr

    @staticmethod
    def _plan_one(a, T, round_tiles, col_labels, row_labels, warp):
        """One lane group per wavefront (sgcn_csplan_*), plain or labelled (see the class docstring)."""
        rowptr = np.ascontiguousarray(a.indptr, dtype=np.int32)
        col = np.ascontiguousarray(a.indices, dtype=np.int32)
        val = np.ascontiguousarray(a.data, dtype=np.float32)
        M = rowptr.shape[0] - 1
        grouped = col_labels is not None or row_labels is not None
        pos2col = None
        if col_labels is not None:
            col_labels = np.ascontiguousarray(col_labels, dtype=np.int32)
            if col_labels.shape[0] != a.shape[1]:
                raise ValueError("col_labels must have one label per column")
            pos2col = np.argsort(col_labels, kind='stable').astype(np.int32)     # sweep position -> vertex
            col2pos = np.empty_like(pos2col)
            col2pos[pos2col] = np.arange(pos2col.shape[0], dtype=np.int32)
            col = np.ascontiguousarray(col2pos[col])                              # the plan lives in positions
        rg = None
        if row_labels is not None:
            rg = np.ascontiguousarray(row_labels, dtype=np.int32)
            if rg.shape[0] != M:
                raise ValueError("row_labels must have one label per row")
        if not T and not grouped:
            T = ColumnSweepCSR.auto_t(rowptr, 1, _cs_round(round_tiles))
        t_build = time.perf_counter()
        built = ColumnSweepCSR._build(rowptr, col, val, M, 1, 16, T, 0, 0, rg.ctypes.data if rg is not None else None, None, 0)
        t_build = time.perf_counter() - t_build
        # the clock's coordinates (grouped plans run unpaced: no table)
        wtab, shift = (None, 0) if grouped else ColumnSweepCSR.make_warp(col, a.shape[1], warp)
        return ColumnSweepCSR._record(built, shape=(int(a.shape[0]), int(a.shape[1])), nnz=int(col.shape[0]), T=int(T),
                                      grouped=grouped, pos2col=pos2col, warp=wtab, warp_shift=shift, host_plan_s=t_build)

    @staticmethod
    def auto_align(K, nnz, M, G, rnd, d_piece_bytes=None):
        """How far (in sweep positions) one bin of a wave may run ahead of the slowest: a third of the L2 window.  An
        XCD's 4 MiB hold 4 MiB / piece bytes of B (8,192 pieces of a 128-column pass); the window is that share of the
        nonzeros an XCD gathers in one round of resident tiles, in positions.  S-Reddit: 1,300 positions -> the measured
        default of 2,048 stays; a sparse block of a large graph (S-RMAT 10 M: 24.6 M nonzeros over 10 M columns in ten
        rounds) gets ~90,000 -- aligned to 2,048 COLUMNS its bins were mostly pads."""
        piece = d_piece_bytes or (512 if G == 2 else 256)
        rows_round = max(rnd * 16 * G, 1)
        rounds = max(-(-int(M) // rows_round), 1)
        nnz_xcd_round = max(int(nnz) / rounds / 8.0, 1.0)
        window = float(K) * ((4 << 20) / piece) / nnz_xcd_round
        return int(max(2048, min(0.35 * window, K / 8.0)))

    @staticmethod
    def auto_t(rowptr, G, rnd):
        """The split threshold for a matrix that does not fill its rounds of resident tiles: rows longer than T become
        strided virtual rows, and a block with few rows (an eighth of S-Reddit: 29 k rows against the 65 k / 131 k a round
        holds) leaves most wavefront slots of its launches empty -- its sweep is latency-bound.  0 = the library's default
        (8 x the mean degree, sgcn_csplan.cpp default_t) when the virtual rows it gives fill >= 3/4 of the rounds they
        need; otherwise the smallest T >= 24 whose virtual rows fill 70 % of those rounds (an eighth of S-Reddit, one
        group: T = 400 -> 1.34 ms per fwd + bwd, 100 -> 1.21, 61 (a full round) -> 1.25)."""
        deg = np.diff(np.asarray(rowptr, dtype=np.int64))
        if deg.shape[0] == 0:
            return 0
        avg = int(deg.sum()) // deg.shape[0]
        t0 = int(min(1024, max(64, 8 * avg)))                   # (sgcn_csplan.cpp default_t)
        cap_round = int(rnd) * 16 * max(int(G), 1)

        def vrows(t):
            return int(np.maximum(1, -(-deg // t)).sum())
        v0 = vrows(t0)
        cap = -(-v0 // cap_round) * cap_round
        if v0 >= 0.75 * cap:
            return 0
        return _smallest_t(lambda t: vrows(t) <= 0.7 * cap, 24, t0)

    # ---- a small row block with its rows split BY COLUMN RANGE (round 6) --------------------------------------------------
    RANGE_FILL = 0.95     # virtual rows of a ranged plan: split until they fill this share of one round of resident tiles

    @staticmethod
    def choose_ranges(M, nnz, K, G, rnd=4096):
        """2 when a block is small enough that its rows are split anyway to fill ONE round of resident tiles (auto_t) and
        the 1-D sweep is bound by B crossing the fabric: an XCD holds M / 8 random rows whose nnz / 8 nonzeros touch
        1 - exp(-nnz / 8K) of B's rows (an eighth of S-Reddit: 79 %, 8 x 0.79 x 561 MB = 3.5 GB for 70 MB of output);
        with the rows cut in two column ranges, range j on XCDs 4j .. 4j + 3, an XCD holds M / 4 half-rows on K / 2
        columns: 2.15 GB.  0 otherwise (a quarter of S-Reddit: 2 x 58 k virtual rows do not fit a round, and two rounds
        sweep every range twice)."""
        if G != 1 or M <= 0 or nnz <= 0 or K < 4096:
            return 0
        if 2 * M > ColumnSweepCSR.RANGE_FILL * int(rnd) * 16:
            return 0
        f1 = 1.0 - np.exp(-nnz / 8.0 / K)
        f2 = 0.5 * (1.0 - np.exp(-nnz / 8.0 / (K / 2.0)))
        return 2 if f2 <= 0.75 * f1 else 0

    @staticmethod
    def _plan_ranged(a, NR, T, round_tiles):
        """Rows split by column range instead of by stride: piece j of a row = its nonzeros in columns [cut_j, cut_j+1)
        (ranges of equal nonzeros, cut on warp-bucket boundaries), the pieces of range j form the tiles of XCDs
        [8 j / NR, 8 (j + 1) / NR) (tiles in range order + the launch's tile range cut into eight contiguous pieces:
        xcd_map), and ALL ranges are swept at once on one clock: the warp table maps a column to its position inside its
        range, scaled to [0, K).  A row's pieces meet in the ordered fix-up like strided pieces do (range 0 first):
        deterministic, and nothing in the kernels changes.  Built from the shipped plan builder: the NR column-restricted
        copies of the block stacked as NR x M rows with the range as the row label, then rows and workspace slots renamed."""
        import scipy.sparse as sp
        if not a.has_sorted_indices:         # (a private copy: the caller's matrix is not reordered behind its back)
            a = a.copy()
            a.sort_indices()
        M, K = int(a.shape[0]), int(a.shape[1])
        rowptr = np.ascontiguousarray(a.indptr, dtype=np.int64)
        col = np.ascontiguousarray(a.indices, dtype=np.int32)
        val = np.ascontiguousarray(a.data, dtype=np.float32)
        shift = 0
        while (K >> shift) > ColumnSweepCSR.WARP_BUCKETS:
            shift += 1
        bucket = 1 << shift
        cum = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=K).astype(np.int64))])
        cuts = [0]
        for j in range(1, NR):
            c = int(np.searchsorted(cum, cum[-1] * j // NR))
            cuts.append(max(cuts[-1], min(K, (c + bucket // 2) // bucket * bucket)))
        cuts = np.asarray(cuts + [K], dtype=np.int64)
        rows_of = np.repeat(np.arange(M, dtype=np.int64), np.diff(rowptr))
        rng_id = np.searchsorted(cuts, col, side="right") - 1
        stacked = sp.csr_matrix((val, (rows_of + rng_id * M, col)), shape=(NR * M, K))      # (columns stay sorted inside a row)
        stacked.sort_indices()
        srp = np.ascontiguousarray(stacked.indptr, dtype=np.int32)
        scol = np.ascontiguousarray(stacked.indices, dtype=np.int32)
        sval = np.ascontiguousarray(stacked.data, dtype=np.float32)
        labels = np.ascontiguousarray(np.repeat(np.arange(NR, dtype=np.int32), M))
        sdeg = np.diff(srp.astype(np.int64))
        if not T:      # split further (by stride, inside a range) until the pieces fill RANGE_FILL of one round
            cap = int(ColumnSweepCSR.RANGE_FILL * _cs_round(round_tiles) * 16)
            pieces = lambda t: int(np.maximum(sdeg > 0, -(-sdeg // t)).sum())      # noqa: E731
            hi = int(max(64, sdeg.max() if sdeg.size else 64))
            T = hi if pieces(hi) > cap else _smallest_t(lambda t: pieces(t) <= cap, 24, hi)
        t_build = time.perf_counter()
        built = ColumnSweepCSR._build(srp, scol, sval, NR * M, 1, 16, int(T), 0, 0, labels.ctypes.data, None, 0)
        _, _, _, tile_rows, tile_slots, fix, _, nfix, _ = built
        # ---- rename: stacked row j * M + r -> row r; its workspace slots -> consecutive slots of row r, range by range
        npieces = (sdeg > 0).astype(np.int64)                      # an empty piece takes no slot (and writes nothing)
        old_first = np.full(NR * M, -1, dtype=np.int64)
        if nfix:
            npieces[fix[:, 0]] = fix[:, 2]
            old_first[fix[:, 0]] = fix[:, 1]
        per_row = npieces.reshape(NR, M)
        total = per_row.sum(axis=0)                                # pieces of original row r
        split = total >= 2
        base = np.zeros(M, dtype=np.int64)
        base[split] = np.cumsum(total[split]) - total[split]
        before = np.cumsum(per_row, axis=0) - per_row              # pieces of row r in the ranges in front of j
        new_first = (base[None, :] + before).reshape(-1)           # first new slot of stacked row j * M + r
        tr, ts = tile_rows.astype(np.int64), tile_slots.astype(np.int64)
        valid = tr >= 0
        srow = np.where(valid, tr, 0)
        q = np.where(ts >= 0, ts - old_first[srow], 0)             # piece index inside the stacked row
        orig = srow % M
        # (an empty piece writes nothing -- except range 0's piece of a row that is empty altogether: it is the row's one
        # writer, C[r] = beta * C[r])
        live = valid & ((sdeg[srow] > 0) | ((srow < M) & (total[orig] == 0)))
        new_rows = np.where(live, orig, -1).astype(np.int32)
        new_slots = np.where(live & split[orig], new_first[srow] + q, -1).astype(np.int32)
        rs = np.nonzero(split)[0]
        new_fix = np.stack([rs, base[rs], total[rs]], axis=1).astype(np.int32) if rs.size else np.zeros((0, 3), np.int32)
        t_build = time.perf_counter() - t_build
        # the clock's coordinates: a column's position INSIDE its range, scaled to [0, K) -- every range starts at 0
        nb = -(-K // bucket)
        first = np.arange(nb, dtype=np.int64) * bucket
        rj = np.searchsorted(cuts, first, side="right") - 1
        lo_, hi_ = cuts[rj], cuts[rj + 1]
        table = ((first - lo_) * K // np.maximum(hi_ - lo_, 1)).astype(np.uint32)
        return ColumnSweepCSR._record(built, shape=(M, K), nnz=int(col.shape[0]), T=int(T), ranged=NR,
                                      range_cuts=[int(x) for x in cuts], tile_rows=new_rows, tile_slots=new_slots, fix=new_fix,
                                      nslots=int(total[split].sum()), warp=table, warp_shift=shift, host_plan_s=t_build)

    @staticmethod
    def _plan_groups(a, G, T, round_tiles, align, warp, dictionary=False):
        """G = 2 / 4 lane groups per wavefront (sgcn_csplang_*); ``dictionary``: offered to sgcn_csbuild_dict, which decides"""
        rowptr = np.ascontiguousarray(a.indptr, dtype=np.int32)
        col = np.ascontiguousarray(a.indices, dtype=np.int32)
        val = np.ascontiguousarray(a.data, dtype=np.float32)
        M, K = rowptr.shape[0] - 1, int(a.shape[1])
        rnd = _cs_round(round_tiles)
        if not T:
            T = ColumnSweepCSR.auto_t(rowptr, G, rnd)
        # the clock's coordinates first: the bins of a wave are aligned in them
        wtab, shift = ColumnSweepCSR.make_warp(col, K, warp)
        if align is None or align == 'auto':
            align = ColumnSweepCSR.auto_align(K, col.shape[0], M, G, rnd)
        t_build = time.perf_counter()
        built, (bits, tile_vals, tile_nvals) = ColumnSweepCSR._build(rowptr, col, val, M, G, 16, T, rnd, int(align), None,
                                                                     wtab.ctypes.data if wtab is not None else None, shift,
                                                                     K=K if dictionary else -1)
        t_build = time.perf_counter() - t_build
        return ColumnSweepCSR._record(built, shape=(int(a.shape[0]), K), nnz=int(col.shape[0]), G=G, T=int(T), align=int(align),
                                      pad_fraction=1.0 - col.shape[0] / max(int(built[1].shape[0]), 1), warp=wtab,
                                      warp_shift=shift, host_plan_s=t_build, dict_bits=bits, tile_vals=tile_vals,
                                      tile_nvals=tile_nvals)

    @staticmethod
    def _build(rowptr, col, val, M, G, R, T, rnd, align, rgp, wp, warp_shift, threads=0, K=None):
        """sgcn_csplan_build + export: the plan's host arrays, built in one pass on every core the process may use.
        ``K`` given: the plan is offered to sgcn_csbuild_dict (K < 0: not offered) and the result is the pair
        (arrays, (dict_bits, tile_vals, tile_nvals)) -- a dictionary plan's value array is None."""
        h = C.c_void_p()
        check(lib.sgcn_csplan_build(rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, M, G, R, int(T), int(rnd), int(align),
                                    rgp, wp, int(warp_shift), int(threads), C.byref(h)))
        try:
            nt, ne, nfix, nslots = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
            check(lib.sgcn_csbuild_sizes(h, C.byref(nt), C.byref(ne), C.byref(nfix), C.byref(nslots), None, None))
            bits = C.c_int32(0)
            if K is not None and K >= 0:
                check(lib.sgcn_csbuild_dict(h, int(K), C.byref(bits)))
            tile_ptr = np.empty(nt.value + 1, dtype=np.int64)
            colrow = np.empty(ne.value, dtype=np.int32)
            valout = np.empty(ne.value, dtype=np.float32) if bits.value == 0 else None
            tile_rows = np.empty(nt.value * R * G, dtype=np.int32)
            tile_slots = np.empty(nt.value * R * G, dtype=np.int32)
            fix = np.empty((nfix.value, 3), dtype=np.int32)
            check(lib.sgcn_csbuild_export(h, tile_ptr.ctypes.data, colrow.ctypes.data, valout.ctypes.data if valout is not None else None,
                                          tile_rows.ctypes.data, tile_slots.ctypes.data,
                                          fix.ctypes.data if nfix.value else None))
            tile_vals = tile_nvals = None
            if bits.value:
                tile_vals = np.empty(nt.value << bits.value, dtype=np.float32)
                tile_nvals = np.empty(nt.value, dtype=np.int32)
                check(lib.sgcn_csbuild_export_dict(h, tile_vals.ctypes.data, tile_nvals.ctypes.data))
        finally:
            lib.sgcn_csbuild_free(h)
        built = tile_ptr, colrow, valout, tile_rows, tile_slots, fix, nt.value, nfix.value, nslots.value
        return built if K is None else (built, (bits.value, tile_vals, tile_nvals))

    # ---- on-disk plan cache (beside the dataset's .npz) -------------------------
    @staticmethod
    def matrix_key(a):
        """Cheap identity of a CSR (shape, nnz, CRC of its three arrays): a cached plan is reused only
        for the matrix it was built from."""
        import zlib
        a = a.tocsr()
        crc = 0
        for x in (a.indptr, a.indices, a.data):
            crc = zlib.crc32(np.ascontiguousarray(x).view(np.uint8), crc)
        return "%dx%d:%d:%08x" % (a.shape[0], a.shape[1], a.nnz, crc)

    @staticmethod
    def choose_g(d, avg_degree=None, rows=None):
        """1, 2 or 4 lane groups per wavefront for operands of width d: a G = 2 launch is ~0.73 of a G = 1 launch
        (measured on S-Reddit: 0.323 ms with the packed-FMA kernel vs 0.445 ms) and a plan needs half the rounds of resident tiles, but
        ceil(d / 128) passes over the feature dimension instead of ceil(d / 320).  What two groups buy is fewer
        fabric misses.  A SPARSE matrix with more rows than one round of two-group tiles holds (a GPU's block of
        S-RMAT 10 M / 200 M: 1.05 M rows of 23 nonzeros) takes four: twice the rows -- and nonzeros -- per sweep of B, which
        is what its L2 hits come from (3.16 against 3.49 ms, profiles/r43_warp_probe.jsonl; the same rule as the LDS
        plan's residual)."""
        if avg_degree is not None and avg_degree <= 40 and rows is not None and rows > 4096 * 32:
            return 4
        dp = (int(d) + 3) // 4 * 4
        # (dense graphs follow the same rule since the split threshold doubled: S-Reddit-114M, degree 490, d = 602: two groups
        # 13.0 ms, one 14.0 -- with the old threshold 15.1 vs 14.7; the hub block of S-RMAT 10 M, 334 nonzeros per row,
        # d = 256: 2.04 vs 2.59 ms)
        # rounds of resident tiles: one group holds 65,536 rows per round, two hold 131,072 -- half the rounds for a full
        # graph, but no fewer for a block that fits one round either way (an eighth of S-Reddit, 29 k rows, d = 602: two
        # passes of one group 1.34 ms per fwd + bwd, five passes of two groups 1.72)
        r1 = r2 = None
        if rows is not None and rows > 0:
            r1, r2 = -(-int(rows) // (4096 * 16)), -(-int(rows) // (4096 * 32))
        if r1 is None:
            r1, r2 = 2, 1
        return 2 if -(-dp // 128) * 0.73 * r2 <= -(-dp // 320) * r1 else 1

    def save(self, path, key):
        if self.grouped or self.ranged:
            raise ValueError("grouped / column-range plans are not cached (they are cheap to rebuild)")
        t = lambda x: x.cpu().numpy()          # noqa: E731
        blob = dict(key=np.array(key), G=self.G, pad_fraction=float(self.pad_fraction),
                    R=self.R, shape=np.array(self.shape, np.int64), nslots=self.nslots,
                    round_tiles=self.round_tiles, tile_ptr=t(self.tile_ptr), colrow=t(self.colrow),
                    val=t(self._val) if self.dict_bits == 0 else np.zeros(0, np.float32),
                    tile_rows=t(self.tile_rows), tile_slots=t(self.tile_slots),
                    fix=t(self.fix) if self.fix is not None else np.zeros((0, 3), np.int32),
                    warp=t(self.warp) if self.warp is not None else np.zeros(0, np.int32), warp_shift=self.warp_shift)
        if self.dict_bits:       # (a plan with a value array writes the file it always wrote)
            blob.update(dict_bits=self.dict_bits, tile_vals=t(self.tile_vals), tile_nvals=t(self.tile_nvals))
        # each operand type's clocks under keys of their own: a build without the bfloat16 operand reads the rest unchanged
        for clock, (pace_key, tuned_key) in zip(self._clocks, self.CLOCK_KEYS):
            blob[pace_key], blob[tuned_key] = clock.to_npz()
        import os
        import tempfile
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        # every rank of a data-parallel job may get here at the same time: each writes its OWN temporary
        # file (same directory, so the rename stays atomic) and the last complete one wins
        fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=os.path.dirname(path) or ".")
        try:
            with os.fdopen(fd, "wb") as f:
                np.savez(f, **blob)
            os.replace(tmp, path)
        except BaseException:
            try:
                os.unlink(tmp)
            except OSError:
                pass
            raise

    @classmethod
    def load(cls, path, device, key, g=None):
        """The plan cached at ``path`` if it was built from the matrix ``key`` identifies (and with ``g`` lane
        groups, when given), else None."""
        import os
        if not os.path.exists(path):
            return None
        try:
            return cls._load(path, device, key, g)
        except Exception:            # truncated / corrupt / foreign file: a cache miss, never a crash at startup
            return None

    @classmethod
    def _load(cls, path, device, key, g):
        z = np.load(path)
        if str(z["key"]) != key:
            return None
        G = int(z["G"]) if "G" in z.files else 1
        if g is not None and G != g:
            return None
        warp = z["warp"] if "warp" in z.files and z["warp"].shape[0] else None
        p = dict(cls._RECORD, G=G, R=int(z["R"]), shape=tuple(int(x) for x in z["shape"]), nnz=int(z["colrow"].shape[0]),
                 pad_fraction=float(z["pad_fraction"]) if "pad_fraction" in z.files else 0.0, nslots=int(z["nslots"]),
                 warp=warp, warp_shift=int(z["warp_shift"]) if warp is not None else 0,
                 **{k: z[k] for k in ("tile_ptr", "colrow", "val", "tile_rows", "tile_slots", "fix")})
        if "dict_bits" in z.files and int(z["dict_bits"]):
            p.update(val=None, dict_bits=int(z["dict_bits"]), tile_vals=z["tile_vals"], tile_nvals=z["tile_nvals"])
        self = cls.__new__(cls)
        self._finish(p, device, int(z["round_tiles"]), tuple(SweepClock.from_npz(z, *keys) for keys in cls.CLOCK_KEYS))
        return self

    @classmethod
    def cached(cls, a, device, path=None, G=1, dictionary=True):
        """Plan of ``a`` (with G lane groups per wavefront): loaded from ``path`` when that file holds such a
        plan of this very matrix, otherwise built (and written to ``path``).  Returns (plan, came_from_cache)."""
        if path is None:
            return cls(a, device, G=G, dictionary=dictionary), False
        # the identity of the matrix AND of the build parameters the plan depends on (tiles per launch round)
        # (cached() builds with the default T / align; d: how the rows were dealt to the bins, sgcn_tune "cs_deal")
        key = "%s:r%d:Tauto:aauto:w1:d%d" % (cls.matrix_key(a), _cs_round(), _ffi.lib.sgcn_tune_get(b"cs_deal"))
        if dictionary and _ffi.lib.sgcn_tune_get(b"cs_dict") > 0:     # (v: the plan was offered to sgcn_csbuild_dict)
            key += ":v1"
        hit = cls.load(path, device, key, g=G)
        if hit is not None:
            return hit, True
        plan = cls(a, device, G=G, dictionary=dictionary)
        plan._cache = (path, key)
        return plan, False

    def store_if_cached(self):
        """Write the plan (with the paces autotuned so far) to the path ``cached`` was given."""
        if self._cache is not None:
            try:
                self.save(*self._cache)
            except OSError:           # read-only dataset directory: the cache is an optimisation only
                pass

    def struct(self, d, bf16=False):
        """The C struct for a product of width d; ``bf16``: with the clock tuned for a bfloat16 operand."""
        self.ws = _fixup_ws(self.ws, self.nslots, d, self.device)
        rnd = _cs_round(self.round_tiles)
        if self._hint_round != rnd:         # heaviest tile of every launch, for pacing
            nl = -(-self.ntiles // rnd)
            pad = np.zeros(nl * rnd, dtype=np.int64)
            pad[:self.ntiles] = self._tile_nnz
            self._hint = np.ascontiguousarray(pad.reshape(nl, rnd).max(axis=1))
            self._hint_round = rnd
        colrow, tables = self.colrow, (self.tile_vals, self.tile_nvals, self.dict_bits)
        if self.dict_bits and self.live_val is not None:
            # a value array handed to a dictionary plan: the product reads it, on the words without their table indices
            # (made once; a plan that is to be re-valued every step is better built with dictionary=False)
            if self._colrow_plain is None:
                self._colrow_plain = torch.from_numpy(np.ascontiguousarray(self.columns_rows())).to(self.device)
            colrow, tables = self._colrow_plain, (None, None, 0)
        return _ffi.CsPlan(self.R, self.ntiles, self.tile_ptr.data_ptr(), colrow.data_ptr(),
                           _ptr(self._val if self.live_val is None else self.live_val), self.tile_rows.data_ptr(),
                           self.tile_slots.data_ptr(),
                           _ptr(self.fix), self.nfix, self.nslots, _ptr(self.ws),
                           0 if self.ws is None else self.ws.numel(), rnd, self._hint.ctypes.data,
                           -1 if self.grouped else int(self.clock(bf16).pace.get(d, 0)), self.G,
                           1 if (self.grouped or self.ranged) else 0, _ptr(self.warp), self.warp_shift,
                           _ptr(tables[0]), _ptr(tables[1]), tables[2])

    def variant(self, d, bf16=False):
        """The kernel variant / launch geometry sgcn_spmm_cs_f32 (``bf16``: sgcn_spmm_cs_b16) uses for this plan and width."""
        buf = C.create_string_buffer(256)
        plan = self.struct(d, bf16)
        check((lib.sgcn_spmm_cs_variant_b16 if bf16 else lib.sgcn_spmm_cs_variant)(C.byref(plan), int(d), buf, 256))
        return buf.value.decode()

    def autotune(self, B, d=None, candidates=None, reps=2, refine=True):
        """Pick the sweep clock for this plan and row width by timing a few candidates (the
        sustainable pace depends on the graph, d and the chip's clocks; too fast loses the
        lock-step and with it the L2 hits, too slow leaves the memory system idle).  The clock is tuned for the TYPE of
        the operand it is handed: a bfloat16 ``B`` tunes ``pace_b16`` and leaves the fp32 clock alone."""
        d = int(B.shape[1] if d is None else d)
        self._tuning = True
        try:
            return self._autotune(B, d, candidates, reps, refine)
        finally:
            self._tuning = False

    def _autotune(self, B, d, candidates, reps, refine):
        if candidates is None:           # ns per step of the heaviest tile (a G = 2 step is one load for two nonzeros)
            candidates = (-1, 230, 250, 270, 290, 310, 340, 380) if self.ranged else \
                (-1, 200, 220, 240, 260, 280, 320, 380) if self.G == 1 else \
                (-1, 130, 160, 190, 210, 230, 250, 280, 320)
        clock = self.clock(B.dtype == torch.bfloat16)
        pace_of, tuned_of, guard_of = clock.pace, clock.tuned_ms, clock.guard
        if self.grouped:                 # grouped plans run unpaced (see the class docstring)
            pace_of[d] = -1
            return (None, -1)
        out = _pitched_out(self.shape[0], d, B.device)
        def timed(p, reps=reps):
            pace_of[d] = p
            spmm_cs(self, B, out=out, d=d)                       # warm
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                spmm_cs(self, B, out=out, d=d)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / reps

        best = None
        for p in candidates:
            t = timed(p)
            if best is None or t < best[0]:
                best = (t, p)
        # a winner at the slow end of the list: the optimum may lie beyond it (sparse blocks of large graphs, whose steps
        # mostly miss the L2: S-RMAT 10 M, 360 - 400 ns per step) -- keep slowing the clock while that pays
        ext = 0
        while refine and best[1] > 0 and best[1] == max(candidates) and best[1] < 2000 and ext < 8:
            ext += 1                                  # (bounded: timing noise must not decide when this ends)
            p = max(best[1] + 1, int(best[1] * 1.15))
            candidates = tuple(candidates) + (p,)
            t = timed(p)
            if t < best[0]:
                best = (t, p)
        if refine and best[1] > 0:
            # The optimum sits right above a cliff (too fast a clock and the waves lose the lock-step for good),
            # and a two-launch burst tolerates a faster clock than a sustained run does (measured: 268 ns wins the
            # burst, 7.5 ms per fwd+bwd sustained; 274 ns: 7.2; 280: 7.4).  So: a finer look around the coarse
            # winner, then a 2 % guard band above the fastest clock that held.
            for p in sorted({int(best[1] * f) for f in (0.94, 0.96, 0.98, 1.02)} - set(candidates)):
                t = timed(p)
                if t < best[0]:
                    best = (t, p)
            # (round 4: 1 % instead of 2 -- the product costs 3.17 ms at 193 ns, 3.22 at 197, 3.39 at 189,
            # profiles/r27_headline_knobs.jsonl -- now that a lost lock-step is detected and re-tuned at run time: _guard_*)
            best = (best[0], int(best[1] * 1.01 + 0.5))
            # ... and a sustained check of the choice: a run of back-to-back products must not cost more than the
            # burst did (a lost lock-step costs 60 %, not a few); if it does, back the clock off in 4 % steps
            burst = best[0]
            for _ in range(4):
                t = timed(best[1], reps=6)
                if t <= 1.06 * burst:
                    best = (t, best[1])
                    break
                best = (t, int(best[1] * 1.04 + 0.5))
        pace_of[d] = best[1]
        tuned_of[d] = float(best[0])
        guard_of.pop(d, None)
        return best

    # ---- lost-lock guard ----------------------------------------------------------------------------
    # The clock-paced sweep is tuned once per plan and width; a pace that has become too fast (another box, a clock or
    # thermal change) loses the lock-step for good and the product costs ~2x, silently.  Every GUARD_EVERY-th product
    # of a tuned plan is timed with a pair of events that are read back -- without waiting -- by a later call; two
    # samples in a row above GUARD_FACTOR x the tuned time re-run the autotune on that call's operand.
    GUARD_EVERY = 8
    GUARD_FACTOR = 1.3
    guard_on = True       # False (per plan): no samples and no re-tunes, e.g. inside a measurement's timed windows

    def _guard_before(self, d, bf16=False):
        """Called by spmm_cs ahead of the launches: returns the event pair to record around them, or None."""
        clock = self.clock(bf16)
        if self.grouped or clock.pace.get(d, 0) <= 0 or d not in clock.tuned_ms:
            return None
        g = clock.guard.setdefault(d, {"calls": 0, "pending": None, "strikes": 0, "retunes": 0, "last_ms": None})
        g["calls"] += 1
        if g["pending"] is not None or g["calls"] % self.GUARD_EVERY:
            return None
        g["pending"] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        return g["pending"]

    def _guard_after(self, d, B):
        """Called by spmm_cs behind the launches: reads a finished sample, re-tunes after two slow ones in a row."""
        clock = self.clock(B.dtype == torch.bfloat16)
        tuned_of, guard_of = clock.tuned_ms, clock.guard
        g = guard_of.get(d)
        if g is None or g["pending"] is None or not g["pending"][1].query():
            return
        e0, e1 = g["pending"]
        g["pending"] = None
        g["last_ms"] = e0.elapsed_time(e1)
        if g["last_ms"] > self.GUARD_FACTOR * tuned_of[d]:
            g["strikes"] += 1
        else:
            g["strikes"] = 0
        if g["strikes"] >= 2:
            n = g["retunes"] + 1
            self.autotune(B, d=d)                      # (resets the guard's state for d)
            guard_of[d] = {"calls": 0, "pending": None, "strikes": 0, "retunes": n, "last_ms": None}


def spmm_cs(A, B, out=None, gidx=None, rscale=None, cscale=None, beta=0.0, d=None):
    """Column-sweep variant of ``spmm`` for a ColumnSweepCSR (sgcn_spmm_cs_f32; sgcn_spmm_cs_b16 on a bfloat16 ``B``, with
    the plan's clock for that operand type)."""
    M, K = A.shape
    bptr, ldb, b16 = _hist2d(B, "B")
    d = int(B.shape[1] if d is None else d)
    if out is None:
        out = _pitched_out(M, d, B.device, beta)
    cptr, ldc = _rows2d(out, "out")
    plan = A.struct(d, b16)
    if A.pos2col is not None:        # the plan's columns are sweep positions: B row = pos2col[position]
        if cscale is not None:
            raise ValueError("a grouped column-sweep plan does not take cscale (scale B instead)")
        gidx = A.pos2col if gidx is None else _dev(gidx, torch.int32, "gidx")[A.pos2col.long()]
    gp, rp, cp = _ptr(_dev(gidx, torch.int32, "gidx")), _ptr(_dev(rscale, torch.float32, "rscale")), \
        _ptr(_dev(cscale, torch.float32, "cscale"))
    watch = A.guard_on and not A._tuning
    ev = A._guard_before(d, b16) if watch else None
    if ev is not None:
        ev[0].record()
    try:
        check((lib.sgcn_spmm_cs_b16 if b16 else lib.sgcn_spmm_cs_f32)(C.byref(plan), M, K, d, bptr, ldb, gp, rp, cp, cptr, ldc, float(beta), _stream()))
        if ev is not None:
            ev[1].record()
    except BaseException:
        if ev is not None:          # a sample whose second event was never recorded must not stay pending
            A.clock(b16).guard[d]["pending"] = None
        raise
    if watch and A.clock(b16).guard:
        A._guard_after(d, B)
    return out


# ---- LDS-staged column sweep for graphs with locality (sgcn_spmm_lds.hip) --------------------------
class LdsPlanHost(object):
    """The host arrays of an LDS-sweep plan (include/sgcn.h sgcn_ldsplan_*): what ``LdsSweepCSR`` uploads, and what
    the CPU tests decode (``decode`` rebuilds the planned matrix from the kernel's own operands)."""

    def __init__(self, a, labels=None, VW=2, T=0, min_reuse=2, general=False, ring_slots=0):
        a = a.tocsr()
        rowptr = np.ascontiguousarray(a.indptr, dtype=np.int32)
        col = np.ascontiguousarray(a.indices, dtype=np.int32)
        val = np.ascontiguousarray(a.data, dtype=np.float32)
        M, K = int(a.shape[0]), int(a.shape[1])
        # One value per COLUMN (the transpose of a row-normalised adjacency: the backward of a mean aggregation) and not one
        # per row: the plan is built on the pattern -- a unit plan -- and the values become a scale of the operand's rows
        # (``col_fold``; ops.spmm_lds multiplies B by it first: M . B = pattern(M) . (col_fold (.) B)).
        self.col_fold = None
        if not general and val.shape[0]:
            vb = val.view(np.int32)
            first = np.zeros(M, dtype=np.int32)
            nz = np.diff(rowptr) > 0
            first[nz] = vb[rowptr[:-1][nz]]
            row_unit = bool(np.all(vb == np.repeat(first, np.diff(rowptr))))
            if not row_unit:
                cf = np.zeros(K, dtype=np.int32)
                cf[col] = vb                                   # (any nonzero of the column: all equal, or the check fails)
                if bool(np.all(cf[col] == vb)):
                    self.col_fold = np.where(np.bincount(col, minlength=K) > 0, cf, np.float32(1.0).view(np.int32)).view(np.float32)
                    val = np.ones_like(val)
        col_pos = row_group = None
        if labels is not None:
            row_labels, col_labels = labels if isinstance(labels, tuple) else (labels, labels)
            if col_labels is not None:
                col_labels = np.ascontiguousarray(col_labels, dtype=np.int32)
                if col_labels.shape[0] != K:
                    raise ValueError("one label per column")
                pos2col = np.argsort(col_labels, kind='stable').astype(np.int32)        # sweep position -> column
                col_pos = np.empty_like(pos2col)
                col_pos[pos2col] = np.arange(K, dtype=np.int32)
            if row_labels is not None:
                row_group = np.ascontiguousarray(row_labels, dtype=np.int32)
                if row_group.shape[0] != M:
                    raise ValueError("one label per row")
        h = C.c_void_p()
        check(lib.sgcn_ldsplan_create(rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, M, K,
                                      col_pos.ctypes.data if col_pos is not None else None,
                                      row_group.ctypes.data if row_group is not None else None,
                                      int(VW), int(T), int(min_reuse), 1 if general else 0, int(ring_slots), C.byref(h)))
        try:
            sizes = np.zeros(19, dtype=np.int64)
            check(lib.sgcn_ldsplan_sizes(h, sizes.ctypes.data))
            nt, nch, nent, nfix, nslots, rnnz, staged, unit = (int(x) for x in sizes[:8])
            self.xcd_tile_ptr = [int(x) for x in sizes[8:17]]
            self.VW, self.NW, self.RW, self.S, self.U, self.unit = int(VW), 8, 192 // int(VW), int(sizes[17]), 8, unit
            self.nparts = int(sizes[18])
            R = self.NW * self.RW
            self.tile_chunk_ptr = np.empty(nt + 1, dtype=np.int32)
            self.chunk_cols = np.empty(nch * self.S, dtype=np.int32)
            self.chunk_hdr = np.empty(nch * self.NW * 32, dtype=np.int32)
            self.ent_ptr = np.empty(nch * self.NW + 1, dtype=np.int64)
            self.words = np.empty(nent + 256, dtype=np.uint32)
            self.vals = np.empty(nent + 256, dtype=np.float32)
            self.row_fold = np.empty(M, dtype=np.float32)
            self.tile_rows = np.empty(nt * R, dtype=np.int32)
            self.tile_slots = np.empty(nt * R, dtype=np.int32)
            self.fix = np.empty((nfix, 3), dtype=np.int32)
            res_rowptr = np.empty(M + 1, dtype=np.int32)
            res_col = np.empty(rnnz, dtype=np.int32)
            res_val = np.empty(rnnz, dtype=np.float32)
            check(lib.sgcn_ldsplan_export(h, self.tile_chunk_ptr.ctypes.data, self.chunk_cols.ctypes.data,
                                          self.chunk_hdr.ctypes.data, self.ent_ptr.ctypes.data, self.words.ctypes.data, self.vals.ctypes.data,
                                          self.row_fold.ctypes.data if M else None, self.tile_rows.ctypes.data,
                                          self.tile_slots.ctypes.data, self.fix.ctypes.data if nfix else None,
                                          res_rowptr.ctypes.data, res_col.ctypes.data if rnnz else None,
                                          res_val.ctypes.data if rnnz else None))
        finally:
            lib.sgcn_ldsplan_destroy(h)
        import scipy.sparse as sp
        self.shape = (M, K)
        self.ntiles, self.nchunks, self.nent, self.nfix, self.nslots, self.staged = nt, nch, nent, nfix, nslots, staged
        self.nnz = int(a.nnz)
        self.residual = sp.csr_matrix((res_val, res_col, res_rowptr), shape=(M, K))
        self.local_nnz = self.nnz - rnnz

    def planned(self):
        """(row, column, value, workspace slot) as ``decode``, with the column values folded back in."""
        r, c, v, sl = self.decode()
        return (r, c, v * self.col_fold[c], sl) if self.col_fold is not None else (r, c, v, sl)

    def decode(self):
        """(row, column, value, workspace slot) of every non-pad entry, read back from the kernel's operands: the ring
        slot of an entry's LDS address -> ``chunk_cols``, its register offset -> ``tile_rows``."""
        piece = 256 * self.VW
        part = self.S * piece
        rows, cols, vals, slots = [], [], [], []
        for t in range(self.ntiles):
            cb, ce = int(self.tile_chunk_ptr[t]), int(self.tile_chunk_ptr[t + 1])
            nc = ce - cb
            for w in range(self.NW):
                base = cb * self.NW + w * nc
                for k in range(nc):
                    e0, e1 = int(self.ent_ptr[base + k]), int(self.ent_ptr[base + k + 1])
                    hd = self.chunk_hdr[((cb + k) * self.NW + w) * 32:((cb + k) * self.NW + w + 1) * 32]
                    per = self.S // self.NW
                    assert np.array_equal(hd[:per], self.chunk_cols[(cb + k) * self.S + w * per:(cb + k) * self.S + (w + 1) * per])
                    assert hd[16] * self.U == e1 - e0 and (int(hd[17]) & 0xffffffff) | (int(hd[18]) << 32) == e0
                    if e1 == e0:
                        continue
                    assert (e1 - e0) % self.U == 0 and e1 - e0 <= (256 if self.unit else 128)
                    word = self.words[e0:e1]
                    addr = word & np.uint32(0x0003fe00)           # (the kernel's mask: LDS address bits of a 512-byte piece)
                    real = addr != self.nparts * part             # pads sit on the zero piece
                    assert self.unit or np.all(self.vals[e0:e1][~real] == 0)
                    assert np.all(addr[real] // part == k % self.nparts), "entry in the wrong part of the ring"
                    npair = int(hd[19]) * self.U                  # the first words of a unit plan's chunk carry TWO rows
                    assert 0 <= npair <= min(e1 - e0, 128) and (self.unit or npair == 0)
                    assert np.all(word[npair:] >> np.uint32(24) == 0)
                    for second in (False, True):
                        sel = real.copy()
                        if second:
                            sel[npair:] = False
                        if not sel.any():
                            continue
                        slot = (addr[sel] % part) // piece
                        lr = ((word[sel] >> np.uint32(24)) if second else (word[sel] & np.uint32(0xff))) // self.VW
                        place = (t * self.NW + w) * self.RW + lr.astype(np.int64)
                        rows.append(self.tile_rows[place])
                        slots.append(self.tile_slots[place])
                        cols.append(self.chunk_cols[(cb + k) * self.S + slot.astype(np.int64)])
                        # (unit plans: the value lives once per row, row_fold -- the words' value slots are not used)
                        vals.append(self.row_fold[self.tile_rows[place]] if self.unit else self.vals[e0:e1][sel])
        cat = lambda x, dt: np.concatenate(x) if x else np.zeros(0, dtype=dt)          # noqa: E731
        return cat(rows, np.int32), cat(cols, np.int32), cat(vals, np.float32), cat(slots, np.int32)


class LdsSweepCSR(object):
    """A static CSR re-laid for the LDS-staged column sweep (sgcn_spmm_lds.hip): for graphs whose rows share columns
    inside a tile of 768 rows (communities; ``labels`` = community per vertex, e.g. from ``reorder_labels``).  The
    nonzeros whose column a tile references fewer than ``min_reuse`` times are multiplied by the ordinary column sweep
    (``self.residual``: a ColumnSweepCSR) into the same output."""

    def __init__(self, a, device, labels=None, VW=2, T=0, min_reuse=2, residual_G=4, host=None, general=False, ring_slots=0,
                 residual_align=8192):
        h = host if host is not None else LdsPlanHost(a, labels=labels, VW=VW, T=T, min_reuse=min_reuse, general=general,
                                                      ring_slots=ring_slots)
        self.host_stats = dict(ntiles=h.ntiles, nchunks=h.nchunks, nent=h.nent, staged=h.staged, nnz=h.nnz,
                               local_nnz=h.local_nnz, pad_fraction=1.0 - h.local_nnz / max(h.nent, 1), unit=h.unit,
                               reuse=h.local_nnz / max(h.staged, 1))
        self.shape, self.nnz, self.device = h.shape, h.nnz, device
        self.VW, self.NW, self.RW, self.S, self.U, self.unit, self.nparts = h.VW, h.NW, h.RW, h.S, h.U, h.unit, h.nparts
        self.xcd_tile_ptr = list(h.xcd_tile_ptr)
        self.ntiles, self.nchunks, self.nent, self.nfix, self.nslots = h.ntiles, h.nchunks, h.nent, h.nfix, h.nslots
        to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)          # noqa: E731
        self.tile_chunk_ptr, self.chunk_cols, self.chunk_hdr = to(h.tile_chunk_ptr), to(h.chunk_cols), to(h.chunk_hdr)
        self.ent_ptr, self.words = to(h.ent_ptr), to(h.words.view(np.int32))
        self.vals = None if h.unit else to(h.vals)
        self.row_fold = to(h.row_fold) if h.unit else None
        self.tile_rows, self.tile_slots = to(h.tile_rows), to(h.tile_slots)
        self.fix = to(h.fix) if h.nfix else None
        self.ws = None
        self.col_fold = to(h.col_fold) if h.col_fold is not None else None       # scale of the operand's rows (see LdsPlanHost)
        self._scaled = None
        self.residual = None
        if h.residual.nnz:
            # four lane groups per wave: the residual's rows are all resident in ONE round of tiles, and a sparse residual is
            # bound by the bytes each XCD pulls over the fabric, not by the step's instructions (S-Reddit-SBM p_in 0.8, 5.0 M
            # nonzeros, sustained: 1.26 ms against 1.50 with two groups; bins aligned to 8,192 columns: profiles/r31_*)
            if residual_G == 4 and h.residual.nnz > 40 * max(h.shape[0], 1):
                residual_G, residual_align = 2, 2048       # a DENSE residual (most of the graph) is the full-graph case: two groups
            # (long residual rows are split at 256 nonzeros, not at the plan's default 8 x the mean row: fewer fix-up slots,
            # the same heaviest bin -- 1.275 -> 1.242 ms, profiles/lds_residual_probe.py 0.8 T)
            self.residual = ColumnSweepCSR(h.residual, device, G=residual_G, align=residual_align,
                                           T=256 if residual_G == 4 else 0) if residual_G else \
                DeviceCSR.from_scipy(h.residual, device)

    def struct(self, d):
        self.ws = _fixup_ws(self.ws, self.nslots, d, self.device)
        return _ffi.LdsPlan(self.VW, self.NW, self.RW, self.S, self.U, self.nparts, self.unit, (C.c_int32 * 9)(*self.xcd_tile_ptr),
                            self.ntiles, self.nchunks, self.nent,
                            self.tile_chunk_ptr.data_ptr(), self.chunk_cols.data_ptr(), self.chunk_hdr.data_ptr(),
                            self.ent_ptr.data_ptr(), self.words.data_ptr(), _ptr(self.vals), _ptr(self.row_fold),
                            self.tile_rows.data_ptr(), self.tile_slots.data_ptr(),
                            _ptr(self.fix), self.nfix, self.nslots, _ptr(self.ws),
                            0 if self.ws is None else self.ws.numel())

    @classmethod
    def for_graph(cls, a, device, min_local=0.6, min_gain=3.0, min_reuse=3):
        """The LDS-sweep plan of a square adjacency IF the graph has the locality that pays for it, else None: communities
        from label propagation on the graph itself (``reorder_labels``), and a plan whose staged pieces serve at least
        ``min_gain`` nonzeros each while leaving at most 1 - ``min_local`` of the nonzeros to the residual sweep (measured
        on S-Reddit-SBM, profiles/r31_*: with 74 % of the nonzeros planned the two-kernel product takes 2.60 ms against 3.20
        for the plain column sweep, with 91 % 2.09 against 3.15; with 40 % the two draw level, 3.21; with 11-14 % it loses,
        3.6-3.7 against 3.2).  A graph without structure (S-Reddit: one label) costs the 0.3 s of the propagation."""
        a = a.tocsr()
        if a.shape[0] != a.shape[1] or a.nnz == 0:
            return None
        labels, ncomm = reorder_labels(a)
        if ncomm < 4:
            return None
        host = LdsPlanHost(a, labels=labels, min_reuse=min_reuse)
        if host.local_nnz < min_local * a.nnz or host.local_nnz < min_gain * host.staged:
            return None
        return cls(a, device, host=cls.auto_host(a, labels, host))

    # A residual costs ten launches and a sweep of B through every XCD however few nonzeros it has; below this share of the
    # nonzeros it is cheaper to stage EVERY column through the ring, single-use pieces included (no residual, no second
    # kernel).  Measured on S-Reddit-SBM, min_reuse 1 against 3 (profiles/r36_*): p_in 0.95 (9 % residual) 1.74 against
    # 2.09 ms, 0.9 (13 %) 2.09 / 2.17, 0.85 (19 %) 2.40 / 2.31, 0.8 (26 %) 2.69 / 2.44.
    ALL_STAGED_BELOW = 0.16

    @classmethod
    def auto_host(cls, a, labels, host=None, min_reuse=3):
        """The host plan for ``a``: ``min_reuse`` 3, or 1 (everything through the ring) when that leaves a small residual."""
        if host is None:
            host = LdsPlanHost(a, labels=labels, min_reuse=min_reuse)
        if 0 < host.residual.nnz < cls.ALL_STAGED_BELOW * max(a.nnz, 1):
            host = LdsPlanHost(a, labels=labels, min_reuse=1)
        return host

    def variant(self, d):
        """What spmm_lds dispatches for this plan and width, as text (bench.py: roofline.kernel)."""
        nslab = (int(d) + 127) // 128
        txt = ("sgcn::lds_spmm_kernel<%d, %d, %s> x 1 launch (%d tiles of 768 rows x %d passes of 128 columns = %d workgroups; "
               "%d chunks, %.1f nonzeros per staged piece, %.1f %% of the nonzeros)"
               % (self.S, self.nparts, "true" if self.unit else "false", self.ntiles, nslab, self.ntiles * nslab, self.nchunks,
                  self.host_stats["reuse"], 100.0 * self.host_stats["local_nnz"] / max(self.nnz, 1)))
        if isinstance(self.residual, ColumnSweepCSR):
            txt += " + residual: " + self.residual.variant(d)
        return txt

    def autotune(self, B, d=None):
        """The residual's sweep clock (the LDS kernel itself is not clock-paced).  (Running the two kernels side by side
        on split compute units -- CU-masked streams -- was measured and lost: profiles/r24_lds_side_by_side_probe.jsonl.)"""
        if isinstance(self.residual, ColumnSweepCSR):
            return self.residual.autotune(B, d=d)
        return None


def spmm_lds(A, B, out=None, rscale=None, beta=0.0, d=None, local_only=False):
    """C = rscale (.) (A B) + beta C for an LdsSweepCSR: the planned nonzeros through the LDS ring
    (sgcn_spmm_lds_f32), then the residual on top (column sweep with beta = 1)."""
    M, K = A.shape
    bptr, ldb = _rows2d(B, "B")
    d = int(B.shape[1] if d is None else d)
    if out is None:
        out = _pitched_out(M, d, B.device, beta)
    cptr, ldc = _rows2d(out, "out")
    if A.col_fold is not None:               # one value per column: B's rows take it (one pass over B), the plan is a unit plan
        pitch = (d + 31) // 32 * 32               # rows on 128-byte lines: a piece of a row never straddles one more line than it must
        if A._scaled is None or A._scaled.shape[0] < K or A._scaled.shape[1] != pitch:
            A._scaled = torch.empty((K, pitch), dtype=torch.float32, device=B.device)
        check(lib.sgcn_scale_rows_f32(bptr, ldb, A.col_fold.data_ptr(), K, d, A._scaled.data_ptr(), pitch, _stream()))
        B = A._scaled[:K, :d]
        bptr, ldb = _rows2d(B, "B")
    plan = A.struct(d)
    check(lib.sgcn_spmm_lds_f32(C.byref(plan), M, K, d, bptr, ldb, _ptr(_dev(rscale, torch.float32, "rscale")),
                                cptr, ldc, float(beta), _stream()))
    if A.residual is not None and not local_only:
        if isinstance(A.residual, ColumnSweepCSR):
            spmm_cs(A.residual, B, out=out, rscale=rscale, beta=1.0, d=d)
        else:
            spmm(A.residual, B, out=out, rscale=rscale, beta=1.0, d=d)
    return out


# ---- fp32 MFMA GEMM / fused dense layer (sgcn_gemm.hip) ------------------------------------------
# Every dense product of the model runs on this library's own kernel, whatever its size (round 3: the size-keyed
# rocBLAS path above 512 M multiply-adds -- Exact-mode and large evaluation batches -- is gone: one code path; the
# kernel is a plain tiled GEMM with split-K, so a 233 k-row operand is just more workgroups).


_GEMM_WS = {}


def _gemm_ws(floats, device):
    """Split-K scratch, one growing buffer per device (all launches share one stream, so the
    next GEMM cannot overwrite partials the previous reduce has not consumed)."""
    w = _GEMM_WS.get(device)
    if w is None or w.numel() < floats:
        w = torch.empty(max(floats, 1 << 20), dtype=torch.float32, device=device)
        _GEMM_WS[device] = w
    return w


def dense_bwd(dy, y, ctx, scale, relu, x, W, dW, doffset=None, dscale=None, need_dx=True, drop=None):
    """Backward of ``dense_fwd`` in one call (sgcn_dense_bwd_f32): accumulates dW (and the LayerNorm
    parameter gradients), returns dx or None.  ``x`` is the UNdropped layer input; ``drop`` the
    dropout site that was applied to it in the forward."""
    gidx = None
    if isinstance(x, GatheredRows):
        x, gidx = x.src, x.idx
    n, N, K = int(dy.shape[0]), int(dy.shape[1]), int(x.shape[1])
    norm = ctx is not None
    gp, ldg = _rows2d(dy, "dy")
    xp, ldx = _rows2d(x, "x")
    wp, ldw = _rows2d(W, "W")
    dwp, lddw = _rows2d(dW, "dW")
    pre = norm or bool(relu)
    yp, ldy = _rows2d(y, "y") if pre else (None, 0)
    g_tmp = torch.empty((n, N), dtype=torch.float32, device=dy.device) if pre else None
    dx = torch.empty((n, K), dtype=torch.float32, device=dy.device) if need_dx else None
    # (the split-K factors, hence the sizes, follow the knob gemm_min_steps: a size cached under another value of it is short)
    key = (n, N, K, norm, int(lib.sgcn_tune_get(b"gemm_min_steps")))
    need = _DENSE_BWD_WS.get(key)
    if need is None:
        need = ((int(lib.sgcn_ln_act_bwd_ws_floats(n, N)) + 3) // 4 * 4 if norm else 0) + \
            max(int(lib.sgcn_gemm_ws_floats(K, N, n)), int(lib.sgcn_gemm_ws_floats(n, K, N)))
        if len(_DENSE_BWD_WS) < 4096:
            _DENSE_BWD_WS[key] = need
    ws = _gemm_ws(need, dy.device) if need else None
    dr = C.byref(drop.struct(K)) if drop is not None else None
    check(lib.sgcn_dense_bwd_f32(n, N, K, gp, ldg, yp, ldy, _ptr(ctx[0]) if norm else None,
                                 _ptr(ctx[1]) if norm else None, _ptr(scale) if norm else None,
                                 int(bool(relu)), xp, ldx, wp, ldw, dwp, lddw, _ptr(doffset), _ptr(dscale),
                                 _ptr(dx), K, dr, _ptr(g_tmp), _ptr(ws), _ptr(gidx), _stream()))
    return dx


_DENSE_BWD_WS = {}


# ---- counter-based dropout (include/sgcn.h sgcn_dropout_t) ---------------------------------------
def _fmix32(h):
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def dropout_key(seed, layer_index, step):
    """The 32-bit key of one dropout site at one step: a hash of (seed, layer index, step)."""
    return _fmix32(_fmix32(int(seed) * 0x9E3779B1 + int(layer_index) * 0x85EBCA77 + 0x27D4EB2F)
                   + int(step) * 0xC2B2AE3D)


class Drop(object):
    """One dropout site: (keep, key) + the activation geometry the mask is defined on."""
    __slots__ = ("keep", "key")

    def __init__(self, keep, key):
        self.keep, self.key = float(keep), int(key)

    def struct(self, width, rows=-1):
        return _ffi.Dropout(self.key, self.keep, int(rows), int(width))


def dropout(x, drop, out=None):
    """x * mask / keep with the hash mask (sgcn_dropout_f32): the unfused form, and -- the mask being
    a function of the element index only -- also its own backward."""
    if x.dim() == 1:
        x2 = x.view(1, -1)
        return dropout(x2, drop, None if out is None else out.view(1, -1)).view(-1)
    xp, ldx = _rows2d(x, "x")
    n, d = int(x.shape[0]), int(x.shape[1])
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=x.device)
    op, ldo = _rows2d(out, "out")
    st = drop.struct(d)
    check(lib.sgcn_dropout_f32(xp, ldx, n, d, C.byref(st), op, ldo, _stream()))
    return out


# ---- edge dropout of a static adjacency (include/sgcn.h SGCN_EDGE_SITE / sgcn_edge_revalue_f32) ------------------------
EDGE_SITE = 0x45444745          # the dropout site of the edge mask: no layer index (a layer's sites: i and i + 4096)
EDGE_ALWAYS = 0xFFFFFFFF        # the pair key of an entry no mask drops: the diagonal, a plan's pads
CS_PAD_BITS = 0x80000000        # the value bits of a pad entry of a G = 2 / 4 column-sweep plan (sgcn_csplang_*)


def _fmix32_np(h):
    """``_fmix32`` on a uint64 array holding 32-bit values."""
    m = np.uint64(0xFFFFFFFF)
    h = h & m
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & m
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & m
    return h ^ (h >> np.uint64(16))


ATTN_SITE = 0x4154544E          # include/sgcn.h SGCN_ATTN_SITE: the coefficient mask of aggregation layer i is site ATTN_SITE + i


def attn_key(seed, layer_index, step):
    """The key of the coefficient mask (--attn_dropout) of the aggregation layer at ``layer_index`` of the model's layer list
    at one training step (the step counter that keys the step's activation dropout)."""
    return dropout_key(seed, ATTN_SITE + int(layer_index), step)


def attn_kept(row, col, head, key, keep):
    """The coefficient mask of sgcn_spattn_drop_* on the host: a bool array, True where entry (row, col) of the pattern stays
    in head ``head`` (NumPy arrays or scalars, broadcast together).  Not symmetric in (row, col); no entry is exempt."""
    m = np.uint64(0xFFFFFFFF)
    i = np.asarray(row, dtype=np.int64).astype(np.uint64) & m
    j = np.asarray(col, dtype=np.int64).astype(np.uint64) & m
    h = np.asarray(head, dtype=np.int64).astype(np.uint64) & m
    rowh = _fmix32_np(i * np.uint64(0x9E3779B1) + np.uint64(int(key) & 0xFFFFFFFF))
    pair = _fmix32_np(rowh + ((j * np.uint64(0x85EBCA77)) & m))
    t = float(np.float32(keep)) * 4294967296.0
    thr = 0xFFFFFFFF if t >= 4294967295.0 else int(t)
    return _fmix32_np(pair + ((h * np.uint64(0x27D4EB2F)) & m)) < np.uint64(thr)


def edge_key(seed, step):
    """The key of the edge mask of one training step (the step counter that keys the step's activation dropout)."""
    return dropout_key(seed, EDGE_SITE, step)


def edge_pair_keys(row, col, pad=None):
    """One uint32 per stored entry: the hash of the unordered pair {row, col} of the ORIGINAL matrix (a matrix and its
    transpose give an edge the same key), EDGE_ALWAYS on the diagonal and where ``pad`` is set."""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    m = np.uint64(0xFFFFFFFF)
    u, v = np.minimum(row, col).astype(np.uint64) & m, np.maximum(row, col).astype(np.uint64) & m
    h = _fmix32_np(_fmix32_np(u * np.uint64(0x9E3779B1) + np.uint64(0x27D4EB2F)) + ((v * np.uint64(0x85EBCA77)) & m))
    h[h == np.uint64(EDGE_ALWAYS)] = np.uint64(EDGE_ALWAYS - 1)
    always = row == col
    if pad is not None:
        always = always | np.asarray(pad, dtype=bool)
    h[always] = np.uint64(EDGE_ALWAYS)
    return np.ascontiguousarray(h.astype(np.uint32))


def csr_entries(rowptr, col):
    """(row, col, pad) of every stored entry of a CSR (a DeviceCSR's value array): no pads."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    row = np.repeat(np.arange(rowptr.shape[0] - 1, dtype=np.int64), np.diff(rowptr))
    return row, np.asarray(col, dtype=np.int64), np.zeros(row.shape[0], dtype=bool)


def cs_entries(tile_ptr, colrow, val, tile_rows, G=1):
    """(row, col, pad) of every stored entry of an unlabelled column-sweep plan without column ranges, decoded from the
    plan's own host records (a built plan and one loaded from the cache alike): entry e of tile t belongs to bin
    g = e mod G, its local row is colrow >> 28, its output row tile_rows[t * 16 G + 16 g + local row] (the virtual rows of
    a split row name the same output row); with G = 2 / 4 an entry whose value bits are CS_PAD_BITS is a pad."""
    G = max(int(G), 1)
    tile_ptr = np.asarray(tile_ptr, dtype=np.int64)
    cr = np.ascontiguousarray(colrow, dtype=np.int32).view(np.uint32).astype(np.int64)
    n = cr.shape[0]
    if tile_ptr.shape[0] == 0 or int(tile_ptr[-1]) != n:
        raise ValueError("the tile pointer does not cover the plan's %d entries" % n)
    tile = np.repeat(np.arange(tile_ptr.shape[0] - 1, dtype=np.int64), np.diff(tile_ptr))
    e = np.arange(n, dtype=np.int64) - tile_ptr[:-1][tile]
    pad = np.zeros(n, dtype=bool) if G == 1 else \
        np.ascontiguousarray(val, dtype=np.float32).view(np.uint32) == np.uint32(CS_PAD_BITS)
    slot = tile * (16 * G) + (e % G) * 16 + (cr >> 28)
    row = np.where(pad, -1, np.asarray(tile_rows, dtype=np.int64)[np.where(pad, 0, slot)] if n else np.zeros(0, np.int64))
    if n and int(row[~pad].min(initial=0)) < 0:
        raise ValueError("a stored entry of the plan sits on a pad row")
    return row, np.where(pad, -1, cr & ((1 << 28) - 1)), pad


def plan_entries(plan):
    """(row, col, pad) of every stored entry of a device plan's value array: a DeviceCSR, or a ColumnSweepCSR as
    full_batch.StaticMatrix builds it (unlabelled, no column ranges); anything else has no decode."""
    if isinstance(plan, DeviceCSR):
        return csr_entries(plan.host_rowptr if plan.host_rowptr is not None else plan.rowptr.cpu().numpy(), plan.col.cpu().numpy())
    if isinstance(plan, ColumnSweepCSR):
        if plan.grouped or plan.ranged or plan.pos2col is not None or plan.R != 16:
            raise ValueError("edge dropout decodes unlabelled column-sweep plans without column ranges only")
        return cs_entries(plan.tile_ptr.cpu().numpy(), plan.columns_rows(), plan.val.cpu().numpy(),
                          plan.tile_rows.cpu().numpy(), plan.G)
    raise ValueError("edge dropout has no decode for a %s (the LDS sweep's unit plans carry no value array)" % type(plan).__name__)


def edge_revalue(base, pair, key, keep, out=None):
    """out[p] = base[p] under the edge mask of ``key`` (sgcn_edge_revalue_f32): the bits of base where pair is EDGE_ALWAYS,
    base * (1 / keep) where the pair is kept, +0.0 where it is dropped.  ``out`` must overlap neither ``base`` nor ``pair``."""
    _dev(base, torch.float32, "base")
    _dev(pair, torch.int32, "pair")            # (uint32 bits; torch has no unsigned 32-bit device type)
    n = int(base.numel())
    if base.dim() != 1 or pair.dim() != 1 or int(pair.numel()) != n or not (base.is_contiguous() and pair.is_contiguous()):
        raise ValueError("base and pair must be contiguous 1-D arrays of one length")
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=base.device)
    _dev(out, torch.float32, "out")
    if out.dim() != 1 or int(out.numel()) != n or not out.is_contiguous():
        raise ValueError("out must be a contiguous 1-D array of base's length")
    check(lib.sgcn_edge_revalue_f32(base.data_ptr(), pair.data_ptr(), n, int(key) & 0xFFFFFFFF, float(keep), out.data_ptr(),
                                    _stream()))
    return out


def gemm(A, B, out=None, trans_a=False, trans_b=False, accumulate=False, drop_a=None, drop_c=None):
    """out = op(A) @ op(B) (+ out)   (sgcn_gemm_f32; exact fp32 on the matrix cores).
    drop_a: the stored A is a dropout input (masked while loaded); drop_c: mask the output."""
    ap, lda = _rows2d(A, "A")
    bp, ldb = _rows2d(B, "B")
    M, K = (A.shape[1], A.shape[0]) if trans_a else (A.shape[0], A.shape[1])
    K2, N = (B.shape[1], B.shape[0]) if trans_b else (B.shape[0], B.shape[1])
    if K != K2:
        raise ValueError("gemm: inner dimensions differ (%d vs %d)" % (K, K2))
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs an existing `out`")
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    cp, ldc = _rows2d(out, "out")
    need = int(lib.sgcn_gemm_ws_floats(int(M), int(N), int(K)))     # > 0: split-K pays (small M x N, long K)
    ws = _gemm_ws(need, A.device) if need else None
    da = C.byref(drop_a.struct(A.shape[1])) if drop_a is not None else None
    dc = C.byref(drop_c.struct(N)) if drop_c is not None else None
    check(lib.sgcn_gemm_f32(int(trans_a), int(trans_b), int(M), int(N), int(K), ap, lda, bp, ldb, cp, ldc,
                            int(accumulate), _ptr(ws), da, dc, _stream()))
    return out


def gemm_bf16(A, B, out=None, trans_a=False, trans_b=False, accumulate=False, drop_a=None, drop_c=None):
    """out = op(A) @ op(B) (+ out) with the multiply in bfloat16 (sgcn_gemm_mb16_f32): operands and result are fp32
    tensors, every operand element is rounded to bfloat16 (nearest even) inside the kernel, products and sums are fp32.
    The signature of ``gemm``; both operands transposed is not provided.  A bfloat16 ``A`` (a table of
    ``history_alloc(..., bf16=True)``'s layout: the feature table under --feature_dtype bf16) goes to sgcn_gemm_mb16_a16:
    half the operand's bytes, the bits of the product of the widened table; there ``trans_b`` is not provided either.
    ``B`` and ``out`` are always fp32."""
    for name, t in (("B", B), ("out", out)):
        if t is not None and t.dtype == torch.bfloat16:
            raise TypeError("gemm_bf16: %s must be torch.float32 (only A may be a bfloat16 table), got %s" % (name, t.dtype))
    ap, lda, a16 = _hist2d(A, "A")
    bp, ldb = _rows2d(B, "B")
    M, K = (A.shape[1], A.shape[0]) if trans_a else (A.shape[0], A.shape[1])
    K2, N = (B.shape[1], B.shape[0]) if trans_b else (B.shape[0], B.shape[1])
    if K != K2:
        raise ValueError("gemm_bf16: inner dimensions differ (%d vs %d)" % (K, K2))
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs an existing `out`")
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    cp, ldc = _rows2d(out, "out")
    need = int(lib.sgcn_gemm_mb16_ws_floats(int(trans_a), int(trans_b), int(M), int(N), int(K)))
    ws = _gemm_ws(need, A.device) if need else None
    da = C.byref(drop_a.struct(A.shape[1])) if drop_a is not None else None
    dc = C.byref(drop_c.struct(N)) if drop_c is not None else None
    check((lib.sgcn_gemm_mb16_a16 if a16 else lib.sgcn_gemm_mb16_f32)(
        int(trans_a), int(trans_b), int(M), int(N), int(K), ap, lda, bp, ldb, cp, ldc, int(accumulate), _ptr(ws), da, dc,
        _stream()))
    return out


class GatheredRows(object):
    """``src[idx]`` that has not been gathered (tf.gather / history.dense_slice of the minibatch's
    input rows, gcn/vrgcn.py:43-45): the first dense layer's GEMMs read the rows through the index
    (dense_fwd / dense_bwd ``gidx``), so the n x F copy is never made.  Any other consumer calls
    ``materialize()``."""

    def __init__(self, src, idx):
        self.src, self.idx, self._m = src, idx, None

    @property
    def shape(self):
        return (int(self.idx.shape[0]), int(self.src.shape[1]))

    def materialize(self):
        if self._m is None:
            self._m = gather_rows(self.src, self.idx)
        return self._m


def dense_fwd(x, W, offset, scale, relu, eps=1e-9, x2=None, drop=None):
    """y = act(LN(x @ W) * scale + offset) in ONE launch (sgcn_dense_fwd_f32).
    Returns (y, ctx) like ln_act_fwd.  x2: a second operand stacked below x ([x ; x2] @ W without
    the concatenation); drop: dropout on the rows of x (never on x2), applied while the operand is
    loaded.  Needs N <= 128 when LayerNorm / ReLU is requested."""
    gidx = gidx2 = None
    if isinstance(x2, GatheredRows):
        x2, gidx2 = x2.src, x2.idx
    if isinstance(x, GatheredRows):
        x, gidx = x.src, x.idx
    n1 = int(x.shape[0] if gidx is None else gidx.shape[0])
    K, N = int(x.shape[1]), int(W.shape[1])
    M = n1 + (0 if x2 is None else int(x2.shape[0] if gidx2 is None else gidx2.shape[0]))
    xp, ldx = _rows2d(x, "x")
    x2p, ldx2 = _rows2d(x2, "x2") if x2 is not None else (None, 0)
    wp, ldw = _rows2d(W, "W")
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    norm = offset is not None
    xhat = torch.empty((M, N), dtype=torch.float32, device=x.device) if norm else None
    rstd = torch.empty((M,), dtype=torch.float32, device=x.device) if norm else None
    dr = C.byref(drop.struct(K, rows=n1)) if drop is not None else None
    need = int(lib.sgcn_gemm_ws_floats(M, N, K)) if N <= 128 else 0        # few tiles, long K: split-K
    ws = _gemm_ws(need, x.device) if need else None
    check(lib.sgcn_dense_fwd_f32(M, N, K, xp, ldx, x2p, ldx2, n1, wp, ldw, _ptr(offset), _ptr(scale),
                                 float(eps), int(bool(relu)), y.data_ptr(), N, _ptr(xhat), _ptr(rstd), dr,
                                 _ptr(ws), _ptr(gidx), _ptr(gidx2), _stream()))
    return y, ((xhat, rstd) if norm else None)


# ---- deterministic dropout: element-/row-wise pieces (sgcn_det.hip; gcn/layers.py:141-202, 236-248, 320-349, 425-428) ----
def _flat(x, name):
    """(pointer, element count) of a contiguous fp32 device array (tensor or DevArray)."""
    if isinstance(x, torch.Tensor):
        _dev(x, torch.float32, name)
        if not x.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
    return x.data_ptr(), int(x.numel())


def _like(x):
    return torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)


def det_pre(mu, var, keep):
    """Variance of dropout(x) / keep for x ~ (mu, var): var / keep + (1 / keep - 1) mu^2 (var None: plain input)."""
    mp, n = _flat(mu, "mu")
    out = _like(mu)
    check(lib.sgcn_det_pre_f32(mp, _flat(var, "var")[0] if var is not None else None, n, float(keep), out.data_ptr(), _stream()))
    return out


def det_pre_bwd(mu, g, keep, d_mu, want_var):
    """d_mu += g 2 (1 / keep - 1) mu; returns d_var = g / keep (or None)."""
    mp, n = _flat(mu, "mu")
    d_var = _like(mu) if want_var else None
    check(lib.sgcn_det_pre_bwd_f32(mp, _flat(g, "g")[0], n, float(keep), _flat(d_mu, "d_mu")[0], _ptr(d_var), _stream()))
    return d_var


def square(x, c=1.0):
    """c * x^2 element-wise (tf.square of a weight matrix / of an adjacency's values)."""
    xp, n = _flat(x, "x")
    out = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
    check(lib.sgcn_square_f32(xp, n, float(c), out.data_ptr(), _stream()))
    return out


def addmul(acc, a, b, c=1.0):
    """acc += c * a * b element-wise."""
    ap, n = _flat(a, "a")
    check(lib.sgcn_addmul_f32(_flat(acc, "acc")[0], ap, _flat(b, "b")[0], n, float(c), _stream()))
    return acc


def det_lnvar_fwd(var1, rstd, scale, eps):
    n, d = int(var1.shape[0]), int(var1.shape[1])
    out = _like(var1)
    check(lib.sgcn_det_lnvar_fwd_f32(_flat(var1, "var1")[0], _ptr(rstd), _ptr(scale), n, d, float(eps), out.data_ptr(), _stream()))
    return out


def det_lnvar_bwd(g, var1, xhat, rstd, scale, eps, d_mu1, dscale):
    """Returns d_var1; adds the variance stream's share to d_mu1 and dscale."""
    n, d = int(var1.shape[0]), int(var1.shape[1])
    d_var1, tmp = _like(var1), _like(var1)
    check(lib.sgcn_det_lnvar_bwd_f32(_flat(g, "g")[0], _flat(var1, "var1")[0], _ptr(xhat), _ptr(rstd), _ptr(scale), n, d, float(eps),
                                     d_var1.data_ptr(), _flat(d_mu1, "d_mu1")[0], _ptr(dscale), tmp.data_ptr(), _stream()))
    return d_var1


def det_relu_fwd(mu, var):
    mp, n = _flat(mu, "mu")
    mo, vo = _like(mu), _like(mu)
    check(lib.sgcn_det_relu_fwd_f32(mp, _flat(var, "var")[0], n, mo.data_ptr(), vo.data_ptr(), _stream()))
    return mo, vo


def det_relu_bwd(mu, var, g_mu, g_var):
    mp, n = _flat(mu, "mu")
    d_mu, d_var = _like(mu), _like(mu)
    check(lib.sgcn_det_relu_bwd_f32(mp, _flat(var, "var")[0], _flat(g_mu, "g_mu")[0], _flat(g_var, "g_var")[0], n,
                                    d_mu.data_ptr(), d_var.data_ptr(), _stream()))
    return d_mu, d_var


def gauss_sample(mu, var, key):
    mp, n = _flat(mu, "mu")
    x = _like(mu)
    check(lib.sgcn_gauss_sample_f32(mp, _flat(var, "var")[0], n, int(key) & 0xFFFFFFFF, x.data_ptr(), _stream()))
    return x


def gauss_sample_bwd(var, g, key):
    vp, n = _flat(var, "var")
    d_var = _like(var)
    check(lib.sgcn_gauss_sample_bwd_f32(vp, _flat(g, "g")[0], n, int(key) & 0xFFFFFFFF, d_var.data_ptr(), _stream()))
    return d_var


def det_agg_prep(mu, var, Hm, Hv, ifield):
    """(delta_mu, ds2, msig2, ds, sbar) of the control-variate aggregator on (mu, var)."""
    n0, d = int(mu.shape[0]), int(mu.shape[1])
    hp, ldh = _rows2d(Hm, "Hm")
    vp, ldv = _rows2d(Hv, "Hv")
    if ldh != ldv:
        raise ValueError("the two histories must share a pitch")
    outs = [_like(mu) for _ in range(5)]
    check(lib.sgcn_det_agg_prep_f32(_flat(mu, "mu")[0], _flat(var, "var")[0], hp, vp, ldh, _ptr(_dev(ifield, torch.int32, "ifield")),
                                    n0, d, *[o.data_ptr() for o in outs], _stream()))
    return outs


def det_agg_prep_bwd(var, ds, sbar, g_ds2, g_msig2, add=None, add_rows=0):
    n0, d = int(var.shape[0]), int(var.shape[1])
    d_var = _like(var)
    ap, ldadd = _rows2d(add, "add") if add is not None else (None, 0)
    check(lib.sgcn_det_agg_prep_bwd_f32(_flat(var, "var")[0], _ptr(ds), _ptr(sbar), _flat(g_ds2, "g_ds2")[0], _flat(g_msig2, "g_msig2")[0],
                                        n0, d, ap, ldadd, int(add_rows), d_var.data_ptr(), _stream()))
    return d_var


def relu_eps(raw, eps, out=None):
    """relu(raw) + eps (out may be a column block of a wider array)."""
    rp, ldr = _rows2d(raw, "raw")
    n, d = int(raw.shape[0]), int(raw.shape[1])
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=raw.device)
    op, ldo = _rows2d(out, "out")
    check(lib.sgcn_relu_eps_f32(rp, ldr, n, d, float(eps), op, ldo, _stream()))
    return out


def gate(raw, g):
    """g where raw > 0, else 0 (dense result; g may be a column block)."""
    rp, ldr = _rows2d(raw, "raw")
    gp, ldg = _rows2d(g, "g")
    n, d = int(raw.shape[0]), int(raw.shape[1])
    out = torch.empty((n, d), dtype=torch.float32, device=raw.device)
    check(lib.sgcn_gate_f32(rp, ldr, gp, ldg, n, d, out.data_ptr(), _stream()))
    return out
