"""Exact full-graph propagation on the static-graph SpMMs (``--full_batch`` / ``--test_full_batch``).

The reference can only approximate it (``--nocv --degree 10000`` with one batch of all train ids: the sampler rebuilds
the CSR of the whole receptive field every step).  Here the graph is what it is -- static: every aggregation layer
multiplies the SAME N x N matrix, forward by ``A`` and backward by ``A^T``, once per epoch, which is the workload the
column sweep, the LDS sweep and their planner / autotuner / plan cache were built for (bench.py times exactly these
two products).

  StaticMatrix   one adjacency with a plan built once, a lazily built transpose (ops.transpose_host) and the product
                 method PlainAggregator calls (``out=`` with a column-offset view, ``add=`` / ``add_rows=``);
                 dispatches to ops.spmm / ops.spmm_cs / ops.spmm_lds; with ``bf16`` (--full_batch_dtype bf16) every product
                 rounds its dense operand into a bfloat16 scratch table and gathers from there (sgcn_spmm_*_b16)
  StaticBatch    what Model.upload / get_data accept in place of a PackedBatch: fields[l] = arange(N), unit scales,
                 the N x C label table, and ``rows`` -- the sorted subset of vertices the loss runs over
                 (ops.softmax_ce / sigmoid_ce ``rows=``)
"""
import numpy as np
import torch

from . import ops
from .flags import FLAGS, _CHOICES

KERNELS = _CHOICES['full_batch_kernel']
DTYPES = _CHOICES['full_batch_dtype']
DENSE_DTYPES = _CHOICES['dense_dtype']


def check_full_batch(flags=None, world=1):
    """Refuses the flag combinations the full-graph modes have no meaning for.  Needs no device."""
    f = FLAGS if flags is None else flags
    if f.full_batch_kernel not in KERNELS:
        raise ValueError("--full_batch_kernel must be one of %s, got %r" % ('/'.join(KERNELS), f.full_batch_kernel))
    dtype = getattr(f, 'full_batch_dtype', 'fp32')
    if dtype not in DTYPES:
        raise ValueError("--full_batch_dtype must be one of %s, got %r" % ('/'.join(DTYPES), dtype))
    if dtype == 'bf16':
        if not (f.full_batch or f.test_full_batch):
            raise ValueError("--full_batch_dtype bf16 needs --full_batch or --test_full_batch: it is the storage type of the "
                             "dense operand of the full-graph products, and no other mode runs them")
        if f.full_batch_kernel == 'lds':
            raise ValueError("--full_batch_dtype bf16 is not supported with --full_batch_kernel lds: the LDS-staged sweep "
                             "stages fp32 pieces of the operand and has no bfloat16 form")
    dense = getattr(f, 'dense_dtype', 'fp32')
    if dense not in DENSE_DTYPES:
        raise ValueError("--dense_dtype must be one of %s, got %r" % ('/'.join(DENSE_DTYPES), dense))
    if dense == 'bf16' and not (f.full_batch or f.test_full_batch):
        raise ValueError("--dense_dtype bf16 needs --full_batch or --test_full_batch: it is the multiply type of the dense "
                         "layers of a pass over the whole graph, and no other mode runs that route")
    if f.full_batch:
        for name, why in (('cv', 'exact propagation has no estimator and no history'),
                          ('cvd', 'exact propagation has no estimator and no history'),
                          ('importance', 'there is no sampler'),
                          ('det_dropout', 'that stack propagates a mean and a variance through the sampled matrices'),
                          ('gradvar', 'the study compares two samplers')):
            if getattr(f, name):
                raise ValueError("--full_batch is not supported with --%s: %s" % (name, why))
        if int(world) > 1:
            raise ValueError("--full_batch is not supported on %d ranks: one step covers the whole graph; sharding its "
                             "products over GPUs is a separate mode" % int(world))
    if f.test_full_batch:
        for name, why in (('test_cv', 'exact propagation has no estimator and no history'),
                          ('test_cvd', 'exact propagation has no estimator and no history'),
                          ('test_importance', 'there is no sampler'),
                          ('det_dropout', 'that stack propagates a mean and a variance through the sampled matrices'),
                          ('gradvar', 'the study draws from the evaluation sampler')):
            if getattr(f, name):
                raise ValueError("--test_full_batch is not supported with --%s: %s" % (name, why))
    return bool(f.full_batch), bool(f.test_full_batch)


def full_batch_bf16(flags=None):
    """--full_batch_dtype as a bool (bfloat16 operand?)."""
    return getattr(FLAGS if flags is None else flags, 'full_batch_dtype', 'fp32') == 'bf16'


def dense_bf16(flags=None):
    """--dense_dtype as a bool (bfloat16 multiplies in the dense layers of a static pass?)."""
    return getattr(FLAGS if flags is None else flags, 'dense_dtype', 'fp32') == 'bf16'


def _aligned(t):
    """Rows of a 2-D fp32 view on 16-byte boundaries (what the sweep kernels' float4 accesses need)."""
    return t.data_ptr() % 16 == 0 and (t.shape[0] <= 1 or t.stride(0) % 4 == 0)


class StaticMatrix(object):
    """A static sparse matrix on the device, multiplied many times: ``kernel`` is 'rows' (the row-gather kernel on a
    DeviceCSR), 'cs' (column sweep) or 'lds' (LDS-staged sweep + residual), or 'auto': train.static_kernel_for(nnz, d,
    products) with ``products`` the number of times the plan will run -- and for a large graph with communities
    ops.LdsSweepCSR.for_graph, exactly as train.pp_products chooses.  ``d`` is the operand width the choice (and the
    column sweep's lane grouping) is made for.

    ``bf16``: every product rounds ``x`` to nearest even into a bfloat16 scratch table -- one per operand width, allocated
    once and reused every epoch -- and runs the kernel's bfloat16-operand form: half the operand's bytes per nonzero, the
    sums and ``out`` fp32, bit for bit the fp32 product of the rounded operand.  The transpose inherits it.  The LDS sweep
    has no such form: forcing it is refused, 'auto' never picks it."""

    bf16 = False          # (the fp32 operand is the default of every instance)

    def __init__(self, a, device, kernel='auto', products=1, d=128, cache_path=None, _transpose_of=None, bf16=False):
        a = a.tocsr()
        self.bf16, self._scratch = bool(bf16), {}
        if self.bf16 and kernel == 'lds':
            raise ValueError("the LDS-staged sweep has no bfloat16-operand form")
        self.a, self.device, self.shape, self.nnz = a, device, (int(a.shape[0]), int(a.shape[1])), int(a.nnz)
        self.requested, self.products, self.d_hint, self.cache_path = kernel, int(products), int(d), cache_path
        self._transpose = _transpose_of
        self._rows = self._plan = None
        self._tuned = set()
        self.plan_from_cache = False
        self.kernel = self._choose(kernel)

    def _choose(self, kernel):
        a, d = self.a, self.d_hint
        if kernel == 'rows':
            return 'rows'
        if kernel == 'lds':
            labels, _ = ops.reorder_labels(a)
            self._plan = ops.LdsSweepCSR(a, self.device, host=ops.LdsSweepCSR.auto_host(a, labels))
            return 'lds'
        if kernel == 'auto':
            from . import train            # (late: train imports this module)
            if train.static_kernel_for(self.nnz, d, self.products) == 'rows':
                return 'rows'
            if self.cache_path is None and self.nnz >= 2000000 and d >= 128 and not self.bf16:
                self._plan = ops.LdsSweepCSR.for_graph(a, self.device)
                if self._plan is not None:
                    return 'lds'
        G = ops.ColumnSweepCSR.choose_g(d, self.nnz / max(self.shape[0], 1), self.shape[0])
        self._plan, self.plan_from_cache = ops.ColumnSweepCSR.cached(a, self.device, self.cache_path, G=G)
        return 'cs'

    @property
    def transpose(self):
        """A^T as a StaticMatrix of the same kind, built on first use (an evaluation-only matrix never builds it)."""
        if self._transpose is None:
            path = self.cache_path[:-4] + ".T.npz" if self.cache_path else None
            self._transpose = StaticMatrix(ops.transpose_host(self.a), self.device, self.requested if self.requested != 'auto'
                                           else ('rows' if self.kernel == 'rows' else 'auto'), self.products, self.d_hint,
                                           path, _transpose_of=self, bf16=self.bf16)
        return self._transpose

    @property
    def rows_csr(self):
        if self._rows is None:
            self._rows = ops.DeviceCSR.from_scipy(self.a, self.device)
        return self._rows

    def _autotune(self, x, d):
        if d in self._tuned:
            return
        self._tuned.add(d)
        if self.kernel == 'lds':
            r = self._plan.residual
            if isinstance(r, ops.ColumnSweepCSR) and d not in r.pace:
                self._plan.autotune(x, d=d)
        elif d not in self._plan.clock(x.dtype == torch.bfloat16).pace:
            self._plan.autotune(x, d=d)                # once per plan, width and operand type; stored with a cached plan
            self._plan.store_if_cached()

    def operand(self, x):
        """What the kernel gathers from: ``x`` itself, or under ``bf16`` this matrix's scratch table of x's width holding
        x rounded to nearest even (ops.operand_round: sgcn_scatter_rows_h16 with no index)."""
        if not self.bf16:
            return x
        n, d = int(x.shape[0]), int(x.shape[1])
        if n != self.shape[1]:
            raise ValueError("the operand has %d rows, the matrix %d columns" % (n, self.shape[1]))
        tab = self._scratch.get(d)
        if tab is None:
            tab = self._scratch[d] = ops.history_alloc(n, d, x.device, bf16=True)
        return ops.operand_round(x, out=tab)

    def kernel_for(self, x, out=None):
        """The kernel one product runs on: the matrix's own, or the row kernel where an operand's rows are not 16-byte
        aligned (a width that is not a multiple of 4: no copy is made for the sweep's sake).  Under ``bf16`` the kernel
        reads the scratch table, which is always aligned: only the width and ``out`` decide."""
        if self.kernel == 'rows':
            return 'rows'
        d = int(x.shape[1])
        if d % 4 or (not self.bf16 and not _aligned(x)) or (out is not None and not _aligned(out)):
            return 'rows'
        return self.kernel

    def product(self, x, out=None, add=None, add_rows=0):
        """out = A x (+ add on the first ``add_rows`` rows), the keyword set of ops.spmm that PlainAggregator uses.  The
        sweep kernels have no epilogue addend: the addend is stored into ``out`` and the product runs with beta = 1."""
        M, d = self.shape[0], int(x.shape[1])
        k = self.kernel_for(x, out)
        x = self.operand(x)
        if k == 'rows':
            return ops.spmm(self.rows_csr, x, out=out, add=add, add_rows=add_rows)
        if out is None:
            out = torch.empty((M, d), dtype=torch.float32, device=x.device)
        self._autotune(x, d)
        beta = 0.0
        if add is not None:
            r = int(add_rows)
            out[:r].copy_(add[:r])
            if r < M:
                out[r:].zero_()
            beta = 1.0
        if k == 'lds':
            return ops.spmm_lds(self._plan, x, out=out, beta=beta, d=d)
        return ops.spmm_cs(self._plan, x, out=out, beta=beta, d=d)


class StaticCur(object):
    """``model.cur`` of a static batch (the attributes of models.DevFeed the eager layer path reads)."""
    __slots__ = ("fields", "host_fields", "scales", "labels", "rows", "adj", "fadj", "ffields", "inputs", "sizes")


class StaticBatch(object):
    """The whole graph as one batch: ``fields[l] = arange(N)`` and ``scales[l] = 1`` for every l, ``labels`` the N x C
    table, ``adj[l]`` ONE shared StaticMatrix, and ``rows`` the vertices the loss runs over -- ascending and unique
    (checked here, on the host: the loss kernel trusts it)."""

    def __init__(self, matrix, labels, rows, L, device=None):
        N = int(matrix.shape[0])
        if matrix.shape[0] != matrix.shape[1]:
            raise ValueError("a static batch needs a square (vertex x vertex) matrix")
        if int(labels.shape[0]) != N:
            raise ValueError("labels has %d rows, the graph %d vertices" % (int(labels.shape[0]), N))
        device = device if device is not None else getattr(matrix, 'device', None)
        self.N, self.L, self.matrix, self.device = N, int(L), matrix, device
        self.dropout = 0.0
        self.host_rows = ops.check_loss_rows(rows, N)
        self.host_field = np.arange(N, dtype=np.int32)
        to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)      # noqa: E731
        self.labels = labels if isinstance(labels, torch.Tensor) else to(np.asarray(labels, dtype=np.float32))
        self.rows = to(self.host_rows)
        field, ones = to(self.host_field), torch.ones(N, dtype=torch.float32, device=device)
        self.fields = [field] * (self.L + 1)
        self.scales = [ones] * self.L
        self.adj = [matrix] * self.L
        nnz = int(getattr(matrix, 'nnz', 0))
        self.sizes = dict(adj=[nnz] * self.L, fadj=[0] * self.L, fields=[N] * (self.L + 1))

    def with_rows(self, rows):
        """The same batch with the loss over another subset (validation / test ids share the matrix, labels, fields)."""
        other = StaticBatch.__new__(StaticBatch)
        other.__dict__.update(self.__dict__)
        other.host_rows = ops.check_loss_rows(rows, self.N)
        other.rows = torch.from_numpy(other.host_rows).to(self.device)
        return other

    def cur(self, inputs):
        c = StaticCur()
        c.fields, c.scales, c.labels, c.rows, c.adj = self.fields, self.scales, self.labels, self.rows, self.adj
        c.host_fields = [self.host_field] * (self.L + 1)
        c.fadj, c.ffields, c.inputs, c.sizes = [], [], inputs, self.sizes
        return c
