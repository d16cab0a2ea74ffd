"""Exact full-graph propagation on the static-graph SpMMs (``--full_batch`` / ``--test_full_batch``).

The reference can only approximate it (``--nocv --degree 10000`` with one batch of all train ids: the sampler rebuilds
the CSR of the whole receptive field every step).  Here the graph is what it is -- static: every aggregation layer
multiplies the SAME N x N matrix, forward by ``A`` and backward by ``A^T``, once per epoch, which is the workload the
column sweep, the LDS sweep and their planner / autotuner / plan cache were built for (bench.py times exactly these
two products).

  StaticMatrix   one adjacency with a plan built once and a lazily built transpose (ops.transpose_host): it alone chooses the
                 kernel, tunes and stores the plan and dispatches to ops.spmm / ops.spmm_cs / ops.spmm_lds.  ``multiply`` is
                 the plain product (train.pp_products); ``product`` is the method PlainAggregator calls (``out=`` with a
                 column-offset view, ``add=`` / ``add_rows=``): it decides on alignment and, with ``bf16`` (--full_batch_dtype
                 bf16), rounds the dense operand into a bfloat16 scratch table the kernel gathers from (sgcn_spmm_*_b16);
                 ``max_product`` / ``max_backward`` are what it calls under --aggregator max: the element-wise maximum over the
                 matrix's pattern and its gradient (ops.spmax / ops.spmax_bwd on the row kernel's CSR); ``attn_product`` /
                 ``attn_backward`` under --aggregator attn: softmax dot-product attention over the same pattern (ops.spattn /
                 ops.spattn_bwd)
  model_matrix   the StaticMatrix of one model's aggregation layers (the operand width its plan is made for)
  EdgeMask       --edge_dropout: the mask a StaticMatrix and its transpose share; inside a training step (begin_step .. end_step)
                 every product of either reads a value array re-drawn from the base values under the step's key
                 (ops.edge_revalue), outside of one the base values -- the product kernels are the same either way
  static_kernel_for   the cost model 'auto' decides by; train.py builds on this module, never the other way round
  StaticBatch    what Model.upload / get_data accept in place of a PackedBatch: fields[l] = arange(N), unit scales,
                 the N x C label table, and ``rows`` -- the sorted subset of vertices the loss runs over
                 (ops.softmax_ce / sigmoid_ce ``rows=``); without labels: a batch for forward passes only (exact_history.py)

--full_batch_parts P (Cluster-GCN, Chiang et al., KDD 2019): more than one optimizer step per epoch without an estimator --
  partition      the vertices cut once into P parts (label-propagation communities, cut to size, packed largest first)
  PartSchedule   per epoch a seeded permutation of the parts in groups of q; a step runs on the union S of a group
  InducedMatrix  the StaticMatrix of A[S, S], over the block ops.csr_induce cut out of the resident CSR on the device
  PartBatch      the StaticBatch of that block: labels[S] and the positions within S of the training vertices
  PulledMatrix   --full_batch_part_history (GNNAutoScale): the InducedMatrix of the 'keep' block that also carries the resident
                 adjacency, the ids and map of S and the model's history tables; ``pull_product`` sums over every stored entry of
                 the rows of S, fresh rows for columns in S and stored rows for the others (ops.spmm_pull); under
                 --full_batch_part_pull with --aggregator attn ``pull_attn_product`` / ``pull_attn_backward`` attend over
                 the same entries (ops.spattn_pull, ops.spattn_pull_bwd_q, then the block's bwd_kv); under
                 --full_batch_part_pull_max ``pull_max_product`` takes the element-wise maximum over them (ops.spmax_pull),
                 the backward being the block's own
  PulledLayer    that matrix as aggregation layer l multiplies by it (PartBatch.adj[l]): one-table calls that pull, then push
"""
import numpy as np
import torch

from . import ops
from .flags import FLAGS, _CHOICES

KERNELS = _CHOICES['full_batch_kernel']
DTYPES = _CHOICES['full_batch_dtype']
DENSE_DTYPES = _CHOICES['dense_dtype']
FEATURE_DTYPES = _CHOICES['feature_dtype']


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


def check_feature_dtype(flags=None):
    """(training model's table bfloat16?, test model's table bfloat16?) under --feature_dtype, with the combinations it has
    no kernel or no meaning for refused.  Needs no device; a sibling of check_full_batch, called beside it.

    The rule is per model: a model's dense feature table is stored as bfloat16 when the flag is bf16 and EVERY pass that
    model ever runs is a static pass -- the training model under --full_batch, the test model under --test_full_batch.  A
    model that runs sampled steps (--cv --cvd beside --test_full_batch) keeps its fp32 table: the fp32 GEMM and the fused
    dense_fwd of those steps have no bfloat16-table loader."""
    f = FLAGS if flags is None else flags
    dtype = getattr(f, 'feature_dtype', 'fp32')
    if dtype not in FEATURE_DTYPES:
        raise ValueError("--feature_dtype must be one of %s, got %r" % ('/'.join(FEATURE_DTYPES), dtype))
    if dtype != 'bf16':
        return False, False
    if getattr(f, 'dense_dtype', 'fp32') != 'bf16':
        raise ValueError("--feature_dtype bf16 needs --dense_dtype bf16: only the bf16-multiply GEMM reads a bfloat16 feature "
                         "table; the fp32 GEMM and the fused dense layer have no loader for one")
    if not (f.full_batch or f.test_full_batch):
        raise ValueError("--feature_dtype bf16 needs --full_batch or --test_full_batch: it is the storage type of the feature "
                         "table of a model whose every pass covers the whole graph, and no other mode has such a model")
    return bool(f.full_batch), bool(f.test_full_batch)


def check_edge_dropout(flags=None):
    """--edge_dropout as a float (0.0 = off), with what it has no kernel or no meaning for refused.  Needs no device; a sibling
    of check_full_batch, called beside it."""
    f = FLAGS if flags is None else flags
    p = float(getattr(f, 'edge_dropout', 0.0))
    if not (0.0 <= p < 1.0):                  # (NaN too; 1 - p is then at least 2^-53, which fp32 holds)
        raise ValueError("--edge_dropout must lie in [0, 1) (0 = off), got %r" % (getattr(f, 'edge_dropout', 0.0),))
    if p > 0:
        if not f.full_batch:
            raise ValueError("--edge_dropout needs --full_batch: it re-draws the values of the static training adjacency once "
                             "per full-graph step, and no other mode trains on one")
        if f.full_batch_kernel == 'lds':
            raise ValueError("--edge_dropout is not supported with --full_batch_kernel lds: the LDS-staged sweep runs unit "
                             "plans, which carry no value array to re-draw")
        if getattr(f, 'gradvar', False):
            raise ValueError("--edge_dropout is not supported with --gradvar: the study compares two samplers on one adjacency")
    return p


AGGREGATORS = _CHOICES['aggregator']


def check_aggregator(flags=None):
    """--aggregator as a bool (element-wise maximum?), with the combinations the maximum has no kernel or no meaning for
    refused.  Needs no device; a sibling of check_full_batch, called beside it."""
    f = FLAGS if flags is None else flags
    agg = getattr(f, 'aggregator', 'sum')
    if agg not in AGGREGATORS:
        raise ValueError("--aggregator must be one of %s, got %r" % ('/'.join(AGGREGATORS), agg))
    if agg == 'attn':
        check_attention(f)                    # (its own refusals; this function's answer stays `maximum?`)
    if agg != 'max':
        return False
    if not (f.full_batch and f.test_full_batch):
        raise ValueError("--aggregator max needs --full_batch and --test_full_batch: a maximum is not linear, so no sampled "
                         "estimator carries it and sampled steps have no such kernel, and the training and the test model "
                         "must aggregate alike")
    if getattr(f, 'full_batch_dtype', 'fp32') == 'bf16':
        raise ValueError("--aggregator max is not supported with --full_batch_dtype bf16: the maximum kernels gather from an "
                         "fp32 table; there is no bfloat16-table form yet")
    if getattr(f, 'feature_dtype', 'fp32') == 'bf16':
        raise ValueError("--aggregator max is not supported with --feature_dtype bf16: the maximum kernels gather from an "
                         "fp32 table; there is no bfloat16-table form yet")
    if float(getattr(f, 'edge_dropout', 0.0)) > 0:
        raise ValueError("--aggregator max is not supported with --edge_dropout: the maximum reads the adjacency's pattern, "
                         "not its values; there is no edge-masked form yet")
    return True


def check_attention(flags=None):
    """(--aggregator attn?, --attn_scale) with the combinations attention has no kernel or no meaning for refused.  Needs no
    device; a sibling of check_aggregator, called beside it.  The scale is 0.0 for `1 / sqrt(d) of the layer's own input
    width` (layers.PlainAggregator works it out per layer) or the positive factor to use as given."""
    f = FLAGS if flags is None else flags
    agg = getattr(f, 'aggregator', 'sum')
    if agg not in AGGREGATORS:
        raise ValueError("--aggregator must be one of %s, got %r" % ('/'.join(AGGREGATORS), agg))
    scale = float(getattr(f, 'attn_scale', 0.0))
    if not (0.0 <= scale < float('inf')):     # (NaN too)
        raise ValueError("--attn_scale must be finite and >= 0 (0 = 1 / sqrt(d) of each aggregation layer's input width), "
                         "got %r" % (getattr(f, 'attn_scale', 0.0),))
    if agg != 'attn':
        if scale != 0.0:
            raise ValueError("--attn_scale needs --aggregator attn: it is the factor on the attention scores, and no other "
                             "aggregator computes any")
        return False, 0.0
    if not (f.full_batch and f.test_full_batch):
        raise ValueError("--aggregator attn needs --full_batch and --test_full_batch: attention is not linear, so no sampled "
                         "estimator carries it and sampled steps have no such kernel, and the training and the test model "
                         "must aggregate alike")
    if getattr(f, 'full_batch_dtype', 'fp32') == 'bf16':
        raise ValueError("--aggregator attn is not supported with --full_batch_dtype bf16: the attention kernels gather from "
                         "an fp32 table; there is no bfloat16-table form yet")
    if getattr(f, 'feature_dtype', 'fp32') == 'bf16':
        raise ValueError("--aggregator attn is not supported with --feature_dtype bf16: the attention kernels gather from an "
                         "fp32 table; there is no bfloat16-table form yet")
    if float(getattr(f, 'edge_dropout', 0.0)) > 0:
        raise ValueError("--aggregator attn is not supported with --edge_dropout: attention reads the adjacency's pattern, "
                         "not its values; there is no edge-masked form yet")
    return True, scale


ATTN_HEADS = (1, 2, 4, 8)


def check_attn_heads(flags=None):
    """--attn_heads as an int, refused where the kernels have no such form (a head is an aligned power-of-two share of a
    lane group: 1/2/4/8) or where nothing would read it.  Needs no device; called right after check_attention.  Whether
    the heads divide a layer's width is known once the widths are (train.Trainer, layers.PlainAggregator)."""
    f = FLAGS if flags is None else flags
    heads = getattr(f, 'attn_heads', 1)
    if isinstance(heads, bool) or not isinstance(heads, int) or heads not in ATTN_HEADS:
        raise ValueError("--attn_heads must be one of 1/2/4/8, got %r" % (heads,))
    if heads != 1 and getattr(f, 'aggregator', 'sum') != 'attn':
        raise ValueError("--attn_heads needs --aggregator attn: it is the number of attention heads, and no other aggregator "
                         "has any")
    return heads


def check_attn_dropout(flags=None):
    """--attn_dropout as a float (0.0 = off), refused outside [0, 1) or where nothing would read it.  Needs no device; called
    right after check_attn_heads.  (check_attention has refused what attention itself cannot run with.)"""
    f = FLAGS if flags is None else flags
    p = float(getattr(f, 'attn_dropout', 0.0))
    if not (0.0 <= p < 1.0):                  # (NaN too; 1 - p is then at least 2^-53, which fp32 holds)
        raise ValueError("--attn_dropout must lie in [0, 1) (0 = off), got %r" % (getattr(f, 'attn_dropout', 0.0),))
    if p > 0 and getattr(f, 'aggregator', 'sum') != 'attn':
        raise ValueError("--attn_dropout needs --aggregator attn: it drops attention coefficients, and no other aggregator "
                         "has any")
    return p


ATTN_SCORES = _CHOICES['attn_score']


def check_attn_score(flags=None):
    """(--attn_score gat?, --attn_slope) with what the learned scores have no meaning for refused.  Needs no device; called
    right after check_attn_dropout."""
    f = FLAGS if flags is None else flags
    score = getattr(f, 'attn_score', 'dot')
    if score not in ATTN_SCORES:
        raise ValueError("--attn_score must be one of %s, got %r" % ('/'.join(ATTN_SCORES), score))
    slope = float(getattr(f, 'attn_slope', 0.2))
    if not (0.0 <= slope <= 1.0):             # (NaN too)
        raise ValueError("--attn_slope must lie in [0, 1], got %r" % (getattr(f, 'attn_slope', 0.2),))
    if score != 'gat':
        if slope != 0.2:
            raise ValueError("--attn_slope needs --attn_score gat: it is the negative slope of the LeakyReLU on the learned "
                             "scores, and the dot-product scores have none")
        return False, slope
    if getattr(f, 'aggregator', 'sum') != 'attn':
        raise ValueError("--attn_score gat needs --aggregator attn: it is how the attention scores are formed, and no other "
                         "aggregator computes any")
    if float(getattr(f, 'attn_scale', 0.0)) != 0.0:
        raise ValueError("--attn_score gat is not supported with --attn_scale: the learned scores have no scale (the vectors "
                         "a_src and a_dst carry it)")
    return True, slope


def attn_heads_divide(heads, width, what):
    """ValueError naming the layer and its width unless the heads cut it evenly."""
    if width % heads:
        raise ValueError("--attn_heads %d does not divide the input width of %s (%d columns): every head is an equal "
                         "slice of the columns" % (heads, what, width))


def full_batch_bf16(flags=None):
    """--full_batch_dtype as a bool (bfloat16 operand?)."""
    return getattr(FLAGS if flags is None else flags, 'full_batch_dtype', 'fp32') == 'bf16'


def dense_bf16(flags=None):
    """--dense_dtype as a bool (bfloat16 multiplies in the dense layers of a static pass?)."""
    return getattr(FLAGS if flags is None else flags, 'dense_dtype', 'fp32') == 'bf16'


# What the static-graph kernels cost end to end on the MI355X (profiles/r60_bench_setup.json, S-Reddit: 23.2 M nonzeros,
# d = 602, 16 host cores): the row-gather kernel needs the CSR in HBM and a row-pointer pass (5 ms) and takes 7.66 ms per
# product; the column sweep needs its host plan + upload (0.185 s: 8 ns per nonzero), a clock autotune worth ~62 products,
# and takes 0.40 of the row kernel's time per product.
# (The constants were fitted with fp32 operands and serve --full_batch_dtype bf16 unchanged: the sweep's product
# with a bfloat16 operand takes 0.835 of the fp32 one at d = 602 (profiles/spmm_b16_products.jsonl); the row kernel's bf16 time
# is not measured, so a bf16 set would move one side of the ratio only.)
CS_PLAN_S_PER_NNZ = 8.0e-9
CS_AUTOTUNE_PRODUCTS = 62
CS_TIME_RATIO = 0.40
ROWS_S_PER_NNZ_FLOAT = 7.66e-3 / (23173306 * 602.0)


def static_kernel_for(nnz, d, products):
    """'rows' or 'cs': the kernel with the lower expected END-TO-END time for `products` products of one static matrix
    with a d-wide dense operand -- setup included.  The reference computes each PP product once (gcn/utils.py:321-322, the
    result cached in the dataset's .npz), and for one product no plan pays: the column sweep breaks even at ~83 products of
    S-Reddit (a full-batch model's layers over a few epochs), which is what bench.py reports as
    setup.products_to_break_even_vs_rows_kernel."""
    t_rows = ROWS_S_PER_NNZ_FLOAT * nnz * d
    rows = products * t_rows
    cs = CS_PLAN_S_PER_NNZ * nnz + (CS_AUTOTUNE_PRODUCTS + products) * CS_TIME_RATIO * t_rows
    return 'cs' if cs < rows else 'rows'


def full_batch_products(which):
    """How many times the plan of a full-graph matrix will run (what static_kernel_for weighs its setup against).  SGDTrain
    leaves on `epoch > FLAGS.epochs` (gcn/train.py:234), i.e. after epochs + 2 epochs: 'train' -- one step in each of them;
    'full' -- one evaluation in each of them and the test."""
    return int(FLAGS.epochs) + 2 if which == 'train' else int(FLAGS.epochs) + 3


def _aligned(t):
    """Rows of a 2-D fp32 view on 16-byte boundaries (what the sweep kernels' float4 accesses need)."""
    return t.data_ptr() % 16 == 0 and (t.shape[0] <= 1 or t.stride(0) % 4 == 0)


class EdgeMask(object):
    """The edge mask of one adjacency (--edge_dropout; the contract: include/sgcn.h SGCN_EDGE_SITE), shared by a StaticMatrix
    and its transpose: ``keep`` = 1 - p, and between begin_step and end_step the step's ``key``.  ``serial`` counts the
    steps: an array drawn for an earlier step is drawn again before it is read."""

    def __init__(self, p):
        self.keep, self.key, self.serial = 1.0 - float(p), None, 0


class StaticMatrix(object):
    """A static sparse matrix on the device, multiplied many times: ``kernel`` is 'rows' (the row-gather kernel on a
    DeviceCSR), 'cs' (column sweep) or 'lds' (LDS-staged sweep + residual), or 'auto': static_kernel_for(nnz, d, products)
    with ``products`` the number of times the plan will run -- and for a large graph with communities and no plan cache
    ops.LdsSweepCSR.for_graph.  ``d`` is the operand width the choice (and the column sweep's lane grouping) is made for.
    Every static-graph product of the package is planned, tuned and run here.

    ``bf16``: every product rounds ``x`` to nearest even into a bfloat16 scratch table -- one per operand width, allocated
    once and reused every epoch -- and runs the kernel's bfloat16-operand form: half the operand's bytes per nonzero, the
    sums and ``out`` fp32, bit for bit the fp32 product of the rounded operand.  The transpose inherits it.  The LDS sweep
    has no such form: forcing it is refused, 'auto' never picks it.

    ``edge_dropout`` p > 0: the matrix keeps its base value arrays untouched and owns, per value array a product can read
    (its plan's; the row kernel's CSR where ``kernel_for`` falls back to it; the same for the transpose), the entries' pair
    keys and one re-drawn array.  ``begin_step(key)`` .. ``end_step()`` bracket a training step: in between, every product
    of the matrix and of its transpose reads values re-drawn under ``key`` -- each array once per step, before its first
    use --, outside the base values.  The values stay fp32, so ``bf16`` is unaffected; the plan cache stores base values;
    the LDS sweep's unit plans have no value array: refused like ``bf16``."""

    bf16 = False          # (the fp32 operand is the default of every instance)
    edge = None           # (no edge mask)

    def __init__(self, a, device, kernel='auto', products=1, d=128, cache_path=None, _transpose_of=None, bf16=False,
                 edge_dropout=0.0):
        a = a.tocsr()
        self.bf16, self._scratch, self._widened = bool(bf16), {}, {}
        if self.bf16 and kernel == 'lds':
            raise ValueError("the LDS-staged sweep has no bfloat16-operand form")
        if _transpose_of is not None:
            self.edge = _transpose_of.edge
        elif edge_dropout:
            if not 0.0 < float(edge_dropout) < 1.0:
                raise ValueError("edge_dropout must lie in [0, 1), got %r" % (edge_dropout,))
            self.edge = EdgeMask(edge_dropout)
        if self.edge is not None and kernel == 'lds':
            raise ValueError("the LDS-staged sweep runs unit plans: there is no value array to re-draw under an edge mask")
        self._redrawn = {}
        self.a, self.device, self.shape, self.nnz = a, device, (int(a.shape[0]), int(a.shape[1])), int(a.nnz)
        self.requested, self.products, self.d_hint, self.cache_path = kernel, int(products), int(d), cache_path
        self._transpose = _transpose_of
        self._rows = self._plan = None
        self._tuned = set()
        self.plan_from_cache = False
        self.kernel = self._choose(kernel)
        if self.edge is not None:
            self._edge_slot(self.kernel)         # the pair keys of the matrix's own plan: decoded and uploaded once, here

    def _choose(self, kernel):
        a, d = self.a, self.d_hint
        if kernel == 'rows':
            return 'rows'
        if kernel == 'lds':
            labels, _ = ops.reorder_labels(a)
            self._plan = ops.LdsSweepCSR(a, self.device, host=ops.LdsSweepCSR.auto_host(a, labels))
            return 'lds'
        if kernel == 'auto':
            if static_kernel_for(self.nnz, d, self.products) == 'rows':
                return 'rows'
            # a large graph WITH communities (>= 90 % of its nonzeros inside tiles that share their columns): the LDS-staged
            # sweep + the column sweep on the rest; anything else: the column sweep alone
            if self.cache_path is None and self.nnz >= 2000000 and d >= 128 and not self.bf16 and self.edge is None:
                self._plan = ops.LdsSweepCSR.for_graph(a, self.device)
                if self._plan is not None:
                    return 'lds'
        G = ops.ColumnSweepCSR.choose_g(d, self.nnz / max(self.shape[0], 1), self.shape[0])
        # (under an edge mask the plan's value array is re-drawn every step: it must have one)
        values = {} if self.edge is None else {"dictionary": False}
        self._plan, self.plan_from_cache = ops.ColumnSweepCSR.cached(a, self.device, self.cache_path, G=G, **values)
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

    # ---- edge dropout ------------------------------------------------------------------------------------------------------
    def _edge_slot(self, k):
        """What kernel ``k`` ('rows' or the matrix's own sweep) reads inside a step: the base value array of its plan, the
        pair key of every stored entry (decoded from the plan's own records, ops.plan_entries), the array the step's
        values are drawn into and -- for the row kernel -- the CSR that carries it."""
        slot = self._redrawn.get(k)
        if slot is None:
            plan = self.rows_csr if k == 'rows' else self._plan
            # (the row kernel's CSR is the host matrix in its stored order: nothing to read back from the device)
            entries = ops.csr_entries(self.a.indptr, self.a.indices) if k == 'rows' else ops.plan_entries(plan)
            pair = torch.from_numpy(ops.edge_pair_keys(*entries).view(np.int32)).to(self.device)
            out = torch.empty_like(plan.val)
            csr = ops.DeviceCSR(plan.shape, plan.rowptr, plan.col, out, plan.plan, host_rowptr=plan.host_rowptr) \
                if k == 'rows' else None
            slot = self._redrawn[k] = dict(base=plan.val, pair=pair, out=out, csr=csr, serial=0)
        return slot

    def _edge_values(self, k):
        """None outside a step; inside one, kernel k's slot with the step's values drawn (once per step and array)."""
        e = self.edge
        if e is None or e.key is None:
            return None
        slot = self._edge_slot(k)
        if slot['serial'] != e.serial:
            ops.edge_revalue(slot['base'], slot['pair'], e.key, e.keep, out=slot['out'])
            slot['serial'] = e.serial
        return slot

    def begin_step(self, key):
        """From here to end_step the products of this matrix and of its transpose read values re-drawn under ``key``: the
        matrix's own array now, ahead of the forward; every other one before its first use in the step."""
        e = self.edge
        if e is not None:
            e.key, e.serial = int(key) & 0xFFFFFFFF, e.serial + 1
            self._edge_values(self.kernel)

    def end_step(self):
        """The base values are back in effect (nothing was written to them)."""
        if self.edge is not None:
            self.edge.key = None

    def _rows_now(self):
        slot = self._edge_values('rows')
        return self.rows_csr if slot is None else slot['csr']

    def _autotune(self, x, d):
        key = (d, x.dtype == torch.bfloat16)
        if key in self._tuned:
            return
        self._tuned.add(key)
        if self.kernel == 'lds':
            r = self._plan.residual
            if isinstance(r, ops.ColumnSweepCSR) and d not in r.pace:
                self._plan.autotune(x, d=d)
        elif d not in self._plan.clock(x.dtype == torch.bfloat16).pace:
            self._plan.autotune(x, d=d)                # once per plan, width and operand type; stored with a cached plan
            self._plan.store_if_cached()

    def operand(self, x, kernel=None):
        """What ``kernel`` (default: the matrix's own) gathers from: ``x`` itself, or under ``bf16`` this matrix's scratch
        table of x's width holding x rounded to nearest even (ops.operand_round: sgcn_scatter_rows_h16 with no index).  An
        ``x`` that is bfloat16 already (the feature table under --feature_dtype bf16) is handed through as it is -- no
        rounding pass, no scratch table -- whatever ``bf16`` says; only a product on the LDS sweep, which has no bfloat16
        form, widens it (exactly) into an fp32 scratch table, and says so once."""
        b16 = x.dtype == torch.bfloat16
        if not (self.bf16 or b16):
            return x
        n, d = int(x.shape[0]), int(x.shape[1])
        if n != self.shape[1]:
            raise ValueError("the operand has %d rows, the matrix %d columns" % (n, self.shape[1]))
        if b16:
            if (self.kernel if kernel is None else kernel) != 'lds':
                return x
            tab = self._widened.get(d)
            if tab is None:
                print("[sgcn] the LDS-staged sweep has no bfloat16-operand form: a bfloat16 operand of width %d is widened into "
                      "an fp32 scratch table of its size on every product (--full_batch_kernel cs or rows reads it directly)" % d)
                tab = self._widened[d] = torch.empty((n, (d + 3) // 4 * 4), dtype=torch.float32, device=x.device)[:, :d]
            return ops.history_widen(x, out=tab)
        tab = self._scratch.get(d)
        if tab is None:
            tab = self._scratch[d] = ops.history_alloc(n, d, x.device, bf16=True)
        return ops.operand_round(x, out=tab)

    def kernel_for(self, x, out=None):
        """The kernel one product runs on: the matrix's own, or the row kernel where an operand's rows are not 16-byte
        aligned (a width that is not a multiple of 4: no copy is made for the sweep's sake).  Under ``bf16`` the kernel
        reads the scratch table, which is always aligned: only the width and ``out`` decide -- and so for a bfloat16 ``x``."""
        if self.kernel == 'rows':
            return 'rows'
        d = int(x.shape[1])
        b16 = self.bf16 or x.dtype == torch.bfloat16        # (a bfloat16 x: a pitch-8 table, or on 'lds' its aligned scratch)
        if d % 4 or (not b16 and not _aligned(x)) or (out is not None and not _aligned(out)):
            return 'rows'
        return self.kernel

    def multiply(self, x, out=None, beta=0.0, kernel=None):
        """out = A x + beta out on ``kernel`` -- the matrix's own, or 'rows' -- with ``x`` as it is handed over: no alignment
        decision and no rounding (``product`` makes both; train.pp_products hands over a width that is no multiple of 4 on
        a padded pitch, which the sweeps take).  A sweep tunes its clock on the first product of a width and operand type."""
        k, d = self.kernel if kernel is None else kernel, int(x.shape[1])
        if k not in ('rows', self.kernel):
            raise ValueError("this matrix runs on %r or on the row kernel, not on %r" % (self.kernel, k))
        if k == 'rows':
            return ops.spmm(self._rows_now(), x, out=out, beta=beta)
        self._autotune(x, d)
        slot = self._edge_values(k)
        if slot is None:
            return (ops.spmm_lds if k == 'lds' else ops.spmm_cs)(self._plan, x, out=out, beta=beta, d=d)
        self._plan.live_val = slot['out']         # (the sweep reads the step's values for this product only)
        try:
            return ops.spmm_cs(self._plan, x, out=out, beta=beta, d=d)
        finally:
            self._plan.live_val = None

    def product(self, x, out=None, add=None, add_rows=0):
        """out = A x (+ add on the first ``add_rows`` rows), the keyword set of ops.spmm that PlainAggregator uses.  The row
        kernel adds in its epilogue; the sweep kernels have none: the addend is stored into ``out`` and the product runs
        with beta = 1."""
        M, d = self.shape[0], int(x.shape[1])
        k = self.kernel_for(x, out)
        x = self.operand(x, k)
        if add is None:
            return self.multiply(x, out=out, kernel=k)
        if k == 'rows':
            return ops.spmm(self._rows_now(), x, out=out, add=add, add_rows=add_rows)
        if out is None:
            out = torch.empty((M, d), dtype=torch.float32, device=x.device)
        r = int(add_rows)
        out[:r].copy_(add[:r])
        if r < M:
            out[r:].zero_()
        return self.multiply(x, out=out, beta=1.0, kernel=k)

    # ---- the element-wise maximum (--aggregator max) -------------------------------------------------------------------------
    def max_product(self, x, out=None, want_arg=True):
        """(out, arg) of ops.spmax over this matrix's PATTERN: out[i] = the element-wise maximum of the rows of ``x`` that
        row i stores an entry for (its own where the normalisation put a diagonal entry), arg the winners' column ids for
        ``max_backward`` (None with ``want_arg=False``).  Reads the row kernel's CSR -- pattern and segment plan -- only: no
        sweep plan, no value array, no operand rounding."""
        if self.bf16 or x.dtype != torch.float32:
            raise ValueError("the element-wise maximum has no bfloat16-operand form")
        if self.edge is not None:
            raise ValueError("the element-wise maximum has no edge-masked form")
        return ops.spmax(self.rows_csr, x, out=out, want_arg=want_arg)

    def max_backward(self, g, arg, add=None, add_rows=0):
        """Called on the TRANSPOSE of the matrix whose ``max_product`` gave ``arg``: the gradient of that maximum with respect
        to its operand, out[j] = the sum of g[i] over the rows i whose winner was j, in ascending i (+ add on the first
        ``add_rows`` rows) -- ops.spmax_bwd, a gather over this matrix's pattern."""
        if self.bf16 or self.edge is not None:
            raise ValueError("the element-wise maximum has no bfloat16-operand and no edge-masked form")
        return ops.spmax_bwd(self.rows_csr, g, arg, add=add, add_rows=add_rows)

    # ---- softmax dot-product attention (--aggregator attn) -------------------------------------------------------------------
    def _attn_staged(self, role, t, d, fill=True):
        """``t`` (n x d) in this matrix's 16-byte-aligned scratch table of that role and width -- one table per (role, width),
        allocated on first use and reused, as the ``_scratch`` tables of the bf16 operand are."""
        key = ('attn', role, int(t.shape[0]), d)
        tab = self._scratch.get(key)
        if tab is None:
            tab = self._scratch[key] = torch.empty((int(t.shape[0]), (d + 3) // 4 * 4), dtype=torch.float32,
                                                   device=t.device)[:, :d]
        if fill:
            tab.copy_(t)
        return tab

    def _attn_refuse(self, x):
        if self.bf16 or x.dtype != torch.float32:
            raise ValueError("attention has no bfloat16-operand form")
        if self.edge is not None:
            raise ValueError("attention has no edge-masked form")

    def _attn_forward(self, launch, x, out, heads):
        """``launch(x, out)`` -> (res, lse) on operands the kernel can hold: it takes d <= 256 * VW columns, so where an
        operand's alignment -- not the head width, which staging cannot widen -- narrows the vectors so far that d is over
        that, ``x`` is staged into an aligned scratch table, and an ``out`` view of that kind is computed aligned and copied."""
        d = int(x.shape[1])
        if d > ops.ATTN_MAX_VECTORS * ops.attn_vw(d, x, out, heads=heads):
            best = ops.attn_vw(d, heads=heads)            # what aligned operands would get
            if ops.attn_vw(d, x, heads=heads) < best:
                x = self._attn_staged('x', x, d)
            if out is not None and ops.attn_vw(d, out, heads=heads) < best:
                res, lse = launch(x, self._attn_staged('out', out, d, fill=False))
                out.copy_(res)
                return out, lse
        return launch(x, out)

    def _attn_backward_operands(self, heads, x, g, out_fwd, add):
        """The backward's four tables (``add`` may be None), each staged where ``_attn_forward`` would stage it."""
        d = int(x.shape[1])
        tabs = dict(x=x, g=g, out_fwd=out_fwd, add=add)
        if d > ops.ATTN_MAX_VECTORS * ops.attn_vw(d, x, g, out_fwd, add, heads=heads):
            best = ops.attn_vw(d, heads=heads)
            for role, t in tabs.items():
                if t is not None and ops.attn_vw(d, t, heads=heads) < best:
                    tabs[role] = self._attn_staged(role, t, d)
        return tabs['x'], tabs['g'], tabs['out_fwd'], tabs['add']

    def attn_product(self, x, scale, out=None, want_lse=True, heads=1, keep=1.0, key=0):
        """(out, lse) of ops.spattn over this matrix's PATTERN with the queries x[:M]: out[i] = the rows of ``x`` that row i
        stores an entry for, weighed by softmax_j(scale * <x[i], x[j]>); lse the rows' log-sum-exp for ``attn_backward``
        (None with ``want_lse=False``).  Reads the row kernel's CSR -- pattern and segment plan -- only.  Misaligned operands
        too wide for the kernel (602-wide features on a pitch of 602 floats: VW = 2) are staged (``_attn_forward``).
        ``heads``: ops.spattn's; lse is then (M, heads).  ``keep``, ``key``: ops.spattn's dropout on the coefficients,
        passed through (keep = 1: none)."""
        self._attn_refuse(x)
        # (the keywords are passed only when set: without dropout the call is the one ops.spattn has always taken)
        drop = dict(keep=keep, key=key) if keep != 1.0 else {}
        return self._attn_forward(lambda x, out: ops.spattn(self.rows_csr, x, scale=scale, out=out, want_lse=want_lse, heads=heads,
                                                            **drop), x, out, heads)

    def attn_backward(self, x, g, out_fwd, lse, scale, add=None, add_rows=0, heads=1, keep=1.0, key=0):
        """Called on the matrix whose ``attn_product(x, scale)`` gave ``out_fwd`` and ``lse``: the gradient with respect to
        ``x`` (as keys / values AND as queries) for g = dL/dout, + add on the first ``add_rows`` rows -- ops.spattn_bwd, a
        gather over this matrix's pattern and one over its transpose's.  Operands are staged as in ``attn_product``.
        ``keep``, ``key``: those of the forward."""
        self._attn_refuse(x)
        x, g, out_fwd, add = self._attn_backward_operands(heads, x, g, out_fwd, add)
        return ops.spattn_bwd(self.rows_csr, self.transpose.rows_csr, x, None, g, out_fwd, lse, scale, add=add, add_rows=add_rows,
                              heads=heads, **(dict(keep=keep, key=key) if keep != 1.0 else {}))[1]

    # ---- learned additive scores (--attn_score gat) ------------------------------------------------------------------------
    def gat_product(self, x, a, slope, out=None, want_lse=True, heads=1, keep=1.0, key=0):
        """(out, lse, S) of ops.gat_scores + ops.spgat over this matrix's PATTERN: S = the score table of ``x`` under the
        layer's vectors ``a`` (2, d), out[i] = the rows of ``x`` that row i stores an entry for, weighed by
        softmax_j(LeakyReLU(S[i, h] + S[j, H + h])) per head h.  lse (M, H) and S are what ``gat_backward`` needs (lse is None
        with ``want_lse=False``).  Operands are staged as in ``attn_product``, and the same operands are refused."""
        self._attn_refuse(x)
        H, M = int(heads), self.shape[0]
        S = ops.gat_scores(x, a, heads=H)
        res, lse = self._attn_forward(lambda x, out: ops.spgat(self.rows_csr, x, S[:M, :H], S[:, H:], slope=slope, out=out,
                                                               want_lse=want_lse, heads=H, keep=keep, key=key), x, out, H)
        return res, lse, S

    def gat_backward(self, x, a, S, g, out_fwd, lse, slope, add=None, add_rows=0, heads=1, keep=1.0, key=0, need_dx=True):
        """Called on the matrix whose ``gat_product(x, a, slope)`` gave ``out_fwd``, ``lse`` and ``S``: (dX or None, da) for
        g = dL/dout -- ops.spgat_bwd (a gather over this matrix's pattern, one over its transpose's, the addend in the
        second one's epilogue), then ops.gat_scores_bwd, which adds the scores' share into dX and reduces da (2, d).
        ``need_dx=False``: dX is not formed (the launch over the transpose still runs, for dV)."""
        self._attn_refuse(x)
        H, M = int(heads), self.shape[0]
        x, g, out_fwd, add = self._attn_backward_operands(H, x, g, out_fwd, add if need_dx else None)
        dB, dU, dV, _ = ops.spgat_bwd(self.rows_csr, self.transpose.rows_csr, x, S[:M, :H], S[:, H:], g, out_fwd, lse, slope=slope,
                                      add=add, add_rows=add_rows if need_dx else 0, heads=H, keep=keep, key=key)
        da = ops.gat_scores_bwd(x, a, dU, dV, dx=dB if need_dx else None, heads=H)
        return (dB if need_dx else None), da

    def describe(self, d):
        """What train.pp_products records of a product of width d: where the plan came from, the sweep clock (the column
        sweep only), the kernel variant, the product count the kernel was chosen for."""
        cs = self.kernel == 'cs'
        kernel = "sgcn::spmm_seg_kernel" if self.kernel == 'rows' else \
            self._plan.variant(d, self.bf16) if cs else self._plan.variant(d)
        return dict(plan_from_cache=self.plan_from_cache, pace=self._plan.clock(self.bf16).pace.get(d) if cs else None,
                    kernel=kernel, products=self.products)


def model_matrix(adj, device, model, products, cache_path=None, kernel=None, bf16=False, layers=None, edge_dropout=0.0):
    """The StaticMatrix of ``adj`` for the aggregation layers of ``model``: the kernel of --full_batch_kernel unless one is
    given, the plan made for the widest operand -- agg0_dim at layer 0, --hidden1 behind it -- of the first ``layers``
    aggregation layers (default: all; an exact history pass counts one less).  ``products`` is the caller's to know."""
    n = model.L if layers is None else max(int(layers), 1)
    widths = [model.agg0_dim if l == 0 else FLAGS.hidden1 for l in range(n)]
    # (the keyword is passed only when set: with the flag off the call is the one the matrix classes -- the recording
    # stand-ins of the CPU tests among them -- have always taken)
    edge = dict(edge_dropout=edge_dropout) if edge_dropout else {}
    if kernel is None and getattr(FLAGS, 'aggregator', 'sum') in ('max', 'attn'):
        # every aggregation of the model is a maximum / an attention over the pattern (max_product and attn_product read
        # rows_csr and its segment plan):
        # no column-sweep or LDS plan, tune or cache file is made for products that never run
        kernel = 'rows'
    return StaticMatrix(adj, device, FLAGS.full_batch_kernel if kernel is None else kernel, products,
                        max(widths or [FLAGS.hidden1]), cache_path, bf16=bf16, **edge)


class StaticCur(object):
    """``model.cur`` of a static batch (the attributes of models.DevFeed the eager layer path reads)."""
    __slots__ = ("fields", "host_fields", "scales", "labels", "rows", "adj", "fadj", "ffields", "inputs", "sizes")


class StaticBatch(object):
    """The whole graph as one batch: ``fields[l] = arange(N)`` and ``scales[l] = 1`` for every l, ``labels`` the N x C
    table, ``adj[l]`` ONE shared StaticMatrix, and ``rows`` the vertices the loss runs over -- ascending and unique
    (checked here, on the host: the loss kernel trusts it).  Without ``labels`` and ``rows`` (both None): a batch for
    forward passes only, with no label table and no loss rows on the device."""

    def __init__(self, matrix, labels, rows, L, device=None):
        N = int(matrix.shape[0])
        if matrix.shape[0] != matrix.shape[1]:
            raise ValueError("a static batch needs a square (vertex x vertex) matrix")
        if labels is None and rows is not None:
            raise ValueError("loss rows need the label table they index")
        if labels is not None and int(labels.shape[0]) != N:
            raise ValueError("labels has %d rows, the graph %d vertices" % (int(labels.shape[0]), N))
        device = device if device is not None else getattr(matrix, 'device', None)
        self.N, self.L, self.matrix, self.device = N, int(L), matrix, device
        self.dropout = 0.0
        self.host_field = np.arange(N, dtype=np.int32)
        to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)      # noqa: E731
        self.host_rows = self.rows = self.labels = None
        if labels is not None:
            self.host_rows = ops.check_loss_rows(rows, N)
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
        if self.labels is None:
            raise ValueError("a forward-only static batch has no loss rows")
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


# ---- Cluster-GCN steps on device-cut subgraphs (--full_batch_parts) ----------------------------------------------------------
PART_NORMS = _CHOICES['full_batch_part_norm']


def check_full_batch_parts(flags=None, num_vertices=None):
    """(P, q, norm) of --full_batch_parts / --full_batch_parts_per_step / --full_batch_part_norm (P = 0: off), with what a part
    batch has no kernel or no meaning for refused.  Needs no device; a sibling of check_full_batch, called beside it -- and
    once more with ``num_vertices`` when the graph is known."""
    f = FLAGS if flags is None else flags
    P, q = getattr(f, 'full_batch_parts', 0), getattr(f, 'full_batch_parts_per_step', 1)
    norm = getattr(f, 'full_batch_part_norm', 'rows')
    for name, v in (('full_batch_parts', P), ('full_batch_parts_per_step', q)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("--%s must be an integer, got %r" % (name, v))
    P, q = int(P), int(q)
    if P < 0:
        raise ValueError("--full_batch_parts must be >= 0 (0 = off: one step over the whole graph), got %d" % P)
    if norm not in PART_NORMS:
        raise ValueError("--full_batch_part_norm must be one of %s, got %r" % ('/'.join(PART_NORMS), norm))
    if P == 0:
        return 0, q, norm
    if not f.full_batch:
        raise ValueError("--full_batch_parts needs --full_batch: its steps are exact steps on induced subgraphs of the "
                         "training adjacency, and no other mode trains on that matrix")
    if not 1 <= q <= P:
        raise ValueError("--full_batch_parts_per_step must lie in [1, --full_batch_parts = %d], got %d" % (P, q))
    if float(getattr(f, 'edge_dropout', 0.0)) > 0:
        raise ValueError("--full_batch_parts is not supported with --edge_dropout: dropping the edges between parts already "
                         "is edge sampling, and a part batch carries no edge mask")
    if getattr(f, 'feature_dtype', 'fp32') == 'bf16':
        raise ValueError("--full_batch_parts is not supported with --feature_dtype bf16: a step gathers its rows of the "
                         "feature table into an fp32 table; there is no bfloat16-table form yet")
    if f.full_batch_kernel in ('cs', 'lds'):
        raise ValueError("--full_batch_parts is not supported with --full_batch_kernel %s: a part batch is cut anew every "
                         "step and runs the row kernels (auto or rows); no sweep plan is made for it" % f.full_batch_kernel)
    if num_vertices is not None and P > int(num_vertices):
        raise ValueError("--full_batch_parts %d is more than the graph's %d vertices: every part holds at least one"
                         % (P, int(num_vertices)))
    return P, q, norm


def _check_part_tables(flags, flag, refuse_aggregator, stored="rows", kernels="kernels'"):
    """(on, bf16) of the part-step flag ``flag`` / --history_dtype: what every two-table mode refuses, in one order -- no parts,
    what ``refuse_aggregator(f, agg)`` speaks for, --reverse, --full_batch_dtype bf16, an unknown --history_dtype."""
    f = FLAGS if flags is None else flags
    if not bool(getattr(f, flag, False)):
        return False, False
    if int(getattr(f, 'full_batch_parts', 0) or 0) <= 0:
        raise ValueError("--%s needs --full_batch_parts > 0: it is the estimator of a part step's "
                         "out-of-part neighbours, and no other mode has them" % flag)
    refuse_aggregator(f, getattr(f, 'aggregator', 'sum'))
    if getattr(f, 'reverse', False):
        raise ValueError("--%s is not supported with --reverse: the aggregator's input would be a "
                         "dropout-masked table, and the stored %s would hold one step's mask" % (flag, stored))
    if getattr(f, 'full_batch_dtype', 'fp32') == 'bf16':
        raise ValueError("--%s is not supported with --full_batch_dtype bf16: the pull %s fresh "
                         "operand is fp32 (--history_dtype bf16 halves the stored rows instead)" % (flag, kernels))
    hd = getattr(f, 'history_dtype', 'fp32')
    if hd not in _CHOICES['history_dtype']:
        raise ValueError("--history_dtype must be one of %s, got %r" % ('/'.join(_CHOICES['history_dtype']), hd))
    return True, hd == 'bf16'


def check_part_history(flags=None):
    """(on, bf16) of --full_batch_part_history / --history_dtype: part steps that read stored rows for their out-of-part
    neighbours (GNNAutoScale), with what the two-table product has no kernel or no meaning for refused.  Needs no device; a
    sibling of check_full_batch_parts, called beside it."""
    def aggregator(f, agg):
        if agg != 'sum':
            raise ValueError("--full_batch_part_history is not supported with --aggregator %s: the maximum and the attention "
                             "kernels gather from one table; a two-table form is a follow-up" % agg)
    return _check_part_tables(flags, 'full_batch_part_history', aggregator, kernels="kernel's")


def check_part_pull(flags=None):
    """(on, bf16) of --full_batch_part_pull / --history_dtype: part steps of the sum AND the attention aggregator that read
    stored rows for their out-of-part neighbours.  With --aggregator sum it is --full_batch_part_history exactly; with
    --aggregator attn every aggregation layer attends over every stored neighbour (ops.spattn_pull).  What the two-table
    kernels have no form or no meaning for is refused.  Needs no device; called beside check_part_history, which keeps its
    own contract and, with both flags on, speaks first."""
    def aggregator(f, agg):
        if agg == 'max':
            raise ValueError("--full_batch_part_pull is not supported with --aggregator max: the maximum kernel gathers from one "
                             "table; a two-table maximum is a follow-up")
        if agg not in ('sum', 'attn'):
            raise ValueError("--full_batch_part_pull is not supported with --aggregator %s" % agg)
        if agg == 'attn':
            if getattr(f, 'attn_score', 'dot') == 'gat':
                raise ValueError("--full_batch_part_pull is not supported with --attn_score gat: its score table would need "
                                 "stale scores for the out-of-part neighbours; a two-table form is a follow-up")
            if float(getattr(f, 'attn_dropout', 0.0) or 0.0) > 0:
                raise ValueError("--full_batch_part_pull is not supported with --attn_dropout > 0: in this version the mask of "
                                 "out-of-part entries is not defined")
    return _check_part_tables(flags, 'full_batch_part_pull', aggregator)


def check_part_pull_gat(flags=None):
    """(on, bf16) of --full_batch_part_pull_gat / --history_dtype: part steps of the attention aggregator with learned
    additive scores (--attn_score gat) that read stored rows AND stored destination scores for their out-of-part
    neighbours (ops.spgat_pull).  What the two-table kernels have no form or no meaning for is refused.  Needs no device;
    called beside check_part_pull, which keeps its own contract and, with both flags on, speaks first."""
    def aggregator(f, agg):
        if agg != 'attn':
            raise ValueError("--full_batch_part_pull_gat needs --aggregator attn (got %s): it is the two-table form of the "
                             "attention with learned scores; --full_batch_part_pull serves the sum" % agg)
        if getattr(f, 'attn_score', 'dot') != 'gat':
            raise ValueError("--full_batch_part_pull_gat needs --attn_score gat: --full_batch_part_pull is the two-table form "
                             "of dot-product attention")
        if float(getattr(f, 'attn_dropout', 0.0) or 0.0) > 0:
            raise ValueError("--full_batch_part_pull_gat is not supported with --attn_dropout > 0: in this version the mask of "
                             "out-of-part entries is not defined")
    return _check_part_tables(flags, 'full_batch_part_pull_gat', aggregator, stored="rows and scores")


def check_part_pull_max(flags=None):
    """(on, bf16) of --full_batch_part_pull_max / --history_dtype: part steps of the maximum aggregator that read stored rows
    for their out-of-part neighbours (ops.spmax_pull): every aggregation layer takes the element-wise maximum over every
    stored entry of its rows.  What the two-table kernel has no form or no meaning for is refused.  Needs no device; called
    beside check_part_pull_gat.  The three older checks keep their own contracts and, where the aggregator is not theirs,
    speak first."""
    def aggregator(f, agg):
        if agg != 'max':
            raise ValueError("--full_batch_part_pull_max needs --aggregator max (got %s): it is the two-table form of the "
                             "element-wise maximum; --full_batch_part_pull serves the sum and dot-product attention, "
                             "--full_batch_part_pull_gat the learned scores" % agg)
        for other in ('full_batch_part_history', 'full_batch_part_pull', 'full_batch_part_pull_gat'):
            if getattr(f, other, False):
                raise ValueError("--full_batch_part_pull_max is not supported together with --%s: not together with "
                                 "--full_batch_part_history, --full_batch_part_pull or --full_batch_part_pull_gat, which "
                                 "are the two-table forms of the other aggregators" % other)
    return _check_part_tables(flags, 'full_batch_part_pull_max', aggregator, kernels="kernel's")


def partition(adj, P, seed=1):
    """The vertices of ``adj`` cut into P parts, as P ascending int32 id arrays; deterministic in (adj, P, seed).

    The communities of ops.reorder_labels(adj, seed=seed) (label propagation on the host), every community larger than
    ceil(N / P) cut into id-contiguous pieces of at most that size, the pieces packed largest first into the currently
    lightest of P bins (ties: the earlier piece, the lower bin).  Where that leaves fewer than P pieces the largest is
    halved until there are P, so that no part is empty."""
    N, P = int(adj.shape[0]), int(P)
    if not 1 <= P <= N:
        raise ValueError("partition: P must lie in [1, %d], got %d" % (N, P))
    comm, _ = ops.reorder_labels(adj, seed=int(seed))
    order = np.argsort(comm, kind='stable')                   # by community, ids ascending inside one
    cuts = np.flatnonzero(np.diff(comm[order])) + 1
    limit = -(-N // P)
    pieces = []
    for members in np.split(order, cuts):
        pieces.extend(members[k:k + limit] for k in range(0, len(members), limit))
    while len(pieces) < P:
        k = max(range(len(pieces)), key=lambda i: (len(pieces[i]), -i))
        big = pieces[k]
        pieces[k:k + 1] = [big[:len(big) // 2], big[len(big) // 2:]]
    bins, weight = [[] for _ in range(P)], [0] * P
    for k in sorted(range(len(pieces)), key=lambda i: (-len(pieces[i]), i)):
        j = min(range(P), key=lambda i: (weight[i], i))
        bins[j].append(pieces[k])
        weight[j] += len(pieces[k])
    return [np.sort(np.concatenate(b)).astype(np.int32) for b in bins]


class PartSchedule(object):
    """Which parts a step unites: ``epoch(e)`` is a permutation of the parts seeded by (seed, e), cut into consecutive groups
    of q (the last one may be shorter) -- ceil(P / q) steps that use every part exactly once.  ``groups(e)`` are the groups'
    part indices, ``epoch(e)`` the sorted union of each group's vertices."""

    def __init__(self, parts, q, seed=1):
        self.parts, self.q, self.seed = [np.asarray(p, dtype=np.int32) for p in parts], int(q), int(seed)
        if not 1 <= self.q <= len(self.parts):
            raise ValueError("PartSchedule: q must lie in [1, %d], got %d" % (len(self.parts), self.q))

    def __len__(self):
        return -(-len(self.parts) // self.q)

    def groups(self, e):
        perm = np.random.RandomState([self.seed & 0xFFFFFFFF, int(e) & 0xFFFFFFFF]).permutation(len(self.parts))
        return [perm[k:k + self.q] for k in range(0, len(perm), self.q)]

    def epoch(self, e):
        return [np.sort(np.concatenate([self.parts[j] for j in g])) for g in self.groups(e)]


class InducedMatrix(StaticMatrix):
    """The StaticMatrix of a part batch, over a block that ops.csr_induce cut on the device (a DeviceCSR with its transpose):
    ``kernel`` is 'rows', ``rows_csr`` the block, ``transpose`` an InducedMatrix over the transposed block.  There is no host
    matrix, no sweep plan, no plan cache and no edge mask; ``product``, ``max_product`` / ``max_backward``, ``attn_product`` /
    ``attn_backward`` and ``gat_product`` / ``gat_backward`` are the inherited methods on the row kernel's CSR.  ``bf16``:
    as StaticMatrix (--full_batch_dtype)."""

    def __init__(self, block, device=None, bf16=False, _transpose_of=None):
        if getattr(block, 'transpose', None) is None:
            raise ValueError("an InducedMatrix needs a DeviceCSR with its transpose (ops.csr_induce)")
        self.bf16, self._scratch, self._widened, self._redrawn = bool(bf16), {}, {}, {}
        self.a, self.device = None, (device if device is not None else block.val.device)
        self.shape, self.nnz = (int(block.shape[0]), int(block.shape[1])), int(block.nnz)
        self.requested = self.kernel = 'rows'
        self.products, self.d_hint, self.cache_path = 1, 0, None
        self._rows, self._plan, self._transpose = block, None, _transpose_of
        self._tuned, self.plan_from_cache = set(), False

    @property
    def transpose(self):
        if self._transpose is None:
            self._transpose = InducedMatrix(self._rows.transpose, self.device, self.bf16, _transpose_of=self)
        return self._transpose

    def describe(self, d):
        return dict(plan_from_cache=False, pace=None, kernel="sgcn::spmm_seg_kernel", products=self.products)


class PulledMatrix(InducedMatrix):
    """The matrix of a part step under --full_batch_part_history: the InducedMatrix of the 'keep' block A[S, S] -- ``transpose``
    and every inherited product are that block's, so the backward, ``A.transpose.product(g, ...)``, sees in-part entries only
    and stored rows are constants -- which also carries what the forward reads instead: the RESIDENT adjacency, the ids of S
    on the device, their position map (the block's, ops.csr_induce) and the model's history tables, one per aggregation
    layer.  ``pull_product(x, l)`` is the neighbour sum of layer l over EVERY stored entry of the rows of S (ops.spmm_pull:
    fresh rows of ``x`` for columns in S, rows of table l for the others); ``push(x, l)`` then stores the layer's input rows
    into table l (ops.scatter_rows) -- columns in S never read the table, so push-after-pull is safe.  A table that is not
    ``owned`` (the resident feature table under an aggregation layer with no layer in front of it) is exact and never written.
    ``pull_attn_product`` / ``pull_attn_backward`` are the attention over the same entries (--full_batch_part_pull).  The pull
    launches take their operands as they are: nothing is staged, so a table too wide for its alignment (602 columns on a pitch
    of 602 floats) is refused with the kernels' width message.  These methods take the layer's index and push nothing; an
    aggregation layer is handed ``layer(l)``, which pulls, then pushes, behind StaticMatrix's one-table signatures.
    ``pull_max`` (--full_batch_part_pull_max; off by default): the switch ``layer(l).max_product`` reads -- on, the maximum
    is ``pull_max_product``, the element-wise maximum over the same entries (ops.spmax_pull) with winners recorded for the
    block's own ``transpose.max_backward``; off, the inherited ``max_product``, the block's in-part maximum."""

    def __init__(self, block, resident, ids_dev, tables, owned, device=None, scores=None, pull_max=False):
        if getattr(block, 'map', None) is None:
            raise ValueError("a PulledMatrix needs the block's position map (ops.csr_induce)")
        super(PulledMatrix, self).__init__(block, device, bf16=False)
        if int(resident.shape[0]) != int(resident.shape[1]) or int(ids_dev.shape[0]) != self.shape[0]:
            raise ValueError("a PulledMatrix needs the square resident matrix and the %d ids of its block" % self.shape[0])
        if len(tables) != len(owned):
            raise ValueError("a PulledMatrix needs one owned flag per history table")
        self.resident, self.ids_dev, self.map, self.tables, self.owned = resident, ids_dev, block.map, list(tables), list(owned)
        # --full_batch_part_pull_gat: one N x H fp32 table of last-seen destination scores per aggregation layer, always owned
        if scores is not None and len(scores) != len(tables):
            raise ValueError("a PulledMatrix needs one score table per history table")
        self.scores = None if scores is None else list(scores)
        self.pull_max = bool(pull_max)

    def pull_product(self, x, l, out=None):
        return ops.spmm_pull(self.resident, self.ids_dev, self.map, x, self.tables[l], out=out)

    def pull_max_product(self, x, l, out=None, want_arg=True):
        """(out, arg) of layer l's element-wise maximum over EVERY stored entry of the rows of S (ops.spmax_pull): a fresh row
        of ``x`` for a column in S, the row of table l for the others, the first maximum in stored order whichever table it
        comes from.  arg holds a fresh winner's position in S, -1 for an empty row and -2 - column for a stale winner, so
        ``transpose.max_backward(g, arg)`` -- the block's one-table backward over A[S, S]^T -- sends the gradient to in-part
        winners and nothing to stored rows.  ``out`` may be a pitched view.  --full_batch_part_pull_max."""
        if x.dtype != torch.float32:
            raise ValueError("the two-table element-wise maximum has no bfloat16-operand form")
        return ops.spmax_pull(self.resident, self.ids_dev, self.map, x, self.tables[l], out=out, want_arg=want_arg)

    def pull_attn_product(self, x, l, scale, out=None, want_lse=True, heads=1):
        """(out, lse) of layer l's attention over EVERY stored entry of the rows of S (ops.spattn_pull): the queries are the
        rows of ``x``, a key / value row is the fresh row of ``x`` for a column in S and the row of table l for the others.
        ``out`` may be a pitched view (the neighbour half of a concatenated output).  --full_batch_part_pull."""
        if x.dtype != torch.float32:
            raise ValueError("attention has no bfloat16-operand form")
        return ops.spattn_pull(self.resident, self.ids_dev, self.map, x, self.tables[l], scale, out=out, want_lse=want_lse,
                               heads=heads)

    def pull_attn_backward(self, x, l, g, out_fwd, lse, scale, add=None, add_rows=0, heads=1):
        """dx, the gradient of ``pull_attn_product(x, l, scale)`` with respect to ``x`` for g = dL/dout (+ add on the first
        ``add_rows`` rows): the query's half over all stored entries (ops.spattn_pull_bwd_q; stored rows are constants, but
        the query's gradient sees them), then the keys' / values' half through in-part entries only -- the block's one-table
        bwd_kv over A[S, S]^T with the full rows' lse and delta and dq as its addend (ops.spattn_pull_bwd_kv).  Called
        after ``push(x, l)``: the backward re-reads only rows outside S, which the step leaves untouched."""
        if x.dtype != torch.float32:
            raise ValueError("attention has no bfloat16-operand form")
        dq, delta = ops.spattn_pull_bwd_q(self.resident, self.ids_dev, self.map, x, self.tables[l], g, out_fwd, lse, scale,
                                          add=add, add_rows=add_rows, heads=heads)
        return ops.spattn_pull_bwd_kv(self.transpose.rows_csr, x, g, lse, delta, dq, scale, heads=heads)

    def push(self, x, l):
        if self.owned[l]:
            ops.scatter_rows(self.tables[l], self.ids_dev, x)

    def _score_table(self, l):
        if self.scores is None:
            raise RuntimeError("this PulledMatrix carries no score tables (--full_batch_part_pull_gat allocates them)")
        return self.scores[l]

    def pull_gat_product(self, x, a, l, slope, out=None, want_lse=True, heads=1):
        """(out, lse, S) of layer l's attention with learned scores over EVERY stored entry of the rows of S
        (ops.gat_scores + ops.spgat_pull): S = the fresh score table of ``x`` under the layer's vectors ``a`` (2, d); a
        value row and its destination score are the fresh ones for a column in S, and those of row table l and score
        table l for the others.  ``out`` may be a pitched view.  lse (n, H) and S are what ``pull_gat_backward`` needs."""
        if x.dtype != torch.float32:
            raise ValueError("attention has no bfloat16-operand form")
        H = int(heads)
        S = ops.gat_scores(x, a, heads=H)
        res, lse = ops.spgat_pull(self.resident, self.ids_dev, self.map, x, self.tables[l], S[:, :H], S[:, H:], self._score_table(l),
                                  slope, out=out, want_lse=want_lse, heads=H)
        return res, lse, S

    def pull_gat_backward(self, x, a, S, l, g, out_fwd, lse, slope, add=None, add_rows=0, heads=1, need_dx=True):
        """(dX or None, da) of ``pull_gat_product(x, a, l, slope)`` for g = dL/dout (+ add on dX's first ``add_rows`` rows):
        dU over all stored entries (ops.spgat_pull_bwd_u; stored rows and scores are constants, but the source score's
        gradient sees them), then dB and dV through in-part entries only -- the block's one-table bwd_v over A[S, S]^T with
        the full rows' lse and delta (ops.spgat_pull_bwd_v) -- then ops.gat_scores_bwd: da[0] sees every stored entry,
        da[1] in-part entries only.  Called after ``push`` / ``push_scores``: the backward re-reads only rows outside S."""
        if x.dtype != torch.float32:
            raise ValueError("attention has no bfloat16-operand form")
        H = int(heads)
        U, V = S[:, :H], S[:, H:]
        dU, delta = ops.spgat_pull_bwd_u(self.resident, self.ids_dev, self.map, x, self.tables[l], U, V, self._score_table(l), g,
                                         out_fwd, lse, slope, heads=H)
        dB, dV = ops.spgat_pull_bwd_v(self.transpose.rows_csr, x, U, V, g, lse, delta, slope, add=add if need_dx else None,
                                      add_rows=add_rows if need_dx else 0, heads=H)
        da = ops.gat_scores_bwd(x, a, dU, dV, dx=dB if need_dx else None, heads=H)
        return (dB if need_dx else None), da

    def push_scores(self, S, l):
        """store the destination half of the fresh score table ``S`` (n, 2 H) into score table l at the rows of S"""
        T = self._score_table(l)
        ops.scatter_rows(T, self.ids_dev, S[:, int(T.shape[1]):])

    def layer(self, l):
        return PulledLayer(self, l)

    def describe(self, d):
        return dict(plan_from_cache=False, pace=None, kernel="sgcn::spmm_pull_kernel", products=self.products)


class PulledLayer(object):
    """A PulledMatrix as aggregation layer ``l`` sees it: StaticMatrix's one-table signatures, answered by the two-table launches
    over table l.  Every forward pulls and THEN pushes the layer's input rows (with score tables: its fresh destination scores
    too) -- columns inside the step's vertex set never read either table, and a backward re-reads only rows outside it.
    ``shape`` and ``transpose`` are the block's: in-part entries only.  So is the maximum of a matrix whose ``pull_max`` is off
    (nothing read, nothing pushed); with it on (--full_batch_part_pull_max) ``max_product`` is the two-table maximum and
    pushes, and its ``arg`` is made for ``transpose.max_backward``, which stays the block's.  ``gat_product`` /
    ``gat_backward`` of a matrix WITHOUT score tables are the block's too and push nothing."""

    def __init__(self, matrix, l):
        self.matrix, self.l, self.shape = matrix, int(l), matrix.shape

    @property
    def transpose(self):
        return self.matrix.transpose

    def _no_dropout(self, keep):
        if keep != 1.0:
            raise RuntimeError("--attn_dropout has no two-table form: the mask of out-of-part entries is not defined")

    def product(self, x, out=None):
        out = self.matrix.pull_product(x, self.l, out)
        self.matrix.push(x, self.l)
        return out

    def max_product(self, x, out=None, want_arg=True):
        M = self.matrix
        if not M.pull_max:
            return M.max_product(x, out=out, want_arg=want_arg)
        res = M.pull_max_product(x, self.l, out=out, want_arg=want_arg)
        M.push(x, self.l)
        return res

    def attn_product(self, x, scale, out=None, want_lse=True, heads=1, keep=1.0, key=0):
        self._no_dropout(keep)
        res = self.matrix.pull_attn_product(x, self.l, scale, out=out, want_lse=want_lse, heads=heads)
        self.matrix.push(x, self.l)
        return res

    def attn_backward(self, x, g, out_fwd, lse, scale, add=None, add_rows=0, heads=1, keep=1.0, key=0):
        return self.matrix.pull_attn_backward(x, self.l, g, out_fwd, lse, scale, add=add, add_rows=add_rows, heads=heads)

    def gat_product(self, x, a, slope, out=None, want_lse=True, heads=1, keep=1.0, key=0):
        M = self.matrix
        if M.scores is None:
            return M.gat_product(x, a, slope, out=out, want_lse=want_lse, heads=heads, keep=keep, key=key)
        self._no_dropout(keep)
        res, lse, S = M.pull_gat_product(x, a, self.l, slope, out=out, want_lse=want_lse, heads=heads)
        M.push(x, self.l)
        M.push_scores(S, self.l)
        return res, lse, S

    def gat_backward(self, x, a, S, g, out_fwd, lse, slope, add=None, add_rows=0, heads=1, keep=1.0, key=0, need_dx=True):
        M = self.matrix
        if M.scores is None:
            return M.gat_backward(x, a, S, g, out_fwd, lse, slope, add=add, add_rows=add_rows, heads=heads, keep=keep, key=key,
                                  need_dx=need_dx)
        return M.pull_gat_backward(x, a, S, self.l, g, out_fwd, lse, slope, add=add, add_rows=add_rows, heads=heads,
                                   need_dx=need_dx)


class PartBatch(StaticBatch):
    """One Cluster-GCN step's batch: the static batch of the induced subgraph over ``ids`` (ascending, unique) -- the
    InducedMatrix, labels[ids] (ops.gather_rows of the resident N x C table) and the loss rows, the POSITIONS within ``ids``
    of the vertices the loss runs over.  ``ids_dev`` are the ids on the device: the model gathers its input rows by them.
    Over a PulledMatrix ``adj[l]`` is its view for layer l (``PulledMatrix.layer``); ``matrix`` stays the matrix itself."""

    def __init__(self, ids, ids_dev, matrix, labels, rows, L, device=None):
        n = int(matrix.shape[0])
        if int(len(ids)) != n or int(ids_dev.shape[0]) != n:
            raise ValueError("a part batch over %d vertices needs a matrix of that size, got %d" % (len(ids), n))
        # (labels and rows both None: a batch for forward passes only -- the refresh of a group without a training vertex)
        super(PartBatch, self).__init__(matrix, None if labels is None else ops.gather_rows(labels, ids_dev), rows, L, device)
        self.ids, self.ids_dev = np.asarray(ids, dtype=np.int32), ids_dev
        if isinstance(matrix, PulledMatrix):
            self.adj = [matrix.layer(l) for l in range(self.L)]


def part_stats(adj, parts, train_ids):
    """What the set-up line of --full_batch_parts reports: part sizes, training vertices per part (min / median / max each)
    and the share of the adjacency's stored entries whose row and column lie in one part."""
    N = int(adj.shape[0])
    owner = np.empty(N, dtype=np.int64)
    for j, p in enumerate(parts):
        owner[p] = j
    a = adj.tocsr()
    rows = np.repeat(np.arange(N), np.diff(a.indptr))
    inside = int(np.count_nonzero(owner[rows] == owner[a.indices]))
    sizes = np.array([len(p) for p in parts])
    train = np.bincount(owner[np.asarray(train_ids, dtype=np.int64)], minlength=len(parts))
    mmm = lambda v: (int(v.min()), float(np.median(v)), int(v.max()))      # noqa: E731
    return dict(sizes=mmm(sizes), train=mmm(train), inside=inside / max(int(a.nnz), 1))
