"""Training driver -- drop-in for gcn/train.py (same flags, same flow, same log lines).

    python -m stochastic_gcn_amd.train --dataset reddit --normalization graphsage --weight_decay 0 \\
        --dropout 0.2 --layer_norm --hidden1 128 --num_fc_layers 2 --epochs 30 --early_stopping 30 \\
        --batch_size=512 --test_batch_size=512 --cv --cvd --test_cv --degree=1 --test_degree=1

(= gcn/config/reddit.config:2 + the CVD+PP switches of README.md:46-55.)  Multi-GPU: launch with
``python -m torch.distributed.run --nproc-per-node N -m stochastic_gcn_amd.train ...``.

Flow (gcn/train.py:73-383): load_data -> PP products on the GPU (K11) -> placeholders ->
train/test models from one template (shared weights) -> two schedulers -> SGDTrain epochs with
validation, the reference's two log lines per epoch, early stopping -> (--gradvar: the bias / variance
study, GradientVariance) -> Test().
"""
from __future__ import division, print_function

import os
import queue
import sys
import threading
from time import time

import numpy as np
import scipy.sparse as sp
import torch

from . import ops
from .flags import FLAGS, check_exact_history, check_history_dtype, check_polyak
from .full_batch import (InducedMatrix, PartBatch, PartSchedule, PulledMatrix, check_full_batch_parts, check_part_history,
                         check_part_pull, check_part_pull_gat, check_part_pull_max, part_stats, partition,
                         StaticBatch, StaticMatrix, attn_heads_divide, check_aggregator, check_attention, check_attn_dropout, check_attn_heads, check_attn_score, check_edge_dropout, check_feature_dtype, check_full_batch, full_batch_bf16,
                         full_batch_products,
                         model_matrix, static_kernel_for)  # noqa: F401  (static_kernel_for: named as train.static_kernel_for elsewhere)
from .models import make_template
from .parallel import DataParallel
from .plaingcn import PlainGCN
from .scheduler import NativePrefetcher, PyScheduler
from .utils import Averager, calc_f1, f1_from_classes, load_data
from .vrgcn import VRGCN


class Placeholder(object):
    """Opaque feed-dict key (the reference uses tf.placeholder objects the same way)."""

    def __init__(self, name, shape=None):
        self.name, self.shape = name, shape

    def __repr__(self):
        return "<ph %s>" % self.name


def make_placeholders(L, num_classes):
    """gcn/train.py:89-103."""
    return {
        'adj': [Placeholder('adj_%d' % l) for l in range(L)],
        'madj': [Placeholder('madj_%d' % l) for l in range(L)],
        'fadj': [Placeholder('fadj_%d' % l) for l in range(L)],
        'fields': [Placeholder('field_%d' % l) for l in range(L + 1)],
        'ffields': [Placeholder('ffield_%d' % l) for l in range(L)],
        'scales': [Placeholder('scale_%d' % l) for l in range(L)],
        'labels': Placeholder('labels', (None, num_classes)),
        'dropout': Placeholder('dropout', ()),
    }


def plan_cache_paths(dataset):
    """Where the column-sweep plans of a dataset's two adjacency matrices are cached: beside the
    reference-schema ``.npz`` dataset cache (utils.cache_path), or under $SGCN_PLAN_CACHE_DIR; None when
    neither exists (synthetic stand-ins without a cache directory rebuild their plans, ~1 s)."""
    import os
    from .utils import cache_path
    root = os.environ.get("SGCN_PLAN_CACHE_DIR")
    if root:
        base = os.path.join(root, os.path.basename(cache_path(dataset))[:-4])
    elif os.path.exists(cache_path(dataset)):
        base = cache_path(dataset)[:-4]
    else:
        return None, None
    return base + ".csplan.train.npz", base + ".csplan.full.npz"


def pp_products(train_adj, full_adj, features, device, cache=(None, None), stats=None, products=1):
    """train_feats = train_adj . feats, test_feats = full_adj . feats (gcn/utils.py:169-170,
    321-322).  Dense features: one product each of a StaticMatrix on the GPU (K11), which chooses the kernel by expected
    end-to-end time for the number of times the product will run with one plan (``products``; ``static_kernel_for``): once,
    as in the reference -- the row-gather kernel sgcn_spmm_csr_f32, no plan; many times -- the column sweep (sgcn_spmm_cs_f32,
    the kernel bench.py times), its host plan cached beside the dataset, or for a graph with communities the LDS-staged
    sweep (ops.LdsSweepCSR.for_graph).  Sparse features: a sparse x sparse product, done once on the host with SciPy
    exactly like the reference."""
    if sp.issparse(features):
        return train_adj.dot(features).tocsr(), full_adj.dot(features).tocsr()
    X = features.to(device) if isinstance(features, torch.Tensor) else \
        torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32)).to(device)
    d = int(X.shape[1])
    if X.stride(0) % 4 != 0:            # the sweep reads 16-byte vectors: pad the row pitch once
        Xp = torch.zeros((X.shape[0], (d + 3) // 4 * 4), dtype=torch.float32, device=device)
        Xp[:, :d] = X
        X = Xp[:, :d]
    out = []
    for a, path in zip((train_adj, full_adj), cache):
        t0 = time()
        m = StaticMatrix(a, device, 'auto', products, d, path)
        out.append(m.multiply(X).contiguous())          # (multiply, not product: d % 4 != 0 on an aligned pitch still sweeps)
        if stats is not None:
            stats.append(m.describe(d))
            if m.kernel == 'rows':
                torch.cuda.synchronize()
                stats[-1]['end_to_end_s'] = time() - t0
    return out[0], out[1]


class Prefetcher(object):
    """Runs ``sch.minibatch`` on a host thread a few batches ahead of the GPU.  The sampler is
    stateful, so there is exactly one producer and batches are consumed in call order -- the
    sample sequence is identical to the synchronous loop."""

    def __init__(self, sch, batch_size, depth, n_steps, slots=None):
        self.q = queue.Queue(maxsize=max(1, depth))
        self.t = threading.Thread(target=self._run, args=(sch, batch_size, n_steps, slots), daemon=True)
        self.t.start()

    def _run(self, sch, batch_size, n_steps, slots):
        t_make = 0.0
        for i in range(n_steps):
            t0 = time()
            b = next_minibatch(sch, batch_size, slots[i % len(slots)] if slots else None)
            t_make += time() - t0
            self.q.put(b)
        self.make_s = t_make          # producer time spent building batches (excludes queue waits)
        self.q.put(None)

    def next(self):
        return self.q.get()


class ParallelPrefetcher(object):
    """NON-PARITY fast mode (``--sampler_threads N``): N sampler instances,
    each with its own private CSR copy and RNG stream (seed + 1000 * k), build batches
    ``k, k + N, k + 2N, ...`` concurrently -- the packed C call runs without the GIL -- and the
    consumer receives them in batch order.  Every batch is a valid draw of the same sampling
    distribution, but the sequence is no longer the reference's single mt19937 stream (that is
    what N = 1, the default, reproduces bit for bit).  Non-PP / NS / Exact runs are sampler-bound
    (S-Reddit NS, L = 2, degree 20: 8.4 ms of host sampling per 512-vertex batch against < 1 ms of
    GPU work), which is what this mode is for."""

    def __init__(self, schedulers, batches, plan_t, slots, depth):
        self.sch, self.batches, self.plan_t, self.slots = schedulers, batches, plan_t, slots
        n = len(schedulers)
        self.window = max(1, depth) * n               # batches allowed in flight ahead of the consumer
        assert len(slots) >= self.window + 2, "staging ring too small for the prefetch window"
        self.cv = threading.Condition()
        self.done, self.consumed, self.pos, self.error = {}, 0, 0, None
        self.threads = [threading.Thread(target=self._run, args=(k,), daemon=True) for k in range(n)]
        for t in self.threads:
            t.start()

    def _run(self, k):
        n = len(self.sch)
        try:
            for i in range(k, len(self.batches), n):
                with self.cv:
                    while i >= self.consumed + self.window and self.error is None:
                        self.cv.wait()
                    if self.error is not None:
                        return
                pb = self.sch[k].batch_packed(self.batches[i], self.plan_t, self.slots[i % len(self.slots)])
                with self.cv:
                    self.done[i] = pb
                    self.cv.notify_all()
        except BaseException as e:          # surface producer failures in the consumer
            with self.cv:
                self.error = e
                self.cv.notify_all()

    def next(self):
        i = self.pos
        if i >= len(self.batches):
            return None
        with self.cv:
            while i not in self.done and self.error is None:
                self.cv.wait()
            if self.error is not None:
                raise self.error
            pb = self.done.pop(i)
            self.consumed = i + 1
            self.cv.notify_all()
        self.pos += 1
        return pb


def epoch_batches(data, batch_size, n_steps):
    """The id slices ``minibatch`` would walk (wrapping like next_minibatch), as a list."""
    out, pos, n = [], 0, len(data)
    for _ in range(n_steps):
        if pos == n:
            pos = 0
        end = min(n, pos + batch_size)
        out.append(data[pos:end])
        pos = end
    return out


def next_minibatch(sch, batch_size, slot=None):
    """The next minibatch as a PackedBatch (one C call: sampler + CSR/plan packing into a pinned
    staging slot), wrapping to the start of the (already shuffled) shard when it runs out: in a
    multi-GPU job every rank must take the same number of steps per epoch, and vertex-range
    shards hold slightly different numbers of train ids."""
    fd = sch.minibatch_packed(batch_size, FLAGS.plan_t, slot)
    if fd is None:
        sch.start = 0
        fd = sch.minibatch_packed(batch_size, FLAGS.plan_t, slot)
    return fd


def stop_verdict(par, epoch, cost_val, amt_data):
    """0 = go on, 1 = early stopping, 2 = epoch / data budget reached (gcn/train.py:231-235), the
    same value on every rank: rank 0's validation history and the job-wide amount of data decide."""
    amt = par.sum_scalar(amt_data)
    stop = 0
    if epoch > FLAGS.early_stopping and cost_val[-1] > np.mean(cost_val[-(FLAGS.early_stopping + 1):-1]):
        stop = 1
    elif amt >= FLAGS.data and epoch > FLAGS.epochs:
        stop = 2
    return int(par.broadcast_scalar(stop))


class Trainer(object):
    """Everything gcn/train.py does between flag parsing and the end of training, as an object
    (so bench.py can time epochs of the real training path).  FLAGS must be set before."""

    def __init__(self, data=None, verbose=True):
        np.random.seed(FLAGS.seed)
        torch.manual_seed(FLAGS.seed)
        # (--full_batch / --test_full_batch with an estimator, a sampler option or several ranks: refused before a device is touched)
        self.full_batch, self.test_full_batch = check_full_batch(world=int(os.environ.get("WORLD_SIZE", "1")))
        # (--edge_dropout outside [0, 1), without --full_batch, on the LDS sweep or with --gradvar: too)
        self.edge_dropout = check_edge_dropout()
        # (--full_batch_parts negative, without --full_batch, q outside [1, P], with an edge mask, a bfloat16 feature table or a
        # sweep kernel: too; P against the number of vertices once the graph is loaded)
        self.parts, self.parts_per_step, self.part_norm = check_full_batch_parts()
        # (--full_batch_part_history without parts, with --aggregator max / attn, --reverse or a bfloat16 operand: too)
        self.part_history, self.part_history_bf16 = check_part_history()
        # (--full_batch_part_pull without parts, with --aggregator max, --attn_score gat, --attn_dropout, --reverse or a bfloat16
        # operand: too.  Either flag turns the part-history machinery on; with both, check_part_history has spoken first)
        self.part_pull, pull_bf16 = check_part_pull()
        if self.part_pull:
            self.part_history, self.part_history_bf16 = True, self.part_history_bf16 or pull_bf16
        # (--full_batch_part_pull_gat without parts, without --aggregator attn --attn_score gat, with --attn_dropout, --reverse or
        # a bfloat16 operand: too.  It turns the same machinery on, with one score table per aggregation layer beside the rows)
        self.part_pull_gat, gat_bf16 = check_part_pull_gat()
        if self.part_pull_gat:
            self.part_history, self.part_history_bf16 = True, self.part_history_bf16 or gat_bf16
        # (--full_batch_part_pull_max without parts, without --aggregator max, with --reverse, a bfloat16 operand or one of the
        # three flags above: too.  It turns the same machinery on; the matrix of a step then takes the two-table maximum)
        self.part_pull_max, max_bf16 = check_part_pull_max()
        if self.part_pull_max:
            self.part_history, self.part_history_bf16 = True, self.part_history_bf16 or max_bf16
        # (--aggregator max without both full-graph modes, with a bfloat16 table or an edge mask: too)
        self.max_aggregator = check_aggregator()
        # (--aggregator attn likewise; --attn_scale negative, non-finite, or set without attn: too)
        self.attn_aggregator, self.attn_scale = check_attention()
        # (--attn_heads outside 1/2/4/8, or set without attn: too; whether it divides the widths is checked once they are known)
        self.attn_heads = check_attn_heads()
        # (--attn_dropout outside [0, 1), or set without attn: too)
        self.attn_dropout = check_attn_dropout()
        # (--attn_score outside dot/gat, gat without attn or with --attn_scale, --attn_slope outside [0, 1] or set without gat: too)
        self.attn_gat, self.attn_slope = check_attn_score()
        # (--feature_dtype bf16 without the bf16 GEMMs or without a full-graph mode: too; which model's table it selects)
        self.feature_bf16 = check_feature_dtype()
        # (--history_init exact / --history_refresh / --history_error without a history, with two of them, on several ranks: too)
        self.history_init_exact, self.history_refresh, self.history_error = \
            check_exact_history(world=int(os.environ.get("WORLD_SIZE", "1")))
        # (--polyak_decay outside [0, 1), or with --gradvar: too)
        self.polyak_decay = check_polyak()
        if not torch.cuda.is_available():
            raise RuntimeError("training needs an MI355X (no CPU fallback for the SpMM/history path)")
        check_history_dtype()             # (--history_dtype bf16 with --det_dropout: refused before anything is built)
        par = DataParallel(device=None, init=False)
        dev_index = par.local_rank % torch.cuda.device_count()
        torch.cuda.set_device(dev_index)
        self.device = device = torch.device('cuda', dev_index)
        self.par = par = DataParallel(device=device)
        if par.world > torch.cuda.device_count():
            # several ranks time-slice ONE GPU (the gloo smoke configuration): every cross-stream event of
            # the step program's auxiliary stream then costs a context switch between the processes
            # (measured: 95 ms per step instead of 1.2) -- keep the program's launches on one stream
            FLAGS.update(agg_overlap=False)
        self.log = log = print if (par.rank == 0 and verbose) else (lambda *a, **k: None)

        (num_data, train_adj, full_adj, features, train_features, test_features, labels,
         train_d, val_d, test_d) = data if data is not None else load_data(FLAGS.dataset)
        self.pp_stats = []
        if train_features is None:
            train_features, test_features = pp_products(train_adj, full_adj, features, device,
                                                        cache=plan_cache_paths(FLAGS.dataset), stats=self.pp_stats,
                                                        products=FLAGS.pp_products)
        if FLAGS.gradvar:
            log('Analyze mode...')
            full_adj = train_adj.copy()
            test_features = train_features
        log('Features shape = {}, training edges = {}, testing edges = {}'.format(
            features.shape, train_adj.nnz, full_adj.nnz))
        log('{} training data, {} validation data, {} testing data.'.format(len(train_d), len(val_d), len(test_d)))
        self.num_data, self.labels = num_data, labels
        self.train_d, self.val_d, self.test_d = train_d, val_d, test_d

        self.multitask = multitask = FLAGS.dataset == 'ppi'
        L = FLAGS.num_layers - 1 if FLAGS.preprocess else FLAGS.num_layers
        test_L = FLAGS.num_layers - 1 if FLAGS.test_preprocess else FLAGS.num_layers
        if self.attn_heads > 1:
            # every head is an equal slice of an aggregation layer's input: the feature width where a model aggregates the
            # features itself (--nopreprocess / --notest_preprocess), hidden1 for every later aggregation layer
            if not (FLAGS.preprocess and FLAGS.test_preprocess):
                attn_heads_divide(self.attn_heads, int(features.shape[1]), "the first aggregation layer (the feature width)")
            if FLAGS.num_layers > 1:
                attn_heads_divide(self.attn_heads, int(FLAGS.hidden1), "the aggregation layers behind a dense layer (--hidden1)")
        self.placeholders = placeholders = make_placeholders(max(L, test_L), labels.shape[1])

        t = time()
        log('Building model...')
        train_cls = VRGCN if FLAGS.cv else PlainGCN
        test_cls = VRGCN if FLAGS.test_cv else PlainGCN

        def model_func(model, nbr_features, adj, preprocess, is_training, cvd, _store=None):
            return model(FLAGS.num_layers, preprocess, placeholders, features, nbr_features, adj, cvd,
                         multitask=multitask, is_training=is_training, device=device, _store=_store,
                         feature_bf16=self.feature_bf16[0 if is_training else 1])
        create_model = make_template('model', model_func)
        self.train_model = create_model(train_cls, nbr_features=train_features, adj=train_adj,
                                        preprocess=FLAGS.preprocess, is_training=True, cvd=FLAGS.cvd)
        self.test_model = create_model(test_cls, nbr_features=test_features, adj=full_adj,
                                       preprocess=FLAGS.test_preprocess, is_training=False, cvd=FLAGS.test_cvd)
        log('Finised in {} seconds'.format(time() - t))
        if self.polyak_decay > 0:
            log('[sgcn] --polyak_decay {:g}: validation and test read an exponential moving average of the weights '
                '(decay {:g} per Adam step, kept by the optimizer\'s launch); training keeps the raw weights'.format(
                    self.polyak_decay, float(np.float32(self.polyak_decay))))
        if par.active:
            par.attach(self.train_model)
            self.train_d = par.shard_ids(train_d, num_data).astype(np.int32)
            # a vertex range without a single train id (tiny or skewed sets, many ranks) would feed
            # empty batches into kernels that reject n == 0 while the peers wait in the all-reduce:
            # every rank falls back to round-robin id sharding when ANY range is empty
            if par.max_scalar(1.0 if len(self.train_d) == 0 else 0.0) > 0:
                self.train_d = np.ascontiguousarray(np.asarray(train_d)[par.rank::par.world], dtype=np.int32)
                if len(self.train_d) == 0:
                    raise RuntimeError("data-parallel training: %d train ids cannot be sharded over %d ranks"
                                       % (len(train_d), par.world))
            # |fields[l]| <= batch * prod(1 + degree): lets the history exchange run without a
            # size round-trip (parallel.DataParallel.sync_history)
            bound = int(FLAGS.batch_size)
            for _ in range(L):
                bound = min(int(num_data), bound * (1 + int(FLAGS.degree)))
            par.set_history_cap(bound, max([int(h.shape[1]) for hs in self.train_model.history for h in hs] or [1]))
            self.train_model.native_coll = par.world if (par.native and par.native_history) else 0

        train_degrees = np.array([FLAGS.degree] * L, dtype=np.int32)
        test_degrees = np.array([FLAGS.test_degree] * test_L, dtype=np.int32)
        self.sess = None   # API compatibility: run_one_step(sess, feed_dict)
        from .scheduler import StagingSlot
        nthr = max(1, int(FLAGS.sampler_threads))
        ring = max(FLAGS.prefetch, 1) * nthr + 3
        self.train_sch = self.eval_sch = None
        self.train_schs, self.eval_schs, self.slots, self.eval_slots = [], [], [], []
        self.static_setup_s = 0.0
        self.static_matrices = []         # (adjacency, StaticMatrix): an exact history pass over the same adjacency shares it
        self._labels_dev = None           # ONE N x C label table on the device for both static batches
        caches = plan_cache_paths(FLAGS.dataset)
        if self.full_batch and self.parts:
            # Cluster-GCN steps: no training StaticMatrix is planned -- train_adj lives once as a DeviceCSR, and every step
            # cuts its own block out of it on the device
            t = time()
            self._setup_parts(train_adj)
            self.static_setup_s += time() - t
        elif self.full_batch:
            # exact full-graph training: no sampler, no prefetcher, no staging slots -- one static batch over train_adj
            t = time()
            self.train_static = self._static_batch(train_adj, 'train', caches[0], self.train_model, self.train_d,
                                                   edge_dropout=self.edge_dropout)
            if self.edge_dropout > 0:
                log('[sgcn] --edge_dropout {:g}: every training step multiplies by the adjacency re-drawn under an edge mask '
                    '(keep {:g}; an undirected edge is dropped as a whole, kept entries are scaled by 1 / keep, the diagonal '
                    'is never dropped); evaluation and every other product read the adjacency itself'.format(
                        self.edge_dropout, float(np.float32(1.0 - self.edge_dropout))))
            self.static_setup_s += time() - t
        else:
            self.train_sch = PyScheduler(train_adj, labels, L, train_degrees, placeholders,
                                         par.sampler_seed(FLAGS.seed), self.train_d, cv=FLAGS.cv,
                                         importance=FLAGS.importance)
            self.train_schs = [self.train_sch]
            for k in range(1, nthr):           # non-parity fast mode: extra sampler instances
                self.train_schs.append(PyScheduler(train_adj, labels, L, train_degrees, placeholders,
                                                   par.sampler_seed(FLAGS.seed) + 1000 * k, cv=FLAGS.cv,
                                                   importance=FLAGS.importance))
            self.slots = [StagingSlot(pin=True) for _ in range(ring)]
        if self.test_full_batch:
            t = time()
            self.eval_static = self._static_batch(full_adj, 'full', caches[1], self.test_model,
                                                  val_d if len(val_d) else test_d)
            self._eval_rows, self._eval_logits_key = {}, None
            self.static_setup_s += time() - t
        else:
            # the evaluation sampler is seeded IDENTICALLY on every rank: all ranks evaluate the same
            # vertices with the same (all-reduced) weights, so validation cost -- and with it the
            # early-stopping decision -- agrees across the job
            self.eval_sch = PyScheduler(full_adj, labels, test_L, test_degrees, placeholders,
                                        int(FLAGS.seed), cv=FLAGS.test_cv,
                                        importance=FLAGS.test_importance)
            self.eval_schs = [self.eval_sch]
            for k in range(1, nthr):
                self.eval_schs.append(PyScheduler(full_adj, labels, test_L, test_degrees, placeholders,
                                                  int(FLAGS.seed) + 1000 * k, cv=FLAGS.test_cv,
                                                  importance=FLAGS.test_importance))
            self.eval_slots = [StagingSlot(pin=True) for _ in range(ring if nthr > 1 else 4)]
        # the exact history passes (exact_history.py): one twin + matrix per model whose history they fill or measure
        self.exact_train = self.exact_test = None
        if FLAGS.cv and (self.history_init_exact or self.history_refresh or self.history_error):
            t = time()
            self.exact_train = self._exact_history(self.train_model, train_adj, 'train', caches[0])
            self.static_setup_s += time() - t
        if FLAGS.test_cv and self.history_init_exact:
            t = time()
            self.exact_test = self._exact_history(self.test_model, full_adj, 'test', caches[1])
            self.static_setup_s += time() - t
        self.cost_val = []
        self.avg_loss = Averager(1)
        self.avg_acc = Averager(1)
        self.last_epoch = {}

    # ---- the full-graph modes (full_batch.py) -----------------------------------------------------
    def _static_batch(self, adj, which, cache_path, model, rows, edge_dropout=0.0):
        """The static batch of one adjacency for one model: the matrix with its plan (kernel by --full_batch_kernel; auto:
        static_kernel_for on the number of times the plan will run), the label table, the loss rows."""
        mat = model_matrix(adj, self.device, model, full_batch_products(which), cache_path, bf16=full_batch_bf16(),
                           edge_dropout=edge_dropout)
        self.static_matrices.append((adj, mat))
        if self._labels_dev is None:
            self._labels_dev = torch.from_numpy(np.ascontiguousarray(self.labels, dtype=np.float32)).to(self.device)
        return StaticBatch(mat, self._labels_dev, np.sort(np.asarray(rows)), model.L, self.device)

    # ---- Cluster-GCN steps on device-cut subgraphs (--full_batch_parts; full_batch.py) --------------------------------------
    def _setup_parts(self, train_adj):
        """The resident training adjacency (ONE DeviceCSR with its transpose, rows sorted: the blocks cut from it keep the
        stored order), the parts, the schedule of their groupings, the label table and the training-vertex mask; prints the
        set-up line."""
        N = int(train_adj.shape[0])
        check_full_batch_parts(num_vertices=N)
        a = train_adj.tocsr()
        if not a.has_sorted_indices:
            a = a.copy()
            a.sort_indices()
        # (with its transpose: the transposed block of a step is then the same cut of that matrix, ops.csr_induce)
        self.train_csr = ops.DeviceCSR.from_scipy(a, self.device, with_plan=False, with_transpose=True)
        if self.max_aggregator:
            ops.check_unique_cols(self.train_csr)     # once, here: every block inherits the answer (ops.csr_induce)
        self.part_ids = partition(a, self.parts, FLAGS.seed)
        self.part_schedule = PartSchedule(self.part_ids, self.parts_per_step, FLAGS.seed)
        self._parts_epoch = 0
        self._train_mask = np.zeros(N, dtype=bool)
        self._train_mask[np.asarray(self.train_d, dtype=np.int64)] = True
        if self._labels_dev is None:
            self._labels_dev = torch.from_numpy(np.ascontiguousarray(self.labels, dtype=np.float32)).to(self.device)
        s = self.part_stats = part_stats(a, self.part_ids, self.train_d)
        self.log('[sgcn] --full_batch_parts {}: {} parts per step, {} steps per epoch on induced subgraphs cut on the device '
                 '(values: {}) | part sizes min / median / max = {} / {:g} / {} | training vertices per part = {} / {:g} / {} | '
                 '{:.1f} % of the nonzeros lie inside parts'.format(
                     self.parts, self.parts_per_step, len(self.part_schedule), 'history' if self.part_history else self.part_norm,
                     s['sizes'][0], s['sizes'][1],
                     s['sizes'][2], s['train'][0], s['train'][1], s['train'][2], 100.0 * s['inside']))
        if self.part_history:
            # out-of-part neighbours read stored rows: one table per aggregation layer, on the training model
            nbytes = self.train_model.alloc_part_history(self.part_history_bf16)
            tables, owned = self.train_model.part_history
            if self.part_pull_gat:
                heads = int(getattr(FLAGS, 'attn_heads', 1))
                sbytes = self.train_model.alloc_part_scores(heads)
                self.log('[sgcn] --full_batch_part_pull_gat: a step attends over every stored entry of its rows with learned '
                         'scores -- fresh rows and scores inside its vertex set, stored rows and stored scores outside | {} row '
                         'table(s) of {} rows, {}: {:.1f} MiB, zero-filled{} | {} score table(s) of {} x {} fp32: {:.2f} MiB, '
                         'zero-filled | the source scores\' gradient sees every stored entry, the values\' and destination '
                         'scores\' in-part entries only | a group without a training vertex runs the forward only and pushes '
                         'its rows and scores'.format(
                             sum(owned), N, 'bf16' if self.part_history_bf16 else 'fp32', nbytes / 2.0 ** 20,
                             '' if all(owned) else '; the first aggregation layer reads the resident feature table',
                             len(self.train_model.part_scores), N, heads, sbytes / 2.0 ** 20))
            else:
                what = '--full_batch_part_history: a step sums over'
                if self.part_pull:
                    what = '--full_batch_part_pull (--aggregator {}): a step {} over'.format(
                        FLAGS.aggregator, 'attends' if FLAGS.aggregator == 'attn' else 'sums')
                if self.part_pull_max:
                    what = '--full_batch_part_pull_max: a step takes the maximum over'
                self.log('[sgcn] {} every stored entry of its rows -- fresh rows inside its '
                         'vertex set, stored rows outside (nothing dropped, nothing rescaled) | {} table(s) of {} rows, {}: {:.1f} '
                         'MiB, zero-filled{} | a group without a training vertex runs the forward only and pushes its rows'.format(
                             what, sum(owned), N, 'bf16' if self.part_history_bf16 else 'fp32', nbytes / 2.0 ** 20,
                             '' if all(owned) else '; the first aggregation layer reads the resident feature table'))

    def part_batch(self, ids):
        """The batch of one step over the vertex set ``ids`` (ascending): the block cut out of the resident adjacency with its
        transpose and plans (ops.csr_induce), labels[ids], and the loss rows -- the positions within ``ids`` of the training
        vertices.  None where ``ids`` holds no training vertex.

        Under --full_batch_part_history the cut is made with norm='keep' and the matrix is a PulledMatrix; a set without a
        training vertex gives a batch for the forward only (no labels, no loss rows)."""
        rows = np.flatnonzero(self._train_mask[ids]).astype(np.int32)
        if rows.size == 0 and not self.part_history:
            return None
        ids_dev = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(self.device, non_blocking=True)
        if self.part_history:
            block = ops.csr_induce(self.train_csr, ids, ids_dev, norm='keep')
            tables, owned = self.train_model.part_history
            matrix = PulledMatrix(block, self.train_csr, ids_dev, tables, owned, self.device,
                                  scores=self.train_model.part_scores if self.part_pull_gat else None,
                                  pull_max=self.part_pull_max)
            if rows.size == 0:
                return PartBatch(ids, ids_dev, matrix, None, None, self.train_model.L, self.device)
            return PartBatch(ids, ids_dev, matrix, self._labels_dev, rows, self.train_model.L, self.device)
        block = ops.csr_induce(self.train_csr, ids, ids_dev, norm=self.part_norm)
        return PartBatch(ids, ids_dev, InducedMatrix(block, self.device, bf16=full_batch_bf16()), self._labels_dev, rows,
                         self.train_model.L, self.device)

    def train_epoch_parts(self):
        """One epoch of Cluster-GCN steps: for every group of the epoch's schedule build the batch, run_one_step, next.  A
        group without a training vertex is skipped and counted; last_epoch['steps'] is the number of steps run.  Under
        --full_batch_part_history such a group is not skipped: it runs the forward only, so that its rows reach the tables
        (Model.refresh_part_history), and is counted as last_epoch['refreshed'].  Building a
        batch synchronises once (the block's row pointers), so the host does not run ahead of the device by more than a step."""
        model = self.train_model
        t = time()
        model.init_counts()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        outs, steps, skipped, refreshed, build_s = None, 0, 0, 0, 0.0
        for ids in self.part_schedule.epoch(self._parts_epoch):
            t1 = time()
            batch = self.part_batch(ids)
            build_s += time() - t1
            if batch is None:
                skipped += 1
                continue
            batch.dropout = FLAGS.dropout
            if batch.rows is None:
                # --full_batch_part_history: skipped, the group's rows would stay zero and every neighbour keep reading zeros
                model.refresh_part_history(batch)
                refreshed += 1
                continue
            outs = model.run_one_step(self.sess, batch, sync=False)
            steps += 1
        self._parts_epoch += 1
        host_loop_s = time() - t
        ev1.record()
        torch.cuda.synchronize()
        model.run_t = max(model.run_t, ev0.elapsed_time(ev1) * 1e-3)
        if outs is not None:          # Averager(1) of the reference = the last step's values
            self.avg_loss.add(float(outs[1]))
            self.avg_acc.add(float(outs[2]))
        self.last_epoch = dict(train_wall_s=time() - t, steps=steps, skipped=skipped, sch_wait_s=build_s, host_loop_s=host_loop_s,
                               producer_s=None, sampled_edges=float(model.adj_sizes.sum()), full_edges=0.0,
                               field0=float(model.field_sizes[0]))
        if self.part_history:
            self.last_epoch['refreshed'] = refreshed
        return t, build_s

    # ---- the exact history passes (exact_history.py) ------------------------------------------------
    def _exact_history(self, model, adj, which, cache_path):
        """The exact pass of one history-owning model over its own adjacency: the matrix another pass or --test_full_batch
        already built for that adjacency where its operand is fp32, else one of its own (the plan-cache path of the
        adjacency; 'auto' on the number of passes the flags imply)."""
        from .exact_history import ExactHistory, history_passes, make_matrix
        mat = next((m for a, m in self.static_matrices if a is adj and not m.bf16), None)
        if mat is None:
            mat = make_matrix(adj, self.device, model, history_passes(which), cache_path)
            self.static_matrices.append((adj, mat))
        return ExactHistory(model, mat)

    def history_pass(self, epoch):
        """What happens to the histories before training epoch ``epoch`` (0-based), ahead of train_epoch() so that the epoch
        lines and their time= token are untouched: --history_init exact fills both models' histories before epoch 0,
        --history_refresh K overwrites the training model's before epochs K, 2K, ..., --history_error measures it before
        every epoch -- ONE exact forward per model and epoch at most, the error taken from the forward that is then
        assigned.  Prints one line per layer and returns the record kept in last_epoch['history'] (None: nothing to do)."""
        from .exact_history import refresh_due
        if epoch == 0 and self.exact_test is not None:
            r = self.exact_test.run(assign=True)
            self.log('[sgcn] history: test model filled by one exact pass | pass {:.5f} s'.format(r['pass_s']))
        ex = self.exact_train
        if ex is None:
            return None
        assign = (epoch == 0 and self.history_init_exact) or refresh_due(epoch, self.history_refresh)
        if not (assign or self.history_error):
            return None
        r = ex.run(measure=self.history_error, assign=assign)
        r['epoch'] = epoch + 1
        for l in range(self.train_model.L):
            e = r['layers'][l] if r['layers'] is not None else None
            self.log('[sgcn] history: epoch {:04d} layer {}'.format(epoch + 1, l)
                     + (' rel_err={:.6e} max_err={:.6e} rows_off={}'.format(e['rel_err'], e['max_err'], e['rows_off'])
                        if e is not None else '')
                     + (' | refreshed' if assign else '') + ' | pass {:.5f} s'.format(r['pass_s']))
        return r

    def _weights_version(self):
        """Changes whenever the shared weights do: Adam steps (either model class steps through adam_t) and in-place torch
        writes (checkpoint load, set_params)."""
        return (int(getattr(self.train_model, 'adam_t', 0)), int(self.test_model.theta._version),
                self.test_model.theta.data_ptr())

    def evaluate_full_batch(self, data):
        """evaluate() under --test_full_batch: ONE exact forward of the test model over the full adjacency -- cached per
        weight version, so validation and test after the same epoch share it -- and the loss over rows = sort(data)."""
        t_test = time()
        model, N = self.test_model, len(data)
        if N == 0:
            return 0.0, 0.0, 0.0, 0.0, time() - t_test
        key = np.asarray(data).tobytes()
        sb = self._eval_rows.get(key)
        if sb is None:
            sb = self._eval_rows[key] = self.eval_static.with_rows(np.sort(np.asarray(data)))
        model.join_history()
        model.dropout = 0.0
        ops.pin_stream()
        try:
            ver = self._weights_version()
            if self._eval_logits_key != ver or model.cur is None or model.outputs is None:
                model.forward(model.get_data(sb))
                self._eval_logits_key = ver
            model.cur.rows = sb.rows
            model.eval_light = not self.multitask
            try:
                los, acc, prd, _ = model.loss_and_grad(model.cur.labels)
            finally:
                model.eval_light = False
        finally:
            ops.unpin_stream()
        vec = model.__dict__.pop('eval_vec', None)
        if vec is not None:       # single-label: [stats | CE | hit | classes per row], 4 bytes per row for the F1 scores
            hv = vec.cpu().numpy()
            v = hv[4 + 2 * N:4 + 3 * N].astype(np.int64)
            micro, macro = f1_from_classes(v // 4096, v % 4096)
            return float(hv[2]), float(hv[3]), micro, macro, (time() - t_test)
        micro, macro = calc_f1(prd.cpu().numpy(), np.asarray(self.labels)[sb.host_rows], self.multitask)
        return float(los), float(acc), micro, macro, (time() - t_test)

    # ---- evaluation (gcn/train.py:133-160) ------------------------------------------------------
    class _EvalSink(object):
        """Pinned host memory the evaluation batches' result vectors are copied into as they are produced (copy engine,
        stream order): no torch arithmetic or concatenation kernel on the evaluation path, one synchronisation per sweep."""

        def __init__(self, floats):
            self.buf = torch.empty(max(int(floats), 1), dtype=torch.float32).pin_memory()
            self.pos = 0

        def push(self, vec):
            n = int(vec.numel())
            if self.pos + n > self.buf.numel():
                raise RuntimeError("evaluation sink overflow")
            out = self.buf[self.pos:self.pos + n]
            out.copy_(vec, non_blocking=True)
            self.pos += n
            return out

    def evaluate(self, data):
        if self.test_full_batch:
            return self.evaluate_full_batch(data)
        total_pred, total_labs, total_cls, stats = [], [], [], []
        t_test = time()
        N = len(data)
        chunks = [data[st:min(st + FLAGS.test_batch_size, N)] for st in range(0, N, FLAGS.test_batch_size)]
        sink = None
        if not self.multitask:
            sink = getattr(self, '_eval_sink', None)
            need = 4 * len(chunks) + 3 * N
            if sink is None or sink.buf.numel() < need:
                sink = self._eval_sink = Trainer._EvalSink(need)
            sink.pos = 0
        if FLAGS.native_prefetch and (FLAGS.prefetch > 0 or len(self.eval_schs) > 1):
            pre = NativePrefetcher(self.eval_schs if len(self.eval_schs) > 1 else self.eval_sch, chunks,
                                   FLAGS.plan_t, depth=max(FLAGS.prefetch, 1))
        elif len(self.eval_schs) > 1:
            pre = ParallelPrefetcher(self.eval_schs, chunks, FLAGS.plan_t, self.eval_slots, max(FLAGS.prefetch, 1))
        else:
            pre = None
        def fetch(i):
            return pre.next() if pre else \
                self.eval_sch.batch_packed(chunks[i], FLAGS.plan_t, self.eval_slots[i % len(self.eval_slots)])
        nxt = fetch(0) if chunks else None
        vecs, rows, slow = [], [], None
        for k in range(len(chunks)):
            batch = nxt
            nxt = fetch(k + 1) if k + 1 < len(chunks) else None
            if nxt is not None and pre is not None:      # its H2D copy starts one batch early (train_epoch)
                self.test_model.stage(nxt)
            self.test_model.eval_light = not self.multitask       # (for this call only: models.py _run_program / loss)
            self.test_model.eval_sink = sink
            try:
                los, acc, prd = self.test_model.run_one_step(self.sess, batch, sync=False)
            finally:
                self.test_model.eval_light = False
                self.test_model.eval_sink = None
            vec = self.test_model.__dict__.pop('eval_vec', None)
            if vec is not None:                 # single-label: ONE vector per batch [stats | CE | hit | classes per row]
                vecs.append(vec)
                rows.append(self.test_model.eval_rows)
                continue
            # the other result forms (multi-label, or a step that ran layer by layer): loss, accuracy and the rows'
            # classes -- or predictions and labels -- go to pinned host memory as they are produced (copy engine, stream
            # order; los / acc are views the next batch overwrites); the sums are taken on the host after ONE
            # synchronisation.  No torch arithmetic or concatenation kernel on this path either.
            cls = getattr(self.test_model, 'eval_classes', None)
            r = int(prd.shape[0])
            if slow is None:
                per_row = 1 if cls is not None else 2 * int(prd.shape[1])
                slow = getattr(self, '_eval_sink_slow', None)
                need = 2 * len(chunks) + per_row * N
                if slow is None or slow.buf.numel() < need:
                    slow = self._eval_sink_slow = Trainer._EvalSink(need)
                slow.pos = 0
            stats.append((slow.push(los.reshape(1)), slow.push(acc.reshape(1)), r))
            if cls is not None:                 # single-label: the loss kernel's class indices, 4 bytes per row
                total_cls.append(slow.push(cls))
            else:
                total_pred.append(slow.push(prd.reshape(-1)).view(r, -1))
                total_labs.append(slow.push(self.test_model.cur.labels.reshape(-1)).view(r, -1))
        if pre is not None and hasattr(pre, 'close'):
            pre.close()
        assert not (vecs and stats), "evaluation batches took both result forms"
        if vecs:
            # the vectors are already on their way to pinned host memory: ONE synchronisation, then (loss, accuracy) x rows
            # per batch summed over the batches in fp32 on the host (no torch kernel on this path)
            torch.cuda.current_stream().synchronize()
            tot = np.zeros(2, dtype=np.float32)
            v = []
            for vec, r in zip(vecs, rows):
                hv = vec.numpy() if not vec.is_cuda else vec.cpu().numpy()
                tot += hv[2:4] * np.float32(r)
                v.append(hv[4 + 2 * r:4 + 3 * r])
            tot = tot / np.float32(max(N, 1))
            v = np.concatenate(v).astype(np.int64)
            micro, macro = f1_from_classes(v // 4096, v % 4096)
            return float(tot[0]), float(tot[1]), micro, macro, (time() - t_test)
        if not stats:
            return 0.0, 0.0, 0.0, 0.0, time() - t_test
        torch.cuda.current_stream().synchronize()                           # the only host sync
        tot = np.zeros(2, dtype=np.float32)
        for los, acc, r in stats:
            tot += np.array([los.numpy()[0], acc.numpy()[0]], dtype=np.float32) * np.float32(r)
        tot = tot / np.float32(max(N, 1))
        if total_cls and not total_pred:
            v = np.concatenate([c.numpy() for c in total_cls]).astype(np.int64)   # argmax(pred) + 4096 * argmax(labels) per row
            micro, macro = f1_from_classes(v // 4096, v % 4096)
        else:
            total_pred = np.concatenate([x.numpy() for x in total_pred])
            total_labs = np.concatenate([x.numpy() for x in total_labs])
            micro, macro = calc_f1(total_pred, total_labs, self.multitask)
        return float(tot[0]), float(tot[1]), micro, macro, (time() - t_test)

    # ---- one training epoch (gcn/train.py:182-209) ----------------------------------------------
    def train_epoch_full_batch(self):
        """One eager step over the whole graph: forward, loss over the train ids, backward, Adam.  No step program: at N
        rows the launch chain is not the bound.  The dropout keys come from the model's step counter, as in any step.
        Under --full_batch_parts: the epoch's Cluster-GCN steps (train_epoch_parts)."""
        if getattr(self, 'parts', 0):
            return self.train_epoch_parts()
        model = self.train_model
        t = time()
        model.init_counts()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        self.train_static.dropout = FLAGS.dropout
        outs = model.run_one_step(self.sess, self.train_static, sync=False)
        host_loop_s = time() - t
        ev1.record()
        torch.cuda.synchronize()
        model.run_t = max(model.run_t, ev0.elapsed_time(ev1) * 1e-3)
        self.avg_loss.add(float(outs[1]))
        self.avg_acc.add(float(outs[2]))
        self.last_epoch = dict(train_wall_s=time() - t, steps=1, sch_wait_s=0.0, host_loop_s=host_loop_s, producer_s=None,
                               sampled_edges=float(model.adj_sizes.sum()), full_edges=0.0,
                               field0=float(model.field_sizes[0]))
        return t, 0.0

    def train_epoch(self):
        if self.full_batch:
            return self.train_epoch_full_batch()
        par, train_model, train_sch = self.par, self.train_model, self.train_sch
        train_sch.shuffle()
        t = time()
        train_model.init_counts()
        tsch = 0
        n_steps = -(-len(self.train_d) // FLAGS.batch_size)
        if FLAGS.max_steps:
            n_steps = min(n_steps, FLAGS.max_steps)
        n_steps = int(par.max_scalar(n_steps))       # same step count on every rank
        slots = self.slots
        if FLAGS.native_prefetch and (FLAGS.prefetch > 0 or len(self.train_schs) > 1):
            # C++ sampler thread(s): one = the reference's sample sequence, N = the non-parity fast mode
            pre = NativePrefetcher(self.train_schs if len(self.train_schs) > 1 else train_sch,
                                   epoch_batches(train_sch.data, FLAGS.batch_size, n_steps),
                                   FLAGS.plan_t, depth=max(FLAGS.prefetch, 1))
        elif len(self.train_schs) > 1:
            pre = ParallelPrefetcher(self.train_schs, epoch_batches(train_sch.data, FLAGS.batch_size, n_steps),
                                     FLAGS.plan_t, slots, max(FLAGS.prefetch, 1))
        else:
            pre = Prefetcher(train_sch, FLAGS.batch_size, FLAGS.prefetch, n_steps, slots) \
                if FLAGS.prefetch > 0 else None
        outs = None
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        def fetch(it):
            return pre.next() if pre else next_minibatch(train_sch, FLAGS.batch_size, slots[it % len(slots)])
        t1 = time()
        nxt = fetch(1) if n_steps > 0 else None
        tsch += time() - t1
        for it in range(1, n_steps + 1):
            batch = nxt
            t1 = time()
            # one batch of lookahead: the NEXT minibatch's H2D copy is started before this step is queued, so that by
            # the time its own step is queued the copy has completed and the step needs no device-side wait for it
            nxt = fetch(it + 1) if it < n_steps else None
            tsch += time() - t1
            if nxt is not None and pre is not None:
                train_model.stage(nxt)
            batch.dropout = FLAGS.dropout
            # no host sync inside the epoch: loss / accuracy stay on the device
            outs = train_model.run_one_step(self.sess, batch, sync=False)
        if pre:
            assert pre.next() is None
            self.producer_s = getattr(pre, 'make_s', None)
            if hasattr(pre, 'close'):
                pre.close()
                self.producer_s = getattr(pre, 'stats', None)
        host_loop_s = time() - t        # everything queued: below the epoch time = the host runs ahead of the GPU
        ev1.record()
        torch.cuda.synchronize()
        # 'TF time' of the epoch line (gcn/train.py:227-229; scripts/analyze-time.py reads it) is the time spent
        # inside sess.run, i.e. INCLUDING the device work.  The steps here are launched asynchronously, so the
        # host-side timer of run_one_step only sees launch time: report the epoch's device-elapsed time
        # (HIP events around the step loop) when that is the larger of the two.
        train_model.run_t = max(train_model.run_t, ev0.elapsed_time(ev1) * 1e-3)
        if outs is not None:      # Averager(1) of the reference = the last step's values
            self.avg_loss.add(float(outs[1]))
            self.avg_acc.add(float(outs[2]))
        self.last_epoch = dict(train_wall_s=time() - t, steps=n_steps, sch_wait_s=tsch, host_loop_s=host_loop_s,
                               producer_s=getattr(self, 'producer_s', None),
                               sampled_edges=float(train_model.adj_sizes.sum()),
                               full_edges=float(train_model.fadj_sizes.sum()),
                               field0=float(train_model.field_sizes[0]))
        return t, tsch

    def SGDTrain(self):
        log, par, train_model = self.log, self.par, self.train_model
        if FLAGS.load:
            train_model.load(self.sess, load_history=FLAGS.gradvar)
            for h1, h2 in zip(train_model.history_vars, self.test_model.history_vars):
                h2.copy_(h1)
            return
        log('Start training...')
        for epoch in range(100000000):
            hist = self.history_pass(epoch)
            t, tsch = self.train_epoch()
            if hist is not None:
                self.last_epoch['history'] = hist
            cost, acc, micro, macro, duration = self.evaluate(self.val_d)
            self.cost_val.append(cost)
            cost_val = self.cost_val
            # the reference's epoch lines (gcn/train.py:217-229); token positions are consumed by
            # scripts/analyze-time.py:39-54 and scripts/plot-convergence.py:78-86
            log("Epoch:", '%04d' % (epoch + 1),
                "train_loss=", "{:.5f}".format(self.avg_loss.mean()),
                "train_acc=", "{:.5f}".format(self.avg_acc.mean()),
                "val_loss=", "{:.5f}".format(cost),
                "val_acc=", "{:.5f}".format(acc),
                "mi F1={:.5f} ma F1={:.5f} ".format(micro, macro),
                "time=", "{:.5f}".format(time() - t),
                "ttime=", "{:.5f}".format(duration),
                "(sch {:.5f} s)".format(tsch),
                "data = {}".format(train_model.amt_data))
            G = float(2 ** 30)
            log('TF time = {}, g time = {}, G GFLOPS = {}, NN GFLOPS = {}, field sizes = {}, adj sizes = {}, fadj sizes = {}'.format(
                train_model.run_t, train_model.g_t, train_model.g_ops / G, train_model.nn_ops / G,
                train_model.field_sizes, train_model.adj_sizes, train_model.fadj_sizes))
            log('[sgcn] epoch train wall = {:.5f} s over {} steps ({} GPU(s))'.format(
                self.last_epoch['train_wall_s'], self.last_epoch['steps'], par.world))
            # the two exits of gcn/train.py:231-235, verbatim conditions (`epoch > FLAGS.epochs`:
            # the reference trains epochs + 2 epochs).  In a multi-GPU job the decision is COLLECTIVE:
            # rank 0 decides on its validation cost and the job-wide amount of data, and broadcasts
            # the verdict -- a rank-local `break` would leave the peers blocked in the next epoch's
            # all-reduce.
            stop = stop_verdict(par, epoch, cost_val, train_model.amt_data)
            if stop == 1:
                log("Early stopping...")
            if stop:
                break
        log("Optimization Finished!")
        if par.rank == 0:
            train_model.save(self.sess)

    # ---- the --gradvar bias / variance study (gcn/train.py:241-276) -------------------------------
    def GradientVariance(self, observer=None):
        """One fixed batch (the first ``batch_size`` training ids), its prediction and first-layer gradient drawn
        ``gradvar_draws`` times under the evaluation sampler with the test model (the 'full' estimator: every neighbour
        under --test_degree=10000) and as often under the training sampler with the training model ('part'); prints
        the reference's seven lines -- bias and stdev of the sampled estimator, normalised by the mean magnitude of the
        full one -- and returns their nine values as a dict.  Same draw sequence as the reference for the same seed.

        The draws are folded into running fp64 statistics on the device (stats.DeviceStat): no per-draw copy or host
        synchronisation.  ``observer(kind, pred, grad)``, kind 'full' or 'part', sees every draw's device tensors
        (the gradient is a view the next draw overwrites).  One rank only: a multi-rank job skips the study."""
        from .stats import DeviceStat, summary
        log, ph = self.log, self.placeholders
        if self.par.world > 1:
            log('--gradvar: the bias / variance study runs on one rank; skipped ({} ranks)'.format(self.par.world))
            return None
        batch = self.train_d[:FLAGS.batch_size]
        times = int(FLAGS.gradvar_draws)

        def draw(sch, model, kind, preds, grads):
            for _ in range(times):
                feed_dict = sch.batch(batch)
                feed_dict[ph['dropout']] = FLAGS.dropout
                pred, grad = model.get_pred_and_grad_device(self.sess, feed_dict)
                preds.add(pred)
                grads.add(grad)
                if observer is not None:
                    observer(kind, pred, grad)

        full_preds, full_grads = DeviceStat(), DeviceStat()
        draw(self.eval_sch, self.test_model, 'full', full_preds, full_grads)
        full_preds_m, full_pred_std, _ = summary(full_preds)
        full_grads_m, full_grad_std, _ = summary(full_grads)
        res = dict(full_pred_stdev=full_pred_std / full_preds_m, full_grad_stdev=full_grad_std / full_grads_m)
        log('Full pred stdev = {}'.format(res['full_pred_stdev']))
        log('Full grad stdev = {}'.format(res['full_grad_stdev']))

        part_preds, part_grads = DeviceStat(), DeviceStat()
        draw(self.train_sch, self.train_model, 'part', part_preds, part_grads)
        _, part_pred_std, part_pred_bias = summary(part_preds, full_preds)
        part_grads_mabs, part_grad_std, part_grad_bias = summary(part_grads, full_grads)
        res.update(part_pred_bias=part_pred_bias / full_preds_m, part_pred_stdev=part_pred_std / full_preds_m,
                   part_grad_bias=part_grad_bias / full_grads_m, part_grad_stdev=part_grad_std / full_grads_m,
                   full_grads_m=full_grads_m, part_grad_std_mean=part_grad_std, part_grad_mean_abs=part_grads_mabs)
        log('Part pred bias = {}'.format(res['part_pred_bias']))
        log('Part pred stdev = {}'.format(res['part_pred_stdev']))
        log('Part grad bias = {}'.format(res['part_grad_bias']))
        log('Part grad stdev = {}'.format(res['part_grad_stdev']))
        log(full_grads_m, part_grad_std, part_grads_mabs)
        return res

    def Test(self):
        test_cost, test_acc, micro, macro, test_duration = self.evaluate(self.test_d)
        self.log("Test set results:", "cost=", "{:.5f}".format(test_cost),
                 "accuracy=", "{:.5f}".format(test_acc),
                 "mi F1={:.5f} ma F1={:.5f} ".format(micro, macro),
                 "time=", "{:.5f}".format(test_duration))
        remaining = np.array(sorted(set(range(self.num_data)) - set(self.test_d.tolist())), dtype=np.int32)
        if FLAGS.test_cv:
            self.evaluate(remaining)


def main(argv=None):
    FLAGS.parse(argv)
    tr = Trainer()
    tr.SGDTrain()
    if FLAGS.gradvar:
        tr.GradientVariance()
    num_runs = FLAGS.num_layers + 1 if FLAGS.test_cv else 1
    for _ in range(num_runs):
        tr.Test()
    tr.par.shutdown()


if __name__ == '__main__':
    main(sys.argv[1:])
