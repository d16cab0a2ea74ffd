"""Exact control-variate history: ``--history_init exact``, ``--history_refresh K``, ``--history_error``.

The sampled estimator of ``--cv / --cvd`` is exact only where the stored history equals the current activations: with a
fresh history ``A (mu - H[ifield]) = 0`` and the control-variate aggregate IS the full-neighbour aggregate, for any sample.
The full-graph path computes those activations for all N vertices in one pass; this module connects the two.

  ExactTwin      a PlainGCN over the OWNER's variable store, feature table and adjacency (nothing is copied: the weights
                 are read live, no second N x F table goes to the device), evaluation mode, dropout 0, cvd off -- the
                 construction by which --cv --cvd --test_full_batch scores shared weights.  A model that owns a history
                 cannot take a static batch itself (Model._upload_static refuses it), so the pass runs on this twin.
  ExactHistory   one owner, its twin and ONE StaticMatrix: ``forward()`` runs the twin up to the last aggregator's input
                 and returns the input of every aggregation layer (the clean stream mu of a --cvd stack; the raw feature
                 table for layer 0 without pre-processing), ``error()`` measures the owner's history against them
                 (ops.history_error, no synchronisation), ``assign()`` overwrites the history IN PLACE
                 (ops.history_assign: rounded to nearest even for a bfloat16 table) -- a step program bakes the history's
                 addresses into its identity (Model._program), so after an assign the compiled program is still the cached one.

The passes are fp32 whatever --dense_dtype / --full_batch_dtype say: those belong to the two full-graph modes.
"""
import math
from time import time

import torch

from . import ops
from .flags import FLAGS
from .full_batch import StaticBatch, model_matrix
from .layers import PlainAggregator, dense_of
from .models import Model
from .plaingcn import PlainGCN


def refresh_due(epoch, every):
    """Is the training model's history overwritten before training epoch ``epoch`` (0-based)?  --history_refresh K: before
    the epochs K+1, 2K+1, ... as the log counts them, i.e. 0-based K, 2K, ...; never before epoch 0 (that is
    --history_init's)."""
    every = int(every)
    return every > 0 and epoch > 0 and epoch % every == 0


def history_passes(which='train', flags=None):
    """How many exact passes the flags imply for a model (what StaticMatrix 'auto' weighs a plan's setup against): 1 for
    --history_init exact, plus -- the training model only -- (epochs + 2) // K refreshes, or epochs + 2 under
    --history_error (SGDTrain runs epochs + 2 epochs, one pass before each at most)."""
    f = FLAGS if flags is None else flags
    n = 1 if f.history_init == 'exact' else 0
    if which == 'train':
        epochs = int(f.epochs) + 2
        if f.history_error:
            n += epochs
        elif int(f.history_refresh) > 0:
            n += epochs // int(f.history_refresh)
    return n


class ExactTwin(PlainGCN):
    """The history-free model of the owner's weights.  GCN.__init__ restated without the feature upload: the feature
    table, the variable store, the adjacency and the placeholders are the owner's own objects."""

    dense_fp32 = True       # (Model.forward: never the bf16 dense route)

    def __init__(self, owner):
        if not owner._history:
            raise ValueError("an exact twin is built for a model that owns a history")
        if any(len(hs) != 1 for hs in owner._history):
            raise ValueError("the exact pass fills ONE history per layer (not the mean / variance pair of --det_dropout)")
        Model.__init__(self, name=owner.name + '_exact', multitask=owner.multitask, is_training=False, device=owner.device,
                       _store=owner._store)
        self.reads_average = owner.reads_average      # (--polyak_decay: the weights the owner reads, raw or averaged)
        self.owner = owner
        self.L = owner.L + (1 if owner.preprocess else 0)
        self.preprocess, self.placeholders = owner.preprocess, owner.placeholders
        # (a sparse feature matrix the owner densified -- no pre-processing -- is a dense input here from the start)
        self.sparse_input = bool(owner.sparse_input and owner.sparse_mm)
        self.input_dim = owner.input_dim
        self.features_dev = owner.features_dev
        self.features = owner.features if self.sparse_input else owner.features_dev
        self.adj, self.cvd = owner.adj, False
        self.build()
        self.init_counts()
        assert self.theta is owner.theta and self.L == owner.L
        self.agg_index = [i for i, layer in enumerate(self.layers) if isinstance(layer, PlainAggregator)]
        assert len(self.agg_index) == owner.L


def make_matrix(adj, device, owner, passes, cache_path=None, kernel=None):
    """The StaticMatrix of an exact history pass over ``adj``: fp32 operand always; the kernel from --full_batch_kernel;
    'auto' weighs the plan against passes x (L - 1) products -- a pass stops at the LAST aggregator's input, so it multiplies
    the matrix L - 1 times (not at all for the two-layer pre-processed recipes)."""
    return model_matrix(adj, device, owner, int(passes) * max(owner.L - 1, 0), cache_path, kernel, bf16=False,
                        layers=owner.L - 1)


class ExactHistory(object):
    def __init__(self, owner, matrix):
        if matrix.bf16:
            raise ValueError("the exact history pass needs an fp32-operand matrix")
        self.owner, self.matrix = owner, matrix
        self.twin = ExactTwin(owner)
        self.batch = StaticBatch(matrix, None, None, owner.L, owner.device)       # (forward only: no labels, no loss rows)
        self.passes = 0

    def forward(self, full=False):
        """One exact pass with the current weights: the inputs of the aggregation layers, [N x dims(l)] fp32 device tensors
        (views of the twin's activations: the next pass replaces them).  ``full``: run the whole stack, so that
        ``twin.outputs`` holds the exact logits of all N vertices as well."""
        twin = self.twin
        self.owner.join_history()
        twin.dropout = 0.0
        ops.pin_stream()
        try:
            twin.forward(twin.upload(self.batch), stop=None if full else twin.agg_index[-1])
        finally:
            ops.unpin_stream()
        self.passes += 1
        return [dense_of(twin.activations[i]) for i in twin.agg_index]

    def error(self, acts):
        """The staleness of the owner's history against ``acts`` as device fp64[4] vectors, one per layer (not synchronised)."""
        return [ops.history_error(x, hs[0]) for x, hs in zip(acts, self.owner.history)]

    def assign(self, acts):
        """history[l] <- acts[l], in place (the tables keep their addresses)."""
        for x, hs in zip(acts, self.owner.history):         # (``history`` joins a pending exchange first)
            ops.history_assign(hs[0], x)

    @staticmethod
    def report(vectors):
        """Host side of ``error``: [dict(rel_err, max_err, rows_off)] per layer from ONE device-to-host copy.  rel_err =
        sqrt(sum (x - H)^2 / sum x^2); 0.0 for an all-zero layer that the history matches."""
        if not vectors:
            return []
        out = []
        for v in torch.stack(vectors).cpu().tolist():
            rel = math.sqrt(v[0] / v[1]) if v[1] > 0 else (0.0 if v[0] == 0 else float('inf'))
            out.append(dict(rel_err=rel, max_err=float(v[2]), rows_off=int(v[3])))
        return out

    def run(self, measure=False, assign=False):
        """One pass at most: the error (if asked) is taken first, from the same forward that is then assigned (if asked).
        Returns dict(layers=[...] or None, refreshed, pass_s) with the pass timed to its completion on the device."""
        t = time()
        acts = self.forward()
        vec = self.error(acts) if measure else None
        if assign:
            self.assign(acts)
        layers = self.report(vec) if measure else None
        torch.cuda.current_stream().synchronize()
        return dict(layers=layers, refreshed=bool(assign), pass_s=time() - t)
