"""An fp64 NumPy statement of the two-table gather product (sgcn_spmm_pull.hip) and of the estimator it serves,
--full_batch_part_history (GNNAutoScale / Cluster-GCN with historical embeddings) -- a test-only helper.

The kernel:   C[i] = sum over the stored entries e of row ids[i] of val[e] * (X[map[col[e]]] if map[col[e]] >= 0 else H[col[e]])

  position_map, pull      the definition, entry by entry, from SciPy's A[ids] and np.where(map[col] >= 0, ...)
  pull_dense              the same number by another road: the dense rows of A[ids] times the merged table (H with the rows of
                          S replaced by X), for tests/test_part_history.py to hold ``pull`` to
  MUTANTS                 two wrong kernels the comparison must reject: one reads H for in-part columns, one drops the
                          out-of-part entries (which is --full_batch_parts without the flag, norm='keep')

The estimator: ``PartHistoryModel`` is oracle.model_np.Model with its forward and backward restated for a plain dense-input
stack (the style of tests/attn_aggregator_ref.py): every matrix product and every sum over rows accumulates in fp64 and is
rounded to fp32 once; an aggregation layer's neighbour half is ``pull`` over the RESIDENT adjacency with that layer's table,
after which the layer's input rows are pushed into the table (a table that is the feature table is exact and never written);
the backward of an aggregation layer goes through the block A[S, S] only -- stored rows are constants.  The parameter
initialisation, LayerNorm, the hash masks, the loss and Adam are the oracle's own, called, not copied."""
import numpy as np
import scipy.sparse as sp

from oracle import model_np as mnp

f32 = np.float32


# ---- the kernel ---------------------------------------------------------------------------------------------------------
def position_map(N, ids):
    """map[v] = position of v in ids, -1 elsewhere (what sgcn_induce_map_i32 writes)"""
    m = np.full(int(N), -1, dtype=np.int64)
    m[np.asarray(ids, dtype=np.int64)] = np.arange(len(ids))
    return m


def _entries(a, ids):
    """(row of the output, column, value as fp64) of every stored entry of the selected rows, in stored order"""
    sub = a.tocsr()[np.asarray(ids, dtype=np.int64)].tocsr()
    n = len(ids)
    return np.repeat(np.arange(n), np.diff(sub.indptr)), sub.indices.astype(np.int64), sub.data.astype(np.float64)


def _sum(n, d, rows, terms):
    out = np.zeros((n, d), dtype=np.float64)
    np.add.at(out, rows, terms)
    return out


def pull(a, ids, X, H):
    """the fp64 value of the kernel; X: len(ids) x d, H: N x d (any float type: a bfloat16 table is handed over widened)"""
    rows, col, val = _entries(a, ids)
    X, H = np.asarray(X, np.float64), np.asarray(H, np.float64)
    m = position_map(a.shape[0], ids)[col]
    src = np.where((m >= 0)[:, None], X[np.maximum(m, 0)], H[col])
    return _sum(len(ids), X.shape[1], rows, val[:, None] * src)


def pull_magnitude(a, ids, X, H):
    """sum of |val| |source row|: what a rounding bound scales with"""
    return pull(abs(a.tocsr()), ids, np.abs(np.asarray(X, np.float64)), np.abs(np.asarray(H, np.float64)))


def merged(ids, X, H):
    """H with the rows of S replaced by X: the one table whose plain product with A[ids] is the kernel's number"""
    Z = np.array(H, dtype=np.float64, copy=True)
    Z[np.asarray(ids, dtype=np.int64)] = np.asarray(X, np.float64)
    return Z


def pull_dense(a, ids, X, H):
    return np.asarray(a.tocsr()[np.asarray(ids, dtype=np.int64)].astype(np.float64).todense()) @ merged(ids, X, H)


def _mutant_stale_in_part(a, ids, X, H):
    rows, col, val = _entries(a, ids)
    return _sum(len(ids), np.asarray(X).shape[1], rows, val[:, None] * np.asarray(H, np.float64)[col])


def _mutant_drop_out_of_part(a, ids, X, H):
    rows, col, val = _entries(a, ids)
    m = position_map(a.shape[0], ids)[col]
    src = np.where((m >= 0)[:, None], np.asarray(X, np.float64)[np.maximum(m, 0)], 0.0)
    return _sum(len(ids), np.asarray(X).shape[1], rows, val[:, None] * src)


MUTANTS = {'stale_in_part': _mutant_stale_in_part, 'drop_out_of_part': _mutant_drop_out_of_part}


def block(a, ids):
    """A[S, S] as a SciPy CSR (the matrix the backward multiplies by, transposed)"""
    ids = np.asarray(ids, dtype=np.int64)
    return a.tocsr()[ids][:, ids].tocsr()


def widen_bf16(bits):
    """a uint16 bfloat16 image as fp32 (bits << 16, exact)"""
    return (np.asarray(bits, np.uint32) << 16).view(np.float32)


def round_bf16(x):
    """fp32 -> the bfloat16 image (uint16), to nearest even: what ops.scatter_rows stores into a bfloat16 table"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    return r.astype(np.uint16)


# ---- the estimator ------------------------------------------------------------------------------------------------------
def _mm(a, b):
    return (np.asarray(a, np.float64) @ np.asarray(b, np.float64)).astype(f32)


class PartHistoryModel(mnp.Model):
    """``resident``: the N x N training adjacency.  ``tables[l]``: layer l's stored rows (N x width, fp32; zero at the start),
    or None where the layer reads the feature table.  ``bf16``: stored rows are rounded to bfloat16 on the push."""

    def attach(self, resident, bf16=False):
        fl = self.flags
        assert not (self.cv or self.cvd or fl['det_dropout'] or sp.issparse(self.features)), "plain dense-input stacks only"
        self.resident, self.bf16 = resident.tocsr(), bool(bf16)
        H = fl['hidden1']
        agg0 = H if self.preprocess else self.input_dim
        self.tables = [None if (l == 0 and not self.preprocess) else np.zeros((resident.shape[0], agg0 if l == 0 else H), f32)
                       for l in range(self.L)]
        return self

    def table(self, l):
        return self.features if self.tables[l] is None else self.tables[l]

    def push(self, l, ids, x):
        if self.tables[l] is not None:
            self.tables[l][np.asarray(ids, np.int64)] = widen_bf16(round_bf16(x)) if self.bf16 else x

    def forward_part(self, ids, dropout, masks, stop_at_last_agg=False):
        """(logits on S, activations); ``pushed[l]`` holds the rows every aggregation layer pushed.  ``stop_at_last_agg``: the
        refresh of a group without a training vertex -- the forward up to the last aggregation layer's input, which is pushed."""
        fl, keep = self.flags, 1.0 - dropout
        concat = fl['normalization'] != 'gcn'
        ids = np.asarray(ids, dtype=np.int64)
        act = self.features[ids]
        blk = block(self.resident, ids)
        tape, acts, self.pushed = [], [], {}
        last_agg = max(li for li, s in enumerate(self.specs) if s[0] == 'agg')
        for li, s in enumerate(self.specs):
            kind = s[0]
            if kind == 'dropout':
                m = masks('L%d' % li, act.shape) if dropout > 0 else None
                act = mnp.dropout_fwd(act, keep, m)
                tape.append(('dropout', m, keep))
            elif kind == 'dense':
                _, name, fin, fout, sparse_in, relu, norm = s
                assert not sparse_in
                y = _mm(act, self.params[name + '/weights'])
                ctx = None
                if norm:
                    y, ctx = mnp.layer_norm_fwd(y, self.params[name + '/offset'], self.params[name + '/scale'])
                pre = y
                if relu:
                    y = np.maximum(y, 0).astype(f32)
                tape.append(('dense', s, act, ctx, pre))
                act = y
            elif kind == 'agg':
                l = s[1]
                if stop_at_last_agg and li == last_agg:
                    self.push(l, ids, act)
                    self.pushed[l] = act
                    break
                C = pull(self.resident, ids, act, self.table(l)).astype(f32)
                self.push(l, ids, act)                    # push after pull: columns in S never read the table
                self.pushed[l] = act
                tape.append(('agg', blk, concat, act.shape[1]))
                act = np.hstack([act, C]).astype(f32) if concat else C
            else:
                raise NotImplementedError(kind)
            acts.append(act)
        self._tape = tape
        return act, acts

    def backward(self, dout):
        grads = {k: np.zeros_like(v) for k, v in self.params.items()}
        g = dout
        self.gtrace = []
        for rec in reversed(self._tape):
            kind = rec[0]
            if kind == 'dense':
                _, s, xin, ctx, pre = rec
                _, name, fin, fout, sparse_in, relu, norm = s
                if relu:
                    g = (g * self._gate(name, pre)).astype(f32)
                if norm:
                    g, doff, dsc = mnp.layer_norm_bwd(g, ctx, self.params[name + '/scale'])
                    grads[name + '/offset'] += doff
                    grads[name + '/scale'] += dsc
                grads[name + '/weights'] += _mm(xin.T, g)
                g = _mm(g, self.params[name + '/weights'].T)
            elif kind == 'dropout':
                _, m, keep = rec
                if m is not None:
                    g = (g * (m * f32(1.0 / keep))).astype(f32)
            elif kind == 'agg':
                _, blk, concat, d = rec                   # through A[S, S] only: stored rows are constants
                gn = np.asarray(g[:, d:] if concat else g, np.float64)
                dx = blk.T.tocsr().astype(np.float64) @ gn
                if concat:
                    dx = dx + np.asarray(g[:, :d], np.float64)
                g = dx.astype(f32)
            self.gtrace.append((kind, g))
        wd = f32(self.flags['weight_decay'])
        for k in self._wd_names():
            grads[k] += wd * self.params[k]
        return grads

    def step(self, ids, rows, labels, dropout, masks):
        """one training step over S = ids with the loss over the positions ``rows``: (logits, acts, loss, grads)"""
        logits, acts = self.forward_part(ids, dropout, masks)
        loss, _, _, dl = self.loss_and_grad(logits[rows], np.asarray(labels)[np.asarray(ids)][rows])
        dout = np.zeros_like(logits)
        dout[rows] = dl
        grads = self.backward(dout)
        self.adam_step(grads)
        return logits, acts, float(loss), grads

    def relu_margin(self):
        """the smallest non-zero |ReLU input| / its layer's largest input magnitude over the last forward"""
        worst = np.inf
        for rec in self._tape:
            if rec[0] == 'dense' and rec[1][5]:
                pre = rec[4]
                nz = np.abs(pre[pre != 0])
                if nz.size:
                    worst = min(worst, float(nz.min()) / float(np.abs(pre).max()))
        return worst


def make_model(case, seed=None, params=None, bf16=False):
    """the PartHistoryModel of a case dict of attn_aggregator_cases.build / full_batch_cases.build, attached to its training
    adjacency"""
    fl = case['flags']
    seed = case['cfg']['init'] if seed is None else seed
    args = (fl, fl['num_layers'], fl['preprocess'], False, False, case['feats'], case['nbr_train'], case['n'], case['classes'])
    if params is None:
        params = mnp.init_params(PartHistoryModel(*args, {}).specs, seed)
    return PartHistoryModel(*args, params).attach(case['train_adj'], bf16=bf16)
