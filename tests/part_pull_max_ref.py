"""An exact NumPy statement of the two-table element-wise maximum (sgcn_spmax_pull.hip) and of the estimator it serves,
--full_batch_part_pull_max -- a test-only helper.  The forward has no arithmetic, so nothing here needs fp64 for it.

The kernel, for selected row i over every stored entry e of row ids[i] in stored order:
    B_e       = X[map[col[e]]] if map[col[e]] >= 0 else H[col[e]]
    C[i, c]   = the FIRST maximum of B_e[c] (a later entry replaces the best only on strict >; an empty row gives +0.0)
    arg[i, c] = the winner:  >= 0 fresh, its POSITION in ids;  -1 empty row;  <= -2 stale, global column -2 - arg

  loops             the definition, one comparison at a time (small matrices only), and the three MUTANTS
  forward           the same result by another road: spmax_ref.forward on (a[ids], merged(ids, X, H)) with its arg -- a
                    global column -- encoded by ``encode``
  encode / decode   global winner column <-> the kernel's arg
  backward          dX (n x d): the scatter of G to IN-PART winners only, in ascending i (spmax_ref.backward: negative
                    words are no targets), + the addend; backward_f64 its fp64 value and bound
  MUTANTS           three wrong kernels the comparisons must reject: 'stale_in_part' reads H for in-part columns too,
                    'drop_out_of_part' leaves the out-of-part entries out (the block's maximum: the mode without the flag),
                    'grad_to_stale' records a stale winner by its bare global column, so that the backward sends its
                    gradient to whichever in-part row has that position

The estimator: ``PartPullMaxModel`` is part_history_ref.PartHistoryModel with every aggregation the maximum above over
the RESIDENT adjacency's pattern with that layer's table, and the aggregation's backward the scatter to in-part winners
(fp64, rounded once).  ``margins`` records, per forward, what the well-posedness scan of part_pull_max_cases.py needs: for
every max layer the smallest non-zero top-two gap over ALL stored entries (stale included) and the largest input magnitude,
for every ReLU the smallest non-zero |input| and the largest; ``winners`` the number of elements won by a fresh and by a stale
row per max layer."""
import numpy as np
import scipy.sparse as sp

import part_history_ref as pr
import spmax_ref
from max_aggregator_ref import top_two_gap
from oracle import model_np as mnp

f32 = np.float32


# ---- the kernel ---------------------------------------------------------------------------------------------------------
def merged32(ids, X, H):
    """H with the rows of S replaced by X, as fp32 (bits kept): the one table whose plain maximum over A[ids] is the kernel's"""
    Z = np.array(H, dtype=np.float32, copy=True)
    Z[np.asarray(ids, dtype=np.int64)] = np.asarray(X, np.float32)
    return Z


def encode(arg_global, N, ids):
    """spmax's arg over the merged table (a global column, -1 for an empty row) as the kernel stores it"""
    g = np.asarray(arg_global, np.int64)
    m = pr.position_map(N, ids)[np.maximum(g, 0)]
    return np.where(g < 0, -1, np.where(m >= 0, m, -2 - g)).astype(np.int32)


def decode(arg, ids):
    """the kernel's arg as global winner columns (-1 for an empty row)"""
    a = np.asarray(arg, np.int64)
    ids = np.asarray(ids, np.int64)
    fresh = ids[np.clip(a, 0, max(len(ids) - 1, 0))] if len(ids) else np.zeros_like(a)
    return np.where(a >= 0, fresh, np.where(a == -1, -1, -2 - a)).astype(np.int32)


def forward(a, ids, X, H):
    """(C, arg) through the one-table reference on the rows ids of ``a`` and the merged table"""
    sub = a.tocsr()[np.asarray(ids, dtype=np.int64)].tocsr()
    C, g = spmax_ref.forward(sub, merged32(ids, X, H))
    return C, encode(g, a.shape[0], ids)


def loops(a, ids, X, H, mutant=None):
    """(C, arg) by the definition, entry by entry; ``mutant``: one of MUTANTS"""
    a = a.tocsr()
    X, H = np.asarray(X, np.float32), np.asarray(H, np.float32)
    n, d = len(ids), X.shape[1]
    m = pr.position_map(a.shape[0], ids)
    C = np.zeros((n, d), np.float32)
    arg = np.full((n, d), -1, np.int32)
    for i, r in enumerate(np.asarray(ids, np.int64)):
        first = True
        for j in a.indices[a.indptr[r]:a.indptr[r + 1]]:
            j = int(j)
            inside = m[j] >= 0
            if mutant == 'drop_out_of_part' and not inside:
                continue
            row = X[m[j]] if inside and mutant != 'stale_in_part' else H[j]
            word = int(m[j]) if inside else (j if mutant == 'grad_to_stale' else -2 - j)
            for c in range(d):
                if first or row[c] > C[i, c]:
                    C[i, c], arg[i, c] = row[c], word
            first = False
    return C, arg


MUTANTS = ('stale_in_part', 'drop_out_of_part', 'grad_to_stale')


def _square(n):
    return sp.csr_matrix((int(n), int(n)), dtype=np.float32)


def backward(n, G, arg, add=None, add_rows=0):
    """dX (n, d) fp32: G[i, c] added to row arg[i, c] where that is a position in S, in ascending i; then the addend"""
    arg = np.asarray(arg)
    assert int(arg.max(initial=-1)) < n
    return spmax_ref.backward(_square(n), G, arg, add=add, add_rows=add_rows)


def backward_f64(n, G, arg, add=None, add_rows=0):
    """(dX in fp64, the per-element fp32 bound of spmax_ref.backward_f64)"""
    return spmax_ref.backward_f64(_square(n), G, np.asarray(arg), add=add, add_rows=add_rows)


def dense(a, ids, X, H):
    """C by np.max over dense masked columns of the merged table (values only; -inf never occurs in the tests that call it)"""
    sub = np.asarray(a.tocsr()[np.asarray(ids, dtype=np.int64)].astype(bool).todense())
    Z = merged32(ids, X, H)
    C = np.zeros((len(ids), Z.shape[1]), np.float32)
    for i in range(len(ids)):
        if sub[i].any():
            C[i] = Z[sub[i]].max(axis=0)
    return C


# ---- the estimator ------------------------------------------------------------------------------------------------------
class PartPullMaxModel(pr.PartHistoryModel):
    """part_history_ref.PartHistoryModel under --aggregator max --full_batch_part_pull_max"""

    def forward_part(self, ids, dropout, masks, stop_at_last_agg=False):
        fl, keep = self.flags, 1.0 - dropout
        concat = fl['normalization'] != 'gcn'
        ids = np.asarray(ids, dtype=np.int64)
        act = self.features[ids]
        tape, acts, self.pushed = [], [], {}
        self.margins, self.winners = [], {}
        last_agg = max(li for li, s in enumerate(self.specs) if s[0] == 'agg')
        sub = self.resident[ids].tocsr()
        for li, s in enumerate(self.specs):
            kind = s[0]
            if kind == 'dropout':
                m = masks('L%d' % li, act.shape) if dropout > 0 else None
                act = mnp.dropout_fwd(act, keep, m)
                tape.append(('dropout', m, keep))
            elif kind == 'dense':
                _, name, fin, fout, sparse_in, relu, norm = s
                assert not sparse_in
                y = pr._mm(act, self.params[name + '/weights'])
                ctx = None
                if norm:
                    y, ctx = mnp.layer_norm_fwd(y, self.params[name + '/offset'], self.params[name + '/scale'])
                pre = y
                if relu:
                    nz = np.abs(pre[pre != 0])
                    self.margins.append(('relu', li, float(nz.min()) if nz.size else np.inf, float(np.abs(pre).max())))
                    y = np.maximum(y, 0).astype(f32)
                tape.append(('dense', s, act, ctx, pre))
                act = y
            elif kind == 'agg':
                l = s[1]
                if stop_at_last_agg and li == last_agg:
                    self.push(l, ids, act)
                    self.pushed[l] = act
                    break
                Z = merged32(ids, act, self.table(l))
                read = np.unique(sub.indices)
                big = float(np.abs(Z[read]).max()) if read.size else 0.0
                self.margins.append(('max', li, top_two_gap(sub, Z), max(big, float(np.abs(act).max()))))
                C, arg = forward(self.resident, ids, act, self.table(l))
                self.winners[l] = (int(np.sum(arg >= 0)), int(np.sum(arg <= -2)))
                self.push(l, ids, act)                    # push after pull: columns in S never read the table
                self.pushed[l] = act
                tape.append(('agg', arg, concat, act.shape[1]))
                act = np.hstack([act, C]).astype(f32) if concat else C
            else:
                raise NotImplementedError(kind)
            acts.append(act)
        self._tape = tape
        return act, acts

    def backward(self, dout):
        grads = {k: np.zeros_like(v) for k, v in self.params.items()}
        g = dout
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
                grads[name + '/weights'] += pr._mm(xin.T, g)
                g = pr._mm(g, self.params[name + '/weights'].T)
            elif kind == 'dropout':
                _, m, keep = rec
                if m is not None:
                    g = (g * (m * f32(1.0 / keep))).astype(f32)
            elif kind == 'agg':
                _, arg, concat, d = rec                   # to in-part winners only: stored rows are constants
                n = g.shape[0]
                if concat:
                    g = backward_f64(n, g[:, d:], arg, add=g[:, :d], add_rows=n)[0].astype(f32)
                else:
                    g = backward_f64(n, g, arg)[0].astype(f32)
        wd = f32(self.flags['weight_decay'])
        for k in self._wd_names():
            grads[k] += wd * self.params[k]
        return grads

    def margin(self):
        """the smallest (non-zero gap or |ReLU input|) / (its layer's largest input magnitude) of the last forward"""
        worst = np.inf
        for kind, li, small, big in self.margins:
            if np.isfinite(small) and big > 0:
                worst = min(worst, small / big)
        return worst


def make_model(case, seed=None, params=None, bf16=False):
    """the PartPullMaxModel of a case dict, attached to its training adjacency (part_history_ref.make_model's signature)"""
    fl = case['flags']
    seed = case['cfg']['init'] if seed is None else seed
    args = (fl, fl['num_layers'], fl['preprocess'], False, False, case['feats'], case['nbr_train'], case['n'], case['classes'])
    if params is None:
        params = mnp.init_params(PartPullMaxModel(*args, {}).specs, seed)
    return PartPullMaxModel(*args, params).attach(case['train_adj'], bf16=bf16)
