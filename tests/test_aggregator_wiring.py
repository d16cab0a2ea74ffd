"""Which launches layers.PlainAggregator makes, with which operands and in which order -- on the CPU, with every launch wrapper the
aggregation path can reach replaced by a recorder.  The layer is a real PlainAggregator over a real full_batch.InducedMatrix /
PulledMatrix built on a stub block, reached the way the model reaches it: ``PartBatch(...).cur(x).adj[l]``.  Each recorded call is
(wrapper, {argument: value}) with the arguments that differ from the wrapper's defaults; a tensor is recorded as
(role, offset, shape, strides) -- the role is the storage it views (x, g, the concatenated output 'cat', table l, score table
l, ids, map, the attention vector, or the result of an earlier launch), the offset its first element's, in elements.  The
expected lists below are written out by hand from the launch sequences the aggregation layer has always made; nothing in them
is computed from the code under test.  This pins wiring, not arithmetic: n = 4 rows of N = 10 vertices, d = 8 columns."""
import inspect
import types

import pytest
import torch

from stochastic_gcn_amd import full_batch, layers, ops
from stochastic_gcn_amd.flags import FLAGS

n, N, d = 4, 10, 8
SEED, INDEX, STEP = 7, 3, 5                   # what the coefficient mask's key is drawn from
SLOPE = 0.3

WRAPPERS = ('spmm', 'spmm_pull', 'scatter_rows', 'gather_rows', 'spmax', 'spmax_bwd', 'spattn', 'spattn_bwd', 'spattn_pull',
            'spattn_pull_bwd_q', 'spattn_pull_bwd_kv', 'gat_scores', 'spgat', 'spgat_bwd', 'spgat_pull', 'spgat_pull_bwd_u',
            'spgat_pull_bwd_v', 'gat_scores_bwd')
SIGNATURES = {name: inspect.signature(getattr(ops, name)) for name in WRAPPERS}          # (the real wrappers': taken once)


@pytest.fixture(autouse=True)
def _reset_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


# ---- the recorders --------------------------------------------------------------------------------------------------------
class Recorder(object):
    """The stand-ins of the launch wrappers: each binds its arguments to the real wrapper's signature, keeps them, and returns
    CPU tensors of the shapes the real one returns (``out`` itself where one is given)."""

    def __init__(self, monkeypatch):
        self.calls, self.names, self.keep = [], {}, []
        for name in WRAPPERS:
            monkeypatch.setattr(ops, name, self._stand_in(name, SIGNATURES[name]))

    def name(self, role, thing):
        """``thing`` (a tensor: its storage; anything else: the object) is known as ``role`` from here on"""
        self.keep.append(thing)               # (alive to the end: no address is ever used twice)
        key = thing.untyped_storage().data_ptr() if isinstance(thing, torch.Tensor) else id(thing)
        self.names[key] = role
        return thing

    def new(self, role, shape, dtype=torch.float32):
        return self.name(role, torch.zeros(shape, dtype=dtype))

    def _stand_in(self, name, sig):
        def call(*args, **kw):
            b = sig.bind(*args, **kw)
            self.calls.append((name, sig, dict(b.arguments)))
            return getattr(self, '_' + name)(**{k: p.default for k, p in sig.parameters.items()
                                                 if p.default is not p.empty and k not in b.arguments}, **b.arguments)
        return call

    def _describe(self, v):
        if isinstance(v, torch.Tensor):
            role = self.names.get(v.untyped_storage().data_ptr(), '?')
            return (role, v.storage_offset(), tuple(v.shape), tuple(v.stride())) + \
                (() if v.dtype == torch.float32 else (str(v.dtype),))
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        return self.names.get(id(v), '?')

    def take(self):
        """the calls so far, described; the record starts over"""
        out = []
        for name, sig, arguments in self.calls:
            shown = {}
            for k, v in arguments.items():
                v, default = self._describe(v), sig.parameters[k].default
                if default is inspect.Parameter.empty or type(v) is not type(default) or v != default:
                    shown[k] = v
            out.append((name, shown))
        self.calls = []
        return out

    # what each wrapper returns
    def _result(self, role, out, shape, dtype=torch.float32):
        return out if out is not None else self.new(role, shape, dtype)

    def _spmm(self, A, B, out, **kw):
        return self._result('out', out, (A.shape[0], B.shape[1]))

    def _spmm_pull(self, A, ids_dev, map_dev, x, H, out):
        return self._result('out', out, (ids_dev.shape[0], x.shape[1]))

    def _scatter_rows(self, H, idx, src, d):
        return H

    def _gather_rows(self, inp, idx, out, d):
        return self._result('gathered', out, (inp.shape[0] if idx is None else idx.shape[0], inp.shape[1]))

    def _spmax(self, A, x, out, want_arg, arg):
        shape = (A.shape[0], x.shape[1])
        return self._result('out', out, shape), (self.new('arg', shape, torch.int32) if want_arg else None)

    def _spmax_bwd(self, At, g, arg, out, add, add_rows):
        return self._result('dx', out, (At.shape[0], g.shape[1]))

    def _lse(self, rows, heads, want_lse, flat):
        return self.new('lse', (rows,) if flat and heads == 1 else (rows, heads)) if want_lse else None

    def _spattn(self, A, x, q, scale, out, want_lse, heads, keep, key):
        return self._result('out', out, (A.shape[0], x.shape[1])), self._lse(A.shape[0], heads, want_lse, True)

    def _spattn_bwd(self, A, At, x, **kw):
        return self.new('dq', (A.shape[0], x.shape[1])), self.new('dx', tuple(x.shape))

    def _spattn_pull(self, A, ids_dev, map_dev, x, H, scale, out, want_lse, heads):
        return self._result('out', out, tuple(x.shape)), self._lse(x.shape[0], heads, want_lse, True)

    def _spattn_pull_bwd_q(self, A, ids_dev, map_dev, x, H, g, out_fwd, lse, scale, add, add_rows, heads):
        return self.new('dq', tuple(x.shape)), self.new('delta', (x.shape[0] * heads,))

    def _spattn_pull_bwd_kv(self, At, x, **kw):
        return self.new('dx', tuple(x.shape))

    def _gat_scores(self, x, a, heads):
        return self.new('S', (x.shape[0], 2 * heads))

    def _spgat(self, A, x, u, v, slope, out, want_lse, heads, keep, key):
        return self._result('out', out, (A.shape[0], x.shape[1])), self._lse(A.shape[0], heads, want_lse, False)

    def _spgat_bwd(self, A, At, x, u, v, g, out_fwd, lse, slope, add, add_rows, heads, keep, key):
        return (self.new('dB', tuple(x.shape)), self.new('dU', (A.shape[0], heads)), self.new('dV', (x.shape[0], heads)),
                self.new('delta', (A.shape[0], heads)))

    def _spgat_pull(self, A, ids_dev, map_dev, x, H, u, v, vh, slope, out, want_lse, heads):
        return self._result('out', out, tuple(x.shape)), self._lse(x.shape[0], heads, want_lse, False)

    def _spgat_pull_bwd_u(self, A, ids_dev, map_dev, x, H, u, v, vh, g, out_fwd, lse, slope, heads):
        return self.new('dU', (x.shape[0], heads)), self.new('delta', (x.shape[0], heads))

    def _spgat_pull_bwd_v(self, At, x, u, v, g, lse, delta, slope, add, add_rows, heads):
        return self.new('dB', tuple(x.shape)), self.new('dV', (x.shape[0], heads))

    def _gat_scores_bwd(self, x, a, dU, dV, dx, heads):
        return self.new('da', (2, x.shape[1]))


# ---- the matrices, the batch, the layer -------------------------------------------------------------------------------------
class Block(object):
    """What ops.csr_induce hands over, as far as the matrix classes look: a shape, a count, values, the position map, no plan
    and a transpose of the same kind."""
    plan = None

    def __init__(self, shape, vmap, transpose=None):
        self.shape, self.nnz, self.val, self.map = shape, 6, torch.zeros(6), vmap
        self.transpose = transpose if transpose is not None else Block((shape[1], shape[0]), vmap, self)


class Rig(object):
    """One part batch of L layers over ``matrix`` in ('induced', 'pulled', 'scored'), its stub model, and the recorder."""

    def __init__(self, monkeypatch, matrix, L=1, owned=None, heads=1, x_dtype=torch.float32, training=True):
        self.rec = rec = Recorder(monkeypatch)
        self.x = rec.name('x', torch.randn(n, d).to(x_dtype))
        ids, vmap = rec.name('ids', torch.arange(n, dtype=torch.int32)), rec.name('map', torch.full((N,), -1, dtype=torch.int32))
        block = rec.name('block', Block((n, n), vmap))
        rec.name('blockT', block.transpose)
        if matrix == 'induced':
            self.matrix = full_batch.InducedMatrix(block, torch.device('cpu'))
        else:
            resident = rec.name('resident', Block((N, N), None))
            tables = [rec.new('table%d' % l, (N, d)) for l in range(L)]
            scores = [rec.new('score%d' % l, (N, heads)) for l in range(L)] if matrix == 'scored' else None
            self.matrix = full_batch.PulledMatrix(block, resident, ids, tables, owned or [True] * L, torch.device('cpu'),
                                                  scores=scores)
        self.batch = full_batch.PartBatch(list(range(n)), ids, self.matrix, None, None, L)
        self.model = types.SimpleNamespace(cur=self.batch.cur(self.x), is_training=training, agg0_dim=d, dropout_seed=SEED,
                                           dropout_step=STEP)

    def layer(self, l=0, need_dx=True):
        layer = layers.PlainAggregator(self.model, l, name='agg%d' % l)
        layer.index, layer.need_dx = INDEX, need_dx
        if layer.param_shapes():
            layer.vars['attn_vec'], layer.grads['attn_vec'] = self.rec.new('a', (2, d)), torch.zeros(2, d)
        return layer

    def forward(self, layer, concat):
        out = layer.forward(self.x)
        if concat:
            assert tuple(out.shape) == (n, 2 * d) and out.is_contiguous()
            self.rec.name('cat', out)
        else:
            assert tuple(out.shape) == (n, d)
        return out, self.rec.take()

    def backward(self, layer, concat):
        g = self.rec.name('g', torch.randn(n, 2 * d if concat else d))
        return layer.backward(g), self.rec.take()


def flags(kind, concat, **more):
    f = dict(normalization='graphsage' if concat else 'gcn')
    if kind in ('attn', 'gat'):
        f.update(aggregator='attn')
    if kind == 'gat':
        f.update(attn_score='gat', attn_slope=SLOPE)
    if kind == 'max':
        f.update(aggregator='max')
    f.update(more)
    FLAGS.update(**f)


# ---- the operands, by name ------------------------------------------------------------------------------------------------------
X = ('x', 0, (n, d), (d, 1))
IDS, MAP = ('ids', 0, (n,), (1,), 'torch.int32'), ('map', 0, (N,), (1,), 'torch.int32')
A_VEC = ('a', 0, (2, d), (d, 1))
CAT_SELF, CAT_NBR = ('cat', 0, (n, d), (2 * d, 1)), ('cat', d, (n, d), (2 * d, 1))
G, G_SELF, G_NBR = ('g', 0, (n, d), (d, 1)), ('g', 0, (n, d), (2 * d, 1)), ('g', d, (n, d), (2 * d, 1))
OUT = ('out', 0, (n, d), (d, 1))
ARG = ('arg', 0, (n, d), (d, 1), 'torch.int32')
DQ, DB = ('dq', 0, (n, d), (d, 1)), ('dB', 0, (n, d), (d, 1))


def TAB(l):
    return ('table%d' % l, 0, (N, d), (d, 1))


def SCORE(l, H):
    return ('score%d' % l, 0, (N, H), (H, 1))


def LSE(H, flat=True):
    return ('lse', 0, (n,), (1,)) if flat and H == 1 else ('lse', 0, (n, H), (H, 1))


def U(H):
    return ('S', 0, (n, H), (2 * H, 1))


def V(H):
    return ('S', H, (n, H), (2 * H, 1))


def PER_HEAD(role, H):
    return (role, 0, (n, H), (H, 1))


def nbr_out(concat):
    """the keyword a forward launch takes its output through: the neighbour half of the concatenated output, or none"""
    return dict(out=CAT_NBR) if concat else {}


def res(concat):
    """what the forward launch returned"""
    return CAT_NBR if concat else OUT


def grad(concat):
    """(g as the backward launch reads it, the self half as its addend)"""
    return (G_NBR, dict(add=G_SELF, add_rows=n)) if concat else (G, {})


def eval_only(training):
    return {} if training else dict(want_lse=False)


# ---- the expected launches, by kind and matrix ------------------------------------------------------------------------------------
def want_sum(pulled, concat, l=0, owned=True):
    g, add = grad(concat)
    if not pulled:
        fwd = [('spmm', dict(A='block', B=X, **nbr_out(concat)))]
    else:
        fwd = [('spmm_pull', dict(A='resident', ids_dev=IDS, map_dev=MAP, x=X, H=TAB(l), **nbr_out(concat)))]
        fwd += [('scatter_rows', dict(H=TAB(l), idx=IDS, src=X))] if owned else []
    return fwd, [('spmm', dict(A='blockT', B=g, **add))]


def want_max(concat, training):
    g, add = grad(concat)
    fwd = [('spmax', dict(A='block', x=X, **nbr_out(concat), **({} if training else dict(want_arg=False))))]
    return fwd, [('spmax_bwd', dict(At='blockT', g=g, arg=ARG, **add))]


def want_attn(pulled, concat, training, H, l=0, owned=True, drop=None):
    g, add = grad(concat)
    scale = float(d // H) ** -0.5
    heads = dict(heads=H) if H != 1 else {}
    if not pulled:
        drop = drop or {}
        fwd = [('spattn', dict(A='block', x=X, scale=scale, **nbr_out(concat), **eval_only(training), **heads, **drop))]
        bwd = [('spattn_bwd', dict(A='block', At='blockT', x=X, q=None, g=g, out_fwd=res(concat), lse=LSE(H), scale=scale, **add, **heads,
                                   **drop))]
        return fwd, bwd
    fwd = [('spattn_pull', dict(A='resident', ids_dev=IDS, map_dev=MAP, x=X, H=TAB(l), scale=scale, **nbr_out(concat),
                                **eval_only(training), **heads))]
    fwd += [('scatter_rows', dict(H=TAB(l), idx=IDS, src=X))] if owned else []
    bwd = [('spattn_pull_bwd_q', dict(A='resident', ids_dev=IDS, map_dev=MAP, x=X, H=TAB(l), g=g, out_fwd=res(concat), lse=LSE(H),
                                      scale=scale, **add, **heads)),
           ('spattn_pull_bwd_kv', dict(At='blockT', x=X, g=g, lse=LSE(H), delta=('delta', 0, (n * H,), (1,)), dq=DQ, scale=scale,
                                       **heads))]
    return fwd, bwd


def want_gat(scored, concat, training, H, need_dx=True, owned=True, drop=None):
    g, add = grad(concat)
    add = add if need_dx else {}
    dx = dict(dx=DB) if need_dx else {}
    scores = ('gat_scores', dict(x=X, a=A_VEC, heads=H))
    scores_bwd = ('gat_scores_bwd', dict(x=X, a=A_VEC, dU=PER_HEAD('dU', H), dV=PER_HEAD('dV', H), heads=H, **dx))
    if not scored:
        drop = drop or {}
        fwd = [scores, ('spgat', dict(A='block', x=X, u=U(H), v=V(H), slope=SLOPE, **nbr_out(concat), **eval_only(training), heads=H,
                                      **drop))]
        bwd = [('spgat_bwd', dict(A='block', At='blockT', x=X, u=U(H), v=V(H), g=g, out_fwd=res(concat), lse=LSE(H, False),
                                  slope=SLOPE, heads=H, **add, **drop)), scores_bwd]
        return fwd, bwd
    fwd = [scores, ('spgat_pull', dict(A='resident', ids_dev=IDS, map_dev=MAP, x=X, H=TAB(0), u=U(H), v=V(H), vh=SCORE(0, H),
                                       slope=SLOPE, **nbr_out(concat), **eval_only(training), heads=H))]
    fwd += [('scatter_rows', dict(H=TAB(0), idx=IDS, src=X))] if owned else []
    fwd += [('scatter_rows', dict(H=SCORE(0, H), idx=IDS, src=V(H)))]
    bwd = [('spgat_pull_bwd_u', dict(A='resident', ids_dev=IDS, map_dev=MAP, x=X, H=TAB(0), u=U(H), v=V(H), vh=SCORE(0, H), g=g,
                                     out_fwd=res(concat), lse=LSE(H, False), slope=SLOPE, heads=H)),
           ('spgat_pull_bwd_v', dict(At='blockT', x=X, u=U(H), v=V(H), g=g, lse=LSE(H, False), delta=PER_HEAD('delta', H),
                                     slope=SLOPE, heads=H, **add)), scores_bwd]
    return fwd, bwd


MATRICES = ('induced', 'pulled', 'scored')
BOTH = (False, True)


def run(rig, layer, concat, want_fwd, want_bwd):
    """forward, and for a training model backward; the launches of each against the expected list"""
    out, got = rig.forward(layer, concat)
    assert got == want_fwd
    if not rig.model.is_training:
        return out, None
    dx, got = rig.backward(layer, concat)
    assert got == want_bwd
    return out, dx


# ---- the kinds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training", BOTH)
@pytest.mark.parametrize("concat", BOTH)
@pytest.mark.parametrize("matrix", MATRICES)
def test_sum(monkeypatch, matrix, concat, training):
    flags('sum', concat)
    rig = Rig(monkeypatch, matrix, training=training)
    layer = rig.layer()
    out, dx = run(rig, layer, concat, *want_sum(matrix != 'induced', concat))
    assert not layer._max and not layer._attn
    if training:
        assert tuple(dx.shape) == (n, d)


def test_sum_widens_a_bf16_self_half_with_gather_rows(monkeypatch):
    """--feature_dtype bf16 with concat: the self half goes through ops.gather_rows, the product reads the table as it is"""
    flags('sum', True)
    rig = Rig(monkeypatch, 'induced', x_dtype=torch.bfloat16)
    xb = X + ('torch.bfloat16',)
    _, got = rig.forward(rig.layer(), True)
    assert got == [('gather_rows', dict(inp=xb, idx=None, out=CAT_SELF)), ('spmm', dict(A='block', B=xb, out=CAT_NBR))]


@pytest.mark.parametrize("training", BOTH)
@pytest.mark.parametrize("concat", BOTH)
@pytest.mark.parametrize("matrix", MATRICES)
def test_max(monkeypatch, matrix, concat, training):
    """the maximum of a PulledMatrix is the block's (ops.spmax on it): no table is read, nothing is pushed"""
    flags('max', concat)
    rig = Rig(monkeypatch, matrix, training=training)
    layer = rig.layer()
    run(rig, layer, concat, *want_max(concat, training))
    assert layer._max
    assert (layer._arg is not None) == training


@pytest.mark.parametrize("training", BOTH)
@pytest.mark.parametrize("concat", BOTH)
@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("H", [1, 2])
def test_attn(monkeypatch, H, matrix, concat, training):
    flags('attn', concat, attn_heads=H)
    rig = Rig(monkeypatch, matrix, heads=H, training=training)
    layer = rig.layer()
    out, dx = run(rig, layer, concat, *want_attn(matrix != 'induced', concat, training, H))
    assert layer._attn and not layer._max and layer._heads == H and layer._scale == float(d // H) ** -0.5 and layer._drop == {}
    if training:
        assert layer._x is rig.x and layer._lse is not None and tuple(dx.shape) == (n, d)
        assert layer._out.data_ptr() == (out[:, d:] if concat else out).data_ptr()
    else:
        assert layer._x is None and layer._lse is None


@pytest.mark.parametrize("training", BOTH)
@pytest.mark.parametrize("concat", BOTH)
def test_attn_dropout_on_a_one_table_matrix(monkeypatch, concat, training):
    """a training model passes (keep, key) to both launches; an evaluation model never masks"""
    flags('attn', concat, attn_dropout=0.25)
    rig = Rig(monkeypatch, 'induced', training=training)
    layer = rig.layer()
    drop = dict(keep=0.75, key=ops.attn_key(SEED, INDEX, STEP)) if training else {}
    run(rig, layer, concat, *want_attn(False, concat, training, 1, drop=drop))
    assert layer._drop == drop


@pytest.mark.parametrize("training", BOTH)
@pytest.mark.parametrize("concat", BOTH)
@pytest.mark.parametrize("matrix", MATRICES)
def test_gat(monkeypatch, matrix, concat, training):
    """a PulledMatrix WITHOUT score tables runs the block's one-table launches and pushes nothing"""
    H = 2
    flags('gat', concat, attn_heads=H)
    rig = Rig(monkeypatch, matrix, heads=H, training=training)
    layer = rig.layer()
    out, dx = run(rig, layer, concat, *want_gat(matrix == 'scored', concat, training, H))
    assert layer._attn and layer._heads == H and layer._drop == {}
    if training:
        assert layer._x is rig.x and layer._lse is not None and layer._S is not None and tuple(dx.shape) == (n, d)
        assert layer._out.data_ptr() == (out[:, d:] if concat else out).data_ptr()
    else:
        assert layer._x is None and layer._lse is None and layer._S is None


@pytest.mark.parametrize("concat", BOTH)
@pytest.mark.parametrize("matrix", MATRICES)
def test_gat_without_dx(monkeypatch, matrix, concat):
    """the model's first parametrised layer: no addend, no dX -- the launch over the transpose still runs, for dV"""
    H = 2
    flags('gat', concat, attn_heads=H)
    rig = Rig(monkeypatch, matrix, heads=H)
    layer = rig.layer(need_dx=False)
    _, dx = run(rig, layer, concat, *want_gat(matrix == 'scored', concat, True, H, need_dx=False))
    assert dx is None


@pytest.mark.parametrize("concat", BOTH)
def test_gat_dropout_on_one_table_launches(monkeypatch, concat):
    """--attn_dropout under learned scores: (keep, key) in both launches, also over a PulledMatrix that carries no score tables"""
    H = 2
    drop = dict(keep=0.5, key=ops.attn_key(SEED, INDEX, STEP))
    for matrix in ('induced', 'pulled'):
        flags('gat', concat, attn_heads=H, attn_dropout=0.5)
        rig = Rig(monkeypatch, matrix, heads=H)
        layer = rig.layer()
        run(rig, layer, concat, *want_gat(False, concat, True, H, drop=drop))
        assert layer._drop == drop


# ---- tables: unowned, per layer ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("concat", BOTH)
@pytest.mark.parametrize("kind", ['sum', 'attn', 'gat'])
def test_an_unowned_table_is_read_and_never_written(monkeypatch, kind, concat):
    H = 2 if kind == 'gat' else 1
    flags(kind, concat, attn_heads=H)
    rig = Rig(monkeypatch, 'scored' if kind == 'gat' else 'pulled', owned=[False], heads=H)
    want = {'sum': lambda: want_sum(True, concat, owned=False), 'attn': lambda: want_attn(True, concat, True, 1, owned=False),
            'gat': lambda: want_gat(True, concat, True, H, owned=False)}[kind]()
    run(rig, rig.layer(), concat, *want)
    assert ('scatter_rows', dict(H=TAB(0), idx=IDS, src=X)) not in want[0]


@pytest.mark.parametrize("kind", ['sum', 'attn'])
def test_two_layers_read_their_own_tables(monkeypatch, kind):
    """layer 0 over the unowned (exact) table 0, layer 1 reads and writes table 1"""
    flags(kind, True)
    rig = Rig(monkeypatch, 'pulled', L=2, owned=[False, True])
    assert len(rig.model.cur.adj) == 2
    for l, owned in ((0, False), (1, True)):
        want = want_sum(True, True, l=l, owned=owned) if kind == 'sum' else want_attn(True, True, True, 1, l=l, owned=owned)
        run(rig, rig.layer(l), True, *want)


# ---- the refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("concat", BOTH)
@pytest.mark.parametrize("kind,matrix", [('attn', 'pulled'), ('attn', 'scored'), ('gat', 'scored')])
def test_attn_dropout_has_no_two_table_form(monkeypatch, kind, matrix, concat):
    flags(kind, concat, attn_heads=2, attn_dropout=0.25)
    rig = Rig(monkeypatch, matrix, heads=2)
    with pytest.raises(RuntimeError, match="--attn_dropout has no two-table form: the mask of out-of-part entries is not defined"):
        rig.layer().forward(rig.x)
    assert rig.rec.take() == []               # refused before any launch, before any push


MAX_ONLY = (r"--aggregator max runs on a full-graph matrix only \(full_batch.StaticMatrix\): a sampled minibatch adjacency has no "
            r"maximum kernel")
ATTN_ONLY = (r"--aggregator attn runs on a full-graph matrix only \(full_batch.StaticMatrix\): a sampled minibatch adjacency has "
             r"no attention kernel")
GAT_ONLY = r"--attn_score gat runs on a full-graph matrix only \(full_batch.StaticMatrix\)"


@pytest.mark.parametrize("concat", BOTH)
@pytest.mark.parametrize("kind,dot_only,msg", [
    ('max', False, MAX_ONLY), ('attn', False, ATTN_ONLY),
    ('gat', False, ATTN_ONLY),                # (a DeviceCSR has no attention of either kind: the first refusal speaks)
    ('gat', True, GAT_ONLY)])                 # (a matrix with dot-product attention alone)
def test_a_minibatch_adjacency_is_refused(monkeypatch, kind, dot_only, msg, concat):
    import numpy as np
    import scipy.sparse as sp
    flags(kind, concat)
    rec = Recorder(monkeypatch)
    A = ops.DeviceCSR.from_scipy(sp.identity(n, format='csr', dtype=np.float32), torch.device('cpu'), with_plan=False)
    if dot_only:
        A = types.SimpleNamespace(shape=A.shape, attn_product=None)
    model = types.SimpleNamespace(cur=types.SimpleNamespace(adj=[A]), is_training=True, agg0_dim=d)
    layer = layers.PlainAggregator(model, 0)
    layer.vars['attn_vec'] = torch.zeros(2, d)
    with pytest.raises(RuntimeError, match=msg):
        layer.forward(torch.zeros(n, d))
    assert rec.take() == []


# ---- a group without a training vertex ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("owned", BOTH)
@pytest.mark.parametrize("scored", BOTH)
def test_refresh_part_history_pushes_the_last_layers_input(monkeypatch, scored, owned):
    """models.GCN.refresh_part_history on a stub model whose forward stops in front of the last aggregation layer: table L-1
    takes the layer's input rows only where it is owned; with score tables, the fresh scores are formed and their destination
    half is stored"""
    from stochastic_gcn_amd import models
    H = 2
    flags('gat' if scored else 'sum', False, attn_heads=H if scored else 1)
    monkeypatch.setattr(ops, 'pin_stream', lambda: None)
    monkeypatch.setattr(ops, 'unpin_stream', lambda: None)
    rig = Rig(monkeypatch, 'scored' if scored else 'pulled', L=2, owned=[False, owned], heads=H)
    last = rig.layer(1)
    stopped = []
    model = types.SimpleNamespace(is_training=True, L=2, layers=[object(), last], activations=[None, rig.x], dropout_step=STEP,
                                  get_data=lambda batch: rig.model.cur, forward=lambda cur, stop: stopped.append((cur, stop)))
    models.GCN.refresh_part_history(model, rig.batch)
    assert stopped == [(rig.model.cur, 1)] and model.dropout_step == STEP + 1 and model.dropout == 0.0
    want = [('scatter_rows', dict(H=TAB(1), idx=IDS, src=X))] if owned else []
    if scored:
        want += [('gat_scores', dict(x=X, a=A_VEC, heads=H)), ('scatter_rows', dict(H=SCORE(1, H), idx=IDS, src=V(H)))]
    assert rig.rec.take() == want
