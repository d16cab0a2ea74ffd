"""Dense test cases: the GEMM's launch plan restated, case catalogues that cover every plan cell, exact (integer) references
and per-element fp64 error bounds for real-valued inputs (test-only helper; the sparse counterpart is sparse_cases.py).

Plans.  ``gemm_plan`` restates sgcn_gemm.hip ``split_factor`` + ``prepare_gemm`` (split-K factor, K chunk, effective
slices, K-groups, vector loads, grid) and ``bwd_plan`` the two guards of ``dense_bwd_run`` (the input gradient in the
LayerNorm / ReLU row pass, and its weights by direct LDS loads).  ``ws_floats`` must equal ``sgcn_gemm_ws_floats``: the
CPU suite checks that for every value of the knob gemm_min_steps the catalogues use.

Catalogues.  ``GEMM_CASES``, ``FWD_CASES`` and ``BWD_CASES`` hold one case for every reachable cell of their plan grid
(``*_cell``); which cells are reachable is found by scanning shapes and knobs (``*_reachable``), so a change of the
rules that opens a cell no case reaches fails the CPU suite.  Shapes are picked per cell from small pools, rotated by
the cell's index, so that every pool value meets several cells (the pairwise trimming of the sparse tests' PAIRS).

Exact inputs.  Small integers for every operand, dropout keeps of 0.5 or 0.8 (1.0f / 0.8f is exactly 1.25 in fp32), so
every term of an output lies on the grid 2^lo and the precondition of sparse_cases.assert_exact makes fp32 exact in any
summation order -- any split over K, any K-groups.  Real-valued inputs: ``gemm_bound``, ``ln_fwd_bound`` and
``ln_bwd_bound``.
"""
import zlib

import numpy as np

from sparse_cases import U, assert_exact, low_exp

kTM, kTN, kTK = 32, 128, 32          # sgcn_gemm.hip: block tile and K-step
DEFAULT_MIN_STEPS = 3                # split_factor's slice floor when the knob is 0
KNOBS = (0, 1, 2, 5, 10, 10 ** 6)    # values of gemm_min_steps the suite sets (10: long slices; 10^6: nothing is split)
NO_SPLIT = 10 ** 6
TINY = 2.0 ** -126                   # a result below it may be flushed to zero by an operation


def _cdiv(a, b):
    return -(-a // b)


# ---- the launch plan (sgcn_gemm.hip) --------------------------------------------------------------------------------------
def split_factor(M, N, K, min_steps=0):
    tiles = _cdiv(M, kTM) * _cdiv(N, kTN)
    s = 256 // max(tiles, 1)
    ms = min_steps if min_steps > 0 else DEFAULT_MIN_STEPS
    return max(min(s, K // (ms * kTK)), 1)


def ws_floats(M, N, K, min_steps=0):
    """sgcn_gemm_ws_floats"""
    if M <= 0 or N <= 0 or K <= 0:
        return 0
    s = split_factor(M, N, K, min_steps)
    return s * M * N if s > 1 else 0


def gemm_plan(M, N, K, ta=False, tb=False, ws=True, aligned_a=True, aligned_b=True, min_steps=0):
    """prepare_gemm: ``ws`` -- the caller passes a split-K workspace; ``aligned_*`` -- base pointer 16-byte aligned and
    row pitch a multiple of 4 floats.  Returns S_split (split_factor), kchunk, S (the effective number of K slices),
    KG, vec_a, vec_b and the grid."""
    vec_a = bool(aligned_a and (M if ta else K) % 4 == 0)
    vec_b = bool(aligned_b and (K if tb else N) % 4 == 0)
    s_split = split_factor(M, N, K, min_steps) if ws else 1
    kchunk = _cdiv(_cdiv(K, s_split), kTK) * kTK
    S = _cdiv(K, kchunk) if K > 0 else 1
    if K == 0:
        kchunk = kTK
    grid = (_cdiv(M, kTM), _cdiv(N, kTN), S)
    steps = _cdiv(min(kchunk, K), kTK)
    blocks = grid[0] * grid[1] * grid[2]
    kg = 4 if (blocks <= 128 and steps >= 8) else (2 if (blocks <= 256 and steps >= 4) else 1)
    return dict(S_split=s_split, kchunk=kchunk, S=S, KG=kg, vec_a=vec_a, vec_b=vec_b, grid=grid)


def ops_gemm_plan(M, N, K, ta=False, tb=False, aligned_a=True, aligned_b=True, min_steps=0, drop_c=False):
    """the plan of ops.gemm: a workspace when sgcn_gemm_ws_floats > 0, none with an output mask"""
    ws = ws_floats(M, N, K, min_steps) > 0 and not drop_c
    return gemm_plan(M, N, K, ta, tb, ws, aligned_a, aligned_b, min_steps)


def fwd_plan(M, N, K, min_steps=0):
    """the plan of ops.dense_fwd (workspace only for N <= 128): its path is 'kg1' / 'kg2' / 'kg4' (gemm_body's own
    epilogue) or 'splitk' (partial tiles, then splitk_ln_act_kernel -- or splitk_reduce_kernel for a plain layer)"""
    p = gemm_plan(M, N, K, ws=N <= kTN and ws_floats(M, N, K, min_steps) > 0, min_steps=min_steps)
    p["path"] = "splitk" if p["S"] > 1 else "kg%d" % p["KG"]
    return p


def bwd_plan(n, N, K, act, drop_keep=None, step_fuse=127, min_steps=0, W_aligned=True):
    """dense_bwd_run: dx in the LayerNorm / ReLU row pass ('row_direct': the weights by direct LDS loads, N in {32, 64,
    128}; 'row_lds': staged through registers and transposed) or by the MFMA launch ('mfma'); kg of the row pass; the
    plan of the weight-gradient GEMM dW[K x N] = x^T g and of the dx GEMM."""
    drop_on = drop_keep is not None and drop_keep < 1.0
    dx, kg = "mfma", 0
    if act != "none" and (step_fuse & 8) and N <= 128 and N % 4 == 0 and K <= 256 and W_aligned and \
            (8 * N + N * (K + 1)) * 4 <= 160 * 1024:
        if drop_on:
            q = gemm_plan(n, K, N, ws=False, min_steps=min_steps)
        else:
            q = gemm_plan(n, K, N, ws=ws_floats(n, K, N, min_steps) > 0, min_steps=min_steps)
        if q["S"] == 1 and q["KG"] <= 2:
            dx, kg = ("row_direct" if N in (32, 64, 128) else "row_lds"), q["KG"]
    ws = (act in ("ln", "ln_relu")) or max(ws_floats(K, N, n, min_steps), ws_floats(n, K, N, min_steps)) > 0
    dw = gemm_plan(K, N, n, ta=True, ws=ws, min_steps=min_steps)
    dxg = gemm_plan(n, K, N, tb=True, ws=ws and not drop_on, min_steps=min_steps)
    return dict(dx=dx, kg=kg, dw=dw, dx_gemm=dxg)


# ---- cells and the scans that find the reachable ones ----------------------------------------------------------------------
def gemm_cell(c):
    p = ops_gemm_plan(c["M"], c["N"], c["K"], c["ta"], c["tb"], c.get("vec_a", "on") == "on", c.get("vec_b", "on") == "on",
                      c.get("knob", 0), bool(c.get("drop_c")))
    return (c["ta"], c["tb"], p["KG"], p["S"] > 1, p["vec_a"], p["vec_b"])


def n_class(N):
    return "1" if N == 1 else "3" if N == 3 else "64" if N == 64 else "128" if N == 128 else \
        "lt64" if N < 64 else "65_127" if N < 128 else "gt128"


EPIS = ("plain", "relu", "ln", "ln_relu")
FWD_PATHS = ("kg1", "kg2", "kg4", "splitk")
N_CLASSES = ("1", "3", "lt64", "64", "65_127", "128")


def fwd_cell(c):
    return (c["epi"], fwd_plan(c["M"], c["N"], c["K"], c.get("knob", 0))["path"], n_class(c["N"]))


ACTS = ("none", "relu", "ln", "ln_relu")
DROPS = ("off", "keep1", "drop")


def _drop_keep(kind):
    return None if kind == "off" else 1.0 if kind == "keep1" else 0.8


def bwd_cell(c):
    p = bwd_plan(c["n"], c["N"], c["K"], c["act"], _drop_keep(c["drop"]))
    return (c["act"], p["dx"], p["kg"], p["dw"]["S"] > 1, c["drop"], bool(c["gidx"]))


SCAN_M = (1, 3, 5, 31, 32, 33, 64, 97, 128, 300, 700, 2042, 4096, 4097, 8192, 9000)
SCAN_K = (0, 1, 24, 64, 70, 96, 97, 128, 160, 191, 192, 224, 225, 256, 300, 602, 960, 1024, 1204, 1280, 4000)


def gemm_reachable():
    """(ta, tb, KG, S > 1, vec_a, vec_b) over shapes, knobs and operand alignments"""
    cells = set()
    for M in SCAN_M:
        for N in (1, 3, 40, 64, 128, 132, 256, 1204):
            for K in SCAN_K:
                for knob in KNOBS:
                    for al_a in (True, False):
                        for al_b in (True, False):
                            for ta in (False, True):
                                for tb in (False, True):
                                    p = ops_gemm_plan(M, N, K, ta, tb, al_a, al_b, knob)
                                    cells.add((ta, tb, p["KG"], p["S"] > 1, p["vec_a"], p["vec_b"]))
    return cells


def fwd_reachable():
    cells = set()
    for M in SCAN_M:
        for N in (1, 3, 30, 64, 100, 128):          # (for N <= 128 the plan does not depend on N: one tile column)
            for K in SCAN_K[1:]:
                for knob in KNOBS:
                    path = fwd_plan(M, N, K, knob)["path"]
                    for epi in EPIS:
                        cells.add((epi, path, n_class(N)))
    return cells


BWD_N = (1, 3, 5, 40, 77, 300, 3000, 4500, 9000)


def bwd_reachable():
    cells = set()
    for n in BWD_N:
        for N in (1, 3, 30, 32, 36, 60, 64, 96, 100, 128, 160):
            for K in (1, 24, 64, 128, 200, 256, 300):
                for act in ACTS:
                    for drop in DROPS:
                        p = bwd_plan(n, N, K, act, _drop_keep(drop))
                        for gidx in (False, True):
                            cells.add((act, p["dx"], p["kg"], p["dw"]["S"] > 1, drop, gidx))
    return cells


def _pick(cands, cell, i):
    """one candidate (rotated by the cell's index, so that the pools spread over the cells)"""
    if not cands:
        raise AssertionError("no candidate reaches the cell %r" % (cell,))
    return cands[(i * 7 + zlib.crc32(repr(cell).encode())) % len(cands)]


# ---- the catalogues --------------------------------------------------------------------------------------------------------
# ops.gemm: per (K-groups, split) a base shape, every width a multiple of 4 so that vec_a / vec_b are decided by the operands'
# pitch or base pointer only; a vector-load-off operand gets a pitch of width + 1 ('pitch') or a base one float past an
# aligned one ('shift'), in turn.  knob: gemm_min_steps for the case.
GEMM_BASE = {
    (1, False): dict(M=36, N=44, K=72),                      # 3 K-steps
    (2, False): dict(M=100, N=60, K=160),                    # 5 K-steps, K < 2 x 96: not split
    (4, False): dict(M=64, N=128, K=300, knob=NO_SPLIT),     # 10 K-steps in one slice
    (1, True): dict(M=128, N=128, K=960),                    # 10 slices of 3 K-steps
    (2, True): dict(M=128, N=132, K=1024),                   # 8 slices of 4 K-steps, a partial column tile
    (4, True): dict(M=96, N=40, K=1280, knob=10),            # 4 slices of 10 K-steps
}


def _gemm_cases():
    cases, i = [], 0
    for (kg, split), base in sorted(GEMM_BASE.items()):
        for ta in (False, True):
            for tb in (False, True):
                for va in ("on", "off"):
                    for vb in ("on", "off"):
                        c = dict(base, ta=ta, tb=tb, knob=base.get("knob", 0),
                                 vec_a=va, vec_b=vb, off_a=("pitch", "shift")[i % 2], off_b=("shift", "pitch")[(i // 2) % 2],
                                 accumulate=i % 3 == 1)
                        assert gemm_cell(c) == (ta, tb, kg, split, va == "on", vb == "on"), c
                        cases.append(c)
                        i += 1
    # odd widths (the scalar path because of the width), the masks, the smallest shapes
    cases += [dict(M=33, N=41, K=70, ta=ta, tb=tb, knob=0, accumulate=ta) for ta in (False, True) for tb in (False, True)]
    cases += [dict(M=31, N=7, K=33, ta=True, tb=True, knob=0), dict(M=1, N=1, K=1, ta=False, tb=False, knob=0),
              dict(M=5, N=3, K=4000, ta=False, tb=True, knob=0, accumulate=True),
              dict(M=300, N=128, K=96, ta=False, tb=False, knob=0, drop_a=0.8),                   # a forward layer's form
              dict(M=96, N=128, K=1000, ta=True, tb=False, knob=0, drop_a=0.5, accumulate=True),  # dW, split
              dict(M=36, N=100, K=300, ta=True, tb=False, knob=NO_SPLIT, drop_a=0.8, vec_a="off", off_a="shift"),
              dict(M=77, N=40, K=41, ta=False, tb=True, knob=0, drop_c=0.8),                      # dx, odd widths
              dict(M=100, N=256, K=300, ta=False, tb=True, knob=0, drop_c=0.5)]                   # dx, K-groups 4
    return cases


GEMM_CASES = _gemm_cases()


N_POOL = {"1": (1,), "3": (3,), "lt64": (16, 41, 60, 30), "64": (64,), "65_127": (65, 100, 127, 96), "128": (128,)}
FWD_M = (300, 5, 31, 700, 97, 64, 1000)
FWD_K = {"kg1": (72, 40, 96), "kg2": (160, 128, 100), "kg4": (300, 256, 602), "splitk": (1204, 602, 400)}


def _fwd_cases():
    cases = []
    cells = sorted(fwd_reachable())
    for i, cell in enumerate(cells):
        epi, path, ncls = cell
        knob = NO_SPLIT if path == "kg4" else 0
        cands = [dict(M=M, N=N, K=K, knob=knob) for M in FWD_M for N in N_POOL[ncls] for K in FWD_K[path]
                 if fwd_plan(M, N, K, knob)["path"] == path]
        c = dict(_pick(cands, cell, i), epi=epi)
        M = c["M"]
        c["split"] = (None, 0, min(37, M), M)[i % 4]             # [x ; x2] stacked at row split (None: no x2)
        c["gather"] = ("none", "x", "x2", "both")[(i // 4) % 4]   # operands read through an index with repeated ids
        c["drop"] = (None, 0.8, 0.5)[i % 3]
        assert fwd_cell(c) == cell
        cases.append(c)
    # wide plain layers (no split-K workspace: N > 128 runs gemm_body with its own K-groups)
    cases += [dict(M=300, N=200, K=300, knob=0, epi="plain", split=37, gather="x", drop=0.8),
              dict(M=64, N=256, K=96, knob=0, epi="plain", split=None, gather="none", drop=None),
              dict(M=2000, N=130, K=1204, knob=0, epi="plain", split=2000, gather="both", drop=0.5)]
    return cases


FWD_CASES = _fwd_cases()


BWD_POOL_N = (30, 32, 36, 64, 100, 128)
BWD_POOL_K = (24, 64, 200, 256, 300)
BWD_POOL_n = (1, 3, 5, 3000, 4500)


def _bwd_cases():
    cases = []
    for i, cell in enumerate(sorted(bwd_reachable())):
        act, dx, kg, split, drop, gidx = cell
        cands = [dict(n=n, N=N, K=K, act=act, drop=drop, gidx=gidx) for n in BWD_POOL_n for N in BWD_POOL_N + (160,)
                 for K in BWD_POOL_K if bwd_cell(dict(n=n, N=N, K=K, act=act, drop=drop, gidx=gidx)) == cell]
        cases.append(_pick(cands, cell, i))
    return cases


BWD_CASES = _bwd_cases()


# ---- exact references -------------------------------------------------------------------------------------------------------
def f32_scale(keep):
    """the kernels' 1 / keep (fp32)"""
    return float(np.float32(1.0) / np.float32(keep))


def _op(x, t):
    x = np.asarray(x, np.float64)
    return x.T if t else x


def gemm_f64(A, B, ta=False, tb=False, C_in=None, accumulate=False, mask_a=None, scale_a=1.0, mask_c=None, scale_c=1.0):
    """(C, mag, lo): the fp64 value of C = op(A m_a s_a) op(B) (* m_c s_c) (+ C_in), the per-element sum of term
    magnitudes, and the grid exponent of its terms.  m_a is a mask of the STORED A, m_c of the output."""
    Ae = np.asarray(A, np.float64) if mask_a is None else np.asarray(A, np.float64) * mask_a * scale_a
    a, b = _op(Ae, ta), _op(B, tb)
    C = a @ b
    mag = np.abs(a) @ np.abs(b)
    lo = low_exp(a) + low_exp(b)
    if mask_c is not None:
        C, mag, lo = C * mask_c * scale_c, mag * scale_c, lo + low_exp(np.float64(scale_c))
    if accumulate:
        C = C + np.asarray(C_in, np.float64)
        mag = mag + np.abs(np.asarray(C_in, np.float64))
        lo = min(lo, low_exp(C_in))
    return C, mag, lo


def gemm_exact(A, B, ta=False, tb=False, C_in=None, accumulate=False, mask_a=None, scale_a=1.0, mask_c=None, scale_c=1.0):
    """the exact product after asserting sparse_cases' precondition on every element (a K-term sum of terms on the grid
    2^lo, below 2^(24 + lo), is exact in fp32 in any order; an output mask's scale is applied to an exact sum)"""
    C, mag, lo = gemm_f64(A, B, ta, tb, C_in, accumulate, mask_a, scale_a, mask_c, scale_c)
    assert_exact(mag, lo, "the GEMM")
    assert np.array_equal(C.astype(np.float32).astype(np.float64), C)
    return C


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def gemm_bound(A, B, ta=False, tb=False, C_in=None, accumulate=False, mask_a=None, scale_a=1.0, mask_c=None, scale_c=1.0):
    """|fp32 result - fp64 value| <= bound, element by element, for the product of gemm_f64.

    Derivation (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Lemma 3.1 and section 3.1).  With
    gamma_k = k u / (1 - k u), u = 2^-24, a quantity formed by k rounded operations is within a factor (1 + theta_k),
    |theta_k| <= gamma_k, of the exact one.  An output element is a sum of K products a_ik b_kj.  Each product is
    rounded at most once (an MFMA's fused multiply-add rounds product and sum together).  However the K terms are
    grouped -- 32-wide K-steps, K-groups that take alternate steps and are added in group order, split-K slices added
    by a reduce kernel in slice order -- the sum of K terms is a binary tree of K - 1 additions, and a term meets at most
    K - 1 of them; the zeros loaded past the end of K add exactly.  The epilogue adds: the accumulate addition (+1), the
    rounding of a dropout-scaled operand x * (1 / keep) before its product (+1 when the operand is masked), the output
    mask's scale (+1).  So, with n = K + 1 + those:

        |fl(C_ij) - C_ij| <= gamma_n (sum_k |a_ik| |b_kj| + |C_in,ij|)

    A result below 2^-126 may be flushed to zero by any of the n operations: an absolute floor of n 2^-126."""
    _, mag, _ = gemm_f64(np.abs(A), np.abs(B), ta, tb, np.abs(C_in) if accumulate else None, accumulate,
                         mask_a, abs(scale_a), mask_c, abs(scale_c))
    K = (np.asarray(A).shape[0] if ta else np.asarray(A).shape[1])
    n = K + 1 + int(accumulate) + int(mask_a is not None) + int(mask_c is not None)
    return gamma(n) * mag + n * TINY


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------
RSQ_ERR = 4 * U          # the relative error of rsqrtf (v_rsq_f32: 1 ulp, taken as 2 ulps = 2^-22)


def ln_f64(v, offset, scale, relu, eps):
    """fp64 (y, xhat, rstd) of act(LN(v) * scale + offset) (ref64.ln_act's formula)"""
    import ref64
    v = np.asarray(v, np.float64)
    y = ref64.ln_act(ref64.t64(v), ref64.t64(offset), ref64.t64(scale), relu, eps).numpy()
    m = v.mean(1, keepdims=True)
    rs = 1.0 / np.sqrt(((v - m) ** 2).mean(1, keepdims=True) + eps)
    return y, (v - m) * rs, rs[:, 0]


def ln_fwd_bound(v, offset, scale, eps, pre_err=None, sum_exact=False):
    """Per-element bounds (y, xhat, rstd) on |fp32 - fp64| for the fused epilogues (gemm_body, splitk_ln_act_kernel),
    given the exact pre-activation v and a bound pre_err on the error of the pre-activation the kernel normalises.

    The kernel (N columns): mean = fl(sum v / N); t = fl(v - mean); rs = rsqrtf(fl(sum t^2 / N) + eps); xhat = fl(t rs);
    y = act(xhat scale + offset).  Let d = v - m be the exact centred values, s^2 = sum d^2 / N, R = (s^2 + eps)^-1/2.
      mean: the sum of N values rounds N - 1 times, the division once: |mean - m| <= dm = mean(pre_err) +
            gamma_N mean(|v| + pre_err) -- or u |m| when the sum is exact (small integers: sum_exact).
      t:    |t - d| <= e = pre_err + dm + u (|d| + pre_err + dm).
      q:    sum t^2 differs from sum d^2 by at most sum (2 |d| e + e^2); the squares, N - 1 additions, the division and
            the + eps round N + 2 times: rho_q = |q - (s^2 + eps)| / (s^2 + eps) <= (sum (2|d|e + e^2) / N +
            gamma_{N+2} (sum (|d| + e)^2 / N + eps)) / (s^2 + eps).
      rs:   (1 - rho)^-1/2 - 1 <= rho / (1 - rho), times the rsqrt error: |rs - R| <= R rho_rs,
            rho_rs = (1 + rho_q / (1 - rho_q)) (1 + RSQ_ERR) - 1   (no bound when rho_q >= 1/2).
      xhat: |fl(t rs) - d R| <= (1 + u) (e R (1 + rho_rs) + |d| R rho_rs) + u |d| R.
      y:    two roundings (a product and a sum, or one fused): |y - Y| <= |dxhat| |scale| (1 + u)^2 +
            gamma_2 ((|d R| + |dxhat|) |scale| + |offset|); ReLU does not increase it.
    The bounds grow with the row's conditioning |m| / s through e / s: a row far from zero mean loses digits to the
    cancellation in v - mean."""
    v = np.asarray(v, np.float64)
    N = v.shape[1]
    pe = np.zeros_like(v) if pre_err is None else np.asarray(pre_err, np.float64)
    m = v.mean(1, keepdims=True)
    d = v - m
    if sum_exact:
        dm = U * np.abs(m) + pe.mean(1, keepdims=True)
    else:
        dm = pe.mean(1, keepdims=True) + gamma(N) * (np.abs(v) + pe).mean(1, keepdims=True)
    e = pe + dm + U * (np.abs(d) + pe + dm)
    q = (d * d).mean(1, keepdims=True) + eps
    rho_q = ((2 * np.abs(d) * e + e * e).mean(1, keepdims=True) +
             gamma(N + 2) * (((np.abs(d) + e) ** 2).mean(1, keepdims=True) + eps)) / q
    with np.errstate(divide="ignore", invalid="ignore"):
        rho_rs = np.where(rho_q < 0.5, (1 + rho_q / (1 - rho_q)) * (1 + RSQ_ERR) - 1, np.inf)
    R = 1.0 / np.sqrt(q)
    with np.errstate(invalid="ignore"):
        bx = (1 + U) * (e * R * (1 + rho_rs) + np.abs(d) * R * rho_rs) + U * np.abs(d) * R
    bx = np.where(np.isfinite(rho_rs), bx, np.inf)
    sc, of = np.abs(np.asarray(scale, np.float64)).reshape(1, -1), np.abs(np.asarray(offset, np.float64)).reshape(1, -1)
    by = bx * sc * (1 + U) ** 2 + gamma(2) * ((np.abs(d) * R + bx) * sc + of) + 2 * TINY
    return by, bx + TINY, (R * rho_rs)[:, 0]


def ln_bwd_f64(v, offset, scale, relu, eps, dy):
    """ref64 autograd of act(LN(v) * scale + offset) at v: (g = d/dv, d offset, d scale) for the upstream dy"""
    import ref64
    _, (g, doff, dsc) = ref64.vjp(lambda a, o, s: ref64.ln_act(a, o, s, relu, eps),
                                  [np.asarray(v, np.float64), np.asarray(offset, np.float64).ravel(),
                                   np.asarray(scale, np.float64).ravel()], [np.asarray(dy, np.float64)])
    return g, doff, dsc


def ln_bwd_bound(gm, xhat64, rstd64, scale):
    """Per-element bound on |g - G| for the LayerNorm backward row pass (sgcn_dense.hip ln_bwd_stats / ln_bwd_out) fed
    the fp32 roundings of the exact xhat and rstd (relative errors <= u each), where gm is the upstream gradient after the
    ReLU mask (exact) and G = R (gm s - M1 - h M2), M1 = mean(gm s), M2 = mean(gm s h) is autograd's value.
      m1 = fl(sum fl(gm s) / N): |m1 - M1| <= E1 = gamma_{N+1} mean(|gm s|);
      m2 = fl(sum fma(fl(gm s), h32) / N), h32 = h (1 + alpha): E2 = gamma_{N+2} mean(|gm s h|);
      X = fma(gm, s, -m1): |X - (gm s - M1)| <= eX = E1 + u (|gm s| + |M1| + E1);
      fma(-h32, m2, X): |h32 m2 - h M2| <= eH = |h| (E2 + u |M2| + u E2);
        |inner - I| <= eI = (eX + eH)(1 + u) + u (|I| + eX + eH),   I = gm s - M1 - h M2;
      r32 * inner, r32 = R (1 + beta): |g - R I| <= R ((1 + u)^2 eI + gamma_2 |I|)."""
    N = gm.shape[1]
    s = np.asarray(scale, np.float64).reshape(1, -1)
    h = np.asarray(xhat64, np.float64)
    R = np.asarray(rstd64, np.float64).reshape(-1, 1)
    gs = gm * s
    M1 = gs.mean(1, keepdims=True)
    M2 = (gs * h).mean(1, keepdims=True)
    E1 = gamma(N + 1) * np.abs(gs).mean(1, keepdims=True)
    E2 = gamma(N + 2) * np.abs(gs * h).mean(1, keepdims=True)
    eX = E1 + U * (np.abs(gs) + np.abs(M1) + E1)
    eH = np.abs(h) * (E2 + U * np.abs(M2) + U * E2)
    I = gs - M1 - h * M2
    eI = (eX + eH) * (1 + U) + U * (np.abs(I) + eX + eH)
    return R * ((1 + U) ** 2 * eI + gamma(2) * np.abs(I)) + 4 * TINY
