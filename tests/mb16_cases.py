"""Cases of the bf16-multiply GEMM (sgcn_gemm_mb16.hip, ops.gemm_bf16): its launch plan restated, a catalogue with one
case for every reachable plan cell, and the references (test-only helper; the fp32 kernel's counterpart is dense_cases.py).

Plan.  A 128 x 128 tile per workgroup, K-steps of 32.  ``split_factor`` restates mb16_split_factor: the K range is cut
until the grid has about 512 workgroups, every slice keeping at least gemm_mb16_slice_k of K (0: 2048); the chunk is
rounded up to whole K-steps, so the effective number of slices can be smaller and the last one is uneven.  The rule is the
same for the three forms.  An operand loads by float4 when its base is 16-byte aligned, its pitch a multiple of 4 floats
and the length of its contiguous runs (K for a k-contiguous operand, M or N for a k-major one) a multiple of 4; otherwise
by scalar loads.  An output mask (drop_c) switches split-K off, as in the fp32 kernel.

Cells.  (form, split, vec_a, vec_b, accumulate, drop) with form in NN / NT / TN and drop in none / a / c.  ``reachable``
scans shapes, knobs and alignments; ``CASES`` holds one case per reachable cell, shapes rotated through the pools.

References.  Exact: small integers (bf16-representable, and so are their products with the fp32 scales 2 and 1.25 of the
keeps 0.5 and 0.8), dense_cases.gemm_exact.  Real-valued: the fp64 product of the operands rounded as the kernel rounds
them (``rounded_operands``), within ``bound``: dense_cases.gemm_bound on the rounded operands with its gamma(n) * mag term
doubled -- that bound takes each of the <= K - 1 additions a term meets as a correctly rounded fp32 addition (half an ulp);
the 16-term sum inside one MFMA is not documented to be one, so one ulp per addition is assumed; mag bounds every partial
sum."""
import numpy as np

import bf16_ref
import dense_cases as dc

kTM, kTN, kTK = 128, 128, 32         # sgcn_gemm_mb16.hip: block tile and K-step
DEFAULT_SLICE_K = 2048               # the slice floor when the knob gemm_mb16_slice_k is 0
TARGET_BLOCKS = 512
NO_SPLIT = 2 ** 30
KNOBS = (0, 64, 300, 1024, NO_SPLIT)  # values of gemm_mb16_slice_k the suite sets
FORMS = {"NN": (False, False), "NT": (False, True), "TN": (True, False)}


def _cdiv(a, b):
    return -(-a // b)


def split_factor(M, N, K, slice_k=0):
    tiles = _cdiv(M, kTM) * _cdiv(N, kTN)
    sk = slice_k if slice_k > 0 else DEFAULT_SLICE_K
    return max(min(TARGET_BLOCKS // max(tiles, 1), K // sk), 1)


def ws_floats(ta, tb, M, N, K, slice_k=0):
    """sgcn_gemm_mb16_ws_floats"""
    if M <= 0 or N <= 0 or K <= 0:
        return 0
    s = split_factor(M, N, K, slice_k)
    return s * M * N if s > 1 else 0


def plan(M, N, K, ta=False, tb=False, aligned_a=True, aligned_b=True, slice_k=0, drop_c=False):
    """what sgcn_gemm_mb16_f32 decides for a call of ops.gemm_bf16 (a workspace exactly when ws_floats > 0 and there is no
    output mask): kchunk, S (effective slices), the last slice's length, vec_a, vec_b, the grid"""
    ws = ws_floats(ta, tb, M, N, K, slice_k) > 0 and not drop_c
    s = split_factor(M, N, K, slice_k) if ws else 1
    kchunk = _cdiv(_cdiv(K, s), kTK) * kTK
    S = _cdiv(K, kchunk) if K > 0 else 1
    if K == 0:
        kchunk = kTK
    return dict(kchunk=kchunk, S=S, last=K - (S - 1) * kchunk,
                vec_a=bool(aligned_a and (M if ta else K) % 4 == 0), vec_b=bool(aligned_b and (K if tb else N) % 4 == 0),
                grid=(_cdiv(M, kTM), _cdiv(N, kTN), S))


def _drop_kind(c):
    return "a" if c.get("drop_a") else "c" if c.get("drop_c") else "none"


def cell(c):
    ta, tb = FORMS[c["form"]]
    p = plan(c["M"], c["N"], c["K"], ta, tb, c.get("vec_a", "on") == "on", c.get("vec_b", "on") == "on", c.get("knob", 0),
             bool(c.get("drop_c")))
    return (c["form"], p["S"] > 1, p["vec_a"], p["vec_b"], bool(c.get("accumulate")), _drop_kind(c))


# shape pools: the issue's, the tile sizes +- 1, and two more multiples of 4 (44, 132) so that vector loads meet partial tiles
POOL_MN = (1, 3, 31, 33, 41, 128, 130, 300, 127, 129, 44, 132)
POOL_K = (1, 7, 8, 15, 16, 17, 40, 602, 1204, 31, 32, 33, 600)
POOL_K_TN = (1, 33, 4097, 70001, 32, 4096)
TN_KNOB = 1024                       # 4097 -> 4 slices of 1056, the last one 929; 70001 -> 67 slices, the last one 305


def reachable():
    cells = set()
    for form, (ta, tb) in FORMS.items():
        for M in POOL_MN:
            for N in POOL_MN:
                for K in (POOL_K_TN if ta else POOL_K):
                    for knob in KNOBS:
                        for al_a in (True, False):
                            for al_b in (True, False):
                                for drop in ("none", "a", "c"):
                                    p = plan(M, N, K, ta, tb, al_a, al_b, knob, drop == "c")
                                    for acc in (False, True):
                                        cells.add((form, p["S"] > 1, p["vec_a"], p["vec_b"], acc, drop))
    return cells


def _cases():
    cases = []
    for i, cl in enumerate(sorted(reachable())):
        form, split, va, vb, acc, drop = cl
        ta, tb = FORMS[form]
        # the widths that decide the load classes: a vector-load operand needs a run length that is a multiple of 4; a
        # scalar-load one gets an odd width (every other case) or a multiple of 4 behind an odd pitch / a shifted base
        odd_a, odd_b = (not va) and i % 2 == 0, (not vb) and (i // 2) % 2 == 0
        if form == "NT":             # both operands' runs are K long: one width decides both
            odd_a = odd_a and not vb
            odd_b = odd_a if not va else False
        ks = (POOL_K_TN if ta else POOL_K)
        if split:
            ks = tuple(k for k in ks if k >= 600)
            knob = TN_KNOB if ta else (64, 300)[i % 2]
        else:
            ks = tuple(k for k in ks if k <= 1204)
            knob = (0, NO_SPLIT)[i % 2]
        cands = []
        for M in POOL_MN:
            for N in POOL_MN:
                for K in ks:
                    if K > 8192 and max(M, N) > 44:          # (the long sums on narrow outputs: the host reference stays quick)
                        continue
                    wa, wb = (M if ta else K), (K if tb else N)
                    if (wa % 4 != 0) != odd_a or (wb % 4 != 0) != odd_b:
                        continue
                    c = dict(form=form, M=M, N=N, K=K, knob=knob, accumulate=acc,
                             vec_a="on" if va else "off", vec_b="on" if vb else "off",
                             off_a=("pitch", "shift")[i % 2], off_b=("shift", "pitch")[(i // 2) % 2])
                    if odd_a:
                        c["vec_a"] = None            # (an odd pitch: width + 3)
                    if odd_b:
                        c["vec_b"] = None
                    if drop != "none":
                        c["drop_" + drop] = (0.5, 0.8)[i % 2]
                    cc = dict(c, vec_a=c["vec_a"] or "on", vec_b=c["vec_b"] or "on")
                    if cell(cc) == cl:
                        cands.append(c)
        cases.append(dc._pick(cands, cl, i))
    # the long weight-gradient sum (K = 70,001: 67 slices) with a mask on the operand, and the smallest shape of every form
    cases.append(dict(form="TN", M=41, N=130, K=70001, knob=TN_KNOB, accumulate=True, drop_a=0.8, vec_a=None, vec_b="off",
                      off_b="shift"))
    cases += [dict(form=f, M=1, N=1, K=1, knob=0) for f in FORMS]
    # every K of the pools in every form that takes it (the rotation above may pass one over)
    for f, (ta, _) in sorted(FORMS.items()):
        for j, K in enumerate(POOL_K_TN if ta else POOL_K):
            if not any(c["form"] == f and c["K"] == K for c in cases):
                cases.append(dict(form=f, M=(33, 130, 41)[j % 3], N=(41, 31, 129)[j % 3], K=K, knob=TN_KNOB if ta else 0,
                                  accumulate=j % 2 == 1))
    return cases


def case_cell(c):
    """the cell of a catalogue case (None in vec_*: an odd width on an ordinary buffer)"""
    return cell(dict(c, vec_a=c.get("vec_a") or "on", vec_b=c.get("vec_b") or "on"))


CASES = _cases()


# ---- references ----------------------------------------------------------------------------------------------------------
def int_range(K, keep=None):
    """the integer range of exact operands: [-8, 8], narrowed where K is long so that dense_cases.gemm_exact's
    precondition holds (K = 70,001 with keep 0.8: terms on the grid 2^-2, |sum| <= 16 * 1.25 * 70,001 < 2^22)"""
    return 8 if K <= 8192 else 4


def rounded_operands(A, B, mask_a=None, scale_a=1.0):
    """the operands as the kernel multiplies them: bf(fp32(a * mask * scale)) and bf(b), as fp64"""
    Af = np.asarray(A, np.float32)
    if mask_a is not None:
        Af = (Af * np.asarray(mask_a, np.float32) * np.float32(scale_a)).astype(np.float32)
    return bf16_ref.round_trip(Af).astype(np.float64), bf16_ref.round_trip(np.asarray(B, np.float32)).astype(np.float64)


def n_ops(K, accumulate=False, mask_c=False):
    """dense_cases.gemm_bound's n for the rounded operands: K products and K - 1 additions at most, the accumulate
    addition and the output mask's scale.  A mask on A adds nothing: the reference's rounded A already carries the mask
    and the fp32 scale, so no further rounding separates the result from the reference."""
    return K + 1 + int(bool(accumulate)) + int(bool(mask_c))


def reference(A, B, ta, tb, C_in=None, accumulate=False, mask_a=None, scale_a=1.0, mask_c=None, scale_c=1.0):
    """(ref, bound, unit): the fp64 product of the rounded operands, the per-element bound 2 gamma(n) mag + n TINY --
    dense_cases.gemm_bound on the rounded operands with its gamma term doubled -- and gamma(n) * mag, the unit the observed
    error is recorded in."""
    Ar, Br = rounded_operands(A, B, mask_a, scale_a)
    kw = dict(mask_c=mask_c, scale_c=scale_c) if mask_c is not None else {}
    ref = dc.gemm_f64(Ar, Br, ta, tb, C_in, accumulate, **kw)[0]
    K = Ar.shape[0] if ta else Ar.shape[1]
    n = n_ops(K, accumulate, mask_c is not None)
    unit = dc.gemm_bound(Ar, Br, ta, tb, C_in, accumulate, **kw) - n * dc.TINY
    return ref, 2.0 * unit + n * dc.TINY, unit
