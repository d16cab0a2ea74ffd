#!/usr/bin/env python
"""What the dictionary plans of the two-group column sweep buy ("the value tables"; sgcn_csplan.cpp
sgcn_csbuild_dict, sgcn_tune "cs_dict"): the plans of S-Reddit built with cs_dict = 0 (a value per entry) and cs_dict = 1 (a
table of distinct values per tile, its index in the column word), side by side in one process, on the bench's matrix and
operands.  Everything is recorded, nothing is gated.

    python profiles/cs_dict_probe.py --cpu [--small]
        plan statistics only (no GPU): distinct values per tile, bytes of the value stream and of the tables per launch
        round, host seconds of the build with and without the dictionary pass
    python profiles/cs_dict_probe.py products [--repeats 4] [--iters 40] [--bf16]
        each plan autotuned for itself, then `repeats` windows of `iters` forward + backward pairs per plan, alternating
    python profiles/cs_dict_probe.py paces [--paces 186,190,...] [--repeats 2]
        both plans at the same forced clocks, alternating: where each loses the lock-step
    rocprofv3 --kernel-trace -f csv -d D -- python profiles/cs_dict_probe.py run --dict 0|1 --pace-fwd P --pace-bwd Q
        `iters` paced pairs on one plan, for a kernel trace (a run of its own per plan; counters likewise, never with a trace)
    python profiles/cs_dict_probe.py kernels --dir D
        the sweep and fix-up launches of such a trace

Records go to stdout as JSON lines (everything else to stderr)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from profiles.cs_deal_probe import D, _matrix, kernels      # noqa: E402


def _dict(v):
    from stochastic_gcn_amd._ffi import check, lib
    check(lib.sgcn_tune(b"cs_dict", int(v)))


def cpu(args):
    from stochastic_gcn_amd import ops
    Cs = ops.ColumnSweepCSR
    a = _matrix(args.small)
    for name, m in (("A", a), ("A^T", ops.transpose_host(a))):
        m = m.tocsr()
        rowptr, col = np.ascontiguousarray(m.indptr, np.int32), np.ascontiguousarray(m.indices, np.int32)
        val = np.ascontiguousarray(m.data, np.float32)
        M, K = m.shape
        rnd = ops._cs_round(None)
        T = Cs.auto_t(rowptr, 2, rnd)
        wtab, shift = Cs.make_warp(col, K, 'auto')
        align = Cs.auto_align(K, col.shape[0], M, 2, rnd)
        for knob in (0, 1):
            _dict(knob)
            t0 = time.perf_counter()
            built, (bits, tv, tn) = Cs._build(rowptr, col, val, M, 2, 16, T, rnd, int(align), None,
                                              wtab.ctypes.data if wtab is not None else None, shift, K=K)
            rec = {"what": "plan", "matrix": name, "graph": "sreddit-small" if args.small else "sreddit", "cs_dict": knob,
                   "build_and_export_s": round(time.perf_counter() - t0, 3), "dict_bits": bits, "ntiles": int(built[6]),
                   "entries": int(built[1].shape[0]), "overall_distinct_values": int(np.unique(val.view(np.uint32)).size)}
            nl = -(-rec["ntiles"] // rnd)
            rec["colrow_MB_per_launch_round"] = round(4e-6 * rec["entries"] / nl, 2)
            rec["val_MB_per_launch_round"] = 0.0 if bits else rec["colrow_MB_per_launch_round"]
            if bits:
                live = tn[tn > 0]
                rec["distinct_per_tile_mean_p99_max"] = [round(float(live.mean()), 1), int(np.percentile(live, 99)), int(live.max())]
                rec["tables_MB_per_launch_round"] = round(4e-6 * float(((tn + 3) // 4 * 4).sum()) / nl, 2)
                rec["tables_MB_uploaded"] = round(4e-6 * tv.shape[0], 2)
            print(json.dumps(rec), flush=True)


def _setup(knobs, bf16=False):
    """{knob: (A, AT)} on the GPU, X, dC (``bf16``: rounded to bfloat16 tables), outputs"""
    import torch
    from stochastic_gcn_amd import ops
    from profiles.spmm_b16_probe import _guard_off, _operands
    dev = torch.device("cuda:0")
    a = _matrix()
    n = a.shape[0]
    at = ops.transpose_host(a)
    G = ops.ColumnSweepCSR.choose_g(D, a.nnz / max(n, 1), n)
    plans, setup = {}, {}
    for knob in knobs:
        _dict(knob)
        plans[knob] = (ops.ColumnSweepCSR(a, dev, G=G), ops.ColumnSweepCSR(at, dev, G=G))
        setup[knob] = [p.setup_s for p in plans[knob]]
        _guard_off(*plans[knob])
    X, dC = _operands(n, D, dev, bf16)
    out = torch.empty((n, (D + 3) // 4 * 4), device=dev)[:, :D]
    out_t = torch.empty((n, (D + 3) // 4 * 4), device=dev)[:, :D]
    return plans, setup, X, dC, out, out_t, G


def _describe(A, AT):
    A.struct(D), AT.struct(D)                 # (makes the plans' per-launch hints)
    return {"kernel": [A.variant(D), AT.variant(D)], "dict_bits": [A.dict_bits, AT.dict_bits],
            "distinct_per_tile_mean_max": [None if P.dict_bits == 0 else [round(float(P.tile_nvals.float().mean()), 1), int(P.tile_nvals.max())]
                                           for P in (A, AT)]}


def products(args):
    import torch
    from stochastic_gcn_amd import ops
    from profiles.spmm_b16_probe import _sustained
    plans, setup, X, dC, out, out_t, G = _setup((0, 1), args.bf16)

    def pair(knob):
        A, AT = plans[knob]
        return lambda: (ops.spmm_cs(A, X, out=out), ops.spmm_cs(AT, dC, out=out_t))

    tuned, bits_of = {}, {}
    for knob, (A, AT) in plans.items():          # each plan tuned for itself
        bf, bb = A.autotune(X), AT.autotune(dC)
        tuned[knob] = dict(fwd_ms=bf[0], fwd_pace=bf[1], bwd_ms=bb[0], bwd_pace=bb[1])
        for P in (A, AT):
            P._guard.clear()
        pair(knob)()
        torch.cuda.synchronize()
        bits_of[knob] = (out.clone(), out_t.clone())
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(bits_of[0], bits_of[1]))
    runs = {knob: [] for knob in plans}
    for _ in range(args.repeats):
        for knob in plans:                       # the plans alternate inside one process
            runs[knob].append(_sustained(pair(knob), args.iters))
    for knob, (A, AT) in plans.items():
        ms = runs[knob]
        rec = {"what": "products", "cs_dict": knob, "operand": "bf16" if args.bf16 else "fp32", "graph": "sreddit", "d": D, "G": G,
               "tuned": tuned[knob], "iters": args.iters, "repeats": args.repeats, "pair_ms": ms, "pair_ms_mean": sum(ms) / len(ms),
               "pair_ms_min": min(ms), "pair_ms_max": max(ms), "setup_fwd_bwd": setup[knob]}
        rec.update(_describe(A, AT))
        print(json.dumps(rec), flush=True)
    o, t = runs[0], runs[1]
    width = max(o) - min(o)
    print(json.dumps({"what": "products verdict", "dict1_minus_dict0_ms": sum(t) / len(t) - sum(o) / len(o),
                      "dict0_min_max": [min(o), max(o)], "dict1_min_max": [min(t), max(t)],
                      "gap_over_dict0_range_width": (min(o) - max(t)) / width if width > 0 else None,
                      "outputs_bit_identical": bool(same), "note": "recorded, not a gate"}), flush=True)


def paces(args):
    from stochastic_gcn_amd import ops
    from profiles.spmm_b16_probe import _sustained
    plans, _, X, dC, out, out_t, G = _setup((0, 1))
    for p in [int(x) for x in args.paces.split(",")]:
        ms = {}
        for knob, (A, AT) in plans.items():
            A.pace[D] = AT.pace[D] = p
            ms[knob] = []
        for _ in range(args.repeats):
            for knob, (A, AT) in plans.items():
                ms[knob].append(_sustained(lambda: (ops.spmm_cs(A, X, out=out), ops.spmm_cs(AT, dC, out=out_t)), args.iters))
        print(json.dumps({"what": "paces", "pace": p, "G": G, "iters": args.iters, "pair_ms_by_cs_dict": ms}), flush=True)


def run(args):
    import torch
    from stochastic_gcn_amd import ops
    plans, _, X, dC, out, out_t, G = _setup((args.dict,))
    A, AT = plans[args.dict]
    A.pace[D], AT.pace[D] = args.pace_fwd, args.pace_bwd
    for _ in range(args.iters):
        ops.spmm_cs(A, X, out=out)
        ops.spmm_cs(AT, dC, out=out_t)
    torch.cuda.synchronize()
    rec = {"what": "run", "cs_dict": args.dict, "iters": args.iters, "G": G, "pace_fwd": args.pace_fwd, "pace_bwd": args.pace_bwd}
    rec.update(_describe(A, AT))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default=None, choices=["products", "paces", "run", "kernels"])
    ap.add_argument("--cpu", action="store_true", help="plan statistics only (no GPU)")
    ap.add_argument("--small", action="store_true", help="--cpu: the tests' small S-Reddit")
    ap.add_argument("--dict", type=int, default=1)
    ap.add_argument("--bf16", action="store_true", help="products: bfloat16 operands (the plans' bfloat16 clocks)")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--pace-fwd", type=int, default=-1)
    ap.add_argument("--pace-bwd", type=int, default=-1)
    ap.add_argument("--paces", default="186,190,194,198,202,206")
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    if args.cpu:
        return cpu(args)
    if args.what is None:
        ap.error("one of --cpu, products, paces, run, kernels")
    {"products": products, "paces": paces, "run": run, "kernels": kernels}[args.what](args)


if __name__ == "__main__":
    main()
