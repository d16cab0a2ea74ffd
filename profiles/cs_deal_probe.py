#!/usr/bin/env python
"""What the column-aware dealing of the lane-group plans buys ("the dealing"; sgcn_csplan.cpp, sgcn_tune
"cs_deal"): the plans of S-Reddit built with cs_deal = 0 (rows dealt to bins by weight alone) and cs_deal = 1, side by side
in one process, on the bench's matrix and operands.  Everything is recorded, nothing is gated.

    python profiles/cs_deal_probe.py --cpu [--cs-g 2] [--threads 0] [--small]
        plan statistics only (no GPU): pad fraction, steps of the heaviest tile per launch round, how far the bins stray
        from the clock, real nonzeros of the heaviest bin, host seconds of the build (all threads and one thread: the
        dealing is the serial part, so the one-thread difference between the two knob values is the dealing by itself)
    python profiles/cs_deal_probe.py products [--repeats 4] [--iters 40] [--bf16]
        each plan autotuned for itself, then `repeats` windows of `iters` forward + backward pairs per plan, alternating
    python profiles/cs_deal_probe.py paces [--paces 186,188,...] [--repeats 2]
        both plans at the same forced clocks, alternating: where each loses the lock-step
    rocprofv3 --kernel-trace -f csv -d D -- python profiles/cs_deal_probe.py run --deal 0|1 --pace-fwd P --pace-bwd Q
        `iters` paced pairs on one plan, for a kernel trace (a run of its own per plan; counters likewise, never with a trace)
    python profiles/cs_deal_probe.py kernels --dir D
        the sweep and fix-up launches of such a trace

Records go to stdout as JSON lines (everything else to stderr)."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 602
PAD = 0x80000000


def _matrix(small=False):
    from stochastic_gcn_amd import synthetic
    if small:
        return synthetic.reddit_like(n=23296, m=1160000, splits=(15241, 2369, 5533), seed=1, with_features=False)[2].tocsr()
    return synthetic.reddit_like(with_features=False)[2].tocsr()


def _deal(v):
    from stochastic_gcn_amd._ffi import check, lib
    check(lib.sgcn_tune(b"cs_deal", int(v)))


def plan_stats(tile_ptr, colrow, val, G, rnd, K, nnz):
    """statistics of a lane-group plan's host arrays"""
    tp = np.asarray(tile_ptr, np.int64)
    nt = tp.shape[0] - 1
    steps = np.diff(tp) // G
    nl = -(-nt // rnd)
    padded = np.zeros(nl * rnd, np.int64)
    padded[:nt] = steps
    per_round = padded.reshape(nl, rnd)
    real = np.asarray(val).view(np.uint32) != PAD
    tile = np.repeat(np.arange(nt), np.diff(tp))
    e = np.arange(tp[-1]) - tp[tile]
    bin_id = tile * G + e % G
    # the clock sweeps [0, K) in as many steps as the round's heaviest tile has
    clock = (e // G) * (K / np.maximum(per_round.max(axis=1), 1)[tile // rnd])
    col = (np.asarray(colrow).view(np.uint32) & 0x0FFFFFFF).astype(np.float64)
    off = np.zeros(nt * G)
    np.maximum.at(off, bin_id[real], np.abs(col - clock)[real])
    live = np.bincount(bin_id[real], minlength=nt * G)
    return {"ntiles": int(nt), "rounds": int(nl), "pad_fraction": round(1.0 - nnz / max(int(tp[-1]), 1), 4),
            "heaviest_tile_steps_per_round": per_round.max(axis=1).tolist(),
            "mean_tile_steps": round(float(steps[steps > 0].mean()), 1), "ideal_steps": round(nnz / max(int((live > 0).sum()), 1), 1),
            "bin_off_clock_columns_mean_p90": [round(float(off[live > 0].mean())), round(float(np.percentile(off[live > 0], 90)))],
            "heaviest_bin_nnz": int(live.max()), "mean_bin_nnz": round(float(live[live > 0].mean()), 1)}


def cpu(args):
    from stochastic_gcn_amd import ops
    Cs = ops.ColumnSweepCSR
    a = _matrix(args.small)
    for name, m in (("A", a), ("A^T", ops.transpose_host(a))):
        m = m.tocsr()
        rowptr, col = np.ascontiguousarray(m.indptr, np.int32), np.ascontiguousarray(m.indices, np.int32)
        val = np.ascontiguousarray(m.data, np.float32)
        M, K = m.shape
        G = args.cs_g
        rnd = args.round or ops._cs_round(None)
        T = Cs.auto_t(rowptr, G, rnd)
        wtab, shift = Cs.make_warp(col, K, 'auto')
        align = args.align or Cs.auto_align(K, col.shape[0], M, G, rnd)
        for deal in [int(x) for x in args.deals.split(',')]:
            _deal(deal)
            secs = {}
            for label, threads in (("all_threads", args.threads), ("one_thread", 1)):
                t0 = time.perf_counter()
                built = Cs._build(rowptr, col, val, M, G, 16, T, rnd, int(align), None,
                                  wtab.ctypes.data if wtab is not None else None, shift, threads=threads)
                secs[label] = round(time.perf_counter() - t0, 3)
            rec = {"what": "plan", "matrix": name, "graph": "sreddit-small" if args.small else "sreddit", "cs_deal": deal, "G": G,
                   "round": rnd, "align": int(align), "T": int(T), "warp": wtab is not None, "build_s": secs}
            rec.update(plan_stats(built[0], built[1], built[2], G, rnd, K, m.nnz))
            print(json.dumps(rec), flush=True)
        if args.small or not args.transpose:
            break


def _setup(deals, bf16=False):
    """{deal: (A, AT)} on the GPU, X, dC (``bf16``: rounded to bfloat16 tables), outputs"""
    import torch
    from stochastic_gcn_amd import ops
    from profiles.spmm_b16_probe import _guard_off, _operands
    dev = torch.device("cuda:0")
    a = _matrix()
    n = a.shape[0]
    at = ops.transpose_host(a)
    G = ops.ColumnSweepCSR.choose_g(D, a.nnz / max(n, 1), n)
    plans, build_s = {}, {}
    for deal in deals:
        _deal(deal)
        t0 = time.perf_counter()
        plans[deal] = (ops.ColumnSweepCSR(a, dev, G=G), ops.ColumnSweepCSR(at, dev, G=G))
        build_s[deal] = round(time.perf_counter() - t0, 3)
        _guard_off(*plans[deal])
    X, dC = _operands(n, D, dev, bf16)
    out = torch.empty((n, (D + 3) // 4 * 4), device=dev)[:, :D]
    out_t = torch.empty((n, (D + 3) // 4 * 4), device=dev)[:, :D]
    return plans, build_s, X, dC, out, out_t, G


def _describe(A, AT):
    A.struct(D), AT.struct(D)                 # (makes the plans' per-launch hints)
    return {"kernel": A.variant(D), "pad_fraction": [round(float(A.pad_fraction), 4), round(float(AT.pad_fraction), 4)],
            "heaviest_tile_steps_per_launch": [A._hint.tolist(), AT._hint.tolist()], "nfix": [A.nfix, AT.nfix]}


def products(args):
    from stochastic_gcn_amd import ops
    from profiles.spmm_b16_probe import _sustained
    plans, build_s, X, dC, out, out_t, G = _setup((0, 1), args.bf16)

    def pair(deal):
        A, AT = plans[deal]
        return lambda: (ops.spmm_cs(A, X, out=out), ops.spmm_cs(AT, dC, out=out_t))

    tuned = {}
    for deal, (A, AT) in plans.items():          # each plan tuned for itself
        bf, bb = A.autotune(X), AT.autotune(dC)
        tuned[deal] = dict(fwd_ms=bf[0], fwd_pace=bf[1], bwd_ms=bb[0], bwd_pace=bb[1])
        for P in (A, AT):
            P._guard.clear()
    runs = {deal: [] for deal in plans}
    for _ in range(args.repeats):
        for deal in plans:                       # the plans alternate inside one process
            runs[deal].append(_sustained(pair(deal), args.iters))
    for deal, (A, AT) in plans.items():
        ms = runs[deal]
        rec = {"what": "products", "cs_deal": deal, "operand": "bf16" if args.bf16 else "fp32", "graph": "sreddit", "d": D, "G": G, "tuned": tuned[deal], "iters": args.iters,
               "repeats": args.repeats, "pair_ms": ms, "pair_ms_mean": sum(ms) / len(ms), "pair_ms_min": min(ms),
               "pair_ms_max": max(ms), "plans_build_and_upload_s": build_s[deal]}
        rec.update(_describe(A, AT))
        print(json.dumps(rec), flush=True)
    o, t = runs[0], runs[1]
    width = max(o) - min(o)
    print(json.dumps({"what": "products verdict", "deal1_minus_deal0_ms": sum(t) / len(t) - sum(o) / len(o),
                      "deal0_min_max": [min(o), max(o)], "deal1_min_max": [min(t), max(t)],
                      "gap_over_deal0_range_width": (min(o) - max(t)) / width if width > 0 else None,
                      "note": "recorded, not a gate"}), flush=True)


def paces(args):
    from stochastic_gcn_amd import ops
    from profiles.spmm_b16_probe import _sustained
    plans, _, X, dC, out, out_t, G = _setup((0, 1))
    for p in [int(x) for x in args.paces.split(",")]:
        ms = {}
        for deal, (A, AT) in plans.items():
            A.pace[D] = AT.pace[D] = p
            ms[deal] = []
        for _ in range(args.repeats):
            for deal, (A, AT) in plans.items():
                ms[deal].append(_sustained(lambda: (ops.spmm_cs(A, X, out=out), ops.spmm_cs(AT, dC, out=out_t)), args.iters))
        print(json.dumps({"what": "paces", "pace": p, "G": G, "iters": args.iters, "pair_ms_by_cs_deal": ms}), flush=True)


def run(args):
    import torch
    from stochastic_gcn_amd import ops
    plans, _, X, dC, out, out_t, G = _setup((args.deal,))
    A, AT = plans[args.deal]
    A.pace[D], AT.pace[D] = args.pace_fwd, args.pace_bwd
    for _ in range(args.iters):
        ops.spmm_cs(A, X, out=out)
        ops.spmm_cs(AT, dC, out=out_t)
    torch.cuda.synchronize()
    rec = {"what": "run", "cs_deal": args.deal, "iters": args.iters, "G": G, "pace_fwd": args.pace_fwd, "pace_bwd": args.pace_bwd}
    rec.update(_describe(A, AT))
    print(json.dumps(rec), flush=True)


def kernels(args):
    f = glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True)
    rows = list(csv.DictReader(open(f[0])))
    for tag, key in (("sweep", "cs_spmm16"), ("fixup", "cs_fix_kernel")):
        us = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if key in r["Kernel_Name"])
        if us:
            print(json.dumps({"what": "kernel", "dir": args.dir, "kernel": tag, "launches": len(us), "avg_us": sum(us) / len(us),
                              "median_us": us[len(us) // 2], "min_us": us[0], "max_us": us[-1]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default=None, choices=["products", "paces", "run", "kernels"])
    ap.add_argument("--cpu", action="store_true", help="plan statistics only (no GPU)")
    ap.add_argument("--small", action="store_true", help="--cpu: the tests' small S-Reddit (round 256, align 224)")
    ap.add_argument("--transpose", action="store_true", help="--cpu: the transposed matrix too")
    ap.add_argument("--cs-g", type=int, default=2, choices=[2, 4])
    ap.add_argument("--round", type=int, default=0)
    ap.add_argument("--align", type=int, default=0)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--deal", type=int, default=1)
    ap.add_argument("--deals", default="0,1", help="--cpu: the knob values to build with")
    ap.add_argument("--bf16", action="store_true", help="products: bfloat16 operands (the plans' bfloat16 clocks)")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--pace-fwd", type=int, default=-1)
    ap.add_argument("--pace-bwd", type=int, default=-1)
    ap.add_argument("--paces", default="186,188,190,192,194,196,198,202")
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    if args.cpu:
        return cpu(args)
    if args.what is None:
        ap.error("one of --cpu, products, paces, run, kernels")
    {"products": products, "paces": paces, "run": run, "kernels": kernels}[args.what](args)


if __name__ == "__main__":
    main()
