#!/usr/bin/env python
"""Measurements of the bfloat16 dense operand of the static-graph products (include/sgcn.h "bfloat16 dense
operand").  Everything is recorded, nothing is gated.

    python profiles/spmm_b16_probe.py products --graph sreddit|rmat10m --dtype fp32|bf16|both [--repeats 4] [--iters 40]
        forward (A . X) and backward (A^T . dC) on separately built, separately autotuned column-sweep plans -- each
        operand type tuned for itself -- as SUSTAINED runs: `iters` back-to-back fwd + bwd pairs between two device events,
        `repeats` times, the types alternating.  sreddit: S-Reddit, d = 602.  rmat10m: block 3 of 8 of S-RMAT 10 M, d = 256.
        `--dtype fp32` touches nothing this change added, so the same file times the parent commit (the yardstick and its
        spread); bf16 is reported as a ratio to the fp32 mean beside that spread.
    rocprofv3 --pmc <counters> -d D -- python profiles/spmm_b16_probe.py run --graph sreddit --dtype bf16 --iters 5
        a counter pass of its own per type (no tracing with it): `run` only multiplies, at the pace recorded by `products`
        (--pace-fwd / --pace-bwd)
    rocprofv3 --kernel-trace --stats -d D -- python profiles/spmm_b16_probe.py run --graph sreddit --dtype bf16 --iters 20
    python profiles/spmm_b16_probe.py kernels --dir D
        the kernel durations of such a trace (the sweep kernels, the fix-up, the rounding pass)
    python profiles/spmm_b16_probe.py epochs --dtype fp32|bf16 [--epochs 8]
        the S-Reddit README recipe without --cv under --full_batch --full_batch_kernel cs: epoch times; with bf16 the rounding
        pass (sgcn_scatter_rows_h16's kernel) is part of the epoch and is timed by itself as well
    python profiles/spmm_b16_probe.py convergence [--seeds 1,2,3,4,5] [--epochs 30]
        --full_batch --test_full_batch per seed in fp32 and bf16: test accuracy, bf16 - fp32 against max(S, 2 se)

Records go to stdout as JSON lines (everything else to stderr)."""
import argparse
import contextlib
import json
import math
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RECIPE = ['--dataset', 's-reddit', '--normalization', 'graphsage', '--weight_decay', '0', '--dropout', '0.2', '--layer_norm',
          '--hidden1', '128', '--num_fc_layers', '2']


def _graph(name):
    """(A, A^T, K, d) as SciPy CSR: the matrices whose products are timed"""
    from stochastic_gcn_amd import ops, synthetic
    if name == "sreddit":
        n, _, full_adj, *_ = synthetic.reddit_like(with_features=False)
        return full_adj.tocsr(), ops.transpose_host(full_adj), n, 602
    from stochastic_gcn_amd.parallel import ShardedSpMM
    n = 10_000_000
    adj = synthetic.cached_graph("rmat_10m_200m_seed1", lambda: synthetic.rmat_like(n, 200_000_000, seed=1))
    sh = ShardedSpMM(types.SimpleNamespace(rank=3, world=8, active=False), adj, None, kernel=None)
    adj_t = ops.transpose_host(adj)
    blk, blk_t = adj[sh.lo:sh.hi].tocsr(), adj_t[sh.lo:sh.hi].tocsr()
    del adj, adj_t
    return blk, blk_t, n, 256


def _plans(a, at, d, dev):
    from stochastic_gcn_amd import ops
    G = ops.ColumnSweepCSR.choose_g(d, a.nnz / max(a.shape[0], 1), a.shape[0])
    return ops.ColumnSweepCSR(a, dev, G=G), ops.ColumnSweepCSR(at, dev, G=G), G


def _guard_off(*plans):
    """the lost-lock guard off for these plans (a checkout without the switch -- the yardstick -- has only the autotuner's flag)"""
    for P in plans:
        if hasattr(type(P), "guard_on"):
            P.guard_on = False
        else:
            P._tuning = True


def _operands(K, d, dev, bf16):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    pitch = (d + 7) // 8 * 8
    X = torch.zeros((K, pitch), device=dev)
    X[:, :d] = torch.randn((K, d), device=dev, generator=g)
    dC = torch.zeros((K, pitch), device=dev)
    dC[:, :d] = torch.randn((K, d), device=dev, generator=g)
    X, dC = X[:, :d], dC[:, :d]
    if bf16:
        from stochastic_gcn_amd import ops
        return ops.operand_round(X), ops.operand_round(dC)
    return X, dC


def _sustained(fn, iters, warm=4):
    import torch
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def products(args):
    import torch
    from stochastic_gcn_amd import ops
    dev = torch.device("cuda:0")
    a, at, K, d = _graph(args.graph)
    types_ = ["fp32", "bf16"] if args.dtype == "both" else [args.dtype]
    A, AT, G = _plans(a, at, d, dev)
    M = a.shape[0]
    out = torch.empty((M, (d + 3) // 4 * 4), device=dev)[:, :d]
    out_t = torch.empty((at.shape[0], (d + 3) // 4 * 4), device=dev)[:, :d]
    ops_, tuned = {}, {}
    for t in types_:
        X, dC = _operands(K, d, dev, t == "bf16")
        t0 = time.time()
        bf, bb = A.autotune(X), AT.autotune(dC)
        tuned[t] = dict(fwd_ms=bf[0], fwd_pace=bf[1], bwd_ms=bb[0], bwd_pace=bb[1], autotune_s=time.time() - t0)
        ops_[t] = (X, dC)
    _guard_off(A, AT)                        # (no guard samples, no re-tunes inside the timed windows)
    runs = {t: dict(fwd=[], bwd=[], pair=[]) for t in types_}
    for _ in range(args.repeats):
        for t in types_:                     # the types alternate inside one process
            X, dC = ops_[t]
            runs[t]["fwd"].append(_sustained(lambda: ops.spmm_cs(A, X, out=out), args.iters))
            runs[t]["bwd"].append(_sustained(lambda: ops.spmm_cs(AT, dC, out=out_t), args.iters))
            runs[t]["pair"].append(_sustained(lambda: (ops.spmm_cs(A, X, out=out), ops.spmm_cs(AT, dC, out=out_t)), args.iters))
    for t in types_:
        bf16 = t == "bf16"
        pair = runs[t]["pair"]
        rec = {"what": "products", "graph": args.graph, "dtype": t, "d": d, "G": G, "M": M, "K": K, "nnz": int(a.nnz),
               "nnz_t": int(at.nnz), "operand_bytes_per_nonzero": d * (2 if bf16 else 4), "iters": args.iters,
               "repeats": args.repeats, "tuned": tuned[t],
               "kernel": A.variant(d, bf16) if bf16 else A.variant(d),
               "fwd_ms": runs[t]["fwd"], "bwd_ms": runs[t]["bwd"], "pair_ms": pair,
               "pair_ms_mean": sum(pair) / len(pair), "pair_ms_spread": max(pair) - min(pair)}
        print(json.dumps(rec), flush=True)
    if len(types_) == 2:
        f, b = runs["fp32"]["pair"], runs["bf16"]["pair"]
        mf, mb = sum(f) / len(f), sum(b) / len(b)
        print(json.dumps({"what": "products ratio", "graph": args.graph, "bf16_over_fp32": mb / mf,
                          "fp32_relative_spread": (max(f) - min(f)) / mf, "bf16_relative_spread": (max(b) - min(b)) / mb,
                          "bf16_faster_beyond_fp32_spread": bool(mb < min(f))}), flush=True)


def run(args):
    """only the products (for a profiler around this process): `iters` fwd + bwd pairs of one operand type"""
    import torch
    from stochastic_gcn_amd import ops
    dev = torch.device("cuda:0")
    a, at, K, d = _graph(args.graph)
    bf16 = args.dtype == "bf16"
    A, AT, _ = _plans(a, at, d, dev)
    X, dC = _operands(K, d, dev, bf16)
    for P, pace in ((A, args.pace_fwd), (AT, args.pace_bwd)):
        (P.pace_b16 if bf16 else P.pace)[d] = pace
    _guard_off(A, AT)
    for _ in range(args.iters):
        ops.spmm_cs(A, X)
        ops.spmm_cs(AT, dC)
    torch.cuda.synchronize()
    print(json.dumps({"what": "run", "graph": args.graph, "dtype": args.dtype, "iters": args.iters,
                      "pace_fwd": args.pace_fwd, "pace_bwd": args.pace_bwd}), flush=True)


def kernels(args):
    """the kernel table of a rocprofv3 --kernel-trace --stats run"""
    import glob
    import sqlite3
    f = glob.glob(os.path.join(args.dir, "**", "*results.db"), recursive=True)
    t = sqlite3.connect(f[0])
    for name, calls, total, avg, pct in t.execute("select name,total_calls,total_duration,average,percentage from top_kernels"):
        print(json.dumps({"what": "kernel", "dir": args.dir, "name": name[:160], "calls": calls, "total_ms": total / 1e3,
                          "avg_us": avg, "pct": pct}), flush=True)


def _trainer(argv, data=None):
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.train import Trainer
    FLAGS.reset()
    FLAGS.parse(argv)
    with contextlib.redirect_stdout(sys.stderr):
        return Trainer(data=data, verbose=False)


def _data():
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.utils import load_data
    FLAGS.reset()
    FLAGS.parse(RECIPE)
    with contextlib.redirect_stdout(sys.stderr):
        return load_data(FLAGS.dataset)


def epochs(args):
    import torch
    from stochastic_gcn_amd import ops
    dev = torch.device("cuda:0")
    data = _data()
    for t in (["fp32", "bf16"] if args.dtype == "both" else [args.dtype]):
        trn = _trainer(RECIPE + ['--full_batch', '--full_batch_kernel', 'cs', '--full_batch_dtype', t,
                                 '--epochs', str(args.epochs)], data)
        times, dev_times = [], []
        for _ in range(args.epochs + 1):
            t0 = time.time()
            trn.train_epoch()
            times.append(time.time() - t0)
            dev_times.append(trn.train_model.run_t)
            trn.train_model.run_t = 0.0
        m = trn.train_static.matrix
        rec = {"what": "full_batch epochs", "dtype": t, "kernel": m.kernel, "N": m.shape[0], "nnz": m.nnz,
               "first_epoch_s": times[0], "epoch_times_s": times[1:], "epoch_time_s": min(times[1:]),
               "device_epoch_s": dev_times[1:], "train_loss_last": trn.avg_loss.mean(),
               "pace": dict(m._plan.pace_b16 if t == "bf16" else m._plan.pace),
               "pace_transpose": dict(m.transpose._plan.pace_b16 if t == "bf16" else m.transpose._plan.pace)}
        if t == "bf16":                      # the rounding pass by itself, per scratch table of the step
            rec["rounding_us"] = {}
            for mat, tag in ((m, "fwd"), (m.transpose, "bwd")):
                for d, tab in mat._scratch.items():
                    x = torch.randn((tab.shape[0], d), device=dev)
                    rec["rounding_us"]["%s d=%d" % (tag, d)] = _sustained(lambda: ops.operand_round(x, out=tab), 50) * 1e3
        print(json.dumps(rec), flush=True)
        del trn
        torch.cuda.empty_cache()


def convergence(args):
    import torch
    seeds = [int(s) for s in args.seeds.split(",")]
    base = RECIPE + ['--full_batch', '--test_full_batch', '--full_batch_kernel', 'cs', '--epochs', str(args.epochs),
                     '--early_stopping', str(args.epochs)]
    data = _data()
    acc = {"fp32": {}, "bf16": {}}
    for seed in seeds:
        for t in ("fp32", "bf16"):
            t0 = time.time()
            trn = _trainer(base + ['--full_batch_dtype', t, '--seed', str(seed)], data)
            with contextlib.redirect_stdout(sys.stderr):
                trn.SGDTrain()
            res = trn.evaluate(trn.test_d)
            acc[t][seed] = res[1]
            print(json.dumps({"what": "convergence", "seed": seed, "dtype": t, "epochs": args.epochs, "test_loss": res[0],
                              "test_acc": res[1], "micro_f1": res[2], "macro_f1": res[3], "n_test": int(len(trn.test_d)),
                              "wall_s": round(time.time() - t0, 1)}), flush=True)
            n_test = int(len(trn.test_d))
            del trn
            torch.cuda.empty_cache()
    f = [acc["fp32"][s] for s in seeds]
    S = max(f) - min(f)
    p = sum(f) / len(f)
    se2 = 2 * math.sqrt(p * (1 - p) / n_test)
    for s in seeds:
        diff = acc["bf16"][s] - acc["fp32"][s]
        print(json.dumps({"what": "convergence verdict", "seed": s, "test_acc_bf16_minus_fp32": diff, "fp32_seed_spread_S": S,
                          "two_standard_errors": se2, "bound": max(S, se2), "within": abs(diff) <= max(S, se2),
                          "note": "recorded, not a gate"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["products", "run", "kernels", "epochs", "convergence"])
    ap.add_argument("--graph", default="sreddit", choices=["sreddit", "rmat10m"])
    ap.add_argument("--dtype", default="both", choices=["fp32", "bf16", "both"])
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--pace-fwd", type=int, default=-1)
    ap.add_argument("--pace-bwd", type=int, default=-1)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--seeds", default="1,2,3,4,5")
    args = ap.parse_args()
    if args.epochs is None:
        args.epochs = 30 if args.what == "convergence" else 8
    {"products": products, "run": run, "kernels": kernels, "epochs": epochs, "convergence": convergence}[args.what](args)


if __name__ == "__main__":
    main()
