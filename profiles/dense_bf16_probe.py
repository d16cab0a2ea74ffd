#!/usr/bin/env python
"""Measurements of the bf16-multiply dense layers of the full-graph modes (--dense_dtype bf16; DESIGN.md 3.5 / 3.7;
include/sgcn.h sgcn_gemm_mb16_f32).  Everything is recorded, nothing is gated.  One box, one session: the two multiply
types alternate inside one process, every shape is warmed first, times are device events.

    python profiles/dense_bf16_probe.py gemms [--repeats 4] [--iters 20]
        the three forms (NN forward, NT input gradient, TN weight gradient) at the layer shapes of the S-Reddit recipe
        (N = 232,965 rows; 1,204 -> 128, 256 -> 128, 128 -> 128, 128 -> 41): sgcn_gemm_f32 against sgcn_gemm_mb16_f32, and
        beside each the floor max(bytes / 6.3 TB/s, flops / 2.5 PF) computed from the shape, with the term that binds
    python profiles/dense_bf16_probe.py epochs --dense_dtype fp32|bf16|both [--epochs 8] [--rounds 2]
        the full-batch epoch of DESIGN.md 3.7's recipe.  `--dense_dtype fp32` touches nothing this change added, so the same
        file times the parent commit from its own checkout (--tag parent); the rounds give the run-to-run spread
    rocprofv3 --kernel-trace --stats -d D -- python profiles/dense_bf16_probe.py run --dense_dtype bf16 --epochs 5
    python profiles/dense_bf16_probe.py kernels --dir D
        the kernel table of such a trace: what ln_act_fwd, ln_act_bwd and the LayerNorm-parameter reduction cost at 233 k rows
    python profiles/dense_bf16_probe.py convergence [--seeds 1,2,3,4,5] [--epochs 30]
        --full_batch --test_full_batch per seed with fp32 and bf16 dense layers: test accuracy and the per-seed difference
        beside the seed-to-seed spread; no threshold

Records go to stdout as JSON lines (everything else to stderr)."""
import argparse
import contextlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RECIPE = ['--dataset', 's-reddit', '--normalization', 'graphsage', '--weight_decay', '0', '--dropout', '0.2', '--layer_norm',
          '--hidden1', '128', '--num_fc_layers', '2']
N_ROWS = 232965
LAYERS = ((1204, 128), (256, 128), (128, 128), (128, 41))      # (fan-in, fan-out) of the recipe's dense layers
HBM_BPS, BF16_FLOPS = 6.3e12, 2.5e15


def _sustained(fn, iters, warm=3):
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


def _floor(M, N, K, ws_floats):
    """(ms, binding term) of max(bytes / HBM, flops / bf16 peak): A, B read once, C written once, the split-K workspace
    written and read once"""
    byts = 4.0 * (M * K + K * N + M * N + 2 * ws_floats)
    flops = 2.0 * M * N * K
    tb, tf = byts / HBM_BPS, flops / BF16_FLOPS
    return max(tb, tf) * 1e3, ("bytes" if tb >= tf else "flops"), byts, flops


def gemms(args):
    import torch
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd._ffi import lib
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    n = args.rows
    for fin, fout in LAYERS:
        x = torch.randn((n, fin), device=dev, generator=g)
        W = torch.randn((fin, fout), device=dev, generator=g) / fin ** 0.5
        gr = torch.randn((n, fout), device=dev, generator=g)
        forms = (("NN", (n, fout, fin), lambda f, o: f(x, W, out=o), (n, fout)),
                 ("NT", (n, fin, fout), lambda f, o: f(gr, W, out=o, trans_b=True), (n, fin)),
                 ("TN", (fin, fout, n), lambda f, o: f(x, gr, out=o, trans_a=True, accumulate=True), (fin, fout)))
        for form, (M, N, K), call, oshape in forms:
            out = torch.zeros(oshape, device=dev)
            runs = {"fp32": [], "bf16": []}
            for _ in range(args.repeats):
                for t, f in (("fp32", ops.gemm), ("bf16", ops.gemm_bf16)):       # the types alternate inside one process
                    runs[t].append(_sustained(lambda: call(f, out), args.iters))
            ta, tb = form == "TN", form == "NT"
            ws = int(lib.sgcn_gemm_mb16_ws_floats(int(ta), int(tb), M, N, K))
            floor_ms, binds, byts, flops = _floor(M, N, K, ws)
            mf, mb = min(runs["fp32"]), min(runs["bf16"])
            print(json.dumps({"what": "gemm", "form": form, "layer": [fin, fout], "M": M, "N": N, "K": K,
                              "fp32_ms": runs["fp32"], "bf16_ms": runs["bf16"], "fp32_ms_best": mf, "bf16_ms_best": mb,
                              "bf16_over_fp32": mb / mf, "bf16_faster": bool(max(runs["bf16"]) < min(runs["fp32"])),
                              "floor_ms": floor_ms, "floor_binds": binds, "bytes": byts, "flops": flops,
                              "bf16_over_floor": mb / floor_ms, "splitk_ws_floats": ws,
                              "iters": args.iters, "repeats": args.repeats}), flush=True)
        del x, gr
        torch.cuda.empty_cache()


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


def _dense_flag(t):
    """(a checkout without the flag -- the parent commit -- is timed with `--dense_dtype fp32`: nothing is passed)"""
    return ['--dense_dtype', t] if t != "fp32" else []


def epochs(args):
    import torch
    data = _data()
    types_ = ["fp32", "bf16"] if args.dense_dtype == "both" else [args.dense_dtype]
    for rnd in range(args.rounds):
        for t in types_:
            trn = _trainer(RECIPE + ['--full_batch', '--full_batch_kernel', 'cs', '--epochs', str(args.epochs)] + _dense_flag(t),
                           data)
            times, dev_times = [], []
            for _ in range(args.epochs + 1):
                t0 = time.time()
                trn.train_epoch()
                times.append(time.time() - t0)
                dev_times.append(trn.train_model.run_t)
                trn.train_model.run_t = 0.0
            m = trn.train_static.matrix
            print(json.dumps({"what": "full_batch epochs", "tag": args.tag, "round": rnd, "dense_dtype": t, "kernel": m.kernel,
                              "N": m.shape[0], "nnz": m.nnz, "first_epoch_s": times[0], "epoch_times_s": times[1:],
                              "epoch_time_s": min(times[1:]), "device_epoch_s": dev_times[1:],
                              "device_epoch_ms_best": min(dev_times[1:]) * 1e3,
                              "train_loss_last": trn.avg_loss.mean()}), flush=True)
            del trn
            torch.cuda.empty_cache()


def run(args):
    """only the epochs (for a profiler around this process)"""
    import torch
    trn = _trainer(RECIPE + ['--full_batch', '--full_batch_kernel', 'cs', '--epochs', str(args.epochs)]
                   + _dense_flag(args.dense_dtype), _data())
    for _ in range(args.epochs):
        trn.train_epoch()
    torch.cuda.synchronize()
    print(json.dumps({"what": "run", "dense_dtype": args.dense_dtype, "epochs": args.epochs}), flush=True)


def kernels(args):
    """the kernel table of a rocprofv3 --kernel-trace --stats run"""
    import glob
    import sqlite3
    # (rocprofv3's default output format: <dir>/<host>/<pid>_results.db with the `top_kernels` view that --stats adds, as
    # full_batch_probe.py summary reads it)
    f = glob.glob(os.path.join(args.dir, "**", "*results.db"), recursive=True)
    if not f:
        sys.exit("no *results.db under %s: run rocprofv3 --kernel-trace --stats -d %s first (default rocpd output)" % (args.dir, args.dir))
    t = sqlite3.connect(f[0])
    for name, calls, total, avg, pct in t.execute("select name,total_calls,total_duration,average,percentage from top_kernels"):
        print(json.dumps({"what": "kernel", "name": name[:160], "calls": calls, "total_ms": total / 1e3, "avg_us": avg,
                          "pct": pct}), flush=True)


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
            trn = _trainer(base + _dense_flag(t) + ['--seed', str(seed)], data)
            with contextlib.redirect_stdout(sys.stderr):
                trn.SGDTrain()
            res = trn.evaluate(trn.test_d)
            acc[t][seed] = res[1]
            print(json.dumps({"what": "convergence", "seed": seed, "dense_dtype": t, "epochs": args.epochs, "test_loss": res[0],
                              "test_acc": res[1], "micro_f1": res[2], "macro_f1": res[3], "n_test": int(len(trn.test_d)),
                              "wall_s": round(time.time() - t0, 1)}), flush=True)
            del trn
            torch.cuda.empty_cache()
    f = [acc["fp32"][s] for s in seeds]
    for s in seeds:
        print(json.dumps({"what": "convergence difference", "seed": s, "test_acc_bf16_minus_fp32": acc["bf16"][s] - acc["fp32"][s],
                          "fp32_seed_spread": max(f) - min(f), "note": "recorded, no threshold"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["gemms", "epochs", "run", "kernels", "convergence"])
    ap.add_argument("--dense_dtype", default="both", choices=["fp32", "bf16", "both"])
    ap.add_argument("--rows", type=int, default=N_ROWS)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--tag", default="this")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--seeds", default="1,2,3,4,5")
    args = ap.parse_args()
    if args.epochs is None:
        args.epochs = 30 if args.what == "convergence" else 8
    if args.what == "run" and args.dense_dtype == "both":
        args.dense_dtype = "bf16"
    {"gemms": gemms, "epochs": epochs, "run": run, "kernels": kernels, "convergence": convergence}[args.what](args)


if __name__ == "__main__":
    main()
