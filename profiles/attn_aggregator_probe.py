#!/usr/bin/env python
"""Measurements of --aggregator attn on S-Reddit.

    python profiles/attn_aggregator_probe.py kernels [--d 128] [--rounds 7] [--reps 10]
        attention's forward and its two-launch backward on train_adj beside the row SpMM's forward and transposed product and
        the maximum's kernels on the same matrix, width and plan, timed in ONE process in interleaved rounds (device events
        around `reps` calls)
    python profiles/attn_aggregator_probe.py epochs [--epochs 8]
        the README full-batch recipe with --aggregator sum and with attn: the times of `epochs` epochs behind one warm epoch
    python profiles/attn_aggregator_probe.py all
        both on one copy of the data
    python profiles/attn_aggregator_probe.py heads [--heads 2 4 8] [--d 128] [--rounds 7] [--reps 10]
        --attn_heads: attention's forward and its two-launch backward at heads = 1 and at every H given, on the same matrix,
        width and plan, in ONE process in interleaved rounds (each head count at its own default scale 1 / sqrt(d / H))

Records go to stdout as JSON lines (everything else to stderr)."""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np

RECIPE = ['--dataset', 's-reddit', '--normalization', 'graphsage', '--weight_decay', '0', '--dropout', '0.2', '--layer_norm',
          '--hidden1', '128', '--num_fc_layers', '2']
FULL = ['--full_batch', '--test_full_batch']


def _trainer(argv, data):
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
    t0 = time.time()
    with contextlib.redirect_stdout(sys.stderr):
        data = load_data(FLAGS.dataset)
    print("data in %.1f s" % (time.time() - t0), file=sys.stderr, flush=True)
    return data


def kernels(args, data):
    import torch
    from stochastic_gcn_amd import ops
    dev = torch.device('cuda:0')
    a = data[1].tocsr()
    n, d = a.shape[0], args.d
    A = ops.DeviceCSR.from_scipy(a, dev, with_transpose=True)
    rng = np.random.RandomState(0)
    x = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev)
    out, dx = torch.empty_like(x), torch.empty_like(x)
    scale = float(d) ** -0.5
    _, arg = ops.spmax(A, x, out=out)
    att = torch.empty_like(x)
    _, lse = ops.spattn(A, x, scale=scale, out=att)
    calls = {"spmm_fwd": lambda: ops.spmm(A, x, out=out),
             "spmm_bwd": lambda: ops.spmm(A.transpose, g, out=dx),
             "spmax_fwd": lambda: ops.spmax(A, x, out=out, arg=arg),
             "spmax_bwd": lambda: ops.spmax_bwd(A.transpose, g, arg, out=dx),
             "spattn_fwd": lambda: ops.spattn(A, x, scale=scale, out=out),
             "spattn_fwd_no_lse": lambda: ops.spattn(A, x, scale=scale, out=out, want_lse=False),
             "spattn_bwd": lambda: ops.spattn_bwd(A, A.transpose, x, None, g, att, lse, scale)}
    for f in calls.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.reps)
    deg = np.diff(a.indptr)
    rec = {"what": "kernels", "matrix": "s-reddit train_adj", "rows": n, "nnz": int(a.nnz), "max_row": int(deg.max()), "d": d,
           "scale": scale, "plan_T": "default", "split_rows": A.plan.nfix, "split_rows_T": A.transpose.plan.nfix,
           "rounds": args.rounds, "reps": args.reps, "gathered_bytes_per_product": int(a.nnz) * d * 4}
    for k, v in ms.items():
        rec[k + "_ms_median"], rec[k + "_ms_min"] = float(np.median(v)), float(min(v))
    rec["fwd_ratio_to_spmm"] = rec["spattn_fwd_ms_median"] / rec["spmm_fwd_ms_median"]
    rec["bwd_ratio_to_spmm"] = rec["spattn_bwd_ms_median"] / rec["spmm_bwd_ms_median"]
    print(json.dumps(rec), flush=True)


def heads(args, data):
    import torch
    from stochastic_gcn_amd import ops
    dev = torch.device('cuda:0')
    a = data[1].tocsr()
    n, d = a.shape[0], args.d
    A = ops.DeviceCSR.from_scipy(a, dev, with_transpose=True)
    rng = np.random.RandomState(0)
    x = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev)
    out = torch.empty_like(x)
    calls = {}
    for H in [1] + [h for h in args.heads if h != 1]:
        scale = float(d // H) ** -0.5
        att = torch.empty_like(x)
        _, lse = ops.spattn(A, x, scale=scale, out=att, heads=H)
        calls["fwd_h%d" % H] = lambda H=H, scale=scale: ops.spattn(A, x, scale=scale, out=out, heads=H)
        calls["bwd_h%d" % H] = lambda H=H, scale=scale, att=att, lse=lse: ops.spattn_bwd(A, A.transpose, x, None, g, att, lse,
                                                                                         scale, heads=H)
    for f in calls.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.reps)
    rec = {"what": "heads", "matrix": "s-reddit train_adj", "rows": n, "nnz": int(a.nnz), "d": d, "plan_T": "default",
           "split_rows": A.plan.nfix, "split_rows_T": A.transpose.plan.nfix, "rounds": args.rounds, "reps": args.reps}
    for k, v in ms.items():
        rec[k + "_ms_median"], rec[k + "_ms_min"], rec[k + "_ms_max"] = float(np.median(v)), float(min(v)), float(max(v))
    print(json.dumps(rec), flush=True)


def epochs(args, data):
    import torch
    for agg in ("sum", "attn", "sum", "attn"):
        trn = _trainer(RECIPE + FULL + ['--aggregator', agg, '--epochs', str(args.epochs)], data)
        trn.train_epoch()                                      # (tunes the widths, builds the transpose)
        torch.cuda.synchronize()
        wall, dev = [], []
        for _ in range(args.epochs):
            t = time.time()
            trn.train_epoch()                                  # (ends in a device synchronise)
            wall.append(time.time() - t)
            dev.append(trn.train_model.run_t)
        m = trn.train_static.matrix
        print(json.dumps({"what": "full_batch epochs", "aggregator": agg, "kernel": m.kernel, "epochs": args.epochs,
                          "epoch_wall_s": wall, "min_wall_s": min(wall), "median_wall_s": float(np.median(wall)),
                          "max_wall_s": max(wall), "min_device_s": min(dev), "static_setup_s": trn.static_setup_s,
                          "nnz": m.nnz}), flush=True)
        del trn, m
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "epochs", "all", "heads"])
    ap.add_argument("--heads", type=int, nargs='+', default=[2, 4, 8])
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=8)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    data = _data()
    for what in (["kernels", "epochs"] if args.what == "all" else [args.what]):
        {"kernels": kernels, "epochs": epochs, "heads": heads}[what](args, data)


if __name__ == "__main__":
    main()
