#!/usr/bin/env python
"""Measurements of the full-graph modes: --full_batch / --test_full_batch and the loss over a row subset.

    python profiles/full_batch_probe.py loss [--subset random|prefix]
        sgcn_softmax_ce_rows_f32 at S-Reddit size (N = 232,965, c = 41, n = 152,410 ids, a uniformly random subset or the
        first n ids): microseconds per call, beside the plain entry point on gathered copies and the call without a
        gradient.  (profiles/full_batch_loss_kernel.jsonl also holds the records of the zero fill that was not kept, "gap
        waves": each row's wave zeroing the gap in front of it, measured on the first form of the kernel.)
    python profiles/full_batch_probe.py epochs --kernel rows|cs|auto [--epochs 8]
        the S-Reddit README recipe without --cv, with --full_batch: setup time (plans, transpose, autotune: the first epoch
        included, which tunes the widths), every epoch's time, torch.cuda.max_memory_allocated
    python profiles/full_batch_probe.py sampled [--budget 400]
        the route that existed before: --nocv --degree 10000 --batch_size 152410, as many epochs as fit the budget (seconds)
    rocprofv3 --kernel-trace --stats -d D -- python profiles/full_batch_probe.py epochs --kernel cs --epochs 3
    python profiles/full_batch_probe.py summary --dir D --kernel cs --epochs 3
        where an epoch's time goes: the two products, the N-row GEMMs, LayerNorm, the loss
    python profiles/full_batch_probe.py convergence [--seeds 1,2,3,4,5] [--epochs 30]
        the README CVD+PP recipe per seed; test accuracy / F1 under --test_cv and, on the same weights, under
        --test_full_batch, the two sweep times, and per seed the difference against the seed-to-seed spread

Records go to stdout as JSON lines (everything else to stderr)."""
import argparse
import contextlib
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RECIPE = ['--dataset', 's-reddit', '--normalization', 'graphsage', '--weight_decay', '0', '--dropout', '0.2', '--layer_norm',
          '--hidden1', '128', '--num_fc_layers', '2']


def _timed(fn, reps, warm=5):
    import torch
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def loss(args):
    import numpy as np
    import torch
    from stochastic_gcn_amd import ops
    dev = torch.device("cuda:0")
    N, c, n = 232965, 41, 152410
    rng = np.random.RandomState(1)
    rows_h = (np.arange(n) if args.subset == "prefix" else np.sort(rng.permutation(N)[:n])).astype(np.int32)
    z = torch.from_numpy(rng.standard_normal((N, c)).astype(np.float32)).to(dev)
    y = torch.zeros((N, c), device=dev)
    y[torch.arange(N, device=dev), torch.from_numpy(rng.randint(0, c, N)).to(dev)] = 1.0
    rows = torch.from_numpy(rows_h).to(dev)
    Z, Y = z[rows.long()].contiguous(), y[rows.long()].contiguous()
    ops.pin_stream()
    rec = {"what": "softmax_ce_rows", "N": N, "c": c, "n": n, "zero_fill": "memset", "subset": args.subset,
           "reps": args.reps}
    # (the allocation of the outputs is part of every call, on both sides: the caching allocator, no device work)
    rec["rows_grad_us"] = _timed(lambda: ops.softmax_ce(z, y, want_grad=True, rows=rows), args.reps)
    rec["rows_nograd_pred_us"] = _timed(lambda: ops.softmax_ce(z, y, want_grad=False, want_pred=True, rows=rows), args.reps)
    rec["plain_on_gathered_grad_us"] = _timed(lambda: ops.softmax_ce(Z, Y, want_grad=True), args.reps)
    a = ops.softmax_ce(z, y, want_grad=True, rows=rows)
    b = ops.softmax_ce(Z, Y, want_grad=True)
    rec["stats_bit_identical"] = bool(torch.equal(a[0], b[0]))
    rec["grad_rows_bit_identical"] = bool(torch.equal(a[1][rows.long()], b[1]))
    off = torch.ones(N, dtype=torch.bool, device=dev)
    off[rows.long()] = False
    rec["off_rows_zero"] = bool((a[1][off].view(torch.int32) == 0).all())
    print(json.dumps(rec), flush=True)


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
    t0 = time.time()
    with contextlib.redirect_stdout(sys.stderr):
        data = load_data(FLAGS.dataset)
    print("data in %.1f s" % (time.time() - t0), file=sys.stderr, flush=True)
    return data


def epochs(args):
    import torch
    dev = torch.device("cuda:0")
    data = _data()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.time()
    trn = _trainer(RECIPE + ['--full_batch', '--full_batch_kernel', args.kernel, '--epochs', str(args.epochs)], data)
    torch.cuda.synchronize()
    build_s = time.time() - t0
    times = []
    for _ in range(args.epochs + 1):
        t = time.time()
        trn.train_epoch()
        times.append(time.time() - t)
    m = trn.train_static.matrix
    plan = getattr(m, '_plan', None)
    rec = {"what": "full_batch epochs", "kernel_flag": args.kernel, "kernel": m.kernel, "transpose_kernel": m.transpose.kernel,
           "products_asked": m.products, "nnz": m.nnz, "N": m.shape[0],
           "trainer_build_s": build_s, "static_setup_s": trn.static_setup_s, "first_epoch_s": times[0],
           "setup_total_s": trn.static_setup_s + max(times[0] - min(times[1:]), 0.0),
           "epoch_time_s": min(times[1:]), "epoch_times_s": times[1:], "device_epoch_s": trn.train_model.run_t,
           "pace": dict(getattr(plan, 'pace', {}) or {}) if plan is not None else None,
           "max_memory_allocated": torch.cuda.max_memory_allocated(dev),
           "train_loss_last": trn.avg_loss.mean(), "train_acc_last": trn.avg_acc.mean()}
    print(json.dumps(rec), flush=True)


def sampled(args):
    import torch
    dev = torch.device("cuda:0")
    data = _data()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    t_all = time.time()
    trn = _trainer(RECIPE + ['--nocv', '--degree', '10000', '--batch_size', '152410', '--epochs', '1'], data)
    times = []
    while time.time() - t_all < args.budget and len(times) < args.epochs:
        t = time.time()
        trn.train_epoch()
        times.append(time.time() - t)
    rec = {"what": "sampled exact route (--nocv --degree 10000 --batch_size 152410)", "budget_s": args.budget,
           "epochs_run": len(times), "epoch_times_s": times, "epoch_time_s": min(times) if times else None,
           "sch_wait_s": trn.last_epoch.get("sch_wait_s"), "sampled_edges": trn.last_epoch.get("sampled_edges"),
           "field0": trn.last_epoch.get("field0"), "max_memory_allocated": torch.cuda.max_memory_allocated(dev),
           "train_loss_last": trn.avg_loss.mean()}
    print(json.dumps(rec), flush=True)


def convergence(args):
    import torch
    seeds = [int(s) for s in args.seeds.split(",")]
    cvd = RECIPE + ['--epochs', str(args.epochs), '--early_stopping', str(args.epochs), '--batch_size=512',
                    '--test_batch_size=512', '--cv', '--cvd', '--degree=1', '--test_degree=1']
    data = _data()
    out = {}
    for seed in seeds:
        t0 = time.time()
        a = _trainer(cvd + ['--test_cv', '--seed', str(seed)], data)
        with contextlib.redirect_stdout(sys.stderr):
            a.SGDTrain()
        a.evaluate(a.val_d)                              # (warm: the sweep's buffers)
        cv_val, cv_test = a.evaluate(a.val_d), a.evaluate(a.test_d)
        params = a.train_model.get_params()
        del a
        torch.cuda.empty_cache()
        b = _trainer(cvd + ['--test_full_batch', '--seed', str(seed)], data)
        b.train_model.set_params(params)
        b.evaluate(b.val_d)                              # (warm: tunes the plan's widths)
        b._eval_logits_key = None
        fb_val = b.evaluate(b.val_d)                     # one forward + the loss
        fb_test = b.evaluate(b.test_d)                   # the loss alone: the logits are shared
        rec = {"seed": seed, "epochs": args.epochs, "n_test": int(len(b.test_d)), "eval_kernel": b.eval_static.matrix.kernel,
               "test_cv": dict(test_loss=cv_test[0], test_acc=cv_test[1], micro_f1=cv_test[2], macro_f1=cv_test[3],
                               val_sweep_s=cv_val[4], test_sweep_s=cv_test[4]),
               "test_full_batch": dict(test_loss=fb_test[0], test_acc=fb_test[1], micro_f1=fb_test[2], macro_f1=fb_test[3],
                                       val_sweep_s=fb_val[4], test_sweep_s_shared_forward=fb_test[4]),
               "wall_s": round(time.time() - t0, 1)}
        out[seed] = rec
        print(json.dumps(rec), flush=True)
        del b
        torch.cuda.empty_cache()
    acc = [out[s]["test_cv"]["test_acc"] for s in seeds]
    S = max(acc) - min(acc)
    p = sum(acc) / len(acc)
    se2 = 2 * math.sqrt(p * (1 - p) / out[seeds[0]]["n_test"])
    for s in seeds:
        diff = out[s]["test_full_batch"]["test_acc"] - out[s]["test_cv"]["test_acc"]
        print(json.dumps({"verdict_seed": s, "test_acc_full_batch_minus_test_cv": diff, "test_cv_seed_spread_S": S,
                          "two_standard_errors": se2, "bound": max(S, se2), "within": abs(diff) <= max(S, se2),
                          "note": "first measurement of the claim, not a gate"}), flush=True)


def summary(args):
    """the kernel table of a rocprofv3 --kernel-trace --stats run of `epochs` (per-epoch calls: against the timed epochs + 1)"""
    import glob
    import sqlite3
    f = glob.glob(os.path.join(args.dir, "**", "*results.db"), recursive=True)
    t = sqlite3.connect(f[0])
    rows = list(t.execute("select name,total_calls,total_duration,average,percentage from top_kernels"))
    n = args.epochs + 1
    print("== rocprofv3 --kernel-trace --stats of `full_batch_probe.py epochs --kernel %s --epochs %d`: %d full-batch epochs of "
          "S-Reddit (one step each), all kernels incl. set-up (PP products, plan autotune)" % (args.kernel, args.epochs, n))
    print("%-100s %8s %11s %12s %10s %6s" % ("kernel", "calls", "calls/epoch", "total_ms", "avg_us", "pct"))
    for r in rows[:40]:
        print("%-100s %8d %11.2f %12.2f %10.2f %6.2f" % (r[0][:100], r[1], r[1] / n, r[2] / 1e3, r[3], r[4]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["loss", "epochs", "sampled", "convergence", "summary"])
    ap.add_argument("--dir", default=None)
    ap.add_argument("--subset", default="random", choices=["random", "prefix"])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--kernel", default="auto")
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--budget", type=float, default=400.0)
    ap.add_argument("--seeds", default="1,2,3,4,5")
    args = ap.parse_args()
    if args.epochs is None:
        args.epochs = 30 if args.what == "convergence" else 8
    {"loss": loss, "epochs": epochs, "sampled": sampled, "convergence": convergence, "summary": summary}[args.what](args)


if __name__ == "__main__":
    main()
