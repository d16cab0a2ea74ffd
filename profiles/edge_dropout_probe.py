#!/usr/bin/env python
"""Measurements of --edge_dropout: what the flag costs when it is off and when it is on.

    python profiles/edge_dropout_probe.py epochs [--root TREE] [--p 0,0.2] [--kernels rows,cs] [--epochs 8] [--tag NAME]
        the S-Reddit README recipe without --cv, with --full_batch --full_batch_kernel K, per kernel and per flag value:
        the times of `epochs` epochs behind one warm epoch.  ``--root`` imports the package of ANOTHER checkout (the parent
        commit's: run it with ``--p none``, which passes no --edge_dropout at all); a comparison alternates the trees, one
        process per tree and round, every process loading the data once.
    python profiles/edge_dropout_probe.py redraw [--kernels rows,cs] [--reps 200]
        one re-draw of every value array of the training adjacency (A and A^T): microseconds per call beside the byte
        floor (12 B per stored entry -- base and pair key read, the value written -- at the 6.3 TB/s HBM streams reach),
        and the extra memory the matrix holds (8 B per stored entry per value array: pair keys + the re-drawn values)
    python profiles/edge_dropout_probe.py convergence [--seeds 1,2,3,4,5] [--p 0,0.2,0.5] [--epochs 30]
        the same recipe with --test_full_batch per seed and P: last training loss, validation loss, test accuracy / F1.
        Recorded only: 30 full-graph steps show no learning curve, nothing about accuracy follows.

Records go to stdout as JSON lines (everything else to stderr)."""
import argparse
import contextlib
import json
import os
import sys
import time

RECIPE = ['--dataset', 's-reddit', '--normalization', 'graphsage', '--weight_decay', '0', '--dropout', '0.2', '--layer_norm',
          '--hidden1', '128', '--num_fc_layers', '2']
HBM_BYTES_PER_S = 6.3e12


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


def _edge_args(p):
    return [] if p is None else ['--edge_dropout', repr(p)]


def epochs(args):
    import torch
    data = _data()
    for kernel in args.kernels:
        for p in args.p:
            trn = _trainer(RECIPE + ['--full_batch', '--full_batch_kernel', kernel, '--epochs', str(args.epochs)] + _edge_args(p), data)
            trn.train_epoch()                                      # (tunes the widths, builds the transpose)
            torch.cuda.synchronize()
            wall, dev = [], []
            for _ in range(args.epochs):
                t = time.time()
                trn.train_epoch()                                  # (ends in a device synchronise)
                wall.append(time.time() - t)
                dev.append(trn.train_model.run_t)
            m = trn.train_static.matrix
            print(json.dumps({"what": "full_batch epochs", "tree": args.tag, "kernel": m.kernel, "edge_dropout": p,
                              "epochs": args.epochs, "epoch_wall_s": wall, "epoch_device_s": dev, "min_wall_s": min(wall),
                              "max_wall_s": max(wall), "min_device_s": min(dev), "max_device_s": max(dev),
                              "train_loss_last": trn.avg_loss.mean(), "nnz": m.nnz}), flush=True)
            del trn, m
            torch.cuda.empty_cache()


def redraw(args):
    import torch
    from stochastic_gcn_amd import ops
    data = _data()
    for kernel in args.kernels:
        trn = _trainer(RECIPE + ['--full_batch', '--full_batch_kernel', kernel, '--edge_dropout', '0.2'], data)
        trn.train_epoch()
        torch.cuda.synchronize()
        mat = trn.train_static.matrix
        for side, m in (("A", mat), ("A^T", mat.transpose)):
            for k, slot in sorted(m._redrawn.items()):
                n = int(slot['base'].numel())
                call = lambda: ops.edge_revalue(slot['base'], slot['pair'], 12345, 0.8, out=slot['out'])      # noqa: E731
                for _ in range(10):
                    call()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.reps):
                    call()
                e1.record()
                e1.synchronize()
                us = e0.elapsed_time(e1) * 1e3 / args.reps
                print(json.dumps({"what": "edge_revalue", "matrix_kernel": kernel, "side": side, "array": k, "entries": n,
                                  "nnz": m.nnz, "us_per_call": us, "bytes": 12 * n, "floor_us": 12 * n / HBM_BYTES_PER_S * 1e6,
                                  "achieved_TB_per_s": 12 * n / (us * 1e-6) / 1e12, "extra_bytes": 8 * n,
                                  "reps": args.reps}), flush=True)
        slots = [s for m in (mat, mat.transpose) for s in m._redrawn.values()]
        print(json.dumps({"what": "edge_dropout memory", "matrix_kernel": kernel, "value_arrays": len(slots),
                          "extra_bytes_held": sum(t.numel() * t.element_size() for s in slots for t in (s['pair'], s['out'])),
                          "extra_bytes_8_per_entry": sum(8 * int(s['base'].numel()) for s in slots)}), flush=True)
        del trn, mat
        torch.cuda.empty_cache()


def convergence(args):
    import torch
    data = _data()
    for seed in args.seeds:
        for p in args.p:
            t0 = time.time()
            trn = _trainer(RECIPE + ['--full_batch', '--test_full_batch', '--epochs', str(args.epochs), '--early_stopping',
                                     str(args.epochs + 2), '--seed', str(seed)] + _edge_args(p), data)
            with contextlib.redirect_stdout(sys.stderr):
                trn.SGDTrain()
            val, test = trn.evaluate(trn.val_d), trn.evaluate(trn.test_d)
            print(json.dumps({"what": "convergence (recorded only)", "seed": seed, "edge_dropout": p, "epochs_flag": args.epochs,
                              "kernel": trn.train_static.matrix.kernel, "train_loss_last": trn.avg_loss.mean(),
                              "val_loss": val[0], "val_acc": val[1], "test_loss": test[0], "test_acc": test[1],
                              "micro_f1": test[2], "macro_f1": test[3], "wall_s": round(time.time() - t0, 1)}), flush=True)
            del trn
            torch.cuda.empty_cache()


def _floats(s):
    return [None if x == "none" else float(x) for x in s.split(",")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["epochs", "redraw", "convergence"])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="this")
    ap.add_argument("--p", type=_floats, default=None)
    ap.add_argument("--kernels", type=lambda s: s.split(","), default=["rows", "cs"])
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--seeds", type=lambda s: [int(x) for x in s.split(",")], default=[1, 2, 3, 4, 5])
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    if args.p is None:
        args.p = [0.0, 0.2, 0.5] if args.what == "convergence" else [0.0, 0.2]
    if args.epochs is None:
        args.epochs = 30 if args.what == "convergence" else 8
    {"epochs": epochs, "redraw": redraw, "convergence": convergence}[args.what](args)


if __name__ == "__main__":
    main()
