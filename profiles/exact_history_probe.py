#!/usr/bin/env python
"""The exact control-variate history (--history_init / --history_refresh / --history_error) on the README's S-Reddit CVD+PP
recipe: what a pass costs, what the staleness kernel costs, how stale the history is, and what a fresh start does to the
first epochs.  No thresholds: every record is a measurement to be read beside its neighbour.

    python profiles/exact_history_probe.py staleness [--epochs 30] [--seed 1]
        per init (zeros, exact): the staleness of the training model's history before every epoch (rel_err, max_err, rows_off
        per layer), the wall time of that epoch's exact pass and the sampled epoch's train wall of the SAME run beside it,
        the validation loss per epoch; then one `pass` record per init: the median pass beside the median sampled epoch
        (the first pass apart: it allocates the twin's activations)
    python profiles/exact_history_probe.py kernel [--reps 30]
        sgcn_hist_error_f32 / _h16 on the recipe's history (N x 128): device-event time of one call (two launches), best and
        median of --reps, beside bytes / 6.3 TB/s with bytes = what the call must read (x and h once)
    python profiles/exact_history_probe.py convergence [--seeds 1,2,3,4,5] [--epochs 5]
        validation loss of epochs 1 .. 5 under both inits per seed, the per-seed difference exact - zeros per epoch, and
        the seed-to-seed spread (max - min over the seeds, per init and epoch) beside it

Records go to stdout as JSON lines (everything else to stderr)."""
import argparse
import contextlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12


def _recipe(epochs):
    # README quick start: the S-Reddit CVD+PP recipe (gcn/config/reddit.config + --cv --cvd --degree=1), through the driver
    return ['--dataset', 's-reddit', '--normalization', 'graphsage', '--weight_decay', '0', '--dropout', '0.2', '--layer_norm',
            '--hidden1', '128', '--num_fc_layers', '2', '--epochs', str(epochs), '--early_stopping', str(epochs + 2),
            '--batch_size=512', '--test_batch_size=512', '--cv', '--cvd', '--test_cv', '--degree=1', '--test_degree=1']


def _data(recipe):
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.utils import load_data
    FLAGS.reset()
    FLAGS.parse(recipe)
    with contextlib.redirect_stdout(sys.stderr):
        return load_data(FLAGS.dataset)


def _run(recipe, extra, data):
    """One training run through Trainer.SGDTrain; (per-epoch history records, per-epoch train wall, validation loss per epoch)."""
    import torch
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.train import Trainer
    FLAGS.reset()
    FLAGS.parse(recipe + extra)
    hist, walls = [], []
    with contextlib.redirect_stdout(sys.stderr):
        trn = Trainer(data=data, verbose=False)
        hp, te = trn.history_pass, trn.train_epoch

        def history_pass(epoch):
            r = hp(epoch)
            hist.append(r)
            return r

        def train_epoch():
            out = te()
            walls.append(trn.last_epoch['train_wall_s'])
            return out
        trn.history_pass, trn.train_epoch = history_pass, train_epoch
        trn.SGDTrain()
    cost = [float(c) for c in trn.cost_val]
    del trn
    torch.cuda.empty_cache()
    return hist, walls, cost


def staleness(args):
    recipe = _recipe(args.epochs)
    data = _data(recipe)
    for init in ("zeros", "exact"):
        hist, walls, cost = _run(recipe, ['--seed', str(args.seed), '--history_error', '--history_init', init], data)
        rows = []
        for r, w, c in zip(hist, walls, cost):
            rows.append({"epoch": r['epoch'], "rel_err": [l['rel_err'] for l in r['layers']],
                         "max_err": [l['max_err'] for l in r['layers']], "rows_off": [l['rows_off'] for l in r['layers']],
                         "refreshed": r['refreshed'], "pass_s": r['pass_s'], "train_wall_s": w, "val_loss": c})
        print(json.dumps({"record": "staleness", "history_init": init, "seed": args.seed, "epochs_flag": args.epochs,
                          "epochs": rows}), flush=True)
        later = [r['pass_s'] for r in hist[1:]]
        print(json.dumps({"record": "pass", "history_init": init, "seed": args.seed, "what": "one exact pass + the staleness "
                          "kernel + one 32-byte copy, timed to completion, beside the sampled epoch of the same run",
                          "first_pass_s": hist[0]['pass_s'], "pass_s_median": statistics.median(later), "pass_s_min": min(later),
                          "pass_s_max": max(later), "train_wall_s_median": statistics.median(walls[1:]),
                          "train_wall_s_min": min(walls[1:]), "passes": len(hist)}), flush=True)


def kernel(args):
    import torch
    from stochastic_gcn_amd import ops
    dev = torch.device("cuda:0")
    n = args.n
    d = args.d
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.randn((n, d), generator=g, device=dev)
    for name, bf16 in (("sgcn_hist_error_f32", False), ("sgcn_hist_error_h16", True)):
        H = ops.history_alloc(n, d, dev, bf16)
        ops.history_assign(H, x + 0.01 * torch.randn((n, d), generator=g, device=dev))
        out = torch.empty(4, dtype=torch.float64, device=dev)
        for _ in range(3):
            ops.history_error(x, H, out=out)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.history_error(x, H, out=out)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        v = out.cpu().tolist()
        nbytes = n * d * (4 + (2 if bf16 else 4))
        best = min(times)
        print(json.dumps({"record": "kernel", "entry": name, "n": n, "d": d, "reps": args.reps, "timed": "device events around "
                          "one call = two launches (the grid of 1,024 workgroups + the one-workgroup sum); the operands "
                          "(%.0f MB) are re-read every call" % (nbytes / 1e6),
                          "call_s_best": best, "call_s_median": statistics.median(times), "bytes": nbytes,
                          "bytes_over_6.3TBps_s": nbytes / HBM_BYTES_PER_S, "best_over_floor": best / (nbytes / HBM_BYTES_PER_S),
                          "GBps_at_best": nbytes / best / 1e9, "rel_err": (v[0] / v[1]) ** 0.5}), flush=True)


def convergence(args):
    seeds = [int(s) for s in args.seeds.split(",")]
    recipe = _recipe(args.epochs)
    data = _data(recipe)
    keep = 5
    val = {}
    for seed in seeds:
        for init in ("zeros", "exact"):
            _, _, cost = _run(recipe, ['--seed', str(seed), '--history_init', init], data)
            val[(init, seed)] = cost[:keep]
            print(json.dumps({"record": "val_loss", "history_init": init, "seed": seed, "val_loss_epochs_1_to_5": cost[:keep]}),
                  flush=True)
    for e in range(keep):
        z = [val[("zeros", s)][e] for s in seeds]
        x = [val[("exact", s)][e] for s in seeds]
        print(json.dumps({"record": "val_loss_difference", "epoch": e + 1, "seeds": seeds,
                          "exact_minus_zeros_per_seed": [a - b for a, b in zip(x, z)],
                          "seed_spread_zeros": max(z) - min(z), "seed_spread_exact": max(x) - min(x),
                          "mean_zeros": sum(z) / len(z), "mean_exact": sum(x) / len(x)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["staleness", "kernel", "convergence"])
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--seeds", default="1,2,3,4,5")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--n", type=int, default=232965)        # S-Reddit's vertex count
    ap.add_argument("--d", type=int, default=128)
    args = ap.parse_args()
    if args.epochs is None:
        args.epochs = 5 if args.what == "convergence" else 30
    {"staleness": staleness, "kernel": kernel, "convergence": convergence}[args.what](args)


if __name__ == "__main__":
    main()
