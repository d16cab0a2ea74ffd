#!/usr/bin/env python
"""--history_dtype fp32 against bf16 on the trainer bench.py times (Reddit CVD+PP, `bench.train_epoch_leg` itself: the
probe only adds the flag to the FLAGS that leg sets), and what the rounding does to training.

    python profiles/history_dtype_probe.py epochs [--dtypes fp32,bf16,fp32,bf16] [--epochs 8] [--root DIR]
        one record per leg: epoch_time_s (best) and every epoch, ms_per_step, gpu_chain_us (bench.step_chain_probe),
        the history's bytes, the `History size` figure and torch.cuda.max_memory_allocated
        (--root DIR: import bench.py and the package from another checkout, e.g. the parent commit's; fp32 legs set no flag,
        so they run on a tree without it)
    rocprofv3 --kernel-trace --stats -d D -- python profiles/history_dtype_probe.py epochs --dtypes bf16 --epochs 2 --no-chain
    python profiles/epoch_profile.py --summarize D 596
    python profiles/history_dtype_probe.py rows
        history rows the aggregator reads and the scatter writes per step of that epoch (from the batches' row counts)
    python profiles/history_dtype_probe.py convergence [--seeds 1,2,3,4,5] [--epochs 30]
        the README's S-Reddit CVD+PP recipe per seed and dtype: final validation loss, validation and test accuracy, and
        the verdict per seed: |acc_bf16 - acc_fp32| <= max(S, 2 sqrt(p (1 - p) / n_test)), S = max - min of the fp32 runs

Records go to stdout as JSON lines (everything else to stderr)."""
import argparse
import contextlib
import json
import math
import os
import sys
import time


def _root(argv):
    for i, a in enumerate(argv):
        if a == "--root":
            return os.path.abspath(argv[i + 1])
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


ROOT = _root(sys.argv)
sys.path.insert(0, ROOT)


@contextlib.contextmanager
def _flags_with(over):
    """FLAGS.update(...) of the code under measurement also applies `over` (as profiles/epoch_profile.py's SGCN_FLAGS)"""
    from stochastic_gcn_amd.flags import FLAGS
    if not over:
        yield
        return
    orig = FLAGS.update
    FLAGS.update = lambda **kw: (orig(**kw), orig(**over))[0]
    try:
        yield
    finally:
        del FLAGS.update


def _hist_bytes(model):
    return sum(h.untyped_storage().nbytes() for hs in getattr(model, '_history', []) for h in hs)


def epochs(args):
    import torch
    import bench
    from stochastic_gcn_amd import synthetic, train
    dev = torch.device("cuda:0")
    data = synthetic.reddit_like(seed=1, with_features=False)
    made = []
    init = train.Trainer.__init__

    def spy(self, *a, **kw):
        init(self, *a, **kw)
        made.append(self)
    train.Trainer.__init__ = spy
    if args.no_chain:
        bench.step_chain_probe = lambda trn, reps=20: {}
    for leg, hd in enumerate(args.dtypes.split(",")):
        del made[:]
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        err = sys.stderr
        log = open(os.devnull, "w") if args.quiet else err
        with _flags_with({} if hd == "fp32" else dict(history_dtype=hd)):
            sys.stderr = log
            try:
                te = bench.train_epoch_leg(data, dev, epochs=args.epochs)
            finally:
                sys.stderr = err
        trn = made[-1]
        rec = {"leg": leg, "history_dtype": hd, "tree": "this commit" if ROOT == os.path.dirname(os.path.dirname(os.path.abspath(__file__))) else os.path.basename(ROOT), "epochs": args.epochs,
               "epoch_time_s": te["epoch_time_s"], "epoch_times_s": te["epoch_times_s"], "ms_per_step": te["ms_per_step"],
               "steps": te["steps"], "gpu_chain_us": te.get("gpu_chain_us"), "host_launch_us": te.get("host_launch_us"),
               "ops_per_step": (te.get("chain_probe") or {}).get("ops_per_step"),
               "history_bytes_train": _hist_bytes(trn.train_model), "history_bytes_test": _hist_bytes(trn.test_model),
               "history_table_dtype": str(trn.train_model._history[0][0].dtype),
               "max_memory_allocated": torch.cuda.max_memory_allocated(dev)}
        print(json.dumps(rec), flush=True)
        del trn, te
        del made[:]


def rows(args):
    """per step of the epoch bench.py times: history rows read by the aggregator (|ffield| through P, |field| through A)
    and written by the scatter, from the sampler's own batches"""
    import numpy as np
    from stochastic_gcn_amd import synthetic
    from stochastic_gcn_amd.scheduler import PyScheduler
    import model_cases as mc  # noqa: F401  (tests/ on the path: placeholders)
    n, train_adj, _, _, _, _, labels, tr, _, _ = synthetic.reddit_like(seed=1, with_features=False)
    ph = mc.placeholders(1, labels.shape[1])
    sch = PyScheduler(train_adj, labels, 1, [1], ph, 1, data=tr.copy(), cv=True)
    p_rows, a_rows, upd = [], [], []
    for _ in range(args.batches):
        fd = sch.minibatch(512)
        p_rows.append(fd[ph['fadj'][0]][0].shape[0])
        a_rows.append(fd[ph['adj'][0]][0].shape[0])
        upd.append(fd[ph['fields'][0]].shape[0])
    d = 128
    rec = {"batches": args.batches, "d": d, "p_nonzeros_per_step": float(np.mean(p_rows)), "a_nonzeros_per_step": float(np.mean(a_rows)),
           "rows_scattered_per_step": float(np.mean(upd))}
    for name, b in (("fp32", 4), ("bf16", 2)):
        rec["aggregator_history_bytes_per_step_" + name] = (rec["p_nonzeros_per_step"] + rec["a_nonzeros_per_step"]) * d * b
        rec["scatter_history_bytes_per_step_" + name] = rec["rows_scattered_per_step"] * d * b
    print(json.dumps(rec), flush=True)


def convergence(args):
    import torch
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.train import Trainer
    from stochastic_gcn_amd.utils import load_data
    seeds = [int(s) for s in args.seeds.split(",")]
    # README quick start: the S-Reddit CVD+PP recipe (gcn/config/reddit.config + --cv --cvd --degree=1), through the driver
    recipe = ['--dataset', 's-reddit', '--normalization', 'graphsage', '--weight_decay', '0', '--dropout', '0.2', '--layer_norm',
              '--hidden1', '128', '--num_fc_layers', '2', '--epochs', str(args.epochs), '--early_stopping', str(args.epochs),
              '--batch_size=512', '--test_batch_size=512', '--cv', '--cvd', '--test_cv', '--degree=1', '--test_degree=1']
    FLAGS.reset()
    FLAGS.parse(recipe)
    with contextlib.redirect_stdout(sys.stderr):
        data = load_data(FLAGS.dataset)
    out = {}
    for hd in ("fp32", "bf16"):
        for seed in seeds:
            FLAGS.reset()
            FLAGS.parse(recipe + ['--seed', str(seed), '--history_dtype', hd])
            t0 = time.time()
            with contextlib.redirect_stdout(sys.stderr):
                trn = Trainer(data=data, verbose=False)
                trn.SGDTrain()
                val = trn.evaluate(trn.val_d)
                test = trn.evaluate(trn.test_d)
            rec = {"history_dtype": hd, "seed": seed, "epochs": args.epochs, "val_loss": float(val[0]), "val_acc": float(val[1]),
                   "test_loss": float(test[0]), "test_acc": float(test[1]), "n_test": int(len(trn.test_d)),
                   "history_bytes_train": _hist_bytes(trn.train_model), "wall_s": round(time.time() - t0, 1)}
            out[(hd, seed)] = rec
            print(json.dumps(rec), flush=True)
            del trn
            torch.cuda.empty_cache()
    acc32 = [out[("fp32", s)]["test_acc"] for s in seeds]
    S = max(acc32) - min(acc32)
    p = sum(acc32) / len(acc32)
    n_test = out[("fp32", seeds[0])]["n_test"]
    se2 = 2 * math.sqrt(p * (1 - p) / n_test)
    bound = max(S, se2)
    for s in seeds:
        diff = out[("bf16", s)]["test_acc"] - out[("fp32", s)]["test_acc"]
        print(json.dumps({"verdict_seed": s, "test_acc_bf16_minus_fp32": diff, "fp32_seed_spread_S": S,
                          "two_standard_errors": se2, "bound": bound, "within": abs(diff) <= bound}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["epochs", "rows", "convergence"])
    ap.add_argument("--dtypes", default="fp32,bf16,fp32,bf16")
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--seeds", default="1,2,3,4,5")
    ap.add_argument("--batches", type=int, default=298)
    ap.add_argument("--root", default=None)
    ap.add_argument("--no-chain", action="store_true")
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args()
    if args.epochs is None:
        args.epochs = 30 if args.what == "convergence" else 8
    if args.what == "rows":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
    {"epochs": epochs, "rows": rows, "convergence": convergence}[args.what](args)


if __name__ == "__main__":
    main()
