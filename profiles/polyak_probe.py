"""--polyak_decay: what it costs and what it does.  Rows go to stdout as JSON lines; the committed record is
profiles/polyak_epochs.jsonl (rows named in profiles/README.md).

  epochs  ONE leg in this process: the README's S-Reddit CVD+PP recipe through bench.train_epoch_leg -- epoch time, the
          train_epoch device chain per step (gpu_chain_us) and the ops per step -- at --decay D.  ``--root DIR`` measures
          another checkout of the project (the parent commit, built in its own tree; it knows no decay but 0).
  cost    the comparison the feature is accepted on: child processes of `epochs`, ALTERNATING parent (--parent DIR) / this
          commit at decay 0 / this commit at decay 0.99, --repeats times each in one session, then a verdict row: this
          commit's median at decay 0 inside the parent's own min-max range?  (If not, the off case is not free and the branch in
          adam_one has to become a template parameter.)  The decay-0.99 rows are recorded beside it: no threshold.
  effect  seeds x decays x {--test_cv, --test_full_batch}: 30 epochs of the recipe, validation loss per epoch and final test
          accuracy per run, then the seed-to-seed spread beside the per-seed differences.  A record, not a gate.
"""
import argparse
import contextlib
import json
import os
import statistics
import subprocess
import sys
import time


def _root(argv):
    for i, a in enumerate(argv):
        if a == "--root":
            return os.path.abspath(argv[i + 1])
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = _root(sys.argv)
sys.path.insert(0, ROOT)

RECIPE = ['--dataset', 's-reddit', '--normalization', 'graphsage', '--weight_decay', '0', '--dropout', '0.2', '--layer_norm',
          '--hidden1', '128', '--num_fc_layers', '2', '--batch_size=512', '--test_batch_size=512', '--cv', '--cvd',
          '--degree=1', '--test_degree=1']


@contextlib.contextmanager
def _flags_with(over):
    """FLAGS.update(...) of the code under measurement also applies `over` (as profiles/history_dtype_probe.py)"""
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
    err = sys.stderr
    with _flags_with(dict(polyak_decay=args.decay) if args.decay > 0 else {}):
        sys.stderr = open(os.devnull, "w") if args.quiet else err
        try:
            te = bench.train_epoch_leg(data, dev, epochs=args.epochs)
        finally:
            sys.stderr = err
    trn = made[-1]
    store = trn.train_model._store
    avg = getattr(store, 'average', None)
    rec = {"what": "epochs", "tree": "this commit" if ROOT == HERE else "parent (%s)" % os.path.basename(ROOT), "decay": args.decay,
           "epochs": args.epochs, "epoch_time_s": te["epoch_time_s"], "epoch_times_s": te["epoch_times_s"],
           "ms_per_step": te["ms_per_step"], "steps": te["steps"], "gpu_chain_us": te.get("gpu_chain_us"),
           "host_launch_us": te.get("host_launch_us"), "ops_per_step": (te.get("chain_probe") or {}).get("ops_per_step"),
           "parameters": int(store.theta.numel()), "average_allocated": avg is not None,
           "test_reads_average": bool(avg is not None and trn.test_model.theta.data_ptr() == avg.data_ptr())}
    print(json.dumps(rec), flush=True)


def cost(args):
    legs = [("this", 0.0), ("this", args.decay)]
    if args.parent:
        legs.insert(0, ("parent", 0.0))
    rows = []
    for rep in range(args.repeats):
        for tree, decay in legs:                       # alternating, one fresh process per leg
            cmd = [sys.executable, os.path.abspath(__file__), "epochs", "--decay", str(decay), "--epochs", str(args.epochs), "--quiet"]
            if tree == "parent":
                cmd += ["--root", os.path.abspath(args.parent)]
            out = subprocess.run(cmd, stdout=subprocess.PIPE, cwd=os.path.abspath(args.parent) if tree == "parent" else HERE,
                                 timeout=args.leg_timeout, check=True).stdout.decode()
            rec = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
            rec.update(repeat=rep, leg=tree)
            rows.append(rec)
            print(json.dumps(rec), flush=True)
    for key in ("epoch_time_s", "gpu_chain_us"):
        col = lambda tree, decay: [r[key] for r in rows if r["leg"] == tree and r["decay"] == decay and r.get(key) is not None]   # noqa: E731
        off, on, par = col("this", 0.0), col("this", args.decay), col("parent", 0.0)
        v = {"what": "cost_verdict", "quantity": key, "repeats": args.repeats,
             "this_off_median": statistics.median(off) if off else None, "this_off": off,
             "this_on_median": statistics.median(on) if on else None, "this_on": on, "decay_on": args.decay,
             "parent": par, "parent_min": min(par) if par else None, "parent_max": max(par) if par else None}
        if off and par:
            v["off_inside_parent_range"] = min(par) <= statistics.median(off) <= max(par)
        if off and on:
            v["on_minus_off_median"] = statistics.median(on) - statistics.median(off)
        print(json.dumps(v), flush=True)


def effect(args):
    import torch
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.train import Trainer
    from stochastic_gcn_amd.utils import load_data
    seeds = [int(s) for s in args.seeds.split(",")]
    decays = [float(d) for d in args.decays.split(",")]
    common = RECIPE + ['--epochs', str(args.epochs), '--early_stopping', str(args.epochs + 3)]
    FLAGS.reset()
    FLAGS.parse(common)
    with contextlib.redirect_stdout(sys.stderr):
        data = load_data(FLAGS.dataset)
    out = {}
    for mode, extra in (("test_cv", ['--test_cv']), ("test_full_batch", ['--test_full_batch'])):
        for decay in decays:
            for seed in seeds:
                FLAGS.reset()
                FLAGS.parse(common + extra + ['--seed', str(seed), '--polyak_decay', str(decay)])
                t0 = time.time()
                val_loss = []
                with contextlib.redirect_stdout(sys.stderr):
                    trn = Trainer(data=data, verbose=False)
                    for epoch in range(args.epochs):
                        trn.history_pass(epoch)
                        trn.train_epoch()
                        val_loss.append(float(trn.evaluate(trn.val_d)[0]))
                    test = trn.evaluate(trn.test_d)
                rec = {"what": "effect", "mode": mode, "decay": decay, "seed": seed, "epochs": args.epochs, "val_loss": val_loss,
                       "test_loss": float(test[0]), "test_acc": float(test[1]), "n_test": int(len(trn.test_d)),
                       "wall_s": round(time.time() - t0, 1)}
                out[(mode, decay, seed)] = rec
                print(json.dumps(rec), flush=True)
                del trn
                torch.cuda.empty_cache()
        base = [out[(mode, decays[0], s)]["test_acc"] for s in seeds]
        for decay in decays:
            acc = [out[(mode, decay, s)]["test_acc"] for s in seeds]
            print(json.dumps({"what": "effect_summary", "mode": mode, "decay": decay, "test_acc": acc,
                              "seed_spread": max(acc) - min(acc), "mean": sum(acc) / len(acc),
                              "minus_first_decay_per_seed": [a - b for a, b in zip(acc, base)],
                              "final_val_loss": [out[(mode, decay, s)]["val_loss"][-1] for s in seeds]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["epochs", "cost", "effect"])
    ap.add_argument("--decay", type=float, default=0.99)
    ap.add_argument("--decays", default="0,0.99,0.999")
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seeds", default="1,2,3,4,5")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, built in its own tree")
    ap.add_argument("--root", default=None)
    ap.add_argument("--leg-timeout", type=int, default=400)
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args()
    if args.epochs is None:
        args.epochs = 30 if args.what == "effect" else 8
    if args.what == "epochs" and args.decay == 0.99 and "--decay" not in sys.argv:
        args.decay = 0.0
    {"epochs": epochs, "cost": cost, "effect": effect}[args.what](args)


if __name__ == "__main__":
    main()
