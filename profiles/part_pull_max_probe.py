#!/usr/bin/env python
"""Measurements of --full_batch_part_pull_max on S-Reddit train_adj parts: (P, q) = (8, 1) and (32, 4), d = 128.

    python profiles/part_pull_max_probe.py pull [--steps 6] [--rounds 7]
        per step of epoch 1, by device events (medians over the rounds after one warm round, the launches alternating inside a
        round, ONE process): the pull launch (ops.spmax_pull) on an fp32 and on a bfloat16 table, next to what the same step
        runs WITHOUT stored rows -- the block's one-table maximum (ops.spmax on A[S, S] with its plan); the step's rows: n, all
        stored entries, in-part entries, the longest and the mean selected row; the share of elements a stale row won.
    python profiles/part_pull_max_probe.py epochs [--rounds 7]
        wall time per epoch of --full_batch_parts --aggregator max without the flag, with it (fp32 tables) and with bfloat16
        tables, the configurations alternating inside a round.
    python profiles/part_pull_max_probe.py convergence [--epochs 30]
        validation accuracy after the README recipe for plain --full_batch --aggregator max and the three configurations of
        both (P, q).  Recorded as found, one seed.
    python profiles/part_pull_max_probe.py all

Records go to stdout as JSON lines (everything else to stderr); profiles/part_pull_max.jsonl is that output."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from full_batch_parts_probe import FULL, PQ, RECIPE, _data, _parts, _trainer      # noqa: E402
from part_history_probe import _events                                             # noqa: E402

MAX = ['--aggregator', 'max']
PULL = {'off': [], 'fp32': ['--full_batch_part_pull_max'], 'bf16': ['--full_batch_part_pull_max', '--history_dtype', 'bf16']}


def pull(args, data):
    import torch
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd.flags import FLAGS
    for P, q in PQ:
        trn = _trainer(RECIPE + FULL + MAX + _parts(P, q) + PULL['fp32'], data)
        A, dev, d = trn.train_csr, trn.device, int(FLAGS.hidden1)
        N = int(A.shape[0])
        g = torch.Generator().manual_seed(1)
        H32 = (0.5 * torch.randn((N, d), generator=g)).to(dev)
        H16 = ops.history_assign(ops.history_alloc(N, d, dev, bf16=True), H32)
        rows = []
        for ids in trn.part_schedule.epoch(1)[:args.steps]:
            batch = trn.part_batch(ids)
            m = batch.matrix
            n, ids_dev, vmap, blk = len(ids), batch.ids_dev, m.map, m.rows_csr
            x = (0.5 * torch.randn((n, d), generator=g)).to(dev)
            out32, arg32 = ops.spmax_pull(A, ids_dev, vmap, x, H32)
            out16, arg16 = ops.spmax_pull(A, ids_dev, vmap, x, H16)
            outb, argb = ops.spmax(blk, x)
            launches = dict(
                pull_f32_ms=lambda: ops.spmax_pull(A, ids_dev, vmap, x, H32, out=out32, arg=arg32),
                pull_h16_ms=lambda: ops.spmax_pull(A, ids_dev, vmap, x, H16, out=out16, arg=arg16),
                block_ms=lambda: ops.spmax(blk, x, out=outb, arg=argb))
            t = {k: [] for k in launches}
            for r in range(args.rounds + 1):
                for k, fn in launches.items():
                    v = _events(fn)
                    if r:
                        t[k].append(v)
            hp = A.host_rowptr
            lens = hp[ids + 1].astype(np.int64) - hp[ids]
            rec = {k: float(np.median(v)) for k, v in t.items()}
            rec.update(n=n, entries=int(lens.sum()), in_part_entries=int(m.nnz), longest_row=int(lens.max()),
                       mean_row=float(lens.mean()), stale_winner_share=float((arg32 <= -2).float().mean()),
                       finite=bool(torch.isfinite(out32).all() and torch.isfinite(out16).all()))
            rows.append(rec)
            print("P %d q %d step: %s" % (P, q, rec), file=sys.stderr, flush=True)
        med = {k: float(np.median([r[k] for r in rows])) for k in rows[0] if k != 'finite'}
        med['longest_row'] = int(max(r['longest_row'] for r in rows))
        print(json.dumps({"what": "part_pull_max", "P": P, "q": q, "d": d, "steps_measured": len(rows), "rounds": args.rounds,
                          "median": med, "steps": rows}), flush=True)
        del trn, A, H32, H16
        torch.cuda.empty_cache()


def epochs(args, data):
    import torch
    from stochastic_gcn_amd.flags import FLAGS
    configs = [(P, q, h) for P, q in PQ for h in ('off', 'fp32', 'bf16')]
    argv = {c: RECIPE + FULL + MAX + _parts(c[0], c[1]) + PULL[c[2]] for c in configs}
    trn = {c: _trainer(argv[c], data) for c in configs}
    wall = {c: [] for c in configs}
    for r in range(args.rounds + 1):
        for c in configs:
            FLAGS.reset()
            FLAGS.parse(argv[c])                              # (the layers read FLAGS at run time)
            torch.cuda.synchronize()
            t = time.time()
            trn[c].train_epoch()                              # (ends in a device synchronise)
            if r:
                wall[c].append(time.time() - t)
    for c in configs:
        le = trn[c].last_epoch
        launches = le['steps'] + le.get('refreshed', 0)
        base = float(np.median(wall[(c[0], c[1], 'off')]))
        print(json.dumps({"what": "epochs", "P": c[0], "q": c[1], "pull_max": c[2], "rounds": args.rounds, "epoch_wall_s": wall[c],
                          "median_wall_s": float(np.median(wall[c])), "min_wall_s": min(wall[c]), "steps": le['steps'],
                          "skipped": le['skipped'], "refreshed": le.get('refreshed', 0),
                          "median_ms_per_step": float(np.median(wall[c])) * 1e3 / max(launches, 1),
                          "ratio_to_parts_without_the_flag": float(np.median(wall[c]) / base)}), flush=True)


def convergence(args, data):
    import contextlib
    import torch
    configs = [(0, 0, 'off')] + [(P, q, h) for P, q in PQ for h in ('off', 'fp32', 'bf16')]
    for P, q, h in configs:
        t0 = time.time()
        t = _trainer(RECIPE + FULL + MAX + _parts(P, q) + PULL[h] + ['--epochs', str(args.epochs), '--early_stopping',
                                                                     str(args.epochs + 2)], data)
        with contextlib.redirect_stdout(sys.stderr):
            t.SGDTrain()
        val = t.evaluate(t.val_d)
        print(json.dumps({"what": "convergence (recorded only, one seed)", "P": P, "q": q, "pull_max": h, "epochs_flag": args.epochs,
                          "adam_steps": int(t.train_model.adam_t), "train_loss_last": t.avg_loss.mean(), "val_loss": val[0],
                          "val_acc": val[1], "wall_s": round(time.time() - t0, 1)}), flush=True)
        del t
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["pull", "epochs", "convergence", "all"])
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=30)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    data = _data()
    for what in (["pull", "epochs", "convergence"] if args.what == "all" else [args.what]):
        {"pull": pull, "epochs": epochs, "convergence": convergence}[what](args, data)


if __name__ == "__main__":
    main()
