#!/usr/bin/env python
"""Measurements of --full_batch_part_history on S-Reddit train_adj with the README recipe at --hidden1 128, for
(P, q) in {(8, 1), (32, 4)}.  Medians of interleaved rounds, everything in ONE process.

    python profiles/part_history_probe.py pull [--steps 6] [--rounds 7]
        per step of the schedule, at the hidden width: the pull launch on an fp32 and on a bfloat16 table (device events, and
        wall time with the synchronisation behind it) against the existing-kernel route to the same numbers --
        ops.scatter_rows of the fresh rows into an fp32 table, ops.csr_slice of the selected rows, scheduler.build_plan, ops.spmm
        over the table -- wall time, host work and synchronisation included; the largest |difference| of the two routes; the
        longest selected row
    python profiles/part_history_probe.py epochs [--rounds 7]
        epoch wall time of --full_batch_parts without the flag (the parent's path, untouched) and with it, fp32 and bfloat16
        tables, interleaved round by round, one warm epoch each first; per epoch and per step (steps + refreshed groups)
    python profiles/part_history_probe.py convergence [--epochs 30]
        validation accuracy after `epochs` epochs for plain --full_batch, parts, parts + history fp32, parts + history bf16.
        Recorded as found, one seed.
    python profiles/part_history_probe.py all

Records go to stdout as JSON lines (everything else to stderr); profiles/part_history.jsonl is that output."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from full_batch_parts_probe import FULL, PQ, RECIPE, _data, _parts, _trainer      # noqa: E402

HIST = {'off': [], 'fp32': ['--full_batch_part_history'], 'bf16': ['--full_batch_part_history', '--history_dtype', 'bf16']}


def _wall(fn):
    import torch
    torch.cuda.synchronize()
    t = time.time()
    fn()
    torch.cuda.synchronize()
    return (time.time() - t) * 1e3


def _events(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def pull(args, data):
    import torch
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.scheduler import build_plan
    for P, q in PQ:
        trn = _trainer(RECIPE + FULL + _parts(P, q) + HIST['fp32'], data)
        A, dev, d = trn.train_csr, trn.device, int(FLAGS.hidden1)
        N = int(A.shape[0])
        g = torch.Generator().manual_seed(1)
        H32 = torch.randn((N, d), generator=g).to(dev)
        H16 = ops.history_assign(ops.history_alloc(N, d, dev, bf16=True), H32)
        Hmerge = H32.clone()
        rows = []
        for ids in trn.part_schedule.epoch(1)[:args.steps]:
            batch = trn.part_batch(ids)                      # (the map of ``ids`` lives in the block it cut)
            n, ids_dev, vmap = len(ids), batch.ids_dev, batch.matrix.map
            x = torch.randn((n, d), generator=g).to(dev)
            out, ref = torch.empty((n, d), device=dev), torch.empty((n, d), device=dev)
            Hmerge.copy_(H32)                                # (the route writes its rows of S; the other rows stay H32's)

            def route():
                # the existing kernels' way to the same numbers: the fresh rows into the table, then one product over it
                ops.scatter_rows(Hmerge, ids_dev, x)
                sl = ops.csr_slice(A, ids, rows_dev=ids_dev)
                seg, fix, nslots = build_plan(sl.host_rowptr, 0)
                sl.plan = ops.DevicePlan(seg, fix, nslots, dev)
                ops.spmm(sl, Hmerge, out=ref)
            t = dict(pull_f32_dev_ms=[], pull_h16_dev_ms=[], pull_f32_wall_ms=[], pull_h16_wall_ms=[], route_wall_ms=[])
            for r in range(args.rounds + 1):
                a = _events(lambda: ops.spmm_pull(A, ids_dev, vmap, x, H32, out=out))
                b = _events(lambda: ops.spmm_pull(A, ids_dev, vmap, x, H16, out=out))
                c = _wall(lambda: ops.spmm_pull(A, ids_dev, vmap, x, H32, out=out))
                e = _wall(lambda: ops.spmm_pull(A, ids_dev, vmap, x, H16, out=out))
                f = _wall(route)
                if r:
                    for k, v in zip(t, (a, b, c, e, f)):
                        t[k].append(v)
            ops.spmm_pull(A, ids_dev, vmap, x, H32, out=out)
            hp = A.host_rowptr
            lens = hp[ids + 1].astype(np.int64) - hp[ids]
            rec = {k: float(np.median(v)) for k, v in t.items()}
            rec.update(n=n, entries=int(lens.sum()), in_part_entries=int(batch.matrix.nnz), longest_row=int(lens.max()),
                       mean_row=float(lens.mean()), max_abs_diff_to_route=float((out - ref).abs().max()),
                       max_abs_ref=float(ref.abs().max()))
            rows.append(rec)
        med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
        med['longest_row'] = int(max(r['longest_row'] for r in rows))
        print(json.dumps({"what": "pull", "P": P, "q": q, "d": d, "steps_measured": len(rows), "rounds": args.rounds,
                          "median": med, "steps": rows}), flush=True)
        del trn, A, H32, H16, Hmerge
        torch.cuda.empty_cache()


def epochs(args, data):
    import torch
    from stochastic_gcn_amd.flags import FLAGS
    configs = [(P, q, h) for P, q in PQ for h in ('off', 'fp32', 'bf16')]
    argv = {c: RECIPE + FULL + _parts(c[0], c[1]) + HIST[c[2]] for c in configs}
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
        print(json.dumps({"what": "epochs", "P": c[0], "q": c[1], "history": c[2], "rounds": args.rounds, "epoch_wall_s": wall[c],
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
        t = _trainer(RECIPE + FULL + _parts(P, q) + HIST[h] + ['--epochs', str(args.epochs), '--early_stopping',
                                                               str(args.epochs + 2)], data)
        with contextlib.redirect_stdout(sys.stderr):
            t.SGDTrain()
        val = t.evaluate(t.val_d)
        print(json.dumps({"what": "convergence (recorded only, one seed)", "P": P, "q": q, "history": h, "epochs_flag": args.epochs,
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
