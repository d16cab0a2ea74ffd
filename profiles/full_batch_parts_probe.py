#!/usr/bin/env python
"""Measurements of --full_batch_parts on S-Reddit train_adj, hidden width 128, for (P, q) in {(8, 1), (32, 4)}.

    python profiles/full_batch_parts_probe.py steps [--steps 8]
        per step: the three induce launches, the transposed block as the same cut of the resident transpose (what a step runs)
        and as sgcn_csr_transpose_index + sgcn_gather_f32 on the block (device events around a replay of ops.csr_induce's calls
        on the trainer's own buffers), the whole build (Trainer.part_batch, wall), the host part of it (build - device), and the
        training step itself (events)
    python profiles/full_batch_parts_probe.py epochs [--rounds 7]
        epoch wall time of --full_batch --full_batch_kernel rows (the code path of a run without the flag, unchanged by it)
        and of both (P, q), in ONE process, interleaved round by round, one warm epoch each first; medians
    python profiles/full_batch_parts_probe.py convergence [--epochs 30] [--aggs sum,attn]
        validation accuracy after `epochs` epochs for plain --full_batch and for both (P, q).  Recorded only.
    python profiles/full_batch_parts_probe.py all

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
PQ = ((8, 1), (32, 4))


def _parts(P, q):
    return ['--full_batch_parts', str(P), '--full_batch_parts_per_step', str(q)] if P else ['--full_batch_kernel', 'rows']


def _trainer(argv, data):
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.train import Trainer
    FLAGS.reset()
    FLAGS.parse(argv)
    with contextlib.redirect_stdout(sys.stderr):
        return Trainer(data=data, verbose=True)


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


def _replay(A, ids_dev, n, bound, norm_rows):
    """ops.csr_induce's device calls once more on A's buffers, by device events: (the three induce launches of the block, the
    transposed block as the same cut of the resident transpose -- what a step runs --, and the transposed block by
    sgcn_csr_transpose_index + sgcn_gather_f32 over the padded block, the path of a matrix without a resident transpose) in ms"""
    import torch
    from stochastic_gcn_amd._ffi import check, lib
    b, At, N, st = A._induce, A.transpose, A.shape[0], torch.cuda.current_stream().cuda_stream
    b.fit(n, bound, transposition=True)                 # (sizes the transposition's workspace, which a step never needs)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ptr = lambda t: t.data_ptr()      # noqa: E731
    rscale = ptr(b.rscale) if norm_rows else None       # (the values of the build that sized the buffers: same work)
    ev[0].record()
    check(lib.sgcn_induce_map_i32(ptr(ids_dev), n, N, ptr(b.map), st))
    check(lib.sgcn_csr_induce_count(ptr(A.rowptr), ptr(A.col), ptr(A.val), ptr(ids_dev), n, ptr(b.map), ptr(b.rowptr), ptr(b.full),
                                    ptr(b.kept), st))
    check(lib.sgcn_csr_induce_fill(ptr(A.rowptr), ptr(A.col), ptr(A.val), ptr(ids_dev), n, ptr(b.map), ptr(b.rowptr), rscale,
                                   ptr(b.col), ptr(b.val), ptr(b.coo), 0, bound, st))
    ev[1].record()
    check(lib.sgcn_csr_induce_count(ptr(At.rowptr), ptr(At.col), None, ptr(ids_dev), n, ptr(b.map), ptr(b.t_rowptr), None, None, st))
    check(lib.sgcn_csr_induce_fill(ptr(At.rowptr), ptr(At.col), ptr(At.val), ptr(ids_dev), n, ptr(b.map), ptr(b.t_rowptr), rscale,
                                   ptr(b.t_row), ptr(b.t_val), None, 1, 0, st))
    ev[2].record()
    check(lib.sgcn_csr_transpose_index(n + 1, bound, ptr(b.col), ptr(b.coo), ptr(b.t_rowptr), ptr(b.t_row), ptr(b.t_src),
                                       ptr(b.ws), st))
    check(lib.sgcn_gather_f32(ptr(b.val), ptr(b.t_src), bound, ptr(b.t_val), st))
    ev[3].record()
    ev[3].synchronize()
    return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), ev[2].elapsed_time(ev[3])


def steps(args, data):
    import torch
    from stochastic_gcn_amd.flags import FLAGS
    for P, q in PQ:
        trn = _trainer(RECIPE + FULL + _parts(P, q), data)
        A, hp = trn.train_csr, trn.train_csr.host_rowptr
        rows = []
        for e in range(2):                                   # (epoch 0 warms the buffers and the allocator up)
            for ids in trn.part_schedule.epoch(e)[:args.steps]:
                torch.cuda.synchronize()
                t0 = time.time()
                batch = trn.part_batch(ids)
                build = time.time() - t0
                if batch is None:
                    continue
                batch.dropout = FLAGS.dropout
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                trn.train_model.run_one_step(None, batch, sync=False)
                e1.record()
                e1.synchronize()
                n, bound = len(ids), int((hp[ids + 1].astype(np.int64) - hp[ids]).sum())
                induce_ms, cut_t_ms, transposition_ms = _replay(A, batch.ids_dev, n, bound, trn.part_norm == 'rows')
                if e:
                    rows.append(dict(n=n, bound=bound, nnz=batch.matrix.nnz, build_ms=build * 1e3, induce_ms=induce_ms,
                                     transpose_by_cut_ms=cut_t_ms, transpose_by_transposition_ms=transposition_ms,
                                     host_ms=build * 1e3 - induce_ms - cut_t_ms, step_ms=e0.elapsed_time(e1)))
        med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
        print(json.dumps({"what": "steps", "P": P, "q": q, "steps_measured": len(rows), "median": med, "part_stats": trn.part_stats,
                          "setup_s": trn.static_setup_s}), flush=True)
        del trn, A
        torch.cuda.empty_cache()


def epochs(args, data):
    import torch
    configs = ((0, 0),) + PQ
    trn = {c: _trainer(RECIPE + FULL + _parts(*c), data) for c in configs}
    wall = {c: [] for c in configs}
    from stochastic_gcn_amd.flags import FLAGS
    for r in range(args.rounds + 1):
        for c in configs:
            FLAGS.reset()
            FLAGS.parse(RECIPE + FULL + _parts(*c))         # (the layers read FLAGS at run time)
            torch.cuda.synchronize()
            t = time.time()
            trn[c].train_epoch()                             # (ends in a device synchronise)
            if r:
                wall[c].append(time.time() - t)
    for c in configs:
        print(json.dumps({"what": "epochs", "P": c[0], "q": c[1], "rounds": args.rounds, "epoch_wall_s": wall[c],
                          "median_wall_s": float(np.median(wall[c])), "min_wall_s": min(wall[c]),
                          "steps_per_epoch": trn[c].last_epoch['steps'],
                          "ratio_to_full_batch_rows": float(np.median(wall[c]) / np.median(wall[(0, 0)]))}), flush=True)


def convergence(args, data):
    import torch
    for agg in args.aggs:
        extra = ['--aggregator', 'attn', '--attn_heads', '2'] if agg == 'attn' else []
        for c in ((0, 0),) + PQ:
            t0 = time.time()
            t = _trainer(RECIPE + FULL + _parts(*c) + extra + ['--epochs', str(args.epochs), '--early_stopping',
                                                               str(args.epochs + 2)], data)
            with contextlib.redirect_stdout(sys.stderr):
                t.SGDTrain()
            val = t.evaluate(t.val_d)
            print(json.dumps({"what": "convergence (recorded only)", "aggregator": agg, "P": c[0], "q": c[1], "epochs_flag": args.epochs,
                              "adam_steps": int(t.train_model.adam_t), "train_loss_last": t.avg_loss.mean(), "val_loss": val[0],
                              "val_acc": val[1], "wall_s": round(time.time() - t0, 1)}), flush=True)
            del t
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["steps", "epochs", "convergence", "all"])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--aggs", type=lambda s: s.split(","), default=["sum", "attn"])
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    data = _data()
    for what in (["steps", "epochs", "convergence"] if args.what == "all" else [args.what]):
        {"steps": steps, "epochs": epochs, "convergence": convergence}[what](args, data)


if __name__ == "__main__":
    main()
