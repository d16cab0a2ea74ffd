#!/usr/bin/env python
"""Measurements of --full_batch_part_pull_gat on S-Reddit train_adj parts, hidden width 128, heads 4, for
(P, q) in {(8, 1), (32, 4)}.

    python profiles/part_pull_gat_probe.py launches [--steps 4] [--rounds 7]
        per step of epoch 1, by device events (medians over the rounds after one warm round, the launches alternating inside a
        round, all in ONE process on the SAME vertex sets and the same x, g and row table):
          ops.spgat_pull next to ops.spattn_pull, ops.spgat_pull_bwd_u next to ops.spattn_pull_bwd_q, each on an fp32 and on a
          bfloat16 row table; the two launches the GAT step adds around them (ops.gat_scores in front, the block's
          ops.spgat_pull_bwd_v behind); the step's rows: n, all stored entries, in-part entries, the longest and the mean row.
        The expectation to confirm or refute: the GAT forward is no slower than the dot forward (no cross-lane reduction).
    python profiles/part_pull_gat_probe.py epochs [--epoch_rounds 3]
        epoch wall time of --full_batch_part_pull_gat --aggregator attn --attn_score gat against --full_batch_part_pull
        --aggregator attn, both at 4 heads, in one process, interleaved round by round behind one warm epoch each; medians.
    python profiles/part_pull_gat_probe.py all

Recorded, not gated.  Records go to stdout as JSON lines (everything else to stderr); profiles/part_pull_gat.jsonl is that
output."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # the package, run from anywhere
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from full_batch_parts_probe import FULL, PQ, RECIPE, _data, _parts, _trainer      # noqa: E402
from part_history_probe import _events                                             # noqa: E402

HEADS = 4
GAT = ['--full_batch_part_pull_gat', '--aggregator', 'attn', '--attn_score', 'gat', '--attn_heads', str(HEADS)]
DOT = ['--full_batch_part_pull', '--aggregator', 'attn', '--attn_heads', str(HEADS)]


def launches(args, data):
    import torch
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd.flags import FLAGS
    heads = HEADS
    for P, q in PQ:
        trn = _trainer(RECIPE + FULL + _parts(P, q) + GAT, data)
        A, dev, d = trn.train_csr, trn.device, int(FLAGS.hidden1)
        N = int(A.shape[0])
        scale, slope = float(d // heads) ** -0.5, float(FLAGS.attn_slope)
        g = torch.Generator().manual_seed(1)
        H32 = (0.5 * torch.randn((N, d), generator=g)).to(dev)
        H16 = ops.history_assign(ops.history_alloc(N, d, dev, bf16=True), H32)
        avec = (torch.randn((2, d), generator=g) * (d // heads) ** -0.5).to(dev)
        VH = ops.gat_scores(H32, avec, heads=heads)[:, heads:].contiguous()         # what a push would have stored
        rows = []
        for ids in trn.part_schedule.epoch(1)[:args.steps]:
            batch = trn.part_batch(ids)
            m = batch.matrix
            n, ids_dev, vmap, blk_t = len(ids), batch.ids_dev, m.map, m.transpose.rows_csr
            x = (0.5 * torch.randn((n, d), generator=g)).to(dev)
            gr = torch.randn((n, d), generator=g).to(dev)
            S = ops.gat_scores(x, avec, heads=heads)
            U, V = S[:, :heads], S[:, heads:]
            og32, lg32 = ops.spgat_pull(A, ids_dev, vmap, x, H32, U, V, VH, slope, heads=heads)
            og16, lg16 = ops.spgat_pull(A, ids_dev, vmap, x, H16, U, V, VH, slope, heads=heads)
            od32, ld32 = ops.spattn_pull(A, ids_dev, vmap, x, H32, scale, heads=heads)
            od16, ld16 = ops.spattn_pull(A, ids_dev, vmap, x, H16, scale, heads=heads)
            dU, delta = ops.spgat_pull_bwd_u(A, ids_dev, vmap, x, H32, U, V, VH, gr, og32, lg32, slope, heads=heads)
            runs = dict(
                gat_pull_fwd_f32_ms=lambda: ops.spgat_pull(A, ids_dev, vmap, x, H32, U, V, VH, slope, out=og32, heads=heads),
                dot_pull_fwd_f32_ms=lambda: ops.spattn_pull(A, ids_dev, vmap, x, H32, scale, out=od32, heads=heads),
                gat_pull_fwd_h16_ms=lambda: ops.spgat_pull(A, ids_dev, vmap, x, H16, U, V, VH, slope, out=og16, heads=heads),
                dot_pull_fwd_h16_ms=lambda: ops.spattn_pull(A, ids_dev, vmap, x, H16, scale, out=od16, heads=heads),
                gat_pull_bwd_u_f32_ms=lambda: ops.spgat_pull_bwd_u(A, ids_dev, vmap, x, H32, U, V, VH, gr, og32, lg32, slope, heads=heads),
                dot_pull_bwd_q_f32_ms=lambda: ops.spattn_pull_bwd_q(A, ids_dev, vmap, x, H32, gr, od32, ld32, scale, heads=heads),
                gat_pull_bwd_u_h16_ms=lambda: ops.spgat_pull_bwd_u(A, ids_dev, vmap, x, H16, U, V, VH, gr, og16, lg16, slope, heads=heads),
                dot_pull_bwd_q_h16_ms=lambda: ops.spattn_pull_bwd_q(A, ids_dev, vmap, x, H16, gr, od16, ld16, scale, heads=heads),
                gat_scores_ms=lambda: ops.gat_scores(x, avec, heads=heads),
                gat_block_bwd_v_ms=lambda: ops.spgat_pull_bwd_v(blk_t, x, U, V, gr, lg32, delta, slope, heads=heads))
            t = {k: [] for k in runs}
            for r in range(args.rounds + 1):
                for k, fn in runs.items():
                    v = _events(fn)
                    if r:
                        t[k].append(v)
            hp = A.host_rowptr
            lens = hp[ids + 1].astype(np.int64) - hp[ids]
            rec = {k: float(np.median(v)) for k, v in t.items()}
            rec.update(n=n, entries=int(lens.sum()), in_part_entries=int(m.nnz), longest_row=int(lens.max()),
                       mean_row=float(lens.mean()), finite=bool(torch.isfinite(og32).all() and torch.isfinite(dU).all()))
            rows.append(rec)
            print("P %d q %d step: %s" % (P, q, rec), file=sys.stderr, flush=True)
        med = {k: float(np.median([r[k] for r in rows])) for k in rows[0] if k != 'finite'}
        med['longest_row'] = int(max(r['longest_row'] for r in rows))
        print(json.dumps({"what": "part_pull_gat launches", "P": P, "q": q, "d": d, "heads": heads, "steps_measured": len(rows),
                          "rounds": args.rounds, "median": med, "steps": rows}), flush=True)
        del trn, A, H32, H16
        torch.cuda.empty_cache()


def epochs(args, data):
    import torch
    from stochastic_gcn_amd.flags import FLAGS
    for P, q in PQ:
        argv = {'gat': RECIPE + FULL + _parts(P, q) + GAT, 'dot': RECIPE + FULL + _parts(P, q) + DOT}
        trn = {k: _trainer(v, data) for k, v in argv.items()}
        wall = {k: [] for k in argv}
        for r in range(args.epoch_rounds + 1):
            for k in argv:
                FLAGS.reset()
                FLAGS.parse(argv[k])                         # (the layers read FLAGS at run time)
                torch.cuda.synchronize()
                t = time.time()
                trn[k].train_epoch()                         # (ends in a device synchronise)
                if r:
                    wall[k].append(time.time() - t)
        print(json.dumps({"what": "part_pull_gat epochs", "P": P, "q": q, "heads": HEADS, "rounds": args.epoch_rounds,
                          "gat_epoch_wall_s": wall['gat'], "dot_epoch_wall_s": wall['dot'],
                          "gat_median_wall_s": float(np.median(wall['gat'])), "dot_median_wall_s": float(np.median(wall['dot'])),
                          "steps_per_epoch": trn['gat'].last_epoch['steps'], "refreshed": trn['gat'].last_epoch['refreshed'],
                          "ratio_gat_to_dot": float(np.median(wall['gat']) / np.median(wall['dot']))}), flush=True)
        del trn
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['launches', 'epochs', 'all'])
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--epoch_rounds', type=int, default=3)
    args = ap.parse_args()
    data = _data()
    if args.what in ('launches', 'all'):
        launches(args, data)
    if args.what in ('epochs', 'all'):
        epochs(args, data)


if __name__ == '__main__':
    main()
