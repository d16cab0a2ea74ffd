#!/usr/bin/env python
"""Measurements of --full_batch_part_pull with --aggregator attn on S-Reddit train_adj parts: P = 32, q = 4,
d = 128, heads 1 and 4.

    python profiles/part_pull_attn_probe.py [--steps 6] [--rounds 7]
        per step of epoch 1 and per heads, by device events (medians over the rounds after one warm round, the launches
        alternating inside a round):
          the pull forward (ops.spattn_pull) and the pull bwd_q (ops.spattn_pull_bwd_q) on an fp32 and on a bfloat16 table;
          next to them what the same step runs WITHOUT stored rows on the induced block A[S, S] with its plan: the forward
          (ops.spattn) and the whole backward (ops.spattn_bwd: bwd_q + bwd_kv), and the block's bwd_kv alone
          (ops.spattn_pull_bwd_kv -- the launch both backwards share), so that block bwd_q = backward - bwd_kv;
          the step's rows: n, all stored entries, in-part entries, the longest and the mean selected row.

Records go to stdout as JSON lines (everything else to stderr); profiles/part_pull_attn.jsonl is that output."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from full_batch_parts_probe import FULL, RECIPE, _data, _parts, _trainer      # noqa: E402
from part_history_probe import _events                                         # noqa: E402

P, Q, HEADS = 32, 4, (1, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    import torch
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd.flags import FLAGS
    data = _data()
    for heads in HEADS:
        trn = _trainer(RECIPE + FULL + _parts(P, Q) + ['--full_batch_part_pull', '--aggregator', 'attn', '--attn_heads', str(heads)],
                       data)
        A, dev, d = trn.train_csr, trn.device, int(FLAGS.hidden1)
        N = int(A.shape[0])
        scale = float(d // heads) ** -0.5
        g = torch.Generator().manual_seed(1)
        H32 = (0.5 * torch.randn((N, d), generator=g)).to(dev)
        H16 = ops.history_assign(ops.history_alloc(N, d, dev, bf16=True), H32)
        rows = []
        for ids in trn.part_schedule.epoch(1)[:args.steps]:
            batch = trn.part_batch(ids)
            m = batch.matrix
            n, ids_dev, vmap, blk, blk_t = len(ids), batch.ids_dev, m.map, m.rows_csr, m.transpose.rows_csr
            x = (0.5 * torch.randn((n, d), generator=g)).to(dev)
            gr = torch.randn((n, d), generator=g).to(dev)
            out32, lse32 = ops.spattn_pull(A, ids_dev, vmap, x, H32, scale, heads=heads)
            out16, lse16 = ops.spattn_pull(A, ids_dev, vmap, x, H16, scale, heads=heads)
            outb, lseb = ops.spattn(blk, x, scale=scale, heads=heads)
            dq, delta = ops.spattn_pull_bwd_q(A, ids_dev, vmap, x, H32, gr, out32, lse32, scale, heads=heads)
            launches = dict(
                pull_fwd_f32_ms=lambda: ops.spattn_pull(A, ids_dev, vmap, x, H32, scale, out=out32, heads=heads),
                pull_fwd_h16_ms=lambda: ops.spattn_pull(A, ids_dev, vmap, x, H16, scale, out=out16, heads=heads),
                block_fwd_ms=lambda: ops.spattn(blk, x, scale=scale, out=outb, heads=heads),
                pull_bwd_q_f32_ms=lambda: ops.spattn_pull_bwd_q(A, ids_dev, vmap, x, H32, gr, out32, lse32, scale, heads=heads),
                pull_bwd_q_h16_ms=lambda: ops.spattn_pull_bwd_q(A, ids_dev, vmap, x, H16, gr, out16, lse16, scale, heads=heads),
                block_bwd_ms=lambda: ops.spattn_bwd(blk, blk_t, x, None, gr, outb, lseb, scale, heads=heads),
                block_bwd_kv_ms=lambda: ops.spattn_pull_bwd_kv(blk_t, x, gr, lse32, delta, dq, scale, heads=heads))
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
                       mean_row=float(lens.mean()), finite=bool(torch.isfinite(out32).all() and torch.isfinite(dq).all()))
            rows.append(rec)
            print("heads %d step: %s" % (heads, rec), file=sys.stderr, flush=True)
        med = {k: float(np.median([r[k] for r in rows])) for k in rows[0] if k != 'finite'}
        med['longest_row'] = int(max(r['longest_row'] for r in rows))
        print(json.dumps({"what": "part_pull_attn", "P": P, "q": Q, "d": d, "heads": heads, "steps_measured": len(rows),
                          "rounds": args.rounds, "median": med, "steps": rows}), flush=True)
        del trn, A, H32, H16
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
