#!/usr/bin/env python
"""Measurements of --attn_score gat on S-Reddit.

    python profiles/gat_aggregator_probe.py kernels [--d 128] [--heads 1 4] [--rounds 7] [--reps 10]
        per head count, in ONE process in interleaved rounds (device events around `reps` calls of one launch): the five launches
        of the learned scores -- gat_scores, spgat (forward), spgat_bwd_u, spgat_bwd_v, gat_scores_bwd (with dX) -- beside the
        dot-product attention's forward and two-launch backward of the same build and the row SpMM's forward and transposed
        product, on train_adj at the default plan
    python profiles/gat_aggregator_probe.py epochs [--epochs 8]
        the README full-batch recipe with --aggregator attn at --attn_score dot and at gat: the times of `epochs` epochs behind
        one warm epoch
    python profiles/gat_aggregator_probe.py all
        both on one copy of the data

Records go to stdout as JSON lines (everything else to stderr); profiles/gat_aggregator.jsonl keeps them."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from profiles.attn_aggregator_probe import FULL, RECIPE, _data, _trainer  # noqa: E402


def kernels(args, data):
    import torch
    from stochastic_gcn_amd import _ffi, ops
    lib, check = _ffi.lib, _ffi.check
    dev = torch.device('cuda:0')
    a = data[1].tocsr()
    n, d = a.shape[0], args.d
    A = ops.DeviceCSR.from_scipy(a, dev, with_transpose=True)
    At = A.transpose
    rng = np.random.RandomState(0)
    x = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev)
    out, dx = torch.empty_like(x), torch.empty_like(x)
    slope = 0.2
    for H in args.heads:
        av = torch.from_numpy((rng.standard_normal((2, d)) * (2.0 / (2 + d)) ** 0.5).astype(np.float32)).to(dev)
        scale = float(d // H) ** -0.5
        S = ops.gat_scores(x, av, heads=H)
        Ut, Vt = S[:, :H], S[:, H:]
        gat_out, gat_lse = ops.spgat(A, x, Ut, Vt, slope=slope, heads=H)
        dB, dU, dV, delta = ops.spgat_bwd(A, At, x, Ut, Vt, g, gat_out, gat_lse, slope=slope, heads=H)
        att, lse = ops.spattn(A, x, scale=scale, heads=H)
        st = ops._stream

        def bwd_u():
            p = A.plan.struct(8)
            check(lib.sgcn_spgat_csr_bwd_u_f32(A.rowptr.data_ptr(), A.col.data_ptr(), n, n, d, H, 1.0, 0, Ut.data_ptr(), 2 * H,
                                               Vt.data_ptr(), 2 * H, x.data_ptr(), d, slope, g.data_ptr(), d, gat_out.data_ptr(), d,
                                               gat_lse.data_ptr(), delta.data_ptr(), dU.data_ptr(), C.byref(p), st()))

        def bwd_v():
            p = At.plan.struct((d + 3) // 4 * 4 + 8)
            check(lib.sgcn_spgat_csr_bwd_v_f32(At.rowptr.data_ptr(), At.col.data_ptr(), n, n, d, H, 1.0, 0, Ut.data_ptr(), 2 * H,
                                               Vt.data_ptr(), 2 * H, x.data_ptr(), d, slope, g.data_ptr(), d, gat_lse.data_ptr(),
                                               delta.data_ptr(), dB.data_ptr(), d, dV.data_ptr(), None, 0, 0, C.byref(p), st()))
        calls = {"spmm_fwd": lambda: ops.spmm(A, x, out=out),
                 "spmm_bwd": lambda: ops.spmm(At, g, out=dx),
                 "dot_fwd": lambda: ops.spattn(A, x, scale=scale, out=out, heads=H),
                 "dot_bwd": lambda: ops.spattn_bwd(A, At, x, None, g, att, lse, scale, heads=H),
                 "gat_scores": lambda: ops.gat_scores(x, av, heads=H),
                 "gat_fwd": lambda: ops.spgat(A, x, Ut, Vt, slope=slope, out=out, heads=H),
                 "gat_bwd_u": bwd_u,
                 "gat_bwd_v": bwd_v,
                 "gat_scores_bwd": lambda: ops.gat_scores_bwd(x, av, dU, dV, dx=dx, heads=H)}
        for f in calls.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / args.reps)
        rec = {"what": "gat kernels", "matrix": "s-reddit train_adj", "rows": n, "nnz": int(a.nnz), "d": d, "heads": H,
               "slope": slope, "plan_T": "default", "split_rows": A.plan.nfix, "split_rows_T": At.plan.nfix,
               "rounds": args.rounds, "reps": args.reps}
        for k, v in ms.items():
            rec[k + "_ms_median"], rec[k + "_ms_min"] = float(np.median(v)), float(min(v))
        med = lambda k: rec[k + "_ms_median"]
        rec["gat_fwd_total_ms_median"] = med("gat_scores") + med("gat_fwd")
        rec["gat_bwd_total_ms_median"] = med("gat_bwd_u") + med("gat_bwd_v") + med("gat_scores_bwd")
        rec["fwd_over_dot"] = rec["gat_fwd_total_ms_median"] / med("dot_fwd")
        rec["bwd_over_dot"] = rec["gat_bwd_total_ms_median"] / med("dot_bwd")
        print(json.dumps(rec), flush=True)


def epochs(args, data):
    import torch
    for score in ("dot", "gat", "dot", "gat"):
        trn = _trainer(RECIPE + FULL + ['--aggregator', 'attn', '--attn_score', score, '--epochs', str(args.epochs)], data)
        trn.train_epoch()                                      # (builds the transpose)
        torch.cuda.synchronize()
        wall, dev = [], []
        for _ in range(args.epochs):
            t = time.time()
            trn.train_epoch()                                  # (ends in a device synchronise)
            wall.append(time.time() - t)
            dev.append(trn.train_model.run_t)
        m = trn.train_static.matrix
        print(json.dumps({"what": "full_batch epochs", "aggregator": "attn", "attn_score": score, "kernel": m.kernel,
                          "epochs": args.epochs, "epoch_wall_s": wall, "min_wall_s": min(wall),
                          "median_wall_s": float(np.median(wall)), "max_wall_s": max(wall), "min_device_s": min(dev),
                          "static_setup_s": trn.static_setup_s, "nnz": m.nnz}), flush=True)
        del trn, m
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "epochs", "all"])
    ap.add_argument("--heads", type=int, nargs='+', default=[1, 4])
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=8)
    args = ap.parse_args()
    data = _data()
    for what in (["kernels", "epochs"] if args.what == "all" else [args.what]):
        {"kernels": kernels, "epochs": epochs}[what](args, data)


if __name__ == "__main__":
    main()
