#!/usr/bin/env python
"""Measurements of the bfloat16 feature table (--feature_dtype bf16; include/sgcn.h
sgcn_gemm_mb16_a16).  Everything is recorded, nothing is gated.  One box, one session: the two table types alternate inside
one process, every shape is warmed first, times are device events.

    python profiles/feature_bf16_probe.py gemms [--repeats 4] [--iters 20]
        the two products that read the table (NN forward, TN weight gradient) at the recipe's first-layer shape
        232,965 x 1,204 x 128: sgcn_gemm_mb16_f32 on the fp32 table against sgcn_gemm_mb16_a16 on the bfloat16 one, beside
        the floor max(bytes / 6.3 TB/s, flops / 2.5 PF) of each and the term that binds; the two results are ASSERTED to be
        the same bits (the fp32 table holds the widened bfloat16 values)
    python profiles/feature_bf16_probe.py epochs --feature_dtype fp32|bf16|both [--epochs 8] [--rounds 2] [--tag this]
        the README full-batch recipe with --dense_dtype bf16 (--full_batch --test_full_batch): epoch and evaluation times
        with their run-to-run spread and max_memory_allocated.  `--feature_dtype fp32` passes nothing this change added, so
        the same file times the parent commit from its own checkout (--tag parent)
    python profiles/feature_bf16_probe.py convergence [--seeds 1,2,3,4,5] [--epochs 30]
        per seed, both table types: validation loss and test accuracy, the per-seed difference beside the seed-to-seed
        spread; no threshold

Records go to stdout as JSON lines (everything else to stderr)."""
import argparse
import contextlib
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RECIPE = ['--dataset', 's-reddit', '--normalization', 'graphsage', '--weight_decay', '0', '--dropout', '0.2', '--layer_norm',
          '--hidden1', '128', '--num_fc_layers', '2']
MODE = ['--full_batch', '--test_full_batch', '--full_batch_kernel', 'cs', '--dense_dtype', 'bf16']
N_ROWS, FAN_IN, FAN_OUT = 232965, 1204, 128
HBM_BPS, BF16_FLOPS = 6.3e12, 2.5e15


def _sustained(fn, iters, warm=3):
    import torch
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def _floor(M, N, K, a_bytes, ws_floats):
    """(ms, binding term, bytes, flops) of max(bytes / HBM, flops / bf16 peak): A (a_bytes per element) and B read once, C
    written once, the split-K workspace written and read once"""
    byts = float(a_bytes) * M * K + 4.0 * (K * N + M * N + 2 * ws_floats)
    flops = 2.0 * M * N * K
    tb, tf = byts / HBM_BPS, flops / BF16_FLOPS
    return max(tb, tf) * 1e3, ("bytes" if tb >= tf else "flops"), byts, flops


def gemms(args):
    import torch
    from stochastic_gcn_amd import ops
    from stochastic_gcn_amd._ffi import lib
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    n, fin, fout = args.rows, FAN_IN, FAN_OUT
    x16 = ops.operand_round(torch.randn((n, fin), device=dev, generator=g))
    x32 = ops.history_widen(x16)                     # the fp32 table holding the same values
    assert x16.dtype == torch.bfloat16 and x16.stride(0) == (fin + 7) // 8 * 8 and x32.dtype == torch.float32
    W = torch.randn((fin, fout), device=dev, generator=g) / fin ** 0.5
    gr = torch.randn((n, fout), device=dev, generator=g)
    drop = ops.Drop(0.8, 12345)
    forms = (("NN", (n, fout, fin), lambda x, o, kw: ops.gemm_bf16(x, W, out=o, **kw), (n, fout)),
             ("TN", (fin, fout, n), lambda x, o, kw: ops.gemm_bf16(x, gr, out=o, trans_a=True, **kw), (fin, fout)))
    for form, (M, N, K), call, oshape in forms:
        for masked in (False, True):
            kw = dict(drop_a=drop) if masked else {}
            o32, o16 = torch.zeros(oshape, device=dev), torch.zeros(oshape, device=dev)
            call(x32, o32, kw)
            call(x16, o16, kw)
            torch.cuda.synchronize()
            same = bool(torch.equal(o32.view(torch.int32), o16.view(torch.int32)))
            assert same, "%s (mask %s): the bfloat16 table does not give the bits of the fp32 one" % (form, masked)
            runs = {"fp32": [], "bf16": []}
            for _ in range(args.repeats):
                for t, x, o in (("fp32", x32, o32), ("bf16", x16, o16)):        # the types alternate inside one process
                    runs[t].append(_sustained(lambda: call(x, o, kw), args.iters))
            ws = int(lib.sgcn_gemm_mb16_ws_floats(int(form == "TN"), 0, M, N, K))
            f32 = _floor(M, N, K, 4, ws)
            f16 = _floor(M, N, K, 2 * x16.stride(0) / float(fin), ws)            # (the pitch padding is read too)
            m32, m16 = min(runs["fp32"]), min(runs["bf16"])
            print(json.dumps({"what": "first-layer gemm", "form": form, "M": M, "N": N, "K": K, "drop_a": masked,
                              "fp32_table_ms": runs["fp32"], "bf16_table_ms": runs["bf16"], "fp32_table_ms_best": m32,
                              "bf16_table_ms_best": m16, "bf16_over_fp32": m16 / m32,
                              "bf16_faster": bool(max(runs["bf16"]) < min(runs["fp32"])),
                              "fp32_floor_ms": f32[0], "fp32_floor_binds": f32[1], "fp32_bytes": f32[2],
                              "bf16_floor_ms": f16[0], "bf16_floor_binds": f16[1], "bf16_bytes": f16[2], "flops": f16[3],
                              "fp32_over_floor": m32 / f32[0], "bf16_over_floor": m16 / f16[0], "splitk_ws_floats": ws,
                              "bits_equal": same, "iters": args.iters, "repeats": args.repeats}), flush=True)


def _trainer(argv, data=None):
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.train import Trainer
    FLAGS.reset()
    FLAGS.parse(argv)
    with contextlib.redirect_stdout(sys.stderr):
        return Trainer(data=data, verbose=False)


def _data():
    """the loader's tuple with the two pre-processing products filled in once (every trainer of the process shares them)"""
    import torch
    from stochastic_gcn_amd import train
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.utils import load_data
    FLAGS.reset()
    FLAGS.parse(RECIPE)
    with contextlib.redirect_stdout(sys.stderr):
        d = list(load_data(FLAGS.dataset))
        if d[4] is None:
            d[4], d[5] = train.pp_products(d[1], d[2], d[3], torch.device("cuda:0"))
    return tuple(d)


def _feature_flag(t):
    """(a checkout without the flag -- the parent commit -- is timed with `--feature_dtype fp32`: nothing is passed)"""
    return ['--feature_dtype', t] if t != "fp32" else []


def epochs(args):
    import torch
    data = _data()
    types_ = ["fp32", "bf16"] if args.feature_dtype == "both" else [args.feature_dtype]
    for rnd in range(args.rounds):
        for t in types_:
            gc.collect()                                         # (a finished trainer is garbage with cycles)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()                 # the shared pre-processing products of this process
            trn = _trainer(RECIPE + MODE + ['--epochs', str(args.epochs)] + _feature_flag(t), data)
            torch.cuda.synchronize()
            setup_peak, resident = torch.cuda.max_memory_allocated(), torch.cuda.memory_allocated()
            times, dev_times, evals = [], [], []
            for e in range(args.epochs + 1):
                if e == 1:                                       # steady state: behind the first epoch's autotunes
                    torch.cuda.reset_peak_memory_stats()
                t0 = time.time()
                trn.train_epoch()
                times.append(time.time() - t0)
                dev_times.append(trn.train_model.run_t)
                trn.train_model.run_t = 0.0
                t0 = time.time()
                res = trn.evaluate(trn.val_d)
                torch.cuda.synchronize()
                evals.append(time.time() - t0)
            m = trn.train_static.matrix
            tabs = [trn.train_model.features_dev, trn.test_model.features_dev]
            print(json.dumps({"what": "full_batch epochs", "tag": args.tag, "round": rnd, "feature_dtype": t, "kernel": m.kernel,
                              "N": m.shape[0], "nnz": m.nnz, "first_epoch_s": times[0], "epoch_times_s": times[1:],
                              "epoch_time_s": min(times[1:]), "epoch_time_spread_s": max(times[1:]) - min(times[1:]),
                              "device_epoch_s": dev_times[1:], "device_epoch_ms_best": min(dev_times[1:]) * 1e3,
                              "eval_times_s": evals[1:], "eval_time_s": min(evals[1:]),
                              "table_dtypes": [str(x.dtype) for x in tabs],
                              "table_bytes": [int(x.stride(0)) * int(x.shape[0]) * x.element_size() for x in tabs],
                              "shared_products_bytes": base, "resident_after_setup_bytes": resident,
                              "max_memory_allocated_setup": setup_peak,
                              "max_memory_allocated_steady": torch.cuda.max_memory_allocated(),
                              "steady_minus_shared_bytes": torch.cuda.max_memory_allocated() - base,
                              "train_loss_last": float(trn.avg_loss.mean()), "val_loss_last": float(res[0])}), flush=True)
            del trn, tabs, m
            torch.cuda.empty_cache()


def convergence(args):
    import torch
    seeds = [int(s) for s in args.seeds.split(",")]
    base = RECIPE + MODE + ['--epochs', str(args.epochs), '--early_stopping', str(args.epochs)]
    data = _data()
    val, acc = {"fp32": {}, "bf16": {}}, {"fp32": {}, "bf16": {}}
    for seed in seeds:
        for t in ("fp32", "bf16"):
            t0 = time.time()
            trn = _trainer(base + _feature_flag(t) + ['--seed', str(seed)], data)
            with contextlib.redirect_stdout(sys.stderr):
                trn.SGDTrain()
            v, res = trn.evaluate(trn.val_d), trn.evaluate(trn.test_d)
            val[t][seed], acc[t][seed] = v[0], res[1]
            print(json.dumps({"what": "convergence", "seed": seed, "feature_dtype": t, "epochs": args.epochs, "val_loss": v[0],
                              "val_acc": v[1], "test_loss": res[0], "test_acc": res[1], "micro_f1": res[2], "macro_f1": res[3],
                              "n_test": int(len(trn.test_d)), "wall_s": round(time.time() - t0, 1)}), flush=True)
            del trn
            torch.cuda.empty_cache()
    fv, fa = [val["fp32"][s] for s in seeds], [acc["fp32"][s] for s in seeds]
    for s in seeds:
        print(json.dumps({"what": "convergence difference", "seed": s,
                          "val_loss_bf16_minus_fp32": val["bf16"][s] - val["fp32"][s], "fp32_val_loss_seed_spread": max(fv) - min(fv),
                          "test_acc_bf16_minus_fp32": acc["bf16"][s] - acc["fp32"][s], "fp32_test_acc_seed_spread": max(fa) - min(fa),
                          "note": "recorded, no threshold"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["gemms", "epochs", "convergence"])
    ap.add_argument("--feature_dtype", default="both", choices=["fp32", "bf16", "both"])
    ap.add_argument("--rows", type=int, default=N_ROWS)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--tag", default="this")
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--seeds", default="1,2,3,4,5")
    args = ap.parse_args()
    if args.epochs is None:
        args.epochs = 30 if args.what == "convergence" else 8
    {"gemms": gemms, "epochs": epochs, "convergence": convergence}[args.what](args)


if __name__ == "__main__":
    main()
