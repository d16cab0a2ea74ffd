#!/usr/bin/env python
"""What the END of a column-sweep launch costs ("the epilogue"; sgcn_spmm_cs.hip cs_epilogue), measured on
two builds of the library inside one process: the tree's own libsgcn.so and another build of it given by --other (the
parent commit's, built from a checkout of that commit and copied aside).  Both run on the SAME plans and operands -- the
plan struct is part of the C ABI -- and alternate window by window; each is autotuned for itself; guard_on is False inside
the windows.  Everything is recorded, nothing is gated.

    python profiles/cs_epilogue_probe.py products --other PATH [--repeats 4] [--iters 40] [--cs-g 0|1|2|4]
        S-Reddit, d = 602: forward (A . X) and backward (A^T . dC) as sustained runs of `iters` fwd + bwd pairs between two
        device events, `repeats` times per build, the builds alternating; then the same products on EMPTY sweeps
        (tile_ptr collapsed to zeros: every wave skips the sweep and runs prologue + epilogue only, unpaced), which is the
        launch's end by itself: (product - fix-up) / launches per launch.
    python profiles/cs_epilogue_probe.py paces --other PATH [--paces 186,188,...] [--repeats 2]
        both builds at the same forced clocks, alternating: where each loses the lock-step
    rocprofv3 --kernel-trace -f csv -d D -- python profiles/cs_epilogue_probe.py run [--other PATH --use other] --pace-fwd P --pace-bwd Q
        `iters` paced products, then `iters` products on empty sweeps, for a kernel trace (a run of its own per build)
    python profiles/cs_epilogue_probe.py kernels --dir D
        the sweep launches of such a trace: the first half of them are the paced products', the second half the empty ones'

Records go to stdout as JSON lines (everything else to stderr)."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 602
CS_ENTRIES = ("sgcn_spmm_cs_f32", "sgcn_spmm_cs_b16")


class LibSwitch(object):
    """ops.lib with the column-sweep entry points of another build of the library while ``use_other`` is set"""

    def __init__(self, base, other_path):
        from stochastic_gcn_amd import _ffi
        self._base, self.use_other = base, False
        self._other = C.CDLL(other_path)
        for name in CS_ENTRIES:
            fn = getattr(self._other, name)
            fn.restype, fn.argtypes = _ffi.SIGNATURES[name]
        assert self._other.sgcn_abi_version() == _ffi.ABI_VERSION, "--other is a build of another ABI"

    def __getattr__(self, name):
        if self.use_other and name in CS_ENTRIES:
            return getattr(self._other, name)
        return getattr(self._base, name)


def _setup(args):
    import torch
    from stochastic_gcn_amd import ops, synthetic
    from profiles.spmm_b16_probe import _guard_off, _operands
    dev = torch.device("cuda:0")
    switch = None
    if args.other:
        switch = ops.lib = LibSwitch(ops.lib, os.path.abspath(args.other))
    n, _, full_adj, *_ = synthetic.reddit_like(with_features=False)
    a, at = full_adj.tocsr(), ops.transpose_host(full_adj)
    G = args.cs_g or ops.ColumnSweepCSR.choose_g(D, a.nnz / max(n, 1), n)
    A, AT = ops.ColumnSweepCSR(a, dev, G=G), ops.ColumnSweepCSR(at, dev, G=G)
    X, dC = _operands(n, D, dev, False)
    out = torch.empty((n, (D + 3) // 4 * 4), device=dev)[:, :D]
    out_t = torch.empty((n, (D + 3) // 4 * 4), device=dev)[:, :D]
    _guard_off(A, AT)
    return dev, switch, A, AT, X, dC, out, out_t, G


class _Empty(object):
    """inside: the plans' sweeps are empty (tile_ptr all zero) and unpaced"""

    def __init__(self, *plans):
        self.plans = plans

    def __enter__(self):
        import torch
        self.saved = [(P.tile_ptr, dict(P.pace)) for P in self.plans]
        for P in self.plans:
            P.tile_ptr = torch.zeros_like(P.tile_ptr)
            P.pace[D] = -1

    def __exit__(self, *exc):
        for P, (tp, pace) in zip(self.plans, self.saved):
            P.tile_ptr = tp
            P.pace.clear()
            P.pace.update(pace)


def _launches(P):
    """sweep launches of one product of plan P at width D (passes x rounds), from the variant string"""
    return int(P.variant(D).split(" x ")[1].split()[0])


def products(args):
    from stochastic_gcn_amd import ops
    from profiles.spmm_b16_probe import _sustained
    dev, switch, A, AT, X, dC, out, out_t, G = _setup(args)
    builds = ["tree"] + (["other"] if switch else [])

    def use(b):
        if switch:
            switch.use_other = b == "other"

    def pair():
        ops.spmm_cs(A, X, out=out)
        ops.spmm_cs(AT, dC, out=out_t)

    tuned = {}
    for b in builds:                         # each build tuned for itself
        use(b)
        bf, bb = A.autotune(X), AT.autotune(dC)
        tuned[b] = dict(fwd_ms=bf[0], fwd_pace=bf[1], bwd_ms=bb[0], bwd_pace=bb[1])
        for P in (A, AT):
            P._guard.clear()
    runs = {b: dict(fwd=[], bwd=[], pair=[]) for b in builds}
    for _ in range(args.repeats):
        for b in builds:                     # the builds alternate inside one process
            use(b)
            A.pace[D], AT.pace[D] = tuned[b]["fwd_pace"], tuned[b]["bwd_pace"]
            runs[b]["fwd"].append(_sustained(lambda: ops.spmm_cs(A, X, out=out), args.iters))
            runs[b]["bwd"].append(_sustained(lambda: ops.spmm_cs(AT, dC, out=out_t), args.iters))
            runs[b]["pair"].append(_sustained(pair, args.iters))
    empty = {b: dict(fwd=[], bwd=[]) for b in builds}
    with _Empty(A, AT):
        for _ in range(args.repeats):
            for b in builds:
                use(b)
                empty[b]["fwd"].append(_sustained(lambda: ops.spmm_cs(A, X, out=out), 4 * args.iters) * 1e3)
                empty[b]["bwd"].append(_sustained(lambda: ops.spmm_cs(AT, dC, out=out_t), 4 * args.iters) * 1e3)
    A.struct(D), AT.struct(D)                 # (makes the plans' per-launch hints)
    for b in builds:
        pair_ms = runs[b]["pair"]
        rec = {"what": "products", "build": b, "graph": "sreddit", "d": D, "G": G, "kernel": A.variant(D),
               "launches_fwd": _launches(A), "launches_bwd": _launches(AT), "nfix": [A.nfix, AT.nfix],
               "heaviest_tile_steps_per_launch": [A._hint.tolist(), AT._hint.tolist()],
               "tuned": tuned[b], "iters": args.iters, "repeats": args.repeats,
               "fwd_ms": runs[b]["fwd"], "bwd_ms": runs[b]["bwd"], "pair_ms": pair_ms,
               "pair_ms_mean": sum(pair_ms) / len(pair_ms), "pair_ms_min": min(pair_ms), "pair_ms_max": max(pair_ms),
               "empty_sweep_product_us": empty[b],
               "empty_sweep_us_per_launch_incl_fixup": {k: min(v) / (_launches(A) if k == "fwd" else _launches(AT))
                                                        for k, v in empty[b].items()}}
        print(json.dumps(rec), flush=True)
    if switch:
        t, o = runs["tree"]["pair"], runs["other"]["pair"]
        width = max(o) - min(o)
        print(json.dumps({"what": "products verdict", "tree_minus_other_ms": sum(t) / len(t) - sum(o) / len(o),
                          "other_min_max": [min(o), max(o)], "tree_min_max": [min(t), max(t)],
                          "gap_over_other_range_width": (min(o) - max(t)) / width if width > 0 else None,
                          "note": "recorded, not a gate"}), flush=True)


def paces(args):
    """both builds at the SAME forced clocks (--paces): where each build's lock-step is lost, apart from what its autotune picks"""
    from stochastic_gcn_amd import ops
    from profiles.spmm_b16_probe import _sustained
    dev, switch, A, AT, X, dC, out, out_t, G = _setup(args)
    builds = ["tree"] + (["other"] if switch else [])

    def pair():
        ops.spmm_cs(A, X, out=out)
        ops.spmm_cs(AT, dC, out=out_t)

    for p in [int(x) for x in args.paces.split(",")]:
        A.pace[D] = AT.pace[D] = p
        ms = {b: [] for b in builds}
        for _ in range(args.repeats):
            for b in builds:
                if switch:
                    switch.use_other = b == "other"
                ms[b].append(_sustained(pair, args.iters))
        print(json.dumps({"what": "paces", "pace": p, "G": G, "iters": args.iters, "pair_ms": ms}), flush=True)


def run(args):
    """only the products (for a profiler around this process): `iters` paced pairs, then `iters` pairs on empty sweeps"""
    import torch
    from stochastic_gcn_amd import ops
    dev, switch, A, AT, X, dC, out, out_t, G = _setup(args)
    if switch:
        switch.use_other = args.use == "other"
    A.pace[D], AT.pace[D] = args.pace_fwd, args.pace_bwd
    for _ in range(args.iters):
        ops.spmm_cs(A, X, out=out)
        ops.spmm_cs(AT, dC, out=out_t)
    torch.cuda.synchronize()
    with _Empty(A, AT):
        for _ in range(args.iters):
            ops.spmm_cs(A, X, out=out)
            ops.spmm_cs(AT, dC, out=out_t)
        torch.cuda.synchronize()
    print(json.dumps({"what": "run", "build": args.use if switch else "tree", "iters": args.iters, "G": G,
                      "pace_fwd": args.pace_fwd, "pace_bwd": args.pace_bwd, "launches": [_launches(A), _launches(AT)],
                      "heaviest_tile_steps_per_launch": [A._hint.tolist(), AT._hint.tolist()]}), flush=True)


def kernels(args):
    """the sweep and fix-up launches of a `run` trace (rocprofv3 --kernel-trace -f csv): first half paced, second half empty"""
    f = glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True)
    rows = list(csv.DictReader(open(f[0])))
    for tag, key in (("sweep", "cs_spmm16"), ("fixup", "cs_fix_kernel")):
        k = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if key in r["Kernel_Name"])
        half = len(k) // 2
        for part, sel in (("paced", k[:half]), ("empty", k[half:])):
            us = sorted((e - s) / 1e3 for s, e in sel)
            gaps = sorted((b[0] - a[1]) / 1e3 for a, b in zip(sel, sel[1:]))
            if us:
                print(json.dumps({"what": "kernel", "dir": args.dir, "kernel": tag, "part": part, "launches": len(us),
                                  "avg_us": sum(us) / len(us), "median_us": us[len(us) // 2], "min_us": us[0], "max_us": us[-1],
                                  "median_gap_to_next_us": gaps[len(gaps) // 2] if gaps else None}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["products", "paces", "run", "kernels"])
    ap.add_argument("--other", default=None, help="another build of libsgcn.so (the parent commit's)")
    ap.add_argument("--use", default="tree", choices=["tree", "other"], help="run: which build multiplies")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--cs-g", type=int, default=0, choices=[0, 1, 2, 4])
    ap.add_argument("--pace-fwd", type=int, default=-1)
    ap.add_argument("--pace-bwd", type=int, default=-1)
    ap.add_argument("--paces", default="186,188,190,192,194,196,198,202")
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    {"products": products, "paces": paces, "run": run, "kernels": kernels}[args.what](args)


if __name__ == "__main__":
    main()
