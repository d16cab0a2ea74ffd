#!/usr/bin/env python
"""What a column-sweep launch costs OFF its clock -- the prologue's load chain and the output burst at its end (DESIGN.md
3.2, "The end of a launch"; sgcn_spmm_cs.hip cs_store / cs_epilogue and the DICT prologue) -- measured on SEVERAL builds of
the library inside one process: the tree's own libsgcn.so and any number of others given as --other NAME=PATH (the parent
commit's build, and builds of this tree with -DSGCN_CS_STORE_C=n / -DSGCN_CS_STORE_WS=n: 0 plain, 1 nt, 2 sc1, 3 sc0 sc1).
All run on the SAME plans and operands -- the plan struct is part of the C ABI -- and alternate window by window; each is
autotuned for itself; the lost-lock guard is off inside the windows.  Everything is recorded, nothing is gated.  The
pattern is profiles/cs_epilogue_probe.py's, whose plumbing this file uses.

    python profiles/cs_boundary_probe.py products --other parent=PATH [--other c_sc1=PATH ...] [--repeats 4] [--iters 40]
        S-Reddit, d = 602: fwd (A . X) + bwd (A^T . dC) pairs as sustained runs of `iters` pairs between two device events,
        `repeats` windows per build, the builds alternating; then the same products on EMPTY sweeps (tile_ptr collapsed to
        zeros: prologue + epilogue only, unpaced), and the fix-up's share of those by itself.
    python profiles/cs_boundary_probe.py paces --other parent=PATH [--paces 186,188,...] [--repeats 2]
        every build at the same forced clocks, alternating: where each loses the lock-step
    rocprofv3 --kernel-trace --stats -d D -- python profiles/cs_boundary_probe.py run [--other NAME=PATH --use NAME] --pace-fwd P --pace-bwd Q
        `iters` paced products, then `iters` products on empty sweeps, for a kernel trace or a counter pass (a run of its
        own per build and per kind of collection)
    python profiles/cs_boundary_probe.py kernels --dir D
        the sweep launches of such a trace (profiles/cs_epilogue_probe.py kernels)

Records go to stdout as JSON lines (everything else to stderr); kept in profiles/cs_boundary_probe.jsonl."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from profiles.cs_epilogue_probe import CS_ENTRIES, D, _Empty, _launches, kernels  # noqa: E402


class LibSwitch(object):
    """ops.lib with the column-sweep entry points of the build named by ``use`` ("tree": the tree's own)"""

    def __init__(self, base, others):
        from stochastic_gcn_amd import _ffi
        self._base, self.use, self._others = base, "tree", {}
        for name, path in others:
            lib = C.CDLL(os.path.abspath(path))
            for entry in CS_ENTRIES:
                fn = getattr(lib, entry)
                fn.restype, fn.argtypes = _ffi.SIGNATURES[entry]
            assert lib.sgcn_abi_version() == _ffi.ABI_VERSION, "%s is a build of another ABI" % path
            self._others[name] = lib

    def __getattr__(self, name):
        if self.use != "tree" and name in CS_ENTRIES:
            return getattr(self._others[self.use], name)
        return getattr(self._base, name)


def _setup(args):
    import torch
    from stochastic_gcn_amd import ops, synthetic
    from profiles.spmm_b16_probe import _guard_off, _operands
    dev = torch.device("cuda:0")
    others = [o.split("=", 1) for o in args.other]
    assert all(len(o) == 2 and o[0] != "tree" for o in others), "--other NAME=PATH"
    switch = ops.lib = LibSwitch(ops.lib, others)
    n, _, full_adj, *_ = synthetic.reddit_like(with_features=False)
    a, at = full_adj.tocsr(), ops.transpose_host(full_adj)
    G = args.cs_g or ops.ColumnSweepCSR.choose_g(D, a.nnz / max(n, 1), n)
    A, AT = ops.ColumnSweepCSR(a, dev, G=G), ops.ColumnSweepCSR(at, dev, G=G)
    X, dC = _operands(n, D, dev, args.bf16)
    out = torch.empty((n, (D + 3) // 4 * 4), device=dev)[:, :D]
    out_t = torch.empty((n, (D + 3) // 4 * 4), device=dev)[:, :D]
    _guard_off(A, AT)
    builds = [b for b in ["tree"] + [o[0] for o in others] if b not in args.skip]
    return switch, builds, A, AT, X, dC, out, out_t, G


def _pace_of(P, args):
    return P.pace_b16 if args.bf16 else P.pace


def products(args):
    from stochastic_gcn_amd import ops
    from profiles.spmm_b16_probe import _sustained
    switch, builds, A, AT, X, dC, out, out_t, G = _setup(args)

    def pair():
        ops.spmm_cs(A, X, out=out)
        ops.spmm_cs(AT, dC, out=out_t)

    tuned = {}
    for b in builds:                         # each build tuned for itself
        switch.use = b
        bf, bb = A.autotune(X), AT.autotune(dC)
        tuned[b] = dict(fwd_ms=bf[0], fwd_pace=bf[1], bwd_ms=bb[0], bwd_pace=bb[1])
        for P in (A, AT):
            P._guard.clear()
    runs = {b: [] for b in builds}
    for _ in range(args.repeats):
        for b in builds:                     # the builds alternate inside one process
            switch.use = b
            _pace_of(A, args)[D], _pace_of(AT, args)[D] = tuned[b]["fwd_pace"], tuned[b]["bwd_pace"]
            runs[b].append(_sustained(pair, args.iters))
    empty = {b: [] for b in builds}
    with _Empty(A, AT):
        if args.bf16:
            A.pace_b16[D] = AT.pace_b16[D] = -1
        for _ in range(args.repeats):
            for b in builds:
                switch.use = b
                empty[b].append(_sustained(pair, 4 * args.iters) * 1e3)
    A.struct(D), AT.struct(D)                 # (makes the plans' per-launch hints)
    launches = _launches(A) + _launches(AT)
    for b in builds:
        ms = runs[b]
        print(json.dumps({"what": "products", "build": b, "graph": "sreddit", "d": D, "G": G, "bf16": args.bf16,
                          "kernel": A.variant(D), "launches_per_pair": launches, "nfix": [A.nfix, AT.nfix],
                          "heaviest_tile_steps_per_launch": [A._hint.tolist(), AT._hint.tolist()],
                          "tuned": tuned[b], "iters": args.iters, "repeats": args.repeats, "pair_ms": ms,
                          "pair_ms_mean": sum(ms) / len(ms), "pair_ms_min": min(ms), "pair_ms_max": max(ms),
                          "empty_pair_us": empty[b],
                          "empty_sweep_us_per_launch_incl_fixup": min(empty[b]) / launches}), flush=True)
    if "parent" in builds:
        o = runs["parent"]
        width = max(o) - min(o)
        for b in builds:
            if b != "parent":
                t = runs[b]
                print(json.dumps({"what": "products verdict", "build": b,
                                  "minus_parent_ms": sum(t) / len(t) - sum(o) / len(o),
                                  "parent_min_max": [min(o), max(o)], "min_max": [min(t), max(t)],
                                  "every_run_below_parents_fastest": max(t) < min(o),
                                  "mean_gap_over_parent_range_width": (sum(o) / len(o) - sum(t) / len(t)) / width if width > 0 else None,
                                  "empty_pair_us_minus_parent": min(empty[b]) - min(empty["parent"]),
                                  "note": "recorded, not a gate"}), flush=True)


def paces(args):
    """every build at the SAME forced clocks (--paces): where each build's lock-step is lost, apart from what its autotune picks"""
    from stochastic_gcn_amd import ops
    from profiles.spmm_b16_probe import _sustained
    switch, builds, A, AT, X, dC, out, out_t, G = _setup(args)

    def pair():
        ops.spmm_cs(A, X, out=out)
        ops.spmm_cs(AT, dC, out=out_t)

    for p in [int(x) for x in args.paces.split(",")]:
        _pace_of(A, args)[D] = _pace_of(AT, args)[D] = p
        ms = {b: [] for b in builds}
        for _ in range(args.repeats):
            for b in builds:
                switch.use = b
                ms[b].append(_sustained(pair, args.iters))
        print(json.dumps({"what": "paces", "pace": p, "G": G, "bf16": args.bf16, "iters": args.iters, "pair_ms": ms}), flush=True)


def run(args):
    """only the products (for a profiler around this process): `iters` paced pairs, then `iters` pairs on empty sweeps"""
    import torch
    from stochastic_gcn_amd import ops
    switch, builds, A, AT, X, dC, out, out_t, G = _setup(args)
    switch.use = args.use
    _pace_of(A, args)[D], _pace_of(AT, args)[D] = args.pace_fwd, args.pace_bwd
    for _ in range(args.iters):
        ops.spmm_cs(A, X, out=out)
        ops.spmm_cs(AT, dC, out=out_t)
    torch.cuda.synchronize()
    with _Empty(A, AT):
        if args.bf16:
            A.pace_b16[D] = AT.pace_b16[D] = -1
        for _ in range(args.iters):
            ops.spmm_cs(A, X, out=out)
            ops.spmm_cs(AT, dC, out=out_t)
        torch.cuda.synchronize()
    print(json.dumps({"what": "run", "build": args.use, "iters": args.iters, "G": G, "bf16": args.bf16,
                      "pace_fwd": args.pace_fwd, "pace_bwd": args.pace_bwd, "launches": [_launches(A), _launches(AT)],
                      "heaviest_tile_steps_per_launch": [A._hint.tolist(), AT._hint.tolist()]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["products", "paces", "run", "kernels"])
    ap.add_argument("--other", action="append", default=[], help="NAME=PATH: another build of libsgcn.so (parent=... is the yardstick)")
    ap.add_argument("--skip", action="append", default=[], help="a build to leave out of the windows (e.g. tree)")
    ap.add_argument("--use", default="tree", help="run: which build multiplies")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--cs-g", type=int, default=0, choices=[0, 1, 2, 4])
    ap.add_argument("--bf16", action="store_true", help="bfloat16 operands (the _b16 entry and its clock)")
    ap.add_argument("--pace-fwd", type=int, default=-1)
    ap.add_argument("--pace-bwd", type=int, default=-1)
    ap.add_argument("--paces", default="186,188,190,192,194,196,198,202")
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    {"products": products, "paces": paces, "run": run, "kernels": kernels}[args.what](args)


if __name__ == "__main__":
    main()
