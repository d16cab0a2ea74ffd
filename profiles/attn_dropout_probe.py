#!/usr/bin/env python
"""Measurements of --attn_dropout on S-Reddit: the three launches of attention with dropout on the coefficients
beside the launches without it -- this tree's and, with --parent_lib, those of ANOTHER build of libsgcn.so (the commit before
the dropout kernels existed), loaded into the same process.

    python profiles/attn_dropout_probe.py kernels [--parent_lib PATH] [--shapes 128:1 128:4 602:1 512:4] [--keep 0.8]
                                                  [--rounds 7] [--reps 10]
        per shape d:H, in ONE process in interleaved rounds (device events around `reps` calls of one launch): forward, bwd_q
        and bwd_kv through  parent  sgcn_spattn_mh_csr_* of --parent_lib,  off  the same exports of this tree (the flag-off
        path),  drop  sgcn_spattn_drop_csr_* at --keep.  The outputs of `off` and `parent` are compared bit for bit.
    python profiles/attn_dropout_probe.py names [--d 128] [--heads 1]
        one forward and one backward with and without dropout and nothing else: the run to put under a kernel trace

Records go to stdout as JSON lines (everything else to stderr)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from profiles.attn_aggregator_probe import _data          # noqa: E402


def _bind(path):
    """another build's three multi-head exports, with this tree's signatures"""
    from stochastic_gcn_amd import _ffi
    lib = C.CDLL(path)
    for name in ("sgcn_spattn_mh_csr_f32", "sgcn_spattn_mh_csr_bwd_q_f32", "sgcn_spattn_mh_csr_bwd_kv_f32"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ffi.SIGNATURES[name]
    return lib


def _launches(lib, A, At, x, g, d, H, scale, drop):
    """{name: (callable, outputs)} of the three launches on buffers of their own, every table on the 16-byte pitch of x"""
    import torch
    from stochastic_gcn_amd.ops import _stream
    M = A.shape[0]
    ld = x.stride(0)
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=x.device)       # noqa: E731
    Cf, lse, delta, dq, dx = new(M, ld), new(M, H), new(M, H), new(M, ld), new(M, ld)
    extra = drop if drop else ()
    pre = "sgcn_spattn_drop_csr_" if drop else "sgcn_spattn_mh_csr_"
    fwd, bq, bkv = (getattr(lib, pre + s) for s in ("f32", "bwd_q_f32", "bwd_kv_f32"))
    ref = lambda p: C.byref(p) if p is not None else None                       # noqa: E731
    pf = A.plan.struct((d + 3) // 4 * 4 + 4 * H) if A.plan is not None else None
    pb = A.plan.struct(d) if A.plan is not None else None
    pt = At.plan.struct(d) if At.plan is not None else None
    ap, ac, tp, tc = A.rowptr.data_ptr(), A.col.data_ptr(), At.rowptr.data_ptr(), At.col.data_ptr()
    xp, gp = x.data_ptr(), g.data_ptr()

    def chk(rc):
        assert rc == 0, rc
    calls = {
        "fwd": lambda: chk(fwd(ap, ac, M, M, d, H, *extra, xp, ld, xp, ld, scale, Cf.data_ptr(), ld, lse.data_ptr(), ref(pf), _stream())),
        "bwd_q": lambda: chk(bq(ap, ac, M, M, d, H, *extra, xp, ld, xp, ld, scale, gp, ld, Cf.data_ptr(), ld, lse.data_ptr(),
                                delta.data_ptr(), dq.data_ptr(), ld, None, 0, 0, ref(pb), _stream())),
        "bwd_kv": lambda: chk(bkv(tp, tc, M, M, d, H, *extra, xp, ld, xp, ld, scale, gp, ld, lse.data_ptr(), delta.data_ptr(),
                                  dx.data_ptr(), ld, dq.data_ptr(), ld, M, ref(pt), _stream())),
    }
    return calls, dict(C=Cf, lse=lse, delta=delta, dq=dq, dx=dx)


def kernels(args, data):
    import torch
    from stochastic_gcn_amd import _ffi, ops
    dev = torch.device('cuda:0')
    a = data[1].tocsr()
    n = a.shape[0]
    A = ops.DeviceCSR.from_scipy(a, dev, with_transpose=True)
    parent = _bind(args.parent_lib) if args.parent_lib else None
    key = ops.attn_key(1, 3, 0)
    for shape in args.shapes:
        d, H = (int(v) for v in shape.split(":"))
        rng = np.random.RandomState(0)
        pitch = (d + 3) // 4 * 4                            # (602 columns: on 604 floats, as StaticMatrix stages them)
        x = torch.from_numpy(rng.standard_normal((n, pitch)).astype(np.float32)).to(dev)
        g = torch.from_numpy(rng.standard_normal((n, pitch)).astype(np.float32)).to(dev)
        scale = float(d // H) ** -0.5
        sets = {"off": _launches(_ffi.lib, A, A.transpose, x, g, d, H, scale, None),
                "drop": _launches(_ffi.lib, A, A.transpose, x, g, d, H, scale, (args.keep, key))}
        if parent is not None:
            sets["parent"] = _launches(parent, A, A.transpose, x, g, d, H, scale, None)
        for calls, _ in sets.values():                      # warm up, in the order the launches depend on each other
            for _ in range(3):
                for k in ("fwd", "bwd_q", "bwd_kv"):
                    calls[k]()
        torch.cuda.synchronize()
        ms = {(s, k): [] for s in sets for k in ("fwd", "bwd_q", "bwd_kv")}
        for _ in range(args.rounds):
            for k in ("fwd", "bwd_q", "bwd_kv"):
                for s, (calls, _) in sets.items():          # the builds alternate inside a round
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.reps):
                        calls[k]()
                    e1.record()
                    e1.synchronize()
                    ms[(s, k)].append(e0.elapsed_time(e1) / args.reps)
        rec = {"what": "attn_dropout kernels", "matrix": "s-reddit train_adj", "rows": n, "nnz": int(a.nnz), "d": d, "heads": H,
               "pitch": pitch, "keep": args.keep, "plan_T": "default", "split_rows": A.plan.nfix, "split_rows_T": A.transpose.plan.nfix,
               "rounds": args.rounds, "reps": args.reps, "parent_lib": bool(parent)}
        for (s, k), v in ms.items():
            rec["%s_%s_ms_median" % (s, k)], rec["%s_%s_ms_min" % (s, k)], rec["%s_%s_ms_max" % (s, k)] = \
                float(np.median(v)), float(min(v)), float(max(v))
        if parent is not None:
            for k in ("fwd", "bwd_q", "bwd_kv"):
                rec["drop_over_parent_" + k] = rec["drop_%s_ms_median" % k] / rec["parent_%s_ms_median" % k]
                rec["off_over_parent_" + k] = rec["off_%s_ms_median" % k] / rec["parent_%s_ms_median" % k]
            rec["off_equals_parent_bits"] = all(bool(torch.equal(sets["off"][1][o].view(torch.int32), sets["parent"][1][o].view(torch.int32)))
                                                for o in ("C", "lse", "delta", "dq", "dx"))
        rec["drop_lse_equals_off_bits"] = bool(torch.equal(sets["off"][1]["lse"].view(torch.int32), sets["drop"][1]["lse"].view(torch.int32)))
        print(json.dumps(rec), flush=True)
        del sets, x, g
        torch.cuda.empty_cache()


def names(args, data):
    import torch
    from stochastic_gcn_amd import ops
    dev = torch.device('cuda:0')
    a = data[1].tocsr()
    A = ops.DeviceCSR.from_scipy(a, dev, with_transpose=True)
    rng = np.random.RandomState(0)
    x = torch.from_numpy(rng.standard_normal((a.shape[0], args.d)).astype(np.float32)).to(dev)
    scale = float(args.d // args.heads) ** -0.5
    for kw in ({}, dict(keep=args.keep, key=7)):
        out, lse = ops.spattn(A, x, scale=scale, heads=args.heads, **kw)
        ops.spattn_bwd(A, A.transpose, x, None, x, out, lse, scale, heads=args.heads, **kw)
    torch.cuda.synchronize()
    print(json.dumps({"what": "attn_dropout names", "d": args.d, "heads": args.heads}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "names"])
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--shapes", nargs='+', default=["128:1", "128:4", "602:1", "512:4"])
    ap.add_argument("--keep", type=float, default=0.8)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--heads", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    data = _data()
    {"kernels": kernels, "names": names}[args.what](args, data)


if __name__ == "__main__":
    main()
