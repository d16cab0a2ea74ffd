"""Child processes of tests/test_history_bf16_gpu.py: every job that opens a process group runs in a fresh interpreter
(``python history_bf16_workers.py <job> ...``) under the caller's timeout.

  rccl  <force> <overlap> <port> <out.npz>   three bfloat16-history training steps of the Reddit recipe, with a one-rank
                                             RCCL process group (SGCN_FORCE_PG=1: gradient all-reduce and history exchange
                                             as ops of the step program on the library's communicator) or without one
  gloo  <rank> <port> <out.npz>              one rank of a two-rank gloo job on cuda:0, three steps
"""
import contextlib
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np      # noqa: E402
import torch            # noqa: E402


def _trainer(steps):
    from stochastic_gcn_amd import synthetic
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.train import Trainer
    torch.cuda.set_device(0)
    data = synthetic.reddit_like(n=6000, m=60000, f=32, classes=6, splits=(3600, 800, 1600), seed=5,
                                 with_features=True, planted=True)
    FLAGS.reset()
    FLAGS.update(dataset='s-reddit', normalization='graphsage', weight_decay=0.0, dropout=0.1, layer_norm=True,
                 hidden1=64, num_fc_layers=2, batch_size=256, test_batch_size=512, cv=True, cvd=True, test_cv=True,
                 degree=1, test_degree=1, seed=1, native_step=True, max_steps=steps, history_dtype='bf16')
    with contextlib.redirect_stdout(io.StringIO()):
        trn = Trainer(data=data, verbose=False)
        trn.train_epoch()
    return trn


def _save(path, trn, **extra):
    m = trn.train_model
    m.join_history()
    torch.cuda.synchronize()
    h = m.history[0][0]
    assert h.dtype == torch.bfloat16 and h.stride(0) % 8 == 0
    progs = [p for p in getattr(m, '_programs', {}).values() if p is not None]
    np.savez(path, theta=m.theta.cpu().numpy(), hist=h.contiguous().view(torch.int16).cpu().numpy().view(np.uint16),
             steps=np.array([m.adam_t]), used_program=np.array([bool(progs)]), **extra)


def rccl(force, overlap, port, out):
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      SGCN_FORCE_PG="1" if force else "0", SGCN_NATIVE_COLL="1", SGCN_EXCHANGE_OVERLAP="1" if overlap else "0")
    os.environ.pop("SGCN_DIST_BACKEND", None)
    import torch.distributed as dist
    from stochastic_gcn_amd.step_program import OP
    trn = _trainer(3)
    m, par = trn.train_model, trn.par
    assert par.active == force and dist.is_initialized() == force
    progs = [p for p in m._programs.values() if p is not None]
    assert progs
    codes = [[op for op, _ in p.ops_fb + p.ops_opt + p.ops_hist] for p in progs]
    if force:
        from stochastic_gcn_amd._ffi import lib
        assert par.native and lib.sgcn_coll_world() == 1 and all(p.native_world == 1 for p in progs)
        assert par.exchange_overlap == overlap == bool(lib.sgcn_coll_has_exchange())
        for p, c in zip(progs, codes):
            # the collectives are ops of the program; the apply is the bfloat16 one, on the exchange stream (in front of
            # the loss) or behind the optimizer
            where = [op for op, _ in (p.ops_fb if overlap else p.ops_hist)]
            assert OP['ALLREDUCE_AVG'] in c and OP['HIST_APPLY'] not in c
            assert all(o in where for o in (OP['HIST_PACK'], OP['ALLGATHER_I32'], OP['HIST_APPLY_H16']))
            assert all(args[-1][2] == (2 if overlap else 0) for op, args in (p.ops_fb if overlap else p.ops_hist)
                       if op in (OP['HIST_PACK'], OP['ALLGATHER_I32'], OP['HIST_APPLY_H16']))
    for c in codes:
        assert OP['VR_AGG_H16'] in c and not any(OP[o] in c for o in ('VR_AGG', 'SCATTER_ROWS', 'AUX_SCATTER_ROWS'))
    _save(out, trn)
    par.shutdown()


def gloo(rank, port, out):
    os.environ.update(RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      SGCN_DIST_BACKEND="gloo")
    trn = _trainer(3)
    assert trn.par.active and trn.par.world == 2
    _save(out, trn)
    trn.par.shutdown()


if __name__ == "__main__":
    job = sys.argv[1]
    if job == "rccl":
        rccl(sys.argv[2] == "1", sys.argv[3] == "1", int(sys.argv[4]), sys.argv[5])
    elif job == "gloo":
        gloo(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
    else:
        raise SystemExit("unknown job %r" % job)
