"""Real step programs through the recording back end of tests/step_trace: what the model hands to sgcn_step_run, op by op.

For every stack of test_step_program_gpu.SUPPORTED, at the grouped default and layer by layer on the auxiliary stream, and
for one --det_dropout stack, one training step runs with native_step=True while the bound sgcn_step_run is wrapped: the op
array, the slot table and the two counts of every call are copied before the call goes through.  The copy is written in
step_trace's file format and run through the PLAIN trace binary in a child process that never opens the GPU (the stubs
print pointers and never follow them).  The trace must end with status 0, every op code must be known, and the hook must
report for every executed op that its case consumed exactly the arguments the compiler emitted, with no read past the
list -- the positional contract between step_program.py's emitters and sgcn_step.cpp's readers, on the programs that
actually run (tests/test_step_trace.py holds the readers against include/sgcn.h, op code by op code).

Measured: the trace binary builds in 2 s (0.7 s on the GPU machine), once per module; the fifteen cases compile their
models at model_cases' small sizes and take 2.4 s together; the child runs 2 ms and gets step_trace's TIMEOUT_S.
"""
import ctypes as C

import pytest
import torch

import model_cases as mc
import step_trace_cases as sc
from test_step_program_gpu import SUPPORTED, _model
from test_step_trace import TIMEOUT_S

pytestmark = pytest.mark.gpu

CASES = [(name, group) for name in SUPPORTED for group in (True, False)] + [(sorted(mc.DET_CASES)[0], True)]


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    binaries, _ = sc.build(tmp_path_factory.mktemp("step_trace_gpu"), ["plain"])
    return binaries["plain"]


@pytest.mark.parametrize("name,group", CASES, ids=["%s-%s" % (n, "grouped" if g else "layerwise") for n, g in CASES])
def test_compiled_program_is_consumed_word_for_word(binary, tmp_path, monkeypatch, name, group):
    from stochastic_gcn_amd import _ffi
    from stochastic_gcn_amd.flags import FLAGS
    from stochastic_gcn_amd.step_program import OP
    case = mc.build_case(name)
    params = mc.make_oracle_model(case, seed=3).params
    m = _model(case, {k: v.copy() for k, v in params.items()}, True, group)
    real = _ffi.lib.sgcn_step_run
    captured = []

    def recording(ops, nops, slots, nslots, stream):
        captured.append((C.string_at(C.addressof(ops), int(nops) * C.sizeof(_ffi.StepOp)), int(nops),
                         C.string_at(int(slots), int(nslots) * 8), int(nslots)))
        return real(ops, nops, slots, nslots, stream)
    monkeypatch.setattr(_ffi.lib, "sgcn_step_run", recording)
    sch = mc.make_scheduler(case, 1)
    pb = sch.minibatch_packed(case['cfg']['batch'], FLAGS.plan_t, None)
    pb.dropout = case['flags']['dropout']
    m.run_one_step(None, pb, sync=True)
    torch.cuda.synchronize()
    monkeypatch.undo()
    progs = getattr(m, '_programs', {})
    assert progs and all(p is not None for p in progs.values()), getattr(m, '_program_note', 'no program was compiled')
    assert captured, "the step did not go through sgcn_step_run"
    codes = set(OP.values())
    for i, (op_bytes, nops, slot_bytes, nslots) in enumerate(captured):
        assert nops > 0
        path = str(tmp_path / ("captured%d.bin" % i))
        sc.write_raw(path, op_bytes, nops, slot_bytes, nslots)
        t = sc.run_trace(binary, path, TIMEOUT_S)
        assert t.ret == 0, t.err
        hooks = t.hooks()
        assert hooks and [h[0] for h in hooks] == sorted({h[0] for h in hooks}) and hooks[-1][0] < nops
        arr = (_ffi.StepOp * nops).from_buffer_copy(op_bytes)
        assert all(arr[k].op in codes for k in range(nops))
        for k, code, nargs, consumed, over in hooks:
            assert code == arr[k].op and nargs == arr[k].nargs
            want = sc.CONSUMED.get(sc.CODE[code], nargs)
            assert consumed == want and over == 0, "op %d (%s): %d words emitted, %d consumed, %d reads past the list" % (
                k, sc.CODE[code], nargs, consumed, over)
            assert nargs == sc.OPS[sc.CODE[code]].n, "op %d (%s) carries %d words, include/sgcn.h documents %d" % (
                k, sc.CODE[code], nargs, sc.OPS[sc.CODE[code]].n)
        print("%s: %d ops, %d executed, %d downstream calls" % (name, nops, len(hooks), len(t.calls())))
