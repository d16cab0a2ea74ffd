"""Hand-built programs for the library's launch loop (sgcn_step_run): ``[(OP['ADAM'], [K(ptr), ...]), ...]`` as the
``StepOp`` array the package's own compiler (stochastic_gcn_amd/step_program.py) emits, run against a slot table.
Test-only; it uses the package's ``StepOp``, ``OP`` and ``K`` as they are."""
import ctypes as C

import numpy as np


def F(x):
    """a float operand: its fp32 bits as a constant"""
    from stochastic_gcn_amd.step_program import K
    return K(int(np.float32(x).view(np.uint32)))


def S(slot, mul=1, add=0):
    """the operand  mul * slots[slot] + add"""
    return (int(mul), int(slot), int(add))


def pack(ops):
    from stochastic_gcn_amd._ffi import StepOp
    arr = (StepOp * max(len(ops), 1))()
    for k, (opc, args) in enumerate(ops):
        o = arr[k]
        o.op, o.nargs = int(opc), len(args)
        for j, a in enumerate(args):
            o.mul[j], o.slot[j], o.add[j] = int(a[0]), int(a[1]), int(a[2])
    return arr


def run(ops, slots=(), stream=None):
    """the status of sgcn_step_run on the program (0: ran)"""
    from stochastic_gcn_amd._ffi import lib
    table = (C.c_int64 * max(len(slots), 1))(*[int(s) for s in slots])
    return int(lib.sgcn_step_run(pack(ops), len(ops), C.addressof(table), len(slots), stream))
