"""Step programs for tests/step_trace/main.cpp and what include/sgcn.h says they must call.

``build`` links csrc/sgcn_step.cpp (unchanged, with -DSGCN_STEP_TRACE) against recording stubs: tests/step_trace/main.cpp
holds the hand-written ones, the stubs of the extern "C" sgcn_* entries that the object leaves undefined are generated here
from the header as the compiler sees it (abi_dump.dump), so a stub prints every argument in the prototype's own type.

``OPS`` restates, per op code, the header's documentation: the entry point the op names, the order of its arguments (= the
entry point's parameters without the stream, a sgcn_dropout_t* flattened to 5 words {on, key, keep, rows, width}, a
sgcn_plan_t* to 8 words {on, seg, nseg, fix, nfix, nslots, ws, ws_elems}), the documented extras (a ``ws_capacity`` word
behind ``ws``, the trailing ``aux``) and what else the op does (joins the auxiliary stream first, two calls for CSR_SLICE).
Nothing here comes from running the code under test.
"""
import ctypes as C
import os
import struct
import subprocess
import time

import abi_dump
import test_host_sanitizers as hs
from stochastic_gcn_amd import _ffi
from stochastic_gcn_amd.step_program import OP

ROOT = abi_dump.ROOT
TRACE_DIR = os.path.join(ROOT, "tests", "step_trace")
STEP_CPP = os.path.join(ROOT, "stochastic_gcn_amd", "csrc", "sgcn_step.cpp")
BUILDS = {b: hs.BUILDS[b] for b in ("plain", "asan")}
SANITIZER_ENV = hs.SANITIZER_ENV
HANDWRITTEN = {"sgcn_tune_get", "sgcn_gemm_ws_floats", "sgcn_ln_act_bwd_ws_floats", "sgcn_csr_transpose_ws_ints",
               "sgcn_step_trace_op"}
STREAM = 7777          # the step's stream in every case
AUX = 9001             # what the aux_fork stub hands out
CODE = {v: k for k, v in OP.items()}


# ---- the build -------------------------------------------------------------------------------------------------------
def _stub_source(d, names):
    src = ['#include <cstdint>', 'void t_begin(const char*); void t_i(long long); void t_u(unsigned); void t_f(float);',
           'void t_p(const void*); void t_drop(const void*); void t_plan(const void*); void t_end(); long long t_rc(const char*);']
    ret_c = {"int32_t": "int", "int64_t": "int64_t"}
    for name in names:
        res, args = d.fn[name]
        params, body = [], []
        for j, t in enumerate(args):
            if t.endswith("*"):
                params.append("const void* a%d" % j)
                body.append({"sgcn_dropout_t*": "t_drop", "sgcn_plan_t*": "t_plan"}.get(t, "t_p") + "(a%d);" % j)
            else:
                params.append("%s a%d" % (t, j))
                body.append({"int32_t": "t_i", "int64_t": "t_i", "uint32_t": "t_u", "float": "t_f"}[t] + "(a%d);" % j)
        src.append('extern "C" %s %s(%s) { t_begin("%s"); %s t_end(); return (%s)t_rc("%s"); }'
                   % (ret_c[res], name, ", ".join(params), name, " ".join(body), ret_c[res], name))
    return "\n".join(src) + "\n"


def build(tmp_dir, wanted):
    """{build: path of the trace binary}, checked to be what they claim (as test_host_sanitizers.drivers does)"""
    d = str(tmp_dir)
    header = abi_dump.dump(tmp_dir)
    flags = hs.HOST_FLAGS + ["-DSGCN_STEP_TRACE"]
    t0 = time.time()
    objs, procs = {}, []
    for b in wanted:                                   # sgcn_step.cpp and main.cpp of every build side by side
        for src in (STEP_CPP, os.path.join(TRACE_DIR, "main.cpp")):
            obj = os.path.join(d, "%s_%s.o" % (b, os.path.basename(src)))
            cmd = ["g++"] + BUILDS[b] + flags + ["-c", src, "-o", obj]
            objs.setdefault(b, []).append(obj)
            procs.append((b, cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for b, cmd, p in procs:
        log, _ = p.communicate(timeout=hs.BUILD_TIMEOUT_S)
        assert p.returncode == 0, "the %s build failed:\n%s\n%s" % (b, " ".join(cmd), log)
    # what sgcn_step.o leaves undefined among the C entries: those get generated stubs
    undefined = subprocess.run(["nm", "-u", objs[wanted[0]][0]], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    names = sorted(s for s in undefined if s.startswith("sgcn_") and s not in HANDWRITTEN)
    assert len(names) >= 40 and set(names) <= set(header.fn), sorted(set(names) - set(header.fn))
    gen = os.path.join(d, "stubs_gen.cpp")
    with open(gen, "w") as f:
        f.write(_stub_source(header, names))
    for b in wanted:
        cmd = ["g++"] + BUILDS[b] + flags + objs[b] + [gen, "-o", os.path.join(d, b)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=hs.BUILD_TIMEOUT_S)
        assert r.returncode == 0, "the %s build failed to link:\n%s\n%s" % (b, " ".join(cmd), r.stdout[-6000:])
    print("step_trace: %s built in %.1f s" % (", ".join(wanted), time.time() - t0))
    for b in wanted:
        exe = os.path.join(d, b)
        symbols = subprocess.run(["nm", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
        assert ("__asan_init" in symbols) == (b == "asan"), "the %s build %s __asan_init" % (b, "lacks" if b == "asan" else "holds")
        assert "__tsan_init" not in symbols
        libs = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
        needed = [ln.split("=>")[0].strip() for ln in libs.splitlines() if "=>" in ln]
        dynamic = subprocess.run(["readelf", "-d", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
        needed += [ln for ln in dynamic.splitlines() if "(NEEDED)" in ln]
        assert len(needed) >= 2 and not any(s in n for n in needed for s in ("libasan", "libubsan", "libtsan", "libamdhip", "libsgcn")), \
            "a sanitizer runtime is linked dynamically, or the library itself:\n" + libs + dynamic
    return {b: os.path.join(d, b) for b in wanted}, header


# ---- programs --------------------------------------------------------------------------------------------------------
def K(v):
    return (0, -1, int(v))


def make_op(code, args, nargs=None):
    """sgcn_step_op_t from [(mul, slot, add) | int]; ``nargs`` overrides the count the op states"""
    o = _ffi.StepOp()
    o.op = code if isinstance(code, int) else OP[code]
    o.nargs = len(args) if nargs is None else nargs
    assert len(args) <= _ffi.STEP_MAX_ARGS
    for j, a in enumerate(args):
        m, s, c = a if isinstance(a, tuple) else K(a)
        o.mul[j], o.slot[j], o.add[j] = m, s, c
    return o


def write_program(path, ops, slots=(), knobs=None, stream=STREAM):
    knobs = dict(knobs or {})
    with open(path, "wb") as f:
        f.write(("SGCNTRACE1 %d %d %d %d\n" % (len(ops), len(slots), len(knobs), stream)).encode())
        for k, v in knobs.items():
            f.write(("%s=%s\n" % (k, v)).encode())
        f.write(struct.pack("<%dq" % len(slots), *slots))
        for o in ops:
            f.write(bytes(o))


def write_raw(path, op_bytes, nops, slot_bytes, nslots, knobs=None, stream=STREAM):
    """a captured program: the arrays as the model handed them to sgcn_step_run"""
    knobs = dict(knobs or {})
    with open(path, "wb") as f:
        f.write(("SGCNTRACE1 %d %d %d %d\n" % (nops, nslots, len(knobs), stream)).encode())
        for k, v in knobs.items():
            f.write(("%s=%s\n" % (k, v)).encode())
        f.write(slot_bytes)
        f.write(op_bytes)


class Trace(object):
    def __init__(self, text):
        self.lines = text.splitlines()
        self.runs = []                       # per run: the lines between `run i` and `ret`
        for ln in self.lines:
            if ln.startswith("run "):
                self.runs.append({"lines": [], "ret": None, "err": None})
            elif ln.startswith("ret "):
                self.runs[-1]["ret"] = int(ln.split()[1])
            elif ln.startswith("err "):
                self.runs[-1]["err"] = ln[4:]
            else:
                self.runs[-1]["lines"].append(ln)

    @property
    def ret(self):
        return self.runs[0]["ret"]

    @property
    def err(self):
        return self.runs[0]["err"]

    def body(self, r=0):
        return self.runs[r]["lines"]

    def calls(self, r=0):
        return [ln.split()[1] for ln in self.body(r) if ln.startswith("call ")]

    def hooks(self, r=0):
        """[(k, code, nargs, consumed, over-reads)]"""
        return [tuple(int(x) for x in ln.split()[1:]) for ln in self.body(r) if ln.startswith("op ")]

    def of_op(self, k, r=0):
        """the call lines issued while op k executed (between the hook line of the executed op before it and its own)"""
        out, cur = {}, []
        lines = self.body(r)[len(prologue_of(self.body(r))):]
        for ln in lines:
            if ln.startswith("op "):
                out[int(ln.split()[1])] = cur
                cur = []
            else:
                cur.append(ln)
        return out.get(k)


def run_trace(binary, path, timeout):
    env = dict(os.environ, **SANITIZER_ENV)
    for k in list(env):
        if k.startswith("SGCN_"):
            del env[k]                       # the knobs of a case come from its file alone
    r = subprocess.run([binary, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=timeout)
    assert r.returncode == 0 and r.stderr == "", "exit status %d\n%s\n%s" % (r.returncode, r.stderr[-8000:], r.stdout[-2000:])
    return Trace(r.stdout)


# ---- what a run does around its ops (include/sgcn.h: DW_FLUSH, GRAD_STORE, MODE) --------------------------------------------
def prologue(grouped=False, store=False, park=False, mode=None):
    out = []
    if mode is not None:
        out.append("call step_mode_override %d %d" % mode)
    if grouped:
        out.append("call dw_group_begin")
    return out + ["call grad_store_mode %d" % store, "call stats_defer %d" % park]


def prologue_of(lines):
    n = 0
    while n < len(lines) and lines[n].split()[:2] in (["call", "step_mode_override"], ["call", "dw_group_begin"],
                                                      ["call", "grad_store_mode"], ["call", "stats_defer"]):
        n += 1
        if lines[n - 1].startswith("call stats_defer"):
            break
    return lines[:n]


def cleanup(grouped=False, mode=False, stream=STREAM):
    """the guards: what runs on EVERY exit path"""
    out = (["call dw_group_abort"] if grouped else []) + ["call grad_store_mode 0", "call stats_defer 0",
                                                        "call reduce_flush p%d" % stream, "call stats_flush p%d" % stream]
    return out + (["call step_mode_override -1 -1"] if mode else [])


def epilogue(grouped=False, mode=False, pending=0, stream=STREAM):
    """a run that reaches its end: joins the auxiliary stream (and the exchange stream, when something is pending there)"""
    return ["call aux_join p%d %d" % (stream, pending)] + cleanup(grouped, mode, stream)


# ---- the ops as the header documents them ------------------------------------------------------------------------------
def fbits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def conv(t, v):
    """word v of a program as the parameter type t receives it, in the trace's notation"""
    if t == "float":
        return "f%08x" % (v & 0xFFFFFFFF)
    if t == "uint32_t":
        return "u%d" % (v & 0xFFFFFFFF)
    if t == "int32_t":
        x = v & 0xFFFFFFFF
        return str(x - (1 << 32) if x >> 31 else x)
    if t == "int64_t":
        x = v & 0xFFFFFFFFFFFFFFFF
        return str(x - (1 << 64) if x >> 63 else x)
    assert t.endswith("*"), t
    return "p%d" % (v & 0xFFFFFFFFFFFFFFFF)


def drop_text(w):
    """{on, key, keep, rows, width}: NULL when on == 0"""
    return "drop(null)" if w[0] == 0 else "drop(%s,%s,%s,%s)" % (conv("uint32_t", w[1]), conv("float", w[2]), conv("int32_t", w[3]), conv("int32_t", w[4]))


def plan_text(w):
    """{on, seg, nseg, fix, nfix, nslots, ws, ws_elems}: NULL when on == 0, dev_fix NULL when nfix == 0"""
    if w[0] == 0:
        return "plan(null)"
    fix = 0 if w[4] == 0 else w[3]
    return "plan(%s,%s,%s,%s,%s,%s,%s)" % (conv("void*", w[1]), conv("int64_t", w[2]), conv("void*", fix), conv("int64_t", w[4]),
                                           conv("int64_t", w[5]), conv("void*", w[6]), conv("int64_t", w[7]))


class Spec(object):
    """One op code.  proto: the entry point whose parameter list the op's arguments follow; call: the name in the trace (the
    internal that stands in for the entry point inside a run, where there is one); extra: {parameter index: a word that
    follows it in the program and is not passed on}; absent: parameters the program does not carry (passed as NULL);
    scratch: the parameter that is passed only when the library asks for scratch; join: the auxiliary stream is joined
    first; aux: a trailing word that says where the op runs; n: the documented argument count (checked against the layout)"""

    def __init__(self, proto, n, call=None, extra=(), absent=(), scratch=None, join=False, aux=False, custom=None):
        self.proto, self.n, self.call, self.extra, self.absent = proto, n, call or proto, set(extra), set(absent)
        self.scratch, self.join, self.aux, self.custom = scratch, join, aux, custom


OPS = {
    "DENSE_FWD": Spec("sgcn_dense_fwd_f32", 27, extra=[19], scratch=19),
    "DENSE_BWD": Spec("sgcn_dense_bwd_f32", 30, call="dense_bwd_overlapped", extra=[23], scratch=23),
    "VR_AGG": Spec("sgcn_vr_aggregate_f32", 31),
    "VR_AGG_H16": Spec("sgcn_vr_aggregate_h16", 31),
    "SPMM": Spec("sgcn_spmm_csr_add_f32", 25),
    "SOFTMAX_CE": Spec("sgcn_softmax_ce_f32", 12, custom="ce"),
    "SIGMOID_CE": Spec("sgcn_sigmoid_ce_f32", 12, custom="ce"),
    "ADAM": Spec("sgcn_adam_f32", 9, custom="adam", join=True),
    "ADAM_EMA": Spec("sgcn_adam_ema_f32", 12, custom="adam", join=True),
    "SCATTER_ROWS": Spec("sgcn_scatter_rows_f32", 7, join=True),
    "SCATTER_ROWS_H16": Spec("sgcn_scatter_rows_h16", 7, join=True),
    "AUX_SCATTER_ROWS": Spec("sgcn_scatter_rows_f32", 7),
    "AUX_SCATTER_ROWS_H16": Spec("sgcn_scatter_rows_h16", 7),
    "MEMSET0": Spec(None, 2, custom="memset", join=True),
    "AUX_MEMSET0": Spec(None, 2, custom="memset"),
    "DROPOUT": Spec("sgcn_dropout_f32", 11),
    "L2_PENALTY": Spec("sgcn_l2_penalty_f32", 6, join=True),
    "GATHER_ROWS": Spec("sgcn_gather_rows_f32", 7),
    "COPY2D": Spec(None, 6, custom="copy2d"),
    "VR_AGG_PRE": Spec("sgcn_vr_aggregate_pre_f32", 18),
    "VR_AGG_PRE_H16": Spec("sgcn_vr_aggregate_pre_h16", 18),
    "VR_AGG_POST": Spec("sgcn_vr_aggregate_post_f32", 19, join=True),
    "VR_AGG_POST_H16": Spec("sgcn_vr_aggregate_post_h16", 19, join=True),
    "DW_FLUSH": Spec(None, 0, custom="dw_flush"),
    "GRAD_STORE": Spec(None, 0, custom="none"),
    "MODE": Spec(None, 2, custom="none"),
    "CSR_SLICE": Spec(None, 9, custom="csr_slice"),
    "LN_ACT_FWD": Spec("sgcn_ln_act_fwd_f32", 12),
    "LN_ACT_BWD": Spec("sgcn_ln_act_bwd_f32", 16, extra=[14]),
    "CSR_TRANSPOSE": Spec("sgcn_csr_transpose_index", 9, extra=[7]),
    "GATHER_F32": Spec("sgcn_gather_f32", 4),
    "ALLREDUCE_AVG": Spec("sgcn_coll_allreduce_avg_f32", 2, custom="allreduce"),
    "HIST_PACK": Spec("sgcn_hist_pack_f32", 8, aux=True),
    "ALLGATHER_I32": Spec("sgcn_coll_allgather_i32", 4, aux=True),
    "HIST_APPLY": Spec("sgcn_hist_apply_f32", 8, aux=True),
    "HIST_APPLY_H16": Spec("sgcn_hist_apply_h16", 8, aux=True),
    "GEMM": Spec("sgcn_gemm_f32", 14, extra=[12], absent=[13, 14], scratch=12),
    "DET_PRE": Spec("sgcn_det_pre_f32", 5),
    "DET_PRE_BWD": Spec("sgcn_det_pre_bwd_f32", 6),
    "SQUARE": Spec("sgcn_square_f32", 4),
    "ADDMUL": Spec("sgcn_addmul_f32", 5),
    "DET_LNVAR_FWD": Spec("sgcn_det_lnvar_fwd_f32", 7),
    "DET_LNVAR_BWD": Spec("sgcn_det_lnvar_bwd_f32", 12),
    "DET_RELU_FWD": Spec("sgcn_det_relu_fwd_f32", 5),
    "DET_RELU_BWD": Spec("sgcn_det_relu_bwd_f32", 7),
    "GAUSS": Spec("sgcn_gauss_sample_f32", 5),
    "GAUSS_BWD": Spec("sgcn_gauss_sample_bwd_f32", 5),
    "DET_AGG_PREP": Spec("sgcn_det_agg_prep_f32", 13),
    "DET_AGG_PREP_BWD": Spec("sgcn_det_agg_prep_bwd_f32", 11),
    "RELU_EPS": Spec("sgcn_relu_eps_f32", 7),
    "GATE": Spec("sgcn_gate_f32", 7),
}
# the twin whose argument list an _H16 op shares (include/sgcn.h: "the argument lists of ops 3 / 14 / 15 / 7 / 16 / 32")
H16_TWIN = {"VR_AGG_H16": "VR_AGG", "VR_AGG_PRE_H16": "VR_AGG_PRE", "VR_AGG_POST_H16": "VR_AGG_POST",
            "SCATTER_ROWS_H16": "SCATTER_ROWS", "AUX_SCATTER_ROWS_H16": "AUX_SCATTER_ROWS", "HIST_APPLY_H16": "HIST_APPLY"}
# MODE's two words are read from the program ahead of the loop (they hold for the WHOLE run), not by the op's own case
CONSUMED = {"MODE": 0}


def layout(header, name):
    """[(kind, type)] of the op's words: kind 'arg' (parameter of the prototype), 'drop' x5, 'plan' x8, 'extra'"""
    s = OPS[name]
    if s.proto is None:
        return None
    params = header.fn[s.proto][1]
    assert params[-1] == "void*"              # the stream comes last
    out = []
    for i, t in enumerate(params[:-1]):
        if i in s.absent:
            continue
        if t == "sgcn_dropout_t*":
            out += [("drop", i)] * 5
        elif t == "sgcn_plan_t*":
            out += [("plan", i)] * 8
        else:
            out.append(("arg", i))
        if i in s.extra:
            out.append(("extra", i))
    if s.aux:
        out.append(("aux", None))
    return out


def sentinel(j, t, wide):
    """argument j: 1000 + j for pointers and sizes, the bits of j + 0.5 in a float position; `wide` sets bits above the low
    32, which an int32 / uint32 / float parameter must drop and an int64 / pointer parameter must keep"""
    v = fbits(j + 0.5) if t == "float" else 1000 + j
    return v | (3 << 33) if wide else v


def position_case(header, name, wide=False, stream=STREAM):
    """(words, expected call lines of the op, at overlap = 0 and with every scratch question answered 0)"""
    s = OPS[name]
    st = "p%d" % stream
    pre = ["call aux_join %s 0" % st] if s.join else []
    if s.custom == "none":
        return [sentinel(j, "int64_t", False) for j in range(s.n)] if name != "MODE" else [0, 127], []
    if s.custom == "dw_flush":
        return [], ["call dw_group_flush %s 0" % st]
    if s.custom == "memset":
        w = [sentinel(0, "void*", wide), sentinel(1, "int64_t", wide)]
        return w, pre + ["call hipMemsetAsync %s 0 %s %s" % (conv("void*", w[0]), conv("int64_t", w[1]), st)]
    if s.custom == "copy2d":        # hipMemcpy2DAsync(dst, ldd, src, lds, rows, cols) in floats: pitches and width in bytes, device to device
        w = [sentinel(j, "int64_t", wide) for j in range(6)]
        return w, ["call hipMemcpy2DAsync %s %d %s %d %d %d 3 %s" % (conv("void*", w[0]), w[1] * 4, conv("void*", w[2]), w[3] * 4,
                                                                   w[5] * 4, w[4], st)]
    if s.custom == "csr_slice":     # (n, rows, a_val, a_col, a_rowptr, o_p, o_d, o_col, o_row)
        w = [sentinel(j, "int64_t", wide) for j in range(9)]
        p = [conv("void*", x) for x in w]
        n = conv("int32_t", w[0])
        return w, ["call sgcn_csr_slice_indptr_dev %s %s %s %s %s" % (n, p[1], p[4], p[5], st),
                   "call sgcn_csr_slice_f32 %s %s %s %s %s %s %s %s %s %s" % (n, p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], st)]
    lay = layout(header, name)
    params = header.fn[s.proto][1]
    words, shown, j = [], {}, 0
    while j < len(lay):
        kind, i = lay[j]
        if kind == "drop":
            w = [sentinel(j, "int64_t", wide), sentinel(j + 1, "uint32_t", wide), sentinel(j + 2, "float", wide),
                 sentinel(j + 3, "int32_t", wide), sentinel(j + 4, "int32_t", wide)]
            shown[i] = drop_text(w)
            words += w
            j += 5
        elif kind == "plan":
            w = [sentinel(j + q, "int64_t", wide) for q in range(8)]
            shown[i] = plan_text(w)
            words += w
            j += 8
        elif kind == "aux":
            words.append(0)                  # 0 = on the step's stream (1 and 2: the exchange cases)
            j += 1
        elif kind == "extra":
            words.append(sentinel(j, "int64_t", wide))
            j += 1
        else:
            words.append(sentinel(j, params[i], wide))
            shown[i] = conv(params[i], words[-1])
            j += 1
    for i in s.absent:
        shown[i] = "drop(null)" if params[i] == "sgcn_dropout_t*" else "p0"
    if s.scratch is not None:
        shown[s.scratch] = "p0"              # the library asks for no scratch: none is passed
    vals = [shown[i] for i in range(len(params) - 1)]
    if s.custom == "ce":
        line = "call ce_impl %d %s %s 0 last(null)" % (name == "SOFTMAX_CE", " ".join(vals), st)
    elif s.custom == "adam":
        if name == "ADAM":                   # (theta, grad, m, v, n, lr, b1, b2, eps): no average
            vals = vals + ["p0", "f00000000", "f00000000"]
        else:                                # (theta, grad, m, v, avg, n, lr, b1, b2, eps, decay, one_minus)
            vals = vals[:4] + vals[5:10] + [vals[4]] + vals[10:]
        line = "call adam_with_stats %s %s" % (" ".join(vals), st)
    elif s.custom == "allreduce":
        return words, ["call aux_join %s 0" % st, "call reduce_flush %s" % st, "call %s %s %s" % (s.call, " ".join(vals), st)]
    else:
        line = "call %s %s %s" % (s.call, " ".join(vals), st)
    return words, pre + [line]


# ---- op builders for the cases with meaningful shapes (word indices as in the layouts above) ---------------------------------
def words_of(header, name, values):
    """the op's words, all zero but {index: value}"""
    n = OPS[name].n
    w = [0] * n
    for k, v in values.items():
        w[k] = v
    return w


def dense_fwd(M, N, Kd, X, ldx, W, ldw, Y, ldy, X2=0, ldx2=0, split=0, off=0, sc=0, relu=0, xhat=0, rstd=0, drop=(0, 0, fbits(1.0), -1, 0),
              ws=5000, ws_cap=1 << 20, g1=0, g2=0):
    return [M, N, Kd, X, ldx, X2, ldx2, split, W, ldw, off, sc, fbits(1e-9), relu, Y, ldy, xhat, rstd] + list(drop) + [ws, ws_cap, g1, g2]


def ce(z, ldz, n, c, lab=6000, ldl=None, dz=6100, lddz=None, pred=0, ldp=0, stats=6200, rowstat=6300):
    return [z, ldz, lab, c if ldl is None else ldl, n, c, dz, c if lddz is None else lddz, pred, ldp, stats, rowstat]


def dense_bwd(n, N, Kd, dy, lddy, W, ldw, dx=7300, lddx=None, xhat=0, rstd=0, sc=0, relu=0, y=7000, x=7100, dW=7200, ws_cap=1 << 20):
    return [n, N, Kd, dy, lddy, y, N, xhat, rstd, sc, relu, x, Kd, W, ldw, dW, N, 0, 0, dx, Kd if lddx is None else lddx,
            0, 0, fbits(1.0), -1, 0, 7400, 5000, ws_cap, 0]


def adam(n=100):
    return [8000, 8100, 8200, 8300, n, fbits(1e-3), fbits(0.9), fbits(0.999), fbits(1e-8)]


def scatter(H=8500, n=10, d=16):
    return [H, d, 8600, n, d, 8700, d]


def account(trace, nops, r=0):
    """{k: 'launched' | 'folded' | 'skipped'}: an executed op (it has a hook line) either issued calls or left its work to a
    later op's call; an op without a hook line was skipped behind a fold"""
    hooks = {h[0] for h in trace.hooks(r)}
    out = {}
    for k in range(nops):
        if k not in hooks:
            out[k] = "skipped"
        else:
            out[k] = "launched" if trace.of_op(k, r) else "folded"
    return out
