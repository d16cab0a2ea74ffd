"""sgcn_step_run's host logic on a recording back end, without a GPU: plain and under AddressSanitizer + UBSan.

tests/step_trace/main.cpp links csrc/sgcn_step.cpp (unchanged; -DSGCN_STEP_TRACE turns its per-op hook on) against stubs
that print every downstream call -- the library's entry points, its internals, the HIP runtime -- and touch nothing.  Each
test writes a small step program, runs the trace binary on it in a child process and compares the lines with what
include/sgcn.h documents (step_trace_cases.OPS restates that, op by op; the prototypes come from the header through the
compiler, abi_dump.py).  Every run must exit 0 with an empty stderr -- a sanitizer's report would be there.

The builds are test_host_sanitizers.py's ``plain`` and ``asan`` flag sets (runtimes linked statically, nothing preloaded,
nothing loaded into python is sanitized), checked the same way; the ``asan`` cases skip where /dev/kfd exists.  No ``tsan``
build: the loop is single-threaded behind its mutex.

Findings the cases pin down (documented in include/sgcn.h rather than changed):
  * MODE's two words are read ahead of the loop, not by the op's case: the hook reports 0 of 2 consumed;
  * the pre-layer fold's 160 KiB bound cannot be exceeded by shapes that pass its other conditions (256 x 128 + 128 x 64
    floats is exactly 160 KiB): the largest shape folds, there is no shape "one past".

Measured on an 8-core machine: both builds side by side take 5 s (plain alone 2 s); a run of the trace binary takes 2 ms
plain and 10 ms under asan, process start included, and no case is slower than that by more than the number of runs it
makes (the slowest test, the joins under asan, makes 130 runs in 1.9 s).  TIMEOUT_S is far above five times a run because a
process start on a loaded machine is the larger term; the margin is against a hang.  The whole file takes 16 s.
"""
import pytest

import step_trace_cases as sc
from step_trace_cases import K, OP, OPS, STREAM, fbits

TIMEOUT_S = 10
FUSE = (0, 1, 4, 16, 17, 127)
BUILD_PARAMS = [pytest.param("plain", id="plain"), pytest.param("asan", id="asan", marks=sc.hs.NO_SANITIZERS_HERE)]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    wanted = ["plain"] + ([] if sc.hs.ON_GPU_MACHINE else ["asan"])
    return sc.build(tmp_path_factory.mktemp("step_trace"), wanted)


@pytest.fixture(params=BUILD_PARAMS)
def trace(request, built, tmp_path):
    binaries, header = built
    n = [0]

    def run(ops, slots=(), knobs=None):
        n[0] += 1
        path = str(tmp_path / ("case%d.bin" % n[0]))
        sc.write_program(path, [sc.make_op(*o) if isinstance(o, tuple) else o for o in ops], slots, knobs)
        return sc.run_trace(binaries[request.param], path, TIMEOUT_S)
    run.header = header
    return run


def hook(k, name, nargs, consumed=None):
    return "op %d %d %d %d 0" % (k, OP[name], nargs, nargs if consumed is None else consumed)


# ---- 1. positions: every op code of the enum ---------------------------------------------------------------------------
def test_every_op_code_is_specified(built):
    _, header = built
    assert {k[len("SGCN_OP_"):] for k in header.enum} == set(OPS) == set(OP)
    for name, s in OPS.items():
        lay = sc.layout(header, name)
        if lay is not None:
            assert len(lay) == s.n, "%s: the prototype's flattened list has %d words, the header's op comment %d" % (name, len(lay), s.n)
        assert s.n <= header.const["SGCN_STEP_MAX_ARGS"]
    for h16, twin in sc.H16_TWIN.items():      # an _H16 op: the _h16 entry with the argument list of its fp32 twin
        a, b = OPS[h16], OPS[twin]
        assert a.proto == b.proto.replace("_f32", "_h16") and (a.n, a.join, a.aux) == (b.n, b.join, b.aux)
        assert [k for k, _ in sc.layout(header, h16)] == [k for k, _ in sc.layout(header, twin)]
        pa, pb = header.fn[a.proto][1], header.fn[b.proto][1]
        assert len(pa) == len(pb) and [x for x, y in zip(pa, pb) if x != y] == ["uint16_t*"]      # the table, and only it


@pytest.mark.parametrize("wide", [False, True], ids=["low", "wide"])
@pytest.mark.parametrize("name", sorted(OPS))
def test_one_op_program_makes_the_documented_call(trace, name, wide):
    s = OPS[name]
    words, lines = sc.position_case(trace.header, name, wide)
    assert len(words) == s.n
    t = trace([(name, words)], knobs={"step_overlap": 0, "step_fuse": 127})
    mode = (words[0], words[1]) if name == "MODE" else None
    want = sc.prologue(grouped=name == "DW_FLUSH", store=name == "GRAD_STORE", mode=mode) + lines \
        + [hook(0, name, s.n, sc.CONSUMED.get(name))] + sc.epilogue(grouped=name == "DW_FLUSH", mode=mode is not None)
    assert t.ret == 0, t.err
    assert t.body() == want


def test_sub_records_and_documented_nulls(trace):
    h = trace.header
    # drop: NULL when on == 0; plan: NULL when on == 0, dev_fix NULL when nfix == 0; SPMM without an addend: the plain entry
    w, _ = sc.position_case(h, "DENSE_FWD")
    w[18] = 0
    t = trace([("DENSE_FWD", w)], knobs={"step_fuse": 0})
    assert " drop(null) p0 " in t.of_op(0)[0]
    w, _ = sc.position_case(h, "VR_AGG")
    w[23] = 0
    assert trace([("VR_AGG", w)]).of_op(0)[0].split()[-2] == "plan(null)"
    w, _ = sc.position_case(h, "VR_AGG")
    w[27] = 0
    assert trace([("VR_AGG", w)]).of_op(0)[0].split()[-2] == "plan(p1024,1025,p0,0,1028,p1029,1030)"
    w, lines = sc.position_case(h, "SPMM")
    w[22] = 0                                                     # add == NULL
    got = trace([("SPMM", w)]).of_op(0)
    want = lines[0].replace("sgcn_spmm_csr_add_f32", "sgcn_spmm_csr_f32").split()
    assert got == [" ".join(want[:-4] + want[-1:])]
    # scratch is passed exactly when the library asks for some, and refused when the op's capacity is below it
    for name, (iw, icap) in {"DENSE_FWD": (23, 24), "DENSE_BWD": (27, 28), "GEMM": (12, 13)}.items():
        w, lines = sc.position_case(h, name)
        if name == "DENSE_FWD":
            w[1] = 64                                             # (split-K scratch is a matter of layers up to 128 wide)
            lines = [lines[0].replace(" 1001 ", " 64 ", 1)]
        t = trace([(name, w)], knobs={"gemm_ws": w[icap], "step_fuse": 0})
        at = len("call x".split()) + sc.OPS[name].scratch
        want = lines[0].split()
        want[at] = "p%d" % w[iw]
        assert t.of_op(0) == [" ".join(want)]
        t = trace([(name, w), ("GATHER_F32", [1, 2, 3, 4])], knobs={"gemm_ws": w[icap] + 1, "step_fuse": 0})
        assert t.ret == -1 and "scratch" in t.err and t.body() == sc.prologue() + sc.cleanup()
    for name, knob in (("LN_ACT_BWD", "ln_ws"), ("CSR_TRANSPOSE", "transpose_ws")):
        w, _ = sc.position_case(h, name)
        icap = [j for j, (k, _) in enumerate(sc.layout(h, name)) if k == "extra"][0]
        assert trace([(name, w)], knobs={knob: w[icap]}).ret == 0
        t = trace([(name, w)], knobs={knob: w[icap] + 1})
        assert t.ret == -1 and "scratch too small" in t.err and t.body() == sc.prologue() + sc.cleanup()
    # ADAM_EMA without an average is refused by the loop itself
    w, _ = sc.position_case(h, "ADAM_EMA")
    w[4] = 0
    t = trace([("ADAM_EMA", w)])
    assert t.ret == -1 and "without an average" in t.err and "adam_with_stats" not in t.calls()


# ---- 2. slots ------------------------------------------------------------------------------------------------------------
def test_slots_are_affine_and_refusals_call_nothing_more(trace):
    slots = [-5, 0, 1 << 40, 3]
    args = [(1, 2, 64), (4, 2, -1), (-3, 0, 7), (1, 1, 9), (0, 3, 5), (7, -1, 123), (-1, 2, 0)]      # GATHER_ROWS (in, ldi, r, n, d, out, ldo)
    line = "call sgcn_gather_rows_f32 p%d %d p22 9 5 p123 %d p%d" % ((1 << 40) + 64, (4 << 40) - 1, -(1 << 40), STREAM)
    good = ("GATHER_ROWS", args)
    t = trace([good], slots)
    assert t.ret == 0 and t.body() == sc.prologue() + [line, hook(0, "GATHER_ROWS", 7)] + sc.epilogue()
    # a negative size computed from a negative slot reaches the entry point as such (the entry point refuses it)
    t = trace([("GATHER_ROWS", [K(1), K(8), K(2), (1, 0, 0), K(4), K(3), K(8)])], slots)
    assert t.of_op(0) == ["call sgcn_gather_rows_f32 p1 8 p2 -5 4 p3 8 p%d" % STREAM]
    last = ("GATHER_F32", [1, 2, 3, 4])
    beyond = ("GATHER_ROWS", args[:3] + [(1, 4, 0)] + args[4:])
    for bad, msg in ((beyond, "reads a slot beyond 4"), (sc.make_op("GATHER_ROWS", args, nargs=-1), "has -1 arguments"),
                     (sc.make_op("GATHER_ROWS", args, nargs=49), "has 49 arguments")):
        for grouped in (False, True):
            t = trace([good, bad, last] + ([("DW_FLUSH", [])] if grouped else []), slots)
            assert t.ret == -1 and msg in t.err
            assert t.body() == sc.prologue(grouped=grouped) + [line, hook(0, "GATHER_ROWS", 7)] + sc.cleanup(grouped=grouped)
    # the slot table as the caller sizes it: one slot fewer, and the first op's slot 3 is beyond it
    t = trace([good], slots, knobs={"say_nslots": 3})
    assert t.ret == -1 and "reads a slot beyond 3" in t.err and t.body() == sc.prologue() + sc.cleanup()
    for knobs in ({"say_nops": -1}, {"say_nslots": -1}, {"null_ops": 1}):
        t = trace([good], slots, knobs=knobs)
        assert t.ret == -1 and "bad argument" in t.err and t.body() == []


# ---- 3. run modes ----------------------------------------------------------------------------------------------------------
def test_run_modes(trace):
    h = trace.header
    w = {n: sc.position_case(h, n)[0] for n in OPS}
    g = ("GATHER_F32", w["GATHER_F32"])
    # DW_FLUSH anywhere: the run is grouped; the reductions ride in an optimizer directly behind it (fuse bit 5)
    for fuse, nxt, park in ((127, "ADAM", 1), (127, "ADAM_EMA", 1), (127, "GATHER_F32", 0), (127 - 32, "ADAM", 0), (127, None, 0)):
        prog = [g, ("DW_FLUSH", [])] + ([(nxt, w[nxt])] if nxt else [])
        t = trace(prog, knobs={"step_fuse": fuse})
        assert t.ret == 0 and t.body()[:3] == sc.prologue(grouped=True)
        assert t.of_op(1) == ["call dw_group_flush p%d %d" % (STREAM, park)]
        assert t.body()[-len(sc.cleanup(grouped=True)):] == sc.cleanup(grouped=True)
    # GRAD_STORE anywhere; the statistics are parked only in a store-mode run with the optimizer after the loss and no L2_PENALTY
    ce_op, ad, l2 = ("SOFTMAX_CE", w["SOFTMAX_CE"]), ("ADAM", w["ADAM"]), ("L2_PENALTY", w["L2_PENALTY"])
    gs = ("GRAD_STORE", [])
    for prog, store, park in (([ce_op, ad, gs], 1, 1), ([gs, ("SIGMOID_CE", w["SIGMOID_CE"]), g, ("ADAM_EMA", w["ADAM_EMA"])], 1, 1),
                              ([ce_op, ad], 0, 0), ([gs, ce_op, l2, ad], 1, 0), ([gs, ad, ce_op], 1, 0), ([gs, ce_op], 1, 0),
                              ([gs, ad], 1, 0), ([gs, ce_op, ad, l2], 1, 0)):
        t = trace(prog)
        assert t.ret == 0 and t.body()[:2] == sc.prologue(store=bool(store), park=bool(park))
        assert t.body()[-4:] == sc.cleanup()
        assert len(t.hooks()) == len(prog) and all(hk[2] == hk[3] and hk[4] == 0 for hk in t.hooks())
    # MODE anywhere: this run's overlap and fusion bits, undone on every exit path; fuse < 0 keeps the process-wide bits
    for words, knobs, want in (([1, 5], {"step_overlap": 0}, (1, 5)), ([0, -1], {"step_fuse": 77}, (0, 77)), ([7, 300], {}, (1, 300 & 127)),
                               ([0, 0], {}, (0, 0))):
        t = trace([("AUX_MEMSET0", w["AUX_MEMSET0"]), ("MODE", words)], knobs=knobs)
        assert t.ret == 0 and t.body()[0] == "call step_mode_override %d %d" % want and t.body()[-1] == "call step_mode_override -1 -1"
        assert ("aux_fork" in t.calls()) == bool(want[0])
        t = trace([g, sc.make_op("GATHER_F32", w["GATHER_F32"], nargs=-1), ("MODE", words)], knobs=knobs)
        assert t.ret == -1 and t.body() == sc.prologue(mode=want) + sc.position_case(h, "GATHER_F32")[1] + [hook(0, "GATHER_F32", 4)] \
            + sc.cleanup(mode=True)
    t = trace([g], knobs={"step_overlap": 1})
    assert "step_mode_override" not in t.calls()
    # a failing entry point: the run stops there, joins both side streams and cleans up
    t = trace([g, ("GATHER_ROWS", w["GATHER_ROWS"]), g, ("MODE", [1, 0])], knobs={"rc.sgcn_gather_rows_f32": -2})
    assert t.ret == -2 and [hk[0] for hk in t.hooks()] == [0, 1]
    assert t.body()[-7:] == ["op 1 %d 7 7 0" % OP["GATHER_ROWS"]] + sc.epilogue(mode=True)


# ---- 4. joins of the auxiliary stream -------------------------------------------------------------------------------------
def test_auxiliary_stream_forks_and_joins(trace):
    h = trace.header
    w = {n: sc.position_case(h, n) for n in OPS}
    bwd = ("DENSE_BWD", sc.dense_bwd(100, 32, 48, 7500, 32, 7600, 32))
    forkers = ["VR_AGG_PRE", "VR_AGG_PRE_H16", "AUX_SCATTER_ROWS", "AUX_SCATTER_ROWS_H16", "AUX_MEMSET0"]
    joiners = ["ADAM", "ADAM_EMA", "L2_PENALTY", "SCATTER_ROWS", "SCATTER_ROWS_H16", "MEMSET0", "VR_AGG_POST", "VR_AGG_POST_H16"]
    for overlap in (1, 0):
        knobs = {"step_overlap": overlap, "step_fuse": 0}
        for f in forkers:
            t = trace([(f, w[f][0])], knobs=knobs)
            own = [ln.replace("p%d" % STREAM, "p%d" % sc.AUX) if overlap else ln for ln in w[f][1]]
            assert t.of_op(0) == (["call aux_fork p%d" % STREAM] if overlap else []) + own
            assert t.body()[-5] == "call aux_join p%d %d" % (STREAM, overlap)         # a run never ends with work pending
            for j in joiners:
                t = trace([(f, w[f][0]), (j, w[j][0])], knobs=knobs)
                assert t.of_op(1) == ["call aux_join p%d %d" % (STREAM, overlap)] + w[j][1][1:]
        # the first DENSE_BWD behind an auxiliary memset joins, the second does not; behind an auxiliary scatter none does
        t = trace([("AUX_MEMSET0", w["AUX_MEMSET0"][0]), ("GATHER_F32", w["GATHER_F32"][0]), bwd, bwd], knobs=knobs)
        assert [c for c in t.calls() if c in ("aux_fork", "aux_join", "dense_bwd_overlapped")] == \
            (["aux_fork", "aux_join", "dense_bwd_overlapped", "dense_bwd_overlapped", "aux_join"] if overlap else
             ["dense_bwd_overlapped", "dense_bwd_overlapped", "aux_join"])
        t = trace([("AUX_SCATTER_ROWS", w["AUX_SCATTER_ROWS"][0]), bwd], knobs=knobs)
        assert [c for c in t.calls() if c in ("aux_fork", "aux_join")] == (["aux_fork"] if overlap else []) + ["aux_join"]
        # nothing else forks or joins
        for name in sorted(set(OPS) - set(forkers) - set(joiners) - {"ALLREDUCE_AVG"}):
            t = trace([(name, w[name][0])], knobs=knobs)
            assert [c for c in t.calls() if c in ("aux_fork", "aux_join")] == ["aux_join"], name


# ---- 5. the exchange stream -------------------------------------------------------------------------------------------------
def _exchange_program(h, aux, h16=False):
    w = {n: sc.position_case(h, n) for n in OPS}
    apply_ = "HIST_APPLY_H16" if h16 else "HIST_APPLY"
    prog = [("GATHER_F32", w["GATHER_F32"][0])]
    for n in ("HIST_PACK", "ALLGATHER_I32"):
        prog.append((n, w[n][0][:-1] + [aux]))
    prog.append(("ALLREDUCE_AVG", w["ALLREDUCE_AVG"][0]))
    prog.append((apply_, w[apply_][0][:-1] + [aux]))
    return prog, w, apply_


@pytest.mark.parametrize("h16", [False, True], ids=["f32", "h16"])
def test_exchange_ops_on_the_three_streams(trace, h16):
    h = trace.header
    S = "p%d" % STREAM
    for aux in (0, 1, 2):
        prog, w, apply_ = _exchange_program(h, aux, h16)
        t = trace(prog, knobs={"env.SGCN_XCHG_NO_PROBE": 1, "runs": 2})
        side = {0: S, 1: "p%d" % sc.AUX, 2: "p101"}[aux]
        on_side = lambda name: w[name][1][0][:-len(S)] + side           # noqa: E731
        gather = on_side("ALLGATHER_I32").replace("sgcn_coll_allgather_i32", "sgcn_coll_allgather_x_i32" if aux == 2 else "sgcn_coll_allgather_i32")
        fork = {0: [], 1: ["call aux_fork " + S], 2: []}[aux]
        create = ["call hipStreamCreateWithFlags p101 1", "call hipEventCreateWithFlags p201 1 1", "call hipEventCreateWithFlags p202 1 1"]
        first = ["call hipEventRecord p201 " + S, "call hipStreamWaitEvent p101 p201 0"]
        for r in (0, 1):
            want = sc.prologue() + w["GATHER_F32"][1] + [hook(0, "GATHER_F32", 4)]
            want += (fork if aux < 2 else (create if r == 0 else []) + first) + [on_side("HIST_PACK"), hook(1, "HIST_PACK", 8)]
            want += fork + [gather, hook(2, "ALLGATHER_I32", 4)]
            # the gradient all-reduce joins the AUXILIARY stream only: no event of the exchange stream in front of it
            want += ["call aux_join %s %d" % (S, aux == 1)] + w["ALLREDUCE_AVG"][1][1:] + [hook(3, "ALLREDUCE_AVG", 2)]
            want += fork + [on_side(apply_), hook(4, apply_, 8)]
            want += ["call aux_join %s %d" % (S, aux == 1)]
            want += ["call hipEventRecord p202 p101", "call hipStreamWaitEvent %s p202 0" % S] if aux == 2 else []
            want += sc.cleanup()
            assert t.runs[r]["ret"] == 0 and t.body(r) == want, (aux, r)
    # SGCN_XCHG_SKIP alone changes nothing; with its companion spelled out it drops the dependency it names
    prog, w, apply_ = _exchange_program(h, 2, h16)
    base = trace(prog, knobs={"env.SGCN_XCHG_NO_PROBE": 1})
    for skip in ("fork", "join", "fork,join"):
        t = trace(prog, knobs={"env.SGCN_XCHG_NO_PROBE": 1, "env.SGCN_XCHG_SKIP": skip})
        assert t.body() == base.body()
        t = trace(prog, knobs={"env.SGCN_XCHG_NO_PROBE": 1, "env.SGCN_XCHG_SKIP": skip, "env.SGCN_XCHG_DROPS_A_DEPENDENCY": 1})
        dropped = [ln for ln in base.body() if ("fork" in skip and "p201" in ln and "Create" not in ln) or
                   ("join" in skip and "p202" in ln and "Create" not in ln)]
        assert len(dropped) == 2 * len(skip.split(",")) and t.body() == [ln for ln in base.body() if ln not in dropped]
    # a failing exchange op: both side streams are joined before the run returns
    t = trace(prog, knobs={"env.SGCN_XCHG_NO_PROBE": 1, "rc.sgcn_coll_allgather_x_i32": -2})
    assert t.ret == -2 and t.body()[-7:] == ["call aux_join %s 0" % S, "call hipEventRecord p202 p101", "call hipStreamWaitEvent %s p202 0" % S] + sc.cleanup()


def test_exchange_stream_is_probed_once(trace):
    prog, w, _ = _exchange_program(trace.header, 2)
    t = trace(prog, knobs={"runs": 2})
    made = [ln.split()[2] for ln in t.body() if ln.startswith("call hipStreamCreateWithFlags")]
    gone = [ln.split()[2] for ln in t.body() if ln.startswith("call hipStreamDestroy")]
    kept = sorted(set(made) - set(gone))
    assert 1 <= len(made) <= 8 and len(kept) == 1 and len(gone) == len(made) - 1
    assert t.body().count("call spin_launch p%d 3000" % STREAM) == len(made)
    assert [ln.split()[-1] for ln in t.body() if ln.startswith("call sgcn_hist_pack_f32")] == kept
    assert not any("Create" in ln or "spin_launch" in ln for ln in t.body(1))
    assert [ln.split()[-1] for ln in t.body(1) if ln.startswith("call sgcn_coll_allgather_x_i32")] == kept


# ---- 6. peephole boundaries ---------------------------------------------------------------------------------------------------
X, W, Y, W2, Y2 = 20000, 30000, 40000, 50000, 60000


def _head_cases():
    """(id, DENSE_FWD keywords, loss keywords, knobs, does the output layer fold into the loss at fuse bit 0)"""
    M = 200

    def case(id_, folds, N=64, Kd=128, knobs=None, ce_kw=None, **kw):
        f = dict(M=M, N=N, Kd=Kd, X=X, ldx=Kd, W=W, ldw=N, Y=Y, ldy=N)
        f.update(kw)
        c = dict(z=Y, ldz=N, n=M, c=N)
        c.update(ce_kw or {})
        return pytest.param(f, c, knobs or {}, folds, id=id_)
    return [case("N64_K128", True), case("N65", False, N=65), case("K129", False, Kd=129), case("N1_K1", True, N=1, Kd=1),
            case("X2", False, X2=X + 64, ldx2=128, split=100), case("g1", False, g1=900), case("g2_only", True, g2=900),
            case("layernorm", False, off=910, sc=920, xhat=930, rstd=940), case("scale_only", False, sc=920), case("relu", False, relu=1),
            case("S2", False, knobs={"fwd_S": 2}), case("kgroups2", True, knobs={"fwd_kgroups": 2}), case("kgroups3", False, knobs={"fwd_kgroups": 3}),
            case("z_differs", False, ce_kw={"z": Y + 4}), case("ldz_differs", False, ce_kw={"ldz": 68}),
            case("n_differs", False, ce_kw={"n": M - 1}), case("c_differs", False, ce_kw={"c": 63})]


@pytest.mark.parametrize("f,c,knobs,folds", _head_cases())
def test_output_layer_folds_into_the_loss_only_within_its_bounds(trace, f, c, knobs, folds):
    prog = [("DENSE_FWD", sc.dense_fwd(**f)), ("SOFTMAX_CE", sc.ce(**c))]
    for fuse in FUSE:
        t = trace(prog, knobs=dict(knobs, step_fuse=fuse))
        assert t.ret == 0
        want = folds and bool(fuse & 1)
        assert sc.account(t, 2) == {0: "folded" if want else "launched", 1: "launched"}, fuse
        assert t.hooks() == [(0, OP["DENSE_FWD"], 27, 27, 0), (1, OP["SOFTMAX_CE"], 12, 12, 0)]
        loss = t.of_op(1)[0]
        if want:        # the loss call carries the layer: W, ldw, K, then its input as the head with the launch's K-groups
            assert t.calls().count("sgcn_dense_fwd_f32") == 0
            assert " last( p%d %d %d tail p0 0 drop(null) head p%d %d %d drop(null) pre 0 )" % (
                W, f["ldw"], f["Kd"], X, f["ldx"], knobs.get("fwd_kgroups", 1)) in loss
        else:
            assert t.calls().count("sgcn_dense_fwd_f32") == 1 and loss.endswith(" last(null)")


def _pre_cases():
    M = 300

    def case(id_, folds, N=128, Kd=256, qN=64, f_kw=None, q_kw=None, ce_kw=None, knobs=None):
        f = dict(M=M, N=N, Kd=Kd, X=X, ldx=Kd, W=W, ldw=N, Y=Y, ldy=N, off=910, sc=920, relu=1, xhat=930, rstd=940)
        f.update(f_kw or {})
        q = dict(M=M, N=qN, Kd=N, X=Y, ldx=N, W=W2, ldw=qN, Y=Y2, ldy=qN)
        q.update(q_kw or {})
        c = dict(z=Y2, ldz=qN, n=M, c=qN)
        c.update(ce_kw or {})
        return pytest.param(f, q, c, knobs or {}, folds, id=id_)
    return [case("N128_K256_at_160KiB", True), case("N129", False, N=129), case("K257", False, Kd=257),
            case("N64_K256", True, N=64), case("N64_K257_within_160KiB", False, N=64, Kd=257),
            case("KN_not_a_multiple_of_4", False, N=127, Kd=255), case("KN_a_multiple_of_4", True, N=127, Kd=252),
            case("ldw_differs", False, f_kw={"ldw": 132}), case("q_ldw_differs", False, q_kw={"ldw": 68}),
            case("X2", False, f_kw=dict(X2=X + 64, ldx2=256, split=100)), case("g1", False, f_kw={"g1": 900}),
            case("plain_lower_layer", True, f_kw=dict(off=0, sc=0, relu=0, xhat=0, rstd=0)),
            case("q_reads_other_rows", False, q_kw={"X": Y + 512}), case("q_M_differs", False, q_kw={"M": M - 1}),
            case("q_relu", False, q_kw={"relu": 1}), case("S0_3", False, knobs={"fwd_S": 3}), case("loss_reads_elsewhere", False, ce_kw={"z": Y2 + 4})]


@pytest.mark.parametrize("f,q,c,knobs,folds", _pre_cases())
def test_pre_layer_folds_only_within_its_bounds(trace, f, q, c, knobs, folds):
    prog = [("DENSE_FWD", sc.dense_fwd(**f)), ("DENSE_FWD", sc.dense_fwd(**q)), ("SIGMOID_CE", sc.ce(**c))]
    # when the pre-layer does not fold, the output layer alone still may (the rules of the test above)
    q_heads = (q["N"] <= 64 and q["Kd"] <= 128 and not q.get("relu") and knobs.get("fwd_S", 1) == 1 and
               c["z"] == q["Y"] and c["ldz"] == q["ldy"] and c["n"] == q["M"] and c["c"] == q["N"])
    for fuse in FUSE:
        t = trace(prog, knobs=dict(knobs, step_fuse=fuse))
        assert t.ret == 0
        pre = folds and (fuse & 17) == 17
        if pre:
            assert sc.account(t, 3) == {0: "folded", 1: "skipped", 2: "launched"}, fuse
            assert t.calls().count("sgcn_dense_fwd_f32") == 0
            assert " head p0 %d 1 drop(null) pre 1 p%d %d %d p%d " % (q["ldx"], X, f["ldx"], f["Kd"], W) in t.of_op(2)[0]
        else:
            head = q_heads and bool(fuse & 1)
            assert sc.account(t, 3) == {0: "launched", 1: "folded" if head else "launched", 2: "launched"}, fuse
            assert t.calls().count("sgcn_dense_fwd_f32") == (1 if head else 2)
            assert " pre 1 " not in t.of_op(2)[0]
        assert all(hk[2] == hk[3] and hk[4] == 0 for hk in t.hooks())


def _pair_cases():
    M = 400

    def case(id_, taken, q_kw=None, f_kw=None, knobs=None):
        f = dict(M=M, N=128, Kd=512, X=X, ldx=512, W=W, ldw=128, Y=Y, ldy=128, off=910, sc=920, relu=1, xhat=930, rstd=940)
        f.update(f_kw or {})
        q = dict(M=M, N=32, Kd=128, X=Y, ldx=128, W=W2, ldw=32, Y=Y2, ldy=32, relu=1)
        q.update(q_kw or {})
        return pytest.param(f, q, dict({"gemm_ws": 4096}, **(knobs or {})), taken, id=id_)
    return [case("all_rows", True), case("no_split_K", False, knobs={"gemm_ws": 0}), case("fewer_rows", False, q_kw={"M": M - 1}),
            case("other_rows", False, q_kw={"X": Y + 512}), case("other_pitch", False, q_kw={"ldx": 256}), case("gathered", False, q_kw={"g1": 900}),
            case("gathered_second", False, q_kw={"g2": 900}), case("K_differs", False, q_kw={"Kd": 64}),
            case("two_halves_of_this_layer", True, q_kw=dict(M=M, X2=Y + 100 * 128 * 4, ldx2=128, split=100)),
            case("second_half_elsewhere", False, q_kw=dict(X2=Y + 101 * 128 * 4, ldx2=128, split=100))]


@pytest.mark.parametrize("f,q,knobs,taken", _pair_cases())
def test_dense_fwd_pair_only_when_the_next_layer_reads_all_rows(trace, f, q, knobs, taken):
    prog = [("DENSE_FWD", sc.dense_fwd(**f)), ("DENSE_FWD", sc.dense_fwd(**q))]
    for fuse in FUSE:
        for fused in (1, 0):
            t = trace(prog, knobs=dict(knobs, step_fuse=fuse, pair_fused=fused))
            assert t.ret == 0
            pair = taken and bool(fuse & 4)
            assert t.calls().count("dense_fwd_pair") == int(pair)
            if pair and fused:
                assert sc.account(t, 2) == {0: "launched", 1: "skipped"} and "sgcn_dense_fwd_f32" not in t.calls()
                line = t.of_op(0)[0]
                assert line.startswith("call dense_fwd_pair %d 128 512 p%d 512 " % (f["M"], X)) and " | 32 p%d 32 " % W2 in line
            else:           # (the kernel may decline: then both layers are launched as usual)
                assert sc.account(t, 2) == {0: "launched", 1: "launched"} and t.calls().count("sgcn_dense_fwd_f32") == 2


def test_backward_folds_account_for_every_op(trace):
    """the loss kernel's dx tail (fuse bit 1), the backward chain (bit 6) and the scatters in the optimizer's launch"""
    M, c, Kd = 200, 40, 96
    loss = ("SOFTMAX_CE", sc.ce(Y, c, M, c))
    up = ("DENSE_BWD", sc.dense_bwd(M, c, Kd, 6100, c, W, c, dx=7300))
    lo = ("DENSE_BWD", sc.dense_bwd(M, Kd, 64, 7300, Kd, W2, Kd, dx=0, xhat=930, rstd=940, sc=920, relu=1))
    prog = [loss, up, lo, ("ADAM", sc.adam()), ("SCATTER_ROWS", sc.scatter(8500)), ("SCATTER_ROWS", sc.scatter(9500)),
            ("SCATTER_ROWS", sc.scatter(10500))]
    for fuse in (0, 2, 64, 66, 127):
        for park in (1, 0):
            t = trace(prog, knobs={"step_fuse": fuse, "scatter_park": park})
            assert t.ret == 0
            got = sc.account(t, len(prog))
            tail = bool(fuse & 2)
            assert (" tail p7300 %d " % Kd in t.of_op(0)[0]) == tail
            if tail:        # that op then only records its weight gradient: no dx of its own, and it cannot head a chain
                assert t.of_op(1)[0].split()[21] == "p0" and got[2] == "launched"
            elif fuse & 64:
                assert t.of_op(1)[0].startswith("call dense_bwd_chain") and got[2] == "skipped"
            else:
                assert got[1] == got[2] == "launched" and t.calls().count("dense_bwd_overlapped") == 2
            # up to two fp32 scatters directly behind the optimizer ride in its launch; the third is a launch of its own
            assert [got[4], got[5], got[6]] == (["skipped", "skipped", "launched"] if park else ["launched"] * 3)
            assert t.calls().count("scatter_park") == (2 if park else 1)
            assert all(hk[2] == hk[3] and hk[4] == 0 for hk in t.hooks())


def test_short_and_long_argument_lists_show_in_the_hook(trace):
    """what the hook is for: a list one word short is read past its end, a list one word long is not consumed"""
    w, _ = sc.position_case(trace.header, "GATHER_ROWS")
    t = trace([sc.make_op("GATHER_ROWS", w, nargs=6)])
    assert t.hooks() == [(0, OP["GATHER_ROWS"], 6, 6, 1)] and t.of_op(0)[0].split()[-2] == "0"
    t = trace([("GATHER_ROWS", w + [5])])
    assert t.hooks() == [(0, OP["GATHER_ROWS"], 8, 7, 0)]
