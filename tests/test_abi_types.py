"""The hand-kept Python copies of include/sgcn.h against the header itself, with the compiler as the parser (no GPU).

tests/abi_dump.py compiles a translation unit that includes the header and prints every prototype (through
``decltype(&name)``), the layout of every struct ``_ffi`` restates, every ``SGCN_OP_*`` enumerator and the constants Python
restates.  test_abi.py keeps comparing the SETS of names; this file compares the TYPES.

The rules (abi_dump.ctype_matches / compare_structs):
  * integers and floats: width, signedness and kind match exactly -- ``c_int32`` binds ``int32_t`` only, ``c_int64``
    ``int64_t`` only, ``c_uint32`` ``uint32_t`` only, ``c_float`` / ``c_double`` their own kind; ``c_int`` counts as ``int32_t``
    (the header's ``int`` results);
  * ``c_void_p`` binds any pointer;
  * ``POINTER(T)`` binds only a pointer whose pointee is ``T`` (constness aside); a struct pointee is bound by name and its
    layout is checked field by field;
  * ``POINTER(c_void_p)`` and ``POINTER(POINTER(..))`` bind pointer-to-pointer only;
  * ``c_char_p`` binds ``char*`` only;
  * results follow the same rules, ``None`` binds ``void``;
  * argument counts are equal;
  * struct fields: the ctypes field names exist in the header (else the dump does not compile), in the same order, with the
    same offset, size and kind (signed / unsigned / floating / pointer, and the element size of an array); total sizes are equal;
  * ``step_program.OP`` equals the enum's map without the ``SGCN_OP_`` prefix, in both directions;
  * ``_ffi.STEP_MAX_ARGS``, ``step_program.MAX_ARGS``, ``_ffi.ABI_VERSION`` (the header states its version in the sentence above
    ``sgcn_abi_version``; the library's own answer is test_abi.py's) and the dropout-site / plan constants of ops.py and
    models.py equal the header's.

Sensitivity: the comparer takes the tables as arguments, and PERTURBATIONS feeds it copies with one mistake each -- the
mistakes that survive every GPU test at test sizes -- and asserts that each is reported with the function and the position
named, and nothing else.

Measured: the C++ unit builds and runs in under 1 s, the C unit in 0.1 s; the whole file takes 1 s.
"""
import ctypes as C

import pytest

import abi_dump
from stochastic_gcn_amd import _ffi, step_program


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    return abi_dump.dump(tmp_path_factory.mktemp("abi_dump"))


def _structs(ffi=_ffi):
    return {cname: getattr(ffi, py) for py, cname in abi_dump.STRUCTS.items()}


def _restated_constants():
    from stochastic_gcn_amd import models, ops
    return {"SGCN_STEP_MAX_ARGS": _ffi.STEP_MAX_ARGS, "ABI_VERSION": _ffi.ABI_VERSION, "SGCN_AGG_PLAN_T": models.AGG_PLAN_T,
            "SGCN_ATTN_SITE": ops.ATTN_SITE, "SGCN_EDGE_SITE": ops.EDGE_SITE, "SGCN_EDGE_ALWAYS": ops.EDGE_ALWAYS}


def test_dump_covers_the_header(header):
    assert len(header.fn) == len(abi_dump.header_functions()) >= 160
    assert set(header.size) == set(abi_dump.STRUCTS.values())
    assert sum(len(getattr(_ffi, py)._fields_) for py in abi_dump.STRUCTS) == len(header.field) >= 85
    assert len(header.enum) >= 51 and header.const["SGCN_STEP_MAX_ARGS"] == 48
    # every type the header uses has a canonical name, but for the opaque handles (which only c_void_p may bind)
    seen = {t.rstrip("*") for res, args in header.fn.values() for t in [res] + args}
    assert seen <= set(abi_dump.LEAVES) | {"opaque"}, sorted(seen)
    assert not any(t == "opaque" for res, args in header.fn.values() for t in [res] + args), "an opaque struct by value"


def test_signatures_bind_the_headers_types(header):
    bad = abi_dump.compare_signatures(header, _ffi.SIGNATURES)
    assert bad == [], "\n".join(m for _, _, m in bad)


def test_struct_layouts_are_the_headers(header):
    bad = abi_dump.compare_structs(header, _structs())
    assert bad == [], "\n".join(m for _, _, m in bad)


def test_step_ops_and_constants_are_the_headers(header):
    bad = abi_dump.compare_ops(header, step_program.OP)
    assert bad == [], "\n".join(m for _, m in bad)
    assert len(set(step_program.OP.values())) == len(step_program.OP)
    bad = abi_dump.compare_constants(header, _restated_constants())
    assert bad == [], "\n".join(m for _, m in bad)
    assert step_program.MAX_ARGS == header.const["SGCN_STEP_MAX_ARGS"]
    assert C.sizeof(_ffi.StepOp) == 8 + 20 * header.const["SGCN_STEP_MAX_ARGS"]
    assert (header.const["SGCN_OK"], header.const["SGCN_ERR_INVALID"], header.const["SGCN_ERR_HIP"]) == (0, -1, -2)


def test_header_is_a_c_header_with_the_same_layouts(header, tmp_path):
    c = abi_dump.dump_c(tmp_path)
    assert c.size == header.size and c.enum == header.enum and c.const == header.const
    assert c.field == {k: v[:2] for k, v in header.field.items()}


# ---- sensitivity -----------------------------------------------------------------------------------------------------
def _with_arg(name, j, t, was):
    def make():
        sig = dict(_ffi.SIGNATURES)
        res, args = sig[name]
        assert args[j] is was or args[j] == was, "the perturbation no longer applies: %s[%d] is %r" % (name, j, args[j])
        sig[name] = (res, list(args[:j]) + [t] + list(args[j + 1:]))
        return sig
    return make


def _with_result(name, t, was):
    def make():
        sig = dict(_ffi.SIGNATURES)
        assert sig[name][0] is was
        sig[name] = (t, sig[name][1])
        return sig
    return make


def _dropped_last(name):
    def make():
        sig = dict(_ffi.SIGNATURES)
        sig[name] = (sig[name][0], list(sig[name][1][:-1]))
        return sig
    return make


def _restruct(py, edit):
    """a copy of the struct table with _ffi.<py>'s field list edited"""
    def make():
        fields = edit(list(getattr(_ffi, py)._fields_))
        cls = type(py, (C.Structure,), {"_fields_": fields})
        out = _structs()
        out[abi_dump.STRUCTS[py]] = cls
        return out
    return make


def _swap(a, b):
    def edit(fields):
        names = [f[0] for f in fields]
        i, j = names.index(a), names.index(b)
        assert j == i + 1
        fields[i], fields[j] = fields[j], fields[i]
        return fields
    return edit


def _retype(name, t):
    return lambda fields: [(f[0], t) if f[0] == name else f for f in fields]


# (id, kind, maker, the (function | struct | op, position | field) that must be reported -- and nothing else)
PERTURBATIONS = [
    ("int64_as_int32_on_the_stack", "sig", _with_arg("sgcn_spmm_csr_f32", 7, C.c_int32, C.c_int64), ("sgcn_spmm_csr_f32", 7)),
    ("int64_as_int32_last_register", "sig", _with_arg("sgcn_csr_transpose_index", 1, C.c_int32, C.c_int64), ("sgcn_csr_transpose_index", 1)),
    ("int32_as_uint32", "sig", _with_arg("sgcn_plan_fill", 1, C.c_uint32, C.c_int32), ("sgcn_plan_fill", 1)),
    ("uint32_as_int32", "sig", _with_arg("sgcn_gauss_sample_f32", 3, C.c_int32, C.c_uint32), ("sgcn_gauss_sample_f32", 3)),
    ("float_as_double", "sig", _with_arg("sgcn_spmm_csr_f32", 13, C.c_double, C.c_float), ("sgcn_spmm_csr_f32", 13)),
    ("double_as_float", "sig", _with_arg("sgcn_cs_warp_table", 5, C.c_float, C.c_double), ("sgcn_cs_warp_table", 5)),
    ("dropped_trailing_argument", "sig", _dropped_last("sgcn_gather_rows_f32"), ("sgcn_gather_rows_f32", -2)),
    ("ws_floats_result_as_int", "sig", _with_result("sgcn_gemm_ws_floats", C.c_int, C.c_int64), ("sgcn_gemm_ws_floats", -1)),
    ("void_result_as_int", "sig", _with_result("sgcn_sched_destroy", C.c_int, None), ("sgcn_sched_destroy", -1)),
    ("int64_out_as_int32_out", "sig", _with_arg("sgcn_plan_count", 3, C.POINTER(C.c_int32), C.POINTER(C.c_int64)), ("sgcn_plan_count", 3)),
    ("int32_out_as_int64_out", "sig", _with_arg("sgcn_csbuild_sizes", 5, C.POINTER(C.c_int64), C.POINTER(C.c_int32)), ("sgcn_csbuild_sizes", 5)),
    ("handle_out_as_plain_pointer", "sig", _with_arg("sgcn_mult_create", 2, C.POINTER(C.c_int32), C.POINTER(C.c_void_p)), ("sgcn_mult_create", 2)),
    ("name_as_int_pointer", "sig", _with_arg("sgcn_tune", 0, C.POINTER(C.c_int32), C.c_char_p), ("sgcn_tune", 0)),
    ("plan_as_another_struct", "sig", _with_arg("sgcn_spmm_cs_f32", 0, C.POINTER(_ffi.Plan), C.POINTER(_ffi.CsPlan)), ("sgcn_spmm_cs_f32", 0)),
    ("csplan_fields_swapped", "struct", _restruct("CsPlan", _swap("nfix", "nslots")), ("sgcn_csplan_t", "nfix")),
    ("csplan_fields_of_two_widths_swapped", "struct", _restruct("CsPlan", _swap("R", "ntiles")), ("sgcn_csplan_t", "ntiles")),
    ("stepop_slot_widened", "struct", _restruct("StepOp", _retype("slot", C.c_int64 * _ffi.STEP_MAX_ARGS)), ("sgcn_step_op_t", "slot")),
    ("dropout_key_signed", "struct", _restruct("Dropout", _retype("key", C.c_int32)), ("sgcn_dropout_t", "key")),
    ("dropout_keep_as_int", "struct", _restruct("Dropout", _retype("keep", C.c_int32)), ("sgcn_dropout_t", "keep")),
    ("op_off_by_one", "op", lambda: dict(step_program.OP, GRAD_STORE=step_program.OP["GRAD_STORE"] + 1), ("GRAD_STORE", None)),
    ("op_unknown_to_python", "op", lambda: {k: v for k, v in step_program.OP.items() if k != "ADAM_EMA"}, ("ADAM_EMA", None)),
    ("op_unknown_to_the_header", "op", lambda: dict(step_program.OP, DENSE_FWD_PAIR=18), ("DENSE_FWD_PAIR", None)),
    ("max_args_off", "const", lambda: dict(_restated_constants(), SGCN_STEP_MAX_ARGS=47), ("SGCN_STEP_MAX_ARGS", None)),
    ("abi_version_behind", "const", lambda: dict(_restated_constants(), ABI_VERSION=_ffi.ABI_VERSION - 1), ("ABI_VERSION", None)),
]


@pytest.mark.parametrize("kind,make,want", [pytest.param(k, m, w, id=i) for i, k, m, w in PERTURBATIONS])
def test_comparer_reports_the_perturbation_and_only_it(header, kind, make, want):
    table = make()
    if kind == "sig":
        bad = abi_dump.compare_signatures(header, table)
        assert [(f, j) for f, j, _ in bad] == [want], bad
        assert want[0] in bad[0][2]
    elif kind == "struct":
        bad = abi_dump.compare_structs(header, table)
        assert bad and (want[0], want[1]) in [(s, f) for s, f, _ in bad], bad
        assert {s for s, _, _ in bad} == {want[0]}, bad
    elif kind == "op":
        bad = abi_dump.compare_ops(header, table)
        assert [k for k, _ in bad] == [want[0]], bad
    else:
        bad = abi_dump.compare_constants(header, table)
        assert [k for k, _ in bad] == [want[0]], bad


def test_a_field_the_header_lacks_does_not_compile(tmp_path):
    class Fake(object):
        pass
    for py in abi_dump.STRUCTS:
        setattr(Fake, py, getattr(_ffi, py))
    Fake.Fix = type("Fix", (C.Structure,), {"_fields_": [("row", C.c_int32), ("first_slot", C.c_int32), ("n_slots", C.c_int32)]})
    with pytest.raises(AssertionError, match="n_slots"):
        abi_dump.dump(tmp_path, ffi=Fake)
