"""include/sgcn.h as the compiler sees it, and the comparison of the hand-kept Python copies with it.

``dump(tmp_dir)`` writes a C++ translation unit that includes the header and, for every function name the header declares
(test_abi._header_symbols' regular expression: it supplies NAMES only), prints the return and parameter types through a
variadic template on ``decltype(&name)`` -- nothing is ODR-used, so nothing is linked.  It also prints sizeof / offsetof /
kind of every struct ``_ffi`` restates (by the ctypes field names: a name the header lacks does not compile), every
enumerator of the ``SGCN_OP_*`` enum and the constants Python restates.  ``dump_c`` builds the struct / constant part once
more as C11.  ``compare`` takes the Python tables as ARGUMENTS, so that test_abi_types.py can feed it perturbed copies.
The rules are stated in test_abi_types.py's docstring; tests/step_trace_cases.py generates its stubs from the same dump.

Lines of the dump:
    fn <name> <ret> <arg> ...          canonical type names, see CANON
    struct <c name> <sizeof>
    field <c name> <field> <offsetof> <sizeof> <kind> <element size>     kind: signed | unsigned | floating | pointer
    enum <enumerator> <value>
    const <macro> <value>
"""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "sgcn.h")

# the eight layouts _ffi restates -> their names in the header
STRUCTS = {"Seg": "sgcn_seg_t", "Fix": "sgcn_fix_t", "Plan": "sgcn_plan_t", "CsPlan": "sgcn_csplan_t",
           "LdsPlan": "sgcn_ldsplan_t", "StepOp": "sgcn_step_op_t", "StepFill": "sgcn_step_fill_t", "Dropout": "sgcn_dropout_t"}
# canonical leaf names; any other pointee (the opaque handles) prints as `opaque`
LEAVES = ["int32_t", "uint32_t", "int64_t", "uint64_t", "uint16_t", "float", "double", "char", "void"] + sorted(STRUCTS.values())
CANON = {C.c_int32: "int32_t", C.c_uint32: "uint32_t", C.c_int64: "int64_t", C.c_uint64: "uint64_t", C.c_uint16: "uint16_t",
         C.c_float: "float", C.c_double: "double", C.c_char: "char"}
CONSTANTS = ["SGCN_STEP_MAX_ARGS", "SGCN_AGG_PLAN_T", "SGCN_ATTN_SITE", "SGCN_EDGE_SITE", "SGCN_EDGE_ALWAYS", "SGCN_OK", "SGCN_ERR_INVALID", "SGCN_ERR_HIP"]
BUILD_TIMEOUT_S = 120          # the C++ unit compiles in about 2 s, the C unit in 0.1 s


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_functions():
    from test_abi import _header_symbols
    return sorted(_header_symbols())


def header_enumerators():
    return sorted(set(re.findall(r"\b(SGCN_OP_[A-Z0-9_]+)\s*=", header_text())))


def header_abi_version():
    """The header keeps its version in the sentence above sgcn_abi_version() (there is no macro): that number."""
    m = re.search(r"ABI version of this header[^:]*:\s*(\d+)\.", open(HEADER).read())
    assert m, "include/sgcn.h no longer states its ABI version above sgcn_abi_version()"
    return int(m.group(1))


def struct_fields(ffi):
    """{c name: [ctypes field names]} of the layouts `ffi` restates"""
    return {cname: [f[0] for f in getattr(ffi, py)._fields_] for py, cname in STRUCTS.items()}


def _body(fields, cxx):
    out = []
    for cname in sorted(fields):
        out.append('    printf("struct %s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in fields[cname]:
            if cxx:
                out.append('    field<decltype(%s::%s)>("%s", "%s", offsetof(%s, %s));' % (cname, f, cname, f, cname, f))
            else:
                out.append('    printf("field %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (cname, f, cname, f, cname, f))
    for e in header_enumerators():
        out.append('    printf("enum %s %%lld\\n", (long long)%s);' % (e, e))
    for c in CONSTANTS:
        out.append('    printf("const %s %%lld\\n", (long long)%s);' % (c, c))
    return out


def source_cxx(fields):
    src = ['#include <cstddef>', '#include <cstdint>', '#include <cstdio>', '#include <type_traits>', '#include "sgcn.h"',
           'template <class T> struct N { static void p() { printf("opaque"); } };']
    src += ['template <> struct N<%s> { static void p() { printf("%s"); } };' % (t, t) for t in LEAVES]
    src += ['template <class T> struct N<const T> { static void p() { N<T>::p(); } };',
            'template <class T> struct N<T*> { static void p() { N<T>::p(); printf("*"); } };',
            'template <class R, class... A> void sig(const char* name, R (*)(A...)) {',
            '    printf("fn %s ", name); N<R>::p(); ((printf(" "), N<A>::p()), ...); printf("\\n");',
            '}',
            'template <class F> void field(const char* s, const char* f, size_t off) {',
            '    using E = typename std::remove_cv<typename std::remove_all_extents<F>::type>::type;',
            '    const char* kind = std::is_pointer<E>::value ? "pointer" : std::is_floating_point<E>::value ? "floating"',
            '                     : std::is_integral<E>::value ? (std::is_signed<E>::value ? "signed" : "unsigned") : "other";',
            '    printf("field %s %s %zu %zu %s %zu\\n", s, f, off, sizeof(F), kind, sizeof(E));',
            '}',
            'int main() {']
    src += ['    sig("%s", (decltype(&%s))nullptr);' % (n, n) for n in header_functions()]
    src += _body(fields, True) + ['    return 0;', '}', '']
    return "\n".join(src)


def source_c(fields):
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "sgcn.h"', 'int main(void) {']
    return "\n".join(src + _body(fields, False) + ['    return 0;', '}', ''])


def _build_and_run(compiler, flags, text, path):
    with open(path, "w") as f:
        f.write(text)
    exe = os.path.splitext(path)[0]
    r = subprocess.run([compiler] + flags + ["-I", INCLUDE, path, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=BUILD_TIMEOUT_S)
    assert r.returncode == 0, "the header dump does not compile (a ctypes field the header lacks?):\n" + r.stdout[-6000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=BUILD_TIMEOUT_S)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    return r.stdout.splitlines()


class Dump(object):
    def __init__(self, lines):
        self.lines = lines
        self.fn, self.size, self.field, self.enum, self.const = {}, {}, {}, {}, {}
        for ln in lines:
            t = ln.split()
            if t[0] == "fn":
                self.fn[t[1]] = (t[2], t[3:])
            elif t[0] == "struct":
                self.size[t[1]] = int(t[2])
            elif t[0] == "field":
                self.field[(t[1], t[2])] = (int(t[3]), int(t[4])) + ((t[5], int(t[6])) if len(t) > 5 else ())
            elif t[0] == "enum":
                self.enum[t[1]] = int(t[2])
            elif t[0] == "const":
                self.const[t[1]] = int(t[2])
            else:
                raise AssertionError("unknown dump line: " + ln)


def dump(tmp_dir, ffi=None):
    if ffi is None:
        from stochastic_gcn_amd import _ffi as ffi
    return Dump(_build_and_run("g++", ["-std=c++17", "-Wall", "-Werror"], source_cxx(struct_fields(ffi)), os.path.join(str(tmp_dir), "abi_dump.cpp")))


def dump_c(tmp_dir, ffi=None):
    if ffi is None:
        from stochastic_gcn_amd import _ffi as ffi
    return Dump(_build_and_run("gcc", ["-std=c11", "-Wall", "-Werror", "-pedantic"], source_c(struct_fields(ffi)), os.path.join(str(tmp_dir), "abi_dump_c.c")))


# ---- the ctypes side ---------------------------------------------------------------------------------------------------
def _is_pointer(t):
    return isinstance(t, type) and issubclass(t, C._Pointer)


def ctype_matches(t, c, struct_names):
    """Does ctypes type `t` (None = no result) bind the C type with canonical name `c`?"""
    if t is None:
        return c == "void"
    if t is C.c_void_p:
        return c.endswith("*")
    if t is C.c_char_p:
        return c == "char*"
    if _is_pointer(t):
        inner = t._type_
        if inner is C.c_void_p or inner is C.c_char_p or _is_pointer(inner):
            return c.endswith("**")
        if isinstance(inner, type) and issubclass(inner, C.Structure):
            return c == struct_names.get(inner.__name__, "?") + "*"        # (the pointee's layout: compare_structs)
        return inner in CANON and c == CANON[inner] + "*"
    return t in CANON and c == CANON[t]


def ctype_name(t):
    if t is None:
        return "None"
    return getattr(t, "__name__", repr(t))


def compare_signatures(d, signatures, struct_names=None):
    """[(function, position, message)]: position -1 = the result, -2 = the argument count, -3 = the set of names"""
    names = dict(STRUCTS if struct_names is None else struct_names)
    bad = []
    for name in sorted(set(d.fn) ^ set(signatures)):
        bad.append((name, -3, "%s is %s" % (name, "not bound" if name in d.fn else "not declared by the header")))
    for name in sorted(set(d.fn) & set(signatures)):
        res, args = signatures[name]
        cres, cargs = d.fn[name]
        if not ctype_matches(res, cres, names):
            bad.append((name, -1, "%s: result %s bound as %s" % (name, cres, ctype_name(res))))
        if len(args) != len(cargs):
            bad.append((name, -2, "%s: %d parameters bound as %d" % (name, len(cargs), len(args))))
        for j, (t, c) in enumerate(zip(args, cargs)):
            if not ctype_matches(t, c, names):
                bad.append((name, j, "%s: parameter %d is %s, bound as %s" % (name, j, c, ctype_name(t))))
    return bad


def _field_kind(t):
    n = 1
    while isinstance(t, type) and issubclass(t, C.Array):
        n *= t._length_
        t = t._type_
    if t is C.c_void_p or t is C.c_char_p or _is_pointer(t):
        kind = "pointer"
    elif t in (C.c_float, C.c_double):
        kind = "floating"
    elif t in (C.c_int32, C.c_int64, C.c_int16, C.c_int8):
        kind = "signed"
    elif t in (C.c_uint32, C.c_uint64, C.c_uint16, C.c_uint8):
        kind = "unsigned"
    else:
        kind = "other"
    return kind, C.sizeof(t), n


def compare_structs(d, structs):
    """structs: {c name: ctypes.Structure subclass}.  [(struct, field or None, message)].  Order is implied: ctypes lays its
    fields out in ITS order by the C rules, so equal offsets, sizes and total size leave no room for a swap or a missing field."""
    bad = []
    for cname, cls in sorted(structs.items()):
        if C.sizeof(cls) != d.size.get(cname):
            bad.append((cname, None, "%s: sizeof %s, restated with %d" % (cname, d.size.get(cname), C.sizeof(cls))))
        last = -1
        for fname, ftype in [f[:2] for f in cls._fields_]:
            want = d.field.get((cname, fname))
            desc = getattr(cls, fname)
            kind, esize, _ = _field_kind(ftype)
            got = (desc.offset, desc.size, kind, esize)
            if want != got:
                bad.append((cname, fname, "%s.%s: (offset, size, kind, element size) %s, restated as %s" % (cname, fname, want, got)))
            if want is not None and want[0] <= last:
                bad.append((cname, fname, "%s.%s: out of the header's order" % (cname, fname)))
            last = want[0] if want is not None else last
    return bad


def compare_ops(d, op_map):
    """both directions: an enumerator Python does not know is a failure too"""
    want = {k[len("SGCN_OP_"):]: v for k, v in d.enum.items()}
    bad = []
    for k in sorted(set(want) | set(op_map)):
        if want.get(k) != op_map.get(k):
            bad.append((k, "OP %s: %s in the header, %s in step_program.OP" % (k, want.get(k), op_map.get(k))))
    return bad


def compare_constants(d, restated):
    """restated: {header macro (or 'ABI_VERSION'): the Python value}"""
    bad = []
    for k, v in sorted(restated.items()):
        want = header_abi_version() if k == "ABI_VERSION" else d.const.get(k)
        if want != v:
            bad.append((k, "%s: %s in the header, %s in Python" % (k, want, v)))
    return bad
