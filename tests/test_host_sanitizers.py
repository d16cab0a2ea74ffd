"""The host planners and the sampler (sgcn_plan.cpp, sgcn_csplan.cpp, sgcn_ldsplan.cpp, sgcn_sched.cpp) under
AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer, without a GPU.

tests/host_san/driver.cpp is linked with the four sources, unchanged, three times: ``plain`` (-O2), ``asan`` and ``tsan``
(runtimes linked statically: nothing is preloaded).  Every (build, battery, case) runs the driver once on a case of
host_san_cases.CASES and asserts that it exits 0, that it wrote nothing to stderr (a sanitizer's report would be there, and
so reaches the assertion message) and that its call lines equal the lines host_san_cases.expected computes through the
production libsgcn.so.  What the equality means is said in host_san_cases.py; DESIGN.md ("Host sanitizers") has the rest.

Measured on an 8-core machine: the builds take 11 s (plain), 38 s (asan) and 14 s (tsan) one after the other, 17 s with
every translation unit compiled side by side as the fixture does; the slowest case of every battery under ``tsan`` is the
community graph ``sbm`` (csplan 21 s, ldsplan 24 s, prefetch 3.2 s, sched 2.1 s, transpose 0.7 s, warp 0.3 s), and
TIMEOUT_S is about five times that; the whole file takes two and a half minutes.
"""
import os
import subprocess
import time

import pytest

import host_san_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stochastic_gcn_amd", "csrc")
SOURCES = [os.path.join(hc.DRIVER_DIR, "driver.cpp")] + [os.path.join(CSRC, f) for f in
                                                          ("sgcn_plan.cpp", "sgcn_csplan.cpp", "sgcn_ldsplan.cpp", "sgcn_sched.cpp")]
HOST_FLAGS = ["-std=c++17", "-pthread", "-ffp-contract=off", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]     # csrc/Makefile's
BUILDS = {
    "plain": ["-O2"],
    "asan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-static-libasan", "-static-libubsan"],
    "tsan": ["-O1", "-g", "-fsanitize=thread", "-static-libtsan"],
}
INIT_SYMBOL = {"asan": "__asan_init", "tsan": "__tsan_init"}
SANITIZER_ENV = {
    "ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1:detect_stack_use_after_return=1",
    "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1",
    "TSAN_OPTIONS": "halt_on_error=1:second_deadlock_stack=1:exitcode=66",
}
# seconds; about 5 x the slowest case under tsan (see the module docstring), so that a deadlock fails instead of blocking
TIMEOUT_S = {"plan": 10, "csplan": 110, "warp": 10, "transpose": 10, "reorder": 10, "ldsplan": 120, "mult": 10, "sched": 15,
             "prefetch": 20, "refusals": 10}
BUILD_TIMEOUT_S = 600

ON_GPU_MACHINE = os.path.exists("/dev/kfd")
NO_SANITIZERS_HERE = pytest.mark.skipif(ON_GPU_MACHINE, reason="sanitizer builds run on the CPU machine only: /dev/kfd exists, "
                                        "and sanitizer runs do not belong on the shared GPU machines")


def _params():
    out = []
    for build in BUILDS:
        for battery in hc.BATTERIES:
            if build == "tsan" and battery not in hc.THREADED:
                continue
            for name in hc.CASES:
                if hc.applies(battery, name):
                    out.append(pytest.param(build, battery, name, id="%s-%s-%s" % (build, battery, name),
                                            marks=() if build == "plain" else NO_SANITIZERS_HERE))
    return out


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    """{build: path of the driver}: built side by side, and checked to be what they claim to be"""
    d = tmp_path_factory.mktemp("host_san")
    wanted = [b for b in BUILDS if b == "plain" or not ON_GPU_MACHINE]
    procs, t0 = [], time.time()
    for b in wanted:                       # every translation unit of every build at once, then one link per build
        for src in SOURCES:
            obj = str(d / ("%s_%s.o" % (b, os.path.basename(src))))
            cmd = ["g++"] + BUILDS[b] + HOST_FLAGS + ["-c", src, "-o", obj]
            procs.append((b, obj, cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for b, _, cmd, p in procs:
        log, _ = p.communicate(timeout=BUILD_TIMEOUT_S)
        assert p.returncode == 0, "the %s build failed:\n%s\n%s" % (b, " ".join(cmd), log)
    for b in wanted:
        cmd = ["g++"] + BUILDS[b] + HOST_FLAGS + [obj for bb, obj, _, _ in procs if bb == b] + ["-o", str(d / b)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=BUILD_TIMEOUT_S)
        assert r.returncode == 0, "the %s build failed to link:\n%s\n%s" % (b, " ".join(cmd), r.stdout)
    print("host_san: %s built in %.0f s" % (", ".join(wanted), time.time() - t0))
    for b in wanted:
        symbols = subprocess.run(["nm", str(d / b)], stdout=subprocess.PIPE, text=True, check=True).stdout
        for which, sym in INIT_SYMBOL.items():
            assert (sym in symbols) == (which == b), "the %s build %s %s" % (b, "lacks" if which == b else "holds", sym)
        # the runtimes are static: none among the binary's own dependencies, neither as ldd resolves them (`name => path`
        # lines; a library that the environment preloads into every process is listed too, as a bare path, and is not the
        # binary's) nor in its dynamic section
        libs = subprocess.run(["ldd", str(d / b)], stdout=subprocess.PIPE, text=True, check=True).stdout
        needed = [ln.split("=>")[0].strip() for ln in libs.splitlines() if "=>" in ln]
        dynamic = subprocess.run(["readelf", "-d", str(d / b)], stdout=subprocess.PIPE, text=True, check=True).stdout
        needed += [ln for ln in dynamic.splitlines() if "(NEEDED)" in ln]
        assert len(needed) >= 2 and not any(s in n for n in needed for s in ("libasan", "libubsan", "libtsan")), \
            "a sanitizer runtime is linked dynamically:\n" + libs + dynamic
    return {b: str(d / b) for b in wanted}


@pytest.fixture(scope="module")
def case_file(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_san_cases")
    made = {}

    def get(name):
        if name not in made:
            made[name] = str(d / (name + ".bin"))
            hc.write_case(name, made[name])
        return made[name]
    return get


@pytest.mark.parametrize("build,battery,name", _params())
def test_driver_is_clean_and_prints_the_production_librarys_lines(drivers, case_file, build, battery, name):
    want = hc.expected(battery, name)
    assert len(want) > 0
    env = dict(os.environ, **SANITIZER_ENV)
    t0 = time.time()
    r = subprocess.run([drivers[build], case_file(name), battery] + hc.tune_pairs(), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, env=env, timeout=TIMEOUT_S[battery])
    print("host_san: %s %s %s ran %.1f s" % (build, battery, name, time.time() - t0))
    assert r.returncode == 0 and r.stderr == "", "exit status %d\n%s" % (r.returncode, r.stderr[-8000:])
    got = r.stdout.splitlines()
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, "call line %d differs from the production library's" % i
    assert len(got) == len(want)
