"""CPU test of csrc/sgcn_seg.h, the host path every row-segment launch shares: a stand-alone program (tests/seg_geometry/main.cpp,
built with g++: the header holds no HIP) prints the lane geometry for nvec in 1..1100, nv_force in 0..4 and six segment
counts, the rungs with_gnv accepts and the width with_vw picks; compared with the formulas the row SpMM, the neighbour maximum
and attention each spelled out before the header existed, restated here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stochastic_gcn_amd", "csrc")
K_BLOCK = 256
NSEGS = (0, 1, 31, 32, 33, 4097)
RUNGS = {(8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4)}


def group_lanes(nvec):
    return 8 if nvec <= 8 else 16 if nvec <= 16 else 32 if nvec <= 32 else 64


def geometry(nvec, nseg, nv_force):
    """spmm_csr_add's block (nv_force = its spmm_nv knob) and, at nv_force = 0, run<BWD>'s of the maximum"""
    G = group_lanes(nvec)
    NV = 1
    if G == 64:
        per_wave = (nvec + 63) // 64
        nslab0 = (per_wave + 3) // 4
        NV = (per_wave + nslab0 - 1) // nslab0
        if nv_force > 0:
            NV = nv_force
    nslab = (nvec + G * NV - 1) // (G * NV)
    nsegblk = (nseg + (K_BLOCK // G) - 1) // (K_BLOCK // G)
    return G, NV, nslab, nsegblk, nsegblk * nslab


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("seg_geometry") / "seg_geometry")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "seg_geometry", "main.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, "the build failed:\n%s\n%s" % (" ".join(cmd), r.stdout)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    out = {}
    for line in r.stdout.splitlines():
        key, *rest = line.split()
        out.setdefault(key, []).append(tuple(int(x) for x in rest))
    return out


def test_geometry_is_the_formulas_each_family_had(printed):
    rows = printed["geom"]
    assert len(rows) == 1100 * 5 * len(NSEGS)
    seen = set()
    for nvec, nv_force, nseg, *got in rows:
        assert tuple(got) == geometry(nvec, nseg, nv_force), (nvec, nv_force, nseg)
        seen.add((nvec, nv_force, nseg))
    assert seen == {(v, f, s) for v in range(1, 1101) for f in range(5) for s in NSEGS}


def test_geometry_covers_every_row_and_every_vector(printed):
    for nvec, nv_force, nseg, G, NV, nslab, nsegblk, nblocks in printed["geom"]:
        assert G * NV * nslab >= nvec > G * NV * (nslab - 1)                       # the slabs cover the row, none is empty
        assert nsegblk * (K_BLOCK // G) >= nseg > (nsegblk - 1) * (K_BLOCK // G)   # the blocks cover the segments
        assert nblocks == nsegblk * nslab
        if nv_force == 0:
            assert (G, NV) in RUNGS                                                # never off the ladder by itself


def test_up_to_256_vectors_are_one_slab(printed):
    """what lets attention's one-head launches (nvec <= 256, no slabs in their kernels) take the same geometry"""
    n = 0
    for nvec, nv_force, nseg, G, NV, nslab, nsegblk, nblocks in printed["geom"]:
        if nvec <= 256 and nv_force == 0:
            assert nslab == 1 and nblocks == nsegblk
            assert G == group_lanes(nvec) and NV == (nvec + 63) // 64             # attn_geometry's own form, as it was
            n += 1
    assert n == 256 * len(NSEGS)


def test_ladders(printed):
    assert len(printed["gnv"]) == 131 * 7
    for G, NV, ok, calls, g, nv in printed["gnv"]:
        # the dispatch_gnv each family had: below 64 lanes NV is not read, the kernel keeps one vector per lane
        want = (G, 1) if G in (8, 16, 32) else (64, NV) if G == 64 and 1 <= NV <= 4 else None
        if want is None:
            assert (ok, calls, g, nv) == (0, 0, -1, -1), (G, NV)
        else:
            assert (ok, calls, g, nv) == (1, 1) + want and want in RUNGS, (G, NV)
    assert printed["vw"] == [(vw, 4 if vw == 4 else 2 if vw == 2 else 1) for vw in range(9)]
    assert printed["pitch"] == [tuple((d + 3) // 4 * 4 for d in range(1, 10))]
    assert printed["fix"] == [(3, 6, 1 << 31)]
