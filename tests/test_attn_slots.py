"""ops.attn_slot against the library: each of the six pattern exports of the attention launches takes a plan whose workspace
holds exactly nslots * attn_slot(...) floats and refuses one float less.  No device: the calls have zero rows and fake,
never dereferenced addresses, so they return after their checks."""
import ctypes

import pytest

from stochastic_gcn_amd import _ffi, ops

A0 = 4096          # (non-null, 16-byte aligned addresses that are never dereferenced)
GRID = [(d, H) for d in (1, 5, 8, 30, 260) for H in (1, 2, 4, 8) if d % H == 0]
lib = _ffi.lib


def _dot_fwd(d, H, ld, plan):
    return lib.sgcn_spattn_drop_csr_f32(A0, 2 * A0, 0, 8, d, H, 0.8, 1, 3 * A0, ld, 4 * A0, ld, 1.0, 5 * A0, ld, 6 * A0, plan, None)


def _dot_bwd_q(d, H, ld, plan):
    return lib.sgcn_spattn_drop_csr_bwd_q_f32(A0, 2 * A0, 0, 8, d, H, 0.8, 1, 3 * A0, ld, 4 * A0, ld, 1.0, 5 * A0, ld, 6 * A0, ld,
                                              7 * A0, 8 * A0, 9 * A0, ld, None, 0, 0, plan, None)


def _dot_bwd_kv(d, H, ld, plan):     # (over the transposed pattern: its rows are the K columns)
    return lib.sgcn_spattn_drop_csr_bwd_kv_f32(A0, 2 * A0, 0, 8, d, H, 0.8, 1, 3 * A0, ld, 4 * A0, ld, 1.0, 5 * A0, ld, 7 * A0,
                                               8 * A0, 9 * A0, ld, None, 0, 0, plan, None)


def _gat_fwd(d, H, ld, plan):
    return lib.sgcn_spgat_csr_f32(A0, 2 * A0, 0, 8, d, H, 0.8, 1, 3 * A0, 8, 10 * A0, 8, 4 * A0, ld, 0.2, 5 * A0, ld, 6 * A0, plan, None)


def _gat_bwd_u(d, H, ld, plan):
    return lib.sgcn_spgat_csr_bwd_u_f32(A0, 2 * A0, 0, 8, d, H, 0.8, 1, 3 * A0, 8, 10 * A0, 8, 4 * A0, ld, 0.2, 5 * A0, ld, 6 * A0, ld,
                                        7 * A0, 8 * A0, 9 * A0, plan, None)


def _gat_bwd_v(d, H, ld, plan):      # (over the transposed pattern)
    return lib.sgcn_spgat_csr_bwd_v_f32(A0, 2 * A0, 0, 8, d, H, 0.8, 1, 3 * A0, 8, 10 * A0, 8, 4 * A0, ld, 0.2, 5 * A0, ld, 7 * A0,
                                        8 * A0, 9 * A0, ld, 11 * A0, None, 0, 0, plan, None)


EXPORTS = [(_dot_fwd, 'fwd'), (_dot_bwd_q, 'bwd'), (_dot_bwd_kv, 'bwd'), (_gat_fwd, 'fwd'), (_gat_bwd_u, 'gat_bwd_u'),
           (_gat_bwd_v, 'gat_bwd_v')]


@pytest.mark.parametrize("fn,kind", EXPORTS, ids=[f.__name__[1:] for f, _ in EXPORTS])
def test_slot_width_mirror_is_the_librarys(fn, kind):
    err = lib.sgcn_last_error
    for d, H in GRID:
        width = ops.attn_slot(kind, d, H)
        ld = (d + 3) // 4 * 4
        what = "%s d=%d heads=%d" % (fn.__name__, d, H)
        short = _ffi.Plan(A0, 8, 12 * A0, 1, 3, 13 * A0, 3 * width - 1)          # nfix = 1, nslots = 3
        assert fn(d, H, ld, ctypes.byref(short)) == -1 and b"workspace too small" in err(), what
        exact = _ffi.Plan(A0, 8, 12 * A0, 1, 3, 13 * A0, 3 * width)
        rc = fn(d, H, ld, ctypes.byref(exact))
        if d <= ops.ATTN_MAX_VECTORS * ops.attn_vw(d, heads=H):
            assert rc == 0, "%s: %s" % (what, err())
        else:
            # (260 columns in 4 heads of 65: vectors of one float, 260 > 256 of them.  No launch serves that width, so the call
            # cannot return SGCN_OK; that it is refused by the check AFTER the workspace's shows the workspace was accepted.)
            assert (d, H) == (260, 4) and rc == -1 and b"over the limit of 256 columns at vector width 1" in err(), what
