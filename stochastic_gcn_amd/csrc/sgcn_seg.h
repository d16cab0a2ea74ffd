// What every row-segment launch derives on the host, in one place (plain C++: no HIP include, so a host compiler can test it).
// A row-segment launch: a group of G lanes owns one row segment of the host plan (include/sgcn.h), a lane keeps NV vectors
// of VW elements, rows wider than G * NV vectors are cut into feature slabs, and split rows meet in an ordered fix-up.
// The row SpMM (sgcn_spmm.hip), the neighbour maximum (sgcn_spmax.hip), attention (sgcn_attn_dev.h) and the control-variate
// aggregator (sgcn_agg.hip) take from here: the checks on a plan, the slot pitch, the lane geometry with its grid, the
// fix-up's grid, and the ladders that turn run-time (VW) and (G, NV) into template arguments.  A family adds its kernels,
// its argument struct and its own operand checks.
#pragma once
#include <type_traits>
#include "sgcn_host.h"
#include "../../include/sgcn.h"

namespace sgcn {

// lanes per row group for `nvec` vectors
inline int group_lanes(int nvec) {
    if (nvec <= 8) return 8;
    if (nvec <= 16) return 16;
    if (nvec <= 32) return 32;
    return 64;
}

// floats between the workspace slots of a d-wide row: every slot starts on a 16-byte boundary
inline int64_t seg_slot_pitch(int64_t d) { return (d + 3) / 4 * 4; }

// The checks on a plan, in two steps for the caller that has one of its own between them (the maximum's id workspace):
// the segment table and, with split rows, the fix-up's tables; then the room for `nslots` slots of `ldw` floats.
inline int seg_plan_tables(const char* who, const sgcn_plan_t* plan, int32_t nrows) {
    SGCN_REQUIRE(plan->dev_seg && plan->nseg >= nrows, "%s: malformed plan", who);
    if (plan->nfix > 0) SGCN_REQUIRE(plan->dev_fix && plan->dev_ws, "%s: plan with split rows needs dev_fix/dev_ws", who);
    return SGCN_OK;
}
inline int seg_plan_room(const char* who, const sgcn_plan_t* plan, int64_t ldw) {
    if (plan->nfix > 0)
        SGCN_REQUIRE(plan->ws_elems >= plan->nslots * ldw, "%s: workspace too small (%lld < %lld floats)", who,
                     (long long)plan->ws_elems, (long long)(plan->nslots * ldw));
    return SGCN_OK;
}
inline int seg_plan_ok(const char* who, const sgcn_plan_t* plan, int32_t nrows, int64_t ldw) {
    if (const int rc = seg_plan_tables(who, plan, nrows)) return rc;
    return seg_plan_room(who, plan, ldw);
}

// The lane geometry of a launch over `nseg` segments of rows `nvec` vectors wide.  Up to 32 vectors a group of that many
// lanes holds the row, one vector per lane; beyond, a wavefront takes the fewest slabs that NV <= 4 allows and the NV that
// covers them evenly.  nv_force > 0 (the SpMM's spmm_nv knob) replaces NV at 64 lanes.  The grid is nsegblk blocks per slab.
struct SegGeom {
    int G, NV, nslab;
    int64_t nsegblk, nblocks;
};
inline SegGeom seg_geometry(int nvec, int64_t nseg, int nv_force = 0) {
    SegGeom g{};
    g.G = group_lanes(nvec);
    g.NV = 1;
    if (g.G == 64) {
        const int per_wave = (nvec + 63) / 64;            // vectors per lane to cover the row
        const int nslab0 = (per_wave + 3) / 4;            // slabs at the NV <= 4 cap
        g.NV = (per_wave + nslab0 - 1) / nslab0;
        if (nv_force > 0) g.NV = nv_force;
    }
    g.nslab = (nvec + g.G * g.NV - 1) / (g.G * g.NV);
    g.nsegblk = (nseg + (kBlock / g.G) - 1) / (kBlock / g.G);
    g.nblocks = g.nsegblk * g.nslab;
    return g;
}

// blocks of a fix-up launch that gives every split row ceil(nvec / kBlock) blocks of one vector per thread
inline int64_t seg_fix_blocks(int nvec, int64_t nfix) { return (int64_t)((nvec + kBlock - 1) / kBlock) * nfix; }

// The ladders.  f receives std::integral_constants, so `decltype(VW)::value` is a template argument inside it.
template <int N> using int_c = std::integral_constant<int, N>;

// f(VW) at the vector width vw: 4, 2, else 1
template <class F>
auto with_vw(int vw, F&& f) {
    if (vw == 4) return f(int_c<4>{});
    if (vw == 2) return f(int_c<2>{});
    return f(int_c<1>{});
}

// f(G, NV) on the seven rungs (8,1) (16,1) (32,1) (64,1..4); false off the ladder, f not called
template <class F>
bool with_gnv(int G, int NV, F&& f) {
    switch (G) {
        case 8: f(int_c<8>{}, int_c<1>{}); return true;
        case 16: f(int_c<16>{}, int_c<1>{}); return true;
        case 32: f(int_c<32>{}, int_c<1>{}); return true;
        case 64:
            switch (NV) {
                case 1: f(int_c<64>{}, int_c<1>{}); return true;
                case 2: f(int_c<64>{}, int_c<2>{}); return true;
                case 3: f(int_c<64>{}, int_c<3>{}); return true;
                case 4: f(int_c<64>{}, int_c<4>{}); return true;
            }
    }
    return false;
}

}  // namespace sgcn
