// Softmax dot-product attention over a CSR pattern for gfx950 (MI355X), and its backward (--aggregator attn):
//   forward   s_ij = scale * <Q[i], B[j]>,  lse_i = log sum_j exp(s_ij),  p_ij = exp(s_ij - lse_i),  C[i] = sum_j p_ij B[j]
//   backward  delta_i = <G[i], C[i]>,  e_ij = p_ij (<G[i], B[j]> - delta_i)
//             dQ[i] = scale * sum_j e_ij B[j]                          (gather over P, row i)
//             dB[j] = sum_i ( p_ij G[i] + scale e_ij Q[i] )            (gather over P^T, row j, source rows i ascending)
// The sums run over the stored entries of row i; stored values are never read.  Nothing nnz-sized is written in either
// direction: the forward keeps a running (m, l, acc) per row segment (online softmax: acc and l are rescaled when the
// maximum m rises) and uses every gathered row twice, for its score and for the weighted sum; the backward recomputes
// p_ij and e_ij per entry from the per-row scalars lse_i and delta_i.  No atomics: dB is a gather over the transposed
// pattern, split rows meet in an ordered fix-up, so every result is bitwise reproducible.
//
// Shape of the kernels: the lane geometry of sgcn_spmm.hip / sgcn_spmax.hip -- a group of G lanes (8/16/32/64 from the
// row width) owns one row segment of the host plan, lane l owns vectors l, l + G, .. of VW elements, the segment's column
// ids are read G at a time and broadcast, U entries' loads are in flight before the first use.  A score needs the WHOLE
// row, so there are no feature slabs: one group holds all d columns, NV <= 4 vectors per lane, d <= 256 * VW.  The dot
// products reduce across the group's lanes with __shfl_xor (no LDS memory); the backward's two dot products per entry
// travel through the reduction together (group_sum2: log2 G + 2 moves for both instead of 2 log2 G).
//
// A chunk of U entries is always processed whole: past the end of the column block the last entry is loaded again and
// its weight forced to exactly 0 (score -inf), which adds +-0 to the sums -- one code path, no remainder loop.
//
// Multi-head (heads = H in {2, 4, 8}, the MH = true instantiations; H = 1 runs the MH = false ones, which are the single-head
// kernels unchanged): head h is the columns [h dh, (h + 1) dh), dh = d / H, and every formula above holds per head, lse and
// delta being M x H tables.  The group's G lanes are cut into H aligned sub-groups of Gh = G / H lanes (Gh a wave-uniform
// run-time value, not a template parameter: the instantiations double, they do not quadruple); sub-group h owns head h,
// its lane r the head's vectors r, r + Gh, .. (NV <= 4 of them).  VW divides dh, so no vector straddles two heads and
// nothing is ragged.  The gathers are the single-head ones; the dot products reduce over the sub-group only (xor offsets
// below Gh stay inside an aligned sub-group; Gh = 1 moves nothing), and the running (m, l, acc) -- per lane already --
// is simply each head's own: lanes of different heads may take the `maximum rises` branch differently, which is plain
// divergence, since nothing inside it crosses lanes.
//
// Dropout on the coefficients (--attn_dropout, the DR = true instantiations; keep == 1 runs the DR = false ones, which are the
// kernels above unchanged): entry (i, j) of head h is kept iff fmix32(pair(i, j) + h * 0x27D4EB2F) < thr, with
// pair(i, j) = fmix32(fmix32(i * 0x9E3779B1 + key) + j * 0x85EBCA77), i the row of P and j its column in all three launches
// (bwd_kv walks P^T: its own row is j, the gathered id i).  A kept coefficient is scaled by mk = 1 / keep AFTER the softmax:
// m, l and lse never see the mask; the forward adds (p * mk) * B[j], the backward uses mk * t_ij in e_ij and p * mk on
// G[i].  The mask is a pure function of (i, j, h, key), recomputed in each launch (drop_bits: by the lane that fetched the
// entry's id, once for all heads): nothing is stored for it.  DR is
// a template parameter, not a run-time branch, and the mask travels in a second kernel argument that the DR = false
// kernels never read: their device code is, instruction for instruction, the code they had before DR existed.
//
// This file holds the three pattern kernels, the backward's fix-up kernel, the launcher that names them (Dot) and the exports'
// own operand checks.  The arguments, the mask, a lane's share of a row, the reductions, the forward's fix-up kernel and the
// backward's epilogue live in sgcn_attn_dev.h, and so does the host path from checked arguments to a launch -- slot widths,
// opening checks, multi-head geometry, the choice of (DR, MH), fix-up step (attn_run) -- which sgcn_spgat.hip (learned additive
// scores) shares; the plan checks, the one-head geometry and the ladders over (VW, G, NV) under it are sgcn_seg.h's.
#include <cmath>
#include "sgcn_attn_dev.h"

namespace sgcn {
namespace {

template <int NV>
struct Unroll { static constexpr int fwd = 4, bwd_q = NV >= 3 ? 2 : 4, bwd_kv = NV >= 2 ? 2 : 4; };

// ---- forward ------------------------------------------------------------------------------------------------------------
template <int G, int NV, int VW, bool MH, bool DR>
__global__ __launch_bounds__(kBlock) void spattn_seg_kernel(AttnArgs a, AttnDrop dm) {
    typedef typename Vec<VW>::type VT;
    constexpr int U = Unroll<NV>::fwd;
    const int lig = threadIdx.x & (G - 1);
    int row, start, end, slot;
    if (!my_segment<G>(a, row, start, end, slot)) return;
    const Lane<G, NV, VW, MH> L(a, lig);

    VT q[NV], acc[NV];
    L.own_row(a.own, a.ldown, row, q);
#pragma unroll
    for (int k = 0; k < NV; k++) acc[k] = vzero<VW>();
    float m = -INFINITY, l = 0.f;
    const char* Bb = reinterpret_cast<const char*>(a.gat);
    const int64_t ldb_bytes = a.ldgat * (int64_t)sizeof(float);

    for (int p0 = start; p0 < end; p0 += G) {
        const int n = min(G, end - p0);
        int mycol = 0;
        if (lig < n) mycol = a.col[p0 + lig];
        [[maybe_unused]] int mybits = 0;
        if constexpr (DR) mybits = drop_bits<MH>(dm, row, mycol, a.heads);
        for (int j = 0; j < n; j += U) {
            VT b[U][NV];
            float s[U];
            [[maybe_unused]] float mk[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int c = bcast_i<G>(mycol, min(j + u, n - 1));
                const char* src = Bb + (int64_t)c * ldb_bytes;   // G == 64: scalar base
                if constexpr (DR) mk[u] = drop_mk(dm, bcast_i<G>(mybits, min(j + u, n - 1)), L.head);
#pragma unroll
                for (int k = 0; k < NV; k++) b[u][k] = vload<VW>(reinterpret_cast<const float*>(src + L.off[k]));
            }
            if (!MH && a.ragged) {
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int k = 0; k < NV; k++) keep_head<VW>(b[u][k], L.cnt[k]);
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                s[u] = 0.f;
#pragma unroll
                for (int k = 0; k < NV; k++) s[u] = vdot<VW>(q[k], b[u][k], s[u]);
            }
            if constexpr (MH) head_sum<G, U>(s, a.gh); else group_sum<G, U>(s);
            float mn = m;
#pragma unroll
            for (int u = 0; u < U; u++) {
                s[u] = j + u < n ? s[u] * a.scale : -INFINITY;
                mn = fmaxf(mn, s[u]);
            }
            if (mn > m) {                      // the maximum rises: what was summed so far shrinks by exp(m - mn)
                const float alpha = expf(m - mn);
                l *= alpha;
#pragma unroll
                for (int k = 0; k < NV; k++) acc[k] *= alpha;
                m = mn;
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const float p = expf(s[u] - m);
                l += p;
                float w = p;                   // (a chunk pad: p = exp(-inf) = 0, so its weight is 0 whatever its mask)
                if constexpr (DR) w = p * mk[u];
#pragma unroll
                for (int k = 0; k < NV; k++) acc[k] = vfma<VW>(w, b[u][k], acc[k]);
            }
        }
    }

    if (slot < 0) {
        const bool empty = start >= end;
#pragma unroll
        for (int k = 0; k < NV; k++)
            if (L.cnt[k]) {
                VT r = vzero<VW>();
                if (!empty) r = acc[k] / l;
                vstore_n<VW>(a.out + (int64_t)row * a.ldo + (int64_t)L.vi[k] * VW, r, L.cnt[k]);
            }
        if constexpr (MH) {
            if (a.lse_out && L.first) a.lse_out[(int64_t)row * a.heads + L.head] = empty ? -INFINITY : lse_of(m, l);
        } else {
            if (a.lse_out && lig == 0) a.lse_out[row] = empty ? -INFINITY : lse_of(m, l);
        }
    } else {
        float* w = a.ws + (int64_t)slot * a.ldw;
#pragma unroll
        for (int k = 0; k < NV; k++)
            if (L.cnt[k]) vstore<VW>(w + (int64_t)L.vi[k] * VW, acc[k]);
        if constexpr (MH) {                    // head h's (m, l): the vector h after the accumulator
            if (L.first) { float* ml = w + (a.ldw - 4 * a.heads) + 4 * L.head; ml[0] = m; ml[1] = l; }
        } else {
            if (lig == 0) { w[a.ldw - 4] = m; w[a.ldw - 3] = l; }
        }
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------
// over P: delta_i and dQ[i] = scale * sum_j e_ij B[j]
template <int G, int NV, int VW, bool MH, bool DR>
__global__ __launch_bounds__(kBlock) void spattn_bwd_q_kernel(AttnArgs a, AttnDrop dm) {
    typedef typename Vec<VW>::type VT;
    constexpr int U = Unroll<NV>::bwd_q;
    const int lig = threadIdx.x & (G - 1);
    int row, start, end, slot;
    if (!my_segment<G>(a, row, start, end, slot)) return;
    const Lane<G, NV, VW, MH> L(a, lig);

    VT q[NV], g[NV], acc[NV];
    L.own_row(a.own, a.ldown, row, q);
    L.own_row(a.G, a.ldg, row, g);
    float delta;
    {
        VT c[NV];
        L.own_row(a.Cf, a.ldcf, row, c);
        // through the tree and the per-lane order of the loop's t = <G[i], B[j]>: where C[i] holds the bits of one B[j] (a
        // softmax that has saturated on one neighbour), t - delta is exactly 0 for it, whatever the sums round to
        float dd[1] = {0.f}, none[1] = {0.f};
#pragma unroll
        for (int k = 0; k < NV; k++) dd[0] = vdot<VW>(g[k], c[k], dd[0]);
        if constexpr (MH) head_sum2<G, 1>(none, dd, lig, a.gh); else group_sum2<G, 1>(none, dd, lig);
        delta = dd[0];
    }
    float lse;
    if constexpr (MH) {                        // per head: element [row, head] of the M x H tables
        const int64_t rh = (int64_t)row * a.heads + L.head;
        if (L.first && start == a.rowptr[row]) a.delta_out[rh] = delta;
        lse = a.lse[rh];
    } else {
        if (lig == 0 && start == a.rowptr[row]) a.delta_out[row] = delta;   // the row's first segment
        lse = a.lse[row];
    }
#pragma unroll
    for (int k = 0; k < NV; k++) acc[k] = vzero<VW>();
    const char* Bb = reinterpret_cast<const char*>(a.gat);
    const int64_t ldb_bytes = a.ldgat * (int64_t)sizeof(float);

    for (int p0 = start; p0 < end; p0 += G) {
        const int n = min(G, end - p0);
        int mycol = 0;
        if (lig < n) mycol = a.col[p0 + lig];
        [[maybe_unused]] int mybits = 0;
        if constexpr (DR) mybits = drop_bits<MH>(dm, row, mycol, a.heads);
        for (int j = 0; j < n; j += U) {
            VT b[U][NV];
            float s[U], t[U];
            [[maybe_unused]] float mk[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int c = bcast_i<G>(mycol, min(j + u, n - 1));
                const char* src = Bb + (int64_t)c * ldb_bytes;
                if constexpr (DR) mk[u] = drop_mk(dm, bcast_i<G>(mybits, min(j + u, n - 1)), L.head);
#pragma unroll
                for (int k = 0; k < NV; k++) b[u][k] = vload<VW>(reinterpret_cast<const float*>(src + L.off[k]));
            }
            if (!MH && a.ragged) {
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int k = 0; k < NV; k++) keep_head<VW>(b[u][k], L.cnt[k]);
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                s[u] = 0.f; t[u] = 0.f;
#pragma unroll
                for (int k = 0; k < NV; k++) {
                    s[u] = vdot<VW>(q[k], b[u][k], s[u]);
                    t[u] = vdot<VW>(g[k], b[u][k], t[u]);
                }
            }
            if constexpr (MH) head_sum2<G, U>(s, t, lig, a.gh); else group_sum2<G, U>(s, t, lig);
#pragma unroll
            for (int u = 0; u < U; u++) {
                const float p = j + u < n ? expf(s[u] * a.scale - lse) : 0.f;
                float tm = t[u];
                if constexpr (DR) tm = mk[u] * t[u];
                const float e = p * (tm - delta);
#pragma unroll
                for (int k = 0; k < NV; k++) acc[k] = vfma<VW>(e, b[u][k], acc[k]);
            }
        }
    }

    if (slot < 0) {
#pragma unroll
        for (int k = 0; k < NV; k++)
            if (L.cnt[k]) bwd_store<VW>(a, row, L.vi[k], acc[k], a.scale);
    } else {
        float* w = a.ws + (int64_t)slot * a.ldw;
#pragma unroll
        for (int k = 0; k < NV; k++)
            if (L.cnt[k]) vstore<VW>(w + (int64_t)L.vi[k] * VW, acc[k]);
    }
}

// over P^T: dB[j] = sum_i ( p_ij G[i] + scale e_ij Q[i] ), two gathered rows per entry
template <int G, int NV, int VW, bool MH, bool DR>
__global__ __launch_bounds__(kBlock) void spattn_bwd_kv_kernel(AttnArgs a, AttnDrop dm) {
    typedef typename Vec<VW>::type VT;
    constexpr int U = Unroll<NV>::bwd_kv;
    const int lig = threadIdx.x & (G - 1);
    int row, start, end, slot;
    if (!my_segment<G>(a, row, start, end, slot)) return;
    const Lane<G, NV, VW, MH> L(a, lig);

    VT b[NV], acc[NV];
    L.own_row(a.own, a.ldown, row, b);
#pragma unroll
    for (int k = 0; k < NV; k++) acc[k] = vzero<VW>();
    const char* Qb = reinterpret_cast<const char*>(a.gat);
    const char* Gb = reinterpret_cast<const char*>(a.G);
    const int64_t ldq_bytes = a.ldgat * (int64_t)sizeof(float), ldg_bytes = a.ldg * (int64_t)sizeof(float);

    for (int p0 = start; p0 < end; p0 += G) {
        const int n = min(G, end - p0);
        int myrow = 0;
        if (lig < n) myrow = a.col[p0 + lig];
        [[maybe_unused]] int mybits = 0;
        if constexpr (DR) mybits = drop_bits<MH>(dm, myrow, row, a.heads);     // pair(i, j): the own row is the COLUMN j
        for (int j = 0; j < n; j += U) {
            VT qi[U][NV], gi[U][NV];
            float s[U], t[U], lse[U], delta[U];
            [[maybe_unused]] float mk[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int i = bcast_i<G>(myrow, min(j + u, n - 1));
                if constexpr (DR) mk[u] = drop_mk(dm, bcast_i<G>(mybits, min(j + u, n - 1)), L.head);
                const char* qs = Qb + (int64_t)i * ldq_bytes;        // G == 64: scalar bases
                const char* gs = Gb + (int64_t)i * ldg_bytes;
                if constexpr (MH) {
                    lse[u] = a.lse[(int64_t)i * a.heads + L.head];
                    delta[u] = a.delta[(int64_t)i * a.heads + L.head];
                } else {
                    lse[u] = a.lse[i];
                    delta[u] = a.delta[i];
                }
#pragma unroll
                for (int k = 0; k < NV; k++) {
                    qi[u][k] = vload<VW>(reinterpret_cast<const float*>(qs + L.off[k]));
                    gi[u][k] = vload<VW>(reinterpret_cast<const float*>(gs + L.off[k]));
                }
            }
            if (!MH && a.ragged) {
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int k = 0; k < NV; k++) {
                        keep_head<VW>(qi[u][k], L.cnt[k]);
                        keep_head<VW>(gi[u][k], L.cnt[k]);
                    }
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                s[u] = 0.f; t[u] = 0.f;
#pragma unroll
                for (int k = 0; k < NV; k++) {
                    s[u] = vdot<VW>(qi[u][k], b[k], s[u]);
                    t[u] = vdot<VW>(gi[u][k], b[k], t[u]);
                }
            }
            if constexpr (MH) head_sum2<G, U>(s, t, lig, a.gh); else group_sum2<G, U>(s, t, lig);
#pragma unroll
            for (int u = 0; u < U; u++) {
                const float p = j + u < n ? expf(s[u] * a.scale - lse[u]) : 0.f;
                float tm = t[u], pg = p;
                if constexpr (DR) { tm = mk[u] * t[u]; pg = p * mk[u]; }
                const float es = a.scale * (p * (tm - delta[u]));
#pragma unroll
                for (int k = 0; k < NV; k++) {
                    acc[k] = vfma<VW>(pg, gi[u][k], acc[k]);
                    acc[k] = vfma<VW>(es, qi[u][k], acc[k]);
                }
            }
        }
    }

    if (slot < 0) {
#pragma unroll
        for (int k = 0; k < NV; k++)
            if (L.cnt[k]) bwd_store<VW>(a, row, L.vi[k], acc[k], 1.f);
    } else {
        float* w = a.ws + (int64_t)slot * a.ldw;
#pragma unroll
        for (int k = 0; k < NV; k++)
            if (L.cnt[k]) vstore<VW>(w + (int64_t)L.vi[k] * VW, acc[k]);
    }
}

// Ordered sum of the workspace slots of every split row, then the direct rows' epilogue (the scheme of spmm_fix_kernel).
template <int VW>
__global__ __launch_bounds__(kBlock) void spattn_bwd_fix_kernel(AttnArgs a, const sgcn_fix_t* fix, int64_t nfix, float mul) {
    typedef typename Vec<VW>::type VT;
    const int64_t f = blockIdx.x;
    if (f >= nfix) return;
    const sgcn_fix_t fx = fix[f];
    const int vi = threadIdx.x;
    if (vi >= a.nvec) return;
    const float* w = a.ws + (int64_t)fx.first_slot * a.ldw + (int64_t)vi * VW;
    VT acc = vzero<VW>();
    for (int q = 0; q < fx.nslots; q++) acc += vload<VW>(w + (int64_t)q * a.ldw);
    bwd_store<VW>(a, fx.row, vi, acc, mul);
}

// the launcher attn_run (sgcn_attn_dev.h) takes: the kernel and the fix-up of one kind of launch
enum Kind { FWD, BWD_Q, BWD_KV };

template <int KIND>
struct Dot {
    static constexpr int64_t max_fix = 1ll << 31;
    template <int G, int NV, int VW, bool MH, bool DR>
    static void launch(dim3 grid, hipStream_t st, const AttnArgs& a, const AttnDrop& dm) {
        const dim3 block(kBlock);
        if constexpr (KIND == FWD) hipLaunchKernelGGL((spattn_seg_kernel<G, NV, VW, MH, DR>), grid, block, 0, st, a, dm);
        else if constexpr (KIND == BWD_Q) hipLaunchKernelGGL((spattn_bwd_q_kernel<G, NV, VW, MH, DR>), grid, block, 0, st, a, dm);
        else hipLaunchKernelGGL((spattn_bwd_kv_kernel<G, NV, VW, MH, DR>), grid, block, 0, st, a, dm);
    }
    static void fix(int vw, const AttnArgs& a, const sgcn_plan_t* plan, hipStream_t st) {
        if constexpr (KIND == FWD) launch_fwd_fix(vw, a, plan, st);
        else {
            const dim3 grid((unsigned)plan->nfix), block(kBlock);      // one workgroup per split row: nvec <= 256 = kBlock threads
            const float mul = KIND == BWD_Q ? a.scale : 1.f;
            with_vw(vw, [&](auto VW) {
                hipLaunchKernelGGL((spattn_bwd_fix_kernel<decltype(VW)::value>), grid, block, 0, st, a, plan->dev_fix, plan->nfix, mul);
            });
        }
    }
};

}  // namespace
}  // namespace sgcn

using namespace sgcn;


// The three host bodies: the single-head exports call them with heads = 1, the _mh_ exports pass theirs on, both with
// keep = 1 (no dropout: the DR = false kernels); the _drop_ exports pass keep and key on as well.
static int spattn_fwd(const int32_t* rowptr, const int32_t* col, int32_t M, int32_t K, int32_t d, int32_t heads,
                      float keep, uint32_t key, const float* Q, int64_t ldq, const float* B, int64_t ldb, float scale,
                      float* C, int64_t ldc, float* lse, const sgcn_plan_t* plan, void* stream) {
    if (const int rc = attn_open("spattn", M, K, d, heads, keep)) return rc;
    SGCN_REQUIRE(rowptr && C && (Q || M == 0) && (B || K == 0), "spattn: null operand");
    SGCN_REQUIRE(ldq >= d && ldb >= d && ldc >= d, "spattn: leading dimension smaller than d");
    SGCN_REQUIRE(std::isfinite(scale), "spattn: scale must be finite");
    const int64_t ldw = fwd_slot(d, heads);
    int vw;
    if (const int rc = attn_plan_width("spattn", plan, M, ldw, d, heads, {Q, B, C, split_ws(plan)}, {ldq, ldb, ldc}, vw)) return rc;
    if (M == 0) return SGCN_OK;

    AttnArgs a{};
    a.rowptr = rowptr; a.col = col; a.own = Q; a.ldown = ldq; a.gat = B; a.ldgat = ldb; a.out = C; a.ldo = ldc;
    a.lse_out = lse; a.scale = scale; a.d = d;
    return attn_run<Dot<FWD>>("spattn", a, M, plan, ldw, vw, heads, drop_of(keep, key), (hipStream_t)stream);
}

static int spattn_bwd_q(const int32_t* rowptr, const int32_t* col, int32_t M, int32_t K, int32_t d, int32_t heads,
                        float keep, uint32_t key, const float* Q, int64_t ldq, const float* B, int64_t ldb, float scale,
                        const float* G, int64_t ldg, const float* C, int64_t ldc, const float* lse,
                        float* delta, float* dQ, int64_t lddq, const float* add, int64_t ldadd,
                        int32_t add_rows, const sgcn_plan_t* plan, void* stream) {
    if (const int rc = attn_open("spattn_bwd_q", M, K, d, heads, keep)) return rc;
    SGCN_REQUIRE(rowptr && dQ && ((Q && G && C && lse && delta) || M == 0) && (B || K == 0), "spattn_bwd_q: null operand");
    SGCN_REQUIRE(ldq >= d && ldb >= d && ldg >= d && ldc >= d && lddq >= d, "spattn_bwd_q: leading dimension smaller than d");
    SGCN_REQUIRE(std::isfinite(scale), "spattn_bwd_q: scale must be finite");
    const bool with_add = add && add_rows > 0;
    if (with_add) SGCN_REQUIRE(ldadd >= d && add_rows <= M, "spattn_bwd_q: bad addend");
    int vw;
    if (const int rc = attn_plan_width("spattn_bwd_q", plan, M, bwd_slot(d), d, heads,
                                       {Q, B, G, C, dQ, with_add ? add : nullptr, split_ws(plan)},
                                       {ldq, ldb, ldg, ldc, lddq, with_add ? ldadd : lddq}, vw)) return rc;
    if (M == 0) return SGCN_OK;

    AttnArgs a{};
    a.rowptr = rowptr; a.col = col; a.own = Q; a.ldown = ldq; a.gat = B; a.ldgat = ldb; a.G = G; a.ldg = ldg;
    a.Cf = C; a.ldcf = ldc; a.lse = lse; a.delta_out = delta; a.out = dQ; a.ldo = lddq; a.scale = scale; a.d = d;
    if (with_add) { a.add = add; a.ldadd = ldadd; a.add_rows = add_rows; }
    return attn_run<Dot<BWD_Q>>("spattn_bwd_q", a, M, plan, bwd_slot(d), vw, heads, drop_of(keep, key), (hipStream_t)stream);
}

static int spattn_bwd_kv(const int32_t* t_rowptr, const int32_t* t_row, int32_t K, int32_t M, int32_t d, int32_t heads,
                         float keep, uint32_t key, const float* Q, int64_t ldq, const float* B, int64_t ldb, float scale,
                         const float* G, int64_t ldg, const float* lse, const float* delta,
                         float* dB, int64_t lddb, const float* add, int64_t ldadd, int32_t add_rows,
                         const sgcn_plan_t* t_plan, void* stream) {
    if (const int rc = attn_open("spattn_bwd_kv", M, K, d, heads, keep)) return rc;
    SGCN_REQUIRE(t_rowptr && dB && ((Q && G && lse && delta) || M == 0) && (B || K == 0), "spattn_bwd_kv: null operand");
    SGCN_REQUIRE(ldq >= d && ldb >= d && ldg >= d && lddb >= d, "spattn_bwd_kv: leading dimension smaller than d");
    SGCN_REQUIRE(std::isfinite(scale), "spattn_bwd_kv: scale must be finite");
    const bool with_add = add && add_rows > 0;
    if (with_add) SGCN_REQUIRE(ldadd >= d && add_rows <= K, "spattn_bwd_kv: bad addend");
    int vw;
    if (const int rc = attn_plan_width("spattn_bwd_kv", t_plan, K, bwd_slot(d), d, heads,
                                       {Q, B, G, dB, with_add ? add : nullptr, split_ws(t_plan)},
                                       {ldq, ldb, ldg, lddb, with_add ? ldadd : lddb}, vw)) return rc;
    if (K == 0) return SGCN_OK;

    AttnArgs a{};
    a.rowptr = t_rowptr; a.col = t_row; a.own = B; a.ldown = ldb; a.gat = Q; a.ldgat = ldq; a.G = G; a.ldg = ldg;
    a.lse = lse; a.delta = delta; a.out = dB; a.ldo = lddb; a.scale = scale; a.d = d;
    if (with_add) { a.add = add; a.ldadd = ldadd; a.add_rows = add_rows; }
    return attn_run<Dot<BWD_KV>>("spattn_bwd_kv", a, K, t_plan, bwd_slot(d), vw, heads, drop_of(keep, key), (hipStream_t)stream);
}

extern "C" int sgcn_spattn_csr_f32(const int32_t* rowptr, const int32_t* col, int32_t M, int32_t K, int32_t d,
                                   const float* Q, int64_t ldq, const float* B, int64_t ldb, float scale,
                                   float* C, int64_t ldc, float* lse, const sgcn_plan_t* plan, void* stream) {
    return spattn_fwd(rowptr, col, M, K, d, 1, 1.0f, 0u, Q, ldq, B, ldb, scale, C, ldc, lse, plan, stream);
}

extern "C" int sgcn_spattn_mh_csr_f32(const int32_t* rowptr, const int32_t* col, int32_t M, int32_t K, int32_t d, int32_t heads,
                                      const float* Q, int64_t ldq, const float* B, int64_t ldb, float scale,
                                      float* C, int64_t ldc, float* lse, const sgcn_plan_t* plan, void* stream) {
    return spattn_fwd(rowptr, col, M, K, d, heads, 1.0f, 0u, Q, ldq, B, ldb, scale, C, ldc, lse, plan, stream);
}

extern "C" int sgcn_spattn_csr_bwd_q_f32(const int32_t* rowptr, const int32_t* col, int32_t M, int32_t K, int32_t d,
                                         const float* Q, int64_t ldq, const float* B, int64_t ldb, float scale,
                                         const float* G, int64_t ldg, const float* C, int64_t ldc, const float* lse,
                                         float* delta, float* dQ, int64_t lddq, const float* add, int64_t ldadd,
                                         int32_t add_rows, const sgcn_plan_t* plan, void* stream) {
    return spattn_bwd_q(rowptr, col, M, K, d, 1, 1.0f, 0u, Q, ldq, B, ldb, scale, G, ldg, C, ldc, lse, delta, dQ, lddq, add, ldadd,
                        add_rows, plan, stream);
}

extern "C" int sgcn_spattn_mh_csr_bwd_q_f32(const int32_t* rowptr, const int32_t* col, int32_t M, int32_t K, int32_t d,
                                            int32_t heads, const float* Q, int64_t ldq, const float* B, int64_t ldb,
                                            float scale, const float* G, int64_t ldg, const float* C, int64_t ldc,
                                            const float* lse, float* delta, float* dQ, int64_t lddq, const float* add,
                                            int64_t ldadd, int32_t add_rows, const sgcn_plan_t* plan, void* stream) {
    return spattn_bwd_q(rowptr, col, M, K, d, heads, 1.0f, 0u, Q, ldq, B, ldb, scale, G, ldg, C, ldc, lse, delta, dQ, lddq, add, ldadd,
                        add_rows, plan, stream);
}

extern "C" int sgcn_spattn_csr_bwd_kv_f32(const int32_t* t_rowptr, const int32_t* t_row, int32_t K, int32_t M, int32_t d,
                                          const float* Q, int64_t ldq, const float* B, int64_t ldb, float scale,
                                          const float* G, int64_t ldg, const float* lse, const float* delta,
                                          float* dB, int64_t lddb, const float* add, int64_t ldadd, int32_t add_rows,
                                          const sgcn_plan_t* t_plan, void* stream) {
    return spattn_bwd_kv(t_rowptr, t_row, K, M, d, 1, 1.0f, 0u, Q, ldq, B, ldb, scale, G, ldg, lse, delta, dB, lddb, add, ldadd,
                         add_rows, t_plan, stream);
}

extern "C" int sgcn_spattn_mh_csr_bwd_kv_f32(const int32_t* t_rowptr, const int32_t* t_row, int32_t K, int32_t M, int32_t d,
                                             int32_t heads, const float* Q, int64_t ldq, const float* B, int64_t ldb,
                                             float scale, const float* G, int64_t ldg, const float* lse, const float* delta,
                                             float* dB, int64_t lddb, const float* add, int64_t ldadd, int32_t add_rows,
                                             const sgcn_plan_t* t_plan, void* stream) {
    return spattn_bwd_kv(t_rowptr, t_row, K, M, d, heads, 1.0f, 0u, Q, ldq, B, ldb, scale, G, ldg, lse, delta, dB, lddb, add, ldadd,
                         add_rows, t_plan, stream);
}

// The coefficient-dropout forms (--attn_dropout): heads, keep and key directly after d; keep == 1 is the call without them.
extern "C" int sgcn_spattn_drop_csr_f32(const int32_t* rowptr, const int32_t* col, int32_t M, int32_t K, int32_t d, int32_t heads,
                                        float keep, uint32_t key, const float* Q, int64_t ldq, const float* B, int64_t ldb,
                                        float scale, float* C, int64_t ldc, float* lse, const sgcn_plan_t* plan, void* stream) {
    return spattn_fwd(rowptr, col, M, K, d, heads, keep, key, Q, ldq, B, ldb, scale, C, ldc, lse, plan, stream);
}

extern "C" int sgcn_spattn_drop_csr_bwd_q_f32(const int32_t* rowptr, const int32_t* col, int32_t M, int32_t K, int32_t d,
                                              int32_t heads, float keep, uint32_t key, const float* Q, int64_t ldq,
                                              const float* B, int64_t ldb, float scale, const float* G, int64_t ldg,
                                              const float* C, int64_t ldc, const float* lse, float* delta, float* dQ,
                                              int64_t lddq, const float* add, int64_t ldadd, int32_t add_rows,
                                              const sgcn_plan_t* plan, void* stream) {
    return spattn_bwd_q(rowptr, col, M, K, d, heads, keep, key, Q, ldq, B, ldb, scale, G, ldg, C, ldc, lse, delta, dQ, lddq, add,
                        ldadd, add_rows, plan, stream);
}

extern "C" int sgcn_spattn_drop_csr_bwd_kv_f32(const int32_t* t_rowptr, const int32_t* t_row, int32_t K, int32_t M, int32_t d,
                                               int32_t heads, float keep, uint32_t key, const float* Q, int64_t ldq,
                                               const float* B, int64_t ldb, float scale, const float* G, int64_t ldg,
                                               const float* lse, const float* delta, float* dB, int64_t lddb, const float* add,
                                               int64_t ldadd, int32_t add_rows, const sgcn_plan_t* t_plan, void* stream) {
    return spattn_bwd_kv(t_rowptr, t_row, K, M, d, heads, keep, key, Q, ldq, B, ldb, scale, G, ldg, lse, delta, dB, lddb, add,
                         ldadd, add_rows, t_plan, stream);
}
