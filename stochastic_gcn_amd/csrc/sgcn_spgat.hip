// Learned additive attention scores (GAT) over a CSR pattern for gfx950 (MI355X), and their backward (--attn_score gat):
//   scores    u_i^h = sum_{c in h} x[i,c] a[0,c],  v_j^h = sum_{c in h} x[j,c] a[1,c]             (gat_scores_kernel)
//   forward   z_ij = u_i + v_j,  s_ij = z_ij > 0 ? z_ij : slope z_ij,  lse_i = log sum_j exp(s_ij),  p_ij = exp(s_ij - lse_i),
//             C[i] = sum_j mk_ij p_ij B[j]                                                         (spgat_seg_kernel)
//   backward  delta_i = <G[i], C[i]>,  e_ij = p_ij (mk_ij <G[i], B[j]> - delta_i),  dz_ij = e_ij (z_ij > 0 ? 1 : slope)
//             dU[i] = sum_j dz_ij                              (gather over P, row i: spgat_bwd_u_kernel)
//             dB[j] = sum_i mk_ij p_ij G[i],  dV[j] = sum_i dz_ij    (gather over P^T, row j, i ascending: spgat_bwd_v_kernel)
//             dX[r,c] += dU[r,h(c)] a[0,c] + dV[r,h(c)] a[1,c],  da[0,c] = sum_r dU[r,h(c)] x[r,c],  da[1,c] likewise with dV
//                                                                                                  (gat_scores_bwd_kernel + reduce)
// The three pattern kernels are those of sgcn_spattn.hip with the score changed: the lane geometry (Lane), the segment plans
// (my_segment), the online softmax with its slots and its ordered fix-up (spattn_fix_kernel, shared through sgcn_attn_dev.h), the
// chunk pads of weight exactly 0, the coefficient mask (drop_bits).  What differs: a score is ONE fp32 addition of two table
// scalars, so the forward moves nothing across lanes; the backward's only dot product is t_ij = <G[i], B[j]>, so the
// transposed launch gathers one row per entry (G[i]; B[j] is its own row) beside the scalars u_i, lse_i, delta_i; and each
// backward launch carries one more per-lane scalar sum (dU, dV), which a split row keeps in its slot beside the row.
// delta and t go through the SAME reduction tree in the same per-lane order, so where C[i] holds the bits of one B[j] (a
// saturated softmax) t - delta is exactly 0 for it.  Nothing nnz-sized is written and there are no atomics.
// The host side is sgcn_attn_dev.h's as well: slot widths, opening checks, lane geometry and fix-up step (attn_run), over the
// plan checks and the ladders of sgcn_seg.h; this file adds the launcher that names its kernels (Gat) and each export's own operand checks
// (GatX, the LeakyReLU and slope_ok: sgcn_gat_dev.h, shared with sgcn_spgat_pull.hip).
#include <cmath>
#include "sgcn_gat_dev.h"

namespace sgcn {
namespace {

// ---- forward ------------------------------------------------------------------------------------------------------------
template <int G, int NV, int VW, bool MH, bool DR>
__global__ __launch_bounds__(kBlock) void spgat_seg_kernel(AttnArgs a, GatX x, AttnDrop dm) {
    typedef typename Vec<VW>::type VT;
    constexpr int U = GatUnroll<NV>::fwd;
    const int lig = threadIdx.x & (G - 1);
    int row, start, end, slot;
    if (!my_segment<G>(a, row, start, end, slot)) return;
    const Lane<G, NV, VW, MH> L(a, lig);

    VT acc[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) acc[k] = vzero<VW>();
    const float ui = x.U[(int64_t)row * x.ldu + L.head];
    const float* Vh = x.V + L.head;
    float m = -INFINITY, l = 0.f;
    const char* Bb = reinterpret_cast<const char*>(a.gat);
    const int64_t ldb_bytes = a.ldgat * (int64_t)sizeof(float);

    for (int p0 = start; p0 < end; p0 += G) {
        const int n = min(G, end - p0);
        int mycol = 0;
        if (lig < n) mycol = a.col[p0 + lig];
        [[maybe_unused]] int mybits = 0;
        if constexpr (DR) mybits = drop_bits<MH>(dm, row, mycol, a.heads);
        [[maybe_unused]] float myv = 0.f;      // one head: the lane that fetched the id fetches v as well; it travels with the id
        if constexpr (!MH) myv = Vh[(int64_t)mycol * x.ldv];
        for (int j = 0; j < n; j += U) {
            VT b[U][NV];
            float s[U];
            [[maybe_unused]] float mk[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int c = bcast_i<G>(mycol, min(j + u, n - 1));
                const char* src = Bb + (int64_t)c * ldb_bytes;
                if constexpr (DR) mk[u] = drop_mk(dm, bcast_i<G>(mybits, min(j + u, n - 1)), L.head);
                if constexpr (MH) s[u] = Vh[(int64_t)c * x.ldv]; else s[u] = bcast_f<G>(myv, min(j + u, n - 1));
#pragma unroll
                for (int k = 0; k < NV; k++) b[u][k] = vload<VW>(reinterpret_cast<const float*>(src + L.off[k]));
            }
            float mn = m;
#pragma unroll
            for (int u = 0; u < U; u++) {
                s[u] = j + u < n ? leaky(ui + s[u], x.slope) : -INFINITY;
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

    // the epilogue and the slot of spattn_seg_kernel (spattn_fix_kernel reads the slots)
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
            if (L.cnt[k]) vstore_n<VW>(w + (int64_t)L.vi[k] * VW, acc[k], L.cnt[k]);
        if constexpr (MH) {
            if (L.first) { float* ml = w + (a.ldw - 4 * a.heads) + 4 * L.head; ml[0] = m; ml[1] = l; }
        } else {
            if (lig == 0) { w[a.ldw - 4] = m; w[a.ldw - 3] = l; }
        }
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------
// over P: delta_i and dU[i] = sum_j dz_ij; one gathered row per entry
template <int G, int NV, int VW, bool MH, bool DR>
__global__ __launch_bounds__(kBlock) void spgat_bwd_u_kernel(AttnArgs a, GatX x, AttnDrop dm) {
    typedef typename Vec<VW>::type VT;
    constexpr int U = GatUnroll<NV>::bwd;
    const int lig = threadIdx.x & (G - 1);
    int row, start, end, slot;
    if (!my_segment<G>(a, row, start, end, slot)) return;
    const Lane<G, NV, VW, MH> L(a, lig);

    VT g[NV];
    L.own_row(a.G, a.ldg, row, g);
    float delta;
    {
        VT c[NV];
        L.own_row(a.Cf, a.ldcf, row, c);
        float dd = 0.f;
#pragma unroll
        for (int k = 0; k < NV; k++) dd = vdot<VW>(g[k], c[k], dd);
        delta = head_total<G, MH>(dd, a.gh);   // the tree and the per-lane order of the loop's t
    }
    const int64_t rh = (int64_t)row * a.heads + L.head;
    if (L.first && start == a.rowptr[row]) a.delta_out[rh] = delta;   // the row's first segment
    const float lse = a.lse[rh];
    const float ui = x.U[(int64_t)row * x.ldu + L.head];
    const float* Vh = x.V + L.head;
    float du = 0.f;
    const char* Bb = reinterpret_cast<const char*>(a.gat);
    const int64_t ldb_bytes = a.ldgat * (int64_t)sizeof(float);

    for (int p0 = start; p0 < end; p0 += G) {
        const int n = min(G, end - p0);
        int mycol = 0;
        if (lig < n) mycol = a.col[p0 + lig];
        [[maybe_unused]] int mybits = 0;
        if constexpr (DR) mybits = drop_bits<MH>(dm, row, mycol, a.heads);
        [[maybe_unused]] float myv = 0.f;
        if constexpr (!MH) myv = Vh[(int64_t)mycol * x.ldv];
        for (int j = 0; j < n; j += U) {
            VT b[U][NV];
            float v[U], t[U];
            [[maybe_unused]] float mk[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int c = bcast_i<G>(mycol, min(j + u, n - 1));
                const char* src = Bb + (int64_t)c * ldb_bytes;
                if constexpr (DR) mk[u] = drop_mk(dm, bcast_i<G>(mybits, min(j + u, n - 1)), L.head);
                if constexpr (MH) v[u] = Vh[(int64_t)c * x.ldv]; else v[u] = bcast_f<G>(myv, min(j + u, n - 1));
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
                float tt = 0.f;
#pragma unroll
                for (int k = 0; k < NV; k++) tt = vdot<VW>(g[k], b[u][k], tt);
                t[u] = tt;
            }
            if constexpr (MH) head_sum<G, U>(t, a.gh); else group_sum<G, U>(t);
#pragma unroll
            for (int u = 0; u < U; u++) {
                const float z = ui + v[u];
                const float p = j + u < n ? expf(leaky(z, x.slope) - lse) : 0.f;
                float tm = t[u];
                if constexpr (DR) tm = mk[u] * t[u];
                const float e = p * (tm - delta);
                du += e * leaky_d(z, x.slope);
            }
        }
    }

    if (L.first) {
        if (slot < 0) x.dU[rh] = du;
        else a.ws[(int64_t)slot * a.ldw + L.head] = du;
    }
}

// a split row's dU: the slots' sums added in slot order, one thread per (split row, head)
__global__ __launch_bounds__(kBlock) void spgat_bwd_u_fix_kernel(AttnArgs a, GatX x, const sgcn_fix_t* fix, int64_t nfix) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nfix * a.heads) return;
    const sgcn_fix_t fx = fix[t / a.heads];
    const int h = (int)(t % a.heads);
    const float* w = a.ws + (int64_t)fx.first_slot * a.ldw + h;
    float s = 0.f;
    for (int q = 0; q < fx.nslots; q++) s += w[(int64_t)q * a.ldw];
    x.dU[(int64_t)fx.row * a.heads + h] = s;
}

// over P^T: dB[j] = sum_i mk_ij p_ij G[i] and dV[j] = sum_i dz_ij; the gathered row is G[i], B[j] the group's own
template <int G, int NV, int VW, bool MH, bool DR>
__global__ __launch_bounds__(kBlock) void spgat_bwd_v_kernel(AttnArgs a, GatX x, AttnDrop dm) {
    typedef typename Vec<VW>::type VT;
    constexpr int U = GatUnroll<NV>::bwd;
    const int lig = threadIdx.x & (G - 1);
    int row, start, end, slot;
    if (!my_segment<G>(a, row, start, end, slot)) return;
    const Lane<G, NV, VW, MH> L(a, lig);

    VT b[NV], acc[NV];
    L.own_row(a.own, a.ldown, row, b);
#pragma unroll
    for (int k = 0; k < NV; k++) acc[k] = vzero<VW>();
    const float vj = x.V[(int64_t)row * x.ldv + L.head];
    const float* Uh = x.U + L.head;
    float dv = 0.f;
    const char* Gb = reinterpret_cast<const char*>(a.G);
    const int64_t ldg_bytes = a.ldg * (int64_t)sizeof(float);

    for (int p0 = start; p0 < end; p0 += G) {
        const int n = min(G, end - p0);
        int myrow = 0;
        if (lig < n) myrow = a.col[p0 + lig];
        [[maybe_unused]] int mybits = 0;
        if constexpr (DR) mybits = drop_bits<MH>(dm, myrow, row, a.heads);     // pair(i, j): the own row is the COLUMN j
        for (int j = 0; j < n; j += U) {
            VT gi[U][NV];
            float t[U], ui[U], lse[U], delta[U];
            [[maybe_unused]] float mk[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int i = bcast_i<G>(myrow, min(j + u, n - 1));
                if constexpr (DR) mk[u] = drop_mk(dm, bcast_i<G>(mybits, min(j + u, n - 1)), L.head);
                const char* gs = Gb + (int64_t)i * ldg_bytes;
                ui[u] = Uh[(int64_t)i * x.ldu];
                lse[u] = a.lse[(int64_t)i * a.heads + L.head];
                delta[u] = a.delta[(int64_t)i * a.heads + L.head];
#pragma unroll
                for (int k = 0; k < NV; k++) gi[u][k] = vload<VW>(reinterpret_cast<const float*>(gs + L.off[k]));
            }
            if (!MH && a.ragged) {
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int k = 0; k < NV; k++) keep_head<VW>(gi[u][k], L.cnt[k]);
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                float tt = 0.f;
#pragma unroll
                for (int k = 0; k < NV; k++) tt = vdot<VW>(gi[u][k], b[k], tt);
                t[u] = tt;
            }
            if constexpr (MH) head_sum<G, U>(t, a.gh); else group_sum<G, U>(t);
#pragma unroll
            for (int u = 0; u < U; u++) {
                const float z = ui[u] + vj;
                const float p = j + u < n ? expf(leaky(z, x.slope) - lse[u]) : 0.f;
                float tm = t[u], pg = p;
                if constexpr (DR) { tm = mk[u] * t[u]; pg = p * mk[u]; }
                const float e = p * (tm - delta[u]);
                dv += e * leaky_d(z, x.slope);
#pragma unroll
                for (int k = 0; k < NV; k++) acc[k] = vfma<VW>(pg, gi[u][k], acc[k]);
            }
        }
    }

    if (slot < 0) {
#pragma unroll
        for (int k = 0; k < NV; k++)
            if (L.cnt[k]) bwd_store<VW>(a, row, L.vi[k], acc[k], 1.f);
        if (L.first) x.dV[(int64_t)row * a.heads + L.head] = dv;
    } else {
        float* w = a.ws + (int64_t)slot * a.ldw;
#pragma unroll
        for (int k = 0; k < NV; k++)
            if (L.cnt[k]) vstore_n<VW>(w + (int64_t)L.vi[k] * VW, acc[k], L.cnt[k]);
        if (L.first) w[a.ldw - kScalarSlot + L.head] = dv;
    }
}

// Ordered sum of the workspace slots of every split row, then the epilogue; thread h < H adds the slots' dV as well
// (nvec >= H: a vector never straddles two heads)
template <int VW>
__global__ __launch_bounds__(kBlock) void spgat_bwd_v_fix_kernel(AttnArgs a, GatX x, const sgcn_fix_t* fix, int64_t nfix) {
    typedef typename Vec<VW>::type VT;
    const int64_t f = blockIdx.x;
    if (f >= nfix) return;
    const sgcn_fix_t fx = fix[f];
    const int vi = threadIdx.x;
    if (vi >= a.nvec) return;
    const float* w0 = a.ws + (int64_t)fx.first_slot * a.ldw;
    const float* w = w0 + (int64_t)vi * VW;
    const int left = min(VW, a.d - vi * VW);
    VT acc = vzero<VW>();
    for (int q = 0; q < fx.nslots; q++) {
        VT s = vload<VW>(w + (int64_t)q * a.ldw);
        keep_head<VW>(s, left);
        acc += s;
    }
    bwd_store<VW>(a, fx.row, vi, acc, 1.f);
    if (vi < a.heads) {
        float s = 0.f;
        for (int q = 0; q < fx.nslots; q++) s += w0[(int64_t)q * a.ldw + a.ldw - kScalarSlot + vi];
        x.dV[(int64_t)fx.row * a.heads + vi] = s;
    }
}

// ---- the scores and their backward --------------------------------------------------------------------------------------
// One wavefront per row, one pass over x.  SUMMATION ORDER of u_r^h (v likewise): lane l of 64 adds the head's columns
// h dh + l, h dh + l + 64, .. in ascending order by fused multiply-add, starting from +0; the 64 lane sums then meet in a
// butterfly, s += s[lane ^ o] for o = 32, 16, 8, 4, 2, 1.
constexpr int kScoreRows = kBlock / kWave;

__global__ __launch_bounds__(kBlock) void gat_scores_kernel(const float* __restrict__ x, int64_t ldx, int32_t rows, int32_t d,
                                                            int32_t heads, const float* __restrict__ a, float* __restrict__ S) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = (int64_t)blockIdx.x * kScoreRows + threadIdx.x / kWave;
    if (r >= rows) return;
    const int dh = d / heads;
    const float* xr = x + r * ldx;
    for (int h = 0; h < heads; h++) {
        float su = 0.f, sv = 0.f;
        for (int c = h * dh + lane; c < (h + 1) * dh; c += kWave) {
            const float xv = xr[c];
            su = __builtin_fmaf(xv, a[c], su);
            sv = __builtin_fmaf(xv, a[d + c], sv);
        }
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            su += __shfl_xor(su, o, kWave);
            sv += __shfl_xor(sv, o, kWave);
        }
        if (lane == 0) {
            S[r * 2 * heads + h] = su;
            S[r * 2 * heads + heads + h] = sv;
        }
    }
}

// Stage 1: workgroup b owns the rows [64 b, 64 b + 64) -- a partition that depends on `rows` alone -- and thread t the columns
// t, t + 256, ..: per column it walks its rows in ascending order, adds the rank-2H term into dX (when there is one) and sums
// dU x and dV x by fused multiply-add from +0 into ws[b][0 / 1][c].  Stage 2: one thread per element of da adds the
// partials in block order.
constexpr int kGatRedRows = 64;

__global__ __launch_bounds__(kBlock) void gat_scores_bwd_kernel(const float* __restrict__ x, int64_t ldx, int32_t rows, int32_t rows_u,
                                                                int32_t d, int32_t heads, const float* __restrict__ a,
                                                                const float* __restrict__ dU, const float* __restrict__ dV,
                                                                float* __restrict__ dX, int64_t lddx, float* __restrict__ ws) {
    const int64_t b = blockIdx.x;
    const int64_t r0 = b * kGatRedRows;
    const int64_t r1 = min((int64_t)rows, r0 + kGatRedRows);
    const int dh = d / heads;
    for (int c = threadIdx.x; c < d; c += kBlock) {
        const int h = c / dh;
        const float a0 = a[c], a1 = a[d + c];
        float s0 = 0.f, s1 = 0.f;
        for (int64_t r = r0; r < r1; r++) {
            const float xv = x[r * ldx + c];
            const float dv = dV[r * heads + h];
            const bool hasu = r < rows_u;
            const float du = hasu ? dU[r * heads + h] : 0.f;
            if (hasu) s0 = __builtin_fmaf(du, xv, s0);
            s1 = __builtin_fmaf(dv, xv, s1);
            if (dX) {
                float t = dX[r * lddx + c];
                if (hasu) t = __builtin_fmaf(du, a0, t);
                t = __builtin_fmaf(dv, a1, t);
                dX[r * lddx + c] = t;
            }
        }
        ws[(b * 2 + 0) * d + c] = s0;
        ws[(b * 2 + 1) * d + c] = s1;
    }
}

__global__ __launch_bounds__(kBlock) void gat_da_reduce_kernel(const float* __restrict__ ws, int64_t nblk, int32_t d, float* __restrict__ da) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= 2 * d) return;
    const float* p = ws + (int64_t)(i / d) * d + (i % d);
    float s = 0.f;
#pragma unroll 8
    for (int64_t b = 0; b < nblk; b++) s += p[b * 2 * d];
    da[i] = s;
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// the launcher attn_run (sgcn_attn_dev.h) takes: the kernel and the fix-up of one kind of launch
enum GatKind { GAT_FWD, GAT_BWD_U, GAT_BWD_V };

template <int KIND>
struct Gat {
    static constexpr int64_t max_fix = (1ll << 31) / 8;      // (bwd_u's fix-up counts nfix * heads threads)
    template <int G, int NV, int VW, bool MH, bool DR>
    static void launch(dim3 grid, hipStream_t st, const AttnArgs& a, const GatX& x, const AttnDrop& dm) {
        const dim3 block(kBlock);
        if constexpr (KIND == GAT_FWD) hipLaunchKernelGGL((spgat_seg_kernel<G, NV, VW, MH, DR>), grid, block, 0, st, a, x, dm);
        else if constexpr (KIND == GAT_BWD_U) hipLaunchKernelGGL((spgat_bwd_u_kernel<G, NV, VW, MH, DR>), grid, block, 0, st, a, x, dm);
        else hipLaunchKernelGGL((spgat_bwd_v_kernel<G, NV, VW, MH, DR>), grid, block, 0, st, a, x, dm);
    }
    static void fix(int vw, const AttnArgs& a, const sgcn_plan_t* plan, hipStream_t st, const GatX& x) {
        if constexpr (KIND == GAT_FWD) launch_fwd_fix(vw, a, plan, st);
        else if constexpr (KIND == GAT_BWD_U) {
            const dim3 g1((unsigned)((plan->nfix * a.heads + kBlock - 1) / kBlock));
            hipLaunchKernelGGL(spgat_bwd_u_fix_kernel, g1, dim3(kBlock), 0, st, a, x, plan->dev_fix, plan->nfix);
        } else {
            const dim3 grid((unsigned)plan->nfix), block(kBlock);      // one workgroup per split row: nvec <= 256 = kBlock threads
            with_vw(vw, [&](auto VW) {
                hipLaunchKernelGGL((spgat_bwd_v_fix_kernel<decltype(VW)::value>), grid, block, 0, st, a, x, plan->dev_fix, plan->nfix);
            });
        }
    }
};

}  // namespace
}  // namespace sgcn

using namespace sgcn;

extern "C" int sgcn_gat_scores_f32(const float* x, int64_t ldx, int32_t rows, int32_t d, int32_t heads, const float* a,
                                   float* S, void* stream) {
    SGCN_REQUIRE(rows >= 0, "gat_scores: negative size");
    SGCN_REQUIRE(d > 0, "gat_scores: d must be positive (got %d)", d);
    { const int rc = heads_ok("gat_scores", d, heads); if (rc) return rc; }
    SGCN_REQUIRE(a && ((x && S) || rows == 0), "gat_scores: null operand");
    SGCN_REQUIRE(ldx >= d, "gat_scores: leading dimension smaller than d");
    if (rows == 0) return SGCN_OK;
    const int64_t nblocks = ((int64_t)rows + kScoreRows - 1) / kScoreRows;
    hipLaunchKernelGGL(gat_scores_kernel, dim3((unsigned)nblocks), dim3(kBlock), 0, (hipStream_t)stream, x, ldx, rows, d, heads, a, S);
    SGCN_HIP_TRY(hipGetLastError());
    return SGCN_OK;
}

extern "C" int sgcn_spgat_csr_f32(const int32_t* rowptr, const int32_t* col, int32_t M, int32_t K, int32_t d, int32_t heads,
                                  float keep, uint32_t key, const float* U, int64_t ldu, const float* V, int64_t ldv,
                                  const float* B, int64_t ldb, float slope, float* C, int64_t ldc, float* lse,
                                  const sgcn_plan_t* plan, void* stream) {
    if (const int rc = attn_open("spgat", M, K, d, heads, keep)) return rc;
    if (const int rc = slope_ok("spgat", slope)) return rc;
    SGCN_REQUIRE(rowptr && C && (U || M == 0) && ((B && V) || K == 0), "spgat: null operand");
    SGCN_REQUIRE(ldb >= d && ldc >= d, "spgat: leading dimension smaller than d");
    SGCN_REQUIRE(ldu >= heads && ldv >= heads, "spgat: score table pitch smaller than heads");
    const int64_t ldw = fwd_slot(d, heads);                  // the forward slot of sgcn_spattn_mh_csr_f32
    int vw;
    if (const int rc = attn_plan_width("spgat", plan, M, ldw, d, heads, {B, C, split_ws(plan)}, {ldb, ldc}, vw)) return rc;
    if (M == 0) return SGCN_OK;

    AttnArgs a{};
    a.rowptr = rowptr; a.col = col; a.gat = B; a.ldgat = ldb; a.out = C; a.ldo = ldc; a.lse_out = lse; a.d = d;
    GatX x{};
    x.U = U; x.ldu = ldu; x.V = V; x.ldv = ldv; x.slope = slope;
    return attn_run<Gat<GAT_FWD>>("spgat", a, M, plan, ldw, vw, heads, drop_of(keep, key), (hipStream_t)stream, x);
}

extern "C" int sgcn_spgat_csr_bwd_u_f32(const int32_t* rowptr, const int32_t* col, int32_t M, int32_t K, int32_t d,
                                        int32_t heads, float keep, uint32_t key, const float* U, int64_t ldu, const float* V,
                                        int64_t ldv, const float* B, int64_t ldb, float slope, const float* G, int64_t ldg,
                                        const float* C, int64_t ldc, const float* lse, float* delta, float* dU,
                                        const sgcn_plan_t* plan, void* stream) {
    if (const int rc = attn_open("spgat_bwd_u", M, K, d, heads, keep)) return rc;
    if (const int rc = slope_ok("spgat_bwd_u", slope)) return rc;
    SGCN_REQUIRE(rowptr && ((U && G && C && lse && delta && dU) || M == 0) && ((B && V) || K == 0), "spgat_bwd_u: null operand");
    SGCN_REQUIRE(ldb >= d && ldg >= d && ldc >= d, "spgat_bwd_u: leading dimension smaller than d");
    SGCN_REQUIRE(ldu >= heads && ldv >= heads, "spgat_bwd_u: score table pitch smaller than heads");
    int vw;      // (the slots hold scalars only: the workspace is no operand of the vector width)
    if (const int rc = attn_plan_width("spgat_bwd_u", plan, M, kGatBwdUSlot, d, heads, {B, G, C}, {ldb, ldg, ldc}, vw)) return rc;
    if (M == 0) return SGCN_OK;

    AttnArgs a{};
    a.rowptr = rowptr; a.col = col; a.gat = B; a.ldgat = ldb; a.G = G; a.ldg = ldg; a.Cf = C; a.ldcf = ldc; a.lse = lse;
    a.delta_out = delta; a.d = d;
    GatX x{};
    x.U = U; x.ldu = ldu; x.V = V; x.ldv = ldv; x.slope = slope; x.dU = dU;
    return attn_run<Gat<GAT_BWD_U>>("spgat_bwd_u", a, M, plan, kGatBwdUSlot, vw, heads, drop_of(keep, key), (hipStream_t)stream, x);
}

extern "C" int sgcn_spgat_csr_bwd_v_f32(const int32_t* t_rowptr, const int32_t* t_row, int32_t K, int32_t M, int32_t d,
                                        int32_t heads, float keep, uint32_t key, const float* U, int64_t ldu, const float* V,
                                        int64_t ldv, const float* B, int64_t ldb, float slope, const float* G, int64_t ldg,
                                        const float* lse, const float* delta, float* dB, int64_t lddb, float* dV,
                                        const float* add, int64_t ldadd, int32_t add_rows, const sgcn_plan_t* t_plan,
                                        void* stream) {
    if (const int rc = attn_open("spgat_bwd_v", M, K, d, heads, keep)) return rc;
    if (const int rc = slope_ok("spgat_bwd_v", slope)) return rc;
    SGCN_REQUIRE(t_rowptr && ((U && G && lse && delta) || M == 0) && ((B && V && dB && dV) || K == 0), "spgat_bwd_v: null operand");
    SGCN_REQUIRE(ldb >= d && ldg >= d && lddb >= d, "spgat_bwd_v: leading dimension smaller than d");
    SGCN_REQUIRE(ldu >= heads && ldv >= heads, "spgat_bwd_v: score table pitch smaller than heads");
    const bool with_add = add && add_rows > 0;
    if (with_add) SGCN_REQUIRE(ldadd >= d && add_rows <= K, "spgat_bwd_v: bad addend");
    int vw;
    if (const int rc = attn_plan_width("spgat_bwd_v", t_plan, K, gat_bwd_v_slot(d), d, heads,
                                       {B, G, dB, with_add ? add : nullptr, split_ws(t_plan)},
                                       {ldb, ldg, lddb, with_add ? ldadd : lddb}, vw)) return rc;
    if (K == 0) return SGCN_OK;

    AttnArgs a{};
    a.rowptr = t_rowptr; a.col = t_row; a.own = B; a.ldown = ldb; a.G = G; a.ldg = ldg; a.lse = lse; a.delta = delta;
    a.out = dB; a.ldo = lddb; a.d = d;
    if (with_add) { a.add = add; a.ldadd = ldadd; a.add_rows = add_rows; }
    GatX x{};
    x.U = U; x.ldu = ldu; x.V = V; x.ldv = ldv; x.slope = slope; x.dV = dV;
    return attn_run<Gat<GAT_BWD_V>>("spgat_bwd_v", a, K, t_plan, gat_bwd_v_slot(d), vw, heads, drop_of(keep, key),
                                    (hipStream_t)stream, x);
}

extern "C" int sgcn_gat_scores_bwd_f32(const float* x, int64_t ldx, int32_t rows, int32_t rows_u, int32_t d, int32_t heads,
                                       const float* a, const float* dU, const float* dV, float* dX, int64_t lddx, float* da,
                                       float* ws, int64_t ws_elems, void* stream) {
    SGCN_REQUIRE(rows >= 0 && rows_u >= 0 && rows_u <= rows, "gat_scores_bwd: need 0 <= rows_u <= rows (got %d, %d)", rows_u, rows);
    SGCN_REQUIRE(d > 0, "gat_scores_bwd: d must be positive (got %d)", d);
    { const int rc = heads_ok("gat_scores_bwd", d, heads); if (rc) return rc; }
    SGCN_REQUIRE(a && da && ((x && dV) || rows == 0) && (dU || rows_u == 0), "gat_scores_bwd: null operand");
    SGCN_REQUIRE(ldx >= d && (!dX || lddx >= d), "gat_scores_bwd: leading dimension smaller than d");
    const int64_t nblk = ((int64_t)rows + kGatRedRows - 1) / kGatRedRows;
    SGCN_REQUIRE(nblk == 0 || (ws && ws_elems >= nblk * 2 * d), "gat_scores_bwd: workspace too small (%lld < %lld floats)",
                 (long long)ws_elems, (long long)(nblk * 2 * d));
    SGCN_REQUIRE(nblk < (1ll << 31), "gat_scores_bwd: grid too large");
    hipStream_t st = (hipStream_t)stream;
    if (nblk > 0) {
        hipLaunchKernelGGL(gat_scores_bwd_kernel, dim3((unsigned)nblk), dim3(kBlock), 0, st, x, ldx, rows, rows_u, d, heads, a, dU, dV,
                           dX, lddx, ws);
        SGCN_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(gat_da_reduce_kernel, dim3((unsigned)((2 * (int64_t)d + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, ws, nblk, d, da);
    SGCN_HIP_TRY(hipGetLastError());
    return SGCN_OK;
}
