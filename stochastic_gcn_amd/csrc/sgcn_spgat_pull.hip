// Two-table attention with learned additive scores (GAT) for gfx950 (MI355X): the attention of a part step that keeps its
// out-of-part entries (--full_batch_part_pull_gat; stale rows AND stale scores).  For the n selected rows ids[i] of the RESIDENT
// N x N adjacency, read in place, and per stored entry e of row ids[i] with c = col[e], m = map[c], per head h:
//
//   B_e = m >= 0 ? X[m, :] : H[c, :]             v_e = m >= 0 ? V[m, h] : VH[c, h]
//   forward   z_e = U[i, h] + v_e,  s_e = z_e > 0 ? z_e : slope z_e,  lse_i = log sum_e exp(s_e),  C[i] = sum_e exp(s_e - lse_i) B_e
//   bwd_u     delta_i = <G[i], C[i]>,  e_e = exp(s_e - lse_i) (<G[i], B_e> - delta_i),  dU[i, h] = sum_e e_e (z_e > 0 ? 1 : slope)
//
// X (n x d, fp32), U and V (n x H) hold what the step computes; H (N x d, fp32 or bfloat16 widened exactly) the last-seen rows
// and VH (N x H, fp32) the last-seen destination scores of every vertex, both read for columns outside the step's vertex set S
// only.  The stale score is STORED, not recomputed from H[c] with the current attention vector: the forward then moves nothing
// across lanes, as in spgat_seg_kernel, and a launch is testable bit for bit.  dU sums over ALL stored entries: stored rows and
// scores are constants, but the source score's gradient sees them.  The gradient to values and destination scores flows
// through in-part entries only, which is sgcn_spgat_csr_bwd_v_f32 unchanged over the transposed induced block A[S, S]^T with
// B = X and the lse and delta of these two launches.  No third kernel.
//
// Shape: the per-row arithmetic is that of spgat_seg_kernel / spgat_bwd_u_kernel (sgcn_spgat.hip) without slots -- the same G,
// NV, VW, U, chunks of U entries with pads of weight exactly 0, online softmax, true division acc / l, lse_of, delta and t through
// one reduction tree in one per-lane order -- so a launch gives, bit for bit, what the one-table launch without a plan gives
// on the merged tables (tests/test_spgat_pull_gpu.py).  The entry handling is that of spattn_pull_kernel: the lane that
// fetches an entry's column id also fetches map[col], folds them into one source word (m >= 0 ? m : ~col) and broadcasts it;
// table, pitch and row base -- of the row AND of the score -- are formed behind the broadcast.  At one head the lane that
// fetched the source word fetches the score as well, and it travels with the word.
//   * ONE GROUP OWNS ONE SELECTED ROW, whatever its length: no plan, no split rows, no workspace.
//   * no dropout instantiations: MH = false / true only.
//   * no atomics, nothing nnz-sized written: the same bits on every run.
#include <cmath>
#include "sgcn_attn_pull_dev.h"
#include "sgcn_gat_dev.h"

namespace sgcn {
namespace {

// the stale score table, a third kernel argument (GatX keeps its layout)
struct PullScore {
    const float* VH;         // element [c * ldvh + h], c a vertex
    int64_t ldvh;
};

// the score of head `head` of the entry with source word w: table, pitch and row behind the word, as for the row itself
__device__ __forceinline__ float pull_score(const GatX& x, const PullScore& ps, int head, int w) {
    const bool stale = w < 0;
    const float* base = stale ? ps.VH : x.V;
    const int64_t ld = stale ? ps.ldvh : x.ldv;
    return base[(int64_t)(stale ? ~w : w) * ld + head];
}

// ---- forward ------------------------------------------------------------------------------------------------------------
template <int G, int NV, int VW, bool MH, class HT>
__global__ __launch_bounds__(kBlock) void spgat_pull_kernel(AttnArgs a, PullTab t, GatX x, PullScore ps) {
    typedef typename Vec<VW>::type VT;
    typedef typename PullRaw<VW>::type RT;
    constexpr int U = GatUnroll<NV>::fwd;
    const int lig = threadIdx.x & (G - 1);
    int row, start, end;
    if (!my_row<G>(a, t, row, start, end)) return;
    const Lane<G, NV, VW, MH> L(a, lig);

    VT acc[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) acc[k] = vzero<VW>();
    const float ui = x.U[(int64_t)row * x.ldu + L.head];
    float m = -INFINITY, l = 0.f;
    const char* Xb = reinterpret_cast<const char*>(a.gat);
    const char* Hb = reinterpret_cast<const char*>(t.H);
    const int64_t ldx_bytes = a.ldgat * (int64_t)sizeof(float);
    const int64_t ldh_bytes = t.ldh * (int64_t)sizeof(HT);

    for (int p0 = start; p0 < end; p0 += G) {
        const int n = min(G, end - p0);
        const int mysrc = my_source(a, t, p0, lig, n);
        [[maybe_unused]] float myv = 0.f;      // one head: the lane that fetched the word fetches v as well; it travels with the word
        if constexpr (!MH) {
            if (lig < n) myv = pull_score(x, ps, 0, mysrc);
        }
        for (int j = 0; j < n; j += U) {
            RT raw[U][NV];
            VT b[U][NV];
            bool stale[U];
            float s[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int w = bcast_i<G>(mysrc, min(j + u, n - 1));
                stale[u] = w < 0;
                const char* src = stale[u] ? Hb + (int64_t)(~w) * ldh_bytes : Xb + (int64_t)w * ldx_bytes;   // G == 64: scalar
                if constexpr (MH) s[u] = pull_score(x, ps, L.head, w); else s[u] = bcast_f<G>(myv, min(j + u, n - 1));
#pragma unroll
                for (int k = 0; k < NV; k++) raw[u][k] = pull_load<VW, HT>(src, L.off[k], stale[u]);
            }
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int k = 0; k < NV; k++) {
                    if constexpr (!std::is_same<HT, float>::value && VW > 1) asm volatile("" : "+v"(raw[u][k]));
                    b[u][k] = pull_value<VW, HT>(raw[u][k], stale[u]);
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
                l += p;                        // (a chunk pad: p = exp(-inf) = 0, so its weight is 0)
#pragma unroll
                for (int k = 0; k < NV; k++) acc[k] = vfma<VW>(p, b[u][k], acc[k]);
            }
        }
    }

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
}

// ---- backward, the source score's half: delta_i and dU[i] over ALL stored entries ------------------------------------------
template <int G, int NV, int VW, bool MH, class HT>
__global__ __launch_bounds__(kBlock) void spgat_pull_bwd_u_kernel(AttnArgs a, PullTab t, GatX x, PullScore ps) {
    typedef typename Vec<VW>::type VT;
    typedef typename PullRaw<VW>::type RT;
    constexpr int U = GatUnroll<NV>::bwd;
    const int lig = threadIdx.x & (G - 1);
    int row, start, end;
    if (!my_row<G>(a, t, row, start, end)) return;
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
    if (L.first) a.delta_out[rh] = delta;
    const float lse = a.lse[rh];
    const float ui = x.U[(int64_t)row * x.ldu + L.head];
    float du = 0.f;
    const char* Xb = reinterpret_cast<const char*>(a.gat);
    const char* Hb = reinterpret_cast<const char*>(t.H);
    const int64_t ldx_bytes = a.ldgat * (int64_t)sizeof(float);
    const int64_t ldh_bytes = t.ldh * (int64_t)sizeof(HT);

    for (int p0 = start; p0 < end; p0 += G) {
        const int n = min(G, end - p0);
        const int mysrc = my_source(a, t, p0, lig, n);
        [[maybe_unused]] float myv = 0.f;
        if constexpr (!MH) {
            if (lig < n) myv = pull_score(x, ps, 0, mysrc);
        }
        for (int j = 0; j < n; j += U) {
            RT raw[U][NV];
            VT b[U][NV];
            bool stale[U];
            float v[U], tt[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int w = bcast_i<G>(mysrc, min(j + u, n - 1));
                stale[u] = w < 0;
                const char* src = stale[u] ? Hb + (int64_t)(~w) * ldh_bytes : Xb + (int64_t)w * ldx_bytes;
                if constexpr (MH) v[u] = pull_score(x, ps, L.head, w); else v[u] = bcast_f<G>(myv, min(j + u, n - 1));
#pragma unroll
                for (int k = 0; k < NV; k++) raw[u][k] = pull_load<VW, HT>(src, L.off[k], stale[u]);
            }
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int k = 0; k < NV; k++) {
                    if constexpr (!std::is_same<HT, float>::value && VW > 1) asm volatile("" : "+v"(raw[u][k]));
                    b[u][k] = pull_value<VW, HT>(raw[u][k], stale[u]);
                }
            if (!MH && a.ragged) {
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int k = 0; k < NV; k++) keep_head<VW>(b[u][k], L.cnt[k]);
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < NV; k++) s = vdot<VW>(g[k], b[u][k], s);
                tt[u] = s;
            }
            if constexpr (MH) head_sum<G, U>(tt, a.gh); else group_sum<G, U>(tt);
#pragma unroll
            for (int u = 0; u < U; u++) {
                const float z = ui + v[u];
                const float p = j + u < n ? expf(leaky(z, x.slope) - lse) : 0.f;
                const float e = p * (tt[u] - delta);
                du += e * leaky_d(z, x.slope);
            }
        }
    }

    if (L.first) x.dU[rh] = du;
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// One launch from its checked arguments: pull_run's path (sgcn_spattn_pull.hip) -- the geometry of attn_run without a plan, the
// kernel off the ladders of sgcn_seg.h; heads == 1 selects the MH = false kernels.
template <bool BWD, class HT>
int gat_pull_run(const char* who, AttnArgs& a, const PullTab& t, const GatX& x, const PullScore& ps, int32_t n, int vw,
                 int32_t heads, hipStream_t st) {
    a.nseg = n;
    int G, NV;
    attn_geometry(a, vw, heads, G, NV);
    const int64_t nblocks = (a.nseg + (kBlock / G) - 1) / (kBlock / G);
    SGCN_REQUIRE(nblocks < (1ll << 31), "%s: grid too large", who);
    const dim3 grid((unsigned)nblocks), block(kBlock);
    auto ladder = [&](auto MH) {
        return with_vw(vw, [&](auto VW) {
            return with_gnv(G, NV, [&](auto g, auto nv) {
                constexpr int kG = decltype(g)::value, kNV = decltype(nv)::value, kVW = decltype(VW)::value;
                constexpr bool kMH = decltype(MH)::value;
                if constexpr (BWD) hipLaunchKernelGGL((spgat_pull_bwd_u_kernel<kG, kNV, kVW, kMH, HT>), grid, block, 0, st, a, t, x, ps);
                else hipLaunchKernelGGL((spgat_pull_kernel<kG, kNV, kVW, kMH, HT>), grid, block, 0, st, a, t, x, ps);
            });
        });
    };
    const bool ok = heads == 1 ? ladder(std::false_type{}) : ladder(std::true_type{});
    SGCN_REQUIRE(ok, "%s: no kernel for G=%d NV=%d", who, G, NV);
    SGCN_HIP_TRY(hipGetLastError());
    return SGCN_OK;
}

}  // namespace

// HT = float: the _f32 exports.  HT = uint16_t: the _h16 ones -- the table's pointer is left out of pick_vw, its pitch is not,
// as in spattn_pull: VW, G and NV are what the f32 call picks for a 16-byte aligned fp32 table of the same element pitch.
template <class HT>
static int spgat_pull(const int32_t* rowptr, const int32_t* col, const int32_t* ids, int32_t n, int32_t N, const int32_t* map,
                      int32_t d, int32_t heads, const float* X, int64_t ldx, const HT* H, int64_t ldh, const float* U, int64_t ldu,
                      const float* V, int64_t ldv, const float* VH, int64_t ldvh, float slope, float* C, int64_t ldc, float* lse,
                      void* stream) {
    constexpr bool kH16 = !std::is_same<HT, float>::value;
    if (const int rc = pull_open("spgat_pull", n, N, d, heads, 1.0f)) return rc;
    if (const int rc = slope_ok("spgat_pull", slope)) return rc;
    SGCN_REQUIRE(ldx >= d && ldh >= d && ldc >= d, "spgat_pull: leading dimension smaller than d");
    SGCN_REQUIRE(ldu >= heads && ldv >= heads && ldvh >= heads, "spgat_pull: score table pitch smaller than heads");
    SGCN_REQUIRE(n == 0 || (rowptr && col && ids && map && X && H && U && V && VH && C), "spgat_pull: null operand");
    if constexpr (kH16) {
        if (n > 0)
            if (const int rc = h16_table_ok("spgat_pull", H, ldh, d)) return rc;
    }
    const int vw = head_vw(pick_vw(d, {X, kH16 ? nullptr : (const void*)H, C}, {ldx, ldh, ldc}), d, heads);
    if (const int rc = width_ok("spgat_pull", d, vw, heads)) return rc;
    if (n == 0) return SGCN_OK;

    AttnArgs a{};
    a.rowptr = rowptr; a.col = col; a.gat = X; a.ldgat = ldx; a.out = C; a.ldo = ldc; a.lse_out = lse; a.d = d;
    const PullTab t{ids, map, H, ldh};
    GatX x{};
    x.U = U; x.ldu = ldu; x.V = V; x.ldv = ldv; x.slope = slope;
    const PullScore ps{VH, ldvh};
    return gat_pull_run<false, HT>("spgat_pull", a, t, x, ps, n, vw, heads, (hipStream_t)stream);
}

template <class HT>
static int spgat_pull_bwd_u(const int32_t* rowptr, const int32_t* col, const int32_t* ids, int32_t n, int32_t N,
                            const int32_t* map, int32_t d, int32_t heads, const float* X, int64_t ldx, const HT* H, int64_t ldh,
                            const float* U, int64_t ldu, const float* V, int64_t ldv, const float* VH, int64_t ldvh, float slope,
                            const float* G, int64_t ldg, const float* C, int64_t ldc, const float* lse, float* delta, float* dU,
                            void* stream) {
    constexpr bool kH16 = !std::is_same<HT, float>::value;
    if (const int rc = pull_open("spgat_pull_bwd_u", n, N, d, heads, 1.0f)) return rc;
    if (const int rc = slope_ok("spgat_pull_bwd_u", slope)) return rc;
    SGCN_REQUIRE(ldx >= d && ldh >= d && ldg >= d && ldc >= d, "spgat_pull_bwd_u: leading dimension smaller than d");
    SGCN_REQUIRE(ldu >= heads && ldv >= heads && ldvh >= heads, "spgat_pull_bwd_u: score table pitch smaller than heads");
    SGCN_REQUIRE(n == 0 || (rowptr && col && ids && map && X && H && U && V && VH && G && C && lse && delta && dU),
                 "spgat_pull_bwd_u: null operand");
    if constexpr (kH16) {
        if (n > 0)
            if (const int rc = h16_table_ok("spgat_pull_bwd_u", H, ldh, d)) return rc;
    }
    const int vw = head_vw(pick_vw(d, {X, kH16 ? nullptr : (const void*)H, G, C}, {ldx, ldh, ldg, ldc}), d, heads);
    if (const int rc = width_ok("spgat_pull_bwd_u", d, vw, heads)) return rc;
    if (n == 0) return SGCN_OK;

    AttnArgs a{};
    a.rowptr = rowptr; a.col = col; a.gat = X; a.ldgat = ldx; a.G = G; a.ldg = ldg; a.Cf = C; a.ldcf = ldc; a.lse = lse;
    a.delta_out = delta; a.d = d;
    const PullTab t{ids, map, H, ldh};
    GatX x{};
    x.U = U; x.ldu = ldu; x.V = V; x.ldv = ldv; x.slope = slope; x.dU = dU;
    const PullScore ps{VH, ldvh};
    return gat_pull_run<true, HT>("spgat_pull_bwd_u", a, t, x, ps, n, vw, heads, (hipStream_t)stream);
}

}  // namespace sgcn

using namespace sgcn;

extern "C" int sgcn_spgat_pull_f32(const int32_t* rowptr, const int32_t* col, const int32_t* ids, int32_t n, int32_t N,
                                   const int32_t* map, int32_t d, int32_t heads, const float* X, int64_t ldx, const float* H,
                                   int64_t ldh, const float* U, int64_t ldu, const float* V, int64_t ldv, const float* VH,
                                   int64_t ldvh, float slope, float* C, int64_t ldc, float* lse, void* stream) {
    return spgat_pull<float>(rowptr, col, ids, n, N, map, d, heads, X, ldx, H, ldh, U, ldu, V, ldv, VH, ldvh, slope, C, ldc, lse,
                             stream);
}

/* mirrors sgcn_spgat_pull_f32 on a bfloat16 row table */
extern "C" int sgcn_spgat_pull_h16(const int32_t* rowptr, const int32_t* col, const int32_t* ids, int32_t n, int32_t N,
                                   const int32_t* map, int32_t d, int32_t heads, const float* X, int64_t ldx, const uint16_t* H,
                                   int64_t ldh, const float* U, int64_t ldu, const float* V, int64_t ldv, const float* VH,
                                   int64_t ldvh, float slope, float* C, int64_t ldc, float* lse, void* stream) {
    return spgat_pull<uint16_t>(rowptr, col, ids, n, N, map, d, heads, X, ldx, H, ldh, U, ldu, V, ldv, VH, ldvh, slope, C, ldc, lse,
                                stream);
}

extern "C" int sgcn_spgat_pull_bwd_u_f32(const int32_t* rowptr, const int32_t* col, const int32_t* ids, int32_t n, int32_t N,
                                         const int32_t* map, int32_t d, int32_t heads, const float* X, int64_t ldx, const float* H,
                                         int64_t ldh, const float* U, int64_t ldu, const float* V, int64_t ldv, const float* VH,
                                         int64_t ldvh, float slope, const float* G, int64_t ldg, const float* C, int64_t ldc,
                                         const float* lse, float* delta, float* dU, void* stream) {
    return spgat_pull_bwd_u<float>(rowptr, col, ids, n, N, map, d, heads, X, ldx, H, ldh, U, ldu, V, ldv, VH, ldvh, slope, G, ldg,
                                   C, ldc, lse, delta, dU, stream);
}

/* mirrors sgcn_spgat_pull_bwd_u_f32 on a bfloat16 row table */
extern "C" int sgcn_spgat_pull_bwd_u_h16(const int32_t* rowptr, const int32_t* col, const int32_t* ids, int32_t n, int32_t N,
                                         const int32_t* map, int32_t d, int32_t heads, const float* X, int64_t ldx,
                                         const uint16_t* H, int64_t ldh, const float* U, int64_t ldu, const float* V, int64_t ldv,
                                         const float* VH, int64_t ldvh, float slope, const float* G, int64_t ldg, const float* C,
                                         int64_t ldc, const float* lse, float* delta, float* dU, void* stream) {
    return spgat_pull_bwd_u<uint16_t>(rowptr, col, ids, n, N, map, d, heads, X, ldx, H, ldh, U, ldu, V, ldv, VH, ldvh, slope, G,
                                      ldg, C, ldc, lse, delta, dU, stream);
}
