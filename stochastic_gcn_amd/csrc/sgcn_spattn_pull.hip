// Two-table softmax dot-product attention for gfx950 (MI355X): the attention of a part step that keeps its out-of-part entries
// (--full_batch_part_pull with --aggregator attn; GNNAutoScale's stale rows under attention).  For the n selected rows
// ids[i] of the RESIDENT N x N adjacency, read in place, and per stored entry e of row ids[i] with c = col[e]:
//
//   B_e = map[c] >= 0 ? X[map[c], :] : H[c, :]
//   forward   s_e = scale * <X[i], B_e>,  lse_i = log sum_e exp(s_e),  C[i] = sum_e exp(s_e - lse_i) B_e
//   bwd_q     delta_i = <G[i], C[i]>,  e_e = exp(s_e - lse_i) (<G[i], B_e> - delta_i),  dQ[i] = scale * sum_e e_e B_e (+ add[i])
//
// per head as in sgcn_spattn.hip.  X (n x d, fp32) holds the rows the step computes: the queries, and the keys / values of the
// columns inside the step's vertex set S; H (N x d, fp32 or bfloat16 widened exactly) the last-seen rows of every vertex, read
// for columns outside S only.  Rows of H inside S are never read, and a row of X is read only as its own query or where map
// says its column is in S.  With stale rows the softmax's normaliser runs over EVERY stored neighbour -- without them every
// coefficient of a cut row is wrong, not just the missing terms.  bwd_q sums over all stored entries too: stored rows are
// constants, but the query's gradient sees them.  The gradient to keys / values flows through in-part entries only, which is
// sgcn_spattn_mh_csr_bwd_kv_f32 unchanged over the transposed induced block A[S, S]^T with Q = B = X, the lse and delta of
// these two launches and add = dQ: the p it recomputes uses the full row's lse, as the estimator requires.  No third kernel.
//
// Shape: the per-row arithmetic is that of spattn_seg_kernel / spattn_bwd_q_kernel (sgcn_spattn.hip) -- the same G, NV, VW, U,
// chunks of U entries processed whole with pads of weight exactly 0, online softmax, true division acc / l, lse = m + log l in
// fp64, the same reductions (sgcn_attn_dev.h) -- so a launch gives, bit for bit, what the one-table launch without a plan
// gives on the merged table (tests/test_spattn_pull_gpu.py).  The entry handling is that of spmm_pull_kernel
// (sgcn_spmm_pull.hip, sgcn_pull_dev.h): the lane that fetches an entry's column id also fetches map[col], folds them into one
// source word (m >= 0 ? m : ~col) and broadcasts it; table, pitch and row base are formed behind the broadcast.
//   * ONE GROUP OWNS ONE SELECTED ROW, whatever its length: no plan, no split rows, no workspace -- the restriction of
//     sgcn_spmm_pull_*.  A launch runs as long as its longest selected row; split rows are the named follow-up.
//   * no dropout instantiations in this version (the mask of out-of-part entries is not defined): MH = false / true only.
//   * no atomics, nothing nnz-sized written: the same bits on every run.
//
// HT: the history's element, float or uint16_t (a bfloat16 table of ops.history_alloc(..., bf16=True)'s layout).  The loads of
// a chunk stay in one raw register image, pinned between the requests and the first use as in spmm_pull_kernel; past the
// widening both instantiations run the same instructions on the same floats.
#include <cmath>
#include "sgcn_attn_pull_dev.h"

namespace sgcn {
namespace {

template <int NV>
struct PullUnroll { static constexpr int fwd = 4, bwd_q = NV >= 3 ? 2 : 4; };    // sgcn_spattn.hip's Unroll

// ---- forward ------------------------------------------------------------------------------------------------------------
template <int G, int NV, int VW, bool MH, class HT>
__global__ __launch_bounds__(kBlock) void spattn_pull_kernel(AttnArgs a, PullTab t) {
    typedef typename Vec<VW>::type VT;
    typedef typename PullRaw<VW>::type RT;
    constexpr int U = PullUnroll<NV>::fwd;
    const int lig = threadIdx.x & (G - 1);
    int row, start, end;
    if (!my_row<G>(a, t, row, start, end)) return;
    const Lane<G, NV, VW, MH> L(a, lig);

    VT q[NV], acc[NV];
    L.own_row(a.own, a.ldown, row, q);
#pragma unroll
    for (int k = 0; k < NV; k++) acc[k] = vzero<VW>();
    float m = -INFINITY, l = 0.f;
    const char* Xb = reinterpret_cast<const char*>(a.gat);
    const char* Hb = reinterpret_cast<const char*>(t.H);
    const int64_t ldx_bytes = a.ldgat * (int64_t)sizeof(float);
    const int64_t ldh_bytes = t.ldh * (int64_t)sizeof(HT);

    for (int p0 = start; p0 < end; p0 += G) {
        const int n = min(G, end - p0);
        const int mysrc = my_source(a, t, p0, lig, n);
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

// ---- backward, the query's half: delta_i and dQ[i] over ALL stored entries ---------------------------------------------------
template <int G, int NV, int VW, bool MH, class HT>
__global__ __launch_bounds__(kBlock) void spattn_pull_bwd_q_kernel(AttnArgs a, PullTab t) {
    typedef typename Vec<VW>::type VT;
    typedef typename PullRaw<VW>::type RT;
    constexpr int U = PullUnroll<NV>::bwd_q;
    const int lig = threadIdx.x & (G - 1);
    int row, start, end;
    if (!my_row<G>(a, t, row, start, end)) return;
    const Lane<G, NV, VW, MH> L(a, lig);

    VT q[NV], g[NV], acc[NV];
    L.own_row(a.own, a.ldown, row, q);
    L.own_row(a.G, a.ldg, row, g);
    float delta;
    {
        VT c[NV];
        L.own_row(a.Cf, a.ldcf, row, c);
        // through the tree and the per-lane order of the loop's t = <G[i], B_e> (spattn_bwd_q_kernel's reason)
        float dd[1] = {0.f}, none[1] = {0.f};
#pragma unroll
        for (int k = 0; k < NV; k++) dd[0] = vdot<VW>(g[k], c[k], dd[0]);
        if constexpr (MH) head_sum2<G, 1>(none, dd, lig, a.gh); else group_sum2<G, 1>(none, dd, lig);
        delta = dd[0];
    }
    float lse;
    if constexpr (MH) {                        // per head: element [i, head] of the n x H tables
        const int64_t rh = (int64_t)row * a.heads + L.head;
        if (L.first) a.delta_out[rh] = delta;
        lse = a.lse[rh];
    } else {
        if (lig == 0) a.delta_out[row] = delta;
        lse = a.lse[row];
    }
#pragma unroll
    for (int k = 0; k < NV; k++) acc[k] = vzero<VW>();
    const char* Xb = reinterpret_cast<const char*>(a.gat);
    const char* Hb = reinterpret_cast<const char*>(t.H);
    const int64_t ldx_bytes = a.ldgat * (int64_t)sizeof(float);
    const int64_t ldh_bytes = t.ldh * (int64_t)sizeof(HT);

    for (int p0 = start; p0 < end; p0 += G) {
        const int n = min(G, end - p0);
        const int mysrc = my_source(a, t, p0, lig, n);
        for (int j = 0; j < n; j += U) {
            RT raw[U][NV];
            VT b[U][NV];
            bool stale[U];
            float s[U], tt[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int w = bcast_i<G>(mysrc, min(j + u, n - 1));
                stale[u] = w < 0;
                const char* src = stale[u] ? Hb + (int64_t)(~w) * ldh_bytes : Xb + (int64_t)w * ldx_bytes;
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
                s[u] = 0.f; tt[u] = 0.f;
#pragma unroll
                for (int k = 0; k < NV; k++) {
                    s[u] = vdot<VW>(q[k], b[u][k], s[u]);
                    tt[u] = vdot<VW>(g[k], b[u][k], tt[u]);
                }
            }
            if constexpr (MH) head_sum2<G, U>(s, tt, lig, a.gh); else group_sum2<G, U>(s, tt, lig);
#pragma unroll
            for (int u = 0; u < U; u++) {
                const float p = j + u < n ? expf(s[u] * a.scale - lse) : 0.f;
                const float tm = tt[u];
                const float e = p * (tm - delta);
#pragma unroll
                for (int k = 0; k < NV; k++) acc[k] = vfma<VW>(e, b[u][k], acc[k]);
            }
        }
    }

#pragma unroll
    for (int k = 0; k < NV; k++)
        if (L.cnt[k]) bwd_store<VW>(a, row, L.vi[k], acc[k], a.scale);
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// One launch from its checked arguments: the geometry of attn_run without a plan (one segment per selected row), the kernel
// off the ladders of sgcn_seg.h; heads == 1 selects the MH = false kernels.
template <bool BWD, class HT>
int pull_run(const char* who, AttnArgs& a, const PullTab& t, int32_t n, int vw, int32_t heads, hipStream_t st) {
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
                if constexpr (BWD) hipLaunchKernelGGL((spattn_pull_bwd_q_kernel<kG, kNV, kVW, kMH, HT>), grid, block, 0, st, a, t);
                else hipLaunchKernelGGL((spattn_pull_kernel<kG, kNV, kVW, kMH, HT>), grid, block, 0, st, a, t);
            });
        });
    };
    const bool ok = heads == 1 ? ladder(std::false_type{}) : ladder(std::true_type{});
    SGCN_REQUIRE(ok, "%s: no kernel for G=%d NV=%d", who, G, NV);
    SGCN_HIP_TRY(hipGetLastError());
    return SGCN_OK;
}

}  // namespace

// HT = float: the _f32 exports.  HT = uint16_t: the _h16 ones -- the table's pointer is left out of pick_vw (its layout never
// limits the vector width), its pitch is not, as in spmm_pull: VW, G and NV are what the f32 call picks for a 16-byte aligned
// fp32 table of the same element pitch.
template <class HT>
static int spattn_pull(const int32_t* rowptr, const int32_t* col, const int32_t* ids, int32_t n, int32_t N, const int32_t* map,
                       int32_t d, int32_t heads, const float* X, int64_t ldx, const HT* H, int64_t ldh, float scale, float* C,
                       int64_t ldc, float* lse, void* stream) {
    constexpr bool kH16 = !std::is_same<HT, float>::value;
    if (const int rc = pull_open("spattn_pull", n, N, d, heads, scale)) return rc;
    SGCN_REQUIRE(ldx >= d && ldh >= d && ldc >= d, "spattn_pull: leading dimension smaller than d");
    SGCN_REQUIRE(n == 0 || (rowptr && col && ids && map && X && H && C), "spattn_pull: null operand");
    if constexpr (kH16) {
        if (n > 0)
            if (const int rc = h16_table_ok("spattn_pull", H, ldh, d)) return rc;
    }
    const int vw = head_vw(pick_vw(d, {X, kH16 ? nullptr : (const void*)H, C}, {ldx, ldh, ldc}), d, heads);
    if (const int rc = width_ok("spattn_pull", d, vw, heads)) return rc;
    if (n == 0) return SGCN_OK;

    AttnArgs a{};
    a.rowptr = rowptr; a.col = col; a.own = X; a.ldown = ldx; a.gat = X; a.ldgat = ldx; a.out = C; a.ldo = ldc;
    a.lse_out = lse; a.scale = scale; a.d = d;
    const PullTab t{ids, map, H, ldh};
    return pull_run<false, HT>("spattn_pull", a, t, n, vw, heads, (hipStream_t)stream);
}

template <class HT>
static int spattn_pull_bwd_q(const int32_t* rowptr, const int32_t* col, const int32_t* ids, int32_t n, int32_t N,
                             const int32_t* map, int32_t d, int32_t heads, const float* X, int64_t ldx, const HT* H, int64_t ldh,
                             float scale, const float* G, int64_t ldg, const float* C, int64_t ldc, const float* lse, float* delta,
                             float* dQ, int64_t lddq, const float* add, int64_t ldadd, int32_t add_rows, void* stream) {
    constexpr bool kH16 = !std::is_same<HT, float>::value;
    if (const int rc = pull_open("spattn_pull_bwd_q", n, N, d, heads, scale)) return rc;
    SGCN_REQUIRE(ldx >= d && ldh >= d && ldg >= d && ldc >= d && lddq >= d, "spattn_pull_bwd_q: leading dimension smaller than d");
    SGCN_REQUIRE(n == 0 || (rowptr && col && ids && map && X && H && G && C && lse && delta && dQ), "spattn_pull_bwd_q: null operand");
    const bool with_add = add && add_rows > 0;
    if (with_add) SGCN_REQUIRE(ldadd >= d && add_rows <= n, "spattn_pull_bwd_q: bad addend");
    if constexpr (kH16) {
        if (n > 0)
            if (const int rc = h16_table_ok("spattn_pull_bwd_q", H, ldh, d)) return rc;
    }
    const int vw = head_vw(pick_vw(d, {X, kH16 ? nullptr : (const void*)H, G, C, dQ, with_add ? add : nullptr},
                                   {ldx, ldh, ldg, ldc, lddq, with_add ? ldadd : lddq}), d, heads);
    if (const int rc = width_ok("spattn_pull_bwd_q", d, vw, heads)) return rc;
    if (n == 0) return SGCN_OK;

    AttnArgs a{};
    a.rowptr = rowptr; a.col = col; a.own = X; a.ldown = ldx; a.gat = X; a.ldgat = ldx; a.G = G; a.ldg = ldg;
    a.Cf = C; a.ldcf = ldc; a.lse = lse; a.delta_out = delta; a.out = dQ; a.ldo = lddq; a.scale = scale; a.d = d;
    if (with_add) { a.add = add; a.ldadd = ldadd; a.add_rows = add_rows; }
    const PullTab t{ids, map, H, ldh};
    return pull_run<true, HT>("spattn_pull_bwd_q", a, t, n, vw, heads, (hipStream_t)stream);
}

}  // namespace sgcn

using namespace sgcn;

extern "C" int sgcn_spattn_pull_f32(const int32_t* rowptr, const int32_t* col, const int32_t* ids, int32_t n, int32_t N,
                                    const int32_t* map, int32_t d, int32_t heads, const float* X, int64_t ldx, const float* H,
                                    int64_t ldh, float scale, float* C, int64_t ldc, float* lse, void* stream) {
    return spattn_pull<float>(rowptr, col, ids, n, N, map, d, heads, X, ldx, H, ldh, scale, C, ldc, lse, stream);
}

/* mirrors sgcn_spattn_pull_f32 on a bfloat16 history */
extern "C" int sgcn_spattn_pull_h16(const int32_t* rowptr, const int32_t* col, const int32_t* ids, int32_t n, int32_t N,
                                    const int32_t* map, int32_t d, int32_t heads, const float* X, int64_t ldx, const uint16_t* H,
                                    int64_t ldh, float scale, float* C, int64_t ldc, float* lse, void* stream) {
    return spattn_pull<uint16_t>(rowptr, col, ids, n, N, map, d, heads, X, ldx, H, ldh, scale, C, ldc, lse, stream);
}

extern "C" int sgcn_spattn_pull_bwd_q_f32(const int32_t* rowptr, const int32_t* col, const int32_t* ids, int32_t n, int32_t N,
                                          const int32_t* map, int32_t d, int32_t heads, const float* X, int64_t ldx,
                                          const float* H, int64_t ldh, float scale, const float* G, int64_t ldg, const float* C,
                                          int64_t ldc, const float* lse, float* delta, float* dQ, int64_t lddq, const float* add,
                                          int64_t ldadd, int32_t add_rows, void* stream) {
    return spattn_pull_bwd_q<float>(rowptr, col, ids, n, N, map, d, heads, X, ldx, H, ldh, scale, G, ldg, C, ldc, lse, delta, dQ,
                                    lddq, add, ldadd, add_rows, stream);
}

/* mirrors sgcn_spattn_pull_bwd_q_f32 on a bfloat16 history */
extern "C" int sgcn_spattn_pull_bwd_q_h16(const int32_t* rowptr, const int32_t* col, const int32_t* ids, int32_t n, int32_t N,
                                          const int32_t* map, int32_t d, int32_t heads, const float* X, int64_t ldx,
                                          const uint16_t* H, int64_t ldh, float scale, const float* G, int64_t ldg, const float* C,
                                          int64_t ldc, const float* lse, float* delta, float* dQ, int64_t lddq, const float* add,
                                          int64_t ldadd, int32_t add_rows, void* stream) {
    return spattn_pull_bwd_q<uint16_t>(rowptr, col, ids, n, N, map, d, heads, X, ldx, H, ldh, scale, G, ldg, C, ldc, lse, delta, dQ,
                                       lddq, add, ldadd, add_rows, stream);
}
