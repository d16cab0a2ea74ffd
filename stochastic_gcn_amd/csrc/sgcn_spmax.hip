// Element-wise neighbour maximum over a CSR pattern for gfx950 (MI355X), and its backward:
//   forward   C[i, c] = max over the stored entries j of row i of B[j, c],  arg[i, c] = the FIRST such j in stored order
//   backward  dB[j, c] = sum over the rows i with arg[i, c] == j of G[i, c], in ascending i  (+ an addend in the epilogue)
//
// GraphSAGE's pooling aggregator without its MLP (--aggregator max, full-graph modes).  The stored values are not read:
// the pattern alone says who the neighbours are.  No arithmetic in the forward -- C holds bits of B -- and no atomics in
// the backward: it is a GATHER over the transposed pattern (row j of A^T lists its source rows i ascending; for each the
// kernel reads G[i, :] and arg[i, :] and adds where the id matches), so the result is bitwise reproducible.
//
// Shape of the kernels: the lane geometry of sgcn_spmm.hip -- a group of G lanes (8/16/32/64 from the row width) owns one
// row segment, every lane keeps NV vectors of VW elements (lane l owns vectors l, l + G, ..: a wavefront reads contiguous
// pieces of a gathered row), the segment's column ids are read G at a time and broadcast, U entries' loads are in flight
// before the first compare / add, wide rows are cut into feature slabs, and power-law rows into segments by the host plan
// of include/sgcn.h: a split row's segments write partial results to workspace slots and an ordered fix-up pass walks
// them -- with the same strict `>` forward, so the first maximum of the WHOLE row survives wherever the cuts fall, and
// by addition in slot order backward (the scheme of spmm_fix_kernel).  The host side of a launch (`run`) takes the plan checks,
// the geometry, the ladders and the fix-up's grid from sgcn_seg.h, as the row SpMM does; the forward's check of the id
// workspace is this file's own.
//
// The tie rule is np.argmax's: the best starts as the first entry, a later entry replaces it only when v > best.  That
// keeps the first of +0.0 / -0.0 and the first of equal values; +-inf are ordinary values; an empty row gives +0.0 and
// arg = -1.  NaN-free input is the caller's promise (a NaN never wins a strict comparison and, once first, never loses).
#include "sgcn_dev.h"
#include "sgcn_max_dev.h"
#include "sgcn_seg.h"

namespace sgcn {
namespace {

// (IVec, iload, isplat, istore_n, vstore_n and the forward's comparison max_take: sgcn_max_dev.h)

// fix-up: slot (v, ids c) against the running best; a slot that saw no entry (id < 0) never counts
template <int VW>
__device__ __forceinline__ void max_merge(typename Vec<VW>::type& best, typename IVec<VW>::type& barg,
                                          const typename Vec<VW>::type& v, const typename IVec<VW>::type& c) {
    if constexpr (VW == 1) {
        const bool t = c >= 0 && (barg < 0 || v > best);
        best = t ? v : best;
        barg = t ? c : barg;
    } else {
#pragma unroll
        for (int e = 0; e < VW; e++) {
            const bool t = c[e] >= 0 && (barg[e] < 0 || v[e] > best[e]);
            best[e] = t ? v[e] : best[e];
            barg[e] = t ? c[e] : barg[e];
        }
    }
}
// backward: acc += g where the winner recorded for this element is `row`
template <int VW>
__device__ __forceinline__ void add_where(typename Vec<VW>::type& acc, const typename Vec<VW>::type& g,
                                          const typename IVec<VW>::type& id, int row) {
    if constexpr (VW == 1) acc = id == row ? acc + g : acc;
    else {
#pragma unroll
        for (int e = 0; e < VW; e++) acc[e] = id[e] == row ? acc[e] + g[e] : acc[e];
    }
}

struct SpmaxArgs {
    const int32_t* rowptr;
    const int32_t* col;      // forward: column ids; backward: the source rows of the transposed pattern
    const sgcn_seg_t* seg;   // nullable: implicit one segment per row
    int64_t nseg;
    int64_t nsegblk;         // blocks per slab
    const float* B;          // forward: the K x d table; backward: the incoming gradient G (M x d)
    int64_t ldb;
    const int32_t* id;       // backward: the forward's arg (M x d)
    int64_t ldid;
    float* C;                // forward: C; backward: dB
    int64_t ldc;
    int32_t* arg;            // forward: nullable (evaluation)
    int64_t ldarg;
    int32_t d;
    int32_t nvec;            // ceil(d / VW)
    float* ws;
    int32_t* wsa;            // forward: the slots' ids, the geometry of ws
    int64_t ldw;
    int32_t slabmajor;
    const float* add;        // backward: dB[row] += add[row] for row < add_rows
    int64_t ldadd;
    int32_t add_rows;
};

// the block's slab and the group's segment (sgcn_spmm.hip spmm_seg_kernel); false: no segment for this group
template <int G>
__device__ __forceinline__ bool my_segment(const SpmaxArgs& a, int& slab, int& row, int& start, int& end, int& slot) {
    constexpr int GPB = kBlock / G;
    const int gib = threadIdx.x / G;
    int64_t sblk;
    if (a.slabmajor) { slab = (int)(blockIdx.x / a.nsegblk); sblk = blockIdx.x % a.nsegblk; }
    else { const int nslab = (int)(gridDim.x / a.nsegblk); slab = blockIdx.x % nslab; sblk = blockIdx.x / nslab; }
    const int64_t s = sblk * GPB + gib;
    if (s >= a.nseg) return false;
    if (a.seg) {
        const sgcn_seg_t sg = a.seg[s];
        row = sg.row; start = sg.start; end = sg.end; slot = sg.slot;
    } else {
        row = (int)s; start = a.rowptr[s]; end = a.rowptr[s + 1]; slot = -1;
    }
    row = uniform_i<G>(row); start = uniform_i<G>(start);
    end = uniform_i<G>(end); slot = uniform_i<G>(slot);
    return true;
}

template <int NV>
struct Unroll { static constexpr int fwd = NV >= 3 ? 4 : 8, bwd = NV >= 3 ? 2 : (NV == 2 ? 4 : 8); };

template <int G, int NV, int VW>
__global__ __launch_bounds__(kBlock) void spmax_seg_kernel(SpmaxArgs a) {
    typedef typename Vec<VW>::type VT;
    typedef typename IVec<VW>::type IT;
    constexpr int U = Unroll<NV>::fwd;
    const int lig = threadIdx.x & (G - 1);
    int slab, row, start, end, slot;
    if (!my_segment<G>(a, slab, row, start, end, slot)) return;

    const int vbase = slab * (G * NV) + lig;
    bool act[NV];
    VT best[NV];
    IT barg[NV];
    // Lanes past the row width re-read the last valid vector instead of branching around the load (their results are
    // never stored): the gather loop stays branch-free.
    uint32_t loff[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) {
        const int vi = vbase + k * G;
        act[k] = vi < a.nvec;
        loff[k] = (uint32_t)min(vi, a.nvec - 1) * (uint32_t)(VW * sizeof(float));
    }
    const char* Bb = reinterpret_cast<const char*>(a.B);
    const int64_t ldb_bytes = a.ldb * (int64_t)sizeof(float);

    // the best starts as the segment's first entry ...
    if (start < end) {
        const int c0 = uniform_i<G>(a.col[start]);
        const char* src = Bb + (int64_t)c0 * ldb_bytes;
#pragma unroll
        for (int k = 0; k < NV; k++) {
            best[k] = vload<VW>(reinterpret_cast<const float*>(src + loff[k]));
            barg[k] = isplat<VW>(c0);
        }
    } else {
#pragma unroll
        for (int k = 0; k < NV; k++) { best[k] = vzero<VW>(); barg[k] = isplat<VW>(-1); }
    }
    // ... and every later one is held against it, in stored order
    for (int p0 = start + 1; p0 < end; p0 += G) {
        const int n = min(G, end - p0);
        int mycol = 0;
        if (lig < n) mycol = a.col[p0 + lig];
        int j = 0;
        for (; j + U <= n; j += U) {
            VT b[U][NV];
            int c[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                c[u] = bcast_i<G>(mycol, j + u);
                const char* src = Bb + (int64_t)c[u] * ldb_bytes;   // G == 64: scalar base
#pragma unroll
                for (int k = 0; k < NV; k++) b[u][k] = vload<VW>(reinterpret_cast<const float*>(src + loff[k]));
            }
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int k = 0; k < NV; k++) max_take<VW>(best[k], barg[k], b[u][k], c[u]);
        }
        for (; j < n; j++) {
            const int c = bcast_i<G>(mycol, j);
            const char* src = Bb + (int64_t)c * ldb_bytes;
#pragma unroll
            for (int k = 0; k < NV; k++)
                max_take<VW>(best[k], barg[k], vload<VW>(reinterpret_cast<const float*>(src + loff[k])), c);
        }
    }

    if (slot < 0) {
#pragma unroll
        for (int k = 0; k < NV; k++)
            if (act[k]) {
                const int vi = vbase + k * G, left = a.d - vi * VW;   // > 0 by construction
                vstore_n<VW>(a.C + (int64_t)row * a.ldc + (int64_t)vi * VW, best[k], left);
                if (a.arg) istore_n<VW>(a.arg + (int64_t)row * a.ldarg + (int64_t)vi * VW, barg[k], left);
            }
    } else {
        const int64_t w = (int64_t)slot * a.ldw + (int64_t)vbase * VW;
#pragma unroll
        for (int k = 0; k < NV; k++)
            if (act[k]) {
                vstore<VW>(a.ws + w + (int64_t)k * G * VW, best[k]);
                *reinterpret_cast<IT*>(a.wsa + w + (int64_t)k * G * VW) = barg[k];
            }
    }
}

// A split row's slots in order, with the forward's own comparison: the first maximum of the whole row.
template <int VW>
__global__ __launch_bounds__(kBlock) void spmax_fix_kernel(SpmaxArgs a, const sgcn_fix_t* fix, int64_t nfix) {
    typedef typename Vec<VW>::type VT;
    typedef typename IVec<VW>::type IT;
    const int nvblk = (a.nvec + kBlock - 1) / kBlock;
    const int64_t f = blockIdx.x / nvblk;
    if (f >= nfix) return;
    const sgcn_fix_t fx = fix[f];
    const int vi = (int)(blockIdx.x % nvblk) * kBlock + threadIdx.x;
    if (vi >= a.nvec) return;
    const int64_t w = (int64_t)fx.first_slot * a.ldw + (int64_t)vi * VW;
    VT best = vzero<VW>();
    IT barg = isplat<VW>(-1);
    for (int q = 0; q < fx.nslots; q++)
        max_merge<VW>(best, barg, vload<VW>(a.ws + w + (int64_t)q * a.ldw), iload<VW>(a.wsa + w + (int64_t)q * a.ldw));
    const int left = a.d - vi * VW;
    vstore_n<VW>(a.C + (int64_t)fx.row * a.ldc + (int64_t)vi * VW, best, left);
    if (a.arg) istore_n<VW>(a.arg + (int64_t)fx.row * a.ldarg + (int64_t)vi * VW, barg, left);
}

template <int VW>
__device__ __forceinline__ void bwd_store(const SpmaxArgs& a, int row, int vi, typename Vec<VW>::type r) {
    const int left = a.d - vi * VW;   // > 0 by construction
    if (a.add && row < a.add_rows) {     // the self half of a concat aggregator
        const float* ad = a.add + (int64_t)row * a.ldadd + (int64_t)vi * VW;
        if (left >= VW) r += vload<VW>(ad);
        else {
#pragma unroll
            for (int e = 0; e < VW; e++)
                if (e < left) {
                    if constexpr (VW == 1) r += ad[0]; else r[e] += ad[e];
                }
        }
    }
    vstore_n<VW>(a.C + (int64_t)row * a.ldc + (int64_t)vi * VW, r, left);
}

template <int G, int NV, int VW>
__global__ __launch_bounds__(kBlock) void spmax_bwd_seg_kernel(SpmaxArgs a) {
    typedef typename Vec<VW>::type VT;
    typedef typename IVec<VW>::type IT;
    constexpr int U = Unroll<NV>::bwd;
    const int lig = threadIdx.x & (G - 1);
    int slab, row, start, end, slot;
    if (!my_segment<G>(a, slab, row, start, end, slot)) return;

    const int vbase = slab * (G * NV) + lig;
    bool act[NV];
    VT acc[NV];
    uint32_t loff[NV];                   // the same byte offset into a row of G and a row of arg: both hold 4-byte elements
#pragma unroll
    for (int k = 0; k < NV; k++) {
        const int vi = vbase + k * G;
        act[k] = vi < a.nvec;
        acc[k] = vzero<VW>();
        loff[k] = (uint32_t)min(vi, a.nvec - 1) * (uint32_t)(VW * sizeof(float));
    }
    const char* Gb = reinterpret_cast<const char*>(a.B);
    const char* Ib = reinterpret_cast<const char*>(a.id);
    const int64_t ldg_bytes = a.ldb * (int64_t)sizeof(float), ldid_bytes = a.ldid * (int64_t)sizeof(int32_t);

    for (int p0 = start; p0 < end; p0 += G) {
        const int n = min(G, end - p0);
        int myrow = 0;
        if (lig < n) myrow = a.col[p0 + lig];
        int j = 0;
        for (; j + U <= n; j += U) {
            VT g[U][NV];
            IT id[U][NV];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int i = bcast_i<G>(myrow, j + u);
                const char* gs = Gb + (int64_t)i * ldg_bytes;       // G == 64: scalar bases
                const char* is = Ib + (int64_t)i * ldid_bytes;
#pragma unroll
                for (int k = 0; k < NV; k++) {
                    g[u][k] = vload<VW>(reinterpret_cast<const float*>(gs + loff[k]));
                    id[u][k] = iload<VW>(reinterpret_cast<const int32_t*>(is + loff[k]));
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int k = 0; k < NV; k++) add_where<VW>(acc[k], g[u][k], id[u][k], row);
        }
        for (; j < n; j++) {
            const int i = bcast_i<G>(myrow, j);
            const char* gs = Gb + (int64_t)i * ldg_bytes;
            const char* is = Ib + (int64_t)i * ldid_bytes;
#pragma unroll
            for (int k = 0; k < NV; k++)
                add_where<VW>(acc[k], vload<VW>(reinterpret_cast<const float*>(gs + loff[k])),
                              iload<VW>(reinterpret_cast<const int32_t*>(is + loff[k])), row);
        }
    }

    if (slot < 0) {
#pragma unroll
        for (int k = 0; k < NV; k++)
            if (act[k]) bwd_store<VW>(a, row, vbase + k * G, acc[k]);
    } else {
        float* w = a.ws + (int64_t)slot * a.ldw + (int64_t)vbase * VW;
#pragma unroll
        for (int k = 0; k < NV; k++)
            if (act[k]) vstore<VW>(w + (int64_t)k * G * VW, acc[k]);
    }
}

// Ordered sum of the workspace slots of every split row, then the same epilogue.
template <int VW>
__global__ __launch_bounds__(kBlock) void spmax_bwd_fix_kernel(SpmaxArgs a, const sgcn_fix_t* fix, int64_t nfix) {
    typedef typename Vec<VW>::type VT;
    const int nvblk = (a.nvec + kBlock - 1) / kBlock;
    const int64_t f = blockIdx.x / nvblk;
    if (f >= nfix) return;
    const sgcn_fix_t fx = fix[f];
    const int vi = (int)(blockIdx.x % nvblk) * kBlock + threadIdx.x;
    if (vi >= a.nvec) return;
    const float* w = a.ws + (int64_t)fx.first_slot * a.ldw + (int64_t)vi * VW;
    VT acc = vzero<VW>();
    for (int q = 0; q < fx.nslots; q++) acc += vload<VW>(w + (int64_t)q * a.ldw);
    bwd_store<VW>(a, fx.row, vi, acc);
}

// A launch from its checked arguments: the plan's tables, the lane geometry and the ladder of sgcn_seg.h, then the ordered
// fix-up where the plan has split rows.  `a` arrives with its operands set; nrows = rows of the pattern at hand.
template <bool BWD>
int run(SpmaxArgs& a, const char* who, int32_t nrows, const sgcn_plan_t* plan, int vw, hipStream_t st) {
    a.nseg = nrows;
    a.slabmajor = tune_get("spmm_slabmajor");
    if (plan) { a.seg = plan->dev_seg; a.nseg = plan->nseg; }
    a.nvec = (a.d + vw - 1) / vw;
    const SegGeom g = seg_geometry(a.nvec, a.nseg);
    a.nsegblk = g.nsegblk;
    SGCN_REQUIRE(g.nblocks < (1ll << 31), "%s: grid too large", who);

    const dim3 grid((unsigned)g.nblocks), block(kBlock);
    const bool ok = with_vw(vw, [&](auto VW) {
        return with_gnv(g.G, g.NV, [&](auto G, auto NV) {
            constexpr int kG = decltype(G)::value, kNV = decltype(NV)::value, kVW = decltype(VW)::value;
            if constexpr (BWD) hipLaunchKernelGGL((spmax_bwd_seg_kernel<kG, kNV, kVW>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((spmax_seg_kernel<kG, kNV, kVW>), grid, block, 0, st, a);
        });
    });
    SGCN_REQUIRE(ok, "%s: no kernel for G=%d NV=%d", who, g.G, g.NV);
    SGCN_HIP_TRY(hipGetLastError());

    if (plan && plan->nfix > 0) {
        const int64_t nfblk = seg_fix_blocks(a.nvec, plan->nfix);
        SGCN_REQUIRE(nfblk < (1ll << 31), "%s: too many split rows", who);
        const dim3 fgrid((unsigned)nfblk);
        with_vw(vw, [&](auto VW) {
            constexpr int kVW = decltype(VW)::value;
            if constexpr (BWD) hipLaunchKernelGGL((spmax_bwd_fix_kernel<kVW>), fgrid, block, 0, st, a, plan->dev_fix, plan->nfix);
            else hipLaunchKernelGGL((spmax_fix_kernel<kVW>), fgrid, block, 0, st, a, plan->dev_fix, plan->nfix);
        });
        SGCN_HIP_TRY(hipGetLastError());
    }
    return SGCN_OK;
}

}  // namespace
}  // namespace sgcn

using namespace sgcn;

extern "C" int sgcn_spmax_csr_f32(const int32_t* rowptr, const int32_t* col, int32_t M, int32_t K, int32_t d,
                                  const float* B, int64_t ldb, float* C, int64_t ldc, int32_t* arg, int64_t ldarg,
                                  const sgcn_plan_t* plan, int32_t* dev_ws_arg, void* stream) {
    SGCN_REQUIRE(M >= 0 && K >= 0, "spmax: negative size");
    SGCN_REQUIRE(d > 0, "spmax: d must be positive (got %d)", d);
    SGCN_REQUIRE(rowptr && C && (B || K == 0), "spmax: null operand");
    SGCN_REQUIRE(ldb >= d && ldc >= d && (!arg || ldarg >= d), "spmax: leading dimension smaller than d");
    const int64_t ldw = seg_slot_pitch(d);
    if (plan) {
        if (const int rc = seg_plan_tables("spmax", plan, M)) return rc;
        SGCN_REQUIRE(plan->nfix <= 0 || dev_ws_arg, "spmax: plan with split rows needs dev_ws_arg (the slots' ids)");
        if (const int rc = seg_plan_room("spmax", plan, ldw)) return rc;
    }
    if (M == 0) return SGCN_OK;

    SpmaxArgs a{};
    a.rowptr = rowptr; a.col = col; a.B = B; a.ldb = ldb; a.C = C; a.ldc = ldc; a.arg = arg; a.ldarg = ldarg; a.d = d;
    const bool split = plan && plan->nfix > 0;
    if (split) { a.ws = plan->dev_ws; a.wsa = dev_ws_arg; a.ldw = ldw; }
    const int vw = pick_vw(d, {B, C, arg, split ? (const void*)a.ws : nullptr, split ? (const void*)a.wsa : nullptr},
                           {ldb, ldc, arg ? ldarg : ldc});
    return run<false>(a, "spmax", M, plan, vw, (hipStream_t)stream);
}

extern "C" int sgcn_spmax_csr_bwd_f32(const int32_t* t_rowptr, const int32_t* t_row, int32_t K, int32_t M, int32_t d,
                                      const float* G, int64_t ldg, const int32_t* arg, int64_t ldarg, float* dB, int64_t lddb,
                                      const float* add, int64_t ldadd, int32_t add_rows, const sgcn_plan_t* t_plan,
                                      void* stream) {
    SGCN_REQUIRE(M >= 0 && K >= 0, "spmax_bwd: negative size");
    SGCN_REQUIRE(d > 0, "spmax_bwd: d must be positive (got %d)", d);
    SGCN_REQUIRE(t_rowptr && dB && ((G && arg) || M == 0), "spmax_bwd: null operand");
    SGCN_REQUIRE(ldg >= d && ldarg >= d && lddb >= d, "spmax_bwd: leading dimension smaller than d");
    const bool with_add = add && add_rows > 0;
    if (with_add) SGCN_REQUIRE(ldadd >= d && add_rows <= K, "spmax_bwd: bad addend");
    const int64_t ldw = seg_slot_pitch(d);
    if (t_plan)
        if (const int rc = seg_plan_ok("spmax_bwd", t_plan, K, ldw)) return rc;
    if (K == 0) return SGCN_OK;

    SpmaxArgs a{};
    a.rowptr = t_rowptr; a.col = t_row; a.B = G; a.ldb = ldg; a.id = arg; a.ldid = ldarg; a.C = dB; a.ldc = lddb; a.d = d;
    if (with_add) { a.add = add; a.ldadd = ldadd; a.add_rows = add_rows; }
    const bool split = t_plan && t_plan->nfix > 0;
    if (split) { a.ws = t_plan->dev_ws; a.ldw = ldw; }
    const int vw = pick_vw(d, {G, arg, dB, a.add, split ? (const void*)a.ws : nullptr},
                           {ldg, ldarg, lddb, with_add ? ldadd : lddb});
    return run<true>(a, "spmax_bwd", K, t_plan, vw, (hipStream_t)stream);
}
