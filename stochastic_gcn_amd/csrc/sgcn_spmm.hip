// CSR x dense SpMM for gfx950 (MI355X):  C = rscale (.) (A (cscale (.) B[g])) + beta C.
//
// Replaces tf.sparse_tensor_dense_matmul at gcn/layers.py:31-37 (K1/K3/K4/K5/K11 in
// SURVEY.md §2.1), fused with the tf.gather of history rows (K2+K7, gcn/layers.py:304-308)
// and, called on the transposed CSR, its autodiff backward dB = A^T dC (K6).
//
// Shape of the kernel (HBM/cache-bound gather; no MFMA on purpose -- the sparse operand has
// no dense tiles to feed a matrix core):
//   * a GROUP of G lanes owns one row segment (G = 8/16/32/64 chosen from the row width so
//     that a group reads whole 16-byte vectors of a B row; G = 64 = one wavefront for wide
//     rows, several rows per wavefront for d <= 128);
//   * the segment's (col, val) pairs are read G at a time, coalesced, one pair per lane, and
//     broadcast with v_readlane (G = 64: the B-row base lives in SGPRs, the lane offset in a
//     VGPR) or ds_bpermute (G < 64);
//   * every lane keeps NV float4 accumulators: lane l owns vectors l, l+G, l+2G.. of the slab,
//     so a wavefront's loads of one B row are contiguous 1 KiB pieces (coalesced HBM/L2
//     reads of the dense operand);
//   * U nonzeros are in flight per group before the first FMA (memory-level parallelism:
//     U * NV dwordx4 loads per lane outstanding);
//   * wide rows can be cut into feature slabs (slab-major block order so one B slab stays
//     resident in the 256 MiB Infinity Cache while every row visits it);
//   * power-law rows are cut into <= T-nonzero segments by a host plan (include/sgcn.h);
//     split rows go through workspace slots and an ordered fix-up pass (deterministic).
// The host side of a launch -- the checks on the plan, G / NV / slabs / grid, the ladders over (VW, G, NV), the fix-up's grid --
// is sgcn_seg.h's, shared with every kernel over a row pattern; spmm_csr_add adds the operand checks, the operand list the
// vector width is picked from, the unroll U and the two tuning knobs (spmm_nv, spmm_unroll).
#include "sgcn_dev.h"
#include "sgcn_seg.h"
#include <cstring>

namespace sgcn {

namespace {
int g_tune_nv = 0;
int g_tune_unroll = 0;
int g_tune_slabmajor = 1;
int g_tune_cs_round = 0;
int g_tune_cs_unroll = 0;
int g_tune_cs_pace = 0;
int g_tune_cs_slack = 0;
int g_tune_cs_noextra = 0;
int g_tune_cs_deal = 1;               // lane-group plans (sgcn_csplan.cpp): 1 = rows dealt to bins by column spread too, 0 = by weight alone
int g_tune_cs_dict = 1;               // lane-group plans (sgcn_csbuild_dict): 1 = per-tile value tables where every tile has few distinct values
int g_tune_step_overlap = 1;
int g_tune_step_fuse = 127;           // bit 0: the output layer's forward as the loss kernel's head, bit 1: its input gradient as the
                                     // tail, bit 2: the dense layer behind a split-K layer in that layer's reduce pass, bit 3: a layer's
                                     // input gradient in its LayerNorm / ReLU backward pass, bit 4: the dense layer in front of the output
                                     // layer as the pre-layer of the loss kernel's head, bit 5: the weight gradients' reductions in the
                                     // optimizer's launch, bit 6: the first layer's LayerNorm backward behind the second layer's row pass
int g_tune_cs_g2_wide = 0;
int g_tune_cs_nowarp = 0;            // experiments: ignore a plan's warp table (the sweep clock linear in the column id)
int g_tune_cs_last_pct = 80;          // (round 4: 80 % holds the lock-step on the 90-column pass of d = 602: 3.16 vs 3.22 ms at 90, 3.43 at 70)
int g_tune_gemm_min_steps = 0;
int g_tune_gemm_mb16_slice_k = 0;   // sgcn_gemm_mb16.hip: least K per split-K slice (0: its default)
int g_tune_lds_wave_bias = 100;    // LDS plan: entries of a tile's waves 0-3 per 100 of its waves 4-7 (100: even; made moot by the s_setprio around the update chain)
int g_tune_lds_mix = 1;            // LDS plan: columns a tile uses once or twice dealt into the chunks among the reused ones (all-staged plans)
int g_tune_lds_dbg = 0;             // experiments on the LDS sweep: bit 0 no ring fills after the first, bit 1 no arithmetic
// a step program's own MODE (sgcn_step_run): seen by the entry points that very thread calls during the run, by nobody else
thread_local int tl_step_overlap = -1, tl_step_fuse = -1;
}  // namespace

void step_mode_override(int overlap, int fuse) { tl_step_overlap = overlap; tl_step_fuse = fuse; }

int tune_get(const char* key) {
    if (!strcmp(key, "spmm_nv")) return g_tune_nv;
    if (!strcmp(key, "spmm_unroll")) return g_tune_unroll;
    if (!strcmp(key, "spmm_slabmajor")) return g_tune_slabmajor;
    if (!strcmp(key, "cs_round")) return g_tune_cs_round;
    if (!strcmp(key, "cs_unroll")) return g_tune_cs_unroll;
    if (!strcmp(key, "cs_pace")) return g_tune_cs_pace;
    if (!strcmp(key, "cs_slack")) return g_tune_cs_slack;
    if (!strcmp(key, "cs_noextra")) return g_tune_cs_noextra;
    if (!strcmp(key, "cs_deal")) return g_tune_cs_deal;
    if (!strcmp(key, "cs_dict")) return g_tune_cs_dict;
    if (!strcmp(key, "step_overlap")) return tl_step_overlap >= 0 ? tl_step_overlap : g_tune_step_overlap;
    if (!strcmp(key, "step_fuse")) return tl_step_fuse >= 0 ? tl_step_fuse : g_tune_step_fuse;
    if (!strcmp(key, "cs_g2_wide")) return g_tune_cs_g2_wide;
    if (!strcmp(key, "cs_nowarp")) return g_tune_cs_nowarp;
    if (!strcmp(key, "cs_last_pct")) return g_tune_cs_last_pct;
    if (!strcmp(key, "gemm_min_steps")) return g_tune_gemm_min_steps;
    if (!strcmp(key, "gemm_mb16_slice_k")) return g_tune_gemm_mb16_slice_k;
    if (!strcmp(key, "lds_wave_bias")) return g_tune_lds_wave_bias;
    if (!strcmp(key, "lds_mix")) return g_tune_lds_mix;
    if (!strcmp(key, "lds_dbg")) return g_tune_lds_dbg;
    return -1;
}

struct SpmmArgs {
    const int32_t* rowptr;
    const int32_t* col;
    const float* val;
    const sgcn_seg_t* seg;   // nullable: implicit one segment per row
    int64_t nseg;
    int64_t nsegblk;         // blocks per slab
    const void* B;           // fp32, or uint16 for a bfloat16 operand (sgcn_spmm_csr_b16): the kernel's BT says which
    int64_t ldb;             // in elements of B
    const int32_t* gidx;
    const float* rscale;
    const float* cscale;
    float* C;
    int64_t ldc;
    float beta;
    int32_t d;
    int32_t nvec;            // ceil(d / VW)
    float* ws;
    int64_t ldw;
    int32_t slabmajor;
    const float* add;        // optional addend: C[row] += add[row] for row < add_rows
    int64_t ldadd;
    int32_t add_rows;
};

template <int VW>
__device__ __forceinline__ void epilogue_store(const SpmmArgs& a, int row, int vi,
                                               typename Vec<VW>::type acc, float rs) {
    float* out = a.C + (int64_t)row * a.ldc + (int64_t)vi * VW;
    typename Vec<VW>::type r = acc * rs;
    const int left = a.d - vi * VW;   // > 0 by construction
    if (a.beta != 0.f) {
        if (left >= VW) r += a.beta * vload<VW>(out);
        else {
#pragma unroll
            for (int e = 0; e < VW; e++)
                if (e < left) {
                    if constexpr (VW == 1) r += a.beta * out[0]; else r[e] += a.beta * out[e];
                }
        }
    }
    if (a.add && row < a.add_rows) {     // e.g. the self term of a concat aggregator's backward
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
    if (left >= VW) vstore<VW>(out, r);
    else vstore_head<VW>(out, r, left);
}

// BT: the dense operand's element -- float, or uint16_t for a bfloat16 table (sgcn_spmm_csr_b16).  The two instantiations
// differ in the load (hraw: 2 * VW bytes per lane instead of 4 * VW), the byte offsets that go with it and the widening in
// front of the multiply-add (hwiden: bits << 16, exact); lanes, order of the sums and epilogue are the same, so the bf16
// form gives the bits of the fp32 form on the widened table.  As in sgcn_agg.hip the raw dwords stay pinned (hpin)
// between the U requests and the updates, or every load would be followed by its wait; and the multiply-add the fp32
// form gets by contraction is spelled out, because the compiler does not contract across the widening shift.  Scalar
// lanes (VW == 1) are the exception, as in sgcn_agg.hip: there the fp32 form's U products are only PARTLY contracted
// (packed multiplies, then adds), and the plain, unpinned expression is what gets the same ones.  That is the compiler's
// choice, not the source's: after a toolchain change tests/test_spmm_b16_gpu.py (d = 1, 3, odd output pitches) says whether
// it still holds, as tests/test_history_bf16_gpu.py does for the aggregator.
template <int G, int NV, int VW, int U, class BT>
__global__ __launch_bounds__(kBlock) void spmm_seg_kernel(SpmmArgs a) {
    typedef typename Vec<VW>::type VT;
    typedef typename HRaw<BT, VW>::type RT;
    constexpr bool kB16 = !std::is_same<BT, float>::value;
    constexpr int GPB = kBlock / G;
    const int lig = threadIdx.x & (G - 1);
    const int gib = threadIdx.x / G;

    int slab;
    int64_t sblk;
    if (a.slabmajor) { slab = (int)(blockIdx.x / a.nsegblk); sblk = blockIdx.x % a.nsegblk; }
    else { const int nslab = (int)(gridDim.x / a.nsegblk); slab = blockIdx.x % nslab; sblk = blockIdx.x / nslab; }
    const int64_t s = sblk * GPB + gib;
    if (s >= a.nseg) return;

    int row, start, end, slot;
    if (a.seg) {
        const sgcn_seg_t sg = a.seg[s];
        row = sg.row; start = sg.start; end = sg.end; slot = sg.slot;
    } else {
        row = (int)s; start = a.rowptr[s]; end = a.rowptr[s + 1]; slot = -1;
    }
    row = uniform_i<G>(row); start = uniform_i<G>(start);
    end = uniform_i<G>(end); slot = uniform_i<G>(slot);

    const int vbase = slab * (G * NV) + lig;
    bool act[NV];
    VT acc[NV];
    // Lanes past the row width re-read the last valid vector instead of branching around the
    // load (their accumulators are never stored): the gather loop stays branch-free.
    uint32_t loff[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) {
        const int vi = vbase + k * G;
        act[k] = vi < a.nvec;
        acc[k] = vzero<VW>();
        loff[k] = (uint32_t)min(vi, a.nvec - 1) * (uint32_t)(VW * sizeof(BT));
    }
    const char* Bb = reinterpret_cast<const char*>(a.B);
    const int64_t ldb_bytes = a.ldb * (int64_t)sizeof(BT);

    for (int p0 = start; p0 < end; p0 += G) {
        const int n = min(G, end - p0);
        int mycol = 0;
        float myval = 0.f;
        if (lig < n) {
            mycol = a.col[p0 + lig];
            myval = a.val[p0 + lig];
            if (a.cscale) myval *= a.cscale[mycol];
            if (a.gidx) mycol = a.gidx[mycol];
        }
        int j = 0;
        for (; j + U <= n; j += U) {
            RT b[U][NV];
            float v[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int c = bcast_i<G>(mycol, j + u);
                v[u] = bcast_f<G>(myval, j + u);
                const char* src = Bb + (int64_t)c * ldb_bytes;   // G == 64: scalar base
#pragma unroll
                for (int k = 0; k < NV; k++)
                    b[u][k] = hraw<VW>(reinterpret_cast<const BT*>(src + loff[k]));
            }
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int k = 0; k < NV; k++) {
                    if constexpr (kB16 && VW > 1) { hpin<BT, VW>(b[u][k]); acc[k] = vfma<VW>(v[u], hwiden<VW>(b[u][k]), acc[k]); }
                    else acc[k] += v[u] * hwiden<VW>(b[u][k]);
                }
        }
        for (; j < n; j++) {
            const int c = bcast_i<G>(mycol, j);
            const float v = bcast_f<G>(myval, j);
            const char* src = Bb + (int64_t)c * ldb_bytes;
#pragma unroll
            for (int k = 0; k < NV; k++) {
                if constexpr (kB16 && VW > 1) acc[k] = vfma<VW>(v, hload<VW>(reinterpret_cast<const BT*>(src + loff[k])), acc[k]);
                else acc[k] += v * hload<VW>(reinterpret_cast<const BT*>(src + loff[k]));
            }
        }
    }

    if (slot < 0) {
        const float rs = a.rscale ? a.rscale[row] : 1.0f;
#pragma unroll
        for (int k = 0; k < NV; k++)
            if (act[k]) epilogue_store<VW>(a, row, vbase + k * G, acc[k], rs);
    } else {
        float* w = a.ws + (int64_t)slot * a.ldw + (int64_t)vbase * VW;
#pragma unroll
        for (int k = 0; k < NV; k++)
            if (act[k]) vstore<VW>(w + (int64_t)k * G * VW, acc[k]);
    }
}

// Ordered sum of the workspace slots of every split row, then the same epilogue.
template <int VW>
__global__ __launch_bounds__(kBlock) void spmm_fix_kernel(SpmmArgs a, const sgcn_fix_t* fix,
                                                          int64_t nfix) {
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
    const float rs = a.rscale ? a.rscale[fx.row] : 1.0f;
    epilogue_store<VW>(a, fx.row, vi, acc, rs);
}

}  // namespace sgcn

using namespace sgcn;

extern "C" int64_t sgcn_tune_get(const char* key) { return key ? tune_get(key) : -1; }

extern "C" int sgcn_tune(const char* key, int64_t value) {
    if (!key) return fail(SGCN_ERR_INVALID, "sgcn_tune: null key");
    if (!strcmp(key, "spmm_nv")) { SGCN_REQUIRE(value >= 0 && value <= 4, "spmm_nv in 0..4"); g_tune_nv = (int)value; return SGCN_OK; }
    if (!strcmp(key, "spmm_unroll")) {
        SGCN_REQUIRE(value == 0 || value == 2 || value == 4 || value == 8, "spmm_unroll in {0,2,4,8}");
        g_tune_unroll = (int)value; return SGCN_OK;
    }
    if (!strcmp(key, "spmm_slabmajor")) { g_tune_slabmajor = value != 0; return SGCN_OK; }
    if (!strcmp(key, "cs_pace")) { SGCN_REQUIRE(value >= 0, "cs_pace >= 0"); g_tune_cs_pace = (int)value; return SGCN_OK; }
    if (!strcmp(key, "cs_slack")) { SGCN_REQUIRE(value >= 0, "cs_slack >= 0"); g_tune_cs_slack = (int)value; return SGCN_OK; }
    if (!strcmp(key, "cs_noextra")) { g_tune_cs_noextra = value != 0; return SGCN_OK; }
    if (!strcmp(key, "cs_deal")) { SGCN_REQUIRE(value == 0 || value == 1, "cs_deal in {0, 1}"); g_tune_cs_deal = (int)value; return SGCN_OK; }
    if (!strcmp(key, "cs_dict")) { SGCN_REQUIRE(value == 0 || value == 1, "cs_dict in {0, 1}"); g_tune_cs_dict = (int)value; return SGCN_OK; }
    if (!strcmp(key, "step_overlap")) { g_tune_step_overlap = value != 0; return SGCN_OK; }
    if (!strcmp(key, "step_fuse")) { SGCN_REQUIRE(value >= 0 && value <= 127, "step_fuse in 0..127"); g_tune_step_fuse = (int)value; return SGCN_OK; }
    if (!strcmp(key, "cs_g2_wide")) { g_tune_cs_g2_wide = value != 0; return SGCN_OK; }
    if (!strcmp(key, "cs_nowarp")) { g_tune_cs_nowarp = value != 0; return SGCN_OK; }
    if (!strcmp(key, "gemm_min_steps")) { g_tune_gemm_min_steps = (int)value; return SGCN_OK; }
    if (!strcmp(key, "gemm_mb16_slice_k")) {
        SGCN_REQUIRE(value >= 0 && value <= 0x7fffffff, "gemm_mb16_slice_k >= 0");
        g_tune_gemm_mb16_slice_k = (int)value; return SGCN_OK;
    }
    if (!strcmp(key, "lds_wave_bias")) { SGCN_REQUIRE(value >= 50 && value <= 300, "lds_wave_bias in 50..300 (per cent)"); g_tune_lds_wave_bias = (int)value; return SGCN_OK; }
    if (!strcmp(key, "lds_mix")) { g_tune_lds_mix = value != 0; return SGCN_OK; }
    if (!strcmp(key, "lds_dbg")) { g_tune_lds_dbg = (int)value; return SGCN_OK; }
    if (!strcmp(key, "cs_last_pct")) { SGCN_REQUIRE(value >= 0 && value <= 100, "cs_last_pct in [0, 100]"); g_tune_cs_last_pct = (int)value; return SGCN_OK; }
    if (!strcmp(key, "cs_round")) { SGCN_REQUIRE(value >= 0, "cs_round >= 0"); g_tune_cs_round = (int)value; return SGCN_OK; }
    if (!strcmp(key, "cs_unroll")) {
        SGCN_REQUIRE(value == 0 || value == 4 || value == 8, "cs_unroll in {0,4,8}");
        g_tune_cs_unroll = (int)value; return SGCN_OK;
    }
    return fail(SGCN_ERR_INVALID, "sgcn_tune: unknown key '%s'", key);
}

// BT = float: sgcn_spmm_csr_add_f32.  BT = uint16_t: sgcn_spmm_csr_add_b16 -- the operand is K x ldb uint16 (ldb in ELEMENTS,
// a multiple of 8, base 16-byte aligned), which never limits the vector width: VW, G, NV and U are what the fp32 call
// picks for a 16-byte aligned fp32 table of the same element pitch (the table's pointer is left out of pick_vw, its pitch
// is not), and every sum is taken in that call's order.
template <class BT>
static int spmm_csr_add(const int32_t* rowptr, const int32_t* col, const float* val,
                        int32_t M, int32_t K, int32_t d, const BT* B, int64_t ldb,
                        const int32_t* gidx, const float* rscale, const float* cscale,
                        float* C, int64_t ldc, float beta, const sgcn_plan_t* plan,
                        const float* add, int64_t ldadd, int32_t add_rows, void* stream) {
    constexpr bool kB16 = !std::is_same<BT, float>::value;
    SGCN_REQUIRE(M >= 0 && K >= 0 && d >= 0, "spmm: negative size");
    if (M == 0 || d == 0) return SGCN_OK;
    SGCN_REQUIRE(rowptr && C && (B || K == 0), "spmm: null operand");
    SGCN_REQUIRE(ldb >= d && ldc >= d, "spmm: leading dimension smaller than d");
    if (kB16) {
        SGCN_REQUIRE(ldb % 8 == 0, "spmm: a bfloat16 operand needs ldb %% 8 == 0 (ldb %lld, d %d)", (long long)ldb, d);
        SGCN_REQUIRE(aligned16(B), "spmm: a bfloat16 operand needs a 16-byte aligned base");
    }
    hipStream_t st = (hipStream_t)stream;

    SpmmArgs a{};
    a.rowptr = rowptr; a.col = col; a.val = val;
    a.B = B; a.ldb = ldb; a.gidx = gidx; a.rscale = rscale; a.cscale = cscale;
    a.C = C; a.ldc = ldc; a.beta = beta; a.d = d;
    a.nseg = M;
    a.slabmajor = g_tune_slabmajor;
    if (add && add_rows > 0) {
        SGCN_REQUIRE(ldadd >= d && add_rows <= M, "spmm: bad addend");
        a.add = add; a.ldadd = ldadd; a.add_rows = add_rows;
    }
    if (plan) {
        a.ldw = seg_slot_pitch(d);
        if (const int rc = seg_plan_ok("spmm", plan, M, a.ldw)) return rc;
        a.seg = plan->dev_seg; a.nseg = plan->nseg; a.ws = plan->dev_ws;
    }
    const int vw = pick_vw(d, {kB16 ? nullptr : (const void*)B, C, plan ? plan->dev_ws : nullptr, a.add},
                           {ldb, ldc, a.add ? a.ldadd : ldc});
    a.nvec = (d + vw - 1) / vw;
    const SegGeom g = seg_geometry(a.nvec, a.nseg, g_tune_nv);
    const int U = g_tune_unroll > 0 ? g_tune_unroll : (g.NV >= 3 ? 4 : 8);
    a.nsegblk = g.nsegblk;
    SGCN_REQUIRE(g.nblocks < (1ll << 31), "spmm: grid too large");

    const dim3 grid((unsigned)g.nblocks), block(kBlock);
    const bool ok = (U == 2 || U == 4 || U == 8) && with_vw(vw, [&](auto VW) {
        return with_gnv(g.G, g.NV, [&](auto G, auto NV) {
            constexpr int kG = decltype(G)::value, kNV = decltype(NV)::value, kVW = decltype(VW)::value;
            if (U == 2) hipLaunchKernelGGL((spmm_seg_kernel<kG, kNV, kVW, 2, BT>), grid, block, 0, st, a);
            else if (U == 4) hipLaunchKernelGGL((spmm_seg_kernel<kG, kNV, kVW, 4, BT>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((spmm_seg_kernel<kG, kNV, kVW, 8, BT>), grid, block, 0, st, a);
        });
    });
    SGCN_REQUIRE(ok, "spmm: no kernel for G=%d NV=%d U=%d", g.G, g.NV, U);
    SGCN_HIP_TRY(hipGetLastError());

    if (plan && plan->nfix > 0) {
        const int64_t nfblk = seg_fix_blocks(a.nvec, plan->nfix);
        SGCN_REQUIRE(nfblk < (1ll << 31), "spmm: too many split rows");
        with_vw(vw, [&](auto VW) {
            hipLaunchKernelGGL((spmm_fix_kernel<decltype(VW)::value>), dim3((unsigned)nfblk), block, 0, st, a, plan->dev_fix, plan->nfix);
        });
        SGCN_HIP_TRY(hipGetLastError());
    }
    return SGCN_OK;
}

extern "C" int sgcn_spmm_csr_add_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                                     int32_t M, int32_t K, int32_t d, const float* B, int64_t ldb,
                                     const int32_t* gidx, const float* rscale, const float* cscale,
                                     float* C, int64_t ldc, float beta, const sgcn_plan_t* plan,
                                     const float* add, int64_t ldadd, int32_t add_rows, void* stream) {
    return spmm_csr_add<float>(rowptr, col, val, M, K, d, B, ldb, gidx, rscale, cscale, C, ldc, beta, plan,
                               add, ldadd, add_rows, stream);
}

extern "C" int sgcn_spmm_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                                 int32_t M, int32_t K, int32_t d, const float* B, int64_t ldb,
                                 const int32_t* gidx, const float* rscale, const float* cscale,
                                 float* C, int64_t ldc, float beta, const sgcn_plan_t* plan,
                                 void* stream) {
    return spmm_csr_add<float>(rowptr, col, val, M, K, d, B, ldb, gidx, rscale, cscale, C, ldc, beta, plan,
                               nullptr, 0, 0, stream);
}

/* mirrors sgcn_spmm_csr_add_f32 on a bfloat16 operand */
extern "C" int sgcn_spmm_csr_add_b16(const int32_t* rowptr, const int32_t* col, const float* val,
                                     int32_t M, int32_t K, int32_t d, const uint16_t* B, int64_t ldb,
                                     const int32_t* gidx, const float* rscale, const float* cscale,
                                     float* C, int64_t ldc, float beta, const sgcn_plan_t* plan,
                                     const float* add, int64_t ldadd, int32_t add_rows, void* stream) {
    return spmm_csr_add<uint16_t>(rowptr, col, val, M, K, d, B, ldb, gidx, rscale, cscale, C, ldc, beta, plan,
                                  add, ldadd, add_rows, stream);
}

/* mirrors sgcn_spmm_csr_f32 on a bfloat16 operand */
extern "C" int sgcn_spmm_csr_b16(const int32_t* rowptr, const int32_t* col, const float* val,
                                 int32_t M, int32_t K, int32_t d, const uint16_t* B, int64_t ldb,
                                 const int32_t* gidx, const float* rscale, const float* cscale,
                                 float* C, int64_t ldc, float beta, const sgcn_plan_t* plan,
                                 void* stream) {
    return spmm_csr_add<uint16_t>(rowptr, col, val, M, K, d, B, ldb, gidx, rscale, cscale, C, ldc, beta, plan,
                                  nullptr, 0, 0, stream);
}
