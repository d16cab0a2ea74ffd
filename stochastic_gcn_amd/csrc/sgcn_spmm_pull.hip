// Two-table gather SpMM for gfx950 (MI355X): the neighbour sum of a part step that keeps its out-of-part entries
// (--full_batch_part_history; GNNAutoScale / Cluster-GCN with historical embeddings):
//
//   C[i, :] = sum over e in [rowptr[ids[i]], rowptr[ids[i] + 1]) of
//             val[e] * ( map[col[e]] >= 0 ? X[map[col[e]], :] : H[col[e], :] )            i = 0 .. n-1
//
// The CSR is the RESIDENT N x N adjacency, read in place through `ids` (the step's vertex set S, ascending and unique); `map`
// is what sgcn_induce_map_i32 wrote for `ids`.  X (n x d, fp32) holds the rows the step computes -- the FRESH operand, never
// rounded, the very rows the backward differentiates; H (N x d, fp32 or bfloat16) the last-seen rows of every vertex -- the
// STALE operand, read for columns outside S only.  A row of X is read only where map says the column is in S, and rows of H
// inside S are never read.
//
// Shape: the lane geometry of spmm_seg_kernel (sgcn_spmm.hip) -- G lanes per row, NV vectors per lane, U entries in flight,
// feature slabs for wide rows, the ladders of sgcn_seg.h.  What differs:
//   * ONE GROUP OWNS ONE SELECTED ROW, whatever its length: there is no host plan and there are no split rows in this
//     version (a plan would need the rows' lengths on the host and a workspace; the step's forward has neither a cut nor a
//     synchronisation of its own).  A launch runs as long as its longest selected row -- measured on S-Reddit (rows of up to
//     9,243 entries against a mean of 65): 0.1 us per entry of that row, which makes the launch slower than slice + plan +
//     row kernel there; split rows are the first follow-up.
//   * the lane that fetches an entry's column id also fetches map[col] -- one more dependent load in front of the gather,
//     N words, L2-resident -- and folds table and row into ONE word, the source: m >= 0 ? m : ~col.  All G lanes of a chunk
//     issue that load before the first broadcast.  The word is broadcast with the value (v_readlane at G = 64, so table,
//     pitch and row base are scalar; ds_bpermute below), the address formed behind the broadcast: one word moved per entry
//     instead of an address's two and a table flag.
//   * the two tables have their own pitches; the vector width is the widest that X, H, C and the three pitches allow.
//   * no atomics, no workspace: a row's sum is taken in stored order by one group -- the same bits on every run.
//
// HT: the history's element -- float, or uint16_t for a bfloat16 table (the layout of ops.history_alloc(..., bf16=True)),
// widened exactly (bits << 16) in front of the multiply-add.  Both instantiations keep the U * NV loads in one raw register
// image (a bfloat16 row fills its lower half), pinned between the requests and the updates (hpin's reason: sgcn_dev.h), and
// BOTH spell the update out as one fused multiply-add per element (vfma).  The row kernel leaves its fp32 form to the
// compiler's contraction, which is why its scalar lanes (VW == 1) need an exception: there the compiler contracts only some
// of the U products.  Here a select sits in front of every product in either form, so nothing is left to contraction: the
// h16 form gives the bits of the f32 form on the widened table by construction, VW == 1 included
// (tests/test_spmm_pull_gpu.py compares them at d = 1 and 3).  Measured: the h16 form takes 2.3 x the f32 form's time on
// S-Reddit at d = 128 -- supposedly the per-entry branch between the two load widths inside the U-deep request loop, which
// the f32 form does not have; a branch-free h16 form is the second follow-up.
#include "sgcn_dev.h"
#include "sgcn_pull_dev.h"
#include "sgcn_seg.h"

namespace sgcn {
namespace {

struct PullArgs {
    const int32_t* rowptr;
    const int32_t* col;
    const float* val;
    const int32_t* ids;
    const int32_t* map;
    int64_t n;               // selected rows
    int64_t nsegblk;         // blocks per slab
    const float* X;
    int64_t ldx;             // in floats
    const void* H;           // fp32, or uint16 for a bfloat16 table: the kernel's HT says which
    int64_t ldh;             // in elements of H
    float* C;
    int64_t ldc;
    int32_t d;
    int32_t nvec;            // ceil(d / VW)
    int32_t slabmajor;
};

template <int G, int NV, int VW, int U, class HT>
__global__ __launch_bounds__(kBlock) void spmm_pull_kernel(PullArgs a) {
    typedef typename Vec<VW>::type VT;
    typedef typename PullRaw<VW>::type RT;
    constexpr int GPB = kBlock / G;
    const int lig = threadIdx.x & (G - 1);
    const int gib = threadIdx.x / G;

    int slab;
    int64_t sblk;
    if (a.slabmajor) { slab = (int)(blockIdx.x / a.nsegblk); sblk = blockIdx.x % a.nsegblk; }
    else { const int nslab = (int)(gridDim.x / a.nsegblk); slab = blockIdx.x % nslab; sblk = blockIdx.x / nslab; }
    const int64_t i = sblk * GPB + gib;
    if (i >= a.n) return;

    const int row = uniform_i<G>(a.ids[i]);
    const int start = uniform_i<G>(a.rowptr[row]);
    const int end = uniform_i<G>(a.rowptr[row + 1]);

    const int vbase = slab * (G * NV) + lig;
    bool act[NV];
    VT acc[NV];
    // Lanes past the row width re-read the last valid vector (their accumulators are never stored), as in the row kernel.
    uint32_t xoff[NV];                 // byte offset inside an fp32 row; half of it inside a bfloat16 row
#pragma unroll
    for (int k = 0; k < NV; k++) {
        const int vi = vbase + k * G;
        act[k] = vi < a.nvec;
        acc[k] = vzero<VW>();
        xoff[k] = (uint32_t)min(vi, a.nvec - 1) * (uint32_t)(VW * sizeof(float));
    }
    const char* Xb = reinterpret_cast<const char*>(a.X);
    const char* Hb = reinterpret_cast<const char*>(a.H);
    const int64_t ldx_bytes = a.ldx * (int64_t)sizeof(float);
    const int64_t ldh_bytes = a.ldh * (int64_t)sizeof(HT);

    for (int p0 = start; p0 < end; p0 += G) {
        const int n = min(G, end - p0);
        int mysrc = 0;                 // m >= 0: row m of X; < 0: row ~mysrc of H
        float myval = 0.f;
        if (lig < n) {
            const int c = a.col[p0 + lig];
            myval = a.val[p0 + lig];
            const int m = a.map[c];
            mysrc = m >= 0 ? m : ~c;
        }
        int j = 0;
        for (; j + U <= n; j += U) {
            RT b[U][NV];
            float v[U];
            bool stale[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int s = bcast_i<G>(mysrc, j + u);
                v[u] = bcast_f<G>(myval, j + u);
                stale[u] = s < 0;
                const char* src = stale[u] ? Hb + (int64_t)(~s) * ldh_bytes : Xb + (int64_t)s * ldx_bytes;   // G == 64: scalar
#pragma unroll
                for (int k = 0; k < NV; k++) b[u][k] = pull_load<VW, HT>(src, xoff[k], stale[u]);
            }
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int k = 0; k < NV; k++) {
                    if constexpr (!std::is_same<HT, float>::value && VW > 1) asm volatile("" : "+v"(b[u][k]));
                    acc[k] = vfma<VW>(v[u], pull_value<VW, HT>(b[u][k], stale[u]), acc[k]);
                }
        }
        for (; j < n; j++) {
            const int s = bcast_i<G>(mysrc, j);
            const float v = bcast_f<G>(myval, j);
            const bool stale = s < 0;
            const char* src = stale ? Hb + (int64_t)(~s) * ldh_bytes : Xb + (int64_t)s * ldx_bytes;
#pragma unroll
            for (int k = 0; k < NV; k++)
                acc[k] = vfma<VW>(v, pull_value<VW, HT>(pull_load<VW, HT>(src, xoff[k], stale), stale), acc[k]);
        }
    }

#pragma unroll
    for (int k = 0; k < NV; k++)
        if (act[k]) {
            const int vi = vbase + k * G;
            float* out = a.C + i * a.ldc + (int64_t)vi * VW;
            const int left = a.d - vi * VW;   // > 0 by construction
            if (left >= VW) vstore<VW>(out, acc[k]);
            else vstore_head<VW>(out, acc[k], left);
        }
}

}  // namespace

// HT = float: sgcn_spmm_pull_f32.  HT = uint16_t: sgcn_spmm_pull_h16 -- the table's pointer is left out of pick_vw (its
// layout never limits the vector width), its pitch is not: VW, G, NV and U are what the f32 call picks for a 16-byte aligned
// fp32 table of the same element pitch, and every sum is taken in that call's order.
template <class HT>
static int spmm_pull(const int32_t* rowptr, const int32_t* col, const float* val, const int32_t* ids, int32_t n, int32_t N,
                     const int32_t* map, int32_t d, const float* X, int64_t ldx, const HT* H, int64_t ldh, float* C,
                     int64_t ldc, void* stream) {
    constexpr bool kH16 = !std::is_same<HT, float>::value;
    SGCN_REQUIRE(n >= 0 && N >= 0, "spmm_pull: negative size");
    SGCN_REQUIRE(n <= N, "spmm_pull: %d rows cannot be unique in [0, %d)", n, N);
    SGCN_REQUIRE(d > 0, "spmm_pull: d must be positive, got %d", d);
    SGCN_REQUIRE(ldx >= d && ldh >= d && ldc >= d, "spmm_pull: leading dimension smaller than d");
    if (n == 0) return SGCN_OK;
    SGCN_REQUIRE(rowptr && col && val && ids && map && X && H && C, "spmm_pull: null operand");
    if constexpr (kH16) {
        if (const int rc = h16_table_ok("spmm_pull", H, ldh, d)) return rc;
    }
    hipStream_t st = (hipStream_t)stream;

    PullArgs a{};
    a.rowptr = rowptr; a.col = col; a.val = val; a.ids = ids; a.map = map; a.n = n;
    a.X = X; a.ldx = ldx; a.H = H; a.ldh = ldh; a.C = C; a.ldc = ldc; a.d = d;
    a.slabmajor = tune_get("spmm_slabmajor");
    const int vw = pick_vw(d, {X, kH16 ? nullptr : (const void*)H, C}, {ldx, ldh, ldc});
    a.nvec = (d + vw - 1) / vw;
    const SegGeom g = seg_geometry(a.nvec, n);
    a.nsegblk = g.nsegblk;
    SGCN_REQUIRE(g.nblocks < (1ll << 31), "spmm_pull: grid too large");

    const dim3 grid((unsigned)g.nblocks), block(kBlock);
    const bool ok = with_vw(vw, [&](auto VW) {
        return with_gnv(g.G, g.NV, [&](auto G, auto NV) {
            constexpr int kG = decltype(G)::value, kNV = decltype(NV)::value, kVW = decltype(VW)::value;
            constexpr int kU = kNV >= 3 ? 4 : 8;           // the row kernel's default unroll
            hipLaunchKernelGGL((spmm_pull_kernel<kG, kNV, kVW, kU, HT>), grid, block, 0, st, a);
        });
    });
    SGCN_REQUIRE(ok, "spmm_pull: no kernel for G=%d NV=%d", g.G, g.NV);
    SGCN_HIP_TRY(hipGetLastError());
    return SGCN_OK;
}

}  // namespace sgcn

using namespace sgcn;

extern "C" int sgcn_spmm_pull_f32(const int32_t* rowptr, const int32_t* col, const float* val, const int32_t* ids, int32_t n,
                                  int32_t N, const int32_t* map, int32_t d, const float* X, int64_t ldx, const float* H,
                                  int64_t ldh, float* C, int64_t ldc, void* stream) {
    return spmm_pull<float>(rowptr, col, val, ids, n, N, map, d, X, ldx, H, ldh, C, ldc, stream);
}

/* mirrors sgcn_spmm_pull_f32 on a bfloat16 history */
extern "C" int sgcn_spmm_pull_h16(const int32_t* rowptr, const int32_t* col, const float* val, const int32_t* ids, int32_t n,
                                  int32_t N, const int32_t* map, int32_t d, const float* X, int64_t ldx, const uint16_t* H,
                                  int64_t ldh, float* C, int64_t ldc, void* stream) {
    return spmm_pull<uint16_t>(rowptr, col, val, ids, n, N, map, d, X, ldx, H, ldh, C, ldc, stream);
}
