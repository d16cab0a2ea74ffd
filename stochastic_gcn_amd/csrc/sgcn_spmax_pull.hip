// Two-table element-wise neighbour maximum for gfx950 (MI355X): the maximum of a part step that keeps its out-of-part entries
// (--full_batch_part_pull_max):
//
//   B_e     = map[col[e]] >= 0 ? X[map[col[e]], :] : H[col[e], :]        e in [rowptr[ids[i]], rowptr[ids[i] + 1]), stored order
//   C[i, c] = the FIRST maximum of B_e[c] over those e                       i = 0 .. n-1
//   arg[i, c] = its winner:  >= 0  fresh, the winner's POSITION in ids (the row of X, the column of the block A[S, S])
//                            == -1 the row stores nothing (C = +0.0)
//                            <= -2 stale, global column -2 - arg
//
// Setting and operands are those of sgcn_spmm_pull.hip: the CSR is the RESIDENT N x N adjacency (its values are not read),
// read in place through `ids` (the step's vertex set S, ascending and unique); `map` is what sgcn_induce_map_i32 wrote for
// `ids`; X (n x d, fp32) holds the rows the step computes, H (N x d, fp32 or bfloat16) the last-seen rows of every vertex,
// read for columns outside S only.  The tie rule is sgcn_spmax.hip's: the best starts as the first entry, a later entry
// replaces it only when v > best -- the first of +0.0 / -0.0 and of equal values wins WHICHEVER TABLE it comes from; +-inf are
// ordinary values; NaN-free input is the caller's promise.  No arithmetic: C holds bits of X or of the (exactly widened) H,
// the bits sgcn_spmax_csr_f32 without a plan gives on the rows `ids` of the matrix and the merged table (H with the rows
// ids replaced by X), and arg decodes to its arg (tests/test_spmax_pull_gpu.py).
//
// The encoding of arg is made for the EXISTING backward: sgcn_spmax_csr_bwd_f32 over the transposed 'keep' block A[S, S]^T
// adds G[i, c] to row j where arg[i, c] == j, j a position in S.  A fresh winner is recorded by exactly that position; a
// stale winner is a constant of the step and gets nothing, and no negative word ever matches a row.  (The broadcast source
// word ~col is not what is stored: ~0 is -1, the empty row's mark.  Stored is ~col - 1.)
//
// Shape: spmax_seg_kernel's body (sgcn_spmax.hip: G lanes per row, NV vectors per lane, U entries' loads in flight before the
// first compare, feature slabs, the ladders of sgcn_seg.h) with spmm_pull_kernel's entry handling (sgcn_spmm_pull.hip,
// sgcn_pull_dev.h): the lane that fetches an entry's column id also fetches map[col] and folds both into ONE source word,
// m >= 0 ? m : ~col, broadcast once per entry (v_readlane at G = 64, so table, pitch, row base and the id to record are
// scalar; ds_bpermute below); the address is formed behind the broadcast.  The U * NV loads of a chunk stay in one raw
// register image, pinned between the requests and the compares in the bfloat16 form (hpin's reason: sgcn_dev.h).
//   * ONE GROUP OWNS ONE SELECTED ROW, whatever its length: no host plan, no split rows, no workspace -- the known limit of
//     the other pull launches (sgcn_spmm_pull.hip's header).  A launch runs as long as its longest selected row; split rows
//     are the first follow-up, a branch-free bfloat16 load the second.
//   * the vector width is the widest that X, H (its pointer left out for a bfloat16 table), C, arg and their four pitches
//     allow.
//   * no atomics: one group walks a row in stored order -- the same bits on every run.
#include "sgcn_dev.h"
#include "sgcn_max_dev.h"
#include "sgcn_pull_dev.h"
#include "sgcn_seg.h"

namespace sgcn {
namespace {

struct MaxPullArgs {
    const int32_t* rowptr;
    const int32_t* col;
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
    int32_t* arg;            // nullable (evaluation)
    int64_t ldarg;
    int32_t d;
    int32_t nvec;            // ceil(d / VW)
    int32_t slabmajor;
};

// what arg records for the source word s: the position in ids of a fresh winner, -2 - col = ~col - 1 of a stale one
__device__ __forceinline__ int pull_arg(int s) { return s >= 0 ? s : s - 1; }

template <int G, int NV, int VW, int U, class HT>
__global__ __launch_bounds__(kBlock) void spmax_pull_kernel(MaxPullArgs a) {
    typedef typename Vec<VW>::type VT;
    typedef typename IVec<VW>::type IT;
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
    VT best[NV];
    IT barg[NV];
    // Lanes past the row width re-read the last valid vector (their results are never stored), as in the row kernel.
    uint32_t xoff[NV];                 // byte offset inside an fp32 row; half of it inside a bfloat16 row
#pragma unroll
    for (int k = 0; k < NV; k++) {
        const int vi = vbase + k * G;
        act[k] = vi < a.nvec;
        xoff[k] = (uint32_t)min(vi, a.nvec - 1) * (uint32_t)(VW * sizeof(float));
    }
    const char* Xb = reinterpret_cast<const char*>(a.X);
    const char* Hb = reinterpret_cast<const char*>(a.H);
    const int64_t ldx_bytes = a.ldx * (int64_t)sizeof(float);
    const int64_t ldh_bytes = a.ldh * (int64_t)sizeof(HT);

    // the best starts as the row's first entry ...
    if (start < end) {
        const int c0 = uniform_i<G>(a.col[start]);
        const int m0 = uniform_i<G>(a.map[c0]);
        const int s0 = m0 >= 0 ? m0 : ~c0;
        const bool stale = s0 < 0;
        const char* src = stale ? Hb + (int64_t)(~s0) * ldh_bytes : Xb + (int64_t)s0 * ldx_bytes;
#pragma unroll
        for (int k = 0; k < NV; k++) {
            best[k] = pull_value<VW, HT>(pull_load<VW, HT>(src, xoff[k], stale), stale);
            barg[k] = isplat<VW>(pull_arg(s0));
        }
    } else {
#pragma unroll
        for (int k = 0; k < NV; k++) { best[k] = vzero<VW>(); barg[k] = isplat<VW>(-1); }
    }
    // ... and every later one is held against it, in stored order
    for (int p0 = start + 1; p0 < end; p0 += G) {
        const int n = min(G, end - p0);
        int mysrc = 0;                 // m >= 0: row m of X; < 0: row ~mysrc of H
        if (lig < n) {
            const int c = a.col[p0 + lig];
            const int m = a.map[c];
            mysrc = m >= 0 ? m : ~c;
        }
        int j = 0;
        for (; j + U <= n; j += U) {
            RT b[U][NV];
            int s[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                s[u] = bcast_i<G>(mysrc, j + u);
                const bool stale = s[u] < 0;
                const char* src = stale ? Hb + (int64_t)(~s[u]) * ldh_bytes : Xb + (int64_t)s[u] * ldx_bytes;   // G == 64: scalar
#pragma unroll
                for (int k = 0; k < NV; k++) b[u][k] = pull_load<VW, HT>(src, xoff[k], stale);
            }
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int k = 0; k < NV; k++) {
                    hpin<HT, VW>(b[u][k]);
                    max_take<VW>(best[k], barg[k], pull_value<VW, HT>(b[u][k], s[u] < 0), pull_arg(s[u]));
                }
        }
        for (; j < n; j++) {
            const int s = bcast_i<G>(mysrc, j);
            const bool stale = s < 0;
            const char* src = stale ? Hb + (int64_t)(~s) * ldh_bytes : Xb + (int64_t)s * ldx_bytes;
#pragma unroll
            for (int k = 0; k < NV; k++)
                max_take<VW>(best[k], barg[k], pull_value<VW, HT>(pull_load<VW, HT>(src, xoff[k], stale), stale), pull_arg(s));
        }
    }

#pragma unroll
    for (int k = 0; k < NV; k++)
        if (act[k]) {
            const int vi = vbase + k * G, left = a.d - vi * VW;   // > 0 by construction
            vstore_n<VW>(a.C + i * a.ldc + (int64_t)vi * VW, best[k], left);
            if (a.arg) istore_n<VW>(a.arg + i * a.ldarg + (int64_t)vi * VW, barg[k], left);
        }
}

}  // namespace

// HT = float: sgcn_spmax_pull_f32.  HT = uint16_t: sgcn_spmax_pull_h16 -- the table's pointer is left out of pick_vw (its
// layout never limits the vector width), its pitch is not, as in spmm_pull: VW, G, NV and U are what the f32 call picks for a
// 16-byte aligned fp32 table of the same element pitch, and every row is walked in that call's order.
template <class HT>
static int spmax_pull(const int32_t* rowptr, const int32_t* col, const int32_t* ids, int32_t n, int32_t N, const int32_t* map,
                      int32_t d, const float* X, int64_t ldx, const HT* H, int64_t ldh, float* C, int64_t ldc, int32_t* arg,
                      int64_t ldarg, void* stream) {
    constexpr bool kH16 = !std::is_same<HT, float>::value;
    SGCN_REQUIRE(n >= 0 && N >= 0, "spmax_pull: negative size");
    SGCN_REQUIRE(n <= N, "spmax_pull: %d rows cannot be unique in [0, %d)", n, N);
    SGCN_REQUIRE(d > 0, "spmax_pull: d must be positive, got %d", d);
    SGCN_REQUIRE(ldx >= d && ldh >= d && ldc >= d && (!arg || ldarg >= d), "spmax_pull: leading dimension smaller than d");
    if (n == 0) return SGCN_OK;
    SGCN_REQUIRE(rowptr && col && ids && map && X && H && C, "spmax_pull: null operand");
    if constexpr (kH16) {
        if (const int rc = h16_table_ok("spmax_pull", H, ldh, d)) return rc;
    }
    hipStream_t st = (hipStream_t)stream;

    MaxPullArgs a{};
    a.rowptr = rowptr; a.col = col; a.ids = ids; a.map = map; a.n = n;
    a.X = X; a.ldx = ldx; a.H = H; a.ldh = ldh; a.C = C; a.ldc = ldc; a.arg = arg; a.ldarg = ldarg; a.d = d;
    a.slabmajor = tune_get("spmm_slabmajor");
    const int vw = pick_vw(d, {X, kH16 ? nullptr : (const void*)H, C, arg}, {ldx, ldh, ldc, arg ? ldarg : ldc});
    a.nvec = (d + vw - 1) / vw;
    const SegGeom g = seg_geometry(a.nvec, n);
    a.nsegblk = g.nsegblk;
    SGCN_REQUIRE(g.nblocks < (1ll << 31), "spmax_pull: grid too large");

    const dim3 grid((unsigned)g.nblocks), block(kBlock);
    const bool ok = with_vw(vw, [&](auto VW) {
        return with_gnv(g.G, g.NV, [&](auto G, auto NV) {
            constexpr int kG = decltype(G)::value, kNV = decltype(NV)::value, kVW = decltype(VW)::value;
            constexpr int kU = kNV >= 3 ? 4 : 8;           // spmax_seg_kernel's forward unroll
            hipLaunchKernelGGL((spmax_pull_kernel<kG, kNV, kVW, kU, HT>), grid, block, 0, st, a);
        });
    });
    SGCN_REQUIRE(ok, "spmax_pull: no kernel for G=%d NV=%d", g.G, g.NV);
    SGCN_HIP_TRY(hipGetLastError());
    return SGCN_OK;
}

}  // namespace sgcn

using namespace sgcn;

extern "C" int sgcn_spmax_pull_f32(const int32_t* rowptr, const int32_t* col, const int32_t* ids, int32_t n, int32_t N,
                                   const int32_t* map, int32_t d, const float* X, int64_t ldx, const float* H, int64_t ldh,
                                   float* C, int64_t ldc, int32_t* arg, int64_t ldarg, void* stream) {
    return spmax_pull<float>(rowptr, col, ids, n, N, map, d, X, ldx, H, ldh, C, ldc, arg, ldarg, stream);
}

/* mirrors sgcn_spmax_pull_f32 on a bfloat16 history */
extern "C" int sgcn_spmax_pull_h16(const int32_t* rowptr, const int32_t* col, const int32_t* ids, int32_t n, int32_t N,
                                   const int32_t* map, int32_t d, const float* X, int64_t ldx, const uint16_t* H, int64_t ldh,
                                   float* C, int64_t ldc, int32_t* arg, int64_t ldarg, void* stream) {
    return spmax_pull<uint16_t>(rowptr, col, ids, n, N, map, d, X, ldx, H, ldh, C, ldc, arg, ldarg, stream);
}
