// bf16-multiply GEMM for the dense layers of a full-graph pass (--dense_dtype bf16), gfx950.
//
//   C[M x N] = op(A)[M x K] . op(B)[K x N] (+ C)        op = identity or transpose; (trans_a, trans_b) != (1, 1)
//
// A, B and C are fp32 IN MEMORY.  Every operand element is rounded to bfloat16 (nearest even, v_cvt_pk_bf16_f32) in
// registers, on its way from the global load to the LDS tile, so the LDS holds 2-byte elements and no bf16 copy of an
// activation ever reaches memory.  The multiply is v_mfma_f32_32x32x16_bf16 (16x the rate of the fp32 matrix-core op that
// sgcn_gemm.hip uses): a product of two bf16 values is exact in fp32, the accumulation is fp32.  At N = 233 k rows the
// three GEMMs of a dense layer are then expected to be bound by the fp32 tables they read, not by the matrix pipe.
//
//   NN (0, 0)  forward x . W            A rows are k-contiguous; W is [K x N] and is staged transposed
//   NT (0, 1)  input gradient g . W^T   both operands k-contiguous
//   TN (1, 0)  weight gradient x^T . g  both operands are stored k-major: both staged transposed; K is cut across
//                                       workgroups (split-K), partial tiles to a workspace, added in slice order
//
// Tile: 128 x 128 per workgroup of 4 wavefronts, each wavefront a 64 x 64 quadrant as 2 x 2 accumulators of 32 x 32;
// K-step 32 = two MFMAs per accumulator.  Both LDS tiles are [row or column][k] with k contiguous and a pitch of 40
// elements (80 bytes: the 16-byte fragment reads of 8 consecutive lanes fall into disjoint banks), double-buffered: the
// global loads of step s + 1 are issued (MbTile::fetch: loads only) before the MFMAs of step s and waited for, selected,
// rounded and written to the other buffer after them (MbTile::stage) -- one barrier per step.  In the aligned
// instantiations the assembly of the loop is 8 global_load_dwordx4, the ds_read_b128 / MFMA block, then the counted waits.
//
// Order of additions (all of it a function of the form, M, N, K, the tuning knob and nothing else): inside a slice the
// K-steps in ascending order into one accumulator, 16 k per MFMA; slices by mb16_reduce_kernel in slice order; the old C
// (accumulate) last.  No atomics.  Edges are handled by selection: an out-of-range row, column or k has its address
// clamped and its value replaced by 0 before the rounding, so padding that holds NaN never reaches a product.
// Subnormal fp32 inputs may be flushed to zero by the conversion, and subnormal products by the MFMA.
//
// sgcn_gemm_mb16_a16 (--feature_dtype bf16): A is a table that is bfloat16 IN MEMORY already (the resident feature table,
// rounded once at set-up); B and C stay fp32.  Forms NN and TN only -- the two that ever read the feature table.  The A tile
// loads half the bytes (8 per run of 4 where the fp32 tile loads 16) and, without a mask, its stored bits go to the LDS
// tile unconverted; with drop_a an element is widened exactly, multiplied by its factor in fp32 and rounded to nearest
// even -- the operations the fp32 tile performs on the widened value.  Everything else (B tile, MFMA block, split rule,
// order of additions, epilogue) is the same code, so on a table without subnormal values the result has the bits of
// sgcn_gemm_mb16_f32 on the widened table.  A subnormal bfloat16 element reaches the MFMA as it is stored here (no
// conversion touches it unless drop_a is on), where the fp32 entry's conversion may already have flushed it: both may end
// as zero in the product, but the two entries are not promised to agree on such a table.
#include "sgcn_dev.h"

namespace sgcn {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));

constexpr int kMbTM = 128, kMbTN = 128, kMbTK = 32;
constexpr int kMbPitch = kMbTK + 8;                  // LDS row pitch in elements (80 bytes)
constexpr int kMbSliceK = 2048;                      // least K per split-K slice when the knob gemm_mb16_slice_k is 0
constexpr int kMbTargetBlocks = 512;                 // split until the grid has about two workgroups per CU

struct Mb16Args {
    const void* A; int64_t lda;       // fp32, or bfloat16 bits (sgcn_gemm_mb16_a16); lda in elements either way
    const float* B; int64_t ldb;
    float* C; int64_t ldc;
    int32_t M, N, K;
    int32_t accumulate;
    int32_t kchunk;                  // blockIdx.z covers k in [z * kchunk, (z + 1) * kchunk)
    float* ws;                       // split-K: partial tiles go to ws[z][M][N]
    DropArgs drop_a, drop_c;
    int32_t vec_a, vec_b;            // 16-byte aligned rows (8-byte: a bfloat16 A), run lengths a multiple of 4: picks the
};                                   // instantiation that loads a run of 4 at once

// One operand tile of a K-step: 128 (x: rows of A / columns of B) by 32 (k), 16 elements per thread.
//   KMAJOR == false  the stored matrix is [X x K], k contiguous: the thread takes 4 consecutive k of rows x = (tid >> 3) + 32 q
//   KMAJOR == true   the stored matrix is [K x X], x contiguous: the thread takes a 4 (k) x 4 (x) block and transposes it
//   VEC              the host verified 16-byte aligned rows and run lengths that are a multiple of 4: a run of 4 is one
//                    float4, all in range or all out
// fetch() only ISSUES the loads of a step -- addresses clamped so that every one is addressable, nothing is looked at -- so
// that the eight float4 of a thread's step are in flight together and stay in flight across the MFMAs of the step before;
// stage() is where they are waited for: it selects 0 for what is out of range (an out-of-range row, column or k never
// reaches a product, whatever the padding holds), applies the dropout factor in fp32, rounds to bf16 and writes the
// [x][k] LDS tile.  Both are straight-line code: the load class is a template parameter, the mask one uniform branch.
// The stored element type T is float, or uint16_t for a table of bfloat16 bits (below).
template <bool KMAJOR, bool VEC>
struct MbMap {
    // is element e of load q inside the operand?  (VEC: e does not matter)
    __device__ __forceinline__ static bool inside(int q, int e, int x0, int X, int k0, int kend, int tid) {
        if (!KMAJOR) {
            const int x = x0 + (tid >> 3) + 32 * q, k = k0 + (tid & 7) * 4;
            return x < X && (VEC ? k + 3 : k + e) < kend;
        } else {
            const int k = k0 + (tid >> 5) * 4 + q, x = x0 + (tid & 31) * 4;
            return k < kend && (VEC ? x + 3 : x + e) < X;
        }
    }
};

template <bool KMAJOR, bool VEC, typename T = float>
struct MbTile : MbMap<KMAJOR, VEC> {
    using MbMap<KMAJOR, VEC>::inside;
    f32x4 r[4];

    __device__ __forceinline__ void fetch(const float* P, int64_t ld, int x0, int X, int k0, int kend, int tid) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            // the row (clamped: always addressable) and the first element of the run
            const int row = KMAJOR ? min(k0 + (tid >> 5) * 4 + q, kend - 1) : min(x0 + (tid >> 3) + 32 * q, X - 1);
            const int first = KMAJOR ? x0 + (tid & 31) * 4 : k0 + (tid & 7) * 4;
            const float* rowp = P + (int64_t)row * ld;
            if (VEC) {
                r[q] = *reinterpret_cast<const f32x4*>(rowp + (inside(q, 0, x0, X, k0, kend, tid) ? first : 0));
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++) r[q][e] = rowp[inside(q, e, x0, X, k0, kend, tid) ? first + e : 0];
            }
        }
    }

    __device__ __forceinline__ void stage(__bf16 (*S)[kMbPitch], int x0, int X, int k0, int kend, const DropArgs& drop, int tid) {
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int e = 0; e < 4; e++) r[q][e] = inside(q, e, x0, X, k0, kend, tid) ? r[q][e] : 0.f;
        if (drop.on) {                   // the stored element [row][col] of the masked activation
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int x = KMAJOR ? x0 + (tid & 31) * 4 + e : x0 + (tid >> 3) + 32 * q;
                    const int k = KMAJOR ? k0 + (tid >> 5) * 4 + q : k0 + (tid & 7) * 4 + e;
                    r[q][e] *= KMAJOR ? drop_factor(drop, k, x) : drop_factor(drop, x, k);
                }
        }
        if (!KMAJOR) {
            const int kq = (tid & 7) * 4;
#pragma unroll
            for (int q = 0; q < 4; q++)
                *reinterpret_cast<bf16x4*>(&S[(tid >> 3) + 32 * q][kq]) = __builtin_convertvector(r[q], bf16x4);
        } else {
            const int kb = (tid >> 5) * 4, xq = (tid & 31) * 4;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const f32x4 col = {r[0][e], r[1][e], r[2][e], r[3][e]};
                *reinterpret_cast<bf16x4*>(&S[xq + e][kb]) = __builtin_convertvector(col, bf16x4);
            }
        }
    }
};

// The same tile of a table stored as bfloat16: the same thread map, 2-byte elements.  VEC: the host verified 8-byte aligned
// rows and run lengths that are a multiple of 4 -- a run of 4 is one 8-byte load (global_load_dwordx2); otherwise 2-byte
// loads.  fetch() only issues loads, addresses clamped.  stage() selects 0 for what is out of range; without a mask the
// stored bits go to the LDS tile as they are (no conversion: the element IS the bfloat16 the fp32 tile would have made of
// its widened value); with a mask the element is widened exactly, multiplied by the factor in fp32 and rounded to nearest
// even, as the fp32 tile does.
template <bool KMAJOR, bool VEC>
struct MbTile<KMAJOR, VEC, uint16_t> : MbMap<KMAJOR, VEC> {
    using MbMap<KMAJOR, VEC>::inside;
    u16x4 r[4];

    __device__ __forceinline__ void fetch(const uint16_t* P, int64_t ld, int x0, int X, int k0, int kend, int tid) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int row = KMAJOR ? min(k0 + (tid >> 5) * 4 + q, kend - 1) : min(x0 + (tid >> 3) + 32 * q, X - 1);
            const int first = KMAJOR ? x0 + (tid & 31) * 4 : k0 + (tid & 7) * 4;
            const uint16_t* rowp = P + (int64_t)row * ld;
            if (VEC) {
                r[q] = *reinterpret_cast<const u16x4*>(rowp + (inside(q, 0, x0, X, k0, kend, tid) ? first : 0));
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++) r[q][e] = rowp[inside(q, e, x0, X, k0, kend, tid) ? first + e : 0];
            }
        }
    }

    __device__ __forceinline__ void stage(__bf16 (*S)[kMbPitch], int x0, int X, int k0, int kend, const DropArgs& drop, int tid) {
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int e = 0; e < 4; e++) r[q][e] = inside(q, e, x0, X, k0, kend, tid) ? r[q][e] : (uint16_t)0;
        if (drop.on) {                   // widen (exact), factor in fp32, round to nearest even
#pragma unroll
            for (int q = 0; q < 4; q++) {
                f32x4 w;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int x = KMAJOR ? x0 + (tid & 31) * 4 + e : x0 + (tid >> 3) + 32 * q;
                    const int k = KMAJOR ? k0 + (tid >> 5) * 4 + q : k0 + (tid & 7) * 4 + e;
                    w[e] = __uint_as_float((uint32_t)r[q][e] << 16) * (KMAJOR ? drop_factor(drop, k, x) : drop_factor(drop, x, k));
                }
                r[q] = __builtin_bit_cast(u16x4, __builtin_convertvector(w, bf16x4));
            }
        }
        if (!KMAJOR) {
            const int kq = (tid & 7) * 4;
#pragma unroll
            for (int q = 0; q < 4; q++) *reinterpret_cast<u16x4*>(&S[(tid >> 3) + 32 * q][kq]) = r[q];
        } else {
            const int kb = (tid >> 5) * 4, xq = (tid & 31) * 4;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const u16x4 col = {r[0][e], r[1][e], r[2][e], r[3][e]};
                *reinterpret_cast<u16x4*>(&S[xq + e][kb]) = col;
            }
        }
    }
};

// AT: the stored element type of A -- float, or uint16_t for bfloat16 bits (sgcn_gemm_mb16_a16: TB is false there)
template <bool TA, bool TB, bool VA, bool VB, typename AT = float>
__global__ __launch_bounds__(kBlock) void gemm_mb16_kernel(Mb16Args g) {
    // (static LDS only, declared 16-byte aligned: the fragment reads are 16-byte ds_read_b128)
    __shared__ __attribute__((aligned(16))) __bf16 As[2][kMbTM][kMbPitch];      // [i][kk]
    __shared__ __attribute__((aligned(16))) __bf16 Bs[2][kMbTN][kMbPitch];      // [j][kk]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = (int)blockIdx.x * kMbTM, n0 = (int)blockIdx.y * kMbTN;
    const int kbeg = (int)blockIdx.z * g.kchunk;
    const int kend = min(g.K, kbeg + g.kchunk);
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;       // the wavefront's quadrant
    f32x16 acc[2][2] = {};
    MbTile<TA, VA, AT> ta;          // A stored [K x M] when TA: k-major
    const AT* gA = static_cast<const AT*>(g.A);
    MbTile<!TB, VB> tb;             // B stored [K x N] unless TB: k-major
    const DropArgs nodrop{};

    const int iters = (kend - kbeg + kMbTK - 1) / kMbTK;
    if (iters > 0) {
        ta.fetch(gA, g.lda, m0, g.M, kbeg, kend, tid);
        tb.fetch(g.B, g.ldb, n0, g.N, kbeg, kend, tid);
        ta.stage(As[0], m0, g.M, kbeg, kend, g.drop_a, tid);
        tb.stage(Bs[0], n0, g.N, kbeg, kend, nodrop, tid);
    }
    __syncthreads();
    for (int it = 0; it < iters; it++) {
        const int cur = it & 1, knext = kbeg + (it + 1) * kMbTK;
        const bool more = it + 1 < iters;
        if (more) {                  // issued here, waited for in stage() behind the MFMAs
            ta.fetch(gA, g.lda, m0, g.M, knext, kend, tid);
            tb.fetch(g.B, g.ldb, n0, g.N, knext, kend, tid);
        }
        // lane l holds A[i = l & 31][k = 8 (l >> 5) + 0..7] and B[k = 8 (l >> 5) + 0..7][j = l & 31] of a 16-wide k-step
        const int fr = lane & 31, fk = (lane >> 5) * 8;
#pragma unroll
        for (int ks = 0; ks < kMbTK; ks += 16) {
            bf16x8 a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                a[t] = *reinterpret_cast<const bf16x8*>(&As[cur][wm + t * 32 + fr][ks + fk]);
                b[t] = *reinterpret_cast<const bf16x8*>(&Bs[cur][wn + t * 32 + fr][ks + fk]);
            }
#pragma unroll
            for (int tm = 0; tm < 2; tm++)
#pragma unroll
                for (int tn = 0; tn < 2; tn++)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[tm], b[tn], acc[tm][tn], 0, 0, 0);
        }
        if (more) {                  // the other buffer: its last readers passed the barrier of the step before
            ta.stage(As[cur ^ 1], m0, g.M, knext, kend, g.drop_a, tid);
            tb.stage(Bs[cur ^ 1], n0, g.N, knext, kend, nodrop, tid);
        }
        __syncthreads();
    }

    // C/D map of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    float* base = g.ws ? g.ws + (int64_t)blockIdx.z * g.M * g.N : g.C;
    const int64_t ld = g.ws ? g.N : g.ldc;
    const bool add = !g.ws && g.accumulate;
#pragma unroll
    for (int tm = 0; tm < 2; tm++) {
#pragma unroll
        for (int tn = 0; tn < 2; tn++) {
            const int col = n0 + wn + tn * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = m0 + wm + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row < g.M && col < g.N) {
                    float* p = base + (int64_t)row * ld + col;
                    float v = acc[tm][tn][r];
                    if (g.drop_c.on) v *= drop_factor(g.drop_c, row, col);
                    *p = add ? *p + v : v;
                }
            }
        }
    }
}

// C (+)= sum_z ws[z]   in z order; one workgroup row per output row (no division), 256 columns per workgroup
__global__ void mb16_reduce_kernel(const float* __restrict__ ws, int32_t S, int32_t M, int32_t N,
                                   float* __restrict__ C, int64_t ldc, int32_t accumulate) {
    const int col = (int)blockIdx.x * (int)blockDim.x + (int)threadIdx.x, row = (int)blockIdx.y;
    if (col >= N) return;
    const int64_t mn = (int64_t)M * N;
    const float* w = ws + (int64_t)row * N + col;
    float s = 0.f;
    for (int z = 0; z < S; z++) s += w[(int64_t)z * mn];
    float* p = C + (int64_t)row * ldc + col;
    *p = accumulate ? *p + s : s;
}

// Split-K factor: the K range is cut until the grid has about kMbTargetBlocks workgroups, every slice keeping at least
// gemm_mb16_slice_k of K (default 2048: the weight gradient of the 233 k-row graph, ten output tiles, gets 51 slices of
// 4.6 k rows; a 256 x 128 one 113 slices, whose partial tiles are 4 % of the operand bytes).  The forward and the input
// gradient at that size have thousands of tiles and are never split.
int mb16_split_factor(int M, int N, int K) {
    const int tiles = ((M + kMbTM - 1) / kMbTM) * ((N + kMbTN - 1) / kMbTN);
    const int slice_k = tune_get("gemm_mb16_slice_k") > 0 ? tune_get("gemm_mb16_slice_k") : kMbSliceK;
    const int s = std::min(kMbTargetBlocks / std::max(tiles, 1), K / slice_k);
    return std::max(s, 1);
}

template <bool TA, bool TB>
void mb16_launch(const Mb16Args& g, dim3 grid, hipStream_t st) {
    if (g.vec_a && g.vec_b) hipLaunchKernelGGL((gemm_mb16_kernel<TA, TB, true, true>), grid, dim3(kBlock), 0, st, g);
    else if (g.vec_a) hipLaunchKernelGGL((gemm_mb16_kernel<TA, TB, true, false>), grid, dim3(kBlock), 0, st, g);
    else if (g.vec_b) hipLaunchKernelGGL((gemm_mb16_kernel<TA, TB, false, true>), grid, dim3(kBlock), 0, st, g);
    else hipLaunchKernelGGL((gemm_mb16_kernel<TA, TB, false, false>), grid, dim3(kBlock), 0, st, g);
}

template <bool TA>
void mb16_launch_a16(const Mb16Args& g, dim3 grid, hipStream_t st) {
    if (g.vec_a && g.vec_b) hipLaunchKernelGGL((gemm_mb16_kernel<TA, false, true, true, uint16_t>), grid, dim3(kBlock), 0, st, g);
    else if (g.vec_a) hipLaunchKernelGGL((gemm_mb16_kernel<TA, false, true, false, uint16_t>), grid, dim3(kBlock), 0, st, g);
    else if (g.vec_b) hipLaunchKernelGGL((gemm_mb16_kernel<TA, false, false, true, uint16_t>), grid, dim3(kBlock), 0, st, g);
    else hipLaunchKernelGGL((gemm_mb16_kernel<TA, false, false, false, uint16_t>), grid, dim3(kBlock), 0, st, g);
}

// The one host path of both entries; a16: A holds bfloat16 bits
int mb16_run(bool a16, int32_t trans_a, int32_t trans_b, int32_t M, int32_t N, int32_t K, const void* A, int64_t lda,
             const float* B, int64_t ldb, float* C, int64_t ldc, int32_t accumulate, float* ws,
             const sgcn_dropout_t* drop_a, const sgcn_dropout_t* drop_c, void* stream) {
    SGCN_REQUIRE(!(trans_a && trans_b), "gemm_mb16: the (trans_a, trans_b) = (1, 1) form is not provided");
    SGCN_REQUIRE(!(a16 && trans_b), "gemm_mb16_a16: the NT form (trans_b) is not provided for a bfloat16 A: the feature "
                                    "table is only ever read by the forward and the weight-gradient products");
    SGCN_REQUIRE(M >= 0 && N >= 0 && K >= 0, "gemm_mb16: negative size");
    if (M == 0 || N == 0) return SGCN_OK;
    // (K = 0: C = 0 or C unchanged, and the operands are never read -- an empty tensor has no address)
    SGCN_REQUIRE(C && (K == 0 || (A && B)), "gemm_mb16: null operand");
    SGCN_REQUIRE(!a16 || K == 0 || (uintptr_t)A % 2 == 0, "gemm_mb16_a16: A must be 2-byte aligned");
    Mb16Args g{};
    g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc;
    g.M = M; g.N = N; g.K = K; g.accumulate = accumulate;
    g.drop_a = drop_args(drop_a);
    g.drop_c = drop_args(drop_c);
    SGCN_REQUIRE(!g.drop_a.on || g.drop_a.width == (trans_a ? M : K), "gemm_mb16: drop_a width must be the stored A's row length");
    SGCN_REQUIRE(!g.drop_c.on || g.drop_c.width == N, "gemm_mb16: drop_c width must be N");
    if (g.drop_c.on) ws = nullptr;           // the output mask is applied in the GEMM's own epilogue
    // (a run of 4 elements is one load: 16 bytes of fp32, 8 bytes of bfloat16)
    auto al = [](const void* p, int64_t ld, int bytes) { return p && ((uintptr_t)p % bytes == 0) && (ld % 4 == 0); };
    // (a run of 4 must be all in range or all out: the run it lies in is a multiple of 4 long -- MbMap::inside)
    g.vec_a = al(A, lda, a16 ? 8 : 16) && (trans_a ? M : K) % 4 == 0;
    g.vec_b = al(B, ldb, 16) && (trans_b ? K : N) % 4 == 0;
    int S = ws ? mb16_split_factor(M, N, K) : 1;
    g.kchunk = ((K + S - 1) / S + kMbTK - 1) / kMbTK * kMbTK;
    S = K > 0 ? (K + g.kchunk - 1) / g.kchunk : 1;
    if (K == 0) g.kchunk = kMbTK;
    g.ws = S > 1 ? ws : nullptr;
    const dim3 grid((unsigned)((M + kMbTM - 1) / kMbTM), (unsigned)((N + kMbTN - 1) / kMbTN), (unsigned)S);
    hipStream_t st = (hipStream_t)stream;
    if (a16) {
        if (trans_a) mb16_launch_a16<true>(g, grid, st);
        else mb16_launch_a16<false>(g, grid, st);
    } else if (!trans_a && !trans_b) mb16_launch<false, false>(g, grid, st);
    else if (trans_a) mb16_launch<true, false>(g, grid, st);
    else mb16_launch<false, true>(g, grid, st);
    if (S > 1) {
        // (a split call has at most kMbTargetBlocks / 2 tiles, so M <= 32,768: within the grid's y range)
        hipLaunchKernelGGL(mb16_reduce_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)M), dim3(256), 0, st,
                           g.ws, S, M, N, C, ldc, accumulate);
    }
    SGCN_HIP_TRY(hipGetLastError());
    return SGCN_OK;
}

}  // namespace
}  // namespace sgcn

using namespace sgcn;

extern "C" int64_t sgcn_gemm_mb16_ws_floats(int32_t trans_a, int32_t trans_b, int32_t M, int32_t N, int32_t K) {
    (void)trans_a; (void)trans_b;            // the split rule is the same for the three forms
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const int S = mb16_split_factor(M, N, K);
    return S > 1 ? (int64_t)S * M * N : 0;
}

extern "C" int sgcn_gemm_mb16_f32(int32_t trans_a, int32_t trans_b, int32_t M, int32_t N, int32_t K,
                                  const float* A, int64_t lda, const float* B, int64_t ldb, float* C,
                                  int64_t ldc, int32_t accumulate, float* ws,
                                  const sgcn_dropout_t* drop_a, const sgcn_dropout_t* drop_c, void* stream) {
    return mb16_run(false, trans_a, trans_b, M, N, K, A, lda, B, ldb, C, ldc, accumulate, ws, drop_a, drop_c, stream);
}

extern "C" int sgcn_gemm_mb16_a16(int32_t trans_a, int32_t trans_b, int32_t M, int32_t N, int32_t K,
                                  const uint16_t* A, int64_t lda, const float* B, int64_t ldb, float* C,
                                  int64_t ldc, int32_t accumulate, float* ws,
                                  const sgcn_dropout_t* drop_a, const sgcn_dropout_t* drop_c, void* stream) {
    return mb16_run(true, trans_a, trans_b, M, N, K, A, lda, B, ldb, C, ldc, accumulate, ws, drop_a, drop_c, stream);
}
