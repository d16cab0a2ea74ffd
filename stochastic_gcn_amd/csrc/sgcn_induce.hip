// The induced subgraph A[S, S] of a resident CSR, cut on the device (gfx950): the column-filtered, relabelled row slice a
// Cluster-GCN step (--full_batch_parts) runs on.  S is n vertex ids, ascending and unique (the host checks it).
//   map    : map[v] = position of v in S, -1 elsewhere -- 4 bytes per vertex, read once per stored entry, L2-resident
//   count  : per selected row the number of stored entries whose column is in S and, with values, the fp32 sums of the
//            row's values over all entries and over the kept ones; then the exclusive scan into o_rowptr (one workgroup)
//   fill   : the kept entries in stored order: o_col = map[col], o_val = val (* rscale[i]), o_coo_row = i
// The transposed block is the same cut of the resident TRANSPOSE (its rows hold the source rows in ascending order, which is the
// stable transposition of the block); there a row's scale belongs to the entry's relabelled COLUMN (scale_cols).
// One wavefront per row, chunks of 64 entries: a wave64 ballot of `kept` and a popcount of the lower lanes give every kept
// entry its slot -- no atomics, no LDS, and count and fill share ONE predicate (kept_slot), so the slots fit the scan.
#include "sgcn_dev.h"

namespace sgcn {
namespace {

constexpr int kRowsPerBlock = kBlock / kWave;

// the relabelled column of entry p (-1: dropped, or p past the row's end)
__device__ __forceinline__ int kept_slot(const int32_t* __restrict__ col, const int32_t* __restrict__ map, int64_t p, int64_t end) {
    return p < end ? map[col[p]] : -1;
}

__device__ __forceinline__ bool my_row(const int32_t* __restrict__ ids, const int32_t* __restrict__ rowptr, int32_t n, int64_t& i,
                                       int& start, int& end) {
    i = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x / kWave;
    if (i >= n) return false;
    const int row = __builtin_amdgcn_readfirstlane(ids[i]);
    start = __builtin_amdgcn_readfirstlane(rowptr[row]);
    end = __builtin_amdgcn_readfirstlane(rowptr[row + 1]);
    return true;
}

__global__ __launch_bounds__(kBlock) void induce_map_kernel(const int32_t* __restrict__ ids, int32_t n, int32_t* __restrict__ map) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) map[ids[i]] = (int32_t)i;
}

// o_rowptr[i + 1] = the row's kept entries (the scan below turns the counts into offsets); o_full / o_kept (with val): every
// lane adds its own entries in stored order, then the 64 partial sums meet in one xor tree -- a fixed order whatever the schedule
__global__ __launch_bounds__(kBlock) void induce_count_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                              const float* __restrict__ val, const int32_t* __restrict__ ids,
                                                              int32_t n, const int32_t* __restrict__ map,
                                                              int32_t* __restrict__ o_rowptr, float* __restrict__ o_full,
                                                              float* __restrict__ o_kept) {
    int64_t i;
    int start, end;
    if (!my_row(ids, rowptr, n, i, start, end)) return;
    const int lane = threadIdx.x & (kWave - 1);
    int cnt = 0;
    float sf = 0.f, sk = 0.f;
    for (int64_t p0 = start; p0 < end; p0 += kWave) {
        const int64_t p = p0 + lane;
        const int m = kept_slot(col, map, p, end);
        cnt += __popcll(__ballot(m >= 0));
        if (val) {
            const float v = p < end ? val[p] : 0.f;
            sf += v;
            sk += m >= 0 ? v : 0.f;
        }
    }
    if (val) {
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            sf += __shfl_xor(sf, o, kWave);
            sk += __shfl_xor(sk, o, kWave);
        }
    }
    if (lane == 0) {
        o_rowptr[i + 1] = cnt;
        if (val) { o_full[i] = sf; o_kept[i] = sk; }
    }
}

// counts in o_rowptr[1 .. n] -> offsets, in place: ONE workgroup, every thread a contiguous run of rows, the run totals
// scanned through LDS (the scheme of csr_slice_indptr_kernel; a thread only ever touches its own run's words)
__global__ __launch_bounds__(kBlock) void induce_scan_kernel(int32_t n, int32_t* __restrict__ o_rowptr) {
    __shared__ int32_t part[kBlock];
    const int t = threadIdx.x;
    const int32_t per = (n + kBlock - 1) / kBlock;
    const int32_t b = min(n, t * per), e = min(n, b + per);
    int32_t s = 0;
    for (int32_t i = b; i < e; i++) s += o_rowptr[i + 1];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int32_t acc = 0;
        for (int k = 0; k < kBlock; k++) { const int32_t v = part[k]; part[k] = acc; acc += v; }
        o_rowptr[0] = 0;
    }
    __syncthreads();
    int32_t acc = part[t];
    for (int32_t i = b; i < e; i++) { acc += o_rowptr[i + 1]; o_rowptr[i + 1] = acc; }
}

// the kept entries of row i at o_rowptr[i] + (kept entries before them in the row): stored order, so a sorted row stays sorted.
// cap > 0: the words [o_rowptr[n], cap) of o_col (and o_coo_row) take the value n -- a pad column behind the last real one, so
// that a transposition launched over `cap` entries, before the host knows o_rowptr[n], sorts the pad behind every real entry
__global__ __launch_bounds__(kBlock) void induce_fill_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                             const float* __restrict__ val, const int32_t* __restrict__ ids,
                                                             int32_t n, const int32_t* __restrict__ map,
                                                             const int32_t* __restrict__ o_rowptr, const float* __restrict__ rscale,
                                                             int32_t* __restrict__ o_col, float* __restrict__ o_val,
                                                             int32_t* __restrict__ o_coo_row, int32_t scale_cols, int64_t cap) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t p = (int64_t)o_rowptr[n] + (int64_t)blockIdx.x * kBlock + threadIdx.x; p < cap; p += stride) {
        o_col[p] = n;
        if (o_coo_row) o_coo_row[p] = n;
    }
    int64_t i;
    int start, end;
    if (!my_row(ids, rowptr, n, i, start, end)) return;
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t below = (1ull << lane) - 1ull;
    const float f = rscale && !scale_cols ? rscale[i] : 1.f;
    int64_t dst = o_rowptr[i];
    for (int64_t p0 = start; p0 < end; p0 += kWave) {
        const int64_t p = p0 + lane;
        const int m = kept_slot(col, map, p, end);
        const uint64_t kept = __ballot(m >= 0);
        if (m >= 0) {
            const int64_t q = dst + __popcll(kept & below);
            o_col[q] = m;
            if (val) o_val[q] = rscale ? val[p] * (scale_cols ? rscale[m] : f) : val[p];
            if (o_coo_row) o_coo_row[q] = (int32_t)i;
        }
        dst += __popcll(kept);
    }
}

}  // namespace
}  // namespace sgcn

using namespace sgcn;

extern "C" int sgcn_induce_map_i32(const int32_t* ids, int32_t n, int32_t N, int32_t* map, void* stream) {
    SGCN_REQUIRE(n >= 0 && N >= 0, "induce_map: negative size");
    SGCN_REQUIRE(n <= N, "induce_map: %d ids cannot be unique in [0, %d)", n, N);
    SGCN_REQUIRE((ids || n == 0) && (map || N == 0), "induce_map: null operand");
    if (N == 0) return SGCN_OK;
    hipStream_t st = (hipStream_t)stream;
    SGCN_HIP_TRY(hipMemsetAsync(map, 0xff, (size_t)N * sizeof(int32_t), st));        // every word -1
    if (n == 0) return SGCN_OK;
    hipLaunchKernelGGL(induce_map_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, ids, n, map);
    SGCN_HIP_TRY(hipGetLastError());
    return SGCN_OK;
}

extern "C" int sgcn_csr_induce_count(const int32_t* rowptr, const int32_t* col, const float* val, const int32_t* ids, int32_t n,
                                     const int32_t* map, int32_t* o_rowptr, float* o_full, float* o_kept, void* stream) {
    SGCN_REQUIRE(n >= 0, "csr_induce_count: negative size");
    SGCN_REQUIRE(o_rowptr || n == 0, "csr_induce_count: null operand");
    SGCN_REQUIRE(n == 0 || (rowptr && col && ids && map), "csr_induce_count: null operand");
    SGCN_REQUIRE(n == 0 || !val || (o_full && o_kept), "csr_induce_count: null operand (values without o_full / o_kept)");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (o_rowptr) SGCN_HIP_TRY(hipMemsetAsync(o_rowptr, 0, sizeof(int32_t), st));
        return SGCN_OK;
    }
    const unsigned blocks = (unsigned)(((int64_t)n + kRowsPerBlock - 1) / kRowsPerBlock);
    hipLaunchKernelGGL(induce_count_kernel, dim3(blocks), dim3(kBlock), 0, st, rowptr, col, val, ids, n, map, o_rowptr, o_full,
                       o_kept);
    hipLaunchKernelGGL(induce_scan_kernel, dim3(1), dim3(kBlock), 0, st, n, o_rowptr);
    SGCN_HIP_TRY(hipGetLastError());
    return SGCN_OK;
}

extern "C" int sgcn_csr_induce_fill(const int32_t* rowptr, const int32_t* col, const float* val, const int32_t* ids, int32_t n,
                                    const int32_t* map, const int32_t* o_rowptr, const float* rscale, int32_t* o_col,
                                    float* o_val, int32_t* o_coo_row, int32_t scale_cols, int64_t cap, void* stream) {
    SGCN_REQUIRE(n >= 0 && cap >= 0, "csr_induce_fill: negative size");
    if (n == 0) return SGCN_OK;
    SGCN_REQUIRE(rowptr && col && ids && map && o_rowptr && o_col, "csr_induce_fill: null operand");
    SGCN_REQUIRE(!val || o_val, "csr_induce_fill: null operand (values without o_val)");
    SGCN_REQUIRE(val || !rscale, "csr_induce_fill: rscale needs values");
    const unsigned blocks = (unsigned)(((int64_t)n + kRowsPerBlock - 1) / kRowsPerBlock);
    hipLaunchKernelGGL(induce_fill_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, rowptr, col, val, ids, n, map,
                       o_rowptr, rscale, o_col, o_val, o_coo_row, scale_cols, cap);
    SGCN_HIP_TRY(hipGetLastError());
    return SGCN_OK;
}
