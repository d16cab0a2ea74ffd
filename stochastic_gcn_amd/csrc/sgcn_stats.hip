// Running statistics of the --gradvar bias / variance study (gcn/train.py:241-276, gcn/stats.py): the reference keeps
// every draw of a prediction / gradient in a host list and reduces it with np.mean / np.std at the end.  Here each draw is
// folded into a running fp64 mean and sum of squared deviations on the device as it is produced (Welford), and the study's
// scalars come out of one fixed-order reduction.  fp64 throughout: a plain sum of x and x^2 loses the variance when the
// stdev is far below the mean, which is the every-neighbour estimator's case (stdev ~ 0).
#include "sgcn_dev.h"

#include <algorithm>
#include <cmath>

namespace sgcn {
namespace {

typedef double double2v __attribute__((ext_vector_type(2)));
typedef float float4v __attribute__((ext_vector_type(4)));

// one Welford step on element i: `count` samples are already in (mean, m2); FIRST (count == 0) reads neither
template <bool FIRST>
__device__ __forceinline__ void welford(double x, double& m, double& s, double n1) {
    if (FIRST) {
        m = x;
        s = 0.0;
    } else {
        const double d = x - m;
        m = m + d / n1;
        s = s + d * (x - m);
    }
}

// Elements [head, head + 4 nvec): x as float4, mean / m2 as two double2 each (all three 16-byte aligned there, checked by
// the caller); the rest -- [0, head) and [head + 4 nvec, n) -- one element per thread.  nvec == 0: the scalar path.
template <bool FIRST>
__global__ __launch_bounds__(kBlock) void moments_add_kernel(const float* __restrict__ x, int64_t n, int64_t head,
                                                             int64_t nvec, double n1, double* __restrict__ mean,
                                                             double* __restrict__ m2) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (int64_t j = t0; j < nvec; j += stride) {
        const int64_t i = head + 4 * j;
        const float4v xv = *reinterpret_cast<const float4v*>(x + i);
        double2v m01 = {}, m23 = {}, s01 = {}, s23 = {};
        if (!FIRST) {
            m01 = *reinterpret_cast<const double2v*>(mean + i);
            m23 = *reinterpret_cast<const double2v*>(mean + i + 2);
            s01 = *reinterpret_cast<const double2v*>(m2 + i);
            s23 = *reinterpret_cast<const double2v*>(m2 + i + 2);
        }
        double m[4] = {m01[0], m01[1], m23[0], m23[1]}, s[4] = {s01[0], s01[1], s23[0], s23[1]};
#pragma unroll
        for (int e = 0; e < 4; e++) welford<FIRST>(xv[e], m[e], s[e], n1);
        *reinterpret_cast<double2v*>(mean + i) = double2v{m[0], m[1]};
        *reinterpret_cast<double2v*>(mean + i + 2) = double2v{m[2], m[3]};
        *reinterpret_cast<double2v*>(m2 + i) = double2v{s[0], s[1]};
        *reinterpret_cast<double2v*>(m2 + i + 2) = double2v{s[2], s[3]};
    }
    const int64_t tail0 = head + 4 * nvec, rest = head + (n - tail0);
    for (int64_t k = t0; k < rest; k += stride) {
        const int64_t i = k < head ? k : tail0 + (k - head);
        double m = FIRST ? 0.0 : mean[i], s = FIRST ? 0.0 : m2[i];
        welford<FIRST>(x[i], m, s, n1);
        mean[i] = m;
        m2[i] = s;
    }
}

// out3 = { mean |mean_a|, mean sqrt(m2_a / count_a), mean |mean_a - mean_b| (0 without mean_b) }: ONE workgroup, every
// thread a fixed strided subset, partials combined by a fixed tree -- bitwise the same on every call.
__global__ __launch_bounds__(kBlock) void moments_summary_kernel(const double* __restrict__ mean_a,
                                                                 const double* __restrict__ m2_a, double count,
                                                                 const double* __restrict__ mean_b, int64_t n,
                                                                 double* __restrict__ out3) {
    __shared__ double red[3][kBlock];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kBlock) {
        const double m = mean_a[i];
        a0 += fabs(m);
        a1 += sqrt(m2_a[i] / count);
        if (mean_b) a2 += fabs(m - mean_b[i]);
    }
    red[0][threadIdx.x] = a0;
    red[1][threadIdx.x] = a1;
    red[2][threadIdx.x] = a2;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
            red[2][threadIdx.x] += red[2][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) out3[threadIdx.x] = red[threadIdx.x][0] / (double)n;     // n == 0: NaN, as np.mean of nothing
}

// ---- staleness of a control-variate history (--history_error): x = the exact activations, h = the stored table ----------
// out4 = { sum (x - h)^2, sum x^2, max |x - h|, rows with any x != h }, every difference and square in fp64 ((double)x -
// (double)h is exact).  A FIXED grid (kHistErrBlocks workgroups whatever the device): wave w of the grid takes rows w, w +
// kHistErrWaves, ..., four of them per trip (their loads are requested before any is added), its lanes stride the columns and
// keep fp64 partials; a workgroup folds its 256 lanes by a fixed tree into ws[4 b ..], and hist_error_final_kernel -- one
// workgroup -- adds the kHistErrBlocks partials in index order.  No atomics: the same bits on every call.
constexpr int kHistErrBlocks = 1024;
constexpr int kHistErrWaves = kHistErrBlocks * (kBlock / kWave);
constexpr int kHistErrRows = 4;

__device__ __forceinline__ float hist_elem(const float* p) { return *p; }
__device__ __forceinline__ float hist_elem(const uint16_t* p) { return __uint_as_float((uint32_t)*p << 16); }

template <class HT>
__global__ __launch_bounds__(kBlock) void hist_error_kernel(const float* __restrict__ x, int64_t ldx, const HT* __restrict__ h,
                                                            int64_t ldh, int64_t n, int32_t d, double* __restrict__ ws) {
    __shared__ double red[4][kBlock];
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    double s_err = 0.0, s_ref = 0.0, s_max = 0.0, s_rows = 0.0;
    for (int64_t r0 = wave; r0 < n; r0 += (int64_t)kHistErrRows * kHistErrWaves) {      // (wave-uniform)
        int off[kHistErrRows] = {};
        for (int c = lane; c < d; c += kWave) {
            float xv[kHistErrRows], hv[kHistErrRows];
#pragma unroll
            for (int u = 0; u < kHistErrRows; u++) {
                const int64_t r = r0 + (int64_t)u * kHistErrWaves;
                const bool in = r < n;
                xv[u] = in ? x[r * ldx + c] : 0.f;
                hv[u] = in ? hist_elem(h + r * ldh + c) : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kHistErrRows; u++) {
                const double xd = (double)xv[u], e = xd - (double)hv[u];
                s_err = __dadd_rn(s_err, __dmul_rn(e, e));          // (no contraction: each square is rounded, then added)
                s_ref = __dadd_rn(s_ref, __dmul_rn(xd, xd));
                s_max = fmax(s_max, fabs(e));
                off[u] |= xv[u] != hv[u];
            }
        }
#pragma unroll
        for (int u = 0; u < kHistErrRows; u++)
            if (__any(off[u]) && lane == 0) s_rows += 1.0;
    }
    red[0][threadIdx.x] = s_err;
    red[1][threadIdx.x] = s_ref;
    red[2][threadIdx.x] = s_max;
    red[3][threadIdx.x] = s_rows;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
            red[2][threadIdx.x] = fmax(red[2][threadIdx.x], red[2][threadIdx.x + s]);
            red[3][threadIdx.x] += red[3][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) ws[4 * (int64_t)blockIdx.x + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(kBlock) void hist_error_final_kernel(const double* __restrict__ ws, double* __restrict__ out4) {
    __shared__ double part[4 * kHistErrBlocks];
    for (int i = threadIdx.x; i < 4 * kHistErrBlocks; i += kBlock) part[i] = ws[i];
    __syncthreads();
    if (threadIdx.x < 4) {
        const int q = threadIdx.x;
        double a = 0.0;
        for (int b = 0; b < kHistErrBlocks; b++) a = q == 2 ? fmax(a, part[4 * b + q]) : a + part[4 * b + q];
        out4[q] = a;
    }
}

template <class HT>
int hist_error_launch(const char* who, const float* x, int64_t ldx, const HT* h, int64_t ldh, int64_t n, int32_t d, double* out4,
                      double* ws, hipStream_t st) {
    SGCN_REQUIRE(n >= 0 && d >= 0, "%s: negative size", who);
    SGCN_REQUIRE(out4 && aligned8(out4), "%s: out4 must be an 8-byte aligned device address", who);
    if (n == 0 || d == 0) {
        SGCN_HIP_TRY(hipMemsetAsync(out4, 0, 4 * sizeof(double), st));
        return SGCN_OK;
    }
    SGCN_REQUIRE(x && h && ws, "%s: null operand", who);
    SGCN_REQUIRE(aligned8(ws) && (reinterpret_cast<uintptr_t>(x) & 3u) == 0, "%s: operand not aligned to its element size", who);
    SGCN_REQUIRE(ldx >= d && ldh >= d, "%s: leading dimension too small", who);
    hipLaunchKernelGGL(hist_error_kernel<HT>, dim3(kHistErrBlocks), dim3(kBlock), 0, st, x, ldx, h, ldh, n, d, ws);
    SGCN_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(hist_error_final_kernel, dim3(1), dim3(kBlock), 0, st, ws, out4);
    SGCN_HIP_TRY(hipGetLastError());
    return SGCN_OK;
}

}  // namespace
}  // namespace sgcn

using namespace sgcn;

extern "C" int sgcn_moments_add_f32(const float* x, int64_t n, int64_t count, double* mean, double* m2, void* stream) {
    SGCN_REQUIRE(n >= 0, "moments_add: negative size");
    SGCN_REQUIRE(count >= 0, "moments_add: negative count");
    SGCN_REQUIRE(x && mean && m2, "moments_add: null operand");
    SGCN_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3u) == 0 && aligned8(mean) && aligned8(m2),
                 "moments_add: operand not aligned to its element size");
    if (n == 0) return SGCN_OK;
    // vector path from the first element at which x is 16-byte aligned, if mean / m2 are 16-byte aligned there as well
    // (x may be a view into the flat gradient buffer at any float offset)
    int64_t head = (int64_t)(((16u - (reinterpret_cast<uintptr_t>(x) & 15u)) & 15u) / 4u);
    int64_t nvec = 0;
    if (head < n && aligned16(mean + head) && aligned16(m2 + head)) nvec = (n - head) / 4;
    if (nvec == 0) head = 0;
    const int64_t work = std::max(nvec, head + (n - head - 4 * nvec));
    const unsigned blocks = (unsigned)std::min<int64_t>((work + kBlock - 1) / kBlock, 2048);
    const double n1 = (double)count + 1.0;
    if (count == 0)
        hipLaunchKernelGGL(moments_add_kernel<true>, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, x, n, head, nvec, n1,
                           mean, m2);
    else
        hipLaunchKernelGGL(moments_add_kernel<false>, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, x, n, head, nvec,
                           n1, mean, m2);
    SGCN_HIP_TRY(hipGetLastError());
    return SGCN_OK;
}

extern "C" int sgcn_moments_summary_f64(const double* mean_a, const double* m2_a, int64_t count_a, const double* mean_b,
                                        int64_t n, double* out3, void* stream) {
    SGCN_REQUIRE(n >= 0, "moments_summary: negative size");
    SGCN_REQUIRE(count_a > 0, "moments_summary: count_a must be positive (got %lld)", (long long)count_a);
    SGCN_REQUIRE(mean_a && m2_a && out3, "moments_summary: null operand");
    hipLaunchKernelGGL(moments_summary_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, mean_a, m2_a,
                       (double)count_a, mean_b, n, out3);
    SGCN_HIP_TRY(hipGetLastError());
    return SGCN_OK;
}

extern "C" int64_t sgcn_hist_error_ws_doubles(void) { return 4 * (int64_t)kHistErrBlocks; }

extern "C" int sgcn_hist_error_f32(const float* x, int64_t ldx, const float* h, int64_t ldh, int64_t n, int32_t d, double* out4,
                                   double* ws, void* stream) {
    SGCN_REQUIRE(!h || (reinterpret_cast<uintptr_t>(h) & 3u) == 0, "hist_error_f32: history not aligned to its element size");
    return hist_error_launch<float>("hist_error_f32", x, ldx, h, ldh, n, d, out4, ws, (hipStream_t)stream);
}

extern "C" int sgcn_hist_error_h16(const float* x, int64_t ldx, const uint16_t* h, int64_t ldh, int64_t n, int32_t d, double* out4,
                                   double* ws, void* stream) {
    // (the bfloat16 history's storage contract, include/sgcn.h: pitch in elements, a multiple of 8, a 16-byte aligned base)
    SGCN_REQUIRE(!h || (ldh % 8 == 0 && aligned16(h)),
                 "hist_error_h16: a bfloat16 history needs ldh %% 8 == 0 and a 16-byte aligned base (ldh %lld)", (long long)ldh);
    return hist_error_launch<uint16_t>("hist_error_h16", x, ldx, h, ldh, n, d, out4, ws, (hipStream_t)stream);
}
