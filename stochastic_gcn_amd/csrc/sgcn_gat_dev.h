// What the kernels with learned additive attention scores (GAT) share: sgcn_spgat.hip over one table, sgcn_spgat_pull.hip over
// the fresh / stale pair of a part step.  The score tables as a kernel argument, the LeakyReLU and its derivative, and the
// check on its slope.
#pragma once
#include <cmath>
#include "sgcn_attn_dev.h"

namespace sgcn {
namespace {

// the score tables and the score gradients, a second kernel argument (AttnArgs keeps its layout); the mask is the third
struct GatX {
    const float* U;          // u: element [i * ldu + h], i a row of P
    int64_t ldu;
    const float* V;          // v: element [j * ldv + h], j a column of P
    int64_t ldv;
    float slope;
    float* dU;               // bwd_u: M x H, contiguous
    float* dV;               // bwd_v: K x H, contiguous
};

__device__ __forceinline__ float leaky(float z, float slope) { return z > 0.f ? z : slope * z; }
__device__ __forceinline__ float leaky_d(float z, float slope) { return z > 0.f ? 1.f : slope; }

template <int G, bool MH>
__device__ __forceinline__ float head_total(float v, int gh) {
    float s[1] = {v};
    if constexpr (MH) head_sum<G, 1>(s, gh); else group_sum<G, 1>(s);
    return s[0];
}

template <int NV>
struct GatUnroll { static constexpr int fwd = 4, bwd = NV >= 3 ? 2 : 4; };

inline int slope_ok(const char* who, float slope) {
    SGCN_REQUIRE(std::isfinite(slope) && slope >= 0.f && slope <= 1.f, "%s: slope must lie in [0, 1] (got %g)", who, (double)slope);
    return SGCN_OK;
}

}  // namespace
}  // namespace sgcn
