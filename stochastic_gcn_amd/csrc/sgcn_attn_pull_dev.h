// What the two-table attention kernels share (sgcn_spattn_pull.hip: dot-product scores; sgcn_spgat_pull.hip: learned additive
// scores) beside sgcn_attn_dev.h and sgcn_pull_dev.h: the second kernel argument, the selected row of a lane group, the
// source word of an entry, and the checks both hosts open with.
#pragma once
#include <cmath>
#include "sgcn_attn_dev.h"
#include "sgcn_pull_dev.h"

namespace sgcn {
namespace {

// what a pull launch reads beside AttnArgs (own = gat = X; rowptr / col the resident matrix's): a second kernel argument
struct PullTab {
    const int32_t* ids;
    const int32_t* map;
    const void* H;           // fp32, or uint16 for a bfloat16 table: the kernel's HT says which
    int64_t ldh;             // in elements of H
};

// the selected row of this group: its position i in ids (the row of X, C, lse, ..) and its entries in the resident CSR
template <int G>
__device__ __forceinline__ bool my_row(const AttnArgs& a, const PullTab& t, int& i, int& start, int& end) {
    constexpr int GPB = kBlock / G;
    const int64_t s = (int64_t)blockIdx.x * GPB + threadIdx.x / G;
    if (s >= a.nseg) return false;
    const int row = t.ids[s];
    i = uniform_i<G>((int)s); start = uniform_i<G>(a.rowptr[row]); end = uniform_i<G>(a.rowptr[row + 1]);
    return true;
}

// the source word of the entry this lane fetched for the chunk at p0 (0 past the chunk's n entries: never used as a key
// with weight, the broadcasts clamp to n - 1)
__device__ __forceinline__ int my_source(const AttnArgs& a, const PullTab& t, int p0, int lig, int n) {
    int src = 0;
    if (lig < n) {
        const int c = a.col[p0 + lig];
        const int m = t.map[c];
        src = m >= 0 ? m : ~c;
    }
    return src;
}

// what every host body opens with: everything attn_open and spmm_pull refuse, and a non-finite scale
inline int pull_open(const char* who, int32_t n, int32_t N, int32_t d, int32_t heads, float scale) {
    if (const int rc = attn_open(who, n, N, d, heads, 1.0f)) return rc;
    SGCN_REQUIRE(n <= N, "%s: %d rows cannot be unique in [0, %d)", who, n, N);
    SGCN_REQUIRE(std::isfinite(scale), "%s: scale must be finite", who);
    return SGCN_OK;
}

}  // namespace
}  // namespace sgcn
