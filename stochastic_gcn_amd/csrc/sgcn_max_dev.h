// What the element-wise maximum kernels share (sgcn_spmax.hip: one table; sgcn_spmax_pull.hip: a fresh and a stale table): the
// vector of winners' ids beside a vector of values, its loads and ragged stores, and the forward's comparison -- the tie
// rule of sgcn_spmax.hip's header lives in `max_take` alone.
#pragma once
#include "sgcn_dev.h"

namespace sgcn {
namespace {

template <int VW> struct IVec;
template <> struct IVec<4> { typedef int32_t type __attribute__((ext_vector_type(4))); };
template <> struct IVec<2> { typedef int32_t type __attribute__((ext_vector_type(2))); };
template <> struct IVec<1> { typedef int32_t type; };

template <int VW>
__device__ __forceinline__ typename IVec<VW>::type iload(const int32_t* p) {
    return *reinterpret_cast<const typename IVec<VW>::type*>(p);
}
template <int VW>
__device__ __forceinline__ typename IVec<VW>::type isplat(int x) {
    if constexpr (VW == 1) return x;
    else {
        typename IVec<VW>::type v;
#pragma unroll
        for (int e = 0; e < VW; e++) v[e] = x;
        return v;
    }
}
// the first `cnt` (<= VW) elements: a whole vector store when cnt == VW, element-wise on the ragged tail
template <int VW>
__device__ __forceinline__ void istore_n(int32_t* p, typename IVec<VW>::type v, int cnt) {
    if (cnt >= VW) *reinterpret_cast<typename IVec<VW>::type*>(p) = v;
    else {
#pragma unroll
        for (int e = 0; e < VW; e++)
            if (e < cnt) {
                if constexpr (VW == 1) p[0] = v; else p[e] = v[e];
            }
    }
}
template <int VW>
__device__ __forceinline__ void vstore_n(float* p, typename Vec<VW>::type v, int cnt) {
    if (cnt >= VW) vstore<VW>(p, v);
    else vstore_head<VW>(p, v, cnt);
}

// forward: entry (v, id c) against the running best -- strictly greater, per element
template <int VW>
__device__ __forceinline__ void max_take(typename Vec<VW>::type& best, typename IVec<VW>::type& barg,
                                         const typename Vec<VW>::type& v, int c) {
    if constexpr (VW == 1) {
        const bool t = v > best;
        best = t ? v : best;
        barg = t ? c : barg;
    } else {
#pragma unroll
        for (int e = 0; e < VW; e++) {
            const bool t = v[e] > best[e];
            best[e] = t ? v[e] : best[e];
            barg[e] = t ? c : barg[e];
        }
    }
}

}  // namespace
}  // namespace sgcn
