// What the two-table gather kernels share (sgcn_spmm_pull.hip: the neighbour sum; sgcn_spattn_pull.hip: attention): an entry's
// operand row comes from the FRESH table X (fp32) where the column lies in the step's vertex set and from the STALE table H
// (fp32, or bfloat16 widened exactly) where it does not.  Both kernels fold table and row into one source word per entry
// (m >= 0 ? m : ~col, with m = map[col]) and form the address behind its broadcast; here are the raw image of a load and
// the two steps -- request, widen -- that turn a source address into VW floats.
#pragma once
#include "sgcn_dev.h"

namespace sgcn {
namespace {

// the raw image of VW operand elements: VW dwords (a fresh fp32 vector; a bfloat16 vector in the lower half)
template <int VW> struct PullRaw { typedef uint32_t type __attribute__((ext_vector_type(VW))); };
template <> struct PullRaw<1> { typedef uint32_t type; };

template <int VW, class HT>
__device__ __forceinline__ typename PullRaw<VW>::type pull_load(const char* src, uint32_t xoff, bool stale) {
    typedef typename PullRaw<VW>::type RT;
    if constexpr (std::is_same<HT, float>::value) {
        return *reinterpret_cast<const RT*>(src + xoff);                        // either table: fp32 rows
    } else {
        RT r = {};
        if (stale) {
            const uint16_t* p = reinterpret_cast<const uint16_t*>(src + (xoff >> 1));
            if constexpr (VW == 4) { const auto h = hraw<4>(p); r.x = h.x; r.y = h.y; }
            else if constexpr (VW == 2) r.x = hraw<2>(p);
            else r = hraw<1>(p);
        } else {
            r = *reinterpret_cast<const RT*>(src + xoff);
        }
        return r;
    }
}

template <int VW, class HT>
__device__ __forceinline__ typename Vec<VW>::type pull_value(typename PullRaw<VW>::type r, bool stale) {
    typedef typename Vec<VW>::type VT;
    if constexpr (VW == 1) {
        if constexpr (!std::is_same<HT, float>::value) { if (stale) return hwiden1(r); }
        return __uint_as_float(r);
    } else {
        VT v;
        if constexpr (!std::is_same<HT, float>::value) {
            if (stale) {
                if constexpr (VW == 2) { v[0] = hwiden1(r.x); v[1] = __uint_as_float(r.x & 0xffff0000u); }
                else {
                    v[0] = hwiden1(r.x); v[1] = __uint_as_float(r.x & 0xffff0000u);
                    v[2] = hwiden1(r.y); v[3] = __uint_as_float(r.y & 0xffff0000u);
                }
                return v;
            }
        }
#pragma unroll
        for (int e = 0; e < VW; e++) v[e] = __uint_as_float(r[e]);
        return v;
    }
}

}  // namespace
}  // namespace sgcn
