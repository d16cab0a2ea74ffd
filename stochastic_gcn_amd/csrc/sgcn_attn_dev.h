// What the attention kernels over a CSR pattern share (sgcn_spattn.hip: dot-product scores; sgcn_spgat.hip: learned additive
// scores).  Device: the kernel arguments, the coefficient mask, a lane's share of a row, the reductions over a group or a
// head, the forward slots' ordered fix-up, the backward's epilogue.  Host: the slot widths, the checks every export opens
// with, and the one path from checked arguments to a launch -- the multi-head geometry, the choice of (DR, MH), the fix-up --
// which each translation unit instantiates with a launcher for its own kernels.  The checks on a plan, the one-head geometry and
// the ladders over (VW, G, NV) are those of every row-segment launch (sgcn_seg.h).
#pragma once
#include <cmath>
#include "sgcn_dev.h"
#include "sgcn_seg.h"

namespace sgcn {
namespace {

constexpr int kMaxVec = 256;   // vectors per row: 64 lanes x NV <= 4

struct AttnArgs {
    const int32_t* rowptr;
    const int32_t* col;      // forward / bwd_q: column ids; bwd_kv: the source rows of the transposed pattern
    const sgcn_seg_t* seg;   // nullable: implicit one segment per row
    int64_t nseg;
    const float* own;        // the table the segment's own row comes from: Q (forward, bwd_q), B (bwd_kv)
    int64_t ldown;
    const float* gat;        // the gathered table: B (forward, bwd_q), Q (bwd_kv)
    int64_t ldgat;
    const float* G;          // bwd_q: the own row's gradient; bwd_kv: gathered beside `gat`
    int64_t ldg;
    const float* Cf;         // bwd_q: the forward's output
    int64_t ldcf;
    const float* lse;        // backward
    const float* delta;      // bwd_kv
    float* delta_out;        // bwd_q
    float* lse_out;          // forward, nullable
    float* out;              // C / dQ / dB
    int64_t ldo;
    float scale;
    int32_t d;
    int32_t nvec;            // ceil(d / VW)
    int32_t ragged;          // d % VW != 0: the last vector over-reads pad elements, which are zeroed after the load
    float* ws;
    int64_t ldw;
    const float* add;        // backward: out[row] += add[row] for row < add_rows
    int64_t ldadd;
    int32_t add_rows;
    int32_t heads;           // H; the MH kernels only read the three below
    int32_t gh;              // lanes per head, G / H (a power of two)
    int32_t nvh;             // vectors per head, dh / VW
};

// the coefficient mask (include/sgcn.h, attention dropout), a second kernel argument: AttnArgs keeps its layout, and the
// kernels without dropout do not read this one
struct AttnDrop {
    uint32_t key, thr;       // kept iff hash < thr
    float mk;                // 1 / keep
};
// The kept bits of entry (i, j) of P: bit h is set iff head h keeps it.  A lane hashes the ONE entry whose id it fetched for the
// chunk of G entries -- all heads of it, 1 + H finalisers per G entries and lane -- and the bits travel with the id's
// broadcast: per entry a lane adds one move and one bit test, not two finalisers.
template <bool MH>
__device__ __forceinline__ int drop_bits(const AttnDrop& a, int i, int j, int heads) {
    const uint32_t pair = fmix32(fmix32((uint32_t)i * 0x9E3779B1u + a.key) + (uint32_t)j * 0x85EBCA77u);
    if constexpr (!MH) return fmix32(pair) < a.thr;
    else {
        int bits = 0;
        for (int h = 0; h < heads; h++) bits |= (int)(fmix32(pair + (uint32_t)h * 0x27D4EB2Fu) < a.thr) << h;
        return bits;
    }
}
__device__ __forceinline__ float drop_mk(const AttnDrop& a, int bits, int head) { return (bits >> head) & 1 ? a.mk : 0.f; }

template <int G>
__device__ __forceinline__ bool my_segment(const AttnArgs& a, int& row, int& start, int& end, int& slot) {
    constexpr int GPB = kBlock / G;
    const int64_t s = (int64_t)blockIdx.x * GPB + threadIdx.x / G;
    if (s >= a.nseg) return false;
    if (a.seg) {
        const sgcn_seg_t sg = a.seg[s];
        row = sg.row; start = sg.start; end = sg.end; slot = sg.slot;
    } else {
        row = (int)s; start = a.rowptr[s]; end = a.rowptr[s + 1]; slot = -1;
    }
    row = uniform_i<G>(row); start = uniform_i<G>(start);
    end = uniform_i<G>(end); slot = uniform_i<G>(slot);
    return true;
}

// zero the elements e >= cnt: the pad a ragged last vector over-read (cnt < VW), a lane past the row width (cnt == 0)
template <int VW>
__device__ __forceinline__ void keep_head(typename Vec<VW>::type& v, int cnt) {
    if constexpr (VW == 1) v = cnt > 0 ? v : 0.f;
    else {
#pragma unroll
        for (int e = 0; e < VW; e++) v[e] = e < cnt ? v[e] : 0.f;
    }
}
template <int VW>
__device__ __forceinline__ float vdot(const typename Vec<VW>::type& x, const typename Vec<VW>::type& y, float acc) {
    if constexpr (VW == 1) return __builtin_fmaf(x, y, acc);
    else {
#pragma unroll
        for (int e = 0; e < VW; e++) acc = __builtin_fmaf(x[e], y[e], acc);
        return acc;
    }
}
template <int VW>
__device__ __forceinline__ void vstore_n(float* p, typename Vec<VW>::type v, int cnt) {
    if (cnt >= VW) vstore<VW>(p, v);
    else vstore_head<VW>(p, v, cnt);
}

// lse = m + log l, once per row: the logarithm and the sum in fp64, rounded once (logf alone was measured 2 ulp off at
// l = 300, and the backward's every weight exp(s - lse) inherits lse's error)
__device__ __forceinline__ float lse_of(float m, float l) { return (float)((double)m + log((double)l)); }

// the sum of U values over the group's G lanes, every lane getting every total; the U chains are independent
template <int G, int U>
__device__ __forceinline__ void group_sum(float (&s)[U]) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1)
#pragma unroll
        for (int u = 0; u < U; u++) s[u] += __shfl_xor(s[u], o, G);
}
// two sums per entry through ONE tree: after the first exchange even lanes carry s and odd lanes t, the steps 2 .. G/2
// reduce both at once, and the last two moves hand every lane both totals
template <int G, int U>
__device__ __forceinline__ void group_sum2(float (&s)[U], float (&t)[U], int lig) {
    const bool odd = lig & 1;
    float v[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const float keep = odd ? t[u] : s[u], send = odd ? s[u] : t[u];
        v[u] = keep + __shfl_xor(send, 1, G);
    }
#pragma unroll
    for (int o = 2; o < G; o <<= 1)
#pragma unroll
        for (int u = 0; u < U; u++) v[u] += __shfl_xor(v[u], o, G);
#pragma unroll
    for (int u = 0; u < U; u++) {
        s[u] = __shfl(v[u], lig & ~1, G);
        t[u] = __shfl(v[u], lig | 1, G);
    }
}

// the multi-head forms: the same sums over the aligned sub-group of `gh` lanes (wave-uniform, a power of two <= G) that the
// lane's head owns; gh == 1: every lane already holds its head's totals
template <int G, int U>
__device__ __forceinline__ void head_sum(float (&s)[U], int gh) {
    for (int o = gh >> 1; o > 0; o >>= 1)
#pragma unroll
        for (int u = 0; u < U; u++) s[u] += __shfl_xor(s[u], o, G);
}
template <int G, int U>
__device__ __forceinline__ void head_sum2(float (&s)[U], float (&t)[U], int lig, int gh) {
    if (gh == 1) return;
    const bool odd = lig & 1;
    float v[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const float keep = odd ? t[u] : s[u], send = odd ? s[u] : t[u];
        v[u] = keep + __shfl_xor(send, 1, G);
    }
    for (int o = 2; o < gh; o <<= 1)
#pragma unroll
        for (int u = 0; u < U; u++) v[u] += __shfl_xor(v[u], o, G);
#pragma unroll
    for (int u = 0; u < U; u++) {
        s[u] = __shfl(v[u], lig & ~1, G);
        t[u] = __shfl(v[u], lig | 1, G);
    }
}

// what a lane owns of a row: NV vectors, their byte offsets (lanes past the row width re-read the last valid vector
// instead of branching around the load) and how many of their elements exist
// MH: the lane's head is lig / gh, and its vectors are r, r + gh, .. (r = lig % gh) of that head's nvh whole ones
template <int G, int NV, int VW, bool MH = false>
struct Lane {
    uint32_t off[NV];
    int cnt[NV];     // 0: no such vector; VW: whole; between: the ragged last one
    int vi[NV];
    int head;        // MH: the head this lane works for (0 otherwise)
    bool first;      // MH: the lane that stores its head's scalars (lane 0 of the group otherwise)
    __device__ __forceinline__ Lane(const AttnArgs& a, int lig) {
        if constexpr (MH) {
            const int r = lig & (a.gh - 1);
            head = lig >> (31 - __builtin_clz(a.gh));
            first = r == 0;
            const int base = head * a.nvh;
#pragma unroll
            for (int k = 0; k < NV; k++) {
                const int v = r + k * a.gh;
                vi[k] = base + v;
                cnt[k] = v < a.nvh ? VW : 0;
                off[k] = (uint32_t)(base + min(v, a.nvh - 1)) * (uint32_t)(VW * sizeof(float));
            }
        } else {
            head = 0;
            first = lig == 0;
#pragma unroll
            for (int k = 0; k < NV; k++) {
                vi[k] = lig + k * G;
                cnt[k] = vi[k] < a.nvec ? min(VW, a.d - vi[k] * VW) : 0;
                off[k] = (uint32_t)min(vi[k], a.nvec - 1) * (uint32_t)(VW * sizeof(float));
            }
        }
    }
    // a row of the segment's own: loaded once, pads and absent vectors zeroed -- a zero there keeps the (finite)
    // gathered element it meets out of every dot product
    __device__ __forceinline__ void own_row(const float* base, int64_t ld, int row, typename Vec<VW>::type (&v)[NV]) const {
        const char* src = reinterpret_cast<const char*>(base) + (int64_t)row * ld * (int64_t)sizeof(float);
#pragma unroll
        for (int k = 0; k < NV; k++) {
            v[k] = vload<VW>(reinterpret_cast<const float*>(src + off[k]));
            keep_head<VW>(v[k], cnt[k]);
        }
    }
};

// A split row's slots: the largest m first, then l and acc added in slot order, each slot scaled by exp(m_q - m).
// MH: the thread's vector belongs to head vi / nvh, whose (m, l) sit 4 * head floats further on; per head the same sum.
template <int VW, bool MH>
__global__ __launch_bounds__(kBlock) void spattn_fix_kernel(AttnArgs a, const sgcn_fix_t* fix, int64_t nfix) {
    typedef typename Vec<VW>::type VT;
    const int64_t f = blockIdx.x;
    if (f >= nfix) return;
    const sgcn_fix_t fx = fix[f];
    const int vi = threadIdx.x;
    if (vi >= a.nvec) return;
    const float* w = a.ws + (int64_t)fx.first_slot * a.ldw;
    int head = 0;
    int64_t mo = a.ldw - 4;                    // where the slot keeps this thread's m; l follows it
    if constexpr (MH) { head = vi / a.nvh; mo = a.ldw - 4 * a.heads + 4 * head; }
    float m = -INFINITY;
    for (int q = 0; q < fx.nslots; q++) m = fmaxf(m, w[(int64_t)q * a.ldw + mo]);
    float l = 0.f;
    VT acc = vzero<VW>();
    for (int q = 0; q < fx.nslots; q++) {
        const float* wq = w + (int64_t)q * a.ldw;
        const float lq = wq[mo + 1];
        if (lq > 0.f) {                        // (a segment always holds an entry; the guard keeps -inf - -inf out)
            const float sc = expf(wq[mo] - m);
            l = __builtin_fmaf(lq, sc, l);
            acc = vfma<VW>(sc, vload<VW>(wq + (int64_t)vi * VW), acc);
        }
    }
    VT r = vzero<VW>();
    if (l > 0.f) r = acc / l;
    vstore_n<VW>(a.out + (int64_t)fx.row * a.ldo + (int64_t)vi * VW, r, min(VW, a.d - vi * VW));
    if constexpr (MH) {
        if (a.lse_out && vi == head * a.nvh) a.lse_out[(int64_t)fx.row * a.heads + head] = l > 0.f ? lse_of(m, l) : -INFINITY;
    } else {
        if (a.lse_out && vi == 0) a.lse_out[fx.row] = l > 0.f ? lse_of(m, l) : -INFINITY;
    }
}

// r = mul * r (+ add[row] for row < add_rows), the first `cnt` elements stored
template <int VW>
__device__ __forceinline__ void bwd_store(const AttnArgs& a, int row, int vi, typename Vec<VW>::type r, float mul) {
    const int left = a.d - vi * VW;   // > 0 by construction
    r *= mul;
    if (a.add && row < a.add_rows) {
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
    vstore_n<VW>(a.out + (int64_t)row * a.ldo + (int64_t)vi * VW, r, left);
}

// the width one group can hold at vector width vw; SGCN_ERR_INVALID beyond it, before any HIP call
int width_ok(const char* who, int32_t d, int vw, int32_t heads) {
    if (heads > 1) {
        SGCN_REQUIRE(((int64_t)d + vw - 1) / vw <= kMaxVec,
                     "%s: d = %d is over the limit of %d columns at vector width %d (d <= 256 * VW; VW = 4 needs 16-byte aligned "
                     "rows of every operand, VW = 2 8-byte aligned ones; with heads = %d VW must also divide d / heads = %d)",
                     who, d, kMaxVec * vw, vw, heads, d / heads);
        return SGCN_OK;
    }
    SGCN_REQUIRE(((int64_t)d + vw - 1) / vw <= kMaxVec,
                 "%s: d = %d is over the limit of %d columns at vector width %d (d <= 256 * VW; VW = 4 needs 16-byte aligned "
                 "rows of every operand, VW = 2 8-byte aligned ones)", who, d, kMaxVec * vw, vw);
    return SGCN_OK;
}

int heads_ok(const char* who, int32_t d, int32_t heads) {
    SGCN_REQUIRE(heads == 1 || heads == 2 || heads == 4 || heads == 8, "%s: heads must be one of 1/2/4/8 (got %d)", who, heads);
    SGCN_REQUIRE(d % heads == 0, "%s: d = %d is not a multiple of heads = %d", who, d, heads);
    return SGCN_OK;
}

// heads > 1: no vector may straddle two heads -- the widest of what the operands allow that divides d / heads
int head_vw(int vw, int32_t d, int32_t heads) {
    if (heads > 1)
        while ((d / heads) % vw) vw >>= 1;
    return vw;
}

// keep as the callers of the _drop_ exports give it: finite and in (0, 1]; SGCN_ERR_INVALID otherwise, before any HIP call
int keep_ok(const char* who, float keep) {
    SGCN_REQUIRE(std::isfinite(keep) && keep > 0.f && keep <= 1.f, "%s: keep must be finite and in (0, 1] (got %g)", who, (double)keep);
    return SGCN_OK;
}

// the mask of a call; keep == 1: mk = 0, which `run` reads as `the kernels without dropout`
inline AttnDrop drop_of(float keep, uint32_t key) {
    AttnDrop dm{};
    if (keep >= 1.0f) return dm;
    sgcn_dropout_t d{};
    d.key = key; d.keep = keep; d.rows = -1; d.width = 0;
    const DropArgs da = drop_args(&d);       // the threshold exactly as for sgcn_dropout_t
    dm.key = da.key; dm.thr = da.thr; dm.mk = da.scale;
    return dm;
}

// ---- the slots of a split row (ops.attn_slot mirrors these four) -----------------------------------------------------------
constexpr int kScalarSlot = 8;   // floats a GAT backward slot keeps for the per-head scalar sums (H <= 8)
// forward, both score kinds: the accumulator on a 16-byte pitch, then one vector (m, l, -, -) per head
inline int64_t fwd_slot(int32_t d, int32_t heads) { return seg_slot_pitch(d) + 4 * (int64_t)heads; }
inline int64_t bwd_slot(int32_t d) { return seg_slot_pitch(d); }                          // dot-product bwd_q / bwd_kv: the row
constexpr int64_t kGatBwdUSlot = kScalarSlot;                                             // GAT bwd_u: the heads' dU alone
inline int64_t gat_bwd_v_slot(int32_t d) { return seg_slot_pitch(d) + kScalarSlot; }      // GAT bwd_v: the row, then the heads' dV

// ---- what the six host bodies open with ------------------------------------------------------------------------------------
// first: the sizes, the width, the heads and the mask's keep
inline int attn_open(const char* who, int32_t M, int32_t K, int32_t d, int32_t heads, float keep) {
    SGCN_REQUIRE(M >= 0 && K >= 0, "%s: negative size", who);
    SGCN_REQUIRE(d > 0, "%s: d must be positive (got %d)", who, d);
    if (const int rc = heads_ok(who, d, heads)) return rc;
    return keep_ok(who, keep);
}

// the workspace of a plan with split rows -- an operand like the others where its slots hold vectors -- else null
inline const void* split_ws(const sgcn_plan_t* plan) { return plan && plan->nfix > 0 ? plan->dev_ws : nullptr; }

// last, after the body's own operand checks: the plan against its slot width `ldw`, then the call's vector width -- the widest
// these operands allow that no head straddles -- and the row width it can hold
inline int attn_plan_width(const char* who, const sgcn_plan_t* plan, int32_t nrows, int64_t ldw, int32_t d, int32_t heads,
                           std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> lds, int& vw) {
    if (plan)
        if (const int rc = seg_plan_ok(who, plan, nrows, ldw)) return rc;
    vw = head_vw(pick_vw(d, ptrs, lds), d, heads);
    return width_ok(who, d, vw, heads);
}

// ---- one launch ------------------------------------------------------------------------------------------------------------
// The lane geometry of a launch: G lanes per row segment and NV vectors per lane from d, vw and heads; fills what the kernels
// read of it (nvec, ragged, heads, gh, nvh).  One head: the row kernels' geometry (seg_geometry), which for nvec <= 256 is one
// slab, past 64 lanes with NV = ceil(nvec / 64).  Several: the smallest group whose sub-groups of G / heads lanes hold a head's nvh vectors one per
// lane, at least 8 lanes; past 64 lanes the sub-group is 64 / heads and a lane takes NV = ceil(nvh / Gh) <= 4 of them
// (heads * nvh <= 256, width_ok).
inline void attn_geometry(AttnArgs& a, int vw, int32_t heads, int& G, int& NV) {
    a.nvec = (a.d + vw - 1) / vw;
    a.ragged = a.d % vw != 0;
    a.heads = heads;
    if (heads == 1) {
        const SegGeom g = seg_geometry(a.nvec, a.nseg);
        G = g.G; NV = g.NV;
        a.gh = G; a.nvh = a.nvec;
    } else {
        a.nvh = a.d / heads / vw;
        int p = 1;
        while (p < a.nvh) p <<= 1;
        if (p * heads <= 64) { G = p * heads < 8 ? 8 : p * heads; NV = 1; }
        else { G = 64; NV = (a.nvh + 64 / heads - 1) / (64 / heads); }
        a.gh = G / heads;
    }
}

// The choice of (DR, MH) is attention's; (VW, G, NV) walk the ladders of sgcn_seg.h.  L is a translation unit's launcher for one
// kind of launch:
//   template <int G, int NV, int VW, bool MH, bool DR> static void launch(dim3 grid, hipStream_t, const KA&... the kernel's arguments)
//   static void fix(int vw, const AttnArgs&, const sgcn_plan_t*, hipStream_t, const X&... what it has beside them)
//   static constexpr int64_t max_fix: the split rows its fix-up's grid can count
//
// A launch from its checked arguments: the segments and the slots from the plan, the geometry, the kernel off the ladder (the
// kernels take a, x..., dm), then L's fix-up where the plan has split rows.  dm.mk == 0 (drop_of: keep == 1) and heads == 1
// select the DR = false and the MH = false kernels.
template <class L, class... X>
int attn_run(const char* who, AttnArgs& a, int32_t nrows, const sgcn_plan_t* plan, int64_t ldw, int vw, int32_t heads,
             const AttnDrop& dm, hipStream_t st, const X&... x) {
    a.nseg = nrows;
    if (plan) { a.seg = plan->dev_seg; a.nseg = plan->nseg; }
    const bool split = plan && plan->nfix > 0;
    if (split) { a.ws = plan->dev_ws; a.ldw = ldw; }
    int G, NV;
    attn_geometry(a, vw, heads, G, NV);
    const int64_t nblocks = (a.nseg + (kBlock / G) - 1) / (kBlock / G);
    SGCN_REQUIRE(nblocks < (1ll << 31), "%s: grid too large", who);

    const dim3 grid((unsigned)nblocks);
    const bool drop = dm.mk > 0.f;
    auto ladder = [&](auto MH, auto DR) {
        return with_vw(vw, [&](auto VW) {
            return with_gnv(G, NV, [&](auto g, auto nv) {
                L::template launch<decltype(g)::value, decltype(nv)::value, decltype(VW)::value, decltype(MH)::value,
                                   decltype(DR)::value>(grid, st, a, x..., dm);
            });
        });
    };
    const bool ok = drop ? (heads == 1 ? ladder(std::false_type{}, std::true_type{}) : ladder(std::true_type{}, std::true_type{}))
                         : (heads == 1 ? ladder(std::false_type{}, std::false_type{}) : ladder(std::true_type{}, std::false_type{}));
    SGCN_REQUIRE(ok, "%s: no kernel for G=%d NV=%d", who, G, NV);
    SGCN_HIP_TRY(hipGetLastError());

    if (split) {
        SGCN_REQUIRE(plan->nfix < L::max_fix, "%s: too many split rows", who);
        L::fix(vw, a, plan, st, x...);
        SGCN_HIP_TRY(hipGetLastError());
    }
    return SGCN_OK;
}

// the forward's fix-up of both score kinds, one workgroup per split row: nvec <= 256 = kBlock threads
template <bool MH>
void launch_fix(int vw, const AttnArgs& a, const sgcn_plan_t* plan, hipStream_t st) {
    const dim3 grid((unsigned)plan->nfix), block(kBlock);
    with_vw(vw, [&](auto VW) {
        hipLaunchKernelGGL((spattn_fix_kernel<decltype(VW)::value, MH>), grid, block, 0, st, a, plan->dev_fix, plan->nfix);
    });
}
inline void launch_fwd_fix(int vw, const AttnArgs& a, const sgcn_plan_t* plan, hipStream_t st) {
    if (a.heads == 1) launch_fix<false>(vw, a, plan, st);
    else launch_fix<true>(vw, a, plan, st);
}

}  // namespace
}  // namespace sgcn
