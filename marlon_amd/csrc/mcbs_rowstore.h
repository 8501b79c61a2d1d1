// mcbs_rowstore.h — writing [rows, A] rows in groups of one vector store: the store side shared by mask_logits_kernel,
// apply_packed_kernel, masked_categorical_grad_kernel and the two feature kernels.
//
// A GROUP is GW consecutive elements of a row = one store of GW * sizeof(T) bytes (16, or 8 where the rows are only 8-byte aligned:
// Chain-10's 14 172 bf16 actions; the feature rows also have 4-byte groups).  VEC = false: the row's base or stride is not aligned to
// the group, everything is stored element by element.  One wavefront owns a row; lane k of it takes group k of a SPAN = the 64 groups
// one store instruction of the wavefront covers.  Spans start on 128-byte lines of MEMORY, not of the row (rows are only 16- or
// 8-byte aligned: Chain-10's fp32 row is 56 688 B): the row's groups are shifted down by `sh`, so that every store instruction writes
// whole lines and no line is shared by two instructions; the first span is short.  All of it is write-only: nothing here reads the row.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace mcbs {

// float -> bfloat16 pattern, round to nearest even; NaN stays a quiet NaN
__host__ __device__ __forceinline__ uint32_t bf16_bits(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// Group geometry of a row of A elements.  The kernels keep their own loops (chunks of 64 spans, a window of mask words, a plain span
// loop) and take the arithmetic from here: span j, lane l -> g = 64 j + l, the group starts at element a0(g, sh).
template <typename LT, uint32_t GW, bool VEC>
struct RowGroups {
    static constexpr uint32_t GB = GW * (uint32_t)sizeof(LT);       // bytes per group
    static constexpr uint32_t NWORD = GB / 4u;                      // dwords per group: 4 or 2
    static_assert(NWORD == 4u || NWORD == 2u, "group = 16 or 8 bytes");
    static constexpr uint32_t ALL = (1u << GW) - 1u;

    static __device__ __forceinline__ uint32_t shift(const LT* row) {        // groups between the row's base and the 128-byte line before it
        return VEC ? (uint32_t)((reinterpret_cast<uintptr_t>(row) / GB) % (128u / GB)) : 0u;
    }
    static __device__ __forceinline__ uint32_t nspan(uint32_t A, uint32_t sh) { return ((A + GW - 1u) / GW + sh + 63u) / 64u; }
    static __device__ __forceinline__ uint32_t a0(uint32_t g, uint32_t sh) { return (g - sh) * GW; }
    // the first span's head, the last span's tail: no group of the row
    static __device__ __forceinline__ bool outside(uint32_t g, uint32_t sh, uint32_t A) { return g < sh || a0(g, sh) >= A; }
    // the elements [first, last) of span j that lie in the row
    static __device__ __forceinline__ uint32_t span_first(uint32_t j, uint32_t sh) { return (j * 64u > sh ? j * 64u - sh : 0u) * GW; }
    static __device__ __forceinline__ uint32_t span_last(uint32_t j, uint32_t sh, uint32_t A) { return (j * 64u + 64u - sh) * GW < A ? (j * 64u + 64u - sh) * GW : A; }
    static __device__ __forceinline__ uint32_t in_row(uint32_t a0, uint32_t A) { return a0 + GW <= A ? ALL : (1u << (A - a0)) - 1u; }    // bit k: a0 + k < A
};

// row[a0 + k] = fill under the bits of `off`: a group that is replaced as a whole is ONE vector store, a mixed group is stored element
// by element, elements under clear bits are left alone
template <typename LT, uint32_t GW, bool VEC>
__device__ __forceinline__ void store_fill_group(LT* __restrict__ row, uint32_t a0, uint32_t off, LT fill) {
    using RG = RowGroups<LT, GW, VEC>;
    if (VEC && off == RG::ALL) {
        if constexpr (sizeof(LT) == 4) {
            const uint32_t f = __float_as_uint(fill);
            *reinterpret_cast<uint4*>(row + a0) = make_uint4(f, f, f, f);
        } else {
            const uint32_t f = (uint32_t)fill, ff = f | (f << 16);
            if constexpr (RG::NWORD == 4u) *reinterpret_cast<uint4*>(row + a0) = make_uint4(ff, ff, ff, ff);
            else *reinterpret_cast<uint2*>(row + a0) = make_uint2(ff, ff);
        }
    } else if (off) {
#pragma unroll
        for (uint32_t k = 0; k < GW; ++k)
            if ((off >> k) & 1u) row[a0 + k] = fill;
    }
}

// One group built in registers (T = uint32_t or uint16_t patterns) to row[a0 ..]: one 16-, 8- or 4-byte store when the group is whole,
// element by element below `limit` at the row's end (and always without VEC)
template <typename T, uint32_t GW, bool VEC>
__device__ __forceinline__ void store_group(T* __restrict__ row, uint32_t a0, uint32_t limit, const T (&v)[GW]) {
    constexpr uint32_t NB = GW * (uint32_t)sizeof(T);                // bytes per group
    static_assert(NB == 16u || NB == 8u || NB == 4u || !VEC, "a group is one 16-, 8- or 4-byte store");
    if (VEC && a0 + GW <= limit) {
        auto w = [&](uint32_t k) -> uint32_t {                       // dword k of the group
            if constexpr (sizeof(T) == 4) return (uint32_t)v[k];
            else return (uint32_t)v[2u * k] | ((uint32_t)v[2u * k + 1u] << 16);
        };
        if constexpr (NB == 16u) *reinterpret_cast<uint4*>(row + a0) = make_uint4(w(0), w(1), w(2), w(3));
        else if constexpr (NB == 8u) *reinterpret_cast<uint2*>(row + a0) = make_uint2(w(0), w(1));
        else *reinterpret_cast<uint32_t*>(row + a0) = w(0);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < GW; ++k)
            if (a0 + k < limit) row[a0 + k] = v[k];
    }
}

} // namespace mcbs
