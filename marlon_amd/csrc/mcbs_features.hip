// mcbs_features.hip — the policy's input features from the attacker wrapper's observation (include/mcbs.h "feature encoder").
//
// What Stable-Baselines3's "MultiInputPolicy" does first with the Dict observation of marlon's wrappers (preprocess_obs +
// CombinedExtractor; marlon/baseline_models/ppo/train.py:79): every Discrete(n) becomes a one-hot of n floats, every element of a
// MultiDiscrete(nvec) a one-hot of its own, every MultiBinary 0.0 / 1.0, concatenated in the Dict's key order into one [n, F] float
// row.  There it is a Python loop of split / one_hot / cat per element (224 of them for Chain-10 at 12/12); here it is ONE launch:
//     out[i, j] = 1 if column j's source value of row i equals column j's class, else 0        (one-hot columns)
//     out[i, j] = bit(i, first_bit + j - first_column)                                         (mask columns, from packed bits)
// The row layout is the caller's (marlon_amd/features.py builds it from the spaces): one 32-bit descriptor per one-hot column and up to
// three ranges of mask columns.  A 924-byte observation expands to 4 - 60 KB of features: DESIGN.md section 7 has the measurements.
#pragma once
#include "mcbs_device.h"
#include "mcbs_rowstore.h"

namespace mcbs {

// descriptor of a one-hot column: bits 0-15 its class, bits 16-30 the index of its source value in the row's int32 values (the five
// observation fields of mcbs_obs_buffers in that order, flattened), bit 31 set on the first column (class 0) of every element
constexpr uint32_t FEAT_MAX_SRC = 1u << 15, FEAT_MAX_CLASS = 1u << 16, FEAT_MAX_RANGES = 3u;

struct FeatGeom {
    uint32_t F, n_desc;                  // columns of a row, one-hot columns among them
    uint32_t V, W;                       // int32 values of a row (all five fields), mask words read per row (0: no mask columns)
    uint32_t len[5], off[5];             // ints per row of each observation field, its first index among the V values
    uint32_t n_ranges;                   // mask-column ranges, ascending by column
    uint32_t rc0[FEAT_MAX_RANGES], rn[FEAT_MAX_RANGES], rb0[FEAT_MAX_RANGES];     // first column, columns, first bit of the packed row
};
struct FeatSrc { const int32_t* f[5]; };                 // dense rows of len[k] ints each; a field the layout never reads may be NULL

// Does the whole group of GW columns from j0 lie inside one mask range?  Then m = its GW bits, taken from two words of the row's
// packed mask (word_at(w), w < W: the ranges' bits lie below 32 * W).
template <uint32_t GW, typename WordAt>
__device__ __forceinline__ bool feat_group_bits(const FeatGeom& G, uint32_t j0, WordAt word_at, uint32_t& m) {
    bool whole = false;
#pragma unroll
    for (uint32_t r = 0; r < FEAT_MAX_RANGES; ++r) {
        if (r < G.n_ranges && j0 >= G.rc0[r] && j0 + GW <= G.rc0[r] + G.rn[r]) {
            const uint32_t b = G.rb0[r] + (j0 - G.rc0[r]), w = b >> 5, s = b & 31u;
            uint32_t x = word_at(w) >> s;
            if (s + GW > 32u) x |= word_at(w + 1u) << (32u - s);
            m = x & ((1u << GW) - 1u);
            whole = true;
        }
    }
    return whole;
}

// Column j is a mask column (true: idx = its bit of the packed row) or a one-hot column (false: idx = j less the mask columns before
// it, its index among the one-hot columns)
__device__ __forceinline__ bool feat_column(const FeatGeom& G, uint32_t j, uint32_t& idx) {
    uint32_t before = 0, bit = ~0u;
#pragma unroll
    for (uint32_t r = 0; r < FEAT_MAX_RANGES; ++r) {
        if (r < G.n_ranges && j >= G.rc0[r]) {
            if (j - G.rc0[r] < G.rn[r]) bit = G.rb0[r] + (j - G.rc0[r]);
            else before += G.rn[r];
        }
    }
    idx = bit != ~0u ? bit : j - before;
    return bit != ~0u;
}

// T: uint32_t (fp32 patterns) or uint16_t (fp16 / bf16: `one` is the caller's bit pattern of 1.0).  GW columns = one store of
// GW * sizeof(T) bytes (16, 8 or 4); VEC = false stores element by element (16-bit rows on odd 2-byte boundaries).
//
// The fallback for layouts beyond the LDS budget of encode_features_rows_kernel below (very large topologies: Chain-100 at 102/102
// has 30 000 one-hot columns and 9.6 M mask bits), and the first form this encoder had: one WAVEFRONT per row, four per workgroup, a
// grid-stride loop over rows; every lane builds whole store groups, so that one store instruction of the wavefront covers 64 * GW
// consecutive columns.  A group that lies inside one mask range takes its GW bits from two words of the row's packed mask; any other
// group is evaluated column by column: descriptor, source value, one compare — all read from global memory (L1 / L2 hits: the table
// is shared by every row, a row's values are 1 - 70 KB).  Write-only: every column below F is stored, nothing from F on is touched.
// (With table, values and bits staged in LDS this form took 150 us for the headline batch's fp32 rows — some 40 vector instructions
// per column: ALU-bound — against 117 us for the per-element kernel.)
//
// out_of_range: an element whose value lies outside [0, classes) leaves its group all zero; since exactly one column of an in-range
// element is 1, the number of such elements in a row is (elements seen) - (ones written among the one-hot columns).  A wavefront owns
// whole rows, sums that over its lanes and rows, and one lane adds it with one atomicAdd when it is not zero.
template <typename T, uint32_t GW, bool VEC>
__global__ __launch_bounds__(256) void encode_features_kernel(FeatGeom G, FeatSrc src, const uint32_t* __restrict__ desc,
                                                              const uint32_t* __restrict__ bits, size_t bits_row_words, T* __restrict__ out,
                                                              size_t out_stride, uint64_t n_rows, T one, uint32_t* __restrict__ out_of_range) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t* D = desc;
    int32_t bad = 0;                                                 // elements seen - ones written, this lane
    for (uint64_t i = (uint64_t)blockIdx.x * 4u + wave; i < n_rows; i += (uint64_t)gridDim.x * 4u) {      // wave-uniform
        const uint32_t* brow = G.W ? bits + i * bits_row_words : nullptr;
        auto value_at = [&](uint32_t s) -> uint32_t {                // source value s of the row (s < V: checked when the layout is created)
            uint32_t k = 0;
#pragma unroll
            for (uint32_t q = 1; q < 5u; ++q) k += (uint32_t)(s >= G.off[q]);
            return (uint32_t)src.f[k][i * G.len[k] + (s - G.off[k])];
        };
        auto word_at = [&](uint32_t w) -> uint32_t {                 // (w < W: the ranges' bits lie below 32 * W)
            return brow[w];
        };
        T* row = out + i * out_stride;
        const uint32_t ngroup = (G.F + GW - 1u) / GW;
        for (uint32_t g = lane; g < ngroup; g += 64u) {
            const uint32_t j0 = g * GW;
            uint32_t m = 0;                                          // bit k: column j0 + k is 1
            if (!feat_group_bits<GW>(G, j0, word_at, m)) {
#pragma unroll
                for (uint32_t k = 0; k < GW; ++k) {
                    const uint32_t j = j0 + k;
                    if (j >= G.F) break;
                    uint32_t idx, on;
                    if (feat_column(G, j, idx)) {
                        on = (word_at(idx >> 5) >> (idx & 31u)) & 1u;
                    } else {
                        const uint32_t d = D[idx];
                        on = (uint32_t)(value_at((d >> 16) & (FEAT_MAX_SRC - 1u)) == (d & (FEAT_MAX_CLASS - 1u)));
                        bad += (int32_t)(d >> 31) - (int32_t)on;
                    }
                    m |= on << k;
                }
            }
            T v[GW];
#pragma unroll
            for (uint32_t k = 0; k < GW; ++k) v[k] = ((m >> k) & 1u) ? one : (T)0;
            store_group<T, GW, VEC>(row, j0, G.F, v);
        }
    }
    if (out_of_range) {                                              // uniform
#pragma unroll
        for (uint32_t d = 32u; d; d >>= 1) bad += __shfl_xor(bad, (int)d);
        if (lane == 0 && bad > 0) atomicAdd(out_of_range, (uint32_t)bad);
    }
}

// The kernel every layout that fits the LDS budget runs (Chain-10, ToyCtf and everything near them).  Evaluating columns one by one
// (descriptor, source value, compare: encode_features_kernel below) costs some 40 vector instructions per column and made the
// launch ALU-bound: 150 us for the 265 MB of the headline batch's fp32 rows, of which the stores need 40.  Here the one-hot part of
// a row is built the other way round, per ELEMENT: each wavefront keeps the row's one-hot columns as finished T patterns in LDS,
// clears them (16 bytes per lane and instruction), then every lane takes one source value straight from global memory (consecutive
// lanes, consecutive values: the elements are indexed by their source value), looks its element up — first one-hot column and class
// count, a table in LDS shared by the workgroup — and, if the value is below the class count, sets ONE column.  The output pass then
// copies 16 bytes per lane from LDS to the row (layouts without mask columns), or, with mask columns, builds whole-mask groups from
// the staged bit words and picks the others from the LDS row column by column.  A wavefront's LDS accesses execute in order, so the
// clearing store and the setting store of a column need no more than the compiler-level ordering the barriers give.
// out_of_range counts in the element pass: a value at or above its class count (negative ones are huge as unsigned).
// (Tried: the five fields as one index space in a loop unrolled four times, to put four loads per lane in flight: 162 against
// 118 us on the headline batch's fp32 rows.  Kept: one loop per field.)
template <typename T, uint32_t GW, bool VEC>
__global__ __launch_bounds__(256) void encode_features_rows_kernel(FeatGeom G, FeatSrc src, const uint2* __restrict__ elems,
                                                                   const uint32_t* __restrict__ bits, size_t bits_row_words, T* __restrict__ out,
                                                                   size_t out_stride, uint64_t n_rows, T one, uint32_t* __restrict__ out_of_range) {
    constexpr uint32_t PER = 16u / (uint32_t)sizeof(T);              // columns per 16 bytes
    extern __shared__ uint4 feat_rows_lds[];                         // elems [V] | per wavefront: one-hot row [n_desc] | bit words [W]
    const uint32_t ev4 = (G.V + 1u) / 2u, rv4 = (G.n_desc + PER - 1u) / PER, bv4 = (G.W + 3u) / 4u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint2* E = reinterpret_cast<uint2*>(feat_rows_lds);
    for (uint32_t i = threadIdx.x; i < G.V; i += 256u) E[i] = elems[i];
    uint4* row4 = feat_rows_lds + ev4 + wave * (rv4 + bv4);
    T* lrow = reinterpret_cast<T*>(row4);
    uint32_t* wbits = reinterpret_cast<uint32_t*>(row4 + rv4);
    __syncthreads();                                                 // (every thread of the workgroup gets here: rows are taken below)
    uint32_t bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 4u + wave; i < n_rows; i += (uint64_t)gridDim.x * 4u) {      // wave-uniform
        __builtin_amdgcn_wave_barrier();                             // (the previous row may still be in use by other lanes)
        for (uint32_t x = lane; x < rv4; x += 64u) row4[x] = make_uint4(0u, 0u, 0u, 0u);
        if (G.W) {
            const uint32_t* brow = bits + i * bits_row_words;
            for (uint32_t x = lane; x < G.W; x += 64u) wbits[x] = brow[x];
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
#pragma unroll
        for (uint32_t k = 0; k < 5u; ++k) {
            if (!src.f[k]) continue;                                 // uniform (no element of the layout reads this field)
            const int32_t* p = src.f[k] + i * G.len[k];
            for (uint32_t x = lane; x < G.len[k]; x += 64u) {
                const uint32_t v = (uint32_t)p[x];
                const uint2 e = E[G.off[k] + x];                     // (first one-hot column, classes); classes 0: not in the layout
                if (v < e.y) lrow[e.x + v] = one;
                else bad += (uint32_t)(e.y != 0u);
            }
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        T* row = out + i * out_stride;
        const uint32_t ngroup = (G.F + GW - 1u) / GW;
        if (G.n_ranges == 0u) {                                      // uniform: the row IS the LDS row
            for (uint32_t g = lane; g < ngroup; g += 64u) {
                const uint32_t j0 = g * GW;
                if (VEC && j0 + GW <= G.F) {                         // a whole group: GW * sizeof(T) bytes from LDS to the row as they are
                    constexpr uint32_t NB = GW * (uint32_t)sizeof(T);
                    if constexpr (NB == 16u) *reinterpret_cast<uint4*>(row + j0) = *reinterpret_cast<const uint4*>(lrow + j0);
                    else if constexpr (NB == 8u) *reinterpret_cast<uint2*>(row + j0) = *reinterpret_cast<const uint2*>(lrow + j0);
                    else *reinterpret_cast<uint32_t*>(row + j0) = *reinterpret_cast<const uint32_t*>(lrow + j0);
                } else {
#pragma unroll
                    for (uint32_t k = 0; k < GW; ++k)
                        if (j0 + k < G.F) row[j0 + k] = lrow[j0 + k];
                }
            }
        } else {
            for (uint32_t g = lane; g < ngroup; g += 64u) {
                const uint32_t j0 = g * GW;
                T v[GW];
                uint32_t m = 0;
                if (feat_group_bits<GW>(G, j0, [&](uint32_t w) { return wbits[w]; }, m)) {
#pragma unroll
                    for (uint32_t k = 0; k < GW; ++k) v[k] = ((m >> k) & 1u) ? one : (T)0;
                } else {
#pragma unroll
                    for (uint32_t k = 0; k < GW; ++k) {
                        const uint32_t j = j0 + k;
                        v[k] = (T)0;
                        if (j >= G.F) continue;
                        uint32_t idx;
                        if (feat_column(G, j, idx)) v[k] = ((wbits[idx >> 5] >> (idx & 31u)) & 1u) ? one : (T)0;
                        else v[k] = lrow[idx];
                    }
                }
                store_group<T, GW, VEC>(row, j0, G.F, v);
            }
        }
    }
    if (out_of_range) {                                              // uniform
#pragma unroll
        for (uint32_t d = 32u; d; d >>= 1) bad += __shfl_xor(bad, (int)d);
        if (lane == 0 && bad) atomicAdd(out_of_range, bad);
    }
}

} // namespace mcbs
