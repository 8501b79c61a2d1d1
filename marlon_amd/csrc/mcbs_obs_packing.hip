// mcbs_obs_packing.hip — the attacker observation's five int32 fields as bit fields (include/mcbs.h "packed observations"): pack the
// live observation per step, unpack stored rows, and encode feature rows straight from stored packed rows through a row index.
//
// Every one of a row's V values is a small enum or a count (Chain-10 at 12/12: 231 values of 2 - 4 bits, 924 B -> 18 words = 72 B), so
// a rollout buffer stores the packed row and the five int32 fields are never gathered: mcbs_encode_features_packed reads row
// index[i] of the storage itself.  One 32-bit descriptor per value, the table shared by all rows (obs_desc_* below); the word / shift
// rule is applied once on the host (mcbs_obs_packing_create).
#pragma once
#include "mcbs_device.h"
#include "mcbs_features.hip"
#include "mcbs_rowstore.h"

namespace mcbs {

// descriptor of a source value: bits 0-15 its valid codes n less one, bits 16-31 its first bit of the packed row (32 * word + shift);
// its width is bit_length(n), its out-of-range code n
constexpr uint32_t OBS_PACK_MAX_CODES = 1u << 16, OBS_PACK_MAX_WORDS = 1u << 11;
__host__ __device__ __forceinline__ uint32_t obs_desc_codes(uint32_t d) { return (d & 0xFFFFu) + 1u; }
__host__ __device__ __forceinline__ uint32_t obs_desc_bit(uint32_t d) { return d >> 16; }
__device__ __forceinline__ uint32_t obs_desc_mask(uint32_t d) { return (2u << (31u - (uint32_t)__clz((int)obs_desc_codes(d)))) - 1u; }   // bit_length(n) ones
// the code of the value described by d in the packed row `prow` (a field lies inside one word)
__device__ __forceinline__ uint32_t obs_decode(const uint32_t* __restrict__ prow, uint32_t d) {
    const uint32_t pos = obs_desc_bit(d);
    return (prow[pos >> 5] >> (pos & 31u)) & obs_desc_mask(d);
}
// Row index[i] (i itself without an index) of n_source_rows, as a wave-uniform value; false: outside the storage, nothing may be read
__device__ __forceinline__ bool obs_source_row(const int64_t* __restrict__ index, uint64_t i, uint64_t n_source_rows, uint64_t& src) {
    uint64_t r = i;
    if (index) {
        const uint64_t v = (uint64_t)index[i];                       // (negative: huge as unsigned)
        r = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)v);
    }
    src = r;
    return r < n_source_rows;
}

struct ObsPackGeom {
    uint32_t V, W;                       // int32 values of a row (all five fields), packed words of a row
    uint32_t len[5], off[5];             // ints per row of each observation field, its first index among the V values
};
struct ObsDst { int32_t* f[5]; };        // dense rows of len[k] ints each; NULL: not written

// x of lane + N within the lane's 16-lane row (DPP row_shl:N, no LDS traffic); `fallback` where that lane lies beyond the row
template <int N>
__device__ __forceinline__ uint32_t obs_row_next(uint32_t fallback, uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)fallback, (int)x, 0x100 + N, 0xF, 0xF, false);
}
constexpr uint32_t OBS_PACK_UNROLL = 4u, OBS_NO_WORD = ~0u;

// Pack is read-bound (924 B in, 72 B out per Chain-10 row).  One WAVEFRONT per row, four per workgroup, a grid-stride loop over rows:
// consecutive lanes load consecutive int32 values of the row (coalesced; the five fields as one index space, OBS_PACK_UNROLL loads per
// lane in flight: with one dependent load per lane the launch ran at 1.2 TB/s, bound by the bytes in flight), clamp them to their code
// and OR `code << shift` into the wavefront's copy of the row in LDS.  Up to 32 values share a word and the LDS serialises lanes that
// hit one word, so the lanes of a word are first OR-ed together in registers, 16-lane row by row; nothing goes through global memory
// and no global atomic touches the output.  The finished words leave with one coalesced store per 64 words, so every word below W is
// written whole and nothing else is.  A wavefront's LDS accesses execute in order: clearing, OR-ing and reading a word need no more
// than the compiler-level ordering of the wave barriers.
__global__ __launch_bounds__(256) void pack_observation_kernel(ObsPackGeom P, FeatSrc src, const uint32_t* __restrict__ pdesc,
                                                               uint32_t* __restrict__ out, size_t out_row_words, uint64_t n_rows,
                                                               uint32_t* __restrict__ out_of_range) {
    extern __shared__ uint32_t obs_pack_lds[];                       // per wavefront: the row's W words
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t* words = obs_pack_lds + wave * P.W;
    uint32_t bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 4u + wave; i < n_rows; i += (uint64_t)gridDim.x * 4u) {      // wave-uniform
        __builtin_amdgcn_wave_barrier();                             // (the previous row may still be read by other lanes)
        for (uint32_t x = lane; x < P.W; x += 64u) words[x] = 0u;
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        // the row's fields as one index space: value s of the row is element s of field k's row shifted down by off[k]
        const int32_t* fp[5];
#pragma unroll
        for (uint32_t k = 0; k < 5u; ++k) fp[k] = src.f[k] + i * P.len[k] - P.off[k];                      // uniform
        for (uint32_t s0 = 0; s0 < P.V; s0 += 64u * OBS_PACK_UNROLL) {
            uint32_t v[OBS_PACK_UNROLL], d[OBS_PACK_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < OBS_PACK_UNROLL; ++u) {         // every load of the pass is issued before the first use
                const uint32_t s = s0 + 64u * u + lane;
                const int32_t* p = fp[0];
#pragma unroll
                for (uint32_t k = 1; k < 5u; ++k) p = s >= P.off[k] ? fp[k] : p;
                v[u] = s < P.V ? (uint32_t)p[s] : 0u;
                d[u] = s < P.V ? pdesc[s] : 0u;
            }
#pragma unroll
            for (uint32_t u = 0; u < OBS_PACK_UNROLL; ++u) {
                const bool live = s0 + 64u * u + lane < P.V;
                const uint32_t n = obs_desc_codes(d[u]), pos = obs_desc_bit(d[u]);
                bad += (uint32_t)(live && v[u] >= n);                // (negative values are huge as unsigned)
                // consecutive lanes hold consecutive values, so the lanes of one word are one run: OR each run of a 16-lane row into
                // its first lane in registers, then one LDS OR per run instead of one per value
                const uint32_t w = live ? pos >> 5 : OBS_NO_WORD;
                uint32_t x = live ? (v[u] < n ? v[u] : n) << (pos & 31u) : 0u;
                x |= obs_row_next<1>(0u, x) & (uint32_t)-(int32_t)(obs_row_next<1>(OBS_NO_WORD, w) == w);
                x |= obs_row_next<2>(0u, x) & (uint32_t)-(int32_t)(obs_row_next<2>(OBS_NO_WORD, w) == w);
                x |= obs_row_next<4>(0u, x) & (uint32_t)-(int32_t)(obs_row_next<4>(OBS_NO_WORD, w) == w);
                x |= obs_row_next<8>(0u, x) & (uint32_t)-(int32_t)(obs_row_next<8>(OBS_NO_WORD, w) == w);
                const uint32_t before = (uint32_t)__builtin_amdgcn_update_dpp((int)OBS_NO_WORD, (int)w, 0x111, 0xF, 0xF, false);   // row_shr:1
                if (live && before != w) atomicOr(&words[w], x);
            }
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        uint32_t* row = out + i * out_row_words;
        for (uint32_t x = lane; x < P.W; x += 64u) row[x] = words[x];
    }
    if (out_of_range) {                                              // uniform
#pragma unroll
        for (uint32_t d = 32u; d; d >>= 1) bad += __shfl_xor(bad, (int)d);
        if (lane == 0 && bad) atomicAdd(out_of_range, bad);
    }
}

// The inverse: one wavefront per output row, lane x decodes value x of a field from the source row's words (72 B: L1 hits, lanes of
// one word read one address) and stores it, consecutive lanes to consecutive ints.  A source row outside the storage reads nothing:
// every value is its out-of-range code.
__global__ __launch_bounds__(256) void unpack_observation_kernel(ObsPackGeom P, const uint32_t* __restrict__ pdesc,
                                                                 const uint32_t* __restrict__ packed, size_t row_words,
                                                                 const int64_t* __restrict__ index, uint64_t n_source_rows, ObsDst dst,
                                                                 uint64_t n_rows) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t i = (uint64_t)blockIdx.x * 4u + wave; i < n_rows; i += (uint64_t)gridDim.x * 4u) {      // wave-uniform
        uint64_t s;
        const bool inside = obs_source_row(index, i, n_source_rows, s);
        const uint32_t* prow = inside ? packed + s * row_words : nullptr;
#pragma unroll
        for (uint32_t k = 0; k < 5u; ++k) {
            if (!dst.f[k]) continue;                                 // uniform
            int32_t* p = dst.f[k] + i * P.len[k];
            for (uint32_t x = lane; x < P.len[k]; x += 64u) {
                const uint32_t d = pdesc[P.off[k] + x];
                p[x] = (int32_t)(inside ? obs_decode(prow, d) : obs_desc_codes(d));
            }
        }
    }
}

// The output pass of the per-element form: the finished one-hot columns of a row (T patterns in LDS) and its staged mask words to the
// row in memory — 16 bytes per lane straight from LDS when the layout has no mask columns, else whole-mask groups from the bit words and
// the others picked column by column.  (encode_features_rows_kernel keeps its own inline copy of this pass: the existing kernels'
// code is left exactly as it is.)
template <typename T, uint32_t GW, bool VEC>
__device__ __forceinline__ void feat_store_lds_row(const FeatGeom& G, const T* lrow, const uint32_t* wbits, T* __restrict__ row, T one, uint32_t lane) {
    const uint32_t ngroup = (G.F + GW - 1u) / GW;
    if (G.n_ranges == 0u) {                                          // uniform: the row IS the LDS row
        for (uint32_t g = lane; g < ngroup; g += 64u) {
            const uint32_t j0 = g * GW;
            if (VEC && j0 + GW <= G.F) {                             // a whole group: GW * sizeof(T) bytes from LDS to the row as they are
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
        return;
    }
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

// The packed encoder every layout that fits the LDS budget runs (Chain-10, ToyCtf and everything near them): the per-ELEMENT form of
// encode_features_rows_kernel on packed rows.  Each wavefront keeps the row's one-hot columns as finished T patterns in LDS, clears
// them, then every lane decodes one value of source row index[i] (the packed row is 72 B: L1 hits, lanes of one word read one address),
// looks its element up — first one-hot column and class count, a table in LDS shared by the workgroup — and sets ONE column where the
// code is below the class count; the out-of-range code never is.  The column-by-column kernel below costs some 40 vector instructions
// per column and took 35 / 43 us for a 16 384-row Chain-10 minibatch in fp32 / bf16 (profiles/obs_packing.md).
template <typename T, uint32_t GW, bool VEC>
__global__ __launch_bounds__(256) void encode_features_packed_rows_kernel(FeatGeom G, const uint2* __restrict__ elems, uint32_t n_elements,
                                                                          const uint32_t* __restrict__ pdesc, const uint32_t* __restrict__ packed,
                                                                          size_t packed_row_words, const uint32_t* __restrict__ bits,
                                                                          size_t bits_row_words, const int64_t* __restrict__ index,
                                                                          uint64_t n_source_rows, T* __restrict__ out, size_t out_stride,
                                                                          uint64_t n_rows, T one, uint32_t* __restrict__ out_of_range) {
    constexpr uint32_t PER = 16u / (uint32_t)sizeof(T);              // columns per 16 bytes
    extern __shared__ uint4 obs_rows_lds[];                          // elems [V] | per wavefront: one-hot row [n_desc] | bit words [W]
    const uint32_t ev4 = (G.V + 1u) / 2u, rv4 = (G.n_desc + PER - 1u) / PER, bv4 = (G.W + 3u) / 4u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint2* E = reinterpret_cast<uint2*>(obs_rows_lds);
    for (uint32_t i = threadIdx.x; i < G.V; i += 256u) E[i] = elems[i];
    uint4* row4 = obs_rows_lds + ev4 + wave * (rv4 + bv4);
    T* lrow = reinterpret_cast<T*>(row4);
    uint32_t* wbits = reinterpret_cast<uint32_t*>(row4 + rv4);
    __syncthreads();                                                 // (every thread of the workgroup gets here: rows are taken below)
    uint32_t bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 4u + wave; i < n_rows; i += (uint64_t)gridDim.x * 4u) {      // wave-uniform
        T* row = out + i * out_stride;
        uint64_t s;
        const bool inside = obs_source_row(index, i, n_source_rows, s);          // uniform
        __builtin_amdgcn_wave_barrier();                             // (the previous row may still be in use by other lanes)
        for (uint32_t x = lane; x < rv4; x += 64u) row4[x] = make_uint4(0u, 0u, 0u, 0u);
        if (G.W) {                                                   // (a row outside the storage: all-zero mask words, nothing read)
            const uint32_t* brow = bits + s * bits_row_words;
            for (uint32_t x = lane; x < G.W; x += 64u) wbits[x] = inside ? brow[x] : 0u;
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        if (inside) {
            const uint32_t* prow = packed + s * packed_row_words;
            for (uint32_t x = lane; x < G.V; x += 64u) {
                const uint32_t code = obs_decode(prow, pdesc[x]);
                const uint2 e = E[x];                                // (first one-hot column, classes); classes 0: not in the layout
                if (code < e.y) lrow[e.x + code] = one;
                else bad += (uint32_t)(e.y != 0u);
            }
        } else if (lane == 0) {
            bad += n_elements;
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        feat_store_lds_row<T, GW, VEC>(G, lrow, wbits, row, one, lane);
    }
    if (out_of_range) {                                              // uniform
#pragma unroll
        for (uint32_t d = 32u; d; d >>= 1) bad += __shfl_xor(bad, (int)d);
        if (lane == 0 && bad) atomicAdd(out_of_range, bad);
    }
}

// The packed encoder of every other layout (the one-hot rows of four wavefronts beyond the LDS budget: Chain-100 at 102/102 has 30 000
// columns; or two elements sharing a value): the column body of encode_features_kernel (whole-mask groups from two bit words, any other
// group column by column: descriptor, source value, one compare; the row-store side of mcbs_rowstore.h) on values that each wavefront
// first decodes ONCE per row into LDS, lane x value x (STAGED; 4 * V bytes per wavefront: Chain-10 924 B, Chain-100 at 102/102 7 KB).
// Layouts whose four rows of values exceed the LDS budget decode every value where a column asks for it instead (!STAGED: the packed
// row is a few hundred bytes of L1 hits).  The source row of output row i is index[i] of `packed` and of `bits` alike — the gather of a
// minibatch happens here, no int32 field is ever materialised; a row index outside the storage reads nothing and writes the row all
// zero, every element of it counted as out of range.  Write-only like the parent: every column below F is stored, nothing from F on.
template <typename T, uint32_t GW, bool VEC, bool STAGED>
__global__ __launch_bounds__(256) void encode_features_packed_kernel(FeatGeom G, const uint32_t* __restrict__ desc, uint32_t n_elements,
                                                                     const uint32_t* __restrict__ pdesc, const uint32_t* __restrict__ packed,
                                                                     size_t packed_row_words, const uint32_t* __restrict__ bits,
                                                                     size_t bits_row_words, const int64_t* __restrict__ index,
                                                                     uint64_t n_source_rows, T* __restrict__ out, size_t out_stride,
                                                                     uint64_t n_rows, T one, uint32_t* __restrict__ out_of_range) {
    extern __shared__ uint32_t obs_values_lds[];                     // STAGED: per wavefront the row's V codes
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t* vals = obs_values_lds + (STAGED ? wave * G.V : 0u);
    const uint32_t ngroup = (G.F + GW - 1u) / GW;
    int32_t bad = 0;                                                 // elements seen - ones written, this lane
    for (uint64_t i = (uint64_t)blockIdx.x * 4u + wave; i < n_rows; i += (uint64_t)gridDim.x * 4u) {      // wave-uniform
        T* row = out + i * out_stride;
        uint64_t s;
        if (!obs_source_row(index, i, n_source_rows, s)) {           // uniform
            T z[GW];
#pragma unroll
            for (uint32_t k = 0; k < GW; ++k) z[k] = (T)0;
            for (uint32_t g = lane; g < ngroup; g += 64u) store_group<T, GW, VEC>(row, g * GW, G.F, z);
            if (lane == 0) bad += (int32_t)n_elements;
            continue;
        }
        const uint32_t* prow = packed + s * packed_row_words;
        const uint32_t* brow = G.W ? bits + s * bits_row_words : nullptr;
        if constexpr (STAGED) {
            __builtin_amdgcn_wave_barrier();                         // (the previous row may still be read by other lanes)
            for (uint32_t x = lane; x < G.V; x += 64u) vals[x] = obs_decode(prow, pdesc[x]);
            __builtin_amdgcn_wave_barrier();
            __threadfence_block();
        }
        auto value_at = [&](uint32_t x) -> uint32_t {                // code of source value x (x < V: checked when the layout is created)
            if constexpr (STAGED) return vals[x];
            else return obs_decode(prow, pdesc[x]);
        };
        auto word_at = [&](uint32_t w) -> uint32_t { return brow[w]; };       // (w < W: the ranges' bits lie below 32 * W)
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
                        const uint32_t d = desc[idx];
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

} // namespace mcbs
