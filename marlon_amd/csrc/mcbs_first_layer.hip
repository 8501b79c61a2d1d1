// mcbs_first_layer.hip — the policy's first Linear layer straight from the observation, and its gradient (include/mcbs.h "first layer
// from the observation").
//
// The feature row mcbs_encode_features writes holds exactly one 1 per one-hot element, so Linear(F, H) on it is the bias plus one
// column of the weight matrix per element, selected by the element's source value: a gather-and-add over the [F, H] table (Chain-10 at
// 12/12: 231 elements in 1 012 columns, 259 KB of fp32 weights at H = 64).  No [n, F] feature tensor exists, and the source values come
// either from the five dense int32 fields (FeatSrc, as mcbs_encode_features reads them) or from stored packed rows through a row index
// (obs_decode / obs_source_row of mcbs_obs_packing.hip).  The gradient is the mirror image: a row's upstream gradient is added into
// the weight columns that row selected.
//
// The elements are walked in ROW ORDER (ascending first column), one float32 add each into ONE accumulator: the table below, built
// when the layout is created, lists them that way whatever order their source values have in the observation.
#pragma once
#include <type_traits>

#include "mcbs_device.h"
#include "mcbs_features.hip"
#include "mcbs_obs_packing.hip"
#include "mcbs_rowstore.h"

namespace mcbs {

// one entry per one-hot element, in row order: x = its first column c_e, y = its classes k_e, z = the index of its source value
using FlElem = uint4;
constexpr uint32_t FL_NONE = ~0u;                                    // "selects no column": the value lay outside [0, k_e)

// the source of a row's values, either form
struct FlSrc {
    FeatSrc dense;                       // dense form: the five int32 fields
    const uint32_t* pdesc;               // packed form: the packing's descriptors [V],
    const uint32_t* packed;              //   the stored rows,
    size_t packed_row_words;
    const int64_t* index;                //   the optional row index [n_rows]
    uint64_t n_source_rows;
};

__device__ __forceinline__ float fl_widen(float w) { return w; }
__device__ __forceinline__ float fl_widen(uint16_t w) { return __uint_as_float((uint32_t)w << 16); }             // bfloat16 widens exactly
__device__ __forceinline__ void fl_narrow(float* p, float v) { *p = v; }
__device__ __forceinline__ void fl_narrow(uint16_t* p, float v) { *p = (uint16_t)bf16_bits(v); }                 // round to nearest even

// source value s of dense row i (s < V; the field a layout's element reads is never NULL: checked on the host)
__device__ __forceinline__ uint32_t fl_dense_value(const FeatGeom& G, const FeatSrc& src, uint64_t i, uint32_t s) {
    const int32_t* p = src.f[0] + i * G.len[0];
#pragma unroll
    for (uint32_t k = 1; k < 5u; ++k) p = s >= G.off[k] ? src.f[k] + i * G.len[k] - G.off[k] : p;
    return (uint32_t)p[s];
}

// ---- forward ----
// A workgroup owns FL_ROWS consecutive rows and 64 of the H outputs (lane = h); each of its four wavefronts keeps FL_RPW rows'
// accumulators in registers.  The table is walked in SLABS of whole elements in row order — at most 64 elements and FL_SLAB_COLS
// columns, so a slab's [columns, 64] weights sit in 32 KB of LDS as float32 — and every wavefront adds the slab's selected columns to
// its rows before the next slab is staged: one trip of the table from L2 per 64 rows instead of one per row.  Within a slab lane l
// works out which column element l selects for each of the wavefront's rows (values read lane-parallel: consecutive elements mostly
// read consecutive values), and the add loop takes that column back as a wave-uniform value (v_readlane): one LDS read of 64
// consecutive floats and one add per (row, element), FL_RPW independent chains in flight.  An element that selects nothing reads the
// slab's spare column of -0.0 instead of branching: x + (-0.0) is x bit for bit for every x (a -0.0 bias stays -0.0), so the add loop
// has no branch and the FL_RPW reads of an element are issued together (with a branch per add every read waited for the LDS: 306 us
// for the headline batch at H = 64).  The order within a row is the contract's: slabs, and elements inside a slab, ascend in row
// order.  An element with more classes than a slab holds is a slab of its own whose selected column is read from memory (DIRECT):
// tables of any width are served, the wide ones slowly.
constexpr uint32_t FL_RPW = 16u, FL_WAVES = 4u, FL_ROWS = FL_RPW * FL_WAVES, FL_SLAB_COLS = 128u, FL_STAGE = 16u;

template <typename WT, typename OT, bool PACKED>
__global__ __launch_bounds__(256) void first_layer_kernel(FeatGeom G, FlSrc S, const FlElem* __restrict__ elems, uint32_t n_elements,
                                                          const WT* __restrict__ weight_t, size_t weight_stride, const WT* __restrict__ bias,
                                                          uint32_t H, OT* __restrict__ out, size_t out_stride, uint64_t n_rows,
                                                          uint32_t* __restrict__ out_of_range) {
    __shared__ float slab[(FL_SLAB_COLS + 1u) * 64u];               // column FL_SLAB_COLS: -0.0, what "nothing selected" adds
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (threadIdx.x < 64u) slab[FL_SLAB_COLS * 64u + threadIdx.x] = -0.0f;                   // (read after the loop's barriers)
    const uint32_t hbase = blockIdx.y * 64u, h = hbase + lane;
    const bool live_h = h < H;
    const uint64_t row0 = ((uint64_t)blockIdx.x * FL_WAVES + wave) * FL_RPW;                 // wave-uniform
    const bool count = out_of_range != nullptr && blockIdx.y == 0u;                          // one h-chunk counts

    // the wavefront's rows: lane r < FL_RPW looks up row r's source row once
    uint32_t src_lo = 0, src_hi = 0, src_ok = 0;
    {
        const uint64_t i = row0 + lane;
        if (lane < FL_RPW && i < n_rows) {
            uint64_t s = i;
            if (PACKED && S.index) s = (uint64_t)S.index[i];         // (negative: huge as unsigned)
            src_lo = (uint32_t)s; src_hi = (uint32_t)(s >> 32);
            src_ok = PACKED ? (uint32_t)(s < S.n_source_rows) : 1u;
        }
    }
    float acc[FL_RPW];
    const float b0 = bias && live_h ? fl_widen(bias[h]) : 0.0f;
#pragma unroll
    for (uint32_t r = 0; r < FL_RPW; ++r) acc[r] = b0;
    uint32_t bad = 0;

    for (uint32_t e0 = 0; e0 < n_elements;) {                        // uniform over the workgroup: a function of the layout alone
        const uint32_t e = e0 + lane;
        const FlElem el = e < n_elements ? elems[e] : make_uint4(0u, 0u, 0u, 0u);
        const uint32_t c_first = __builtin_amdgcn_readfirstlane(el.x);
        const uint64_t fits = __ballot(e < n_elements && el.x + el.y - c_first <= FL_SLAB_COLS);       // a prefix: columns ascend
        uint32_t n = ~fits ? (uint32_t)__builtin_ctzll(~fits) : 64u;
        const bool direct = n == 0u;                                 // element e0 alone is wider than a slab
        n = direct ? 1u : n;
        const uint32_t c_end = __builtin_amdgcn_readfirstlane(__shfl(el.x + el.y, (int)(n - 1u)));
        const uint32_t ncols = direct ? 0u : c_end - c_first;

        __syncthreads();                                             // (the slab before this one is no longer read)
        // four columns per pass and wavefront, FL_STAGE passes' loads in flight before the first is stored (one load at a time left
        // the 32 passes of a full slab waiting for L2 one after the other)
        for (uint32_t x0 = threadIdx.x; x0 < ncols * 64u; x0 += 256u * FL_STAGE) {
            const uint32_t hh = hbase + (x0 & 63u);                  // (x0 + 256 u names the same h)
            float w[FL_STAGE];
#pragma unroll
            for (uint32_t u = 0; u < FL_STAGE; ++u) {
                const uint32_t x = x0 + 256u * u;
                w[u] = x < ncols * 64u && hh < H ? fl_widen(weight_t[(size_t)(c_first + (x >> 6)) * weight_stride + hh]) : 0.0f;
            }
#pragma unroll
            for (uint32_t u = 0; u < FL_STAGE; ++u)
                if (x0 + 256u * u < ncols * 64u) slab[x0 + 256u * u] = w[u];
        }
        __syncthreads();

        // lane l: the column element e0 + l selects in each of the wavefront's rows (staged: as the slab's float index of its h = 0)
        uint32_t sel[FL_RPW];
        const uint32_t none = direct ? FL_NONE : FL_SLAB_COLS * 64u;
        const uint32_t pd = PACKED && lane < n ? S.pdesc[el.z] : 0u;
#pragma unroll
        for (uint32_t r = 0; r < FL_RPW; ++r) {
            const uint64_t i = row0 + r;
            sel[r] = none;
            if (i >= n_rows) continue;                               // uniform
            uint32_t v = FL_NONE;
            if constexpr (PACKED) {
                const uint64_t s = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)src_hi, (int)r) << 32) |
                                   (uint32_t)__builtin_amdgcn_readlane((int)src_lo, (int)r);
                if (__builtin_amdgcn_readlane((int)src_ok, (int)r) && lane < n)              // a row outside the storage reads nothing
                    v = obs_decode(S.packed + s * S.packed_row_words, pd);
            } else {
                if (lane < n) v = fl_dense_value(G, S.dense, i, el.z);
            }
            if (lane < n) {
                if (v < el.y) sel[r] = direct ? el.x + v : (el.x - c_first + v) * 64u;       // (negative values are huge as unsigned)
                else bad += 1u;
            }
        }
        if (direct) {
            for (uint32_t j = 0; j < n; ++j) {
#pragma unroll
                for (uint32_t r = 0; r < FL_RPW; ++r) {
                    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)sel[r], (int)j);
                    if (c != FL_NONE && live_h) acc[r] = acc[r] + fl_widen(weight_t[(size_t)c * weight_stride + h]);
                }
            }
        } else {
            for (uint32_t j = 0; j < n; ++j) {
#pragma unroll
                for (uint32_t r = 0; r < FL_RPW; ++r) {
                    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)sel[r], (int)j);
                    acc[r] = acc[r] + slab[c + lane];                // c / 64 < ncols <= FL_SLAB_COLS, or the -0.0 column
                }
            }
        }
        e0 += n;
    }
    if (live_h) {
#pragma unroll
        for (uint32_t r = 0; r < FL_RPW; ++r)
            if (row0 + r < n_rows) fl_narrow(out + (row0 + r) * out_stride + h, acc[r]);
    }
    if (count) {                                                     // uniform
#pragma unroll
        for (uint32_t d = 32u; d; d >>= 1) bad += __shfl_xor(bad, (int)d);
        if (lane == 0 && bad) atomicAdd(out_of_range, bad);
    }
}

// ---- gradient ----
// Distinct elements own disjoint column ranges, so different wavefronts add into different columns and nothing conflicts: a
// WAVEFRONT owns FLG_EPW consecutive elements, one block of MCBS_FIRST_LAYER_GRAD_ROW_BLOCK rows and 64 of the H outputs (lane = h), and
// walks the block's rows in ascending order: one coalesced read of the row's 64 gradients, then one add into the column each of its
// elements selects — `s = s + g`, started at +0.0, the contract's order.  The columns live in the wavefront's own 24 KB of LDS when
// its elements have at most FLG_WAVE_COLS of them (every layout near Chain-10 and ToyCtf: four credentials of Chain-10's cache matrix
// are 80 columns; with room for 48 the wavefronts of such elements fell to the other path and set the launch's time), else in the
// block's partial in the workspace itself (the same lane reads and writes an address: program order).  Which column a row selects is worked out for 64 rows
// at a time, lane = row, and taken back as a wave-uniform value in the row loop.  The wavefront of the first elements also sums the
// bias gradient of its block.  No wavefront waits for another: there is no barrier.  Partials [n_blocks][F + 1][H] (row F: the
// bias); first_layer_grad_reduce_kernel adds them in ascending block order.
constexpr uint32_t FLG_EPW = 8u, FLG_WAVES = 4u, FLG_WAVE_COLS = 88u, FLG_SUB = 16u, FLG_ROW_BLOCK = 512u;

template <bool PACKED>
__global__ __launch_bounds__(256) void first_layer_grad_kernel(FeatGeom G, FlSrc S, const FlElem* __restrict__ elems, uint32_t n_elements,
                                                               uint32_t n_slabs, const float* __restrict__ grad_out, size_t grad_stride,
                                                               uint32_t H, float* __restrict__ partials, uint64_t n_rows, bool do_weight,
                                                               bool do_bias) {
    __shared__ float cols[FLG_WAVES][(FLG_WAVE_COLS + FLG_EPW) * 64u];     // per wavefront: its columns, then a spare one per element
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t blk = blockIdx.x / n_slabs, slab = blockIdx.x % n_slabs;
    const uint32_t h = blockIdx.y * 64u + lane;
    const bool live_h = h < H;
    const uint32_t eb = (slab * FLG_WAVES + wave) * FLG_EPW;
    const uint32_t ne = do_weight && eb < n_elements ? (n_elements - eb < FLG_EPW ? n_elements - eb : FLG_EPW) : 0u;
    const bool bias_duty = do_bias && slab == 0u && wave == 0u;
    if (ne == 0u && !bias_duty) return;                              // (no barrier below)
    const uint32_t F = G.F;
    float* part = partials + (size_t)blk * (F + 1u) * H;             // this block's [F + 1, H]
    const uint64_t i_begin = (uint64_t)blk * FLG_ROW_BLOCK;
    const uint64_t i_end = i_begin + FLG_ROW_BLOCK < n_rows ? i_begin + FLG_ROW_BLOCK : n_rows;

    FlElem el[FLG_EPW];
    uint32_t pd[FLG_EPW];
#pragma unroll
    for (uint32_t j = 0; j < FLG_EPW; ++j) {                         // uniform
        el[j] = j < ne ? elems[eb + j] : make_uint4(0u, 0u, 0u, 0u);
        pd[j] = PACKED && j < ne ? S.pdesc[el[j].z] : 0u;
    }
    const uint32_t c_lo = el[0].x;
    uint32_t c_hi = c_lo;
#pragma unroll
    for (uint32_t j = 0; j < FLG_EPW; ++j) c_hi = j < ne ? el[j].x + el[j].y : c_hi;
    const uint32_t ncols = c_hi - c_lo;

    // acc[c * stride]: column c_lo + c of this lane's h.  FAST: the columns are the wavefront's LDS, with a spare column per element
    // that takes the adds of the rows in which the element selects nothing, so that a row is FLG_EPW reads, then FLG_EPW writes to
    // distinct addresses with no branch, and the gradients of FLG_SUB rows are loaded ahead (with a branch and a load per row every
    // LDS and memory latency of the walk was exposed: 974 us for a 16 384-row Chain-10 minibatch at H = 64).
    auto walk = [&](float* acc, size_t stride, auto fast) {
        constexpr bool FAST = decltype(fast)::value;
        const bool mine = FAST || live_h;
        if (mine)
            for (uint32_t c = 0; c < ncols; ++c) acc[c * stride] = 0.0f;
        if constexpr (FAST) {
#pragma unroll
            for (uint32_t j = 0; j < FLG_EPW; ++j) acc[(FLG_WAVE_COLS + j) * stride] = 0.0f;
        }
        float bsum = 0.0f;
        for (uint64_t i0 = i_begin; i0 < i_end; i0 += 64u) {
            const uint64_t i = i0 + lane;
            uint64_t s = i;
            bool inside = i < i_end;
            if (PACKED && inside) {
                if (S.index) s = (uint64_t)S.index[i];               // (negative: huge as unsigned)
                inside = s < S.n_source_rows;                        // a row outside the storage selects nothing and reads nothing
            }
            uint32_t sel[FLG_EPW];
#pragma unroll
            for (uint32_t j = 0; j < FLG_EPW; ++j) {
                sel[j] = FAST ? FLG_WAVE_COLS + j : FL_NONE;
                if (j < ne && inside) {
                    uint32_t v;
                    if constexpr (PACKED) v = obs_decode(S.packed + s * S.packed_row_words, pd[j]);
                    else v = fl_dense_value(G, S.dense, i, el[j].z);
                    if (v < el[j].y) sel[j] = el[j].x - c_lo + v;
                }
            }
            if constexpr (FAST) {
                for (uint32_t r0 = 0; r0 < 64u && i0 + r0 < i_end; r0 += FLG_SUB) {          // uniform
                    float g[FLG_SUB];
#pragma unroll
                    for (uint32_t q = 0; q < FLG_SUB; ++q)           // (a row past the block's end: +0.0 into the spare columns)
                        g[q] = live_h && i0 + r0 + q < i_end ? grad_out[(i0 + r0 + q) * grad_stride + h] : 0.0f;
#pragma unroll
                    for (uint32_t q = 0; q < FLG_SUB; ++q) {
                        bsum = bsum + g[q];
                        uint32_t c[FLG_EPW];
                        float a[FLG_EPW];
#pragma unroll
                        for (uint32_t j = 0; j < FLG_EPW; ++j) c[j] = (uint32_t)__builtin_amdgcn_readlane((int)sel[j], (int)(r0 + q)) * 64u;
#pragma unroll
                        for (uint32_t j = 0; j < FLG_EPW; ++j) a[j] = acc[c[j]];             // c / 64 < FLG_WAVE_COLS + FLG_EPW, all distinct
#pragma unroll
                        for (uint32_t j = 0; j < FLG_EPW; ++j) acc[c[j]] = a[j] + g[q];
                    }
                }
            } else {
                const uint32_t nr = i_end - i0 < 64u ? (uint32_t)(i_end - i0) : 64u;
                for (uint32_t r = 0; r < nr; ++r) {
                    const float g = live_h ? grad_out[(i0 + r) * grad_stride + h] : 0.0f;
                    bsum = bsum + g;
#pragma unroll
                    for (uint32_t j = 0; j < FLG_EPW; ++j) {
                        const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)sel[j], (int)r);
                        if (c != FL_NONE && mine) acc[c * stride] = acc[c * stride] + g;     // c < ncols
                    }
                }
            }
        }
        return bsum;
    };
    float bsum;
    if (ncols <= FLG_WAVE_COLS) {
        float* acc = &cols[wave][lane];
        bsum = walk(acc, 64u, std::true_type{});
        if (live_h)
            for (uint32_t c = 0; c < ncols; ++c) part[(size_t)(c_lo + c) * H + h] = acc[c * 64u];
    } else {
        bsum = walk(part + (size_t)c_lo * H + h, H, std::false_type{});
    }
    if (bias_duty && live_h) part[(size_t)F * H + h] = bsum;
}

// grad_weight_t[c, h] / grad_bias[h] = the block partials added in ascending block order, starting FROM partial 0; without a block
// (n_rows == 0) +0.0.  One thread per (c, h), consecutive threads consecutive h.
__global__ __launch_bounds__(256) void first_layer_grad_reduce_kernel(const float* __restrict__ partials, uint32_t n_blocks, uint32_t F, uint32_t H,
                                                                      float* __restrict__ grad_weight_t, size_t grad_weight_stride,
                                                                      float* __restrict__ grad_bias) {
    const uint64_t first = grad_weight_t ? 0u : (uint64_t)F * H, last = ((uint64_t)F + (grad_bias ? 1u : 0u)) * H;
    const size_t per_block = ((size_t)F + 1u) * H;
    for (uint64_t x = first + (uint64_t)blockIdx.x * 256u + threadIdx.x; x < last; x += (uint64_t)gridDim.x * 256u) {
        float s = 0.0f;
        if (n_blocks) s = partials[x];
        for (uint32_t b = 1; b < n_blocks; ++b) s = s + partials[(size_t)b * per_block + x];
        const uint32_t c = (uint32_t)(x / H), h = (uint32_t)(x % H);
        if (c < F) grad_weight_t[(size_t)c * grad_weight_stride + h] = s;
        else grad_bias[h] = s;
    }
}

} // namespace mcbs
