// mcbs_categorical_grad.hip — the backward pass of the masked categorical head (include/mcbs.h "masked categorical head: gradient").
//
// MaskablePPO's update differentiates log_prob(actions) and the masked entropy of `Categorical(logits=where(mask, logits, -1e8))` with
// respect to the logits.  With p the softmax over the ALLOWED actions S, H the entropy, c the chosen action and g_lp, g_H the incoming
// gradients of the row:
//   a in S:      grad[a] = p_a * (-g_lp - g_H * (log p_a + H)) + (a == c ? g_lp : 0)
//   a not in S:  grad[a] = +0.0     (the composite's `where` passes nothing to a masked logit, chosen or not)
// so the kernel reads the packed mask and the logits under set bits, as the forward does, and writes n * A * sizeof(dtype) bytes: a write
// stream with the store side of mcbs_rowstore.h.
//
// One WAVEFRONT per row (four per workgroup, grid-striding over the rows).
//   Phase A  sweeps 1 and 2 of masked_categorical_kernel (CatRow: the same code, so K, m, Z, log Z and H are the forward's bit for bit); the
//            row's mask words stay in the wavefront's LDS cache.
//   Phase B  the row in groups of GW elements (mcbs_rowstore.h).  Every element below A is written exactly once: a group is built in
//            registers, zeros under clear bits (the logits found in L2; a whole 16-byte load where the logits rows are aligned like the
//            gradient's, else one load per set bit), and stored whole, or element by element (store_group).  A logit under a clear bit
//            may be loaded but is dropped by a select before any arithmetic reaches an output.
// fp32 throughout, no atomics, nothing depends on the launch geometry: two calls give bit-identical output, whatever the alignment.
#pragma once
#include <type_traits>
#include "mcbs_categorical.hip"

namespace mcbs {

struct CatGradIO {
    const void* logits;        // [n, row_stride]
    size_t row_stride;
    const int64_t* actions;
    const float* g_lp;         // nullable: all zeros
    const float* g_ent;        // nullable: all zeros
    void* grad;                // [n, grad_stride], the dtype of logits
    size_t grad_stride;
    uint64_t n_rows;
    uint32_t A;
    uint32_t logits_vec;       // the logits rows are aligned to the gradient's groups: whole-group loads
};

// What a row contributes to the gradient of each of its allowed logits: the forward's m, log Z, 1 / Z and entropy, the incoming gradients
// and the chosen action.  32 bytes: mcbs_linear_categorical_grad.hip keeps one per row in its workspace.
struct CatGradRow {
    float m, logZ, rZ, H, g_lp, g_H;
    uint32_t c;                // the chosen action (meaningful where live)
    uint32_t live;             // 0: K == 0 or the action lies outside [0, A): the whole row is +0.0
};

// The gradient with respect to the logit x of ALLOWED action a, in float32 before any output rounding.  The ONE place it is computed:
// masked_categorical_grad_kernel and the kernels of mcbs_linear_categorical_grad.hip call this, so their g agree bit for bit.
__device__ __forceinline__ float cat_grad_term(const CatGradRow& r, uint32_t a, float x) {
    const float d = x - r.m;
    const float ex = expf(d);
    const float lq = d - r.logZ;
    const float prod = ex > 0.f ? (ex * r.rZ) * (-r.g_lp - r.g_H * (lq + r.H)) : 0.f;      // (-inf) * 0 is no term
    return (a == r.c ? r.g_lp : 0.f) + prod;
}

template <typename LT, uint32_t GW, bool VEC>
__global__ __launch_bounds__(256) void masked_categorical_grad_kernel(const uint32_t* __restrict__ bits, size_t bits_row_words, CatGradIO io) {
    using RG = RowGroups<LT, GW, VEC>;
    constexpr uint32_t NWORD = RG::NWORD, ALL = RG::ALL;
    static_assert(32u % GW == 0u, "a group's bits lie in one word");
    using PT = std::conditional_t<sizeof(LT) == 4, uint32_t, uint16_t>;      // an element of the gradient as its bit pattern
    auto pattern = [](float v) -> PT {
        if constexpr (sizeof(LT) == 4) return __float_as_uint(v);
        else return (PT)bf16_bits(v);
    };
    __shared__ uint32_t c_word[4][CAT_CACHE];
    __shared__ float c_sum[4][CAT_CACHE];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t A = io.A, W = (A + 31u) / 32u;
    const uint32_t tail = (A & 31u) ? (1u << (A & 31u)) - 1u : ~0u;
    const LT* L = static_cast<const LT*>(io.logits);
    LT* Gr = static_cast<LT*>(io.grad);
    for (uint64_t i = (uint64_t)blockIdx.x * 4u + wv; i < io.n_rows; i += (uint64_t)gridDim.x * 4u) {     // wave-uniform
        const LT* row = L + i * io.row_stride;
        LT* out = Gr + i * io.grad_stride;
        const CatRow<LT, false> R{nullptr, bits + i * bits_row_words, row, W, tail, lane, c_word[wv], c_sum[wv]};
        __builtin_amdgcn_wave_barrier();                 // (the previous row's cached words may still be in use by other lanes)

        // ---- phase A: the forward's K, m, Z, log Z and H
        float m;
        uint32_t arg, last, K;
        R.sweep1(m, arg, last, K);
        const int64_t act = io.actions[i];
        const bool live = K != 0u && act >= 0 && act < (int64_t)A;      // else the whole row is +0.0
        const uint32_t c = (uint32_t)act;
        const float g_lp = io.g_lp ? io.g_lp[i] : 0.f, g_H = io.g_ent ? io.g_ent[i] : 0.f;
        float rZ = 0.f, logZ = 0.f, H = 0.f;
        if (live) {
            float Z, Tt;
            R.sweep2(m, Z, Tt);
            logZ = cat_log(Z);
            H = logZ - Tt / Z;
            rZ = 1.0f / Z;
        }
        // the words cached by sweep 1 are read by other lanes below
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // gradient of allowed action a with logit x
        const CatGradRow gr{m, logZ, rZ, H, g_lp, g_H, c, live ? 1u : 0u};
        auto value = [&](uint32_t a, float x) -> float { return cat_grad_term(gr, a, x); };

        // ---- phase B
        const uint32_t sh = RG::shift(out);
        const uint32_t nspan = RG::nspan(A, sh);
        for (uint32_t j = 0; j < nspan; ++j) {
            const uint32_t g = j * 64u + lane;
            const uint32_t a0 = RG::a0(g, sh);
            if (RG::outside(g, sh, A)) continue;
            const uint32_t word = live ? R.word_of(a0 >> 5) : 0u;
            const uint32_t in_row = RG::in_row(a0, A);
            const uint32_t on = (word >> (a0 & 31u)) & in_row;                          // bit k: action a0 + k is allowed
            PT v[GW];
#pragma unroll
            for (uint32_t k = 0; k < GW; ++k) v[k] = 0u;
            if (VEC && in_row == ALL && on && io.logits_vec) {
                uint32_t x[NWORD];
                if constexpr (NWORD == 4u) {
                    const uint4 q = *reinterpret_cast<const uint4*>(row + a0);
                    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
                } else {
                    const uint2 q = *reinterpret_cast<const uint2*>(row + a0);
                    x[0] = q.x; x[1] = q.y;
                }
#pragma unroll
                for (uint32_t k = 0; k < GW; ++k) {
                    float xf;
                    if constexpr (sizeof(LT) == 4) xf = __uint_as_float(x[k]);
                    else xf = __uint_as_float(((x[k >> 1] >> ((k & 1u) * 16u)) & 0xFFFFu) << 16);
                    v[k] = ((on >> k) & 1u) ? pattern(value(a0 + k, xf)) : (PT)0u;
                }
            } else {
#pragma unroll
                for (uint32_t k = 0; k < GW; ++k)
                    if ((on >> k) & 1u) v[k] = pattern(value(a0 + k, cat_logit(row, a0 + k)));
            }
            store_group<PT, GW, VEC>(reinterpret_cast<PT*>(out), a0, A, v);
        }
    }
}

} // namespace mcbs
