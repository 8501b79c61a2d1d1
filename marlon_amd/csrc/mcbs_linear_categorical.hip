// mcbs_linear_categorical.hip — the masked action head from the policy's latent (include/mcbs.h "masked action head from the latent").
//
// MaskableActorCriticPolicy ends in action_net = Linear(latent_dim_pi, A); of its A logits per row the masked categorical head reads
// only those under set mask bits (mcbs_categorical.hip).  This kernel computes only those: x_a = bias[a] + latent[i, :] . weight[a, :] for
// the allowed actions of the row, and hands them to the same three sweeps (cat_row_finish) through a logit source, so no logits tensor
// ever exists.  Everything after x_a is the masked categorical head's, bit for bit.
//
// One WAVEFRONT per row, four per workgroup, as there.  Per row:
//   0a the latent row is widened to float32 into LDS (wave-uniform data: every dot product reads it by broadcast)
//   0b the first CAT_CACHE mask words go to the word cache, each with the number of set bits before it (an exclusive wave scan per block
//      of 64 words), and the first LIN_STASH allowed actions are listed in LDS in ascending order
//   0c the listed actions are dealt to the lanes round-robin — lane l computes entries l, l + 64, ... — whatever word they sit in: the
//      mask's set bits cluster in a few words, and a lane per WORD would leave most lanes idle.  x_a replaces the action in the list.
//   1-3 the sweeps of the masked categorical head; cat_logit finds x_a in the list at (set bits before the word) + (set bits below a in
//      its word), or, for an allowed action beyond the list or beyond the word cache, computes it again
// lin_logit is the ONE place a logit is computed: the same operations in the same order for every caller, so x_a depends on the latent
// row, the weight row and the bias element only — not on which lane computes it, on whether it was listed, on the form or the mode.
#pragma once
#include "mcbs_categorical.hip"

namespace mcbs {

constexpr uint32_t LIN_MAX_H = 512u;        // = MCBS_LINEAR_MAX_H
constexpr uint32_t LIN_STASH = 512u;        // allowed actions per row whose logit is kept in LDS between the sweeps

struct LinIO {
    const void* latent;        // [n, latent_stride]
    const void* weight;        // [A, weight_stride]
    const void* bias;          // [A] or NULL
    size_t latent_stride, weight_stride;
    uint32_t H;
};

__device__ __forceinline__ float lin_widen(float v) { return v; }
__device__ __forceinline__ float lin_widen(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }      // bfloat16

// The wavefront's view of the linear layer for one row; all pointers below `H` are the wavefront's LDS.
template <typename WT>
struct LinSrc {
    const WT* weight;
    const WT* bias;
    size_t weight_stride;
    uint32_t H;
    const float* lat;          // the latent row as float32, 16-byte aligned
    const uint32_t* cw;        // CatRow's word cache, filled by lin_prepare
    const uint16_t* before;    // per cached word: the row's set bits in the words before it
    const uint32_t* stash;     // float32 patterns of the first LIN_STASH allowed logits
    __device__ __forceinline__ explicit operator bool() const { return true; }
};
template <typename WT> inline constexpr bool cat_src_fills_word_cache<LinSrc<WT>> = true;

// x_a in the header's order: four partial sums, element h goes to sum h mod 4 in ascending h with one fmaf each, then
// ((s0 + s1) + (s2 + s3)) + bias.  A 16-byte aligned weight row is read with 16-byte loads, any other element by element: the same
// values enter the same operations.
template <typename WT>
__device__ __forceinline__ float lin_logit(const LinSrc<WT>& s, uint32_t a) {
    const WT* __restrict__ wr = s.weight + (size_t)a * s.weight_stride;
    const float* __restrict__ lat = s.lat;
    const uint32_t H = s.H;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    uint32_t h = 0u;
    if ((reinterpret_cast<uintptr_t>(wr) & 15u) == 0u) {
        if constexpr (sizeof(WT) == 4) {
#pragma unroll 4
            for (; h + 4u <= H; h += 4u) {
                const float4 v = *reinterpret_cast<const float4*>(wr + h);
                const float4 l = *reinterpret_cast<const float4*>(lat + h);
                s0 = fmaf(l.x, v.x, s0); s1 = fmaf(l.y, v.y, s1); s2 = fmaf(l.z, v.z, s2); s3 = fmaf(l.w, v.w, s3);
            }
        } else {
#pragma unroll 2
            for (; h + 8u <= H; h += 8u) {
                const uint4 v = *reinterpret_cast<const uint4*>(wr + h);         // little endian: the lower half of a dword is the earlier element
                const float4 l = *reinterpret_cast<const float4*>(lat + h), k = *reinterpret_cast<const float4*>(lat + h + 4u);
                s0 = fmaf(l.x, __uint_as_float(v.x << 16), s0); s1 = fmaf(l.y, __uint_as_float(v.x & 0xFFFF0000u), s1);
                s2 = fmaf(l.z, __uint_as_float(v.y << 16), s2); s3 = fmaf(l.w, __uint_as_float(v.y & 0xFFFF0000u), s3);
                s0 = fmaf(k.x, __uint_as_float(v.z << 16), s0); s1 = fmaf(k.y, __uint_as_float(v.z & 0xFFFF0000u), s1);
                s2 = fmaf(k.z, __uint_as_float(v.w << 16), s2); s3 = fmaf(k.w, __uint_as_float(v.w & 0xFFFF0000u), s3);
            }
        }
    }
    for (; h < H; h += 4u) {           // h is a multiple of four here
        s0 = fmaf(lat[h], lin_widen(wr[h]), s0);
        if (h + 1u < H) s1 = fmaf(lat[h + 1u], lin_widen(wr[h + 1u]), s1);
        if (h + 2u < H) s2 = fmaf(lat[h + 2u], lin_widen(wr[h + 2u]), s2);
        if (h + 3u < H) s3 = fmaf(lat[h + 3u], lin_widen(wr[h + 3u]), s3);
    }
    return ((s0 + s1) + (s2 + s3)) + (s.bias ? lin_widen(s.bias[a]) : 0.f);
}

// the logit of an ALLOWED action a (its bit is set in the row's mask)
template <typename WT>
__device__ __forceinline__ float cat_logit(const LinSrc<WT>& s, uint32_t a) {
    const uint32_t w = a >> 5;
    if (w < CAT_CACHE) {
        const uint32_t slot = (uint32_t)s.before[w] + (uint32_t)__popc(s.cw[w] & ((1u << (a & 31u)) - 1u));
        if (slot < LIN_STASH) return __uint_as_float(s.stash[slot]);
    }
    return lin_logit(s, a);
}

// LDS written by one lane is read by another of the same wavefront: a wavefront's LDS operations execute in order, the compiler must
// only keep them in order
__device__ __forceinline__ void lin_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// steps 0a-0c for one row
template <typename WT, typename ROW>
__device__ __forceinline__ void lin_prepare(const ROW& R, const LinSrc<WT>& s, const WT* __restrict__ latent_row, float* lat, uint16_t* before,
                                            uint32_t* stash) {
    const uint32_t lane = R.lane;
    lin_wave_sync();                                   // the previous row's reads are done
    for (uint32_t h = lane; h < s.H; h += 64u) lat[h] = lin_widen(latent_row[h]);
    uint32_t base = 0u;
    const uint32_t Wc = R.W < CAT_CACHE ? R.W : CAT_CACHE;
    for (uint32_t wb = 0; wb < Wc; wb += 64u) {        // w < CAT_CACHE: CAT_CACHE is a multiple of 64
        const uint32_t w = wb + lane, word = R.fetch(w);
        R.cw[w] = word;
        if (!__ballot(word != 0u)) continue;
        const uint32_t pc = (uint32_t)__popc(word), incl = cat_wave_scan(pc, lane);
        uint32_t off = base + incl - pc;
        before[w] = (uint16_t)off;                     // at most 32 * (CAT_CACHE - 1)
        for (uint32_t rest = word; rest && off < LIN_STASH; rest &= rest - 1u) stash[off++] = w * 32u + (uint32_t)__builtin_ctz(rest);
        base += (uint32_t)__shfl((int)incl, 63);
    }
    lin_wave_sync();
    const uint32_t n = base < LIN_STASH ? base : LIN_STASH;
    for (uint32_t k = lane; k < n; k += 64u) stash[k] = __float_as_uint(lin_logit(s, stash[k]));
    lin_wave_sync();
}

template <typename WT, bool LIVE, bool OWN = false>
__global__ __launch_bounds__(256) void masked_linear_categorical_kernel(DevState S, Topo T, const StepCfg* __restrict__ Cp,
                                                                        const ObsDigest* __restrict__ digest, LogitsGeom G,
                                                                        const uint32_t* __restrict__ bits, size_t bits_row_words, LinIO lin, CatIO io) {
    __shared__ uint32_t c_word[4][CAT_CACHE];
    __shared__ float c_sum[4][CAT_CACHE];
    __shared__ __attribute__((aligned(16))) float c_lat[4][LIN_MAX_H];
    __shared__ uint32_t c_stash[4][LIN_STASH];
    __shared__ uint16_t c_before[4][CAT_CACHE];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t A = io.A, W = (A + 31u) / 32u;
    const uint32_t tail = (A & 31u) ? (1u << (A & 31u)) - 1u : ~0u;
    const WT* latent = static_cast<const WT*>(lin.latent);
    const LinSrc<WT> src{static_cast<const WT*>(lin.weight), static_cast<const WT*>(lin.bias), lin.weight_stride, lin.H,
                         c_lat[wv], c_word[wv], c_before[wv], c_stash[wv]};
    for (uint64_t i = (uint64_t)blockIdx.x * 4u + wv; i < io.n_rows; i += (uint64_t)gridDim.x * 4u) {     // wave-uniform
        const ObsDigest d = LIVE ? digest[i] : ObsDigest{};
        using Mask = DigestMaskOf<DiscoveryOf<OWN>>;
        const Mask lv = LIVE ? Mask::make(S, T, Cp, d, G, (uint32_t)i, 32u) : Mask{G, d, DiscoveryOf<OWN>::of(S, nullptr, nullptr, 0u, d), 0u, 0u, 0ull};
        const CatRow<float, LIVE, LinSrc<WT>, Mask> R{&lv, LIVE ? nullptr : bits + i * bits_row_words, src, W, tail, lane, c_word[wv], c_sum[wv]};
        lin_prepare(R, src, latent + i * lin.latent_stride, c_lat[wv], c_before[wv], c_stash[wv]);
        cat_row_finish(R, io, i);
    }
}

} // namespace mcbs
