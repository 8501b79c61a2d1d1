// mcbs_linear_categorical_grad.hip — the backward pass of the masked action head from the latent (include/mcbs.h "masked action head from
// the latent: gradient").
//
// With x_a = bias[a] + latent[i, :] . weight[a, :] the logit of an allowed action (lin_logit: the forward's device code) and g_{i,a} the
// gradient of the masked categorical head with respect to it (cat_grad_term: the logits-gradient kernel's device code), the update needs
//   grad_latent[i, h] = sum over the allowed a of row i   g_{i,a} * w_{a,h}
//   grad_weight[a, h] = sum over the rows i                g_{i,a} * l_{i,h}
//   grad_bias[a]      = sum over the rows i                g_{i,a}
// and no [n, A] tensor exists on the way: g is computed where it is used, twice (once per direction of the sum).  No floating-point
// atomics; every sum has the order the header spells out, a function of (n_rows, the masks, H) only.
//
// Three launches (one when neither grad_weight nor grad_bias is asked for):
//   row pass      one WAVEFRONT per row, four per workgroup, as the forward: lin_prepare, sweeps 1 and 2 (K, m, Z, log Z and the entropy
//                 are the forward's bit for bit), the row's CatGradRow to the workspace, then grad_latent with the lanes over h: the allowed
//                 actions in ascending order, the k-th into partial sum k mod 4.  The actions whose logit lin_prepare left in the stash
//                 are listed again next to it (in the LDS sweep 2 no longer needs) and taken 64 at a time: every lane one g, then the
//                 weight rows eight to a batch of loads.  Actions beyond the stash or the word cache follow one by one (cat_logit).
//   action pass   one workgroup per (mask word, block of LIN_GRAD_ROW_BLOCK rows).  The block's column of the word goes to LDS once for
//                 the four wavefronts, dead rows cleared (one 4-byte word per row: n * W cache lines in all; grouping adjacent words into
//                 one workgroup was measured and lost, see LIN_GRAD_WORDS).  Wavefront v owns byte v of the word: 8 actions, their
//                 [8][H] partial sums in registers, lanes over h.  64 / NH rows at a time: the latent rows whose word is set go to an
//                 LDS tile the four wavefronts share (all loads in flight before the first store), each wavefront lists its (row, action)
//                 pairs in ascending order, one lane per pair recomputes x and g, and the pairs are added into the chains in list order.
//   reduce pass   one wavefront per action: the block partials added in ascending block order, every element of grad_weight / grad_bias
//                 written exactly once (+0.0 for an action no row allows).
#pragma once
#include "mcbs_categorical_grad.hip"
#include "mcbs_linear_categorical.hip"

namespace mcbs {

constexpr uint32_t LIN_GRAD_ROW_BLOCK = 512u;      // = MCBS_LINEAR_GRAD_ROW_BLOCK
// adjacent mask words per workgroup of the action pass, taken one after the other.  Measured on the headline minibatch (16 384 rows,
// A = 14 172, H = 64, fp32): 1 -> 490 us, 2 -> 756 us, 4 -> 1 083 us.  The pass takes as long as its busiest workgroup (a few words are
// set in nearly every row), so sharing the column fetch among more words only lengthens it.
constexpr uint32_t LIN_GRAD_WORDS = 1u;

struct LinGradIO {
    const int64_t* actions;
    const float* g_lp;         // nullable: all zeros
    const float* g_ent;        // nullable: all zeros
    float* grad_latent;        // [n, grad_latent_stride] or NULL
    size_t grad_latent_stride;
    float* grad_weight;        // [A, grad_weight_stride] or NULL
    size_t grad_weight_stride;
    float* grad_bias;          // [A] or NULL
    CatGradRow* stats;         // workspace: [n], NULL when there is no action pass
    float* part_w;             // workspace: [n_blocks][32 W][H]
    float* part_b;             // workspace: [n_blocks][32 W]
    uint64_t n_rows;
    uint32_t A, n_blocks;
};

__device__ __forceinline__ float lin_readlane(float v, uint32_t l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), (int)l));
}

template <typename WT>
__global__ __launch_bounds__(256) void masked_linear_categorical_grad_row_kernel(const uint32_t* __restrict__ bits, size_t bits_row_words, LinIO lin,
                                                                                 LinGradIO io) {
    __shared__ uint32_t c_word[4][CAT_CACHE];
    __shared__ float c_sum[4][CAT_CACHE];
    __shared__ __attribute__((aligned(16))) float c_lat[4][LIN_MAX_H];
    __shared__ uint32_t c_stash[4][LIN_STASH];
    __shared__ uint16_t c_before[4][CAT_CACHE];
    static_assert(LIN_STASH <= CAT_CACHE, "the listed actions take the place of sweep 2's sums");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t A = io.A, W = (A + 31u) / 32u, H = lin.H;
    const uint32_t tail = (A & 31u) ? (1u << (A & 31u)) - 1u : ~0u;
    const WT* latent = static_cast<const WT*>(lin.latent);
    const WT* weight = static_cast<const WT*>(lin.weight);
    const LinSrc<WT> src{weight, static_cast<const WT*>(lin.bias), lin.weight_stride, H, c_lat[wv], c_word[wv], c_before[wv], c_stash[wv]};
    uint32_t* acts = reinterpret_cast<uint32_t*>(c_sum[wv]);
    const uint32_t* stash = c_stash[wv];
    for (uint64_t i = (uint64_t)blockIdx.x * 4u + wv; i < io.n_rows; i += (uint64_t)gridDim.x * 4u) {     // wave-uniform
        const CatRow<float, false, LinSrc<WT>> R{nullptr, bits + i * bits_row_words, src, W, tail, lane, c_word[wv], c_sum[wv]};
        lin_prepare(R, src, latent + i * lin.latent_stride, c_lat[wv], c_before[wv], c_stash[wv]);

        // ---- the forward's K, m, Z, log Z and H (phase A of masked_categorical_grad_kernel)
        float m;
        uint32_t arg, last, K;
        R.sweep1(m, arg, last, K);
        const int64_t act = io.actions[i];
        const bool live = K != 0u && act >= 0 && act < (int64_t)A;      // else the whole row is +0.0
        const float g_lp = io.g_lp ? io.g_lp[i] : 0.f, g_H = io.g_ent ? io.g_ent[i] : 0.f;
        float rZ = 0.f, logZ = 0.f, Hent = 0.f;
        if (live) {
            float Z, Tt;
            R.sweep2(m, Z, Tt);
            logZ = cat_log(Z);
            Hent = logZ - Tt / Z;
            rZ = 1.0f / Z;
        }
        const CatGradRow gr{m, logZ, rZ, Hent, g_lp, g_H, (uint32_t)act, live ? 1u : 0u};
        if (io.stats && lane == 0u) io.stats[i] = gr;
        if (!io.grad_latent) continue;

        // ---- the actions lin_prepare listed (their logits are in the stash), listed again: the sums of sweep 2 are not needed any more
        uint32_t n_list = 0u;
        if (live) {
            lin_wave_sync();
            uint32_t cnt = 0u;
            const uint32_t Wc = W < CAT_CACHE ? W : CAT_CACHE;
            for (uint32_t wb = 0u; wb < Wc; wb += 64u) {
                const uint32_t w = wb + lane, word = R.cw[w];
                if (!__ballot(word != 0u)) continue;
                cnt += (uint32_t)__popc(word);
                uint32_t off = src.before[w];
                for (uint32_t rest = word; rest && off < LIN_STASH; rest &= rest - 1u) acts[off++] = w * 32u + (uint32_t)__builtin_ctz(rest);
            }
            cnt = cat_wave_sum(cnt);
            n_list = cnt < LIN_STASH ? cnt : LIN_STASH;
            lin_wave_sync();
        }

        // ---- grad_latent: lanes over h, the allowed actions in ascending order, the k-th into partial sum k mod 4
        float* __restrict__ out = io.grad_latent + i * io.grad_latent_stride;
        for (uint32_t h0 = 0u; h0 < H; h0 += 64u) {
            const uint32_t h = h0 + lane;
            const bool on = h < H;
            const WT* __restrict__ wcol = weight + (on ? h : 0u);
            float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
            for (uint32_t k0 = 0u; k0 < n_list; k0 += 64u) {           // k0 + q is a multiple of four
                const uint32_t cnt = n_list - k0 < 64u ? n_list - k0 : 64u;
                uint32_t a_l = 0u;
                float g_l = 0.f;
                if (lane < cnt) {
                    a_l = acts[k0 + lane];
                    g_l = cat_grad_term(gr, a_l, __uint_as_float(stash[k0 + lane]));
                }
                for (uint32_t q = 0u; q < cnt; q += 8u) {
                    float wq[8], gq[8];
#pragma unroll
                    for (uint32_t e = 0u; e < 8u; ++e) {               // a lane beyond cnt holds action 0: loaded, never used
                        const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)a_l, (int)(q + e));
                        gq[e] = lin_readlane(g_l, q + e);
                        wq[e] = lin_widen(wcol[(size_t)a * lin.weight_stride]);
                    }
                    t0 = fmaf(gq[0], wq[0], t0);
                    t1 = q + 1u < cnt ? fmaf(gq[1], wq[1], t1) : t1;
                    t2 = q + 2u < cnt ? fmaf(gq[2], wq[2], t2) : t2;
                    t3 = q + 3u < cnt ? fmaf(gq[3], wq[3], t3) : t3;
                    t0 = q + 4u < cnt ? fmaf(gq[4], wq[4], t0) : t0;
                    t1 = q + 5u < cnt ? fmaf(gq[5], wq[5], t1) : t1;
                    t2 = q + 6u < cnt ? fmaf(gq[6], wq[6], t2) : t2;
                    t3 = q + 7u < cnt ? fmaf(gq[7], wq[7], t3) : t3;
                }
            }
            if (live && K > n_list) {                                  // beyond the stash or the word cache: one by one
                uint32_t k = 0u;
                for (uint32_t wb = 0u; wb < W; wb += 64u) {
                    const uint32_t word = R.word_of(wb + lane);
                    for (uint64_t nz = __ballot(word != 0u); nz; nz &= nz - 1ull) {
                        const uint32_t sl = (uint32_t)__builtin_ctzll(nz);
                        const uint32_t uw = (uint32_t)__builtin_amdgcn_readlane((int)word, (int)sl);
                        if (k + (uint32_t)__popc(uw) <= n_list) {      // the whole word was listed
                            k += (uint32_t)__popc(uw);
                            continue;
                        }
                        for (uint32_t rest = uw; rest; rest &= rest - 1u, ++k) {
                            if (k < n_list) continue;
                            const uint32_t a = (wb + sl) * 32u + (uint32_t)__builtin_ctz(rest);      // wave-uniform
                            const float g = cat_grad_term(gr, a, cat_logit(src, a));
                            const float wah = lin_widen(wcol[(size_t)a * lin.weight_stride]);
                            switch (k & 3u) {
                                case 0u: t0 = fmaf(g, wah, t0); break;
                                case 1u: t1 = fmaf(g, wah, t1); break;
                                case 2u: t2 = fmaf(g, wah, t2); break;
                                default: t3 = fmaf(g, wah, t3); break;
                            }
                        }
                    }
                }
            }
            if (on) out[h] = (t0 + t1) + (t2 + t3);
        }
    }
}

// NH: the 64-wide chunks of h a lane owns, H <= 64 * NH (1, 2, 4 or 8: the partial sums are registers); the LDS tile holds 64 / NH rows
template <typename WT, uint32_t NH>
__global__ __launch_bounds__(256) void masked_linear_categorical_grad_action_kernel(const uint32_t* __restrict__ bits, size_t bits_row_words, LinIO lin,
                                                                                    LinGradIO io) {
    constexpr uint32_t RC = 64u / NH;                  // rows per tile
    constexpr uint32_t RW = RC / 4u;                   // of which each wavefront loads
    constexpr uint32_t NQ = LIN_GRAD_ROW_BLOCK / 64u;  // 64-row groups per block
    constexpr uint64_t RC_MASK = RC == 64u ? ~0ull : (1ull << RC) - 1ull;
    __shared__ __attribute__((aligned(16))) float c_tile[RC * (64u * NH + 4u)];      // [RC][LS] float32 latent rows
    __shared__ uint16_t c_pair[4][RC * 8u];            // per wavefront: (row in tile) * 8 + bit, ascending
    __shared__ uint32_t c_col[LIN_GRAD_WORDS][LIN_GRAD_ROW_BLOCK];      // the row block's columns of the group's mask words
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t A = io.A, W = (A + 31u) / 32u, H = lin.H;
    const uint32_t LS = ((H + 3u) & ~3u) + 4u;         // 16-byte aligned rows, four floats apart from a multiple of the bank count
    const uint32_t tail = (A & 31u) ? (1u << (A & 31u)) - 1u : ~0u;
    const WT* latent = static_cast<const WT*>(lin.latent);
    const uint32_t wg0 = blockIdx.x * LIN_GRAD_WORDS;  // the grid's x is ceil(W / LIN_GRAD_WORDS)
    uint16_t* pair = c_pair[wv];
    for (uint32_t j = blockIdx.y; j < io.n_blocks; j += gridDim.y) {        // uniform over the workgroup
        const uint64_t r0 = (uint64_t)j * LIN_GRAD_ROW_BLOCK;
        const uint64_t r1 = r0 + LIN_GRAD_ROW_BLOCK < io.n_rows ? r0 + LIN_GRAD_ROW_BLOCK : io.n_rows;
        // the block's columns of the group's words, dead rows cleared, tail bits dropped
        __syncthreads();                                               // the previous block's columns are no longer read
        for (uint32_t rr = threadIdx.x; rr < LIN_GRAD_ROW_BLOCK; rr += 256u) {
            const uint64_t il = r0 + rr;
            uint32_t v[LIN_GRAD_WORDS];
#pragma unroll
            for (uint32_t e = 0u; e < LIN_GRAD_WORDS; ++e) v[e] = 0u;
            if (il < r1) {
                const uint32_t* __restrict__ br = bits + il * bits_row_words;
                uint32_t any = 0u;
#pragma unroll
                for (uint32_t e = 0u; e < LIN_GRAD_WORDS; ++e) {
                    if (wg0 + e < W) v[e] = br[wg0 + e];
                    if (wg0 + e == W - 1u) v[e] &= tail;
                    any |= v[e];
                }
                if (any && !io.stats[il].live) {
#pragma unroll
                    for (uint32_t e = 0u; e < LIN_GRAD_WORDS; ++e) v[e] = 0u;
                }
            }
#pragma unroll
            for (uint32_t e = 0u; e < LIN_GRAD_WORDS; ++e) c_col[e][rr] = v[e];
        }
        __syncthreads();
      for (uint32_t wi = 0u; wi < LIN_GRAD_WORDS && wg0 + wi < W; ++wi) {  // the group's words, one after the other
        const uint32_t w = wg0 + wi;
        const uint32_t a0 = w * 32u + wv * 8u;         // this wavefront's 8 actions
        float acc[8][NH], accb[8];
#pragma unroll
        for (uint32_t b = 0u; b < 8u; ++b) {
            accb[b] = 0.f;
#pragma unroll
            for (uint32_t c = 0u; c < NH; ++c) acc[b][c] = 0.f;
        }
        for (uint32_t q = 0u; q < NQ; ++q) {
            const uint32_t word = c_col[wi][q * 64u + lane];           // every wavefront of the workgroup sees the same values
            const uint64_t nzw = __ballot(word != 0u);
            if (!nzw) continue;
            for (uint32_t s = 0u; s < NH; ++s) {
                const uint64_t sub = (nzw >> (s * RC)) & RC_MASK;      // the same in the four wavefronts: the barriers below are uniform
                if (!sub) continue;
                const uint64_t rt = r0 + q * 64u + s * RC;             // the tile's first row
                __syncthreads();                                       // the previous tile is no longer read
                // the tile: wavefront v brings rows v * RW .. of it, all its loads in flight before the first LDS store
                float tv[RW][NH];
#pragma unroll
                for (uint32_t u = 0u; u < RW; ++u) {
                    const uint32_t r = wv * RW + u;
                    const WT* __restrict__ lr = latent + (rt + r) * lin.latent_stride;
#pragma unroll
                    for (uint32_t c = 0u; c < NH; ++c) {
                        const uint32_t h = lane + c * 64u;
                        tv[u][c] = ((sub >> r) & 1ull) && h < H ? lin_widen(lr[h]) : 0.f;
                    }
                }
#pragma unroll
                for (uint32_t u = 0u; u < RW; ++u) {
                    const uint32_t r = wv * RW + u;
#pragma unroll
                    for (uint32_t c = 0u; c < NH; ++c) {
                        const uint32_t h = lane + c * 64u;
                        if (((sub >> r) & 1ull) && h < H) c_tile[r * LS + h] = tv[u][c];
                    }
                }
                __syncthreads();
                // this wavefront's pairs, rows ascending, bits ascending
                const uint32_t rl = lane - s * RC;                     // the lane's row in the tile (if < RC)
                const uint32_t byte = rl < RC ? (word >> (wv * 8u)) & 0xFFu : 0u;
                const uint32_t pc = (uint32_t)__popc(byte), incl = cat_wave_scan(pc, lane);
                const uint32_t P = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                if (!P) continue;
                uint32_t off = incl - pc;
                for (uint32_t rest = byte; rest; rest &= rest - 1u) pair[off++] = (uint16_t)(rl * 8u + (uint32_t)__builtin_ctz(rest));
                lin_wave_sync();
                for (uint32_t k0 = 0u; k0 < P; k0 += 64u) {
                    // one lane per pair: x and g
                    const uint32_t cnt = P - k0 < 64u ? P - k0 : 64u;
                    uint32_t pr_l = 0u;
                    float g_l = 0.f;
                    if (lane < cnt) {
                        pr_l = pair[k0 + lane];
                        const uint32_t r = pr_l >> 3, a = a0 + (pr_l & 7u);
                        const LinSrc<WT> src{static_cast<const WT*>(lin.weight), static_cast<const WT*>(lin.bias), lin.weight_stride, H, c_tile + r * LS,
                                             nullptr, nullptr, nullptr};
                        g_l = cat_grad_term(io.stats[rt + r], a, lin_logit(src, a));
                    }
                    // the chains, in list order, four pairs to a batch of LDS reads; a pair beyond cnt changes nothing
                    for (uint32_t p0 = 0u; p0 < cnt; p0 += 4u) {
                        float lq[4][NH], gq[4];
                        uint32_t bq[4];
#pragma unroll
                        for (uint32_t e = 0u; e < 4u; ++e) {
                            const uint32_t pr = (uint32_t)__builtin_amdgcn_readlane((int)pr_l, (int)(p0 + e));
                            gq[e] = lin_readlane(g_l, p0 + e);
                            bq[e] = p0 + e < cnt ? pr & 7u : 8u;
#pragma unroll
                            for (uint32_t c = 0u; c < NH; ++c) {
                                const uint32_t h = lane + c * 64u;
                                lq[e][c] = h < H ? c_tile[(pr >> 3) * LS + h] : 0.f;
                            }
                        }
#pragma unroll
                        for (uint32_t e = 0u; e < 4u; ++e) {
#pragma unroll
                            for (uint32_t bb = 0u; bb < 8u; ++bb) {
                                const bool take = bq[e] == bb;         // wave-uniform
                                accb[bb] = take ? accb[bb] + gq[e] : accb[bb];
#pragma unroll
                                for (uint32_t c = 0u; c < NH; ++c) acc[bb][c] = take ? fmaf(gq[e], lq[e][c], acc[bb][c]) : acc[bb][c];
                            }
                        }
                    }
                }
            }
        }
        float* __restrict__ pw = io.part_w + ((size_t)j * W * 32u + a0) * H;
        float* __restrict__ pb = io.part_b + (size_t)j * W * 32u + a0;
#pragma unroll
        for (uint32_t b = 0u; b < 8u; ++b) {
#pragma unroll
            for (uint32_t c = 0u; c < NH; ++c) {
                const uint32_t h = lane + c * 64u;
                if (h < H) pw[(size_t)b * H + h] = acc[b][c];
            }
            if (lane == 0u) pb[b] = accb[b];
        }
      }
    }
}

// the block partials in ascending block order; no block (n_rows == 0): +0.0
__global__ __launch_bounds__(256) void masked_linear_categorical_grad_reduce_kernel(LinGradIO io, uint32_t H) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = threadIdx.x >> 6;
    const uint32_t A = io.A, W = (A + 31u) / 32u;
    const size_t per_block = (size_t)W * 32u;
    for (uint32_t a = blockIdx.x * 4u + wv; a < A; a += gridDim.x * 4u) {
        if (io.grad_weight) {
            for (uint32_t h = lane; h < H; h += 64u) {
                float s = 0.f;
                if (io.n_blocks) s = io.part_w[(size_t)a * H + h];
                for (uint32_t j = 1u; j < io.n_blocks; ++j) s += io.part_w[((size_t)j * per_block + a) * H + h];
                io.grad_weight[(size_t)a * io.grad_weight_stride + h] = s;
            }
        }
        if (io.grad_bias && lane == 0u) {
            float s = 0.f;
            if (io.n_blocks) s = io.part_b[a];
            for (uint32_t j = 1u; j < io.n_blocks; ++j) s += io.part_b[(size_t)j * per_block + a];
            io.grad_bias[a] = s;
        }
    }
}

} // namespace mcbs
