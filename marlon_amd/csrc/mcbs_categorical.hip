// mcbs_categorical.hip — the masked categorical head of a MaskablePPO policy on the device (include/mcbs.h "masked categorical head").
//
// sb3_contrib's MaskableCategorical (train_marl_multi.py:259-293) turns the policy's logits and action_masks() into
// `where(mask, logits, -1e8)`, a log_softmax over the row, a sample, its log_prob and the entropy with the masked terms zeroed.  A
// masked-out action contributes exp(-1e8 - max) == 0 in fp32, so the distribution is exactly the softmax over the ALLOWED actions: this
// kernel reads only the logits under set mask bits and writes 16-20 bytes per row.  The logits are never modified and the mask never
// exists as bytes.  With no logits at all it is the reference's masked random agent: uniform over np.flatnonzero(action_masks()).
//
// One WAVEFRONT per row (four independent ones per workgroup, grid-striding over the rows).  Lane k owns mask words k, k + 64, ... of
// the row: the stored packed words (one coalesced load per 64 words) or, in the live form, the words rebuilt from the env's digest
// (DigestMask::word, the words pack_mask_kernel stores).  Three sweeps over the words, blocks of 64 words without any set bit skipped
// by a ballot:
//   1  K = number of set bits, m = the largest allowed logit and its lowest index (a gather of the logits under the set bits)
//   2  per word s_w = sum of exp(x - m) and t_w = sum of (x - m) exp(x - m), bits in ascending order; per block of 64 words an
//      inclusive wave scan of s_w; Z = the block totals added up in block order
//   3  (SAMPLE) the same scan again with a running base: the first word whose cumulative sum exceeds u * Z, then a walk over its bits
// The later sweeps find the logits in L2.  The first CAT_CACHE words of a row and their s_w are kept in LDS between the sweeps (every
// lane reads back only what it wrote itself: no barrier); words beyond are rebuilt and summed again, with the same operations in the
// same order, so a row's results do not depend on where the cache ends.  All arithmetic is fp32 with expf, the order of every sum is
// fixed: two calls give bit-identical outputs, and so do the live and the packed form of the same mask.  The one logarithm per row (of
// the fp32 Z, K or A) is the correctly rounded fp32 of a double-precision log: the device's logf is up to two ulp off (measured: K = 301),
// and -log K is documented to one.
#pragma once
#include "mcbs_device.h"
#include "mcbs_packed_mask.hip"

namespace mcbs {

constexpr uint32_t CAT_SAMPLE = 0u, CAT_ARGMAX = 1u, CAT_EVALUATE = 2u;     // = MCBS_CATEGORICAL_*
constexpr uint32_t CAT_DOMAIN = 0xCA7E6041u;                                // = MCBS_CATEGORICAL_PHILOX_DOMAIN
constexpr uint32_t CAT_CACHE = 512u;                                        // mask words (and their partial sums) per wavefront kept in LDS

struct CatIO {
    const void* logits;        // [n, row_stride] or NULL (all-zero logits)
    size_t row_stride;
    int64_t* actions;
    float* log_prob;
    float* entropy;            // nullable
    uint32_t* n_allowed;       // nullable
    const float* uniforms;     // nullable
    uint32_t* bad_actions;     // nullable
    uint64_t seed, step, key_base, n_rows;
    uint32_t mode, A;
};

__device__ __forceinline__ float cat_logit(const float* row, uint32_t a) { return row[a]; }
__device__ __forceinline__ float cat_logit(const uint16_t* row, uint32_t a) { return __uint_as_float((uint32_t)row[a] << 16); }    // bfloat16

__device__ __forceinline__ float cat_log(float z) { return (float)log((double)z); }     // one per row: see the comment at the top

// every lane ends with the same value: level by level, lanes l and l ^ o add the same two numbers
__device__ __forceinline__ float cat_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t cat_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}
template <typename V>
__device__ __forceinline__ V cat_wave_scan(V v, uint32_t lane) {            // inclusive, lane order
#pragma unroll
    for (uint32_t o = 1u; o < 64u; o <<= 1) {
        const V t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

// One row as its wavefront sees it, and sweeps 1 and 2 over it: shared by masked_categorical_kernel and masked_categorical_grad_kernel
// (mcbs_categorical_grad.hip), so that K, m, Z and the entropy sum of the backward pass are the forward's, bit for bit.
// SRC, the row's logit source: the row pointer, or an object with cat_logit(src, a) and a conversion to bool (false: all-zero logits)
// such as LinSrc (mcbs_linear_categorical.hip), which computes the logit from the policy's latent row.
template <typename SRC> inline constexpr bool cat_src_fills_word_cache = false;      // true: cw[0 .. CAT_CACHE) is valid BEFORE sweep 1
template <typename LT, bool LIVE, typename SRC = const LT*, typename MASK = DigestMask>
struct CatRow {
    const MASK* lv;      // LIVE: the env's digest as a mask (uniform per wavefront: scalar loads);  else
    const uint32_t* brow;      // the row's stored packed words
    SRC row;                   // the row's logits, or NULL (all-zero logits)
    uint32_t W, tail, lane;    // tail: word W-1: bits from A on are ignored, not trusted to be zero
    uint32_t* cw;              // the wavefront's LDS cache: the first CAT_CACHE mask words of the row ...
    float* cs;                 // ... and their sums s_w

    __device__ __forceinline__ uint32_t fetch(uint32_t w) const {       // word w of the row's mask (0 beyond W)
        if (w >= W) return 0u;
        uint32_t m;
        if constexpr (LIVE) m = lv->word(w); else m = brow[w];
        return w == W - 1u ? m & tail : m;
    }
    __device__ __forceinline__ uint32_t word_of(uint32_t w) const { return w < CAT_CACHE ? cw[w] : fetch(w); }     // after sweep 1
    // per-word sums of sweep 2, bits in ascending order
    __device__ __forceinline__ void word_sums(uint32_t w, uint32_t word, float m, float& s, float& t) const {
        s = 0.f; t = 0.f;
        for (uint32_t rest = word; rest; rest &= rest - 1u) {
            const float d = cat_logit(row, w * 32u + (uint32_t)__builtin_ctz(rest)) - m;
            const float ex = expf(d);
            s += ex;
            t += ex > 0.f ? d * ex : 0.f;            // (-inf) * 0 is no term of the entropy
        }
    }

    // ---- sweep 1: K, the largest allowed logit and its lowest index, the last allowed action; fills the word cache
    __device__ __forceinline__ void sweep1(float& m_out, uint32_t& arg_out, uint32_t& last_out, uint32_t& K) const {
        float m = 0.f;
        uint32_t arg = ~0u, last = 0u, cnt = 0u;
        for (uint32_t wb = 0; wb < W; wb += 64u) {
            const uint32_t w = wb + lane;
            uint32_t word;
            if constexpr (cat_src_fills_word_cache<SRC>) word = word_of(w);
            else {
                word = fetch(w);
                if (wb < CAT_CACHE) cw[w] = word;
            }
            if (!__ballot(word != 0u)) continue;
            if (!word) continue;
            cnt += (uint32_t)__popc(word);
            last = w * 32u + 31u - (uint32_t)__builtin_clz(word);
            if (!row) {
                if (arg == ~0u) arg = w * 32u + (uint32_t)__builtin_ctz(word);
                continue;
            }
            for (uint32_t rest = word; rest; rest &= rest - 1u) {      // a lane's actions ascend: `>` keeps the lowest index of equal logits
                const uint32_t a = w * 32u + (uint32_t)__builtin_ctz(rest);
                const float x = cat_logit(row, a);
                if (arg == ~0u || x > m) { m = x; arg = a; }
            }
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            const float om = __shfl_xor(m, o);
            const uint32_t oa = (uint32_t)__shfl_xor((int)arg, o);
            if (oa != ~0u && (arg == ~0u || om > m || (om == m && oa < arg))) { m = om; arg = oa; }
            const uint32_t ol = (uint32_t)__shfl_xor((int)last, o);
            last = ol > last ? ol : last;
        }
        m_out = m; arg_out = arg; last_out = last;
        K = cat_wave_sum(cnt);
    }

    // ---- sweep 2 (row != NULL): Z and the entropy sum; fills the sum cache
    __device__ __forceinline__ void sweep2(float m, float& Z_out, float& T_out) const {
        float Z = 0.f, Tt = 0.f;
        for (uint32_t wb = 0; wb < W; wb += 64u) {
            const uint32_t w = wb + lane, word = word_of(w);
            if (!__ballot(word != 0u)) continue;
            float s, t;
            word_sums(w, word, m, s, t);
            if (wb < CAT_CACHE) cs[w] = s;
            Z += __shfl(cat_wave_scan(s, lane), 63);
            Tt += cat_wave_sum(t);
        }
        Z_out = Z; T_out = Tt;
    }
};

// Everything of one row after its CatRow is set up: the three sweeps, the row's random number and the 16-20 bytes of results.  Shared by
// masked_categorical_kernel and masked_linear_categorical_kernel (mcbs_linear_categorical.hip): a logit source that returns the values
// a logits buffer would hold gives bit for bit what that buffer gives.
template <typename ROW>
__device__ __forceinline__ void cat_row_finish(const ROW& R, const CatIO& io, uint64_t i) {
    const uint32_t A = io.A, W = R.W, lane = R.lane;
    const auto& row = R.row;
    const float* cs = R.cs;
    auto word_of = [&](uint32_t w) { return R.word_of(w); };          // sweep 3 (w = block + lane: the branch is wave-uniform)
    auto word_sums = [&](uint32_t w, uint32_t word, float m, float& s, float& t) { R.word_sums(w, word, m, s, t); };

    float m;
    uint32_t arg, last, K;
    R.sweep1(m, arg, last, K);

    // the row's uniform number (SAMPLE)
    uint32_t u24 = 0u;
    if (io.mode == CAT_SAMPLE) {
        if (io.uniforms) {
            const float uf = io.uniforms[i] * 16777216.0f;
            u24 = uf >= 16777215.0f ? 16777215u : (uf >= 0.f ? (uint32_t)uf : 0u);
        } else {
            const uint64_t key = io.key_base + i;
            uint32_t r[4];
            philox4x32_10((uint32_t)key, (uint32_t)(key >> 32), (uint32_t)io.step, (uint32_t)(io.step >> 32),
                          (uint32_t)io.seed ^ CAT_DOMAIN, (uint32_t)(io.seed >> 32), r);
            u24 = r[0] >> 8;
        }
    }
    int64_t act = 0;
    bool bad = false;
    if (io.mode == CAT_EVALUATE) {
        act = io.actions[i];
        bad = act < 0 || act >= (int64_t)A;
    }
    float lp, ent;
    if (K == 0u) {
        // blank observation / all-zero row: MaskableCategorical degenerates to uniform over all A actions, entropy 0
        lp = -cat_log((float)A);
        ent = 0.f;
        if (io.mode == CAT_SAMPLE) act = (int64_t)(((uint64_t)u24 * A) >> 24);
        else if (io.mode == CAT_ARGMAX) act = 0;
    } else {
        // ---- sweep 2: Z and the entropy sum
        float Z = 0.f, Tt = 0.f;
        if (!row) {
            Z = (float)K;
        } else {
            R.sweep2(m, Z, Tt);
        }
        const float logZ = cat_log(Z);
        ent = logZ - Tt / Z;
        float x_act = 0.f;                          // the chosen action's logit (an action that is not allowed: -1e8, the reference's `where`)
        if (io.mode == CAT_ARGMAX) {
            act = (int64_t)arg;
            x_act = m;
        } else if (io.mode == CAT_EVALUATE) {
            if (!bad) {
                const uint32_t a = (uint32_t)act;
                const bool on = (R.fetch(a >> 5) >> (a & 31u)) & 1u;
                x_act = on ? (row ? cat_logit(row, a) : 0.f) : -1e8f;
            }
        } else if (!row) {
            // uniform law: the ((u24 * K) >> 24)-th allowed action, in integers
            const uint32_t k = (uint32_t)(((uint64_t)u24 * K) >> 24);
            uint32_t base = 0u, sel = last;
            for (uint32_t wb = 0; wb < W; wb += 64u) {
                const uint32_t w = wb + lane, word = word_of(w);
                if (!__ballot(word != 0u)) continue;
                const uint32_t incl = cat_wave_scan((uint32_t)__popc(word), lane);
                const uint64_t cross = __ballot(word != 0u && base + incl > k);
                if (cross) {
                    const int src = __builtin_ctzll(cross);
                    uint32_t rest = word;
                    for (uint32_t r = k - (base + incl - (uint32_t)__popc(word)); lane == (uint32_t)src && r; --r) rest &= rest - 1u;
                    sel = (uint32_t)__shfl((int)(w * 32u + (uint32_t)__builtin_ctz(rest | 0x80000000u)), src);
                    break;
                }
                base += (uint32_t)__shfl((int)incl, 63);
            }
            act = (int64_t)sel;
        } else {
            // ---- sweep 3: inverse CDF in ascending action order: the first allowed action whose cumulative sum exceeds u * Z
            const float thr = (float)u24 * (1.0f / 16777216.0f) * Z;
            float base = 0.f;
            uint32_t sel = last;                    // rounding may leave no crossing: the last allowed action
            for (uint32_t wb = 0; wb < W; wb += 64u) {
                const uint32_t w = wb + lane, word = word_of(w);
                if (!__ballot(word != 0u)) continue;
                float s, t;
                if (wb < CAT_CACHE) s = cs[w]; else word_sums(w, word, m, s, t);
                const float incl = cat_wave_scan(s, lane);
                float excl = __shfl_up(incl, 1u);
                if (lane == 0u) excl = 0.f;
                const uint64_t cross = __ballot(word != 0u && base + incl > thr);
                if (cross) {
                    const int src = __builtin_ctzll(cross);
                    uint32_t pick = 0u;
                    if (lane == (uint32_t)src) {
                        // the word's last bit stands for the word's whole sum (base + incl, which did cross)
                        pick = w * 32u + 31u - (uint32_t)__builtin_clz(word);
                        float c = base + excl;
                        for (uint32_t rest = word; rest & (rest - 1u); rest &= rest - 1u) {
                            const uint32_t a = w * 32u + (uint32_t)__builtin_ctz(rest);
                            c += expf(cat_logit(row, a) - m);
                            if (c > thr) { pick = a; break; }
                        }
                    }
                    sel = (uint32_t)__shfl((int)pick, src);
                    break;
                }
                base += __shfl(incl, 63);
            }
            act = (int64_t)sel;
            x_act = cat_logit(row, sel);
        }
        lp = (x_act - m) - logZ;
    }
    if (bad) lp = __uint_as_float(0x7FC00000u);
    if (lane == 0u) {
        if (io.mode != CAT_EVALUATE) io.actions[i] = act;
        io.log_prob[i] = lp;
        if (io.entropy) io.entropy[i] = ent;
        if (io.n_allowed) io.n_allowed[i] = K;
        if (bad && io.bad_actions) atomicAdd(io.bad_actions, 1u);
    }
}

template <typename LT, bool LIVE, bool OWN = false>
__global__ __launch_bounds__(256) void masked_categorical_kernel(DevState S, Topo T, const StepCfg* __restrict__ Cp, const ObsDigest* __restrict__ digest,
                                                                 LogitsGeom G, const uint32_t* __restrict__ bits, size_t bits_row_words, CatIO io) {
    __shared__ uint32_t c_word[4][CAT_CACHE];
    __shared__ float c_sum[4][CAT_CACHE];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t A = io.A, W = (A + 31u) / 32u;
    const uint32_t tail = (A & 31u) ? (1u << (A & 31u)) - 1u : ~0u;
    const LT* L = static_cast<const LT*>(io.logits);
    uint32_t* cw = c_word[wv];
    float* cs = c_sum[wv];
    for (uint64_t i = (uint64_t)blockIdx.x * 4u + wv; i < io.n_rows; i += (uint64_t)gridDim.x * 4u) {     // wave-uniform
        const LT* row = L ? L + i * io.row_stride : nullptr;
        // the mask's source: the env's digest (uniform per wavefront: scalar loads) or the row's stored words
        const ObsDigest d = LIVE ? digest[i] : ObsDigest{};
        using Mask = DigestMaskOf<DiscoveryOf<OWN>>;
        const Mask lv = LIVE ? Mask::make(S, T, Cp, d, G, (uint32_t)i, 32u) : Mask{G, d, DiscoveryOf<OWN>::of(S, nullptr, nullptr, 0u, d), 0u, 0u, 0ull};
        const CatRow<LT, LIVE, const LT*, Mask> R{&lv, LIVE ? nullptr : bits + i * bits_row_words, row, W, tail, lane, cw, cs};
        cat_row_finish(R, io, i);
    }
}

} // namespace mcbs
