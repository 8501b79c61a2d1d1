// mcbs_packed_mask.hip — the Discrete attacker action mask as one bit per action (include/mcbs.h "bit-packed action masks").
//
// A MaskablePPO trainer needs each step's mask twice: at rollout time (mcbs_mask_logits covers that straight from the digest) and
// at update time, when evaluate_actions replays stored observations and the digest has long moved on.  The mask must then have been
// stored; as bytes that is 14 172 B per Chain-10 env and step, as bits 443 dwords = 1 772 B.  Three kernels:
//   pack_mask_kernel      digest of the last observation -> bits[e, 0 .. W)   (W = ceil(A / 32); the tail bits of word W-1 are zero)
//   apply_packed_kernel   logits[i, a] = bit(i, a) ? logits[i, a] : fill       (any number of rows: a gathered minibatch)
//   unpack_mask_kernel    out[i, a] = bit(i, a)                                (0 / 1 bytes)
// Bit a of a row lives in word a >> 5, bit a & 31; the action order is MaskedDiscreteAttackerWrapper's (connect, local, remote).
#pragma once
#include "mcbs_device.h"
#include "mcbs_obs.hip"
#include "mcbs_logits.hip"

namespace mcbs {

// The mask words of one env, rebuilt from its digest with the predicates of mask_logits_kernel: word w = the 32 actions
// [32 w, 32 w + 32) of the env's Discrete mask as bits (bits from A on are zero).  Shared by pack_mask_kernel (which stores the words) and
// masked_categorical_kernel (mcbs_categorical.hip, which only reads the logits under the set bits).  Everything but w is uniform per
// wavefront: d = the env's digest, n_disc = 0 for a blank observation, pp = digest_cred_pattern.
__device__ __forceinline__ uint64_t digest_cred_pattern(const LogitsGeom& G, uint32_t n_creds) {
    uint64_t pp = 0;                                     // credential pattern of one period, repeated to at least C + 32 bits
    if (G.C + 32u <= 64u) {
        const uint64_t one = n_creds >= 64u ? ~0ull : ((1ull << n_creds) - 1ull);
        for (uint32_t sh = 0; sh < 64u; sh += G.C) pp |= one << sh;
    }
    return pp;
}

__device__ __forceinline__ uint32_t digest_mask_word(const DevState& S, const ObsDigest& d, const LogitsGeom& G, const mcbs_node_static* NS,
                                                     const uint8_t* body, uint32_t e, uint32_t n_disc, uint32_t n_creds, uint64_t pp, uint32_t w) {
    const uint32_t remote0 = G.M + G.ML;
    auto own = [&](uint32_t s) -> bool { return s < G.N && ((d.own_ext[(s >> 6) & 3u] >> (s & 63u)) & 1ull); };
    auto pair_on = [&](uint32_t q) -> bool {             // row q = (source s, target t): s owned (hence discovered), t discovered
        const uint32_t s = fdiv(q, G.dN), t = q - s * G.N;
        return own(s) && t < n_disc;
    };
    // bits [lo, hi) of a block of `rowlen`-long rows (hi - lo <= 32) as bits 0 .. hi-lo-1: rowbits(q, k) = the bits of row q from its
    // k-th one on (only the low hi-lo are used)
    auto rows_in = [&](uint32_t lo, uint32_t hi, uint32_t rowlen, const FastDiv& dRow, auto rowbits) -> uint32_t {
        uint32_t m = 0, q = fdiv(lo, dRow), r0 = q * rowlen;
        for (uint32_t j = lo; j < hi; ++q, r0 += rowlen) {
            const uint32_t end = r0 + rowlen < hi ? r0 + rowlen : hi;
            m |= (uint32_t)((rowbits(q, j - r0) & ((1ull << (end - j)) - 1ull)) << (j - lo));
            j = end;
        }
        return m;
    };
    auto whole_row = [&](uint32_t q, uint32_t) -> uint64_t { return pair_on(q) ? ~0ull : 0ull; };   // connect / remote: on or off as a whole
    auto local_row = [&](uint32_t i, uint32_t k) -> uint64_t {                                     // local[i][l] = owned(i) && l applies to node i
        if (!(own(i) && i < n_disc)) return 0ull;
        return (uint64_t)NS[S.disc_at(body, e, i)].local_mask >> k;
    };
    const uint32_t a0 = w * 32u, a1 = a0 + 32u < G.A ? a0 + 32u : G.A;      // actions [a0, a1); bits from A on stay zero
    uint32_t m = 0;
    if (a0 < G.M) {
        // connect[s][t][p][c] = on(s, t) && c < n_creds: the dword overlaps ceil(32 / RL) + 1 rows at most, and since RL = P*C and the
        // block starts at action 0, the credential index of action a is a mod C in every row
        const uint32_t rows = rows_in(a0, a1 < G.M ? a1 : G.M, G.RL, G.dRL, whole_row);
        if (rows) {
            const uint32_t c0 = a0 - fdiv(a0, G.dC) * G.C;
            uint32_t cred = 0;
            if (G.C + 32u <= 64u) {
                cred = (uint32_t)(pp >> c0);
            } else {
                uint32_t c = c0;
                for (uint32_t i = 0; i < 32u; ++i) {
                    cred |= (uint32_t)(c < n_creds) << i;
                    c = c + 1u == G.C ? 0u : c + 1u;
                }
            }
            m = rows & cred;
        }
    }
    if (a1 > G.M && a0 < remote0) {                  // local block: rows of L bits, the node's vulnerability mask
        const uint32_t lo = a0 > G.M ? a0 : G.M, hi = a1 < remote0 ? a1 : remote0;
        m |= rows_in(lo - G.M, hi - G.M, G.L, G.dL, local_row) << (lo - a0);
    }
    if (a1 > remote0) {                              // remote[s][t][r] = on(s, t)
        const uint32_t lo = a0 > remote0 ? a0 : remote0;
        m |= rows_in(lo - remote0, a1 - remote0, G.R, G.dR, whole_row) << (lo - a0);
    }
    return m;
}

// One WAVEFRONT per env (four per workgroup), each lane builds whole dwords of 32 actions from the env's digest with the predicates
// of mask_logits_kernel and stores them as dwords (one 256-byte store per wavefront instruction), words 0 .. W-1 only: words from W up
// to the row stride are never written.  A pure write stream; far below the bandwidth its 1 772 bytes per env would allow (DESIGN.md
// section 7 has the measurements and the SQ counters).  (Kernel trace, 65 536 Chain-10 envs, one run, us per launch: lane k building
// dwords 4k .. 4k+3 for one 16-byte store 387, this form 131 in the same run.)
__global__ __launch_bounds__(256) void pack_mask_kernel(DevState S, Topo T, const StepCfg* __restrict__ Cp, const ObsDigest* __restrict__ digest,
                                                        uint32_t* __restrict__ bits, size_t row_words, LogitsGeom G) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t e = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // wave-uniform
    if (e >= S.E) return;
    const ObsDigest d = digest[e];                       // uniform per wavefront: scalar loads
    const uint32_t n_disc = d.blank ? 0u : d.n_disc, n_creds = d.n_creds;
    const uint32_t W = (G.A + 31u) / 32u;
    const uint8_t* body = S.body + (size_t)e * S.body_stride;
    const mcbs_node_static* NS = reinterpret_cast<const mcbs_node_static*>(T.base + Cp->off_node);
    uint32_t* row = bits + (size_t)e * row_words;
    const uint64_t pp = digest_cred_pattern(G, n_creds);
    for (uint32_t w = lane; w < W; w += 64u) row[w] = digest_mask_word(S, d, G, NS, body, e, n_disc, n_creds, pp, w);
}

// logits[i, a] = bit(i, a) ? logits[i, a] : fill for rows i < n_rows (a wavefront takes rows i, i + 4 * gridDim.x, ...).  The store
// side is mask_logits_kernel's: one WAVEFRONT per row, groups of GW actions = one vector store, spans of 64 groups starting on 128-byte lines of memory, write-only (an all-masked group is
// one vector store of `fill`, a mixed group is stored element by element, allowed actions are left alone).  The bits: GW divides 32,
// so a group's bits lie in one dword.  The wavefront keeps a window of 64 consecutive words of the row in registers (lane k: word
// wb + k, one coalesced 256-byte load) and every lane takes its group's word from it with one cross-lane read (ds_bpermute); a span
// needs at most 17 words, and the window moves on (a wave-uniform branch) when the next span would leave it.
template <typename LT, uint32_t GW, bool VEC>
__global__ __launch_bounds__(256) void apply_packed_kernel(const uint32_t* __restrict__ bits, size_t bits_row_words, LT* __restrict__ logits,
                                                           size_t row_stride, uint64_t n_rows, LT fill, uint32_t A) {
    constexpr uint32_t NWORD = GW * (uint32_t)sizeof(LT) / 4u;      // dwords per group: 4 or 2
    static_assert(NWORD == 4u || NWORD == 2u, "group = 16 or 8 bytes");
    static_assert(32u % GW == 0u, "a group's bits lie in one word");
    constexpr uint32_t ALL = (1u << GW) - 1u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i0 = (uint64_t)blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // wave-uniform
    for (uint64_t i = i0; i < n_rows; i += (uint64_t)gridDim.x * 4u) {     // rows beyond one grid's worth (any n_rows)
        const uint32_t* brow = bits + i * bits_row_words;
        LT* row = logits + i * row_stride;
        const uint32_t W = (A + 31u) / 32u;
        constexpr uint32_t GB = GW * (uint32_t)sizeof(LT);
        const uint32_t sh = VEC ? (uint32_t)((reinterpret_cast<uintptr_t>(row) / GB) % (128u / GB)) : 0u;
        const uint32_t nspan = ((A + GW - 1u) / GW + sh + 63u) / 64u;
        uint32_t wb = ~0u, win = 0u;                         // the window: lane k holds word wb + k of the row
        for (uint32_t c0s = blockIdx.y * 64u; c0s < nspan; c0s += gridDim.y * 64u) {      // chunks of 64 spans
            const uint32_t ns = nspan - c0s < 64u ? nspan - c0s : 64u;
            for (uint32_t j = 0; j < ns; ++j) {
                const uint32_t sg = (c0s + j) * 64u;         // the span: groups [sg - sh, sg + 64 - sh) of the row, clipped to [0, A)
                const uint32_t fa = (sg > sh ? sg - sh : 0u) * GW, la = ((sg + 64u - sh) * GW < A ? (sg + 64u - sh) * GW : A) - 1u;
                if (wb == ~0u || (la >> 5) >= wb + 64u) {    // wave-uniform
                    wb = fa >> 5;
                    win = wb + lane < W ? brow[wb + lane] : 0u;
                }
                const uint32_t g = sg + lane;
                const uint32_t a0 = (g - sh) * GW;
                const uint32_t word = __shfl(win, (int)(((a0 >> 5) - wb) & 63u));     // every lane takes part in the exchange
                if (g < sh || a0 >= A) continue;             // the first span's head, the last span's tail
                const uint32_t m = (word >> (a0 & 31u)) & ALL;                          // bit j: action a0 + j is allowed
                const uint32_t in_row = a0 + GW <= A ? ALL : (1u << (A - a0)) - 1u;
                const uint32_t off = ~m & in_row;            // bit j: action a0 + j is replaced
                if (VEC && off == ALL) {
                    if constexpr (sizeof(LT) == 4) {
                        const uint32_t f = __float_as_uint(fill);
                        *reinterpret_cast<uint4*>(row + a0) = make_uint4(f, f, f, f);
                    } else {
                        const uint32_t f = (uint32_t)fill, ff = f | (f << 16);
                        if constexpr (NWORD == 4u) *reinterpret_cast<uint4*>(row + a0) = make_uint4(ff, ff, ff, ff);
                        else *reinterpret_cast<uint2*>(row + a0) = make_uint2(ff, ff);
                    }
                } else if (off) {
    #pragma unroll
                    for (uint32_t k = 0; k < GW; ++k)
                        if ((off >> k) & 1u) row[a0 + k] = fill;
                }
            }
        }
    }
}

// out[i, a] = bit(i, a) as a 0 / 1 byte for a < A.  One WAVEFRONT per row, one lane per 16 bytes: pieces start on 16-byte boundaries of
// MEMORY (rows of a dense [n, A] byte array are only as aligned as A is: Chain-10's 14 172), so every piece but the row's first and last
// is 16 bits of the row (half a dword, or straddling two) spread to one 16-byte vector store; a partial head or tail piece is stored
// byte by byte.  Bytes from A up to the row stride are never written.
__global__ __launch_bounds__(256) void unpack_mask_kernel(const uint32_t* __restrict__ bits, size_t bits_row_words, uint8_t* __restrict__ out,
                                                          size_t out_stride, uint64_t n_rows, uint32_t A) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i0 = (uint64_t)blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // wave-uniform
    for (uint64_t i = i0; i < n_rows; i += (uint64_t)gridDim.x * 4u) {     // rows beyond one grid's worth (any n_rows)
        const uint32_t* brow = bits + i * bits_row_words;
        uint8_t* row = out + i * out_stride;
        const uint32_t h = (uint32_t)(reinterpret_cast<uintptr_t>(row) & 15u);   // piece k = actions [16k - h, 16k + 16 - h)
        const uint32_t npiece = (A + h + 15u) / 16u;
        auto spread = [](uint32_t nib) -> uint32_t { return (nib * 0x00204081u) & 0x01010101u; };      // 4 bits -> 4 bytes of 0 / 1
        for (uint32_t k = blockIdx.y * 64u + lane; k < npiece; k += gridDim.y * 64u) {
            if (16u * k >= h && 16u * k - h + 16u <= A) {
                const uint32_t a0 = 16u * k - h, w = a0 >> 5, s = a0 & 31u;
                uint32_t v = brow[w] >> s;
                if (s > 16u) v |= brow[w + 1u] << (32u - s);                      // the piece straddles two words (then word w+1 < W)
                *reinterpret_cast<uint4*>(row + a0) = make_uint4(spread(v & 15u), spread((v >> 4) & 15u), spread((v >> 8) & 15u), spread((v >> 12) & 15u));
            } else {
                for (uint32_t b = 0; b < 16u; ++b) {
                    const uint32_t a = 16u * k + b;          // action a - h
                    if (a < h || a - h >= A) continue;
                    row[a - h] = (uint8_t)((brow[(a - h) >> 5] >> ((a - h) & 31u)) & 1u);
                }
            }
        }
    }
}

} // namespace mcbs
