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

// One WAVEFRONT per env (four per workgroup), each lane builds whole dwords of 32 actions from the env's digest (DigestMask::word)
// and stores them as dwords (one 256-byte store per wavefront instruction), words 0 .. W-1 only: words from W up
// to the row stride are never written.  A pure write stream; far below the bandwidth its 1 772 bytes per env would allow (DESIGN.md
// section 7 has the measurements and the SQ counters).  (Kernel trace, 65 536 Chain-10 envs, one run, us per launch: lane k building
// dwords 4k .. 4k+3 for one 16-byte store 387, this form 131 in the same run.)
template <bool OWN = false>
__global__ __launch_bounds__(256) void pack_mask_kernel(DevState S, Topo T, const StepCfg* __restrict__ Cp, const ObsDigest* __restrict__ digest,
                                                        uint32_t* __restrict__ bits, size_t row_words, LogitsGeom G) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t e = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // wave-uniform
    if (e >= S.E) return;
    const ObsDigest d = digest[e];                       // uniform per wavefront: scalar loads
    const auto M = DigestMaskOf<DiscoveryOf<OWN>>::make(S, T, Cp, d, G, e, 32u);
    const uint32_t W = (G.A + 31u) / 32u;
    uint32_t* row = bits + (size_t)e * row_words;
    for (uint32_t w = lane; w < W; w += 64u) row[w] = M.word(w);
}

// logits[i, a] = bit(i, a) ? logits[i, a] : fill for rows i < n_rows (a wavefront takes rows i, i + 4 * gridDim.x, ...).  The store
// side is mcbs_rowstore.h's: one WAVEFRONT per row, write-only.  The bits: GW divides 32,
// so a group's bits lie in one dword.  The wavefront keeps a window of 64 consecutive words of the row in registers (lane k: word
// wb + k, one coalesced 256-byte load) and every lane takes its group's word from it with one cross-lane read (ds_bpermute); a span
// needs at most 17 words, and the window moves on (a wave-uniform branch) when the next span would leave it.
template <typename LT, uint32_t GW, bool VEC>
__global__ __launch_bounds__(256) void apply_packed_kernel(const uint32_t* __restrict__ bits, size_t bits_row_words, LT* __restrict__ logits,
                                                           size_t row_stride, uint64_t n_rows, LT fill, uint32_t A) {
    using RG = RowGroups<LT, GW, VEC>;
    static_assert(32u % GW == 0u, "a group's bits lie in one word");
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i0 = (uint64_t)blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // wave-uniform
    for (uint64_t i = i0; i < n_rows; i += (uint64_t)gridDim.x * 4u) {     // rows beyond one grid's worth (any n_rows)
        const uint32_t* brow = bits + i * bits_row_words;
        LT* row = logits + i * row_stride;
        const uint32_t W = (A + 31u) / 32u;
        const uint32_t sh = RG::shift(row);
        const uint32_t nspan = RG::nspan(A, sh);
        uint32_t wb = ~0u, win = 0u;                         // the window: lane k holds word wb + k of the row
        for (uint32_t c0s = blockIdx.y * 64u; c0s < nspan; c0s += gridDim.y * 64u) {      // chunks of 64 spans
            const uint32_t ns = nspan - c0s < 64u ? nspan - c0s : 64u;
            for (uint32_t j = 0; j < ns; ++j) {
                const uint32_t fa = RG::span_first(c0s + j, sh), la = RG::span_last(c0s + j, sh, A) - 1u;      // the span's actions [fa, la]
                if (wb == ~0u || (la >> 5) >= wb + 64u) {    // wave-uniform
                    wb = fa >> 5;
                    win = wb + lane < W ? brow[wb + lane] : 0u;
                }
                const uint32_t g = (c0s + j) * 64u + lane;
                const uint32_t a0 = RG::a0(g, sh);
                const uint32_t word = __shfl(win, (int)(((a0 >> 5) - wb) & 63u));     // every lane takes part in the exchange
                if (RG::outside(g, sh, A)) continue;
                const uint32_t m = (word >> (a0 & 31u)) & RG::ALL;                      // bit j: action a0 + j is allowed
                store_fill_group<LT, GW, VEC>(row, a0, ~m & RG::in_row(a0, A), fill);
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
