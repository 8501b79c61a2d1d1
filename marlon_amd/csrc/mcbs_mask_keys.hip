// mcbs_mask_keys.hip — the Discrete attacker action mask as a KEY: the few words it is a function of (include/mcbs.h "action-mask keys").
//
// The packed mask of mcbs_packed_mask.hip is W = ceil(A / 32) words per env and step (Chain-10 at 12/12: 443 words, 1 772 B), yet
// DigestMask rebuilds every one of its bits from the digest's owned-source bits and two counts plus, for the local-vulnerability block,
// which node sits at each discovery index.  Only that last input lives in the env's state, which has moved on by update time.  A row
// that carries the discovery order next to the digest's three inputs is self-contained: Wk = 1 + ceil(Nk / 32) + ceil(Nk / 4) words
// (Chain-10: 5 words, 20 B).  Two kernels:
//   store_mask_keys_kernel    digest + discovery list of the last observation -> keys[e, 0 .. Wk)
//   expand_mask_keys_kernel   keys[index[i], 0 .. Wk) -> bits[i, 0 .. W), the words pack_mask_kernel would have stored (DigestMask::word
//                             over a key-backed discovery source: the mask rule exists once)
#pragma once
#include "mcbs_device.h"
#include "mcbs_obs.hip"
#include "mcbs_logits.hip"
#include "mcbs_obs_packing.hip"

namespace mcbs {

struct MaskKeyGeom {       // layout of a key row, set up on the host
    uint32_t Nk, own_words, node_words, Wk;      // nodes a key can name, ceil(Nk / 32), ceil(Nk / 4), 1 + own_words + node_words
    FastDiv dWk;
};

// One THREAD per key word: thread x builds word x mod Wk of env x / Wk, so consecutive lanes store consecutive words and dense rows leave
// as whole cache lines (Chain-10: five words per env, 1.3 MB for 65 536 envs).  Every thread issues its loads — the digest's counts, one
// owned-source word, four entries of the discovery list — side by side and unconditionally, then stores once: no load waits for
// another's result, and none is issued behind a store.  List entries are fetched at indices clamped to the list and masked by the count
// afterwards.  Words from Wk on are never written.
template <bool OWN = false>
__global__ __launch_bounds__(256) void store_mask_keys_kernel(DevState S, const ObsDigest* __restrict__ digest, uint32_t* __restrict__ keys,
                                                              size_t row_words, MaskKeyGeom K, uint32_t total) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= total) return;
    const uint32_t e = fdiv(x, K.dWk), w = x - e * K.Wk;
    const uint8_t* body = S.body + (size_t)e * S.body_stride;
    // ---------------- loads ----------------
    const uint4 counts = *reinterpret_cast<const uint4*>(&digest[e].n_disc);       // n_disc, n_creds, blank, pad
    const uint32_t ow = w - 1u < K.own_words ? w - 1u : 0u;                          // the owned-source word this thread might need
    const uint64_t own64 = digest[e].own_ext[(ow >> 1) & 3u];
    const uint32_t i0 = w > K.own_words ? (w - 1u - K.own_words) * 4u : 0u;          // ... and its four list entries
    uint32_t node[4];
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) node[j] = S.disc_at(body, e, i0 + j < S.N ? i0 + j : S.N - 1u);
    if constexpr (OWN) {                                                             // a digest that carries its own discovery order (counts.w; mcbs_logits.hip)
        const uint2 own_list = *reinterpret_cast<const uint2*>(digest[e].pad2);
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) node[j] = counts.w ? DevState::list_nibble(own_list.x, own_list.y, (i0 + j) & 15u) : node[j];
    }
    // ---------------- the word ----------------
    const uint32_t n_disc = counts.z ? 0u : (counts.x < K.Nk ? counts.x : K.Nk);    // the effective count: 0 for a blank observation
    auto below = [](uint32_t first, uint32_t n) -> uint32_t {                       // bit j: first + j < n
        return n <= first ? 0u : (n - first >= 32u ? ~0u : (1u << (n - first)) - 1u);
    };
    uint32_t v;
    if (w == 0u) v = n_disc | (counts.y << 16);
    else if (w <= K.own_words) v = (uint32_t)(own64 >> ((ow & 1u) * 32u)) & below(ow * 32u, n_disc);
    else {
        v = 0u;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) v |= (i0 + j < n_disc ? node[j] & 0xFFu : 0u) << (8u * j);
    }
    keys[(size_t)e * row_words + w] = v;
}

// The discovery source of a DigestMask over a key row: the local-vulnerability mask of the node at discovery index i, staged per
// wavefront in LDS before the first word is built (entries below the key's count only)
struct KeyDiscovery {
    const uint32_t* lmask;
    __device__ __forceinline__ uint32_t local_mask(uint32_t i) const { return lmask[i]; }
};

// One WAVEFRONT per output row (four per workgroup, rows beyond one grid's worth in a loop).  The key row is fetched wave-uniformly
// (scalar loads of a uniform address): its counts and owned-source words become a digest in registers.  The lanes then resolve the
// node bytes to local-vulnerability masks through the topology's static node table, one discovery index per lane, into the wavefront's
// LDS — every load of the row is done before its first store — and build whole words with DigestMask::word, as pack_mask_kernel does.
// A malformed key cannot read out of bounds: the count is clamped to Nk (the LDS holds MCBS_MAX_NODES entries), a node id at or above the
// topology's node count contributes no local bits, and owned-source bits at or above the count are dropped.  A source row outside
// [0, n_source_rows) reads nothing: the row is zeros.  Words from W on are never written.
__global__ __launch_bounds__(256) void expand_mask_keys_kernel(const mcbs_node_static* __restrict__ NS, uint32_t n_nodes, MaskKeyGeom K, LogitsGeom G,
                                                               const uint32_t* __restrict__ keys, size_t key_row_words,
                                                               const int64_t* __restrict__ index, uint64_t n_source_rows,
                                                               uint32_t* __restrict__ bits, size_t bits_row_words, uint64_t n_rows) {
    __shared__ uint32_t lmask_lds[4][MCBS_MAX_NODES];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t* lmask = lmask_lds[wave];
    const uint32_t W = (G.A + 31u) / 32u;
    for (uint64_t i = (uint64_t)blockIdx.x * 4u + wave; i < n_rows; i += (uint64_t)gridDim.x * 4u) {      // wave-uniform
        uint32_t* row = bits + i * bits_row_words;
        uint64_t s;
        if (!obs_source_row(index, i, n_source_rows, s)) {           // uniform
            for (uint32_t w = lane; w < W; w += 64u) row[w] = 0u;
            continue;
        }
        const uint32_t* krow = keys + s * key_row_words;
        const uint32_t w0 = krow[0];
        ObsDigest d;
        d.n_disc = (w0 & 0xFFFFu) < K.Nk ? (w0 & 0xFFFFu) : K.Nk;
        d.n_creds = w0 >> 16;
        d.blank = 0u;
#pragma unroll
        for (uint32_t c = 0; c < 4u; ++c) {
            const uint32_t lo = 2u * c < K.own_words ? krow[1u + 2u * c] : 0u, hi = 2u * c + 1u < K.own_words ? krow[2u + 2u * c] : 0u;
            const uint32_t n = d.n_disc > 64u * c ? d.n_disc - 64u * c : 0u;      // bits of this word below the count
            d.own_ext[c] = (((uint64_t)hi << 32) | lo) & (n >= 64u ? ~0ull : (1ull << n) - 1ull);
        }
        __builtin_amdgcn_wave_barrier();                             // (the previous row's masks may still be read by other lanes)
        for (uint32_t j = lane; j < d.n_disc; j += 64u) {
            const uint32_t id = (krow[1u + K.own_words + (j >> 2)] >> (8u * (j & 3u))) & 0xFFu;
            lmask[j] = id < n_nodes ? NS[id].local_mask : 0u;
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        const DigestMaskOf<KeyDiscovery> M = DigestMaskOf<KeyDiscovery>::from(G, d, KeyDiscovery{lmask}, 32u);
        for (uint32_t w = lane; w < W; w += 64u) row[w] = M.word(w);
    }
}

} // namespace mcbs
