// mcbs_logits.hip — on-device "action mask -> logits" for the Discrete attacker action space.
//
// MaskedDiscreteAttackerWrapper.action_masks() (marlon/baseline_models/env_wrappers/action_masking.py:90-110) hands MaskablePPO
// one bool per Discrete action — connect block ((src*N+tgt)*P+port)*C+cred, then local src*L+vuln, then remote
// (src*N+tgt)*R+vuln — and the policy turns it into `where(mask, logits, -1e8)` (sb3_contrib MaskableCategorical).  Materialised,
// that mask is N*N*P*C + N*L + N*N*R bytes per env and step (Chain-10 at 12/12: 14 172 B, 929 MB for 65 536 envs) written by the
// observation kernel only to be read back once.  This kernel applies it to the logits in place, straight from the 64-byte
// per-env digest the last observation left (owned-source bits by external index, discovered-node and cached-credential
// counts, blank flag: exactly what the mask bytes of THAT observation were computed from), so the mask never exists in memory:
//     logits[e, a] = mask(e, a) ? logits[e, a] : fill
// The logits are never READ: masked-out actions are overwritten, allowed ones left alone.  Bound: HBM write of the masked-out logits
// (nearly all of them).
#pragma once
#include <type_traits>

#include "mcbs_device.h"
#include "mcbs_obs.hip"
#include "mcbs_rowstore.h"

namespace mcbs {

struct LogitsGeom {        // Discrete layout of the batch, set up on the host
    uint32_t A, M, ML, RL, C, N, L, R;     // total actions, connect block, local block, connect row length P*C, credentials, nodes, local / remote ids
    FastDiv dRL, dC, dN, dL, dR;
};

// Where DigestMask finds "the node at discovery index i".  Only the local-vulnerability block asks: its bits are that node's static
// local_mask.  LiveDiscovery is the env's live discovery list (the state), which agrees with the digest only until the env moves on;
// mcbs_mask_keys.hip has the other source, a stored key row that carries the discovery order itself.
struct LiveDiscovery {
    const DevState& S;
    const mcbs_node_static* NS;
    const uint8_t* body;       // the env's body
    uint32_t e;
    __device__ __forceinline__ uint32_t local_mask(uint32_t i) const { return NS[S.disc_at(body, e, i)].local_mask; }
    static __device__ __forceinline__ LiveDiscovery of(const DevState& S, const mcbs_node_static* NS, const uint8_t* body, uint32_t e, const ObsDigest&) {
        return LiveDiscovery{S, NS, body, e};
    }
};
// The same for a batch whose digests may carry the discovery order of their OWN observation (ObsDigest::pad != 0, the list in pad2[0..1]:
// the two-agent training turn, which can re-initialise an env under an attacker observation that stands): such a digest's list is read
// instead of the live one.  The kernels below are instantiated with it as well (OWN), and mcbs_api.hip launches those instantiations
// only for a batch the training turn has stepped: every other batch runs the instructions it ran before.
struct OwnListDiscovery {
    LiveDiscovery live;
    uint32_t own_list, list_lo, list_hi;
    __device__ __forceinline__ uint32_t local_mask(uint32_t i) const {
        return live.NS[own_list ? DevState::list_nibble(list_lo, list_hi, i & 15u) : live.S.disc_at(live.body, live.e, i)].local_mask;
    }
    static __device__ __forceinline__ OwnListDiscovery of(const DevState& S, const mcbs_node_static* NS, const uint8_t* body, uint32_t e, const ObsDigest& d) {
        return OwnListDiscovery{LiveDiscovery{S, NS, body, e}, d.pad, d.pad2[0], d.pad2[1]};
    }
};
template <bool OWN> using DiscoveryOf = std::conditional_t<OWN, OwnListDiscovery, LiveDiscovery>;

// One env's digest seen as its Discrete mask: the predicates every kernel that rebuilds the mask of the last observation uses
// (mask_logits_kernel, pack_mask_kernel, the live form of masked_categorical_kernel, expand_mask_keys_kernel).  Built once per
// wavefront: everything here is uniform per wavefront (scalar loads); G and d are references to the kernel's own locals, nothing is
// copied.  Disc: the source of the node at a discovery index (above); the default is the live list.
template <typename Disc = LiveDiscovery>
struct DigestMaskOf {
    const LogitsGeom& G;
    const ObsDigest& d;        // the env's digest
    Disc disc;
    uint32_t n_disc, n_creds;              // n_disc = 0 for a blank observation
    uint64_t pp;               // credential pattern of one period, repeated to at least C + span bits; 0 when that exceeds 64

    // span: the longest run of actions the caller takes from `pp` with one shift (a logits group, or a word of 32)
    static __device__ __forceinline__ DigestMaskOf from(const LogitsGeom& G, const ObsDigest& d, const Disc& disc, uint32_t span) {
        uint64_t pp = 0;
        if (G.C + span <= 64u) {
            const uint64_t one = d.n_creds >= 64u ? ~0ull : ((1ull << d.n_creds) - 1ull);
            for (uint32_t sh = 0; sh < 64u; sh += G.C) pp |= one << sh;
        }
        return DigestMaskOf{G, d, disc, d.blank ? 0u : d.n_disc, d.n_creds, pp};
    }
    // ... through the live list of env e
    static __device__ __forceinline__ DigestMaskOf make(const DevState& S, const Topo& T, const StepCfg* __restrict__ Cp, const ObsDigest& d,
                                                        const LogitsGeom& G, uint32_t e, uint32_t span) {
        return from(G, d, Disc::of(S, reinterpret_cast<const mcbs_node_static*>(T.base + Cp->off_node), S.body + (size_t)e * S.body_stride, e, d),
                    span);
    }
    __device__ __forceinline__ uint32_t remote0() const { return G.M + G.ML; }
    __device__ __forceinline__ bool own(uint32_t s) const { return s < G.N && ((d.own_ext[(s >> 6) & 3u] >> (s & 63u)) & 1ull); }
    __device__ __forceinline__ bool pair_on(uint32_t q) const {       // row q = (source s, target t): s owned (hence discovered), t discovered
        const uint32_t s = fdiv(q, G.dN), t = q - s * G.N;
        return own(s) && t < n_disc;
    }
    // node i's local vulnerabilities as bits (0: i is not an owned, discovered node)      (env.py:653-663)
    __device__ __forceinline__ uint32_t local_bits(uint32_t i) const {
        if (!(own(i) && i < n_disc)) return 0u;
        return disc.local_mask(i);
    }
    __device__ __forceinline__ bool at(uint32_t a) const {            // one action, any region
        if (a < G.M) {                                   // connect[s][t][p][c] = on(s, t) && c < n_creds      (env.py:664-677)
            const uint32_t q = fdiv(a, G.dRL), r = a - q * G.RL, c = r - fdiv(r, G.dC) * G.C;
            return c < n_creds && pair_on(q);
        }
        if (a < remote0()) {                             // local[i][l] = owned(i) && vulnerability l applies to node i
            const uint32_t b = a - G.M, i = fdiv(b, G.dL), l = b - i * G.L;
            return (local_bits(i) >> l) & 1u;
        }
        return a < G.A && pair_on(fdiv(a - remote0(), G.dR));   // remote[s][t][r] = on(s, t)
    }
    // word w = the 32 actions [32 w, 32 w + 32) as bits (bits from A on are zero): the words pack_mask_kernel stores
    __device__ __forceinline__ uint32_t word(uint32_t w) const {
        const uint32_t remote0 = this->remote0();
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
        auto local_row = [&](uint32_t i, uint32_t k) -> uint64_t { return (uint64_t)local_bits(i) >> k; };
        const uint32_t a0 = w * 32u, a1 = a0 + 32u < G.A ? a0 + 32u : G.A;      // actions [a0, a1); bits from A on stay zero
        uint32_t m = 0;
        if (a0 < G.M) {
            // connect[s][t][p][c] = on(s, t) && c < n_creds: the dword overlaps ceil(32 / RL) + 1 rows at most, and since RL = P*C and the
            // block starts at action 0, the credential index of action a is a mod C in every row
            const uint32_t rows = rows_in(a0, a1 < G.M ? a1 : G.M, G.RL, G.dRL, whole_row);
            if (rows) m = rows & cred_bits<32u>(a0 - fdiv(a0, G.dC) * G.C);
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
    // bit i: credential (c0 + i) mod C is cached, i < SPAN (the SPAN this was made with).  One credential period plus SPAN bits fits
    // 64 bits (Chain-10: C = 12, ToyCtf: 10): `pp` = the periodic pattern "n_creds ones, C - n_creds zeros" as a bit string, so the
    // bits are one shift; else the index just counts on modulo C
    template <uint32_t SPAN>
    __device__ __forceinline__ uint32_t cred_bits(uint32_t c0) const {
        if (G.C + SPAN <= 64u) return (uint32_t)(pp >> c0);
        uint32_t m = 0, c = c0;
        for (uint32_t i = 0; i < SPAN; ++i) {
            m |= (uint32_t)(c < n_creds) << i;
            c = c + 1u == G.C ? 0u : c + 1u;
        }
        return m;
    }
};
using DigestMask = DigestMaskOf<>;

// LT: float, or uint16_t for 16-bit logits (bf16 patterns are only replaced).  GW: actions per group (mcbs_rowstore.h).
//
// One WAVEFRONT per env (four independent ones per workgroup: no LDS, no barrier).  Nearly every span holds no allowed action at all (a few dozen of Chain-10's
// 14 172 actions are allowed): for each chunk of 64 spans, lane k first decides whether span k is LIVE — some (source, target) row
// overlapping it is on, or it touches the local block — and one ballot turns that into a scalar mask; a span that is not live costs
// one scalar bit test and one store.  (Measured on the way here, 65 536 Chain-10 envs, fp32 / bf16 logits, us per launch: read-modify-write with one
// division chain per group 1 390 / -; write-only 1 008 / 882; row bits in LDS + span bits per four-wavefront workgroup 785 / 595 — the
// same time for half the bytes: bound by instruction issue and the two barriers; a persistent grid of such workgroups 950; this
// kernel 745 / 414.  Reference points on the same buffer: a plain fill 536 / 270, this store pattern with no mask work at all 700 / 367,
// torch.where with a materialised mask 1 440 / 830.  Non-temporal stores: no change.  tools/bench_logits.py.)
template <typename LT, uint32_t GW, bool VEC, bool OWN = false>
__global__ __launch_bounds__(256) void mask_logits_kernel(DevState S, Topo T, const StepCfg* __restrict__ Cp, const ObsDigest* __restrict__ digest,
                                                          LT* __restrict__ logits, size_t row_stride, LT fill, LogitsGeom G) {
    using RG = RowGroups<LT, GW, VEC>;
    constexpr uint32_t ALL = RG::ALL;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t e = blockIdx.y * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // wave-uniform
    if (e >= S.E) return;
    const ObsDigest d = digest[e];                       // uniform per wavefront: scalar loads
    const auto M = DigestMaskOf<DiscoveryOf<OWN>>::make(S, T, Cp, d, G, e, GW);
    const uint32_t remote0 = M.remote0();
    LT* row = logits + (size_t)e * row_stride;
    // bit j: the (source, target) row that action rel + j of a block of `rowlen`-long rows belongs to is on (rowlen >= GW: two rows at most)
    auto rows_mask = [&](uint32_t rel, const FastDiv& dRow, uint32_t rowlen, uint32_t& r0) -> uint32_t {
        const uint32_t q0 = fdiv(rel, dRow);
        r0 = rel - q0 * rowlen;
        const uint32_t first = rowlen - r0 < GW ? rowlen - r0 : GW, lo = (1u << first) - 1u;
        return (M.pair_on(q0) ? lo : 0u) | ((first < GW && M.pair_on(q0 + 1u)) ? (ALL & ~lo) : 0u);
    };
    const uint32_t sh = RG::shift(row);
    const uint32_t nspan = RG::nspan(G.A, sh);
    for (uint32_t c0s = blockIdx.x * 64u; c0s < nspan; c0s += gridDim.x * 64u) {      // chunks of 64 spans
        bool live = false;                               // lane k: span c0s + k holds an allowed action (or might)
        {
            const uint32_t s0 = RG::span_first(c0s + lane, sh), s1 = RG::span_last(c0s + lane, sh, G.A);      // its actions [s0, s1)
            auto any_row = [&](uint32_t lo, uint32_t hi, const FastDiv& dRow) {                    // rows of actions lo .. hi (relative to their block)
                const uint32_t qa = fdiv(lo, dRow), qb = fdiv(hi, dRow);
                if (qb - qa > 8u) { live = true; return; }
                for (uint32_t q = qa; q <= qb; ++q) live |= M.pair_on(q);
            };
            if (s0 < s1) {
                if (s0 < G.M) any_row(s0, (s1 < G.M ? s1 : G.M) - 1u, G.dRL);
                if (s1 > G.M && s0 < remote0) live = true;                                         // local block: per-node vulnerability masks
                if (s1 > remote0) any_row((s0 > remote0 ? s0 : remote0) - remote0, s1 - 1u - remote0, G.dR);
            }
        }
        const uint64_t live_mask = __ballot(live);
        const uint32_t ns = nspan - c0s < 64u ? nspan - c0s : 64u;
#pragma unroll 4
        for (uint32_t j = 0; j < ns; ++j) {
            const uint32_t g = (c0s + j) * 64u + lane;
            const uint32_t a0 = RG::a0(g, sh);
            if (RG::outside(g, sh, G.A)) continue;
            uint32_t m = 0, r0;                          // bit j: action a0 + j is allowed
            if (!((live_mask >> j) & 1ull)) {            // scalar test
            } else if (a0 + GW <= G.M && G.RL >= GW) {
                // the whole group lies in the connect block: at most two (source, target) rows, each on or off as a whole; within an
                // on row the credential index just counts on modulo C (RL is a multiple of C)
                const uint32_t rows = rows_mask(a0, G.dRL, G.RL, r0);
                if (rows) m = M.template cred_bits<GW>(r0 - fdiv(r0, G.dC) * G.C) & rows;
            } else if (a0 >= remote0 && a0 + GW <= G.A && G.R >= GW) {
                m = rows_mask(a0 - remote0, G.dR, G.R, r0);     // the whole group lies in the remote block: remote[s][t][r] = on(s, t)
            } else {
#pragma unroll
                for (uint32_t i = 0; i < GW; ++i) m |= (uint32_t)M.at(a0 + i) << i;
            }
            // write-only: allowed actions are left alone — the logits are never read
            store_fill_group<LT, GW, VEC>(row, a0, ~m & RG::in_row(a0, G.A), fill);
        }
    }
}

} // namespace mcbs
