// mcbs_defender_obs_packing.hip — the learned defender's observation as one bit per MultiBinary element (include/mcbs.h "packed
// defender observations"): W_def = ceil(F / 32) words per row, F = 6N + N + 6N + S, bit c = column c of DefenderVecEnv.features():
//     [0, 6N)     incoming_firewall_status  column 6n + k
//     [6N, 7N)    infected_nodes            column 6N + n
//     [7N, 13N)   outgoing_firewall_status  column 7N + 6n + k
//     [13N, F)    services_status           column 13N + s
// bit c & 31 of word c >> 5 (the packed action masks' convention); bits from F on are zero.
//
//   defender_turn_post_packed_kernel : defender_turn_post_kernel (mcbs_defend.hip) with the packed store side: the same turn, the same
//                                      shaping, an LDS stage of finished words — and W_def words per env leave instead of 13N + S bytes
//   defender_obs_packed_kernel       : the rows of the live state, any N and any words per set: a thread per (env, word)
//   pack / unpack / encode           : dense int8 rows <-> packed rows, and either of them -> the float feature rows
// Services never change state, so their bits are a W_def-word image built on the host when the batch is created (DefPackGeom::svc):
// the kernels that read the live state OR it in.  Everything here is written with plain vector stores.
#pragma once
#include "mcbs_device.h"
#include "mcbs_defend.hip"
#include "mcbs_rowstore.h"

namespace mcbs {

struct DefPackGeom {
    uint32_t N, S, F, W;                 // nodes, services, columns, words of a row
    const uint32_t* svc;                 // [W] the services' bits of a row (device; the batch's own)
    FastDiv dW;
};
constexpr uint32_t DEF_WMAX = (13u * DEF_NMAX + DEF_SMAX + 31u) / 32u;     // words of a row the turn kernels write themselves: 21
struct DefDense { const int8_t* f[4]; };     // the four fields in COLUMN order: incoming, infected, outgoing, services (NULL: skipped)
struct DefDenseOut { int8_t* f[4]; };

// column c < F of a row -> its field (0 .. 3) and its element in that field's row; row lengths by field: 6N, N, 6N, S
__device__ __forceinline__ uint32_t def_field_of(const DefPackGeom& G, uint32_t c, uint32_t& at, uint32_t& len) {
    const uint32_t N = G.N;
    if (c < 6u * N) { at = c; len = 6u * N; return 0u; }
    if (c < 7u * N) { at = c - 6u * N; len = N; return 1u; }
    if (c < 13u * N) { at = c - 7u * N; len = 6u * N; return 2u; }
    at = c - 13u * N; len = G.S;
    return 3u;
}

// v's bits from bit `pos` of a word upwards (pos may be negative: the word starts inside v); what falls outside the word is dropped
__device__ __forceinline__ uint32_t def_place(uint32_t v, int pos) {
    return pos >= 0 ? (pos < 32 ? v << pos : 0u) : (pos > -32 ? v >> (-pos) : 0u);
}

// Word w of a row, the three per-node fields only (the caller ORs the services in): inst_bits(n0, cnt) = cnt <= 32 bits of the
// agent-installed set from node n0, fw6(n, dir) = the six rule-name bits of node n's incoming (dir 0) or outgoing (dir 1) list
template <class Inst, class Fw>
__device__ __forceinline__ uint32_t def_obs_word(const uint32_t N, const uint32_t w, Inst inst_bits, Fw fw6) {
    const uint32_t c0 = w * 32u, c1 = c0 + 32u;
    uint32_t acc = 0;
    // (a word covers at most seven nodes' six bits: a fixed, unrolled run of seven, so that the seven reads behind fw6 are issued
    // together — a loop over the run's own length waits for every read in turn)
    auto fw_field = [&](const uint32_t base, const uint32_t dir) {
        const uint32_t lo = c0 > base ? c0 : base, hi = c1 < base + 6u * N ? c1 : base + 6u * N;
        if (lo >= hi) return;
        const uint32_t n0 = (lo - base) / 6u, n1 = (hi - 1u - base) / 6u;
        uint32_t v[7];
#pragma unroll
        for (uint32_t k = 0; k < 7u; ++k) v[k] = fw6(n0 + k <= n1 ? n0 + k : n1, dir);
#pragma unroll
        for (uint32_t k = 0; k < 7u; ++k)
            if (n0 + k <= n1) acc |= def_place(v[k] & 63u, (int)(base + 6u * (n0 + k)) - (int)c0);
    };
    fw_field(0u, 0u);
    {
        const uint32_t base = 6u * N, lo = c0 > base ? c0 : base, hi = c1 < base + N ? c1 : base + N;
        if (lo < hi) acc |= inst_bits(lo - base, hi - lo) << (lo - c0);
    }
    fw_field(7u * N, 1u);
    return acc;
}

// ---- the turn with the packed store side (variant.fused_defender_obs: N <= 32, W <= DEF_WMAX) ----
// The lane that took env e's turn parks the env's finished WORDS in LDS (slot * W + w): it walks the nodes once, as defender_park does,
// and pushes the six incoming bits of each node into one bit stream (from bit 0, followed by the N agent-installed bits) and the six
// outgoing bits into a second one (from bit 7N); a stream hands a word over whenever it has 32 bits.  The two streams meet inside one
// word, so the row is cleared first and every word is OR-ed in.  N is uniform, so is every branch here.  After the barrier the
// workgroup's n_env * W words leave env-major, OR-ed with the services' words: consecutive threads write consecutive words, four
// words and one 16-byte store per thread where the rows follow each other without a gap (row_words == W: the region of a workgroup
// starts on a 16-byte boundary, 128 * W words from the base), else word by word.
// (The first form parked defender_park's raw bits and had thread t build word (env, w) after the barrier, a node's six bits at a
// time: 17.1 us per ToyCtf turn at 16 384 envs against 12.9 us for the int8 kernel — some 150 vector instructions per word, eight
// words on the slowest thread.  profiles/defender_obs_packing.md has both.)
template <int WT>
__device__ __forceinline__ void defender_park_words(const DevState& S, const Topo& T, const uint32_t e, const uint32_t W, uint32_t* __restrict__ row) {
    const uint32_t N = S.N;
    const uint8_t* body = S.body + (size_t)e * S.body_stride;
    const uint16_t* fw = reinterpret_cast<const uint16_t*>(body + S.off_fw);
    const mcbs_node_static* NS = reinterpret_cast<const mcbs_node_static*>(T.base + T.H().off_node);
    for (uint32_t w = 0; w < W; ++w) row[w] = 0u;
    uint64_t a = 0, b = 0;                                           // the streams' pending bits, fa / fb of them, for words wa / wb
    uint32_t fa = 0, wa = 0, fb = (7u * N) & 31u, wb = (7u * N) >> 5;
    for (uint32_t n = 0; n < N; ++n) {                               // (uniform: node statics through the scalar cache)
        const uint32_t lists = NS[n].fw_lists;
        a |= (uint64_t)(fw[lists & 0xFFFFu] & 63u) << fa;
        b |= (uint64_t)(fw[lists >> 16] & 63u) << fb;
        fa += 6u; fb += 6u;
        if (fa >= 32u) { row[wa++] |= (uint32_t)a; a >>= 32; fa -= 32u; }
        if (fb >= 32u) { row[wb++] |= (uint32_t)b; b >>= 32; fb -= 32u; }
    }
    const uint32_t inst = (uint32_t)S.get(M_INST, 0u, e) & (N >= 32u ? ~0u : (1u << N) - 1u);      // N <= 32: the low bits of word 0
    a |= (uint64_t)inst << fa;
    fa += N;
    if (fa >= 32u) { row[wa++] |= (uint32_t)a; a >>= 32; fa -= 32u; }
    if (fa) row[wa] |= (uint32_t)a;                                  // (ends at bit 7N, where the second stream began)
    if (fb) row[wb] |= (uint32_t)b;                                  // (ends at bit 13N: below W * 32 whenever a bit is pending)
}

template <uint32_t ENVS, uint32_t THREADS>
__device__ __forceinline__ void defender_stream_words(const uint32_t E, const DefPackGeom& G, uint32_t* __restrict__ out, const size_t row_words,
                                                      const uint32_t tid, const uint32_t e0, const uint32_t* words, const uint32_t* svc) {
    const uint32_t W = G.W;
    const uint32_t n_env = E - e0 < ENVS ? E - e0 : ENVS;
    const uint32_t R = n_env * W;
    if (row_words == W) {                                            // uniform
        uint32_t* p = out + (size_t)e0 * W;
        for (uint32_t x0 = tid * 4u; x0 < R; x0 += THREADS * 4u) {
            uint32_t w = x0 - fdiv(x0, G.dW) * W, v[4];
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                v[j] = x0 + j < R ? words[x0 + j] | svc[w] : 0u;
                if (++w == W) w = 0;
            }
            if (x0 + 4u <= R) *reinterpret_cast<uint4*>(p + x0) = make_uint4(v[0], v[1], v[2], v[3]);
            else {
#pragma unroll
                for (uint32_t j = 0; j < 4u; ++j)
                    if (x0 + j < R) p[x0 + j] = v[j];
            }
        }
    } else {
        for (uint32_t x = tid; x < R; x += THREADS) {
            const uint32_t env = fdiv(x, G.dW), w = x - env * W;
            out[(size_t)(e0 + env) * row_words + w] = words[x] | svc[w];
        }
    }
}

template <int WT>
__global__ __launch_bounds__(128) void defender_turn_post_packed_kernel(DevState S, Topo T, const StepCfg* __restrict__ Cp, const int64_t* actions,
                                                                        mcbs_defender_wrapper_buffers w, mcbs_defender_wrapper_cfg c, DefPackGeom G,
                                                                        uint32_t* __restrict__ out, size_t row_words) {
    __shared__ uint32_t words[DEF_WG * DEF_WMAX];                    // 10.5 KB: slot * W + w
    __shared__ uint32_t svc[DEF_WMAX];                               // the services' words of a row: fetched before the turn, whose loads hide this one
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = e < S.E;
    const uint32_t svc_word = threadIdx.x < G.W ? G.svc[threadIdx.x] : 0u;
    if (valid) {
        bool ok, evicted;
        double avail;
        defender_turn<WT>(S, T, *Cp, actions, e, ok, avail, evicted);
        const_cast<uint8_t*>(w.valid)[e] = ok ? 1 : 0;
        const_cast<double*>(w.availability)[e] = avail;
        const_cast<uint8_t*>(w.evicted)[e] = evicted ? 1 : 0;
        defender_shape(w, c, e, ok, avail, evicted);
        defender_park_words<WT>(S, T, e, G.W, words + threadIdx.x * G.W);
    }
    if (threadIdx.x < G.W) svc[threadIdx.x] = svc_word;
    __syncthreads();
    defender_stream_words<DEF_WG, DEF_WG>(S.E, G, out, row_words, threadIdx.x, blockIdx.x * DEF_WG, words, svc);
}

// ---- the rows of the live state, any topology: one thread per (env, word) ----
__global__ __launch_bounds__(256) void defender_obs_packed_kernel(DevState S, Topo T, DefPackGeom G, uint32_t* __restrict__ out, size_t row_words) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;        // (E * W < 2^32: checked by the host)
    if (g >= S.E * G.W) return;
    const uint32_t e = fdiv(g, G.dW), w = g - e * G.W;
    const uint16_t* fw = reinterpret_cast<const uint16_t*>(S.body + (size_t)e * S.body_stride + S.off_fw);
    const mcbs_node_static* NS = reinterpret_cast<const mcbs_node_static*>(T.base + T.H().off_node);
    const uint32_t word = G.svc[w] | def_obs_word(S.N, w,
        [&](uint32_t n0, uint32_t cnt) {                             // cnt <= 32 bits from node n0: they span at most two 64-bit words of the set
            const uint32_t q = n0 >> 6, s = n0 & 63u;
            uint64_t x = S.get(M_INST, q, e) >> s;
            if (s + cnt > 64u) x |= S.get(M_INST, q + 1u, e) << (64u - s);
            return (uint32_t)x & (cnt >= 32u ? ~0u : (1u << cnt) - 1u);
        },
        [&](uint32_t n, uint32_t dir) {
            const uint32_t lists = NS[n].fw_lists;
            return (uint32_t)fw[dir ? lists >> 16 : lists & 0xFFFFu];
        });
    out[(size_t)e * row_words + w] = word;
}

// ---- dense int8 rows -> packed rows: one thread per (row, word); a bit is set where the byte is not zero ----
__global__ __launch_bounds__(256) void pack_defender_obs_kernel(DefPackGeom G, DefDense src, uint64_t n_rows, uint32_t* __restrict__ out, size_t row_words) {
    const uint32_t lane_w = threadIdx.x % 8u, lane_r = threadIdx.x / 8u;                  // 32 rows x 8 words per pass of a workgroup
    for (uint64_t i = (uint64_t)blockIdx.x * 32u + lane_r; i < n_rows; i += (uint64_t)gridDim.x * 32u) {
        for (uint32_t w = lane_w; w < G.W; w += 8u) {
            uint32_t acc = 0;
            for (uint32_t j = 0; j < 32u; ++j) {
                const uint32_t c = w * 32u + j;
                if (c >= G.F) break;
                uint32_t at, len;
                const uint32_t k = def_field_of(G, c, at, len);
                acc |= (uint32_t)(src.f[k][i * len + at] != 0) << j;
            }
            out[i * row_words + w] = acc;
        }
    }
}

// ---- packed rows -> dense int8 rows (0 / 1), through an optional row index: one thread per (row, word) ----
__global__ __launch_bounds__(256) void unpack_defender_obs_kernel(DefPackGeom G, const uint32_t* __restrict__ packed, size_t row_words,
                                                                  const int64_t* __restrict__ index, uint64_t n_source_rows, uint64_t n_rows, DefDenseOut dst) {
    const uint32_t lane_w = threadIdx.x % 8u, lane_r = threadIdx.x / 8u;
    for (uint64_t i = (uint64_t)blockIdx.x * 32u + lane_r; i < n_rows; i += (uint64_t)gridDim.x * 32u) {
        const int64_t s = index ? index[i] : (int64_t)i;
        const bool inside = s >= 0 && (uint64_t)s < n_source_rows;   // an index outside the storage reads nothing: the row is all zero
        for (uint32_t w = lane_w; w < G.W; w += 8u) {
            const uint32_t bits = inside ? packed[(uint64_t)s * row_words + w] : 0u;
            for (uint32_t j = 0; j < 32u; ++j) {
                const uint32_t c = w * 32u + j;
                if (c >= G.F) break;
                uint32_t at, len;
                const uint32_t k = def_field_of(G, c, at, len);
                if (dst.f[k]) dst.f[k][i * len + at] = (int8_t)((bits >> j) & 1u);
            }
        }
    }
}

// ---- the float feature rows (0.0 / 1.0, F columns) from dense int8 rows or from packed rows, through an optional row index ----
// The store side of mcbs_features.hip: a thread owns a GROUP of GW columns = one store of 16 (8, 4) bytes, consecutive threads own
// consecutive groups of a row.  A ToyCtf row is 18 bf16 groups, so a wavefront per row would leave 46 lanes idle: the rows are dealt
// to the workgroup's 256 threads RB = 256 / groups at a time (14 bf16 ToyCtf rows: 252 threads store), and rows of more than 256
// groups take one row per pass.  A group's GW bits come from two words of the packed row (L1 / L2 hits: 20 bytes a row), or from GW
// bytes of the dense fields.  Write-only: every column below F is stored, nothing from F on is touched.
// store_group of mcbs_rowstore.h, restated: one 16-, 8- or 4-byte store for a whole group, element by element below `limit` at the
// row's end and always without VEC.  (A copy on purpose: instantiating the shared template here as well changed the instructions
// hipcc emits for the attacker's GW = 2 feature kernels, which this file has no business touching.)
template <typename T, uint32_t GW, bool VEC>
__device__ __forceinline__ void def_store_group(T* __restrict__ row, uint32_t a0, uint32_t limit, const T (&v)[GW]) {
    constexpr uint32_t NB = GW * (uint32_t)sizeof(T);
    if (VEC && a0 + GW <= limit) {
        uint32_t w[(NB + 3u) / 4u];
#pragma unroll
        for (uint32_t k = 0; k < (NB + 3u) / 4u; ++k) {
            if constexpr (sizeof(T) == 4) w[k] = (uint32_t)v[k];
            else w[k] = (uint32_t)v[2u * k] | ((uint32_t)v[2u * k + 1u] << 16);
        }
        if constexpr (NB == 16u) *reinterpret_cast<uint4*>(row + a0) = make_uint4(w[0], w[1], w[2], w[3]);
        else if constexpr (NB == 8u) *reinterpret_cast<uint2*>(row + a0) = make_uint2(w[0], w[1]);
        else *reinterpret_cast<uint32_t*>(row + a0) = w[0];
    } else {
#pragma unroll
        for (uint32_t k = 0; k < GW; ++k)
            if (a0 + k < limit) row[a0 + k] = v[k];
    }
}

template <typename T, uint32_t GW, bool VEC, bool PACKED>
__global__ __launch_bounds__(256) void encode_defender_features_kernel(DefPackGeom G, DefDense dense, const uint32_t* __restrict__ packed, size_t row_words,
                                                                       const int64_t* __restrict__ index, uint64_t n_source_rows, uint64_t n_rows,
                                                                       T* __restrict__ out, size_t out_stride, T one, uint32_t ngroup, uint32_t RB, FastDiv dG,
                                                                       int32_t* __restrict__ bad_rows) {
    const uint64_t n_pass = (n_rows + RB - 1u) / RB;
    for (uint64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
        for (uint32_t x = threadIdx.x; x < RB * ngroup; x += 256u) {
            const uint32_t r = fdiv(x, dG), g = x - r * ngroup;
            const uint64_t i = pass * RB + r;
            if (i >= n_rows) break;
            const int64_t s = index ? index[i] : (int64_t)i;
            const bool inside = s >= 0 && (uint64_t)s < n_source_rows;
            if (!inside && g == 0u && bad_rows) atomicAdd(bad_rows, 1);
            const uint32_t j0 = g * GW;
            uint32_t m = 0;                                          // bit k: column j0 + k is 1
            if (inside) {
                if (PACKED) {
                    const uint32_t* row = packed + (uint64_t)s * row_words;
                    const uint32_t w = j0 >> 5, sh = j0 & 31u;
                    m = row[w] >> sh;
                    if (sh + GW > 32u && w + 1u < G.W) m |= row[w + 1u] << (32u - sh);
                    const uint32_t live = G.F - j0;                  // (j0 < F) columns from j0 that exist: stored rows may carry anything past F
                    m &= live >= GW ? (1u << GW) - 1u : (1u << live) - 1u;
                } else {
#pragma unroll
                    for (uint32_t k = 0; k < GW; ++k) {
                        if (j0 + k >= G.F) break;
                        uint32_t at, len;
                        const uint32_t f = def_field_of(G, j0 + k, at, len);
                        m |= (uint32_t)(dense.f[f][(uint64_t)s * len + at] != 0) << k;
                    }
                }
            }
            T v[GW];
#pragma unroll
            for (uint32_t k = 0; k < GW; ++k) v[k] = ((m >> k) & 1u) ? one : (T)0;
            def_store_group<T, GW, VEC>(out + i * out_stride, j0, G.F, v);
        }
    }
}

} // namespace mcbs
