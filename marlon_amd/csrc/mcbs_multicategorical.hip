// mcbs_multicategorical.hip — the MultiDiscrete action head of a PPO policy on the device, forward and backward (include/mcbs.h
// "MultiDiscrete head").
//
// Stable-Baselines3's MultiCategoricalDistribution (the defender's MultiDiscrete([5,N,N,6,2,N,6,2,N,3,N,3]), defend_wrapper.py:162-195, and
// the attacker's unmasked MultiDiscrete([3,N,L,N,N,R,N,N,P,C]), attack_wrapper.py:206-227) splits a row of A = sum nvec logits into D
// segments, builds a Categorical per segment and sums their log_prob and entropy.  Here a row is one pass: 30 MB of logits read once.
//
// One LANE per (row, dimension): a 256-lane workgroup serves R = floor(256 / D) rows at a time, lane r * D + d walks dimension d of row r,
// and grid-strides over groups of R rows.  The dimensions are 2-12 wide in the reference's environments, so a lane's walk is one short
// serial chain in ascending index order and no sum ever crosses lanes:
//   walk 1   m = the largest logit and its lowest index
//   walk 2   Z = sum exp(x - m), T = sum (x - m) exp(x - m): per block of 32 consecutive indices from +0 in ascending index order, the
//            block totals from +0 in ascending block order (dimensions of up to 32 choices: one serial chain)
//   walk 3   (SAMPLE) the running sum of walk 2 again — the earlier blocks' total plus the block's partial sum — stopped at the first
//            index at which it exceeds u * Z
// Then the row's first lane adds the D partial log-probs and entropies from +0 in ascending d (through LDS: rows straddle wavefronts).
// The order depends on nvec alone — not on n_rows, strides, alignment, dtype, mode or on which of the two paths below ran.
//
// STAGED (A * R floats fit MC_LDS_FLOATS; R is cut down to make a row of up to 8 192 logits fit): the workgroup's R rows are first copied
// into LDS as float32, with 16-byte loads where the rows are contiguous (row_stride == A; the run's unaligned head and tail go element by
// element), else element by element with consecutive lanes on consecutive elements.  The gradient is assembled in the same LDS words
// (lane (r, d) owns elements [off_d, off_d + nvec[d]) of row r, reads each logit before it overwrites it) and leaves the same way.
// DIRECT (wider rows, or no logits at all): every lane reads its logits from global memory and writes its gradients there.
// Both paths feed the same float32 values to the same walks (McWalk), so the results are the same bit for bit.
#pragma once
#include "mcbs_categorical.hip"
#include "mcbs_rowstore.h"

namespace mcbs {

constexpr uint32_t MC_MAX_DIMS = 16u;                  // = MCBS_MAX_ACTION_DIMS
constexpr uint32_t MC_DOMAIN = 0x3C47E6A1u;            // = MCBS_MULTICATEGORICAL_PHILOX_DOMAIN
constexpr uint32_t MC_LDS_FLOATS = 8192u;              // staged logits per workgroup: 32 KiB, four workgroups per CU
constexpr uint32_t MC_LANES = 256u;
constexpr uint32_t MC_BLOCK = 32u;                     // indices per block of a dimension's sums (a serial chain of 1 000 terms drifts by tens of ulp)
constexpr uint32_t MC_LDS_HEAD = 3u * MC_LANES;        // floats in front of the staged rows: the lanes' partial log-probs, entropies, flags

struct McGeom {                // part of the argument block: the host's nvec and its prefix sums
    uint32_t nvec[MC_MAX_DIMS];
    uint32_t off[MC_MAX_DIMS];
    uint32_t D, A, R;          // R: rows per workgroup pass, R * D <= 256 (STAGED: R * A <= MC_LDS_FLOATS)
};

struct McIO {
    const void* logits;        // [n, row_stride] or NULL (the uniform law)
    size_t row_stride;
    int64_t* actions;          // [n, D]
    float* log_prob;
    float* entropy;            // nullable
    const float* uniforms;     // [n, D], nullable
    uint32_t* bad_actions;     // nullable
    uint64_t seed, step, key_base, n_rows;
    uint32_t mode;
};

struct McGradIO {
    const void* logits;        // [n, row_stride]
    size_t row_stride;
    const int64_t* actions;    // [n, D]
    const float* g_lp;         // nullable: all zeros
    const float* g_ent;        // nullable: all zeros
    void* grad;                // [n, grad_stride], the dtype of logits
    size_t grad_stride;
    uint64_t n_rows;
};

// m, its lowest index, Z and the entropy sum of one dimension: the walks every kernel here shares.  x(a) = the a-th logit as float32.
struct McWalk {
    float m, Z, T;
    uint32_t arg;
    template <typename X>
    __device__ __forceinline__ McWalk(const X& x, uint32_t n) {
        m = x(0u); arg = 0u;
        for (uint32_t a = 1u; a < n; ++a) {              // ascending: `>` keeps the lowest index of equal logits
            const float v = x(a);
            if (v > m) { m = v; arg = a; }
        }
        Z = 0.f; T = 0.f;
        for (uint32_t a0 = 0u; a0 < n; a0 += MC_BLOCK) {     // blocks of MC_BLOCK indices: a block's terms, then the block totals, each from +0
            const uint32_t a1 = a0 + MC_BLOCK < n ? a0 + MC_BLOCK : n;
            float s = 0.f, t = 0.f;
            for (uint32_t a = a0; a < a1; ++a) {
                const float d = x(a) - m;
                const float ex = expf(d);
                s += ex;
                t += ex > 0.f ? d * ex : 0.f;            // (-inf) * 0 is no term of the entropy
            }
            Z += s;
            T += t;
        }
    }
};

__device__ __forceinline__ void mc_unpack(const uint4& q, float (&v)[4]) {
    v[0] = __uint_as_float(q.x); v[1] = __uint_as_float(q.y); v[2] = __uint_as_float(q.z); v[3] = __uint_as_float(q.w);
}
__device__ __forceinline__ void mc_unpack(const uint4& q, float (&v)[8]) {     // eight bfloat16
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) v[k] = __uint_as_float(((w[k >> 1] >> ((k & 1u) * 16u)) & 0xFFFFu) << 16);
}

// rows [i0, i0 + rows) of L -> xs[row * A + col] as float32
template <typename LT>
__device__ __forceinline__ void mc_stage(float* __restrict__ xs, const LT* __restrict__ L, uint64_t i0, uint32_t rows, uint32_t A, size_t stride,
                                         uint32_t tid) {
    constexpr uint32_t GW = 16u / sizeof(LT);
    const uint32_t N = rows * A;
    const LT* p = L + i0 * stride;
    if (stride == A && reinterpret_cast<uintptr_t>(p) % sizeof(LT) == 0u) {
        // one contiguous run: whole 16-byte groups from the first 16-byte boundary on, the rest element by element
        uint32_t head = (uint32_t)(((16u - (reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / sizeof(LT));
        head = head < N ? head : N;
        const uint32_t ngroups = (N - head) / GW, tail0 = head + ngroups * GW;
        for (uint32_t j = tid; j < ngroups; j += MC_LANES) {
            const uint32_t e = head + j * GW;
            float v[GW];
            mc_unpack(*reinterpret_cast<const uint4*>(p + e), v);
#pragma unroll
            for (uint32_t k = 0; k < GW; ++k) xs[e + k] = v[k];
        }
        for (uint32_t j = tid; j < head + (N - tail0); j += MC_LANES) {
            const uint32_t e = j < head ? j : tail0 + (j - head);
            xs[e] = cat_logit(p, e);
        }
    } else {
        for (uint32_t j = tid; j < N; j += MC_LANES) {
            const uint32_t row = j / A, col = j - row * A;
            xs[j] = cat_logit(p + (size_t)row * stride, col);
        }
    }
}

__device__ __forceinline__ void mc_put(float* p, float v) { *p = v; }
__device__ __forceinline__ void mc_put(uint16_t* p, float v) { *p = (uint16_t)bf16_bits(v); }

// xs[row * A + col] -> rows [i0, i0 + rows) of Gr in its dtype; every element [row, 0 .. A) exactly once, nothing beyond
template <typename LT>
__device__ __forceinline__ void mc_unstage(const float* __restrict__ xs, LT* __restrict__ Gr, uint64_t i0, uint32_t rows, uint32_t A, size_t stride,
                                           uint32_t tid) {
    constexpr uint32_t GW = 16u / sizeof(LT);
    const uint32_t N = rows * A;
    LT* p = Gr + i0 * stride;
    if (stride == A && reinterpret_cast<uintptr_t>(p) % sizeof(LT) == 0u) {
        uint32_t head = (uint32_t)(((16u - (reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / sizeof(LT));
        head = head < N ? head : N;
        const uint32_t ngroups = (N - head) / GW, tail0 = head + ngroups * GW;
        for (uint32_t j = tid; j < ngroups; j += MC_LANES) {
            const uint32_t e = head + j * GW;
            uint4 q;
            if constexpr (sizeof(LT) == 4) {
                q = make_uint4(__float_as_uint(xs[e]), __float_as_uint(xs[e + 1u]), __float_as_uint(xs[e + 2u]), __float_as_uint(xs[e + 3u]));
            } else {
                uint32_t w[4];
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) w[k] = bf16_bits(xs[e + 2u * k]) | (bf16_bits(xs[e + 2u * k + 1u]) << 16);
                q = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *reinterpret_cast<uint4*>(p + e) = q;
        }
        for (uint32_t j = tid; j < head + (N - tail0); j += MC_LANES) {
            const uint32_t e = j < head ? j : tail0 + (j - head);
            mc_put(p + e, xs[e]);
        }
    } else {
        for (uint32_t j = tid; j < N; j += MC_LANES) {
            const uint32_t row = j / A, col = j - row * A;
            mc_put(p + (size_t)row * stride + col, xs[j]);
        }
    }
}

template <typename LT, bool STAGED>
__global__ __launch_bounds__(256) void multicategorical_kernel(McGeom G, McIO io) {
    extern __shared__ __attribute__((aligned(16))) float mc_smem[];
    float* p_lp = mc_smem;
    float* p_H = mc_smem + MC_LANES;
    uint32_t* p_bad = reinterpret_cast<uint32_t*>(mc_smem + 2u * MC_LANES);
    float* xs = mc_smem + MC_LDS_HEAD;
    const uint32_t tid = threadIdx.x, D = G.D, A = G.A, R = G.R;
    const uint32_t r = tid / D, d = tid - r * D;
    const bool lane_used = r < R;
    const uint32_t n = lane_used ? G.nvec[d] : 1u, off = lane_used ? G.off[d] : 0u;
    const LT* L = static_cast<const LT*>(io.logits);
    const uint32_t mode = io.mode;
    const uint64_t groups = (io.n_rows + R - 1u) / R;
    for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {           // workgroup-uniform
        const uint64_t i0 = g * R;
        const uint32_t rows = io.n_rows - i0 < R ? (uint32_t)(io.n_rows - i0) : R;
        __syncthreads();                                                  // the previous pass has read its partial results and its rows
        if constexpr (STAGED) {
            mc_stage<LT>(xs, L, i0, rows, A, io.row_stride, tid);
            __syncthreads();
        }
        const bool on = r < rows;
        const uint64_t i = i0 + r;
        if (on) {
            uint32_t u24 = 0u;
            if (mode == CAT_SAMPLE && n > 1u) {
                if (io.uniforms) {
                    const float uf = io.uniforms[i * D + d] * 16777216.0f;
                    u24 = uf >= 16777215.0f ? 16777215u : (uf >= 0.f ? (uint32_t)uf : 0u);
                } else {
                    const uint64_t key = io.key_base + i;
                    uint32_t w[4];
                    philox4x32_10((uint32_t)key, (uint32_t)(key >> 32), (uint32_t)io.step, (uint32_t)(io.step >> 32) | ((d >> 2) << 16),
                                  (uint32_t)io.seed ^ MC_DOMAIN, (uint32_t)(io.seed >> 32), w);
                    const uint32_t k = d & 3u;
                    u24 = (k == 0u ? w[0] : k == 1u ? w[1] : k == 2u ? w[2] : w[3]) >> 8;
                }
            }
            int64_t act = 0;
            bool bad = false;
            if (mode == CAT_EVALUATE) {
                act = io.actions[i * D + d];
                bad = act < 0 || act >= (int64_t)n;
            }
            float lp = 0.f, H = 0.f;
            if (n == 1u) {
                // a dimension of one choice: exactly nothing
            } else if (!L) {
                // the uniform law, in integers
                const float lg = cat_log((float)n);
                lp = -lg; H = lg;
                if (mode == CAT_SAMPLE) act = (int64_t)(((uint64_t)u24 * n) >> 24);
            } else {
                const LT* row = L + i * io.row_stride + off;
                const float* xr = xs + r * A + off;
                auto x = [&](uint32_t a) -> float {
                    if constexpr (STAGED) return xr[a]; else return cat_logit(row, a);
                };
                const McWalk w(x, n);
                const float logZ = cat_log(w.Z);
                H = logZ - w.T / w.Z;
                uint32_t sel = 0u;
                if (mode == CAT_ARGMAX) {
                    sel = w.arg;
                } else if (mode == CAT_EVALUATE) {
                    sel = bad ? 0u : (uint32_t)act;
                } else {
                    // inverse CDF: the running sum that produced Z, stopped at the first index where it exceeds u * Z
                    const float thr = (float)u24 * (1.0f / 16777216.0f) * w.Z;
                    float base = 0.f;
                    bool found = false;
                    sel = n - 1u;                                        // rounding may leave no crossing: the last index
                    for (uint32_t a0 = 0u; a0 < n && !found; a0 += MC_BLOCK) {
                        const uint32_t a1 = a0 + MC_BLOCK < n ? a0 + MC_BLOCK : n;
                        float s = 0.f;
                        for (uint32_t a = a0; a < a1; ++a) {
                            s += expf(x(a) - w.m);
                            if (base + s > thr) { sel = a; found = true; break; }
                        }
                        base += s;                                       // = the running sum at the block's last index
                    }
                }
                if (mode != CAT_EVALUATE) act = (int64_t)sel;
                lp = (x(sel) - w.m) - logZ;
            }
            p_lp[tid] = lp;
            p_H[tid] = H;
            p_bad[tid] = bad ? 1u : 0u;
            if (mode != CAT_EVALUATE) io.actions[i * D + d] = act;
        }
        __syncthreads();
        if (on && d == 0u) {
            float lp = 0.f, H = 0.f;
            uint32_t bad = 0u;
            for (uint32_t k = 0u; k < D; ++k) {                            // ascending d, from +0
                lp += p_lp[tid + k];
                H += p_H[tid + k];
                bad |= p_bad[tid + k];
            }
            io.log_prob[i] = bad ? __uint_as_float(0x7FC00000u) : lp;
            if (io.entropy) io.entropy[i] = H;
            if (bad && io.bad_actions) atomicAdd(io.bad_actions, 1u);
        }
    }
}

template <typename LT, bool STAGED>
__global__ __launch_bounds__(256) void multicategorical_grad_kernel(McGeom G, McGradIO io) {
    extern __shared__ __attribute__((aligned(16))) float mc_smem[];
    uint32_t* p_bad = reinterpret_cast<uint32_t*>(mc_smem + 2u * MC_LANES);
    float* xs = mc_smem + MC_LDS_HEAD;
    const uint32_t tid = threadIdx.x, D = G.D, A = G.A, R = G.R;
    const uint32_t r = tid / D, d = tid - r * D;
    const bool lane_used = r < R;
    const uint32_t n = lane_used ? G.nvec[d] : 1u, off = lane_used ? G.off[d] : 0u;
    const LT* L = static_cast<const LT*>(io.logits);
    LT* Gr = static_cast<LT*>(io.grad);
    const uint64_t groups = (io.n_rows + R - 1u) / R;
    for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {           // workgroup-uniform
        const uint64_t i0 = g * R;
        const uint32_t rows = io.n_rows - i0 < R ? (uint32_t)(io.n_rows - i0) : R;
        __syncthreads();                                                  // the previous pass has stored its rows and read its flags
        if constexpr (STAGED) mc_stage<LT>(xs, L, i0, rows, A, io.row_stride, tid);
        const bool on = r < rows;
        const uint64_t i = i0 + r;
        int64_t act = 0;
        if (on) {
            act = io.actions[i * D + d];
            p_bad[tid] = act < 0 || act >= (int64_t)n ? 1u : 0u;
        }
        __syncthreads();
        if (on) {
            uint32_t bad = 0u;
            for (uint32_t k = 0u; k < D; ++k) bad |= p_bad[tid - d + k];
            const float g_lp = io.g_lp ? io.g_lp[i] : 0.f, g_H = io.g_ent ? io.g_ent[i] : 0.f;
            const LT* row = L + i * io.row_stride + off;
            LT* out = Gr + i * io.grad_stride + off;
            float* xr = xs + r * A + off;
            auto x = [&](uint32_t a) -> float {
                if constexpr (STAGED) return xr[a]; else return cat_logit(row, a);
            };
            auto put = [&](uint32_t a, float v) {
                if constexpr (STAGED) xr[a] = v; else mc_put(out + a, v);
            };
            if (bad || n == 1u) {
                // a row with a component outside its range, and a dimension of one choice: +0.0
                for (uint32_t a = 0u; a < n; ++a) put(a, 0.f);
            } else {
                // the forward's m, Z, log Z and H: the same walks
                const McWalk w(x, n);
                const float logZ = cat_log(w.Z);
                const float H = logZ - w.T / w.Z;
                const float rZ = 1.0f / w.Z;
                const uint32_t c = (uint32_t)act;
                for (uint32_t a = 0u; a < n; ++a) {
                    const float dd = x(a) - w.m;
                    const float ex = expf(dd);
                    const float lq = dd - logZ;
                    const float prod = ex > 0.f ? (ex * rZ) * (-g_lp - g_H * (lq + H)) : 0.f;      // (-inf) * 0 is no term
                    put(a, (a == c ? g_lp : 0.f) + prod);
                }
            }
        }
        if constexpr (STAGED) {
            __syncthreads();
            mc_unstage<LT>(xs, Gr, i0, rows, A, io.grad_stride, tid);
        }
    }
}

} // namespace mcbs
