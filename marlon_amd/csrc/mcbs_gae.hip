// mcbs_gae.hip — generalized advantage estimation over a whole [T, E] rollout in one launch (include/mcbs.h "generalized advantage
// estimation"): what Stable-Baselines3's RolloutBuffer.compute_returns_and_advantage does with T Python iterations over [E] vectors.
//
// The recurrence runs backwards in time and is sequential per env, with nothing to share inside one env: ONE LANE per env column,
// one-wavefront workgroups, env index fastest (the step kernel's mapping), so every access of a wavefront is one contiguous burst of a row.
//
// Time loop: blocks of U steps from the end of the rollout.  All loads of a block (rewards, values, episode_starts, optionally bootstrap)
// are issued before the first is consumed, and the loads of the NEXT block are issued before the stores of the current one: gfx9 retires
// loads and stores in order on one counter (vmcnt), so a load issued behind a store would wait for the store's acknowledgement.  With
// this order the arithmetic of a block waits with s_waitcnt vmcnt(N), N = the loads of the next block still in flight.  The T mod U
// steps left over (the LAST steps of the rollout, done first) use the same arithmetic, one element at a time.
//
// Arithmetic: float32, every operation rounded on its own, in the order the header documents (the library is built with
// -ffp-contract=off: no fused multiply-add); values[t] and episode_starts[t] are loaded once and serve step t and, as "next value" and
// "next non-terminal", step t - 1.  BOOT is a template parameter: without a bootstrap array its two operations are not executed at all
// (rewards + 0 would turn a -0.0 reward into +0.0).  No LDS, no scratch, no atomics; nothing depends on the launch geometry.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#ifndef MCBS_GAE_U
#define MCBS_GAE_U 4      // steps per block: the fastest of 4, 8 and 16 at [128, 65 536] (DESIGN.md section 7 "GAE"; tools/bench_gae.py times the three)
#endif

namespace mcbs {

struct GaeIO {
    const float* rewards;             // [T, s_rew]
    const float* values;              // [T, s_val]
    const uint8_t* starts;            // [T, s_start]
    const float* bootstrap;           // [T, s_boot]; read by the BOOT instantiation only
    const float* last_values;         // [E]
    const uint8_t* last_dones;        // [E]
    float* adv;                       // [T, s_adv]
    float* ret;                       // [T, s_ret] or NULL
    uint64_t T, E;
    size_t s_rew, s_val, s_start, s_boot, s_adv, s_ret;      // row strides in elements
    float g, gl;                      // (float)gamma, (float)(gamma * gae_lambda) with the product taken in double
};

// one step of the recurrence for one env: (r, v, start) of step t, (nv, nnt, last) carried from step t + 1
template <bool BOOT>
__device__ __forceinline__ void gae_step(float g, float gl, float r, float boot, float v, uint32_t start, float& nv, float& nnt, float& last,
                                         float& ret) {
    if constexpr (BOOT) r = r + g * boot;
    const float delta = (r + (g * nv) * nnt) - v;
    last = delta + (gl * nnt) * last;
    ret = last + v;
    nv = v;
    nnt = start ? 0.0f : 1.0f;
}

template <uint32_t U, bool BOOT, bool RET>
__global__ __launch_bounds__(64) void gae_kernel(GaeIO io) {
    const uint64_t e = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (e >= io.E) return;
    // running row pointers of this lane's column, walking from row T - 1 down (64-bit: T * stride may pass 2^32 elements); rd_* are
    // one block ahead of wr_* in the block loop
    const uint64_t T = io.T;
    const float* __restrict__ rd_r = io.rewards + (T - 1u) * io.s_rew + e;
    const float* __restrict__ rd_v = io.values + (T - 1u) * io.s_val + e;
    const uint8_t* __restrict__ rd_s = io.starts + (T - 1u) * io.s_start + e;
    const float* __restrict__ rd_b = BOOT ? io.bootstrap + (T - 1u) * io.s_boot + e : nullptr;
    float* __restrict__ wr_a = io.adv + (T - 1u) * io.s_adv + e;
    float* __restrict__ wr_q = RET ? io.ret + (T - 1u) * io.s_ret + e : nullptr;
    const float g = io.g, gl = io.gl;
    float nv = io.last_values[e];
    float nnt = io.last_dones[e] ? 0.0f : 1.0f;
    float last = 0.0f;

    // element j of a block's registers is its j-th step going DOWN in time
    auto load = [&](float (&lr)[U], float (&lv)[U], float (&lb)[U], uint32_t (&ls)[U]) {
#pragma unroll
        for (uint32_t j = 0; j < U; ++j) {
            lr[j] = *rd_r; rd_r -= io.s_rew;
            lv[j] = *rd_v; rd_v -= io.s_val;
            ls[j] = *rd_s; rd_s -= io.s_start;            // (a register each: bytes would be packed, which waits for them)
            if constexpr (BOOT) { lb[j] = *rd_b; rd_b -= io.s_boot; }
            else lb[j] = 0.0f;
        }
        __builtin_amdgcn_sched_barrier(0);                // keep the block's loads together, ahead of the stores that follow in the source
    };
    auto finish = [&](const float (&lr)[U], const float (&lv)[U], const float (&lb)[U], const uint32_t (&ls)[U]) {
        float a[U], q[U];
#pragma unroll
        for (uint32_t j = 0; j < U; ++j) {
            gae_step<BOOT>(g, gl, lr[j], lb[j], lv[j], ls[j], nv, nnt, last, q[j]);
            a[j] = last;
        }
#pragma unroll
        for (uint32_t j = 0; j < U; ++j) {
            *wr_a = a[j]; wr_a -= io.s_adv;
            if constexpr (RET) { *wr_q = q[j]; wr_q -= io.s_ret; }
        }
    };

    // ---- the T mod U last steps of the rollout, one at a time
    for (uint32_t n = (uint32_t)(T % U); n > 0; --n) {
        float ret;
        float bt = 0.0f;
        if constexpr (BOOT) { bt = *rd_b; rd_b -= io.s_boot; }
        gae_step<BOOT>(g, gl, *rd_r, bt, *rd_v, *rd_s, nv, nnt, last, ret);
        rd_r -= io.s_rew; rd_v -= io.s_val; rd_s -= io.s_start;
        *wr_a = last; wr_a -= io.s_adv;
        if constexpr (RET) { *wr_q = ret; wr_q -= io.s_ret; }
    }

    // ---- blocks of U steps, two register sets in turn: the next block's loads go out before this block's stores
    uint64_t k = T / U;
    if (k == 0) return;
    float r0[U], v0[U], b0[U], r1[U], v1[U], b1[U];
    uint32_t s0[U], s1[U];
    load(r0, v0, b0, s0);
    for (--k; k >= 2; k -= 2) {                           // k: blocks not loaded yet
        load(r1, v1, b1, s1);
        finish(r0, v0, b0, s0);
        load(r0, v0, b0, s0);
        finish(r1, v1, b1, s1);
    }
    if (k) load(r1, v1, b1, s1);
    finish(r0, v0, b0, s0);
    if (k) finish(r1, v1, b1, s1);
}

} // namespace mcbs
