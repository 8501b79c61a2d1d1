// mcbs_step_narrow_tu.hip — the narrow lean step kernel and its launch, a translation unit of its own.
//
// The narrow lean launch is step_kernel<0, 0, false, NONE> instantiated for what the batch's topology can do (kNarrowStepCan, mcbs_step.hip).
// It is chosen once, in mcbs_batch_create, for a lean batch whose topology has no other trait (MCBS_TOPO_*, found on the host with the
// hot image): Chain-10, the headline.  Same kernel name as the full and the lean launch; the argument list is its own.
//
// Why a unit of its own: the Makefile compiles this file, and only this file, with -mllvm -amdgpu-kernarg-preload-count=16.  gfx950 then
// places the first 14 argument dwords in SGPRs before the wavefront starts, and the kernel forms its level-1 addresses without a scalar
// load and its wait: a tenth of the wavefront's life at one wavefront per SIMD, 0.33 us of 3.45 (profiles/step_arg_preload.md).  The
// option is a backend option for a whole compilation and the toolchain has no per-kernel spelling of it, so the kernel must not share a
// compilation with the others: every other device function of libmcbs.so keeps the code it had.  The compiler also emits the prologue
// that loads the same dwords for firmware that does not preload; the kernel is correct either way.
//
// What the preload dictates about the argument list:
//   * only scalar and pointer parameters are preloaded, nothing of a struct passed by value: the level-1 block of LeanStepArgs (h0, masks,
//     body, h1, actions, episode, E, body_stride: exactly 14 dwords) is eight parameters, first in the list;
//   * the node count is not among them, so the fourth row vector is decided from body_stride (step_body_narrow), and N does not travel;
//   * the config pointer follows as a __restrict__ parameter of its own, as in the lean kernel (mcbs_step.hip): the reset tail keeps reading
//     the reset image through the scalar cache behind the step's stores;
//   * then ONE by-value block (NarrowCfg, mcbs_step.hip): what the main path needs later (hot image base, output pointers, row format)
//     and the main path's config words, copied at every launch from the batch's host StepCfg — one scalar round trip on the argument
//     pointer behind the level-1 loads, where config words read through Cp took two (profiles/step_decode.md; left out once for a
//     noisy job, profiles/step_arg_preload.md); `pending` for the reset tail closes the list.
// -DMCBS_NARROW_PRED=0 builds the kernel on step_body with the lean kernel's struct argument list (nothing of it is preloaded).
#include <hip/hip_runtime.h>

#include <cstring>

#include "mcbs.h"
#include "mcbs_device.h"
#include "mcbs_step.hip"

namespace mcbs {

#if MCBS_NARROW_PRED
#ifdef MCBS_DIAG
#define MCBS_NARROW_STAMPS_PARAM , unsigned long long* stamps
#define MCBS_NARROW_STAMPS_ARG , a.stamps
#else
#define MCBS_NARROW_STAMPS_PARAM
#define MCBS_NARROW_STAMPS_ARG
#endif

template <int PHASE, int WTP, bool TOPO_LDS, int DEFK>
__global__ __launch_bounds__(256) void step_kernel(uint4* h0, uint64_t* masks, uint8_t* body, double2* h1, const int32_t* actions, uint32_t* episode,
                                                   uint32_t E, uint32_t body_stride, const StepCfg* __restrict__ Cp, NarrowCfg K,
                                                   double* pending MCBS_NARROW_STAMPS_PARAM) {
    static_assert(PHASE == 0 && WTP == 0 && !TOPO_LDS && DEFK == MCBS_DEFENDER_NONE, "the narrow kernel serves the packed, attacker-only whole step");
    static_assert(kNarrowStepCan == (MCBS_TOPO_PROBE | MCBS_TOPO_WIDE_ROWS), "step_body_narrow is written for exactly these traits");
    DevState S{};
    S.h0 = h0; S.masks = masks; S.body = body; S.h1 = h1; S.episode = episode; S.pending = pending;
    S.E = E; S.body_stride = body_stride; S.tiny_p = K.tiny_p; S.tiny_v = K.tiny_v;   // (step_body_narrow does not read N)
    S.NW = S.SW = S.TW = S.WT = 1u; S.packed = 1u;
    StepIO io{};
    io.actions = actions; io.reward = K.reward; io.terminated = K.terminated;
#ifdef MCBS_DIAG
    io.stamps = stamps;
#endif
    step_body_narrow(S, K, Cp, io);
}

void launch_step_narrow(dim3 grid, hipStream_t st, const StepCfg* C_dev, const StepCfg& C, const LeanStepArgs& a) {
    NarrowCfg K{};
    memcpy(&K.goal_reward, &C.goal_reward, 8); memcpy(&K.winning_reward, &C.winning_reward, 8); memcpy(&K.losing_reward, &C.losing_reward, 8);
    K.hot = a.hot; K.reward = a.reward; K.terminated = a.terminated;
    K.L = C.L; K.R = C.R; K.P = C.P; K.has_attacker_goal = C.has_attacker_goal; K.goal_own_atleast = C.goal_own_atleast;
    K.goal_own_pct_min = C.goal_own_pct_min; K.defender_goal_eviction = C.defender_goal_eviction; K.auto_reset = C.auto_reset;
    K.max_episode_steps = C.max_episode_steps; K.hot_node = C.hot_node; K.hot_desc = C.hot_desc; K.hot_auth = C.hot_auth;
    K.auth_words = C.auth_words; K.tiny_p = a.tiny_p; K.tiny_v = a.tiny_v;
    // the level-1 block, the config pointer, the block, `pending` (and the stamps); with the hidden arguments' first 16 bytes within 256
    // bytes (mcbs_api.hip make_io)
    static_assert(offsetof(LeanStepArgs, N) + sizeof(void*) + sizeof(NarrowCfg) + 2 * sizeof(void*) + 16 <= 256, "step kernel arguments spill into a fifth cache line (make_io)");
    hipLaunchKernelGGL((step_kernel<0, 0, false, MCBS_DEFENDER_NONE>), grid, dim3(64), 0, st, a.h0, a.masks, a.body, a.h1, a.actions, a.episode, a.E,
                       a.body_stride, C_dev, K, a.pending MCBS_NARROW_STAMPS_ARG);
}

#else   // MCBS_NARROW_PRED=0: step_body instantiated with kNarrowStepCan, the lean kernel's argument list in a type of its own

struct NarrowStepArgs { LeanStepArgs a; };

template <int PHASE, int WTP, bool TOPO_LDS, int DEFK>
__global__ __launch_bounds__(256) void step_kernel(const StepCfg* __restrict__ Cp, NarrowStepArgs na) {
    static_assert(PHASE == 0 && WTP == 0 && !TOPO_LDS && DEFK == MCBS_DEFENDER_NONE, "the lean argument block serves the packed, attacker-only whole step");
    const LeanStepArgs& a = na.a;
    DevState S{};
    S.h0 = a.h0; S.masks = a.masks; S.body = a.body; S.h1 = a.h1; S.episode = a.episode; S.pending = a.pending;
    S.E = a.E; S.body_stride = a.body_stride; S.N = a.N; S.tiny_p = a.tiny_p; S.tiny_v = a.tiny_v;
    S.NW = S.SW = S.TW = S.WT = 1u; S.packed = 1u;
    const Topo T{nullptr, a.hot};
    StepIO io{};
    io.actions = a.actions; io.reward = a.reward; io.terminated = a.terminated;
#ifdef MCBS_DIAG
    io.stamps = a.stamps;
#endif
    NoHook nh;
    step_body<0, 0, MCBS_DEFENDER_NONE, false, true, NoHook, kNarrowStepCan>(S, T, Cp, io, RollArgs{}, nh);
}

void launch_step_narrow(dim3 grid, hipStream_t st, const StepCfg* C_dev, const StepCfg&, const LeanStepArgs& a) {
    hipLaunchKernelGGL((step_kernel<0, 0, false, MCBS_DEFENDER_NONE>), grid, dim3(64), 0, st, C_dev, NarrowStepArgs{a});
}

#endif

} // namespace mcbs
