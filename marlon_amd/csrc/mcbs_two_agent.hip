// mcbs_two_agent.hip — one JOINT turn of marlon's two wrappers for a batch of small topologies in ONE launch (gfx950):
// AttackerEnvWrapper.step, then DefenderEnvWrapper.step, then the episode bookkeeping of marl_algorithm.run_episode
// (marl_algorithm.py:197-250; marlon_amd/simulate.py run_episode) — mcbs_two_agent_step.
//
// The reference's defender predicts from the observation its OWN previous step returned (marl_algorithm.py:222-225), so both agents'
// actions of a turn exist before the turn starts, and the two wrapper steps can share a launch.  Until now they were two launches
// (mcbs_wrapper_fused.hip, mcbs_defend.hip: 11-12 us each at 16 384 ToyCtf envs) with a dozen small tensor kernels and a host
// synchronisation between and around them; the second launch re-read from memory the state the first had just stored.
//
// Launch shape: wrapper_fused_kernel's — 256 threads per 64 envs.  The first wavefront runs the attacker's wrapper step, lane = env
// (step_body<0, 0, MCBS_DEFENDER_EXTERNAL, false> with FusedHook's hook points: the same code, the same stores).  Behind the step's
// own stores the SAME lane takes its env's defender turn on the state it has just stored (same thread, program order):
//   defender_turn (validity on the state before the tick, tick, action) with the action's kind replaced by -2 for an env whose
//   episode is over — earlier (`alive` is 0) or on the attacker's side this turn — as run_episode writes into its copy of the actions;
//   defender_shape with the attacker's reward of THIS turn; the six episode arrays (mcbs_episode_buffers, rules in mcbs.h).
// It then parks the defender observation's bits in LDS (DefStageT<64>: agent-installed word, six incoming and six outgoing rule-name
// bits per node), and after the fused kernel's LDS barriers all four wavefronts stream BOTH observations out as 16-byte stores over the
// workgroup's contiguous 64-env blocks.  The attacker's observation was staged between its action and the defender's turn (stage_obs,
// where the fused kernel has it): it does not see the defender's action of this turn.
//
// Not part of the joint turn: attacker auto-reset (the caller owns the episode boundary, as run_episode does), mask fields, anything
// outside the fused wrapper step's scope.  mcbs_api.hip refuses those; there is no multi-launch fallback.
#pragma once
#include "mcbs_defend.hip"
#include "mcbs_wrapper_fused.hip"

namespace mcbs {

struct TwoAgentArgs {                          // second kernel argument block, by value, named members only (no array the compiler could index)
    const int64_t* actions;                    // the defender's [E, 12] rows (never written)
    mcbs_defender_wrapper_buffers dw;
    mcbs_defender_wrapper_cfg dcfg;
    DefObs obs;
    mcbs_episode_buffers ep;                   // all six NULL: no episode bookkeeping, every env counts as alive
};
using TwoAgentStage = DefStageT<64u>;

// FusedHook with the defender's turn, the shaping and the episode bookkeeping behind the attacker's finish.  One object per lane.
struct TwoAgentHook : FusedHook {
    const TwoAgentArgs& D;
    TwoAgentStage& dstage;
    uint8_t ep_alive, ep_adone, ep_ddone;      // level-1 loads of the episode block
    int64_t ep_len;

    __device__ __forceinline__ void level1(uint32_t ec) {
        FusedHook::level1(ec);
        if (D.ep.alive) { ep_alive = D.ep.alive[ec]; ep_len = D.ep.lengths[ec]; ep_adone = D.ep.attacker_done[ec]; ep_ddone = D.ep.defender_done[ec]; }
    }

    __device__ __forceinline__ void finish(const DevState& S, const StepCfg& C, const Topo& T, uint32_t e, bool active, float reward, bool terminated,
                                           uint32_t episode) {
        FusedHook::finish(S, C, T, e, active, reward, terminated, episode);
        if (!active) return;
        // what the attacker's finish has just stored to w.rewards / w.terminated | w.truncated (auto_reset is 0 here)
        const float shaped = reward + (invalid ? A.modifier : 0.0f);
        const bool att_done = terminated || (ts + 1 >= A.max_timesteps);
        const bool alive = D.ep.alive ? ep_alive != 0 : true;
        const bool d1 = alive && att_done;
        const double r1 = alive ? (double)shaped : 0.0;
        // the defender's turn on the state this lane has stored; its shaping reads the attacker's last_cyber_reward of this turn
        bool ok, evicted;
        double avail;
        defender_turn<1, true>(S, T, C, D.actions, e, ok, avail, evicted, !alive || d1);
        const_cast<uint8_t*>(D.dw.valid)[e] = ok ? 1 : 0;
        const_cast<double*>(D.dw.availability)[e] = avail;
        const_cast<uint8_t*>(D.dw.evicted)[e] = evicted ? 1 : 0;
        const DefShaped sh = defender_shape(D.dw, D.dcfg, e, ok, avail, evicted);
        if (D.ep.alive) {
            // marl_algorithm.run_episode's bookkeeping; the reset_request rule of defend_wrapper.py:269-271 (its -0.0 included)
            const bool stepped = alive && !d1;
            const bool d2 = (stepped && (sh.terminated || sh.truncated)) || d1;
            D.ep.attacker_reward[e] = r1;
            D.ep.defender_reward[e] = stepped ? sh.reward : (d1 ? -r1 : 0.0);
            D.ep.lengths[e] = ep_len + (alive ? 1 : 0);
            D.ep.attacker_done[e] = (ep_adone || d1) ? 1 : 0;
            D.ep.defender_done[e] = (ep_ddone || (d2 && alive)) ? 1 : 0;
            D.ep.alive[e] = (alive && !(d1 || d2)) ? 1 : 0;
        }
        // the defender's observation, from the state after its action
        if (D.obs.fused) defender_park<1>(S, T, e, lane, dstage);
    }
};

__global__ __launch_bounds__(FUSED_THREADS) void two_agent_kernel(DevState S, Topo T, const StepCfg* __restrict__ Cp, StepIO io, FusedArgs A, TwoAgentArgs D) {
    __shared__ uint32_t lds[64u * (FUSED_STAGE_DWORDS + FUSED_RAW_DWORDS) + FUSED_FRESH_DWORDS + 32u + 16u];
    __shared__ TwoAgentStage dstage;
    const uint32_t tid = threadIdx.x;
    TwoAgentHook hook{{A, lds, tid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, {0, 0, 0, 0, 0}, false}, D, dstage, 1, 0, 0, 0};
    // the first wavefront takes the workgroup's 64 envs through both agents' turns; the others meanwhile park the service flags
    if (tid < 64u) step_body<0, 0, MCBS_DEFENDER_EXTERNAL, false>(S, T, Cp, io, RollArgs{}, hook);
    else defender_park_services(T, D.obs, tid - 64u, FUSED_THREADS - 64u, dstage);
    // LDS-only barriers, as in wrapper_fused_kernel: the records are complete (lgkmcnt(0)), nobody waits for the global stores in flight
#define MCBS_LDS_BARRIER() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_s_waitcnt(0xC07F); \
                                __builtin_amdgcn_s_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
    MCBS_LDS_BARRIER();
    hook.convert_nodes(S);
    MCBS_LDS_BARRIER();
    hook.convert_creds();
    MCBS_LDS_BARRIER();
#undef MCBS_LDS_BARRIER
    hook.stream(S, blockIdx.x * 64u);
    if (D.obs.fused) defender_stream<64u, FUSED_THREADS>(S, D.obs, tid, blockIdx.x * 64u, dstage);
}

} // namespace mcbs
