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
// The TRAINING turn (two_agent_train_kernel, at the end of this file) is the same launch with both wrappers' auto-resets and the
// reset_request hand-shake between them: marl_algorithm.collect_rollouts' turn — mcbs_two_agent_train_step; two_agent_train_packed_kernel
// behind it is that turn with both observations written as packed rows — mcbs_two_agent_train_step_packed.
#pragma once
#include "mcbs_defend.hip"
#include "mcbs_defender_obs_packing.hip"
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

// ------------------------------------------------------------------ the TRAINING turn (mcbs_two_agent_train_step; rules in mcbs.h)
// marl_algorithm.collect_rollouts' turn: both wrappers auto-reset, and a reset on one side reaches the other through reset_request.
// two_agent_kernel's launch shape and halves with another hook behind them, an instantiation of its own (the kernels above compile to
// what they compiled to before):
//   attacker half : FusedHook's bookkeeping with auto_reset, and truncated |= the request byte; an env that ends is re-initialised by
//                   its own lane (stores only) and its fresh rows and digest come from LDS, as in wrapper_fused_kernel;
//   defender half : defender_turn / defender_shape on the state the lane has just stored — a fresh one when the attacker ended —, the
//                   request override, and for an env the defender ends a SECOND re-initialisation, the cleared defender counters and the
//                   request byte for the attacker's next step;
//   store side    : the attacker's as in wrapper_fused_kernel, except that a written digest carries the observation's discovery order
//                   (the env under an attacker observation that stands may be a re-initialised one); the defender's observation after
//                   its action goes to the TERMINAL arrays for every env, then the lanes whose env the defender ended replace their
//                   record in the stage by the fresh one — built by the non-stepping wavefronts from the one-row arrays — and the stage
//                   goes out again, to the live arrays.
struct TrainArgs {                             // third argument block, by value, named members only
    const int64_t* actions;                    // the defender's [E, 12] rows (never written)
    mcbs_defender_wrapper_buffers dw;
    mcbs_defender_wrapper_cfg dcfg;
    DefObs obs, term;                          // live and terminal observation arrays (the same divisors)
    const int8_t* fresh_infected; const int8_t* fresh_fw_in; const int8_t* fresh_fw_out;
    uint8_t* request;
    double* dreturn;
    int64_t* a_valid_out; int64_t* a_invalid_out;
    double* d_return_out; int32_t* d_length_out; int64_t* d_valid_out; int64_t* d_invalid_out;
    uint8_t* d_dones;
};
struct TrainStage { uint32_t fresh_inst; uint16_t fresh_fw[DEF_NMAX]; uint8_t ended[64]; };

// the re-initialisation of one env of a packed batch by its own lane, stores only: FusedHook::finish's and mcbs_step.hip's reset tail
__device__ __forceinline__ void train_reinit(const DevState& S, const StepCfg& C, uint32_t e, uint32_t new_episode) {
    uint4* dst = reinterpret_cast<uint4*>(S.body + (size_t)e * S.body_stride);
    const uint32_t nv = S.body_stride >> 4;
#pragma unroll
    for (uint32_t i = 0; i < 16u; ++i)
        if (i < nv) dst[i] = make_uint4(C.init_image[4 * i], C.init_image[4 * i + 1], C.init_image[4 * i + 2], C.init_image[4 * i + 3]);
    reinterpret_cast<uint4*>(S.masks)[e] = make_uint4(C.init_packed[0], C.init_packed[1], C.init_packed[2], C.init_packed[3]);
    reinterpret_cast<uint4*>(S.masks)[S.E + e] = make_uint4(C.init_lists[0], C.init_lists[1], C.init_lists[2], C.init_lists[3]);
    if (S.ring) for (uint32_t s = 0; s < 16u; ++s) S.ring[(size_t)s * S.E + e] = 0ull;
    S.h0[e] = make_uint4(0u, 0u, C.n_init, C.n_init);
    S.h1[e] = make_double2(0.0, 1.0);
    S.episode[e] = new_episode;
    S.pending[e] = 0.0;
}

// The defender's store side of a stepping lane, in LDS: park(S, T, e, lane) leaves the env's observation after the defender's action
// there, ended()[lane] tells the workgroup which envs the defender ended.  TrainDenseSide: the int8 form's raw bits; TrainPackedSide
// (with two_agent_train_packed_kernel, below): the packed row's finished words.
struct TrainDenseSide {
    TwoAgentStage& dstage;
    TrainStage& tstage;
    __device__ __forceinline__ uint8_t* ended() const { return tstage.ended; }
    __device__ __forceinline__ void park(const DevState& S, const Topo& T, uint32_t e, uint32_t lane) const { defender_park<1>(S, T, e, lane, dstage); }
};

template <class Args, class Side>
struct TrainHookT : FusedHook {
    const Args& D;
    Side side;
    uint8_t rq;                                // level-1 loads: the request byte, the defender's running return
    double dret;

    __device__ __forceinline__ void level1(uint32_t ec) {
        FusedHook::level1(ec);
        rq = D.request[ec];
        dret = D.dreturn[ec];
    }

    // (dense side) the fresh defender record from the one-row arrays, by the wavefronts that do not step (threads t of nt; N <= DEF_NMAX)
    __device__ __forceinline__ void fill_fresh_defender(const DevState& S, uint32_t t, uint32_t nt) const {
        const uint32_t N = S.N;
        for (uint32_t n = t; n < N; n += nt) {
            uint32_t f = 0;
#pragma unroll
            for (uint32_t k = 0; k < 6u; ++k)
                f |= (D.fresh_fw_in[n * 6u + k] ? 1u << k : 0u) | (D.fresh_fw_out[n * 6u + k] ? 1u << (8u + k) : 0u);
            side.tstage.fresh_fw[n] = (uint16_t)f;
        }
        if (t == nt - 1u) {
            uint32_t bits = 0;
            for (uint32_t n = 0; n < N; ++n) bits |= D.fresh_infected[n] ? 1u << n : 0u;
            side.tstage.fresh_inst = bits;
        }
    }

    __device__ __forceinline__ void finish(const DevState& S, const StepCfg& C, const Topo& T, uint32_t e, bool active, float reward, bool terminated,
                                           uint32_t episode) {
        if (!active) { if (lane < 64u) side.ended()[lane] = 0; return; }
        const mcbs_wrapper_buffers& w = A.w;
        // ---- the attacker's bookkeeping: FusedHook::finish with auto_reset, truncated |= q ----
        const bool q = rq != 0;
        int32_t* o = A.decoded + (size_t)e * 5;
        o[0] = row[0]; o[1] = row[1]; o[2] = row[2]; o[3] = row[3]; o[4] = row[4];
        const_cast<uint8_t*>(w.invalid)[e] = invalid ? 1 : 0;
        const int32_t t = ts + 1;
        const float shaped = reward + (invalid ? A.modifier : 0.0f);
        const double r2 = ret + (double)shaped;
        const bool trunc = (t >= A.max_timesteps) || q;
        const bool done1 = terminated || trunc;
        const int64_t nv = n_valid + (invalid ? 0 : 1), ni = n_invalid + (invalid ? 1 : 0);
        w.timesteps[e] = done1 ? 0 : t;
        w.valid_action_count[e] = done1 ? 0 : nv;
        w.invalid_action_count[e] = done1 ? 0 : ni;
        w.episode_returns[e] = done1 ? 0.0 : r2;
        w.last_cyber_reward[e] = reward;
        w.has_cyber_reward[e] = done1 ? 0 : 1;
        w.rewards[e] = shaped;
        w.truncated[e] = trunc ? 1 : 0;
        w.dones[e] = done1 ? 1 : 0;
        w.episode_return_out[e] = r2;
        w.episode_length_out[e] = t;
        if (w.executed) w.executed[e] = invalid ? 0 : 1;
        D.a_valid_out[e] = nv;
        D.a_invalid_out[e] = ni;
        if (done1) train_reinit(S, C, e, episode + 1u);
        stage(lane).meta() |= done1 ? FM_ENDED : 0u;
        const bool n = done1 && !q;            // the attacker's reset notifies the defender only when the attacker had not been asked
        // ---- the defender's turn and shaping on the state as it now stands (this lane's own stores, program order) ----
        bool ok, evicted;
        double avail;
        defender_turn<1>(S, T, C, D.actions, e, ok, avail, evicted);
        const_cast<uint8_t*>(D.dw.valid)[e] = ok ? 1 : 0;
        const_cast<double*>(D.dw.availability)[e] = avail;
        const_cast<uint8_t*>(D.dw.evicted)[e] = evicted ? 1 : 0;
        const DefShaped sh = defender_shape(D.dw, D.dcfg, e, ok, avail, evicted);
        const double r_def = n ? -(double)shaped : sh.reward;                   // (defend_wrapper.py:269-271, -0.0 included)
        if (n) { D.dw.reward[e] = r_def; D.dw.truncated[e] = 1; }
        const bool done2 = sh.terminated || sh.truncated || n;
        const double dret2 = dret + r_def;
        const int32_t dt = D.dw.timesteps[e];                                    // as defender_shape left them
        const int64_t dv = D.dw.valid_action_count[e], di = D.dw.invalid_action_count[e];
        D.d_return_out[e] = dret2;
        D.d_length_out[e] = dt;
        D.d_valid_out[e] = dv;
        D.d_invalid_out[e] = di;
        D.d_dones[e] = done2 ? 1 : 0;
        D.dreturn[e] = done2 ? 0.0 : dret2;
        D.request[e] = (done2 && !n) ? 1 : 0;
        // the defender's observation after its action (the terminal one where done2), before the second re-initialisation
        side.park(S, T, e, lane);
        side.ended()[lane] = done2 ? 1 : 0;
        if (done2) {
            train_reinit(S, C, e, episode + (done1 ? 2u : 1u));
            D.dw.timesteps[e] = 0;
            D.dw.valid_action_count[e] = 0;
            D.dw.invalid_action_count[e] = 0;
            D.dw.has_breached_sla[e] = 0;
            D.dw.prev_availability[e] = 1.0;                                     // h1.y of a re-initialised env
        }
    }

    // (dense side) FusedHook::stream's five fields (its digest loop is replaced by stream_digests below)
    __device__ __forceinline__ void stream_fields(const DevState& S, uint32_t e0) {
        const uint32_t n_env = S.E - e0 < 64u ? S.E - e0 : 64u;
        const uint32_t* fr = fresh_lds();
        stream_field<1>(e0, n_env); stream_field<2>(e0, n_env); stream_field<3>(e0, n_env); stream_field<4>(e0, n_env);
        if (A.obs[0]) {
            const uint32_t total = n_env * 7u;
            int32_t* out = A.obs[0] + (size_t)e0 * 7u;
            int32_t* tout = A.term[0] + (size_t)e0 * 7u;
            for (uint32_t q = lane; q < total; q += FUSED_THREADS) {
                const uint32_t env = fdiv(q, A.d_u4[0]), j = q - env * 7u;
                const FusedStage st = stage(env);
                const uint32_t meta = st.meta();
                const int32_t v = scalar_value(st, j);
                if (meta & FM_ENDED) { if (meta & FM_LIVE) tout[q] = v; else tout[q] = out[q]; out[q] = (int32_t)fr[A.fresh_off[0] + j]; }
                else if (meta & FM_LIVE) out[q] = v;
            }
        }
    }

    // wrapper_fused_kernel's digest stream, with the observation's discovery order in a written digest (ObsDigest::pad, pad2)
    __device__ __forceinline__ void stream_digests(const DevState& S, uint32_t e0) {
        const uint32_t n_env = S.E - e0 < 64u ? S.E - e0 : 64u;
        uint4* out = reinterpret_cast<uint4*>(A.digest + e0);
        const uint4* rd = reinterpret_cast<const uint4*>(rdig_lds());
        for (uint32_t q = lane; q < n_env * 4u; q += FUSED_THREADS) {
            const uint32_t env = q >> 2, part = q & 3u;
            const FusedStage st = stage(env);
            const FusedRaw rw = raw(env);
            const uint32_t meta = st.meta();
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (part == 0u) v.x = st.own();
            else if (part == 2u) v = make_uint4(meta & 0xFFu, (meta >> 8) & 0xFFu, (meta & FM_BLANK) ? 1u : 0u, 1u);
            else if (part == 3u) v = make_uint4(rw.p[0], rw.p[1], 0u, 0u);
            if (meta & FM_ENDED) out[q] = rd[part];
            else if (meta & FM_LIVE) out[q] = v;
        }
    }
};
using TrainHook = TrainHookT<TrainArgs, TrainDenseSide>;

__global__ __launch_bounds__(FUSED_THREADS) void two_agent_train_kernel(DevState S, Topo T, const StepCfg* __restrict__ Cp, StepIO io, FusedArgs A, TrainArgs D) {
    __shared__ uint32_t lds[64u * (FUSED_STAGE_DWORDS + FUSED_RAW_DWORDS) + FUSED_FRESH_DWORDS + 32u + 16u];
    __shared__ TwoAgentStage dstage;
    __shared__ TrainStage tstage;
    const uint32_t tid = threadIdx.x;
    TrainHook hook{{A, lds, tid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, {0, 0, 0, 0, 0}, false}, D, {dstage, tstage}, 0, 0.0};
    if (tid < 64u) step_body<0, 0, MCBS_DEFENDER_EXTERNAL, false>(S, T, Cp, io, RollArgs{}, hook);
    else {
        hook.fill_reset_rows(tid - 64u, FUSED_THREADS - 64u);
        defender_park_services(T, D.obs, tid - 64u, FUSED_THREADS - 64u, dstage);
        hook.fill_fresh_defender(S, tid - 64u, FUSED_THREADS - 64u);
    }
#define MCBS_LDS_BARRIER() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_s_waitcnt(0xC07F); \
                                __builtin_amdgcn_s_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
    MCBS_LDS_BARRIER();
    hook.convert_nodes(S);
    MCBS_LDS_BARRIER();
    hook.convert_creds();
    MCBS_LDS_BARRIER();
    const uint32_t e0 = blockIdx.x * 64u;
    hook.stream_fields(S, e0);
    hook.stream_digests(S, e0);
    defender_stream<64u, FUSED_THREADS>(S, D.term, tid, e0, dstage);
    MCBS_LDS_BARRIER();                                                          // every thread has read the records it streams
    if (tid < 64u && tstage.ended[tid]) {
        dstage.inst[tid] = tstage.fresh_inst;
        for (uint32_t n = 0; n < S.N; ++n) dstage.fw[tid * DEF_NMAX + n] = tstage.fresh_fw[n];
    }
    MCBS_LDS_BARRIER();
#undef MCBS_LDS_BARRIER
    defender_stream<64u, FUSED_THREADS>(S, D.obs, tid, e0, dstage);
}

// ------------------------------------------------------------------ the TRAINING turn, both observations as PACKED rows
// (mcbs_two_agent_train_step_packed; rules in mcbs.h)
// two_agent_train_kernel with the two packed store sides in place of the dense ones, an instantiation of its own: the same step_body,
// the same TrainHookT::finish, the same digest stream.
//   attacker : FusedPackedStore (mcbs_wrapper_fused.hip) builds the W_obs words of a row from the LDS records and stores them as
//              wrapper_fused_packed_kernel does: live row, terminal row of an env that ended (read back from the live row that stands
//              when its action was intercepted), the fresh row from LDS.  It builds its words OVER the hand-over records, whose first two
//              words stream_digests still needs (the discovery order of a written digest): here the digests leave first, a barrier
//              between.  After a defender-side reset neither row nor digest of the attacker is touched.
//   defender : the stepping lane parks its env's finished words (defender_park_words, where the dense turn parks the raw bits: after
//              the defender's action, before the second re-initialisation); the workgroup streams them, OR-ed with the services' words,
//              to the terminal rows of every env; the lanes whose env the defender ended then replace their words by the caller's fresh
//              row, and the stage leaves again, to the live rows.  Fresh row and service words are fetched into LDS by the wavefronts
//              that do not step.
// FusedPackedArgs is read where it is used (fused_packed_args): it sits at the offset it has in wrapper_fused_packed_kernel's argument
// segment, and TrainPackedKernArgs with the static_assert behind the kernel holds that.  The defender's store side likewise.
struct TrainPackedArgs {                       // by value, named members only: what the stepping lane's finish reads
    const int64_t* actions;                    // the defender's [E, 12] rows (never written)
    mcbs_defender_wrapper_buffers dw;
    mcbs_defender_wrapper_cfg dcfg;
    uint32_t W, pad;                           // words of a packed defender row (W <= DEF_WMAX)
    uint8_t* request;
    double* dreturn;
    int64_t* a_valid_out; int64_t* a_invalid_out;
    double* d_return_out; int32_t* d_length_out; int64_t* d_valid_out; int64_t* d_invalid_out;
    uint8_t* d_dones;
};
// The defender's store side has an argument block of its own, read WHERE IT IS USED like FusedPackedArgs and for the same reason: as
// by-value members of TrainPackedArgs its scalar registers stay live across step_body, where scalar registers are what the kernel
// is short of (it spills 37 of them to vector lanes as it is).
struct TrainPackedStoreArgs {
    DefPackGeom G;                             // the batch's own
    uint32_t* packed;                          // [E, row_words] live rows
    uint32_t* term;                            // [E, row_words] the rows after the defender's action
    const uint32_t* fresh;                     // [W] the row of a freshly reset env
    size_t row_words;
};
// restates two_agent_train_packed_kernel's parameter list, member for parameter (the static_assert behind the kernel)
struct TrainPackedKernArgs { DevState S; Topo T; const StepCfg* Cp; StepIO io; FusedArgs A; FusedPackedArgs P; TrainPackedArgs D; TrainPackedStoreArgs Q; };
__device__ __forceinline__ TrainPackedStoreArgs train_packed_store_args() {
    uint64_t q = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(TrainPackedKernArgs, Q);
    asm volatile("" : "+s"(q));
#define MCBS_KARG(T, member) fused_karg<T>(q + offsetof(TrainPackedStoreArgs, member))
    TrainPackedStoreArgs Q{};                  // (G.N, G.S, G.F: not read by the store side)
    Q.G.W = MCBS_KARG(uint32_t, G.W); Q.G.svc = MCBS_KARG(const uint32_t*, G.svc);
    Q.G.dW.mul = MCBS_KARG(uint32_t, G.dW.mul); Q.G.dW.sh1 = MCBS_KARG(uint32_t, G.dW.sh1); Q.G.dW.sh2 = MCBS_KARG(uint32_t, G.dW.sh2);
    Q.packed = MCBS_KARG(uint32_t*, packed); Q.term = MCBS_KARG(uint32_t*, term); Q.fresh = MCBS_KARG(const uint32_t*, fresh);
    Q.row_words = MCBS_KARG(size_t, row_words);
#undef MCBS_KARG
    return Q;
}
struct TrainPackedStage { uint32_t words[64u * DEF_WMAX]; uint32_t svc[DEF_WMAX]; uint32_t fresh[DEF_WMAX]; uint8_t ended[64]; };
struct TrainPackedSide {
    TrainPackedStage& ps;
    uint32_t W;
    __device__ __forceinline__ uint8_t* ended() const { return ps.ended; }
    __device__ __forceinline__ void park(const DevState& S, const Topo& T, uint32_t e, uint32_t lane) const {
        defender_park_words<1>(S, T, e, W, ps.words + lane * W);
    }
};
using TrainPackedHook = TrainHookT<TrainPackedArgs, TrainPackedSide>;

__global__ __launch_bounds__(FUSED_THREADS) void two_agent_train_packed_kernel(DevState S, Topo T, const StepCfg* __restrict__ Cp, StepIO io, FusedArgs A,
                                                                               FusedPackedArgs P, TrainPackedArgs D, TrainPackedStoreArgs Q) {
    __shared__ uint32_t lds[64u * (FUSED_STAGE_DWORDS + FUSED_RAW_DWORDS) + FUSED_FRESH_DWORDS + 32u + 16u];
    __shared__ TrainPackedStage ps;
    const uint32_t tid = threadIdx.x;
    (void)P; (void)Q;                                                                    // (read through fused_packed_args / train_packed_store_args)
    TrainPackedHook hook{{A, lds, tid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, {0, 0, 0, 0, 0}, false}, D, {ps, D.W}, 0, 0.0};
    if (tid < 64u) step_body<0, 0, MCBS_DEFENDER_EXTERNAL, false>(S, T, Cp, io, RollArgs{}, hook);
    else {
        const uint32_t t = tid - 64u;
        // (the condition always holds here; it is wrapper_fused_packed_kernel's line: with the call unconditional the compiler left the kernel
        // a 20-byte private segment that no instruction touched, and with it a scratch set-up per dispatch)
        if (A.auto_reset) hook.fill_reset_digest(t);
        FusedPackedStore{hook, fused_packed_args()}.fill(t, FUSED_THREADS - 64u);
        const TrainPackedStoreArgs q = train_packed_store_args();
        if (t < q.G.W) { ps.svc[t] = q.G.svc[t]; ps.fresh[t] = q.fresh[t]; }             // (W <= DEF_WMAX < 192)
    }
#define MCBS_LDS_BARRIER() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_s_waitcnt(0xC07F); \
                                __builtin_amdgcn_s_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
    MCBS_LDS_BARRIER();
    hook.convert_nodes(S);
    MCBS_LDS_BARRIER();
    hook.convert_creds();
    MCBS_LDS_BARRIER();
    const uint32_t e0 = blockIdx.x * 64u, n_env = S.E - e0 < 64u ? S.E - e0 : 64u;
    hook.stream_digests(S, e0);                                                  // reads the hand-over records' discovery order ...
    MCBS_LDS_BARRIER();                                                          // ... which the attacker's words are now built over
    FusedPackedStore{hook, fused_packed_args()}.stream(e0, n_env);
    const TrainPackedStoreArgs q = train_packed_store_args();
    const uint32_t W = q.G.W;
    defender_stream_words<64u, FUSED_THREADS>(S.E, q.G, q.term, q.row_words, tid, e0, ps.words, ps.svc);
    MCBS_LDS_BARRIER();                                                          // every thread has read the words it streams
    if (tid < 64u && ps.ended[tid])
        for (uint32_t w = 0; w < W; ++w) ps.words[tid * W + w] = ps.fresh[w];
    MCBS_LDS_BARRIER();
#undef MCBS_LDS_BARRIER
    defender_stream_words<64u, FUSED_THREADS>(S.E, q.G, q.packed, q.row_words, tid, e0, ps.words, ps.svc);
}
static_assert(std::is_same<decltype(&two_agent_train_packed_kernel),
                           void (*)(DevState, Topo, const StepCfg*, StepIO, FusedArgs, FusedPackedArgs, TrainPackedArgs, TrainPackedStoreArgs)>::value &&
                  std::is_same<decltype(TrainPackedKernArgs::S), DevState>::value && std::is_same<decltype(TrainPackedKernArgs::T), Topo>::value &&
                  std::is_same<decltype(TrainPackedKernArgs::Cp), const StepCfg*>::value && std::is_same<decltype(TrainPackedKernArgs::io), StepIO>::value &&
                  std::is_same<decltype(TrainPackedKernArgs::A), FusedArgs>::value && std::is_same<decltype(TrainPackedKernArgs::P), FusedPackedArgs>::value &&
                  std::is_same<decltype(TrainPackedKernArgs::D), TrainPackedArgs>::value &&
                  std::is_same<decltype(TrainPackedKernArgs::Q), TrainPackedStoreArgs>::value &&
                  offsetof(TrainPackedKernArgs, P) == offsetof(FusedPackedKernArgs, P) &&
                  sizeof(TrainPackedKernArgs) == offsetof(TrainPackedKernArgs, Q) + sizeof(TrainPackedStoreArgs) &&
                  std::is_trivially_copyable<TrainPackedKernArgs>::value,
              "fused_packed_args() reads FusedPackedArgs at offsetof(FusedPackedKernArgs, P) of the kernel-argument segment and "
              "train_packed_store_args() TrainPackedStoreArgs at offsetof(TrainPackedKernArgs, Q): TrainPackedKernArgs must restate this kernel's "
              "parameter list, with P where it lies in wrapper_fused_packed_kernel's");

} // namespace mcbs
