/* mcbs.h — C ABI of the MI355X-native batched CyberBattleSim step engine (libmcbs.so).
 *
 * Drop-in boundary for ONE hot path of zsh239040/MARLon: the attacker/defender environment
 * step behind `cyberbattle._env.cyberbattle_env.CyberBattleEnv.step` as driven by
 * `marlon.simulate` and marlon's env wrappers.  The reference is pure Python (no FFI of its
 * own); every entry point below names the reference interface it replaces.  Conventions:
 *   - plain pointers and sizes only, no torch / C++ types;
 *   - return 0 on success, a negative MCBS_E* code otherwise; mcbs_last_error() gives the
 *     thread-local message;
 *   - the library owns the environment state (HBM), the caller owns every I/O buffer
 *     (device pointers, e.g. torch-ROCm `tensor.data_ptr()`);
 *   - every call is asynchronous on the caller's stream (`void* stream` is a hipStream_t,
 *     NULL = the null stream) and performs no hidden synchronisation unless stated;
 *   - one batch handle is not re-entrant; different handles are independent (one per GPU).
 *
 * The same topology blob is read by the CPU oracle (oracle/cbs_oracle.c), which is test
 * infrastructure and never linked into this library.
 */
#ifndef MCBS_H
#define MCBS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCBS_ABI_VERSION 1u

/* ---- error codes ---- */
#define MCBS_OK           0
#define MCBS_EINVAL      -1   /* bad argument / malformed blob */
#define MCBS_ELIMIT      -2   /* topology exceeds an engine limit (see MCBS_MAX_*) */
#define MCBS_EHIP        -3   /* HIP runtime error (message has hipGetErrorString) */
#define MCBS_ENOMEM      -4
#define MCBS_ESTATE      -5   /* call not valid in the current state */

/* ---- engine limits ---- */
#define MCBS_MAX_NODES        256   /* node ids are u8; masks are <= 4 x u64 */
#define MCBS_MAX_PORTS         32   /* firewall / listen tables are u32 port masks */
#define MCBS_MAX_PROPS         60   /* property sets share a u64 with the 4 privilege tags of a node row */
#define MCBS_MAX_SLOTS         32   /* vulnerabilities applicable to one node (library + own) */
#define MCBS_MAX_LOCAL_VULNS   32   /* local-vulnerability mask per node is u32 */
#define MCBS_MAX_VULN_COLUMNS 255   /* n_local + n_remote (at most 223 remote ids next to 32 local ones).  A CHOSEN cap of the format, not a
                                       necessity of any field width: it keeps every column a byte-sized value (as the random-events key
                                       lists store them, which exist only up to 64 columns) and is the largest count the tests step.  The
                                       kernels index columns with 32-bit arithmetic; their own first limit is the descriptor table's
                                       32-bit offsets (n_nodes * columns * 64 bytes, about 262 000 columns at 256 nodes), and the
                                       observation's per-source remote blocks fall back to another writer past the LDS budget */
#define MCBS_MAX_CRED_STRINGS 256    /* every set is held in <= 4 x u64 registers per env */
#define MCBS_MAX_TRIPLES      1024  /* distinct (node, port, credential) triples; more than 256 are kept as a wide set in memory */

/* ================================================================================
 * Topology blob ("MCBT", little endian, every section 16-byte aligned).
 * Built on the host by marlon_amd.flatten from a model.Environment
 * (reference records: simulation/model.py:63-77,226-247,263-345,347-362,377-396).
 * ================================================================================ */
#define MCBS_TOPO_MAGIC 0x5442434Du /* "MCBT" */

/* outcome kinds (reference classes, simulation/model.py:118-198) */
enum {
    MCBS_OUT_NONE = 0,
    MCBS_OUT_LEAKED_CREDENTIALS = 1,
    MCBS_OUT_LEAKED_NODES = 2,
    MCBS_OUT_PRIVILEGE_ESCALATION = 3,
    MCBS_OUT_LATERAL_MOVE = 4,
    MCBS_OUT_CUSTOMER_DATA = 5,
    MCBS_OUT_PROBE_SUCCEEDED = 6,
    MCBS_OUT_PROBE_FAILED = 7,
    MCBS_OUT_EXPLOIT_FAILED = 8,
    MCBS_OUT_OTHER = 9
};

/* precondition byte code (oracle only; the GPU uses mcbs_vuln_slot.precond_tt) */
enum {
    MCBS_OP_PROP_BASE = 0x00, /* 0x00..0x3F push static property bit i */
    MCBS_OP_TAG_BASE = 0x40,  /* 0x40..0x43 push tag privilege_k */
    MCBS_OP_TRUE = 0x80,
    MCBS_OP_FALSE = 0x81,
    MCBS_OP_NOT = 0x82,
    MCBS_OP_AND = 0x83,
    MCBS_OP_OR = 0x84
};

#define MCBS_NODE_INSTALLED0 0x01u /* agent_installed in the initial environment */
#define MCBS_NODE_REIMAGABLE 0x02u

typedef struct mcbs_topo_header { /* 192 bytes */
    uint32_t magic, abi_version, total_bytes, header_bytes;
    uint32_t n_nodes, n_ports, n_props, n_local, n_remote;
    uint32_t n_cred_strings, n_triples, max_slots;
    uint32_t n_slots_total, n_payload, n_services, n_allowed, n_code;
    uint32_t max_leak_per_action; /* longest LeakedCredentials list (env.py:421-428) */
    uint32_t avail_any_order;     /* 1: every availability term is an exact multiple of one power of two,
                                     so the node-order sum of actions.py:728-745 is order independent */
    uint32_t reserved0;
    double   total_sla_weight;    /* sum of node sla weights, node order */
    double   full_availability;   /* availability with every node Running (node-order sum / total) */
    uint32_t off_node;            /* mcbs_node_static[n_nodes] */
    uint32_t off_slot_of;         /* uint8[n_nodes * (n_local + n_remote)], 0xFF = not present */
    uint32_t off_slot;            /* mcbs_vuln_slot[n_nodes * max_slots] */
    uint32_t off_payload;         /* mcbs_payload[n_payload] */
    uint32_t off_service;         /* mcbs_service[n_services] */
    uint32_t off_allowed;         /* uint16[n_allowed] credential-string ids */
    uint32_t off_triple;          /* mcbs_triple[n_triples] */
    uint32_t off_code;            /* uint8[n_code] precondition byte code */
    uint32_t off_init_order;      /* uint8[n_nodes]: nodes owned at reset, network order, then 0xFF */
    uint32_t n_init_owned;
    double   full_sum;            /* node-order sum of every avail_term (numerator of full_availability) */
    /* learned-defender tier (marlon/defender_agents/defender.py): firewall rule lists by NAME */
    /* Rule LISTS are first-class: topologies routinely hand the same Python list object to several nodes / directions
     * (toy_ctf.py:14-19,25,73; chainpattern.py:49-54,103), copy.deepcopy keeps that aliasing inside each env, so an edit
     * through one node is seen through every alias.  A node refers to its two lists by id. */
    uint32_t off_fw_rule;         /* mcbs_fw_rule[n_fw_rules]: the rules of list 0, then list 1, ... in list order (oracle) */
    uint32_t n_fw_rules;
    uint32_t off_fw_range;        /* uint16[n_fw_lists * 2]: {offset, count} of each list in the rule array */
    uint32_t n_names;             /* firewall port names: ids 0..n_ports-1 are the identifier ports, then other names */
    uint8_t  rule_name[8];        /* name ids of LearningDefender.firewall_rule_list = RDP, SSH, HTTPS, HTTP, su, sudo (6 used) */
    uint8_t  rule_port[8];        /* identifier-port index of each of those names, 0xFF if it is not an identifier port */
    uint32_t n_fw_lists;          /* distinct rule list objects */
    uint32_t off_fw_list0;        /* uint16[n_fw_lists]: initial state of the six manageable names in each list: bit r = a rule named r
                                     exists, bit 6+r = the first one is ALLOW */
    uint32_t off_ere;             /* mcbs_ere_tables + arrays: what the ExternalRandomEvents defender needs (defender.py:58-148) */
    uint32_t reserved;
} mcbs_topo_header;

/* Tables of the ExternalRandomEvents defender; array offsets are relative to the start of this structure.  A vulnerability
 * "column" is its index in the identifiers: local l -> l, remote r -> n_local + r (at most 64 columns). */
typedef struct mcbs_ere_tables { /* 40 bytes */
    uint32_t n_library;       /* global library vulnerabilities = the first n_library slots of every node */
    uint32_t key_cap;         /* capacity of a node's key list: the longest own list + n_library */
    uint32_t off_own_keys;    /* uint8[n_nodes][key_cap]: the node's OWN vulnerability dictionary keys in order, as columns (0xFF pad) */
    uint32_t off_own_cnt;     /* uint8[n_nodes] */
    uint32_t off_lib_sorted;  /* uint8[n_library]: library columns in name order (numpy.setdiff1d returns sorted names) */
    uint32_t pad;
    uint64_t lib_cols;        /* bit c: column c is a library vulnerability */
    uint8_t  sample_name[8];  /* firewall name ids of model.SAMPLE_IDENTIFIERS.ports (7 used): the ports firewall_change_add opens */
} mcbs_ere_tables;

typedef struct mcbs_node_static { /* 64 bytes */
    uint64_t props;        /* static properties that are declared identifiers (bit = index) */
    double   sla_weight;
    double   avail_term;   /* sla_weight * (1 + running service weights) / (1 + all service weights) */
    int32_t  value;
    uint32_t fw_in_allow;  /* port bit set iff the FIRST incoming rule for the port is ALLOW */
    uint32_t fw_out_allow;
    uint32_t listen;       /* port bit set iff some service has that name (running or not) */
    uint32_t local_mask;   /* bit l set iff local vuln id l is in the library or in the node's dict (env.py:658-663) */
    uint16_t svc_off, svc_cnt;
    uint8_t  flags;        /* MCBS_NODE_* */
    uint8_t  priv0;        /* initial privilege level */
    uint8_t  tags0;        /* privilege_k tags literally present in the initial property list */
    uint8_t  n_slots;
    uint32_t fw_lists;     /* rule list ids: incoming | outgoing << 16 (learned-defender tier) */
    uint32_t pad[2];
} mcbs_node_static;

typedef struct mcbs_fw_rule { /* 2 bytes */
    uint8_t name;          /* firewall port name id */
    uint8_t allow;         /* RulePermission.ALLOW */
} mcbs_fw_rule;

typedef struct mcbs_vuln_slot { /* 32 bytes; slot s of node n applies to target n */
    double   cost;
    uint64_t probe_mask;   /* ProbeSucceeded: declared, non-tag properties it reveals */
    uint32_t payload_off;
    uint16_t payload_cnt;
    uint16_t precond_tt;   /* bit t = precondition value on this node when its tag set is t (4 bits) */
    uint32_t code_off;     /* oracle byte code */
    uint16_t code_len;
    uint8_t  kind;         /* MCBS_OUT_* */
    uint8_t  level;        /* PrivilegeEscalation level */
} mcbs_vuln_slot;

typedef struct mcbs_payload { /* 8 bytes: one LeakedCredentials / LeakedNodesId list entry */
    uint16_t node;
    uint16_t cred;         /* credential-string id (LeakedCredentials) */
    uint16_t triple;       /* (node, port, credential) triple id (LeakedCredentials) */
    uint16_t port;
} mcbs_payload;

typedef struct mcbs_service { /* 16 bytes */
    double   sla_weight;
    uint16_t allowed_off, allowed_cnt;
    uint8_t  port, running;
    uint16_t pad;
} mcbs_service;

typedef struct mcbs_triple { /* 8 bytes */
    uint16_t node, cred;
    uint16_t port, pad;
} mcbs_triple;

/* ================================================================================
 * Batch configuration = CyberBattleEnv constructor arguments (env.py:470-485) plus the
 * in-env defender (defender.py:27-55) and batching knobs.
 * ================================================================================ */
#define MCBS_DEFENDER_NONE 0
#define MCBS_DEFENDER_SCAN_AND_REIMAGE 1 /* ScanAndReimageCompromisedMachines */
#define MCBS_FW_GROWTH 120             /* ExternalRandomEvents: rules a list may gain beyond its initial length before the overflow flag */
#define MCBS_DEFENDER_RANDOM_EVENTS 3    /* ExternalRandomEvents (defender.py:58-148): random patching / planting of vulnerabilities,
                                           service stops and firewall edits, every step, on every node */
#define MCBS_DEFENDER_EXTERNAL 2         /* no in-env defender; a learned defender acts through mcbs_defender_step
                                           (marlon: DefenderEnvWrapper + LearningDefender) */

#define MCBS_RNG_PHILOX 0 /* draw i of a step = half (i&1) of Philox4x32-10(key = (seed lo, seed hi ^ env id hi),
                             ctr = (global env id lo, episode, step_count, i>>1)), 53-bit doubles (hi>>5, lo>>6) */
#define MCBS_ACTION_SKIP 3

#define MCBS_RNG_TAPE   1 /* draws read from a caller tape (parity against the reference's global RNGs) */

typedef struct mcbs_batch_cfg {
    uint32_t abi_version;
    uint32_t n_envs;
    int32_t  device;                 /* HIP device ordinal */
    uint32_t maximum_node_count;     /* bounds (env.py:172-224) */
    uint32_t maximum_total_credentials;
    uint32_t maximum_discoverable_credentials_per_action;
    /* AttackerGoal (env.py:227-241); has_attacker_goal = 0 means attacker_goal=None */
    uint32_t has_attacker_goal;
    uint32_t goal_own_atleast;
    double   goal_reward;
    double   goal_low_availability;
    double   goal_own_atleast_percent;
    /* DefenderGoal / DefenderConstraint (env.py:244-254) */
    uint32_t defender_goal_eviction;
    uint32_t defender_kind;
    double   maintain_sla;
    double   winning_reward, losing_reward;
    /* ScanAndReimageCompromisedMachines(probability, scan_capacity, scan_frequency) */
    double   scan_probability;
    uint32_t scan_capacity, scan_frequency;
    /* batching */
    uint32_t auto_reset;             /* 1: an env that ends is re-initialised inside the same step (VecEnv semantics) */
    uint32_t max_episode_steps;      /* 0 = unlimited; else `truncated` is raised at this step count */
    uint32_t rng_kind;
    uint32_t reserved0;
    uint64_t seed;
    uint64_t env_id_base;            /* global id of env 0 of this shard (multi-GPU: rank * n_envs) */
} mcbs_batch_cfg;

typedef struct mcbs_topology mcbs_topology;
typedef struct mcbs_batch mcbs_batch;

/* Observation buffers, marlon-flat layout = what AttackerEnvWrapper.transform_observation
 * returns (marlon/baseline_models/env_wrappers/attack_wrapper.py:474-522; fields built at
 * env.py:753-773,859-933).  Any pointer may be NULL to skip that field.  E = n_envs,
 * N = maximum_node_count, C = maximum_total_credentials, K = max discoverable per action. */
typedef struct mcbs_obs_buffers {
    int32_t* scalars;                     /* [E,7]: newly_discovered_nodes_count, lateral_move, customer_data_found,
                                             probe_result, escalation, credential_cache_length, discovered_node_count */
    int32_t* leaked_credentials;          /* [E,K,4] rows (used, cache_idx, target ext idx, port idx) */
    int32_t* credential_cache_matrix;     /* [E,C,2] rows (target ext idx, port idx) */
    int32_t* discovered_nodes_properties; /* [E,N,n_props] */
    int32_t* nodes_privilegelevel;        /* [E,N] */
    int8_t*  mask_local;                  /* [E,N,L] */
    int8_t*  mask_remote;                 /* [E,N,N,R] */
    int8_t*  mask_connect;                /* [E,N,N,P,C] */
    int8_t*  mask_discrete;               /* [E, N*N*P*C + N*L + N*N*R]: MaskedDiscreteAttackerWrapper.action_masks()
                                             order (action_masking.py:96-110): connect, local, remote */
} mcbs_obs_buffers;

/* Per-step outputs of mcbs_step beyond reward/terminated (StepInfo, env.py:1176-1182). */
typedef struct mcbs_info_buffers {
    double*  network_availability; /* [E] */
    int32_t* step_count;           /* [E] */
    uint8_t* truncated;            /* [E] */
    uint8_t* out_of_bound;         /* [E] 1 = OutOfBoundIndexError path was taken (env.py:1171-1174) */
    float*   raw_reward;           /* [E] ActionResult.reward before the clamp / terminal override of env.py:1162-1169
                                      (0 on the out-of-bound path); parity and reward-shaping aid */
} mcbs_info_buffers;

const char* mcbs_last_error(void);
uint32_t    mcbs_abi_version(void);

/* model.Environment (+ identifiers) -> device-resident tables.  Replaces the deep-copied
 * networkx graph of env.py:375-376. */
int  mcbs_topology_create(const void* blob, size_t nbytes, int32_t device, mcbs_topology** out);
void mcbs_topology_destroy(mcbs_topology*);

/* CyberBattleEnv.__init__ (env.py:470-566) for n_envs environments sharing one topology. */
int  mcbs_batch_create(const mcbs_topology*, const mcbs_batch_cfg*, mcbs_batch** out);
void mcbs_batch_destroy(mcbs_batch*);

/* CyberBattleEnv.reset (env.py:1187-1209) for every env, or for the envs whose byte in the
 * device array env_mask[E] is non-zero (NULL = all). */
int  mcbs_reset(mcbs_batch*, const uint8_t* env_mask, void* stream);

/* Every env back to the state mcbs_batch_create left it in: mcbs_reset for the whole batch with the episode counters at 0 again
 * (mcbs_reset advances them, so that an env's next episode draws fresh defender randomness: Philox is keyed by (seed, global env id,
 * episode, step)).  The reference's counterpart is constructing the environment anew (env.py:470-566); used to replay a recorded
 * trajectory from its start (bench.py, tools/). */
int  mcbs_rewind(mcbs_batch*, void* stream);

/* CyberBattleEnv.step (env.py:1145-1185) for all envs in one launch, observation excluded.
 * actions: device int32 [E,5] rows (kind, a, b, c, d):
 *     kind 0 local_vulnerability  (source, vuln)              -- action dict order of env.py:540-559
 *     kind 1 remote_vulnerability (source, target, vuln)
 *     kind 2 connect              (source, target, port, credential index)
 *     kind 3 skip                 the env is not stepped at all (no step count, no defender, state untouched);
 *                                 reward 0, terminated 0.  This is how marlon's AttackerEnvWrapper handles an
 *                                 action whose node index is not discovered yet (attack_wrapper.py:286-308).
 * reward: device float [E]; terminated: device uint8 [E]; info may be NULL.
 * An env that is done and not auto-reset is left untouched (reward 0, terminated 1): the
 * single-env facade raises the reference's RuntimeError (env.py:1146-1147) on the host. */
int  mcbs_step(mcbs_batch*, const int32_t* actions, float* reward, uint8_t* terminated,
               const mcbs_info_buffers* info, void* stream);

/* n_steps consecutive steps of every env in ONE launch, for action sequences that are known in advance (recorded traces,
 * scripted plans, pre-sampled random agents: marlon.simulate's random-agent loops, marlon/simulate.py:14-35):
 * actions [n_steps, E, 5], reward / terminated [n_steps, E].  Identical in effect to n_steps calls of mcbs_step without info
 * buffers (auto-reset and truncation included); needs the Philox generator when a defender is configured.  The reference has
 * no counterpart; what it saves is the cost between dependent launches. */
int  mcbs_step_many(mcbs_batch*, const int32_t* actions, float* reward, uint8_t* terminated, uint32_t n_steps, void* stream);

/* Random agents on the device: n_steps steps in one launch, each env's action drawn inside the kernel from its own state
 * (valid != 0: the distribution of CyberBattleEnv.sample_valid_action, env.py:959-1047; else uniform over the action space) with
 * Philox keyed by (seed, global env id, first_step + k) — the action mcbs_sample_actions(valid, seed, first_step + k) would give.
 * actions_out [n_steps, E, 5] may be NULL.  marlon.simulate's loop for random agents (marlon/simulate.py:14-35). */
int  mcbs_rollout_random(mcbs_batch*, int32_t valid, uint64_t seed, uint64_t first_step, uint32_t n_steps,
                         int32_t* actions_out, float* reward, uint8_t* terminated, void* stream);

/* Same transition, but the observation is written exactly where the reference assembles it:
 * after the attacker's action and BEFORE the defender acts (env.py:1153 vs 1156-1158).
 * Three launches: attacker phase, observation, defender + goals. */
int  mcbs_step_observe(mcbs_batch*, const int32_t* actions, float* reward, uint8_t* terminated,
                       const mcbs_info_buffers* info, const mcbs_obs_buffers* obs, void* stream);

/* Observation of the current state: the reset observation (env.py:1197-1200) right after
 * mcbs_reset; otherwise the state-aggregated fields with the per-step flags of the last action. */
int  mcbs_observe(mcbs_batch*, const mcbs_obs_buffers* obs, void* stream);

/* mcbs_observe restricted to the envs whose byte in the device array env_mask[E] is non-zero; the buffers of the other
 * envs are left as they are (VecEnv auto-reset: only the envs that were just reset get a fresh observation). */
int  mcbs_observe_masked(mcbs_batch*, const mcbs_obs_buffers* obs, const uint8_t* env_mask, void* stream);

/* CyberBattleEnv.compute_action_mask (env.py:679-683): the three masks (and/or mask_discrete) of the CURRENT state,
 * whatever the last step was (mcbs_observe returns all-zero masks after an out-of-bound step, like the reference's
 * blank observation).  Only the mask_* members of the buffers are used. */
int  mcbs_action_mask(mcbs_batch*, const mcbs_obs_buffers* masks, void* stream);

/* Row stride of mcbs_obs_buffers.mask_discrete in bytes for this batch (0 = dense: mcbs_discrete_action_count bytes per env, the default).
 * The flat mask's length is rarely a multiple of a cache line (Chain-10 @12/12: 14 172 bytes), so dense rows share 128-byte lines with
 * their neighbours; a caller that pads its rows to a multiple of 128 bytes (and aligns the array) gets every env's mask on lines of its
 * own — the connect region is then streamed with aligned non-temporal stores like mask_connect.  Bytes of a row beyond the action count
 * are never written.  Applies to mcbs_observe / mcbs_step_observe / mcbs_action_mask / mcbs_observe_masked / mcbs_attacker_wrapper_step. */
int  mcbs_set_mask_discrete_stride(mcbs_batch*, size_t stride_bytes);

/* StepInfo fields without stepping. */
int  mcbs_step_info(mcbs_batch*, const mcbs_info_buffers* info, void* stream);

/* Random-agent harness (env.py:935-1055): `valid` != 0 draws like sample_valid_action (source
 * among owned nodes, target among discovered, rejection against the action mask); 0 draws every
 * component uniformly in its bound, invalid actions included.  Philox stream separate from the
 * defender's.  actions_out: device int32 [E,5]. */
int  mcbs_sample_actions(mcbs_batch*, int32_t valid, uint64_t seed, uint64_t step, int32_t* actions_out, void* stream);

/* marlon's attacker action encodings -> engine action rows, on the device.
 *   multidiscrete: int64 [E,10] = AttackerEnvWrapper's MultiDiscrete (attack_wrapper.py:206-227,255-267):
 *                  [kind, l_src, l_vuln, r_src, r_tgt, r_vuln, c_src, c_tgt, c_port, c_cred]; or NULL
 *   discrete:      int64 [E]    = MaskedDiscreteAttackerWrapper's Discrete index (action_masking.py:112-142):
 *                  connect block ((src*N+tgt)*P+port)*C+cred, then local src*L+vuln, then remote (src*N+tgt)*R+vuln
 * Exactly one of the two is non-NULL.  An action whose source / target index is not below the env's discovered-node
 * count is turned into a skip row and flagged in invalid[E] (attack_wrapper.py:236-253,286-308).  So is everything outside the
 * action space: a Discrete index below 0 or not below mcbs_discrete_action_count, a MultiDiscrete kind other than 0, 1, 2, a negative
 * MultiDiscrete component of the chosen kind (the reference raises on these before it steps: action_masking.py:109-110,
 * attack_wrapper.py:262) — the env is not stepped.  The same holds for the decoders inside mcbs_attacker_wrapper_step. */
int  mcbs_decode_attacker_actions(mcbs_batch*, const int64_t* multidiscrete, const int64_t* discrete,
                                  int32_t* actions_out, uint8_t* invalid_out, void* stream);

/* ---- on-device action mask -> logits (what MaskablePPO does with action_masks(), train_marl_multi.py:259-293) ----
 * logits: device [E, row_stride] float32 (MCBS_LOGITS_F32) or bfloat16 (MCBS_LOGITS_BF16), row e = the Discrete action scores of env e in
 * MaskedDiscreteAttackerWrapper's order (action_masking.py:96-142: connect, local, remote; mcbs_discrete_action_count entries).
 * In place: logits[e, a] = mask(e, a) ? logits[e, a] : fill, where mask is EXACTLY the mask_discrete the last observation call on this
 * batch (mcbs_step_observe / mcbs_observe / mcbs_observe_masked / mcbs_action_mask) wrote or would have written — it is rebuilt from the
 * per-env digest that call left (owned-source bits, discovered-node and cached-credential counts), so the N*N*P*C-byte mask itself need
 * not be requested from the observation at all.  Not available for MCBS_DEFENDER_RANDOM_EVENTS batches (MCBS_ESTATE).
 * MCBS_ESTATE too while the digests cannot be trusted: before the first whole-batch observation, after mcbs_reset (whole batch: until the
 * next observation; by mask: until mcbs_observe_masked has re-observed those envs) and after mcbs_set_state.  (The local-vulnerability
 * block is read through the env's live discovery list, which only agrees with the digest's counts in those states.)
 * Every launching entry point of this header selects the batch's device for its own duration (the caller's current device is restored). */
#define MCBS_LOGITS_F32  0
#define MCBS_LOGITS_BF16 1
uint64_t mcbs_discrete_action_count(const mcbs_batch*);
int  mcbs_mask_logits(mcbs_batch*, void* logits, int32_t dtype, size_t row_stride, float fill, void* stream);

/* ---- bit-packed Discrete action masks: stored per rollout step, applied at update time (MaskablePPO's evaluate_actions) ----
 * Format: row e covers env (or stored sample) e, device uint32_t [rows, row_words].  Bit a of a row is bit (a & 31) of word (a >> 5),
 * set iff action a is allowed in MaskedDiscreteAttackerWrapper's order (connect ((s*N+t)*P+p)*C+c, then local s*L+l, then remote
 * (s*N+t)*R+r: the order of mcbs_mask_logits and mask_discrete).  W = ceil(A / 32) words carry the mask, A =
 * mcbs_discrete_action_count; bits from A on in word W-1 are zero; words from W up to row_words are never touched.
 *
 * mcbs_pack_action_mask: the packed mask of the LAST observation of every env, rebuilt from the per-env digest exactly like
 *   mcbs_mask_logits (same preconditions: MCBS_ESTATE under MCBS_DEFENDER_RANDOM_EVENTS and while the digests cannot be trusted).
 *   MCBS_EINVAL when bits is NULL or row_words < W.
 * mcbs_apply_packed_mask: logits[i, a] = bit(i, a) ? logits[i, a] : fill for i < n_rows, a < A.  n_rows is any count (e.g. a shuffled
 *   minibatch gathered from stored masks); the batch only supplies the device and A, so no digest is needed (ExternalRandomEvents
 *   batches too, given bits packed by the caller).  dtype, the write-only contract (logits never read, allowed actions left alone)
 *   and the bfloat16 rounding of `fill` are those of mcbs_mask_logits.  logits_row_stride in elements, >= A.
 * mcbs_unpack_action_mask: out[i, a] = bit(i, a) as a 0 / 1 byte for i < n_rows, a < A; bytes from A up to out_row_stride are untouched. */
int  mcbs_pack_action_mask(mcbs_batch*, uint32_t* bits, size_t row_words, void* stream);
int  mcbs_apply_packed_mask(const mcbs_batch*, const uint32_t* bits, size_t bits_row_words, void* logits, int32_t dtype, size_t logits_row_stride,
                            uint64_t n_rows, float fill, void* stream);
int  mcbs_unpack_action_mask(const mcbs_batch*, const uint32_t* bits, size_t bits_row_words, uint8_t* out, size_t out_row_stride,
                             uint64_t n_rows, void* stream);

/* ---- action-mask keys: store the few words the packed mask is a function of, rebuild the bits for a minibatch at update time ----
 * The packed mask above is rebuilt from the observation digest (owned-source bits by discovery index, discovered-node and cached-
 * credential counts) and, for the local-vulnerability block only, from which node sits at each discovery index.  A key row carries
 * exactly those inputs, so it expands to the packed mask of its step long after the env has moved on (Chain-10 at 12/12: 5 words = 20 B
 * per env and step instead of 443 words = 1 772 B).
 *
 * Format: device uint32_t [rows, row_words], little-endian bit and byte order within a word.
 *   Nk = min(cfg.maximum_node_count, the topology's node count), Wk = 1 + ceil(Nk / 32) + ceil(Nk / 4) words carry a key.
 *   word 0                        bits 0-15: the discovered-node count, the EFFECTIVE one (0 for a blank observation); bits 16-31: the
 *                                 cached-credential count
 *   words 1 .. ceil(Nk / 32)      bit i (bit i & 31 of word 1 + (i >> 5)): the node at discovery index i has the agent installed, for i
 *                                 below the effective count (the digest's owned-source bits, cut to Nk)
 *   the next ceil(Nk / 4) words   byte i (byte i & 3 of word i >> 2 of these): the node id at discovery index i, for i below the effective count
 *   Everything else is zero: bits and bytes at or beyond the effective count, and padding.  Words from Wk up to row_words are never
 *   touched.  One env's key is a pure function of its digest and discovery list; two envs with equal masks need not have equal keys.
 *
 * mcbs_mask_key_words: Wk (0 for a NULL batch).
 * mcbs_store_mask_keys: the key of the LAST observation of every env, keys[e, 0 .. Wk), each word written whole, in one launch.  The
 *   preconditions of mcbs_pack_action_mask: MCBS_ESTATE under MCBS_DEFENDER_RANDOM_EVENTS and while the digests cannot be trusted;
 *   MCBS_EINVAL when keys is NULL or row_words < Wk.
 * mcbs_expand_mask_keys: bits[i, 0 .. W) = the packed mask, in the format of mcbs_pack_action_mask, that call would have written for the
 *   env and step key row index[i] was stored at, bit for bit; index NULL: key row i, and then n_rows <= n_source_rows (MCBS_EINVAL
 *   otherwise).  Write-only, words from W on untouched, n_rows any count (0 is a no-op), one launch.  An index outside
 *   [0, n_source_rows) reads no memory and gives an all-zero row.  The batch supplies the device, the geometry and the topology's static
 *   local-vulnerability table; no per-env state and no digest is read, so every defender kind is served, given keys by the caller.
 *   MCBS_EINVAL when keys or bits is NULL, key_row_words < Wk or bits_row_words < W.
 *   Malformed keys never read out of bounds: a count above Nk acts as Nk; owned-source bits at or beyond the (clamped) count are
 *   ignored; a node id at or above the topology's node count contributes no local-vulnerability bits; the credential count is used
 *   as it stands (at or above maximum_total_credentials: every credential).  marlon_amd/mask_keys.py is the host mirror of the format
 *   and of this rule. */
uint64_t mcbs_mask_key_words(const mcbs_batch*);
int  mcbs_store_mask_keys(mcbs_batch*, uint32_t* keys, size_t row_words, void* stream);
int  mcbs_expand_mask_keys(const mcbs_batch*, const uint32_t* keys, size_t key_row_words, const int64_t* index, uint64_t n_source_rows,
                           uint32_t* bits, size_t bits_row_words, uint64_t n_rows, void* stream);

/* ---- masked categorical head: sample, log-prob and entropy of MaskablePPO's action distribution, one launch ----
 * What sb3_contrib's MaskableCategorical does with the policy's logits and action_masks() (train_marl_multi.py:259-293):
 * `where(mask, logits, -1e8)`, log_softmax over the row, then sample / log_prob / entropy with the masked terms zeroed; evaluate_actions
 * repeats it on stored masks at update time.  A masked-out action contributes exp(-1e8 - max) == 0 in float32, so the distribution is
 * exactly the softmax over the ALLOWED actions: these calls read only the logits under set mask bits and write 16-20 bytes per row.
 * The logits are READ-ONLY (never modified, unlike mcbs_mask_logits) and the mask is never written anywhere.
 *
 * mcbs_masked_categorical (live form): one row per env, n = n_envs; the mask is that of the LAST observation of every env, rebuilt from
 *   the per-env digest exactly like mcbs_mask_logits (same preconditions: MCBS_ESTATE under MCBS_DEFENDER_RANDOM_EVENTS and while the
 *   digests cannot be trusted).  Row e is keyed by the GLOBAL env id env_id_base + e: shards of one batch draw what the whole batch would.
 * mcbs_masked_categorical_packed: any n_rows (e.g. a shuffled minibatch gathered from stored masks; 0 is a no-op); the mask of row i is
 *   bits[i, 0 .. W) in the format of mcbs_pack_action_mask, bits_row_words >= W (MCBS_EINVAL otherwise).  Bits at or beyond A in word
 *   W-1 are ignored, not trusted to be zero.  The batch only supplies the device and A: no digest is needed, every defender kind is
 *   served.  Row i is keyed by i.
 *
 * Common arguments (all device pointers):
 *   logits      float32 (MCBS_LOGITS_F32) or bfloat16 (MCBS_LOGITS_BF16) [n, row_stride], row_stride in elements, >= A (MCBS_EINVAL
 *               otherwise); any alignment.  NULL = all-zero logits: the uniform law over the allowed actions, which is the reference's masked
 *               random agent (uniform over np.flatnonzero(action_masks()): random_marlon_agent.py:88-95) — dtype and row_stride are ignored.
 *   mode        MCBS_CATEGORICAL_SAMPLE / _ARGMAX / _EVALUATE
 *   actions     int64 [n]: written in SAMPLE and ARGMAX, read in EVALUATE
 *   log_prob    float [n]: log p of the row's action
 *   entropy     float [n] or NULL
 *   n_allowed   uint32 [n] or NULL: K, the number of allowed actions of the row
 *   uniforms    float [n] or NULL (SAMPLE; see "random numbers")
 *   seed, step  key of the row's random number when uniforms is NULL
 *   bad_actions optional uint32_t, INCREASED by the number of EVALUATE rows whose action lies outside [0, A) (not zeroed by the call)
 *
 * Semantics for the allowed set S of a row, K = |S|, x_a = (float)logits[a]; float32 arithmetic throughout with expf (the one logarithm per row, of the float32
 * Z, K or A, is the correctly rounded float32 of a double-precision log: the device's logf is up to two ulp off), no floating-point
 * atomics, every sum in a fixed order: two calls give bit-identical outputs, and the packed form on the mask mcbs_pack_action_mask stored
 * gives bit for bit what the live form gave.
 *   m = max_S x,  Z = sum_S exp(x_a - m),  log p_a = (x_a - m) - log Z,  entropy = log Z - (sum_S (x_a - m) exp(x_a - m)) / Z
 *   (order of the sums: per mask word in ascending bit order; the words of each block of 64 consecutive words by an inclusive scan in
 *   word order; the blocks' totals one after the other.)
 *   ARGMAX    the allowed action with the largest logit, the lowest index among equal ones.
 *   SAMPLE    inverse CDF in ascending action order: the first allowed action whose cumulative sum (same order as Z) exceeds u * Z; if
 *             rounding leaves none, the last allowed action.
 *   EVALUATE  log p of actions[i]; an action inside [0, A) that is not allowed gets (-1e8f - m) - log Z (the reference's `where`); an
 *             action outside [0, A) gets NaN and counts one bad_action.
 *   logits == NULL: log_prob = -log K, entropy = log K, ARGMAX = the lowest allowed action, SAMPLE = the ((u24 * K) >> 24)-th allowed
 *             action (0-based, ascending), in exact integer arithmetic.
 *   K == 0 (blank observation — the digest's blank flag — or an all-zero packed row): MaskableCategorical degenerates to uniform over all A
 *             actions with entropy 0: log_prob = -log A, entropy = 0, SAMPLE = (u24 * A) >> 24, ARGMAX = 0.
 *
 * Random numbers: u24 is a 24-bit integer, u = u24 * 2^-24.  With uniforms: u24 = min(2^24 - 1, floor(uniforms[i] * 2^24)) (for graph
 * capture, where seed and step would be frozen, and for tests).  Otherwise u24 = word 0 >> 8 of ONE Philox4x32-10 block with
 *   counter = (key_lo, key_hi, step_lo, step_hi),   key = (seed_lo ^ MCBS_CATEGORICAL_PHILOX_DOMAIN, seed_hi)
 * where key = the row key (env_id_base + e, or the row index i) and _lo / _hi are the low / high 32 bits.  The domain constant differs
 * from the random-agent sampler's (0x5A17ACED): the same (seed, step) may be used for both. */
#define MCBS_CATEGORICAL_SAMPLE   0
#define MCBS_CATEGORICAL_ARGMAX   1
#define MCBS_CATEGORICAL_EVALUATE 2
#define MCBS_CATEGORICAL_PHILOX_DOMAIN 0xCA7E6041u
int  mcbs_masked_categorical(mcbs_batch*, const void* logits, int32_t dtype, size_t row_stride, int32_t mode, int64_t* actions, float* log_prob,
                             float* entropy, uint32_t* n_allowed, const float* uniforms, uint64_t seed, uint64_t step, uint32_t* bad_actions,
                             void* stream);
int  mcbs_masked_categorical_packed(const mcbs_batch*, const uint32_t* bits, size_t bits_row_words, uint64_t n_rows, const void* logits,
                                    int32_t dtype, size_t row_stride, int32_t mode, int64_t* actions, float* log_prob, float* entropy,
                                    uint32_t* n_allowed, const float* uniforms, uint64_t seed, uint64_t step, uint32_t* bad_actions, void* stream);

/* ---- masked action head from the latent: the masked categorical head without a logits tensor, one launch ----
 * sb3_contrib's MaskableActorCriticPolicy ends in action_net = Linear(latent_dim_pi, A); the masked categorical head above reads only
 * the logits under set mask bits of what that layer wrote.  These two calls COMPUTE only those: the logit of an allowed action is a
 * dot product of the row's latent with that action's weight row, and no [n, A] tensor exists.  Same two forms, same preconditions
 * (MCBS_ESTATE for the live form as mcbs_masked_categorical), same row keys, same outputs.
 *
 *   latent      [n, latent_row_stride], the policy's latent_pi
 *   weight      [A, weight_row_stride], torch.nn.Linear's layout: one row per action
 *   bias        [A] or NULL (zeros)
 *   H           the layer's input width, 1 <= H <= MCBS_LINEAR_MAX_H; both strides are in elements and >= H; any alignment
 *   dtype       MCBS_LOGITS_F32 or MCBS_LOGITS_BF16, of latent, weight and bias alike.  All three are READ-ONLY.
 *   mode, actions, log_prob, entropy, n_allowed, uniforms, seed, step, bad_actions: as for mcbs_masked_categorical.
 *
 * The logit of an allowed action a of row i, with l_h = (float)latent[i, h], w_h = (float)weight[a, h] (bfloat16 widens exactly), in
 * float32, in ONE fixed order:
 *   four partial sums s_0 .. s_3 start at +0; for h = 0, 1, ..., H - 1 in ascending order  s_(h mod 4) = fmaf(l_h, w_h, s_(h mod 4))
 *   (fused: one rounding per step);  x_a = ((s_0 + s_1) + (s_2 + s_3)) + (float)bias[a]   (bias == NULL: + 0.0f).
 * x_a is a function of the latent row, the weight row and the bias element only: it does not depend on the row's index, the form, the
 * mode, the launch geometry, alignment, strides, or on whether the kernel kept it in LDS between its sweeps or computed it again.
 * Everything after x_a — m, Z, log p, entropy, ARGMAX ties, SAMPLE's inverse CDF and its order, K == 0, EVALUATE of a disallowed or
 * out-of-range action, bad_actions, uniforms / Philox with MCBS_CATEGORICAL_PHILOX_DOMAIN — is the masked categorical head's contract:
 * the outputs are bit for bit those of mcbs_masked_categorical[_packed] on a logits buffer holding these x_a.  (A GEMM sums in another
 * order: against torch.nn.functional.linear the logits agree to rounding, exactly where every partial sum is exact.)
 * No allocation, no host synchronisation, asynchronous on `stream`, capturable in a graph with `uniforms`.
 * MCBS_EINVAL: latent or weight NULL (the uniform law is mcbs_masked_categorical's logits == NULL), H outside [1, MCBS_LINEAR_MAX_H], a
 * stride < H, another dtype, a bad mode, actions or log_prob NULL; packed form: bits NULL, bits_row_words < W.  n_rows == 0 is a no-op. */
#define MCBS_LINEAR_MAX_H 512
int  mcbs_masked_linear_categorical(mcbs_batch*, const void* latent, size_t latent_row_stride, const void* weight, size_t weight_row_stride,
                                    const void* bias, uint32_t H, int32_t dtype, int32_t mode, int64_t* actions, float* log_prob, float* entropy,
                                    uint32_t* n_allowed, const float* uniforms, uint64_t seed, uint64_t step, uint32_t* bad_actions, void* stream);
int  mcbs_masked_linear_categorical_packed(const mcbs_batch*, const uint32_t* bits, size_t bits_row_words, uint64_t n_rows, const void* latent,
                                           size_t latent_row_stride, const void* weight, size_t weight_row_stride, const void* bias, uint32_t H,
                                           int32_t dtype, int32_t mode, int64_t* actions, float* log_prob, float* entropy, uint32_t* n_allowed,
                                           const float* uniforms, uint64_t seed, uint64_t step, uint32_t* bad_actions, void* stream);

/* ---- masked categorical head: gradient — the backward pass of EVALUATE on stored rows, one launch ----
 * What autograd gives for the composite `where(mask, logits, -1e8)` -> Categorical -> log_prob(actions) and the entropy with the masked
 * terms zeroed, differentiated with respect to the logits, from the allowed logits alone.  Packed form only (gradients are taken at
 * update time, on stored rows): bits, bits_row_words, n_rows, logits, dtype, row_stride and actions are those of
 * mcbs_masked_categorical_packed in EVALUATE mode; the batch only supplies the device and A, every defender kind is served; n_rows == 0
 * is a no-op.
 *   grad_log_prob  float [n] or NULL: g_lp, the incoming gradient of log_prob[i]; NULL = all zeros
 *   grad_entropy   float [n] or NULL: g_H, the incoming gradient of entropy[i]; NULL = all zeros
 *   grad_logits    [n, grad_row_stride] in the dtype of logits, grad_row_stride in elements, >= A; any alignment.  WRITE-ONLY: every
 *                  element [i, 0 .. A) is written exactly once (the caller need not clear it), elements from A up to grad_row_stride are
 *                  never written.  bfloat16 output is the float32 value rounded to nearest even.
 * For the allowed set S of row i: K, m, Z, log Z and H = the entropy are exactly the forward's (the same sums in the same order, the same
 * device code), c = actions[i],  p_a = exp(x_a - m) * (1 / Z),  log p_a = (x_a - m) - log Z.
 *   a in S:       grad_logits[i, a] = p_a * (-g_lp - g_H * (log p_a + H)) + (a == c ? g_lp : 0); the product term is exactly 0 where
 *                 exp(x_a - m) underflows to 0 (the forward's rule: (-inf) * 0 is no term)
 *   a not in S:   exactly +0.0, also when a == c: the composite's `where` passes no gradient to a masked logit (a chosen action that is
 *                 not allowed still contributes -g_lp * p_a to the allowed ones)
 *   K == 0 (all-zero packed row) or c outside [0, A): the whole row is +0.0 (the forward has returned NaN for such a c and counted it; the
 *                 gradient call counts nothing)
 * float32 arithmetic throughout in a fixed order, no floating-point atomics: two calls give bit-identical output, and it does not depend on
 * the alignment or the strides of the rows.  logits is READ-ONLY; the value of a logit under a clear mask bit never reaches any output
 * (whole 16-byte groups of logits may be loaded).
 * MCBS_EINVAL: bits, logits, actions or grad_logits NULL (the uniform law has no gradient); a dtype other than MCBS_LOGITS_F32 / _BF16;
 * bits_row_words < W; row_stride < A or grad_row_stride < A; the grad_logits rows overlap the logits rows (rows of equal stride interleaved
 * in one buffer are accepted; with different strides the two extents may not intersect at all). */
int  mcbs_masked_categorical_grad(const mcbs_batch*, const uint32_t* bits, size_t bits_row_words, uint64_t n_rows, const void* logits,
                                  int32_t dtype, size_t row_stride, const int64_t* actions, const float* grad_log_prob,
                                  const float* grad_entropy, void* grad_logits, size_t grad_row_stride, void* stream);

/* ---- masked action head from the latent: gradient — the backward pass of mcbs_masked_linear_categorical_packed in EVALUATE mode ----
 * The gradients of log_prob(actions) and the entropy with respect to latent, weight and bias, without an [n, A] tensor.  Packed form only,
 * like mcbs_masked_categorical_grad; the batch only supplies the device and A, every defender kind is served.  bits, bits_row_words, n_rows,
 * latent, latent_row_stride, weight, weight_row_stride, bias, H, dtype and actions are those of mcbs_masked_linear_categorical_packed in
 * EVALUATE mode (float32 or bfloat16, READ-ONLY), grad_log_prob / grad_entropy those of mcbs_masked_categorical_grad (NULL = zeros).
 *
 * For row i, x_a is the forward's logit (the same device code: bit for bit), K, m, Z, log Z and the entropy are the forward's, and
 * g_{i,a} is the float32 value mcbs_masked_categorical_grad computes, before its output rounding, on a float32 logits buffer holding
 * these x_a: the formula there for an allowed a, 0 for a masked one, a whole row of zeros when K == 0 or actions[i] lies outside [0, A)
 * (a DEAD row).  With S_i the allowed set of row i, l = (float)latent, w = (float)weight:
 *   grad_latent  float [n, grad_latent_row_stride]   grad_latent[i, h] = sum over a in S_i of g_{i,a} * w_{a,h}
 *   grad_weight  float [A, grad_weight_row_stride]   grad_weight[a, h] = sum over i with a in S_i of g_{i,a} * l_{i,h}
 *   grad_bias    float [A]                           grad_bias[a]      = sum over i with a in S_i of g_{i,a}
 * All three are float32 whatever `dtype`, each may be NULL (all three NULL: MCBS_EINVAL), strides in elements and >= H, any alignment.
 * WRITE-ONLY: every element [*, 0 .. H) and [0 .. A) is written exactly once (the caller need not clear them), elements from H up to the
 * stride never.  A dead row of grad_latent, and an action no live row allows, is +0.0.  The value of a weight, bias or logit under a
 * clear mask bit never reaches an output.
 *
 * The order of every sum, in float32, a function of (n_rows, the masks, H) only — not of the launch geometry, strides, alignment, dtype
 * or what the workspace held.  No floating-point atomics; two calls give bit-identical outputs.
 *   grad_latent[i, h]: four partial sums t_0 .. t_3 start at +0; the k-th allowed action a of the row (k = 0, 1, ... in ascending a) does
 *     t_(k mod 4) = fmaf(g_{i,a}, w_{a,h}, t_(k mod 4));  the result is (t_0 + t_1) + (t_2 + t_3).
 *   grad_weight[a, h]: the rows are cut into blocks of MCBS_LINEAR_GRAD_ROW_BLOCK consecutive rows (block j = rows [j B, (j+1) B)); the
 *     partial of block j starts at +0.0 and does  s = fmaf(g_{i,a}, l_{i,h}, s)  for the block's live rows that allow a, in ascending i;
 *     the result is the partials added in ascending j, starting FROM partial 0:  (..(p_0 + p_1) + p_2 ..).
 *   grad_bias[a]: the same with  s = s + g_{i,a}.
 * So a sum with a single term is that term's rounded product added to +0.0 (a product of -0.0 comes out as +0.0, every other value as
 * itself), and a sum without a term is +0.0.
 *
 * workspace: device memory of at least mcbs_masked_linear_categorical_grad_workspace(batch, n_rows, H) bytes (0 for n_rows == 0 or an H
 * outside [1, MCBS_LINEAR_MAX_H]): 32 bytes per row and (H + 1) * 4 bytes per action (A rounded up to whole mask words) and row block —
 * 118 MB for 16 384 rows of Chain-10's 14 172 actions at H = 64, an eighth of one float32 [n, A] tensor.  Its contents on entry do not
 * matter and are undefined on return.  Launches: ONE (the row pass) when grad_weight and grad_bias are both NULL, else THREE (row pass,
 * action pass, the pass that adds the block partials); n_rows == 0 writes +0.0 to grad_weight / grad_bias in one launch.  No allocation,
 * no host synchronisation, asynchronous on `stream`, capturable in a graph.
 * MCBS_EINVAL: all three outputs NULL; bits, latent, weight or actions NULL; H outside [1, MCBS_LINEAR_MAX_H]; a stride < H;
 * bits_row_words < W; another dtype; workspace NULL or smaller than the query's answer; an output or the workspace sharing a byte with
 * an input, with each other (the extents from the first to the last byte of each array are compared). */
#define MCBS_LINEAR_GRAD_ROW_BLOCK 512
size_t mcbs_masked_linear_categorical_grad_workspace(const mcbs_batch*, uint64_t n_rows, uint32_t H);
int  mcbs_masked_linear_categorical_grad(const mcbs_batch*, const uint32_t* bits, size_t bits_row_words, uint64_t n_rows, const void* latent,
                                         size_t latent_row_stride, const void* weight, size_t weight_row_stride, const void* bias, uint32_t H,
                                         int32_t dtype, const int64_t* actions, const float* grad_log_prob, const float* grad_entropy,
                                         float* grad_latent, size_t grad_latent_row_stride, float* grad_weight, size_t grad_weight_row_stride,
                                         float* grad_bias, void* workspace, size_t workspace_bytes, void* stream);

/* ---- MultiDiscrete head: sample, log-prob, entropy and gradient of PPO's MultiCategorical action distribution, one launch each way ----
 * What Stable-Baselines3's MultiCategoricalDistribution does with the policy's logits for a MultiDiscrete(nvec) action — the defender's
 * [5,N,N,6,2,N,6,2,N,3,N,3] (defend_wrapper.py:162-195) and the attacker's unmasked [3,N,L,N,N,R,N,N,P,C] (attack_wrapper.py:206-227):
 * `split` the row by nvec, one Categorical per segment, sample / log_prob / entropy of each, summed over the segments; and what autograd
 * gives for log_prob(actions) and the entropy differentiated with respect to the logits.  No masks: the reference has none for these heads.
 *
 * D = n_dims, off_d = sum of nvec[j] over j < d, A = sum of nvec.  The batch only supplies the device (as for mcbs_gae).  nvec is a HOST
 * array of n_dims entries, copied into the kernel's argument block: no allocation, no synchronisation, asynchronous on `stream`.
 * n_rows == 0 is a no-op.  All other pointers are device memory:
 *   logits      float32 (MCBS_LOGITS_F32) or bfloat16 (MCBS_LOGITS_BF16) [n, row_stride], row_stride in elements, >= A; any alignment;
 *               READ-ONLY.  mcbs_multicategorical only: NULL = the uniform law per dimension (dtype and row_stride are ignored).
 *   mode        MCBS_CATEGORICAL_SAMPLE / _ARGMAX / _EVALUATE
 *   actions     int64 [n, D] contiguous: written in SAMPLE and ARGMAX, read in EVALUATE and by the gradient
 *   log_prob    float [n];  entropy  float [n] or NULL
 *   uniforms    float [n, D] contiguous or NULL (SAMPLE; see "random numbers")
 *   seed, step, row_key_base   key of the row's random numbers when uniforms is NULL; step < 2^48
 *   bad_actions optional uint32_t, INCREASED by one per EVALUATE row with a component outside [0, nvec[d]) (not zeroed by the call)
 *
 * Semantics for dimension d of a row, x_a = (float)logits[off_d + a], 0 <= a < nvec[d]; float32 arithmetic throughout with expf, every
 * operation rounded on its own (no fused multiply-add), no floating-point atomics:
 *   m_d = max_a x_a,  Z_d = sum_a exp(x_a - m_d),  log p_{d,a} = (x_a - m_d) - log Z_d,
 *   H_d = log Z_d - (sum_a (x_a - m_d) exp(x_a - m_d)) / Z_d      (a term whose exp underflows to 0 is no term)
 *   log Z_d is the correctly rounded float32 of a double-precision log of the float32 Z_d, one per dimension.
 *   log_prob = sum_d log p_{d,c_d},  entropy = sum_d H_d.
 * ORDER OF THE SUMS: the indices of a dimension are taken in blocks of 32 consecutive ones ([0, 32), [32, 64), ...; the last one
 * shorter).  Z_d and the entropy sum each add a block's terms from +0 one after the other in ascending a, then the blocks' totals from +0
 * in ascending block order; a dimension of up to 32 choices — every one of the reference's environments — is therefore one serial chain
 * in ascending a (a chain of 1 000 float32 terms would drift by tens of ulp).  The running sum at index a, which SAMPLE compares, is the
 * total of the earlier blocks plus its block's partial sum up to a; at the last index it is Z_d.  log_prob and entropy start from +0 and
 * add the dimensions' values in ascending d.  The order depends on nvec
 * alone: not on n_rows, the strides, the alignment, the dtype's load path, the mode or the row's position.  Hence two calls give
 * bit-identical outputs, the log_prob and entropy of SAMPLE / ARGMAX equal EVALUATE's on the returned actions bit for bit, and the
 * gradient's m_d, Z_d, log Z_d and H_d are the forward's (the same device code).
 *   ARGMAX    per dimension the largest logit, the lowest index among equal ones.
 *   SAMPLE    per dimension inverse CDF in ascending index order: the first a at which the running sum that produced Z_d exceeds
 *             u_d * Z_d; the last index if rounding leaves none.
 *   EVALUATE  reads actions.  A row with any component outside [0, nvec[d]) gets log_prob = NaN (its entropy is still the row's) and
 *             counts one bad_action.
 *   logits == NULL: a_d = (u24_d * nvec[d]) >> 24 in integer arithmetic (ARGMAX: 0), log_prob = sum_d -log nvec[d], entropy =
 *             sum_d log nvec[d] (each log the correctly rounded float32): action_space.sample() of the reference's random agents in law.
 *   nvec[d] == 1 contributes exactly 0 to log_prob and to the entropy, action 0, and exactly zero gradient; its logit is never used.
 *   A logit of -inf is an ordinary value as long as its dimension holds one finite logit.  A NaN logit, a +inf logit or an all -inf
 *   dimension leave that row's log_prob, entropy and gradient unspecified; nothing is read or written out of bounds and every sampled
 *   component stays inside [0, nvec[d]).
 *
 * Random numbers: u24 is a 24-bit integer, u = u24 * 2^-24.  With uniforms: u24_d = min(2^24 - 1, floor(uniforms[i, d] * 2^24)).
 * Otherwise row i has key k = row_key_base + i and dimension d takes word (d & 3) >> 8 of the Philox4x32-10 block
 *   counter = (k_lo, k_hi, step_lo, step_hi | ((d >> 2) << 16)),   key = (seed_lo ^ MCBS_MULTICATEGORICAL_PHILOX_DOMAIN, seed_hi)
 * (_lo / _hi: the low / high 32 bits).  A caller that passes its env_id_base as row_key_base draws in a shard what the whole batch would
 * draw.  The domain constant differs from the masked head's (0xCA7E6041) and the random-agent sampler's (0x5A17ACED).
 *
 * mcbs_multicategorical_grad: the backward pass of EVALUATE.  nvec, n_dims, n_rows, logits, dtype, row_stride and actions as above;
 *   grad_log_prob  float [n] or NULL: g_lp, the incoming gradient of log_prob[i]; NULL = all zeros
 *   grad_entropy   float [n] or NULL: g_H, the incoming gradient of entropy[i]; NULL = all zeros
 *   grad_logits    [n, grad_row_stride] in the dtype of logits, grad_row_stride in elements, >= A; any alignment.  WRITE-ONLY: every
 *                  element [i, 0 .. A) is written exactly once (the caller need not clear it), elements from A up to grad_row_stride are
 *                  never written.  bfloat16 output is the float32 value rounded to nearest even.
 *   grad_logits[i, off_d + a] = p_{d,a} * (-g_lp - g_H * (log p_{d,a} + H_d)) + (a == c_d ? g_lp : 0),  p_{d,a} = exp(x_a - m_d) * (1 / Z_d);
 *   the product term is exactly 0 where the exp underflows to 0.  A row with a component outside its range is +0.0 throughout (the
 *   forward has returned NaN for it and counted it; the gradient call counts nothing).
 *
 * MCBS_EINVAL (the message names the argument): batch or nvec NULL; n_dims outside [1, MCBS_MAX_ACTION_DIMS]; an nvec[d] outside
 * [1, 65536]; a mode other than the three above; step >= 2^48; a dtype other than MCBS_LOGITS_F32 / _BF16; row_stride < A or
 * grad_row_stride < A; with n_rows > 0 a required pointer NULL (actions, log_prob; for the gradient logits, actions, grad_logits: the
 * uniform law has no gradient); the grad_logits rows overlap the logits rows (the rule of mcbs_masked_categorical_grad). */
#define MCBS_MAX_ACTION_DIMS 16
#define MCBS_MULTICATEGORICAL_PHILOX_DOMAIN 0x3C47E6A1u
int  mcbs_multicategorical(const mcbs_batch*, const uint32_t* nvec, uint32_t n_dims, uint64_t n_rows, const void* logits, int32_t dtype,
                           size_t row_stride, int32_t mode, int64_t* actions, float* log_prob, float* entropy, const float* uniforms,
                           uint64_t seed, uint64_t step, uint64_t row_key_base, uint32_t* bad_actions, void* stream);
int  mcbs_multicategorical_grad(const mcbs_batch*, const uint32_t* nvec, uint32_t n_dims, uint64_t n_rows, const void* logits, int32_t dtype,
                                size_t row_stride, const int64_t* actions, const float* grad_log_prob, const float* grad_entropy,
                                void* grad_logits, size_t grad_row_stride, void* stream);

/* ---- generalized advantage estimation: advantages and returns of a whole [T, E] rollout, one launch ----
 * The step between "rollout finished" and "first minibatch": what Stable-Baselines3 2.x's RolloutBuffer.compute_returns_and_advantage
 * does with T Python iterations over [E] host vectors (the reference reaches it through on_rollout_end,
 * marlon/baseline_models/multiagent/marl_algorithm.py:51-52).  All arrays are device memory; [T, E] arrays are rows of E elements
 * whose starts lie `*_stride` ELEMENTS apart (>= n_envs; a [T, :E] view of a wider buffer is served), element [t, e] = base[t * stride + e].
 *   rewards, values           float   [T, E]   inputs
 *   episode_starts            uint8_t [T, E]   nonzero = the observation of step t was the first of an episode
 *   bootstrap                 float   [T, E]   or NULL: the value of the terminal observation where step t was truncated, 0 elsewhere
 *   last_values, last_dones   float / uint8_t [E]: the value of the observation after the last step, and whether that step ended an episode
 *   advantages                float   [T, E]   output
 *   returns                   float   [T, E]   output or NULL
 * THE CONTRACT is this float32 recurrence, every operation rounded to float32 on its own, in exactly this order, no fused multiply-add:
 *   g = (float)gamma;  gl = (float)(gamma * gae_lambda)        (the product taken in double)
 *   last = 0;  nv = last_values[e];  nnt = last_dones[e] ? 0.0f : 1.0f
 *   for t = T-1 ... 0:
 *       r     = rewards[t, e]                                  without bootstrap: the reward itself (a -0.0 keeps its sign)
 *       r     = rewards[t, e] + g * bootstrap[t, e]            with bootstrap
 *       delta = (r + (g * nv) * nnt) - values[t, e]
 *       last  = delta + (gl * nnt) * last
 *       advantages[t, e] = last;   returns[t, e] = last + values[t, e]
 *       nv = values[t, e];  nnt = episode_starts[t, e] ? 0.0f : 1.0f
 * which is that loop of SB3 written out under NumPy's float32 rules (tests/gae_ref.py restates it; SB3 itself is not available to the
 * tests, so parity with it is not pinned).  Denormals are kept.  NaN payloads are not promised.  Inputs are read-only; elements beyond
 * column E of any row are neither read nor written; two calls give bit-identical output, whatever the strides.
 * The batch only supplies the device: n_envs is the call's own (a defender's buffer is served by an attacker's batch).  Asynchronous on
 * `stream`, no allocation, no synchronisation.  n_steps == 0 or n_envs == 0 is a no-op.
 * MCBS_EINVAL (the message names the argument): batch or io NULL; a required pointer NULL; a stride below n_envs; gamma or gae_lambda not
 * finite or outside [0, 1]; an output that overlaps an input or the other output (rows of equal byte stride interleaved in one buffer are
 * accepted; otherwise the two extents may not intersect).  MCBS_ELIMIT: n_envs of 2^37 or more. */
typedef struct mcbs_gae_io {
    const float* rewards;
    const float* values;
    const uint8_t* episode_starts;
    const float* bootstrap;
    const float* last_values;
    const uint8_t* last_dones;
    float* advantages;
    float* returns;
    uint64_t n_steps;
    uint64_t n_envs;
    size_t rewards_stride;
    size_t values_stride;
    size_t episode_starts_stride;
    size_t bootstrap_stride;
    size_t advantages_stride;
    size_t returns_stride;
    double gamma;
    double gae_lambda;
} mcbs_gae_io;
int  mcbs_gae(const mcbs_batch*, const mcbs_gae_io* io, void* stream);

/* ---- feature encoder: observation rows -> the float rows a policy's first layer takes, one launch ----
 * What Stable-Baselines3's "MultiInputPolicy" (marlon/baseline_models/ppo/train.py:79) does first with the wrappers' Dict observation
 * (preprocess_obs + CombinedExtractor): a Discrete(n) becomes a one-hot of n, every element of a MultiDiscrete a one-hot of its own, a
 * MultiBinary 0.0 / 1.0, all concatenated in key order.  The row layout is the caller's (marlon_amd/features.py derives it from the
 * reference's spaces) and is handed over once:
 *   desc[n_desc]: one word per one-hot column, in row order with the mask columns left out: bits 0-15 the column's class, bits 16-30 the
 *     index of its source value among the row's int32 values — the five int32 fields of mcbs_obs_buffers in the struct's order,
 *     flattened: scalars [7], leaked_credentials [K*4], credential_cache_matrix [C*2], discovered_nodes_properties [N*n_props],
 *     nodes_privilegelevel [N] — and bit 31 set on the first column of every element.  The columns of an element are consecutive,
 *     classes 0, 1, 2, ... of one source (MCBS_EINVAL otherwise; MCBS_ELIMIT for a source index beyond 32 767 or 65 536 classes).
 *   mask_ranges[n_mask_ranges][3] (at most three, ascending, not overlapping): (first column of the row, columns, first bit): columns
 *     copied as 0 / 1 from the packed action mask (the format of mcbs_pack_action_mask; bits beyond mcbs_discrete_action_count:
 *     MCBS_EINVAL).
 *   F = n_desc + the ranges' columns (mcbs_feature_layout_width).
 * mcbs_encode_features: out[i, j] for i < n_rows, j < F = 1 where column j's source value of row i equals its class (its mask bit is
 *   set), else 0, as float32 / bfloat16 / float16 (exactly 0 and 1 in each).  obs: the five int32 fields as DENSE rows of their own width,
 *   n_rows rows (a field the layout never reads may be NULL; the mask pointers are ignored); bits [n_rows, bits_row_words >= W] is read
 *   only when the layout has mask columns (NULL then: MCBS_EINVAL).  n_rows is any count: the live observation of the batch or a
 *   minibatch gathered from a rollout buffer; the batch supplies the device and the geometry only — no digest is read, so every defender
 *   kind is served.  out_row_stride in elements, >= F (MCBS_EINVAL otherwise); elements from F up to the stride are never touched, and
 *   every column below F is written (zeros too): the buffer need not be cleared.  Rows on 16-byte boundaries are written with 16-byte
 *   stores, rows on 8- / 4- / 2-byte boundaries with narrower ones.
 *   A value outside [0, classes) leaves its element's columns all zero; out_of_range (optional device uint32_t) is INCREASED by the
 *   number of such elements (not zeroed by the call). */
#define MCBS_FEATURES_F32  0    /* = MCBS_LOGITS_F32 */
#define MCBS_FEATURES_BF16 1    /* = MCBS_LOGITS_BF16 */
#define MCBS_FEATURES_F16  2
typedef struct mcbs_feature_layout mcbs_feature_layout;
int  mcbs_feature_layout_create(const mcbs_batch*, const uint32_t* desc, size_t n_desc, const uint32_t* mask_ranges, size_t n_mask_ranges,
                                mcbs_feature_layout** out);
void mcbs_feature_layout_destroy(mcbs_feature_layout*);
uint64_t mcbs_feature_layout_width(const mcbs_feature_layout*);
int  mcbs_encode_features(const mcbs_batch*, const mcbs_feature_layout*, const mcbs_obs_buffers* obs, const uint32_t* bits, size_t bits_row_words,
                          void* out, int32_t dtype, size_t out_row_stride, uint64_t n_rows, uint32_t* out_of_range, void* stream);

/* ---- packed observations: the five int32 fields of a row as bit fields, stored per step, encoded to features later ----
 * THE PACKED ROW FORMAT (marlon_amd/features.py ObservationPacking is its host mirror).  A row's source values are the V int32 values
 * mcbs_encode_features indexes: the five int32 fields of mcbs_obs_buffers in the struct's order, flattened.
 *   valid codes  value s has n_s valid codes 0 .. n_s - 1 (1 <= n_s <= 65 536; features.py takes the class counts of the observation
 *                spaces, the two counts with C + 1 and N + 1 codes, so a packed row serves either feature layout).
 *   bit width    value s occupies b_s = bit_length(n_s) bits (the position of n_s's highest set bit, counted from 1), which always
 *                leaves a spare code: the stored code is v where 0 <= v < n_s (v read as signed int32) and n_s, the OUT-OF-RANGE
 *                code, for every other v.
 *   placement    the fields follow each other in source order from bit 0 of word 0 upwards; a field never straddles a 32-bit word (one
 *                that does not fit in what is left of the current word starts at bit 0 of the next); unused bits are 0.  W_obs = the
 *                words used (mcbs_obs_packing_words), at most 2 048.
 *   decoding     returns the code: in-range rows round-trip exactly, any other value comes back as n_s — which every feature layout whose
 *                class count of that value is <= n_s encodes like the original: an all-zero group, counted as out of range.
 *   Inside the library a value is one 32-bit descriptor, the table shared by all rows: bits 0-15 n_s - 1, bits 16-31 the field's first
 *   bit 32 * word + shift; b_s follows from n_s.
 * mcbs_obs_packing_create: valid_codes[n_values], n_values = the batch's V (MCBS_EINVAL otherwise); a count of 0 or above 65 536, or more
 *   than 2 048 words: MCBS_ELIMIT.  Word and shift are derived here by the rule above; the descriptors are uploaded once, and behind them
 *   a table of W_obs + 1 entries, each word's first value index in bits 0-30 (the values of a word are a contiguous run:
 *   what mcbs_attacker_wrapper_step_packed builds its words from); bit 31 of an entry is reserved for the library: it marks a word
 *   whose values are all two-code properties, which that kernel builds by a bit-spread.  ObservationPacking.word_first on the host is
 *   the plain index.
 * mcbs_pack_observation: obs = the five fields as DENSE int32 rows, n_rows of them, all five required; out[i, 0 .. W_obs) is written for
 *   every i < n_rows (each word whole: the buffer need not be cleared), out_row_words >= W_obs (MCBS_EINVAL otherwise), words from W_obs
 *   on are never touched.  out_of_range (optional device uint32_t) is INCREASED by the number of values stored as their out-of-range
 *   code.  One launch.
 * mcbs_unpack_observation: the inverse, into dense int32 rows: out->field[i] = the codes of packed row index[i] (index NULL: row i), for
 *   i < n_rows; a field pointer may be NULL (not written; the mask pointers are ignored).  index: optional device int64 [n_rows] into the
 *   n_source_rows rows of `packed` (without it n_rows <= n_source_rows: MCBS_EINVAL otherwise); an index outside [0, n_source_rows)
 *   reads nothing, and that row's values all come back as their out-of-range codes.
 * mcbs_encode_features_packed: mcbs_encode_features with the source values taken from packed rows — the same write-only contract (every
 *   column below F written, nothing from F on touched, the same store widths by alignment, float32 / bfloat16 / float16, out_of_range
 *   INCREASED by the elements whose code lies outside the layout's class count).  With index (device int64 [n_rows]) output row i is
 *   built from row index[i] of BOTH `packed` and `bits`: pass the whole [T * E, ...] storage of a rollout buffer and a minibatch's row
 *   index, the gather happens inside the launch.  An index outside [0, n_source_rows) never reads memory: that row is written all zero
 *   and out_of_range grows by the layout's element count.  MCBS_EINVAL where the layout gives a value more classes than the packing
 *   has valid codes (such a value could not be told from an out-of-range one). */
typedef struct mcbs_obs_packing mcbs_obs_packing;
int  mcbs_obs_packing_create(const mcbs_batch*, const uint32_t* valid_codes, size_t n_values, mcbs_obs_packing** out);
void mcbs_obs_packing_destroy(mcbs_obs_packing*);
uint64_t mcbs_obs_packing_words(const mcbs_obs_packing*);
int  mcbs_pack_observation(const mcbs_batch*, const mcbs_obs_packing*, const mcbs_obs_buffers* obs, uint32_t* out, size_t out_row_words,
                           uint64_t n_rows, uint32_t* out_of_range, void* stream);
int  mcbs_unpack_observation(const mcbs_batch*, const mcbs_obs_packing*, const uint32_t* packed, size_t row_words, const int64_t* index,
                             uint64_t n_source_rows, uint64_t n_rows, const mcbs_obs_buffers* out, void* stream);
int  mcbs_encode_features_packed(const mcbs_batch*, const mcbs_feature_layout*, const mcbs_obs_packing*, const uint32_t* packed,
                                 size_t packed_row_words, const uint32_t* bits, size_t bits_row_words, const int64_t* index,
                                 uint64_t n_source_rows, void* out, int32_t dtype, size_t out_row_stride, uint64_t n_rows,
                                 uint32_t* out_of_range, void* stream);

/* ---- first layer from the observation: Linear(F, H) on the one-hot feature row without the feature row, and its gradient ----
 * The row mcbs_encode_features writes holds exactly one 1 per one-hot element, so the policy's first torch.nn.Linear on it is the bias
 * plus one column of the weight matrix per element, picked by the element's source value.  These calls compute that from the source
 * values themselves — the five dense int32 fields, or stored packed rows through a row index — and no [n, F] tensor exists.
 *
 * For a feature layout with n_elements one-hot elements in ROW ORDER (ascending first column; element e has first column c_e and k_e
 * classes) and a row i whose source value of element e is v_{i,e} (read as mcbs_encode_features[_packed] reads it):
 *     acc = bias ? (float)bias[h] : +0.0f
 *     for e = 0 .. n_elements - 1, in row order:
 *         if 0 <= v_{i,e} < k_e:  acc = acc + (float)weight_t[c_e + v_{i,e}, h]          (one float32 add, no multiply)
 *     out[i, h] = acc                              (float32, or rounded to nearest even to bfloat16)
 * ONE accumulator, ONE chain, the elements in row order: out[i, h] is a function of the row's values, the table and the bias only, not
 * of the row's index, the source form, the launch geometry, alignment or strides, and two calls give the same bits.  This is
 * torch.nn.functional.linear(features, W, b) with W = weight_t transposed, summed in this order (a GEMM sums in another: the two agree
 * to rounding, exactly where every partial sum is exact).  An out-of-range value contributes nothing; out_of_range (optional device
 * uint32_t) is INCREASED by the number of such elements, as mcbs_encode_features does.
 *
 *   weight_t    [F, weight_row_stride]: the TRANSPOSE of torch.nn.Linear's weight, so that the H values of one feature column are
 *               contiguous; float32 or bfloat16 (weight_dtype: MCBS_FEATURES_F32 / MCBS_FEATURES_BF16; bfloat16 widens exactly)
 *   bias        [H] of the same dtype, or NULL
 *   H           1 <= H <= MCBS_LINEAR_MAX_H; every stride is in elements and >= H; any alignment
 *   out         [n_rows, out_row_stride], float32 or bfloat16 (out_dtype), chosen independently of weight_dtype.  Every out[i, 0 .. H) is
 *               written, nothing from H up to the stride is touched.
 * mcbs_first_layer: the rows are the five dense int32 fields of obs, n_rows rows, read as mcbs_encode_features reads them (a field the
 *   layout never reads may be NULL; no digest is read: every defender kind is served).
 * mcbs_first_layer_packed: the source values of output row i are those of packed row index[i] (index NULL: row i, n_rows <=
 *   n_source_rows), by the rules of mcbs_encode_features_packed: the gather happens inside the launch; an index outside
 *   [0, n_source_rows) reads no memory, that row comes out as the bias alone (+0.0 without one) and out_of_range grows by n_elements;
 *   MCBS_EINVAL where the layout gives a value more classes than the packing has valid codes.
 * Each is ONE launch, no allocation, no host synchronisation, asynchronous on `stream`, capturable in a graph; n_rows == 0 succeeds
 * without a launch.
 *
 * mcbs_first_layer_grad: the backward pass of both forms.  The source is EITHER obs (dense; packing and packed NULL) OR packing +
 *   packed (+ index, n_source_rows; obs NULL), exactly as the forward took it.
 *   grad_out       float [n_rows, grad_out_row_stride]: the incoming gradient of out
 *   grad_weight_t  float [F, grad_weight_row_stride]   grad_weight_t[c, h] = sum of grad_out[i, h] over the rows i whose element selects c
 *   grad_bias      float [H]                           grad_bias[h]        = sum of grad_out[i, h] over all rows
 *   Each may be NULL, not both.  WRITE-ONLY: every element [c, 0 .. H) for c < F and [0 .. H) is written (the caller need not clear
 *   them; a column no row selects is +0.0), elements from H up to the stride never.  No floating-point atomics; two calls give
 *   identical bits whatever the workspace held.  The order, the scheme of mcbs_masked_linear_categorical_grad: the rows are cut into
 *   blocks of MCBS_FIRST_LAYER_GRAD_ROW_BLOCK consecutive rows; the partial of a block for (c, h) starts at +0.0 and does
 *   s = s + grad_out[i, h] over the block's rows that select c, in ascending i; the result is the partials added in ascending block
 *   order, starting FROM partial 0: (..(p_0 + p_1) + p_2 ..).  grad_bias[h]: the same over all rows of a block.  A row whose index
 *   lies outside the storage contributes to grad_bias only.  n_rows == 0 writes +0.0 everywhere.
 *   workspace: device memory of at least mcbs_first_layer_grad_workspace(batch, layout, n_rows, H) bytes = blocks * (F + 1) * H * 4
 *   (8.3 MB for 16 384 Chain-10 rows at H = 64; 0 for n_rows == 0, an H out of range or a layout with mask columns); its contents on
 *   entry do not matter and are undefined on return.  TWO launches (the row-block pass, the pass that adds the partials), no
 *   allocation, no host synchronisation, capturable in a graph.
 *
 * MCBS_EINVAL, all with a message: a layout that has mask columns (include_masks is out of scope of these calls); H outside
 * [1, MCBS_LINEAR_MAX_H]; a stride below H; a dtype other than the two; a NULL required pointer (a field the layout reads, weight_t, out,
 * packed, grad_out; both gradients NULL; both sources or neither); a layout or packing of another batch geometry; packed_row_words <
 * W_obs; no index and n_rows > n_source_rows; a workspace that is NULL or too small; an output or the workspace sharing a byte with an
 * input or with each other (the extents from the first to the last byte of each array are compared). */
#define MCBS_FIRST_LAYER_GRAD_ROW_BLOCK 512
int  mcbs_first_layer(const mcbs_batch*, const mcbs_feature_layout*, const mcbs_obs_buffers* obs, uint64_t n_rows, const void* weight_t,
                      size_t weight_row_stride, const void* bias, int32_t weight_dtype, uint32_t H, void* out, int32_t out_dtype,
                      size_t out_row_stride, uint32_t* out_of_range, void* stream);
int  mcbs_first_layer_packed(const mcbs_batch*, const mcbs_feature_layout*, const mcbs_obs_packing*, const uint32_t* packed,
                             size_t packed_row_words, const int64_t* index, uint64_t n_source_rows, uint64_t n_rows, const void* weight_t,
                             size_t weight_row_stride, const void* bias, int32_t weight_dtype, uint32_t H, void* out, int32_t out_dtype,
                             size_t out_row_stride, uint32_t* out_of_range, void* stream);
size_t mcbs_first_layer_grad_workspace(const mcbs_batch*, const mcbs_feature_layout*, uint64_t n_rows, uint32_t H);
int  mcbs_first_layer_grad(const mcbs_batch*, const mcbs_feature_layout*, const mcbs_obs_buffers* obs, const mcbs_obs_packing*,
                           const uint32_t* packed, size_t packed_row_words, const int64_t* index, uint64_t n_source_rows, uint64_t n_rows,
                           const float* grad_out, size_t grad_out_row_stride, uint32_t H, float* grad_weight_t, size_t grad_weight_row_stride,
                           float* grad_bias, void* workspace, size_t workspace_bytes, void* stream);

/* ---- learned defender: marlon/baseline_models/env_wrappers/defend_wrapper.py:197-327,329-412,492-534
 * and marlon/defender_agents/defender.py:31-107, for batches created with MCBS_DEFENDER_EXTERNAL ---- */
typedef struct mcbs_defender_obs {   /* DefenderEnvWrapper.observe: four MultiBinary fields, int8, network node order */
    int8_t* infected_nodes;            /* [E, n_nodes]      agent_installed */
    int8_t* incoming_firewall_status;  /* [E, n_nodes * 6]  a rule named RDP/SSH/HTTPS/HTTP/su/sudo exists in the incoming list */
    int8_t* outgoing_firewall_status;  /* [E, n_nodes * 6] */
    int8_t* services_status;           /* [E, n_services]   service.running, node order then service order */
} mcbs_defender_obs;

/* One defender turn for every env: validity of the action (is_defender_action_valid), then
 * LearningDefender.executeAction = DefenderAgentActions.on_attacker_step_taken() followed by the action if it was valid.
 * actions: device int64 [E,12] = DefenderEnvWrapper's MultiDiscrete [5,N,N,6,2,N,6,2,N,3,N,3]:
 *   [0] kind: 0 reimage([1]) 1 block_traffic([2] node,[3] rule name,[4] incoming) 2 allow_traffic([5],[6],[7])
 *       3 stop_service([8],[9]) 4 start_service([10],[11]); kind -1 = the empty action (the defender skips its turn, the
 *       tick still happens); kind <= -2 = the env takes no part in this call (no tick, state untouched).
 * Outputs (device): valid[E], availability[E] (after the tick), evicted[E] (= __defender_goal_reached), obs (may be NULL).
 * Reference defects reproduced as they are: stop/start_service never match a service (defender.py:45-48 hands a
 * ListeningService object to actions.py:782-794) so they change nothing; allow_traffic appends to the INCOMING list in
 * both branches (defender.py:68).  Not reproduced (DESIGN.md "Q14"): the reference's defender keeps acting on the
 * environment object that existed before the first reset(); here it always acts on the live environment. */
int  mcbs_defender_step(mcbs_batch*, const int64_t* actions, uint8_t* valid, double* availability, uint8_t* evicted,
                        const mcbs_defender_obs* obs, void* stream);
int  mcbs_defender_observe(mcbs_batch*, const mcbs_defender_obs* obs, void* stream);

/* Defender draw tape for MCBS_RNG_TAPE: device double [E, draws_per_step] consumed by the next
 * step (scan draws first, then detection draws in consumption order). */
int  mcbs_set_draw_tape(mcbs_batch*, const double* tape, uint32_t draws_per_step);

/* Bookkeeping of marlon's AttackerEnvWrapper.step around the environment step (attack_wrapper.py:286-354), for every env in one
 * launch: step / action counters, the reward modifier of an intercepted action, truncation at max_timesteps, episode returns.
 * All pointers are device arrays of n_envs elements owned by the caller (a batched wrapper keeps them next to its observation). */
typedef struct mcbs_wrapper_buffers {
    const uint8_t* invalid;        /* in : from mcbs_decode_attacker_actions */
    const float*   reward;         /* in : from mcbs_step / mcbs_step_observe */
    const uint8_t* terminated;     /* in */
    int32_t* timesteps;            /* in/out: wrapper steps of the current episode (invalid ones included) */
    int64_t* valid_action_count;   /* in/out */
    int64_t* invalid_action_count; /* in/out */
    double*  episode_returns;      /* in/out: sum of the wrapper's rewards */
    float*   last_cyber_reward;    /* out: the environment's own reward of this step (AttackerEnvWrapper.cyber_rewards[-1]) */
    uint8_t* has_cyber_reward;     /* out: 1 */
    float*   rewards;              /* out: reward + invalid * invalid_action_reward_modifier */
    uint8_t* truncated;            /* out: timesteps >= max_timesteps */
    uint8_t* dones;                /* out: terminated | truncated */
    double*  episode_return_out;   /* out: copies for the info dict, taken before a reset clears the counters */
    int32_t* episode_length_out;   /* out */
    int32_t* n_done;               /* out: one int32, number of envs with dones != 0 (zeroed by the call) */
    uint8_t* executed;             /* out, optional (may be NULL): !invalid — info["cyber_step_executed"] (mcbs_attacker_wrapper_finish only) */
} mcbs_wrapper_buffers;
int  mcbs_attacker_wrapper_post(mcbs_batch*, const mcbs_wrapper_buffers* w, float invalid_action_reward_modifier, int32_t max_timesteps,
                                void* stream);
/* ... and the counters of the envs whose dones flag is set back to zero (what the wrapper's reset() does for them). */
int  mcbs_attacker_wrapper_clear(mcbs_batch*, const mcbs_wrapper_buffers* w, void* stream);

/* dst[i][e] = src[i][e] (rows of row_bytes[i] bytes, device arrays of n_envs rows) for the envs whose byte in env_mask is non-zero and up to
 * eight arrays in one launch: the terminal observation of the envs that just ended — what SB3's DummyVecEnv keeps in
 * infos[i]["terminal_observation"] before it resets an env.  A batched wrapper calls it with mcbs_wrapper_buffers.dones as the mask, then
 * mcbs_reset + mcbs_observe_masked with the same mask: no host round trip to learn which envs ended.  Like those two it scans the mask
 * 64 envs per wavefront, so it costs a few microseconds when no env ended. */
typedef struct mcbs_row_copies {
    uint32_t n, pad;
    const void* src[8];
    void*       dst[8];
    size_t      row_bytes[8];
} mcbs_row_copies;
int  mcbs_copy_rows_masked(mcbs_batch*, const mcbs_row_copies* copies, const uint8_t* env_mask, void* stream);

/* One whole step of marlon's attacker wrappers for the batch — AttackerEnvWrapper.step (attack_wrapper.py:255-372) under
 * MaskedDiscreteAttackerWrapper (action_masking.py:112-142) under SB3's DummyVecEnv — enqueued by ONE call:
 *   mcbs_decode_attacker_actions (exactly one of multidiscrete [n_envs, 10] / discrete [n_envs]; `decoded` [n_envs, 5] receives the rows,
 *   w->invalid the interception flags), mcbs_step_observe (w->reward and w->terminated receive the environment's reward and done flags:
 *   the three `in` arrays of mcbs_wrapper_buffers are written by this call), mcbs_attacker_wrapper_finish.
 * Stream-ordered, no host synchronisation, hipGraph-capturable (three launches: decode + attacker half, observation, defender half + finish). */

/* Everything an auto-resetting attacker wrapper does after the environment step, in ONE launch: mcbs_attacker_wrapper_post for every env
 * (n_done may be NULL here: nothing is counted; `executed` is written if given), then for the envs whose `dones` it has just set — what SB3's DummyVecEnv.step_wait does
 * with an env that reports done (baseline_marlon_agent.py:100-167 runs the wrappers under it) —
 *   keep:   dst[i][e] = src[i][e]        the episode's last observation (infos[e]["terminal_observation"]),
 *   the env is reset (mcbs_reset for it: reset image, episode counter + 1),
 *   fresh:  dst[i][e] = src[i][0]        the reset observation: `src` arrays hold ONE row, the observation of a freshly reset env
 *                                        (every env resets to the same state, so the wrapper keeps row 0 of its first observation),
 *   the env's digest (mcbs_mask_logits) becomes that of a freshly reset env, and its wrapper counters go back to zero (wrapper_clear).
 * keep / fresh may be NULL (or n = 0); with auto_reset == 0 only the bookkeeping runs.  The batch must have been reset as a whole
 * (mcbs_reset with a NULL mask) and observed once before the first call, so that the library holds a reset env's digest:
 * MCBS_ESTATE otherwise.  Replaces five launches and a memset of the round-2 wrapper step. */
int  mcbs_attacker_wrapper_step(mcbs_batch*, const int64_t* multidiscrete, const int64_t* discrete, int32_t* decoded,
                                const mcbs_info_buffers* info, const mcbs_obs_buffers* obs, const mcbs_wrapper_buffers* w,
                                float invalid_action_reward_modifier, int32_t max_timesteps, int32_t auto_reset,
                                const mcbs_row_copies* keep, const mcbs_row_copies* fresh, void* stream);
int  mcbs_attacker_wrapper_finish(mcbs_batch*, const mcbs_wrapper_buffers* w, float invalid_action_reward_modifier, int32_t max_timesteps,
                                  int32_t auto_reset, const mcbs_row_copies* keep, const mcbs_row_copies* fresh, void* stream);
/* How many kernel launches one mcbs_attacker_wrapper_step of this batch takes: 1 for small topologies (packed batch, at most 16 nodes and
 * cached credentials) when no mask field is requested (with_masks == 0) — the whole step, observation included, is then ONE launch
 * (marlon_amd/csrc/mcbs_wrapper_fused.hip) and replaying it from a hipGraph would only add the graph's own launch cost —, else 3. */
int32_t mcbs_attacker_wrapper_step_launches(const mcbs_batch*, int32_t with_masks);

/* mcbs_attacker_wrapper_step for a trainer that stores PACKED observations: the same step — decode, environment step, observation taken
 * before the defender's turn, bookkeeping, auto-reset — in ONE launch whose observation is the packed row of `packing` ("packed
 * observations" above) instead of the five int32 fields: W_obs words per env (Chain-10 at 12/12: 72 B instead of 924 B), built from the
 * kernel's own records; no int32 field is written or read, no second launch packs anything.
 *   packed           [n_envs, row_words]: the live rows.  Row e receives the observation of this step; an env whose action was intercepted
 *                    keeps the row it has, so the array must be the one the previous step (or a pack of the reset observation) wrote.
 *   packed_terminal  [n_envs, row_words]: row e receives the episode's last observation for the envs this step ends (the row that stands,
 *                    for an env that ends on an intercepted action); other rows are not touched.
 *   packed_fresh     [W_obs]: the packed row of a freshly reset env (mcbs_pack_observation of the reset observation), which becomes the
 *                    live row of every env this step ends.
 *   packed_terminal and packed_fresh are required with auto_reset != 0 and ignored (may be NULL) without it.  row_words >= W_obs; every
 *   word below W_obs of a written row is stored whole, words from W_obs on are never touched.  A value outside its valid codes is stored
 *   as its out-of-range code (nothing is counted here: mcbs_encode_features_packed counts at use).
 * The digests (mcbs_mask_logits, mcbs_pack_action_mask, mcbs_store_mask_keys) and every array of `w`, `decoded` and `info` are written
 * exactly as by mcbs_attacker_wrapper_step's single launch.  Stream-ordered, no host synchronisation, hipGraph-capturable.
 * Scope: batches for which mcbs_attacker_wrapper_step_launches(batch, 0) is 1; there is no multi-launch fallback.  MCBS_EINVAL (nothing
 * launched, no state changed) for a batch outside that scope, a packing created for another device or geometry, row_words < W_obs, a
 * row beyond the room the kernel keeps in LDS (W_obs <= 128 and W_obs + 1 + V <= 896: every batch in scope with the default bounds),
 * missing terminal or fresh rows under auto_reset, both or neither action encodings, and arrays that share bytes (packed,
 * packed_terminal, decoded against each other, the fresh row, the actions and every array of `w` and `info`).  MCBS_ESTATE as for mcbs_attacker_wrapper_step. */
int  mcbs_attacker_wrapper_step_packed(mcbs_batch*, const int64_t* multidiscrete, const int64_t* discrete, int32_t* decoded,
                                       const mcbs_info_buffers* info, const mcbs_obs_packing* packing, uint32_t* packed,
                                       uint32_t* packed_terminal, const uint32_t* packed_fresh, size_t row_words,
                                       const mcbs_wrapper_buffers* w, float invalid_action_reward_modifier, int32_t max_timesteps,
                                       int32_t auto_reset, void* stream);

/* The reward shaping of marlon's DefenderEnvWrapper.step (defend_wrapper.py:228-282) around mcbs_defender_step, for every env in one
 * launch and in the wrapper's own order of double-precision operations: invalid-action penalty, minus the attacker's last environment
 * reward, loss_reward when availability first drops below maintain_sla (terminating if reset_on_constraint_broken), a penalty
 * proportional to the worsening while breached, winning_reward when the attacker is evicted; truncation at max_timesteps. */
typedef struct mcbs_defender_wrapper_buffers {
    const uint8_t* valid;          /* in : mcbs_defender_step outputs */
    const double*  availability;   /* in */
    const uint8_t* evicted;        /* in */
    const uint8_t* attacker_has_cyber_reward;  /* in : the attacker wrapper's buffers (mcbs_wrapper_buffers) */
    const float*   attacker_last_cyber_reward; /* in */
    int32_t* timesteps;            /* in/out */
    int64_t* valid_action_count;   /* in/out */
    int64_t* invalid_action_count; /* in/out */
    uint8_t* has_breached_sla;     /* in/out */
    double*  prev_availability;    /* in/out */
    double*  reward;               /* out */
    uint8_t* terminated;           /* out */
    uint8_t* truncated;            /* out */
    uint8_t* breached;             /* out: availability < maintain_sla */
    uint8_t* won;                  /* out: attacker evicted */
} mcbs_defender_wrapper_buffers;
typedef struct mcbs_defender_wrapper_cfg {
    double invalid_action_penalty, loss_reward, sla_worsening_penalty_scale, maintain_sla, winning_reward;
    int32_t reset_on_constraint_broken, max_timesteps;
} mcbs_defender_wrapper_cfg;
int  mcbs_defender_wrapper_post(mcbs_batch*, const mcbs_defender_wrapper_buffers* w, const mcbs_defender_wrapper_cfg* cfg, void* stream);
/* One whole step of marlon's DefenderEnvWrapper for the batch (defend_wrapper.py:197-327): mcbs_defender_step and mcbs_defender_wrapper_post
 * in ONE launch — the shaping takes the turn's results from registers; w->valid / availability / evicted (the `in` members) are written
 * by this call.  When obs is given the observation is written by the same launch (topologies of up to 32 nodes, arrays on 16-byte
 * boundaries) or by a second one. */
int  mcbs_defender_wrapper_step(mcbs_batch*, const int64_t* actions, const mcbs_defender_obs* obs, const mcbs_defender_wrapper_buffers* w,
                                const mcbs_defender_wrapper_cfg* cfg, void* stream);

/* ---- packed defender observations: one bit per MultiBinary element, stored per step, encoded to features later ----
 * THE PACKED DEFENDER ROW (marlon_amd/features.py DefenderObservationPacking is its host mirror).  With N = n_nodes and S = n_services a
 * row has F = 6N + N + 6N + S columns, the four fields of mcbs_defender_obs in SORTED KEY order — the order of DefenderVecEnv.features():
 *     incoming_firewall_status  column 6n + k            infected_nodes   column 6N + n
 *     outgoing_firewall_status  column 7N + 6n + k       services_status  column 13N + s
 * and is stored as W_def = ceil(F / 32) uint32_t words: column c is bit c & 31 of word c >> 5 (the packed action masks' convention).
 * Bits at or past F in the last word are zero, always.  ToyCtf: N = 10, S = 13, F = 143: 5 words = 20 B instead of 143 B.
 * A dense element packs to 1 when it is not zero (the observation only ever holds 0 and 1) and unpacks to 0 / 1.
 * Row strides (row_words, in words; out_row_stride, in elements) may exceed the row: every word below W_def / column below F of a
 * written row is stored whole (the buffers need not be cleared), nothing beyond is touched.  index: optional device int64 [n_rows] into
 * the n_source_rows source rows (without it n_rows <= n_source_rows: MCBS_EINVAL otherwise) — the gather happens inside the launch; an
 * index outside [0, n_source_rows) reads nothing and that row comes out all zero.
 * mcbs_defender_obs_words: W_def; 0 for NULL or a batch not created with MCBS_DEFENDER_EXTERNAL.
 * mcbs_defender_observe_packed: mcbs_defender_observe for the packed form: the rows of the live state of all envs, one launch.
 * mcbs_pack_defender_observation: n_rows dense int8 rows (all four arrays required) to packed rows, one launch.
 * mcbs_unpack_defender_observation: packed rows to int8 fields, one launch; a NULL member of `out` is skipped.
 * mcbs_encode_defender_features: the float rows DefenderVecEnv.features() builds, 0.0 / 1.0 as float32 / bfloat16 / float16
 *   (MCBS_FEATURES_*), F columns, from EITHER `dense` (all four arrays, n_source_rows rows; packed NULL) OR `packed` (dense NULL), one
 *   launch.  bad_rows (optional device int32_t) is INCREASED by the number of rows whose index lay outside the storage.  Rows on 16-byte
 *   boundaries are written with 16-byte stores, others with narrower ones.
 * mcbs_defender_wrapper_step_packed: mcbs_defender_wrapper_step with the packed row as its observation output.  On batches whose
 *   variant has fused_defender_obs (N <= 32, S <= 256) and with packed_out on a 16-byte boundary the turn launch writes the rows itself
 *   from its LDS stage: ONE launch; otherwise the turn runs without an observation and the kernel of mcbs_defender_observe_packed
 *   follows: two.  Everything else the call writes (every array of `w`) is bit for bit what mcbs_defender_wrapper_step writes.
 *   mcbs_defender_wrapper_step_packed_launches: 1 or 2 by the batch (an aligned packed_out assumed); 0 for NULL or a batch without a
 *   learned defender.
 * MCBS_EINVAL with a message, nothing launched: a NULL required pointer, a batch not created with MCBS_DEFENDER_EXTERNAL, row_words <
 * W_def, out_row_stride < F, an unknown dtype, both sources or neither, no index and n_rows > n_source_rows.  n_rows == 0 succeeds
 * without a launch.  All calls are stream-ordered, allocate nothing and never synchronise with the host. */
uint32_t mcbs_defender_obs_words(const mcbs_batch*);
int  mcbs_defender_observe_packed(mcbs_batch*, uint32_t* out, size_t row_words, void* stream);
int  mcbs_pack_defender_observation(const mcbs_batch*, const mcbs_defender_obs* dense, uint64_t n_rows, uint32_t* out, size_t row_words,
                                    void* stream);
int  mcbs_unpack_defender_observation(const mcbs_batch*, const uint32_t* packed, size_t row_words, const int64_t* index,
                                      uint64_t n_source_rows, uint64_t n_rows, const mcbs_defender_obs* out, void* stream);
int  mcbs_encode_defender_features(const mcbs_batch*, const mcbs_defender_obs* dense, const uint32_t* packed, size_t row_words,
                                   const int64_t* index, uint64_t n_source_rows, uint64_t n_rows, void* out, size_t out_row_stride,
                                   int32_t dtype, int32_t* bad_rows, void* stream);
int  mcbs_defender_wrapper_step_packed(mcbs_batch*, const int64_t* actions, uint32_t* packed_out, size_t row_words,
                                       const mcbs_defender_wrapper_buffers* w, const mcbs_defender_wrapper_cfg* cfg, void* stream);
int32_t mcbs_defender_wrapper_step_packed_launches(const mcbs_batch*);

/* ---- the two-agent turn: marl_algorithm.run_episode's loop body (marlon/baseline_models/multiagent/marl_algorithm.py:197-250) ---- */
typedef struct mcbs_episode_buffers {   /* 48 bytes: run_episode's per-env bookkeeping (marlon_amd/simulate.py), device arrays of n_envs */
    uint8_t* alive;            /* in/out: the env's episode is still running */
    double*  attacker_reward;  /* out: this turn's row of the attacker trace */
    double*  defender_reward;  /* out: this turn's row of the defender trace */
    int64_t* lengths;          /* in/out */
    uint8_t* attacker_done;    /* in/out */
    uint8_t* defender_done;    /* in/out */
} mcbs_episode_buffers;

/* 1: mcbs_two_agent_step serves this batch, in one launch; 0: it does not (the batch is outside the scope below; NULL: 0). */
int32_t mcbs_two_agent_step_launches(const mcbs_batch*);
/* One JOINT turn of both wrappers for every env in ONE launch (marlon_amd/csrc/mcbs_two_agent.hip): the attacker's wrapper step, the
 * defender's wrapper step and run_episode's bookkeeping.  The reference's defender predicts from the observation its own previous
 * step returned (marl_algorithm.py:222-225), so both agents' actions exist before the turn starts.
 * Scope: batches and requests for which mcbs_attacker_wrapper_step is one launch (packed, at most 16 nodes and cached credentials, no
 * mask field in obs, 16-byte aligned arrays) created with MCBS_DEFENDER_EXTERNAL, defender_obs given with its arrays on 16-byte
 * boundaries.  Anything else is MCBS_EINVAL with a message naming the reason; then nothing was launched and no state
 * changed.  There is no multi-launch fallback: a caller that needs one has mcbs_attacker_wrapper_step + mcbs_defender_wrapper_step.
 * Per env e, with a = ep->alive[e] on entry (1 when ep is NULL), the call equals that sequence bit for bit:
 *  1. the attacker half is mcbs_attacker_wrapper_step(..., auto_reset = 0, NULL, NULL) for EVERY env, alive or not: decode and
 *     interception, step, the five-field observation and the digest — taken between the attacker's action and the defender's turn —,
 *     `decoded`, every output of w and of info.  Attacker auto-reset is not part of this call: the episode boundary is the caller's.
 *  2. d1 = a && (w->terminated[e] | w->truncated[e]);  attacker_reward[e] = a ? (double)w->rewards[e] : 0.0.
 *  3. the defender half is mcbs_defender_wrapper_step for this env with the kind component of defender_actions[e] taken as -2 when
 *     !a || d1 (the array itself is never written): validity on the state before the tick, tick, action, then the reward shaping
 *     — which reads THIS turn's w->last_cyber_reward / has_cyber_reward and counts a parked env's turn as today's call does —,
 *     dw->valid / availability / evicted and every output of dw, then the four fields of defender_obs from the state after the action.
 *  4. stepped = a && !d1;  d2 = (stepped && (dw->terminated[e] | dw->truncated[e])) || d1;
 *     defender_reward[e] = stepped ? dw->reward[e] : (d1 ? -attacker_reward[e] : 0.0)    (defend_wrapper.py:269-271, -0.0 included).
 *  5. lengths[e] += a;  attacker_done[e] |= d1;  defender_done[e] |= d2 && a;  alive[e] = a && !(d1 || d2).
 * ep may be NULL: steps 2, 4 and 5 store nothing, and the attacker's own dones of this turn still park the defender (step 3). */
int  mcbs_two_agent_step(mcbs_batch*, const int64_t* multidiscrete, const int64_t* discrete, int32_t* decoded,
                         const mcbs_info_buffers* info, const mcbs_obs_buffers* obs, const mcbs_wrapper_buffers* w,
                         float invalid_action_reward_modifier, int32_t attacker_max_timesteps,
                         const int64_t* defender_actions, const mcbs_defender_obs* defender_obs,
                         const mcbs_defender_wrapper_buffers* dw, const mcbs_defender_wrapper_cfg* dcfg,
                         const mcbs_episode_buffers* ep, void* stream);

/* ---- the two-agent TRAINING turn: marl_algorithm.collect_rollouts' loop body (marlon/baseline_models/multiagent/marl_algorithm.py:17-54) ----
 * There each agent takes one perform_step per turn through its own DummyVecEnv, which resets its wrapper as soon as that wrapper reports
 * done.  Both wrappers share one environment, so a reset on one side reaches the other through the reset_request protocol
 * (attack_wrapper.py:342-343, 433-435; defend_wrapper.py:269-271, 446-447, 479-482; environment_event_source.py:30-38). */
typedef struct mcbs_training_buffers {   /* 136 bytes: device arrays of n_envs rows unless stated otherwise */
    uint8_t* attacker_reset_request;     /* in/out: AttackerEnvWrapper.reset_request — the defender reset the shared env on its own last turn */
    double*  defender_return;            /* in/out: the defender's running episode return */
    int64_t* attacker_valid_out;         /* out: the attacker's action counts including this step, taken before a reset clears them */
    int64_t* attacker_invalid_out;       /* out   (what the wrapper keeps as last_valid_action_count / last_invalid_action_count at a reset) */
    double*  defender_return_out;        /* out: return, length and action counts of the defender's episode including this step */
    int32_t* defender_length_out;        /* out */
    int64_t* defender_valid_out;         /* out */
    int64_t* defender_invalid_out;       /* out */
    uint8_t* defender_dones;             /* out: dw->terminated | dw->truncated of this turn */
    int8_t*  terminal_infected_nodes;            /* out [n_envs, N]: the defender's observation after its action — the terminal observation */
    int8_t*  terminal_incoming_firewall_status;  /* out [n_envs, N, 6]   of the envs whose defender_dones is set; other rows hold the same */
    int8_t*  terminal_outgoing_firewall_status;  /* out [n_envs, N, 6]   observation and mean nothing */
    int8_t*  terminal_services_status;           /* out [n_envs, S] */
    const int8_t* fresh_infected_nodes;           /* in [N]: the defender's observation of a freshly reset env, ONE row each */
    const int8_t* fresh_incoming_firewall_status; /* in [N, 6] */
    const int8_t* fresh_outgoing_firewall_status; /* in [N, 6] */
    const int8_t* fresh_services_status;          /* in [S]   (services never change: required, compared by nobody) */
} mcbs_training_buffers;

/* 1: mcbs_two_agent_train_step serves this batch, in one launch; 0: it does not (NULL: 0).  The scope is mcbs_two_agent_step's. */
int32_t mcbs_two_agent_train_step_launches(const mcbs_batch*);
/* One training turn of both auto-resetting wrappers for every env in ONE launch (marlon_amd/csrc/mcbs_two_agent.hip): what
 * collect_rollouts' two perform_step calls do to one shared environment, both DummyVecEnv resets and the hand-shake between them
 * included.  Scope and refusals are mcbs_two_agent_step's — MCBS_EINVAL with a message naming the reason, nothing launched, no state
 * changed, no multi-launch fallback — plus: keep / fresh must pair every requested observation field with its terminal array and its
 * reset row (as mcbs_attacker_wrapper_step's single launch needs them), every array of `tr` is required, the defender's terminal arrays
 * lie on 16-byte boundaries, and no array this call writes may share a byte with another array it reads or writes.  MCBS_ESTATE as
 * for mcbs_attacker_wrapper_step with auto_reset.
 * Per env e, with q = tr->attacker_reset_request[e] on entry, the call equals this sequence bit for bit:
 *  1. the attacker half is mcbs_attacker_wrapper_step(..., auto_reset = 1, keep, fresh) with ONE addition: w->truncated[e] |= q, so that
 *     w->dones[e] is raised as well (attack_wrapper.py:341-346).  With done1 = w->dones[e], everything that call does for an env that
 *     ends happens unchanged: terminal rows (for an intercepted action the live row as it stood — after a defender-side reset that is the
 *     gone episode's row), re-initialisation, wrapper_clear, fresh rows, a fresh digest, episode + 1.  tr->attacker_valid_out /
 *     attacker_invalid_out receive the counts including this step.  n = done1 && !q: the attacker's reset notifies the defender only
 *     when the attacker had not itself been asked (attack_wrapper.py:433-435).
 *  2. the defender half is mcbs_defender_wrapper_step for this env on the state as it now stands — freshly re-initialised when done1,
 *     and then without the attacker component, since step 1 cleared has_cyber_reward (the reference's cyber_rewards = []).
 *     If n: dw->truncated[e] = 1 and dw->reward[e] = -(double)w->rewards[e], which overrides the shaped value, -0.0 included;
 *     dw->terminated[e] stays as shaped (defend_wrapper.py:267-273).  done2 = dw->terminated[e] | dw->truncated[e] -> tr->defender_dones[e].
 *     tr->defender_return[e] += dw->reward[e]; the four defender_*_out arrays receive return, dw->timesteps and both counts, all
 *     including this step.  The four terminal_* arrays receive the observation after the defender's action.
 *  3. if done2: the env is re-initialised AGAIN (episode + 1 once more: the reference's second cyber_env.reset(), which discards what the
 *     defender just did); dw->timesteps, both counts, has_breached_sla and tr->defender_return go to zero, dw->prev_availability becomes
 *     the availability of a re-initialised env, and the live defender observation becomes the fresh rows; otherwise it is the terminal
 *     one.  tr->attacker_reset_request[e] = done2 && !n (defend_wrapper.py:446-447).  The attacker's observation rows, digest and
 *     counters are NOT touched: it keeps predicting from the observation of the episode that is gone, and so does its action mask
 *     (action_masking.py:90-94 builds it from the cached observation; the digest carries that observation's discovery order for it).
 *     Only the range check of its next action sees the new env.
 * The defender's actions are never written. */
int  mcbs_two_agent_train_step(mcbs_batch*, const int64_t* multidiscrete, const int64_t* discrete, int32_t* decoded,
                               const mcbs_info_buffers* info, const mcbs_obs_buffers* obs, const mcbs_wrapper_buffers* w,
                               float invalid_action_reward_modifier, int32_t attacker_max_timesteps,
                               const mcbs_row_copies* keep, const mcbs_row_copies* fresh,
                               const int64_t* defender_actions, const mcbs_defender_obs* defender_obs,
                               const mcbs_defender_wrapper_buffers* dw, const mcbs_defender_wrapper_cfg* dcfg,
                               const mcbs_training_buffers* tr, void* stream);

/* ---- the training turn for a trainer that stores PACKED observations on both sides ----
 * mcbs_training_buffers with the defender's packed rows in place of its eight int8 arrays: the nine per-env arrays keep their
 * order and meaning. */
typedef struct mcbs_training_packed_buffers {   /* 88 bytes: device arrays of n_envs rows unless stated otherwise */
    uint8_t* attacker_reset_request;     /* in/out */
    double*  defender_return;            /* in/out */
    int64_t* attacker_valid_out;         /* out */
    int64_t* attacker_invalid_out;       /* out */
    double*  defender_return_out;        /* out */
    int32_t* defender_length_out;        /* out */
    int64_t* defender_valid_out;         /* out */
    int64_t* defender_invalid_out;       /* out */
    uint8_t* defender_dones;             /* out */
    uint32_t* terminal_defender_packed;      /* out [n_envs, defender_row_words]: the defender's packed row after its action — the terminal
                                                observation of the envs whose defender_dones is set; other rows hold the same row and mean nothing */
    const uint32_t* fresh_defender_packed;   /* in [W_def]: the defender's packed row of a freshly reset env, ONE row */
} mcbs_training_packed_buffers;

/* 1: mcbs_two_agent_train_step_packed serves this batch with this packing, in one launch; 0: it does not (NULL: 0). */
int32_t mcbs_two_agent_train_step_packed_launches(const mcbs_batch*, const mcbs_obs_packing* packing);
/* mcbs_two_agent_train_step with BOTH observations written as packed rows by the same ONE launch (marlon_amd/csrc/mcbs_two_agent.hip
 * two_agent_train_packed_kernel): the attacker's as mcbs_attacker_wrapper_step_packed writes them (packing, packed, packed_terminal,
 * packed_fresh, row_words: see there), the defender's as the W_def words of "packed defender observations" above — defender_packed
 * [n_envs, defender_row_words] the live rows, tr->terminal_defender_packed the rows after the defender's action, and
 * tr->fresh_defender_packed the row that becomes the live row of an env the defender ends.  No int32 or int8 observation array exists
 * in this call, nothing is packed by a second launch, nothing dense is read back.
 * Contract.  Per env the call equals mcbs_two_agent_train_step bit for bit in every array of w, info, dw, decoded, the digests, the
 * nine shared members of tr and the env state.  Live and terminal rows equal mcbs_pack_observation of the attacker's rows and
 * mcbs_pack_defender_observation of the defender's rows as that call writes them: the attacker's live row of an env whose action was
 * intercepted stands, its terminal rows are written for the envs the attacker's step ends only, and after a defender-side reset the
 * attacker's rows and digest are not touched; the defender's terminal and live rows are written for every env.  Every word below W
 * (W_obs, W_def) of a written row is stored whole; words from W on, and rows that stand, are never touched.
 * Scope: the intersection of mcbs_two_agent_train_step's batches, the packed step's LDS room (W_obs <= 128 and W_obs + 1 + V <= 896) and
 * the defender turn that writes its own observation (N <= 32, S <= 256: W_def <= 21).  There is no multi-launch form and no mixed
 * form (one side packed, the other dense).  MCBS_EINVAL with a message naming the reason — nothing launched, no state changed — for:
 * a batch outside the scope; a packing created for another device or geometry; row_words < W_obs or defender_row_words < W_def;
 * defender_packed or tr->terminal_defender_packed off a 16-byte boundary, or defender rows that neither follow each other without a gap
 * (defender_row_words == W_def) nor are a multiple of 4 words apart (the turn kernels' 16-byte store condition); a NULL argument or
 * member; both action encodings or neither; any written array that shares a byte with another array of the call.  MCBS_ESTATE as for
 * mcbs_two_agent_train_step. */
int  mcbs_two_agent_train_step_packed(mcbs_batch*, const int64_t* multidiscrete, const int64_t* discrete, int32_t* decoded,
                                      const mcbs_info_buffers* info, const mcbs_obs_packing* packing, uint32_t* packed,
                                      uint32_t* packed_terminal, const uint32_t* packed_fresh, size_t row_words,
                                      const mcbs_wrapper_buffers* w, float invalid_action_reward_modifier, int32_t attacker_max_timesteps,
                                      const int64_t* defender_actions, uint32_t* defender_packed, size_t defender_row_words,
                                      const mcbs_defender_wrapper_buffers* dw, const mcbs_defender_wrapper_cfg* dcfg,
                                      const mcbs_training_packed_buffers* tr, void* stream);

/* Parity / debugging: canonical per-env state records (layout: mcbs_state_record below),
 * host buffers, synchronous.  The record does not carry what only MCBS_DEFENDER_RANDOM_EVENTS mutates (vulnerability keys,
 * service flags, firewall rule lists): mcbs_set_state puts those back to the topology's initial ones for the envs it writes. */
size_t mcbs_state_record_bytes(const mcbs_batch*);
int  mcbs_get_state(mcbs_batch*, void* host_buf, size_t nbytes);
int  mcbs_set_state(mcbs_batch*, const void* host_buf, size_t nbytes);

/* Which compiled variant this batch's calls dispatch to, decided at batch creation (tests assert the cell they reach).  Read-only: the
 * query changes no dispatch decision.  Per-call conditions are not included (mcbs_defender_step also needs 16-byte aligned observation
 * arrays for the fused observation; mcbs_attacker_wrapper_step's single launch also needs no mask field and aligned rows). */
typedef struct mcbs_batch_variant_info {   /* 32 bytes */
    uint32_t packed;              /* 1: packed sets (16-bit fields, 4-byte rows): N <= 16 and few credentials */
    uint32_t words_per_set;       /* 1, 2 or 4: 64-bit words of a per-env node / credential set in the general layout */
    uint32_t wide;                /* 1: the cached-triple set lives in a column of its own (more than 256 cacheable credentials) */
    uint32_t coop;                /* 1: mcbs_step runs the G-lanes-per-env kernel (G = words_per_set) */
    uint32_t lds_topo;            /* always 0: the step kernel that staged the topology's hot image in LDS is gone; the field keeps the layout */
    uint32_t defender_kind;       /* MCBS_DEFENDER_* of the batch */
    uint32_t fused_wrapper;       /* 1: the batch admits the one-launch mcbs_attacker_wrapper_step */
    uint32_t fused_defender_obs;  /* 1: learned-defender turns can write the observation themselves (N <= 32, at most 256 services) */
} mcbs_batch_variant_info;
int  mcbs_batch_variant(const mcbs_batch*, mcbs_batch_variant_info* out);
/* 1: an mcbs_step of this batch with (with_info != 0) or without info buffers takes the lean launch — the packed, attacker-only whole
 * step with the argument block that holds only what it reads (marlon_amd/csrc/mcbs_step.hip); 0: the full argument list, or a null
 * batch.  Decided at batch creation except for the info buffers, which are per call.  (A query of its own: the variant record above
 * is fixed at 32 bytes.) */
int32_t mcbs_step_is_lean(const mcbs_batch*, int32_t with_info);

/* Topology traits: what the vulnerability descriptors and the node count of a topology make possible, found on the host when the
 * topology's tables are built and fixed for the life of every batch on it.  A bit that is CLEAR is a rule of the reference no step of
 * this topology can trigger; the narrow lean step kernel (marlon_amd/csrc/mcbs_step.hip) compiles such rules out. */
#define MCBS_TOPO_ESCALATION      1u   /* some vulnerability's outcome is a privilege escalation */
#define MCBS_TOPO_LATERAL_EXPLOIT 2u   /* some vulnerability's outcome is a lateral move (connecting with a credential is not meant) */
#define MCBS_TOPO_PRECONDITION    4u   /* some vulnerability's precondition is false for some tag set of its node (precond_tt != 0xFFFF) */
#define MCBS_TOPO_PROBE           8u   /* some vulnerability's outcome is ProbeSucceeded */
#define MCBS_TOPO_MULTI_LEAK      16u  /* some vulnerability leaks more than one node id / credential */
#define MCBS_TOPO_WIDE_ROWS       32u  /* more than 12 nodes: a packed env's node rows need a fourth 16-byte vector (reported; no kernel assumes it away) */
#define MCBS_TOPO_ANY             63u
/* The traits of a topology blob (the one mcbs_topology_create takes), computed on the host alone: no device is touched.  MCBS_OK, or
 * the error mcbs_topology_create would report for the blob. */
int  mcbs_topology_traits(const void* blob, size_t nbytes, uint32_t* traits);
/* 1: an mcbs_step of this batch with (with_info != 0) or without info buffers takes the NARROW lean kernel — the lean launch above
 * instantiated for topologies without privilege escalation, lateral-move exploits, preconditions and multi-entry leaks; 0: any other
 * kernel, or a null batch.  Decided at batch creation: the batch is lean and its topology has none of the traits
 * the instantiation assumes away.  *traits (may be null) receives the topology's MCBS_TOPO_* bits. */
int32_t mcbs_step_topo_traits(const mcbs_batch*, int32_t with_info, uint32_t* traits);

/* Kernel timing hook for bench.py: HIP events recorded on `stream` around each mcbs_step launch
 * while enabled; mcbs_timing_read synchronises and returns the summed kernel milliseconds. */
int  mcbs_timing_enable(mcbs_batch*, int32_t on);
int  mcbs_timing_read(mcbs_batch*, double* total_ms, uint64_t* launches);

/* Canonical state record (host side, used by get/set_state and the oracle's dump):
 * fixed header followed by n_nodes node records, the discovery order and the credential cache. */
typedef struct mcbs_state_header { /* 64 bytes */
    uint32_t step_count, done, truncated, episode;
    uint32_t n_discovered, n_creds;
    uint32_t last_outcome_kind, last_escalation;
    uint32_t last_new_nodes, last_new_creds, last_oob, pad0;
    double   cum_reward;
    double   availability;
} mcbs_state_header;

typedef struct mcbs_state_node { /* 32 bytes */
    uint64_t discovered_props;
    uint32_t attacked_ever;   /* bit s: slot s exploited at least once (actions.py:396-407) */
    uint32_t attacked_since;  /* bit s: ... since the node's last re-imaging */
    uint8_t  discovered, installed, ever_owned, running;
    uint8_t  privilege, tags, countdown, pad;
    uint32_t pad1[2];
} mcbs_state_node;
/* followed by uint16 discovery_order[n_nodes] and uint16 credential_cache[max_total_credentials] (triple ids) */

#ifdef __cplusplus
}
#endif
#endif /* MCBS_H */
