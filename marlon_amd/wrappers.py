"""Batched counterparts of marlon's attacker env wrappers.

`AttackerVecEnv` is `AttackerEnvWrapper` (marlon/baseline_models/env_wrappers/attack_wrapper.py) for a whole batch
of environments living on the GPU, with the Stable-Baselines3 `VecEnv` calling convention the reference reaches
through `DummyVecEnv([...])` (marlon/baseline_models/ppo_multi/train_marl_multi.py:181-183):

  * action: MultiDiscrete `[3, N, L, N, N, R, N, N, P, C]` rows `[kind, l_src, l_vuln, r_src, r_tgt, r_vuln, c_src,
    c_tgt, c_port, c_cred]` (attack_wrapper.py:206-227) or, with `discrete=True`, the single Discrete index of
    `MaskedDiscreteAttackerWrapper` (action_masking.py:30-142) — decoded on the device by `mcbs_decode_attacker_actions`;
  * an action whose node index is not discovered yet does NOT step the env: the last observation is returned,
    reward is `0 + invalid_action_reward_modifier`, `info["invalid_action"]` is set (attack_wrapper.py:286-308);
  * observation: the flat dict of attack_wrapper.py:474-522, every value a device tensor with a leading env axis
    (`scalars` also split into the seven named integer keys); `action_masks()` = action_masking.py:90-110;
  * `timesteps` counts wrapper steps (invalid ones included) and truncates at `max_timesteps` (:346-352);
  * finished envs are reset inside `step` like a VecEnv does; the observation that ended the episode is kept in
    `terminal_observation` for the envs flagged in `dones`;
  * a step's output tensors (rewards, flags, info) are valid until the step after next (two alternating sets; with `use_graph` the
    one persistent set is overwritten by the next step); the observation tensors are the wrapper's own persistent buffers;
  * `observation_format="packed"` (small topologies, `materialize_masks=False`): the step itself writes each env's observation as the
    bit-packed row of `features.ObservationPacking` (mcbs_attacker_wrapper_step_packed, one launch) and no int32 field exists:
    `observation` is `{"packed": int32 [E, W_obs]}`, `features()` / `first_layer()` / `rollout_buffer()` work from those rows.

All simulation work is in the HIP kernels; the few tensor expressions here are the wrapper's own bookkeeping
(timestep counters, reward modifier).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from ._abi import EnvSpec
from .cyberbattle_env import (SCALAR_KEYS, AttackerGoal, DefenderConstraint, DefenderGoal, spec_from_kwargs)
from .flatten import FlatTopology, flatten

# what the engine writes; the three separate action masks of marlon's observation dict are VIEWS into mask_discrete
# (connect | local | remote, action_masking.py:96-110): the same bytes, written once
FLAT_FIELDS = ["scalars", "leaked_credentials", "credential_cache_matrix", "discovered_nodes_properties",
               "nodes_privilegelevel", "mask_discrete"]

# a step's alternating output sets: name and dtype of each [n_envs] tensor (_output_set)
_ATTACKER_OUTPUTS = (("invalid", "uint8"), ("executed", "bool"), ("rewards", "float32"), ("truncated", "uint8"), ("ret", "float64"),
                     ("length", "int32"), ("terminated", "uint8"))
_DEFENDER_OUTPUTS = (("valid", "uint8"), ("availability", "float64"), ("reward", "float64"), ("terminated", "uint8"), ("truncated", "uint8"),
                     ("breached", "uint8"), ("won", "uint8"))
_TRAINING_OUTPUTS = (("attacker_valid_out", "int64"), ("attacker_invalid_out", "int64"), ("defender_return_out", "float64"),
                     ("defender_length_out", "int32"), ("defender_valid_out", "int64"), ("defender_invalid_out", "int64"), ("defender_dones", "uint8"))


def _output_set(venv, table) -> Dict[str, object]:
    t = venv.torch
    return {k: t.empty(venv.num_envs, dtype=getattr(t, dtype), device=venv.engine.device) for k, dtype in table}


def _as_actions(att, a, shape, wording: str):
    """Whatever the caller passed as actions -> a contiguous int64 tensor of `shape` on the device of `att` (an AttackerVecEnv).  The
    common case — the policy's own int64 tensor — is returned as it is.  Another shape is a ValueError opening with the caller's wording."""
    t = att.torch
    if not (type(a) is t.Tensor and a.dtype is t.int64 and a.is_cuda and a.get_device() == att._dev_index and a.is_contiguous()):
        a = a if isinstance(a, t.Tensor) else t.as_tensor(np.asarray(a))
        a = a.to(device=att.engine.device, dtype=t.int64).contiguous()
    if a.shape != shape:
        raise ValueError(f"{wording} {tuple(shape)}, got {tuple(a.shape)}")
    return a


def _stage_actions(venv, actions):
    """use_graph: the caller's actions copied into the wrapper's persistent action buffer, which the step then reads."""
    t = venv.torch
    a = actions if isinstance(actions, t.Tensor) else t.as_tensor(np.asarray(actions))
    venv._act_in.copy_(a.to(device=venv.engine.device).reshape(venv._act_in.shape), non_blocking=True)
    return venv._act_in


def _observation_storage(venv, store_observations: bool, pack_observations: Optional[bool], fields, words, wrapper: str, kind: str):
    """What rollout_buffer() hands DeviceRolloutBuffer as obs: None, the wrapper's fields() or one "packed" key of words() words per row
    (pack_observations; the default for a wrapper with observation_format="packed", which has no `kind` field to store instead;
    `wrapper`: the class's name in that refusal)."""
    if pack_observations is None:
        pack_observations = venv._packed_mode
    if venv._packed_mode and store_observations and not pack_observations:
        raise ValueError(f"rollout_buffer(pack_observations=False): this {wrapper} was created with observation_format='packed' "
                         f"and keeps no {kind} field to store")
    if not store_observations:
        return None
    if pack_observations:
        return {"packed": venv.torch.zeros((venv.num_envs, words()), dtype=venv.torch.int32, device=venv.engine.device)}
    return fields()


def _two_agent_refusal(att, dfd, turn: str, auto_reset: bool, auto_reset_why: str, launches: str, packed_launches: Optional[str] = None) -> Optional[str]:
    """Why the `turn` ("joint" / "training") turn does not take this attacker wrapper, or this pair: the first of nine conditions that
    fails, else None.  launches: the engine's query for the turn's entry point.  packed_launches: the query for the entry point that
    writes BOTH observations as packed rows, where the turn has one — a packed attacker is then taken together with a packed defender
    (with dfd None: asked about), and only the mixed pairs are refused."""
    from ._abi import DEFENDER_EXTERNAL
    if not isinstance(att, AttackerVecEnv):
        return "the attacker side must be an AttackerVecEnv"
    if att.engine._cfg.defender_kind != DEFENDER_EXTERNAL:
        return "the AttackerVecEnv must be created with learned_defender=True"
    if bool(att.auto_reset) != auto_reset:
        return f"the AttackerVecEnv must be created with auto_reset={auto_reset} ({auto_reset_why})"
    if att.materialize_masks:
        return f"the AttackerVecEnv must be created with materialize_masks=False (the {turn} turn writes no mask field)"
    if att.use_graph:
        return "the AttackerVecEnv must be created with use_graph=False"
    # a packed attacker is one half of a packed pair where the turn has an entry point that writes packed rows and that entry point
    # serves this batch (an engine without the query serves none); everywhere else the fields form is what to ask for
    packed_query = getattr(att.engine, packed_launches, None) if packed_launches is not None and att.observation_format == "packed" else None
    packed_pair = packed_query is not None and packed_query(att._packing_handle()) == 1
    if att.observation_format != "fields" and not packed_pair:
        return f"the AttackerVecEnv must be created with observation_format='fields' (the {turn} turn writes the int32 fields, not packed rows)"
    if not packed_pair and getattr(att.engine, launches)() != 1:
        return f"the library does not serve this batch with a {turn} turn (mcbs_{launches}: small packed topologies only)"
    if dfd is not None and not (isinstance(dfd, DefenderVecEnv) and dfd.attacker is att and not dfd.use_graph):
        return "the defender side must be the DefenderVecEnv created on this AttackerVecEnv (use_graph=False)"
    if dfd is not None and packed_pair and dfd.observation_format != "packed":
        return ("both wrappers of a pair must have the same observation_format: this AttackerVecEnv writes packed rows, so the DefenderVecEnv "
                f"must be created with observation_format='packed' too (the {turn} turn has no mixed form)")
    if dfd is not None and not packed_pair and dfd.observation_format != "dense":
        return "the DefenderVecEnv must be created with observation_format='dense' (these turns write the int8 fields, not packed rows)"
    return None


class _MultiDiscreteHead:
    """The MultiDiscrete head (mcbs_multicategorical) for a wrapper with `engine`, `num_envs` and `nvec`: SB3's
    MultiCategoricalDistribution over the wrapper's MultiDiscrete(nvec) action, one launch each way."""

    def _check_multidiscrete(self) -> None:
        pass

    def sample_actions(self, logits, seed: int, step: int, deterministic: bool = False, uniforms=None, out=None):
        """An action row per env from the policy's logits [n_envs, >= sum(nvec)] (float32 / bfloat16, never modified): per dimension a
        Categorical over its own segment of the row -> MultiCategorical(actions int64 [n_envs, D], log_prob, entropy), the latter two
        summed over the dimensions.  deterministic: per dimension the largest logit (lowest index among equal ones).  Rows are keyed by
        (seed, global env id, step): shards of one batch draw what the whole batch would; pass the rollout step as `step`.  uniforms
        (device float32 [n_envs, D] in [0, 1)) replaces the key, e.g. under graph capture."""
        self._check_multidiscrete()
        if logits is not None and logits.shape[0] != self.num_envs:
            raise ValueError(f"logits has {logits.shape[0]} rows, the wrapper {self.num_envs} envs")
        return self.engine.multicategorical(logits, self._nvec, mode="argmax" if deterministic else "sample", seed=seed, step=step,
                                            uniforms=uniforms, row_key_base=self.engine.spec.env_id_base, out=out)

    def sample_uniform(self, seed: int, step: int, uniforms=None, out=None):
        """action_space.sample() of the reference's random agents in law: every component uniform over its range = sample_actions with no
        logits at all (log_prob = -sum log nvec[d])."""
        self._check_multidiscrete()
        return self.engine.multicategorical(None, self._nvec, mode="sample", seed=seed, step=step, uniforms=uniforms,
                                            row_key_base=self.engine.spec.env_id_base, out=out)

    def evaluate_actions(self, logits, actions, differentiable: bool = False, bad_actions=None, out=None):
        """PPO's evaluate_actions for stored rows: log_prob of `actions` int64 [n, D] and the entropy under logits [n, >= sum(nvec)], any
        n.  The log_prob of an action sample_actions drew from the same logits comes back bit for bit.  differentiable=True: the same
        numbers, and log_prob and entropy carry an autograd graph into `logits` (engine.multicategorical_evaluate: the backward pass is
        one launch of mcbs_multicategorical_grad); out= cannot be combined with it."""
        self._check_multidiscrete()
        if differentiable:
            if out is not None:
                raise ValueError("evaluate_actions(differentiable=True) allocates its outputs: out= is not supported")
            return self.engine.multicategorical_evaluate(logits, self._nvec, actions, bad_actions=bad_actions)
        return self.engine.multicategorical(logits, self._nvec, mode="evaluate", actions=actions, bad_actions=bad_actions, out=out)


class AttackerVecEnv(_MultiDiscreteHead):
    def __init__(self, initial_environment, n_envs: int, maximum_total_credentials: int = 1000, maximum_node_count: int = 100,
                 maximum_discoverable_credentials_per_action: int = 5, defender_agent=None,
                 attacker_goal: Optional[AttackerGoal] = AttackerGoal(own_atleast_percent=1.0),
                 defender_goal=DefenderGoal(eviction=True), defender_constraint=DefenderConstraint(maintain_sla=0.0),
                 winning_reward=5000.0, losing_reward=0.0, max_timesteps: int = 2000, invalid_action_reward_modifier=-1,
                 discrete: bool = False, auto_reset: bool = True, device: Optional[str] = None, seed: int = 0,
                 env_id_base: int = 0, rng_kind: int = 0, learned_defender: bool = False, materialize_masks: bool = True,
                 use_graph: bool = False, observation_format: str = "fields"):
        from .engine import BatchEngine
        if observation_format not in ("fields", "packed"):
            raise ValueError(f"observation_format must be 'fields' or 'packed', got {observation_format!r}")
        # observation_format="packed": the step itself writes the packed row (features.ObservationPacking; Chain-10 at 12/12: 72 B per env
        # instead of 924 B) and the wrapper keeps no int32 observation at all: `observation` is {"packed": rows}, features() and
        # first_layer() read the rows, rollout_buffer() stores them.  One launch per step (mcbs_attacker_wrapper_step_packed): small
        # topologies, no materialised masks.
        self.observation_format = observation_format
        self._packed_mode = observation_format == "packed"
        if self._packed_mode and materialize_masks:
            raise ValueError("observation_format='packed' needs materialize_masks=False: the packed step writes no mask field "
                             "(apply the mask with mask_logits / action_masks_packed)")
        self.topo: FlatTopology = initial_environment if isinstance(initial_environment, FlatTopology) else flatten(initial_environment)
        # the wrapper owns truncation and resets (its clock counts invalid actions too), so the engine's own are off
        self.spec: EnvSpec = spec_from_kwargs(n_envs, maximum_total_credentials, maximum_node_count,
                                              maximum_discoverable_credentials_per_action, defender_agent, attacker_goal,
                                              defender_goal, defender_constraint, winning_reward, losing_reward,
                                              auto_reset=False, max_episode_steps=0, seed=seed, env_id_base=env_id_base, rng_kind=rng_kind)
        if learned_defender:
            if defender_agent is not None:
                raise ValueError("a learned defender replaces the in-env defender_agent (multiagent_universe.py:160-167)")
            self.spec.defender = ("external",)
        self.engine = BatchEngine(self.topo, self.spec, device=device)
        t = self.torch = self.engine.torch
        self.num_envs = n_envs
        self.max_timesteps = int(max_timesteps)
        self.invalid_action_reward_modifier = float(invalid_action_reward_modifier)
        self.discrete = bool(discrete)
        self.auto_reset = bool(auto_reset)
        N, Cm = maximum_node_count, maximum_total_credentials
        L, R, P = len(self.topo.local_vulnerabilities), len(self.topo.remote_vulnerabilities), len(self.topo.ports)
        self.nvec = np.array([3, N, L, N, N, R, N, N, P, Cm], dtype=np.int64)                      # attack_wrapper.py:206-227
        self._nvec = tuple(int(v) for v in self.nvec)
        self.discrete_n = N * N * P * Cm + N * L + N * N * R                                         # action_masking.py:74-80
        dev = self.engine.device
        # materialize_masks=False: the three action masks (94 % of the observation's bytes) are not written at all; a policy applies them
        # to its logits with mask_logits() (mcbs_mask_logits: rebuilt on the device from the observation's digest).  The observation
        # dict then has no local_vulnerability / remote_vulnerability / connect entries and action_masks() raises.
        self.materialize_masks = bool(materialize_masks)
        if self.materialize_masks:
            # rows of the flat mask padded to whole 128-byte lines: dense rows (Chain-10: 14 172 bytes) share cache lines with their
            # neighbours, which cost the Discrete observation a quarter of its write bandwidth; consumers see [:, :discrete_n] views
            self.engine.set_mask_discrete_stride((self.discrete_n + 127) // 128 * 128)
        self._obs_packing = None                                   # observation_packed(): the packing handle, made on first use
        if self._packed_mode:
            why = None
            if self.engine.wrapper_step_launches(False) != 1:
                why = ("the wrapper step of this batch is not one launch (engine.wrapper_step_launches(False) != 1: small topologies of at "
                       "most 16 nodes and cached credentials, not the random-events defender)")
            elif not self._packing_handle().packing.fits_packed_step:
                why = "the packed row is beyond the room the step keeps for it (features.PACKED_STEP_MAX_WORDS)"
            if why:
                self.engine.close()
                raise ValueError(f"observation_format='packed': {why}")
            # no int32 observation is kept: the live rows (persistent: an intercepted env's row must stand), the terminal rows, one fresh row
            W = self._packing_handle().words
            self._obs = self._terminal = None
            self.packed_observation = t.zeros((n_envs, W), dtype=t.int32, device=dev)
            self.terminal_packed_observation = t.zeros((n_envs, W), dtype=t.int32, device=dev)
            self._packed_fresh = None
        else:
            self._obs = self.engine.alloc_obs(FLAT_FIELDS if self.materialize_masks else FLAT_FIELDS[:-1])
            self._terminal = {k: t.zeros_like(v) for k, v in self._obs.items()}
        self._mask_split = (N * N * P * Cm, N * L, (N, N, P, Cm), (N, L), (N, N, R))
        self._rows = t.zeros((n_envs, 5), dtype=t.int32, device=dev)
        self._invalid = t.zeros(n_envs, dtype=t.uint8, device=dev)
        self.timesteps = t.zeros(n_envs, dtype=t.int32, device=dev)
        self.valid_action_count = t.zeros(n_envs, dtype=t.int64, device=dev)
        self.invalid_action_count = t.zeros(n_envs, dtype=t.int64, device=dev)
        self.episode_returns = t.zeros(n_envs, dtype=t.float64, device=dev)
        self.last_cyber_reward = t.zeros(n_envs, dtype=t.float32, device=dev)
        self.has_cyber_reward = t.zeros(n_envs, dtype=t.bool, device=dev)    # AttackerEnvWrapper.cyber_rewards is non-empty
        # outputs of the fused bookkeeping / auto-reset launch (mcbs_attacker_wrapper_finish) and its argument blocks
        self._rewards = t.zeros(n_envs, dtype=t.float32, device=dev)
        self._truncated = t.zeros(n_envs, dtype=t.uint8, device=dev)
        self._dones = t.zeros(n_envs, dtype=t.uint8, device=dev)
        self._ret_out = t.zeros(n_envs, dtype=t.float64, device=dev)
        self._len_out = t.zeros(n_envs, dtype=t.int32, device=dev)
        self._n_done = t.zeros(1, dtype=t.int32, device=dev)
        self._wb = self._keep = self._fresh = self._obs_block = self._reset_rows = None
        self._calls = {}                                   # bound library calls (engine.wrapper_step_call), one per output set and settings
        self._dev_index = self.engine.device.index if self.engine.device.index is not None else t.cuda.current_device()
        self._action_shape = (n_envs,) if self.discrete else (n_envs, 10)
        self._obs_views = self._terminal_views = None
        self._ring, self._slot = None, 0
        self._one_launch = None
        # use_graph: the whole wrapper step (decode, environment step + observation, bookkeeping, terminal-observation copy, reset and reset
        # observation of the envs that ended) is captured into ONE hipGraph on the first call and replayed afterwards: the step has no
        # host round trip, so what remains on the host is one graph launch.  Outputs are then the wrapper's own buffers (overwritten
        # by the next step) instead of copies.  Not with a draw tape (its address changes per step).
        self.use_graph = bool(use_graph)
        if self.use_graph and rng_kind == 1:
            raise ValueError("use_graph replays fixed kernel arguments: it cannot be combined with a defender draw tape (rng_kind=TAPE)")
        self._graph = None
        self._act_in = t.zeros((n_envs,) if self.discrete else (n_envs, 10), dtype=t.int64, device=dev)
        self._executed = t.zeros(n_envs, dtype=t.bool, device=dev)
        self._graph_out = self._terminated_out = None
        self._feature_handles, self._feature_bits = {}, None       # features(): layout handles per option set, the packed-mask scratch
        self.reset()

    # -- observation plumbing --
    def _public(self, obs: Dict[str, object]) -> Dict[str, object]:
        M, ML, s_connect, s_local, s_remote = self._mask_split
        out = {}
        if "mask_discrete" in obs:
            flat = obs["mask_discrete"][:, :self.discrete_n]          # (rows are padded to whole cache lines)
            out = {"local_vulnerability": flat[:, M:M + ML].unflatten(1, s_local), "remote_vulnerability": flat[:, M + ML:].unflatten(1, s_remote),
                   "connect": flat[:, :M].unflatten(1, s_connect)}
        out.update({
               "leaked_credentials": obs["leaked_credentials"].reshape(self.num_envs, -1),
               "credential_cache_matrix": obs["credential_cache_matrix"].reshape(self.num_envs, -1),
               "discovered_nodes_properties": obs["discovered_nodes_properties"].reshape(self.num_envs, -1),
               "nodes_privilegelevel": obs["nodes_privilegelevel"]})
        for i, k in enumerate(SCALAR_KEYS):
            out[k] = obs["scalars"][:, i]
        return out

    @property
    def observation(self) -> Dict[str, object]:
        # views of the wrapper's persistent observation tensors: built once (a dozen view operations cost more host time than the
        # device needs for the whole step)
        if self._packed_mode:
            return {"packed": self.packed_observation}
        if self._obs_views is None:
            self._obs_views = self._public(self._obs)
        return dict(self._obs_views)

    @property
    def terminal_observation(self) -> Dict[str, object]:
        if self._packed_mode:
            return {"packed": self.terminal_packed_observation}
        if self._terminal_views is None:
            self._terminal_views = self._public(self._terminal)
        return dict(self._terminal_views)

    def action_masks(self):
        """[n_envs, N*N*P*C + N*L + N*N*R] bool, MaskedDiscreteAttackerWrapper order (connect, local, remote)."""
        if not self.materialize_masks:
            raise RuntimeError("this AttackerVecEnv was created with materialize_masks=False: apply the mask with mask_logits(logits)")
        return self._obs["mask_discrete"].view(self.torch.bool)[:, :self.discrete_n]      # the int8 mask holds 0 / 1 only: a bool view (rows padded
                                                                                           # to whole cache lines), no second gigabyte

    def mask_logits(self, logits, fill: float = -1e8):
        """`where(action_masks(), logits, fill)` in place on the device, without the mask: what MaskablePPO's MaskableCategorical does
        with action_masks() (train_marl_multi.py:259-293), straight from the digest of the observation this env last returned."""
        return self.engine.mask_logits(logits, fill)

    def action_masks_packed(self, out=None):
        """action_masks() as one bit per action: device int32 [n_envs, row_words] (engine.pack_action_mask), bit a of row e = bit
        (a & 31) of word a >> 5.  Works whether or not the masks are materialised (with materialize_masks=False the step stays one
        launch and this is a second).  out=: write straight into a preallocated buffer, e.g. buffer[t] of a [T, n_envs, row_words]
        rollout buffer, for apply_packed_mask at update time."""
        return self.engine.pack_action_mask(out)

    def action_mask_keys(self, out=None):
        """action_masks_packed() as a KEY: device int32 [n_envs, Wk] (engine.store_mask_keys; Chain-10 at 12/12: 5 words instead of
        443), the few words the mask of the observation this env last returned is a function of.  expand_mask_keys turns stored keys
        back into exactly the packed masks, at any later time.  out=: write straight into a preallocated buffer, e.g. buffer[t] of a
        [T, n_envs, Wk] rollout buffer.  Not under ExternalRandomEvents (the mask is no function of the key there)."""
        return self.engine.store_mask_keys(out)

    def expand_mask_keys(self, keys, index=None, out=None):
        """Stored keys [n_source, >= Wk] -> packed masks [n, row_words], row i from key row index[i] (int64 [n]; without an index:
        row i): what action_masks_packed() returned at the step each key was stored, for apply_packed_mask / evaluate_masked /
        evaluate_masked_from_latent / encode_features_packed.  out=: a preallocated int32 [n, >= W] tensor."""
        return self.engine.expand_mask_keys(keys, index, out)

    def apply_packed_mask(self, bits, logits, fill: float = -1e8):
        """`where(mask, logits, fill)` in place for stored packed masks bits [n, >= W] and logits [n, >= A], any n."""
        return self.engine.apply_packed_mask(bits, logits, fill)

    def unpack_action_mask(self, bits, out=None):
        """Packed masks [n, >= W] -> bool [n, A] (what action_masks() returns for the same step)."""
        return self.engine.unpack_action_mask(bits, out)

    # -- the MultiDiscrete head (discrete=False: the reference's unmasked PPO attacker): sample_actions / sample_uniform / evaluate_actions --
    def _check_multidiscrete(self) -> None:
        if self.discrete:
            raise RuntimeError("this AttackerVecEnv was created with discrete=True, its action is one Discrete index: use sample_masked / "
                               "sample_masked_uniform / evaluate_masked")

    # -- the masked categorical head (mcbs_masked_categorical): MaskableCategorical's sample / log_prob / entropy in one launch --
    def _live_bits(self, caller: str = "the masked categorical head"):
        """None where the live form serves (the mask is rebuilt from the digest); under ExternalRandomEvents, where it cannot be, the
        materialised mask packed with torch expressions (rows are then keyed by their index).  caller: who asks, for the refusal."""
        from ._abi import DEFENDER_RANDOM_EVENTS
        if self.engine._cfg.defender_kind != DEFENDER_RANDOM_EVENTS:
            return None
        if not self.materialize_masks:
            raise RuntimeError(f"{caller} under ExternalRandomEvents needs the materialised masks (the mask cannot be "
                               "rebuilt from the observation digest there): create the env with materialize_masks=True")
        return self._pack_bits_from_mask(self.action_masks())

    def sample_masked(self, logits, seed: int, step: int, deterministic: bool = False, uniforms=None, out=None):
        """An action per env from `Categorical(logits=where(action_masks(), logits, -1e8))` for the observation this env last returned,
        without the mask and without touching the logits: -> MaskedCategorical(actions, log_prob, entropy, n_allowed).
        deterministic: the allowed action with the largest logit (lowest index among equal ones).  Rows are keyed by (seed, global env
        id, step): pass the rollout step as `step`; uniforms (device float32 [n_envs] in [0, 1)) replaces the key, e.g. under graph
        capture."""
        return self.engine.masked_categorical(logits, bits=self._live_bits(), mode="argmax" if deterministic else "sample", seed=seed, step=step,
                                              uniforms=uniforms, out=out)

    def sample_masked_uniform(self, seed: int, step: int, uniforms=None, out=None):
        """The reference's masked random agent: uniform over np.flatnonzero(action_masks()) (random_marlon_agent.py:88-95) =
        sample_masked with no logits at all."""
        return self.sample_masked(None, seed, step, uniforms=uniforms, out=out)

    def evaluate_masked(self, bits, logits, actions, bad_actions=None, out=None, differentiable: bool = False):
        """MaskablePPO's evaluate_actions for stored rows: log_prob of `actions` [n] and the entropy under logits [n, >= A] and the stored
        packed masks bits [n, >= W] (action_masks_packed), any n.  The log_prob of an action sample_masked drew under the same mask and
        logits comes back bit for bit.  differentiable=True: the same numbers, and log_prob and entropy carry an autograd graph into
        `logits` (engine.masked_evaluate: the backward pass is one launch of mcbs_masked_categorical_grad); out= cannot be combined
        with it."""
        if differentiable:
            if out is not None:
                raise ValueError("evaluate_masked(differentiable=True) allocates its outputs: out= is not supported")
            return self.engine.masked_evaluate(logits, bits, actions, bad_actions=bad_actions)
        return self.engine.masked_categorical(logits, bits=bits, mode="evaluate", actions=actions, bad_actions=bad_actions, out=out)

    # -- the same head from the policy's latent (mcbs_masked_linear_categorical): action_net's logits are never materialised --
    def sample_masked_from_latent(self, latent, weight, bias, seed: int, step: int, deterministic: bool = False, uniforms=None, out=None):
        """sample_masked for a policy whose action_net is Linear(H, A), from what goes INTO that layer: latent [n_envs, H] (latent_pi),
        weight [A, H] and bias [A] or None (action_net.weight / .bias), float32 or bfloat16 alike.  Only the logits of allowed actions are
        computed, in the kernel; the result is bit for bit sample_masked's on logits holding those values (against F.linear, which sums
        in another order, the stored log_prob agrees to rounding)."""
        return self.engine.masked_linear_categorical(latent, weight, bias, bits=self._live_bits(), mode="argmax" if deterministic else "sample",
                                                     seed=seed, step=step, uniforms=uniforms, out=out)

    def evaluate_masked_from_latent(self, bits, latent, weight, bias, actions, bad_actions=None, out=None, differentiable: bool = False):
        """evaluate_masked from the latent: log_prob of `actions` [n] and the entropy under stored packed masks bits [n, >= W], latent
        [n, H], weight [A, H], bias [A] or None.  The log_prob of an action sample_masked_from_latent drew under the same mask, latent
        and layer comes back bit for bit.  differentiable=True: the same numbers, and log_prob and entropy carry an autograd graph into
        latent, weight and bias (engine.masked_linear_evaluate: the backward pass is one call of mcbs_masked_linear_categorical_grad,
        no [n, A] tensor either way); out= cannot be combined with it."""
        if differentiable:
            if out is not None:
                raise ValueError("evaluate_masked_from_latent(differentiable=True) allocates its outputs: out= is not supported")
            return self.engine.masked_linear_evaluate(latent, weight, bias, bits, actions, bad_actions=bad_actions)
        return self.engine.masked_linear_categorical(latent, weight, bias, bits=bits, mode="evaluate", actions=actions, bad_actions=bad_actions,
                                                     out=out)

    # -- the policy's input features (marlon_amd/features.py, mcbs_encode_features) --
    def _feature_handle(self, include_masks: bool, reference_counts: bool, keys=None):
        key = (bool(include_masks), bool(reference_counts), None if keys is None else tuple(keys))
        h = self._feature_handles.get(key)
        if h is None:
            from .features import FeatureLayout
            h = self._feature_handles[key] = self.engine.feature_layout(FeatureLayout(self.topo, self.spec, keys=keys, include_masks=include_masks,
                                                                                      reference_counts=reference_counts))
        return h

    def feature_layout(self, include_masks: bool = False, reference_counts: bool = False, keys=None):
        """The `features.FeatureLayout` behind features() / encode_features() for these options: `width` sizes a policy's first layer,
        `segments` (key -> (first column, columns)) slices the row."""
        return self._feature_handle(include_masks, reference_counts, keys).layout

    def _pack_bits_from_mask(self, mask):
        """bool [n, A] -> packed int32 [n, row_words] with torch expressions: for batches whose packed mask cannot be rebuilt from the
        observation digest (ExternalRandomEvents).  About exactness, not speed."""
        t = self.torch
        W, row_words = self.engine.packed_mask_words()
        n = mask.shape[0]
        m = t.zeros((n, row_words * 32), dtype=t.int64, device=mask.device)
        m[:, :self.discrete_n] = mask
        words = (m.view(n, row_words, 32) << t.arange(32, dtype=t.int64, device=mask.device)).sum(dim=2)
        return words.to(t.int32)                         # (values up to 2^32 - 1 wrap to the same 32 bits)

    def features(self, out=None, dtype=None, include_masks: bool = False, reference_counts: bool = False, out_of_range=None):
        """The observation this env last returned as the float rows Stable-Baselines3's MultiInputPolicy would build from it
        (every Discrete / MultiDiscrete element one-hot, concatenated in sorted key order; features.FeatureLayout), one launch:
        [n_envs, F] float32 / bfloat16 / float16.  out=: write into a preallocated [n_envs, >= F] tensor, e.g. buffer[t] of a rollout
        buffer; without it a new tensor with rows padded to whole 128-byte lines is allocated and its [:, :F] view returned.
        include_masks: also the three action masks as 0 / 1 columns; the mask is packed first (action_masks_packed), whether or not
        the masks are materialised — under ExternalRandomEvents, where the digest cannot give the mask, the materialised mask is packed
        instead (materialize_masks=False then raises).  reference_counts / out_of_range: see FeatureLayout / engine.encode_features."""
        bits = None
        if include_masks:
            bits = self._live_bits("features(include_masks=True)")
            if bits is None:
                if self._feature_bits is None:
                    self._feature_bits = self.torch.zeros((self.num_envs, self.engine.packed_mask_words()[1]), dtype=self.torch.int32,
                                                          device=self.engine.device)
                bits = self.action_masks_packed(out=self._feature_bits)
        if self._packed_mode:                               # the same bits from the rows the step wrote (mcbs_encode_features_packed)
            return self.engine.encode_features_packed(self._feature_handle(include_masks, reference_counts), self._packing_handle(),
                                                      self.packed_observation, bits=bits, out=out, dtype=dtype, out_of_range=out_of_range)
        return self.engine.encode_features(self._feature_handle(include_masks, reference_counts), self._obs, bits=bits, out=out, dtype=dtype,
                                           out_of_range=out_of_range)

    def encode_features(self, obs, bits=None, out=None, dtype=None, reference_counts: bool = False, out_of_range=None):
        """features() for any n stored observation rows (a shuffled minibatch gathered from a rollout buffer): obs holds the int32
        fields `scalars` [n, 7] (or the seven named counts [n]), `leaked_credentials`, `credential_cache_matrix`,
        `discovered_nodes_properties`, `nodes_privilegelevel` with a leading row axis; bits = the rows' packed masks [n, >= W]
        (action_masks_packed) adds the mask columns."""
        return self.engine.encode_features(self._feature_handle(bits is not None, reference_counts), self._stored_fields(obs), bits=bits, out=out,
                                           dtype=dtype, out_of_range=out_of_range)

    def _stored_fields(self, obs) -> Dict[str, object]:
        """Stored observation rows as the contiguous int32 fields the engine reads: `scalars` stacked from the seven named counts where
        it is not there itself."""
        t = self.torch
        if "scalars" not in obs:
            obs = dict(obs, scalars=t.stack([obs[k] for k in SCALAR_KEYS], dim=1).to(t.int32))
        return {k: obs[k].contiguous() for k in FLAT_FIELDS[:5] if k in obs}

    # -- packed observations (features.ObservationPacking, mcbs_pack_observation): store per step, encode features later --
    def _packing_handle(self):
        if self._obs_packing is None:
            from .features import ObservationPacking
            self._obs_packing = self.engine.observation_packing(ObservationPacking(self.topo, self.spec))
        return self._obs_packing

    def observation_packing(self):
        """The `features.ObservationPacking` behind observation_packed(): `words` is the row width W_obs, `pack_host` / `unpack_host`
        the same format on the host."""
        return self._packing_handle().packing

    def observation_packed(self, out=None, out_of_range=None):
        """The observation this env last returned as bit fields: device int32 [n_envs, W_obs], one launch — 72 B instead of 924 B per
        Chain-10 row.  out=: write straight into a preallocated [n_envs, >= W_obs] buffer, e.g.
        `buf.observations["packed"][buf.pos]` of rollout_buffer(pack_observations=True).  A value outside its valid codes is stored as
        its out-of-range code (and counted into out_of_range), which encodes to the same all-zero group.
        observation_format="packed": the step has written the rows already — without out= they are returned as they are
        (`packed_observation`, the wrapper's persistent tensor), with out= they are copied; nothing is packed, out_of_range is not
        counted (encode_features_packed counts at use)."""
        if self._packed_mode:
            if out is None:
                return self.packed_observation
            self.engine._packed_obs_rows(out, self._packing_handle(), "out", self.num_envs)
            out[:, :self.packed_observation.shape[1]].copy_(self.packed_observation)
            return out
        return self.engine.pack_observation(self._packing_handle(), self.observation_fields, out=out, out_of_range=out_of_range)

    def unpack_observation(self, packed, index=None):
        """Packed rows [m, >= W_obs] -> the five int32 fields (`observation_fields`' keys and shapes) of those rows, or of rows
        index[i] with index (device int64 [n])."""
        return self.engine.unpack_observation(self._packing_handle(), packed, index=index)

    def encode_features_packed(self, packed, bits=None, index=None, out=None, dtype=None, reference_counts: bool = False, out_of_range=None):
        """encode_features() straight from stored packed rows [m, >= W_obs] (bits: their packed masks [m, >= W], adds the mask
        columns).  With index (device int64 [n]) the rows are read where they are stored, no int32 field and no mask row is gathered:
            x = venv.encode_features_packed(buf.observations["packed"].view(T * E, -1), bits=buf.mask_bits.view(T * E, -1),
                                            index=batch.index, dtype=torch.bfloat16)"""
        return self.engine.encode_features_packed(self._feature_handle(bits is not None, reference_counts), self._packing_handle(), packed,
                                                  bits=bits, index=index, out=out, dtype=dtype, out_of_range=out_of_range)

    # -- the policy's first layer straight from the observation (mcbs_first_layer): no feature rows --
    def _first_layer_call(self, reference_counts: bool, weight, bias, source: dict, out, dtype, out_of_range, weight_t, differentiable: bool):
        handle = self._feature_handle(False, reference_counts)
        if differentiable:
            if out is not None:
                raise ValueError("differentiable=True allocates its output: out= is not supported")
            return self.engine.first_layer_evaluate(handle, weight, bias, dtype=dtype, out_of_range=out_of_range, weight_t=weight_t, **source)
        if weight_t is None:
            weight_t = weight.detach().t().contiguous()
        return self.engine.first_layer(handle, weight_t, None if bias is None else bias.detach(), out=out, dtype=dtype, out_of_range=out_of_range,
                                       **source)

    def first_layer(self, weight, bias=None, out=None, dtype=None, reference_counts: bool = False, out_of_range=None, weight_t=None):
        """torch.nn.functional.linear(features(), weight, bias) of the observation this env last returned, without the [n_envs, F]
        feature rows: one launch that adds, per env, the weight column each one-hot element selects to the bias ([n_envs, H] float32 or
        bfloat16; engine.first_layer has the order of the sum).  weight [H, F] / bias [H]: torch's Linear parameters, float32 or
        bfloat16 (F = feature_layout(reference_counts=...).width; the masks are not part of this layer's input).  weight_t=: the
        transposed copy `weight.t().contiguous()` a rollout loop makes once per update instead of once per call.  To serve SB3's
        policy_net[0] and value_net[0] with one call, concatenate their weights into one [2H, F] (and their biases into [2H])."""
        if self._packed_mode:                               # the same bits from the rows the step wrote (mcbs_first_layer_packed)
            source = dict(packing=self._packing_handle(), packed=self.packed_observation, index=None)
        else:
            source = dict(obs=self.observation_fields)
        return self._first_layer_call(reference_counts, weight, bias, source, out, dtype, out_of_range, weight_t, False)

    def encode_first_layer(self, obs, weight, bias=None, out=None, dtype=None, reference_counts: bool = False, out_of_range=None, weight_t=None,
                           differentiable: bool = False):
        """first_layer() for any n stored observation rows: obs as encode_features() takes it (`scalars` [n, 7] or the seven named counts,
        and the four array fields).  differentiable=True: the result carries an autograd graph into weight and bias whose backward is
        one call of engine.first_layer_grad (no feature tensor is kept alive for it)."""
        return self._first_layer_call(reference_counts, weight, bias, dict(obs=self._stored_fields(obs)), out, dtype, out_of_range, weight_t,
                                      differentiable)

    def encode_first_layer_packed(self, packed, weight, bias=None, index=None, out=None, dtype=None, reference_counts: bool = False,
                                  out_of_range=None, weight_t=None, differentiable: bool = False):
        """first_layer() straight from stored packed rows [m, >= W_obs]; with index (device int64 [n]) the rows are read where they are
        stored, as encode_features_packed reads them:
            h = venv.encode_first_layer_packed(buf.observations["packed"].view(T * E, -1), lin.weight, lin.bias, index=batch.index,
                                               differentiable=True)"""
        source = dict(packing=self._packing_handle(), packed=packed, index=index)
        return self._first_layer_call(reference_counts, weight, bias, source, out, dtype, out_of_range, weight_t, differentiable)

    # -- the rollout buffer (marlon_amd/rollout.py, mcbs_gae) --
    @property
    def observation_fields(self) -> Dict[str, object]:
        """The observation this env last returned as the five int32 fields the engine writes (`scalars` [E, 7] unsplit, the others in
        their own shapes): what encode_features() accepts and what rollout_buffer() stores; the wrapper's persistent tensors, not copies."""
        if self._packed_mode:
            raise RuntimeError("this AttackerVecEnv was created with observation_format='packed' and keeps no int32 field: "
                               "unpack_observation(venv.packed_observation) rebuilds them from the packed rows")
        return {k: self._obs[k] for k in FLAT_FIELDS[:5]}

    def rollout_buffer(self, n_steps: int, gamma: float = 0.99, gae_lambda: float = 0.95, store_observations: bool = True,
                       pack_observations: Optional[bool] = None, mask_storage: str = "bits"):
        """A `rollout.DeviceRolloutBuffer` of n_steps x n_envs transitions for this env: it stores the int32 observation fields
        encode_features() accepts (not the mask fields — with discrete=True the packed masks of action_masks_packed() are stored
        instead, `mask_bits`), actions of this wrapper's shape, and computes advantages and returns with one launch.  Its add() takes
        `observation_fields` as obs.
        mask_storage="keys" (discrete=True): the buffer holds `mask_keys` [T, E, Wk] instead of `mask_bits` — fill row `pos` with
        action_mask_keys(out=buf.mask_keys[buf.pos]) or pass keys= to add() — and get() expands each minibatch's `mask_bits` from them
        (Chain-10 at 12/12: 20 B instead of 1 772 B per transition).
        store_observations=False: no observation storage (a trainer that keeps feature rows of its own).
        pack_observations=True: the observation storage is ONE key, `observations["packed"]` int32 [T, E, W_obs], instead of the five
        fields: fill row `pos` with observation_packed(out=buf.observations["packed"][buf.pos]) and pass obs=None to add(); at update
        time encode_features_packed(..., index=batch.index) reads the storage itself.  The default is False, and True for a wrapper
        created with observation_format="packed", which has nothing else to store: False is refused there."""
        from .rollout import DeviceRolloutBuffer
        obs = _observation_storage(self, store_observations, pack_observations, lambda: self.observation_fields, lambda: self._packing_handle().words,
                                   "AttackerVecEnv", "int32")
        if mask_storage not in ("bits", "keys"):
            raise ValueError(f"mask_storage must be 'bits' or 'keys', got {mask_storage!r}")
        keys = self.discrete and mask_storage == "keys"
        return DeviceRolloutBuffer(self.engine, n_steps, self.num_envs, obs=obs, action_shape=self._action_shape[1:],
                                   mask_words=self.engine.packed_mask_words()[1] if self.discrete else None, gamma=gamma, gae_lambda=gae_lambda,
                                   mask_key_words=self.engine.mask_key_words() if keys else None)

    # -- VecEnv surface --
    def reset(self):
        self.engine.reset()
        if self._packed_mode:
            # two launches into a transient int32 scratch (the library needs the reset observation's digest anyway), dropped afterwards
            scratch = self.engine.observe(self.engine.alloc_obs(FLAT_FIELDS[:5]))
            self.engine.pack_observation(self._packing_handle(), scratch, out=self.packed_observation)
            del scratch
            if self._packed_fresh is None:
                self._packed_fresh = self.packed_observation[0:1].clone()
        else:
            self.engine.observe(self._obs)
            if self._reset_rows is None:
                self._reset_rows = {k: v[0:1].clone() for k, v in self._obs.items()}
        self.timesteps.zero_()
        self.valid_action_count.zero_()
        self.invalid_action_count.zero_()
        self.episode_returns.zero_()
        self.has_cyber_reward.zero_()
        return self.observation

    @property
    def action_buffer(self):
        """use_graph: the int64 device tensor the captured step reads its actions from ([E] Discrete, [E, 10] MultiDiscrete).  A policy
        that writes into it and calls `step(venv.action_buffer)` saves the copy."""
        return self._act_in

    def _step_device(self, actions) -> None:
        """Everything a wrapper step does on the device, enqueued on the current stream by ONE call into the library
        (mcbs_attacker_wrapper_step) without any host round trip: decode + interception of out-of-range actions, environment step and
        observation, then — one launch — counters, reward modifier of intercepted actions (attack_wrapper.py:296,354), truncation
        (:350-352), episode returns and what DummyVecEnv.step_wait does for an env that reports done: keep its last observation, reset
        it, return the reset observation (every env resets to the same state, so that is row 0 of reset()'s observation)."""
        a = _as_actions(self, actions, self._action_shape, "expected actions of shape")
        if self._wb is None:                               # (use_graph: the one persistent set; eager steps install theirs in _next_output_set)
            self._wb = self._wrapper_buffers(self._persistent_set())
        # the library call with every argument block bound once per (output set, wrapper settings): engine.wrapper_step_call
        key = (id(self._wb), self.invalid_action_reward_modifier, self.max_timesteps, self.auto_reset)
        call = self._calls.get(key)
        if call is None:
            settings = (self._wb,) + key[1:]
            if self._packed_mode:
                call = self.engine.wrapper_step_packed_call(self.discrete, self._rows, self._packing_handle(), self.packed_observation,
                                                            self.terminal_packed_observation, self._packed_fresh, *settings)
            else:
                obs_block, keep, fresh = self._blocks()
                call = self.engine.wrapper_step_call(self.discrete, self._rows, obs_block, *settings, keep, fresh)
            self._calls[key] = call
        call(a.data_ptr())

    def _blocks(self):
        """-> (ObsBuffers of the observation, RowCopies observation -> terminal observation, RowCopies reset row -> observation): the
        argument blocks of the fields form's calls (engine.wrapper_step_call and the two-agent calls), built on first use."""
        if self._keep is None:
            eng = self.engine
            self._keep = eng.row_copies([(self._obs[k], self._terminal[k]) for k in self._obs])
            self._fresh = eng.row_copies([(self._reset_rows[k], self._obs[k]) for k in self._obs], one_row_src=True)
            self._obs_block = eng.obs_struct(self._obs)
        return self._obs_block, self._keep, self._fresh

    def _persistent_set(self) -> Dict[str, object]:
        """The wrapper's own output tensors under the names of _ATTACKER_OUTPUTS: what a use_graph step writes, every step."""
        return dict(invalid=self._invalid, executed=self._executed, rewards=self._rewards, truncated=self._truncated, ret=self._ret_out,
                    length=self._len_out, terminated=self.engine.terminated)

    def _wrapper_buffers(self, o):
        from ._abi import WrapperBuffers
        return WrapperBuffers(*[x.data_ptr() for x in (
            o["invalid"], self.engine.reward, o["terminated"], self.timesteps, self.valid_action_count, self.invalid_action_count, self.episode_returns,
            self.last_cyber_reward, self.has_cyber_reward, o["rewards"], o["truncated"], self._dones, o["ret"], o["length"], self._n_done, o["executed"])])

    def _info(self, o) -> Dict[str, object]:
        """A step's info dict over the output set o."""
        return {"invalid_action": o["invalid"].view(self.torch.bool), "cyber_step_executed": o["executed"],
                "network_availability": self.engine.info["network_availability"], "step_count": self.engine.info["step_count"],
                "episode_return": o["ret"], "episode_length": o["length"]}

    def step(self, actions):
        """-> (observation dict, rewards f32 [E], terminated u8 [E], truncated u8 [E], info dict of tensors)."""
        t = self.torch
        if self.use_graph:
            if actions is not self._act_in:                    # a policy may write its actions straight into `action_buffer`: no copy then
                _stage_actions(self, actions)
            if self._one_launch is None:
                self._one_launch = self.engine.wrapper_step_launches(self.materialize_masks) == 1
            if self._one_launch:
                # the whole step is ONE kernel: launched directly on the persistent buffers (a one-node hipGraph replay costs the device
                # ~8 us more than the launch it wraps: 30 vs 20 us per step at 65 536 Chain-10 envs)
                self._step_device(self._act_in)
            elif self._graph is None:
                self._step_device(self._act_in)            # this step runs eagerly (it also creates the argument blocks) ...
                t.cuda.synchronize(self.engine.device)
                g = t.cuda.CUDAGraph()
                side = t.cuda.Stream(device=self.engine.device)
                side.wait_stream(t.cuda.current_stream(self.engine.device))
                with t.cuda.stream(side):
                    with t.cuda.graph(g, stream=side):
                        self._step_device(self._act_in)
                t.cuda.current_stream(self.engine.device).wait_stream(side)
                self._graph = g
                # ... and is then captured for the steps to come (capturing executes nothing)
            else:
                self._graph.replay()
            if self._graph_out is None:                        # the same persistent buffers every step: built once
                self._graph_out = (self.observation, self._rewards, self.engine.terminated, self._truncated, self._info(self._persistent_set()))
            return self._graph_out
        o, _, info = self._next_output_set()
        self._step_device(actions)
        return self.observation, o["rewards"], o["terminated"], o["truncated"], dict(info)

    def _next_output_set(self):
        """eager: the step's outputs alternate between TWO sets of tensors allocated once (a step's outputs stay valid until the step after
        next; consumers that keep them longer clone them).  Seven allocations and a rebuilt argument block per step cost more host time
        than the device needs for the whole wrapper step (20 us at 65 536 envs).  -> (tensors, WrapperBuffers, info) of the set the
        coming step writes, installed as the wrapper's current outputs."""
        if self._ring is None:
            sets = [_output_set(self, _ATTACKER_OUTPUTS) for _ in range(2)]
            self._ring = [(o, self._wrapper_buffers(o), self._info(o)) for o in sets]
        self._slot ^= 1
        o, wb, info = self._ring[self._slot]
        self._invalid, self._executed, self._rewards, self._truncated = o["invalid"], o["executed"], o["rewards"], o["truncated"]
        self._ret_out, self._len_out, self._terminated_out, self._wb = o["ret"], o["length"], o["terminated"], wb
        return o, wb, info

    def close(self) -> None:
        self.engine.close()


class DefenderVecEnv(_MultiDiscreteHead):
    """`DefenderEnvWrapper` + `LearningDefender` (marlon/baseline_models/env_wrappers/defend_wrapper.py,
    marlon/defender_agents/defender.py) for the batch an `AttackerVecEnv(..., learned_defender=True)` owns: the two
    wrappers share one environment batch, as in MultiAgentUniverse.build (multiagent_universe.py:160-199).

    step(actions[E,12]) = validity check + executeAction AND the wrapper's reward shaping in one launch, then the observation
    (`mcbs_defender_wrapper_step`).  The shaping (defend_wrapper.py:228-282): invalid-action penalty, minus the attacker's last environment reward, a one-time
    `loss_reward` when availability first drops below `maintain_sla` (terminating if reset_on_constraint_broken), a
    worsening penalty while breached, `winning_reward` on eviction; truncation at max_timesteps.
    The learned defender always acts on the live environment.

    observation_format="packed": the wrapper keeps no int8 field.  Its observation is `{"packed": rows}`, `packed_observation` int32
    [n_envs, W_def]: one bit per MultiBinary element in features()' column order (features.DefenderObservationPacking; ToyCtf: 20 B
    instead of 143 B per row), written by the step itself (`mcbs_defender_wrapper_step_packed`: the turn launch writes the rows on
    topologies of up to 32 nodes, a second launch elsewhere).  features(), rollout_buffer() and encode_features_packed() read the
    rows; unpack_observation() rebuilds the int8 fields.  TwoAgentTrainVecEnv takes such a wrapper together with an AttackerVecEnv of
    observation_format="packed"; the joint turn (TwoAgentVecEnv) writes the dense form only and refuses it."""

    def __init__(self, attacker: AttackerVecEnv, max_timesteps: int = 100, invalid_action_reward: float = 0.0,
                 reset_on_constraint_broken: bool = True, loss_reward: float = -5000.0, sla_worsening_penalty_scale: float = 200.0,
                 use_graph: bool = False, observation_format: str = "dense"):
        if observation_format not in ("dense", "packed"):
            raise ValueError(f"observation_format must be 'dense' or 'packed', got {observation_format!r}")
        self.observation_format = observation_format
        self._packed_mode = observation_format == "packed"
        self._packing = None
        self.attacker = attacker
        self.engine = attacker.engine
        t = self.torch = attacker.torch
        E, dev = attacker.num_envs, self.engine.device
        self.num_envs = E
        self.max_timesteps = int(max_timesteps)
        self.invalid_action_penalty = float(invalid_action_reward)
        self.reset_on_constraint_broken = bool(reset_on_constraint_broken)
        self.loss_reward = float(loss_reward)
        self.sla_worsening_penalty_scale = float(sla_worsening_penalty_scale)
        self.maintain_sla = float(attacker.spec.maintain_sla)
        self.winning_reward = float(attacker.spec.winning_reward)
        N = attacker.topo.n_nodes
        self.nvec = np.array([5, N, N, 6, 2, N, 6, 2, N, 3, N, 3], dtype=np.int64)          # defend_wrapper.py:162-195
        self._nvec = tuple(int(v) for v in self.nvec)
        self._sizes = self.engine._defender_field_sizes()
        if self._packed_mode:
            self.packed_observation = t.zeros((E, self.engine.defender_obs_words()), dtype=t.int32, device=dev)
            self._obs = {"packed": self.packed_observation}
        else:
            self._obs = self.engine.alloc_defender_obs()
        self.timesteps = t.zeros(E, dtype=t.int32, device=dev)
        self.has_breached_sla = t.zeros(E, dtype=t.bool, device=dev)
        self.prev_availability = t.ones(E, dtype=t.float64, device=dev)
        self.valid_action_count = t.zeros(E, dtype=t.int64, device=dev)
        self.invalid_action_count = t.zeros(E, dtype=t.int64, device=dev)
        self._evicted = None
        self._ring, self._slot = None, 0
        # use_graph: outputs are the wrapper's own persistent buffers (overwritten by the next step) and the actions are copied into a
        # persistent buffer; the turn's two launches are issued directly (see step)
        self.use_graph = bool(use_graph)
        self._act_in = t.zeros((E, 12), dtype=t.int64, device=dev)
        self.reset()

    @property
    def observation(self) -> Dict[str, object]:
        return self._obs

    # -- the policy's input features and the rollout buffer --
    FEATURE_KEYS = ("incoming_firewall_status", "infected_nodes", "outgoing_firewall_status", "services_status")      # sorted key order

    @property
    def feature_width(self) -> int:
        """Columns of a features() row: the four MultiBinary fields' sizes added up."""
        return sum(self._sizes[k] for k in self.FEATURE_KEYS)

    def features(self, out=None, dtype=None):
        """The observation this env last returned as the float rows Stable-Baselines3's MultiInputPolicy would build from it
        (preprocess_obs + CombinedExtractor): the four int8 MultiBinary fields as 0.0 / 1.0, flattened and concatenated in sorted key
        order (FEATURE_KEYS) -> [n_envs, feature_width] float32 (or `dtype`).  out=: write into a preallocated [n_envs, >= feature_width]
        tensor, e.g. buffer[t] of a rollout buffer; columns beyond feature_width are left alone.  float32, bfloat16 and float16 rows are
        ONE launch (mcbs_encode_defender_features), from the int8 fields or, with observation_format="packed", from the packed rows;
        any other floating dtype takes four converting `copy_`s from the int8 fields (refused in packed mode)."""
        t = self.torch
        E, F = self.num_envs, self.feature_width
        want = out.dtype if isinstance(out, t.Tensor) else (dtype if dtype is not None else t.float32)
        kernel = want in (t.float32, t.bfloat16, t.float16)
        if self._packed_mode and not kernel:
            raise ValueError(f"features(): {want} rows are built from the int8 fields, which a DefenderVecEnv with observation_format='packed' "
                             "does not keep (float32, bfloat16 and float16 are encoded from the packed rows)")
        if out is None:
            if kernel:
                return self.engine.encode_defender_features(**self._feature_source(), dtype=want)
            out = t.empty((E, F), dtype=want, device=self.engine.device)
        elif (not isinstance(out, t.Tensor) or out.dim() != 2 or out.shape[0] != E or out.shape[1] < F or not out.is_floating_point()
              or out.device != self.engine.device or (dtype is not None and out.dtype != dtype)):
            raise ValueError(f"out must be a floating-point device tensor [{E}, >= {F}]" + (f" of {dtype}" if dtype is not None else ""))
        if kernel and out.stride(1) == 1:
            return self.engine.encode_defender_features(**self._feature_source(), out=out)
        if self._packed_mode:
            raise ValueError("features(out=): the rows of out must be contiguous")
        c = 0
        for k in self.FEATURE_KEYS:
            x = self._obs[k].reshape(E, -1)
            out[:, c:c + x.shape[1]].copy_(x)
            c += x.shape[1]
        return out[:, :F]

    def _feature_source(self) -> dict:
        return dict(packed=self.packed_observation) if self._packed_mode else dict(dense=self._obs)

    # -- packed observations (features.DefenderObservationPacking): store 20 B per ToyCtf step, encode features later --
    def observation_packing(self):
        """The `features.DefenderObservationPacking` of this topology: `words` is the row width W_def, `fields` the four (offset, size)
        pairs, `pack_host` / `unpack_host` the same format on the host."""
        if self._packing is None:
            from .features import DefenderObservationPacking
            self._packing = DefenderObservationPacking(self.attacker.topo)
        return self._packing

    def observation_packed(self, out=None):
        """The observation this env last returned as packed rows: device int32 [n_envs, W_def].  Dense mode: one pack launch.  Packed
        mode: the step has written them — without out= the wrapper's persistent `packed_observation` is returned, with out= it is copied.
        out=: a preallocated [n_envs, >= W_def] buffer, e.g. `buf.observations["packed"][buf.pos]` of rollout_buffer(pack_observations=True);
        words from W_def on are not touched."""
        if self._packed_mode:
            if out is None:
                return self.packed_observation
            self.engine._defender_packed_rows(out, "out", self.num_envs)
            out[:, :self.packed_observation.shape[1]].copy_(self.packed_observation)
            return out
        return self.engine.pack_defender_observation(self._obs, out=out)

    def unpack_observation(self, packed, index=None):
        """Packed rows [m, >= W_def] -> the four int8 fields (0 / 1) of those rows, or of rows index[i] with index (device int64 [n])."""
        return self.engine.unpack_defender_observation(packed, index=index)

    def encode_features_packed(self, packed, index=None, out=None, dtype=None, bad_rows=None):
        """features() rows straight from stored packed rows [m, >= W_def], one launch.  With index (device int64 [n]) the rows are read
        where they are stored, nothing is gathered first:
            x = dfd.encode_features_packed(buf.observations["packed"].view(T * E, -1), index=batch.index, dtype=torch.bfloat16)
        An index outside [0, m) gives an all-zero row and adds one to bad_rows (optional device int32 [1])."""
        return self.engine.encode_defender_features(packed=packed, index=index, out=out, dtype=dtype, bad_rows=bad_rows)

    def rollout_buffer(self, n_steps: int, gamma: float = 0.99, gae_lambda: float = 0.95, store_observations: bool = True,
                       pack_observations: Optional[bool] = None):
        """A `rollout.DeviceRolloutBuffer` of n_steps x n_envs transitions for the defender: it stores the four int8 observation fields,
        actions [12] and no packed masks (a MultiDiscrete head has none), and computes advantages and returns with one launch.  Its add()
        takes `observation` as obs.  store_observations=False: no observation storage (a trainer that keeps features() rows of its own).
        pack_observations=True: the observation storage is ONE key, `observations["packed"]` int32 [T, E, W_def]: fill row `pos` with
        observation_packed(out=buf.observations["packed"][buf.pos]) and pass obs=None to add(); at update time
        encode_features_packed(..., index=batch.index) reads the storage itself.  The default is False, and True for a wrapper created
        with observation_format="packed", which has nothing else to store: False is refused there."""
        from .rollout import DeviceRolloutBuffer
        obs = _observation_storage(self, store_observations, pack_observations, lambda: self._obs, self.engine.defender_obs_words,
                                   "DefenderVecEnv", "int8")
        return DeviceRolloutBuffer(self.engine, n_steps, self.num_envs, obs=obs, action_shape=(12,), mask_words=None, gamma=gamma,
                                   gae_lambda=gae_lambda)

    def reset(self, env_mask=None):
        """Wrapper state of the envs in env_mask (all if None); the environment itself is reset by the attacker side."""
        t = self.torch
        if self._packed_mode:
            self.engine.defender_observe_packed(out=self.packed_observation)
        else:
            self.engine.defender_observe(self._obs)
        avail = self.engine.step_info()["network_availability"]
        keep = t.zeros(self.num_envs, dtype=t.bool, device=self.engine.device) if env_mask is None else ~(env_mask != 0)
        self.timesteps *= keep
        self.valid_action_count *= keep
        self.invalid_action_count *= keep
        self.has_breached_sla &= keep
        self.prev_availability.copy_(t.where(keep, self.prev_availability, avail))    # in place: the fused shaping launch holds its address
        return self._obs

    def step(self, actions):
        """-> (observation dict, reward f64 [E], terminated u8 [E], truncated u8 [E], info)."""
        if self.use_graph:
            # (persistent outputs, actions copied into a persistent buffer — what a captured turn offered; the turn itself is two
            # launches issued directly: replaying them from a hipGraph cost the device more than the launches it wraps, 23 vs 12 us
            # per turn at 16 384 ToyCtf envs)
            actions = _stage_actions(self, actions)
        # eager: ONE library call per turn (mcbs_defender_wrapper_step: the turn and the reward shaping in one launch, then the observation)
        o, _, info, call = self._next_output_set()
        call(_as_actions(self.attacker, actions, (self.num_envs, 12), "defender actions must have shape").data_ptr())
        return self._obs, o["reward"], o["terminated"], o["truncated"], dict(info)

    def _next_output_set(self):
        """-> (tensors, DefenderWrapperBuffers, info, bound library call) of the set the coming turn writes: the two sets of _output_ring
        in turn (a turn's outputs stay valid until the turn after next); under use_graph the first one, every turn."""
        if self._ring is None:
            self._output_ring()
        if not self.use_graph:
            self._slot ^= 1
        return self._ring[self._slot]

    def _output_ring(self) -> None:
        """The turn's outputs alternate between two sets of tensors allocated once (valid until the turn after next): per set the tensors,
        the DefenderWrapperBuffers block, the info dict and the bound library call."""
        t = self.torch
        E, dev = self.num_envs, self.engine.device
        from ._abi import DefenderObs, DefenderWrapperBuffers, DefenderWrapperCfg
        self._evicted = t.zeros(E, dtype=t.uint8, device=dev)
        self._obs_block = None if self._packed_mode else DefenderObs(**{k: x.data_ptr() for k, x in self._obs.items()})
        self._wc = DefenderWrapperCfg(self.invalid_action_penalty, self.loss_reward, self.sla_worsening_penalty_scale, self.maintain_sla,
                                      self.winning_reward, int(self.reset_on_constraint_broken), self.max_timesteps)
        self._ring = []
        for _ in range(2):
            o = _output_set(self, _DEFENDER_OUTPUTS)
            wb = DefenderWrapperBuffers(*[x.data_ptr() for x in (
                o["valid"], o["availability"], self._evicted, self.attacker.has_cyber_reward, self.attacker.last_cyber_reward, self.timesteps,
                self.valid_action_count, self.invalid_action_count, self.has_breached_sla, self.prev_availability, o["reward"], o["terminated"],
                o["truncated"], o["breached"], o["won"])])
            info = {"valid_action": o["valid"].view(t.bool), "network_availability": o["availability"], "sla_breached": o["breached"].view(t.bool),
                    "defender_won": o["won"].view(t.bool)}
            call = (self.engine.defender_wrapper_step_packed_call(self.packed_observation, wb, self._wc) if self._packed_mode
                    else self.engine.defender_wrapper_step_call(self._obs_block, wb, self._wc))
            self._ring.append((o, wb, info, call))


class EpisodeState:
    """The six arrays of mcbs_episode_buffers (marl_algorithm.run_episode's per-env bookkeeping) as device tensors: `alive`,
    `attacker_done`, `defender_done` uint8 [E], `lengths` int64 [E], and the turn's two reward rows `attacker_reward` / `defender_reward`
    float64 [E] — its own by default; a driver that keeps traces points them at the turn's rows of its storage (TwoAgentVecEnv.step)."""

    def __init__(self, torch, n_envs: int, device):
        t = torch
        self.alive = t.ones(n_envs, dtype=t.uint8, device=device)
        self.lengths = t.zeros(n_envs, dtype=t.int64, device=device)
        self.attacker_done = t.zeros(n_envs, dtype=t.uint8, device=device)
        self.defender_done = t.zeros(n_envs, dtype=t.uint8, device=device)
        self.attacker_reward = t.zeros(n_envs, dtype=t.float64, device=device)
        self.defender_reward = t.zeros(n_envs, dtype=t.float64, device=device)
        self._block = None

    def tensors(self) -> Dict[str, object]:
        from ._abi import EPISODE_FIELDS
        return {k: getattr(self, k) for k in EPISODE_FIELDS}

    def block(self, attacker_row=None, defender_row=None):
        """The _abi.EpisodeBuffers argument block, built once; the two reward members follow the rows given for this turn."""
        from ._abi import EPISODE_FIELDS, episode_buffers
        if self._block is None:
            self._block = episode_buffers(**{k: x.data_ptr() for k, x in self.tensors().items()})
        a = self.attacker_reward if attacker_row is None else attacker_row
        d = self.defender_reward if defender_row is None else defender_row
        for x in (a, d):
            if x.dtype != self.attacker_reward.dtype or x.shape != self.attacker_reward.shape or not x.is_contiguous() or x.device != self.alive.device:
                raise ValueError("a reward row is a contiguous float64 device tensor [n_envs]")
        self._block[EPISODE_FIELDS.index("attacker_reward")] = a.data_ptr()
        self._block[EPISODE_FIELDS.index("defender_reward")] = d.data_ptr()
        self._rows = (a, d)                                # (kept alive while the block names them)
        return self._block


class TwoAgentVecEnv:
    """Both wrappers' steps of one joint turn — `att.step(attacker_actions)`, then `dfd.step(defender_actions)` with run_episode's parking
    of finished envs — and the episode bookkeeping in ONE launch (mcbs_two_agent_step, marlon_amd/csrc/mcbs_two_agent.hip).

    `att` must be `AttackerVecEnv(..., learned_defender=True, auto_reset=False, materialize_masks=False)` on a small topology (the batch's
    wrapper step is one launch) and `dfd` the `DefenderVecEnv` on it; anything else is a ValueError (`supported(att)` asks first).  The
    joint step writes into the two wrappers' own persistent state — counters, `att.observation`, `dfd.observation`, the alternating
    output sets — so everything that reads it (`att.mask_logits`, `att.features()`, `dfd.features()`, `sample_masked*`, ...) works as
    after the separate steps, and separate and joint steps may be mixed.

    The defender's action of a turn is chosen BEFORE the attacker's step of that turn, from the observation the defender's own previous
    step returned: the reference's data flow (marl_algorithm.py:222-225)."""

    def __init__(self, att: AttackerVecEnv, dfd: "DefenderVecEnv"):
        why = self._refusal(att, dfd)
        if why:
            raise ValueError(f"TwoAgentVecEnv: {why}")
        self.att, self.dfd = att, dfd
        self.engine, self.torch, self.num_envs = att.engine, att.torch, att.num_envs
        self._calls = {}

    @staticmethod
    def _refusal(att, dfd=None) -> Optional[str]:
        return _two_agent_refusal(att, dfd, "joint", auto_reset=False, auto_reset_why="the episode boundary belongs to the caller",
                                  launches="two_agent_step_launches")

    @staticmethod
    def supported(att) -> bool:
        """Whether TwoAgentVecEnv(att, DefenderVecEnv(att)) would be accepted."""
        return TwoAgentVecEnv._refusal(att) is None

    def episode_state(self) -> EpisodeState:
        """Freshly allocated episode bookkeeping: every env alive, nothing counted."""
        return EpisodeState(self.torch, self.num_envs, self.engine.device)

    def step(self, attacker_actions, defender_actions, episode: Optional[EpisodeState] = None, reward_rows=None):
        """-> ((obs, rewards, terminated, truncated, info), (dobs, dreward, dterminated, dtruncated, dinfo)): exactly the tuples
        `att.step(attacker_actions)` and `dfd.step(defender_actions)` return.  The defender's turn of an env whose episode is over — `episode.alive`
        is 0, or the attacker's step has just ended it — is parked (kind -2), whatever `defender_actions` says; the array is not modified.
        `episode`: an episode_state() to book the turn into (mcbs.h states the rules); `reward_rows` = (attacker row, defender row), float64
        [E] device tensors that receive the turn's two trace rows instead of `episode.attacker_reward` / `.defender_reward`."""
        att, dfd = self.att, self.dfd
        a = _as_actions(att, attacker_actions, att._action_shape, "attacker actions must have shape")
        d = _as_actions(att, defender_actions, (self.num_envs, 12), "defender actions must have shape")
        if reward_rows is not None and episode is None:
            raise ValueError("reward_rows go with an episode state")
        block = episode.block(*(reward_rows or ())) if episode is not None else None
        o, wb, info = att._next_output_set()
        do, dwb, dinfo, _ = dfd._next_output_set()
        key = (id(wb), id(dwb), att.invalid_action_reward_modifier, att.max_timesteps)
        call = self._calls.get(key)
        if call is None:
            call = self._calls[key] = self.engine.two_agent_step_call(att.discrete, att._rows, att._blocks()[0], wb, att.invalid_action_reward_modifier,
                                                                      att.max_timesteps, dfd._obs_block, dwb, dfd._wc)
        call(a.data_ptr(), d.data_ptr(), block)
        return ((att.observation, o["rewards"], o["terminated"], o["truncated"], dict(info)),
                (dfd._obs, do["reward"], do["terminated"], do["truncated"], dict(dinfo)))


class TwoAgentTrainVecEnv:
    """One TRAINING turn of both agents in ONE launch (mcbs_two_agent_train_step, marlon_amd/csrc/mcbs_two_agent.hip): what
    `marl_algorithm.collect_rollouts` does per turn — `attacker.perform_step`, then `defender.perform_step`, each through its own
    DummyVecEnv, which resets its wrapper as soon as it reports done — for a whole batch.  The two wrappers share one environment, so a
    reset on one side reaches the other (reset_request: attack_wrapper.py:433-435, defend_wrapper.py:269-271, 446-447; include/mcbs.h
    states the rules):

      * the attacker ends (goal, its own timeout, or a request): its env is re-initialised, it gets a fresh observation, and — unless it
        had been asked — the defender's step of the same turn returns `-1 * the attacker's last reward`, truncated, and is reset too;
      * the defender ends on its own (SLA breach, eviction, its timeout): the env is re-initialised, the defender gets a fresh
        observation, and `attacker_reset_request` is raised: the attacker's NEXT step is truncated, whatever it does.  Until then the
        attacker keeps the observation — and the action mask — of the episode that is gone, as in the reference.

    `att` must be `AttackerVecEnv(..., learned_defender=True, auto_reset=True, materialize_masks=False)` on a small topology and `dfd`
    the `DefenderVecEnv` on it; anything else is a ValueError naming the reason (`supported(att)` asks first).  The turn writes into the
    two wrappers' own persistent state, so `att.mask_logits`, `att.features()`, `dfd.features()`, `sample_masked*` ... work as after
    separate steps.  But separate `att.step` / `dfd.step` calls must NOT be mixed with this class's `step`: they know nothing of the
    request byte, of the defender's running return, or of the defender-side reset.

    A pair in which BOTH wrappers were created with observation_format="packed" is taken as well: the same launch then writes both
    observations as packed rows (mcbs_two_agent_train_step_packed) into `att.packed_observation` / `att.terminal_packed_observation` and
    `dfd.packed_observation`, no int32 or int8 field exists, and `terminal_observation` is `{"packed": rows}` like the attacker's.  A
    mixed pair (one side packed, the other not) is refused."""

    def __init__(self, att: AttackerVecEnv, dfd: "DefenderVecEnv"):
        why = self._refusal(att, dfd)
        if why:
            raise ValueError(f"TwoAgentTrainVecEnv: {why}")
        self.att, self.dfd = att, dfd
        self.engine, self.torch, self.num_envs = att.engine, att.torch, att.num_envs
        t, E, dev = self.torch, self.num_envs, self.engine.device
        self._request = t.zeros(E, dtype=t.uint8, device=dev)
        self.defender_returns = t.zeros(E, dtype=t.float64, device=dev)
        self._packed_mode = att._packed_mode                # (both sides: _refusal has refused a mixed pair)
        self._terminal = {k: t.zeros_like(v) for k, v in dfd._obs.items()}      # (packed mode: the one key "packed")
        self._fresh_rows = None
        self._ring, self._slot = None, 0
        self._calls = {}
        self.reset()

    @staticmethod
    def _refusal(att, dfd=None) -> Optional[str]:
        return _two_agent_refusal(att, dfd, "training", auto_reset=True, auto_reset_why="both agents' DummyVecEnv resets are part of the training turn",
                                  launches="two_agent_train_step_launches", packed_launches="two_agent_train_step_packed_launches")

    @staticmethod
    def supported(att) -> bool:
        """Whether TwoAgentTrainVecEnv(att, dfd) would be accepted with the DefenderVecEnv on att of the same observation format:
        DefenderVecEnv(att) for an attacker with observation_format="fields", DefenderVecEnv(att, observation_format="packed") for one with
        observation_format="packed"."""
        return TwoAgentTrainVecEnv._refusal(att) is None

    @property
    def attacker_reset_request(self):
        """bool [E]: the defender reset the shared env on its own last turn, so the attacker's next step is truncated
        (AttackerEnvWrapper.reset_request).  A view of the byte the kernel reads and writes."""
        return self._request.view(self.torch.bool)

    @property
    def terminal_observation(self) -> Dict[str, object]:
        """The defender's observation after its action of the last turn: its episode's last observation for the envs whose defender
        `dones` was set (SB3's infos[e]["terminal_observation"]); rows of other envs mean nothing.  The attacker's is
        `att.terminal_observation`.  A packed pair: `{"packed": int32 [E, W_def]}`."""
        return self._terminal

    def reset(self):
        """Both sides' `env.reset()` of marl_algorithm.setup_learn, and no request pending.  -> (attacker observation, defender observation)"""
        obs = self.att.reset()
        dobs = self.dfd.reset()
        self._request.zero_()
        self.defender_returns.zero_()
        t = self.torch
        # (attacker, defender) dones of the last turn: the next turn's episode_starts (simulate.collect_rollouts carries them here)
        self.last_dones = (t.ones(self.num_envs, dtype=t.uint8, device=self.engine.device), t.ones(self.num_envs, dtype=t.uint8, device=self.engine.device))
        if self._fresh_rows is None:
            self._fresh_rows = {k: v[0:1].clone() for k, v in dobs.items()}     # every env resets to the same state (packed mode:
                                                                                 # dfd.packed_observation[0:1])
        return obs, dobs

    def _output_ring(self) -> None:
        from ._abi import training_buffers, training_packed_buffers
        fixed = dict(attacker_reset_request=self._request.data_ptr(), defender_return=self.defender_returns.data_ptr())
        if self._packed_mode:
            fixed.update(terminal_defender_packed=self._terminal["packed"].data_ptr(), fresh_defender_packed=self._fresh_rows["packed"].data_ptr())
        else:
            fixed.update({"terminal_" + k: v.data_ptr() for k, v in self._terminal.items()})       # (the four keys of mcbs_defender_obs)
            fixed.update({"fresh_" + k: v.data_ptr() for k, v in self._fresh_rows.items()})
        block = training_packed_buffers if self._packed_mode else training_buffers
        self._ring = []
        for _ in range(2):
            o = _output_set(self, _TRAINING_OUTPUTS)
            self._ring.append((o, block(**fixed, **{k: v.data_ptr() for k, v in o.items()})))

    def step(self, attacker_actions, defender_actions):
        """-> ((obs, rewards, terminated, truncated, info), (dobs, dreward, dterminated, dtruncated, dinfo)): what the two agents'
        DummyVecEnvs return for this turn.  An env whose flags are set has ALREADY been reset: its observation is the fresh one, its
        episode's last observation is in `att.terminal_observation` / `terminal_observation`, and the info dicts carry the episode that
        ended — `episode_return`, `episode_length`, `episode_valid_actions`, `episode_invalid_actions` (what the reference logs at episode
        end and keeps as last_valid_action_count / last_invalid_action_count), meaningful where `dones` is set.  The attacker's
        `truncated` includes a reset request; the defender's reward on a request step is `-1 * the attacker's reward of this turn`.
        Outputs are valid until the turn after next.  The defender's action of a turn is chosen before the attacker's step of that turn."""
        att, dfd = self.att, self.dfd
        a = _as_actions(att, attacker_actions, att._action_shape, "attacker actions must have shape")
        d = _as_actions(att, defender_actions, (self.num_envs, 12), "defender actions must have shape")
        o, wb, info = att._next_output_set()
        do, dwb, dinfo, _ = dfd._next_output_set()
        if self._ring is None:
            self._output_ring()
        self._slot ^= 1
        to, tb = self._ring[self._slot]
        key = (id(wb), id(dwb), id(tb), att.invalid_action_reward_modifier, att.max_timesteps)
        call = self._calls.get(key)
        if call is None and self._packed_mode:
            call = self._calls[key] = self.engine.two_agent_train_step_packed_call(
                att.discrete, att._rows, att._packing_handle(), att.packed_observation, att.terminal_packed_observation, att._packed_fresh, wb,
                att.invalid_action_reward_modifier, att.max_timesteps, dfd.packed_observation, dwb, dfd._wc, tb)
        elif call is None:
            obs_block, keep, fresh = att._blocks()
            call = self._calls[key] = self.engine.two_agent_train_step_call(att.discrete, att._rows, obs_block, wb, att.invalid_action_reward_modifier,
                                                                            att.max_timesteps, keep, fresh, dfd._obs_block, dwb, dfd._wc, tb)
        call(a.data_ptr(), d.data_ptr())
        ainfo = dict(info, dones=att._dones, episode_valid_actions=to["attacker_valid_out"], episode_invalid_actions=to["attacker_invalid_out"])
        dinfo = dict(dinfo, dones=to["defender_dones"], episode_return=to["defender_return_out"], episode_length=to["defender_length_out"],
                     episode_valid_actions=to["defender_valid_out"], episode_invalid_actions=to["defender_invalid_out"])
        return ((att.observation, o["rewards"], o["terminated"], o["truncated"], ainfo),
                (dfd._obs, do["reward"], do["terminated"], do["truncated"], dinfo))
