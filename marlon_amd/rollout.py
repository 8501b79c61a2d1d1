"""A device-resident rollout buffer for MaskablePPO: what Stable-Baselines3's (Maskable)RolloutBuffer is to a trainer, for batches that
live on the GPU.

The reference fills SB3's buffer one env step at a time and calls `on_rollout_end(new_obs, dones)`
(marlon/baseline_models/multiagent/marl_algorithm.py:51-52), which runs RolloutBuffer.compute_returns_and_advantage; `train()` then draws
shuffled minibatches.  SB3's buffer is host NumPy with `n_steps` Python iterations over `[n_envs]` vectors; this one keeps `[T, E, ...]`
device tensors, computes advantages and returns with ONE launch of mcbs_gae (bit for bit SB3's float32 loop, include/mcbs.h) and hands
out shuffled minibatches of device tensors.  torch is plumbing here (allocation, `copy_`, `randperm`, gathers); the arithmetic is the
kernel's.  Importing this module needs neither a GPU nor torch.
"""
from __future__ import annotations

import collections

# one minibatch of DeviceRolloutBuffer.get(): every field a gathered device tensor with leading axis n (`index`: the flat rows drawn,
# `observations`: dict key -> [n, ...] or None, `mask_bits`: packed masks [n, mask_words] or None — gathered from the stored bits or, for a
# buffer that stores mask keys, expanded from them into a tensor the NEXT minibatch overwrites)
RolloutBatch = collections.namedtuple("RolloutBatch", ["index", "observations", "actions", "old_values", "old_log_prob", "advantages",
                                                       "returns", "mask_bits"])


class DeviceRolloutBuffer:
    """`n_steps` x `n_envs` transitions on `engine`'s device.

    obs: dict of example `[E, ...]` tensors (storage takes their dtypes and trailing shapes) or None to store no observations.
    action_shape: trailing shape of one env's action (() for Discrete).  mask_words: the packed row width `engine.packed_mask_words()[1]`
    to store packed action masks, or None.  Storage — public, so producers can write rows in place, e.g.
    `env.action_masks_packed(out=buf.mask_bits[buf.pos])`: observations (dict), actions int64, rewards / values / log_probs /
    advantages / returns float32, episode_starts uint8, mask_bits int32, all `[T, E, ...]`; bootstrap float32 `[T, E]` appears with the
    first `terminal_values`.
    mask_key_words: `engine.mask_key_words()` to store mask KEYS instead of bits (needs mask_words too): the storage is `mask_keys`
    int32 `[T, E, Wk]`, `mask_bits` is None, and get() rebuilds each minibatch's `mask_bits` with one `engine.expand_mask_keys` call
    over the whole flattened key storage through the minibatch's `index`.  That tensor is ONE buffer reused by every minibatch (and
    every later get()): a RolloutBatch's `mask_bits` is valid until the next minibatch is drawn; clone it to keep it longer."""

    def __init__(self, engine, n_steps: int, n_envs: int, obs=None, action_shape=(), mask_words=None, gamma: float = 0.99,
                 gae_lambda: float = 0.95, mask_key_words=None):
        if int(n_steps) <= 0 or int(n_envs) <= 0:
            raise ValueError(f"n_steps and n_envs must be positive, got {n_steps} and {n_envs}")
        t = self.torch = engine.torch
        self.engine = engine
        self.device = dev = engine.device
        self.n_steps, self.n_envs = T, E = int(n_steps), int(n_envs)
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.action_shape = tuple(int(d) for d in action_shape)
        self.observations = None
        if obs is not None:
            for k, v in obs.items():
                if v.shape[0] != E:
                    raise ValueError(f"obs[{k!r}] has {v.shape[0]} rows, the buffer {E} envs")
            self.observations = {k: t.zeros((T,) + tuple(v.shape), dtype=v.dtype, device=dev) for k, v in obs.items()}
        self.actions = t.zeros((T, E) + self.action_shape, dtype=t.int64, device=dev)
        self.rewards = t.zeros((T, E), dtype=t.float32, device=dev)
        self.values = t.zeros((T, E), dtype=t.float32, device=dev)
        self.log_probs = t.zeros((T, E), dtype=t.float32, device=dev)
        self.advantages = t.zeros((T, E), dtype=t.float32, device=dev)
        self.returns = t.zeros((T, E), dtype=t.float32, device=dev)
        self.episode_starts = t.zeros((T, E), dtype=t.uint8, device=dev)
        if mask_key_words is not None and mask_words is None:
            raise ValueError("mask_key_words needs mask_words: the row width of the packed masks the keys expand to")
        self.mask_words = None if mask_words is None else int(mask_words)
        self.mask_keys = None if mask_key_words is None else t.zeros((T, E, int(mask_key_words)), dtype=t.int32, device=dev)
        self.mask_bits = None if mask_words is None or self.mask_keys is not None else t.zeros((T, E, self.mask_words), dtype=t.int32, device=dev)
        self._expanded = None              # keys: the minibatch's expanded mask_bits, allocated by the first get()
        self.bootstrap = None
        self.reset()

    def reset(self) -> None:
        """Empty the buffer for the next rollout (storage is kept and overwritten)."""
        self.pos = 0
        self.full = False
        self.ready = False                 # advantages and returns belong to the stored rollout
        self._use_bootstrap = False

    def add(self, obs, actions, rewards, episode_starts, values, log_probs, bits=None, terminal_values=None, keys=None) -> None:
        """Store one step of all envs in row `pos` (device-to-device `copy_`, converting dtypes as `copy_` does), then `pos += 1`.  Pass
        None for anything the producer has already written in place into row `pos`.  episode_starts: whether each env's observation
        was the first of an episode (the previous step's terminated | truncated).  terminal_values: float [E], the value of the
        terminal observation where this step was TRUNCATED and 0 elsewhere (SB3's `rewards[idx] += gamma * terminal_value`, applied by
        compute_returns_and_advantage); a rollout in which it was never given runs without those two operations.  bits / keys: the
        step's packed masks / mask keys, for the storage this buffer was built with."""
        if self.full:
            raise RuntimeError(f"the rollout buffer is full ({self.n_steps} steps): compute_returns_and_advantage, get, then reset")
        p = self.pos
        if obs is not None:
            if self.observations is None:
                raise ValueError("this buffer stores no observations (obs=None at construction)")
            for k, dst in self.observations.items():       # (a stored key missing from obs is a KeyError, not a silent gap)
                dst[p].copy_(obs[k].reshape(dst[p].shape))
        for src, dst in ((actions, self.actions), (rewards, self.rewards), (episode_starts, self.episode_starts), (values, self.values),
                         (log_probs, self.log_probs)):
            if src is not None:
                dst[p].copy_(src.reshape(dst[p].shape))
        if bits is not None:
            if self.mask_bits is None:
                raise ValueError("this buffer stores no packed masks (mask_words=None at construction)")
            self.mask_bits[p].copy_(bits)
        if keys is not None:
            if self.mask_keys is None:
                raise ValueError("this buffer stores no mask keys (mask_key_words=None at construction)")
            self.mask_keys[p].copy_(keys)
        if terminal_values is not None:
            if self.bootstrap is None:
                self.bootstrap = self.torch.zeros((self.n_steps, self.n_envs), dtype=self.torch.float32, device=self.device)
            elif not self._use_bootstrap:
                self.bootstrap.zero_()     # (rows of an earlier rollout)
            self._use_bootstrap = True
            self.bootstrap[p].copy_(terminal_values.reshape(self.n_envs))
        self.pos = p + 1
        self.full = self.pos == self.n_steps
        self.ready = False

    def compute_returns_and_advantage(self, last_values, dones) -> None:
        """SB3's call of the same name, one launch of mcbs_gae on the stored arrays: last_values float [E] = the value of the observation
        after the last step, dones [E] = whether that step ended an episode.  Fills `advantages` and `returns`."""
        if not self.full:
            raise RuntimeError(f"the rollout buffer holds {self.pos} of {self.n_steps} steps: fill it before computing advantages")
        t = self.torch
        lv = last_values.reshape(self.n_envs).to(device=self.device, dtype=t.float32).contiguous()
        ld = dones.reshape(self.n_envs).to(device=self.device, dtype=t.uint8).contiguous()
        self.engine.gae(self.rewards, self.values, self.episode_starts, lv, ld, self.gamma, self.gae_lambda,
                        bootstrap=self.bootstrap if self._use_bootstrap else None, advantages=self.advantages, returns=self.returns)
        self.ready = True

    def get(self, batch_size=None, generator=None):
        """Shuffled minibatches of the whole rollout: one `torch.randperm(T * E)` on the device (`generator`: a device torch.Generator,
        for a reproducible order), then RolloutBatch tuples of `batch_size` gathered rows each — the last one shorter when batch_size
        does not divide T * E, as in SB3; batch_size=None yields everything as one batch.  Flat row i is (t, e) = (i // E, i % E).
        SB3 flattens env-major instead ((e, t) = (i // T, i % T)); the permutation is uniform over all T * E rows either way, so the
        law of the minibatches is the same, only the meaning of `index` differs.  A buffer that stores mask keys hands out `mask_bits`
        expanded into one reused tensor: each RolloutBatch's `mask_bits` is valid until the next one is drawn."""
        if not self.ready:
            raise RuntimeError("advantages are not computed for this rollout: call compute_returns_and_advantage first")
        if batch_size is not None and int(batch_size) <= 0:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        return self._batches(batch_size, generator)

    def _batches(self, batch_size, generator):
        t = self.torch
        n = self.n_steps * self.n_envs
        size = n if batch_size is None else int(batch_size)
        perm = t.randperm(n, device=self.device, generator=generator)
        flat = lambda x: x.reshape((n,) + tuple(x.shape[2:]))
        obs = None if self.observations is None else {k: flat(v) for k, v in self.observations.items()}
        cols = [flat(x) for x in (self.actions, self.values, self.log_probs, self.advantages, self.returns)]
        bits = None if self.mask_bits is None else flat(self.mask_bits)
        keys = None if self.mask_keys is None else flat(self.mask_keys)
        if keys is not None and (self._expanded is None or self._expanded.shape[0] < min(size, n)):
            self._expanded = t.zeros((min(size, n), self.mask_words), dtype=t.int32, device=self.device)
        for start in range(0, n, size):
            idx = perm[start:start + size]
            if keys is not None:
                mb = self.engine.expand_mask_keys(keys, idx, out=self._expanded[:idx.shape[0]])
            else:
                mb = None if bits is None else bits.index_select(0, idx)
            yield RolloutBatch(idx, None if obs is None else {k: v.index_select(0, idx) for k, v in obs.items()},
                               *[c.index_select(0, idx) for c in cols], mb)
