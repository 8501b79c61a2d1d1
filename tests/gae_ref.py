"""Reference restatements of generalized advantage estimation for the tests of mcbs_gae (include/mcbs.h) — NumPy only, no GPU, no
library.

`gae_f32` is the loop of Stable-Baselines3 2.x's RolloutBuffer.compute_returns_and_advantage, written as SB3 writes it: float32 arrays,
Python-float coefficients, `last_gae_lam = 0`.  Under NumPy's rules every operation in it is ONE float32 operation, in the order the header
documents; the kernel must give the same bits.  SB3 itself is not installed where these tests run, so parity with SB3 is what this
file claims to restate, not something a test pins.  `gae_f64` is the same recurrence in float64, for error bounds.
"""
import numpy as np


def gae_f32(rewards, values, episode_starts, last_values, last_dones, gamma, gae_lambda, bootstrap=None):
    """rewards, values float32 [T, E]; episode_starts, last_dones 0 / 1 flags [T, E], [E] (any nonzero byte is a flag); last_values
    float32 [E]; gamma, gae_lambda Python floats; bootstrap: optional float32 [T, E] (SB3's `rewards[idx] += gamma * terminal_value`, with
    0 where nothing was truncated).  -> (advantages, returns) float32 [T, E]."""
    gamma, gae_lambda = float(gamma), float(gae_lambda)
    rewards = np.array(rewards, dtype=np.float32)
    values = np.asarray(values, dtype=np.float32)
    episode_starts = (np.asarray(episode_starts) != 0).astype(np.float32)
    last_dones = (np.asarray(last_dones) != 0).astype(np.float32)
    last_values = np.asarray(last_values, dtype=np.float32)
    if bootstrap is not None:
        rewards = rewards + gamma * np.asarray(bootstrap, dtype=np.float32)
    n_steps = rewards.shape[0]
    advantages = np.zeros_like(rewards)
    last_gae_lam = 0
    for step in reversed(range(n_steps)):
        if step == n_steps - 1:
            next_non_terminal = 1.0 - last_dones
            next_values = last_values
        else:
            next_non_terminal = 1.0 - episode_starts[step + 1]
            next_values = values[step + 1]
        delta = rewards[step] + gamma * next_values * next_non_terminal - values[step]
        last_gae_lam = delta + gamma * gae_lambda * next_non_terminal * last_gae_lam
        advantages[step] = last_gae_lam
    returns = advantages + values
    assert advantages.dtype == np.float32 and returns.dtype == np.float32
    return advantages, returns


def gae_f64(rewards, values, episode_starts, last_values, last_dones, gamma, gae_lambda, bootstrap=None):
    """The same recurrence with every array and every operation in float64.  -> (advantages, returns) float64 [T, E]."""
    gamma, gae_lambda = float(gamma), float(gae_lambda)
    rewards = np.array(rewards, dtype=np.float64)
    values = np.asarray(values, dtype=np.float64)
    episode_starts = (np.asarray(episode_starts) != 0).astype(np.float64)
    last_dones = (np.asarray(last_dones) != 0).astype(np.float64)
    last_values = np.asarray(last_values, dtype=np.float64)
    if bootstrap is not None:
        rewards = rewards + gamma * np.asarray(bootstrap, dtype=np.float64)
    n_steps = rewards.shape[0]
    advantages = np.zeros_like(rewards)
    last_gae_lam = 0
    for step in reversed(range(n_steps)):
        if step == n_steps - 1:
            next_non_terminal = 1.0 - last_dones
            next_values = last_values
        else:
            next_non_terminal = 1.0 - episode_starts[step + 1]
            next_values = values[step + 1]
        delta = rewards[step] + gamma * next_values * next_non_terminal - values[step]
        last_gae_lam = delta + gamma * gae_lambda * next_non_terminal * last_gae_lam
        advantages[step] = last_gae_lam
    return advantages, advantages + values
