"""marlon_amd.rollout.DeviceRolloutBuffer on a live AttackerVecEnv: a 12-step rollout of 64 Chain-4 envs that truncate every 5 steps is
stored with add(), advantages and returns come from ONE mcbs_gae launch and equal tests/gae_ref.py's float32 loop bit for bit (with and
without the truncation bootstrap), get() hands out a permutation of the stored rows whose fields belong together (the head re-evaluates
every stored action to its stored log-prob, bit for bit), and the state checks raise."""
import functools

import numpy as np
import pytest

from tests.gae_ref import gae_f32

pytestmark = pytest.mark.gpu

T, E = 12, 64


def _env():
    from marlon_amd.samples import chainpattern
    from marlon_amd.wrappers import AttackerVecEnv
    return AttackerVecEnv(chainpattern.new_environment(4), E, maximum_node_count=6, maximum_total_credentials=6, discrete=True,
                          materialize_masks=False, max_timesteps=5, seed=3)


def _rollout_no_obs(env, buf, with_terminal_values):
    return _rollout(env, buf, with_terminal_values, store_obs=False)


def _rollout(env, buf, with_terminal_values, store_obs=True):
    """Fill `buf` from `env`: packed masks written in place, actions from the masked head on seeded random logits, seeded random values.
    -> (logits [T, E, A], last_values [E], last dones [E], terminal values [T, E] or None)."""
    import torch
    dev = env.engine.device
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    A = env.discrete_n
    logits = torch.randn((T, E, A), generator=g, device=dev)
    values = 3.0 * torch.randn((T, E), generator=g, device=dev)
    tvals = 3.0 * torch.randn((T, E), generator=g, device=dev)
    env.reset()
    starts = torch.ones(E, dtype=torch.bool, device=dev)
    for t in range(T):
        assert buf.pos == t and not buf.full
        env.action_masks_packed(out=buf.mask_bits[buf.pos])
        d = env.sample_masked(logits[t], seed=99, step=t)
        # the observation the action was chosen on (the wrapper's persistent tensors are overwritten by the step)
        obs_fields = {k: v.clone() for k, v in env.observation_fields.items()} if store_obs else None
        _, rewards, terminated, truncated, _ = env.step(d.actions)
        tv = None
        if with_terminal_values:
            tvals[t] = torch.where(truncated.bool() & ~terminated.bool(), tvals[t], torch.zeros_like(tvals[t]))
            tv = tvals[t]
        buf.add(obs_fields, d.actions, rewards, starts, values[t], d.log_prob, bits=None, terminal_values=tv)
        starts = terminated.bool() | truncated.bool()
    assert buf.pos == T and buf.full
    last_values = 3.0 * torch.randn(E, generator=g, device=dev)
    return logits, last_values, starts, (tvals if with_terminal_values else None)


def _check_gae(buf, last_values, dones, tvals):
    r, v, s = (x.cpu().numpy() for x in (buf.rewards, buf.values, buf.episode_starts))
    adv, ret = gae_f32(r, v, s, last_values.cpu().numpy(), dones.cpu().numpy(), buf.gamma, buf.gae_lambda,
                       bootstrap=None if tvals is None else tvals.cpu().numpy())
    assert np.array_equal(buf.advantages.cpu().numpy().view(np.int32), adv.view(np.int32))
    assert np.array_equal(buf.returns.cpu().numpy().view(np.int32), ret.view(np.int32))
    return adv


@functools.lru_cache(maxsize=None)
def _filled():
    """The env, its buffer after a rollout without terminal values and compute_returns_and_advantage, and what the rollout used."""
    env = _env()
    buf = env.rollout_buffer(T)
    assert buf.n_steps == T and buf.n_envs == E and buf.mask_bits.shape == (T, E, env.engine.packed_mask_words()[1])
    assert set(buf.observations) == {"scalars", "leaked_credentials", "credential_cache_matrix", "discovered_nodes_properties",
                                     "nodes_privilegelevel"} and buf.actions.shape == (T, E)
    with pytest.raises(RuntimeError):
        buf.compute_returns_and_advantage(buf.values[0], buf.episode_starts[0])            # not full
    logits, last_values, dones, _ = _rollout(env, buf, False)
    with pytest.raises(RuntimeError):
        buf.get(100)                                                                        # before compute_returns_and_advantage
    with pytest.raises(RuntimeError):
        buf.add(None, None, None, None, None, None)                                         # full
    buf.compute_returns_and_advantage(last_values, dones)
    return env, buf, logits, last_values, dones


def test_advantages_and_returns_equal_the_float32_loop():
    env, buf, logits, last_values, dones = _filled()
    s = buf.episode_starts.cpu().numpy()
    # max_timesteps = 5: every env is truncated at steps 4 and 9 at the latest, so steps 5 and 10 start episodes
    assert s[0].all() and s[5].all() and s[10].all() and s[1:].any()
    assert buf.bootstrap is None
    adv = _check_gae(buf, last_values, dones, None)
    assert np.isfinite(adv).all() and np.abs(adv).max() > 0


def test_minibatches_are_a_permutation_of_rows_that_belong_together():
    import torch
    env, buf, logits, last_values, dones = _filled()
    dev = env.engine.device
    g1, g2 = torch.Generator(device=dev), torch.Generator(device=dev)
    g1.manual_seed(7)
    g2.manual_seed(7)
    batches = list(buf.get(100, generator=g1))
    assert [len(mb.index) for mb in batches] == [100] * 7 + [68]
    index = torch.cat([mb.index for mb in batches])
    assert torch.equal(index.sort().values, torch.arange(T * E, device=dev))
    assert not torch.equal(index, torch.arange(T * E, device=dev))
    assert torch.equal(index, torch.cat([mb.index for mb in buf.get(100, generator=g2)]))
    flat_logits = logits.view(T * E, -1)
    for mb in batches:
        t, e = mb.index // E, mb.index % E
        for got, stored in ((mb.actions, buf.actions), (mb.old_values, buf.values), (mb.old_log_prob, buf.log_probs),
                            (mb.advantages, buf.advantages), (mb.returns, buf.returns), (mb.mask_bits, buf.mask_bits)):
            assert got.device == dev and torch.equal(got, stored[t, e])
        assert set(mb.observations) == set(buf.observations)
        for k, stored in buf.observations.items():
            assert torch.equal(mb.observations[k], stored[t, e])
        # the stored rows belong together: the head gives every stored action its stored log-prob back, bit for bit
        d = env.evaluate_masked(mb.mask_bits, flat_logits[mb.index], mb.actions)
        assert torch.equal(d.log_prob.view(torch.int32), mb.old_log_prob.view(torch.int32))
    whole = list(buf.get())
    assert len(whole) == 1 and len(whole[0].index) == T * E and whole[0].mask_bits.shape == (T * E, buf.mask_bits.shape[2])
    with pytest.raises(ValueError):
        buf.get(0)


def test_reset_refills_and_terminal_values_bootstrap_the_truncated_steps():
    """A buffer of its own on the shared env (the shared buffer stays as it is): a rollout with terminal values, then reset() and the
    first rollout again without them."""
    import torch
    env, shared, _, _, _ = _filled()
    buf = env.rollout_buffer(T, store_observations=False)
    assert buf.observations is None
    logits, last_values, dones, tvals = _rollout_no_obs(env, buf, True)
    assert buf.bootstrap is not None and bool((buf.bootstrap != 0).any()) and torch.equal(buf.bootstrap, tvals)
    assert bool((buf.bootstrap[4] != 0).any()) and bool((buf.bootstrap[3] == 0).all())     # only truncated steps carry a terminal value
    buf.compute_returns_and_advantage(last_values, dones)
    _check_gae(buf, last_values, dones, tvals)
    assert not torch.equal(buf.advantages, shared.advantages)
    assert all(mb.observations is None for mb in buf.get(500))
    buf.reset()
    assert buf.pos == 0 and not buf.full and not buf.ready
    with pytest.raises(RuntimeError):
        buf.get()
    # the same rollout once more without terminal values: the bootstrap of the previous rollout is not used
    _, last_values, dones, _ = _rollout_no_obs(env, buf, False)
    buf.compute_returns_and_advantage(last_values, dones)
    _check_gae(buf, last_values, dones, None)
    assert torch.equal(buf.advantages, shared.advantages) and torch.equal(buf.mask_bits, shared.mask_bits)      # the env and the seeds repeat


def test_generic_buffer_round_trips_any_producer():
    """The generic constructor: two observation fields of different dtypes, a 2-column action, no masks, another env count."""
    import torch
    from marlon_amd.rollout import DeviceRolloutBuffer, RolloutBatch
    env, _, _, _, _ = _filled()
    eng, dev = env.engine, env.engine.device
    n_steps, n_envs = 3, 5
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    obs = [{"grid": torch.randint(0, 9, (n_envs, 2, 3), generator=g, device=dev, dtype=torch.int32),
            "flag": torch.rand(n_envs, generator=g, device=dev) < 0.5} for _ in range(n_steps)]
    acts = torch.randint(0, 4, (n_steps, n_envs, 2), generator=g, device=dev)
    rew, val, lp = (torch.randn((n_steps, n_envs), generator=g, device=dev) for _ in range(3))
    starts = torch.rand((n_steps, n_envs), generator=g, device=dev) < 0.3
    buf = DeviceRolloutBuffer(eng, n_steps, n_envs, obs=obs[0], action_shape=(2,), gamma=0.9, gae_lambda=0.8)
    assert buf.mask_bits is None and buf.observations["grid"].dtype == torch.int32 and buf.observations["flag"].dtype == torch.bool
    assert buf.observations["grid"].shape == (n_steps, n_envs, 2, 3) and buf.actions.shape == (n_steps, n_envs, 2)
    with pytest.raises(ValueError):
        DeviceRolloutBuffer(eng, n_steps, n_envs + 1, obs=obs[0])
    for t in range(n_steps):
        if t == 1:                                                                      # a producer that writes in place passes None
            buf.rewards[buf.pos].copy_(rew[t])
            buf.add(obs[t], acts[t], None, starts[t], val[t], lp[t])
        else:
            buf.add(obs[t], acts[t], rew[t], starts[t], val[t], lp[t])
    with pytest.raises(ValueError):
        DeviceRolloutBuffer(eng, 1, n_envs).add(obs[0], acts[0, :, 0], rew[0], starts[0], val[0], lp[0])      # stores no observations
    last_values, dones = torch.randn(n_envs, generator=g, device=dev), torch.rand(n_envs, generator=g, device=dev) < 0.5
    buf.compute_returns_and_advantage(last_values, dones)
    adv, ret = gae_f32(rew.cpu().numpy(), val.cpu().numpy(), starts.cpu().numpy(), last_values.cpu().numpy(), dones.cpu().numpy(), 0.9, 0.8)
    assert np.array_equal(buf.advantages.cpu().numpy().view(np.int32), adv.view(np.int32))
    assert np.array_equal(buf.returns.cpu().numpy().view(np.int32), ret.view(np.int32))
    batches = list(buf.get(4))
    assert [len(mb.index) for mb in batches] == [4, 4, 4, 3] and all(isinstance(mb, RolloutBatch) and mb.mask_bits is None for mb in batches)
    for mb in batches:
        t, e = mb.index // n_envs, mb.index % n_envs
        assert torch.equal(mb.actions, acts[t, e]) and torch.equal(mb.old_values, val[t, e]) and torch.equal(mb.old_log_prob, lp[t, e])
        assert torch.equal(mb.observations["grid"], torch.stack([o["grid"] for o in obs])[t, e])
        assert torch.equal(mb.observations["flag"], torch.stack([o["flag"] for o in obs])[t, e])
        assert torch.equal(mb.advantages, buf.advantages[t, e]) and torch.equal(mb.returns, buf.returns[t, e])
