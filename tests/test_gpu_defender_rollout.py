"""The defender's side of a PPO loop on device tensors: DefenderVecEnv.features() / feature_width (the four MultiBinary fields as SB3's
MultiInputPolicy would flatten them) and DefenderVecEnv.rollout_buffer() filled by the MultiDiscrete head, its advantages and returns
equal to tests/gae_ref.py's float32 loop bit for bit."""
import numpy as np
import pytest

from tests.gae_ref import gae_f32
from tests.test_gpu_multicategorical import _toyctf_pair

pytestmark = pytest.mark.gpu

KEYS = ["incoming_firewall_status", "infected_nodes", "outgoing_firewall_status", "services_status"]


def _played_pair(steps=3):
    att, dfd = _toyctf_pair(64, discrete=True)
    for t in range(steps):
        att.step(att.sample_masked_uniform(seed=5, step=t).actions)
        dfd.step(dfd.sample_uniform(seed=5, step=t).actions)
    return att, dfd


def test_features_are_the_four_fields_in_sorted_key_order():
    import torch
    att, dfd = _played_pair()
    obs = dfd.observation
    assert sorted(obs) == KEYS == list(dfd.FEATURE_KEYS)
    assert [int(np.prod(obs[k].shape[1:])) for k in KEYS] == [60, 10, 60, 13] and dfd.feature_width == 143
    want = torch.cat([obs[k].reshape(64, -1) for k in KEYS], dim=1)
    assert bool(want.any()) and bool(((want == 0) | (want == 1)).all())
    for dt in (torch.float32, torch.bfloat16):
        got = dfd.features(dtype=dt)
        assert got.shape == (64, 143) and got.dtype == dt and torch.equal(got, want.to(dt))
        wide = torch.full((64, 150), 7.0, dtype=dt, device=want.device)
        ret = dfd.features(out=wide)
        assert ret.data_ptr() == wide.data_ptr() and ret.shape == (64, 143)
        assert torch.equal(wide[:, :143], want.to(dt)) and bool((wide[:, 143:] == 7.0).all())
    assert dfd.features().dtype == torch.float32
    for bad in (lambda: dfd.features(out=torch.zeros((64, 142), device=want.device)),
                lambda: dfd.features(out=torch.zeros((63, 143), device=want.device)),
                lambda: dfd.features(out=torch.zeros((64, 143), dtype=torch.int32, device=want.device)),
                lambda: dfd.features(out=torch.zeros((64, 143), device=want.device), dtype=torch.bfloat16)):
        with pytest.raises(ValueError):
            bad()
    att.close()


def test_eight_step_rollout_fills_the_buffer():
    import torch
    att, dfd = _played_pair(steps=0)
    dev = att.engine.device
    E, T = 64, 8
    buf = dfd.rollout_buffer(T, gamma=0.97, gae_lambda=0.9)
    assert buf.actions.shape == (T, E, 12) and buf.mask_bits is None and sorted(buf.observations) == KEYS
    assert all(buf.observations[k].dtype == torch.int8 and buf.observations[k].shape[:2] == (T, E) for k in KEYS)
    assert dfd.rollout_buffer(T, store_observations=False).observations is None
    g = torch.Generator(device=dev).manual_seed(4)
    values = torch.randn((T, E), generator=g, device=dev)
    starts = torch.ones(E, dtype=torch.uint8, device=dev)
    stored_obs, stored_actions = [], []
    for t in range(T):
        att.step(att.sample_masked_uniform(seed=9, step=t).actions)
        logits = torch.randn((E, 77), generator=g, device=dev) * 2.0
        d = dfd.sample_actions(logits, seed=9, step=t)
        obs = {k: v.clone() for k, v in dfd.observation.items()}
        _, reward, terminated, truncated, _ = dfd.step(d.actions)
        buf.add(obs, d.actions, reward, starts, values[t], d.log_prob)
        stored_obs.append(obs)
        stored_actions.append(d.actions.clone())
        starts = (terminated | truncated).to(torch.uint8)
    assert buf.full
    last_values = torch.randn(E, generator=g, device=dev)
    buf.compute_returns_and_advantage(last_values, starts)
    adv, ret = gae_f32(buf.rewards.cpu().numpy(), values.cpu().numpy(), buf.episode_starts.cpu().numpy(), last_values.cpu().numpy(),
                       starts.cpu().numpy(), 0.97, 0.9)
    assert np.array_equal(buf.advantages.cpu().numpy().view(np.int32), adv.view(np.int32))
    assert np.array_equal(buf.returns.cpu().numpy().view(np.int32), ret.view(np.int32))
    assert bool(buf.rewards.any())
    actions = torch.stack(stored_actions).view(T * E, 12)
    seen = []
    for batch in buf.get(96, generator=torch.Generator(device=dev).manual_seed(1)):
        n = batch.index.shape[0]
        assert batch.actions.shape == (n, 12) and batch.mask_bits is None
        assert torch.equal(batch.actions, actions[batch.index])
        for k in KEYS:
            flat = torch.stack([o[k] for o in stored_obs]).view(T * E, -1)
            assert torch.equal(batch.observations[k].view(n, -1), flat[batch.index])
        assert torch.equal(batch.old_log_prob, buf.log_probs.view(-1)[batch.index])
        seen.append(batch.index)
    assert [len(s) for s in seen] == [96] * 5 + [32]
    assert torch.equal(torch.cat(seen).sort().values, torch.arange(T * E, device=dev))
    # the stored rows evaluate to the stored log-probs only under the logits that drew them; the head serves any n stored rows
    e = dfd.evaluate_actions(torch.zeros((T * E, 77), device=dev), actions)
    assert bool(torch.isfinite(e.log_prob).all()) and e.log_prob.shape == (T * E,)
    att.close()
