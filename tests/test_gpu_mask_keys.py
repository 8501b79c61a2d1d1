"""Action-mask keys on the device (include/mcbs.h: mcbs_mask_key_words, mcbs_store_mask_keys, mcbs_expand_mask_keys): expand(store())
against pack_action_mask, the oracle's masks packed on the host and the host mirror (marlon_amd/mask_keys.py) on the keys read back;
keys stored, the envs moved on, then expanded through a shuffled index; observation bounds; the write-only contract; the state guards;
malformed keys; and the rollout buffer storing keys next to one storing bits."""
import functools

import numpy as np
import pytest

from tests import parity

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
SMALL = ["scalars", "nodes_privilegelevel"]
MASKS = ["mask_local", "mask_remote", "mask_connect"]


def pack_host(mask) -> np.ndarray:
    """bool [n, A] -> uint32 [n, ceil(A / 32)], tail bits zero (as tests/test_gpu_packed_masks.py packs the oracle's fields)."""
    mask = np.asarray(mask, dtype=bool)
    n, A = mask.shape
    W = (A + 31) // 32
    b = np.packbits(mask, axis=1, bitorder="little")
    out = np.zeros((n, 4 * W), dtype=np.uint8)
    out[:, :b.shape[1]] = b
    return out.view("<u4")


def oracle_mask(oo, E):
    return np.concatenate([oo["mask_connect"].reshape(E, -1), oo["mask_local"].reshape(E, -1), oo["mask_remote"].reshape(E, -1)], axis=1) != 0


def u32(x):
    return x.cpu().numpy().view(np.uint32)


def check_step(eng, topo, spec, want, ctx):
    """store -> expand on the live batch: the words equal pack_action_mask's, the oracle's (want, or None) and the host mirror's on the
    keys read back; -> (keys, bits)."""
    from marlon_amd import mask_keys
    W, row_words = eng.packed_mask_words()
    Wk = eng.mask_key_words()
    assert Wk == mask_keys.key_words(topo, spec)
    keys = eng.store_mask_keys()
    assert tuple(keys.shape) == (eng.E, Wk)
    bits = eng.expand_mask_keys(keys)
    assert tuple(bits.shape) == (eng.E, row_words)
    packed = eng.pack_action_mask()
    got = u32(bits)
    np.testing.assert_array_equal(got, u32(packed), err_msg=f"{ctx}: expand(store()) vs pack_action_mask")
    if want is not None:
        np.testing.assert_array_equal(got[:, :W], want, err_msg=f"{ctx}: expand(store()) vs the oracle")
    np.testing.assert_array_equal(mask_keys.expand_host(u32(keys), topo, spec), got[:, :W], err_msg=f"{ctx}: host mirror on the device's keys")
    return keys, bits


@pytest.mark.parametrize("trace,E", [("chain10_mix_s3", 1024), ("toyctf_defender_s11", 1024), ("random24_defender_s51", 256)])
def test_expand_of_store_equals_pack_and_the_oracle(trace, E):
    """Mixed valid / invalid actions, auto-resets, the defender acting; packed lists words (Chain-10, ToyCtf) and general bodies with
    more than 16 nodes (Random-24)."""
    from marlon_amd import engine
    from marlon_amd._abi import RNG_PHILOX
    from oracle.oracle import Oracle
    _, sj = parity.load_trace(trace)
    topo = parity.topology_for(trace)
    spec = parity.spec_from_json(sj, n_envs=E, auto_reset=True, rng_kind=RNG_PHILOX, seed=17, max_episode_steps=60)
    eng = engine.BatchEngine(topo, spec)
    assert bool(eng.variant()["packed"]) == (trace != "random24_defender_s51")
    orc = Oracle(topo, spec)
    obs = eng.alloc_obs(SMALL)
    seen_on, key_rows = 0, set()
    for t in range(50):
        a = eng.sample_actions(t % 5 != 4, seed=9, step=t)
        check = t % 7 == 6 or t == 49
        oo = orc.alloc_obs(SMALL + MASKS) if check else None
        if check:
            eng.step_observe(a, obs)
        else:
            eng.step(a)
        orc.step(a.cpu().numpy(), obs=oo)
        if not check:
            continue
        mask = oracle_mask(oo, E)
        keys, _ = check_step(eng, topo, spec, pack_host(mask), f"{trace} step {t}")
        seen_on += int(mask.sum())
        key_rows.update(map(bytes, u32(keys)))
    assert seen_on > 0 and len(key_rows) > 1          # (the envs were not all in one state)
    eng.close()


def test_store_move_on_expand_through_a_shuffled_index():
    """Keys and bits of 8 consecutive steps in [8, E, .] buffers, 20 more steps, then every stored row expanded through a shuffled int64
    index with duplicates: the bits are those stored at the time, not those of the envs' present state."""
    import torch
    from marlon_amd import engine
    from marlon_amd._abi import RNG_PHILOX
    trace = "chain10_mix_s3"
    _, sj = parity.load_trace(trace)
    topo = parity.topology_for(trace)
    E, T = 512, 8
    eng = engine.BatchEngine(topo, parity.spec_from_json(sj, n_envs=E, auto_reset=True, rng_kind=RNG_PHILOX, seed=5, max_episode_steps=60))
    W, row_words = eng.packed_mask_words()
    Wk = eng.mask_key_words()
    assert Wk == 5
    obs = eng.alloc_obs(SMALL)
    keys = torch.zeros((T, E, Wk), dtype=torch.int32, device=eng.device)
    bits = torch.zeros((T, E, row_words), dtype=torch.int32, device=eng.device)
    for t in range(6):
        eng.step(eng.sample_actions(True, seed=2, step=t))
    for t in range(T):
        eng.step_observe(eng.sample_actions(t % 3 != 2, seed=3, step=t), obs)
        assert eng.store_mask_keys(out=keys[t]).data_ptr() == keys[t].data_ptr()
        eng.pack_action_mask(bits[t])
    for t in range(20):
        eng.step_observe(eng.sample_actions(True, seed=4, step=t), obs)
    assert not torch.equal(eng.pack_action_mask(), bits[T - 1])                    # the envs have moved on
    g = torch.Generator(device=eng.device).manual_seed(12)
    index = torch.randint(0, T * E, (T * E,), generator=g, device=eng.device)       # shuffled, with duplicates
    assert index.unique().numel() < T * E
    flat_keys, flat_bits = keys.view(T * E, Wk), bits.view(T * E, -1)
    got = eng.expand_mask_keys(flat_keys, index)
    assert torch.equal(got, flat_bits.index_select(0, index))
    assert torch.equal(eng.expand_mask_keys(flat_keys), flat_bits)                  # no index: row i
    assert not torch.equal(bits[0], bits[T - 1]) and bool(flat_bits.any())
    eng.close()


# from tests/test_gpu_packed_masks.py BOUNDS: RL 35; C + 32 > 64 (the per-bit credential pattern); a word spans four connect rows;
# the node bound above the topology's node count
KEY_BOUNDS = [("toyctf_defender_s11", (10, 5)), ("chain4_defender_s21", (7, 36)), ("tiny_defender_s62", (4, 3)), ("tiny_defender_s62", (15, 5))]


@pytest.mark.parametrize("trace,bounds", KEY_BOUNDS, ids=[f"{t}-{n}x{c}" for t, (n, c) in KEY_BOUNDS])
def test_keys_over_observation_bounds_and_blank_observations(trace, bounds):
    """Every step checked, out-of-bound actions in between: rows whose digest is blank have the zero count in their key and expand to
    the blank mask."""
    from marlon_amd import engine
    from marlon_amd._abi import RNG_PHILOX
    from oracle.oracle import Oracle
    _, sj = parity.load_trace(trace)
    topo = parity.topology_for(trace)
    nm, cm = bounds
    E = 256
    spec = parity.spec_from_json(sj, n_envs=E, auto_reset=True, rng_kind=RNG_PHILOX, seed=77, max_episode_steps=30,
                                 maximum_node_count=nm, maximum_total_credentials=cm)
    eng = engine.BatchEngine(topo, spec)
    orc = Oracle(topo, spec)
    obs = eng.alloc_obs(SMALL)
    seen_on = seen_blank = 0
    for t in range(24):
        a = eng.sample_actions(t % 4 != 3, seed=5, step=t)
        if t % 5 == 1:
            a[::4, 1] = nm + 2                          # out of bound: the blank observation
        oo = orc.alloc_obs(SMALL + MASKS)
        eng.step_observe(a, obs)
        orc.step(a.cpu().numpy(), obs=oo)
        mask = oracle_mask(oo, E)
        keys, bits = check_step(eng, topo, spec, pack_host(mask), f"{trace} bounds {bounds} step {t}")
        blank = (u32(keys)[:, 0] & 0xFFFF) == 0
        assert not u32(keys)[blank, 1:].any() and not u32(bits)[blank].any() and not mask[blank].any()
        seen_on += int(mask.sum())
        seen_blank += int(blank.sum())
    assert seen_on > 0 and seen_blank > 0
    eng.close()


def _chain4(n_envs=64, **over):
    from marlon_amd import engine
    from marlon_amd._abi import EnvSpec
    from marlon_amd.flatten import flatten
    from marlon_amd.samples import chainpattern
    topo = flatten(chainpattern.new_environment(4))
    spec = EnvSpec(**dict(dict(n_envs=n_envs, maximum_node_count=6, maximum_total_credentials=6, attacker_goal=dict(own_atleast_percent=1.0)), **over))
    return topo, spec, engine.BatchEngine(topo, spec)


def test_write_discipline_and_indices_outside_the_storage():
    import torch
    topo, spec, eng = _chain4()
    E, dev = eng.E, eng.device
    obs = eng.alloc_obs(SMALL)
    for t in range(6):
        eng.step_observe(eng.sample_actions(True, seed=1, step=t), obs)
    W, row_words = eng.packed_mask_words()
    Wk = eng.mask_key_words()
    keys = eng.store_mask_keys()
    want_bits = eng.pack_action_mask()[:, :W]
    assert bool(want_bits.any())
    # store: rows padded with sentinel words, and an offset view whose rows are aligned to 4 bytes only
    padded = torch.full((E, Wk + 4), SENTINEL, dtype=torch.int32, device=dev)
    eng.store_mask_keys(out=padded)
    assert torch.equal(padded[:, :Wk], keys) and bool((padded[:, Wk:] == SENTINEL).all())
    wide = torch.full((E, Wk + 3), SENTINEL, dtype=torch.int32, device=dev)
    eng.store_mask_keys(out=wide[:, 1:Wk + 1])
    assert torch.equal(wide[:, 1:Wk + 1], keys) and bool((wide[:, 0] == SENTINEL).all()) and bool((wide[:, Wk + 1:] == SENTINEL).all())
    # expand: from both of those key layouts into padded rows and into an offset view
    for src in (padded, wide[:, 1:Wk + 1]):
        out = torch.full((E, row_words + 4), SENTINEL, dtype=torch.int32, device=dev)
        eng.expand_mask_keys(src, out=out)
        assert torch.equal(out[:, :W], want_bits) and bool((out[:, W:] == SENTINEL).all())
        ow = torch.full((E, W + 3), SENTINEL, dtype=torch.int32, device=dev)
        eng.expand_mask_keys(src, out=ow[:, 1:W + 1])
        assert torch.equal(ow[:, 1:W + 1], want_bits) and bool((ow[:, 0] == SENTINEL).all()) and bool((ow[:, W + 1:] == SENTINEL).all())
    # an index of -1 or n_source_rows: a zero row; any row count (7 is no multiple of the four wavefronts of a workgroup)
    index = torch.tensor([3, -1, E, 0, E - 1, 2 ** 40, 3], dtype=torch.int64, device=dev)
    out = torch.full((7, row_words), SENTINEL, dtype=torch.int32, device=dev)
    eng.expand_mask_keys(keys, index, out=out)
    for i, s in enumerate(index.tolist()):
        if 0 <= s < E:
            assert torch.equal(out[i, :W], want_bits[s]), i
        else:
            assert not bool(out[i, :W].any()), i
    assert bool((out[:, W:] == SENTINEL).all())
    # short rows
    with pytest.raises(ValueError):
        eng.store_mask_keys(out=padded[:, :Wk - 1])
    with pytest.raises(ValueError):
        eng.expand_mask_keys(padded[:, :Wk - 1])
    torch.cuda.synchronize(dev)
    lib, h, st = eng.lib, eng._h, eng._stream()
    assert lib.mcbs_store_mask_keys(h, padded.data_ptr(), Wk - 1, st) == -1                                        # MCBS_EINVAL
    assert lib.mcbs_store_mask_keys(h, None, Wk, st) == -1
    big = torch.zeros((E, row_words), dtype=torch.int32, device=dev)
    assert lib.mcbs_expand_mask_keys(h, keys.data_ptr(), Wk - 1, None, E, big.data_ptr(), row_words, E, st) == -1
    assert lib.mcbs_expand_mask_keys(h, keys.data_ptr(), Wk, None, E, big.data_ptr(), W - 1, E, st) == -1
    assert lib.mcbs_expand_mask_keys(h, keys.data_ptr(), Wk, None, E, big.data_ptr(), row_words, E + 1, st) == -1   # no index: n_rows <= n_source_rows
    assert lib.mcbs_expand_mask_keys(h, None, Wk, None, E, big.data_ptr(), row_words, E, st) == -1
    assert lib.mcbs_expand_mask_keys(h, keys.data_ptr(), Wk, None, E, big.data_ptr(), row_words, 0, st) == 0        # a no-op
    eng.close()


def test_state_guards_and_expand_without_a_digest():
    """store_mask_keys shares pack_action_mask's preconditions; expand_mask_keys needs no digest: it serves a batch that was never
    observed and an ExternalRandomEvents batch, given keys."""
    import torch
    from marlon_amd import engine, mask_keys
    topo, spec, eng = _chain4()
    small = eng.alloc_obs(SMALL)
    with pytest.raises(engine.McbsError, match=r"\(-5\).*no observation"):
        eng.store_mask_keys()
    eng.observe(small)
    eng.store_mask_keys()
    for t in range(5):
        eng.step_observe(eng.sample_actions(True, seed=1, step=t), small)
    keys = eng.store_mask_keys()
    bits = eng.pack_action_mask()
    mask = torch.zeros(eng.E, dtype=torch.uint8, device=eng.device)
    mask[::3] = 1
    eng.reset(mask)
    with pytest.raises(engine.McbsError, match=r"\(-5\).*reset by mask"):
        eng.store_mask_keys()
    assert torch.equal(eng.expand_mask_keys(keys), bits)          # the stored keys still expand
    eng.observe(small, env_mask=mask)
    eng.store_mask_keys()
    eng.reset()
    with pytest.raises(engine.McbsError, match=r"\(-5\).*no observation"):
        eng.store_mask_keys()
    eng.close()

    _, _, fresh = _chain4()                                       # never observed
    assert torch.equal(fresh.expand_mask_keys(keys.to(fresh.device)), bits.to(fresh.device))
    fresh.close()

    _, ere_spec, ere = _chain4(defender=("random_events",))
    ere.observe(ere.alloc_obs(SMALL))
    with pytest.raises(engine.McbsError, match=r"\(-5\).*ExternalRandomEvents"):
        ere.store_mask_keys()
    got = ere.expand_mask_keys(keys.to(ere.device))
    W = ere.packed_mask_words()[0]
    np.testing.assert_array_equal(u32(got)[:, :W], mask_keys.expand_host(u32(keys), topo, ere_spec))
    assert torch.equal(got.cpu(), bits.cpu())
    ere.close()


@pytest.mark.parametrize("trace", ["toyctf_defender_s11", "random24_defender_s51"])
def test_malformed_keys_equal_the_host_mirror(trace):
    """64 rows of arbitrary words (counts up to 0xFFFF, node bytes up to 0xFF, owned-source bits anywhere), some with their count cut
    into the valid range: the device applies the header's rule exactly as mask_keys.expand_host does, and stays inside its tables."""
    import torch
    from marlon_amd import engine, mask_keys
    from marlon_amd._abi import RNG_PHILOX
    _, sj = parity.load_trace(trace)
    topo = parity.topology_for(trace)
    spec = parity.spec_from_json(sj, n_envs=4, rng_kind=RNG_PHILOX)
    eng = engine.BatchEngine(topo, spec)
    Wk, W = eng.mask_key_words(), eng.packed_mask_words()[0]
    rng = np.random.default_rng(41)
    keys = rng.integers(0, 2 ** 32, size=(64, Wk + 2), dtype=np.uint64).astype(np.uint32)
    keys[16:40, 0] = rng.integers(0, topo.n_nodes + 2, size=24).astype(np.uint32) | (rng.integers(0, 2 * spec.maximum_total_credentials, size=24).astype(np.uint32) << 16)
    keys[40:48, 1 + (topo.n_nodes + 31) // 32:Wk] = 0xFFFFFFFF                   # no such node anywhere
    keys[48:52, 0] = 0xFFFF | (0xFFFF << 16)
    dev_keys = torch.as_tensor(keys.view(np.int32)).to(eng.device)
    got = u32(eng.expand_mask_keys(dev_keys))[:, :W]
    want = mask_keys.expand_host(keys, topo, spec)
    np.testing.assert_array_equal(got, want)
    assert want.any() and not want.all()
    eng.close()


@functools.lru_cache(maxsize=None)
def _two_buffers():
    """One 6-step rollout of 256 Chain-4 envs stored twice: mask_storage='keys' (filled in place) and 'bits'."""
    import torch
    from marlon_amd.samples import chainpattern
    from marlon_amd.wrappers import AttackerVecEnv
    from marlon_amd import cyberbattle_env as ce
    E, T = 256, 6
    env = AttackerVecEnv(chainpattern.new_environment(4), E, maximum_node_count=6, maximum_total_credentials=6,
                         attacker_goal=ce.AttackerGoal(own_atleast_percent=1.0), max_timesteps=25, discrete=True, materialize_masks=False)
    dev = env.engine.device
    kb = env.rollout_buffer(T, mask_storage="keys")
    bb = env.rollout_buffer(T)
    Wk = env.engine.mask_key_words()
    assert kb.mask_bits is None and tuple(kb.mask_keys.shape) == (T, E, Wk) and kb.mask_keys.dtype == torch.int32
    assert bb.mask_keys is None and tuple(bb.mask_bits.shape) == (T, E, env.engine.packed_mask_words()[1])
    with pytest.raises(ValueError):
        env.rollout_buffer(T, mask_storage="bytes")
    with pytest.raises(ValueError):
        bb.add(None, None, None, None, None, None, keys=kb.mask_keys[0])
    g = torch.Generator(device=dev).manual_seed(6)
    zeros = torch.zeros(E, device=dev)
    logits = torch.randn((T, E, env.discrete_n), generator=g, device=dev)
    for t in range(T):
        for k in range(4):                                   # steps between stored ones: the stored rows differ
            env.step(env.sample_masked_uniform(seed=8, step=10 * t + k).actions)
        d = env.sample_masked(logits[t], seed=9, step=t)
        rewards = torch.rand(E, generator=g, device=dev)
        if t % 2:
            env.action_mask_keys(out=kb.mask_keys[kb.pos])
            kb.add(env.observation_fields, d.actions, rewards, zeros, zeros, d.log_prob)
        else:
            kb.add(env.observation_fields, d.actions, rewards, zeros, zeros, d.log_prob, keys=env.action_mask_keys())
        bb.add(env.observation_fields, d.actions, rewards, zeros, zeros, d.log_prob, bits=env.action_masks_packed())
        env.step(d.actions)
    for b in (kb, bb):
        b.compute_returns_and_advantage(zeros, zeros)
    return env, kb, bb, logits


def test_rollout_buffer_keys_yield_the_minibatches_of_bits():
    import torch
    env, kb, bb, logits = _two_buffers()
    dev = env.engine.device
    T, E = kb.n_steps, kb.n_envs
    g1, g2 = torch.Generator(device=dev).manual_seed(7), torch.Generator(device=dev).manual_seed(7)
    flat_logits = logits.view(T * E, -1)
    sizes, ptrs = [], set()
    for a, b in zip(kb.get(500, generator=g1), bb.get(500, generator=g2)):
        assert torch.equal(a.index, b.index)
        assert a.mask_bits.shape == b.mask_bits.shape and a.mask_bits.dtype == torch.int32 and torch.equal(a.mask_bits, b.mask_bits)
        assert torch.equal(a.actions, b.actions) and torch.equal(a.old_log_prob, b.old_log_prob)
        da = env.evaluate_masked(a.mask_bits, flat_logits[a.index], a.actions)
        db = env.evaluate_masked(b.mask_bits, flat_logits[b.index], b.actions)
        assert torch.equal(da.log_prob.view(torch.int32), db.log_prob.view(torch.int32))
        assert torch.equal(da.log_prob.view(torch.int32), a.old_log_prob.view(torch.int32))      # the mask each action was drawn under
        sizes.append(len(a.index))
        ptrs.add(a.mask_bits.data_ptr())
    assert sizes == [500, 500, 500, 36] and len(ptrs) == 1          # one output tensor, reused by every minibatch
    whole_k, whole_b = list(kb.get()), list(bb.get())
    assert len(whole_k) == 1 and torch.equal(whole_k[0].mask_bits, bb.mask_bits.view(T * E, -1).index_select(0, whole_k[0].index))
    assert len(whole_b) == 1 and bool(bb.mask_bits.any()) and not torch.equal(bb.mask_bits[0], bb.mask_bits[T - 1])
