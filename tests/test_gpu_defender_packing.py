"""Packed defender observations on the device (include/mcbs.h "packed defender observations", marlon_amd/csrc/mcbs_defender_obs_packing.hip):
DefenderVecEnv(observation_format="packed") next to a dense twin, the pack / unpack / encode kernels through a row index, the rollout
idiom and the refusals.  References: the dense wrapper's int8 fields through features.DefenderObservationPacking.pack_host, the
oracle's defender_observe(), and torch.cat of the gathered dense fields.

Shapes: ToyCtf at 64 envs (fused, 5 words) and random_net at 24, 70 and 129 nodes with E = 133 — one full and one partial workgroup;
words per set 1, 2 and 4; the turn writes the rows itself at 24 nodes and ToyCtf, a second launch does at 70 and 129."""
import functools

import numpy as np
import pytest

from tests.test_gpu_defender_layouts import _draw_attacker, _rows_of

pytestmark = pytest.mark.gpu

KEYS = ("incoming_firewall_status", "infected_nodes", "outgoing_firewall_status", "services_status")       # sorted: features()' column order
NAMES = ["toyctf", "random24", "random70", "random129"]
LAUNCHES = {"toyctf": 1, "random24": 1, "random70": 2, "random129": 2}
# turns of the lock-step: past the attacker's own truncation (50 steps for _toyctf_pair, 23 for the random networks), so that its
# auto-reset and the defender wrappers' reset(mask) that follows are part of every run
TURNS = {"toyctf": 52, "random24": 25, "random70": 25, "random129": 25}


def _pair(name, fmt, **kw):
    """(attacker, defender wrapper in observation format `fmt`) on a batch of its own"""
    from marlon_amd.wrappers import DefenderVecEnv
    if name == "toyctf":
        from tests.test_gpu_multicategorical import _toyctf_pair
        att, dfd = _toyctf_pair(64, **kw)
        return att, dfd if fmt == "dense" else DefenderVecEnv(att, max_timesteps=50, invalid_action_reward=-1, loss_reward=-5000.0, observation_format=fmt)
    from marlon_amd import cyberbattle_env as ce, flatten as F, model
    from marlon_amd.samples import random_net
    from marlon_amd.wrappers import AttackerVecEnv
    n = int(name[6:])
    env_m = random_net.build(model, n, 5)
    for _, info in env_m.nodes():
        info.reimagable = True
    topo = F.flatten(env_m)
    att = AttackerVecEnv(topo, 133, maximum_node_count=n, maximum_total_credentials=max(1, len(topo.triples)),
                         maximum_discoverable_credentials_per_action=8, attacker_goal=ce.AttackerGoal(own_atleast_percent=1.0),
                         defender_constraint=ce.DefenderConstraint({24: 0.9, 70: 0.95, 129: 0.97}[n]), losing_reward=0.0, max_timesteps=23, seed=29,
                         learned_defender=True, materialize_masks=False, **kw)
    return att, DefenderVecEnv(att, max_timesteps=17, invalid_action_reward=-3.0, reset_on_constraint_broken=False, loss_reward=-700.0,
                               sla_worsening_penalty_scale=137.0, observation_format=fmt)


def _host(obs):
    return {k: obs[k].cpu().numpy() for k in KEYS}


def _words(x):
    return x.cpu().numpy().view(np.uint32)


def _draw_defender(rng, nvec, installed):
    """Random defender vectors as tests/test_gpu_defender_layouts.py draws them: kinds -1 and -2 included, re-imaging aimed at held nodes"""
    E = installed.shape[0]
    da = (rng.random((E, 12)) * nvec).astype(np.int64)
    da[rng.random(E) < 0.3, 0] = 0
    for e in np.flatnonzero(rng.random(E) < 0.15):
        held = np.flatnonzero(installed[e])
        if held.size:
            da[e, 0], da[e, 1] = 0, held[rng.integers(held.size)]
    da[rng.random(E) < 0.05, 0] = -1
    da[rng.random(E) < 0.05, 0] = -2
    return da


@functools.lru_cache(maxsize=None)
def _lock_step(name):
    """A dense-mode and a packed-mode pair driven with the same actions for TURNS[name] turns, everything compared every turn; -> the two
    pairs in the state after the last turn (the other tests read it and leave it as it is)."""
    from oracle.oracle import Oracle
    (att_d, dfd_d), (att_p, dfd_p) = _pair(name, "dense"), _pair(name, "packed")
    t = att_d.torch
    dev = att_d.engine.device
    E = att_d.num_envs
    P = dfd_p.observation_packing()
    W = P.words
    assert dfd_d.observation_packing().words == W == att_p.engine.defender_obs_words() == att_d.engine.defender_obs_words()
    assert att_p.engine.defender_wrapper_step_packed_launches() == LAUNCHES[name]
    assert att_p.engine.variant()["fused_defender_obs"] == (1 if LAUNCHES[name] == 1 else 0)
    assert set(dfd_p.observation) == {"packed"} and dfd_p.observation["packed"] is dfd_p.packed_observation
    assert dfd_p.packed_observation.dtype == t.int32 and tuple(dfd_p.packed_observation.shape) == (E, W)
    assert not any(hasattr(v, "dtype") and v.dtype == t.int8 and v.dim() == 2 for v in vars(dfd_p).values()), "packed mode allocates no int8 field"
    np.testing.assert_array_equal(_words(dfd_p.packed_observation), P.pack_host(_host(dfd_d.observation)), err_msg=f"{name} reset rows")
    orc = Oracle(att_d.topo, att_d.spec)
    orc.reset()                                          # as the attacker wrapper's reset() did
    rng = np.random.Generator(np.random.PCG64(31))
    n_disc = np.ones(E, np.int64)
    att_t = np.zeros(E, np.int64)
    maxt_a = att_d.max_timesteps
    after_reset = oracle_checks = ones = 0
    kinds = set()
    for turn in range(TURNS[name]):
        ctx = f"{name} turn {turn}"
        a = _draw_attacker(rng, att_d.nvec, n_disc, 0.8)
        rows, _ = _rows_of(a, n_disc)
        obs, r, term, trunc, _ = att_d.step(a)
        _, r2, term2, trunc2, _ = att_p.step(a)
        assert t.equal(r, r2) and t.equal(term, term2) and t.equal(trunc, trunc2), ctx + " attacker sides"
        o = orc.step(rows)
        att_t += 1
        a_done = (o["terminated"] != 0) | (att_t >= maxt_a)
        np.testing.assert_array_equal((term.cpu().numpy() != 0) | (trunc.cpu().numpy() != 0), a_done, err_msg=ctx + " attacker dones")
        for i in np.flatnonzero(a_done):
            orc.reset(int(i))
        att_t[a_done] = 0
        n_disc = obs["discovered_node_count"].cpu().numpy().astype(np.int64)
        if a_done.any():                                 # the attacker's auto-reset: both defender wrappers start over for those envs
            mask = t.as_tensor(a_done.astype(np.uint8), device=dev)
            dfd_d.reset(mask)
            got = dfd_p.reset(mask)
            assert got["packed"] is dfd_p.packed_observation
            np.testing.assert_array_equal(_words(dfd_p.packed_observation), P.pack_host(_host(dfd_d.observation)), err_msg=ctx + " rows after dfd.reset(mask)")
            after_reset += int(a_done.sum())
        da = _draw_defender(rng, dfd_d.nvec, orc.get_state()[1]["installed"])
        kinds.update(np.unique(da[:, 0]).tolist())
        od, rd, td, ud, info_d = dfd_d.step(da)
        op, rp, tp, up, info_p = dfd_p.step(da)
        orc.defender_step(da)
        assert op["packed"] is dfd_p.packed_observation
        want = P.pack_host(_host(od))
        got = _words(dfd_p.packed_observation)
        np.testing.assert_array_equal(got, want, err_msg=ctx + " packed rows against pack_host of the dense observation")
        ones += int(np.unpackbits(got.view(np.uint8)).sum())
        np.testing.assert_array_equal(rp.cpu().numpy().view(np.uint64), rd.cpu().numpy().view(np.uint64), err_msg=ctx + " reward bits")
        assert t.equal(tp, td) and t.equal(up, ud), ctx + " terminated / truncated"
        assert set(info_p) == set(info_d)
        for k in info_d:
            x, y = info_p[k], info_d[k]
            assert x.dtype == y.dtype and t.equal(x.view(t.uint8), y.view(t.uint8)), f"{ctx} info[{k!r}]"
        for k in ("timesteps", "valid_action_count", "invalid_action_count", "has_breached_sla"):
            assert t.equal(getattr(dfd_p, k), getattr(dfd_d, k)), f"{ctx} {k}"
        assert t.equal(dfd_p.prev_availability.view(t.int64), dfd_d.prev_availability.view(t.int64)), ctx + " prev_availability bits"
        if turn in (7, TURNS[name] - 1):                       # ... and against the oracle's own observation
            oo = orc.defender_observe()
            np.testing.assert_array_equal(got, P.pack_host({k: np.asarray(oo[k]).reshape(E, -1) for k in KEYS}), err_msg=ctx + " rows against the oracle")
            oracle_checks += 1
        d_done = (td.cpu().numpy() != 0) | (ud.cpu().numpy() != 0)
        if d_done.any():
            mask = t.as_tensor(d_done.astype(np.uint8), device=dev)
            dfd_d.reset(mask)
            dfd_p.reset(mask)
    assert after_reset > 0 and oracle_checks == 2 and ones > 0 and {-2, -1, 0, 1, 2}.issubset(kinds), (after_reset, ones, kinds)
    return (att_d, dfd_d), (att_p, dfd_p)


@pytest.mark.parametrize("name", NAMES)
def test_lock_step_packed_against_dense_and_oracle(name):
    """The packed wrapper's rows equal pack_host of the dense wrapper's fields every turn, after every masked reset, and the oracle's
    observation; rewards (bits), flags, info and counters are identical; 1 launch at ToyCtf and 24 nodes, 2 at 70 and 129."""
    _lock_step(name)


@pytest.mark.parametrize("name", NAMES)
def test_observation_packed_and_out_discipline(name):
    """observation_packed() of the dense wrapper (one pack launch) gives the packed wrapper's words; out= into rows of W_def + 3 words
    pre-filled with 0xFFFFFFFF: every word below W_def written whole with the tail bits zero, the three beyond untouched — for the pack
    kernel, the live-state kernel and the packed wrapper's copy."""
    (att_d, dfd_d), (att_p, dfd_p) = _lock_step(name)
    t = att_d.torch
    E, P = att_d.num_envs, dfd_p.observation_packing()
    W, F = P.words, P.width
    want = P.pack_host(_host(dfd_d.observation))
    np.testing.assert_array_equal(_words(dfd_p.packed_observation), want)
    np.testing.assert_array_equal(_words(dfd_d.observation_packed()), want)
    assert dfd_p.observation_packed() is dfd_p.packed_observation
    for what, fill in (("dense observation_packed", lambda o: dfd_d.observation_packed(out=o)),
                       ("packed observation_packed", lambda o: dfd_p.observation_packed(out=o)),
                       ("defender_observe_packed", lambda o: att_d.engine.defender_observe_packed(out=o)),
                       ("pack_defender_observation", lambda o: att_p.engine.pack_defender_observation(dict(dfd_d.observation), out=o))):
        wide = t.full((E, W + 3), -1, dtype=t.int32, device=att_d.engine.device)
        assert fill(wide) is wide
        got = _words(wide)
        np.testing.assert_array_equal(got[:, :W], want, err_msg=what)
        assert (got[:, W:] == 0xFFFFFFFF).all(), what + ": words from W_def on were touched"
        if F % 32:
            assert not (got[:, W - 1] >> np.uint32(F % 32)).any(), what + ": tail bits"
    # v != 0 is the bit: a dense row holding other non-zero values packs to the same words
    odd = {k: v * 5 for k, v in dfd_d.observation.items()}
    np.testing.assert_array_equal(_words(att_d.engine.pack_defender_observation(odd)), want)


def _index(rng, n, m):
    """permuting, repeating row index [n] into m rows with ONE entry outside [0, m) (n >= 1)"""
    idx = rng.integers(0, m, n).astype(np.int64)
    if n:
        idx[n // 2] = m + 5 if n % 2 else -1
    return idx


@pytest.mark.parametrize("name", NAMES)
def test_unpack_and_encode_through_an_index(name):
    """unpack_defender_observation and encode_defender_features through a permuting, repeating index with one out-of-range entry,
    0 / 1 / 65 / 300 rows: the int8 fields and fp32 / bf16 / fp16 rows against torch.cat of the gathered dense fields (bit for bit), the
    row of the bad index all zero and counted once; wide out= keeps its sentinel columns; the dense source gives the packed source's rows."""
    (att_d, dfd_d), (att_p, dfd_p) = _lock_step(name)
    t = att_d.torch
    dev, eng = att_d.engine.device, att_p.engine
    E, F = att_d.num_envs, dfd_p.feature_width
    dense = dfd_d.observation
    packed = dfd_p.packed_observation
    before = packed.clone()
    rng = np.random.Generator(np.random.PCG64(7))
    cat = t.cat([dense[k].reshape(E, -1) for k in KEYS], dim=1)                 # [E, F] int8: features()' columns
    assert cat.shape[1] == F
    for n in (0, 1, 65, 300):
        idx_h = _index(rng, n, E)
        idx = t.as_tensor(idx_h, device=dev)
        inside = t.as_tensor((idx_h >= 0) & (idx_h < E), device=dev)
        gathered = cat.index_select(0, idx.clamp(0, E - 1)) * inside[:, None].to(t.int8)
        un = dfd_p.unpack_observation(packed, index=idx)
        assert set(un) == set(KEYS)
        assert t.equal(t.cat([un[k] for k in KEYS], dim=1), gathered), f"unpack n={n}"
        for dt in (t.float32, t.bfloat16, t.float16):
            want = gathered.to(dt)
            bad = t.zeros(1, dtype=t.int32, device=dev)
            got = dfd_p.encode_features_packed(packed, index=idx, dtype=dt, bad_rows=bad)
            assert got.dtype == dt and tuple(got.shape) == (n, F)
            bits = t.int32 if dt == t.float32 else t.int16
            assert t.equal(got.contiguous().view(bits), want.view(bits)), f"encode packed n={n} {dt}"
            assert int(bad) == (1 if n else 0), f"bad_rows n={n}"
            wide = t.full((n, F + 5), 7.0, dtype=dt, device=dev)
            ret = eng.encode_defender_features(dense=dict(dense), index=idx, out=wide, bad_rows=bad)
            assert ret.data_ptr() == wide.data_ptr() and t.equal(ret, want), f"encode dense n={n} {dt}"
            assert (wide[:, F:] == 7.0).all(), "columns from F on were touched"
            assert int(bad) == (2 if n else 0)
            odd = t.full((n + 1, F + 3), 7.0, dtype=dt, device=dev)                 # rows on odd boundaries: the narrow store paths
            ret = dfd_p.encode_features_packed(packed, index=idx, out=odd[1:, 1:F + 2])
            assert t.equal(ret, want) and (odd[:, 0] == 7.0).all() and (odd[:, F + 1:] == 7.0).all() and (odd[0] == 7.0).all()
    un = dfd_p.unpack_observation(packed)                                        # no index: row for row
    assert all(t.equal(un[k], dense[k].reshape(E, -1)) for k in KEYS)
    part = {KEYS[1]: t.full((E, dense[KEYS[1]].shape[1]), 3, dtype=t.int8, device=dev)}
    assert eng.unpack_defender_observation(packed, out=part) is part and t.equal(part[KEYS[1]], dense[KEYS[1]])     # a missing member is skipped
    assert t.equal(packed, before), "the source rows were modified"


@pytest.mark.parametrize("name", NAMES)
def test_features_packed_mode_equals_dense_mode(name):
    (att_d, dfd_d), (att_p, dfd_p) = _lock_step(name)
    t = att_d.torch
    E, F = att_d.num_envs, dfd_d.feature_width
    before = dfd_p.packed_observation.clone()
    cat = t.cat([dfd_d.observation[k].reshape(E, -1) for k in KEYS], dim=1)
    for dt in (t.float32, t.bfloat16, t.float16):
        a, b = dfd_d.features(dtype=dt), dfd_p.features(dtype=dt)
        assert a.dtype == b.dtype == dt and tuple(a.shape) == tuple(b.shape) == (E, F)
        assert t.equal(a, b) and t.equal(a, cat.to(dt)), dt
        wide = t.full((E, F + 7), -3.0, dtype=dt, device=att_d.engine.device)
        assert t.equal(dfd_p.features(out=wide), a) and (wide[:, F:] == -3.0).all()
    assert t.equal(dfd_d.features(dtype=t.float64), cat.double())               # another floating dtype: the four copies, dense mode only
    with pytest.raises(ValueError, match="observation_format='packed'"):
        dfd_p.features(dtype=t.float64)
    assert t.equal(dfd_p.packed_observation, before)


def test_rollout_idiom_packed_buffer_next_to_a_dense_one():
    """rollout_buffer(pack_observations=True) filled with observation_packed(out=buf.observations["packed"][buf.pos]) and add(obs=None)
    next to a dense buffer on a lock-step pair: every minibatch's encode_features_packed(storage, index=mb.index) equals the features
    of the dense minibatch."""
    (att_d, dfd_d), (att_p, dfd_p) = _pair("toyctf", "dense"), _pair("toyctf", "packed")
    t = att_d.torch
    dev, E, T = att_d.engine.device, att_d.num_envs, 8
    W = dfd_p.observation_packing().words
    buf_d, buf_p = dfd_d.rollout_buffer(T), dfd_p.rollout_buffer(T)             # the default is the wrapper's mode
    assert set(buf_d.observations) == set(KEYS) and set(buf_p.observations) == {"packed"}
    assert buf_p.observations["packed"].dtype == t.int32 and tuple(buf_p.observations["packed"].shape) == (T, E, W)
    buf_x = dfd_d.rollout_buffer(T, pack_observations=True)                     # a dense wrapper may store packed rows too: one pack launch per step
    rng = np.random.Generator(np.random.PCG64(3))
    g = t.Generator(device=dev).manual_seed(5)
    zeros = t.zeros(E, device=dev)
    for step in range(T):
        buf_d.add(dfd_d.observation, None, zeros, zeros, zeros, zeros)
        dfd_p.observation_packed(out=buf_p.observations["packed"][buf_p.pos])
        buf_p.add(None, None, zeros, zeros, zeros, zeros)
        dfd_d.observation_packed(out=buf_x.observations["packed"][buf_x.pos])
        buf_x.add(None, None, zeros, zeros, zeros, zeros)
        a = att_d.sample_uniform(seed=3, step=step).actions
        att_d.step(a)
        att_p.step(a)
        da = (rng.random((E, 12)) * dfd_d.nvec).astype(np.int64)
        dfd_d.step(da)
        dfd_p.step(da)
    assert t.equal(buf_x.observations["packed"], buf_p.observations["packed"])
    assert len(t.unique(buf_p.observations["packed"].view(T * E, W), dim=0)) > 1, "the stored rows never changed"
    for b in (buf_d, buf_p):
        b.compute_returns_and_advantage(zeros, zeros)
    storage = buf_p.observations["packed"].view(T * E, -1)
    batches = 0
    for mb in buf_d.get(100, generator=g):
        want = t.cat([mb.observations[k].reshape(mb.index.shape[0], -1) for k in KEYS], dim=1)
        for dt in (t.float32, t.bfloat16):
            assert t.equal(dfd_p.encode_features_packed(storage, index=mb.index, dtype=dt), want.to(dt))
        batches += 1
    assert batches == -(-T * E // 100)
    for mb in buf_p.get(128):
        assert t.equal(mb.observations["packed"], storage.index_select(0, mb.index))


def test_misaligned_and_strided_rows_take_other_paths_with_equal_results():
    """mcbs_defender_wrapper_step_packed on a fused batch with packed_out off a 16-byte boundary takes the two-launch path, and rows
    further apart than W_def the word-by-word store side of the turn: the same rows, the same outputs, nothing outside the rows written."""
    from marlon_amd._abi import DefenderWrapperBuffers
    pairs = [_pair("toyctf", "packed") for _ in range(3)]
    t = pairs[0][0].torch
    dev, E = pairs[0][0].engine.device, 64
    W = pairs[0][1].observation_packing().words
    wides = [None, t.full((E, W + 3), -1, dtype=t.int32, device=dev), t.full((E, W + 4), -1, dtype=t.int32, device=dev)]
    views = [pairs[0][1].packed_observation, wides[1][:, 1:], wides[2][:, :W + 1]]
    assert views[1].data_ptr() % 16 == 4 and views[2].data_ptr() % 16 == 0 and views[2].stride(0) != W
    calls = [None]
    for (att, dfd), view in list(zip(pairs, views))[1:]:
        dfd._output_ring()
        calls.append([att.engine.defender_wrapper_step_packed_call(view, wb, dfd._wc) for _, wb, _, _ in dfd._ring])
        assert isinstance(dfd._ring[0][1], DefenderWrapperBuffers)
    rng = np.random.Generator(np.random.PCG64(13))
    for step in range(6):
        a = pairs[0][0].sample_uniform(seed=9, step=step).actions
        for att, _ in pairs:
            att.step(a)
        da = t.as_tensor((rng.random((E, 12)) * pairs[0][1].nvec).astype(np.int64), device=dev)
        _, r0, t0, u0, i0 = pairs[0][1].step(da)
        for k in (1, 2):
            dfd = pairs[k][1]
            calls[k][step % 2](da.data_ptr())
            o = dfd._ring[step % 2][0]
            assert t.equal(views[k][:, :W], pairs[0][1].packed_observation), f"step {step} path {k} rows"
            assert t.equal(o["reward"].view(t.int64), r0.view(t.int64)) and t.equal(o["terminated"], t0) and t.equal(o["truncated"], u0)
            assert t.equal(o["valid"], i0["valid_action"].view(t.uint8)) and t.equal(o["availability"].view(t.int64), i0["network_availability"].view(t.int64))
            assert t.equal(dfd.valid_action_count, pairs[0][1].valid_action_count) and t.equal(dfd.timesteps, pairs[0][1].timesteps)
    assert (wides[1][:, 0] == -1).all() and (wides[1][:, W + 1:] == -1).all() and (wides[2][:, W:] == -1).all()


def test_refusals():
    import ctypes as C
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.engine import McbsError
    from marlon_amd.wrappers import AttackerVecEnv, DefenderVecEnv, TwoAgentTrainVecEnv, TwoAgentVecEnv
    from tests import parity
    from tests.test_gpu_multicategorical import _toyctf_pair
    # a batch without a learned defender: no words, every call MCBS_EINVAL
    plain = AttackerVecEnv(parity.topology_for("toyctf"), 64, maximum_node_count=12, maximum_total_credentials=10,
                           attacker_goal=ce.AttackerGoal(own_atleast=6), max_timesteps=50)
    t, eng = plain.torch, plain.engine
    dev = eng.device
    assert eng.defender_obs_words() == 0 and eng.defender_wrapper_step_packed_launches() == 0
    rows = t.zeros((64, 8), dtype=t.int32, device=dev)
    for call in (lambda: eng.defender_observe_packed(out=rows), lambda: eng.unpack_defender_observation(rows),
                 lambda: eng.encode_defender_features(packed=rows)):
        with pytest.raises(McbsError, match=r"\(-1\).*MCBS_DEFENDER_EXTERNAL"):
            call()
    plain.close()

    att, dfd = _pair("toyctf", "packed")
    eng, lib = att.engine, att.engine.lib
    W, F = eng.defender_obs_words(), dfd.feature_width
    assert (W, F) == (5, 143)
    good = t.zeros((64, W), dtype=t.int32, device=dev)
    before = dfd.packed_observation.clone()
    # rows shorter than W_def: refused by the binding's checks, and by the library itself
    for call in (lambda: eng.defender_observe_packed(out=good[:, :W - 1]), lambda: eng.unpack_defender_observation(good[:, :W - 1]),
                 lambda: eng.encode_defender_features(packed=good[:, :W - 1]), lambda: dfd.observation_packed(out=good[:, :W - 1]),
                 lambda: eng.defender_wrapper_step_packed_call(good[:, :W - 1], None, None)):
        with pytest.raises(ValueError, match=f">= {W}"):
            call()
    st = eng._stream()
    assert lib.mcbs_defender_observe_packed(eng._h, good.data_ptr(), W - 1, st) == -1 and b"row_words 4 is shorter than the 5 words" in lib.mcbs_last_error()
    feats = t.zeros((64, F), device=dev)
    assert lib.mcbs_encode_defender_features(eng._h, None, good.data_ptr(), W, None, 64, 64, feats.data_ptr(), F - 1, 0, None, st) == -1
    assert b"out_row_stride" in lib.mcbs_last_error()
    assert lib.mcbs_encode_defender_features(eng._h, None, good.data_ptr(), W, None, 64, 64, feats.data_ptr(), F, 3, None, st) == -1
    assert b"dtype" in lib.mcbs_last_error()
    assert lib.mcbs_encode_defender_features(eng._h, None, None, W, None, 64, 64, feats.data_ptr(), F, 0, None, st) == -1 and b"exactly one" in lib.mcbs_last_error()
    assert lib.mcbs_encode_defender_features(eng._h, None, good.data_ptr(), W, None, 64, 65, feats.data_ptr(), F, 0, None, st) == -1
    assert b"no index" in lib.mcbs_last_error()
    assert lib.mcbs_unpack_defender_observation(eng._h, good.data_ptr(), W, None, 64, 65, C.byref(eng._defender_dense({}, "out", 65, partial=True)[0]), st) == -1
    assert b"no index" in lib.mcbs_last_error()
    # a wrong dtype or device
    for bad in (t.zeros((64, W), dtype=t.int64, device=dev), t.zeros((64, W), dtype=t.float32, device=dev), t.zeros((64, W), dtype=t.int32),
                t.zeros((63, W), dtype=t.int32, device=dev), t.zeros((64, 2 * W), dtype=t.int32, device=dev)[:, ::2]):
        with pytest.raises(ValueError, match="out must be a device int32 tensor"):
            eng.defender_observe_packed(out=bad)
        with pytest.raises(ValueError, match="out must be a device int32 tensor"):
            dfd.observation_packed(out=bad)
    with pytest.raises(ValueError, match="int64"):
        dfd.encode_features_packed(good, index=t.zeros(4, dtype=t.int32, device=dev))
    with pytest.raises(ValueError, match="float32, bfloat16 or float16"):
        dfd.encode_features_packed(good, dtype=t.float64)
    with pytest.raises(ValueError, match="out must be"):
        dfd.encode_features_packed(good, out=t.zeros((64, F - 1), device=dev))
    with pytest.raises(ValueError, match="bad_rows"):
        dfd.encode_features_packed(good, bad_rows=t.zeros(1, dtype=t.int64, device=dev))
    with pytest.raises(ValueError, match="exactly one"):
        eng.encode_defender_features()
    with pytest.raises(ValueError, match="four int8 fields"):
        eng.pack_defender_observation({"infected_nodes": t.zeros((64, 10), dtype=t.int8, device=dev)})
    with pytest.raises(ValueError, match="observation_format"):
        DefenderVecEnv(att, observation_format="bits")
    # the rollout buffer of a packed wrapper stores packed rows only
    with pytest.raises(ValueError, match="pack_observations=False"):
        dfd.rollout_buffer(4, pack_observations=False)
    assert dfd.rollout_buffer(4, store_observations=False).observations is None
    assert t.equal(dfd.packed_observation, before), "a refused call wrote rows"
    # the two-agent turns write the dense form only
    att_j, _ = _toyctf_pair(64, auto_reset=False, materialize_masks=False)
    assert TwoAgentVecEnv.supported(att_j)
    with pytest.raises(ValueError, match="TwoAgentVecEnv: .*observation_format='dense'"):
        TwoAgentVecEnv(att_j, DefenderVecEnv(att_j, observation_format="packed"))
    att_t, _ = _toyctf_pair(64, auto_reset=True, materialize_masks=False)
    assert TwoAgentTrainVecEnv.supported(att_t)
    with pytest.raises(ValueError, match="TwoAgentTrainVecEnv: .*observation_format='dense'"):
        TwoAgentTrainVecEnv(att_t, DefenderVecEnv(att_t, observation_format="packed"))
