"""The two-agent training turn with BOTH observations written as packed rows (mcbs_two_agent_train_step_packed,
two_agent_train_packed_kernel in marlon_amd/csrc/mcbs_two_agent.hip; `TwoAgentTrainVecEnv` on a pair of observation_format="packed"
wrappers).  Everything is compared bit for bit.

* lock-step with the dense training turn (itself held to the reference's traces and to the composition by
  tests/test_gpu_two_agent_training.py), at that file's two parameter sets and with its action recipe;
* replay of the reference's four recorded training loops, observations compared in the packed domain;
* `collect_rollouts` with packed buffers: a packed pair (row copies) against a dense pair (pack launches);
* write discipline and refusals of the C entry point; the consumers of the wrappers' state; a closed engine."""
import ctypes as C
import json
import os
import zlib

import numpy as np
import pytest

from tests import parity
from tests.test_gpu_two_agent import assert_same, assert_same_state, bits, defender_actions, md_rows, same_state
from tests.test_gpu_two_agent_training import (CASES, DKEYS, OBS, TRACES, all_rows, attacker_side, defender_side, lockstep_goal, make_pair)

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


def make_packed_pair(topo, E, nodes, creds, discrete, att_T, def_T, **kw):
    """make_pair with both wrappers in packed mode (its own dense DefenderVecEnv is dropped)"""
    from marlon_amd.wrappers import DefenderVecEnv
    att, _ = make_pair(topo, E, nodes, creds, discrete, att_T, def_T, observation_format="packed", **kw)
    return att, DefenderVecEnv(att, max_timesteps=def_T, invalid_action_reward=-1, loss_reward=-5000.0, observation_format="packed")


def u32(x):
    """a device int32 tensor of packed rows, or a host array of them, as uint32 on the host"""
    a = x if isinstance(x, np.ndarray) else x.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a.astype(np.uint32)


def host_fields(fields):
    return {k: v.cpu().numpy() for k, v in fields.items()}


COUNTERS_A = ("timesteps", "valid_action_count", "invalid_action_count", "episode_returns", "last_cyber_reward", "has_cyber_reward")
COUNTERS_D = ("timesteps", "valid_action_count", "invalid_action_count", "has_breached_sla", "prev_availability")


def counters(att, dfd, train):
    s = {"request": train.attacker_reset_request, "defender_return": train.defender_returns}
    s.update({"a." + k: getattr(att, k) for k in COUNTERS_A})
    s.update({"d." + k: getattr(dfd, k) for k in COUNTERS_D})
    return {k: bits(v) for k, v in s.items()}


def packed_lockstep(topo, E, nodes, creds, discrete, turns, att_T, def_T, seed, state_turns, **kw):
    """Pair A: TwoAgentTrainVecEnv on fields / dense wrappers.  Pair B: the same on packed / packed wrappers.  The action recipe of
    tests/test_gpu_two_agent_training.py lockstep(), the masked-valid actions drawn from pair A.  -> the cases pair A saw."""
    import torch as t
    from marlon_amd.wrappers import TwoAgentTrainVecEnv
    att_a, dfd_a = make_pair(topo, E, nodes, creds, discrete, att_T, def_T, **kw)
    att_b, dfd_b = make_packed_pair(topo, E, nodes, creds, discrete, att_T, def_T, **kw)
    assert TwoAgentTrainVecEnv.supported(att_b) and att_b.engine.two_agent_train_step_packed_launches(att_b._packing_handle()) == 1
    ta, tb = TwoAgentTrainVecEnv(att_a, dfd_a), TwoAgentTrainVecEnv(att_b, dfd_b)
    assert set(tb.terminal_observation) == {"packed"} and set(att_b.terminal_observation) == {"packed"}
    pk, dpk = att_a.observation_packing(), dfd_a.observation_packing()
    W, Wd = pk.words, dpk.words
    assert att_b.packed_observation.shape == (E, W) and dfd_b.packed_observation.shape == (E, Wd)
    rng = np.random.default_rng(seed)
    N, dev = att_a.topo.n_nodes, att_a.engine.device
    assert_same_state(att_a, att_b, f"{topo}: after both resets")
    np.testing.assert_array_equal(u32(att_a.observation_packed()), u32(att_b.packed_observation), err_msg="first attacker rows")
    np.testing.assert_array_equal(dpk.pack_host(host_fields(dfd_a.observation)), u32(dfd_b.packed_observation), err_msg="first defender rows")
    seen = dict.fromkeys(CASES, 0)
    seen.update(attacker_terminal_rows=0, defender_terminal_rows=0, stale_rows=0)
    for turn in range(1, turns + 1):
        ctx = f"{topo} E={E} turn {turn}"
        if turn % 2 == 1:                                                  # uniformly random indices: mostly intercepted
            a1 = (rng.random(att_a._action_shape) * (att_a.discrete_n if discrete else att_a.nvec)).astype(np.int64)
        elif discrete:                                                     # masked-valid ones, under the mask the attacker holds (a stale one included)
            a1 = att_a.sample_masked_uniform(seed=seed, step=turn).actions.cpu().numpy()
        else:
            a1 = md_rows(att_a.engine.sample_actions(valid=True, seed=seed, step=turn).cpu().numpy().astype(np.int64))
        a2 = defender_actions(rng, dfd_a, N)
        a1_d, a2_d = t.as_tensor(a1, device=dev), t.as_tensor(a2, device=dev)
        q = ta.attacker_reset_request.cpu().numpy()
        live_before = u32(att_b.packed_observation).copy()
        out_a, dout_a = ta.step(a1_d.clone(), a2_d.clone())
        a2_keep = a2_d.clone()
        out_b, dout_b = tb.step(a1_d, a2_d)
        assert t.equal(a2_d, a2_keep), f"{ctx}: the packed training turn modified the defender's actions"
        assert set(out_b[0]) == {"packed"} and out_b[0]["packed"] is att_b.packed_observation and dout_b[0]["packed"] is dfd_b.packed_observation
        A, D = attacker_side(att_a, out_a, out_a[4]), defender_side(dfd_a, dout_a, dout_a[4])
        assert_same({k: bits(v) for k, v in A.items()}, {k: bits(v) for k, v in attacker_side(att_b, out_b, out_b[4]).items()}, ctx + " attacker")
        assert_same({k: bits(v) for k, v in D.items()}, {k: bits(v) for k, v in defender_side(dfd_b, dout_b, dout_b[4]).items()}, ctx + " defender")
        assert_same(counters(att_a, dfd_a, ta), counters(att_b, dfd_b, tb), ctx + " counters")
        if discrete:                                                       # the digests, through the mask they give: stale after a defender-side reset
            np.testing.assert_array_equal(bits(att_a.action_masks_packed()), bits(att_b.action_masks_packed()), err_msg=ctx + ": packed action masks")
        done1, done2 = A["dones"].cpu().numpy() != 0, D["dones"].cpu().numpy() != 0
        invalid = A["invalid_action"].cpu().numpy() != 0
        # the attacker's rows: live rows of every env, terminal rows of the envs its step ended
        live_b = u32(att_b.packed_observation)
        np.testing.assert_array_equal(u32(att_a.observation_packed()), live_b, err_msg=ctx + ": attacker live rows")
        term_a = att_a.engine.pack_observation(att_a._packing_handle(), {k: att_a._terminal[k] for k in OBS})
        np.testing.assert_array_equal(u32(term_a)[done1], u32(att_b.terminal_packed_observation)[done1], err_msg=ctx + ": attacker terminal rows")
        stands = invalid & ~done1                                          # intercepted, not ended: the row stands (a stale one too)
        np.testing.assert_array_equal(live_b[stands], live_before[stands], err_msg=ctx + ": a row that stands was rewritten")
        # the defender's rows: live rows of every env, terminal rows of the envs the defender ended
        np.testing.assert_array_equal(dpk.pack_host(host_fields(dfd_a.observation)), u32(dfd_b.packed_observation), err_msg=ctx + ": defender live rows")
        np.testing.assert_array_equal(dpk.pack_host(host_fields(ta.terminal_observation))[done2], u32(tb.terminal_observation["packed"])[done2],
                                      err_msg=ctx + ": defender terminal rows")
        if turn in state_turns:
            assert_same_state(att_a, att_b, ctx)
            np.testing.assert_array_equal(pk.pack_host(host_fields(att_a.observation_fields)), live_b, err_msg=ctx + ": host pack of the attacker's fields")
        # the cases, counted on pair A's side as tests/test_gpu_two_agent_training.py counts them
        term1, term2 = A["terminated"].cpu().numpy() != 0, D["terminated"].cpu().numpy() != 0
        own_timeout = A["episode_length"].cpu().numpy() >= att_T
        n = done1 & ~q
        seen["attacker_goal"] += int(term1.sum())
        seen["attacker_timeout"] += int((own_timeout & ~term1).sum())
        seen["attacker_request"] += int((q & ~term1 & ~own_timeout).sum())
        seen["intercepted_request"] += int((q & invalid).sum())
        seen["defender_request"] += int(n.sum())
        seen["defender_breach"] += int((term2 & D["sla_breached"].cpu().numpy()).sum())
        seen["defender_timeout"] += int((~n & ~term2 & (D["episode_length"].cpu().numpy() >= def_T)).sum())
        seen["attacker_terminal_rows"] += int(done1.sum())
        seen["defender_terminal_rows"] += int(done2.sum())
        seen["stale_rows"] += int(ta.attacker_reset_request.sum())
    att_a.close()
    att_b.close()
    return seen


def test_lockstep_with_the_dense_turn_toyctf_discrete():
    """E = 200: four workgroups, the last with 8 envs; 150 turns, both timeouts at 8, the goal that lets attacker steps terminate.  Every
    case of the hand-shake occurs on the dense pair's side (the existing lock-step asserts the same counts at these parameters)."""
    seen = packed_lockstep("toyctf", 200, 12, 10, True, turns=150, att_T=8, def_T=8, seed=0, state_turns=(1, 9, 25, 150), **lockstep_goal())
    print(seen)
    for case in CASES:
        assert seen[case] > 0, f"the run never showed the case `{case}`: {seen}"
    assert seen["stale_rows"] > 0 and seen["attacker_terminal_rows"] > 0 and seen["defender_terminal_rows"] > 0


def test_lockstep_with_the_dense_turn_chain10_multidiscrete():
    """Other row sizes (W_obs = 18 words, W_def = 6), the MultiDiscrete decode, timeouts 12 / 10.  `attacker_timeout` cannot
    occur here: the defender's timeout (or the attacker's goal) always resets the attacker's clock before it reaches 12."""
    seen = packed_lockstep("chain10", 200, 12, 12, False, turns=150, att_T=12, def_T=10, seed=0, state_turns=(1, 9, 25, 150), **lockstep_goal())
    print(seen)
    for case in CASES:
        if case == "attacker_timeout":
            continue
        assert seen[case] > 0, f"the run never showed the case `{case}`: {seen}"
    assert seen["stale_rows"] > 0


@pytest.mark.parametrize("E", [1, 130])
@pytest.mark.parametrize("name", TRACES)
def test_replay_of_the_reference_training_loops_in_packed_rows(name, E):
    """tests/test_gpu_two_agent_training.py's replay through a packed pair: rewards, flags, counters and infos as there; every observation
    as pack_host of the trace's row against the packed live, terminal and fresh row (the clamp rule applies to both sides alike)."""
    import torch as t
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.wrappers import TwoAgentTrainVecEnv
    z = np.load(os.path.join(parity.GOLDEN, name + ".npz"))
    sj = json.loads(bytes(z["spec_json"]).decode())
    att, dfd = make_packed_pair("toyctf", E, 12, 10, sj["discrete"], sj["max_timesteps"], sj["defender_max_timesteps"],
                                goal=ce.AttackerGoal(**sj["attacker_goal"]))
    train = TwoAgentTrainVecEnv(att, dfd)
    train.reset()
    dev = att.engine.device
    pk, dpk = att.observation_packing(), dfd.observation_packing()

    def a_row(prefix, i=None):
        return pk.pack_host({k: np.asarray(z[prefix + k] if i is None else z[prefix + k][i]).reshape(1, -1) for k in OBS}).view(np.int32)

    def d_row(prefix, i=None):
        return dpk.pack_host({k: np.asarray(z[prefix + k] if i is None else z[prefix + k][i]).reshape(1, -1) for k in DKEYS}).view(np.int32)
    first_a, first_d = a_row("first_a_"), d_row("first_d_")
    all_rows(att.packed_observation, first_a, f"{name}: first attacker row")
    all_rows(dfd.packed_observation, first_d, f"{name}: first defender row")
    T = len(z["a_reward"])
    shape_a = (E,) if sj["discrete"] else (E, 10)
    last = dict(a_valid=np.zeros(E, np.int64), a_invalid=np.zeros(E, np.int64), d_valid=np.zeros(E, np.int64), d_invalid=np.zeros(E, np.int64))
    stale_masks = 0
    for i in range(T):
        ctx = f"{name} E={E} turn {i}"
        all_rows(train.attacker_reset_request, z["a_request"][i] != 0, ctx + ": reset_request before the attacker's step")
        if sj["discrete"]:                                         # the mask the reference's policy saw: stale after a defender-side reset
            packed = att.action_masks_packed()
            assert bool((packed == packed[0:1]).all()), ctx + ": packed masks differ between envs"
            m = att.unpack_action_mask(packed[0:1])[0].cpu().numpy().astype(np.int8)
            assert (zlib.crc32(m.tobytes()), int(m.sum())) == (int(z["a_mask_crc_before"][i]), int(z["a_mask_sum_before"][i])), ctx + ": action mask"
            stale_masks += int(z["a_request"][i])
        a1 = t.as_tensor(np.broadcast_to(z["a_action"][i], shape_a).copy(), device=dev)
        a2 = t.as_tensor(np.broadcast_to(z["d_action"][i], (E, 12)).copy(), device=dev)
        (o, r1, term1, trunc1, info), (do, r2, term2, trunc2, dinfo) = train.step(a1, a2)
        all_rows(r1, np.float32(z["a_reward"][i]), ctx + ": attacker reward")
        all_rows(term1, z["a_terminated"][i], ctx + ": attacker terminated")
        all_rows(trunc1, z["a_truncated"][i], ctx + ": attacker truncated")
        all_rows(info["invalid_action"], z["a_invalid"][i] != 0, ctx + ": invalid_action")
        done1 = bool(z["a_terminated"][i] or z["a_truncated"][i])
        all_rows(info["dones"], done1, ctx + ": attacker dones")
        all_rows(att.terminal_packed_observation if done1 else o["packed"], a_row("a_", i), ctx + ": attacker row")
        if done1:
            all_rows(o["packed"], first_a, ctx + ": fresh attacker row")
        all_rows(r2, np.float64(z["d_reward"][i]), ctx + ": defender reward")
        all_rows(term2, z["d_terminated"][i], ctx + ": defender terminated")
        all_rows(trunc2, z["d_truncated"][i], ctx + ": defender truncated")
        all_rows(dinfo["valid_action"], z["d_valid"][i] != 0, ctx + ": defender valid_action")
        all_rows(dinfo["network_availability"], np.float64(z["d_availability"][i]), ctx + ": availability")
        done2 = bool(z["d_terminated"][i] or z["d_truncated"][i])
        all_rows(dinfo["dones"], done2, ctx + ": defender dones")
        all_rows(train.terminal_observation["packed"] if done2 else do["packed"], d_row("d_", i), ctx + ": defender row")
        if done2:
            all_rows(do["packed"], first_d, ctx + ": fresh defender row")
        for x, k in ((att.timesteps, "a_timesteps"), (att.valid_action_count, "a_valid_count"), (att.invalid_action_count, "a_invalid_count"),
                     (dfd.timesteps, "d_timesteps"), (dfd.valid_action_count, "d_valid_count"), (dfd.invalid_action_count, "d_invalid_count")):
            all_rows(x, z[k][i], f"{ctx}: {k} after the turn")
        if done1:
            last["a_valid"], last["a_invalid"] = info["episode_valid_actions"].cpu().numpy(), info["episode_invalid_actions"].cpu().numpy()
        if done2:
            last["d_valid"], last["d_invalid"] = dinfo["episode_valid_actions"].cpu().numpy(), dinfo["episode_invalid_actions"].cpu().numpy()
        for k, rec in (("a_valid", "a_last_valid"), ("a_invalid", "a_last_invalid"), ("d_valid", "d_last_valid"), ("d_invalid", "d_last_invalid")):
            assert (last[k] == z[rec][i]).all(), f"{ctx}: {rec}"
    if sj["discrete"]:
        assert stale_masks >= 10, "the Discrete trace never asked for a mask after a defender-side reset"
    att.close()


def test_collect_rollouts_packed_pair_against_dense_pair_with_pack_launches():
    """64 envs x 8 steps, timeouts at 3 and 5, two consecutive rollouts into rollout_buffer(8, pack_observations=True) buffers: the packed
    pair (whose observation_packed(out=) is a row copy) against the dense pair (whose rows come from the pack launches)."""
    import torch as t
    from marlon_amd.simulate import collect_rollouts
    from marlon_amd.wrappers import TwoAgentTrainVecEnv
    E, T = 64, 8
    pairs = [make_pair("toyctf", E, 12, 10, True, 3, 5), make_packed_pair("toyctf", E, 12, 10, True, 3, 5)]
    trains = [TwoAgentTrainVecEnv(a, d) for a, d in pairs]
    bufs = [(a.rollout_buffer(T, pack_observations=True), d.rollout_buffer(T, pack_observations=True)) for a, d in pairs]
    for ba, bd in bufs:
        assert set(ba.observations) == {"packed"} and set(bd.observations) == {"packed"}
    dev = pairs[0][0].engine.device

    def policies():
        step = {"a": 0, "d": 0}

        def pa(env):
            step["a"] += 1
            out = env.sample_masked_uniform(seed=11, step=step["a"])
            return out.actions, out.entropy, out.log_prob              # (the entropy stands in for a value head)

        def pd(env):
            step["d"] += 1
            out = env.sample_uniform(seed=12, step=step["d"])
            return out.actions, out.entropy, out.log_prob
        return pa, pd
    for rollout in range(2):                                           # twice: episode_starts are carried from one call to the next
        dones = [collect_rollouts(train, *policies(), ba, bd, T) for train, (ba, bd) in zip(trains, bufs)]
        for i, who in ((0, "attacker"), (1, "defender")):
            want, got = bufs[0][i], bufs[1][i]
            assert got.full and want.full
            for k in ("actions", "rewards", "values", "log_probs", "episode_starts"):
                np.testing.assert_array_equal(bits(getattr(want, k)), bits(getattr(got, k)), err_msg=f"rollout {rollout} {who} {k}")
            np.testing.assert_array_equal(bits(want.observations["packed"]), bits(got.observations["packed"]), err_msg=f"rollout {rollout} {who} rows")
            np.testing.assert_array_equal(bits(dones[0][i]), bits(dones[1][i]), err_msg=f"rollout {rollout} {who} dones")
            assert int(got.episode_starts.sum()) > E, "no episode ended inside the rollout"
        np.testing.assert_array_equal(bits(bufs[0][0].mask_bits), bits(bufs[1][0].mask_bits), err_msg=f"rollout {rollout} mask bits")
        lv = t.zeros(E, device=dev)
        for i in (0, 1):
            bufs[1][i].compute_returns_and_advantage(lv, dones[1][i])
    for a, _ in pairs:
        a.close()


# ---- the C entry point: write discipline and refusals ----
def raw_packed_call(att, request=None, actions=None, **change):
    """mcbs_two_agent_train_step_packed through ctypes on rows allocated here: attacker rows of W_obs + 3 words, defender rows of W_def
    rounded up to a multiple of 4, plus 4, every word prefilled with SENTINEL but the live attacker rows' first W_obs, which hold the
    rows that stand (sentinel_live: those too).  change: what a refusal case alters, or other row strides.
    -> (return code, message, the arrays)"""
    import torch as t
    from marlon_amd._abi import TRAINING_PACKED_FIELDS, DefenderWrapperBuffers, DefenderWrapperCfg, training_packed_buffers
    eng = att.engine
    E, dev = att.num_envs, eng.device
    handle = change.get("packing", att._packing_handle())
    W, Wd = att._packing_handle().words, eng.defender_obs_words()
    rw, drw = change.get("row_words", W + 3), change.get("defender_row_words", (Wd + 3) // 4 * 4 + 4)
    _, wb, _ = att._next_output_set()

    def sentinel_rows(width):                                              # [E, width] in a buffer with four spare words behind
        flat = t.full((E * width + 4,), SENTINEL, dtype=t.int32, device=dev)
        return flat, flat[:E * width].view(E, width)
    flats, rows = {}, {}
    for k, width in (("packed", max(rw, W)), ("packed_terminal", max(rw, W)), ("defender_packed", max(drw, Wd)), ("terminal_defender_packed", max(drw, Wd))):
        flats[k], rows[k] = sentinel_rows(width)
    if not change.get("sentinel_live"):
        rows["packed"][:, :W] = att.observation_packed()[:, :W]
    fresh = att.observation_packed()[0:1, :W].clone()
    dfresh = eng.defender_observe_packed()[0:1].clone()
    mk = lambda dt: t.zeros(E, dtype=dt, device=dev)
    dts = (t.uint8, t.float64, t.uint8, t.uint8, t.float32, t.int32, t.int64, t.int64, t.uint8, t.float64, t.float64, t.uint8, t.uint8, t.uint8, t.uint8)
    dbuf = [mk(dt) for dt in dts]
    dbuf[9].fill_(1.0)                                                     # prev_availability of a fresh env
    dwb = DefenderWrapperBuffers(*[x.data_ptr() for x in dbuf])
    cfg = DefenderWrapperCfg(-1.0, -5000.0, 200.0, 0.6, 5000.0, 1, 40)
    tdt = dict(attacker_reset_request=t.uint8, defender_return=t.float64, attacker_valid_out=t.int64, attacker_invalid_out=t.int64,
               defender_return_out=t.float64, defender_length_out=t.int32, defender_valid_out=t.int64, defender_invalid_out=t.int64, defender_dones=t.uint8)
    arrays = {k: mk(dt) for k, dt in tdt.items()}
    if request is not None:
        arrays["attacker_reset_request"].copy_(t.as_tensor(request.astype(np.uint8), device=dev))
    ptr = {k: v.data_ptr() for k, v in arrays.items()}
    ptr.update(terminal_defender_packed=rows["terminal_defender_packed"].data_ptr(), fresh_defender_packed=dfresh.data_ptr())
    dpacked = rows["defender_packed"].data_ptr()
    if change.get("misalign") == "defender_packed":
        dpacked += 4
    if change.get("misalign") == "terminal_defender_packed":
        ptr["terminal_defender_packed"] += 4
    if change.get("alias") == "block":
        ptr["defender_dones"] = ptr["attacker_reset_request"]
    if change.get("alias") == "rows":
        ptr["terminal_defender_packed"] = dpacked
    if "missing" in change:
        ptr[change["missing"]] = None
    assert set(ptr) == set(TRAINING_PACKED_FIELDS)
    tb = training_packed_buffers(**ptr)
    a1 = t.zeros(att._action_shape, dtype=t.int64, device=dev) if actions is None else t.as_tensor(actions, device=dev)
    a2 = t.zeros((E, 12), dtype=t.int64, device=dev)
    a2[:, 0] = -1                                                          # the empty defender action
    p = a1.data_ptr()
    md, dc = (None, p) if att.discrete else (p, None)
    if "encodings" in change:
        md, dc = (p, p) if change["encodings"] == "both" else (None, None)
    terminal = rows["packed"] if change.get("alias") == "attacker rows" else rows["packed_terminal"]
    rc = eng.lib.mcbs_two_agent_train_step_packed(eng._h, md, dc, att._rows.data_ptr(), C.byref(eng._info_struct), handle.ptr, rows["packed"].data_ptr(),
                                                  terminal.data_ptr(), fresh.data_ptr(), rw, C.byref(wb), -1.0, 24, a2.data_ptr(), dpacked, drw,
                                                  C.byref(dwb), C.byref(cfg), C.byref(tb), None)
    t.cuda.synchronize(dev)
    rows.update(arrays, fresh=fresh, dfresh=dfresh, invalid=att._invalid, dones=att._dones, spare={k: v[-4:] for k, v in flats.items()})
    return rc, eng.lib.mcbs_last_error().decode(), rows


def test_write_discipline_and_refusals_of_the_entry_point():
    """E = 70 (two workgroups, the second with 6 envs), ToyCtf Discrete.  Every refusal returns -1 with its message and leaves the env
    state as it was; the same call with valid arguments then succeeds, and writes exactly the words it owns."""
    import torch as t
    from marlon_amd.wrappers import DefenderVecEnv, TwoAgentTrainVecEnv, TwoAgentVecEnv
    E = 70
    # a batch outside the scope (more cached credentials than the one-launch wrapper step takes)
    out, _ = make_pair("chain10", 64, 12, 20, False, 24, 40)
    before = out.engine.get_state()
    assert out.engine.two_agent_train_step_packed_launches(out._packing_handle()) == 0
    rc, msg, _ = raw_packed_call(out)
    assert rc == -1 and "one launch" in msg and same_state(before, out.engine.get_state())
    other, _ = make_pair("chain10", 64, 12, 12, False, 24, 40)
    att, _ = make_pair("toyctf", E, 12, 10, True, 24, 40)
    eng = att.engine
    W, Wd = att._packing_handle().words, eng.defender_obs_words()
    assert eng.two_agent_train_step_packed_launches(att._packing_handle()) == 1
    assert eng.two_agent_train_step_packed_launches(other._packing_handle()) == 0
    before = eng.get_state()
    odd = next(r for r in range(Wd + 1, Wd + 5) if r % 4)                   # longer than a row, neither W_def nor a multiple of 4
    refusals = [(dict(packing=other._packing_handle()), "another device or geometry"), (dict(row_words=W - 1), "shorter"),
                (dict(defender_row_words=Wd - 1), "shorter"), (dict(misalign="defender_packed"), "16-byte"),
                (dict(misalign="terminal_defender_packed"), "16-byte"), (dict(defender_row_words=odd), "multiple of 4"),
                (dict(missing="defender_dones"), "every array is required"), (dict(missing="fresh_defender_packed"), "every array is required"),
                (dict(encodings="both"), "exactly one action encoding"), (dict(encodings="neither"), "exactly one action encoding"),
                (dict(alias="block"), "overlaps"), (dict(alias="rows"), "overlaps"), (dict(alias="attacker rows"), "overlaps")]
    for change, word in refusals:
        rc, msg, _ = raw_packed_call(att, **change)
        assert rc == -1 and word in msg, (change, rc, msg)
        assert same_state(before, eng.get_state()), f"{change}: a refused call changed the env state"
    other.close()
    out.close()
    # the valid call: odd envs send an undiscovered node index (intercepted), every third env has been asked to reset (it ends)
    env = np.arange(E)
    intercepted, asked = env % 2 == 1, env % 3 == 0
    actions = np.where(intercepted, att.discrete_n - 1, 0).astype(np.int64)
    rc, msg, r = raw_packed_call(att, request=asked, actions=actions, sentinel_live=True)
    assert rc == 0, msg
    assert not same_state(before, eng.get_state())
    np.testing.assert_array_equal(r["invalid"].cpu().numpy() != 0, intercepted)
    np.testing.assert_array_equal(r["dones"].cpu().numpy() != 0, asked)
    live, term = u32(r["packed"]), u32(r["packed_terminal"])
    dlive, dterm = u32(r["defender_packed"]), u32(r["terminal_defender_packed"])
    assert live.shape == (E, W + 3) and dlive.shape == (E, (Wd + 3) // 4 * 4 + 4)
    for x, w, what in ((live, W, "packed"), (term, W, "packed_terminal"), (dlive, Wd, "defender_packed"), (dterm, Wd, "terminal_defender_packed")):
        assert (x[:, w:] == SENTINEL).all() and (u32(r["spare"][what]) == SENTINEL).all(), f"{what}: a word from W on was written"
    assert (term[~asked] == SENTINEL).all(), "a terminal row of an env that did not end was written"
    assert (live[intercepted & ~asked] == SENTINEL).all(), "the row of an intercepted env that did not end was written"
    np.testing.assert_array_equal(live[asked, :W], np.broadcast_to(u32(r["fresh"]), (int(asked.sum()), W)), err_msg="fresh rows of the envs that ended")
    assert (term[asked & intercepted, :W] == SENTINEL).all(), "an env that ended on an intercepted action: its terminal row is the live row that stood"
    assert (live[~intercepted & ~asked, :W] != SENTINEL).all(), "an env that stepped: every word of its row is stored"
    assert (term[asked & ~intercepted, :W] != SENTINEL).all(), "an env that stepped and ended: every word of its terminal row is stored"
    # the defender's rows: written for every env; where the defender did not end they are the rows of the state as it stands
    ddone = r["defender_dones"].cpu().numpy() != 0
    now = u32(eng.defender_observe_packed())
    np.testing.assert_array_equal(dterm[~ddone, :Wd], now[~ddone])
    np.testing.assert_array_equal(dlive[~ddone, :Wd], now[~ddone])
    np.testing.assert_array_equal(dlive[ddone, :Wd], np.broadcast_to(u32(r["dfresh"]), (int(ddone.sum()), Wd)))
    # the same with rows that follow each other without a gap (the defender's: 16-byte stores across rows of W_def = 5 words)
    rc, msg, r = raw_packed_call(att, row_words=W, defender_row_words=Wd)
    assert rc == 0, msg
    ddone = r["defender_dones"].cpu().numpy() != 0
    now = u32(eng.defender_observe_packed())
    assert r["defender_packed"].shape == (E, Wd) and r["packed"].shape == (E, W)
    np.testing.assert_array_equal(u32(r["defender_packed"])[~ddone], now[~ddone])
    np.testing.assert_array_equal(u32(r["terminal_defender_packed"])[~ddone], now[~ddone])
    for what, spare in r["spare"].items():
        assert (u32(spare) == SENTINEL).all(), f"{what}: a word behind the last row was written"
    att.close()
    # the wrappers: mixed pairs stay refused, and so does the joint turn
    att, dfd = make_pair("toyctf", 64, 12, 10, True, 24, 40)
    with pytest.raises(ValueError, match="TwoAgentTrainVecEnv: .*observation_format='dense'"):
        TwoAgentTrainVecEnv(att, DefenderVecEnv(att, observation_format="packed"))
    TwoAgentTrainVecEnv(att, dfd)
    att.close()
    att, dfd = make_pair("toyctf", 64, 12, 10, True, 24, 40, observation_format="packed")
    assert TwoAgentTrainVecEnv.supported(att)
    with pytest.raises(ValueError, match="TwoAgentTrainVecEnv: .*observation_format"):
        TwoAgentTrainVecEnv(att, dfd)
    att.close()
    att, dfd = make_pair("toyctf", 64, 12, 10, True, 24, 40, auto_reset=False, observation_format="packed")
    assert not TwoAgentVecEnv.supported(att)
    with pytest.raises(ValueError, match="TwoAgentVecEnv: .*observation_format='fields'"):
        TwoAgentVecEnv(att, dfd)
    att.close()
    att, dfd = make_pair("toyctf", 64, 12, 10, True, 24, 40, auto_reset=False)
    with pytest.raises(ValueError, match="TwoAgentVecEnv: .*observation_format='dense'"):
        TwoAgentVecEnv(att, DefenderVecEnv(att, observation_format="packed"))
    att.close()


def test_consumers_after_a_defender_side_reset():
    """At the turns that follow a defender-side reset (the attacker holds the row of the episode that is gone) everything that reads the
    wrappers' persistent state gives the packed pair what it gives the dense pair."""
    import torch as t
    from marlon_amd.wrappers import TwoAgentTrainVecEnv
    E = 200
    att_a, dfd_a = make_pair("toyctf", E, 12, 10, True, 8, 5, **lockstep_goal())          # the defender's timeout first: it resets on its own
    att_b, dfd_b = make_packed_pair("toyctf", E, 12, 10, True, 8, 5, **lockstep_goal())
    ta, tb = TwoAgentTrainVecEnv(att_a, dfd_a), TwoAgentTrainVecEnv(att_b, dfd_b)
    rng = np.random.default_rng(3)
    dev = att_a.engine.device
    compared = 0
    for turn in range(1, 25):
        a1 = att_a.sample_masked_uniform(seed=5, step=turn).actions
        a2 = t.as_tensor(defender_actions(rng, dfd_a, att_a.topo.n_nodes), device=dev)
        ta.step(a1.clone(), a2.clone())
        tb.step(a1, a2)
        stale = int(ta.attacker_reset_request.sum())
        if not stale:
            continue
        assert t.equal(ta.attacker_reset_request, tb.attacker_reset_request)
        fa, fb = att_a.features(dtype=t.bfloat16), att_b.features(dtype=t.bfloat16)
        assert fa.shape == fb.shape and t.equal(fa.view(t.int16), fb.view(t.int16)), f"turn {turn}: att.features(bf16)"
        assert t.equal(dfd_a.features(), dfd_b.features()), f"turn {turn}: dfd.features()"
        assert t.equal(att_a.sample_masked_uniform(seed=9, step=turn).actions, att_b.sample_masked_uniform(seed=9, step=turn).actions), f"turn {turn}"
        compared += stale
    assert compared >= 10, "no turn followed a defender-side reset"
    att_a.close()
    att_b.close()


def test_bound_call_on_a_closed_engine():
    import torch as t
    from marlon_amd.engine import McbsError
    from marlon_amd.wrappers import TwoAgentTrainVecEnv
    att, dfd = make_packed_pair("toyctf", 64, 12, 10, True, 24, 40)
    train = TwoAgentTrainVecEnv(att, dfd)
    a1 = t.zeros(64, dtype=t.int64, device=att.engine.device)
    a2 = t.zeros((64, 12), dtype=t.int64, device=att.engine.device)
    train.step(a1, a2)
    call = att.engine.two_agent_train_step_packed_call(att.discrete, att._rows, att._packing_handle(), att.packed_observation,
                                                       att.terminal_packed_observation, att._packed_fresh, att._wb, -1.0, 24, dfd.packed_observation,
                                                       dfd._ring[0][1], dfd._wc, train._ring[0][1])
    call(a1.data_ptr(), a2.data_ptr())
    t.cuda.synchronize()
    clocks = [(x, x.clone()) for x in (att.timesteps, dfd.timesteps, att.packed_observation, dfd.packed_observation)]
    att.close()
    with pytest.raises(McbsError):
        call(a1.data_ptr(), a2.data_ptr())
    for bound in train._calls.values():
        with pytest.raises(McbsError):
            bound(a1.data_ptr(), a2.data_ptr())
    t.cuda.synchronize()
    for clock, was in clocks:
        assert t.equal(clock, was), "a call on a closed engine stepped a clock"
