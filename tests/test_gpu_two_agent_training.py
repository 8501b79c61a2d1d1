"""The two-agent TRAINING turn (mcbs_two_agent_train_step, two_agent_train_kernel in marlon_amd/csrc/mcbs_two_agent.hip;
`TwoAgentTrainVecEnv`, `simulate.collect_rollouts`): both wrappers' auto-resets and the reset_request hand-shake in one launch.
Everything is compared bit for bit (floats as their bits): the launch and what it is held to perform the same operations in the same order.

* replay: the reference's recorded training loops (tests/golden/wrap_training_*.npz) through `TwoAgentTrainVecEnv.step`, at E = 1 and at
  E = 130 (three workgroups, the last one partial).  A batch has ONE pair of max_timesteps and one action encoding, so the traces cannot
  be dealt over the envs of one batch: every env of a batch replays the batch's trace, and the lockstep below is what tells envs apart;
* lockstep against the composition from existing calls (tests/training_compose.py) with the numpy rules (tests/training_ref.py) run
  beside it, ToyCtf Discrete and Chain-10 MultiDiscrete, with a goal low enough that attacker steps terminate;
* refusals: nothing launched, state unchanged;  `collect_rollouts` against a hand-written loop over `step` + `add`."""
import ctypes as C
import json
import os
import zlib

import numpy as np
import pytest

from tests import parity
from tests.test_gpu_two_agent import assert_same, assert_same_state, bits, defender_actions, md_rows, same_state
from tests.training_compose import ComposedTrainingTurn
from tests.training_ref import TrainingBook

pytestmark = pytest.mark.gpu

TRACES = ["wrap_training_toyctf_s81", "wrap_training_toyctf_discrete_s82", "wrap_training_toyctf_s83", "wrap_training_toyctf_s84"]
OBS = ["leaked_credentials", "credential_cache_matrix", "discovered_nodes_properties", "nodes_privilegelevel", "scalars"]
DKEYS = ["infected_nodes", "incoming_firewall_status", "outgoing_firewall_status", "services_status"]


def make_pair(topo, E, nodes, creds, discrete, att_T, def_T, goal=None, seed=0, **kw):
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.wrappers import AttackerVecEnv, DefenderVecEnv
    args = dict(maximum_node_count=nodes, maximum_total_credentials=creds, attacker_goal=goal or ce.AttackerGoal(own_atleast=6),
                defender_constraint=ce.DefenderConstraint(maintain_sla=0.60), losing_reward=-5000.0, max_timesteps=att_T, auto_reset=True,
                learned_defender=True, materialize_masks=False, discrete=discrete, seed=seed)
    args.update(kw)
    att = AttackerVecEnv(parity.topology_for(topo), E, **args)
    dfd = DefenderVecEnv(att, max_timesteps=def_T, invalid_action_reward=-1, loss_reward=-5000.0) if args["learned_defender"] else None
    return att, dfd


def all_rows(x, want, ctx):
    """every env's row of the device tensor x equals `want` (the trace's value for this turn)"""
    got = bits(x)
    want = np.asarray(want)
    if want.dtype.kind == "f":
        want = want.astype(got.dtype.str.replace("i", "f")).view(got.dtype)
    np.testing.assert_array_equal(got.reshape(got.shape[0], -1), np.broadcast_to(want.reshape(1, -1), (got.shape[0], want.size)), err_msg=ctx)


@pytest.mark.parametrize("E", [1, 130])
@pytest.mark.parametrize("name", TRACES)
def test_replay_of_the_reference_training_loops(name, E):
    import torch as t
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.wrappers import TwoAgentTrainVecEnv
    z = np.load(os.path.join(parity.GOLDEN, name + ".npz"))
    sj = json.loads(bytes(z["spec_json"]).decode())
    att, dfd = make_pair("toyctf", E, 12, 10, sj["discrete"], sj["max_timesteps"], sj["defender_max_timesteps"],
                         goal=ce.AttackerGoal(**sj["attacker_goal"]))
    assert TwoAgentTrainVecEnv.supported(att) and att.engine.two_agent_train_step_launches() == 1
    train = TwoAgentTrainVecEnv(att, dfd)
    obs, dobs = train.reset()
    dev = att.engine.device
    for k in OBS:
        all_rows(att.observation_fields[k], z["first_a_" + k], f"{name}: first attacker observation, {k}")
    for k in DKEYS:
        all_rows(dobs[k], z["first_d_" + k], f"{name}: first defender observation, {k}")
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
        for k in OBS:                                              # an env that ended: terminal rows hold the step's observation, live rows the fresh one
            all_rows((att._terminal if done1 else att.observation_fields)[k], z["a_" + k][i], f"{ctx}: attacker observation {k}")
            if done1:
                all_rows(att.observation_fields[k], z["first_a_" + k], f"{ctx}: fresh attacker observation {k}")
        all_rows(r2, np.float64(z["d_reward"][i]), ctx + ": defender reward")
        all_rows(term2, z["d_terminated"][i], ctx + ": defender terminated")
        all_rows(trunc2, z["d_truncated"][i], ctx + ": defender truncated")
        all_rows(dinfo["valid_action"], z["d_valid"][i] != 0, ctx + ": defender valid_action")
        all_rows(dinfo["network_availability"], np.float64(z["d_availability"][i]), ctx + ": availability")
        done2 = bool(z["d_terminated"][i] or z["d_truncated"][i])
        all_rows(dinfo["dones"], done2, ctx + ": defender dones")
        for k in DKEYS:
            all_rows((train.terminal_observation if done2 else do)[k], z["d_" + k][i], f"{ctx}: defender observation {k}")
            if done2:
                all_rows(do[k], z["first_d_" + k], f"{ctx}: fresh defender observation {k}")
        for x, k in ((att.timesteps, "a_timesteps"), (att.valid_action_count, "a_valid_count"), (att.invalid_action_count, "a_invalid_count"),
                     (dfd.timesteps, "d_timesteps"), (dfd.valid_action_count, "d_valid_count"), (dfd.invalid_action_count, "d_invalid_count")):
            all_rows(x, z[k][i], f"{ctx}: {k} after the turn")
        # the counts of the episode that ended last (the wrappers' last_*_action_count), from the infos of the turns that ended one
        if done1:
            last["a_valid"], last["a_invalid"] = info["episode_valid_actions"].cpu().numpy(), info["episode_invalid_actions"].cpu().numpy()
        if done2:
            last["d_valid"], last["d_invalid"] = dinfo["episode_valid_actions"].cpu().numpy(), dinfo["episode_invalid_actions"].cpu().numpy()
        for k, rec in (("a_valid", "a_last_valid"), ("a_invalid", "a_last_invalid"), ("d_valid", "d_last_valid"), ("d_invalid", "d_last_invalid")):
            assert (last[k] == z[rec][i]).all(), f"{ctx}: {rec}"
    if sj["discrete"]:
        assert stale_masks >= 10, "the Discrete trace never asked for a mask after a defender-side reset"
    att.close()


def attacker_side(att, out, info):
    s = {"rewards": out[1], "terminated": out[2], "truncated": out[3], "decoded": att._rows}
    s.update({k: info[k] for k in ("dones", "invalid_action", "cyber_step_executed", "network_availability", "step_count", "episode_return",
                                   "episode_length", "episode_valid_actions", "episode_invalid_actions")})
    return s


def defender_side(dfd, out, dinfo):
    s = {"reward": out[1], "terminated": out[2], "truncated": out[3], "evicted": dfd._evicted}
    s.update({k: dinfo[k] for k in ("dones", "episode_return", "episode_length", "episode_valid_actions", "episode_invalid_actions", "valid_action",
                                    "network_availability", "sla_breached", "defender_won")})
    return s


def wrapper_state(att, dfd, request, dret, mask):
    s = {"request": request, "defender_return": dret, "a.mask": mask}
    s.update({"a.obs." + k: v for k, v in att.observation_fields.items()})
    for k in ("timesteps", "valid_action_count", "invalid_action_count", "episode_returns", "last_cyber_reward", "has_cyber_reward"):
        s["a.counter." + k] = getattr(att, k)
    s.update({"d.obs." + k: v for k, v in dfd.observation.items()})
    for k in ("timesteps", "valid_action_count", "invalid_action_count", "has_breached_sla", "prev_availability"):
        s["d.counter." + k] = getattr(dfd, k)
    return s


def lockstep(topo, E, nodes, creds, discrete, turns, att_T, def_T, goal, seed, state_turns=(), **kw):
    """Pair A: the composition from existing calls, with the numpy rules beside it.  Pair B: TwoAgentTrainVecEnv.step.  -> the cases pair A saw."""
    import torch as t
    from marlon_amd.wrappers import TwoAgentTrainVecEnv
    att_a, dfd_a = make_pair(topo, E, nodes, creds, discrete, att_T, def_T, goal=goal, **kw)
    att_b, dfd_b = make_pair(topo, E, nodes, creds, discrete, att_T, def_T, goal=goal, **kw)
    comp = ComposedTrainingTurn(att_a, dfd_a)
    train = TwoAgentTrainVecEnv(att_b, dfd_b)
    book = TrainingBook(E, att_T, def_T)
    rng = np.random.default_rng(seed)
    N, dev = att_a.topo.n_nodes, att_a.engine.device
    episode0 = att_b.engine.get_state()[0]["episode"].astype(np.int64)
    assert_same_state(att_a, att_b, f"{topo}: after both resets")
    seen = dict(attacker_goal=0, attacker_timeout=0, attacker_request=0, defender_breach=0, defender_timeout=0, defender_request=0,
                intercepted_request=0, attacker_terminal_rows=0, defender_terminal_rows=0)
    for turn in range(1, turns + 1):
        ctx = f"{topo} E={E} turn {turn}"
        if turn % 2 == 1:                                                  # uniformly random indices: mostly intercepted
            a1 = (rng.random(att_b._action_shape) * (att_b.discrete_n if discrete else att_b.nvec)).astype(np.int64)
        elif discrete:                                                     # masked-valid ones, under the mask the attacker holds (a stale one included)
            a1 = att_b.sample_masked_uniform(seed=seed, step=turn).actions.cpu().numpy()
        else:
            a1 = md_rows(att_b.engine.sample_actions(valid=True, seed=seed, step=turn).cpu().numpy().astype(np.int64))
        a2 = defender_actions(rng, dfd_a, N)
        a1_d, a2_d = t.as_tensor(a1, device=dev), t.as_tensor(a2, device=dev)
        q = comp.request.cpu().numpy()
        A, D = comp.step(a1_d.clone(), a2_d.clone())
        a2_keep = a2_d.clone()
        out_b, dout_b = train.step(a1_d, a2_d)
        assert t.equal(a2_d, a2_keep), f"{ctx}: the training turn modified the defender's actions"
        got_a, got_d = attacker_side(att_b, out_b, out_b[4]), defender_side(dfd_b, dout_b, dout_b[4])
        assert_same({k: bits(A[k]) for k in got_a}, {k: bits(v) for k, v in got_a.items()}, ctx + " attacker")
        assert_same({k: bits(D[k]) for k in got_d}, {k: bits(v) for k, v in got_d.items()}, ctx + " defender")
        assert_same({k: bits(v) for k, v in wrapper_state(att_a, dfd_a, comp.request, comp.defender_returns, comp.mask).items()},
                    {k: bits(v) for k, v in wrapper_state(att_b, dfd_b, train.attacker_reset_request, train.defender_returns,
                                                         att_b.action_masks_packed()).items()}, ctx + " state")
        done1, done2 = A["dones"].cpu().numpy() != 0, D["dones"].cpu().numpy() != 0
        for k in att_a._terminal:                                          # terminal observations, where an episode ended
            np.testing.assert_array_equal(bits(att_a._terminal[k])[done1], bits(att_b._terminal[k])[done1], err_msg=f"{ctx}: attacker terminal {k}")
        for k in comp.terminal:
            np.testing.assert_array_equal(bits(comp.terminal[k])[done2], bits(train.terminal_observation[k])[done2], err_msg=f"{ctx}: defender terminal {k}")
        if turn in state_turns:
            assert_same_state(att_a, att_b, ctx)
        # the numpy rules, fed what the existing calls computed
        term1, invalid = A["terminated"].cpu().numpy() != 0, A["invalid_action"].cpu().numpy()
        ra = book.attacker(A["rewards"].cpu().numpy(), term1, invalid)
        np.testing.assert_array_equal(ra["requested"], q, err_msg=ctx + ": request byte")
        for k in ("truncated", "dones", "episode_valid_actions", "episode_invalid_actions", "episode_length"):
            np.testing.assert_array_equal(ra[k].astype(np.int64), A[k].cpu().numpy().astype(np.int64), err_msg=f"{ctx}: rules, attacker {k}")
        term2 = D["terminated"].cpu().numpy() != 0
        rd = book.defender(D["reward"].cpu().numpy(), term2, D["valid_action"].cpu().numpy())
        for k in ("truncated", "dones", "episode_valid_actions", "episode_invalid_actions", "episode_length"):
            np.testing.assert_array_equal(rd[k].astype(np.int64), D[k].cpu().numpy().astype(np.int64), err_msg=f"{ctx}: rules, defender {k}")
        np.testing.assert_array_equal(rd["reward"].view(np.int64), bits(D["reward"]), err_msg=ctx + ": rules, defender reward")
        np.testing.assert_array_equal(rd["episode_return"].view(np.int64), bits(D["episode_return"]), err_msg=ctx + ": rules, defender return")
        np.testing.assert_array_equal(book.request, train.attacker_reset_request.cpu().numpy(), err_msg=ctx + ": rules, next request")
        own_timeout = ra["episode_length"] >= att_T
        seen["attacker_goal"] += int(term1.sum())
        seen["attacker_timeout"] += int((own_timeout & ~term1).sum())
        seen["attacker_request"] += int((q & ~term1 & ~own_timeout).sum())
        seen["intercepted_request"] += int((q & invalid).sum())
        n = rd["request_step"]
        seen["defender_request"] += int(n.sum())
        seen["defender_breach"] += int((term2 & D["sla_breached"].cpu().numpy()).sum())
        seen["defender_timeout"] += int((~n & ~term2 & (rd["episode_length"] >= def_T)).sum())
        seen["attacker_terminal_rows"] += int(done1.sum())
        seen["defender_terminal_rows"] += int(done2.sum())
    hdr_a, hdr_b = att_a.engine.get_state()[0], att_b.engine.get_state()[0]
    np.testing.assert_array_equal(hdr_a["episode"] - episode0, book.reinitialised, err_msg="every re-initialisation increments the episode counter once")
    np.testing.assert_array_equal(hdr_b["episode"] - episode0, book.reinitialised)
    att_a.close()
    att_b.close()
    return seen


CASES = ("attacker_goal", "attacker_timeout", "attacker_request", "defender_breach", "defender_timeout", "defender_request", "intercepted_request")


def lockstep_goal():
    """A goal low enough that attacker steps TERMINATE: a cumulative reward of 10, which the first successful exploit reaches.  (The
    reference traces have no terminated attacker step.)  An SLA of 0.80, so that two nodes re-imaging at once breach it."""
    from marlon_amd import cyberbattle_env as ce
    return dict(goal=ce.AttackerGoal(reward=10.0, own_atleast=0, own_atleast_percent=0.0), defender_constraint=ce.DefenderConstraint(maintain_sla=0.80))


def test_lockstep_toyctf_discrete():
    """E = 200: four workgroups, the last with 8 envs; 150 turns, both timeouts at 8.  With equal timeouts an attacker's own timeout ends
    both episodes (the defender's step is a request step); once a breach has ended a defender episode on its own, the attacker's clock
    lags by one turn, the defender times out first and the request meets the attacker's own timeout.  Every case of the hand-shake must
    occur on the composition's side."""
    seen = lockstep("toyctf", 200, 12, 10, True, turns=150, att_T=8, def_T=8, seed=0, state_turns=(1, 9, 25, 150), **lockstep_goal())
    print(seen)
    for case in CASES:
        assert seen[case] > 0, f"the run never showed the case `{case}`: {seen}"


def test_lockstep_chain10_multidiscrete():
    """Other row sizes (NP, 12 credentials), the MultiDiscrete decode; the attacker's timeout at 12 beyond the defender's at 10, so that
    requests reach an attacker whose own clock has not run out.  One case cannot occur here: the defender's timeout (or the attacker's
    goal) always resets the attacker's clock before it reaches 12, so no attacker episode ends by its OWN timeout in this run (the
    ToyCtf run above has 2 788 of them); the other six are asserted."""
    seen = lockstep("chain10", 200, 12, 12, False, turns=150, att_T=12, def_T=10, seed=0, state_turns=(1, 11, 150), **lockstep_goal())
    print(seen)
    for case in CASES:                                                     # (attacker_timeout: see above)
        if case == "attacker_timeout":
            continue
        assert seen[case] > 0, f"the run never showed the case `{case}`: {seen}"


def raw_train_call(att, dobs=None, alias=False):
    """mcbs_two_agent_train_step through ctypes with blocks built here -> (return code, message)"""
    import torch as t
    from marlon_amd._abi import TRAINING_FIELDS, DefenderObs, DefenderWrapperBuffers, DefenderWrapperCfg, training_buffers
    eng = att.engine
    E, dev = att.num_envs, eng.device
    _, wb, _ = att._next_output_set()
    obs = eng.obs_struct(att._obs)
    keep = eng.row_copies([(att._obs[k], att._terminal[k]) for k in att._obs])
    fresh = eng.row_copies([(att._reset_rows[k], att._obs[k]) for k in att._obs], one_row_src=True)
    dobs = dobs if dobs is not None else eng.alloc_defender_obs()
    dob = DefenderObs(**{k: x.data_ptr() for k, x in dobs.items()})
    mk = lambda dt: t.zeros(E, dtype=dt, device=dev)
    dts = (t.uint8, t.float64, t.uint8, t.uint8, t.float32, t.int32, t.int64, t.int64, t.uint8, t.float64, t.float64, t.uint8, t.uint8, t.uint8, t.uint8)
    dbuf = [mk(dt) for dt in dts]
    dwb = DefenderWrapperBuffers(*[x.data_ptr() for x in dbuf])
    cfg = DefenderWrapperCfg(-1.0, -5000.0, 200.0, 0.6, 5000.0, 1, 40)
    term = eng.alloc_defender_obs()
    tdt = dict(attacker_reset_request=t.uint8, defender_return=t.float64, attacker_valid_out=t.int64, attacker_invalid_out=t.int64,
               defender_return_out=t.float64, defender_length_out=t.int32, defender_valid_out=t.int64, defender_invalid_out=t.int64, defender_dones=t.uint8)
    arrays = {k: mk(dt) for k, dt in tdt.items()}
    arrays.update({"terminal_" + k: v for k, v in term.items()})
    arrays.update({"fresh_" + k: v[0:1].clone() for k, v in term.items()})
    if alias:
        arrays["defender_dones"] = arrays["attacker_reset_request"]
    assert set(arrays) == set(TRAINING_FIELDS)
    tb = training_buffers(**{k: v.data_ptr() for k, v in arrays.items()})
    a1 = t.zeros(att._action_shape, dtype=t.int64, device=dev)
    a2 = t.zeros((E, 12), dtype=t.int64, device=dev)
    p = a1.data_ptr()
    rc = eng.lib.mcbs_two_agent_train_step(eng._h, None if att.discrete else p, p if att.discrete else None, att._rows.data_ptr(),
                                           C.byref(eng._info_struct), C.byref(obs), C.byref(wb), -1.0, 24, C.byref(keep), C.byref(fresh), a2.data_ptr(),
                                           C.byref(dob), C.byref(dwb), C.byref(cfg), C.byref(tb), None)
    t.cuda.synchronize(dev)
    return rc, eng.lib.mcbs_last_error().decode()


def test_refusals_launch_nothing():
    import torch as t
    from marlon_amd.wrappers import TwoAgentTrainVecEnv, TwoAgentVecEnv
    # an attacker that does not auto-reset: the wrapper's to refuse (the joint turn without resets is TwoAgentVecEnv, which takes it)
    att, dfd = make_pair("toyctf", 64, 12, 10, True, 24, 40, auto_reset=False)
    assert att.engine.two_agent_train_step_launches() == 1 and not TwoAgentTrainVecEnv.supported(att) and TwoAgentVecEnv.supported(att)
    with pytest.raises(ValueError, match="auto_reset=True"):
        TwoAgentTrainVecEnv(att, dfd)
    att.close()
    # materialised masks: a mask field in the request
    att, dfd = make_pair("toyctf", 64, 12, 10, True, 24, 40, materialize_masks=True)
    before = att.engine.get_state()
    assert not TwoAgentTrainVecEnv.supported(att)
    with pytest.raises(ValueError, match="materialize_masks"):
        TwoAgentTrainVecEnv(att, dfd)
    rc, msg = raw_train_call(att)
    assert rc == -1 and "mask field" in msg and same_state(before, att.engine.get_state())
    att.close()
    # no learned defender
    att, _ = make_pair("toyctf", 64, 12, 10, True, 24, 40, learned_defender=False)
    before = att.engine.get_state()
    assert att.engine.two_agent_train_step_launches() == 0 and not TwoAgentTrainVecEnv.supported(att)
    with pytest.raises(ValueError, match="learned_defender"):
        TwoAgentTrainVecEnv(att, None)
    rc, msg = raw_train_call(att)
    assert rc == -1 and "MCBS_DEFENDER_EXTERNAL" in msg and same_state(before, att.engine.get_state())
    att.close()
    # outside the packed scope
    att, dfd = make_pair("chain10", 64, 12, 20, False, 24, 40)
    before = att.engine.get_state()
    assert att.engine.two_agent_train_step_launches() == 0 and not TwoAgentTrainVecEnv.supported(att)
    with pytest.raises(ValueError, match="does not serve"):
        TwoAgentTrainVecEnv(att, dfd)
    rc, msg = raw_train_call(att)
    assert rc == -1 and "one launch" in msg and same_state(before, att.engine.get_state())
    att.close()
    # packed observation rows
    att, dfd = make_pair("toyctf", 64, 12, 10, True, 24, 40, observation_format="packed")
    with pytest.raises(ValueError, match="observation_format"):
        TwoAgentTrainVecEnv(att, dfd)
    att.close()
    # a defender observation array off a 16-byte boundary; two arrays of the new block sharing bytes; then the same call goes through
    att, dfd = make_pair("toyctf", 64, 12, 10, True, 24, 40)
    before = att.engine.get_state()
    assert TwoAgentTrainVecEnv.supported(att)
    dobs = att.engine.alloc_defender_obs()
    N = dobs["infected_nodes"].shape[1]
    raw = t.zeros(64 * N + 16, dtype=t.int8, device=att.engine.device)
    dobs["infected_nodes"] = raw[1:1 + 64 * N].view(64, N)
    rc, msg = raw_train_call(att, dobs)
    assert rc == -1 and "16-byte" in msg and same_state(before, att.engine.get_state())
    rc, msg = raw_train_call(att, alias=True)
    assert rc == -1 and "overlaps" in msg and same_state(before, att.engine.get_state())
    rc, msg = raw_train_call(att)
    assert rc == 0, msg
    assert not same_state(before, att.engine.get_state())
    att.close()


def test_collect_rollouts_fills_both_buffers_like_a_hand_written_loop():
    """64 envs x 8 steps, timeouts at 3 and 5 so that episodes end on both sides inside the rollout: `collect_rollouts` on one pair against
    `step` + `add` written out on another, every stored array and the returned dones compared."""
    import torch as t
    from marlon_amd.simulate import collect_rollouts
    from marlon_amd.wrappers import TwoAgentTrainVecEnv
    E, T = 64, 8
    pairs = [make_pair("toyctf", E, 12, 10, True, 3, 5) for _ in range(2)]
    trains = [TwoAgentTrainVecEnv(a, d) for a, d in pairs]
    bufs = [(a.rollout_buffer(T), d.rollout_buffer(T)) for a, d in pairs]
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
    # twice, so that episode_starts are carried from one call to the next
    for rollout in range(2):
        pa, pd = policies()
        dones = collect_rollouts(trains[0], pa, pd, bufs[0][0], bufs[0][1], T)
        (att, dfd), train, (ba, bd) = pairs[1], trains[1], bufs[1]
        pa, pd = policies()
        ba.reset()
        bd.reset()
        starts = train.last_dones
        for _ in range(T):
            a1, v1, l1 = pa(att)
            a2, v2, l2 = pd(dfd)
            bits_row = att.action_masks_packed()
            obs_a = {k: v.clone() for k, v in att.observation_fields.items()}
            obs_d = {k: v.clone() for k, v in dfd.observation.items()}
            (_, r1, te1, tr1, _), (_, r2, te2, tr2, _) = train.step(a1, a2)
            ba.add(obs_a, a1, r1, starts[0], v1, l1, bits=bits_row)
            bd.add(obs_d, a2, r2, starts[1], v2, l2)
            starts = ((te1 | tr1).clone(), (te2 | tr2).clone())
        train.last_dones = starts
        for got, want, who in ((bufs[0][0], ba, "attacker"), (bufs[0][1], bd, "defender")):
            assert got.full and want.full
            for k in ("actions", "rewards", "values", "log_probs", "episode_starts"):
                np.testing.assert_array_equal(bits(getattr(got, k)), bits(getattr(want, k)), err_msg=f"rollout {rollout} {who} {k}")
            for k in want.observations:
                np.testing.assert_array_equal(bits(got.observations[k]), bits(want.observations[k]), err_msg=f"rollout {rollout} {who} observation {k}")
        np.testing.assert_array_equal(bits(bufs[0][0].mask_bits), bits(ba.mask_bits), err_msg=f"rollout {rollout} mask bits")
        for x, y in zip(dones, starts):
            np.testing.assert_array_equal(bits(x), bits(y))
        assert int(bufs[0][0].episode_starts.sum()) > E and int(bufs[0][1].episode_starts.sum()) > E, "no episode ended inside the rollout"
        lv = t.zeros(E, device=dev)
        bufs[0][0].compute_returns_and_advantage(lv, dones[0])
        bufs[0][1].compute_returns_and_advantage(lv, dones[1])
    for a, _ in pairs:
        a.close()
