"""The two-agent turn (mcbs_two_agent_step, marlon_amd/csrc/mcbs_two_agent.hip; `TwoAgentVecEnv`, `run_episode_joint`): one launch per
joint turn must equal, bit for bit and env by env, the sequence it replaces — `att.step`, the parking of finished envs, `dfd.step` and
run_episode's host bookkeeping (restated in tests/episode_ref.py).

* the reference's recorded two-agent episodes through `run_episode_joint`;
* lockstep of two identically configured wrapper pairs, one stepped the old way, one with the joint turn, every output, observation,
  counter and episode array compared after every turn, the engine state at chosen turns (ToyCtf Discrete, Chain-10 MultiDiscrete);
* the call without an episode block; the refusals; `simulate(joint=True)`."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import parity
from tests.episode_ref import EpisodeBook

pytestmark = pytest.mark.gpu


def make_pair(topo, E, nodes, creds, discrete, att_T, def_T, seed=0, **kw):
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.wrappers import AttackerVecEnv, DefenderVecEnv
    args = dict(maximum_node_count=nodes, maximum_total_credentials=creds, attacker_goal=ce.AttackerGoal(own_atleast=6),
                defender_constraint=ce.DefenderConstraint(maintain_sla=0.60), losing_reward=-5000.0, max_timesteps=att_T, auto_reset=False,
                learned_defender=True, materialize_masks=False, discrete=discrete, seed=seed)
    args.update(kw)
    att = AttackerVecEnv(parity.topology_for(topo), E, **args)
    dfd = DefenderVecEnv(att, max_timesteps=def_T, invalid_action_reward=-1, loss_reward=-5000.0) if args["learned_defender"] else None
    return att, dfd


def bits(x):
    """a device tensor as a host array compared exactly: floating point as the integers of its bits"""
    a = x.detach().cpu().numpy()
    return a.view({4: np.int32, 8: np.int64}[a.itemsize]) if a.dtype.kind == "f" else a


def snapshot(att, dfd, a_out, d_out):
    """everything a joint turn writes on the two wrappers' side"""
    _, r, term, trunc, info = a_out
    _, dr, dterm, dtrunc, dinfo = d_out
    s = {"a.rewards": r, "a.terminated": term, "a.truncated": trunc, "a.dones": att._dones, "a.decoded": att._rows,
         "a.digest": att.action_masks_packed()}
    s.update({"a.info." + k: v for k, v in info.items()})
    s.update({"a.obs." + k: v for k, v in att.observation_fields.items()})
    for k in ("timesteps", "valid_action_count", "invalid_action_count", "episode_returns", "last_cyber_reward", "has_cyber_reward"):
        s["a.counter." + k] = getattr(att, k)
    s.update({"d.reward": dr, "d.terminated": dterm, "d.truncated": dtrunc, "d.evicted": dfd._evicted})
    s.update({"d.info." + k: v for k, v in dinfo.items()})
    s.update({"d.obs." + k: v for k, v in dfd.observation.items()})
    for k in ("timesteps", "valid_action_count", "invalid_action_count", "has_breached_sla", "prev_availability"):
        s["d.counter." + k] = getattr(dfd, k)
    return {k: bits(v) for k, v in s.items()}


def assert_same(a, b, ctx):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{ctx}: {k}")


def assert_same_state(att_a, att_b, ctx):
    for x, y, what in zip(att_a.engine.get_state(), att_b.engine.get_state(), ("headers", "nodes", "discovery order", "credential cache")):
        np.testing.assert_array_equal(x, y, err_msg=f"{ctx}: engine state, {what}")


def defender_actions(rng, dfd, N):
    """uniform over nvec, then fixed subsets of rows: the empty action, a parked env, a node index equal to N, a negative node index"""
    E = dfd.num_envs
    a = (rng.random((E, 12)) * dfd.nvec).astype(np.int64)
    rows = np.arange(E)
    a[rows % 11 == 3, 0] = -1
    a[rows % 13 == 5, 0] = -2
    for c in (1, 2, 5, 8, 10):                                             # the node component of each of the five kinds
        a[rows % 7 == 2, c] = N
        a[rows % 9 == 4, c] = -1 - (rows[rows % 9 == 4] % 3)
    return a


def lockstep(topo, E, nodes, creds, discrete, turns, att_T, def_T, seed, state_turns=(), with_episode=True):
    """Pair A: att.step, run_episode's parking, dfd.step, the bookkeeping on the host.  Pair B: TwoAgentVecEnv.step.  -> what pair A saw."""
    import torch as t
    from marlon_amd.wrappers import TwoAgentVecEnv
    att_a, dfd_a = make_pair(topo, E, nodes, creds, discrete, att_T, def_T)
    att_b, dfd_b = make_pair(topo, E, nodes, creds, discrete, att_T, def_T)
    assert TwoAgentVecEnv.supported(att_b) and att_b.engine.two_agent_step_launches() == 1
    joint = TwoAgentVecEnv(att_b, dfd_b)
    ep = joint.episode_state() if with_episode else None
    book = EpisodeBook(E, track_alive=with_episode)
    rng = np.random.default_rng(seed)
    N = att_a.topo.n_nodes
    dev = att_a.engine.device
    seen = dict(attacker_ended=0, defender_ended_early=0, reimage=0, block=0, allow_appended=0, invalid_defender=0, intercepted=0, parked_turns=None)
    parked_turns = np.zeros(E, np.int64)
    for turn in range(1, turns + 1):
        ctx = f"{topo} E={E} turn {turn}"
        if turn % 2 == 1:                                                  # uniformly random indices: mostly intercepted
            a1 = (rng.random(att_a._action_shape) * (att_a.discrete_n if discrete else att_a.nvec)).astype(np.int64)
        elif discrete:                                                     # masked-valid ones (the law of simulate.random_policy)
            a1 = att_a.sample_masked_uniform(seed=seed, step=turn).actions.cpu().numpy()
        else:
            a1 = att_a.engine.sample_actions(valid=True, seed=seed, step=turn).cpu().numpy().astype(np.int64)
            a1 = md_rows(a1)
        a2 = defender_actions(rng, dfd_a, N)
        a1_d, a2_d = t.as_tensor(a1, device=dev), t.as_tensor(a2, device=dev)
        # pair A, as run_episode does it
        fw_before = dfd_a.observation["incoming_firewall_status"].cpu().numpy().copy()
        out_a = att_a.step(a1_d.clone())
        parked = book.attacker(out_a[1].cpu().numpy(), out_a[2].cpu().numpy(), out_a[3].cpu().numpy())
        a2_host = a2.copy()
        a2_host[parked, 0] = -2
        dout_a = dfd_a.step(t.as_tensor(a2_host, device=dev))
        d2 = book.defender(dout_a[1].cpu().numpy(), dout_a[2].cpu().numpy(), dout_a[3].cpu().numpy())
        # pair B
        a2_keep = a2_d.clone()
        out_b, dout_b = joint.step(a1_d, a2_d, episode=ep)
        assert t.equal(a2_d, a2_keep), f"{ctx}: the joint turn modified the defender's actions"
        assert_same(snapshot(att_a, dfd_a, out_a, dout_a), snapshot(att_b, dfd_b, out_b, dout_b), ctx)
        if with_episode:
            got = {k: bits(v) for k, v in ep.tensors().items()}
            want = {k: (v.view(np.int64) if v.dtype.kind == "f" else v) for k, v in book.arrays().items()}
            assert_same(want, got, ctx + " episode block")
        if turn in state_turns:
            assert_same_state(att_a, att_b, ctx)
        # what pair A — the existing path — went through
        stepped = ~parked & (a2[:, 0] > -2)
        valid = dout_a[4]["valid_action"].cpu().numpy()
        fw_after = dfd_a.observation["incoming_firewall_status"].cpu().numpy()
        parked_turns += parked
        seen["attacker_ended"] += int(book._d1.sum())
        seen["defender_ended_early"] += int((d2 & ~book._d1 & book._a).sum()) if turn < att_T else 0
        seen["reimage"] += int((stepped & valid & (a2[:, 0] == 0)).sum())
        seen["block"] += int((stepped & valid & (a2[:, 0] == 1)).sum())
        seen["allow_appended"] += int((stepped & valid & (a2[:, 0] == 2) & ((fw_after > fw_before).any(axis=1))).sum())
        seen["invalid_defender"] += int((stepped & ~valid).sum())
        seen["intercepted"] += int(out_a[4]["invalid_action"].cpu().numpy().sum())
    seen["parked_turns"] = parked_turns
    att_a.close()
    att_b.close()
    return seen


def md_rows(rows5):
    """engine rows (kind, a, b, c, d) -> the wrapper's MultiDiscrete rows [kind, l_src, l_vuln, r_src, r_tgt, r_vuln, c_src, c_tgt, c_port, c_cred]"""
    out = np.zeros((len(rows5), 10), np.int64)
    out[:, 0] = rows5[:, 0]
    for i, (k, a, b, c, d) in enumerate(rows5):
        if k == 0:
            out[i, 1:3] = (a, b)
        elif k == 1:
            out[i, 3:6] = (a, b, c)
        else:
            out[i, 6:10] = (a, b, c, d)
    return out


# seeds at which pair A — existing code alone — goes through every case the tests below ask for (the first ones tried on an MI355X did)
TOYCTF_SEED = 0
CHAIN_SEED = 0


def test_lockstep_toyctf_discrete_four_workgroups():
    """E = 200: four workgroups, the last with 8 envs; attacker truncation at 24, 32 turns: every env is parked for at least 8 of them."""
    seen = lockstep("toyctf", 200, 12, 10, True, turns=32, att_T=24, def_T=40, seed=TOYCTF_SEED, state_turns=(1, 8, 32))
    assert seen["parked_turns"].min() >= 8
    for case in ("attacker_ended", "defender_ended_early", "reimage", "block", "allow_appended", "invalid_defender", "intercepted"):
        assert seen[case] > 0, f"the run never showed the case `{case}` on the existing path: {seen}"


def test_lockstep_toyctf_one_full_workgroup():
    lockstep("toyctf", 64, 12, 10, True, turns=8, att_T=24, def_T=40, seed=TOYCTF_SEED + 1, state_turns=(8,))


def test_lockstep_chain10_multidiscrete_one_env_tail():
    """Other row sizes (NP, 12 credentials), MultiDiscrete decode, a workgroup with a single env."""
    from marlon_amd.wrappers import TwoAgentVecEnv
    att, _ = make_pair("chain10", 65, 12, 12, False, 8, 10)
    ok = TwoAgentVecEnv.supported(att)
    att.close()
    assert ok, "Chain-10 at 12/12 with a learned defender is in the joint turn's scope"
    seen = lockstep("chain10", 65, 12, 12, False, turns=12, att_T=8, def_T=10, seed=CHAIN_SEED, state_turns=(1, 12))
    assert seen["attacker_ended"] > 0 and seen["intercepted"] > 0 and seen["parked_turns"].min() >= 4


def test_without_an_episode_block():
    """ep == NULL: nothing is booked, every env counts as alive, and the attacker's own dones of the turn still park the defender."""
    seen = lockstep("toyctf", 64, 12, 10, True, turns=4, att_T=3, def_T=40, seed=5, with_episode=False)
    assert seen["attacker_ended"] >= 2 * 64                                # truncated at turns 3 and 4: parked from the attacker's dones alone


@pytest.mark.parametrize("name", ["wrap_episode_toyctf_s73", "wrap_episode_toyctf_s74", "wrap_episode_toyctf_s75"])
def test_run_episode_joint_replays_reference_two_agent_episodes(name):
    """tests/test_gpu_episodes.py::test_run_episode_replays_reference_two_agent_episodes through the joint driver; sync_every=4, so that
    up to three trailing all-parked iterations are taken and trimmed (the replaying policies repeat their last action there)."""
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.simulate import run_episode_joint
    from marlon_amd.wrappers import AttackerVecEnv, DefenderVecEnv
    z = np.load(os.path.join(parity.GOLDEN, name + ".npz"))
    sj = json.loads(bytes(z["spec_json"]).decode())
    att = AttackerVecEnv(parity.topology_for("toyctf"), 1, maximum_node_count=12, maximum_total_credentials=10,
                         attacker_goal=ce.AttackerGoal(**sj["attacker_goal"]), defender_constraint=ce.DefenderConstraint(sj["maintain_sla"]),
                         losing_reward=sj["losing_reward"], max_timesteps=sj["max_timesteps"], auto_reset=False, learned_defender=True,
                         materialize_masks=False)
    dfd = DefenderVecEnv(att, max_timesteps=sj["max_timesteps"], invalid_action_reward=-1, loss_reward=-5000.0)
    ep = z["episode"]
    ends = {"attacker": 0, "defender": 0, "max_steps": 0}
    trimmed = 0
    for e in range(int(ep.max()) + 1):
        idx = np.flatnonzero(ep == e)
        cur = {"a": 0, "d": 0}

        def pa(env, idx=idx, cur=cur):
            a = z["a_action"][idx[min(cur["a"], len(idx) - 1)]].reshape(1, 10)
            cur["a"] += 1
            return a

        def pd(env, idx=idx, cur=cur):
            d = z["d_action"][idx[min(cur["d"], len(idx) - 1)]].reshape(1, 12)
            cur["d"] += 1
            return d
        out = run_episode_joint(att, dfd, pa, pd, max_steps=sj["max_steps"], sync_every=4)
        n = len(idx)
        trimmed += cur["a"] - n
        ctx = f"{name} episode {e}"
        assert int(out["lengths"][0]) == n and out["steps"] == n, f"{ctx}: {int(out['lengths'][0])} steps, the reference took {n}"
        assert out["attacker_rewards"].shape == (n, 1) and out["defender_rewards"].shape == (n, 1), ctx
        np.testing.assert_array_equal(out["attacker_rewards"][:, 0].cpu().numpy(), z["a_reward"][idx], err_msg=ctx + " attacker rewards")
        np.testing.assert_array_equal(out["defender_rewards"][:, 0].cpu().numpy(), z["d_reward"][idx], err_msg=ctx + " defender rewards")
        assert bool(out["attacker_done"][0]) == bool(z["a_done"][idx[-1]]) and bool(out["defender_done"][0]) == bool(z["d_done"][idx[-1]]), ctx
        ends["attacker" if z["a_done"][idx[-1]] else ("defender" if z["d_done"][idx[-1]] else "max_steps")] += 1
        if z["a_done"][idx[-1]]:                       # reset_request rule (defend_wrapper.py:269-271), as the reference returned it
            assert z["d_reward"][idx[-1]] == -z["a_reward"][idx[-1]]
            assert np.signbit(out["defender_rewards"][-1, 0].item()) == np.signbit(z["d_reward"][idx[-1]]), ctx + ": the sign of a zero"
    assert sum(ends.values()) == len(sj["ends"])
    if name == "wrap_episode_toyctf_s73":
        assert trimmed > 0, "no episode ended between two looks at `alive`: trimming was not exercised"
    att.close()


def raw_two_agent_call(att, dobs=None):
    """mcbs_two_agent_step through ctypes with blocks built here (no DefenderVecEnv needed) -> the library's return code"""
    import torch as t
    from marlon_amd._abi import DefenderObs, DefenderWrapperBuffers, DefenderWrapperCfg
    eng = att.engine
    E, dev = att.num_envs, eng.device
    _, wb, _ = att._next_output_set()
    obs = eng.obs_struct(att._obs)
    dobs = dobs if dobs is not None else eng.alloc_defender_obs()
    dob = DefenderObs(**{k: x.data_ptr() for k, x in dobs.items()})
    mk = lambda dt: t.zeros(E, dtype=dt, device=dev)
    dts = (t.uint8, t.float64, t.uint8, t.uint8, t.float32, t.int32, t.int64, t.int64, t.uint8, t.float64, t.float64, t.uint8, t.uint8, t.uint8, t.uint8)
    keep = [mk(dt) for dt in dts]
    dwb = DefenderWrapperBuffers(*[x.data_ptr() for x in keep])
    cfg = DefenderWrapperCfg(-1.0, -5000.0, 200.0, 0.6, 5000.0, 1, 40)
    a1 = t.zeros(att._action_shape, dtype=t.int64, device=dev)
    a2 = t.zeros((E, 12), dtype=t.int64, device=dev)
    p = a1.data_ptr()
    rc = eng.lib.mcbs_two_agent_step(eng._h, None if att.discrete else p, p if att.discrete else None, att._rows.data_ptr(), C.byref(eng._info_struct),
                                     C.byref(obs), C.byref(wb), -1.0, 24, a2.data_ptr(), C.byref(dob), C.byref(dwb), C.byref(cfg), None, None)
    t.cuda.synchronize(dev)
    return rc, eng.lib.mcbs_last_error().decode()


def same_state(before, after):
    return all(np.array_equal(x, y) for x, y in zip(before, after))


def test_refusals_launch_nothing():
    import torch as t
    from marlon_amd.wrappers import DefenderVecEnv, TwoAgentVecEnv
    # an auto-resetting attacker: the call itself has no auto-reset, so this one is the wrapper's to refuse
    att, dfd = make_pair("toyctf", 64, 12, 10, True, 24, 40, auto_reset=True)
    assert att.engine.two_agent_step_launches() == 1 and not TwoAgentVecEnv.supported(att)
    with pytest.raises(ValueError, match="auto_reset"):
        TwoAgentVecEnv(att, dfd)
    att.close()
    # materialised masks: a mask field in the request
    att, dfd = make_pair("toyctf", 64, 12, 10, True, 24, 40, materialize_masks=True)
    before = att.engine.get_state()
    assert att.engine.two_agent_step_launches() == 1 and not TwoAgentVecEnv.supported(att)
    with pytest.raises(ValueError, match="materialize_masks"):
        TwoAgentVecEnv(att, dfd)
    rc, msg = raw_two_agent_call(att)
    assert rc == -1 and "mask field" in msg and same_state(before, att.engine.get_state())
    att.close()
    # no learned defender
    att, _ = make_pair("toyctf", 64, 12, 10, True, 24, 40, learned_defender=False)
    before = att.engine.get_state()
    assert att.engine.two_agent_step_launches() == 0 and not TwoAgentVecEnv.supported(att)
    with pytest.raises(ValueError, match="learned_defender"):
        TwoAgentVecEnv(att, None)
    rc, msg = raw_two_agent_call(att)
    assert rc == -1 and "MCBS_DEFENDER_EXTERNAL" in msg and same_state(before, att.engine.get_state())
    att.close()
    # outside the packed scope
    att, dfd = make_pair("chain10", 64, 12, 20, False, 24, 40)
    before = att.engine.get_state()
    assert att.engine.two_agent_step_launches() == 0 and not TwoAgentVecEnv.supported(att)
    with pytest.raises(ValueError, match="does not serve"):
        TwoAgentVecEnv(att, dfd)
    rc, msg = raw_two_agent_call(att)
    assert rc == -1 and "one launch" in msg and same_state(before, att.engine.get_state())
    att.close()
    # a defender observation array that is not on a 16-byte boundary
    att, dfd = make_pair("toyctf", 64, 12, 10, True, 24, 40)
    before = att.engine.get_state()
    assert att.engine.two_agent_step_launches() == 1 and TwoAgentVecEnv.supported(att)
    dobs = att.engine.alloc_defender_obs()
    N = dobs["infected_nodes"].shape[1]
    raw = t.zeros(64 * N + 16, dtype=t.int8, device=att.engine.device)
    dobs["infected_nodes"] = raw[1:1 + 64 * N].view(64, N)
    assert dobs["infected_nodes"].data_ptr() % 16 == 1
    rc, msg = raw_two_agent_call(att, dobs)
    assert rc == -1 and "16-byte" in msg and same_state(before, att.engine.get_state())
    rc, msg = raw_two_agent_call(att)                                      # ... and the same call with aligned arrays goes through
    assert rc == 0, msg
    assert not same_state(before, att.engine.get_state())
    att.close()


def test_simulate_joint_equals_simulate():
    import torch as t
    from marlon_amd.simulate import simulate
    kw = dict(n_envs=64, seed=3, maximum_node_count=12, maximum_total_credentials=10)
    a = simulate(60, "Random", "Random", joint=True, **kw)
    b = simulate(60, "Random", "Random", joint=False, **kw)
    assert a.keys() == b.keys() and a["steps"] == b["steps"]
    for k in a:
        if k != "steps":
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg=k)
