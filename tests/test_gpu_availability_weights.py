"""network_availability under unequal SLA weights, on every kernel that ticks the in-env defender, against the CPU oracle, bitwise.

defender_tick (mcbs_step.hip, copied by hand into mcbs_step_coop.hip) sums the availability in one of three ways: the uniform shortcut
(every node has the same term: full_sum - n * term), the any-order subtraction (flatten.py proved sums exact: full_sum - the terms of
the nodes being re-imaged; the cooperative kernel adds the G lanes' partial sums with DPP) and the reference's node-order loop (the
cooperative kernel gathers the G words into every lane).  Every sample topology has the term 1.0, so only the weighted topologies of
tests/endings.py reach the other two: `dyadic` (any-order, unequal terms) and `odd` (node-order).  tests/test_endings_script.py proves
from the oracle alone that their scripts put enough different sets of nodes out of the sum, that a kernel on another branch returns
other bits on hundreds of steps, and that `sla_eq` / `sla_up` (maintain_sla = an attained availability v / the next double above)
turn a sum that is one ulp off into another reward and another `terminated`, which is all mcbs_step_many returns.

| entry point | cells (test_gpu_episode_endings.CELLS; packed and toyctf_general play the kitchen-sink topology) | test |
|---|---|---|
| step | all eight | test_step_sums_availability_as_the_oracle |
| step_many, two launches (header availability of the state after each) | packed, general1, lane2, lane4, wide | test_step_many_sums_availability_as_the_oracle |
| step / step_observe / step_many alternating on one cooperative batch | coop2, coop4 | test_cooperative_batch_sums_availability_on_every_entry_point |
| step_observe on every step (the defender ticks in phase 2) | packed, lane2, wide | test_step_observe_sums_availability_as_the_oracle |
| rollout_random, recorded actions replayed through the oracle | general1, coop4 (its one-lane kernel) | test_rollout_random_sums_availability_as_the_oracle |
| AttackerVecEnv + ScanAndReimage: one launch, three launches | packed; general1 (always three) | test_attacker_vec_env_sums_availability_as_the_oracle |

Every case is 203 envs and at most 120 steps.  Each batch asserts its variant before it steps.
"""
import numpy as np
import pytest

from tests import endings as En
from tests.test_gpu_episode_endings import CELLS, _compare_states, _create, _multidiscrete, _plan, _replay

pytestmark = pytest.mark.gpu

# the packed layouts play the kitchen-sink topology (endings.weighted_settings: ToyCtf keeps one node out of the sum at most)
TOPOLOGY = {cell: ("sink" if topo == "toyctf" else topo) for cell, (topo, _, _) in CELLS.items()}
assert set(TOPOLOGY.values()) == set(En.WEIGHT_TOPOLOGIES)


def _weighted(cell, spec_name, monkeypatch):
    c, eng = _create(cell, spec_name, monkeypatch, topo_name=TOPOLOGY[cell])
    kind = spec_name.rsplit("_", 1)[1]
    assert int(c.topo.header()["avail_any_order"]) == (1 if kind == "dyadic" else 0) and c.imaging is not None
    return c, eng


@pytest.mark.parametrize("spec_name", En.WEIGHT_SPECS)
@pytest.mark.parametrize("cell", sorted(CELLS))
def test_step_sums_availability_as_the_oracle(cell, spec_name, monkeypatch):
    """mcbs_step: every output of every step (the availability as uint64), the state after every step in which an env ended and after
    the last one."""
    c, eng = _weighted(cell, spec_name, monkeypatch)
    _replay(c, eng, _plan(c, [("step", 1)]), f"{cell} {spec_name}")
    eng.close()


MANY_CUTS = (50, 110)      # neither is a multiple of an episode bound (40, 60): the envs are in mid-episode when the state is compared


@pytest.mark.parametrize("spec_name", En.WEIGHT_SPECS)
@pytest.mark.parametrize("cell", ["packed", "general1", "lane2", "lane4", "wide"])
def test_step_many_sums_availability_as_the_oracle(cell, spec_name, monkeypatch):
    """mcbs_step_many (the looping kernel) in two launches.  It returns rewards and terminations only: under sla_eq / sla_up those
    depend on the last bit of the sum; under avail the header availability of the state after each launch is what is compared, and
    at least 8 envs hold there a value that another branch would have got wrong."""
    c, eng = _weighted(cell, spec_name, monkeypatch)
    a, b = MANY_CUTS
    if spec_name.startswith("avail"):
        held = [int((En.discriminating(c)[t - 1] & En.compared(c)[t - 1]).sum()) for t in MANY_CUTS]
        assert min(held) >= 8, f"envs holding a discriminating availability after each launch: {held}"
    _replay(c, eng, [("many", 0, a), ("many", a, b - a)], f"{cell} {spec_name}")
    eng.close()


@pytest.mark.parametrize("spec_name", En.WEIGHT_SPECS)
@pytest.mark.parametrize("cell", ["coop2", "coop4"])
def test_cooperative_batch_sums_availability_on_every_entry_point(cell, spec_name, monkeypatch):
    """One cooperative batch advanced by step (the G-lane kernel: the DPP sum of the lanes' partial sums, or the gather of the G words),
    step_observe and step_many (the one-lane kernels) in turn, on one state."""
    c, eng = _weighted(cell, spec_name, monkeypatch)
    used = _replay(c, eng, _plan(c, [("step", 1), ("observe", 1), ("many", 3), ("step", 1), ("observe", 1)]), f"{cell} {spec_name}")
    assert used == {"step", "observe", "many"}
    eng.close()


@pytest.mark.parametrize("spec_name", En.WEIGHT_SPECS)
@pytest.mark.parametrize("cell", ["packed", "lane2", "wide"])
def test_step_observe_sums_availability_as_the_oracle(cell, spec_name, monkeypatch):
    """mcbs_step_observe on every step: the defender ticks, and the SLA is judged, in the phase-2 kernel."""
    c, eng = _weighted(cell, spec_name, monkeypatch)
    _replay(c, eng, _plan(c, [("observe", 1)]), f"{cell} {spec_name}")
    eng.close()


@pytest.mark.parametrize("kind", En.WEIGHT_KINDS)
@pytest.mark.parametrize("cell", ["general1", "coop4"])
def test_rollout_random_sums_availability_as_the_oracle(cell, kind, monkeypatch):
    """mcbs_rollout_random (the device draws the actions; on the cooperative batch it is the one-lane kernel that runs) under `avail`.
    A random agent seldom holds a second node, so the first 30 rows of the script are played first (one step_many launch: the
    attacker holds several nodes, some are being re-imaged), then twelve launches of 7 random steps, which end in mid-episode
    (37, 44, ...: no multiple of 40 or 60).  The recorded actions replayed through the oracle give the same rewards and terminations
    and the same state, header availability included, after every launch; at least 8 of those header values are ones a kernel on
    another branch gets wrong (endings.discriminating_of, from the oracle's node states around the launch's last step)."""
    from oracle.oracle import Oracle
    c, eng = _weighted(cell, f"avail_{kind}", monkeypatch)
    orc = Oracle(c.topo, c.spec)
    N, lead, per = c.topo.n_nodes, 30, 7
    eng.step_many(eng.torch.as_tensor(c.actions[:lead], device=eng.device))
    for t in range(lead):
        orc.step(c.actions[t])
    held = 0
    for i in range(12):
        first = lead + per * i
        r, d, acts = eng.rollout_random(per, valid=i % 3 != 2, seed=5, first_step=first, record_actions=True)
        rn, dn, an = r.double().cpu().numpy(), d.cpu().numpy(), acts.cpu().numpy()
        for k in range(per):
            before = orc.get_state()[1]["running"][:, :N] if k == per - 1 else None
            o = orc.step(an[k])
            np.testing.assert_array_equal(rn[k], o["reward"], err_msg=f"{cell} {kind} rollout step {first + k} reward")
            np.testing.assert_array_equal(dn[k], o["terminated"], err_msg=f"{cell} {kind} rollout step {first + k} terminated")
        st = orc.get_state()
        _compare_states(eng.get_state(), st, f"{cell} {kind} after rollout launch {i}")
        played = (o["oob"] == 0) & (o["terminated"] == 0) & (o["truncated"] == 0)
        held += int((En.discriminating_of(c.topo, (before == 0) & (st[1]["running"][:, :N] == 0)) & played).sum())
    assert held >= 8, f"{held} header availabilities that tell the branches apart"
    eng.close()


@pytest.mark.parametrize("kind", En.WEIGHT_KINDS)
@pytest.mark.parametrize("cell,launches", [("packed", 1), ("packed", 3), ("general1", 3)])
def test_attacker_vec_env_sums_availability_as_the_oracle(cell, launches, kind, monkeypatch):
    """AttackerVecEnv with ScanAndReimage on a weighted topology, under the sla_up threshold: the wrapper step in one launch
    (wrapper_fused_kernel) and in three (decode_step1_kernel, the observation, step2_finish_kernel; MCBS_NO_FUSED_WRAPPER=1 on the
    packed batch, always on a general one).  Rows from the host policy, some intercepted; rewards, terminated, truncated and the
    availability of the infos against the oracle at every step."""
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.wrappers import AttackerVecEnv
    from oracle.oracle import Oracle
    want = CELLS[cell][2]
    topo_name = TOPOLOGY[cell]
    case = En.case(f"{topo_name}-sla_up_{kind}")
    topo, s = case.topo, case.spec
    E, T, MAXT = En.E, 100, 30
    if cell == "packed" and launches == 3:
        monkeypatch.setenv("MCBS_NO_FUSED_WRAPPER", "1")
    env = AttackerVecEnv(topo, E, maximum_node_count=s.maximum_node_count, maximum_total_credentials=s.maximum_total_credentials,
                         maximum_discoverable_credentials_per_action=s.maximum_discoverable_credentials_per_action,
                         attacker_goal=ce.AttackerGoal(**s.attacker_goal), defender_agent=ce.ScanAndReimageCompromisedMachines(*s.defender[1:]),
                         defender_goal=ce.DefenderGoal(eviction=False), defender_constraint=ce.DefenderConstraint(s.maintain_sla),
                         winning_reward=En.WIN, losing_reward=En.LOSE, max_timesteps=MAXT, seed=4242, env_id_base=500, materialize_masks=False)
    v = env.engine.variant()
    assert {k: v[k] for k in want} == want and v["defender_kind"] == 1 and v["fused_wrapper"] == (1 if launches == 1 else 0), v
    assert env.engine.wrapper_step_launches(False) == launches
    assert env.spec.maintain_sla == s.maintain_sla and not env.spec.defender_goal_eviction
    orc = Oracle(topo, env.spec)
    orc.reset()                                          # the wrapper's reset() began episode 1
    pol = En.Policy(topo, env.spec, 19)
    full = float(topo.header()["full_availability"])
    timesteps, n_disc = np.zeros(E, np.int64), np.ones(E, np.int64)
    below, values, sla = 0, set(), np.zeros(E, bool)
    for t in range(T):
        a = np.minimum(_multidiscrete(pol.rows(orc.get_state())), env.nvec - 1)
        kd = a[:, 0]
        src = np.where(kd == 0, a[:, 1], np.where(kd == 1, a[:, 3], a[:, 6]))
        tgt = np.where(kd == 0, 0, np.where(kd == 1, a[:, 4], a[:, 7]))
        valid = (src < n_disc) & ((kd == 0) | (tgt < n_disc))            # attack_wrapper.py:286-308
        played = np.zeros((E, 5), np.int32)
        played[:, 0] = np.where(valid, kd, 3)
        played[:, 1] = src
        played[:, 2] = np.where(kd == 0, a[:, 2], tgt)
        played[:, 3] = np.where(kd == 1, a[:, 5], np.where(kd == 2, a[:, 8], 0))
        played[:, 4] = np.where(kd == 2, a[:, 9], 0)
        obs, r, term, trunc, info = env.step(a)
        o = orc.step(played)
        timesteps += 1
        ctx = f"{cell} {kind} {launches} launch(es) step {t}"
        np.testing.assert_array_equal(r.double().cpu().numpy(), o["reward"] + np.where(valid, 0.0, -1.0), err_msg=ctx + " reward")
        np.testing.assert_array_equal(term.cpu().numpy(), o["terminated"], err_msg=ctx + " terminated")
        np.testing.assert_array_equal(trunc.cpu().numpy(), (timesteps >= MAXT).astype(np.uint8), err_msg=ctx + " truncated")
        np.testing.assert_array_equal(info["invalid_action"].cpu().numpy(), ~valid, err_msg=ctx + " interception")
        np.testing.assert_array_equal(info["network_availability"].cpu().numpy().view(np.uint64), o["availability"].view(np.uint64),
                                      err_msg=ctx + " availability bits")
        np.testing.assert_array_equal(info["step_count"].cpu().numpy(), o["step_count"], err_msg=ctx + " step_count")
        dones = (o["terminated"] != 0) | (timesteps >= MAXT)
        sla |= En.reason(o, env.spec) == "sla"
        av = o["availability"][valid & (o["availability"] < full)]
        below += av.size
        values.update(av.tolist())
        for i in np.flatnonzero(dones):
            orc.reset(int(i))
        timesteps[dones] = 0
        n_disc = obs["discovered_node_count"].cpu().numpy().astype(np.int64)
    assert below >= 200 and len(values) >= 5 and int(sla.sum()) >= 8, \
        f"{below} availabilities below full of {len(values)} values, {int(sla.sum())} envs ended by SLA"
    env.close()
