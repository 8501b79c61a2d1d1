"""Episode endings on every step-kernel layout, against the CPU oracle, bitwise.

Every step kernel decides at the end of a step whether the episode is over (mcbs_step.hip and, copied by hand, mcbs_step_coop.hip),
from the cumulative reward, the availability, the host-derived goal_own_pct_min and the running counter `owned`, which each layout
keeps for itself, mcbs_get_state does not export and mcbs_set_state recomputes: no state comparison can see it drift.  The scripts of
tests/endings.py make episodes END on every layout, by every reason (tests/test_endings_script.py asserts that they do, from the
oracle alone), and each case here replays one of them.

| layout cell | topology | switches | variant asserted |
|---|---|---|---|
| packed | ToyCtf | | packed=1 |
| general1 | random_net 24 | | packed=0, words_per_set=1 |
| toyctf_general | ToyCtf | MCBS_NO_PACKED_SETS=1 | packed=0, words_per_set=1 |
| lane2 | random_net 100 | MCBS_NO_COOP=1 | words_per_set=2, coop=0 |
| coop2 | random_net 100 | | words_per_set=2, coop=1 (G = 2) |
| lane4 | random_net 129 | MCBS_NO_COOP=1 | words_per_set=4, coop=0 |
| coop4 | random_net 129 | | words_per_set=4, coop=1 (G = 4) |
| wide | ActiveDirectory-6 | | wide=1 |

| spec (endings.case) | what ends the episodes |
|---|---|
| mixed | own 2 nodes, eviction, truncation; the bound is a step count at which a first episode wins (done wins, truncated stays 0) |
| updown | own 3 nodes under a defender that re-images often: the counter goes up, down and up again inside an episode |
| frozen | mixed with auto_reset off: ended envs stay frozen next to running neighbours, then reset(mask) by hand |
| reward, reward_def | cumulative reward >= R, R met with equality; with a defender the goal waits for the availability |
| sla, lowavail, sla_evict | maintain_sla / low_availability just below 1; SLA and eviction on one step (the win takes precedence) |
| pct_eq, pct_below, pct_above | own_atleast_percent = k/N and its two neighbouring doubles (k, k and k + 1 nodes) |

| entry point | cells | test |
|---|---|---|
| step | all eight | test_step_ends_episodes_as_the_oracle |
| step_many, two launches with endings and re-initialisations inside | general1, lane2, lane4, wide | test_step_many_ends_episodes_as_the_oracle |
| step / step_observe / step_many alternating on ONE state (the cooperative kernel, the phase kernels and the looping one-lane kernel hand `owned` and the slack list entry to each other) | coop2, coop4 | test_cooperative_batch_alternates_entry_points |
| step_observe (goals evaluated in phase 2), small observation fields | lane2, wide | test_step_observe_ends_episodes_as_the_oracle |
| AttackerVecEnv (decode_step1_kernel / step2_finish_kernel) | general1, mixed | test_attacker_vec_env_endings_against_oracle |

Compared with the oracle, as bits: reward (fp64 of the fp32), raw_reward, terminated, truncated, out_of_bound, step_count and the
availability (uint64) of every step (step_many returns rewards and terminations only), and the canonical state after every step or
launch in which any env ended and after the last one: the reset image, the episode counter, the n_discovered / n_creds headers, the
cumulative reward.  The steps after a reset are checked like any other: the next episode's Philox draws are keyed by the new episode
index.  Output buffers are filled with sentinels before each launch.
"""
import numpy as np
import pytest

from tests import endings as En

pytestmark = pytest.mark.gpu

SMALL = ["scalars", "leaked_credentials", "credential_cache_matrix", "discovered_nodes_properties", "nodes_privilegelevel"]

# cell: (topology, environment switches read at batch creation, variant)
CELLS = {
    "packed": ("toyctf", {}, dict(packed=1, words_per_set=1, wide=0, coop=0, lds_topo=0)),
    "general1": ("random24", {}, dict(packed=0, words_per_set=1, wide=0, coop=0, lds_topo=0)),
    "toyctf_general": ("toyctf", {"MCBS_NO_PACKED_SETS": "1"}, dict(packed=0, words_per_set=1, wide=0, coop=0, lds_topo=0)),
    "lane2": ("random100", {"MCBS_NO_COOP": "1"}, dict(packed=0, words_per_set=2, wide=0, coop=0, lds_topo=0)),
    "coop2": ("random100", {}, dict(packed=0, words_per_set=2, wide=0, coop=1, lds_topo=0)),
    "lane4": ("random129", {"MCBS_NO_COOP": "1"}, dict(packed=0, words_per_set=4, wide=0, coop=0, lds_topo=0)),
    "coop4": ("random129", {}, dict(packed=0, words_per_set=4, wide=0, coop=1, lds_topo=0)),
    "wide": ("ad6", {}, dict(packed=0, wide=1, coop=0, lds_topo=0)),
}


def _engine():
    from marlon_amd import engine
    return engine


def _create(cell, spec_name, monkeypatch, topo_name=None):
    """The case's script and a batch on the cell's layout (variant asserted: a moved threshold fails loudly).  topo_name: another
    topology than the cell's own (it must land on the same layout)."""
    own, switches, want = CELLS[cell]
    c = En.case(f"{topo_name or own}-{spec_name}")
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    eng = _engine().BatchEngine(c.topo, c.spec)
    for k in switches:
        monkeypatch.delenv(k)
    v = eng.variant()
    got = {k: v[k] for k in want}
    assert got == want and v["defender_kind"] == (1 if c.spec.defender else 0), f"batch dispatches to {v}, the test expects {want}"
    return c, eng


def _compare_states(a, b, ctx):
    for x, y, what in zip(a, b, ("header", "nodes", "order", "cache")):
        if x.dtype.names:
            for f in x.dtype.names:
                if not f.startswith("pad"):
                    np.testing.assert_array_equal(x[f], y[f], err_msg=f"{ctx}: state {what}.{f}")
        else:
            np.testing.assert_array_equal(x, y, err_msg=f"{ctx}: state {what}")


def _sentinels(eng):
    eng.reward.fill_(-12345.0)
    eng.terminated.fill_(0xA5)
    eng.info["network_availability"].fill_(-3.0)
    eng.info["step_count"].fill_(-7)
    eng.info["truncated"].fill_(0xA5)
    eng.info["out_of_bound"].fill_(0xA5)
    eng.info["raw_reward"].fill_(-12345.0)


def _compare_step(eng, r, d, want, t, ctx):
    np.testing.assert_array_equal(r.double().cpu().numpy(), want["reward"][t], err_msg=ctx + " reward")
    np.testing.assert_array_equal(d.cpu().numpy(), want["terminated"][t], err_msg=ctx + " terminated")
    np.testing.assert_array_equal(eng.info["raw_reward"].double().cpu().numpy(), want["raw_reward"][t], err_msg=ctx + " raw reward")
    np.testing.assert_array_equal(eng.info["truncated"].cpu().numpy(), want["truncated"][t], err_msg=ctx + " truncated")
    np.testing.assert_array_equal(eng.info["out_of_bound"].cpu().numpy(), want["oob"][t], err_msg=ctx + " out_of_bound")
    np.testing.assert_array_equal(eng.info["step_count"].cpu().numpy(), want["step_count"][t], err_msg=ctx + " step_count")
    np.testing.assert_array_equal(eng.info["network_availability"].cpu().numpy().view(np.uint64), want["availability"][t].view(np.uint64),
                                  err_msg=ctx + " availability bits")


def _plan(c, cycle):
    """[(entry point, first row, rows)] covering the script with `cycle` repeated; no segment crosses the reset by hand or the end."""
    T = c.actions.shape[0]
    stops = sorted({T, c.reset_at} - {-1})
    plan, t, i = [], 0, 0
    while t < T:
        how, k = cycle[i % len(cycle)]
        k = min(k, next(s for s in stops if s > t) - t)
        plan.append((how, t, k))
        t, i = t + k, i + 1
    return plan


def _replay(c, eng, plan, ctx):
    """Run the plan on the engine and a live oracle (for the states); every output against the RECORDED outputs of the case."""
    from oracle.oracle import Oracle
    t_ = eng.torch
    orc = Oracle(c.topo, c.spec)
    acts = t_.as_tensor(c.actions, device=eng.device)
    ended, used = 0, set()
    for how, t0, k in plan:
        used.add(how)
        where = f"{ctx} {how} rows {t0}..{t0 + k - 1}"
        if t0 == c.reset_at:
            eng.reset(t_.as_tensor(c.reset_mask, device=eng.device))
            for i in np.flatnonzero(c.reset_mask):
                orc.reset(int(i))
            _compare_states(eng.get_state(), orc.get_state(), where + " after reset(mask)")
        any_end = bool(c.ended[t0:t0 + k].any())
        oo = None
        _sentinels(eng)
        if how == "many":
            rw = t_.full((k, c.spec.n_envs), -12345.0, dtype=t_.float32, device=eng.device)
            tm = t_.full((k, c.spec.n_envs), 0xA5, dtype=t_.uint8, device=eng.device)
            eng.step_many(acts[t0:t0 + k], rw, tm)
            np.testing.assert_array_equal(rw.double().cpu().numpy(), c.out["reward"][t0:t0 + k], err_msg=where + " rewards")
            np.testing.assert_array_equal(tm.cpu().numpy(), c.out["terminated"][t0:t0 + k], err_msg=where + " terminated")
        elif how == "observe":
            obs = eng.alloc_obs(SMALL)
            r, d = eng.step_observe(acts[t0], obs)
            _compare_step(eng, r, d, c.out, t0, where)
            oo = orc.alloc_obs(SMALL)
        else:
            r, d = eng.step(acts[t0])
            _compare_step(eng, r, d, c.out, t0, where)
        for t in range(t0, t0 + k):
            o = orc.step(c.actions[t], obs=oo)
            for key in En.OUT_KEYS:                                # the live oracle repeats the recording
                assert np.array_equal(o[key].view(np.uint8), c.out[key][t].view(np.uint8)), f"{where}: the oracle no longer returns the recorded {key}"
        if oo is not None and any_end:
            rows = np.flatnonzero(c.live[t0])                      # (an env frozen after its end is not observed anew)
            for f in SMALL:
                np.testing.assert_array_equal(obs[f].cpu().numpy()[rows], oo[f][rows], err_msg=f"{where} observation {f}")
        if any_end or t0 + k == c.actions.shape[0]:
            _compare_states(eng.get_state(), orc.get_state(), where)
        ended += int(c.ended[t0:t0 + k].sum())
    assert ended > 0
    return used


@pytest.mark.parametrize("spec_name", En.SPECS)
@pytest.mark.parametrize("cell", sorted(CELLS))
def test_step_ends_episodes_as_the_oracle(cell, spec_name, monkeypatch):
    """mcbs_step on every layout cell x every spec: every output of every step, the state after every step in which an env ended."""
    c, eng = _create(cell, spec_name, monkeypatch)
    _replay(c, eng, _plan(c, [("step", 1)]), f"{cell} {spec_name}")
    eng.close()


@pytest.mark.parametrize("spec_name", En.SPECS)
@pytest.mark.parametrize("cell", ["general1", "lane2", "lane4", "wide"])
def test_step_many_ends_episodes_as_the_oracle(cell, spec_name, monkeypatch):
    """mcbs_step_many (the looping kernel): the script in two launches, each with endings and re-initialisations inside it; rewards and
    terminations [K, E] and the state after each launch."""
    c, eng = _create(cell, spec_name, monkeypatch)
    T = c.actions.shape[0]
    plan = _plan(c, [("many", T if c.reset_at > 0 else (T + 1) // 2)])          # (frozen: the reset by hand is the cut)
    assert len(plan) == 2 and all(c.ended[t0:t0 + k].any() for _, t0, k in plan)
    _replay(c, eng, plan, f"{cell} {spec_name}")
    eng.close()


@pytest.mark.parametrize("spec_name", En.SPECS)
@pytest.mark.parametrize("cell", ["coop2", "coop4"])
def test_cooperative_batch_alternates_entry_points(cell, spec_name, monkeypatch):
    """One cooperative batch advanced in a fixed pattern of seven script rows — step (the G-lane kernel), step_observe (the phase-1 /
    phase-2 one-lane kernels), step_many over three rows (the looping one-lane kernel), step, step_observe — with nothing in between
    that would recompute `owned` or the lists' slack entry.  The counts of tests/test_endings_script.py are the oracle's and hold here
    as they do for any entry point: the same script is replayed."""
    c, eng = _create(cell, spec_name, monkeypatch)
    used = _replay(c, eng, _plan(c, [("step", 1), ("observe", 1), ("many", 3), ("step", 1), ("observe", 1)]), f"{cell} {spec_name}")
    assert used == {"step", "observe", "many"}
    eng.close()


@pytest.mark.parametrize("spec_name", En.SPECS)
@pytest.mark.parametrize("cell", ["lane2", "wide"])
def test_step_observe_ends_episodes_as_the_oracle(cell, spec_name, monkeypatch):
    """mcbs_step_observe on every step: the goals are evaluated in phase 2, from what phase 1 left pending.  The small observation
    fields are compared on the steps where envs end (the observation of the step that ended the episode)."""
    c, eng = _create(cell, spec_name, monkeypatch)
    _replay(c, eng, _plan(c, [("observe", 1)]), f"{cell} {spec_name}")
    eng.close()


def _multidiscrete(rows):
    """Engine rows [E, 5] as marlon's MultiDiscrete(10) attacker actions (attack_wrapper.py:206-227)."""
    a = np.zeros((rows.shape[0], 10), np.int64)
    k = rows[:, 0]
    a[:, 0] = k
    for kind, cols in ((0, (1, 2)), (1, (3, 4, 5)), (2, (6, 7, 8, 9))):
        for j, col in enumerate(cols):
            a[:, col] = np.where(k == kind, rows[:, 1 + j], 0)
    return a


def test_attacker_vec_env_endings_against_oracle():
    """AttackerVecEnv on a general one-word batch (fused_wrapper == 0: decode_step1_kernel, the observation, step2_finish_kernel) with
    the `mixed` goals: rows written by the host policy from the oracle's state, some intercepted (undiscovered index), the wrapper's
    own truncation and auto-reset.  Rewards, terminated, truncated, dones, the terminal observation rows, episode returns and lengths
    against the oracle plus the wrapper's bookkeeping restated here; goal, eviction and truncation each end at least 8 envs."""
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.cyberbattle_env import SCALAR_KEYS
    from marlon_amd.wrappers import AttackerVecEnv
    from oracle.oracle import Oracle
    topo = En.topology("random24")
    E, T, MAXT = 96, 150, 12
    Nm, Cm = topo.n_nodes, max(1, len(topo.triples))
    K = max(8, int(topo.header()["max_leak_per_action"]))
    env = AttackerVecEnv(topo, E, maximum_node_count=Nm, maximum_total_credentials=Cm, maximum_discoverable_credentials_per_action=K,
                         attacker_goal=ce.AttackerGoal(own_atleast=2, own_atleast_percent=0.0, low_availability=2.0),
                         defender_agent=ce.ScanAndReimageCompromisedMachines(0.5, 2, 3), defender_constraint=ce.DefenderConstraint(0.0),
                         winning_reward=En.WIN, losing_reward=En.LOSE, max_timesteps=MAXT, seed=4242, env_id_base=500, materialize_masks=False)
    v = env.engine.variant()
    assert (v["packed"], v["words_per_set"], v["wide"], v["fused_wrapper"], v["defender_kind"]) == (0, 1, 0, 0, 1), v
    assert env.engine.wrapper_step_launches(False) == 3
    orc = Oracle(topo, env.spec)
    orc.reset()                                          # the wrapper's reset() began episode 1
    pol = En.Policy(topo, env.spec, 19)
    timesteps, returns = np.zeros(E, np.int64), np.zeros(E, np.float64)
    n_disc = np.ones(E, np.int64)
    ends = {k: np.zeros(E, bool) for k in ("goal", "evicted", "truncated")}
    terminal_checked = after_reset = 0
    was_reset = np.zeros(E, bool)
    for t in range(T):
        rows = pol.rows(orc.get_state())
        a = _multidiscrete(rows)
        a = np.minimum(a, env.nvec - 1)                 # (the policy's far node index lies past the MultiDiscrete bound)
        kind = a[:, 0]
        src = np.where(kind == 0, a[:, 1], np.where(kind == 1, a[:, 3], a[:, 6]))
        tgt = np.where(kind == 0, 0, np.where(kind == 1, a[:, 4], a[:, 7]))
        valid = (src < n_disc) & ((kind == 0) | (tgt < n_disc))          # attack_wrapper.py:286-308
        played = np.zeros((E, 5), np.int32)
        played[:, 0] = np.where(valid, kind, 3)
        played[:, 1] = src
        played[:, 2] = np.where(kind == 0, a[:, 2], tgt)
        played[:, 3] = np.where(kind == 1, a[:, 5], np.where(kind == 2, a[:, 8], 0))
        played[:, 4] = np.where(kind == 2, a[:, 9], 0)
        oo = orc.alloc_obs(SMALL)
        obs, r, term, trunc, info = env.step(a)
        o = orc.step(played, obs=oo)
        timesteps += 1
        ctx = f"random24 wrapper step {t}"
        want_r = o["reward"] + np.where(valid, 0.0, -1.0)
        np.testing.assert_array_equal(r.double().cpu().numpy(), want_r, err_msg=ctx + " reward")
        np.testing.assert_array_equal(term.cpu().numpy(), o["terminated"], err_msg=ctx + " terminated")
        np.testing.assert_array_equal(trunc.cpu().numpy(), (timesteps >= MAXT).astype(np.uint8), err_msg=ctx + " truncated")
        np.testing.assert_array_equal(info["invalid_action"].cpu().numpy(), ~valid, err_msg=ctx + " interception")
        returns += want_r.astype(np.float32).astype(np.float64)
        dones = (o["terminated"] != 0) | (timesteps >= MAXT)
        why = En.reason(o, env.spec)
        ends["goal"] |= why == "goal"
        ends["evicted"] |= why == "evicted"
        ends["truncated"] |= (timesteps >= MAXT) & (o["terminated"] == 0)
        if dones.any():
            sel = np.flatnonzero(dones)
            np.testing.assert_array_equal(info["episode_return"].cpu().numpy()[sel], returns[sel], err_msg=ctx + " episode return")
            np.testing.assert_array_equal(info["episode_length"].cpu().numpy()[sel], timesteps[sel], err_msg=ctx + " episode length")
        for view, sel, what in ((env.observation, np.flatnonzero(valid & ~dones), "observation"),
                                (env.terminal_observation, np.flatnonzero(valid & dones), "terminal observation")):
            if not sel.size:
                continue
            got = np.stack([view[k].cpu().numpy() for k in SCALAR_KEYS], axis=1)
            np.testing.assert_array_equal(got[sel], oo["scalars"][sel], err_msg=f"{ctx} {what} scalars")
            for k in SMALL[1:]:
                np.testing.assert_array_equal(view[k].cpu().numpy().reshape(E, -1)[sel], oo[k].reshape(E, -1)[sel], err_msg=f"{ctx} {what} {k}")
            if what == "observation":
                after_reset += int(was_reset[sel].sum())
            else:
                terminal_checked += sel.size
        for i in np.flatnonzero(dones):
            orc.reset(int(i))
        was_reset |= dones
        timesteps[dones] = 0
        returns[dones] = 0.0
        n_disc = obs["discovered_node_count"].cpu().numpy().astype(np.int64)
        _, _, order, _ = orc.get_state()
        np.testing.assert_array_equal(n_disc, (order != 0xFFFF).sum(axis=1), err_msg=ctx + " discovered count after reset")
    counts = {k: int(v.sum()) for k, v in ends.items()}
    assert min(counts.values()) >= 8, f"envs ended by reason: {counts}"
    assert terminal_checked > 0 and after_reset > 0
    env.close()
