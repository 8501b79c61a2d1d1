"""The scripts of tests/endings.py reach what they claim, from the CPU oracle alone: tests/test_gpu_episode_endings.py replays them on
every step-kernel layout, and a script whose episodes never end by goal, by eviction or by the SLA would compare nothing there.

Every condition is asserted, none is merely reported:

  * each reason a spec is meant to produce (endings.MEANT) ends at least 8 different envs, on every topology;
  * the classifier endings.reason (outputs of one step) agrees with endings.derive (the goals restated from the terminal state of a
    second oracle: owned count from the privileges, availability, cumulative reward before the step), at every env and step;
  * `updown`: some env's hidden counter goes to 2 or more, comes down by a re-image, goes up again at a later step, and the episode
    ends only after that; at least 8 evictions happen in envs that had owned 2 or more nodes earlier in that episode.  (`mixed` cannot
    show this between steps: with own_atleast=2, two owned nodes at the end of a step are the win.  `updown` is `mixed` with three
    nodes to win and a defender that re-images more often.)
  * cooperative layouts (random_net 100: G = 2, random_net 129: G = 4): on some step two envs of one wavefront end together, and
    some ending falls into the last, partial wavefront;
  * `mixed`: a win on the step where step_count == max_episode_steps, truncated staying 0; `reward`: a win with the cumulative reward
    equal to R; `reward_def`: an env with the reward reached that has to wait for the availability; `sla_evict`: an SLA win on a step
    that leaves no node owned;
  * `pct_*`: the owned count each threshold needs, from fractions.Fraction, is k, k, k + 1, and no env wins with fewer;
  * `frozen`: ended envs return reward 0, their old flags and step count until the reset by hand, and end again after it.
"""
import numpy as np
import pytest

from tests import endings as En

CASES = [f"{t}-{s}" for t in En.TOPOLOGIES for s in En.SPECS]
COOP_LANES = {"random100": 2, "random129": 4}


@pytest.mark.parametrize("name", CASES)
def test_script_reaches_what_it_claims(name):
    c = En.case(name)
    topo_name, spec_name = name.split("-")
    r = c.reasons()
    counts = c.envs_by_reason()
    print(f"{name}: envs (endings) by reason {counts} {c.params}")
    assert c.shadow_equal, "the hand-reset oracle diverged from the recording one"
    np.testing.assert_array_equal(r, En.derive(c), err_msg="classifier vs the goals restated from the terminal state")
    for why in En.MEANT[spec_name]:
        assert counts[why][0] >= 8, f"{why} ends {counts[why][0]} envs"
    ended = c.ended
    assert np.array_equal(ended, r != "")
    won = (r == "goal") | (r == "sla")
    assert np.all(c.out["reward"][won] == En.WIN) and np.all(c.out["reward"][r == "evicted"] == En.LOSE)
    assert not np.any(ended & (c.out["oob"] != 0) & (r != "truncated")), "an out-of-bound step ended by goal"
    assert int(c.out["oob"].sum()) >= 8

    if spec_name == "updown":
        assert int((ended & c.up_down_up).any(axis=0).sum()) >= 1, "no env's counter went up, down and up again before its episode ended"
        assert int((ended & (r == "evicted") & c.had_two).sum()) >= 8, "evictions after two or more owned nodes"
    if topo_name in COOP_LANES:
        per_wave = 64 // COOP_LANES[topo_name]
        wave = np.arange(En.E) // per_wave
        together = max(int(np.bincount(wave[ended[t]], minlength=wave[-1] + 1).max()) for t in range(ended.shape[0]))
        assert together >= 2, "no step ends two envs of one wavefront"
        assert En.E % per_wave and ended[:, wave == wave[-1]].any(), "no ending in the last, partial wavefront"
    if spec_name in ("mixed", "frozen"):
        at_bound = (r == "goal") & (c.out["step_count"] == c.spec.max_episode_steps)
        assert at_bound.any() and not c.out["truncated"][at_bound].any(), "no win on the step of the truncation bound"
    if spec_name == "reward":
        assert ((r == "goal") & (c.cum_before == c.params["R"])).any(), "no win with the cumulative reward equal to R"
        assert not ((r == "goal") & (c.cum_before < c.params["R"])).any()
    if spec_name == "reward_def":
        waits = c.live & (c.cum_before >= c.params["R"]) & (c.out["oob"] == 0) & (r == "") & (c.out["availability"] >= 1.0)
        assert waits.any(), "no env had to wait for the availability to drop"
    if spec_name == "sla_evict":
        both = (r == "sla") & (c.owned_after == 0)
        assert both.any(), "SLA and eviction never met on one step"
        assert np.all(c.out["reward"][both] == En.WIN) and not (r == "evicted").any()
    if spec_name.startswith("pct_"):
        N, k = c.topo.n_nodes, c.params["k"]
        pct = c.spec.attacker_goal["own_atleast_percent"]
        assert {s: En.needed_owned(v, N) for s, (v, _) in En.percent_values(k, N).items()} == {"pct_eq": k, "pct_below": k, "pct_above": k + 1}
        assert En.needed_owned(pct, N) == c.params["need"]
        assert int(c.owned_after[r == "goal"].min()) == c.params["need"]
    if spec_name == "frozen":
        idle = ~c.live
        assert idle.any() and np.all(c.out["reward"][idle] == 0.0) and np.all(c.out["raw_reward"][idle] == 0.0)
        for t in np.flatnonzero(idle.any(axis=1)):
            e = idle[t]
            for k in ("terminated", "truncated", "step_count"):
                np.testing.assert_array_equal(c.out[k][t][e], c.out[k][t - 1][e], err_msg=f"step {t}: {k} of frozen envs")
        wave = np.arange(En.E) // 64
        assert any((idle[t] & (wave == w)).any() and (c.live[t] & (wave == w)).any() for t in range(c.reset_at) for w in range(wave[-1] + 1)), \
            "no wavefront neighbour kept going next to a frozen env"
        assert counts["evicted"][0] >= 1          # two short episodes per env: evictions stay rare on the large topologies
        assert int(c.reset_mask.sum()) >= 8 and ended[c.reset_at:].any(), "nothing ended again after the reset by hand"


def test_classifier_on_hand_made_outputs():
    """endings.reason on one step's outputs written by hand: each reason, the order of precedence, and a defender-less spec (no SLA)."""
    topo = En.topology("toyctf")
    spec = En.make_spec(topo, defender=En.SCAN, maintain_sla=0.5)
    out = dict(terminated=np.array([0, 1, 1, 1, 0, 1], np.uint8), truncated=np.array([0, 0, 0, 0, 1, 0], np.uint8),
               reward=np.array([3.0, En.WIN, En.WIN, En.LOSE, 0.0, En.WIN]), availability=np.array([1.0, 0.4, 0.5, 0.4, 0.4, 1.0]))
    assert En.reason(out, spec).tolist() == ["", "sla", "goal", "evicted", "truncated", "goal"]
    assert En.reason(out, En.make_spec(topo, defender=None, maintain_sla=0.5)).tolist() == ["", "goal", "goal", "evicted", "truncated", "goal"]
