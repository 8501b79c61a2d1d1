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

The weighted cases (endings.WEIGHT_SPECS: unequal SLA weights, for tests/test_gpu_availability_weights.py) prove, per topology and
weight kind, that the availability they make the kernels compute tells the three ways of summing apart
(test_weighted_script_tells_the_sums_apart): the classification flatten.py makes, a NumPy fp64 restatement that agrees with the oracle
on every compared step, and enough steps on which a kernel that took another branch would return other bits.
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


@pytest.mark.parametrize("kind", En.WEIGHT_KINDS)
@pytest.mark.parametrize("topo_name", En.WEIGHT_TOPOLOGIES)
def test_weighted_script_tells_the_sums_apart(topo_name, kind):
    """From the oracle alone, for `avail`, `sla_eq` and `sla_up` of one topology and weight kind.  Compared pairs: (step, env) played,
    not ending the episode.  Conditions (each a lower bound set beforehand, the counts are in the messages):
      1  avail_any_order is 1 for dyadic, 0 for odd, and the terms are not all equal
      2  the node-order restatement (endings.availability_sums) has the oracle's bits on every compared pair, in all three cases
      a  >= 200 pairs with a node being re-imaged
      u  >= 100 pairs on which the uniform shortcut full_sum - n * term[0] gives other bits
      b  odd: >= 100 pairs on which full_sum - (terms of the nodes being re-imaged), subtracted one by one AND summed first, both give
         other bits than the node-order sum; dyadic: no pair on which either does (the claim of flatten.py)
      c  more than 64 nodes: >= 100 pairs whose re-imaging nodes lie in two or more 64-bit words
      d  >= 100 pairs with three or more nodes being re-imaged
      e  >= 8 envs end by SLA under sla_up on a step that sla_eq plays through with the same row, the availability being exactly v"""
    c = En.case(f"{topo_name}-avail_{kind}")
    h, term = c.topo.header(), c.topo.node_table()["avail_term"]
    N = c.topo.n_nodes
    assert int(h["avail_any_order"]) == (1 if kind == "dyadic" else 0)
    assert np.unique(term).size > 1, "every node has the same availability term"
    assert c.spec.maintain_sla == 0.0 and c.shadow_equal
    counts = c.envs_by_reason()
    assert counts["truncated"][0] >= 8 and not any(counts[k][1] for k in ("goal", "sla", "evicted")), f"avail: envs (endings) by reason {counts}"
    np.testing.assert_array_equal(c.reasons(), En.derive(c))

    bits = En._bits
    s = En.availability_sums(c)
    cmp_ = En.compared(c)
    order = bits(s["order"])
    agree = order == bits(c.out["availability"])
    n_cmp = int(cmp_.sum())
    assert n_cmp > 0 and int((agree & cmp_).sum()) == n_cmp, f"restatement agrees on {int((agree & cmp_).sum())} of {n_cmp} pairs"
    a = cmp_ & (s["n"] > 0)
    wrong_sub = (bits(s["sub_seq"]) != order) & (bits(s["sub_sum"]) != order)
    any_sub = (bits(s["sub_seq"]) != order) | (bits(s["sub_sum"]) != order)
    u = a & (bits(s["uniform"]) != order)
    words = sum(c.imaging[:, :, w:w + 64].any(axis=2).astype(np.int64) for w in range(0, N, 64))
    n = dict(a=int(a.sum()), u=int(u.sum()), b=int((a & wrong_sub).sum()), b_any=int((a & any_sub).sum()), c=int((a & (words >= 2)).sum()),
             d=int((a & (s["n"] >= 3)).sum()), sets=len({r.tobytes() for r in c.imaging[a]}))
    msg = f"{topo_name} {kind}: {n} over {n_cmp} compared pairs"
    print(msg)
    assert n["a"] >= 200 and n["u"] >= 100 and n["d"] >= 100, msg
    assert n["b"] >= 100 if kind == "odd" else n["b_any"] == 0, msg
    assert n["c"] >= 100 or N <= 64, msg
    assert np.array_equal(En.discriminating(c), (s["n"] > 0) & (bits(s["uniform"]) != order) & (wrong_sub | (kind == "dyadic")))

    eq, up = En.case(f"{topo_name}-sla_eq_{kind}"), En.case(f"{topo_name}-sla_up_{kind}")
    v = eq.params["v"]
    assert v < float(h["full_availability"]) and eq.spec.maintain_sla == v and up.spec.maintain_sla == float(np.nextafter(v, np.inf)) > v
    for k in (eq, up):
        assert k.shadow_equal
        np.testing.assert_array_equal(k.reasons(), En.derive(k))
        sk = En.availability_sums(k)
        ck = En.compared(k)
        assert np.array_equal(bits(sk["order"])[ck], bits(k.out["availability"])[ck]), f"{k.name}: restatement vs oracle"
    cand = En.sla_candidates(c, v)
    low = En.first_episode(c) & c.live & (c.out["oob"] == 0) & (c.out["availability"] <= v)
    t0 = np.argmax(low, axis=0)[cand]
    for k in (eq, up):                                            # the pilot's first episodes are the twins' up to the step in question
        assert all(np.array_equal(k.actions[:t + 1, e], c.actions[:t + 1, e]) for t, e in zip(t0, cand))
        assert np.all(k.out["availability"][t0, cand] == v) and np.all(En.discriminating(k)[t0, cand])
    ends_up = up.reasons()[t0, cand] == "sla"
    ends_eq = eq.ended[t0, cand]
    e_msg = f"{topo_name} {kind}: v = {v!r}, {cand.size} candidate envs, sla_up ends {int(ends_up.sum())} of them there, sla_eq {int(ends_eq.sum())}; " \
            f"envs (endings) by SLA: sla_eq {eq.envs_by_reason()['sla']}, sla_up {up.envs_by_reason()['sla']}"
    print(e_msg)
    assert int(ends_up.sum()) >= 8 and ends_up.all() and not ends_eq.any(), e_msg
    assert not (eq.ended & (eq.out["availability"] == v) & (eq.reasons() == "sla")).any(), "equality ended an episode"


def test_classifier_on_hand_made_outputs():
    """endings.reason on one step's outputs written by hand: each reason, the order of precedence, and a defender-less spec (no SLA)."""
    topo = En.topology("toyctf")
    spec = En.make_spec(topo, defender=En.SCAN, maintain_sla=0.5)
    out = dict(terminated=np.array([0, 1, 1, 1, 0, 1], np.uint8), truncated=np.array([0, 0, 0, 0, 1, 0], np.uint8),
               reward=np.array([3.0, En.WIN, En.WIN, En.LOSE, 0.0, En.WIN]), availability=np.array([1.0, 0.4, 0.5, 0.4, 0.4, 1.0]))
    assert En.reason(out, spec).tolist() == ["", "sla", "goal", "evicted", "truncated", "goal"]
    assert En.reason(out, En.make_spec(topo, defender=None, maintain_sla=0.5)).tolist() == ["", "goal", "goal", "evicted", "truncated", "goal"]
