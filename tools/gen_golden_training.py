#!/usr/bin/env python
"""Golden traces of the two-agent TRAINING loop, captured from the UNMODIFIED reference wrappers
(marlon/baseline_models/env_wrappers/attack_wrapper.py, defend_wrapper.py, action_masking.py) over one shared reference CyberBattleEnv,
in the call order of marl_algorithm.collect_rollouts (marlon/baseline_models/multiagent/marl_algorithm.py:17-54; that module itself
needs Stable-Baselines3 and cannot be imported).  Build container only, never imported by a test:

    python tools/gen_golden_training.py        ->  tests/golden/wrap_training_*.npz

Each agent's `.env` there is a DummyVecEnv, which resets its wrapper inside step_wait as soon as the wrapper reports done; a reset on
one side reaches the other through reset_request (attack_wrapper.py:342-343, 433-435; defend_wrapper.py:269-271, 446-447, 479-482).
The loop below issues exactly those calls on the reference's own objects — wired, and the defender re-bound to the live environment
after every reset (quirk Q14), as oracle/refharness/gen_golden_wrappers.py run_two_agent_episodes does — and records what they return.
There is no `break` and no `on_reset(0)` between episodes: the loop never stops, as in training.

Data only.  Per turn, for both sides: action, reward, terminated, truncated, invalid / valid, every non-mask observation field returned
(the three mask fields as CRC32 and sum of the flat Discrete mask), both reset_request flags before the step, timesteps and counts after
the turn, the last_*_action_count pairs; the first (fresh) observations once — every later reset observation is asserted equal to them.
The Discrete trace steps through MaskedDiscreteAttackerWrapper and records CRC32 and sum of action_masks() BEFORE each attacker step:
after a defender-side reset that mask is the one of the episode that is gone (action_masking.py:90-94).
"""
from __future__ import annotations

import json
import os
import sys
import zlib

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(REPO, "oracle", "refharness"))
import gen_golden_wrappers as W  # noqa: E402  (loads the reference exactly as the wrapper traces do)

G, ref = W.G, W.ref
OBS = ["leaked_credentials", "credential_cache_matrix", "discovered_nodes_properties", "nodes_privilegelevel"]
DKEYS = ["infected_nodes", "incoming_firewall_status", "outgoing_firewall_status", "services_status"]


def flat_mask(obs):
    return np.concatenate([np.asarray(obs[k], np.int8).reshape(-1) for k in ("connect", "local_vulnerability", "remote_vulnerability")])


def snap(obs):
    out = {k: np.asarray(obs[k], np.int32) for k in OBS}
    out["scalars"] = np.array([int(obs[k]) for k in W.SCALARS], np.int32)
    m = flat_mask(obs)
    out["mask_crc"], out["mask_sum"] = zlib.crc32(m.tobytes()), int(m.sum())
    return out


def dsnap(dobs):
    return {k: np.asarray(dobs[k], np.int8) for k in DKEYS}


def run_training(name, make_cyber_env, spec, turns, seed, a_max, d_max, discrete=False, p_in_range=0.85):
    from marlon.baseline_models.env_wrappers.defend_wrapper import DefenderEnvWrapper
    from marlon.baseline_models.env_wrappers.environment_event_source import EnvironmentEventSource
    rng = np.random.Generator(np.random.PCG64(seed))
    cyber = make_cyber_env()
    events = EnvironmentEventSource()
    aw = W.AttackerEnvWrapper(cyber, event_source=events, max_timesteps=a_max, invalid_action_reward_modifier=-1)
    dw = DefenderEnvWrapper(cyber, attacker_reward_store=aw, event_source=events, defender=True, max_timesteps=d_max,
                            invalid_action_reward=-1, reset_on_constraint_broken=True, loss_reward=-5000.0)
    m = W.MaskedDiscreteAttackerWrapper(aw) if discrete else None

    def rebind():
        dw._actuator = cyber._defender_actuator
        dw.defender._actuator = cyber._defender_actuator
        dw.defender._environment = cyber.environment

    def attacker_env_reset():      # DummyVecEnv.reset / the auto-reset inside step_wait
        obs, _ = (m or aw).reset()
        rebind()
        return obs

    def defender_env_reset():
        dobs, _ = dw.reset()
        rebind()
        dw._prev_network_availability = float(dw._actuator.network_availability)
        dw.last_availability = dw._prev_network_availability
        return dw.observe()

    nvec_a, nvec_d = np.asarray(aw.action_space.nvec), np.asarray(dw.action_space.nvec)
    N, L, R, P, C = (int(nvec_a[i]) for i in (1, 2, 5, 8, 9))
    nodes = list(cyber.environment.network.nodes)
    first = snap(attacker_env_reset())               # setup_learn: attacker env.reset(), then defender env.reset()
    dfirst = dsnap(defender_env_reset())
    assert not aw.reset_request and not dw.reset_request
    names = (["a_action", "a_reward", "a_terminated", "a_truncated", "a_invalid", "a_request", "a_mask_crc_before", "a_mask_sum_before",
              "a_mask_crc", "a_mask_sum", "a_timesteps", "a_valid_count", "a_invalid_count", "a_last_valid", "a_last_invalid", "a_scalars"]
             + ["a_" + k for k in OBS]
             + ["d_action", "d_reward", "d_terminated", "d_truncated", "d_valid", "d_availability", "d_request", "d_timesteps", "d_valid_count",
                "d_invalid_count", "d_last_valid", "d_last_invalid"] + ["d_" + k for k in DKEYS])
    rec = {k: [] for k in names}
    for _ in range(turns):
        # ---- the action law of run_two_agent_episodes ----
        a = (rng.random(10) * nvec_a).astype(np.int64)
        nd = len(cyber._CyberBattleEnv__discovered_nodes)
        if rng.random() < p_in_range:
            for i in (1, 3, 4, 6, 7):
                a[i] = rng.integers(0, nd)
            a[9] = rng.integers(0, max(1, len(cyber._CyberBattleEnv__credential_cache)))
        if discrete:                 # the same action as the Discrete index of action_masking.py:107-136
            if a[0] == 2:
                act = ((int(a[6]) * N + int(a[7])) * P + int(a[8])) * C + int(a[9])
            elif a[0] == 0:
                act = N * N * P * C + int(a[1]) * L + int(a[2])
            else:
                act = N * N * P * C + N * L + (int(a[3]) * N + int(a[4])) * R + int(a[5])
            before = m.action_masks().astype(np.int8)
            rec["a_mask_crc_before"].append(zlib.crc32(before.tobytes())); rec["a_mask_sum_before"].append(int(before.sum()))
        else:
            act = a
            rec["a_mask_crc_before"].append(0); rec["a_mask_sum_before"].append(0)
        rec["a_request"].append(int(bool(aw.reset_request)))
        assert not dw.reset_request
        # ---- attacker.perform_step ----
        obs, r1, term1, trunc1, info = m.step(np.int64(act)) if discrete else aw.step(act)
        s = snap(obs)
        rec["a_action"].append(act); rec["a_reward"].append(float(r1)); rec["a_terminated"].append(int(bool(term1)))
        rec["a_truncated"].append(int(bool(trunc1))); rec["a_invalid"].append(int(bool(info.get("invalid_action", False))))
        rec["a_mask_crc"].append(s["mask_crc"]); rec["a_mask_sum"].append(s["mask_sum"]); rec["a_scalars"].append(s["scalars"])
        for k in OBS:
            rec["a_" + k].append(s[k])
        if term1 or trunc1:
            r = snap(attacker_env_reset())
            for k in OBS + ["scalars", "mask_crc"]:
                assert np.array_equal(r[k], first[k]), f"{name}: a reset observation differs from the first one in {k}"
        # ---- defender.perform_step ----
        d = (rng.random(12) * nvec_d).astype(np.int64)
        if rng.random() < 0.3:
            owned = [i for i, n in enumerate(nodes) if cyber.environment.get_node(n).agent_installed]
            d[0] = 0
            d[1] = int(rng.choice(owned)) if owned and rng.random() < 0.7 else d[1]
        rec["d_request"].append(int(bool(dw.reset_request)))
        dobs, r2, term2, trunc2, _ = dw.step(d)
        ds = dsnap(dobs)
        rec["d_action"].append(d); rec["d_reward"].append(float(r2)); rec["d_terminated"].append(int(bool(term2)))
        rec["d_truncated"].append(int(bool(trunc2))); rec["d_valid"].append(int(bool(dw.last_action_valid)))
        rec["d_availability"].append(float(dw.last_availability))
        for k in DKEYS:
            rec["d_" + k].append(ds[k])
        if term2 or trunc2:
            rs = dsnap(defender_env_reset())
            for k in DKEYS:
                assert np.array_equal(rs[k], dfirst[k]), f"{name}: a defender reset observation differs from the first one in {k}"
        # ---- after the turn ----
        rec["a_timesteps"].append(int(aw.timesteps)); rec["a_valid_count"].append(int(aw.valid_action_count))
        rec["a_invalid_count"].append(int(aw.invalid_action_count)); rec["a_last_valid"].append(int(aw.last_valid_action_count))
        rec["a_last_invalid"].append(int(aw.last_invalid_action_count))
        rec["d_timesteps"].append(int(dw.timesteps)); rec["d_valid_count"].append(int(dw.valid_action_count))
        rec["d_invalid_count"].append(int(dw.invalid_action_count)); rec["d_last_valid"].append(int(dw.last_valid_action_count))
        rec["d_last_invalid"].append(int(dw.last_invalid_action_count))
    out = {k: np.asarray(v) for k, v in rec.items()}
    for k in ("a_mask_crc_before", "a_mask_crc"):
        out[k] = out[k].astype(np.uint32)
    for k in ("a_terminated", "a_truncated", "a_invalid", "a_request", "d_terminated", "d_truncated", "d_valid", "d_request"):
        out[k] = out[k].astype(np.uint8)
    for k in OBS + ["scalars"]:
        out["first_a_" + k] = first[k]
    out["first_a_mask_crc"] = np.uint32(first["mask_crc"])
    for k in DKEYS:
        out["first_d_" + k] = dfirst[k]
    out["spec_json"] = np.frombuffer(json.dumps(dict(spec, max_timesteps=a_max, defender_max_timesteps=d_max, discrete=bool(discrete))).encode(),
                                     dtype=np.uint8)
    path = os.path.join(G.GOLDEN, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 100 * 1024, f"{name}: {size} bytes: shorten the trace"
    c = counts(out, a_max)
    print(f"{name:30s} turns={turns} {a_max}/{d_max} {c} size={size / 1024:.0f} KiB")
    return c


def counts(z, a_max):
    """What the whole set must contain (main() asserts the sums)."""
    a_done = (z["a_terminated"] | z["a_truncated"]) != 0
    d_done = (z["d_terminated"] | z["d_truncated"]) != 0
    q = z["a_request"] != 0
    own = d_done & (z["d_request"] == 0)                          # episodes the defender ended on its own
    # the attacker's clock before its reset: timesteps after the turn is 0 where it ended, so count from the trace
    ts, t = [], 0
    for i in range(len(q)):
        t += 1
        ts.append(t)
        if a_done[i]:
            t = 0
    timeout = np.asarray(ts) >= a_max
    return dict(attacker_ended=int((a_done & ~q).sum()), defender_ended=int(own.sum()), defender_terminated=int((own & (z["d_terminated"] != 0)).sum()),
                defender_timed_out=int((own & (z["d_terminated"] == 0)).sum()), request_intercepted=int((q & (z["a_invalid"] != 0)).sum()),
                request_positive=int((q & (z["a_reward"] > 0)).sum()), timeout_meets_request=int((q & timeout).sum()),
                attacker_terminated=int((z["a_terminated"] != 0).sum()))


def main():
    AG, DC = ref.env.AttackerGoal, ref.env.DefenderConstraint
    sp = dict(maximum_node_count=12, maximum_total_credentials=10, maximum_discoverable_credentials_per_action=5,
              attacker_goal=dict(reward=0.0, low_availability=1.0, own_atleast=6, own_atleast_percent=1.0),
              winning_reward=5000.0, losing_reward=-5000.0, maintain_sla=0.60, defender=["external"])

    def toyctf_marl():   # multiagent_universe.py:160-165: no in-env defender_agent, SLA 0.60, losing_reward -5000
        return ref.CyberBattleToyCtf(attacker_goal=AG(own_atleast=6), defender_constraint=DC(maintain_sla=0.60), losing_reward=-5000.0,
                                     maximum_node_count=12, maximum_total_credentials=10, throws_on_invalid_actions=False)
    total = {}
    for c in (run_training("wrap_training_toyctf_s81", toyctf_marl, sp, 500, 81, 40, 60),
              run_training("wrap_training_toyctf_discrete_s82", toyctf_marl, sp, 500, 82, 300, 25, discrete=True),
              run_training("wrap_training_toyctf_s83", toyctf_marl, sp, 500, 83, 12, 100, p_in_range=0.5),
              run_training("wrap_training_toyctf_s84", toyctf_marl, sp, 500, 84, 30, 30)):
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
    print("whole set:", total)
    need = dict(attacker_ended=10, defender_ended=10, defender_terminated=1, defender_timed_out=5, request_intercepted=2, request_positive=1,
                timeout_meets_request=5)
    for k, v in need.items():
        assert total[k] >= v, f"the set has {total[k]} of {k}, needs {v}: pick other seeds"


if __name__ == "__main__":
    main()
