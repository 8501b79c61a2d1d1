#!/usr/bin/env python3
"""The joint turn of marlon's two learned agents as ONE launch (TwoAgentVecEnv.step, mcbs_two_agent_step) against the two launches it
replaces (AttackerVecEnv.step; DefenderVecEnv.step), ToyCtf @12/10, Discrete, materialize_masks=False, in ONE process:

  (a) turn      : `att.step; dfd.step` | `TwoAgentVecEnv.step` (no episode block) | the same with an episode block — device events
                  around blocks of turns, BLOCKS x TURNS >= 2 000 turns per form and repeat, the forms alternating block by block,
                  three repeats: us per turn of each repeat;
  (b) loop body : one iteration of run_episode's loop body | of run_episode_joint's (sync_every 16), the same device-side random
                  policies — host clock ending in a synchronise: this is where the glue kernels and the per-turn host look show.

Every block starts from freshly reset wrappers (outside the timed span): with auto_reset=False envs end for good, and a batch of ended
envs is not the workload.  One JSON line per size and form.
    python tools/bench_two_agent_turn.py [envs ...]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from marlon_amd.samples import toy_ctf  # noqa: E402
from marlon_amd.simulate import random_defender_policy  # noqa: E402
from marlon_amd.wrappers import AttackerVecEnv, DefenderVecEnv, TwoAgentVecEnv  # noqa: E402

SIZES = [int(a) for a in sys.argv[1:]] or [16384, 65536]
BLOCKS, TURNS, REPEATS = 8, 250, 3          # (a): 2 000 turns per form and repeat
LOOP_BLOCKS, LOOP_TURNS = 4, 128            # (b): 512 iterations per form and repeat
MAX_T = 100000                              # neither wrapper truncates inside a block


def spread(xs):
    return dict(us=[round(x, 2) for x in xs], median_us=round(statistics.median(xs), 2), min_us=round(min(xs), 2), max_us=round(max(xs), 2))


def main():
    for E in SIZES:
        att = AttackerVecEnv(toy_ctf.new_environment(), E, maximum_node_count=12, maximum_total_credentials=10, discrete=True, learned_defender=True,
                             materialize_masks=False, auto_reset=False, max_timesteps=MAX_T)
        dfd = DefenderVecEnv(att, max_timesteps=MAX_T)
        joint = TwoAgentVecEnv(att, dfd)
        dev = att.engine.device
        g = torch.Generator(device=dev).manual_seed(0)
        a_acts = [torch.randint(0, att.discrete_n, (E,), generator=g, device=dev) for _ in range(8)]
        nv = torch.as_tensor(dfd.nvec, device=dev)
        d_acts = [(torch.rand((E, 12), generator=g, device=dev) * nv).long() for _ in range(8)]

        def fresh():
            att.reset()
            dfd.reset()
            torch.cuda.synchronize(dev)

        # ---------------- (a) the turn itself ----------------
        def turn_sequential(i, ep):
            att.step(a_acts[i & 7])
            dfd.step(d_acts[i & 7])

        def turn_joint(i, ep):
            joint.step(a_acts[i & 7], d_acts[i & 7])

        def turn_joint_episode(i, ep):
            joint.step(a_acts[i & 7], d_acts[i & 7], episode=ep)
        forms = (("sequential", turn_sequential), ("joint", turn_joint), ("joint_episode", turn_joint_episode))
        for _, f in forms:                                        # warm-up: output rings, bound calls
            fresh()
            ep = joint.episode_state()
            for i in range(16):
                f(i, ep)
        results = {name: [] for name, _ in forms}
        for _ in range(REPEATS):
            ms = {name: 0.0 for name, _ in forms}
            for _ in range(BLOCKS):
                for name, f in forms:
                    fresh()
                    ep = joint.episode_state()
                    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    for i in range(TURNS):
                        f(i, ep)
                    end.record()
                    end.synchronize()
                    ms[name] += start.elapsed_time(end)
            for name in ms:
                results[name].append(ms[name] * 1e3 / (BLOCKS * TURNS))
        for name, _ in forms:
            print(json.dumps(dict(measure="turn, device events", envs=E, form=name, turns_per_repeat=BLOCKS * TURNS, **spread(results[name]))), flush=True)

        # ---------------- (b) one iteration of the episode drivers' loops ----------------
        d_pol = random_defender_policy(1)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        state = {}

        def a_pol(step):
            return att.sample_masked_uniform(seed=0, step=step).actions

        def loop_start():
            fresh()
            state.update(alive=torch.ones(E, dtype=torch.bool, device=dev), lengths=torch.zeros(E, dtype=torch.int64, device=dev),
                         a_done=torch.zeros(E, dtype=torch.bool, device=dev), d_done=torch.zeros(E, dtype=torch.bool, device=dev),
                         a_rew=[], d_rew=[], ep=joint.episode_state(), n=0)

        def body_run_episode(i):                                  # simulate.run_episode's loop body, statement for statement
            alive = state["alive"]
            actions1 = a_pol(i)
            _, r1, term1, trunc1, _ = att.step(actions1)
            dones1 = ((term1 | trunc1) != 0) & alive
            r1 = torch.where(alive, r1.double(), zero)
            state["a_rew"].append(r1)
            actions2 = torch.as_tensor(d_pol(dfd), device=dev).long().clone()
            actions2[~alive | dones1, 0] = -2
            _, r2, term2, trunc2, _ = dfd.step(actions2)
            stepped = alive & ~dones1
            dones2 = (((term2 | trunc2) != 0) & stepped) | dones1
            r2 = torch.where(stepped, r2, torch.where(dones1, -r1, zero))
            state["d_rew"].append(r2)
            state["lengths"] += alive
            ended = dones1 | dones2
            state["a_done"] |= dones1
            state["d_done"] |= dones2 & alive
            state["alive"] = alive & ~ended
            bool(state["alive"].any())                            # (the loop's look at the host; the bench goes on either way)

        def body_run_episode_joint(i, sync_every=16):             # simulate.run_episode_joint's
            row = state["n"] % sync_every
            if row == 0:
                state["a_rew"].append(torch.zeros((sync_every, E), dtype=torch.float64, device=dev))
                state["d_rew"].append(torch.zeros((sync_every, E), dtype=torch.float64, device=dev))
            actions1 = a_pol(i)
            actions2 = d_pol(dfd)
            joint.step(actions1, actions2, episode=state["ep"], reward_rows=(state["a_rew"][-1][row], state["d_rew"][-1][row]))
            state["n"] += 1
            if state["n"] % sync_every == 0:
                bool(state["ep"].alive.any())
        loops = (("run_episode", body_run_episode), ("run_episode_joint", body_run_episode_joint))
        for _, f in loops:
            loop_start()
            for i in range(16):
                f(i)
        results = {name: [] for name, _ in loops}
        for _ in range(REPEATS):
            sec = {name: 0.0 for name, _ in loops}
            for _ in range(LOOP_BLOCKS):
                for name, f in loops:
                    loop_start()
                    t0 = time.perf_counter()
                    for i in range(LOOP_TURNS):
                        f(i)
                    torch.cuda.synchronize(dev)
                    sec[name] += time.perf_counter() - t0
            for name in sec:
                results[name].append(sec[name] * 1e6 / (LOOP_BLOCKS * LOOP_TURNS))
        for name, _ in loops:
            print(json.dumps(dict(measure="episode loop iteration, host clock", envs=E, form=name, iterations_per_repeat=LOOP_BLOCKS * LOOP_TURNS,
                                  **spread(results[name]))), flush=True)
        att.close()


if __name__ == "__main__":
    main()
