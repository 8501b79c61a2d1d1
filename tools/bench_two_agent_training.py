#!/usr/bin/env python3
"""The two-agent TRAINING turn as ONE launch (TwoAgentTrainVecEnv.step, mcbs_two_agent_train_step) against the only way to run that
loop without it — the composition from existing calls (tests/training_compose.py: att.step, dfd.step, two masked engine resets, a masked
observation, dfd.reset and the masked tensor assignments between them) — and against TwoAgentVecEnv.step, the same turn without any
reset, as the floor.  ToyCtf @12/10, Discrete, materialize_masks=False (tools/bench_two_agent_turn.py's shapes), in ONE process:

  (a) turn            : training | composition | floor — device events around blocks of turns, BLOCKS x TURNS = 2 000 turns per leg and
                        repeat, the legs alternating block by block, three repeats: us per turn of each repeat.  The training legs
                        truncate at 40 / 60 wrapper steps (the reference's order of magnitude: every turn ~4 % of the envs end on one side
                        or the other); the floor never ends an episode.  Every block starts from freshly reset wrappers.
                        The same blocks also time the turn that writes PACKED rows (a pair of observation_format="packed" wrappers,
                        mcbs_two_agent_train_step_packed) and what a rollout that stores packed rows pays per turn on either pair:
                          training_turn_packed            the packed turn, bare
                          training_turn+pack_launches     the dense turn, then att.observation_packed(out=) and dfd.observation_packed(out=)
                                                          into rollout-buffer rows: two pack launches that read the dense rows back
                          training_turn_packed+row_copies the packed turn, then the same two calls: row copies;
  (b) collect_rollouts: one iteration of simulate.collect_rollouts (64-step buffers) with device-side random policies
                        (sample_masked_uniform, sample_uniform) — host clock ending in a synchronise: the dense pair with dense buffers,
                        then the dense and the packed pair with rollout_buffer(pack_observations=True) buffers.

One JSON line per size and leg.
    python tools/bench_two_agent_training.py [envs ...]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from marlon_amd.samples import toy_ctf  # noqa: E402
from marlon_amd.simulate import collect_rollouts  # noqa: E402
from marlon_amd.wrappers import AttackerVecEnv, DefenderVecEnv, TwoAgentTrainVecEnv, TwoAgentVecEnv  # noqa: E402
from tests.training_compose import ComposedTrainingTurn  # noqa: E402

SIZES = [int(a) for a in sys.argv[1:]] or [16384, 65536]
BLOCKS, TURNS, REPEATS = 8, 250, 3
ATT_T, DEF_T = 40, 60
ROLLOUT_STEPS, ROLLOUTS = 64, 4


def spread(xs):
    return dict(us=[round(x, 2) for x in xs], median_us=round(statistics.median(xs), 2), min_us=round(min(xs), 2), max_us=round(max(xs), 2))


def pair(E, auto_reset, att_T, def_T, packed=False):
    att = AttackerVecEnv(toy_ctf.new_environment(), E, maximum_node_count=12, maximum_total_credentials=10, discrete=True, learned_defender=True,
                         materialize_masks=False, auto_reset=auto_reset, max_timesteps=att_T, observation_format="packed" if packed else "fields")
    return att, DefenderVecEnv(att, max_timesteps=def_T, observation_format="packed" if packed else "dense")


def main():
    for E in SIZES:
        att_t, dfd_t = pair(E, True, ATT_T, DEF_T)
        att_c, dfd_c = pair(E, True, ATT_T, DEF_T)
        att_f, dfd_f = pair(E, False, 100000, 100000)
        att_p, dfd_p = pair(E, True, ATT_T, DEF_T, packed=True)
        train, comp, floor = TwoAgentTrainVecEnv(att_t, dfd_t), ComposedTrainingTurn(att_c, dfd_c), TwoAgentVecEnv(att_f, dfd_f)
        train_p = TwoAgentTrainVecEnv(att_p, dfd_p)
        # rollout-buffer rows for the packed observations of either pair
        packed_bufs = {id(tr): (tr.att.rollout_buffer(ROLLOUT_STEPS, pack_observations=True), tr.dfd.rollout_buffer(ROLLOUT_STEPS, pack_observations=True))
                       for tr in (train, train_p)}

        def turn_and_rows(tr):
            rows_a, rows_d = (b.observations["packed"] for b in packed_bufs[id(tr)])

            def f(i):
                tr.step(a_acts[i & 7], d_acts[i & 7])
                tr.att.observation_packed(out=rows_a[i % ROLLOUT_STEPS])
                tr.dfd.observation_packed(out=rows_d[i % ROLLOUT_STEPS])
            return f
        dev = att_t.engine.device
        g = torch.Generator(device=dev).manual_seed(0)
        a_acts = [torch.randint(0, att_t.discrete_n, (E,), generator=g, device=dev) for _ in range(8)]
        nv = torch.as_tensor(dfd_t.nvec, device=dev)
        d_acts = [(torch.rand((E, 12), generator=g, device=dev) * nv).long() for _ in range(8)]

        def fresh_floor():
            att_f.reset()
            dfd_f.reset()
        legs = (("training_turn", train.reset, lambda i: train.step(a_acts[i & 7], d_acts[i & 7])),
                ("composition", comp.reset, lambda i: comp.step(a_acts[i & 7], d_acts[i & 7], with_mask=False)),
                ("floor_no_reset", fresh_floor, lambda i: floor.step(a_acts[i & 7], d_acts[i & 7])),
                ("training_turn_packed", train_p.reset, lambda i: train_p.step(a_acts[i & 7], d_acts[i & 7])),
                ("training_turn+pack_launches", train.reset, turn_and_rows(train)),
                ("training_turn_packed+row_copies", train_p.reset, turn_and_rows(train_p)))
        for _, fresh, f in legs:                                  # warm-up: output rings, bound calls
            fresh()
            for i in range(16):
                f(i)
        results = {name: [] for name, _, _ in legs}
        for _ in range(REPEATS):
            ms = {name: 0.0 for name, _, _ in legs}
            for _ in range(BLOCKS):
                for name, fresh, f in legs:
                    fresh()
                    torch.cuda.synchronize(dev)
                    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    for i in range(TURNS):
                        f(i)
                    end.record()
                    end.synchronize()
                    ms[name] += start.elapsed_time(end)
            for name in ms:
                results[name].append(ms[name] * 1e3 / (BLOCKS * TURNS))
        for name, _, _ in legs:
            print(json.dumps(dict(measure="turn, device events", envs=E, leg=name, turns_per_repeat=BLOCKS * TURNS, **spread(results[name]))), flush=True)

        # ---------------- (b) one collect_rollouts iteration, host clock ----------------
        step = {"n": 0}

        def pa(env):
            step["n"] += 1
            out = env.sample_masked_uniform(seed=0, step=step["n"])
            return out.actions, out.entropy, out.log_prob

        def pd(env):
            out = env.sample_uniform(seed=1, step=step["n"])
            return out.actions, out.entropy, out.log_prob
        runs = (("collect_rollouts", train, (att_t.rollout_buffer(ROLLOUT_STEPS), dfd_t.rollout_buffer(ROLLOUT_STEPS))),
                ("collect_rollouts, packed buffers, dense pair", train, packed_bufs[id(train)]),
                ("collect_rollouts, packed buffers, packed pair", train_p, packed_bufs[id(train_p)]))
        for _, tr, (buf_a, buf_d) in runs:
            tr.reset()
            collect_rollouts(tr, pa, pd, buf_a, buf_d, ROLLOUT_STEPS)
        per_turn = {leg: [] for leg, _, _ in runs}
        for _ in range(REPEATS):
            for leg, tr, (buf_a, buf_d) in runs:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(ROLLOUTS):
                    collect_rollouts(tr, pa, pd, buf_a, buf_d, ROLLOUT_STEPS)
                torch.cuda.synchronize(dev)
                per_turn[leg].append((time.perf_counter() - t0) * 1e6 / (ROLLOUTS * ROLLOUT_STEPS))
        for leg, _, _ in runs:
            print(json.dumps(dict(measure="collect_rollouts iteration, host clock", envs=E, leg=leg,
                                  iterations_per_repeat=ROLLOUTS * ROLLOUT_STEPS, **spread(per_turn[leg]))), flush=True)
        for a in (att_t, att_c, att_f, att_p):
            a.close()


if __name__ == "__main__":
    main()
