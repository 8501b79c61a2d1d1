#!/usr/bin/env python3
"""The one-launch attacker wrapper step that writes the packed observation row itself (AttackerVecEnv(observation_format="packed"),
mcbs_attacker_wrapper_step_packed) against the int32 one-launch step and what a packing rollout paid on top of it, in ONE process:

  (A) int32_step          `AttackerVecEnv.step` of the int32 mode, one launch (mcbs_wrapper_fused.hip wrapper_fused_kernel)
  (B) int32_step_pack     A + `observation_packed(out=row)` (mcbs_pack_observation): the way to the packed rows before — THE BAR for C
  (C) packed_step         `AttackerVecEnv.step` of the packed mode, one launch (wrapper_fused_packed_kernel)
  (D) int32_step_features / packed_step_features: A + `features(bf16, out=)` against C + `features(bf16, out=)`

Workloads: 65 536 Chain-10 envs at 12/12 and 16 384 ToyCtf envs at 12/10, Discrete, materialize_masks=False.  The actions are masked
uniformly random ones, recorded once from the int32 wrapper for BLOCK steps after a reset; every timed block replays them from a reset
(outside the timed span), so every leg runs the same trajectory and the observation rows are the same bits (checked).  Device events
around blocks of steps, the legs alternating block by block after a warm-up, BLOCKS x BLOCK >= 2 000 steps per leg and repeat, three
repeats: us per step of each repeat, their median and spread.  One JSON line per workload and leg, then one with the comparisons.
    python tools/bench_packed_step.py [headline|config3 ...]"""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
from marlon_amd.wrappers import AttackerVecEnv  # noqa: E402
from tools import workloads as Wl  # noqa: E402

BLOCKS, BLOCK, REPEATS, WARMUP = 8, 250, 3, 16


def spread(xs):
    return dict(us=[round(x, 2) for x in xs], median_us=round(statistics.median(xs), 2), min_us=round(min(xs), 2), max_us=round(max(xs), 2))


def main():
    for name in sys.argv[1:] or ["headline", "config3"]:
        environment, E, kw = Wl.wrapper_workload(name)
        kw = dict(kw, discrete=True, materialize_masks=False, seed=7)
        fields = AttackerVecEnv(environment, E, **kw)
        packed = AttackerVecEnv(environment, E, observation_format="packed", **kw)
        dev = fields.engine.device
        W = packed.observation_packing().words
        # the trajectory: BLOCK masked uniformly random actions per env from a reset, recorded from the int32 wrapper
        actions = torch.empty((BLOCK, E), dtype=torch.int64, device=dev)
        fields.reset()
        for t in range(BLOCK):
            actions[t] = fields.sample_masked_uniform(seed=7, step=t).actions
            fields.step(actions[t])
        row = torch.empty((E, W), dtype=torch.int32, device=dev)
        layout = fields.feature_layout()
        feat = torch.empty((E, layout.padded_width(2)), dtype=torch.bfloat16, device=dev)[:, :layout.width]
        # the same bits at the end of the trajectory, by all three routes
        packed.reset()
        for t in range(BLOCK):
            packed.step(actions[t])
        same_rows = bool(torch.equal(fields.observation_packed(out=row), packed.packed_observation))
        same_features = bool(torch.equal(fields.features(dtype=torch.bfloat16), packed.features(dtype=torch.bfloat16)))

        def leg_a(t):
            fields.step(actions[t])

        def leg_b(t):
            fields.step(actions[t])
            fields.observation_packed(out=row)

        def leg_c(t):
            packed.step(actions[t])

        def leg_da(t):
            fields.step(actions[t])
            fields.features(out=feat)

        def leg_dc(t):
            packed.step(actions[t])
            packed.features(out=feat)
        legs = (("int32_step", fields, leg_a), ("int32_step_pack", fields, leg_b), ("packed_step", packed, leg_c),
                ("int32_step_features", fields, leg_da), ("packed_step_features", packed, leg_dc))
        for _, env, f in legs:
            env.reset()
            for t in range(WARMUP):
                f(t)
        torch.cuda.synchronize(dev)
        results = {leg: [] for leg, _, _ in legs}
        for _ in range(REPEATS):
            ms = {leg: 0.0 for leg, _, _ in legs}
            for _ in range(BLOCKS):
                for leg, env, f in legs:
                    env.reset()
                    torch.cuda.synchronize(dev)
                    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    for t in range(BLOCK):
                        f(t)
                    end.record()
                    end.synchronize()
                    ms[leg] += start.elapsed_time(end)
            for leg in ms:
                results[leg].append(ms[leg] * 1e3 / (BLOCKS * BLOCK))
        out = {leg: spread(results[leg]) for leg, _, _ in legs}
        for leg, _, _ in legs:
            print(json.dumps(dict(workload=name, envs=E, leg=leg, steps_per_repeat=BLOCKS * BLOCK, **out[leg])), flush=True)
        a, b, c = out["int32_step"], out["int32_step_pack"], out["packed_step"]
        noise = max(b["max_us"] - b["min_us"], c["max_us"] - c["min_us"])
        print(json.dumps(dict(workload=name, envs=E, packed_words=W, values_per_row=packed.observation_packing().values_per_row,
                              rows_bit_equal=same_rows, features_bit_equal=same_features,
                              packed_step_over_int32_step_pack=round(c["median_us"] / b["median_us"], 3),
                              packed_step_over_int32_step=round(c["median_us"] / a["median_us"], 3),
                              packed_features_over_int32_features=round(out["packed_step_features"]["median_us"] / out["int32_step_features"]["median_us"], 3),
                              run_to_run_spread_us=round(noise, 2),
                              verdict="FASTER than step + pack" if b["median_us"] - c["median_us"] > noise else "SLOWER or within the spread of step + pack")),
              flush=True)
        fields.close()
        packed.close()
        del fields, packed, actions, row, feat


if __name__ == "__main__":
    main()
