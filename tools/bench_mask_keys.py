#!/usr/bin/env python3
"""Action-mask keys (mcbs_store_mask_keys, mcbs_expand_mask_keys) against the stored bits they replace, on the MI355X: one JSON line.
Two workloads: 65 536 Chain-10 envs at 12/12 and 16 384 ToyCtf envs at 12/10 (AttackerVecEnv, discrete, masks not materialised),
advanced by 40 masked uniformly random steps, then T = 8 more stored both ways.  Legs alternate inside one process, device events
around groups of launches after a warm-up, every leg timed over at least 100 calls and 0.2 s; reported: median and minimum over the
groups.
  (a) store     `action_mask_keys(out=row)` against `action_masks_packed(out=row)`, one launch each
  (b) minibatch a 16 384-row minibatch drawn from the T stored steps into one preallocated output: `bits.index_select(0, index)`
                (a copy) against `expand_mask_keys(keys, index)` (a recomputation); outputs checked bit-equal
  (c) bytes     mask bytes per row and of a [128, E] rollout buffer, both ways (computed from the shapes, not allocated)"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
from marlon_amd.wrappers import AttackerVecEnv  # noqa: E402
from tools import workloads as Wl  # noqa: E402

T, BATCH, ADVANCE, ROLLOUT_STEPS = 8, 16384, 40, 128
MIN_CALLS, MIN_SECONDS, GROUP, MAX_CALLS = 100, 0.2, 20, 20000


def timed(legs):
    """Alternate the legs in groups until each has MIN_CALLS calls and MIN_SECONDS of device time -> {leg: [us per call per group]}."""
    per = {k: [] for k in legs}
    total = {k: 0.0 for k in legs}
    count = {k: 0 for k in legs}
    while True:
        todo = [k for k in legs if count[k] < MIN_CALLS or (total[k] < MIN_SECONDS and count[k] < MAX_CALLS)]
        if not todo:
            return per
        for k in todo:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(GROUP):
                legs[k]()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            per[k].append(ms * 1e3 / GROUP)
            total[k] += ms * 1e-3
            count[k] += GROUP


def summary(per):
    out = {}
    for k, xs in per.items():
        xs = sorted(xs)
        out[f"{k}_us"] = round(xs[len(xs) // 2], 2)
        out[f"{k}_us_min"] = round(xs[0], 2)
        out[f"{k}_calls"] = len(xs) * GROUP
    return out


def main():
    rows = []
    for name in sys.argv[1:] or ["headline", "config3"]:
        environment, E, kw = Wl.wrapper_workload(name)
        env = AttackerVecEnv(environment, E, discrete=True, materialize_masks=False, seed=7, **kw)
        dev = env.engine.device
        for t in range(ADVANCE):
            env.step(env.sample_masked_uniform(seed=7, step=t).actions)
        W, row_words = env.engine.packed_mask_words()
        Wk = env.engine.mask_key_words()
        keys = torch.zeros((T, E, Wk), dtype=torch.int32, device=dev)
        bits = torch.zeros((T, E, row_words), dtype=torch.int32, device=dev)
        for t in range(T):
            env.action_mask_keys(out=keys[t])
            env.action_masks_packed(out=bits[t])
            env.step(env.sample_masked_uniform(seed=7, step=ADVANCE + t).actions)
        row = dict(workload=name, envs=E, actions=env.discrete_n, mask_words=W, mask_row_words=row_words, key_words=Wk,
                   row_bytes_bits=row_words * 4, row_bytes_keys=Wk * 4,
                   rollout_mask_bytes_bits=ROLLOUT_STEPS * E * row_words * 4, rollout_mask_bytes_keys=ROLLOUT_STEPS * E * Wk * 4)
        # (a) the live step's mask into row 0 of each storage
        legs = {"store_keys": lambda: env.action_mask_keys(out=keys[0]), "store_bits": lambda: env.action_masks_packed(out=bits[0])}
        for fn in legs.values():
            fn()
        row["store_expand_bit_equal"] = bool(torch.equal(env.expand_mask_keys(keys[0]), bits[0]))
        torch.cuda.synchronize()
        row.update(summary(timed(legs)))
        row["store_bits_over_keys"] = round(row["store_bits_us"] / row["store_keys_us"], 2)
        # (b) a shuffled minibatch of the T stored steps (row 0 of both storages now holds the live step: still a matching pair)
        idx = torch.randperm(T * E, device=dev, generator=torch.Generator(device=dev).manual_seed(1))[:BATCH].contiguous()
        flat_keys, flat_bits = keys.view(T * E, Wk), bits.view(T * E, row_words)
        out_a = torch.zeros((BATCH, row_words), dtype=torch.int32, device=dev)
        out_b = torch.zeros_like(out_a)
        legs = {"batch_gather_bits": lambda: torch.index_select(flat_bits, 0, idx, out=out_a),
                "batch_expand_keys": lambda: env.expand_mask_keys(flat_keys, idx, out=out_b)}
        for fn in legs.values():
            fn()
        row["batch_bit_equal"] = bool(torch.equal(out_a, out_b))
        row["batch_allowed_per_row"] = round(float(env.unpack_action_mask(out_b).sum()) / BATCH, 2)
        torch.cuda.synchronize()
        row.update(summary(timed(legs)))
        row["batch_expand_over_gather"] = round(row["batch_expand_keys_us"] / row["batch_gather_bits_us"], 2)
        rows.append(row)
        env.close()
        del env, keys, bits, out_a, out_b
    print(json.dumps(dict(tool="bench_mask_keys", stored_steps=T, minibatch=BATCH, rollout_steps=ROLLOUT_STEPS, min_calls=MIN_CALLS,
                          min_seconds=MIN_SECONDS, workloads=rows)), flush=True)
    assert all(r["store_expand_bit_equal"] and r["batch_bit_equal"] for r in rows), "expanded keys differ from the stored bits"


if __name__ == "__main__":
    main()
