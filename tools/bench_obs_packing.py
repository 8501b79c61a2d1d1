#!/usr/bin/env python3
"""Packed observations (mcbs_pack_observation, mcbs_encode_features_packed) against the int32 path they replace, on the MI355X: one
JSON line.  Two workloads: 65 536 Chain-10 envs at 12/12 and 16 384 ToyCtf envs at 12/10 (AttackerVecEnv, discrete, masks not
materialised), advanced by 40 masked uniformly random steps, then T = 8 more stored both ways.  Legs alternate inside one process, device
events around groups of launches after a warm-up, every leg timed over at least 100 calls and 0.2 s; reported: median and minimum over
the groups.
  (a) store     `observation_packed(out=row)` (one launch) against the five `copy_`s of `buf.add(obs=observation_fields, ...)`
  (b) minibatch a 16 384-row minibatch drawn from the T stored steps, fp32 and bf16, into one preallocated output:
                five `index_select`s + `encode_features` against `encode_features_packed(storage, index=...)`; outputs checked bit-equal
  (c) bytes     observation bytes of a [128, E] rollout buffer, both ways (computed from the shapes, not allocated)"""
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
        packed_buf = env.rollout_buffer(T, pack_observations=True)
        plain_buf = env.rollout_buffer(T)
        for t in range(T):
            env.observation_packed(out=packed_buf.observations["packed"][t])
            for k, v in env.observation_fields.items():
                plain_buf.observations[k][t].copy_(v)
            env.step(env.sample_masked_uniform(seed=7, step=ADVANCE + t).actions)
        W = env.observation_packing().words
        V = env.observation_packing().values_per_row
        row = dict(workload=name, envs=E, values_per_row=V, packed_words=W,
                   rollout_obs_bytes_int32=ROLLOUT_STEPS * E * V * 4, rollout_obs_bytes_packed=ROLLOUT_STEPS * E * W * 4)
        # (a) one step's observation into row 0 of each buffer
        fields = env.observation_fields

        def copies():
            for k, dst in plain_buf.observations.items():
                dst[0].copy_(fields[k].reshape(dst[0].shape))

        legs = {"store_packed": lambda: env.observation_packed(out=packed_buf.observations["packed"][0]), "store_copies": copies}
        for fn in legs.values():
            fn()
        assert torch.equal(env.unpack_observation(packed_buf.observations["packed"][0])["scalars"], plain_buf.observations["scalars"][0])
        torch.cuda.synchronize()
        row.update(summary(timed(legs)))
        row["store_copies_over_packed"] = round(row["store_copies_us"] / row["store_packed_us"], 2)
        # (b) a shuffled minibatch of the T stored steps
        idx = torch.randperm(T * E, device=dev, generator=torch.Generator(device=dev).manual_seed(1))[:BATCH].contiguous()
        storage = packed_buf.observations["packed"].view(T * E, -1)
        flat = {k: v.view((T * E,) + tuple(v.shape[2:])) for k, v in plain_buf.observations.items()}
        layout = env.feature_layout()
        for label, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            item = torch.empty((), dtype=dtype).element_size()
            out_a = torch.empty((BATCH, layout.padded_width(item)), dtype=dtype, device=dev)
            out_b = torch.empty_like(out_a)
            legs = {f"batch_{label}_gather_encode": lambda: env.encode_features({k: v.index_select(0, idx) for k, v in flat.items()}, out=out_a[:, :layout.width]),
                    f"batch_{label}_packed": lambda: env.encode_features_packed(storage, index=idx, out=out_b[:, :layout.width])}
            for fn in legs.values():
                fn()
            row[f"batch_{label}_bit_equal"] = bool(torch.equal(out_a[:, :layout.width], out_b[:, :layout.width]))
            torch.cuda.synchronize()
            row.update(summary(timed(legs)))
            row[f"batch_{label}_gather_over_packed"] = round(row[f"batch_{label}_gather_encode_us"] / row[f"batch_{label}_packed_us"], 2)
            del out_a, out_b
        rows.append(row)
        env.close()
        del env, packed_buf, plain_buf, storage, flat
    print(json.dumps(dict(tool="bench_obs_packing", stored_steps=T, minibatch=BATCH, min_calls=MIN_CALLS, min_seconds=MIN_SECONDS, workloads=rows)),
          flush=True)
    assert all(r["batch_fp32_bit_equal"] and r["batch_bf16_bit_equal"] for r in rows), "the packed encoder's rows differ from the int32 path's"


if __name__ == "__main__":
    main()
