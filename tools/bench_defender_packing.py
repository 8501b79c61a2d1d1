#!/usr/bin/env python3
"""Packed defender observations (mcbs_defender_wrapper_step_packed, mcbs_encode_defender_features) against the int8 path they stand
next to, on the MI355X: one JSON line.  Two workloads: 16 384 ToyCtf envs at 12/10 and 65 536 Chain-10 envs at 12/12, each as a
dense-mode and a packed-mode AttackerVecEnv(learned_defender=True) + DefenderVecEnv pair advanced by the same 40 turns, then T = 8
more stored both ways.  All legs run in ONE process and alternate in groups, device events around groups of calls after a warm-up,
every leg timed over at least 100 calls and 0.2 s; reported: median and minimum over the groups.
  (1) step       `dfd.step(actions)`, dense against packed (the same actions; the turn kernel writes the observation either way)
  (2) store      one step into a rollout buffer: the dense step + four `copy_`s into the int8 storage against the packed step +
                 `observation_packed(out=row)`; and the two storing halves alone
  (3) features   live rows, fp32 and bf16, into one preallocated output: the four converting `copy_`s features() was before
                 (kept here as the baseline) against the kernel, from the int8 fields and from the packed rows
  (4) minibatch  a 16 384-row minibatch drawn from the T stored steps, fp32 and bf16: four `index_select`s + four converting `copy_`s
                 against `encode_features_packed(storage, index=...)`; outputs checked bit-equal
  (5) bytes      observation bytes of a [128, E] rollout buffer, both ways (computed from the shapes, not allocated)"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from marlon_amd.wrappers import AttackerVecEnv, DefenderVecEnv  # noqa: E402
from tools import workloads as Wl  # noqa: E402
from tools.bench_obs_packing import summary, timed  # noqa: E402

T, BATCH, ADVANCE, ROLLOUT_STEPS = 8, 16384, 40, 128
KEYS = DefenderVecEnv.FEATURE_KEYS


def four_copies(fields, out):
    """DefenderVecEnv.features() as it was before the encoder kernel: four converting copy_s, sorted key order"""
    c = 0
    for k in KEYS:
        x = fields[k].reshape(out.shape[0], -1)
        out[:, c:c + x.shape[1]].copy_(x)
        c += x.shape[1]
    return out


def pair(environment, E, kw, fmt):
    att = AttackerVecEnv(environment, E, materialize_masks=False, learned_defender=True, seed=7, max_timesteps=1 << 30, **kw)
    return att, DefenderVecEnv(att, max_timesteps=1 << 30, observation_format=fmt)


def main():
    rows = []
    for name in sys.argv[1:] or ["config3", "headline"]:
        environment, E, kw = Wl.wrapper_workload(name)
        (att_d, dfd_d), (att_p, dfd_p) = pair(environment, E, kw, "dense"), pair(environment, E, kw, "packed")
        dev = att_d.engine.device
        rng = np.random.Generator(np.random.PCG64(1))
        acts = [torch.as_tensor((rng.random((E, 12)) * dfd_d.nvec).astype(np.int64), device=dev) for _ in range(4)]
        buf_d, buf_p = dfd_d.rollout_buffer(T), dfd_p.rollout_buffer(T)

        def turn(t):
            a = att_d.sample_uniform(seed=7, step=t).actions
            att_d.step(a)
            att_p.step(a)
            dfd_d.step(acts[t % 4])
            dfd_p.step(acts[t % 4])

        for t in range(ADVANCE):
            turn(t)
        for t in range(T):
            for k, v in dfd_d.observation.items():
                buf_d.observations[k][t].copy_(v)
            dfd_p.observation_packed(out=buf_p.observations["packed"][t])
            turn(ADVANCE + t)
        P = dfd_p.observation_packing()
        W, F = P.words, P.width
        assert torch.equal(dfd_d.observation_packed(), dfd_p.packed_observation), "the two pairs left lock-step"
        row = dict(workload=name, envs=E, columns=F, packed_words=W, step_launches=att_p.engine.defender_wrapper_step_packed_launches(),
                   rollout_obs_bytes_int8=ROLLOUT_STEPS * E * F, rollout_obs_bytes_packed=ROLLOUT_STEPS * E * W * 4)

        # (1) the step, (2) the step and its store
        def copies():
            for k, dst in buf_d.observations.items():
                dst[0].copy_(dfd_d.observation[k])

        def store_packed():
            dfd_p.observation_packed(out=buf_p.observations["packed"][0])

        def dense_step_store():
            dfd_d.step(acts[0])
            copies()

        def packed_step_store():
            dfd_p.step(acts[0])
            store_packed()

        legs = {"step_dense": lambda: dfd_d.step(acts[0]), "step_packed": lambda: dfd_p.step(acts[0]), "store_copies": copies,
                "store_packed": store_packed, "step_store_dense": dense_step_store, "step_store_packed": packed_step_store}
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        row.update(summary(timed(legs)))
        for a, b in (("step_dense", "step_packed"), ("store_copies", "store_packed"), ("step_store_dense", "step_store_packed")):
            row[f"{a}_over_{b}"] = round(row[f"{a}_us"] / row[f"{b}_us"], 2)
        assert torch.equal(dfd_d.observation_packed(), dfd_p.packed_observation)

        # (3) live features
        for label, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            per = 16 // torch.empty((), dtype=dtype).element_size()
            outs = [torch.empty((E, (F + per - 1) // per * per), dtype=dtype, device=dev) for _ in range(3)]
            legs = {f"features_{label}_four_copies": lambda: four_copies(dfd_d.observation, outs[0]),
                    f"features_{label}_kernel_dense": lambda: dfd_d.features(out=outs[1]),
                    f"features_{label}_kernel_packed": lambda: dfd_p.features(out=outs[2])}
            for fn in legs.values():
                fn()
            row[f"features_{label}_bit_equal"] = bool(torch.equal(outs[0][:, :F], outs[1][:, :F]) and torch.equal(outs[0][:, :F], outs[2][:, :F]))
            torch.cuda.synchronize()
            row.update(summary(timed(legs)))
            for k in ("dense", "packed"):
                row[f"features_{label}_four_copies_over_kernel_{k}"] = round(row[f"features_{label}_four_copies_us"] / row[f"features_{label}_kernel_{k}_us"], 2)
            del outs

        # (4) a shuffled minibatch of the T stored steps
        idx = torch.randperm(T * E, device=dev, generator=torch.Generator(device=dev).manual_seed(1))[:BATCH].contiguous()
        storage = buf_p.observations["packed"].view(T * E, -1)
        flat = {k: v.view(T * E, -1) for k, v in buf_d.observations.items()}
        for label, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            per = 16 // torch.empty((), dtype=dtype).element_size()
            out_a = torch.empty((BATCH, (F + per - 1) // per * per), dtype=dtype, device=dev)
            out_b = torch.empty_like(out_a)
            legs = {f"batch_{label}_gather_copies": lambda: four_copies({k: v.index_select(0, idx) for k, v in flat.items()}, out_a),
                    f"batch_{label}_packed": lambda: dfd_p.encode_features_packed(storage, index=idx, out=out_b)}
            for fn in legs.values():
                fn()
            row[f"batch_{label}_bit_equal"] = bool(torch.equal(out_a[:, :F], out_b[:, :F]))
            torch.cuda.synchronize()
            row.update(summary(timed(legs)))
            row[f"batch_{label}_gather_over_packed"] = round(row[f"batch_{label}_gather_copies_us"] / row[f"batch_{label}_packed_us"], 2)
            del out_a, out_b
        rows.append(row)
        att_d.close()
        att_p.close()
        del att_d, att_p, dfd_d, dfd_p, buf_d, buf_p, storage, flat
    print(json.dumps(dict(tool="bench_defender_packing", stored_steps=T, minibatch=BATCH, workloads=rows)), flush=True)
    assert all(r[f"{k}_{d}_bit_equal"] for r in rows for k in ("features", "batch") for d in ("fp32", "bf16")), "the encoder's rows differ from the four copies'"


if __name__ == "__main__":
    main()
