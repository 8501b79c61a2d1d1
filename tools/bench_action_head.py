#!/usr/bin/env python3
"""The masked action head from the latent (mcbs_masked_linear_categorical) against the path it replaces, on the headline batch (65 536
Chain-10 envs) and config 3 (16 384 ToyCtf envs) 40 steps into an episode, H = 64 (MultiInputPolicy's latent_dim_pi), fp32 and bf16
(randn latent, randn / 8 weights, randn bias), us per call by HIP events, the legs alternating inside one timed loop:
  (a) linear_then_sample   torch.nn.functional.linear producing the [n_envs, A] logits, then masked_categorical(mode="sample") on them
  (b) linear               the same linear alone
  (c) fused_live_sample    masked_linear_categorical(mode="sample") on the live rows: no logits tensor
  (d) fused_packed_evaluate  masked_linear_categorical(bits=..., mode="evaluate") on a gathered minibatch of 16 384 stored rows
and, for scale, (e) mb_linear_then_evaluate: the linear on the minibatch's latent and masked_categorical(bits=..., mode="evaluate") on
its logits.  Every leg reports the mean and the [min, max] of its REPS timings."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from tools import workloads as W  # noqa: E402

REPS = int(os.environ.get("BENCH_ACTION_HEAD_REPS", "10"))
H = 64
names = sys.argv[1:] or ["headline", "config3"]
for name in names:
    ring = W.record_ring(name, 40)
    eng, topo, spec, desc = W.make_engine(name)
    for t in range(40):
        eng.step(ring[t], with_info=False)
    eng.observe(eng.alloc_obs(W.OBS_FIELDS[:5]))
    E, A, dev = eng.E, eng.discrete_action_count(), eng.device
    bits = eng.pack_action_mask()
    g = torch.Generator(device=dev).manual_seed(0)
    mb = min(16384, E)
    perm = torch.randperm(E, generator=g, device=dev)[:mb]
    mb_bits = bits[perm].contiguous()
    for dtype in (torch.float32, torch.bfloat16):
        latent = torch.randn((E, H), generator=g, device=dev).to(dtype)
        weight = (torch.randn((A, H), generator=g, device=dev) / 8.0).to(dtype)
        bias = torch.randn(A, generator=g, device=dev).to(dtype)
        mb_latent = latent[perm].contiguous()
        first = eng.masked_linear_categorical(latent, weight, bias, mode="sample", seed=1, step=0)
        mb_actions = first.actions[perm].contiguous()
        # the two paths give the same distribution: the same K, log_prob to rounding
        check = eng.masked_categorical(F.linear(latent, weight, bias), mode="evaluate", actions=first.actions)
        assert torch.equal(check.n_allowed, first.n_allowed)
        lp_diff = float((check.log_prob - first.log_prob).abs().max())
        del check
        legs = {
            "linear_then_sample": lambda: eng.masked_categorical(F.linear(latent, weight, bias), mode="sample", seed=1, step=1),
            "linear": lambda: F.linear(latent, weight, bias),
            "fused_live_sample": lambda: eng.masked_linear_categorical(latent, weight, bias, mode="sample", seed=1, step=1),
            "fused_packed_evaluate": lambda: eng.masked_linear_categorical(mb_latent, weight, bias, bits=mb_bits, mode="evaluate", actions=mb_actions),
            "mb_linear_then_evaluate": lambda: eng.masked_categorical(F.linear(mb_latent, weight, bias), bits=mb_bits, mode="evaluate", actions=mb_actions),
        }
        for fn in legs.values():                         # warm up every shape
            fn()
        torch.cuda.synchronize()
        each = {k: [] for k in legs}
        for _ in range(REPS):                            # alternating legs: drift of the shared machine hits all alike
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                each[k].append(e0.elapsed_time(e1))
        K = first.n_allowed.double()
        row = dict(workload=name, envs=E, actions=A, H=H, dtype=str(dtype).split(".")[-1], reps=REPS, minibatch_rows=mb,
                   allowed_mean=round(float(K.mean()), 1), allowed_max=int(K.max()), logits_bytes=E * A * latent.element_size(),
                   weight_bytes=A * H * latent.element_size(), log_prob_max_abs_diff_vs_linear=lp_diff)
        for k, v in each.items():
            row[f"{k}_us"] = round(sum(v) / len(v) * 1e3, 1)
            row[f"{k}_us_min_max"] = [round(min(v) * 1e3, 1), round(max(v) * 1e3, 1)]
        print(json.dumps(row), flush=True)
        del latent, weight, bias, mb_latent, first
    eng.close()
