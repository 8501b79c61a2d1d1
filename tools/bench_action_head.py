#!/usr/bin/env python3
"""The masked action head from the latent (mcbs_masked_linear_categorical) against the path it replaces, on the headline batch (65 536
Chain-10 envs) and config 3 (16 384 ToyCtf envs) 40 steps into an episode, H = 64 (MultiInputPolicy's latent_dim_pi), fp32 and bf16
(randn latent, randn / 8 weights, randn bias), us per call by HIP events, the legs alternating inside one timed loop:
  (a) linear_then_sample   torch.nn.functional.linear producing the [n_envs, A] logits, then masked_categorical(mode="sample") on them
  (b) linear               the same linear alone
  (c) fused_live_sample    masked_linear_categorical(mode="sample") on the live rows: no logits tensor
  (d) fused_packed_evaluate  masked_linear_categorical(bits=..., mode="evaluate") on a gathered minibatch of 16 384 stored rows
and, for scale, (e) mb_linear_then_evaluate: the linear on the minibatch's latent and masked_categorical(bits=..., mode="evaluate") on
its logits.  Every leg reports the mean and the [min, max] of its REPS timings.

The update legs (a second JSON line per dtype, "leg": "update"): forward + backward of PPO's loss on the same minibatch of 16 384 stored
rows, gradients into latent, weight and bias,
  (f) fused_update       masked_linear_evaluate (mcbs_masked_linear_categorical in EVALUATE mode, mcbs_masked_linear_categorical_grad)
  (g) composite_update   F.linear, masked_evaluate(differentiable) on the [n, A] logits, torch's two GEMMs in the backward pass
alternating in one timed loop, with the peak of torch.cuda.max_memory_allocated above what each path starts from, the workspace bytes,
and the largest difference between the two paths' gradients.  BENCH_ACTION_HEAD_LEGS=forward or =update runs one kind only."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from tools import workloads as W  # noqa: E402

REPS = int(os.environ.get("BENCH_ACTION_HEAD_REPS", "10"))
H = 64
KINDS = os.environ.get("BENCH_ACTION_HEAD_LEGS", "forward,update").split(",")


def timed(legs):
    """us per call of every leg, REPS times, alternating: drift of the shared machine hits all alike."""
    for fn in legs.values():                             # warm up every shape
        fn()
    torch.cuda.synchronize()
    each = {k: [] for k in legs}
    for _ in range(REPS):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            each[k].append(e0.elapsed_time(e1))
    return each


def report(row, each):
    for k, v in each.items():
        row[f"{k}_us"] = round(sum(v) / len(v) * 1e3, 1)
        row[f"{k}_us_min_max"] = [round(min(v) * 1e3, 1), round(max(v) * 1e3, 1)]
    print(json.dumps(row), flush=True)


def update_legs(eng, name, dtype, mb_latent, weight, bias, mb_bits, mb_actions, old_lp, g):
    n, A = mb_latent.shape[0], weight.shape[0]
    adv = torch.randn(n, generator=g, device=mb_latent.device)
    lat, w, b = (x.clone().requires_grad_(True) for x in (mb_latent, weight, bias))

    def loss(r):
        return -(adv * torch.exp(r.log_prob - old_lp)).mean() - 0.01 * r.entropy.mean()

    def fused():
        lat.grad = w.grad = b.grad = None
        loss(eng.masked_linear_evaluate(lat, w, b, mb_bits, mb_actions)).backward()

    def composite():
        lat.grad = w.grad = b.grad = None
        loss(eng.masked_evaluate(F.linear(lat, w, b), mb_bits, mb_actions)).backward()

    peak, grads = {}, {}
    for k, fn in (("fused_update", fused), ("composite_update", composite)):
        lat.grad = w.grad = b.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - start
        grads[k] = [x.grad.float().clone() for x in (lat, w, b)]
    diff = [float((x - y).abs().max()) for x, y in zip(grads["fused_update"], grads["composite_update"])]
    del grads
    row = dict(workload=name, leg="update", rows=n, actions=A, H=H, dtype=str(dtype).split(".")[-1], reps=REPS,
               workspace_bytes=eng.masked_linear_categorical_grad_workspace(n, H), logits_bytes=n * A * mb_latent.element_size(),
               fused_update_peak_bytes=peak["fused_update"], composite_update_peak_bytes=peak["composite_update"],
               grad_max_abs_diff_latent_weight_bias=diff)
    report(row, timed({"fused_update": fused, "composite_update": composite}))


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
        if "forward" in KINDS:
            legs = {
                "linear_then_sample": lambda: eng.masked_categorical(F.linear(latent, weight, bias), mode="sample", seed=1, step=1),
                "linear": lambda: F.linear(latent, weight, bias),
                "fused_live_sample": lambda: eng.masked_linear_categorical(latent, weight, bias, mode="sample", seed=1, step=1),
                "fused_packed_evaluate": lambda: eng.masked_linear_categorical(mb_latent, weight, bias, bits=mb_bits, mode="evaluate", actions=mb_actions),
                "mb_linear_then_evaluate": lambda: eng.masked_categorical(F.linear(mb_latent, weight, bias), bits=mb_bits, mode="evaluate", actions=mb_actions),
            }
            K = first.n_allowed.double()
            row = dict(workload=name, envs=E, actions=A, H=H, dtype=str(dtype).split(".")[-1], reps=REPS, minibatch_rows=mb,
                       allowed_mean=round(float(K.mean()), 1), allowed_max=int(K.max()), logits_bytes=E * A * latent.element_size(),
                       weight_bytes=A * H * latent.element_size(), log_prob_max_abs_diff_vs_linear=lp_diff)
            report(row, timed(legs))
        if "update" in KINDS:
            update_legs(eng, name, dtype, mb_latent, weight, bias, mb_bits, mb_actions, first.log_prob[perm].contiguous(), g)
        del latent, weight, bias, mb_latent, first
    eng.close()
