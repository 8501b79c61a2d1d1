#!/usr/bin/env python3
"""The masked categorical head (mcbs_masked_categorical) against what it replaces, on the headline batch (65 536 Chain-10 envs) and config 3
(16 384 ToyCtf envs) 40 steps into an episode, fp32 and bf16 logits (randn * 4), us per call by HIP events, the four legs alternating
inside one timed loop:
  (a) composite   mask_logits + torch.distributions.Categorical(logits=...) with .sample(), .log_prob() and MaskableCategorical's masked
                  entropy, on the same tensors (the bool mask it needs is materialised once, outside the timing)
  (b) mask_logits alone
  (c) live        masked_categorical(mode="sample") on the live rows
  (d) packed      masked_categorical(bits=..., mode="evaluate") on a gathered minibatch of 16 384 stored rows
and the bytes (c) needs per row by its own count: the logits under set bits + the 64-byte digest + 20 bytes of results.
The update's forward + backward on the same minibatch, the loss sum(w1 * log_prob + w2 * entropy), the gradient taken with respect to the
logits (torch.autograd.grad: no accumulation into .grad):
  (e) composite_fwd_bwd   where(mask, logits, -1e8) -> Categorical -> log_prob / masked entropy in torch, forward and backward (the bool mask
                          [n, A] it needs is materialised once, outside the timing)
  (f) evaluate_fwd_bwd    evaluate_masked(differentiable=True)'s path (engine.masked_evaluate) forward and backward: two launches
  (g) apply_packed_grad   apply_packed_mask on a buffer of the gradient's shape: the floor of this store pattern
and masked_categorical_grad alone (grad_only), whose n * A * sizeof(dtype) written bytes over its time is grad_write_GBps.  These legs
report the median and the [min, max] of the REPS timings."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from tools import workloads as W  # noqa: E402

REPS = int(os.environ.get("BENCH_CATEGORICAL_REPS", "10"))
names = sys.argv[1:] or ["headline", "config3"]
for name in names:
    ring = W.record_ring(name, 40)
    eng, topo, spec, desc = W.make_engine(name)
    for t in range(40):
        eng.step(ring[t], with_info=False)
    eng.observe(eng.alloc_obs(W.OBS_FIELDS[:5]))
    E, A, dev = eng.E, eng.discrete_action_count(), eng.device
    bits = eng.pack_action_mask()
    mask = eng.unpack_action_mask(bits)
    g = torch.Generator(device=dev).manual_seed(0)
    mb = min(16384, E)
    perm = torch.randperm(E, generator=g, device=dev)[:mb]
    mb_bits = bits[perm].contiguous()
    mb_mask = mask[perm].contiguous()
    w1, w2 = torch.randn(mb, generator=g, device=dev), torch.randn(mb, generator=g, device=dev)
    zero = torch.zeros((), device=dev)
    for dtype in (torch.float32, torch.bfloat16):
        src = (torch.randn((E, A), generator=g, device=dev) * 4.0).to(dtype)
        work = src.clone()
        mb_logits = src[perm].contiguous()
        first = eng.masked_categorical(src, mode="sample", seed=1, step=0)
        mb_actions = first.actions[perm].contiguous()

        def composite():
            eng.mask_logits(work, fill=-1e8)
            dist = torch.distributions.Categorical(logits=work)
            a = dist.sample()
            lp = dist.log_prob(a)
            ent = -torch.where(mask, dist.logits * dist.probs, zero.to(dist.logits.dtype)).sum(-1)
            return a, lp, ent

        leaf = mb_logits.clone().requires_grad_(True)
        grad_buf = torch.empty_like(mb_logits)
        fill = torch.tensor(-1e8, dtype=dtype, device=dev)

        def composite_fwd_bwd():
            dist = torch.distributions.Categorical(logits=torch.where(mb_mask, leaf, fill))
            lp = dist.log_prob(mb_actions)
            ent = -torch.where(mb_mask, dist.logits * dist.probs, zero.to(dtype)).sum(-1)
            return torch.autograd.grad((lp * w1).sum() + (ent * w2).sum(), leaf)[0]

        def evaluate_fwd_bwd():
            r = eng.masked_evaluate(leaf, mb_bits, mb_actions)
            return torch.autograd.grad((r.log_prob * w1).sum() + (r.entropy * w2).sum(), leaf)[0]

        legs = {
            "composite": composite,
            "mask_logits": lambda: eng.mask_logits(work, fill=-1e8),
            "live_sample": lambda: eng.masked_categorical(src, mode="sample", seed=1, step=1),
            "packed_evaluate": lambda: eng.masked_categorical(mb_logits, bits=mb_bits, mode="evaluate", actions=mb_actions),
            "composite_fwd_bwd": composite_fwd_bwd,
            "evaluate_fwd_bwd": evaluate_fwd_bwd,
            "apply_packed_grad": lambda: eng.apply_packed_mask(mb_bits, grad_buf, fill=0.0),
            "grad_only": lambda: eng.masked_categorical_grad(mb_logits, mb_bits, mb_actions, w1, w2, out=grad_buf),
        }
        spread_legs = ("composite_fwd_bwd", "evaluate_fwd_bwd", "apply_packed_grad", "grad_only")
        for fn in legs.values():                         # warm up every shape
            fn()
        torch.cuda.synchronize()
        ms = {k: 0.0 for k in legs}
        each = {k: [] for k in legs}
        for _ in range(REPS):                            # alternating legs: drift of the shared machine hits all four alike
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[k] += e0.elapsed_time(e1)
                each[k].append(e0.elapsed_time(e1))
        K = first.n_allowed.double()
        row = dict(workload=name, envs=E, actions=A, dtype=str(dtype).split(".")[-1], reps=REPS, minibatch_rows=mb,
                   allowed_mean=round(float(K.mean()), 1), allowed_max=int(K.max()),
                   live_bytes_per_row=round(float(K.mean()) * src.element_size() + 64 + 20, 1),
                   composite_logits_bytes_per_row=A * src.element_size())
        row.update({f"{k}_us": round(v / REPS * 1e3, 1) for k, v in ms.items() if k not in spread_legs})
        for k in spread_legs:
            v = sorted(each[k])
            row[f"{k}_us"] = round(v[len(v) // 2] * 1e3, 1)
            row[f"{k}_us_min_max"] = [round(v[0] * 1e3, 1), round(v[-1] * 1e3, 1)]
        row["grad_bytes_written"] = mb * A * src.element_size()
        row["grad_write_GBps"] = round(row["grad_bytes_written"] / (row["grad_only_us"] * 1e-6) / 1e9, 1)
        row["apply_packed_write_GBps"] = round(row["grad_bytes_written"] / (row["apply_packed_grad_us"] * 1e-6) / 1e9, 1)
        print(json.dumps(row), flush=True)
        del src, work, mb_logits, leaf, grad_buf
    eng.close()
