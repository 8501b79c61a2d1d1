#!/usr/bin/env python3
"""The MultiDiscrete head (mcbs_multicategorical / mcbs_multicategorical_grad) against what it replaces — Stable-Baselines3's
MultiCategoricalDistribution written out in torch — at the shapes the reference's two PPO agents produce:
  chain10_defender   65 536 rows, nvec [5,N,N,6,2,N,6,2,N,3,N,3] at N = 12              (A = 87)
  chain10_attacker   65 536 rows, nvec [3,N,L,N,N,R,N,N,P,C] at N = C = 12, L, R, P = 5, 2, 8   (A = 90)
  toyctf_defender    16 384 rows, the defender's nvec at N = 10                        (A = 77)
fp32 and bf16 logits (randn * 4), us per call by device events around five calls, every leg alternating inside one timed loop, the
median and the [min, max] of the REPS timings:
  (a) composite          split + one torch.distributions.Categorical per dimension: sample, log_prob, entropy, stacked and summed
  (b) kernel_sample      multicategorical(mode="sample"): one launch
  (c) composite_fwd_bwd  the update on a minibatch of 16 384 rows: split -> Categorical -> log_prob(actions).sum + entropy.sum, the loss
                         sum(w1 * log_prob + w2 * entropy), its gradient with respect to the logits (torch.autograd.grad)
      evaluate_fwd_bwd   the same through multicategorical_evaluate (evaluate_actions(differentiable=True)'s path): one launch each way
      evaluate_only / grad_only   the two launches on their own
  (d) copy_sample / copy_grad   a `copy_` of as many bytes as (b) and grad_only move (logits in, results out / logits in, gradient out):
                         how far from a plain stream the kernels are
The head takes only its device from the engine, so a small Chain-4 batch stands behind every shape."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from marlon_amd import engine  # noqa: E402
from marlon_amd._abi import EnvSpec  # noqa: E402
from marlon_amd.flatten import flatten  # noqa: E402
from marlon_amd.samples import chainpattern  # noqa: E402

REPS = int(os.environ.get("BENCH_MULTICATEGORICAL_REPS", "20"))
INNER = 5                                                # calls between two events: a single launch is too short a window


def defender_nvec(N):
    return [5, N, N, 6, 2, N, 6, 2, N, 3, N, 3]


SHAPES = {
    "chain10_defender": (65536, defender_nvec(12)),
    "chain10_attacker": (65536, [3, 12, 5, 12, 12, 2, 12, 12, 8, 12]),
    "toyctf_defender": (16384, defender_nvec(10)),
}


def composite_parts(logits, nvec):
    return [torch.distributions.Categorical(logits=s) for s in torch.split(logits, nvec, dim=1)]


def main(names):
    eng = engine.BatchEngine(flatten(chainpattern.new_environment(4)),
                             EnvSpec(n_envs=64, maximum_node_count=6, maximum_total_credentials=6, attacker_goal=dict(own_atleast_percent=1.0)))
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(0)
    for name in names:
        n, nvec = SHAPES[name]
        D, A = len(nvec), sum(nvec)
        mb = min(16384, n)
        w1, w2 = torch.randn(mb, generator=g, device=dev), torch.randn(mb, generator=g, device=dev)
        for dtype in (torch.float32, torch.bfloat16):
            src = (torch.randn((n, A), generator=g, device=dev) * 4.0).to(dtype)
            mb_logits = src[torch.randperm(n, generator=g, device=dev)[:mb]].contiguous()
            mb_actions = eng.multicategorical(mb_logits, nvec, seed=1, step=0).actions
            out = (torch.empty((n, D), dtype=torch.int64, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev))
            leaf = mb_logits.clone().requires_grad_(True)
            grad_buf = torch.empty_like(mb_logits)
            es = src.element_size()
            sample_bytes = n * (A * es + D * 8 + 8)             # logits in; actions, log_prob and entropy out
            grad_bytes = mb * (2 * A * es + D * 8 + 8)         # logits, actions and the two incoming gradients in; the gradient out
            copy_a, copy_b = (torch.empty(sample_bytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
            copy_c, copy_d = (torch.empty(grad_bytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))

            def composite():
                dists = composite_parts(src, nvec)
                a = torch.stack([q.sample() for q in dists], dim=1)
                lp = torch.stack([q.log_prob(c) for q, c in zip(dists, torch.unbind(a, dim=1))], dim=1).sum(dim=1)
                ent = torch.stack([q.entropy() for q in dists], dim=1).sum(dim=1)
                return a, lp, ent

            def composite_fwd_bwd():
                dists = composite_parts(leaf, nvec)
                lp = torch.stack([q.log_prob(c) for q, c in zip(dists, torch.unbind(mb_actions, dim=1))], dim=1).sum(dim=1)
                ent = torch.stack([q.entropy() for q in dists], dim=1).sum(dim=1)
                return torch.autograd.grad((lp * w1).sum() + (ent * w2).sum(), leaf)[0]

            def evaluate_fwd_bwd():
                r = eng.multicategorical_evaluate(leaf, nvec, mb_actions)
                return torch.autograd.grad((r.log_prob * w1).sum() + (r.entropy * w2).sum(), leaf)[0]

            legs = {
                "composite": composite,
                "kernel_sample": lambda: eng.multicategorical(src, nvec, mode="sample", seed=1, step=1, out=out),
                "copy_sample": lambda: copy_b.copy_(copy_a),
                "composite_fwd_bwd": composite_fwd_bwd,
                "evaluate_fwd_bwd": evaluate_fwd_bwd,
                "evaluate_only": lambda: eng.multicategorical(mb_logits, nvec, mode="evaluate", actions=mb_actions),
                "grad_only": lambda: eng.multicategorical_grad(mb_logits, nvec, mb_actions, w1, w2, out=grad_buf),
                "copy_grad": lambda: copy_d.copy_(copy_c),
            }
            for fn in legs.values():                         # warm up every shape
                fn()
                fn()
            torch.cuda.synchronize()
            each = {k: [] for k in legs}
            for _ in range(REPS):                            # alternating legs: drift of the shared machine hits all alike
                for k, fn in legs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(INNER):
                        fn()
                    e1.record()
                    e1.synchronize()
                    each[k].append(e0.elapsed_time(e1) / INNER)
            row = dict(shape=name, rows=n, dims=D, logits_per_row=A, dtype=str(dtype).split(".")[-1], reps=REPS, minibatch_rows=mb,
                       sample_bytes=sample_bytes, grad_bytes=grad_bytes)
            for k, v in each.items():
                v = sorted(v)
                row[f"{k}_us"] = round(v[len(v) // 2] * 1e3, 1)
                row[f"{k}_us_min_max"] = [round(v[0] * 1e3, 1), round(v[-1] * 1e3, 1)]
            row["sample_speedup"] = round(row["composite_us"] / row["kernel_sample_us"], 1)
            row["fwd_bwd_speedup"] = round(row["composite_fwd_bwd_us"] / row["evaluate_fwd_bwd_us"], 1)
            row["sample_over_copy"] = round(row["kernel_sample_us"] / row["copy_sample_us"], 2)
            row["grad_over_copy"] = round(row["grad_only_us"] / row["copy_grad_us"], 2)
            row["sample_GBps"] = round(sample_bytes / (row["kernel_sample_us"] * 1e-6) / 1e9, 1)
            row["grad_GBps"] = round(grad_bytes / (row["grad_only_us"] * 1e-6) / 1e9, 1)
            print(json.dumps(row), flush=True)
            del src, mb_logits, leaf, grad_buf, copy_a, copy_b, copy_c, copy_d
    eng.close()


if __name__ == "__main__":
    main(sys.argv[1:] or list(SHAPES))
