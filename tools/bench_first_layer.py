#!/usr/bin/env python3
"""The first layer from the observation (mcbs_first_layer, mcbs_first_layer_packed, mcbs_first_layer_grad) against the composite it
replaces — feature rows, then torch.nn.functional.linear — on the MI355X: one JSON line.  Two workloads: 65 536 Chain-10 envs at 12/12
and 16 384 ToyCtf envs at 12/10 (AttackerVecEnv, discrete, masks not materialised), advanced by 40 masked uniformly random steps, then
T = 8 more stored as packed rows.  Both sides of every comparison alternate inside one process, device events around groups of calls
after a warm-up, every leg timed over at least 100 calls and 0.2 s; reported: median and minimum over the groups.  H in {64, 128},
float32 and bfloat16 parameters (the feature rows and the outputs in the parameters' dtype).
  (a) live     `features(out=)` + `F.linear(x, W, b)` against `first_layer(W, b, weight_t=, out=)` on the live observation
  (b) update   a 16 384-row minibatch drawn from the T stored steps, forward and backward of a scalar loss:
               `encode_features_packed(index=)` + `F.linear` + autograd against `encode_first_layer_packed(differentiable=True)`;
               peak memory of each side from torch.cuda.max_memory_allocated (above what was allocated before the leg); and the fused
               side's two library calls on their own, without autograd around them (`forward_call`, `grad_call`)
The fused outputs are checked against the composite's to rounding before anything is timed."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402
from marlon_amd.wrappers import AttackerVecEnv  # noqa: E402
from tools import workloads as Wl  # noqa: E402
from tools.bench_obs_packing import summary, timed  # noqa: E402

T, BATCH, ADVANCE = 8, 16384, 40
HS = (64, 128)


def peak_of(fn):
    """bytes allocated at the peak of fn() above what was allocated before it"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    rows = []
    for name in sys.argv[1:] or ["headline", "config3"]:
        environment, E, kw = Wl.wrapper_workload(name)
        env = AttackerVecEnv(environment, E, discrete=True, materialize_masks=False, seed=7, **kw)
        dev = env.engine.device
        for t in range(ADVANCE):
            env.step(env.sample_masked_uniform(seed=7, step=t).actions)
        buf = env.rollout_buffer(T, pack_observations=True)
        for t in range(T):
            env.observation_packed(out=buf.observations["packed"][t])
            env.step(env.sample_masked_uniform(seed=7, step=ADVANCE + t).actions)
        storage = buf.observations["packed"].view(T * E, -1)
        idx = torch.randperm(T * E, device=dev, generator=torch.Generator(device=dev).manual_seed(1))[:BATCH].contiguous()
        layout = env.feature_layout()
        F = layout.width
        row = dict(workload=name, envs=E, columns=F, elements=layout.n_elements)
        for H in HS:
            for label, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
                tag = f"h{H}_{label}"
                g = torch.Generator(device=dev).manual_seed(H)
                weight = (torch.randn((H, F), device=dev, generator=g) / 16).to(dtype).requires_grad_(True)
                bias = torch.randn((H,), device=dev, generator=g).to(dtype).requires_grad_(True)
                weight_t = weight.detach().t().contiguous()
                item = weight.element_size()
                # (a) the live observation
                x_live = torch.empty((E, layout.padded_width(item)), dtype=dtype, device=dev)
                out_live = torch.empty((E, H), dtype=dtype, device=dev)
                with torch.no_grad():
                    legs = {f"live_{tag}_composite": lambda: TF.linear(env.features(out=x_live[:, :F]), weight, bias),
                            f"live_{tag}_fused": lambda: env.first_layer(weight, bias, weight_t=weight_t, out=out_live)}
                    a, b = (fn() for fn in legs.values())
                    tol = 1e-4 if dtype == torch.float32 else 2e-2
                    row[f"live_{tag}_max_diff"] = float((a.float() - b.float()).abs().max())
                    assert torch.allclose(a.float(), b.float(), rtol=tol, atol=tol), f"{name} {tag}: the fused first layer differs from the composite"
                    torch.cuda.synchronize()
                    row.update(summary(timed(legs)))
                row[f"live_{tag}_composite_over_fused"] = round(row[f"live_{tag}_composite_us"] / row[f"live_{tag}_fused_us"], 2)
                del x_live, out_live
                # (b) a minibatch of the stored steps, forward and backward
                coef = torch.randn((BATCH, H), device=dev, generator=g).to(dtype)

                def composite():
                    weight.grad = bias.grad = None
                    x = env.encode_features_packed(storage, index=idx, dtype=dtype)
                    (TF.linear(x, weight, bias) * coef).sum().backward()

                def fused():
                    weight.grad = bias.grad = None
                    h = env.encode_first_layer_packed(storage, weight, bias, index=idx, dtype=dtype, differentiable=True)
                    (h * coef).sum().backward()

                legs = {f"update_{tag}_composite": composite, f"update_{tag}_fused": fused}
                grads = []
                for fn in legs.values():
                    fn()
                    grads.append((weight.grad.float().clone(), bias.grad.float().clone()))
                row[f"update_{tag}_grad_max_diff"] = float((grads[0][0] - grads[1][0]).abs().max())
                scale = float(grads[0][0].abs().max())
                assert row[f"update_{tag}_grad_max_diff"] <= (1e-4 if dtype == torch.float32 else 2e-2) * max(scale, 1.0), f"{name} {tag}: weight gradients differ"
                del grads
                for k, fn in legs.items():
                    row[f"{k}_peak_bytes"] = peak_of(fn)
                torch.cuda.synchronize()
                row.update(summary(timed(legs)))
                row[f"update_{tag}_composite_over_fused"] = round(row[f"update_{tag}_composite_us"] / row[f"update_{tag}_fused_us"], 2)
                # the fused side's two library calls on their own (preallocated output and workspace, no autograd around them)
                handle, pk = env._feature_handle(False, False), env._packing_handle()
                gout = coef.float()
                out_mb = torch.empty((BATCH, H), dtype=dtype, device=dev)
                ws = torch.empty(env.engine.first_layer_grad_workspace(handle, BATCH, H), dtype=torch.uint8, device=dev)
                gw, gb = torch.empty((F, H), device=dev), torch.empty((H,), device=dev)
                with torch.no_grad():
                    legs = {f"update_{tag}_forward_call": lambda: env.engine.first_layer(handle, weight_t, bias, packing=pk, packed=storage, index=idx, out=out_mb),
                            f"update_{tag}_grad_call": lambda: env.engine.first_layer_grad(handle, gout, packing=pk, packed=storage, index=idx, out=(gw, gb),
                                                                                          workspace=ws)}
                    for fn in legs.values():
                        fn()
                    torch.cuda.synchronize()
                    row.update(summary(timed(legs)))
                del gout, out_mb, ws, gw, gb
                weight.grad = bias.grad = None
                del coef
        rows.append(row)
        env.close()
        del env, buf, storage
    print(json.dumps(dict(tool="bench_first_layer", stored_steps=T, minibatch=BATCH, workloads=rows)), flush=True)


if __name__ == "__main__":
    main()
