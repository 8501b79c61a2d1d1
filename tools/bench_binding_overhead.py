#!/usr/bin/env python3
"""Host-side cost of the BatchEngine calls whose wall time is mostly Python: per-call wall time at a shape where the kernels are short,
64 Chain-4 envs (6 nodes, 6 credentials).  N calls enqueued back to back after a warm-up, one synchronize, us per call; one JSON line per
process.  To compare two commits, run it from each tree alternately, several processes each: the figure moves by some percent from
process to process.  Legs: masked_categorical and masked_linear_categorical (live, mode "sample", fp32, H = 64), apply_packed_mask,
multicategorical ("sample" over the defender's MultiDiscrete for N = 6), gae (T = 32).  The first two run at the device's pace."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from marlon_amd import engine, flatten  # noqa: E402
from marlon_amd._abi import EnvSpec  # noqa: E402
from marlon_amd.samples import chainpattern  # noqa: E402

label = sys.argv[1] if len(sys.argv) > 1 else ""
N = int(os.environ.get("BENCH_BINDING_CALLS", "3000"))
E, H, T = 64, 64, 32
eng = engine.BatchEngine(flatten.flatten(chainpattern.new_environment(4)), EnvSpec(n_envs=E, maximum_node_count=6, maximum_total_credentials=6))
dev = eng.device
eng.reset()
eng.observe(eng.alloc_obs(["scalars", "nodes_privilegelevel"]))
A = eng.discrete_action_count()
g = torch.Generator().manual_seed(0)
rand = lambda *shape: torch.randn(*shape, generator=g).to(dev)
logits, latent, weight, bias = rand(E, A), rand(E, H), rand(A, H), rand(A)
work, bits = logits.clone(), eng.pack_action_mask()
nvec = (5, 6, 6, 6, 2, 6, 6, 2, 6, 3, 6, 3)
mlogits = rand(E, sum(nvec))
rew, val, lv = rand(T, E), rand(T, E), rand(E)
starts, ld = torch.zeros((T, E), dtype=torch.uint8, device=dev), torch.zeros(E, dtype=torch.uint8, device=dev)
adv, ret = torch.empty_like(rew), torch.empty_like(rew)
legs = {
    "masked_categorical": lambda i: eng.masked_categorical(logits, mode="sample", seed=1, step=i),
    "masked_linear_categorical": lambda i: eng.masked_linear_categorical(latent, weight, bias, mode="sample", seed=1, step=i),
    "apply_packed_mask": lambda i: eng.apply_packed_mask(bits, work),
    "multicategorical": lambda i: eng.multicategorical(mlogits, nvec, mode="sample", seed=1, step=i),
    "gae": lambda i: eng.gae(rew, val, starts, lv, ld, 0.99, 0.95, advantages=adv, returns=ret),
}
row = {"label": label, "envs": E, "calls": N}
for name, fn in legs.items():
    for i in range(200):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(N):
        fn(i)
    torch.cuda.synchronize()
    row[f"{name}_us"] = round((time.perf_counter() - t0) / N * 1e6, 3)
eng.close()
print(json.dumps(row), flush=True)
