#!/usr/bin/env python3
"""Host-side cost of one `step` of the four wrapper classes, at a shape where the kernels are short and the call is all host: 64 Chain-4
envs (6 nodes, 6 credentials), Discrete attacker, masks not materialised.  N calls enqueued back to back after a warm-up, one
synchronize, us per call; one JSON line per process.  To compare two commits, run it from each tree alternately, several processes each
(tools/bench_binding_overhead.py has the method).  Legs: AttackerVecEnv (fields and packed observations), DefenderVecEnv (dense and
packed; one attacker step is not part of the timed call), TwoAgentVecEnv, TwoAgentTrainVecEnv.  The actions are one contiguous int64
device tensor per side, handed in unchanged every call: the policy's own tensor, the wrappers' fast path."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from marlon_amd.samples import chainpattern  # noqa: E402
from marlon_amd.wrappers import AttackerVecEnv, DefenderVecEnv, TwoAgentTrainVecEnv, TwoAgentVecEnv  # noqa: E402

label = sys.argv[1] if len(sys.argv) > 1 else ""
N = int(os.environ.get("BENCH_WRAPPER_CALLS", "3000"))
E = 64
env = chainpattern.new_environment(4)


def attacker(**kw):
    return AttackerVecEnv(env, E, maximum_node_count=6, maximum_total_credentials=6, discrete=True, materialize_masks=False, **kw)


def attacker_leg(**kw):
    att = attacker(**kw)
    a = torch.zeros(E, dtype=torch.int64, device=att.engine.device)
    return att, lambda: att.step(a)


def defender_leg(**kw):
    att = attacker(learned_defender=True)
    dfd = DefenderVecEnv(att, **kw)
    d = torch.zeros((E, 12), dtype=torch.int64, device=att.engine.device)
    return att, lambda: dfd.step(d)


def two_agent_leg(cls, auto_reset):
    att = attacker(learned_defender=True, auto_reset=auto_reset)
    turn = cls(att, DefenderVecEnv(att))
    a = torch.zeros(E, dtype=torch.int64, device=att.engine.device)
    d = torch.zeros((E, 12), dtype=torch.int64, device=att.engine.device)
    return att, lambda: turn.step(a, d)


legs = {
    "attacker": attacker_leg,
    "attacker_packed": lambda: attacker_leg(observation_format="packed"),
    "defender": defender_leg,
    "defender_packed": lambda: defender_leg(observation_format="packed"),
    "two_agent": lambda: two_agent_leg(TwoAgentVecEnv, False),
    "two_agent_train": lambda: two_agent_leg(TwoAgentTrainVecEnv, True),
}
row = {"label": label, "envs": E, "calls": N}
for name, make in legs.items():
    att, fn = make()
    for _ in range(200):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(N):
        fn()
    torch.cuda.synchronize()
    row[f"{name}_us"] = round((time.perf_counter() - t0) / N * 1e6, 3)
    att.close()
print(json.dumps(row), flush=True)
