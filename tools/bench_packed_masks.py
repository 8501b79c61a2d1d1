#!/usr/bin/env python3
"""Bit-packed Discrete action masks on the headline batch (65 536 Chain-10 envs): us per launch of mcbs_pack_action_mask,
mcbs_apply_packed_mask (fp32 / bf16 logits, dense [E, A] rows) and mcbs_unpack_action_mask after 1 / 40 / 200 steps, with
mcbs_mask_logits on the same shape next to them; then the lean wrapper step + pack against the materialised-mask wrapper step.
One JSON line per case.  Bytes are what each kernel must move (apply and mask_logits are write-only: the masked-out logits; apply
and unpack also read the bits); `of_8TBps` = those bytes over the time, as a share of the 8 TB/s peak."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from tools import workloads as Wl  # noqa: E402

PEAK = 8.0e12
name = sys.argv[1] if len(sys.argv) > 1 else "headline"


def launch_us(fn, reps: int = 10) -> float:
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def emit(row, nbytes, us):
    row.update(us=round(us, 1), bytes=int(nbytes), GBps=round(nbytes / us / 1e3, 1), of_8TBps=round(nbytes / (us * 1e-6) / PEAK, 3))
    print(json.dumps(row), flush=True)


ring = Wl.record_ring(name, 200)
eng, topo, spec, desc = Wl.make_engine(name)
E, A = eng.E, eng.discrete_action_count()
W, row_words = eng.packed_mask_words()
obs = eng.alloc_obs(Wl.OBS_FIELDS[:5])
bits = torch.zeros((E, row_words), dtype=torch.int32, device=eng.device)
t = 0
for upto in (1, 40, 200):
    while t < upto:
        eng.step(ring[t], with_info=False)
        t += 1
    eng.observe(obs)
    base = dict(workload=name, envs=E, actions=A, words=W, row_words=row_words, after_steps=upto)
    emit(dict(base, op="pack"), E * W * 4, launch_us(lambda: eng.pack_action_mask(bits)))
    allowed = int(eng.unpack_action_mask(bits).sum())
    base["allowed_per_env"] = round(allowed / E, 2)
    for dtype in (torch.float32, torch.bfloat16):
        k = str(dtype).split(".")[-1]
        logits = torch.zeros((E, A), dtype=dtype, device=eng.device)
        written = (E * A - allowed) * logits.element_size()
        emit(dict(base, op=f"apply_{k}"), written + E * W * 4, launch_us(lambda: eng.apply_packed_mask(bits, logits)))
        emit(dict(base, op=f"mask_logits_{k}"), written, launch_us(lambda: eng.mask_logits(logits)))
        assert torch.equal(eng.apply_packed_mask(bits, logits.zero_()), eng.mask_logits(logits.clone().zero_()))
        del logits
    out = torch.empty((E, A), dtype=torch.bool, device=eng.device)
    emit(dict(base, op="unpack"), E * W * 4 + E * A, launch_us(lambda: eng.unpack_action_mask(bits, out)))
    del out
eng.close()
del bits

# the wrapper tier: the materialised-mask step against the lean step followed by the pack, on the same recorded actions
from marlon_amd.wrappers import AttackerVecEnv  # noqa: E402
env, E, kw = Wl.wrapper_workload(name)
K = 30
full = AttackerVecEnv(env, E, discrete=True, **kw)
g = torch.Generator(device=full.engine.device).manual_seed(0)
acts = []
for _ in range(K + 5):
    m = full.action_masks()
    acts.append(torch.where(m, torch.rand(m.shape, generator=g, device=m.device), torch.full((1,), -1.0, device=m.device)).argmax(dim=1))
    full.step(acts[-1])
full.reset()
lean = AttackerVecEnv(env, E, discrete=True, materialize_masks=False, **kw)
buf = torch.zeros((K + 5, E, lean.engine.packed_mask_words()[1]), dtype=torch.int32, device=lean.engine.device)


def per_step(fn) -> float:
    for i in range(5):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(5, K + 5):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / K * 1e6


full_us = per_step(lambda i: full.step(acts[i]))
full.close()
lean_pack_us = per_step(lambda i: (lean.step(acts[i]), lean.action_masks_packed(out=buf[i])))
lean.reset()
lean_us = per_step(lambda i: lean.step(acts[i]))
print(json.dumps(dict(workload=name, envs=E, op="wrapper_step", materialised_masks_us=round(full_us, 1), lean_us=round(lean_us, 1),
                      lean_plus_pack_us=round(lean_pack_us, 1), lean_plus_pack_over_materialised=round(lean_pack_us / full_us, 3))), flush=True)
lean.close()
