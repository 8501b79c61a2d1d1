#!/usr/bin/env python3
"""The feature encoder (mcbs_encode_features) on the headline batch (65 536 Chain-10 envs at 12/12) and ToyCtf (config 3, 16 384 envs),
fp32 and bf16, without and with the mask columns; HIP events around 10 launches after a warm-up.  One JSON line per case with us and
GB/s (bytes = the feature rows written, E * F * itemsize) of
  (a) kernel      mcbs_encode_features into rows padded to whole 128-byte lines (what AttackerVecEnv.features allocates),
  (b) composite   what Stable-Baselines3's preprocess_obs + CombinedExtractor does with the same device tensors: per key split(1, dim=1),
                  one F.one_hot per element, cat, .float(); masks .float(); then one cat over the keys (sorted),
  (c) fill        a plain fill_ of the kernel's output buffer: the practical store ceiling for these bytes.
`kernel_over_fill` = (c) / (a) is the share of the plain fill's store rate the kernel reaches."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402
from marlon_amd.features import ARRAY_KEYS, MASK_KEYS, SCALAR_KEYS, FeatureLayout  # noqa: E402
from tools import workloads as Wl  # noqa: E402

names = sys.argv[1:] or ["headline", "config3"]


def launch_us(fn, reps: int = 10) -> float:
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def composite(obs, masks, layout, dtype):
    """SB3-style: obs = the wrapper's observation keys as device tensors ([E] counts, [E, n] arrays), masks = key -> bool [E, n]"""
    classes = {}
    for k, _, n in layout.groups:
        classes.setdefault(k, []).append(n)
    parts = []
    for k in layout.keys:
        if k in masks:
            parts.append(masks[k].to(dtype))
            continue
        v = obs[k].long().reshape(obs[k].shape[0], -1)
        parts.append(torch.cat([TF.one_hot(col.squeeze(1), n) for col, n in zip(v.split(1, dim=1), classes[k])], dim=1).to(dtype))
    return torch.cat(parts, dim=1)


for name in names:
    ring = Wl.record_ring(name, 40)
    eng, topo, spec, desc = Wl.make_engine(name)
    E = eng.E
    fields = eng.alloc_obs(Wl.OBS_FIELDS[:5])
    for t in range(40):
        eng.step(ring[t], with_info=False)
    eng.observe(fields)
    bits = eng.pack_action_mask()
    obs = {k: fields["scalars"][:, i] for i, k in enumerate(SCALAR_KEYS)}
    obs.update({k: fields[k].reshape(E, -1) for k in ARRAY_KEYS})
    for include_masks in (False, True):
        layout = FeatureLayout(topo, spec, include_masks=include_masks)
        handle = eng.feature_layout(layout)
        masks = {}
        if include_masks:
            flat = eng.unpack_action_mask(bits)
            masks = {k: flat[:, layout.mask_ranges[i][2]:layout.mask_ranges[i][2] + layout.mask_ranges[i][1]]
                     for i, k in enumerate(k for k in layout.keys if k in MASK_KEYS)}
        for dtype in (torch.float32, torch.bfloat16):
            item = torch.empty((), dtype=dtype).element_size()
            out = torch.empty((E, layout.padded_width(item)), dtype=dtype, device=eng.device)
            nbytes = E * layout.width * item
            row = dict(workload=name, envs=E, columns=layout.width, masks=include_masks, dtype=str(dtype).split(".")[-1], bytes=nbytes)
            k_us = launch_us(lambda: eng.encode_features(handle, fields, bits=bits if include_masks else None, out=out))
            got = out[:, :layout.width].clone()
            f_us = launch_us(lambda: out.fill_(1.0))
            want = composite(obs, masks, layout, dtype)
            assert torch.equal(got, want), "kernel and composite disagree"
            del want, got
            c_us = launch_us(lambda: composite(obs, masks, layout, dtype), reps=3)
            row.update(kernel_us=round(k_us, 1), kernel_GBps=round(nbytes / k_us / 1e3, 1), composite_us=round(c_us, 1),
                       composite_GBps=round(nbytes / c_us / 1e3, 1), fill_us=round(f_us, 1), fill_GBps=round(out.numel() * item / f_us / 1e3, 1),
                       composite_over_kernel=round(c_us / k_us, 1), kernel_over_fill=round(f_us / k_us, 3))
            print(json.dumps(row), flush=True)
            del out
        handle.close()
        del masks
    eng.close()
