#!/usr/bin/env python3
"""mcbs_gae (generalized advantage estimation, one launch for a whole [T, E] rollout) on the MI355X, one JSON line.  Three shapes:
[128, 65 536], [2 048, 4 096] (the reference's N_STEPS; only 64 wavefronts: latency-bound, reported as it is) and [128, 65 536] with the
truncation bootstrap.  Per shape, legs alternating inside one process, device events around groups of launches after a warm-up, every leg
timed over at least 100 launches and 0.2 s (the torch loop: at least 3 runs):
  (a) kernel     engine.gae of the product library: us per launch and bytes / time, bytes from the shape (17 B per (t, e): rewards,
                 values, advantages, returns 4 B each + 1 B of episode_starts; 21 B with bootstrap)
  (b) torch      the same loop as T iterations of torch expressions on the device; its outputs are checked bit-equal to the kernel's
  (c) copy       a `copy_` that reads and writes as many bytes in all as (a) does: the achievable-bandwidth yardstick
  (d) u4/u8/u16  the kernel built with each candidate block length (`make -C marlon_amd/csrc gae-variants`, built here when missing:
                 a compile-time switch, -DMCBS_GAE_U=n; the product reads no environment variable), outputs checked bit-equal to (a)'s
Reported per leg: the median and the minimum over the groups."""
import ctypes as C
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
from marlon_amd import engine  # noqa: E402
from marlon_amd._abi import EnvSpec, GaeIO  # noqa: E402
from marlon_amd.flatten import flatten  # noqa: E402
from marlon_amd.samples import chainpattern  # noqa: E402

SHAPES = [(128, 65536, False), (2048, 4096, False), (128, 65536, True)]
CANDIDATES = (4, 8, 16)
GAMMA, LAMBDA = 0.99, 0.95
MIN_LAUNCHES, MIN_SECONDS, GROUP = 100, 0.2, 25


def variant_path(u):
    return os.path.join(REPO, "marlon_amd", f"libmcbs_gae_u{u}.so")


def variant_call(u, topo, spec):
    """mcbs_gae of the library built with MCBS_GAE_U = u, with a batch of its own (which only supplies the device) -> call(io, stream)."""
    lib = engine.load_library(variant_path(u))
    blob = bytes(topo.blob)
    topo_h, batch_h = C.c_void_p(), C.c_void_p()
    assert lib.mcbs_topology_create(blob, len(blob), spec.device, C.byref(topo_h)) == 0, lib.mcbs_last_error()
    cfg = spec.to_cfg()
    assert lib.mcbs_batch_create(topo_h, C.byref(cfg), C.byref(batch_h)) == 0, lib.mcbs_last_error()

    def call(io, stream):
        assert lib.mcbs_gae(batch_h, C.byref(io), stream) == 0, lib.mcbs_last_error()
    call.keep = (lib, topo_h, batch_h, cfg, blob)
    return call


def torch_loop(r, v, s, lv, ld, b, adv, ret):
    """The loop of tests/gae_ref.py as torch expressions on the device: one small launch per operation."""
    T = r.shape[0]
    nstart = 1.0 - s.float()
    last = 0
    for t in reversed(range(T)):
        nnt, nv = (1.0 - ld.float(), lv) if t == T - 1 else (nstart[t + 1], v[t + 1])
        rew = r[t] if b is None else r[t] + GAMMA * b[t]
        delta = rew + GAMMA * nv * nnt - v[t]
        last = delta + GAMMA * LAMBDA * nnt * last
        adv[t] = last
    torch.add(adv, v, out=ret)


def timed(legs, floors):
    """Alternate the legs in groups until each has its floor of launches and MIN_SECONDS of device time -> {leg: [us per launch per group]}."""
    per = {k: [] for k in legs}
    total = {k: 0.0 for k in legs}
    count = {k: 0 for k in legs}
    while True:
        todo = [k for k in legs if count[k] < floors[k][0] or (total[k] < MIN_SECONDS and count[k] < floors[k][2])]
        if not todo:
            return per
        for k in todo:
            n = floors[k][1]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                legs[k]()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            per[k].append(ms * 1e3 / n)
            total[k] += ms * 1e-3
            count[k] += n


def main():
    missing = [u for u in CANDIDATES if not os.path.exists(variant_path(u))]
    if missing:
        subprocess.run(["make", "-C", os.path.join(REPO, "marlon_amd", "csrc"), "gae-variants"], check=True)
    topo = flatten(chainpattern.new_environment(4))
    spec = EnvSpec(n_envs=64, maximum_node_count=6, maximum_total_credentials=6, attacker_goal=dict(own_atleast_percent=1.0))
    eng = engine.BatchEngine(topo, spec)
    dev = eng.device
    variants = {u: variant_call(u, topo, spec) for u in CANDIDATES}
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for T, E, boot in SHAPES:
        r = 5.0 * torch.randn((T, E), generator=g, device=dev)
        v = 3.0 * torch.randn((T, E), generator=g, device=dev)
        s = (torch.rand((T, E), generator=g, device=dev) < 0.01).to(torch.uint8)
        lv = 3.0 * torch.randn(E, generator=g, device=dev)
        ld = (torch.rand(E, generator=g, device=dev) < 0.5).to(torch.uint8)
        b = torch.where(torch.rand((T, E), generator=g, device=dev) < 0.01, 3.0 * torch.randn((T, E), generator=g, device=dev),
                        torch.zeros((), device=dev)) if boot else None
        adv, ret = torch.empty_like(r), torch.empty_like(r)
        adv_t, ret_t = torch.empty_like(r), torch.empty_like(r)
        adv_u, ret_u = torch.empty_like(r), torch.empty_like(r)
        nbytes = T * E * (21 if boot else 17)
        src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev), torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        io = GaeIO(r.data_ptr(), v.data_ptr(), s.data_ptr(), b.data_ptr() if boot else None, lv.data_ptr(), ld.data_ptr(), adv_u.data_ptr(),
                   ret_u.data_ptr(), T, E, E, E, E, E if boot else 0, E, E, GAMMA, LAMBDA)
        legs = {"kernel": lambda: eng.gae(r, v, s, lv, ld, GAMMA, LAMBDA, bootstrap=b, advantages=adv, returns=ret),
                "torch": lambda: torch_loop(r, v, s, lv, ld, b, adv_t, ret_t),
                "copy": lambda: dst.copy_(src)}
        for u, call in variants.items():
            legs[f"u{u}"] = (lambda call=call: call(io, eng._stream()))
        # warm up every leg, and check the outputs against each other bit for bit
        legs["kernel"]()
        legs["torch"]()
        legs["copy"]()
        same = {"torch": bool(torch.equal(adv.view(torch.int32), adv_t.view(torch.int32)) and torch.equal(ret.view(torch.int32), ret_t.view(torch.int32)))}
        for u in CANDIDATES:
            adv_u.zero_()
            ret_u.zero_()
            legs[f"u{u}"]()
            same[f"u{u}"] = bool(torch.equal(adv.view(torch.int32), adv_u.view(torch.int32)) and torch.equal(ret.view(torch.int32), ret_u.view(torch.int32)))
        torch.cuda.synchronize()
        # (least launches, launches per group, most launches): the torch loop is T * ~8 launches a run, so a few runs must do
        floors = {k: (MIN_LAUNCHES, GROUP, 20000) for k in legs}
        floors["torch"] = (3, 1, 3)
        per = timed(legs, floors)
        row = dict(T=T, E=E, bootstrap=boot, bytes=nbytes, bit_equal=same)
        for k, xs in per.items():
            xs = sorted(xs)
            row[f"{k}_us"] = round(xs[len(xs) // 2], 2)
            row[f"{k}_us_min"] = round(xs[0], 2)
            row[f"{k}_launches"] = len(xs) * floors[k][1]
        for k in ("kernel", "copy") + tuple(f"u{u}" for u in CANDIDATES):
            row[f"{k}_GBps"] = round(nbytes / (row[f"{k}_us"] * 1e-6) / 1e9, 1)
        row["kernel_share_of_copy"] = round(row["copy_us"] / row["kernel_us"], 3)
        rows.append(row)
        del r, v, s, b, adv, ret, adv_t, ret_t, adv_u, ret_u, src, dst
    print(json.dumps(dict(tool="bench_gae", candidates=list(CANDIDATES), gamma=GAMMA, gae_lambda=LAMBDA,
                          min_launches=MIN_LAUNCHES, min_seconds=MIN_SECONDS, shapes=rows)), flush=True)
    assert all(all(row["bit_equal"].values()) for row in rows), "a leg's outputs differ from the kernel's"
    eng.close()


if __name__ == "__main__":
    main()
