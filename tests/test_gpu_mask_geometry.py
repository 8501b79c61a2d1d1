"""The four Discrete mask kernels (mcbs_mask_logits, mcbs_pack_action_mask, mcbs_apply_packed_mask, mcbs_unpack_action_mask) at the
geometries, layouts, digest writers and fill values where their branches differ, every check against the oracle's materialised masks
(mask_connect | mask_local | mask_remote in MaskedDiscreteAttackerWrapper's order) or a plain torch expression, bitwise:

* mask_logits over observation bounds that reach the per-bit credential loop (C + GW > 64), connect rows shorter than a group, remote
  rows shorter than a group, odd A and A % 8 == 4, through each launch the host dispatch can pick (fp32 on 16-byte rows and offset
  by one element; bf16 on 16-byte rows, on 8-byte rows and offset by one element), padding filled with a sentinel;
* topologies of 65, 100 and 200 nodes (owned-source bits 64-255 of the digest, action spaces of 1.5 M to 48 M: grid loops and the
  moving bit window), driven by a host policy built from the oracle's observation;
* apply / unpack on random bits of densities 0 .. 1 over those long rows;
* every observation kernel that writes the digest (four envs per wavefront, a wavefront per env, the masked re-observation after a
  reset by mask, the three-launch wrapper step) and steps taken without an observation;
* the bfloat16 rounding of `fill` (ties, overflow to inf, zeros, subnormals, NaN) and the refusals of BatchEngine.mask_logits."""
import struct

import numpy as np
import pytest

from tests import parity
from tests.test_gpu_episodes import _decode_discrete
from tests.test_gpu_packed_masks import BOUNDS, SENTINEL, check_pack, oracle_mask, pack_host

pytestmark = pytest.mark.gpu

MASKS = ["mask_local", "mask_remote", "mask_connect"]
# (name, dtype, elements per row group the stride is a multiple of, offset of the row's first element): the five launches of
# mask_logits / apply_packed_mask — fp32 GW=4 vector stores, fp32 element stores, bf16 GW=8 vector stores (16-byte rows), bf16 GW=4
# vector stores (8-byte rows), bf16 element stores
VARIANTS = [("fp32 16-byte rows", "float32", 4, 0), ("fp32 offset 1", "float32", 4, 1), ("bf16 16-byte rows", "bfloat16", 8, 0),
            ("bf16 8-byte rows", "bfloat16", 8, 4), ("bf16 offset 1", "bfloat16", 8, 1)]


def _f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def _iv(dt):
    import torch
    return torch.int16 if dt == torch.bfloat16 else torch.int32


def _fill_bits(fill, dt):
    """The stored pattern of `fill` in dtype dt (torch's float32 -> bfloat16 rounding: round to nearest even) as a Python int."""
    import torch
    return int(torch.tensor(fill, dtype=torch.float32).to(dt).view(_iv(dt)).item())


def _logits(n, A, g, dev):
    """fp32 [n, A]: normal values with NaNs carrying payloads (quiet and signalling), +inf and -inf sprinkled in; a write-only kernel
    leaves them as they are where the mask allows."""
    import torch
    x = torch.randn((n, A), generator=g, device=dev)
    flat = x.view(-1).view(torch.int32)
    for k, (start, step, bits) in enumerate(((0, 37, 0x7FC01234), (5, 41, 0x7F800001 + 0x55), (11, 43, 0x7F800000), (17, 47, -0x00800000),
                                            (23, 53, -0x003FEDCC))):
        flat[start::step] = bits
    return x


def run_variants(call, logits, mask, fill, ctx, variants=VARIANTS):
    """For every launch variant: a buffer of sentinel patterns, `logits` copied into a view of it at the variant's stride and offset,
    call(view) masks it in place.  The view equals where(mask, logits, fill) bitwise; every element outside it keeps the sentinel."""
    import torch
    n, A = logits.shape
    for name, dts, group, off in variants:
        dt = getattr(torch, dts)
        iv = _iv(dt)
        src = logits.to(dt)
        want = torch.where(mask, src.view(iv), _fill_bits(fill, dt))
        stride = (A + off + group - 1) // group * group + group
        sent = SENTINEL if iv == torch.int32 else SENTINEL & 0x7FFF
        buf = torch.full((n, stride), sent, dtype=iv, device=logits.device)
        v = buf.view(dt)[:, off:off + A]
        esz = v.element_size()
        assert buf.data_ptr() % 16 == 0 and (stride * esz) % 16 == 0
        assert (v.data_ptr() % 16 == 0) == (off == 0) and (v.data_ptr() % 8 == 0) == (off * esz % 8 == 0), f"{ctx} {name}: layout"
        v.copy_(src)
        call(v)
        assert torch.equal(v.view(iv), want), f"{ctx} {name}: {int((v.view(iv) != want).sum())} elements differ"
        rest = buf.clone()
        rest[:, off:off + A] = sent
        assert bool((rest == sent).all()), f"{ctx} {name}: written outside the rows"
        del buf, v, rest, want, src


def _masked_logits_check(eng, mask_np, g, ctx, fill=-1e8):
    import torch
    dev = eng.device
    mask = torch.as_tensor(mask_np).to(dev)
    logits = _logits(eng.E, mask.shape[1], g, dev)
    run_variants(lambda v: eng.mask_logits(v, fill), logits, mask, fill, f"{ctx} mask_logits")
    d = logits.clone()                                  # the dense [E, A] tensor as a caller allocates it
    eng.mask_logits(d, fill)
    assert torch.equal(d.view(torch.int32), torch.where(mask, logits.view(torch.int32), _fill_bits(fill, torch.float32))), f"{ctx} dense fp32"
    return mask, logits


# ---------------------------------------------------------------------------------------------------------------- 1. bounds sweep
# (trace, (maximum_node_count, maximum_total_credentials)) beyond test_gpu_packed_masks.BOUNDS: credential periods with C + 4 > 64
# (fp32 and bf16 take the per-bit loop) and C + 8 > 64 only (bf16 GW=8 alone), connect rows shorter than a group (RL = P*C < GW:
# mask_at per element), remote rows shorter than 8 (Kitchen-sink, R = 5), odd A and A % 8 == 4
LOGITS_BOUNDS = BOUNDS + [
    ("toyctf_defender_s11", (10, 61)),      # C + 4 > 64; A 43 530
    ("toyctf_defender_s11", (11, 64)),      # C = 64; A 55 209 (odd)
    ("chain4_defender_s21", (6, 57)),       # C + 8 > 64 > C + 4
    ("tiny_defender_s62", (4, 1)),          # RL 3 < 4; A 84 (A % 8 == 4)
    ("tiny_defender_s62", (4, 2)),          # RL 6 < 8; A 132 (A % 8 == 4)
    ("sink_defender_s43", (7, 8)),          # R 5; A 2 261 (odd)
]


@pytest.mark.parametrize("trace,bounds", LOGITS_BOUNDS, ids=[f"{t}-{n}x{c}" for t, (n, c) in LOGITS_BOUNDS])
def test_mask_logits_over_observation_bounds(trace, bounds):
    """mask_logits == where(oracle mask, logits, fill) through every launch variant and the dense tensor, pack == the host packing,
    at each step of random, valid and out-of-bound actions (blank observations)."""
    import torch
    from marlon_amd import engine
    from marlon_amd._abi import RNG_PHILOX
    from oracle.oracle import Oracle
    _, sj = parity.load_trace(trace)
    topo = parity.topology_for(trace)
    nm, cm = bounds
    assert nm >= topo.n_nodes and cm >= max(1, len(topo.triples))
    E = 256
    spec = parity.spec_from_json(sj, n_envs=E, auto_reset=True, rng_kind=RNG_PHILOX, seed=79, max_episode_steps=30,
                                 maximum_node_count=nm, maximum_total_credentials=cm)
    eng = engine.BatchEngine(topo, spec)
    orc = Oracle(topo, spec)
    A = eng.discrete_action_count()
    g = torch.Generator(device=eng.device).manual_seed(nm * 100 + cm)
    small = ["scalars", "nodes_privilegelevel"]
    obs = eng.alloc_obs(small)
    seen_on = blanks = 0
    for t in range(24):
        a = eng.sample_actions(t % 4 != 3, seed=6, step=t)
        if t % 5 == 1:
            a[::4, 1] = nm + 2                          # out of bound: the blank observation
        oo = orc.alloc_obs(small + MASKS)
        eng.step_observe(a, obs)
        out = orc.step(a.cpu().numpy(), obs=oo)
        blanks += int(out["oob"].sum())
        mask = oracle_mask(oo, E)
        assert mask.shape == (E, A)
        ctx = f"{trace} bounds {bounds} step {t}"
        _masked_logits_check(eng, mask, g, ctx)
        check_pack(eng, pack_host(mask), ctx)
        seen_on += int(mask.sum())
    assert seen_on > 0 and blanks > 0
    eng.close()


# ------------------------------------------------------------------------------------------------------- 2. large topologies
def _large_topology(name):
    from marlon_amd import flatten as F
    from marlon_amd import model
    from marlon_amd.samples import generate_network, random_net
    if name == "generated65":
        return F.flatten(generate_network.new_environment(15, seed=4))
    if name == "random100":
        return F.flatten(random_net.build(model, 100, 7))
    # 200 nodes: with its single start node the attacker is stuck at 6 discovered nodes (n000 blocks outgoing SSH, and its leaked
    # credentials are SSH ones); four start nodes open the network
    return F.flatten(random_net.build(model, 200, 7, n_start=4))


def _large_spec(topo, E):
    from marlon_amd._abi import EnvSpec
    return EnvSpec(n_envs=E, maximum_node_count=topo.n_nodes, maximum_total_credentials=max(1, len(topo.triples)), attacker_goal=None,
                   maximum_discoverable_credentials_per_action=32)      # the 65-node network leaks up to 10 credentials at once


def host_policy(oo, geom, rng, tried):
    """A Discrete index per env from the oracle's observation: a connect (owned source, cached credential's node and port, credential
    index) to a node not owned yet, else a local exploit, else a remote one on a node not owned (each tried once per env), else any of
    those at random."""
    N, L, R, P, C = geom
    E = oo["scalars"].shape[0]
    out = np.zeros(E, np.int64)
    for e in range(E):
        nd, nc = int(oo["scalars"][e, 6]), int(oo["scalars"][e, 5])
        priv, cm = oo["nodes_privilegelevel"][e], oo["credential_cache_matrix"][e]
        owned = np.flatnonzero(priv[:nd] > 0)
        conn = [(((s * N + int(cm[c, 0])) * P + int(cm[c, 1])) * C + c) for c in range(min(nc, C)) if priv[int(cm[c, 0])] == 0 for s in owned]
        loc = [N * N * P * C + int(i) * L + int(v) for i, v in np.argwhere(oo["mask_local"][e] != 0)]
        rem = [N * N * P * C + N * L + (int(s) * N + int(t)) * R + int(r) for s, t, r in np.argwhere(oo["mask_remote"][e] != 0) if priv[t] == 0]
        for fresh in ([a for a in conn if a not in tried[e]], [a for a in loc if a not in tried[e]], [a for a in rem if a not in tried[e]],
                      conn + loc + rem):
            if fresh:
                out[e] = fresh[rng.integers(len(fresh))]
                tried[e].add(int(out[e]))
                break
    return out


# (topology, envs, steps, checkpoints, deepest owned external index some env must reach)
LARGE = [("generated65", 8, 60, (20, 59), 8),
         ("random100", 4, 180, (60, 179), 64),
         ("random200", 3, 260, (259,), 128)]


@pytest.mark.parametrize("name,E,T,checks,deep", LARGE, ids=[x[0] for x in LARGE])
def test_large_topologies_deep_owned_nodes(name, E, T, checks, deep):
    """Envs driven by the host policy (Discrete indices decoded on the host) on the engine and the oracle alike; at each checkpoint
    mask_logits (every launch variant), pack, unpack(pack) and apply(pack) equal the oracle's mask.  Asserts that some env owns a
    node at external index >= `deep` (digest words 1..3 in use)."""
    import torch
    from marlon_amd import engine
    from oracle.oracle import Oracle
    topo = _large_topology(name)
    spec = _large_spec(topo, E)
    eng = engine.BatchEngine(topo, spec)
    orc = Oracle(topo, spec)
    N, C = spec.maximum_node_count, spec.maximum_total_credentials
    geom = (N, len(topo.local_vulnerabilities), len(topo.remote_vulnerabilities), len(topo.ports), C)
    A = eng.discrete_action_count()
    assert A == N * N * geom[3] * C + N * geom[1] + N * N * geom[2]
    small = ["scalars", "credential_cache_matrix", "nodes_privilegelevel", "mask_local", "mask_remote"]
    obs = eng.alloc_obs(["scalars", "nodes_privilegelevel"])
    oo = orc.observe(orc.alloc_obs(small), reset_obs=True)
    rng = np.random.default_rng(3)
    tried = [set() for _ in range(E)]
    g = torch.Generator(device=eng.device).manual_seed(4)
    deepest = -1
    for t in range(T):
        rows = _decode_discrete(host_policy(oo, geom, rng, tried), *geom)
        a = torch.as_tensor(rows).to(eng.device)
        check = t in checks
        oo = orc.alloc_obs(small + (["mask_connect"] if check else []))
        out = orc.step(rows, obs=oo)
        assert not out["terminated"].any() and out["errors"] == 0
        if not check:
            eng.step(a)
            continue
        eng.step_observe(a, obs)
        np.testing.assert_array_equal(obs["nodes_privilegelevel"].cpu().numpy(), oo["nodes_privilegelevel"], err_msg=f"{name} step {t}")
        own = oo["nodes_privilegelevel"] > 0
        deepest = max(deepest, max(int(np.flatnonzero(r).max(initial=-1)) for r in own))
        ctx = f"{name} (A {A}) step {t}"
        mask = oracle_mask(oo, E)
        assert mask.shape == (E, A) and mask.any()
        mask_dev, logits = _masked_logits_check(eng, mask, g, ctx)
        bits = check_pack(eng, pack_host(mask), ctx)
        assert torch.equal(eng.unpack_action_mask(bits), mask_dev), f"{ctx}: unpack(pack)"
        run_variants(lambda v: eng.apply_packed_mask(bits, v, -2.5), logits, mask_dev, -2.5, f"{ctx} apply(pack)")
        del mask_dev, logits, bits, mask
    print(f"{name}: A {A}, deepest owned external index {deepest}")
    assert deepest >= deep, f"{name}: deepest owned external index {deepest} < {deep}"
    eng.close()


# ------------------------------------------------------------------------------------------ 3. apply / unpack on long random rows
DENSITIES = (0.0, 0.01, 0.5, 0.99, 1.0)


def _random_bits(n, W, g, dev):
    """Bits of densities DENSITIES (row i: DENSITIES[(n + i) % 5]), tail bits of word W-1 included -> (int32 [n, W], bool [n, 32 W])."""
    import torch
    dens = torch.tensor([DENSITIES[(n + i) % 5] for i in range(n)], device=dev)
    m = torch.rand((n, W * 32), generator=g, device=dev) < dens[:, None]
    w = (m.view(n, W, 32).to(torch.int64) << torch.arange(32, device=dev)).sum(-1)
    return (w - ((w >> 31) << 32)).to(torch.int32), m


@pytest.mark.parametrize("name,rows", [("generated65", (1, 3, 5)), ("random100", (1, 3, 5)), ("random200", (1, 3))])
def test_apply_and_unpack_long_random_rows(name, rows):
    """apply_packed_mask == torch.where(bits, logits, fill) through every launch variant (rows of all ones come back bitwise unchanged,
    NaN payloads and infinities included), with dense bits rows and rows of W + 5 words whose extra words hold a sentinel; unpack into a
    dense tensor and into an offset view of a sentinel-filled buffer.  Action spaces of 1.5 M, 5.9 M and 48 M actions."""
    import torch
    from marlon_amd import engine
    topo = _large_topology(name)
    eng = engine.BatchEngine(topo, _large_spec(topo, 1))
    dev = eng.device
    A = eng.discrete_action_count()
    W = (A + 31) // 32
    assert A >= 1_500_000
    g = torch.Generator(device=dev).manual_seed(A % 1000)
    for n in rows:
        bits, m = _random_bits(n, W, g, dev)
        mask = m[:, :A]
        del m
        assert n < 5 or (not bool(mask[(5 - n) % 5].any()) and bool(mask[(9 - n) % 5].all()))
        logits = _logits(n, A, g, dev)
        wide = torch.full((n, W + 5), SENTINEL, dtype=torch.int32, device=dev)
        wide[:, :W] = bits
        for bname, b in (("dense bits", bits), ("bits rows of W + 5 words", wide)):
            ctx = f"{name} A {A} n {n} {bname}"
            run_variants(lambda v: eng.apply_packed_mask(b, v, -3.0), logits, mask, -3.0, f"{ctx} apply")
            assert torch.equal(eng.unpack_action_mask(b), mask), f"{ctx}: unpack"
        ob = torch.full((n, A + 40), 9, dtype=torch.uint8, device=dev)
        eng.unpack_action_mask(wide, out=ob[:, 3:A + 3])
        assert torch.equal(ob[:, 3:A + 3].bool(), mask), f"{name} n {n}: unpack into an offset view"
        assert bool((ob[:, :3] == 9).all()) and bool((ob[:, A + 3:] == 9).all()), f"{name} n {n}: unpack wrote outside the view"
        assert bool((wide[:, W:] == SENTINEL).all())
        del bits, mask, logits, wide, ob
    eng.close()


# ------------------------------------------------------------------------------------------------------ 4. every digest writer
def _toyctf_spec(E):
    """ToyCtf at 12 x 10 with its re-imaging defender, in which no env ever ends (no attacker goal, no eviction, no SLA, no step
    limit): stepping after an observation never resets an env, so the digest's discovery counts stay valid."""
    from marlon_amd._abi import RNG_PHILOX
    _, sj = parity.load_trace("toyctf_defender_s11")
    return parity.spec_from_json(sj, n_envs=E, auto_reset=False, rng_kind=RNG_PHILOX, seed=41, max_episode_steps=0, attacker_goal=None,
                                 maintain_sla=0.0, defender_goal_eviction=False)


@pytest.mark.parametrize("switch", ["MCBS_QUAD_OBS", "MCBS_NO_QUAD_OBS"])
def test_digest_of_observation_with_mask_fields(switch, monkeypatch):
    """observe() with mask fields through obs_quad_kernel (MCBS_QUAD_OBS=1) and obs_small_kernel (MCBS_NO_QUAD_OBS=1): mask_logits and
    pack equal the oracle mask of the observation, and so does the mask_discrete that same call wrote (into a sentinel-filled buffer)."""
    import torch
    from marlon_amd import engine
    from oracle.oracle import Oracle
    topo = parity.topology_for("toyctf_defender_s11")
    E = 515                                             # neither the last workgroup nor the last wavefront full
    spec = _toyctf_spec(E)
    monkeypatch.setenv(switch, "1")
    eng = engine.BatchEngine(topo, spec)
    monkeypatch.delenv(switch)
    orc = Oracle(topo, spec)
    A = eng.discrete_action_count()
    g = torch.Generator(device=eng.device).manual_seed(8)
    fields = parity.OBS_FIELDS
    blanks = 0
    for t in range(30):
        a = eng.sample_actions(t % 3 != 0, seed=12, step=t)
        if t % 4 == 1:
            a[::3, 1] = spec.maximum_node_count + 1     # out of bound: the blank observation
        _, term = eng.step(a)
        out = orc.step(a.cpu().numpy())
        assert not term.any() and out["errors"] == 0
        blanks += int(out["oob"].sum())
        if t % 3 != 2:
            continue
        o = eng.alloc_obs(fields + ["mask_discrete"])
        for v in o.values():
            v.fill_(5)
        eng.observe(o)
        oo = orc.observe(orc.alloc_obs(fields))
        mask = oracle_mask(oo, E)
        ctx = f"{switch} step {t}"
        np.testing.assert_array_equal(o["mask_discrete"].cpu().numpy() != 0, mask, err_msg=f"{ctx}: mask_discrete")
        assert set(np.unique(o["mask_discrete"].cpu().numpy())) <= {0, 1}
        _masked_logits_check(eng, mask, g, ctx)
        check_pack(eng, pack_host(mask), ctx)
    assert blanks > 0
    eng.close()


def test_digest_of_masked_reobservation_after_reset():
    """reset(mask) + observe(env_mask=mask) (obs_scan_kernel): the reset envs get the mask of their reset observation, the others keep
    the mask of their previous observation, for mask_logits and pack."""
    import torch
    from marlon_amd import engine
    from oracle.oracle import Oracle
    topo = parity.topology_for("toyctf_defender_s11")
    E = 300
    spec = _toyctf_spec(E)
    eng = engine.BatchEngine(topo, spec)
    orc = Oracle(topo, spec)
    g = torch.Generator(device=eng.device).manual_seed(9)
    small = ["scalars", "nodes_privilegelevel"]
    obs = eng.alloc_obs(small)
    for rnd in range(3):
        for t in range(6):
            a = eng.sample_actions(True, seed=20 + rnd, step=t)
            eng.step_observe(a, obs)
            oo = orc.alloc_obs(small + MASKS)
            out = orc.step(a.cpu().numpy(), obs=oo)
            assert out["errors"] == 0
        prev = oracle_mask(oo, E)
        keep = torch.zeros(E, dtype=torch.uint8, device=eng.device)
        keep[rnd::3] = 1
        keep[7 + rnd::11] = 1
        eng.reset(keep)
        eng.observe(obs, env_mask=keep)
        sel = keep.cpu().numpy() != 0
        for i in np.flatnonzero(sel):
            orc.reset(int(i))
        fresh = oracle_mask(orc.observe(orc.alloc_obs(small + MASKS), reset_obs=True), E)
        mask = np.where(sel[:, None], fresh, prev)
        assert (prev[~sel] != fresh[np.flatnonzero(sel)[0]]).any(axis=1).sum() > E // 4, "the untouched envs' masks look like reset ones"
        assert (prev[sel] != fresh[sel]).any(), "no reset env's mask changed"
        ctx = f"round {rnd}"
        m_dev, _ = _masked_logits_check(eng, mask, g, ctx)
        bits = check_pack(eng, pack_host(mask), ctx)
        got = eng.unpack_action_mask(bits)
        assert torch.equal(got[torch.as_tensor(sel, device=eng.device)], m_dev[torch.as_tensor(sel, device=eng.device)]), f"{ctx}: reset envs"
        assert torch.equal(got[torch.as_tensor(~sel, device=eng.device)], m_dev[torch.as_tensor(~sel, device=eng.device)]), f"{ctx}: untouched envs"
    eng.close()


def test_digest_survives_steps_without_observation():
    """Steps without an observation between observe() and the call (the defender re-imaging, no env ending): mask_logits and pack give
    the mask of the LAST OBSERVATION, not of the current state."""
    import torch
    from marlon_amd import engine
    from oracle.oracle import Oracle
    topo = parity.topology_for("toyctf_defender_s11")
    E = 256
    spec = _toyctf_spec(E)
    eng = engine.BatchEngine(topo, spec)
    orc = Oracle(topo, spec)
    g = torch.Generator(device=eng.device).manual_seed(10)
    small = ["scalars", "nodes_privilegelevel"]
    obs = eng.alloc_obs(small)
    changed = 0
    for rnd in range(4):
        for t in range(5):
            a = eng.sample_actions(True, seed=30 + rnd, step=t)
            eng.step_observe(a, obs)
            oo = orc.alloc_obs(small + MASKS)
            orc.step(a.cpu().numpy(), obs=oo)
        mask = oracle_mask(oo, E)
        for t in range(3):                              # no observation from here on
            a = eng.sample_actions(t != 1, seed=40 + rnd, step=t)
            _, term = eng.step(a)
            out = orc.step(a.cpu().numpy())
            assert not term.any() and not out["terminated"].any() and out["errors"] == 0
        now = orc.alloc_obs(MASKS)
        orc.observe(now)
        changed += int((oracle_mask(now, E) != mask).any(axis=1).sum())
        ctx = f"round {rnd}, three steps after the observation"
        _masked_logits_check(eng, mask, g, ctx)
        check_pack(eng, pack_host(mask), ctx)
    assert changed > 0, "no env's mask changed after its observation: the test would not notice a mask of the current state"
    eng.close()


def test_lean_wrapper_three_launch_step_masks():
    """AttackerVecEnv(materialize_masks=False) on ToyCtf at 11 x 25, where the one-launch step is refused (the step, the masked
    re-observation after auto-resets and the wrapper's bookkeeping are separate launches): at every step mask_logits and
    action_masks_packed equal the materialised action_masks() of the mask-writing wrapper (pinned to the reference's wrapper traces by
    tests/test_gpu_vecenv.py), auto-resets and intercepted actions included; for the first steps also the oracle's mask."""
    import torch
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.samples import toy_ctf
    from marlon_amd.wrappers import AttackerVecEnv
    from oracle.oracle import Oracle
    E = 512
    kw = dict(maximum_node_count=11, maximum_total_credentials=25, attacker_goal=ce.AttackerGoal(own_atleast_percent=1.0), max_timesteps=12,
              discrete=True)
    full = AttackerVecEnv(toy_ctf.new_environment(), E, **kw)
    lean = AttackerVecEnv(toy_ctf.new_environment(), E, materialize_masks=False, **kw)
    assert lean.engine.wrapper_step_launches(False) > 1 and full.engine.wrapper_step_launches(True) > 1
    orc = Oracle(lean.topo, lean.spec)
    orc.observe(orc.alloc_obs(MASKS), reset_obs=True)
    geom = (11, len(lean.topo.local_vulnerabilities), len(lean.topo.remote_vulnerabilities), len(lean.topo.ports), 25)
    W, _ = lean.engine.packed_mask_words()
    g = torch.Generator(device=full.engine.device).manual_seed(12)
    resets = 0
    for t in range(40):
        m = full.action_masks()
        if t < 8:                                       # no env has ended yet (max_timesteps 12): the oracle steps alongside
            oo = orc.alloc_obs(MASKS)
            orc.observe(oo)
            assert torch.equal(m.cpu(), torch.as_tensor(oracle_mask(oo, E))), f"step {t}: mask-writing wrapper vs oracle"
            assert bool(m.any(dim=1).all())             # the masked argmax below picks an allowed action in every env
        logits = _logits(E, m.shape[1], g, m.device)
        fill = -1e8 if t % 2 else float("-inf")
        run_variants(lambda v: lean.mask_logits(v, fill), logits, m, fill, f"step {t} lean mask_logits",
                     variants=VARIANTS if t % 5 == 0 else VARIANTS[:1] + VARIANTS[3:4])
        bits = lean.action_masks_packed()
        np.testing.assert_array_equal(bits.cpu().numpy().view(np.uint32)[:, :W], pack_host(m.cpu().numpy()), err_msg=f"step {t} packed")
        scores = torch.rand(m.shape, generator=g, device=m.device)
        actions = torch.where(m, scores, torch.full_like(scores, -1.0)).argmax(dim=1)
        if t % 6 == 3:
            actions[::5] = full.discrete_n - 1          # undiscovered: intercepted, the env keeps its last observation (and digest)
        if t < 8:
            rows = _decode_discrete(actions.cpu().numpy(), *geom)
            rows[actions.cpu().numpy() == full.discrete_n - 1] = (3, 0, 0, 0, 0)     # intercepted: MCBS_ACTION_SKIP, the env is not stepped
            assert orc.step(rows)["errors"] == 0
        _, _, te1, tr1, _ = full.step(actions)
        _, _, te2, tr2, _ = lean.step(actions)
        assert torch.equal(te1, te2) and torch.equal(tr1, tr2), f"step {t}"
        resets += int((te1 | tr1).sum())
    assert resets > 0
    full.close()
    lean.close()


# ------------------------------------------------------------------------------------------------------ 5. fills, 6. refusals
FILLS = [-1e8, _f32(0x3F808000), _f32(0x3F818000), -3.4028235e38, _f32(0x7F7F8000), float("inf"), float("-inf"), -0.0, 1e-40]


@pytest.fixture(scope="module")
def chain4_observed():
    from marlon_amd import engine
    from marlon_amd._abi import RNG_PHILOX
    from oracle.oracle import Oracle
    _, sj = parity.load_trace("chain4_defender_s21")
    topo = parity.topology_for("chain4_defender_s21")
    E = 64
    spec = parity.spec_from_json(sj, n_envs=E, auto_reset=True, rng_kind=RNG_PHILOX, seed=5, max_episode_steps=30)
    eng = engine.BatchEngine(topo, spec)
    orc = Oracle(topo, spec)
    obs = eng.alloc_obs(["scalars"])
    for t in range(6):
        a = eng.sample_actions(True, seed=2, step=t)
        oo = orc.alloc_obs(MASKS)
        eng.step_observe(a, obs)
        orc.step(a.cpu().numpy(), obs=oo)
    mask = oracle_mask(oo, E)
    assert mask.any() and not mask.all()
    yield eng, mask
    eng.close()


@pytest.mark.parametrize("fill", FILLS, ids=[repr(f) for f in FILLS])
def test_fill_rounding(fill, chain4_observed):
    """The stored fill: float32 bitwise (-0.0 and the subnormal included), bfloat16 == torch's round-to-nearest-even of the float32
    (ties both ways, overflow to +-inf), for mask_logits and apply_packed_mask through every launch variant."""
    import torch
    eng, mask_np = chain4_observed
    assert _fill_bits(_f32(0x3F808000), torch.bfloat16) == 0x3F80 and _fill_bits(_f32(0x3F818000), torch.bfloat16) == 0x3F82
    assert _fill_bits(-3.4028235e38, torch.bfloat16) == -0x80 and _fill_bits(_f32(0x7F7F8000), torch.bfloat16) == 0x7F80
    g = torch.Generator(device=eng.device).manual_seed(13)
    mask, logits = _masked_logits_check(eng, mask_np, g, f"fill {fill!r}", fill)
    bits = eng.pack_action_mask()
    run_variants(lambda v: eng.apply_packed_mask(bits, v, fill), logits, mask, fill, f"fill {fill!r} apply")


def test_nan_fill(chain4_observed):
    """A NaN fill: every replaced element is a NaN (the library keeps the sign, torch canonicalises), every allowed one unchanged."""
    import torch
    eng, mask_np = chain4_observed
    mask = torch.as_tensor(mask_np).to(eng.device)
    bits = eng.pack_action_mask()
    g = torch.Generator(device=eng.device).manual_seed(14)
    for fill in (float("nan"), -float("nan"), _f32(0x7FA00001)):
        for dt in (torch.float32, torch.bfloat16):
            src = _logits(eng.E, mask.shape[1], g, eng.device).to(dt)
            for name, call in (("mask_logits", lambda x: eng.mask_logits(x, fill)), ("apply", lambda x: eng.apply_packed_mask(bits, x, fill))):
                for off in (0, 1):
                    buf = torch.zeros((eng.E, mask.shape[1] + 8), dtype=dt, device=eng.device)
                    v = buf[:, off:off + mask.shape[1]]
                    v.copy_(src)
                    call(v)
                    iv = _iv(dt)
                    assert bool(torch.isnan(v[~mask]).all()), f"{name} {dt} offset {off} fill {fill!r}: replaced elements not NaN"
                    assert torch.equal(v.view(iv)[mask], src.view(iv)[mask]), f"{name} {dt} offset {off}: allowed elements changed"


def test_mask_logits_refusals(chain4_observed):
    """Refused with ValueError before any launch: a view narrower than A whose row stride is still >= A (the C side checks the stride
    only), float16 logits, logits whose elements are not contiguous.  The column past the narrow view is untouched."""
    import torch
    eng, _ = chain4_observed
    A = eng.discrete_action_count()
    for dt in (torch.float32, torch.bfloat16):
        wide = torch.full((eng.E, A + 4), 7.0, dtype=dt, device=eng.device)
        with pytest.raises(ValueError):
            eng.mask_logits(wide[:, :A - 1])
        torch.cuda.synchronize(eng.device)
        assert bool((wide == 7.0).all()), f"{dt}: written through a refused view"
    with pytest.raises(ValueError):
        eng.mask_logits(torch.zeros((eng.E, A), dtype=torch.float16, device=eng.device))
    with pytest.raises(ValueError):
        eng.mask_logits(torch.zeros((eng.E, 2 * A), device=eng.device)[:, ::2])
    eng.mask_logits(torch.zeros((eng.E, A), device=eng.device))       # and the well-formed call still passes
