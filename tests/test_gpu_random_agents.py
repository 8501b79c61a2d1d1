"""The random-agent sampler (sample_action: mcbs_sample_actions, and inside the step kernel mcbs_rollout_random) held to its law.

Every other GPU module draws its actions with BatchEngine.sample_actions and feeds the same rows to engine and oracle: that proves the
step and nothing about the sampler.  Here the sampler itself is the subject.

  1. law: all 65 536 envs of a batch are put into ONE state (oracle record, broadcast with set_state), K = 64 steps are drawn (4.2 M
     rows), and the histogram over the Discrete action indices is compared with tests/sampler_law.py (the reference's procedure in
     float64, tied to the reference by tests/test_sampler_law.py): not one row outside the support, Pearson chi-square below the
     1 - 1e-9 quantile, independence between consecutive steps and between neighbouring envs.  Before a draw is looked at the test
     asserts, from the law alone, that every merged bin expects >= 50 draws and that the kernel's 64 redraws cannot plausibly run out
     (E K (1 - Z)^64 < 1e-6).
  2. validity along trajectories: ExternalRandomEvents batches (which cannot be broadcast) and every case of tests/test_gpu_parity.py.
  3. keying: bitwise repeatability, every word of (seed, step, env_id_base) matters, shard invariance.
  4. rollouts: mcbs_rollout_random == sample + step == the oracle on the layouts test_gpu_parity does not reach, and
     simulate.run_random_agents for three chunk sizes.

Seeds are fixed, so the module is deterministic; the quantiles say how unlikely a false alarm was when the seeds were picked.
"""
import json
import os

import numpy as np
import pytest

from tests import parity, sampler_law as SL

pytestmark = pytest.mark.gpu

E_LAW = 65536
K_LAW = 64
MASKS = ["mask_local", "mask_remote", "mask_connect"]


def _engine():
    from marlon_amd import engine
    return engine


def _inside_space(geo, rows):
    """Per row (NumPy or torch [., 5]): every component inside the action space of the row's kind, unused components zero."""
    k, a, b, c, d = (rows[:, i] for i in range(5))
    nodes = (a >= 0) & (a < geo.N) & (b >= 0) & (c >= 0) & (d >= 0)
    loc = (k == 0) & (b < geo.L) & (c == 0) & (d == 0)
    rem = (k == 1) & (b < geo.N) & (c < geo.R) & (d == 0)
    con = (k == 2) & (b < geo.N) & (c < geo.P) & (d < geo.C)
    return nodes & (loc | rem | con)


def _assert_variant(eng, **want):
    v = eng.variant()
    got = {k: v[k] for k in want}
    assert got == want, f"batch dispatches to {v}, the test expects {want}"


# ------------------------------------------------------------------------------------------------------------------ states (CPU)
def _spec(topo, E, N=None, C=None, **over):
    from marlon_amd._abi import EnvSpec
    kw = dict(n_envs=E, maximum_node_count=N or topo.n_nodes, maximum_total_credentials=C or max(1, len(topo.triples)),
              attacker_goal=None, maximum_discoverable_credentials_per_action=max(32, int(topo.header()["max_leak_per_action"])))
    kw.update(over)
    return EnvSpec(**kw)


def _fixture_state(name):
    """A state of tests/golden/sampler_histograms.json — the very state the reference's histogram was drawn in — on the oracle."""
    with open(os.path.join(parity.GOLDEN, "sampler_histograms.json")) as f:
        rec = {s["name"]: s for s in json.load(f)["states"]}[name]
    topo = parity.topology_for(rec["topology"])
    orc = _oracle(topo, _spec(topo, 1, rec["spec"]["maximum_node_count"], rec["spec"]["maximum_total_credentials"]))
    for a in rec["script"]:
        assert not orc.step(np.asarray([a], np.int32))["oob"][0]
    return topo, orc


def _oracle(topo, spec):
    from oracle.oracle import Oracle
    return Oracle(topo, spec)


def _driven(topo, E, T, seed=3):
    """E oracle envs driven for T steps by tests/test_gpu_mask_geometry.host_policy (connects to nodes not owned yet first)."""
    from tests.test_gpu_mask_geometry import _decode_discrete, host_policy
    spec = _spec(topo, E)
    orc = _oracle(topo, spec)
    geom = (spec.maximum_node_count, len(topo.local_vulnerabilities), len(topo.remote_vulnerabilities), len(topo.ports),
            spec.maximum_total_credentials)
    small = ["scalars", "credential_cache_matrix", "nodes_privilegelevel", "mask_local", "mask_remote"]
    oo = orc.observe(orc.alloc_obs(small), reset_obs=True)
    rng = np.random.default_rng(seed)
    tried = [set() for _ in range(E)]
    for _ in range(T):
        rows = _decode_discrete(host_policy(oo, geom, rng, tried), *geom)
        oo = orc.alloc_obs(small)
        out = orc.step(rows, obs=oo)
        assert not out["terminated"].any() and out["errors"] == 0
    return orc


def _random24():
    """Random-24 with three start nodes: with its single one the attacker is stuck at 5 discovered nodes and 1 owned."""
    from marlon_amd import flatten as F, model
    from marlon_amd.samples import random_net
    return F.flatten(random_net.build(model, 24, 7, n_start=3))


def _owned_external(st):
    return [i for i, n in enumerate(st["order"]) if st["privilege"][n] >= 1]


def _deepest_env(orc):
    full = orc.get_state()
    deep = [max(_owned_external(SL.env_state(full, e))) for e in range(orc.E)]
    return int(np.argmax(deep))


# name: builder -> (topology, oracle, env of the oracle to take, engine spec overrides, env switches, expected variant, check(state))
def _state(name):
    from tests.test_gpu_mask_geometry import _large_topology
    none = dict(defender_kind=0)
    if name in ("chain10_reset", "toyctf_reset"):
        topo = parity.topology_for(name.split("_")[0])
        N, C = (12, 12) if name.startswith("chain10") else (12, 10)
        orc = _oracle(topo, _spec(topo, 1, N, C))
        return topo, orc, 0, {}, {}, dict(packed=1, words_per_set=1, wide=0, coop=0, **none), \
            lambda st: len(_owned_external(st)) == 1 and st["n_creds"] == 0
    if name in ("toyctf_mid", "chain4_mid"):
        topo, orc = _fixture_state(name)
        return topo, orc, 0, {}, {}, dict(packed=1, words_per_set=1, wide=0, coop=0, **none), \
            lambda st: len(_owned_external(st)) >= 3 and st["n_creds"] > 0 and (name == "chain4_mid" or
                                                                              _owned_external(st) != list(range(len(_owned_external(st)))))
    if name == "toyctf_reimaged":
        # the re-imaging ScanAndReimage performs (oracle actuator, defender.py:42-55 -> actions.py reimage_node) on the owned node at
        # external index 1 of the mid-episode state: discovered, no longer owned, in the middle of the discovery order
        topo, orc = _fixture_state("toyctf_mid")
        st = SL.env_state(orc.get_state())
        assert _owned_external(st)[:2] == [0, 1]
        orc.reimage_node(st["order"][1])
        return topo, orc, 0, dict(defender=("scan_and_reimage", 0.6, 2, 5), maintain_sla=0.5), {}, \
            dict(packed=1, words_per_set=1, wide=0, coop=0, defender_kind=1), \
            lambda st: 1 not in _owned_external(st) and _owned_external(st)[0] == 0 and max(_owned_external(st)) > 1 and st["n_discovered"] > 2
    if name == "random24":
        topo = _random24()
        orc = _driven(topo, 4, 80)
        return topo, orc, _deepest_env(orc), {}, {}, dict(packed=0, words_per_set=1, wide=0, coop=0, **none), \
            lambda st: len(_owned_external(st)) >= 3 and st["n_creds"] > 0
    if name in ("random100", "random100_coop"):
        topo = _large_topology("random100")
        orc = _driven(topo, 4, 180)
        coop = name.endswith("coop")
        return topo, orc, _deepest_env(orc), {}, {}, \
            dict(packed=0, words_per_set=2, wide=0, coop=int(coop), **none), lambda st: max(_owned_external(st)) >= 64
    if name == "random200":
        topo = _large_topology("random200")
        orc = _driven(topo, 3, 260)
        return topo, orc, _deepest_env(orc), {}, {}, dict(packed=0, words_per_set=4, wide=0, **none), \
            lambda st: max(_owned_external(st)) >= 128
    if name == "ad6":
        topo = parity.topology_for("ad6_mix_s70")
        orc = _driven(topo, 4, 40)
        return topo, orc, _deepest_env(orc), {}, {}, dict(packed=0, wide=1, **none), \
            lambda st: len(_owned_external(st)) >= 2 and st["n_creds"] > 0
    raise KeyError(name)


STATES = ["chain10_reset", "toyctf_reset", "chain4_mid", "toyctf_mid", "toyctf_reimaged", "random24", "random100", "random100_coop",
          "random200", "ad6"]
# the G-lanes-per-env step kernel takes batches of up to 32 768 envs: the coop batch draws twice as many steps from half as many envs
BATCH = {"random100_coop": (32768, 128)}


def _broadcast_engine(name, E=E_LAW, monkeypatch=None, **spec_over):
    """(engine with all E envs in the state, geometry, law)."""
    topo, orc, env, over, switches, variant, check = _state(name)
    full = orc.get_state()
    st = SL.env_state(full, env)
    assert check(st), f"{name}: the state is not what the case is for: {st}"
    geo = SL.Geometry(topo, orc.spec)
    law = SL.valid_law(topo, geo, st)
    obs = orc.observe(orc.alloc_obs(MASKS))                  # the helper's mask rule against the oracle's masks for this very state
    flat = np.concatenate([obs[f][env].reshape(-1) for f in ("mask_connect", "mask_local", "mask_remote")])
    np.testing.assert_array_equal(SL.mask_indices(topo, geo, st), np.flatnonzero(flat), err_msg=f"{name}: mask rule vs Oracle.observe")
    del obs, flat
    kw = dict(over)
    kw.update(spec_over)
    spec = _spec(topo, E, orc.spec.maximum_node_count, orc.spec.maximum_total_credentials, **kw)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    eng = _engine().BatchEngine(topo, spec)
    for k in switches:
        monkeypatch.delenv(k)
    _assert_variant(eng, **variant)
    eng.set_state(*(np.repeat(x[env:env + 1], E, axis=0) for x in full))
    return eng, geo, law


# ------------------------------------------------------------------------------------------------------------------ 1. the law
def _histogram(eng, geo, law, K, seed, first_step, ctx, keep_positions=False):
    """K draws per env -> (counts over the law's support, positions [K, E] or None); asserts that no row leaves the support."""
    t = eng.torch
    support = t.as_tensor(law["idx"], device=eng.device)
    S = len(support)
    counts = t.zeros(S, dtype=t.int64, device=eng.device)
    positions = []
    for k in range(K):
        rows = eng.sample_actions(True, seed=seed, step=first_step + k)
        idx = geo.encode(rows)
        pos = t.searchsorted(support, idx).clamp_(max=S - 1)
        inside = support[pos] == idx
        if not bool(inside.all()):
            bad = t.nonzero(~inside)[:, 0]
            raise AssertionError(f"{ctx} step {first_step + k}: {len(bad)} of {eng.E} valid=True rows are outside the law's support "
                                 f"(their mask bit is clear), first env {int(bad[0])}: {rows[bad[0]].tolist()}")
        counts += t.bincount(pos, minlength=S)
        if keep_positions:
            positions.append(pos)
    return counts.cpu().numpy(), (t.stack(positions).cpu().numpy() if keep_positions else None)


def _assert_preconditions(law, draws, ctx):
    """From the law alone, before any device draw is looked at."""
    assert abs(law["p"].sum() - 1.0) < 1e-12
    ex = SL.exhaustion_bound(law["Z"], draws)
    assert ex < 1e-6, f"{ctx}: Z = {law['Z']:.4f}: {ex:.3g} of {draws} draws expected to exhaust the 64 redraws — not a state for this test"
    e, _ = SL.merge_bins(law["p"] * draws, np.zeros(len(law["p"]), np.int64))
    assert e.min() >= SL.MIN_EXPECTED and len(e) >= 2, f"{ctx}: {len(e)} merged bins, the smallest expects {e.min():.1f}"


def _assert_fit(law, counts, ctx):
    stat, df, bound = SL.pearson(law["p"], counts)
    print(f"{ctx}: support {len(law['p'])}, Z {law['Z']:.4f}, {int(counts.sum())} draws, chi2 {stat:.1f} (df {df}, bound {bound:.1f})")
    assert stat < bound, f"{ctx}: chi2 {stat:.1f} >= {bound:.1f} (df {df}) over {int(counts.sum())} draws"


@pytest.mark.parametrize("name", STATES)
def test_valid_sampler_follows_the_law(name, monkeypatch):
    E, K = BATCH.get(name, (E_LAW, K_LAW))
    assert E * K >= 4_000_000
    eng, geo, law = _broadcast_engine(name, E=E, monkeypatch=monkeypatch)
    _assert_preconditions(law, E * K, name)
    counts, _ = _histogram(eng, geo, law, K, seed=20 + len(name), first_step=0, ctx=name)
    assert counts.sum() == E * K
    _assert_fit(law, counts, name)
    eng.close()


@pytest.mark.parametrize("name", ["chain10_reset", "toyctf_reset"])
def test_draws_are_independent_between_steps_and_between_envs(name):
    """Small support (fresh reset): pairs (env e at step s, same env at step s + 1) and (env e, env e + 1 at the same step), disjoint
    pairs, against the product of the law with itself."""
    eng, geo, law = _broadcast_engine(name)
    _assert_preconditions(law, E_LAW * K_LAW, name)
    _, pos = _histogram(eng, geo, law, K_LAW, seed=5, first_step=1000, ctx=name, keep_positions=True)
    for what, first, second in (("steps s, s+1", pos[0::2].reshape(-1), pos[1::2].reshape(-1)),
                                ("envs e, e+1", pos[:, 0::2].reshape(-1), pos[:, 1::2].reshape(-1))):
        stat, df, bound = SL.independence(law["p"], first, second)
        print(f"{name} {what}: {len(first)} pairs, chi2 {stat:.1f} (df {df}, bound {bound:.1f})")
        assert stat < bound, f"{name} {what}: contingency chi2 {stat:.1f} >= {bound:.1f} (df {df})"
    eng.close()


def _uniform_rows(eng, geo, K, seed):
    t = eng.torch
    out = []
    for k in range(K):
        rows = eng.sample_actions(False, seed=seed, step=k)
        assert bool(_inside_space(geo, rows).all()), f"valid=0 step {k}: a component outside the action space"
        out.append(rows.clone())
    return t.cat(out)


def test_uniform_sampler_every_bin_chain4():
    """valid=0 on Chain-4 at 6/6: uniform over kind, then over the DECLARED bounds (maximum_node_count, L, R, P,
    maximum_total_credentials) — every one of the 1 830 Discrete bins."""
    topo = parity.topology_for("chain4")
    eng = _engine().BatchEngine(topo, _spec(topo, E_LAW, 6, 6))
    geo = SL.Geometry(topo, eng.spec)
    p = SL.uniform_law(geo)
    assert p.min() * E_LAW * K_LAW >= SL.MIN_EXPECTED
    rows = _uniform_rows(eng, geo, K_LAW, seed=9)
    k = rows[:, 0]
    assert bool((rows[k == 0][:, 2] < geo.L).all() and (rows[k == 0][:, 3:] == 0).all())
    assert bool((rows[k == 1][:, 3] < geo.R).all() and (rows[k == 1][:, 4] == 0).all())
    assert bool((rows[k == 2][:, 3] < geo.P).all())
    counts = eng.torch.bincount(geo.encode(rows), minlength=geo.total).cpu().numpy()
    assert len(counts) == geo.total
    stat, df, bound = SL.pearson(p, counts)
    print(f"chain4 valid=0: chi2 {stat:.1f} (df {df}, bound {bound:.1f})")
    assert df == geo.total - 1 and stat < bound, f"chi2 {stat:.1f} >= {bound:.1f}"
    eng.close()


def test_uniform_sampler_marginals_chain10():
    """valid=0 on Chain-10 at 12/12: the kind, and given the kind every component's marginal, uniform over the declared bound."""
    topo = parity.topology_for("chain10")
    eng = _engine().BatchEngine(topo, _spec(topo, E_LAW, 12, 12))
    geo = SL.Geometry(topo, eng.spec)
    rows = _uniform_rows(eng, geo, K_LAW, seed=10).cpu().numpy()
    bounds = {0: (geo.N, geo.L, 1, 1), 1: (geo.N, geo.N, geo.R, 1), 2: (geo.N, geo.N, geo.P, geo.C)}
    checks = [("kind", rows[:, 0], 3)]
    for kind, bs in bounds.items():
        sel = rows[rows[:, 0] == kind]
        for j, b in enumerate(bs):
            if b == 1:
                assert (sel[:, 1 + j] == 0).all(), f"kind {kind}: unused component {1 + j} is not zero"
            else:
                checks.append((f"kind {kind} component {1 + j}", sel[:, 1 + j], b))
    for what, values, b in checks:
        counts = np.bincount(values, minlength=b)
        assert len(counts) == b, f"{what}: a value beyond the declared bound {b}"
        stat, df, bound = SL.pearson(np.full(b, 1.0 / b), counts)
        print(f"chain10 valid=0 {what}: chi2 {stat:.1f} (df {df}, bound {bound:.1f})")
        assert df == b - 1 and stat < bound, f"{what}: chi2 {stat:.1f} >= {bound:.1f} (df {df})"
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 2. validity along trajectories
def _allowed_by_oracle_masks(orc, rows, full_connect):
    """Per env: is the row's bit set in the masks Oracle.observe returns for the CURRENT state?  mask_connect is read directly where it
    is small; elsewhere its bit is (mask_remote[src, tgt, 0] and port < P and credential < cache length), which is how the reference
    fills the two in one loop iteration (cyberbattle_env.py:666-677)."""
    fields = ["scalars", "mask_local", "mask_remote"] + (["mask_connect"] if full_connect else [])
    oo = orc.observe(orc.alloc_obs(fields))
    e = np.arange(orc.E)
    k, a, b, c, d = (rows[:, i].astype(np.int64) for i in range(5))
    N, L = oo["mask_local"].shape[1:]
    R = oo["mask_remote"].shape[3]
    inb = (a >= 0) & (a < N) & (b >= 0) & (c >= 0) & (d >= 0)
    a0, b0 = np.where(inb, a, 0), np.where(inb & (b < N), b, 0)
    loc = inb & (b < L) & (oo["mask_local"][e, a0, np.where(b < L, b, 0) * inb] != 0)
    rem = inb & (b < N) & (c < R) & (oo["mask_remote"][e, a0, b0, np.where(c < R, c, 0) * inb] != 0)
    if full_connect:
        P, C = oo["mask_connect"].shape[3:]
        con = inb & (b < N) & (c < P) & (d < C) & (oo["mask_connect"][e, a0, b0, np.where(c < P, c, 0) * inb, np.where(d < C, d, 0) * inb] != 0)
    else:
        P = len(orc.topo.ports)
        con = inb & (b < N) & (oo["mask_remote"][e, a0, b0, 0] != 0) & (c < P) & (d < oo["scalars"][:, 5])
    return np.where(k == 0, loc, np.where(k == 1, rem, np.where(k == 2, con, False)))


def _validity_along(eng, orc, steps, seed, ctx):
    """Engine and oracle side by side on the sampler's own valid=True rows.  Every live env with an owned node: mask bit set.  An env
    without one (evicted attacker) has no valid action — the reference would raise: the row only has to be inside the action space.
    Every call is repeated once: same rows."""
    t = eng.torch
    geo = SL.Geometry(orc.topo, orc.spec)
    full_connect = orc.E * geo.connect_size <= 1 << 26
    checked = ownerless = 0
    for s in range(steps):
        a = eng.sample_actions(True, seed=seed, step=s)
        assert t.equal(a, eng.sample_actions(True, seed=seed, step=s)), f"{ctx} step {s}: a repeated call gave other rows"
        rows = a.cpu().numpy()
        hdr, nodes, _, _ = orc.get_state()
        has_owner = (nodes["privilege"] >= 1).any(axis=1)
        live = hdr["done"] == 0
        ok = _allowed_by_oracle_masks(orc, rows, full_connect)
        bad = np.flatnonzero(live & has_owner & ~ok)
        assert bad.size == 0, f"{ctx} step {s}: env {bad[0]} drew {rows[bad[0]].tolist()} under valid=True, its mask bit is clear ({bad.size} envs)"
        out = np.flatnonzero(~_inside_space(geo, rows))
        assert out.size == 0, f"{ctx} step {s}: env {out[0]} drew {rows[out[0]].tolist()}, outside the action-space bounds ({out.size} envs)"
        checked += int((live & has_owner).sum())
        ownerless += int((live & ~has_owner).sum())
        r, d = eng.step(a)
        o = orc.step(rows)
        np.testing.assert_array_equal(r.double().cpu().numpy(), o["reward"], err_msg=f"{ctx} step {s} reward")
        np.testing.assert_array_equal(d.cpu().numpy(), o["terminated"], err_msg=f"{ctx} step {s} terminated")
    return checked, ownerless


@pytest.mark.parametrize("name", ["toyctf", "random24"])
def test_valid_rows_under_random_events(name):
    """ExternalRandomEvents batches cannot be broadcast (set_state drops the overlay): 60 steps next to the oracle, validity only —
    mask_local is the env's own (keys patched away, library columns planted)."""
    from tests.test_gpu_defender_layouts import LAYOUTS, _ere_spec, _weighted_topology
    E, want = LAYOUTS[name]
    topo = _weighted_topology(name)
    spec = _ere_spec(topo, E)
    eng = _engine().BatchEngine(topo, spec)
    _assert_variant(eng, defender_kind=3, **want)
    checked, _ = _validity_along(eng, _oracle(topo, spec), 60, seed=41, ctx=f"random events {name}")
    assert checked > 50 * E
    eng.close()


def test_valid_rows_over_the_parity_cases():
    """The same per-step assertion over every case of tests/test_gpu_parity.py (its topologies, bounds, defenders), 256 envs each."""
    from marlon_amd._abi import RNG_PHILOX
    from tests.test_gpu_parity import CASES
    for case in sorted(CASES):
        trace, over, _, steps = CASES[case]
        _, sj = parity.load_trace(trace)
        topo = parity.topology_for(trace)
        spec = parity.spec_from_json(sj, n_envs=256, auto_reset=True, rng_kind=RNG_PHILOX, seed=0xBEEF + len(case), env_id_base=1000,
                                     max_episode_steps=150, **over)
        eng = _engine().BatchEngine(topo, spec)
        checked, ownerless = _validity_along(eng, _oracle(topo, spec), min(steps, 120), seed=43, ctx=case)
        print(f"{case}: {checked} rows checked, {ownerless} env-steps without an owned node")
        assert checked > 0
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ 3. keying
def test_every_word_of_the_key_matters():
    """Same (state, seed, step, env_id_base) -> same rows, bitwise.  Change any one 32-bit word of seed, step or env_id_base and the
    rows are a fresh draw: two independent draws from the law agree with probability sum(law^2), so the number of equal rows among E
    is Binomial(E, sum(law^2)); the bound is its 1 - 1e-9 quantile, not a guessed percentage."""
    seed, step = 0x1234_5678_9ABC_DEF1, 7
    eng, geo, law = _broadcast_engine("toyctf_mid", env_id_base=5)
    t = eng.torch
    p_equal = float((law["p"] ** 2).sum())
    limit = SL.agreement_bound(p_equal, E_LAW)
    assert limit < E_LAW // 20, f"sum(law^2) = {p_equal}: the state is too small to tell a fresh draw from a copy"
    base = eng.sample_actions(True, seed=seed, step=step).clone()
    assert t.equal(base, eng.sample_actions(True, seed=seed, step=step))
    others = {"seed low word": eng.sample_actions(True, seed=seed ^ 1, step=step).clone(),
              "seed high word": eng.sample_actions(True, seed=seed ^ (1 << 32), step=step).clone(),
              "step low word": eng.sample_actions(True, seed=seed, step=step + 1).clone(),
              "step high word": eng.sample_actions(True, seed=seed, step=step + (1 << 32)).clone()}
    eng.close()
    for what, base_id in (("env_id_base low word", 6), ("env_id_base high word", (1 << 32) + 5)):
        other, _, _ = _broadcast_engine("toyctf_mid", env_id_base=base_id)
        others[what] = other.sample_actions(True, seed=seed, step=step).clone()
        if what.endswith("high word"):                       # ... and the pooled law still holds up there, with steps beyond 2^32
            _assert_preconditions(law, E_LAW * K_LAW, what)
            counts, _ = _histogram(other, geo, law, K_LAW, seed=seed, first_step=(1 << 32) + 100, ctx="env_id_base 2^32+5, step 2^32+100")
            _assert_fit(law, counts, "env_id_base 2^32+5, step 2^32+100")
        other.close()
    for what, rows in others.items():
        same = int((rows == base).all(dim=1).sum())
        print(f"{what} changed: {same} of {E_LAW} rows equal (independent draws: {p_equal * E_LAW:.0f} expected, bound {limit})")
        assert same <= limit, f"{what} changed: {same} of {E_LAW} rows stayed equal, independent draws give at most {limit}"


def test_shard_invariance():
    """A batch with env_id_base 2048 and 1 024 envs draws rows [2048:3072] of a batch with base 0 and 4 096 envs in the same state."""
    whole, _, _ = _broadcast_engine("toyctf_mid", E=4096, env_id_base=0)
    shard, _, _ = _broadcast_engine("toyctf_mid", E=1024, env_id_base=2048)
    for valid in (True, False):
        for step in (0, 3, (1 << 32) + 9):
            a = whole.sample_actions(valid, seed=77, step=step)
            b = shard.sample_actions(valid, seed=77, step=step)
            assert whole.torch.equal(a[2048:3072], b), f"valid={valid} step {step}: the shard's rows differ from the whole batch's"
    whole.close()
    shard.close()


# ------------------------------------------------------------------------------------------------------------------ 4. rollouts
def _compare_states(a, b, ctx):
    for x, y, what in zip(a, b, ("header", "nodes", "order", "cache")):
        if x.dtype.names:
            for f in x.dtype.names:
                if not f.startswith("pad"):
                    np.testing.assert_array_equal(x[f], y[f], err_msg=f"{ctx}: state {what}.{f}")
        else:
            np.testing.assert_array_equal(x, y, err_msg=f"{ctx}: state {what}")


ROLLOUTS = {
    # name: (topology, spec overrides, env switches, expected variant)
    "random24": ("random24", dict(defender=("scan_and_reimage", 0.5, 3, 4), maintain_sla=0.3), {}, dict(packed=0, words_per_set=1, coop=0, defender_kind=1)),
    "random100_one_lane": ("random100", {}, {"MCBS_NO_COOP": "1"}, dict(packed=0, words_per_set=2, coop=0)),
    "random100_coop": ("random100", dict(defender=("scan_and_reimage", 0.5, 3, 2), maintain_sla=0.3), {}, dict(packed=0, words_per_set=2, coop=1)),
    "random200": ("random200", {}, {}, dict(packed=0, words_per_set=4)),
    "random24_random_events": ("random24", dict(defender=("random_events",)), {}, dict(packed=0, words_per_set=1, defender_kind=3)),
}


@pytest.mark.parametrize("valid", [True, False], ids=["valid", "uniform"])
@pytest.mark.parametrize("name", sorted(ROLLOUTS))
def test_rollout_random_equals_sample_then_step_and_the_oracle(name, valid, monkeypatch):
    """mcbs_rollout_random(record_actions) == mcbs_sample_actions + mcbs_step, step by step (actions, rewards, terminated, final state),
    and the recorded actions replayed through the oracle give the same rewards / terminated bitwise.  203 envs (a partial last
    wavefront), episodes truncate at 25 steps and auto-reset inside the launch."""
    from marlon_amd._abi import RNG_PHILOX
    from tests.test_gpu_mask_geometry import _large_topology
    tname, over, switches, variant = ROLLOUTS[name]
    topo = _random24() if tname == "random24" else _large_topology(tname)
    E, K = 203, 90
    spec = _spec(topo, E, attacker_goal=dict(own_atleast_percent=0.6), auto_reset=True, max_episode_steps=25, rng_kind=RNG_PHILOX, seed=99,
                 env_id_base=(1 << 32) + 1000, **over)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    one, fused = _engine().BatchEngine(topo, spec), _engine().BatchEngine(topo, spec)
    for k in switches:
        monkeypatch.delenv(k)
    _assert_variant(one, **variant)
    t = one.torch
    acts, rews, dones = [], [], []
    first = (1 << 32) - 40                                   # the step counter crosses 2^32 inside the launch
    for k in range(K):
        a = one.sample_actions(valid, seed=123, step=first + k)
        r, d = one.step(a, with_info=False)
        acts.append(a.clone()); rews.append(r.clone()); dones.append(d.clone())
    r2, d2, a2 = fused.rollout_random(K, valid=valid, seed=123, first_step=first, record_actions=True)
    assert t.equal(a2, t.stack(acts)), f"{name}: the rollout's recorded actions differ from mcbs_sample_actions"
    assert t.equal(r2, t.stack(rews)) and t.equal(d2, t.stack(dones)), f"{name}: rewards / terminated differ from mcbs_step"
    _compare_states(one.get_state(), fused.get_state(), name)
    orc = _oracle(topo, spec)
    an, rn, dn = a2.cpu().numpy(), r2.double().cpu().numpy(), d2.cpu().numpy()
    ended = 0
    for k in range(K):
        o = orc.step(an[k])
        np.testing.assert_array_equal(rn[k], o["reward"], err_msg=f"{name} step {k}: reward vs oracle")
        np.testing.assert_array_equal(dn[k], o["terminated"], err_msg=f"{name} step {k}: terminated vs oracle")
        if valid:
            assert not o["oob"].any(), f"{name} step {k}: a valid=True action took the out-of-bound path"
        ended += int(o["terminated"].sum()) + int(o["truncated"].sum())
    assert ended >= E, f"{name}: {ended} episode ends for {E} envs"
    _compare_states(fused.get_state(), orc.get_state(), name + " vs oracle")
    one.close()
    fused.close()


def test_run_random_agents_chunking_and_oracle():
    """simulate.run_random_agents: the same rewards / dones whatever the chunk size, equal to one mcbs_rollout_random launch; replayed
    through the oracle no valid=True step of a live env is an out-of-bound step."""
    from marlon_amd import simulate
    from marlon_amd._abi import RNG_PHILOX
    topo = parity.topology_for("toyctf")
    E, T = 512, 600
    spec = _spec(topo, E, 12, 10, attacker_goal=dict(own_atleast=6, own_atleast_percent=1.0), maintain_sla=0.8, defender=("scan_and_reimage", 0.6, 2, 5),
                 auto_reset=True, max_episode_steps=100, rng_kind=RNG_PHILOX, seed=4321, env_id_base=64)
    eng = _engine().BatchEngine(topo, spec)
    t = eng.torch
    runs = {}
    for chunk in (7, 256, 600):
        eng.rewind()
        out = simulate.run_random_agents(eng, T, seed=17, chunk=chunk)
        runs[chunk] = (out["rewards"].clone(), out["dones"].clone())
        assert runs[chunk][0].shape == (T, E) and runs[chunk][1].shape == (T, E)
    eng.rewind()
    r, d, a = eng.rollout_random(T, valid=True, seed=17, first_step=0, record_actions=True)
    for chunk, (rc, dc) in runs.items():
        assert t.equal(rc, r) and t.equal(dc, d), f"chunk {chunk}: rewards / dones differ from one launch of {T} steps"
    orc = _oracle(topo, spec)
    an, rn, dn = a.cpu().numpy(), r.double().cpu().numpy(), d.cpu().numpy()
    ended = 0
    for k in range(T):
        o = orc.step(an[k])
        ended += int(o["terminated"].sum()) + int(o["truncated"].sum())
        assert not o["oob"].any(), f"step {k}: env {int(np.flatnonzero(o['oob'])[0])} took the out-of-bound path with {an[k][np.flatnonzero(o['oob'])[0]].tolist()}"
        np.testing.assert_array_equal(rn[k], o["reward"], err_msg=f"step {k}: reward vs oracle")
        np.testing.assert_array_equal(dn[k], o["terminated"], err_msg=f"step {k}: dones vs oracle")
    assert ended >= 5 * E, f"{ended} episode ends for {E} envs in {T} steps of at most 100"
    _compare_states(eng.get_state(), orc.get_state(), "run_random_agents vs oracle")
    eng.close()
