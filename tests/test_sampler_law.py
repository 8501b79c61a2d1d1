"""The law helper (tests/sampler_law.py) against the reference itself, on the CPU.

tests/golden/sampler_histograms.json (oracle/refharness/gen_golden_sampler.py) holds, for four fixed states of the imported reference
env, the action script that reaches the state and the histogram of 400 000 sample_valid_action() draws taken there.  The script is
replayed through the CPU oracle, the law is computed from the oracle's canonical state, and the recorded counts must follow it:
no draw outside the support, Pearson chi-square below the 1 - 1e-9 quantile.  The GPU tests (tests/test_gpu_random_agents.py) hold the
device sampler to the same helper; this module is what ties the helper to the reference and not to a reading of it.
"""
import json
import os

import numpy as np
import pytest

from tests import parity, sampler_law as SL

with open(os.path.join(parity.GOLDEN, "sampler_histograms.json")) as _f:
    STATES = {s["name"]: s for s in json.load(_f)["states"]}


def _replayed(rec):
    from marlon_amd._abi import EnvSpec
    from oracle.oracle import Oracle
    topo = parity.topology_for(rec["topology"])
    spec = EnvSpec(n_envs=1, attacker_goal=dict(own_atleast_percent=1.0), auto_reset=False, **rec["spec"])
    orc = Oracle(topo, spec)
    for a in rec["script"]:
        o = orc.step(np.asarray([a], np.int32))
        assert not o["terminated"][0] and not o["oob"][0]
    return topo, spec, orc


def oracle_mask_indices(orc, e=0):
    """Discrete indices allowed by the masks Oracle.observe returns (connect | local | remote, action_masking.py:96-105)."""
    obs = orc.observe(orc.alloc_obs(["mask_local", "mask_remote", "mask_connect"]))
    flat = np.concatenate([obs["mask_connect"][e].reshape(-1), obs["mask_local"][e].reshape(-1), obs["mask_remote"][e].reshape(-1)])
    return np.flatnonzero(flat).astype(np.int64)


@pytest.mark.parametrize("name", sorted(STATES))
def test_reference_histogram_follows_the_law(name):
    rec = STATES[name]
    topo, spec, orc = _replayed(rec)
    geo = SL.Geometry(topo, spec)
    st = SL.env_state(orc.get_state())
    assert st["n_creds"] == rec["n_creds"] and sum(p >= 1 for p in st["privilege"]) == rec["owned"]
    np.testing.assert_array_equal(SL.mask_indices(topo, geo, st), oracle_mask_indices(orc), err_msg=f"{name}: mask rule vs Oracle.observe")
    law = SL.valid_law(topo, geo, st)
    n = rec["draws"]
    assert abs(law["p"].sum() - 1.0) < 1e-12 and law["p"].min() * n >= SL.MIN_EXPECTED, f"{name}: rarest action expects {law['p'].min() * n:.1f}"
    rows = np.asarray([c[:5] for c in rec["counts"]], np.int64)
    cnt = np.asarray([c[5] for c in rec["counts"]], np.int64)
    assert cnt.sum() == n
    idx = geo.encode(rows)
    pos = np.searchsorted(law["idx"], idx)
    inside = (pos < len(law["idx"])) & (law["idx"][np.minimum(pos, len(law["idx"]) - 1)] == idx)
    assert inside.all(), f"{name}: the reference drew actions outside the law's support: {rows[~inside][:5].tolist()}"
    observed = np.zeros(len(law["idx"]), np.int64)
    observed[pos] = cnt
    stat, df, bound = SL.pearson(law["p"], observed)
    print(f"{name}: support {len(law['idx'])}, Z {law['Z']:.4f}, chi2 {stat:.1f} (df {df}, bound {bound:.1f})")
    assert stat < bound, f"{name}: chi2 {stat:.1f} >= {bound:.1f} (df {df})"


def test_states_cover_two_and_three_kinds_and_non_contiguous_sources():
    """What the fixture is for: reset states draw two kinds from one source, mid-episode states three kinds from >= 3 sources."""
    for name, rec in STATES.items():
        kinds = {c[0] for c in rec["counts"]}
        sources = {c[1] for c in rec["counts"]}
        if name.endswith("_reset"):
            assert kinds == {0, 1} and sources == {0}, name
        else:
            assert kinds == {0, 1, 2} and len(sources) >= 3, name
    assert sorted({c[1] for c in STATES["toyctf_mid"]["counts"]}) != list(range(3))          # a hole in the owned external indices


def test_law_helper_statistics():
    """The statistics helpers on known cases: quantile (issue: df 278 -> 443.5 / 443.9), bin merging, a detectably wrong law."""
    assert abs(SL.chi2_quantile(278) - 443.5) < 0.6
    e, o = SL.merge_bins(np.array([30.0, 30.0, 10.0, 60.0, 5.0]), np.array([1, 2, 3, 4, 5]))
    assert e.tolist() == [60.0, 75.0] and o.tolist() == [3.0, 12.0]
    rng = np.random.Generator(np.random.PCG64(5))
    p = np.full(279, 1.0 / 279)
    good = rng.multinomial(4_000_000, p)
    stat, df, bound = SL.pearson(p, good)
    assert df == 278 and stat < bound
    q = p.copy()
    q[:93] *= 1.02                                            # 2 % excess weight on one of three sources' bins
    q /= q.sum()
    stat, _, bound = SL.pearson(p, rng.multinomial(4_000_000, q))
    assert stat > bound
    first, second = rng.choice(20, 400_000, p=np.full(20, 0.05)), rng.choice(20, 400_000, p=np.full(20, 0.05))
    stat, df, bound = SL.independence(np.full(20, 0.05), first, second)
    assert stat < bound
    stat, _, bound = SL.independence(np.full(20, 0.05), first, np.where(rng.random(400_000) < 0.02, first, second))
    assert stat > bound
    assert SL.agreement_bound(0.1, 65536) > 6554 and SL.agreement_bound(0.1, 65536) < 7200
    assert SL.exhaustion_bound(1.0 / 3.0, 4_000_000) < 1e-4


def test_uniform_law_and_decode_roundtrip():
    from marlon_amd._abi import EnvSpec
    topo = parity.topology_for("chain4")
    geo = SL.Geometry(topo, EnvSpec(maximum_node_count=6, maximum_total_credentials=6))
    p = SL.uniform_law(geo)
    assert abs(p.sum() - 1.0) < 1e-12
    rows = np.asarray([geo.decode(i) for i in range(geo.total)], np.int64)
    np.testing.assert_array_equal(geo.encode(rows), np.arange(geo.total))
    for k, size in ((2, geo.connect_size), (0, geo.local_size), (1, geo.remote_size)):
        assert abs(p[rows[:, 0] == k].sum() - 1.0 / 3.0) < 1e-12 and (rows[:, 0] == k).sum() == size
