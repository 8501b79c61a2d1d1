"""marlon_amd/features.py on the host: the layout of the policy's one-hot input row (widths, segment offsets, descriptors) against the
class counts of the reference's spaces computed here independently, and `encode_host` against a restatement written with
torch.nn.functional.one_hot per element and torch.cat on observations the CPU oracle produced."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from marlon_amd import flatten
from marlon_amd._abi import EnvSpec
from marlon_amd.features import FeatureLayout
from marlon_amd.samples import chainpattern, toy_ctf

SCALARS = ["newly_discovered_nodes_count", "lateral_move", "customer_data_found", "probe_result", "escalation",
           "credential_cache_length", "discovered_node_count"]
ARRAYS = ["leaked_credentials", "credential_cache_matrix", "discovered_nodes_properties", "nodes_privilegelevel"]
MASKS = ["connect", "local_vulnerability", "remote_vulnerability"]


def key_classes(N, C, K, L, R, P, NP, reference_counts):
    """key -> class count of every element, in element order (cyberbattle_env.py:262-320); a mask key -> its number of 0 / 1 values."""
    return {
        "newly_discovered_nodes_count": [N + 1], "lateral_move": [2], "customer_data_found": [2], "probe_result": [3], "escalation": [4],
        "credential_cache_length": [C if reference_counts else C + 1], "discovered_node_count": [N if reference_counts else N + 1],
        "leaked_credentials": [2, C, N, P] * K, "credential_cache_matrix": [N, P] * C, "discovered_nodes_properties": [3] * (N * NP),
        "nodes_privilegelevel": [4] * N,
    }, {"connect": N * N * P * C, "local_vulnerability": N * L, "remote_vulnerability": N * N * R}


def restate(obs, classes, mask_sizes, keys):
    """The SB3-style encoding with torch on CPU tensors: per key, per element, one_hot of the element's class count; masks as floats; cat.
    An element outside [0, classes) becomes an all-zero group and is counted.  -> (float32 [n, F], count)"""
    n = len(obs["nodes_privilegelevel"])
    parts, bad = [], 0
    for k in keys:
        if k in mask_sizes:
            parts.append((torch.as_tensor(np.asarray(obs[k])).reshape(n, mask_sizes[k]) != 0).float())
            continue
        v = torch.as_tensor(np.asarray(obs[k])).reshape(n, -1).long()
        assert v.shape[1] == len(classes[k]), k
        for col, ncls in zip(v.split(1, dim=1), classes[k]):
            col = col.reshape(n)
            ok = (col >= 0) & (col < ncls)
            bad += int((~ok).sum())
            parts.append(TF.one_hot(torch.where(ok, col, torch.zeros_like(col)), ncls).float() * ok.unsqueeze(1))
    return torch.cat(parts, dim=1), bad


def public_obs(oo):
    """the oracle's fields as the wrapper's observation keys"""
    E = oo["scalars"].shape[0]
    out = {k: oo["scalars"][:, i] for i, k in enumerate(SCALARS)}
    out.update({k: oo[k].reshape(E, -1) for k in ARRAYS})
    if "mask_connect" in oo:
        out.update(connect=oo["mask_connect"].reshape(E, -1), local_vulnerability=oo["mask_local"].reshape(E, -1),
                   remote_vulnerability=oo["mask_remote"].reshape(E, -1))
    return out


def valid_rows(oo, rng):
    """one uniformly random valid engine action row [kind, a, b, c, d] per env from the oracle's masks (every env has one: a local
    vulnerability of the first owned node at least, or any allowed entry)"""
    E = oo["mask_local"].shape[0]
    rows = np.zeros((E, 5), np.int32)
    for e in range(E):
        loc, rem, con = (np.argwhere(oo[f][e] != 0) for f in ("mask_local", "mask_remote", "mask_connect"))
        i = int(rng.integers(len(loc) + len(rem) + len(con)))
        if i < len(loc):
            rows[e, :3] = [0, *loc[i]]
        elif i < len(loc) + len(rem):
            rows[e, :4] = [1, *rem[i - len(loc)]]
        else:
            rows[e] = [2, *con[i - len(loc) - len(rem)]]
    return rows


def stepped_observation(env, N, C, steps, E=8, seed=3):
    from oracle.oracle import Oracle
    topo = flatten.flatten(env)
    spec = EnvSpec(n_envs=E, maximum_node_count=N, maximum_total_credentials=C)
    orc = Oracle(topo, spec)
    rng = np.random.default_rng(seed)
    oo = orc.observe(orc.alloc_obs(), reset_obs=True)
    for _ in range(steps):
        rows = valid_rows(oo, rng)
        oo = orc.alloc_obs()
        out = orc.step(rows, obs=oo)
        assert out["errors"] == 0
        if out["terminated"].any():
            break
    return topo, spec, oo


def dims(topo, spec):
    return (spec.maximum_node_count, spec.maximum_total_credentials, spec.maximum_discoverable_credentials_per_action,
            len(topo.local_vulnerabilities), len(topo.remote_vulnerabilities), len(topo.ports), len(topo.properties))


def test_chain10_and_toyctf_widths():
    topo = flatten.flatten(chainpattern.new_environment(10))
    spec = EnvSpec(n_envs=1, maximum_node_count=12, maximum_total_credentials=12)
    assert dims(topo, spec) == (12, 12, 5, 5, 2, 8, 14)
    assert FeatureLayout(topo, spec, reference_counts=True).width == 1010
    assert FeatureLayout(topo, spec).width == 1012
    assert FeatureLayout(topo, spec, include_masks=True).width == 1012 + 14172
    assert FeatureLayout(topo, spec, include_masks=True, reference_counts=True).width == 1010 + 14172
    lay = FeatureLayout(topo, spec)
    assert lay.n_elements == 7 + 20 + 24 + 168 + 12 and lay.values_per_row * 4 == 924
    assert lay.padded_width(4) == 1024 and lay.padded_width(2) == 1024 and FeatureLayout(topo, spec, reference_counts=True).padded_width(2) == 1024
    toy = flatten.flatten(toy_ctf.new_environment())
    tspec = EnvSpec(n_envs=1, maximum_node_count=12, maximum_total_credentials=10)
    N, C, K, L, R, P, NP = dims(toy, tspec)
    want = (N + 1) + 2 + 2 + 3 + 4 + (C + 1) + (N + 1) + K * (2 + C + N + P) + C * (N + P) + 3 * N * NP + 4 * N
    assert FeatureLayout(toy, tspec).width == want and FeatureLayout(toy, tspec, reference_counts=True).width == want - 2
    assert FeatureLayout(toy, tspec, include_masks=True).width == want + N * N * P * C + N * L + N * N * R


@pytest.mark.parametrize("env_name,N,C,K", [("chain10", 12, 12, 5), ("toyctf", 12, 10, 5), ("chain4", 6, 5, 3), ("chain4", 9, 7, 1),
                                            ("toyctf", 13, 15, 8), ("toyctf", 10, 40, 2)])
@pytest.mark.parametrize("include_masks", [False, True])
@pytest.mark.parametrize("reference_counts", [False, True])
def test_segments_and_descriptors(env_name, N, C, K, include_masks, reference_counts):
    env = {"chain10": lambda: chainpattern.new_environment(10), "chain4": lambda: chainpattern.new_environment(4),
           "toyctf": toy_ctf.new_environment}[env_name]()
    topo = flatten.flatten(env)
    spec = EnvSpec(n_envs=1, maximum_node_count=N, maximum_total_credentials=C, maximum_discoverable_credentials_per_action=K)
    classes, mask_sizes = key_classes(*dims(topo, spec), reference_counts)
    lay = FeatureLayout(topo, spec, include_masks=include_masks, reference_counts=reference_counts)
    keys = sorted(list(classes) + (MASKS if include_masks else []))
    assert lay.keys == keys
    col = 0
    for k in keys:
        w = mask_sizes[k] if k in mask_sizes else sum(classes[k])
        assert lay.segments[k] == (col, w), k
        col += w
    assert lay.width == col
    # the descriptors: one per one-hot column, classes 0 .. n-1 of one source value, the first flagged; sources name the row's values
    d = lay.descriptors
    assert d.dtype == np.uint32 and len(d) == col - (sum(mask_sizes.values()) if include_masks else 0)
    first, cls, src = d >> 31, d & 0xFFFF, (d >> 16) & 0x7FFF
    widths = [n for k in keys if k in classes for n in classes[k]]
    starts = np.cumsum([0] + widths[:-1])
    assert int(first.sum()) == len(widths) == lay.n_elements and (np.flatnonzero(first) == starts).all()
    for s, n in zip(starts, widths):
        assert (cls[s:s + n] == np.arange(n)).all() and (src[s:s + n] == src[s]).all()
    assert sorted(src[starts].tolist()) == list(range(lay.values_per_row))      # every value of the row is the source of exactly one element
    # mask ranges: (first column, columns, first bit) in connect | local | remote bit order
    M, ML = mask_sizes["connect"], mask_sizes["local_vulnerability"]
    want = [(lay.segments[k][0], mask_sizes[k], b0) for k, b0 in (("connect", 0), ("local_vulnerability", M), ("remote_vulnerability", M + ML))] if include_masks else []
    assert sorted(map(tuple, lay.mask_ranges.tolist())) == sorted(want)


def test_key_order_and_subsets():
    topo = flatten.flatten(chainpattern.new_environment(4))
    spec = EnvSpec(n_envs=1, maximum_node_count=6, maximum_total_credentials=5)
    lay = FeatureLayout(topo, spec, keys=["nodes_privilegelevel", "escalation", "connect"], include_masks=True)
    N, C, K, L, R, P, NP = dims(topo, spec)
    assert lay.segments == {"nodes_privilegelevel": (0, 4 * N), "escalation": (4 * N, 4), "connect": (4 * N + 4, N * N * P * C)}
    assert lay.width == 4 * N + 4 + N * N * P * C and lay.mask_ranges.tolist() == [[4 * N + 4, N * N * P * C, 0]]
    with pytest.raises(ValueError, match="include_masks"):
        FeatureLayout(topo, spec, keys=["connect"])
    with pytest.raises(ValueError, match="unknown"):
        FeatureLayout(topo, spec, keys=["nodes"])
    with pytest.raises(ValueError, match="twice"):
        FeatureLayout(topo, spec, keys=["escalation", "escalation"])


@pytest.mark.parametrize("env_name,N,C,steps", [("chain10", 12, 12, 60), ("toyctf", 12, 10, 60)])
def test_encode_host_equals_one_hot_restatement(env_name, N, C, steps):
    env = chainpattern.new_environment(10) if env_name == "chain10" else toy_ctf.new_environment()
    topo, spec, oo = stepped_observation(env, N, C, steps)
    obs = public_obs(oo)
    assert obs["discovered_node_count"].max() > 1 and (oo["nodes_privilegelevel"] > 0).any()       # the run left the reset state
    classes, mask_sizes = key_classes(*dims(topo, spec), False)
    for include_masks in (False, True):
        keys = sorted(list(classes) + (MASKS if include_masks else []))
        lay = FeatureLayout(topo, spec, include_masks=include_masks)
        want, bad = restate(obs, classes, mask_sizes, keys)
        got, got_bad = lay.encode_host(obs, return_out_of_range=True)
        assert bad == 0 and got_bad == 0
        assert got.dtype == np.float32 and got.shape == tuple(want.shape) and np.array_equal(got, want.numpy())
        # the engine's field dict (scalars [n, 7], arrays in their own shapes) encodes the same
        fields = {k: oo[k] for k in ["scalars"] + ARRAYS}
        fields.update({k: obs[k] for k in MASKS if include_masks})
        assert np.array_equal(lay.encode_host(fields), got)
    # a caller-given order, keys left out
    keys = ["nodes_privilegelevel", "remote_vulnerability", "credential_cache_matrix", "discovered_node_count", "connect", "leaked_credentials"]
    lay = FeatureLayout(topo, spec, keys=keys, include_masks=True)
    want, _ = restate(obs, classes, mask_sizes, keys)
    assert np.array_equal(lay.encode_host(obs), want.numpy())
    assert np.array_equal(lay.encode_host(obs, dtype=np.float16), want.numpy().astype(np.float16))


def test_out_of_range_values_leave_their_group_zero():
    topo, spec, oo = stepped_observation(chainpattern.new_environment(10), 12, 12, 40, E=4)
    N = 12
    obs = {k: np.array(v) for k, v in public_obs(oo).items()}
    obs["discovered_node_count"][0] = N                      # the full count: class N of N + 1, beyond Discrete(N)
    obs["nodes_privilegelevel"][1, 3] = -1                   # negative
    obs["credential_cache_matrix"][2, 5] = 1000              # too large (port index of credential 2)
    obs["leaked_credentials"][3, 1] = 12                     # cache index C of Discrete(C)
    for reference_counts, bad_want in ((True, 4), (False, 3)):
        classes, mask_sizes = key_classes(*dims(topo, spec), reference_counts)
        lay = FeatureLayout(topo, spec, reference_counts=reference_counts)
        want, bad = restate(obs, classes, mask_sizes, sorted(classes))
        got, got_bad = lay.encode_host(obs, return_out_of_range=True)
        assert bad == bad_want == got_bad
        assert np.array_equal(got, want.numpy())
        c0, w = lay.segments["discovered_node_count"]
        assert w == (N if reference_counts else N + 1)
        assert got[0, c0:c0 + w].sum() == (0 if reference_counts else 1) and (reference_counts or got[0, c0 + N] == 1)
        assert (got[1:, c0:c0 + w].sum(axis=1) == 1).all()
        p0, _ = lay.segments["nodes_privilegelevel"]
        assert not got[1, p0 + 12:p0 + 16].any() and got[1, p0 + 8:p0 + 12].sum() == 1 and got[1, p0 + 16:p0 + 20].sum() == 1     # neighbours intact
        m0, _ = lay.segments["credential_cache_matrix"]
        g = m0 + 2 * (N + 8) + N                              # credential 2's port group (elements of N and P = 8 classes)
        assert not got[2, g:g + 8].any() and got[2, g - N:g].sum() == 1 and got[2, g + 8:g + 8 + N].sum() == 1
        # every other element of every row is a proper one-hot: ones = elements - bad
        assert int(got.sum()) == 4 * lay.n_elements - bad_want


def test_header_and_exports_name_the_encoder():
    import os
    import re
    from marlon_amd import engine
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mcbs.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mcbs_[a-z_]+)\s*\(", text))
    for name in ("mcbs_feature_layout_create", "mcbs_feature_layout_destroy", "mcbs_feature_layout_width", "mcbs_encode_features"):
        assert name in declared and name in engine.EXPORTS
    lib = engine.load_library()
    assert lib.mcbs_feature_layout_create(None, None, 0, None, 0, None) == -1 and b"null" in lib.mcbs_last_error()
    assert lib.mcbs_encode_features(None, None, None, None, 0, None, 0, 0, 0, None, None) == -1
    assert lib.mcbs_feature_layout_width(None) == 0
    lib.mcbs_feature_layout_destroy(None)
