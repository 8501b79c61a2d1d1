"""The non-vacuity conditions of tests/test_gpu_capacity_limits.py, asserted on the CPU oracle alone: the scripts of tests/capacity.py
REACH the bit positions and thresholds the GPU tests are there for.  A condition that fails means the script must be lengthened or
steered, never that the assertion goes.  Also here: the two refusals at the limits (the oracle's, for ExternalRandomEvents on a
topology without its tables, and flatten's, one vulnerability column past the format's bound)."""
import numpy as np
import pytest

from tests import capacity


def _counts(name):
    return capacity.header_counts(capacity.reference(name).topo)


def test_row_limits_topology_sits_on_the_limits():
    from marlon_amd import flatten as F
    h = _counts("limits:67")
    assert (h["n_ports"], h["n_props"], h["n_local"], h["max_slots"]) == (F.MAX_PORTS, F.MAX_PROPS, F.MAX_LOCAL, F.MAX_SLOTS) == (32, 60, 32, 32)
    topo = capacity.reference("limits:67").topo
    nt = topo.node_table()
    assert (nt["n_slots"] == 32).all() and (nt["listen"] == 0x80000001).all()
    assert [hex(int(x)) for x in nt["fw_in_allow"]] == ["0xffffffff", "0xffffffff", "0x7fffffff", "0xffffffff", "0xffffffff", "0xffffffff"]
    assert (nt["local_mask"][0::2] == 0x3FFFFFFF).all() and (nt["local_mask"][1::2] == 0xFFFFFFFC).all()
    assert [int(x >> np.uint64(59)) for x in nt["props"]] == [1, 1, 1, 0, 1, 1], "every node but node 3 owns property 59"
    assert capacity.expected_variant(topo, capacity.reference("limits:67").spec) == dict(packed=0, words_per_set=1, wide=0)


@pytest.mark.parametrize("name", ["limits:67", "limits:67:scan", "limits:130", "limits:67:external"])
def test_row_limits_script_reaches_every_edge(name):
    ref = capacity.reference(name)
    seen = ref.seen
    assert ref.errors == 0
    assert seen["ever31"] and seen["since31"], "bit 31 of attacked_ever / attacked_since (vulnerability slot 31)"
    assert seen["top_prop_with_tags"], "discovered_props bit 59 on a node whose tags are non-zero"
    assert seen["local_last_positive"] and seen["remote_last_positive"], "local id 31 / remote id R - 1 exploited with a positive reward"
    assert seen["precondition_failed"] and seen["precondition_held"], "the precondition on property 59, failing (node 3) and holding"
    assert seen["connect_last_port_ok"] and seen["connect_last_port_blocked"], "a connect through port 31: one succeeds, one the firewall blocks"
    if ":scan" in name or ":external" in name:
        assert seen["since31_cleared"], "bit 31 of attacked_since cleared again by a re-image"
    ended = (ref.out["terminated"] != 0) | (ref.out["truncated"] != 0)
    assert ended.any(axis=0).all(), "every env ends (and is reset) at least once"
    if ":external" in name:
        status = [o[k].reshape(67, 6, 6) for o in ref.defender["obs"] for k in ("outgoing_firewall_status",)]
        assert any((x[:, :, 5] == 0).any() for x in status) and any((x[:, :, 0] == 0).any() for x in status), \
            "the learned defender blocks the managed rule of port 31 (sudo) and of port 0 (RDP)"


@pytest.mark.parametrize("name", ["limits:1", "limits:67:ere", "limits:67:R40", "limits:67:R223", "limits:33:n66", "limits:67:n66:scan",
                                  "limits:33:n130:scan", "limits:67:n130"])
def test_row_limits_variants_reach_bit_31(name):
    ref = capacity.reference(name)
    seen, h = ref.seen, capacity.header_counts(ref.topo)
    assert ref.errors == 0 and seen["ever31"] and seen["since31"] and seen["top_prop_with_tags"] and seen["connect_last_port_ok"]
    assert seen["remote_last_positive"], f"remote id {h['n_remote'] - 1} exploited with a positive reward"
    if ":ere" in name:
        assert h["n_local"] + h["n_remote"] == 64 and h["off_ere"], "column 63 of the presence masks"
    if ":R" in name:
        assert not h["off_ere"] and h["n_remote"] == int(name.split(":R")[1])
    if ":n" in name:
        want = dict(packed=0, words_per_set=2 if ":n66" in name else 4, wide=0)
        assert capacity.expected_variant(ref.topo, ref.spec) == want, "two / four words per set, narrow triples: the cooperative kernel's batch"
        assert seen["max_node_discovered"] == h["n_nodes"] - 1, "the node with the highest bit of the node sets is discovered"


@pytest.mark.parametrize("edge", capacity.PACKED_EDGES)
def test_packed_edge_layouts(edge):
    """eng.variant()'s expectation, recomputed from the header: row widths of 32 bits pack, 33 and 34 do not."""
    p, s = edge
    for E in (1, 65, 130):
        ref = capacity.reference(f"packed:{p}x{s}:{E}")
        h = capacity.header_counts(ref.topo)
        assert (h["n_props"], h["max_slots"], h["n_nodes"]) == (p, s, 16) and h["n_triples"] <= 15 and h["n_cred_strings"] <= 16
        assert capacity.expected_variant(ref.topo, ref.spec)["packed"] == int(p + 4 + 2 * s <= 32)
        assert p + 4 + 2 * s in (32, 33, 34)
        assert ref.errors == 0 and ref.seen["positive"] > 0
        assert (ref.final[0]["episode"] >= 4).all(), "every env is reset inside the kernel several times"
    ref = capacity.reference(f"packed:{p}x{s}:130")
    nodes = np.concatenate([st[1] for st in ref.states.values()])
    top_slot = np.uint32(1 << (s - 1))
    assert (nodes["attacked_ever"] & top_slot).any() and (nodes["attacked_since"] & top_slot).any(), f"slot {s - 1}: the top bit of both slot fields"
    assert ((nodes["discovered_props"] >> np.uint64(p - 1)) & np.uint64(1)).any() or s == 1, f"property {p - 1}: the bit below the tags"
    assert (nodes["tags"] != 0).any() or s == 1


@pytest.mark.parametrize("name", ["creds:256", "creds:257", "creds:1024", "creds:257:scan", "creds:1024:scan"])
def test_credential_limits_script(name):
    ref = capacity.reference(name)
    nt = int(name.split(":")[1])
    h, seen = capacity.header_counts(ref.topo), ref.seen
    assert (h["n_triples"], h["n_cred_strings"], h["n_ports"]) == (nt, 256, 32)
    assert capacity.expected_variant(ref.topo, ref.spec) == dict(packed=0, words_per_set=4, wide=int(nt > 256)), "TW = 4 / 5 / 16"
    assert ref.errors == 0
    assert seen["top_string"] == 255, "credential string 255 gathered"
    assert seen["last_triple_cached"] and seen["last_triple_used"], f"triple {nt - 1} cached and a connect through it succeeds"
    assert seen["max_creds"] == nt == ref.spec.maximum_total_credentials, "n_creds reaches maximum_total_credentials"
    assert seen["last_cache_position_used"], f"a connect with credential index {nt - 1}"
    if nt != 257:        # (triple 256 sits on port (256 // 8) % 32 = 0 and the prefix connects through the last triple and the last cache
        #                   position only: at 257 triples no scripted connect goes through port 31)
        assert seen["connect_last_port_ok"], "a connect through port 31 succeeds"
    if nt == 1024:
        assert h["max_leak_per_action"] == 1023 and seen["max_new_creds"] == 1023, "one step adds 1 023 credentials"
    ended = (ref.out["terminated"] != 0) | (ref.out["truncated"] != 0)
    assert ended.any(), "an env with a full cache is reset"


@pytest.mark.parametrize("bounds", capacity.BOUNDS)
def test_observation_bounds_straddle_the_row_thresholds(bounds):
    """RL = P * Cmax on each side of RL / 16 <= 64, RL / gcd(RL, 16) <= 64 and RL + 4 <= 1040 (launch_obs_inner)."""
    P, C_ = bounds
    RL = P * C_
    assert RL in (512, 1024, 1056, 1036, 1040, 1064, 504, 520)
    for nmax in (8, 16):
        ref = capacity.reference(f"bounds:{P}x{C_}:{nmax}")
        assert capacity.header_counts(ref.topo)["n_ports"] == P and ref.spec.maximum_total_credentials == C_ and ref.errors == 0
        assert any(o["mask_connect"].any() for o in ref.obs.values()) and len(ref.obs) >= 8
        assert any((o["mask_connect"].reshape(35, -1, P, C_)[:, :, P - 1, :].any()) for o in ref.obs.values()), "the row's last port is on somewhere"


def test_oracle_refuses_random_events_without_tables():
    """More than 64 vulnerability columns: flatten writes no ExternalRandomEvents tables, mcbs_batch_create refuses that defender with
    MCBS_EINVAL, and the oracle must raise the same message instead of reading tables that are not there (it used to crash)."""
    from marlon_amd._abi import EnvSpec
    from oracle.oracle import Oracle
    topo = capacity.topology("limits", 6, 32, 33)
    h = capacity.header_counts(topo)
    assert h["n_local"] + h["n_remote"] == 65 and h["off_ere"] == 0
    spec = EnvSpec(n_envs=3, maximum_node_count=8, maximum_total_credentials=16, defender=("random_events",))
    with pytest.raises(ValueError, match=r"the topology blob carries no ExternalRandomEvents tables \(off_ere\)"):
        Oracle(topo, spec)
    import ctypes as C
    from oracle import oracle as om
    blob = np.frombuffer(topo.blob, dtype=np.uint8).copy()
    cfg = spec.to_cfg()
    assert not om._load().cbo_create(blob.ctypes.data, blob.size, C.byref(cfg)), "the C entry point refuses too"
    Oracle(topo, EnvSpec(n_envs=3, maximum_node_count=8, maximum_total_credentials=16)).step(np.zeros((3, 5), np.int32))   # other defenders: fine
    assert capacity.header_counts(capacity.topology("limits", 6, 32, 32))["off_ere"], "64 columns still carry the tables"


def test_flatten_refuses_one_vulnerability_column_too_many():
    """n_local + n_remote <= 255 (MCBS_MAX_VULN_COLUMNS): 32 + 223 flattens, 32 + 224 is refused by name."""
    from marlon_amd import flatten as F, model
    from marlon_amd.samples import capacity as samples
    assert F.MAX_COLUMNS == 255
    h = capacity.header_counts(capacity.topology("limits", 6, 32, 223))
    assert h["n_local"] + h["n_remote"] == 255
    with pytest.raises(ValueError, match="256 vulnerability identifiers .* at most 255"):
        F.flatten(samples.row_limits(model, n_remote=224))
    with open(__file__.replace("tests/test_capacity_script.py", "include/mcbs.h")) as f:
        assert "#define MCBS_MAX_VULN_COLUMNS 255" in f.read()


@pytest.mark.parametrize("name", ["limits_script_s71", "limits_defender_s72", "credlimits257_script_s73"])
def test_reference_traces_at_the_limits_reach_the_edges(name):
    """The traces recorded from the reference on the capacity topologies (oracle/refharness/gen_golden.py; replayed through the oracle by
    test_oracle_golden.py and through the engine by test_gpu_parity.py) go where the older traces never do."""
    from tests import parity
    z, spec = parity.load_trace(name)
    a, raw = z["actions"], z["raw_reward"]
    assert ((a[:, 0] == 2) & (a[:, 3] == 31) & (raw > 0)).any(), "a connect through port 31 that succeeds"
    if name.startswith("limits"):
        assert ((a[:, 0] == 0) & (a[:, 2] == 31) & (raw > 0)).any(), "local id 31 exploited with a positive reward"
        assert z["discovered_nodes_properties"].shape[2] == 60 and (z["discovered_nodes_properties"][:, :, 59] == 1).any(), "property 59 discovered"
        assert ((a[:, 0] == 1) & (a[:, 3] == 7) & (raw > 0)).any(), "the last remote id exploited with a positive reward"
        if spec["defender"]:
            assert z["availability"].min() < 1.0 and z["tape"].shape == (len(a), 4), "the defender re-images"
    else:
        assert int(z["n_cache"].max()) == 257 == spec["maximum_total_credentials"] and (z["cache"] == 256).any(), "a full cache that holds triple 256"


def test_defender_vec_env_script_reaches_the_edges():
    """The oracle-side record of the DefenderVecEnv cell: every branch of the reward shaping fires, re-images clear rows whose
    attacked_since holds bit 31, the managed rules of port 31 (sudo) and port 0 (RDP) are toggled, most attacker actions are played."""
    ref = capacity.defender_vec_env_reference()
    E, T = capacity.VEC_E, capacity.VEC_T
    assert all(v > 0 for v in ref["counts"].values()), f"shaping branches taken: {ref['counts']}"
    assert ref["seen"]["since31_cleared"] >= 8 and ref["seen"]["played"] > E * T // 2
    status = lambda k: [st["obs"][k].reshape(E, 6, 6) for st in ref["steps"]]          # noqa: E731  [env, node, managed rule]
    out, inc = status("outgoing_firewall_status"), status("incoming_firewall_status")
    assert (out[0][:, :, 5] == 1).mean() > 0.9 and any((x[:, :, 5] == 0).any() for x in out), "an outgoing port-31 rule is blocked"
    assert any((x[:, :, 0] == 0).any() for x in out), "an outgoing port-0 rule is blocked"
    assert any((x[:, 2, 5] == 1).any() for x in inc) and any((x[:, 2, 5] == 0).any() for x in inc), "node 2's blocked port 31 is opened again"
    acted = sum(int((np.isin(st["da"][:, 0], (1, 2)) & (st["od"]["valid"] != 0)).sum()) for st in ref["steps"])
    assert acted > 200, "valid firewall actions"
