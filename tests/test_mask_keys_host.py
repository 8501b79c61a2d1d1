"""The action-mask key format on the host (marlon_amd/mask_keys.py, include/mcbs.h "action-mask keys"): the word count, keys built from
the oracle's state records expanded back to the oracle's own observation masks, and the documented rule for malformed keys.  No GPU:
tests/test_gpu_mask_keys.py holds the device to the same mirror."""
import numpy as np

from marlon_amd import mask_keys
from marlon_amd._abi import EnvSpec
from tests import parity


def pack_host(mask) -> np.ndarray:
    """bool [n, A] -> uint32 [n, ceil(A / 32)], tail bits zero (as tests/test_gpu_packed_masks.py packs the oracle's fields)."""
    mask = np.asarray(mask, dtype=bool)
    n, A = mask.shape
    W = (A + 31) // 32
    b = np.packbits(mask, axis=1, bitorder="little")
    out = np.zeros((n, 4 * W), dtype=np.uint8)
    out[:, :b.shape[1]] = b
    return out.view("<u4")


def oracle_mask(oo, E):
    return np.concatenate([oo["mask_connect"].reshape(E, -1), oo["mask_local"].reshape(E, -1), oo["mask_remote"].reshape(E, -1)], axis=1) != 0


def test_key_words_follow_the_rule():
    topo10 = parity.topology_for("chain10_mix_s3")
    assert topo10.n_nodes == 12
    assert mask_keys.key_words(topo10, EnvSpec(maximum_node_count=12, maximum_total_credentials=12)) == 5           # 1 + 1 + 3: 20 B
    assert mask_keys.key_words(topo10, EnvSpec(maximum_node_count=40, maximum_total_credentials=12)) == 5           # Nk = the topology's 12
    for trace in ("toyctf_defender_s11", "chain4_defender_s21", "tiny_defender_s62", "random24_defender_s51"):
        topo = parity.topology_for(trace)
        for bound in (topo.n_nodes, topo.n_nodes + 1, topo.n_nodes + 40):
            nk = min(bound, topo.n_nodes)
            spec = EnvSpec(maximum_node_count=bound, maximum_total_credentials=30)
            assert mask_keys.key_node_bound(topo, spec) == nk
            assert mask_keys.key_words(topo, spec) == 1 + -(-nk // 32) + -(-nk // 4)

    class Big:                                   # the format's largest topology: 256 nodes, 1 + 8 + 64 words
        n_nodes = 256
    assert mask_keys.key_words(Big, EnvSpec(maximum_node_count=256)) == 73
    assert mask_keys.key_words(Big, EnvSpec(maximum_node_count=33)) == 1 + 2 + 9


def test_keys_from_oracle_state_expand_to_the_oracle_masks():
    """chain10_mix_s3 without a defender, 64 envs spread over the trace (every env plays the trace's actions in order, each at its own
    pace, and random in-range actions in between; auto-resets included): every few steps the keys built from the oracle's state record
    expand to the oracle's mask_connect | mask_local | mask_remote, packed."""
    from oracle.oracle import Oracle
    z, sj = parity.load_trace("chain10_mix_s3")
    assert sj.get("defender") is None
    topo = parity.topology_for("chain10_mix_s3")
    E = 64
    spec = parity.spec_from_json(sj, n_envs=E, auto_reset=True, max_episode_steps=45)
    orc = Oracle(topo, spec)
    acts = np.asarray(z["actions"], dtype=np.int32)
    rng = np.random.default_rng(3)
    N, C = spec.maximum_node_count, spec.maximum_total_credentials
    hi = np.array([3, N, N, max(len(topo.ports), len(topo.local_vulnerabilities), len(topo.remote_vulnerabilities)), C])
    ptr = np.zeros(E, dtype=np.int64)
    fields = ["mask_local", "mask_remote", "mask_connect"]
    seen_on = seen_counts = checked = 0
    for t in range(90):
        play = rng.random(E) < 0.75
        a = np.where(play[:, None], acts[ptr % len(acts)], rng.integers(0, hi, size=(E, 5)).astype(np.int32))
        ptr += play
        oo = orc.alloc_obs(fields)
        out = orc.step(a, obs=oo)
        ptr[(out["terminated"] != 0) | (out["truncated"] != 0)] = 0
        if t % 4 != 3:
            continue
        hdr, nodes, order, _ = orc.get_state()
        keys = mask_keys.keys_from_state(hdr, nodes, order, topo, spec)
        assert keys.shape == (E, 5) and keys.dtype == np.uint32
        want = pack_host(oracle_mask(oo, E))
        np.testing.assert_array_equal(mask_keys.expand_host(keys, topo, spec), want, err_msg=f"step {t}")
        seen_on += int(oracle_mask(oo, E).sum())
        seen_counts = max(seen_counts, len(set((keys[:, 0] & 0xFFFF).tolist())))
        checked += 1
    assert checked >= 20 and seen_on > 0 and seen_counts >= 3          # the envs really were in different states


def test_malformed_keys_follow_the_documented_rule():
    """count 0xFFFF acts as Nk; node bytes 0xFF (no such node) give no local bits; owned-source bits at or beyond the count are ignored;
    the credential count is used as it stands."""
    topo = parity.topology_for("toyctf_defender_s11")
    spec = EnvSpec(maximum_node_count=12, maximum_total_credentials=10)
    nk, wk = mask_keys.key_node_bound(topo, spec), mask_keys.key_words(topo, spec)
    assert nk == topo.n_nodes <= 12
    nb = 1
    N, C = 12, 10
    P, L, R = len(topo.ports), len(topo.local_vulnerabilities), len(topo.remote_vulnerabilities)
    M, ML = N * N * P * C, N * L
    table = topo.node_table()["local_mask"]

    def unpack(words):
        return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")[:, :M + ML + N * N * R] != 0

    keys = np.zeros((4, wk), dtype=np.uint32)
    # row 0: count 0xFFFF, 0xFFFF credentials, every owned bit set, node ids 0 .. nk-1 in order
    keys[0, 0] = 0xFFFFFFFF
    keys[0, 1] = 0xFFFFFFFF
    ids = np.zeros(4 * (wk - 1 - nb), dtype=np.uint8)
    ids[:nk] = np.arange(nk)
    keys[0, 1 + nb:] = ids.view("<u4")
    # row 1: the same with every node byte 0xFF
    keys[1] = keys[0]
    keys[1, 1 + nb:] = 0xFFFFFFFF
    # row 2: count 2, owned bits beyond it set, 3 credentials
    keys[2, 0] = 2 | (3 << 16)
    keys[2, 1] = 0xFFFFFFFE
    keys[2, 1 + nb:] = keys[0, 1 + nb:]
    # row 3: count 0 with everything else set: the blank row
    keys[3] = 0xFFFFFFFF
    keys[3, 0] = 0xFFFF0000
    m = unpack(mask_keys.expand_host(keys, topo, spec))
    connect, local, remote = m[:, :M].reshape(4, N, N, P, C), m[:, M:M + ML].reshape(4, N, L), m[:, M + ML:].reshape(4, N, N, R)
    # row 0: Nk discovered nodes, all owned, all credentials
    assert connect[0, :nk, :nk].all() and not connect[0, nk:].any() and not connect[0, :, nk:].any()
    assert remote[0, :nk, :nk].all() and not remote[0, nk:].any() and not remote[0, :, nk:].any()
    for i in range(nk):
        assert local[0, i].tolist() == [bool((int(table[i]) >> l) & 1) for l in range(L)]
    assert not local[0, nk:].any() and local[0].any()
    # row 1: the same connect / remote blocks, no local bit at all
    assert np.array_equal(connect[1], connect[0]) and np.array_equal(remote[1], remote[0]) and not local[1].any()
    # row 2: only discovery index 1 is an owned source (bit 0 is clear, bits from 2 on lie beyond the count); targets 0 and 1; credentials 0 .. 2
    assert connect[2, 1, :2, :, :3].all() and connect[2].sum() == 2 * P * 3
    assert remote[2, 1, :2].all() and remote[2].sum() == 2 * R
    assert local[2, 1].tolist() == [bool((int(table[1]) >> l) & 1) for l in range(L)] and local[2].sum() == local[2, 1].sum()
    assert not m[3].any()
    # words past Wk are not part of the key
    wide = np.full((4, wk + 3), 0xDEADBEEF, dtype=np.uint32)
    wide[:, :wk] = keys
    np.testing.assert_array_equal(mask_keys.expand_host(wide, topo, spec), mask_keys.expand_host(keys, topo, spec))


def test_header_and_exports_name_the_key_calls():
    import os
    import re
    from marlon_amd import engine
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "mcbs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = engine.load_library()
    for name in ("mcbs_mask_key_words", "mcbs_store_mask_keys", "mcbs_expand_mask_keys"):
        assert re.search(rf"\b{name}\s*\(", code) and name in engine.EXPORTS and hasattr(lib, name), name
    assert lib.mcbs_mask_key_words(None) == 0
    assert lib.mcbs_store_mask_keys(None, None, 0, None) == -1 and lib.mcbs_expand_mask_keys(None, None, 0, None, 0, None, 0, 0, None) == -1
