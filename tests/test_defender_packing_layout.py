"""The packed row of the learned defender's observation on the host (include/mcbs.h "packed defender observations",
marlon_amd/features.py DefenderObservationPacking): W_def = ceil(F / 32) words, F = 6N + N + 6N + S, bit c of the row = column c of
DefenderVecEnv.features() — the four MultiBinary fields in sorted key order.  The oracle's defender_observe() is the source of the
bits; no GPU is needed."""
import numpy as np
import pytest

KEYS = ("incoming_firewall_status", "infected_nodes", "outgoing_firewall_status", "services_status")       # sorted
NEW_EXPORTS = ["mcbs_defender_obs_words", "mcbs_defender_observe_packed", "mcbs_pack_defender_observation", "mcbs_unpack_defender_observation",
               "mcbs_encode_defender_features", "mcbs_defender_wrapper_step_packed", "mcbs_defender_wrapper_step_packed_launches"]


def _topology(name):
    from marlon_amd import flatten as F, model
    from marlon_amd.samples import random_net, toy_ctf
    if name == "toyctf":
        return F.flatten(toy_ctf.new_environment())
    env = random_net.build(model, int(name[6:]), 5)
    for _, info in env.nodes():
        info.reimagable = True
    return F.flatten(env)


def _oracle_after_turns(topo, E=16):
    """An oracle batch after defender turns that block rules that exist, allow rules that do not, and re-image the owned node."""
    from marlon_amd._abi import EnvSpec
    from oracle.oracle import Oracle
    spec = EnvSpec(n_envs=E, maximum_node_count=topo.n_nodes, maximum_total_credentials=max(1, len(topo.triples)),
                   maximum_discoverable_credentials_per_action=max(8, int(topo.header()["max_leak_per_action"])),
                   attacker_goal=dict(own_atleast_percent=1.0), maintain_sla=0.0, defender=("external",), seed=3)
    orc = Oracle(topo, spec)
    N = int(topo.n_nodes)
    rng = np.random.Generator(np.random.PCG64(5))
    first = orc.defender_observe()
    first = {k: np.array(first[k]).reshape(E, -1) for k in KEYS}
    for turn in range(4):
        da = np.zeros((E, 12), np.int64)
        for e in range(E):
            n, k = int(rng.integers(N)), int(rng.integers(6))
            if e % 4 == 0:                               # block a rule the incoming list has
                have = np.flatnonzero(first["incoming_firewall_status"][e])
                c = int(have[rng.integers(have.size)]) if have.size else 0
                da[e, 0], da[e, 2], da[e, 3], da[e, 4] = 1, c // 6, c % 6, 1
            elif e % 4 == 1:                             # allow a rule name (appended where the list has none)
                da[e, 0], da[e, 5], da[e, 6], da[e, 7] = 2, n, k, int(rng.integers(2))
            elif e % 4 == 2 and turn == 1:               # re-image a node the attacker holds
                held = np.flatnonzero(first["infected_nodes"][e])
                da[e, 0], da[e, 1] = 0, int(held[0]) if held.size else 0
            else:
                da[e, 0] = -1
        orc.defender_step(da)
    obs = orc.defender_observe()
    return first, {k: np.array(obs[k]).reshape(E, -1) for k in KEYS}


@pytest.mark.parametrize("name", ["toyctf", "random24", "random70"])
def test_widths_offsets_and_bit_placement(name):
    from marlon_amd.features import DEFENDER_KEYS, DefenderObservationPacking
    topo = _topology(name)
    N, S = int(topo.n_nodes), int(topo.header()["n_services"])
    P = DefenderObservationPacking(topo)
    F = 13 * N + S
    assert tuple(DEFENDER_KEYS) == KEYS == tuple(sorted(KEYS))
    assert P.width == F and P.words == -(-F // 32)
    assert P.fields == {KEYS[0]: (0, 6 * N), KEYS[1]: (6 * N, N), KEYS[2]: (7 * N, 6 * N), KEYS[3]: (13 * N, S)}
    if name == "toyctf":
        assert (N, S, F, P.words, F - 32 * (P.words - 1)) == (10, 13, 143, 5, 15)         # 20 B a row; 15 live bits in the last word
    else:
        assert any(off % 32 for off, _ in P.fields.values()) and any(size > 64 for _, size in P.fields.values())   # mid-word starts, several words
    first, obs = _oracle_after_turns(topo)
    assert any((first[k] != obs[k]).any() for k in (KEYS[0], KEYS[2])), "the turns changed no firewall bit"
    assert (first[KEYS[1]] != obs[KEYS[1]]).any() or name == "toyctf", "no node was re-imaged"
    for k in (KEYS[0], KEYS[1]):
        assert (obs[k] == 0).any() and (obs[k] == 1).any(), k
    cols = np.concatenate([obs[k] for k in KEYS], axis=1)
    assert cols.shape[1] == F
    rows = P.pack_host(obs)
    assert rows.dtype == np.uint32 and rows.shape == (cols.shape[0], P.words)
    for c in range(F):
        np.testing.assert_array_equal((rows[:, c >> 5] >> np.uint32(c & 31)) & 1, cols[:, c], err_msg=f"bit {c}")
    if F % 32:
        assert not (rows[:, -1] >> np.uint32(F % 32)).any(), "tail bits must be zero"
    # column c of the named formulas
    n, k = N - 1, 4
    assert P.fields[KEYS[0]][0] + 6 * n + k == 6 * n + k and P.fields[KEYS[2]][0] + 6 * n + k == 7 * N + 6 * n + k
    assert P.fields[KEYS[1]][0] + n == 6 * N + n and P.fields[KEYS[3]][0] == 13 * N


@pytest.mark.parametrize("name", ["toyctf", "random70"])
def test_round_trip_tail_bits_and_nonzero_rule(name):
    from marlon_amd.features import DefenderObservationPacking
    topo = _topology(name)
    P = DefenderObservationPacking(topo)
    rng = np.random.Generator(np.random.PCG64(11))
    x = {k: rng.integers(0, 2, (37, size)).astype(np.int8) for k, (_, size) in P.fields.items()}
    rows = P.pack_host(x)
    back = P.unpack_host(rows)
    assert set(back) == set(KEYS)
    for k in KEYS:
        assert back[k].dtype == np.int8
        np.testing.assert_array_equal(back[k], x[k], err_msg=k)
    np.testing.assert_array_equal(P.unpack_host(rows.view(np.int32))[KEYS[0]], x[KEYS[0]])          # int32 rows, as the device keeps them
    wide = np.concatenate([rows, np.full((37, 3), 0xFFFFFFFF, np.uint32)], axis=1)                   # words beyond W_def are not part of the row
    np.testing.assert_array_equal(P.unpack_host(wide)[KEYS[3]], x[KEYS[3]])
    ones = P.pack_host({k: np.ones_like(v) for k, v in x.items()})
    live = P.width - 32 * (P.words - 1)
    assert (ones[:, :-1] == 0xFFFFFFFF).all() and (ones[:, -1] == (1 << live) - 1).all()             # tail bits zero even for an all-ones row
    # the bit is v != 0: any non-zero value packs to 1 and unpacks to 1
    odd = {k: (v.astype(np.int16) * rng.integers(-128, 128, v.shape)).astype(np.int8) for k, v in x.items()}
    np.testing.assert_array_equal(P.pack_host(odd), P.pack_host({k: (v != 0).astype(np.int8) for k, v in odd.items()}))
    for k in KEYS:
        np.testing.assert_array_equal(P.unpack_host(P.pack_host(odd))[k], (odd[k] != 0).astype(np.int8))
    # trailing shapes [n, N, 6] pack like [n, 6N]
    shaped = dict(x, incoming_firewall_status=x[KEYS[0]].reshape(37, -1, 6))
    np.testing.assert_array_equal(P.pack_host(shaped), rows)


def test_new_entry_points_are_exported():
    from marlon_amd import engine
    for name in NEW_EXPORTS:
        assert name in engine.EXPORTS, name
    lib = engine.load_library()
    assert lib.mcbs_defender_obs_words(None) == 0 and lib.mcbs_defender_wrapper_step_packed_launches(None) == 0
    assert lib.mcbs_defender_observe_packed(None, None, 0, None) == -1 and b"null" in lib.mcbs_last_error()
    assert lib.mcbs_encode_defender_features(None, None, None, 0, None, 0, 0, None, 0, 0, None, None) == -1
