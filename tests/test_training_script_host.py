"""The Chain-10 script schedule (tests/training_script.py) without a GPU: the conditions tests/test_gpu_training_masks.py relies on.
The schedule must put most envs of the batch into a state where the discovery order of the attacker's standing observation and that
of its re-initialised env give DIFFERENT masks, some of them with an owned node in the second list word (index >= 8), next to envs
whose digest was never written by a training turn; and the recorded masks, the script's order and the key mirror must agree."""
import numpy as np
import pytest

from marlon_amd import mask_keys
from marlon_amd._abi import EnvSpec
from tests import parity
from tests import training_script as ts
from tests.test_mask_keys_host import pack_host

E, TURNS = 130, 57


@pytest.fixture(scope="module")
def script():
    return ts.Script()


@pytest.fixture(scope="module")
def schedule(script):
    return ts.Schedule(script, script.geometry(), E, TURNS)


def test_script_facts(script):
    """What the schedule is built on: every script action lies inside the mask recorded before it and inside the discovered range (the
    Discrete wrapper intercepts none), the waiting action lies in no recorded mask, node 2 sits at index 1 from step 3 on, an owned
    node at index 8 from step 39 on, the goal falls at the last step only."""
    geo = script.geometry()
    a = geo.encode(script.rows)
    held = np.arange(-1, script.n_steps - 1)
    m = script.expected_mask(held)
    assert m.shape == (56, geo.total) and geo.total == 14172
    assert m[np.arange(56), a].all(), "a script action outside the mask recorded before it"
    nodes = np.maximum(script.rows[:, 1], np.where(script.rows[:, 0] == 0, 0, script.rows[:, 2]))
    assert (nodes < script.n_disc[held + 1]).all()
    every = script.expected_mask(np.arange(-1, script.n_steps))
    assert not every[:, script.wait_action(geo)].any()
    assert len({r.tobytes() for r in np.packbits(every[1:], axis=1)}) == 26
    deep = script.deepest_owned_index(np.arange(-1, script.n_steps))
    # (rows of `deep`: 0 the fresh env, i + 1 after script step i) the third step, index 2, is the first owned by a node at index 1;
    # the 39th, index 38, the first with an owned index 8
    assert (deep[:3] == 0).all() and (deep[3:] >= 1).all() and int(np.argmax(deep >= 8)) - 1 == 38
    assert script.order[-1].tolist() == [0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 1] and script.order[0].tolist() == [0] + [0xFFFF] * 11
    K = every.sum(1)
    assert (K[1], K[-2]) == (21, 11926) and (np.diff(K[1:]) >= 0).all()       # (K[-1]: the terminal observation's)
    sj = script.spec_json
    assert sj["maintain_sla"] == 0.0 and sj["attacker_goal"]["own_atleast_percent"] == 1.0
    # the live-list mask differs exactly where an owned node sits at an index >= 1
    differs = (every != script.live_list_mask(np.arange(-1, script.n_steps))).any(axis=1)
    np.testing.assert_array_equal(differs, deep >= 1)


def test_schedule_events_and_counts(script, schedule):
    s = schedule
    # turn 50: every defender episode times out, every request byte is set, every observation stands; turn 51: every attacker step is
    # truncated into the fresh observation; nothing else ends an episode in 57 turns
    assert not s.request[:49].any() and s.request[49].all() and not s.request[50:].any()
    assert not s.dones[:50].any() and s.dones[50].all() and not s.dones[51:].any()
    assert (s.held[50] == ts.RESET).all()
    d = s.delay
    np.testing.assert_array_equal(s.held[49], np.where(d <= 49, 49 - d, ts.RESET))
    np.testing.assert_array_equal(s.held[56], np.where(d <= 5, 5 - d, ts.RESET))
    np.testing.assert_array_equal(s.held[29], np.where(d <= 29, 29 - d, ts.RESET))
    # terminal observations of turn 51: the standing one where the action was intercepted, script step 0's for the env that played it
    np.testing.assert_array_equal(s.terminal[50], np.where(d == 50, 0, s.held[49]))
    held = s.held[49]
    expected, live = script.expected_mask(held), script.live_list_mask(held)
    differs = (expected != live).any(axis=1)
    deep = script.deepest_owned_index(held) >= 8
    never = ~s.acted[49]
    K = expected.sum(1)
    print(f"after turn 50 at E = {E}: {int(differs.sum())} envs whose own-list and live-list masks differ, {int(deep.sum())} with an owned "
          f"index >= 8, {int(never.sum())} that never acted; largest K {int(K.max())}")
    # after turn 50 env e has played 50 - d_e steps and holds step index 49 - d_e: the masks differ from index 2 on (d_e <= 47: 48 + 48 +
    # 26 envs), an owned index 8 stands from index 38 on (d_e <= 11: 3 x 12), and d_e = 50, 51 have not played a step (2 x 2)
    np.testing.assert_array_equal(differs, d <= 47)
    np.testing.assert_array_equal(deep, d <= 11)
    np.testing.assert_array_equal(never, d >= 50)
    assert (int(differs.sum()), int(deep.sum()), int(never.sum())) == (122, 36, 4)
    assert differs.sum() >= 100 and deep.sum() >= 20 and never.sum() >= 2
    assert K[s.stale(50)].max() > 2048
    # the local block is where they differ, and only there
    geo = s.geo
    cols = np.flatnonzero((expected != live).any(axis=0))
    assert cols.min() >= geo.connect_size + geo.L and cols.max() < geo.connect_size + geo.local_size


def test_scheduled_actions_lie_inside_the_mask_held_before(script, schedule):
    s = schedule
    wait = script.wait_action(s.geo)
    for turn in range(1, TURNS + 1):
        m = script.expected_mask(s.held_before(turn))
        a, played = s.actions[turn - 1], s.played[turn - 1]
        assert m[played >= 0, a[played >= 0]].all(), f"turn {turn}: a script action outside the mask its attacker holds"
        assert (a[played < 0] == wait).all() and not m[played < 0, wait].any(), f"turn {turn}"
    assert (s.played >= 0).sum() > 3000


def test_key_mirror_on_the_script_order_gives_the_recorded_masks(script, schedule):
    """mask_keys.keys_from_state on the expected counts, owned bits and script order expands (expand_host) to the recorded masks: the
    key words the GPU test compares the device's with describe the masks it compares the device's with."""
    topo = parity.topology_for("chain10_script")
    spec = EnvSpec(maximum_node_count=12, maximum_total_credentials=12)
    for held in (np.arange(-1, script.n_steps), schedule.held[49]):
        keys = mask_keys.keys_from_state(*script.key_state(held, topo), topo, spec)
        assert keys.shape[1] == 5
        np.testing.assert_array_equal(mask_keys.expand_host(keys, topo, spec), pack_host(script.expected_mask(held)))


def test_other_bounds_pad_with_zeros(script):
    """13/13: A = 17 979 (odd), the local block starts at bit 8 of a word; the schedule is the same with the waiting action at node
    index 12; masks and observations are the recorded ones inside [:12] and zero outside."""
    geo = script.geometry(13, 13)
    assert geo.total == 17979 and geo.connect_size % 32 == 8
    s13 = ts.Schedule(script, geo, E, 51)
    s12 = ts.Schedule(script, script.geometry(), E, 51)
    for k in ("held", "request", "dones", "played", "acted"):
        np.testing.assert_array_equal(getattr(s13, k), getattr(s12, k))
    assert geo.decode(script.wait_action(geo)) == (0, 12, 0, 0, 0)
    held = s13.held[49]
    m = script.expected_mask(held, 13, 13)
    assert m.shape == (E, geo.total) and int(m.sum()) == int(script.expected_mask(held).sum())
    assert m[np.arange(E)[s13.played[50] >= 0], s13.actions[50][s13.played[50] >= 0]].all()
    topo = parity.topology_for("chain10_script")
    spec = EnvSpec(maximum_node_count=13, maximum_total_credentials=13)
    keys = mask_keys.keys_from_state(*script.key_state(held, topo), topo, spec)
    np.testing.assert_array_equal(mask_keys.expand_host(keys, topo, spec), pack_host(m))
    assert ((m != script.live_list_mask(held, 13, 13)).any(axis=1) == (s13.delay <= 47)).all()
    obs = script.observation(held, 13, 13)
    assert obs["nodes_privilegelevel"].shape == (E, 13) and obs["credential_cache_matrix"].shape == (E, 13, 2)
    assert not obs["nodes_privilegelevel"][:, 12].any() and not obs["discovered_nodes_properties"][:, 12].any()
