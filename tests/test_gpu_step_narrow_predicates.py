"""The narrow lean step kernel's own formulation (mcbs_step.hip `step_body_narrow`): predicates held as bit masks, the eight sets kept as
the four dwords they are stored as, the row updated in its packed form, `max(0, raw)` formed from an integer and the vulnerability's cost
without the raw reward in between, flags, counts and the step counter assembled from masks.  It must compute what the general code
computes.  What can go wrong: a predicate combined wrongly (any failure reason taking effect, or a success not
taking effect); a set bit landing in the neighbouring 16-bit field of its dword (node, credential or triple index >= 8, the lists word's
dword boundary); `old | add` missing a bit or the "changed" test missing a store; a reward arm that is positive for a failure; flags,
counts and the step counter assembled wrongly for envs that are done, skipped, out of bounds, won, truncated or reset in the launch.

Every case is stepped against the CPU oracle, bit for bit: reward and terminated per step, the canonical state (get_state, the episode
counter included) a third of the way, two thirds of the way and at the end.

* env counts 1, 64, 65; topologies Chain-10, ToyCtf attacker-only, and the narrow hand-made networks `base` and `nodes13`
  (tests/topo_traits_nets.py); every one of them must report the narrow kernel.
* scripts: 85 % of the rows come from tests/endings.py Policy (valid rows written from the oracle's own state) — of which one in twelve
  is turned into a connect from the same source to a random discovered node, on a random port, with a random cached credential, so that
  every connect check fails somewhere — the rest are arbitrary (kinds outside 0..3, skips, indices below zero and past every bound,
  credential indices outside the cache).  450 steps, truncation after 300 with auto-reset (Chain-10 episodes get deep: both lists grow
  past nine entries); the attacker wins by owning nine tenths of the nodes (11 of Chain-10's 12), so some envs win and some are truncated.
* the reference builder classifies every (env, step) from the oracle's state before, the row, the oracle's outputs and its state after;
  the first test asserts that the events listed in COVERAGE all occur (in the Chain-10 scripts, but for the two that Chain-10 cannot
  produce: a connect blocked by the target's incoming rules alone and a CustomerData outcome, which ToyCtf shows) and those in
  COVERAGE_SMALL in every other case with 64 or more envs.
* the four dwords of the packed sets: a leaked node changes dword 0 alone (discovered), a leaked credential dword 3 alone, a repeated
  action none.  Dwords 1 (ever owned | running) and 2 (privilege planes) cannot change alone in an attacker-only batch: only taking a
  node changes them, which sets `installed` in dword 0 as well; COVERAGE asks for that step ("sets dwords 0, 1 and 2 change together")
  and for a connect to a node owned before (none of them changes).
* a second test runs the Chain-10 scripts with all five info buffers (the full launch, the general code): rewards as bit patterns, flags
  and the final state equal the narrow run's.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import endings
from tests.test_gpu_packed_lists import _assert_layout, _same_state
from tests.test_gpu_step_narrow import _arbitrary, _environment, _topology

pytestmark = pytest.mark.gpu

T, TRUNC, SKIP = 450, 300, 3
ENVS = [1, 64, 65]
TOPOLOGIES = ["chain10", "toyctf", "base", "nodes13"]
POLICY_SHARE, CONNECT_SHARE = 0.85, 0.08
# mcbs.h MCBS_OUT_*
NONE, LEAKED_CREDENTIALS, LEAKED_NODES, LATERAL_MOVE, CUSTOMER_DATA, PROBE_SUCCEEDED = 0, 1, 2, 4, 5, 6

# what the Chain-10 scripts (all env counts together) must show, from the oracle alone
COVERAGE = (
    "okind none", "okind leaked credentials", "okind leaked nodes", "okind lateral move", "okind customer data", "okind probe succeeded",
    "source not owned", "vulnerability absent", "blocked outgoing", "blocked incoming", "port not listening", "wrong credential",
    "repeated connect", "exploit first time (+7)", "exploit repeated (0)",
    "probe adds bits", "probe adds none", "leak new node", "leak old node", "leak new credential", "leak old credential",
    "credential index outside the cache", "out of bounds", "skip",
    "discovery list 7->8", "discovery list 8->9", "credential list 7->8", "credential list 8->9",
    "source index >= 8", "target index >= 8", "cache index >= 8 in a connect",
    "only sets dword 0 changes", "only sets dword 3 changes", "sets dwords 0, 1 and 2 change together", "no set changes",
    "row changes", "row unchanged", "won", "truncated", "reset inside a launch after a win", "reset inside a launch after truncation",
)
# ... and what every other case with a full wavefront must show (small networks: no deep lists, whatever outcome kinds they have)
COVERAGE_SMALL = ("okind none", "source not owned", "credential index outside the cache", "out of bounds", "skip", "row changes", "row unchanged",
                  "no set changes", "truncated", "reset inside a launch after truncation")


def _spec(name, E):
    from marlon_amd._abi import EnvSpec
    topo = _topology(name)
    if name in ("chain10", "toyctf"):
        kw = dict(maximum_node_count=12, maximum_total_credentials=12 if name == "chain10" else 10,
                  attacker_goal=dict(reward=0.0, low_availability=1.0, own_atleast=0, own_atleast_percent=0.9))
    else:
        kw = dict(maximum_node_count=topo.n_nodes, maximum_total_credentials=4, attacker_goal=None)
    return EnvSpec(n_envs=E, seed=78, env_id_base=9, auto_reset=True, max_episode_steps=TRUNC, **kw)


def _set_dwords(nodes, hdr, cache, order):
    """The four dwords of the packed sets as the canonical state implies them: {discovered | installed << 16, ever owned | running << 16,
    privilege bit 0 | bit 1 << 16}; the fourth (gathered credentials | cached triples << 16) is represented by the cache's content."""
    w = (1 << np.arange(nodes.shape[1], dtype=np.int64))[None, :]
    f = lambda a: ((a != 0) * w).sum(axis=1)
    d0 = f(nodes["discovered"]) | (f(nodes["installed"]) << 16)
    d1 = f(nodes["ever_owned"]) | (f(nodes["running"]) << 16)
    d2 = f(nodes["privilege"] & 1) | (f(nodes["privilege"] & 2) << 16)
    return d0, d1, d2


def _classify(topo, spec, before, rows, out, after, seen):
    """Add the events of one step of every env to `seen`, from the oracle's state before and after, the rows and the oracle's outputs."""
    hdr, nodes, order, cache = before
    hdr2, nodes2, order2, cache2 = after
    nt = topo.node_table()
    E, N = order.shape
    L, R, P = len(topo.local_vulnerabilities), len(topo.remote_vulnerabilities), len(topo.ports)
    ar = np.arange(E)
    kind, a1, a2, a3, a4 = (rows[:, k].astype(np.int64) for k in range(5))
    nd, nc = hdr["n_discovered"].astype(np.int64), hdr["n_creds"].astype(np.int64)
    live = (hdr["done"] == 0) & (hdr["truncated"] == 0)
    oob = out["oob"] != 0
    raw = out["raw_reward"]
    ended = (out["terminated"] != 0) | (out["truncated"] != 0)            # reset inside the launch: `after` is the fresh env
    stay = live & ~ended
    valid_kind = (kind >= 0) & (kind <= 2)
    skip_cred = live & (kind == 2) & ((a4 < 0) | (a4 >= nc))
    X = live & valid_kind & ~oob & ~skip_cred
    note = lambda name, m: seen.add(name) if np.any(m) else None
    note("skip", live & (kind == SKIP))
    note("out of bounds", oob)
    note("credential index outside the cache", skip_cred & ~oob & (raw == -1.0))
    i1 = np.where(X, a1, 0)
    i2 = np.where(X & (kind != 0), a2, i1)
    i4 = np.where(X & (kind == 2), a4, 0)
    src, tgt = order[ar, i1].astype(np.int64), order[ar, i2].astype(np.int64)
    trip = np.minimum(cache[ar, i4].astype(np.int64), max(len(topo.triples) - 1, 0))
    port = np.where(X & (kind == 2), a3, 0)
    so = X & (nodes["installed"][ar, src] != 0)
    note("source not owned", X & ~so & (raw == -1.0))
    note("source index >= 8", so & (i1 >= 8))
    note("target index >= 8", so & (kind != 0) & (i2 >= 8))
    note("cache index >= 8 in a connect", so & (kind == 2) & (i4 >= 8))
    running = nodes["running"][ar, tgt] != 0
    # connects, in the reference's order of checks
    con = so & (kind == 2)
    out_ok = ((nt["fw_out_allow"][src] >> port) & 1) != 0
    in_ok = ((nt["fw_in_allow"][tgt] >> port) & 1) != 0
    listen = ((nt["listen"][tgt] >> port) & 1) != 0
    note("blocked outgoing", con & ~out_ok & (raw == -10.0))
    note("blocked incoming", con & out_ok & ~in_ok & (raw == -10.0))
    note("port not listening", con & out_ok & in_ok & ~listen & (raw == -10.0))
    note("wrong credential", con & out_ok & in_ok & listen & running & (raw == -10.0))
    okind = hdr2["last_outcome_kind"].astype(np.int64)
    moved = con & stay & (okind == LATERAL_MOVE)
    note("repeated connect", moved & (raw == -1.0) & (nodes["installed"][ar, tgt] != 0))
    # exploits
    exp = so & (kind != 2)
    note("vulnerability absent", exp & running & (raw == -5.0))
    took = exp & stay & (okind != NONE)
    slot_new = (nodes2["attacked_ever"][ar, tgt] != nodes["attacked_ever"][ar, tgt])
    note("exploit first time (+7)", took & slot_new)
    note("exploit repeated (0)", took & ~slot_new & (nodes["attacked_since"][ar, tgt] == nodes2["attacked_since"][ar, tgt]))
    for name, k in (("none", NONE), ("leaked credentials", LEAKED_CREDENTIALS), ("leaked nodes", LEAKED_NODES), ("lateral move", LATERAL_MOVE),
                    ("customer data", CUSTOMER_DATA), ("probe succeeded", PROBE_SUCCEEDED)):
        note("okind " + name, stay & live & ~(kind == SKIP) & (okind == k))
    props_new = nodes2["discovered_props"][ar, tgt] != nodes["discovered_props"][ar, tgt]
    note("probe adds bits", took & (okind == PROBE_SUCCEEDED) & props_new)
    note("probe adds none", took & (okind == PROBE_SUCCEEDED) & ~props_new)
    nd2, nc2 = hdr2["n_discovered"].astype(np.int64), hdr2["n_creds"].astype(np.int64)
    leak = took & ((okind == LEAKED_CREDENTIALS) | (okind == LEAKED_NODES))
    note("leak new node", leak & (nd2 == nd + 1))
    note("leak old node", leak & (nd2 == nd))
    note("leak new credential", leak & (okind == LEAKED_CREDENTIALS) & (nc2 == nc + 1))
    note("leak old credential", leak & (okind == LEAKED_CREDENTIALS) & (nc2 == nc))
    for a, b in ((7, 8), (8, 9)):
        note(f"discovery list {a}->{b}", stay & (nd == a) & (nd2 == b))
        note(f"credential list {a}->{b}", stay & (nc == a) & (nc2 == b))
    # the four dwords of the packed sets (the fourth: gathered credentials | cached triples, seen through the cache's count; a gathered
    # credential without a new cache entry does not occur in these topologies' single-entry leaks)
    b0, b1, b2 = _set_dwords(nodes, hdr, cache, order)
    c0, c1, c2 = _set_dwords(nodes2, hdr2, cache2, order2)
    ch = np.stack([b0 != c0, b1 != c1, b2 != c2, nc2 != nc], axis=1) & stay[:, None]
    for q in range(4):
        note(f"only sets dword {q} changes", ch[:, q] & (ch.sum(axis=1) == 1))
    note("sets dwords 0, 1 and 2 change together", ch[:, 0] & ch[:, 1] & ch[:, 2] & ~ch[:, 3])
    note("no set changes", stay & live & X & ~ch.any(axis=1))
    row_ch = stay & (props_new | slot_new | (nodes["attacked_since"][ar, tgt] != nodes2["attacked_since"][ar, tgt]))
    note("row changes", row_ch)
    note("row unchanged", stay & X & ~row_ch)
    won = live & (out["terminated"] != 0) & (out["reward"] == spec.winning_reward)
    note("won", won)
    note("truncated", live & (out["truncated"] != 0))
    fresh = (hdr2["step_count"] == 0) & (hdr2["episode"] == hdr["episode"] + 1)
    note("reset inside a launch after a win", won & fresh)
    note("reset inside a launch after truncation", live & (out["truncated"] != 0) & fresh)


@functools.lru_cache(maxsize=None)
def _reference(name, E):
    """(topology, spec, script [T, E, 5], the oracle's outputs per step, its states after T/3, 2T/3 and T steps, the events seen); computed
    once per case and never changed."""
    from oracle.oracle import Oracle
    topo, spec = _topology(name), _spec(name, E)
    orc = Oracle(topo, spec)
    pol = endings.Policy(topo, spec, seed=700 + E)
    rng = np.random.Generator(np.random.PCG64(9100 + E))
    script, outs, marks, seen = [], [], {}, set()
    before = orc.get_state()
    for t in range(T):
        valid = pol.rows(before)
        nd, nc = before[0]["n_discovered"].astype(np.int64), before[0]["n_creds"].astype(np.int64)
        probe = np.stack([np.full(E, 2), valid[:, 1], (rng.random(E) * nd).astype(np.int64), rng.integers(0, max(1, len(topo.ports)), E),
                          (rng.random(E) * nc).astype(np.int64)], axis=1)
        valid = np.where(((rng.random(E) < CONNECT_SHARE) & (nc > 0))[:, None], probe, valid)
        rows = np.where((rng.random(E) < POLICY_SHARE)[:, None], valid, _arbitrary(rng, E, spec)).astype(np.int32)
        script.append(rows)
        out = orc.step(rows)
        outs.append(out)
        after = orc.get_state()
        _classify(topo, spec, before, rows, out, after, seen)
        before = after
        if t + 1 in (T // 3, 2 * T // 3, T):
            marks[t + 1] = after
    return topo, spec, np.stack(script), outs, marks, frozenset(seen)


def test_the_scripts_show_every_event_the_formulation_handles():
    """From the oracle alone (no GPU code runs here): the union over Chain-10's env counts shows every event of COVERAGE, every other
    case with a full wavefront those of COVERAGE_SMALL."""
    seen = frozenset().union(*(_reference("chain10", E)[5] for E in ENVS))
    seen |= frozenset().union(*(_reference("toyctf", E)[5] for E in ENVS)) & {"blocked incoming", "okind customer data"}
    assert not [c for c in COVERAGE if c not in seen], f"the scripts do not show: {[c for c in COVERAGE if c not in seen]}"
    for name in TOPOLOGIES[1:]:
        for E in ENVS[1:]:
            got = _reference(name, E)[5]
            assert not [c for c in COVERAGE_SMALL if c not in got], f"{name}, {E} envs: not shown: {[c for c in COVERAGE_SMALL if c not in got]}"


def _step_through(eng, script, outs, marks, info, ctx):
    """Step the script; per step reward / terminated against the oracle; state at the marks.  Returns rewards, flags and the final state."""
    torch = eng.torch
    acts = torch.as_tensor(script, dtype=torch.int32, device=eng.device).contiguous()
    rewards, flags = [], []
    for t, o in enumerate(outs):
        rc = eng.lib.mcbs_step(eng._h, acts[t].data_ptr(), eng.reward.data_ptr(), eng.terminated.data_ptr(),
                               C.byref(info) if info is not None else None, eng._stream())
        assert rc == 0, eng.lib.mcbs_last_error().decode()
        r, d = eng.reward.cpu().numpy().copy(), eng.terminated.cpu().numpy().copy()
        np.testing.assert_array_equal(r.astype(np.float64), o["reward"], err_msg=f"{ctx}, step {t}: reward")
        np.testing.assert_array_equal(d, o["terminated"], err_msg=f"{ctx}, step {t}: terminated")
        rewards.append(r)
        flags.append(d)
        if t + 1 in marks:
            _same_state(eng.get_state(), marks[t + 1], f"{ctx}, state after {t + 1} steps")
    return np.stack(rewards), np.stack(flags), eng.get_state()


@pytest.mark.parametrize("E", ENVS)
@pytest.mark.parametrize("name", TOPOLOGIES)
def test_narrow_kernel_against_the_oracle(name, E):
    from marlon_amd import engine
    topo, spec, script, outs, marks, _ = _reference(name, E)
    eng = engine.BatchEngine(topo, spec)
    try:
        _assert_layout(eng, "packed")
        assert eng.step_topo_traits(False)[0], f"{name} must take the narrow kernel"
        _step_through(eng, script, outs, marks, None, f"{name}, {E} envs, narrow kernel")
    finally:
        eng.close()


@pytest.mark.parametrize("E", ENVS)
def test_full_launch_with_info_buffers_equals_the_narrow_run(E):
    from marlon_amd import engine
    from marlon_amd._abi import InfoBuffers
    topo, spec, script, outs, marks, _ = _reference("chain10", E)
    got = []
    for with_info in (False, True):
        eng = engine.BatchEngine(topo, spec)
        try:
            assert eng.step_topo_traits(with_info)[0] == (not with_info)
            info = InfoBuffers(**{m: eng.info[m].data_ptr() for m in ("network_availability", "step_count", "truncated", "out_of_bound",
                                                                      "raw_reward")}) if with_info else None
            got.append(_step_through(eng, script, outs, marks, info, f"chain10, {E} envs, {'with' if with_info else 'without'} info buffers"))
        finally:
            eng.close()
    np.testing.assert_array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32), err_msg="rewards of the two launches, as bit patterns")
    np.testing.assert_array_equal(got[0][1], got[1][1], err_msg="terminated flags of the two launches")
    _same_state(got[0][2], got[1][2], f"chain10, {E} envs: final state of the two launches")
