"""The narrow lean step kernel's decode and the block it runs beside the table loads (marlon_amd/csrc/mcbs_step.hip step_body_narrow):
an action that is not valid — a kind outside 0..2, MCBS_ACTION_SKIP, an index at or past its bound, an env that has ended — must leave
the env as the reference leaves it, whatever its words point at.  The scripts are written for a decode that forms table addresses from
the raw action words (built, measured and left out: profiles/step_decode.md) and are kept for the one that is there: what can go wrong
is a set bit, a row word, a reward or a discovered node taken from the node, descriptor or authorisation word a WRONG index pointed at
(an index whose low four bits name a real entry: 16, 17, a valid index + 16; or one whose low bits are all set: -1, 0x7FFFFFFF); an
ended or skipped env whose header moves; the row pick of 13 nodes; a store address, a list shift or the reward half of the goal formed
ahead of the wait for the tables from a register that the wait's loads still own; a config word that travels as a kernel argument
baked stale into a captured graph.

* oracle parity, bit for bit — reward and terminated per step, the canonical state half way and at the end — at 1, 64 and 65 envs on
  Chain-10, ToyCtf and the hand-made 13-node network; all three must report the narrow kernel.  No auto-reset and truncation at step
  30 of 44, so every env plays its last 14 rows after it has ended.
* the scripts: per row one of eleven recipes, applied to a valid row the policy of tests/endings.py wrote from the oracle's own
  state — left alone; MCBS_ACTION_SKIP; a kind outside 0..3 (among them 16, 17, 18: the low bits name a kind); the source, the target,
  the local or remote vulnerability, the port, the credential index moved to or past its bound (n_disc, L, R, P, n_creds) — to the
  bound itself, the bound + 8, a valid index + 16, 16, 17, 0x7FFFFFFF or -1; columns the kind does not read filled with the same values.
* the expected class of every row is worked out from the oracle's state before the step and checked against the oracle's own
  out-of-bound flag; every class must occur per topology, alone, with an index column >= 8 and with an aliasing value.
* eight steps of Chain-10 at 65 envs captured as one graph and replayed twice from rewind() equal the eager run.
"""
import functools

import numpy as np
import pytest

from tests import endings
from tests.test_gpu_packed_lists import _assert_layout, _same_state
from tests.test_gpu_step_narrow import _spec, _step_through, _topology

pytestmark = pytest.mark.gpu

T, TRUNC, SKIP = 44, 30, 3
ENVS = [1, 64, 65]
TOPOLOGIES = ["chain10", "toyctf", "nodes13"]
GRAPH_STEPS = 8
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
ALIASES = (16, 17, INT_MAX, -1)
BAD_KINDS = np.array([-1, 4, 7, 16, 17, 18, 1000, INT_MIN, INT_MAX], np.int64)
RECIPES = ("valid", "skip", "kind", "src", "tgt", "local", "remote", "port", "cred", "fill", "valid")
CLASSES = ("valid", "skip", "kind", "src", "tgt", "local", "remote", "port", "cred", "ended")


def _past(rng, bound, E):
    """[E] values at or past `bound` ([E] or scalar): the bound, bound + 8, a valid index + 16 (or 16), 17, 0x7FFFFFFF, -1."""
    bound = np.broadcast_to(np.asarray(bound, np.int64), (E,))
    valid16 = 16 + (rng.random(E) * np.maximum(bound, 1)).astype(np.int64)
    table = np.stack([bound, bound + 8, valid16, np.full(E, 16), np.full(E, 17), np.full(E, INT_MAX), np.full(E, -1)])
    out = table[rng.integers(0, table.shape[0], E), np.arange(E)]
    return np.where((out >= 0) & (out < bound), bound, out)        # (16 or 17 below a larger bound: the bound itself)


def _mutate(rng, valid, nd, nc, L, R, P):
    """Rows [E, 5] from the policy's valid rows: one recipe per env."""
    E = valid.shape[0]
    rows = valid.astype(np.int64).copy()
    recipe = np.array(RECIPES)[rng.integers(0, len(RECIPES), E)]
    kind = rows[:, 0]
    fill = np.stack([_past(rng, 0, E) if rng.random() < 0.5 else rng.integers(0, 16, E) for _ in range(5)], axis=1)
    m = recipe == "skip"
    rows[m] = fill[m]
    rows[m, 0] = SKIP
    m = recipe == "kind"
    half = m & (rng.random(E) < 0.5)
    rows[half] = fill[half]
    rows[m, 0] = BAD_KINDS[rng.integers(0, BAD_KINDS.size, E)][m]
    m = recipe == "src"
    rows[m, 1] = _past(rng, nd, E)[m]
    m = recipe == "tgt"                                           # a remote exploit or a connect names a target node
    rows[m & (kind == 0), 0] = 1
    rows[m, 2] = _past(rng, nd, E)[m]
    m = recipe == "local"
    rows[m, 0] = 0
    rows[m, 2] = _past(rng, L, E)[m]
    m = recipe == "remote"
    rows[m & (kind == 0), 2] = 0                                   # (external index 0 is always discovered)
    rows[m, 0] = 1
    rows[m, 3] = _past(rng, R, E)[m]
    m = (recipe == "port") & (nc > 0)                              # a connect checks its credential first: it needs a cached one
    rows[m & (kind == 0), 2] = 0
    rows[m & (kind != 2), 4] = 0
    rows[m, 0] = 2
    rows[m, 3] = _past(rng, P, E)[m]
    m = recipe == "cred"
    rows[m & (kind == 0), 2] = 0
    rows[m, 0] = 2
    rows[m, 4] = _past(rng, nc, E)[m]
    m = recipe == "fill"                                           # columns the kind does not read: anything
    rows[m & (kind == 0), 3] = fill[m & (kind == 0), 3]
    rows[m & (kind != 2), 4] = fill[m & (kind != 2), 4]
    return np.clip(rows, INT_MIN, INT_MAX).astype(np.int32)


def _classify(rows, hdr, L, R, P):
    """[E] class names from the oracle's state before the step (actions.py's order of checks: ended or skipped envs do not play; a kind
    outside 0..2; a connect's credential index; then the indices, in the order source, target or local vulnerability, remote
    vulnerability or port) and [E] the out-of-bound flag that class implies."""
    k, a1, a2, a3, a4 = (rows[:, i].astype(np.int64) & 0xFFFFFFFF for i in range(5))     # the engine compares unsigned
    nd, nc = hdr["n_discovered"].astype(np.int64), hdr["n_creds"].astype(np.int64)
    ended = (hdr["done"] != 0) | (hdr["truncated"] != 0)
    cls = np.full(rows.shape[0], "valid", dtype="<U8")
    for name, cond in reversed([("ended", ended), ("skip", k == SKIP), ("kind", k > 3), ("cred", (k == 2) & (a4 >= nc)), ("src", a1 >= nd),
                                ("local", (k == 0) & (a2 >= L)), ("tgt", (k != 0) & (a2 >= nd)), ("remote", (k == 1) & (a3 >= R)),
                                ("port", (k == 2) & (a3 >= P))]):
        cls[cond] = name
    return cls, np.isin(cls, ("kind", "src", "tgt", "local", "remote", "port"))


@functools.lru_cache(maxsize=None)
def _reference(name, E):
    """(topology, spec, script [T, E, 5], the oracle's outputs per step, its state after T / 2 and after T steps, what the script covers:
    {class: set of tags}); computed once per case and never changed."""
    import dataclasses
    from oracle.oracle import Oracle
    topo = _topology(name)
    spec = dataclasses.replace(_spec(name, E), auto_reset=False, max_episode_steps=TRUNC)
    L, R, P = len(topo.local_vulnerabilities), len(topo.remote_vulnerabilities), len(topo.ports)
    orc = Oracle(topo, spec)
    pol = endings.Policy(topo, spec, seed=700 + E)
    rng = np.random.Generator(np.random.PCG64(9100 + E))
    script, outs, mid, covered = [], [], None, {c: set() for c in CLASSES}
    for t in range(T):
        state = orc.get_state()
        hdr = state[0]
        rows = _mutate(rng, pol.rows(state), hdr["n_discovered"].astype(np.int64), hdr["n_creds"].astype(np.int64), L, R, P)
        cls, oob = _classify(rows, hdr, L, R, P)
        out = orc.step(rows)
        np.testing.assert_array_equal(out["oob"] != 0, oob, err_msg=f"{name}, step {t}: the classes do not give the oracle's out-of-bound flags")
        assert not (out["raw_reward"][np.isin(cls, ("ended", "skip"))] != 0).any() and not (out["raw_reward"][cls != "valid"] > 0).any(), \
            "only a valid action can earn something"
        for e in range(E):
            idx = rows[e, 1:].astype(np.int64)
            covered[cls[e]] |= {"any"} | ({"hi"} if (idx >= 8).any() else set()) | ({"alias"} if np.isin(idx, ALIASES).any() or rows[e, 0] in (16, 17) else set())
        script.append(rows)
        outs.append(out)
        if t == T // 2 - 1:
            mid = orc.get_state()
    final = orc.get_state()
    assert ((final[0]["done"] != 0) | (final[0]["truncated"] != 0)).all(), "every env has ended by truncation at the latest"
    return topo, spec, np.stack(script), outs, mid, final, covered


@pytest.mark.parametrize("name", TOPOLOGIES)
def test_the_scripts_cover_every_class(name):
    """(No GPU work: the scripts of the 64- and 65-env cases together, from the oracle alone.)"""
    topo = _topology(name)
    L, R, P = len(topo.local_vulnerabilities), len(topo.remote_vulnerabilities), len(topo.ports)
    covered = {c: _reference(name, 64)[6][c] | _reference(name, 65)[6][c] for c in CLASSES}
    outs = _reference(name, 64)[3] + _reference(name, 65)[3]
    assert L > 0 and R > 0 and P > 0, "all three topologies have every kind of action, so each can produce every class"
    for c in CLASSES:
        assert covered[c] >= {"any", "hi", "alias"}, f"{name}: class {c} occurs with {sorted(covered[c])} only"
    assert any((o["raw_reward"] > 0.0).any() for o in outs) and any((o["raw_reward"] < 0.0).any() for o in outs), "valid rows succeed and fail"


@pytest.mark.parametrize("E", ENVS)
@pytest.mark.parametrize("name", TOPOLOGIES)
def test_narrow_kernel_against_the_oracle(name, E):
    from marlon_amd import engine
    topo, spec, script, outs, mid, final, _ = _reference(name, E)
    assert (topo.n_nodes > 12) == (name == "nodes13"), "nodes13 alone picks the row out of four vectors"
    eng = engine.BatchEngine(topo, spec)
    try:
        _assert_layout(eng, "packed")
        assert eng.step_topo_traits(False)[0], f"{name} must take the narrow kernel"
        _step_through(eng, script, outs, mid, final, None, f"{name}, {E} envs, narrow kernel")
    finally:
        eng.close()


def test_captured_graph_replays_equal_the_eager_run():
    import torch
    from marlon_amd import engine
    E = 65
    topo, spec, script, outs, _, _, _ = _reference("chain10", E)
    eng = engine.BatchEngine(topo, spec)
    try:
        assert eng.step_topo_traits(False)[0]
        acts = torch.as_tensor(script[:GRAPH_STEPS], dtype=torch.int32, device=eng.device).contiguous()
        rewards = torch.zeros((GRAPH_STEPS, E), dtype=torch.float32, device=eng.device)
        flags = torch.zeros((GRAPH_STEPS, E), dtype=torch.uint8, device=eng.device)

        def run_steps(stream):
            for t in range(GRAPH_STEPS):
                rc = eng.lib.mcbs_step(eng._h, acts[t].data_ptr(), rewards[t].data_ptr(), flags[t].data_ptr(), None, stream)
                assert rc == 0, eng.lib.mcbs_last_error().decode()

        run_steps(eng._stream())
        torch.cuda.synchronize()
        eager = rewards.cpu().numpy().copy(), flags.cpu().numpy().copy(), eng.get_state()
        for t in range(GRAPH_STEPS):
            np.testing.assert_array_equal(eager[0][t].astype(np.float64), outs[t]["reward"], err_msg=f"eager step {t}: reward")
            np.testing.assert_array_equal(eager[1][t], outs[t]["terminated"], err_msg=f"eager step {t}: terminated")
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                run_steps(torch.cuda.current_stream().cuda_stream)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        for replay in (1, 2):
            eng.rewind()
            rewards.zero_()
            flags.fill_(255)
            graph.replay()
            torch.cuda.synchronize()
            np.testing.assert_array_equal(rewards.cpu().numpy().view(np.uint32), eager[0].view(np.uint32), err_msg=f"replay {replay}: rewards")
            np.testing.assert_array_equal(flags.cpu().numpy(), eager[1], err_msg=f"replay {replay}: terminated")
            _same_state(eng.get_state(), eager[2], f"replay {replay}: state after {GRAPH_STEPS} steps")
    finally:
        eng.close()
