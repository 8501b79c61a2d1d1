"""The attacker action decoder against a NumPy / Python-integer restatement of the reference, bitwise.

Three copies of one routine turn marlon's Discrete index / MultiDiscrete vector into the engine's [E,5] rows and `invalid` flags:
decode_body behind mcbs_decode_attacker_actions, the same body inside decode_step1_kernel (the three-launch wrapper step), and the
register restatement in the one-launch wrapper step.  The reference is MaskedDiscreteAttackerWrapper._decode (action_masking.py:107-136)
followed by AttackerEnvWrapper._action_in_discovered_range (attack_wrapper.py:233-253).

  * test_every_discrete_index: EVERY index 0 .. A-1 of nine geometries through mcbs_decode_attacker_actions, envs at two or more
    discovered-node counts.  (At the geometry whose A exceeds 2^31 — the only one that reaches the 64-bit quotient path inside the
    contract — all indices within +-2 of every region boundary and of every source / target boundary plus a fixed random 2^22: the
    share left out there is 1 - 2^22 / A, over 99.8 %.  Every other geometry is exhaustive.)
  * test_wrapper_copies_decode_every_index: every index through AttackerVecEnv.step, three-launch and one-launch.
  * test_multidiscrete_*: in-bound vectors of every kind, components at 0 / n_discovered - 1 / n_discovered / N - 1, junk in the
    components of the other kinds.
  * test_outside_the_contract_*: indices and components no action space holds.  The reference raises on each before env.step
    (action_masking.py:109-110; attack_wrapper.py:262 looks the kind up in a dict), so all three copies must return a skip row with
    invalid = 1, and stepping that row must leave the env untouched.
"""
import numpy as np
import pytest

from tests import parity, sampler_law as SL

pytestmark = pytest.mark.gpu

SKIP = 3                                                     # MCBS_ACTION_SKIP


def _engine():
    from marlon_amd import engine
    return engine


def _topology(name):
    from marlon_amd import flatten as F, model
    from marlon_amd.samples import random_net
    if name == "random100":
        return F.flatten(random_net.build(model, 100, 7))
    return parity.topology_for(name)


def _spec(topo, E, N, C, **over):
    from marlon_amd._abi import EnvSpec
    kw = dict(n_envs=E, maximum_node_count=N, maximum_total_credentials=C, attacker_goal=None,
              maximum_discoverable_credentials_per_action=32)
    kw.update(over)
    return EnvSpec(**kw)


# ------------------------------------------------------------------------------------------------------------------ restatements
def ref_decode_discrete(geo, idx, nd):
    """action_masking.py:112-136 + attack_wrapper.py:244-252 for in-space indices, int64 NumPy (// and % on non-negative values)."""
    idx = np.asarray(idx, np.int64)
    assert ((idx >= 0) & (idx < geo.total)).all()
    is_c = idx < geo.connect_size
    is_l = ~is_c & (idx < geo.connect_size + geo.local_size)
    rows = np.zeros((len(idx), 5), np.int64)
    i = idx[is_c]
    cred, i = i % geo.C, i // geo.C
    port, i = i % geo.P, i // geo.P
    rows[is_c] = np.stack([np.full_like(i, 2), i // geo.N, i % geo.N, port, cred], 1)
    i = idx[is_l] - geo.connect_size
    rows[is_l] = np.stack([np.zeros_like(i), i // geo.L, i % geo.L, np.zeros_like(i), np.zeros_like(i)], 1)
    is_r = ~is_c & ~is_l
    i = idx[is_r] - geo.connect_size - geo.local_size
    vuln, i = i % geo.R, i // geo.R
    rows[is_r] = np.stack([np.ones_like(i), i // geo.N, i % geo.N, vuln, np.zeros_like(i)], 1)
    return _intercept(rows, nd)


def _intercept(rows, nd):
    nd = np.asarray(nd, np.int64)
    ok = np.where(rows[:, 0] == 0, rows[:, 1] < nd, (rows[:, 1] < nd) & (rows[:, 2] < nd))
    rows = rows.copy()
    rows[~ok, 0] = SKIP
    return rows.astype(np.int32), (~ok).astype(np.uint8)


def ref_decode_multidiscrete(md, nd):
    """attack_wrapper.py:262-267 (kind picks its slice, the other components are not read) + :244-252, in-space vectors."""
    md = np.asarray(md, np.int64)
    k = md[:, 0]
    assert ((k >= 0) & (k <= 2)).all()
    z = np.zeros_like(k)
    a = np.where(k == 0, md[:, 1], np.where(k == 1, md[:, 3], md[:, 6]))
    b = np.where(k == 0, md[:, 2], np.where(k == 1, md[:, 4], md[:, 7]))
    c = np.where(k == 0, z, np.where(k == 1, md[:, 5], md[:, 8]))
    d = np.where(k == 2, md[:, 9], z)
    return _intercept(np.stack([k, a, b, c, d], 1), nd)


def test_restatement_agrees_with_python_integers():
    """The vectorised restatement against the line-by-line one (sampler_law.Geometry.decode, Python integers) — no device involved."""
    from marlon_amd._abi import EnvSpec
    geo = SL.Geometry(_topology("chain10"), EnvSpec(maximum_node_count=12, maximum_total_credentials=12))
    idx = np.arange(geo.total)
    rows, inv = ref_decode_discrete(geo, idx, np.full(geo.total, 12))
    assert not inv.any()
    np.testing.assert_array_equal(rows, np.asarray([geo.decode(i) for i in idx], np.int32))


# ------------------------------------------------------------------------------------------------------------------ batches
def _mixed_batch(name, N, C, E, steps=40):
    """A batch whose first half is at reset and whose second half has taken `steps` sampled valid steps: n_discovered differs."""
    topo = _topology(name)
    assert N >= topo.n_nodes and C >= max(1, len(topo.triples))
    spec = _spec(topo, E, N, C)
    eng = _engine().BatchEngine(topo, spec)
    fresh = eng.get_state()
    for t in range(steps):
        eng.step(eng.sample_actions(True, seed=31, step=t), with_info=False)
    st = eng.get_state()
    for adv, new in zip(st, fresh):
        adv[:E // 2] = new[:E // 2]
    eng.set_state(*st)
    nd = eng.get_state()[0]["n_discovered"].astype(np.int64)
    assert len(np.unique(nd)) >= 2 and nd.max() > nd[0], f"{name}: n_discovered takes the values {np.unique(nd)}"
    geo = SL.Geometry(topo, spec)
    assert eng.discrete_action_count() == geo.total
    return eng, geo, nd


def _check_discrete(eng, geo, nd, idx, ctx):
    """Decode len(idx) <= E indices (padded with 0), spread over the envs by a fixed bijection so that every region meets every count."""
    E = eng.E
    full = np.zeros(E, np.int64)
    full[:len(idx)] = idx
    perm = (np.arange(E, dtype=np.int64) * 40503 + 977) % E if E & (E - 1) == 0 else np.arange(E)
    full = full[perm]
    rows, inv = eng.decode_attacker_actions(discrete=full)
    want_rows, want_inv = ref_decode_discrete(geo, full, nd)
    rows, inv = rows.cpu().numpy(), inv.cpu().numpy()
    bad = np.flatnonzero((rows != want_rows).any(1) | (inv != want_inv))
    assert bad.size == 0, (f"{ctx}: {bad.size} of {E} differ, first: index {full[bad[0]]} n_discovered {nd[bad[0]]} -> row {rows[bad[0]].tolist()} "
                           f"invalid {inv[bad[0]]}, reference {want_rows[bad[0]].tolist()} invalid {want_inv[bad[0]]}")
    return int(want_inv.sum())


# (topology, N, C, E)
GEOMETRIES = [("chain4", 6, 6, 1024), ("chain10", 12, 12, 4096), ("toyctf", 10, 61, 16384), ("toyctf", 11, 64, 16384), ("tiny", 4, 1, 64),
              ("sink", 7, 8, 1024), ("random24", 24, 40, 65536), ("random100", 100, 0, 65536), ("random24", 256, 8192, 8192)]


@pytest.mark.parametrize("name,N,C,E", GEOMETRIES, ids=[f"{n}-{a}x{c or 'triples'}" for n, a, c, _ in GEOMETRIES])
def test_every_discrete_index(name, N, C, E):
    C = C or len(_topology(name).triples)
    eng, geo, nd = _mixed_batch(name, N, C, E)
    A = geo.total
    flagged = total = 0
    if A <= 1 << 26:
        todo = np.arange(A, dtype=np.int64)
    else:                                                    # beyond 2^31: the 64-bit quotient path, sampled (module docstring)
        assert A > 1 << 31
        near = np.arange(-2, 3, dtype=np.int64)
        edges = [np.array([0, geo.connect_size, geo.connect_size + geo.local_size, A, 1 << 31], np.int64),
                 np.arange(geo.N + 1, dtype=np.int64) * (geo.N * geo.P * geo.C),                      # connect: source boundaries
                 np.arange(geo.N * 40, dtype=np.int64) * (geo.P * geo.C),                             # connect: target boundaries, 40 sources
                 geo.connect_size + np.arange(geo.N + 1, dtype=np.int64) * geo.L,                     # local: source boundaries
                 geo.connect_size + geo.local_size + np.arange(geo.N * geo.N + 1, dtype=np.int64) * geo.R]   # remote: every target boundary
        todo = np.unique(np.concatenate([(e[:, None] + near[None, :]).reshape(-1) for e in edges] +
                                        [np.random.Generator(np.random.PCG64(7)).integers(0, A, 1 << 22)]))
        todo = todo[(todo >= 0) & (todo < A)]
        assert (todo >= 1 << 31).sum() > 1 << 20
    for lo in range(0, len(todo), E):
        chunk = todo[lo:lo + E]
        flagged += _check_discrete(eng, geo, nd, chunk, f"{name} {N}x{C} indices {chunk[0]}..{chunk[-1]}")
        total += len(chunk)
    assert 0 < flagged < total, f"{name} {N}x{C}: {flagged} of {total} intercepted — the batch does not show both values"
    eng.close()


# The one-launch step exists for batches of at most 16 nodes and 16 cacheable credentials (mcbs_attacker_wrapper_step_launches), so
# ToyCtf at 10 x 61 can only take the three-launch path; the register copy sees ToyCtf at its 12 x 10 bounds and Chain-10 instead.
WRAPPED = [("chain4", 6, 6, False), ("toyctf", 10, 61, False), ("chain4", 6, 6, True), ("toyctf", 12, 10, True), ("chain10", 12, 12, True)]


@pytest.mark.parametrize("name,N,C,one_launch", WRAPPED, ids=[f"{n}-{a}x{c}-{'one_launch' if o else 'three_launches'}" for n, a, c, o in WRAPPED])
def test_wrapper_copies_decode_every_index(name, N, C, one_launch):
    """decode_step1_kernel (masks materialised: three launches) and the one-launch step's register copy: every index, the batch re-reset
    before each chunk so that n_discovered is the reset value."""
    from marlon_amd.wrappers import AttackerVecEnv
    topo = _topology(name)
    E = 2048
    att = AttackerVecEnv(topo, E, maximum_node_count=N, maximum_total_credentials=C, attacker_goal=None, discrete=True,
                         materialize_masks=not one_launch, max_timesteps=1000)
    launches = att.engine.wrapper_step_launches(not one_launch)
    assert launches == (1 if one_launch else 3), f"mcbs_attacker_wrapper_step_launches = {launches}"
    geo = SL.Geometry(topo, att.spec)
    assert att.discrete_n == geo.total
    att.reset()
    nd0 = att.engine.get_state()[0]["n_discovered"].astype(np.int64)
    flagged = 0
    for lo in range(0, geo.total, E):
        idx = np.zeros(E, np.int64)
        n = min(E, geo.total - lo)
        idx[:n] = np.arange(lo, lo + n)
        att.reset()
        att.step(idx)
        want_rows, want_inv = ref_decode_discrete(geo, idx, nd0)
        rows, inv = att._rows.cpu().numpy(), att._invalid.cpu().numpy()
        bad = np.flatnonzero((rows != want_rows).any(1) | (inv != want_inv))
        assert bad.size == 0, (f"{name} {N}x{C} launches {launches}: index {idx[bad[0]]} -> row {rows[bad[0]].tolist()} invalid {inv[bad[0]]}, "
                               f"reference {want_rows[bad[0]].tolist()} invalid {want_inv[bad[0]]}")
        flagged += int(want_inv.sum())
    assert 0 < flagged < geo.total
    att.close()


# ------------------------------------------------------------------------------------------------------------------ MultiDiscrete
def _md_vectors(geo, nd, rng):
    """[E,10] in-space vectors: the chosen kind's components uniform in their bound, or pinned to an edge; the rest junk."""
    E = len(nd)
    nvec = np.array([3, geo.N, geo.L, geo.N, geo.N, geo.R, geo.N, geo.N, geo.P, geo.C], np.int64)
    md = (rng.random((E, 10)) * nvec).astype(np.int64)
    edge = rng.integers(0, 6, E)                             # 0, 1: leave uniform; 2..5: pin source and / or target
    pins = {2: np.zeros(E, np.int64), 3: np.maximum(nd - 1, 0), 4: np.minimum(nd, geo.N - 1), 5: np.full(E, geo.N - 1)}
    src_col, tgt_col = np.array([1, 3, 6])[md[:, 0]], np.array([2, 4, 7])[md[:, 0]]
    for e_val, v in pins.items():
        rows = np.flatnonzero(edge == e_val)
        which = rng.integers(0, 3, len(rows))                # source, target, both
        s = rows[which != 1]
        md[s, src_col[s]] = v[s]
        t = rows[(which != 0) & (md[rows, 0] != 0)]
        md[t, tgt_col[t]] = v[t]
    used = np.zeros((E, 10), bool)
    used[:, 0] = True
    for k, cols in ((0, (1, 2)), (1, (3, 4, 5)), (2, (6, 7, 8, 9))):
        used[np.ix_(md[:, 0] == k, cols)] = True
    junk = rng.integers(-2 ** 62, 2 ** 62, (E, 10))
    junk[rng.random((E, 10)) < 0.3] = -1
    return np.where(used, md, junk)


@pytest.mark.parametrize("name,N,C", [("chain10", 12, 12), ("toyctf", 11, 64), ("random100", 100, 0)], ids=["chain10", "toyctf", "random100"])
def test_multidiscrete_vectors(name, N, C):
    C = C or len(_topology(name).triples)
    E = 16384
    eng, geo, nd = _mixed_batch(name, N, C, E)
    rng = np.random.Generator(np.random.PCG64(N * 1000 + C))
    seen = set()
    for rep in range(4):
        md = _md_vectors(geo, nd, rng)
        rows, inv = eng.decode_attacker_actions(multidiscrete=md)
        want_rows, want_inv = ref_decode_multidiscrete(md, nd)
        rows, inv = rows.cpu().numpy(), inv.cpu().numpy()
        bad = np.flatnonzero((rows != want_rows).any(1) | (inv != want_inv))
        assert bad.size == 0, (f"{name} rep {rep}: vector {md[bad[0]].tolist()} n_discovered {nd[bad[0]]} -> row {rows[bad[0]].tolist()} invalid "
                               f"{inv[bad[0]]}, reference {want_rows[bad[0]].tolist()} invalid {want_inv[bad[0]]}")
        seen.update(zip(md[:, 0].tolist(), want_inv.tolist()))
    assert seen == {(k, v) for k in (0, 1, 2) for v in (0, 1)}, f"{name}: (kind, invalid) pairs seen {sorted(seen)}"
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ outside the contract
def _outside_discrete(A):
    return np.array([-1, -A, A, A + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 40, -2 ** 40, -2, -A - 1, -2 ** 31, -2 ** 63, 2 ** 63 - 1], np.int64)


def _outside_multidiscrete(geo, rng, n):
    """In-space vectors spoiled in one place: kind -1 / 3 / 2^33, or one component of the chosen kind negative."""
    nvec = np.array([3, geo.N, geo.L, geo.N, geo.N, geo.R, geo.N, geo.N, geo.P, geo.C], np.int64)
    md = (rng.random((n, 10)) * nvec).astype(np.int64)
    md[:, [1, 3, 4, 6, 7]] = 0                               # sources and targets in range at every n_discovered: only the spoiled place counts
    how = np.arange(n) % 5
    md[how == 0, 0] = -1
    md[how == 1, 0] = 3
    md[how == 2, 0] = 2 ** 33
    cols = {0: (1, 2), 1: (3, 4, 5), 2: (6, 7, 8, 9)}
    for e in np.flatnonzero(how >= 3):
        c = cols[int(md[e, 0])]
        md[e, c[int(rng.integers(len(c)))]] = -1 if how[e] == 3 else -int(rng.integers(2, 2 ** 40))
    return md


def _assert_skipped(rows, inv, what, ctx):
    rows, inv = rows.cpu().numpy(), inv.cpu().numpy()
    bad = np.flatnonzero((rows[:len(what), 0] != SKIP) | (inv[:len(what)] != 1))
    assert bad.size == 0, f"{ctx}: {what[bad[0]].tolist()} -> row {rows[bad[0]].tolist()} invalid {inv[bad[0]]}; the reference raises and never steps"


@pytest.mark.parametrize("name,N,C", [("chain4", 6, 6), ("toyctf", 10, 61), ("random100", 100, 0)], ids=["chain4", "toyctf", "random100"])
def test_outside_the_contract_is_skipped_by_the_decode_kernel(name, N, C):
    C = C or len(_topology(name).triples)
    E = 1024
    eng, geo, nd = _mixed_batch(name, N, C, E)
    before = eng.get_state()
    out = _outside_discrete(geo.total)
    idx = np.zeros(E, np.int64)
    idx[:len(out)] = out
    rows, inv = eng.decode_attacker_actions(discrete=idx)
    _assert_skipped(rows, inv, out, f"{name} Discrete")
    md = _outside_multidiscrete(geo, np.random.Generator(np.random.PCG64(11)), E)
    rows_md, inv_md = eng.decode_attacker_actions(multidiscrete=md)
    _assert_skipped(rows_md, inv_md, md, f"{name} MultiDiscrete")
    # a skip row does not step: state, step count and defender untouched
    rows[len(out):, 0] = SKIP
    eng.step(rows)
    assert not eng.info["out_of_bound"].any()
    eng.step(rows_md)
    assert not eng.info["out_of_bound"].any()
    for x, y, what in zip(before, eng.get_state(), ("header", "nodes", "order", "cache")):
        assert x.tobytes() == y.tobytes(), f"{name}: stepping the skip rows changed state {what}"
    eng.close()


@pytest.mark.parametrize("one_launch", [False, True], ids=["three_launches", "one_launch"])
@pytest.mark.parametrize("discrete", [True, False], ids=["discrete", "multidiscrete"])
def test_outside_the_contract_is_skipped_by_the_wrapper_step(discrete, one_launch):
    from marlon_amd.wrappers import AttackerVecEnv
    topo = _topology("chain4")
    E = 256
    att = AttackerVecEnv(topo, E, maximum_node_count=6, maximum_total_credentials=6, attacker_goal=None, discrete=discrete,
                         materialize_masks=not one_launch, max_timesteps=1000)
    launches = att.engine.wrapper_step_launches(not one_launch)
    assert launches == (1 if one_launch else 3), f"mcbs_attacker_wrapper_step_launches = {launches}"
    geo = SL.Geometry(topo, att.spec)
    att.reset()
    before = att.engine.get_state()
    if discrete:
        what = _outside_discrete(geo.total)
        actions = np.full(E, -1, np.int64)
        actions[:len(what)] = what
        what = actions
    else:
        what = actions = _outside_multidiscrete(geo, np.random.Generator(np.random.PCG64(12)), E)
    _, _, _, _, info = att.step(actions)
    _assert_skipped(att._rows, att._invalid, what, f"chain4 wrapper step, {launches} launch(es)")
    assert not info["cyber_step_executed"].any() and info["invalid_action"].all()
    for x, y, name in zip(before, att.engine.get_state(), ("header", "nodes", "order", "cache")):
        assert x.tobytes() == y.tobytes(), f"wrapper step on out-of-space actions changed state {name}"
    att.close()
