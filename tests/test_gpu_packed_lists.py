"""Packed batches (at most 16 nodes, fewer than 16 credential triples) keep both per-env lists — the discovery order and the credential
cache — as the nibbles of ONE 16-byte word per env (mcbs_device.h): the step kernel picks its source, target and credential with a
shift, ORs a leaked element in at 4 * count in registers and stores the word back once if it changed; every other kernel reads the
lists through DevState::disc_at / cred_at, which hide that layout and the general one (u8 / u16 arrays in the env's body).

Every case here runs against the CPU oracle, on a packed batch (BatchEngine.variant() is asserted) and again with MCBS_NO_PACKED_SETS=1,
which puts the same topology on the general layout: the accessors must hide both.

* state round trip: get_state -> set_state -> get_state is the identity, also into a batch whose lists were longer (the words must be
  cleared, not OR-ed over); with both lists filled to capacity mcbs_step, mcbs_step_many, mcbs_rollout_random and the one-launch
  wrapper step continue bit-equal to the oracle (picks from the upper halves of the words);
* leak paths: no shipped packed topology leaks more than four entries at once (KitchenSink: 4), so `leaky_environment` below is a
  13-node network whose client leaks 6 and 12 node ids and 5 and 10 credentials in single actions, in scrambled id order: entries 4..7
  of a payload take the kernel's second prefetch batch, entries from 8 on its tail loop.  The sequences were chosen with the oracle on
  the CPU; the test asserts from the oracle's own digest that both paths are reached;
* duplicates: a leak of known nodes / credentials only leaves both lists and both counts as they were;
* `leaky16` is the same network at the packed layout's limits, 16 nodes and 15 credential triples: the leak and full-lists cases run
  on it too, so every nibble of both halves of the word is written and picked, and the discovery count reaches 16;
* the in-launch auto-reset, mcbs_reset(mask) and the wrapper's reset restore the lists word (canonical state, and the steps after).
"""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAYOUTS = ("packed", "general")
OBS_FIELDS = ["scalars", "leaked_credentials", "credential_cache_matrix", "discovered_nodes_properties", "nodes_privilegelevel"]


NETS = {"leaky": (12, 10), "leaky16": (15, 15)}              # name: (nodes beside the client, credentials)


def leaky_environment(others=12, creds=10):
    """client (agent installed) + n1..n<others>, each listening on SSH with a credential of its own.  The client's four local
    vulnerabilities leak 6 / all node ids and 5 / all `creds` credentials at once; n1's and n9's remote one leaks the node ids from n7 on."""
    from marlon_amd import model as m
    names = [f"n{i}" for i in range(1, others + 1)]

    def cred(i):
        return m.CachedCredential(node=f"n{i}", port="SSH", credential=f"c{i}")

    def local(outcome):
        return m.VulnerabilityInfo(description="", outcome=outcome, cost=1.0, type=m.VulnerabilityType.LOCAL)

    if (others, creds) == (12, 10):
        six, every = (8, 2, 11, 0, 6, 4), (5, 8, 0, 10, 3, 11, 1, 7, 2, 9, 4, 6)
        five, all_creds = (7, 2, 10, 4, 1), (3, 9, 1, 6, 10, 2, 8, 5, 7, 4)
    else:                                                     # scrambled by strides coprime to the lengths
        six, every = [(11 * i + 8) % others for i in range(6)], [(7 * i + 5) % others for i in range(others)]
        five, all_creds = [1 + (11 * i + 6) % creds for i in range(5)], [1 + (7 * i + 2) % creds for i in range(creds)]
    six, every = [names[i] for i in six], [names[i] for i in every]
    nodes = {"client": m.NodeInfo(services=[], value=0, properties=["CLIENT"], agent_installed=True, reimagable=False, vulnerabilities={
        "LeakSix": local(m.LeakedNodesId(six)),
        "LeakAll": local(m.LeakedNodesId(every)),
        "LeakFiveCreds": local(m.LeakedCredentials([cred(i) for i in five])),
        "LeakTenCreds": local(m.LeakedCredentials([cred(i) for i in all_creds])),
    })}
    for i, n in enumerate(names, 1):
        vs = {}
        if i in (1, 9):      # (whichever of them an env discovers first sits at discovery index 1 or 2)
            vs["ScanNeighbours"] = m.VulnerabilityInfo(description="", outcome=m.LeakedNodesId(names[6:]), cost=1.0, type=m.VulnerabilityType.REMOTE)
        nodes[n] = m.NodeInfo(services=[m.ListeningService("SSH", allowedCredentials=[f"c{i}"])], value=10 * i, properties=["SRV"],
                              vulnerabilities=vs)
    ids = m.infer_constants_from_nodes(list(nodes.items()), {})
    return m.Environment(network=m.create_network(nodes), vulnerability_library={}, identifiers=ids)


def _topology(name):
    from marlon_amd import flatten
    from marlon_amd.samples import chainpattern, toy_ctf
    if name == "chain10":
        return flatten.flatten(chainpattern.new_environment(10))
    if name == "toyctf":
        return flatten.flatten(toy_ctf.new_environment())
    return flatten.flatten(leaky_environment(*NETS[name]))


def _spec(name, E, **over):
    from marlon_amd._abi import EnvSpec
    if name == "chain10":
        kw = dict(maximum_node_count=12, maximum_total_credentials=12)
    elif name == "toyctf":
        kw = dict(maximum_node_count=12, maximum_total_credentials=10, attacker_goal=dict(own_atleast=6, own_atleast_percent=1.0),
                  maintain_sla=0.8, defender=("scan_and_reimage", 0.6, 2, 5))
    else:
        kw = dict(attacker_goal=None, **_bounds(name))
    kw.update(n_envs=E, seed=77)
    kw.update(over)
    return EnvSpec(**kw)


def _bounds(name):
    others, creds = NETS[name]
    return dict(maximum_node_count=others + 1, maximum_total_credentials=12 if name == "leaky" else creds,
                maximum_discoverable_credentials_per_action=creds)


def _assert_layout(eng, layout):
    v = eng.variant()
    assert v["packed"] == (1 if layout == "packed" else 0) and v["coop"] == 0, f"batch dispatches to {v}, the test expects the {layout} layout"


def _engine(topo, spec, layout, monkeypatch):
    from marlon_amd import engine
    if layout == "general":
        monkeypatch.setenv("MCBS_NO_PACKED_SETS", "1")
    eng = engine.BatchEngine(topo, spec)
    monkeypatch.delenv("MCBS_NO_PACKED_SETS", raising=False)
    _assert_layout(eng, layout)
    return eng


def _wrapper(layout, monkeypatch, E, net="leaky", **kw):
    """The attacker wrapper over a leaky network, MultiDiscrete actions, no mask fields: ONE launch on the packed layout."""
    from marlon_amd.wrappers import AttackerVecEnv
    if layout == "general":
        monkeypatch.setenv("MCBS_NO_PACKED_SETS", "1")
    w = AttackerVecEnv(leaky_environment(*NETS[net]), E, attacker_goal=None, discrete=False, materialize_masks=False, **_bounds(net), **kw)
    monkeypatch.delenv("MCBS_NO_PACKED_SETS", raising=False)
    _assert_layout(w.engine, layout)
    assert w.engine.wrapper_step_launches(False) == (1 if layout == "packed" else 3)
    return w


def _same_state(a, b, ctx, but=()):
    for x, y, what in zip(a, b, ("header", "nodes", "order", "cache")):
        if x.dtype.names:
            for f in x.dtype.names:
                if not f.startswith("pad") and f not in but:
                    np.testing.assert_array_equal(x[f], y[f], err_msg=f"{ctx}: state {what}.{f}")
        else:
            np.testing.assert_array_equal(x, y, err_msg=f"{ctx}: state {what}")


def _state_bytes(st):
    return [np.ascontiguousarray(x).tobytes() for x in st]


def _multidiscrete(rows):
    """Engine rows [E, 5] (kind, a1..a4) as the wrapper's MultiDiscrete(10) rows (attack_wrapper.py:206-227)."""
    md = np.zeros((rows.shape[0], 10), np.int64)
    k = rows[:, 0]
    md[:, 0] = k
    for kind, cols in ((0, (1, 2)), (1, (3, 4, 5)), (2, (6, 7, 8, 9))):
        sel = k == kind
        for j, c in enumerate(cols):
            md[sel, c] = rows[sel, 1 + j]
    return md


def _leak_script(topo, E, net="leaky"):
    """[16, E, 5] engine rows.  Env e plays the client's four leaks in the order of permutation e % 24, a remote exploit and a connect in
    between, then the same eight actions again (every leak a duplicate by then).  After the first eight both lists are full."""
    L = list(topo.local_vulnerabilities)
    others, creds = NETS[net]
    perms = list(itertools.permutations([L.index(n) for n in ("LeakSix", "LeakAll", "LeakFiveCreds", "LeakTenCreds")]))
    rows = np.zeros((8, E, 5), np.int32)
    for e in range(E):
        p = perms[e % 24]
        remote = (1, 0, 1 + e % 2, 0, 0)
        for t, a in enumerate(((0, 0, p[0], 0, 0), remote, (0, 0, p[1], 0, 0), (2, 0, 1 + e % 5, 0, e % 3),
                               (0, 0, p[2], 0, 0), remote, (0, 0, p[3], 0, 0), (2, 0, 1 + (e // 5) % others, 0, (e // 3) % creds))):
            rows[t, e] = a
    return np.concatenate([rows, rows]), [L.index("LeakSix"), L.index("LeakAll"), L.index("LeakFiveCreds"), L.index("LeakTenCreds")]


def _assert_obs(wr, oo, ctx):
    for f in OBS_FIELDS:
        np.testing.assert_array_equal(wr._obs[f].cpu().numpy().reshape(wr.num_envs, -1), oo[f].reshape(wr.num_envs, -1), err_msg=f"{ctx}: observation {f}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("net", sorted(NETS))
def test_leaks_of_more_than_four_and_more_than_eight_entries_and_duplicates(net, layout, monkeypatch):
    from oracle.oracle import Oracle
    E = 24 * 9 + 13                                           # a partial last wavefront
    others, creds = NETS[net]
    topo = _topology(net)
    wr = _wrapper(layout, monkeypatch, E, net, max_timesteps=10 ** 6)
    spec = wr.spec
    eng, many = _engine(topo, spec, layout, monkeypatch), _engine(topo, spec, layout, monkeypatch)
    orc = Oracle(topo, spec)
    oo = orc.alloc_obs(OBS_FIELDS)
    torch = eng.torch
    script, leaks = _leak_script(topo, E, net)
    rewards, dones = [], []
    seen_nodes, seen_creds, duplicates = set(), set(), 0
    for t in range(script.shape[0]):
        before = eng.get_state()
        a = torch.as_tensor(script[t], device=eng.device)
        r, d = eng.step(a)
        rewards.append(r.clone()); dones.append(d.clone())
        o = orc.step(script[t], obs=oo)
        ctx = f"{net} {layout} step {t}"
        np.testing.assert_array_equal(r.double().cpu().numpy(), o["reward"], err_msg=ctx + " reward")
        assert not o["oob"].any(), ctx + ": the script left the action space"
        want = orc.get_state()
        after = eng.get_state()
        _same_state(after, want, ctx)
        wr.step(torch.as_tensor(_multidiscrete(script[t]), device=eng.device))
        assert not wr._invalid.any(), ctx + ": the wrapper intercepted a scripted action"
        # (the wrapper's constructor resets its batch, which starts episode 1; nothing here draws from the episode-keyed generator)
        _same_state(wr.engine.get_state(), want, ctx + " (wrapper step)", but=("episode",))
        _assert_obs(wr, oo, ctx + " (wrapper step)")
        h = want[0]
        seen_nodes.update(h["last_new_nodes"].tolist()); seen_creds.update(h["last_new_creds"].tolist())
        # a leak that names only known nodes / credentials: both lists and both counts stay as they were
        dup = np.isin(script[t][:, 2], leaks) & (script[t][:, 0] == 0) & (h["last_new_nodes"] == 0) & (h["last_new_creds"] == 0)
        if t >= 8:
            assert dup[script[t][:, 0] == 0].all(), ctx + ": a repeated leak found something new"
        duplicates += int(dup.sum())
        for k in (2, 3):
            np.testing.assert_array_equal(after[k][dup], before[k][dup], err_msg=ctx + ": a duplicate leak changed a list")
        for f in ("n_discovered", "n_creds"):
            np.testing.assert_array_equal(after[0][f][dup], before[0][f][dup], err_msg=ctx + f": a duplicate leak changed {f}")
    # the paths the case is about were reached: second prefetch batch (5..8 new entries), tail loop (more than 8)
    assert {5, 6, others} <= seen_nodes and {5, creds} <= seen_creds, f"new nodes {sorted(seen_nodes)}, new credentials {sorted(seen_creds)}"
    assert duplicates >= 4 * E
    final = orc.get_state()
    assert (final[0]["n_discovered"] == others + 1).all() and (final[0]["n_creds"] == creds).all()
    r2, d2 = many.step_many(torch.as_tensor(script, device=eng.device))
    assert torch.equal(r2, torch.stack(rewards)) and torch.equal(d2, torch.stack(dones)), f"{layout}: step_many differs from mcbs_step"
    _same_state(many.get_state(), final, f"{layout}: step_many vs the oracle")
    for x in (eng, many, wr):
        x.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("net", sorted(NETS))
def test_full_lists_continue_bit_equal_to_the_oracle(net, layout, monkeypatch):
    """Both lists at capacity (13 of 13 nodes and 10 of 10 credentials; leaky16: 16 of 16 and 15 of 15), put there with mcbs_set_state; then 30 steps of the valid-action
    sampler through mcbs_step, mcbs_step_many, mcbs_rollout_random and the wrapper step."""
    from oracle.oracle import Oracle
    E, K = 200, 30
    others, creds = NETS[net]
    topo = _topology(net)
    wr = _wrapper(layout, monkeypatch, E, net, max_timesteps=10 ** 6)
    spec = wr.spec
    one, many, roll = [_engine(topo, spec, layout, monkeypatch) for _ in range(3)]
    orc = Oracle(topo, spec)
    oo = orc.alloc_obs(OBS_FIELDS)
    script, _ = _leak_script(topo, E, net)
    for t in range(8):
        orc.step(script[t])
    full = orc.get_state()
    assert (full[0]["n_discovered"] == others + 1).all() and (full[0]["n_creds"] == creds).all(), "the script must fill both lists"
    for x in (one, many, roll, wr.engine):
        x.set_state(*full)
        _same_state(x.get_state(), full, f"{layout}: set_state -> get_state")
    torch = one.torch
    acts, rews, dones = [], [], []
    for t in range(K):
        a = one.sample_actions(True, seed=9, step=t)
        r, d = one.step(a)
        acts.append(a.clone()); rews.append(r.clone()); dones.append(d.clone())
        o = orc.step(a.cpu().numpy(), obs=oo)
        ctx = f"{net} {layout} step {t}"
        np.testing.assert_array_equal(r.double().cpu().numpy(), o["reward"], err_msg=ctx + " reward")
        assert not o["oob"].any()
        want = orc.get_state()
        _same_state(one.get_state(), want, ctx)
        wr.step(torch.as_tensor(_multidiscrete(a.cpu().numpy()), device=one.device))
        assert not wr._invalid.any()
        _same_state(wr.engine.get_state(), want, ctx + " (wrapper step)")
        _assert_obs(wr, oo, ctx + " (wrapper step)")
    ring = torch.stack(acts)
    an = ring.cpu().numpy()
    connect = an[:, :, 0] == 2
    assert (an[:, :, 1] >= 8).any() and (an[:, :, 2][an[:, :, 0] != 0] >= 8).any() and (an[:, :, 4][connect] >= 8).any(), \
        "no pick from the upper half of a list"
    if net == "leaky16":                                       # ... and from the last slot of either list
        assert (an[:, :, 2][an[:, :, 0] != 0] == 15).any() and (an[:, :, 4][connect] == 14).any(), "no pick from a list's last slot"
    r2, d2 = many.step_many(ring)
    assert torch.equal(r2, torch.stack(rews)) and torch.equal(d2, torch.stack(dones)), f"{layout}: step_many differs from mcbs_step"
    _same_state(many.get_state(), orc.get_state(), f"{layout}: step_many vs the oracle")
    r3, d3, a3 = roll.rollout_random(K, valid=True, seed=9, first_step=0, record_actions=True)
    assert torch.equal(a3, ring), f"{layout}: the rollout sampled other actions than mcbs_sample_actions"
    assert torch.equal(r3, torch.stack(rews)) and torch.equal(d3, torch.stack(dones)), f"{layout}: rollout_random differs from mcbs_step"
    _same_state(roll.get_state(), orc.get_state(), f"{layout}: rollout_random vs the oracle")
    for x in (one, many, roll, wr):
        x.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["chain10", "leaky", "toyctf"])
def test_state_round_trip(name, layout, monkeypatch):
    from oracle.oracle import Oracle
    E = 203
    topo, spec = _topology(name), _spec(name, E)
    a_eng, b_eng = _engine(topo, spec, layout, monkeypatch), _engine(topo, spec, layout, monkeypatch)
    torch = a_eng.torch
    fresh = a_eng.get_state()
    script = _leak_script(topo, E)[0] if name == "leaky" else None

    def play(eng, t, seed):
        return eng.step(torch.as_tensor(script[t], device=eng.device) if script is not None and t < 16 else eng.sample_actions(True, seed=seed, step=t))

    for t in range(5 if name == "leaky" else 60):
        play(a_eng, t, 3)
    for t in range(16 if name == "leaky" else 90):            # the other batch is somewhere else, with longer lists
        play(b_eng, t, 4)
    st = a_eng.get_state()
    longer = b_eng.get_state()
    assert st[0]["n_discovered"].max() > 1 and (longer[0]["n_discovered"] > st[0]["n_discovered"]).any()
    b_eng.set_state(*st)
    assert _state_bytes(b_eng.get_state()) == _state_bytes(st), f"{name} {layout}: get_state -> set_state -> get_state is not the identity"
    # ... and back to a fresh env: shorter lists than the batch holds, then on against an oracle that starts fresh
    b_eng.set_state(*fresh)
    assert _state_bytes(b_eng.get_state()) == _state_bytes(fresh), f"{name} {layout}: set_state of the reset state"
    orc = Oracle(topo, spec)
    for t in range(16 if name == "leaky" else 60):
        a = torch.as_tensor(script[t], device=b_eng.device) if script is not None else b_eng.sample_actions(True, seed=5, step=t)
        r, d = b_eng.step(a)
        o = orc.step(a.cpu().numpy())
        ctx = f"{name} {layout} step {t} after set_state"
        np.testing.assert_array_equal(r.double().cpu().numpy(), o["reward"], err_msg=ctx + " reward")
        np.testing.assert_array_equal(d.cpu().numpy(), o["terminated"], err_msg=ctx + " terminated")
        if t % 10 == 9 or name == "leaky":
            _same_state(b_eng.get_state(), orc.get_state(), ctx)
    a_eng.close()
    b_eng.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["chain10", "leaky"])
def test_auto_reset_and_reset_by_mask_restore_the_lists(name, layout, monkeypatch):
    """Episodes truncate every 5 steps and the envs are re-initialised inside the launch (mcbs_step and mcbs_step_many), then a third
    of the envs is reset with mcbs_reset(mask) in the middle of an episode: the canonical state equals the oracle's after every step,
    and so do the steps that follow."""
    from oracle.oracle import Oracle
    E, T = 203, 17 if name == "leaky" else 42                 # (the last step is not an episode's last: the envs hold something to reset)
    topo = _topology(name)
    spec = _spec(name, E, auto_reset=True, max_episode_steps=5)
    eng, many = _engine(topo, spec, layout, monkeypatch), _engine(topo, spec, layout, monkeypatch)
    orc = Oracle(topo, spec)
    torch = eng.torch
    script = _leak_script(topo, E)[0] if name == "leaky" else None
    fresh = eng.get_state()
    acts, rews = [], []
    resets = 0

    def step(t, ctx):
        # (leaky: the script's indices assume its own history; where an episode was cut they may leave the action space, which both
        # sides must treat alike)
        a = torch.as_tensor(script[t % 16], device=eng.device) if script is not None else eng.sample_actions(True, seed=21, step=t)
        r, d = eng.step(a)
        o = orc.step(a.cpu().numpy())
        np.testing.assert_array_equal(r.double().cpu().numpy(), o["reward"], err_msg=ctx + " reward")
        np.testing.assert_array_equal(eng.info["truncated"].cpu().numpy(), o["truncated"], err_msg=ctx + " truncated")
        _same_state(eng.get_state(), orc.get_state(), ctx)
        return a, r, o

    for t in range(T):
        a, r, o = step(t, f"{name} {layout} step {t}")
        acts.append(a.clone()); rews.append(r.clone())
        ended = (o["truncated"] != 0) | (o["terminated"] != 0)
        resets += int(ended.sum())
        if ended.any():                                        # the env is fresh again, lists included
            st = eng.get_state()
            for k in (2, 3):
                np.testing.assert_array_equal(st[k][ended], fresh[k][ended], err_msg=f"{name} {layout} step {t}: list after the auto-reset")
    assert resets >= 3 * E
    r2, _ = many.step_many(torch.stack(acts))
    assert torch.equal(r2, torch.stack(rews)), f"{name} {layout}: step_many differs from mcbs_step"
    _same_state(many.get_state(), orc.get_state(), f"{name} {layout}: step_many vs the oracle")
    mid = eng.get_state()
    mask = np.arange(E) % 3 == 0
    assert (mid[0]["n_discovered"][mask] > fresh[0]["n_discovered"][mask]).any(), "the envs to reset must hold more than a fresh env does"
    eng.reset(torch.as_tensor(mask.astype(np.uint8), device=eng.device))
    for i in np.flatnonzero(mask):
        orc.reset(int(i))
    st = eng.get_state()
    _same_state(st, orc.get_state(), f"{name} {layout}: after mcbs_reset(mask)")
    for k in (2, 3):
        np.testing.assert_array_equal(st[k][mask], fresh[k][mask], err_msg=f"{name} {layout}: list after mcbs_reset(mask)")
        np.testing.assert_array_equal(st[k][~mask], mid[k][~mask], err_msg=f"{name} {layout}: mcbs_reset(mask) touched another env's list")
    for t in range(T, T + 8):
        step(t, f"{name} {layout} step {t} after mcbs_reset(mask)")
    eng.close()
    many.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_wrapper_reset_restores_the_lists(layout, monkeypatch):
    """The wrapper truncates every 5 steps and resets the env itself (one-launch step: by the env's own lane, from the config's
    constants; three launches: wrapper_finish).  The oracle is reset where the wrapper reports done."""
    from oracle.oracle import Oracle
    E = 203
    topo = _topology("leaky")
    wr = _wrapper(layout, monkeypatch, E, max_timesteps=5)
    orc = Oracle(topo, wr.spec)
    orc.reset()                                                # as the wrapper's constructor does: episode 1
    oo = orc.alloc_obs(OBS_FIELDS)
    orc.observe(oo, reset_obs=True)                            # the observation reset() returns: what a done env shows next
    reset_obs = {f: oo[f][0].copy() for f in OBS_FIELDS}
    script, _ = _leak_script(topo, E)
    torch = wr.torch
    ends = 0
    for t in range(22):
        rows = script[t % 5]                                   # every episode replays the script's first five actions: always in bounds
        _, r, te, tr, _ = wr.step(torch.as_tensor(_multidiscrete(rows), device=wr.engine.device))
        o = orc.step(rows, obs=oo)
        ctx = f"{layout} wrapper step {t}"
        assert not wr._invalid.any()
        np.testing.assert_array_equal(r.double().cpu().numpy(), o["reward"], err_msg=ctx + " reward")
        done = (te.cpu().numpy() != 0) | (tr.cpu().numpy() != 0)
        assert done.all() == ((t + 1) % 5 == 0) and done.any() == done.all(), ctx
        for i in np.flatnonzero(done):
            orc.reset(int(i))
            for f in OBS_FIELDS:
                oo[f][i] = reset_obs[f]
        ends += int(done.sum())
        _same_state(wr.engine.get_state(), orc.get_state(), ctx)
        _assert_obs(wr, oo, ctx)
    assert ends == 4 * E
    wr.close()
