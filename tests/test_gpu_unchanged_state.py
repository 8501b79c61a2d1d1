"""The step kernel stores a node row, a set word, a header or a list entry only when its bits changed (mcbs_step.hip; the looping
mcbs_step_many shares its body).  A skipped store leaves the bytes that were there, so these tests check two things on Chain-10 and
ToyCtf packed, ToyCtf in the general layout (one word per set), and Chain-100, whose mcbs_step runs the cooperative kernel while its
mcbs_step_many runs mcbs_step.hip:

* steps that cannot change an env leave every byte of its canonical state (mcbs_get_state) as it was: skip actions, steps after the
  episode ended without auto-reset; an out-of-bounds action moves only the step counter and the outcome digest;
* over 1 000 steps with auto-resets, valid, uniform and skip actions mixed, mcbs_step and mcbs_step_many give the same outputs and the
  same state, and both equal the CPU oracle.

Reach: the no-op tests would pass on kernels that store every value back unchanged too; they pin that a guard never drops a change
an ended or skipped env must not see, not that the store is skipped (mcbs_get_state cannot show the list slack slot, and write
traffic is measured by profiles/round3_step_headline.json).  The comparison with the oracle and with mcbs_step_many (whose looping
variant keeps unconditional stores) is what checks the guards.  For chain100_coop, mcbs_step runs the cooperative kernel, which has
no guards.  The split-phase (mcbs_step_observe) and fused wrapper instantiations of the guarded stores are covered by the existing
parity and wrapper tests."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SKIP = 3   # MCBS_ACTION_SKIP

# name: (envs, expected variant of the mcbs_step batch)
LAYOUTS = {
    "chain10": (333, dict(packed=1, words_per_set=1, coop=0)),
    "toyctf_defender": (333, dict(packed=1, words_per_set=1, coop=0)),
    "toyctf_general": (333, dict(packed=0, words_per_set=1, coop=0)),
    "chain100_coop": (131, dict(packed=0, words_per_set=2, coop=1)),
}


def _topology(name):
    from marlon_amd import flatten
    from marlon_amd.samples import chainpattern, toy_ctf
    if name == "chain10":
        return flatten.flatten(chainpattern.new_environment(10))
    if name == "chain100_coop":
        return flatten.flatten(chainpattern.new_environment(100))
    return flatten.flatten(toy_ctf.new_environment())


def _spec(name, E, **over):
    from marlon_amd._abi import EnvSpec
    if name == "chain10":
        kw = dict(maximum_node_count=12, maximum_total_credentials=12)
    elif name == "chain100_coop":
        kw = dict(maximum_node_count=102, maximum_total_credentials=102, attacker_goal=dict(own_atleast_percent=1.0),
                  defender=("scan_and_reimage", 0.6, 2, 5))
    else:
        kw = dict(maximum_node_count=12, maximum_total_credentials=10, attacker_goal=dict(own_atleast=6, own_atleast_percent=1.0),
                  maintain_sla=0.8, defender=("scan_and_reimage", 0.6, 2, 5))
    kw.update(n_envs=E, auto_reset=True, max_episode_steps=120, seed=4242)
    kw.update(over)
    return EnvSpec(**kw)


def _engine(name, spec, monkeypatch, want=None):
    from marlon_amd import engine
    if name == "toyctf_general":
        monkeypatch.setenv("MCBS_NO_PACKED_SETS", "1")
    eng = engine.BatchEngine(_topology(name), spec)
    monkeypatch.delenv("MCBS_NO_PACKED_SETS", raising=False)
    if want is not None:
        v = eng.variant()
        assert {k: v[k] for k in want} == want, f"batch dispatches to {v}, the test expects {want}"
    return eng


def _state_bytes(st):
    return [np.ascontiguousarray(x).tobytes() for x in st]


def _assert_same_state(a, b, ctx):
    for x, y, what in zip(a, b, ("header", "nodes", "order", "cache")):
        if x.dtype.names:
            for f in x.dtype.names:
                if not f.startswith("pad"):
                    np.testing.assert_array_equal(x[f], y[f], err_msg=f"{ctx}: state {what}.{f}")
        else:
            np.testing.assert_array_equal(x, y, err_msg=f"{ctx}: state {what}")


def _mixed_actions(eng, t, seed):
    """Valid actions on two steps of three, uniform (out-of-bounds included) on the third; a rotating tenth of the envs skips."""
    a = eng.sample_actions(t % 3 != 2, seed=seed, step=t)
    skip = (eng.torch.arange(eng.E, device=a.device) + t) % 10 == 0
    a[skip, 0] = SKIP
    return a


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_no_op_steps_leave_every_state_byte(name, monkeypatch):
    E, want = LAYOUTS[name]
    eng = _engine(name, _spec(name, E, max_episode_steps=1000), monkeypatch, want)
    torch = eng.torch
    for t in range(40):
        eng.step(eng.sample_actions(True, seed=11, step=t))
    before = eng.get_state()
    assert int(before[0]["n_discovered"].max()) > 1, "the warm-up discovered nothing: the state is too trivial to test"

    skip = torch.zeros((E, 5), dtype=torch.int32, device=eng.device)
    skip[:, 0] = SKIP
    for k in range(3):
        r, d = eng.step(skip)
        assert _state_bytes(eng.get_state()) == _state_bytes(before), f"{name}: skip step {k} changed the state"
        assert not r.any() and not d.any()

    oob = torch.zeros((E, 5), dtype=torch.int32, device=eng.device)
    oob[:, 1] = 255                                          # local exploit from a discovery index no env has
    r, d = eng.step(oob)
    after = eng.get_state()
    assert not r.any() and not d.any()
    for x, y, what in zip(before[1:], after[1:], ("nodes", "order", "cache")):
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), f"{name}: an out-of-bounds step changed the {what}"
    h0, h1 = before[0], after[0]
    np.testing.assert_array_equal(h1["step_count"], h0["step_count"] + 1)
    np.testing.assert_array_equal(h1["last_oob"], np.ones(E))
    for f in ("done", "truncated", "episode", "n_discovered", "n_creds", "cum_reward", "availability"):
        assert h0[f].tobytes() == h1[f].tobytes(), f"{name}: an out-of-bounds step changed header field {f}"
    eng.close()


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_steps_after_the_end_leave_every_state_byte(name, monkeypatch):
    """Without auto-reset an env that ended stays as it ended: further steps store nothing and report its flags."""
    E, want = LAYOUTS[name]
    T = 25
    eng = _engine(name, _spec(name, E, auto_reset=False, max_episode_steps=T), monkeypatch, want)
    for t in range(T):
        eng.step(eng.sample_actions(True, seed=5, step=t))
    ended = eng.get_state()
    assert (ended[0]["done"] | ended[0]["truncated"]).all(), "every env must have ended after max_episode_steps"
    for t in range(T, T + 4):
        r, d = eng.step(eng.sample_actions(t % 2 == 0, seed=5, step=t))
        assert _state_bytes(eng.get_state()) == _state_bytes(ended), f"{name}: step {t} after the end changed the state"
        assert not r.any()
        np.testing.assert_array_equal(d.cpu().numpy(), ended[0]["done"].astype(np.uint8))
    eng.close()


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_step_and_step_many_match_the_oracle_over_1000_steps(name, monkeypatch):
    from oracle.oracle import Oracle
    E, want = LAYOUTS[name]
    spec = _spec(name, E)
    eng = _engine(name, spec, monkeypatch, want)
    many = _engine(name, spec, monkeypatch)
    orc = Oracle(_topology(name), spec)
    torch = eng.torch
    T, K = 1000, 250
    ring = torch.empty((T, E, 5), dtype=torch.int32, device=eng.device)
    rewards = torch.empty((T, E), dtype=torch.float32, device=eng.device)
    dones = torch.empty((T, E), dtype=torch.uint8, device=eng.device)
    ended = 0
    for t in range(T):
        a = _mixed_actions(eng, t, seed=29)
        ring[t] = a
        r, d = eng.step(a)
        rewards[t], dones[t] = r, d
        o = orc.step(a.cpu().numpy())
        ctx = f"{name} step {t}"
        np.testing.assert_array_equal(r.double().cpu().numpy(), o["reward"], err_msg=ctx + " reward")
        np.testing.assert_array_equal(d.cpu().numpy(), o["terminated"], err_msg=ctx + " terminated")
        np.testing.assert_array_equal(eng.info["out_of_bound"].cpu().numpy(), o["oob"], err_msg=ctx + " oob")
        np.testing.assert_array_equal(eng.info["network_availability"].cpu().numpy().view(np.uint64), o["availability"].view(np.uint64),
                                      err_msg=ctx + " availability bits")
        ended += int(d.sum()) + int(eng.info["truncated"].sum())
        if t % 100 == 99:
            _assert_same_state(eng.get_state(), orc.get_state(), ctx)
    assert ended >= E, f"{name}: {ended} episode ends for {E} envs: the resets were not exercised"
    for c in range(T // K):
        r, d = many.step_many(ring[c * K:(c + 1) * K])
        assert torch.equal(r, rewards[c * K:(c + 1) * K]), f"{name}: step_many rewards differ from mcbs_step in steps {c * K}..{(c + 1) * K - 1}"
        assert torch.equal(d, dones[c * K:(c + 1) * K]), f"{name}: step_many terminated flags differ from mcbs_step"
    _assert_same_state(many.get_state(), eng.get_state(), f"{name}: step_many vs mcbs_step after {T} steps")
    _assert_same_state(eng.get_state(), orc.get_state(), f"{name}: mcbs_step vs the oracle after {T} steps")
    eng.close()
    many.close()
