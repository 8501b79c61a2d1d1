"""The narrow lean step kernel (mcbs_step.hip `step_kernel(cfg, NarrowStepArgs)`): the lean launch of the packed, attacker-only step
instantiated for topologies without privilege escalations, lateral-move exploits, preconditions and multi-entry leaks, with those
rules compiled out.  mcbs_batch_create picks it from the topology's traits (MCBS_TOPO_*, found on the host); a
topology with any of them keeps the general lean kernel.  What can go wrong: a trait derived wrongly, so that a batch whose topology
CAN escalate (move laterally, fail a precondition, leak two entries) runs the code without that rule; the narrow forms themselves —
the single predicated leak entry, the privilege change from NoAccess alone — disagreeing with the reference; the fourth row vector of
a 13-node topology; inactive lanes of a partial wavefront; an env that resets inside the kernel.

Every case is stepped against the CPU oracle, bit for bit: reward and terminated per step, the canonical state (get_state, the episode
counter included) half way and at the end.

* env counts 1, 63, 64, 65, 130; 60 steps; truncation at 20 steps with auto-reset, so every env ends and is re-initialised inside the run.
* actions are seeded: about a third of the rows come from tests/endings.py Policy (valid rows written from the oracle's own state), the
  rest are arbitrary — kinds outside 0..3, MCBS_ACTION_SKIP, node / vulnerability / port indices below zero and past every bound,
  credential indices outside the cache.
* topologies: Chain-10 (must report the narrow kernel); the hand-made networks of tests/topo_traits_nets.py that each switch on exactly
  one trait and their base network (no trait: narrow); ToyCtf attacker-only, whichever it gets.  A network with an escalation, a
  lateral-move exploit, a false precondition or a two-entry leak must report that it did NOT take the narrow kernel.  The 13-node
  network reports its trait and takes the narrow kernel all the same: "at most 12 nodes" was measured not to pay
  (profiles/step_topo_traits.md), so the narrow kernel does not assume it and still handles the fourth row vector — checked here.
* Chain-10 again with all five info buffers (the full launch, general code): the same rewards and flags as the call without.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import endings
from tests.test_gpu_packed_lists import _assert_layout, _same_state
from tests.topo_traits_nets import HANDMADE, NARROW_CAN, describe, handmade, traits_of

pytestmark = pytest.mark.gpu

T, TRUNC, SKIP = 60, 20, 3
ENVS = [1, 63, 64, 65, 130]
TOPOLOGIES = ["chain10", "toyctf"] + sorted(HANDMADE)
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def _environment(name):
    from marlon_amd.samples import chainpattern, toy_ctf
    if name == "chain10":
        return chainpattern.new_environment(10)
    if name == "toyctf":
        return toy_ctf.new_environment()
    return handmade(name)


@functools.lru_cache(maxsize=None)
def _topology(name):
    from marlon_amd import flatten
    return flatten.flatten(_environment(name))


def _spec(name, E):
    from marlon_amd._abi import EnvSpec
    topo = _topology(name)
    if name in ("chain10", "toyctf"):
        kw = dict(maximum_node_count=12, maximum_total_credentials=12 if name == "chain10" else 10)
    else:
        kw = dict(maximum_node_count=topo.n_nodes, maximum_total_credentials=4, attacker_goal=None)
    return EnvSpec(n_envs=E, seed=77, env_id_base=5, auto_reset=True, max_episode_steps=TRUNC, **kw)


def _arbitrary(rng, E, spec):
    """Rows nobody checked: every column from a mix of small in-range values, values just outside a bound and extreme ones."""
    far = np.array([-1, -2, INT_MIN, INT_MAX, 2 ** 20, int(spec.maximum_node_count), int(spec.maximum_node_count) + 3,
                    int(spec.maximum_total_credentials), 15, 16, 17, 255], np.int64)
    rows = np.empty((E, 5), np.int64)
    rows[:, 0] = np.where(rng.random(E) < 0.8, rng.integers(0, 4, E), np.array([-1, 4, 7, 1000, INT_MIN, INT_MAX], np.int64)[rng.integers(0, 6, E)])
    for col in (1, 2, 3, 4):
        small = rng.integers(0, 8 if col != 4 else 4, E)
        rows[:, col] = np.where(rng.random(E) < 0.7, small, far[rng.integers(0, far.size, E)])
    return rows.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _reference(name, E):
    """(topology, spec, script [T, E, 5], the oracle's outputs per step, its state after T / 2 and after T steps); computed once per
    case and never changed."""
    from oracle.oracle import Oracle
    topo, spec = _topology(name), _spec(name, E)
    orc = Oracle(topo, spec)
    pol = endings.Policy(topo, spec, seed=500 + E)
    rng = np.random.Generator(np.random.PCG64(9000 + E))
    script, outs, mid = [], [], None
    for t in range(T):
        valid = pol.rows(orc.get_state())
        rows = np.where((rng.random(E) < 1.0 / 3.0)[:, None], valid, _arbitrary(rng, E, spec)).astype(np.int32)
        script.append(rows)
        outs.append(orc.step(rows))
        if t == T // 2 - 1:
            mid = orc.get_state()
    script = np.stack(script)
    final = orc.get_state()
    kinds = script[:, :, 0]
    assert (kinds == SKIP).any() and ((kinds < 0) | (kinds > 3)).any() and (script[:, :, 1:] < 0).any() and (script[:, :, 1:] > 15).any()
    assert (final[0]["episode"] >= 2).all(), "every env ends by truncation and is reset inside the run"
    if E >= 63:
        assert any(o["oob"].any() for o in outs) and any((o["raw_reward"] == -1.0).any() for o in outs)
        assert any((o["raw_reward"] > 0.0).any() for o in outs), "no action of the script succeeds"
        assert any((o["reward"] != 0).any() for o in outs)
    return topo, spec, script, outs, mid, final


def _step_through(eng, script, outs, mid, final, info, ctx):
    """Step the script; per step reward / terminated against the oracle; state half way and at the end.  Returns the rewards and flags."""
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
        if t == len(outs) // 2 - 1:
            _same_state(eng.get_state(), mid, f"{ctx}, state after {t + 1} steps")
    _same_state(eng.get_state(), final, f"{ctx}, final state")
    return np.stack(rewards), np.stack(flags)


@pytest.mark.parametrize("E", ENVS)
@pytest.mark.parametrize("name", TOPOLOGIES)
def test_step_against_the_oracle_on_the_kernel_the_traits_choose(name, E):
    from marlon_amd import engine
    topo, spec, script, outs, mid, final = _reference(name, E)
    want = traits_of(_environment(name))
    eng = engine.BatchEngine(topo, spec)
    try:
        _assert_layout(eng, "packed")
        assert eng.step_is_lean(False) and not eng.step_is_lean(True)
        narrow, traits = eng.step_topo_traits(False)
        assert traits == want, f"{name}: the batch reports {describe(traits)}, the model objects give {describe(want)}"
        assert narrow == (not traits & ~NARROW_CAN), f"{name} ({describe(traits)}): narrow kernel {'taken' if narrow else 'not taken'}"
        assert eng.step_topo_traits(True) == (False, traits), "a call with info buffers never takes the narrow kernel"
        if name == "chain10":
            assert narrow, "Chain-10, the headline, runs the narrow kernel"
        elif name in HANDMADE and name != "base":
            assert traits == HANDMADE[name]
            assert narrow == (name == "nodes13"), "a network with a rule the narrow kernel compiled out keeps the general lean kernel"
        _step_through(eng, script, outs, mid, final, None, f"{name}, {E} envs, {'narrow' if narrow else 'general lean'} kernel")
    finally:
        eng.close()


@pytest.mark.parametrize("E", ENVS)
def test_chain10_with_info_buffers_gives_the_same_rewards_and_flags(E):
    from marlon_amd import engine
    from marlon_amd._abi import InfoBuffers
    topo, spec, script, outs, mid, final = _reference("chain10", E)
    got = []
    for with_info in (False, True):
        eng = engine.BatchEngine(topo, spec)
        try:
            assert eng.step_topo_traits(with_info)[0] == (not with_info)
            info = InfoBuffers(**{m: eng.info[m].data_ptr() for m in ("network_availability", "step_count", "truncated", "out_of_bound",
                                                                      "raw_reward")}) if with_info else None
            got.append(_step_through(eng, script, outs, mid, final, info, f"chain10, {E} envs, {'with' if with_info else 'without'} info buffers"))
        finally:
            eng.close()
    np.testing.assert_array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32), err_msg="rewards of the two launches")
    np.testing.assert_array_equal(got[0][1], got[1][1], err_msg="terminated flags of the two launches")
