"""The lean launch of the packed, attacker-only step (mcbs_step.hip `step_kernel(cfg, LeanStepArgs)`; mcbs_api.hip launch_step): mcbs_step
without info buffers passes the config pointer and an argument block that holds only what the kernel reads.  In that instantiation
the five optional outputs, the draw tape, the ring and the wave-level reset copy are compiled out (an env that ends is re-initialised
by its own lane from the config's reset image) and the eight sets are held in 32-bit words.  A call WITH info buffers takes the
instantiation that carries them: the full argument list, the outputs tested at run time, the sets in 64-bit words.  What can go wrong:
a word missing from the lean block or filled from the wrong field, inactive lanes of a partial wavefront, the fourth row vector
(more than 12 nodes), element 15 of a set in a narrower word, an env that resets inside the kernel several times, an ended env that
must stay as it is — and the two instantiations disagreeing.

Every case is stepped against the CPU oracle by seven engines that differ only in the info buffers they hand to mcbs_step: none (the
lean launch: asserted through mcbs_step_is_lean), all five, and each of the five alone (the full launch).  Per step: reward, terminated
and every requested info output (a buffer that was not requested must stay zero); after the run: the canonical state from get_state,
the episode counter included.

* env counts 1, 63, 64, 65, 130: inactive lanes, exactly one wavefront, one lane into the next, two wavefronts and two lanes; a non-zero
  env_id_base.
* topologies: Chain-10 with the 12 / 12 bounds (three row vectors), the 16-node leaky network of test_gpu_packed_lists.py (the fourth
  row vector, element 15 of every set), ToyCtf (another row format: tiny_p, tiny_v).
* actions, 60 steps, written on the CPU from the oracle's own state (tests/endings.py Policy: valid rows, some uniform over the bounds);
  env e at step t then gets, by (e + t) % 8: 4 an action kind outside 0..3, 5 an index that is negative as int32, 6 a connect whose
  credential index lies past the cache, 7 MCBS_ACTION_SKIP; 0..3 the policy's row.
* endings: truncation at 7 steps with auto-reset (every env resets inside the kernel several times; the counter must equal the
  oracle's) and without (the steps after the end must leave the env untouched); one goal-reached script of tests/endings.py.
"""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from tests import endings
from tests.test_gpu_packed_lists import NETS, _assert_layout, _bounds, _same_state, leaky_environment

pytestmark = pytest.mark.gpu

BASE, T, TRUNC, SKIP = 7, 60, 7, 3
INFO = (("network_availability", "availability"), ("step_count", "step_count"), ("truncated", "truncated"), ("out_of_bound", "oob"),
        ("raw_reward", "raw_reward"))
MODES = ((), tuple(m for m, _ in INFO)) + tuple((m,) for m, _ in INFO)     # none (lean), all five, each alone
INT_MIN = -2 ** 31


@functools.lru_cache(maxsize=None)
def _topology(name):
    from marlon_amd import flatten
    from marlon_amd.samples import chainpattern, toy_ctf
    if name == "chain10":
        return flatten.flatten(chainpattern.new_environment(10))
    if name == "toyctf":
        return flatten.flatten(toy_ctf.new_environment())
    return flatten.flatten(leaky_environment(*NETS["leaky16"]))


def _spec(name, E, auto_reset):
    from marlon_amd._abi import EnvSpec
    if name == "leaky16":
        kw = dict(attacker_goal=None, **_bounds("leaky16"))
    else:
        kw = dict(maximum_node_count=12, maximum_total_credentials=12 if name == "chain10" else 10)
    return EnvSpec(n_envs=E, seed=31, env_id_base=BASE, auto_reset=auto_reset, max_episode_steps=TRUNC, **kw)


def _spoil(rows, state, t, spec):
    """The rows of step t with the envs of categories 4..7 overwritten (module docstring)."""
    hdr = state[0]
    E = rows.shape[0]
    e = np.arange(E)
    cat = (e + t) % 8
    turn = (e + t) // 8
    out = rows.copy()
    bad_kind = np.array([4, 7, -1, 1000, INT_MIN, 2 ** 31 - 1], np.int64)[turn % 6]
    out[:, 0] = np.where(cat == 4, bad_kind, out[:, 0])
    neg = np.array([-1, INT_MIN, -17], np.int64)[turn % 3]
    for col in (1, 2, 3, 4):
        out[:, col] = np.where((cat == 5) & (turn % 4 == col - 1), neg, out[:, col])
    out[:, 0] = np.where((cat == 5) & (turn % 4 == 3), 2, out[:, 0])                 # (only a connect reads its credential index)
    past = hdr["n_creds"].astype(np.int64) + np.array([0, 1, int(spec.maximum_total_credentials), 2 ** 20], np.int64)[turn % 4]
    out[:, 0] = np.where(cat == 6, 2, out[:, 0])
    out[:, 4] = np.where(cat == 6, past, out[:, 4])
    out[:, 0] = np.where(cat == 7, SKIP, out[:, 0])
    return out.astype(np.int32)


def _record(topo, spec, script_of):
    """(script [T, E, 5], the oracle's outputs per step, its final state); script_of(t, oracle state) -> rows."""
    from oracle.oracle import Oracle
    orc = Oracle(topo, spec)
    script, outs = [], []
    for t in range(10 ** 6):
        rows = script_of(t, orc.get_state())
        if rows is None:
            break
        script.append(rows)
        outs.append(orc.step(rows))
    return np.stack(script), outs, orc.get_state()


@functools.lru_cache(maxsize=None)
def _reference(name, E, auto_reset):
    """Computed once per case, shared by nothing else and never changed."""
    topo, spec = _topology(name), _spec(name, E, auto_reset)
    pol = endings.Policy(topo, spec, seed=1000 + E)

    def script_of(t, state):
        return _spoil(pol.rows(state), state, t, spec) if t < T else None

    script, outs, final = _record(topo, spec, script_of)
    kinds = script[:, :, 0]
    ended = np.stack([(o["terminated"] != 0) | (o["truncated"] != 0) for o in outs])
    assert (kinds == SKIP).any() and ((kinds < 0) | (kinds > 3)).any() and (script[:, :, 1:] < 0).any()
    assert any(o["oob"].any() for o in outs) and any((o["raw_reward"] == -1.0).any() for o in outs)
    assert any((o["raw_reward"] > 0.0).any() for o in outs), "no action of the script succeeds"
    if auto_reset:
        assert (final[0]["episode"] >= 4).all(), "every env must have been reset inside the kernel several times"
        assert sum(o["errors"] for o in outs) == 0
    else:
        assert ended[-1].all() and (final[0]["episode"] == 0).all() and sum(o["errors"] for o in outs) > 0, "every env ends and is stepped on"
    return topo, spec, script, outs, final


@functools.lru_cache(maxsize=None)
def _goal_reference():
    """A script of tests/endings.py whose episodes end because the attacker's reward goal is reached (no defender: the lean kernel's batch)."""
    case = endings.case("toyctf-reward")
    script, outs, final = _record(case.topo, case.spec, lambda t, state: case.actions[t] if t < case.actions.shape[0] else None)
    for k in endings.OUT_KEYS:
        np.testing.assert_array_equal(np.stack([o[k] for o in outs]), case.out[k], err_msg=f"replaying the script: {k}")
    assert case.spec.defender is None and case.envs_by_reason()["goal"][0] >= 8
    return case.topo, case.spec, script, outs, final


def _run(topo, spec, script, outs, final, what):
    from marlon_amd import engine
    from marlon_amd._abi import InfoBuffers
    for mode in MODES:
        eng = engine.BatchEngine(topo, dataclasses.replace(spec))
        _assert_layout(eng, "packed")
        assert eng.variant()["defender_kind"] == 0
        assert eng.step_is_lean(False) and not eng.step_is_lean(True), "a packed, attacker-only batch: lean without info buffers, full with them"
        torch = eng.torch
        info = InfoBuffers(**{m: eng.info[m].data_ptr() for m in mode}) if mode else None
        acts = torch.as_tensor(script, dtype=torch.int32, device=eng.device).contiguous()
        for t, o in enumerate(outs):
            rc = eng.lib.mcbs_step(eng._h, acts[t].data_ptr(), eng.reward.data_ptr(), eng.terminated.data_ptr(),
                                   C.byref(info) if info is not None else None, eng._stream())
            assert rc == 0, eng.lib.mcbs_last_error().decode()
            ctx = f"{what}, info {mode or 'none'}, step {t}"
            np.testing.assert_array_equal(eng.reward.double().cpu().numpy(), o["reward"], err_msg=ctx + ": reward")
            np.testing.assert_array_equal(eng.terminated.cpu().numpy(), o["terminated"], err_msg=ctx + ": terminated")
            for mine, theirs in INFO:
                got = eng.info[mine].cpu().numpy()
                if mine not in mode:
                    assert not got.any(), f"{ctx}: info {mine} was written without being requested"
                    continue
                want = o[theirs]
                if mine == "network_availability":
                    got, want = got.view(np.uint64), want.view(np.uint64)
                np.testing.assert_array_equal(got.astype(np.float64) if mine == "raw_reward" else got, want, err_msg=f"{ctx}: info {mine}")
        _same_state(eng.get_state(), final, f"{what}, info {mode or 'none'}, final state")
        eng.close()


@pytest.mark.parametrize("auto_reset", [True, False], ids=["autoreset", "frozen"])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("name", ["chain10", "leaky16", "toyctf"])
def test_lean_and_info_launches_against_the_oracle(name, E, auto_reset):
    topo, spec, script, outs, final = _reference(name, E, auto_reset)
    assert (topo.n_nodes > 12) == (name == "leaky16"), "only the leaky network needs the fourth row vector"
    _run(topo, spec, script, outs, final, f"{name}, {E} envs, {'auto-reset' if auto_reset else 'no auto-reset'}")


def test_goal_reached_script():
    topo, spec, script, outs, final = _goal_reference()
    _run(topo, spec, script, outs, final, "toyctf-reward")
