"""The narrow lean step kernel's argument list (marlon_amd/csrc/mcbs_step_narrow_tu.hip): the level-1 block as eight scalar / pointer
parameters that gfx950 preloads into SGPRs, the fourth row vector decided from the body stride instead of the node count, the config
pointer and the rest behind them; the kernel is built in a translation unit of its own and launched through a host function of that
unit.  Results must be what they were.  What can go wrong: an argument in the wrong slot; an inactive lane's clamp reading another
argument (1 and 65 envs); the fourth row vector missing for 13 nodes; a config word taken from another batch or baked stale into a
captured graph (the main path's config words as kernel arguments were built and measured with these tests, and left out:
profiles/step_arg_preload.md); a reset that reads a word which no longer travels.

* oracle parity, bit for bit — reward and terminated per step, the canonical state half way and at the end — at 1, 64 and 65 envs on
  Chain-10, ToyCtf and the hand-made 13-node network; the scripts are tests/test_gpu_step_narrow.py's (60 seeded steps, a third valid,
  truncation at 20 with auto-reset, so every env is reset inside the run); all three topologies must report the narrow kernel;
* graph replay: 8 steps of Chain-10 at 65 envs captured as one graph and replayed twice from rewind() equal the eager run;
* two batches of one topology with different max_episode_steps, auto_reset, goal and winning reward, stepped alternately, each follow
  their own oracle (no entry point changes a config word after creation);
* the same Chain-10 scripts with all five info buffers take the full launch (general code): rewards as bit patterns, flags and the
  final state equal the narrow run's.
"""
import dataclasses
import functools

import numpy as np
import pytest

from tests.test_gpu_packed_lists import _assert_layout, _same_state
from tests.test_gpu_step_narrow import _reference, _step_through

pytestmark = pytest.mark.gpu

ENVS = [1, 64, 65]
TOPOLOGIES = ["chain10", "toyctf", "nodes13"]
GRAPH_STEPS = 8


@pytest.mark.parametrize("E", ENVS)
@pytest.mark.parametrize("name", TOPOLOGIES)
def test_narrow_kernel_against_the_oracle(name, E):
    from marlon_amd import engine
    topo, spec, script, outs, mid, final = _reference(name, E)
    assert (topo.n_nodes > 12) == (name == "nodes13"), "nodes13 alone needs the fourth row vector"
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
    topo, spec, script, outs, _, _ = _reference("chain10", E)
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


@functools.lru_cache(maxsize=None)
def _two_settings():
    """Chain-10 at 65 envs under two settings, one script: (topology, script, (spec, the oracle's outputs, its final state) x 2)."""
    from oracle.oracle import Oracle
    topo, spec_a, script, outs_a, _, final_a = _reference("chain10", 65)
    spec_b = dataclasses.replace(spec_a, max_episode_steps=7, auto_reset=False, winning_reward=321.0,
                                 attacker_goal=dict(reward=0.0, low_availability=1.0, own_atleast=2, own_atleast_percent=0.0))
    orc = Oracle(topo, spec_b)
    outs_b = [orc.step(rows) for rows in script]
    final_b = orc.get_state()
    assert any((o["reward"] == 321.0).any() for o in outs_b) and not any((o["reward"] == 321.0).any() for o in outs_a), "only b wins, and early"
    assert any(o["truncated"].any() for o in outs_b[:8]) and not any(o["truncated"].any() for o in outs_a[:8]), "only b truncates at 7"
    assert (final_b[0]["episode"] == 0).all() and (final_a[0]["episode"] >= 2).all(), "only a resets by itself"
    return topo, script, ((spec_a, outs_a, final_a), (spec_b, outs_b, final_b))


def test_two_batches_follow_their_own_config_words():
    from marlon_amd import engine
    topo, script, settings = _two_settings()
    engs = [engine.BatchEngine(topo, spec) for spec, _, _ in settings]
    try:
        torch = engs[0].torch
        acts = torch.as_tensor(script, dtype=torch.int32, device=engs[0].device).contiguous()
        for eng in engs:
            assert eng.step_topo_traits(False)[0]
        for t in range(script.shape[0]):
            for which, (eng, (_, outs, _)) in enumerate(zip(engs, settings)):
                rc = eng.lib.mcbs_step(eng._h, acts[t].data_ptr(), eng.reward.data_ptr(), eng.terminated.data_ptr(), None, eng._stream())
                assert rc == 0, eng.lib.mcbs_last_error().decode()
                np.testing.assert_array_equal(eng.reward.cpu().numpy().astype(np.float64), outs[t]["reward"], err_msg=f"batch {'ab'[which]}, step {t}: reward")
                np.testing.assert_array_equal(eng.terminated.cpu().numpy(), outs[t]["terminated"], err_msg=f"batch {'ab'[which]}, step {t}: terminated")
        for which, (eng, (_, _, final)) in enumerate(zip(engs, settings)):
            _same_state(eng.get_state(), final, f"batch {'ab'[which]}: final state")
    finally:
        for eng in engs:
            eng.close()


@pytest.mark.parametrize("E", ENVS)
def test_full_launch_with_info_buffers_equals_the_narrow_run(E):
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
            got.append(_step_through(eng, script, outs, mid, final, info, f"chain10, {E} envs, {'with' if with_info else 'without'} info buffers")
                       + (eng.get_state(),))
        finally:
            eng.close()
    np.testing.assert_array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32), err_msg="rewards of the two launches, as bit patterns")
    np.testing.assert_array_equal(got[0][1], got[1][1], err_msg="terminated flags of the two launches")
    _same_state(got[0][2], got[1][2], f"chain10, {E} envs: final state of the two launches")
