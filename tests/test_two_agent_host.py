"""The two-agent turn without a GPU: its Python surface, the C struct it adds, and its bookkeeping rules (tests/episode_ref.py, the
host side of tests/test_gpu_two_agent.py) against the reference's recorded two-agent episodes."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import parity
from tests.episode_ref import EpisodeBook

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_python_surface():
    from marlon_amd import engine, simulate, wrappers
    sig = inspect.signature(simulate.run_episode_joint)
    assert list(sig.parameters) == ["att", "dfd", "attacker_policy", "defender_policy", "max_steps", "sync_every"]
    assert sig.parameters["max_steps"].default == 2000 and sig.parameters["sync_every"].default == 16
    assert "BEFORE" in simulate.run_episode_joint.__doc__ and "marl_algorithm.py:222" in simulate.run_episode_joint.__doc__
    joint = inspect.signature(simulate.simulate).parameters["joint"]
    assert joint.default is False and list(inspect.signature(simulate.simulate).parameters)[-1] == "joint"
    cls = wrappers.TwoAgentVecEnv
    assert list(inspect.signature(cls.__init__).parameters)[1:] == ["att", "dfd"]
    assert list(inspect.signature(cls.step).parameters)[1:3] == ["attacker_actions", "defender_actions"]
    assert isinstance(inspect.getattr_static(cls, "supported"), staticmethod) and callable(cls.episode_state)
    for name in ("two_agent_step_launches", "two_agent_step_call"):
        assert callable(getattr(engine.BatchEngine, name))
    with pytest.raises(ValueError, match="AttackerVecEnv"):
        cls(object(), None)
    assert cls.supported(object()) is False


def test_episode_buffers_mirror_the_header():
    from marlon_amd import _abi
    text = open(os.path.join(REPO, "include", "mcbs.h")).read()
    m = re.search(r"typedef struct mcbs_episode_buffers \{\s*/\* (\d+) bytes(.*?)\} mcbs_episode_buffers;", text, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", "/*" + m.group(2), flags=re.S)
    members = re.findall(r"(\w+)\s*\*\s*(\w+);", body)
    assert [n for _, n in members] == list(_abi.EPISODE_FIELDS) and len(re.findall(r";", body)) == len(members), "six pointers, this order"
    assert C.sizeof(_abi.EpisodeBuffers) == int(m.group(1)) == len(members) * C.sizeof(C.c_void_p)
    block = _abi.episode_buffers(**{n: 16 * (i + 1) for i, n in enumerate(_abi.EPISODE_FIELDS)})
    assert list(block) == [16 * (i + 1) for i in range(6)]
    with pytest.raises(ValueError):
        _abi.episode_buffers(alive=16)
    assert list(_abi.PROTOTYPES).index("mcbs_two_agent_step") == list(_abi.PROTOTYPES).index("mcbs_two_agent_step_launches") + 1
    assert len(_abi.PROTOTYPES["mcbs_two_agent_step"][1]) == 15


def test_launches_query_refuses_null_without_a_gpu():
    from marlon_amd import engine
    lib = engine.load_library()
    assert lib.mcbs_two_agent_step_launches(None) == 0
    assert lib.mcbs_two_agent_step(*([None] * 7), 0.0, 1, *([None] * 6)) == -1 and b"null" in lib.mcbs_last_error()


@pytest.mark.parametrize("name", ["wrap_episode_toyctf_s73", "wrap_episode_toyctf_s74", "wrap_episode_toyctf_s75"])
def test_bookkeeping_rules_reproduce_the_reference_episodes(name):
    """Fed the recorded per-step rewards and done flags — with the defender's own result of a step the attacker had ended replaced by a
    sentinel, as the device's is discarded there — the rules give the recorded traces (the -last attacker reward rule, -0.0 included),
    lengths and ended-by flags; and further turns of the finished episode book nothing."""
    z = np.load(os.path.join(parity.GOLDEN, name + ".npz"))
    ep = z["episode"]
    seen = {"attacker": 0, "defender_only": 0, "max_steps": 0}
    for e in range(int(ep.max()) + 1):
        idx = np.flatnonzero(ep == e)
        book = EpisodeBook(1)
        a_trace, d_trace = [], []
        for k, i in enumerate(idx):
            assert book.alive[0], f"{name} episode {e}: over before recorded step {k}"
            parked = book.attacker(z["a_reward"][i:i + 1], z["a_done"][i:i + 1], [0])
            assert bool(parked[0]) == bool(z["a_done"][i])
            d_raw = np.array([12345.0]) if parked[0] else z["d_reward"][i:i + 1]
            book.defender(d_raw, z["d_terminated"][i:i + 1], z["d_truncated"][i:i + 1])
            a_trace.append(book.attacker_reward[0])
            d_trace.append(book.defender_reward[0])
        ctx = f"{name} episode {e}"
        np.testing.assert_array_equal(np.array(a_trace).view(np.int64), z["a_reward"][idx].view(np.int64), err_msg=ctx)
        np.testing.assert_array_equal(np.array(d_trace).view(np.int64), z["d_reward"][idx].view(np.int64), err_msg=ctx)
        last = idx[-1]
        ended = bool(z["a_done"][last] or z["d_done"][last])              # (else the reference's loop stopped at max_steps)
        assert book.lengths[0] == len(idx) and bool(book.alive[0]) == (not ended), ctx
        assert bool(book.attacker_done[0]) == bool(z["a_done"][last]) and bool(book.defender_done[0]) == bool(z["d_done"][last]), ctx
        seen["attacker" if z["a_done"][last] else ("defender_only" if ended else "max_steps")] += 1
        if not ended:
            continue
        before = {k: v.copy() for k, v in book.arrays().items()}
        assert book.attacker([7.0], [1], [1])[0]                      # a turn of the finished episode: parked, zero rows, nothing counted
        book.defender([9.0], [1], [1])
        after = book.arrays()
        assert after["attacker_reward"][0] == 0.0 and after["defender_reward"][0] == 0.0 and not np.signbit(after["defender_reward"][0])
        for k in ("alive", "lengths", "attacker_done", "defender_done"):
            np.testing.assert_array_equal(before[k], after[k], err_msg=f"{ctx} {k}")
    assert sum(seen.values()) == int(ep.max()) + 1 and (name != "wrap_episode_toyctf_s73" or seen["attacker"] > 0)


def test_without_an_episode_block_every_env_counts_as_alive():
    book = EpisodeBook(3, track_alive=False)
    for _ in range(2):
        parked = book.attacker([1.0, 2.0, 3.0], [0, 1, 0], [0, 0, 1])
        np.testing.assert_array_equal(parked, [False, True, True])
        book.defender([5.0, 6.0, 7.0], [1, 1, 1], [0, 0, 0])
        np.testing.assert_array_equal(book.lengths, 0)
        np.testing.assert_array_equal(book.alive, True)
