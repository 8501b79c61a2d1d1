"""The two-agent training turn without a GPU: its Python surface, the C struct it adds, the NULL refusal, and its hand-shake rules
(tests/training_ref.py, the host side of tests/test_gpu_two_agent_training.py) against the reference's recorded training loops."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

from tests import parity
from tests.training_ref import TrainingBook

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TRACES = ["wrap_training_toyctf_s81", "wrap_training_toyctf_discrete_s82", "wrap_training_toyctf_s83", "wrap_training_toyctf_s84"]


def test_python_surface():
    from marlon_amd import engine, simulate, wrappers
    cls = wrappers.TwoAgentTrainVecEnv
    assert list(inspect.signature(cls.__init__).parameters)[1:] == ["att", "dfd"]
    assert list(inspect.signature(cls.step).parameters)[1:] == ["attacker_actions", "defender_actions"]
    assert isinstance(inspect.getattr_static(cls, "supported"), staticmethod) and callable(cls.reset)
    assert isinstance(inspect.getattr_static(cls, "attacker_reset_request"), property)
    assert isinstance(inspect.getattr_static(cls, "terminal_observation"), property)
    assert "must NOT be mixed" in cls.__doc__
    with pytest.raises(ValueError, match="AttackerVecEnv"):
        cls(object(), None)
    assert cls.supported(object()) is False
    for name in ("two_agent_train_step_launches", "two_agent_train_step_call"):
        assert callable(getattr(engine.BatchEngine, name))
    sig = inspect.signature(simulate.collect_rollouts)
    assert list(sig.parameters) == ["train", "attacker_policy", "defender_policy", "attacker_buffer", "defender_buffer", "n_steps"]
    assert "marl_algorithm" in simulate.collect_rollouts.__doc__
    # the joint turn that refuses an auto-resetting attacker is still there, unchanged
    assert "auto_reset=False" in inspect.getsource(wrappers.TwoAgentVecEnv._refusal)


def test_training_buffers_mirror_the_header():
    from marlon_amd import _abi
    text = open(os.path.join(REPO, "include", "mcbs.h")).read()
    m = re.search(r"typedef struct mcbs_training_buffers \{\s*/\* (\d+) bytes(.*?)\} mcbs_training_buffers;", text, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", "/*" + m.group(2), flags=re.S)
    members = re.findall(r"(\w+)\s*\*\s*(\w+);", body)
    assert [n for _, n in members] == list(_abi.TRAINING_FIELDS) and len(re.findall(r";", body)) == len(members), "pointers only, this order"
    assert C.sizeof(_abi.TrainingBuffers) == int(m.group(1)) == len(members) * C.sizeof(C.c_void_p)
    block = _abi.training_buffers(**{n: 16 * (i + 1) for i, n in enumerate(_abi.TRAINING_FIELDS)})
    assert list(block) == [16 * (i + 1) for i in range(len(members))]
    with pytest.raises(ValueError):
        _abi.training_buffers(attacker_reset_request=16)
    names = list(_abi.PROTOTYPES)
    assert names.index("mcbs_two_agent_train_step") == names.index("mcbs_two_agent_train_step_launches") + 1 == names.index("mcbs_two_agent_step") + 2
    # what mcbs_two_agent_step takes, minus the episode block, plus keep / fresh and the new struct
    assert len(_abi.PROTOTYPES["mcbs_two_agent_train_step"][1]) == len(_abi.PROTOTYPES["mcbs_two_agent_step"][1]) - 1 + 3


def test_entry_points_refuse_null_without_a_gpu():
    from marlon_amd import engine
    lib = engine.load_library()
    assert lib.mcbs_two_agent_train_step_launches(None) == 0
    assert lib.mcbs_two_agent_train_step(*([None] * 7), 0.0, 1, *([None] * 8)) == -1 and b"null" in lib.mcbs_last_error()


@pytest.mark.parametrize("name", TRACES)
def test_rules_reproduce_the_reference_training_loops(name):
    """Fed the recorded per-step results — the attacker's reward, terminated and invalid flags; the defender's validity and terminated
    flag and its reward, the latter replaced by a sentinel on a request step, where the shaped value is discarded — the rules give every
    recorded flag, the defender's reward bit pattern (the negated attacker reward, -0.0 included), every counter after the turn, both
    reset_request flags and the last_*_action_count pairs of every turn."""
    z = np.load(os.path.join(parity.GOLDEN, name + ".npz"))
    sj = json.loads(bytes(z["spec_json"]).decode())
    book = TrainingBook(1, sj["max_timesteps"], sj["defender_max_timesteps"])
    seen = dict(attacker_ended=0, defender_ended=0, request_steps=0, requested_attacker=0, negative_zero=0)
    for i in range(len(z["a_reward"])):
        ctx = f"{name} turn {i}"
        assert bool(book.request[0]) == bool(z["a_request"][i]), ctx + ": the attacker's reset_request before its step"
        a = book.attacker(z["a_reward"][i:i + 1].astype(np.float32), z["a_terminated"][i:i + 1], z["a_invalid"][i:i + 1])
        assert np.float32(z["a_reward"][i]) == z["a_reward"][i], ctx                       # (the wrapper's rewards are float32 values)
        assert bool(a["truncated"][0]) == bool(z["a_truncated"][i]) and bool(a["dones"][0]) == bool(z["a_terminated"][i] or z["a_truncated"][i]), ctx
        assert bool(a["notify"][0]) == bool(z["d_request"][i]), ctx + ": the defender's reset_request before its step"
        raw = np.array([12345.0]) if a["notify"][0] else z["d_reward"][i:i + 1]
        d = book.defender(raw, z["d_terminated"][i:i + 1], z["d_valid"][i:i + 1])
        assert d["reward"].view(np.int64)[0] == z["d_reward"][i:i + 1].view(np.int64)[0], ctx + ": the defender's reward, bit for bit"
        assert bool(d["truncated"][0]) == bool(z["d_truncated"][i]) and bool(d["terminated"][0]) == bool(z["d_terminated"][i]), ctx
        for got, want in ((book.a_timesteps, "a_timesteps"), (book.a_valid, "a_valid_count"), (book.a_invalid, "a_invalid_count"),
                          (book.a_last_valid, "a_last_valid"), (book.a_last_invalid, "a_last_invalid"), (book.d_timesteps, "d_timesteps"),
                          (book.d_valid, "d_valid_count"), (book.d_invalid, "d_invalid_count"), (book.d_last_valid, "d_last_valid"),
                          (book.d_last_invalid, "d_last_invalid")):
            assert int(got[0]) == int(z[want][i]), f"{ctx}: {want}"
        seen["attacker_ended"] += int(a["notify"][0])
        seen["defender_ended"] += int(d["dones"][0] and not d["request_step"][0])
        seen["request_steps"] += int(d["request_step"][0])
        seen["requested_attacker"] += int(a["requested"][0])
        seen["negative_zero"] += int(d["request_step"][0] and d["reward"][0] == 0.0 and np.signbit(d["reward"][0]))
    assert seen["request_steps"] == seen["attacker_ended"] and seen["requested_attacker"] in (seen["defender_ended"], seen["defender_ended"] - 1)
    assert seen["attacker_ended"] + seen["defender_ended"] >= 10, seen              # (every trace: at least ten episode ends)


def test_the_set_of_traces_holds_what_the_generator_promises():
    """The minimum counts tools/gen_golden_training.py asserts over the whole set, recounted from the committed files."""
    total = dict(attacker_ended=0, defender_ended=0, defender_terminated=0, defender_timed_out=0, intercepted=0, positive=0, timeout_meets_request=0)
    discrete = 0
    for name in TRACES:
        z = np.load(os.path.join(parity.GOLDEN, name + ".npz"))
        assert os.path.getsize(os.path.join(parity.GOLDEN, name + ".npz")) < 100 * 1024
        sj = json.loads(bytes(z["spec_json"]).decode())
        discrete += int(sj["discrete"])
        q, own = z["a_request"] != 0, ((z["d_terminated"] | z["d_truncated"]) != 0) & (z["d_request"] == 0)
        a_done = (z["a_terminated"] | z["a_truncated"]) != 0
        clock, t = np.zeros(len(q), np.int64), 0
        for i in range(len(q)):
            t += 1
            clock[i] = t
            t = 0 if a_done[i] else t
        total["attacker_ended"] += int((a_done & ~q).sum())
        total["defender_ended"] += int(own.sum())
        total["defender_terminated"] += int((own & (z["d_terminated"] != 0)).sum())
        total["defender_timed_out"] += int((own & (z["d_terminated"] == 0)).sum())
        total["intercepted"] += int((q & (z["a_invalid"] != 0)).sum())
        total["positive"] += int((q & (z["a_reward"] > 0)).sum())
        total["timeout_meets_request"] += int((q & (clock >= sj["max_timesteps"])).sum())
    need = dict(attacker_ended=10, defender_ended=10, defender_terminated=1, defender_timed_out=5, intercepted=2, positive=1, timeout_meets_request=5)
    assert discrete == 1 and all(total[k] >= v for k, v in need.items()), total
