"""The two-agent training turn that writes both observations as packed rows (mcbs_two_agent_train_step_packed), without a GPU: the C
struct it adds against its Python mirror, the NULL refusals, and the Python surface, which keeps its signatures."""
import ctypes as C
import inspect
import os
import re

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def header_struct(name):
    """-> (stated size, [(C type, member)]) of `typedef struct name { /* n bytes ... */ ... } name;` of include/mcbs.h"""
    text = open(os.path.join(REPO, "include", "mcbs.h")).read()
    m = re.search(r"typedef struct %s \{\s*/\* (\d+) bytes(.*?)\} %s;" % (name, name), text, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", "/*" + m.group(2), flags=re.S)
    members = re.findall(r"(\w+)\s*\*\s*(\w+);", body)
    assert len(re.findall(r";", body)) == len(members), f"{name}: pointers only"
    return int(m.group(1)), members


def test_training_packed_buffers_mirror_the_header():
    from marlon_amd import _abi
    size, members = header_struct("mcbs_training_packed_buffers")
    assert [n for _, n in members] == list(_abi.TRAINING_PACKED_FIELDS), "these members in this order"
    assert C.sizeof(_abi.TrainingPackedBuffers) == size == len(members) * C.sizeof(C.c_void_p) == 88
    # the first nine members are mcbs_training_buffers' first nine, type for type; then the two packed arrays
    _, dense = header_struct("mcbs_training_buffers")
    assert members[:9] == dense[:9] and [n for _, n in members[:9]] == list(_abi.TRAINING_FIELDS[:9])
    assert members[9:] == [("uint32_t", "terminal_defender_packed"), ("uint32_t", "fresh_defender_packed")]
    block = _abi.training_packed_buffers(**{n: 16 * (i + 1) for i, n in enumerate(_abi.TRAINING_PACKED_FIELDS)})
    assert list(block) == [16 * (i + 1) for i in range(len(members))]
    with pytest.raises(ValueError):
        _abi.training_packed_buffers(attacker_reset_request=16)
    with pytest.raises(ValueError):                                           # the dense block's members are not this block's
        _abi.training_packed_buffers(**{n: 16 for n in _abi.TRAINING_FIELDS})
    names = list(_abi.PROTOTYPES)
    i = names.index("mcbs_two_agent_train_step")
    assert names[i + 1:i + 3] == ["mcbs_two_agent_train_step_packed_launches", "mcbs_two_agent_train_step_packed"]
    # batch, two encodings, decoded, info | packing, packed, terminal, fresh, row_words | w, modifier, timesteps | defender actions, rows,
    # row_words, dw, dcfg | the block, the stream
    assert len(_abi.PROTOTYPES["mcbs_two_agent_train_step_packed"][1]) == 5 + 5 + 3 + 5 + 2
    assert _abi.PROTOTYPES["mcbs_two_agent_train_step_packed"][1][9] is C.c_size_t and _abi.PROTOTYPES["mcbs_two_agent_train_step_packed"][1][15] is C.c_size_t


def test_entry_points_refuse_null_without_a_gpu():
    from marlon_amd import engine
    lib = engine.load_library()
    assert lib.mcbs_two_agent_train_step_packed_launches(None, None) == 0
    rc = lib.mcbs_two_agent_train_step_packed(*([None] * 9), 0, None, 0.0, 1, None, None, 0, None, None, None, None)
    assert rc == -1 and b"null" in lib.mcbs_last_error()


def test_python_surface():
    from marlon_amd import engine, simulate, wrappers
    cls = wrappers.TwoAgentTrainVecEnv
    assert list(inspect.signature(cls.__init__).parameters)[1:] == ["att", "dfd"]
    assert list(inspect.signature(cls.step).parameters)[1:] == ["attacker_actions", "defender_actions"]
    assert "observation_format=\"packed\"" in cls.__doc__ and "mixed pair" in cls.__doc__
    assert "observation_format=\"packed\"" in cls.supported.__doc__
    for name in ("two_agent_train_step_packed_launches", "two_agent_train_step_packed_call"):
        assert callable(getattr(engine.BatchEngine, name))
    assert list(inspect.signature(engine.BatchEngine.two_agent_train_step_packed_launches).parameters)[1:] == ["packing"]
    assert "no pack kernel is launched on either side" in " ".join(simulate.collect_rollouts.__doc__.split())
    # the joint turn still refuses both packed forms: it has no packed entry point to ask
    src = inspect.getsource(wrappers.TwoAgentVecEnv._refusal)
    assert "auto_reset=False" in src and "packed_launches" not in src
    assert "packed_launches=" in inspect.getsource(cls._refusal)
