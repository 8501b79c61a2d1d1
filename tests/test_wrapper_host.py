"""The two-agent classes' refusal lists without a GPU and without the library: `TwoAgentVecEnv._refusal` and
`TwoAgentTrainVecEnv._refusal` walked on bare wrapper objects, one condition violated at a time and two at a time.  Every expected text
is a literal: a user who was refused with these words keeps being refused with them, in this order of precedence."""
import itertools
import types

import pytest

from marlon_amd import wrappers
from marlon_amd._abi import DEFENDER_EXTERNAL, DEFENDER_NONE

TURNS = {
    "joint": dict(
        cls=wrappers.TwoAgentVecEnv, auto_reset=False,
        auto_reset_text="the AttackerVecEnv must be created with auto_reset=False (the episode boundary belongs to the caller)",
        masks_text="the AttackerVecEnv must be created with materialize_masks=False (the joint turn writes no mask field)",
        format_text="the AttackerVecEnv must be created with observation_format='fields' (the joint turn writes the int32 fields, not packed rows)",
        launches="two_agent_step_launches",
        launches_text="the library does not serve this batch with a joint turn (mcbs_two_agent_step_launches: small packed topologies only)"),
    "training": dict(
        cls=wrappers.TwoAgentTrainVecEnv, auto_reset=True,
        auto_reset_text="the AttackerVecEnv must be created with auto_reset=True (both agents' DummyVecEnv resets are part of the training turn)",
        masks_text="the AttackerVecEnv must be created with materialize_masks=False (the training turn writes no mask field)",
        format_text="the AttackerVecEnv must be created with observation_format='fields' (the training turn writes the int32 fields, not packed rows)",
        launches="two_agent_train_step_launches",
        launches_text="the library does not serve this batch with a training turn (mcbs_two_agent_train_step_launches: small packed topologies only)"),
}
DEFENDER_TEXT = "the defender side must be the DefenderVecEnv created on this AttackerVecEnv (use_graph=False)"
DEFENDER_FORMAT_TEXT = "the DefenderVecEnv must be created with observation_format='dense' (these turns write the int8 fields, not packed rows)"


def accepted_pair(turn):
    """A bare attacker / defender pair (no engine behind them) that the turn's list accepts."""
    att = object.__new__(wrappers.AttackerVecEnv)
    att.engine = types.SimpleNamespace(_cfg=types.SimpleNamespace(defender_kind=DEFENDER_EXTERNAL), two_agent_step_launches=lambda: 1,
                                       two_agent_train_step_launches=lambda: 1)
    att.auto_reset, att.materialize_masks, att.use_graph, att.observation_format = turn["auto_reset"], False, False, "fields"
    dfd = object.__new__(wrappers.DefenderVecEnv)
    dfd.attacker, dfd.use_graph, dfd.observation_format = att, False, "dense"
    return att, dfd


def violations(turn):
    """[(what, violate(att, dfd) -> (att, dfd), expected text, needs a defender)] in the list's order: nine conditions, the eighth
    (three ways to hand in a wrong defender) three times."""
    def swap_att(att, dfd):
        return object(), dfd

    def kind(att, dfd):
        att.engine._cfg.defender_kind = DEFENDER_NONE
        return att, dfd

    def auto_reset(att, dfd):
        att.auto_reset = not turn["auto_reset"]
        return att, dfd

    def masks(att, dfd):
        att.materialize_masks = True
        return att, dfd

    def graph(att, dfd):
        att.use_graph = True
        return att, dfd

    def fmt(att, dfd):
        att.observation_format = "packed"
        return att, dfd

    def launches(att, dfd):
        setattr(att.engine, turn["launches"], lambda: 0)
        return att, dfd

    def not_a_defender(att, dfd):
        return att, types.SimpleNamespace()

    def other_attacker(att, dfd):
        dfd.attacker = accepted_pair(turn)[0]
        return att, dfd

    def defender_graph(att, dfd):
        dfd.use_graph = True
        return att, dfd

    def defender_fmt(att, dfd):
        dfd.observation_format = "packed"
        return att, dfd

    return [("attacker type", swap_att, "the attacker side must be an AttackerVecEnv", False),
            ("defender kind", kind, "the AttackerVecEnv must be created with learned_defender=True", False),
            ("auto_reset", auto_reset, turn["auto_reset_text"], False),
            ("materialize_masks", masks, turn["masks_text"], False),
            ("use_graph", graph, "the AttackerVecEnv must be created with use_graph=False", False),
            ("observation_format", fmt, turn["format_text"], False),
            ("launches", launches, turn["launches_text"], False),
            ("defender type", not_a_defender, DEFENDER_TEXT, True),
            ("defender of another attacker", other_attacker, DEFENDER_TEXT, True),
            ("defender use_graph", defender_graph, DEFENDER_TEXT, True),
            ("defender observation_format", defender_fmt, DEFENDER_FORMAT_TEXT, True)]


@pytest.mark.parametrize("name", sorted(TURNS))
def test_each_condition_alone(name):
    turn = TURNS[name]
    cls = turn["cls"]
    att, dfd = accepted_pair(turn)
    assert cls._refusal(att) is None and cls._refusal(att, None) is None and cls._refusal(att, dfd) is None
    assert cls.supported(att) is True
    assert isinstance(cls.__dict__["_refusal"], staticmethod) and isinstance(cls.__dict__["supported"], staticmethod)
    for what, violate, text, needs_defender in violations(turn):
        att, dfd = violate(*accepted_pair(turn))
        assert cls._refusal(att, dfd) == text, f"{name}: {what}"
        # without a defender the two defender conditions are not asked
        assert cls._refusal(att) == (None if needs_defender else text), f"{name}: {what}, dfd=None"
        assert cls.supported(att) is needs_defender, f"{name}: {what}"
        with pytest.raises(ValueError) as err:
            cls(att, dfd)
        assert str(err.value) == f"{cls.__name__}: {text}", f"{name}: {what}"


@pytest.mark.parametrize("name", sorted(TURNS))
def test_the_earlier_condition_wins(name):
    turn = TURNS[name]
    cls = turn["cls"]
    rows = violations(turn)
    pairs = 0
    for (i, first), (j, second) in itertools.combinations(enumerate(rows), 2):
        if i == 0 or first[2] == second[2]:                 # (an object() attacker has nothing further to violate; same text: no order to see)
            continue
        att, dfd = second[1](*first[1](*accepted_pair(turn)))
        assert cls._refusal(att, dfd) == first[2], f"{name}: {first[0]} and {second[0]}"
        if not first[3]:
            assert cls._refusal(att) == first[2], f"{name}: {first[0]} and {second[0]}, dfd=None"
        pairs += 1
    assert pairs == 42


def test_the_two_lists_differ_only_where_the_turns_do():
    joint, training = violations(TURNS["joint"]), violations(TURNS["training"])
    differing = [a[0] for a, b in zip(joint, training) if a[2] != b[2]]
    assert differing == ["auto_reset", "materialize_masks", "observation_format", "launches"]
