"""The host side of the four wrapper classes' `step` (marlon_amd/wrappers.py over the bound calls of marlon_amd/engine.py): what the
caller may hand in as actions, what a wrong shape does, how long a step's outputs live, separate and joint turns on one pair, and a
bound call after `engine.close()`.  Small batches — 3 envs (a partial wavefront) and 65 (one env past a 64-env workgroup) of Chain-4 at
6 nodes / 6 credentials, at most 12 turns — and every comparison is bit for bit against a twin stepped with a contiguous int64 device
tensor."""
import numpy as np
import pytest

from tests import parity
from tests.test_gpu_two_agent import assert_same, bits, defender_actions, md_rows, snapshot

pytestmark = pytest.mark.gpu

TOPO, NODES, CREDS = "chain4", 6, 6
SIZES = (3, 65)
TURNS = 12
FORMS = ("list", "numpy int32", "cpu int64", "strided view")


def attacker(E, **kw):
    from marlon_amd.wrappers import AttackerVecEnv
    args = dict(maximum_node_count=NODES, maximum_total_credentials=CREDS, max_timesteps=7, materialize_masks=False, seed=3)
    args.update(kw)
    return AttackerVecEnv(parity.topology_for(TOPO), E, **args)


def pair(E, auto_reset, dfd_kw=None, **kw):
    from marlon_amd.wrappers import DefenderVecEnv
    att = attacker(E, learned_defender=True, discrete=True, auto_reset=auto_reset, **kw)
    return att, DefenderVecEnv(att, max_timesteps=5, invalid_action_reward=-1, **(dfd_kw or {}))


def in_form(form, a, dev):
    """the int64 host array `a` the way a caller might hand it in"""
    import torch as t
    if form == "list":
        return a.tolist()
    if form == "numpy int32":
        return a.astype(np.int32)
    if form == "cpu int64":
        return t.as_tensor(a)
    if form == "strided view":
        v = t.stack([t.as_tensor(a, device=dev), t.full(a.shape, -7, dtype=t.int64, device=dev)], dim=-1)[..., 0]
        assert v.dtype == t.int64 and v.is_cuda and not v.is_contiguous()
        return v
    raise KeyError(form)


def attacker_actions(att, rng, turn):
    """odd turns: uniformly random indices (mostly intercepted); even turns: valid ones for the state `att` is in"""
    if turn % 2 == 1:
        return (rng.random(att._action_shape) * (att.discrete_n if att.discrete else att.nvec)).astype(np.int64)
    if att.discrete:
        return att.sample_masked_uniform(seed=11, step=turn).actions.cpu().numpy()
    return md_rows(att.engine.sample_actions(valid=True, seed=11, step=turn).cpu().numpy().astype(np.int64))


def attacker_side(att, out):
    obs, r, term, trunc, info = out
    s = {"rewards": r, "terminated": term, "truncated": trunc, "rows": att._rows, "timesteps": att.timesteps, "dones": att._dones}
    s.update({"info." + k: v for k, v in info.items()})
    s.update({"obs." + k: v for k, v in obs.items()})
    s.update({"terminal." + k: v for k, v in att.terminal_observation.items()})
    return {k: bits(v) for k, v in s.items()}


def defender_side(dfd, out):
    obs, r, term, trunc, info = out
    s = {"reward": r, "terminated": term, "truncated": trunc, "timesteps": dfd.timesteps, "evicted": dfd._evicted}
    s.update({"info." + k: v for k, v in info.items()})
    s.update({"obs." + k: v for k, v in obs.items()})
    return {k: bits(v) for k, v in s.items()}


ATTACKER_KINDS = {
    "fields discrete": dict(discrete=True),
    "fields multidiscrete": dict(discrete=False),
    "fields discrete with masks": dict(discrete=True, materialize_masks=True),
    "packed discrete": dict(discrete=True, observation_format="packed"),
    "packed multidiscrete": dict(discrete=False, observation_format="packed"),
}


@pytest.mark.parametrize("E", SIZES)
@pytest.mark.parametrize("kind", sorted(ATTACKER_KINDS))
def test_attacker_step_takes_every_action_form(kind, E):
    import torch as t
    twin, env = attacker(E, **ATTACKER_KINDS[kind]), attacker(E, **ATTACKER_KINDS[kind])
    dev, rng = env.engine.device, np.random.default_rng(E)
    ended = 0
    for turn in range(1, TURNS + 1):
        a = attacker_actions(twin, rng, turn)
        form = FORMS[turn % len(FORMS)]
        want = attacker_side(twin, twin.step(t.as_tensor(a, device=dev)))
        assert_same(want, attacker_side(env, env.step(in_form(form, a, dev))), f"{kind} E={E} turn {turn} ({form})")
        ended += int(want["dones"].sum())
    assert ended >= E, "every env reached the wrapper's time limit and was reset"
    twin.close()
    env.close()


@pytest.mark.parametrize("E", SIZES)
@pytest.mark.parametrize("kind", ["fields discrete", "packed multidiscrete"])
def test_attacker_step_under_use_graph(kind, E):
    """the actions are copied into `action_buffer`; handed the buffer itself, the step reads what the caller wrote there"""
    import torch as t
    twin, env = attacker(E, **ATTACKER_KINDS[kind]), attacker(E, use_graph=True, **ATTACKER_KINDS[kind])
    dev, rng = env.engine.device, np.random.default_rng(E)
    assert env.action_buffer.dtype == t.int64 and tuple(env.action_buffer.shape) == env._action_shape
    for turn in range(1, TURNS + 1):
        a = attacker_actions(twin, rng, turn)
        want = attacker_side(twin, twin.step(t.as_tensor(a, device=dev)))
        if turn % 3 == 0:
            form, handed = "action_buffer", env.action_buffer
            handed.copy_(t.as_tensor(a, device=dev))
        else:
            form = FORMS[turn % len(FORMS)]
            handed = in_form(form, a, dev)
        assert_same(want, attacker_side(env, env.step(handed)), f"{kind} E={E} turn {turn} ({form})")
        np.testing.assert_array_equal(env.action_buffer.cpu().numpy(), a)
    twin.close()
    env.close()


@pytest.mark.parametrize("E", SIZES)
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("fmt", ["dense", "packed"])
def test_defender_step_takes_every_action_form(fmt, use_graph, E):
    import torch as t
    (att_a, twin), (att_b, env) = pair(E, True, dict(observation_format=fmt)), pair(E, True, dict(observation_format=fmt, use_graph=use_graph))
    dev, rng = att_a.engine.device, np.random.default_rng(E + 1)
    for turn in range(1, TURNS + 1):
        a1 = t.as_tensor(attacker_actions(att_a, rng, turn), device=dev)
        a2 = defender_actions(rng, twin, att_a.topo.n_nodes)
        form = FORMS[turn % len(FORMS)]
        assert_same(attacker_side(att_a, att_a.step(a1)), attacker_side(att_b, att_b.step(a1.clone())), f"{fmt} E={E} turn {turn}: attacker")
        want = defender_side(twin, twin.step(t.as_tensor(a2, device=dev)))
        assert_same(want, defender_side(env, env.step(in_form(form, a2, dev))), f"{fmt} graph={use_graph} E={E} turn {turn} ({form})")
    att_a.close()
    att_b.close()


def two_agent(name, att, dfd):
    from marlon_amd import wrappers
    cls = {"joint": wrappers.TwoAgentVecEnv, "training": wrappers.TwoAgentTrainVecEnv}[name]
    assert cls.supported(att), f"{cls.__name__} does not take {TOPO} at {NODES}/{CREDS}"
    return cls(att, dfd)


def two_agent_sides(env, outs):
    s = {"a." + k: v for k, v in attacker_side(env.att, outs[0]).items()}
    s.update({"d." + k: v for k, v in defender_side(env.dfd, outs[1]).items()})
    return s


@pytest.mark.parametrize("E", SIZES)
@pytest.mark.parametrize("name", ["joint", "training"])
def test_two_agent_step_takes_every_action_form(name, E):
    import torch as t
    twin, env = two_agent(name, *pair(E, name == "training")), two_agent(name, *pair(E, name == "training"))
    dev, rng = env.engine.device, np.random.default_rng(E + 2)
    for turn in range(1, TURNS + 1):
        a1 = attacker_actions(twin.att, rng, turn)
        a2 = defender_actions(rng, twin.dfd, twin.att.topo.n_nodes)
        f1, f2 = FORMS[turn % len(FORMS)], FORMS[(turn // 2) % len(FORMS)]
        want = two_agent_sides(twin, twin.step(t.as_tensor(a1, device=dev), t.as_tensor(a2, device=dev)))
        assert_same(want, two_agent_sides(env, env.step(in_form(f1, a1, dev), in_form(f2, a2, dev))), f"{name} E={E} turn {turn} ({f1} / {f2})")
    twin.att.close()
    env.att.close()


def test_a_wrong_shape_is_refused_before_anything_is_launched():
    import torch as t
    E = 3
    att, dfd = pair(E, False)
    md = attacker(E, discrete=False, observation_format="packed")
    joint = two_agent("joint", att, dfd)
    train = two_agent("training", *pair(E, True))
    dev = att.engine.device
    good1, good2 = t.zeros(E, dtype=t.int64, device=dev), t.zeros((E, 12), dtype=t.int64, device=dev)
    clocks = [att.timesteps, dfd.timesteps, md.timesteps, train.att.timesteps, train.dfd.timesteps]
    for env in (att, md, train.att):
        env.step(t.zeros(env._action_shape, dtype=t.int64, device=dev))               # (so that the clocks are not at their reset value)
    before = [c.clone() for c in clocks]

    def refused(fn, text):
        with pytest.raises(ValueError) as err:
            fn()
        assert str(err.value) == text

    refused(lambda: att.step(t.zeros((E, 1), dtype=t.int64, device=dev)), "expected actions of shape (3,), got (3, 1)")
    refused(lambda: att.step([0, 0]), "expected actions of shape (3,), got (2,)")
    refused(lambda: md.step(np.zeros((E, 9), np.int32)), "expected actions of shape (3, 10), got (3, 9)")
    refused(lambda: md.step(t.zeros(E, dtype=t.int64, device=dev)), "expected actions of shape (3, 10), got (3,)")
    refused(lambda: dfd.step(t.zeros((E, 10), dtype=t.int64, device=dev)), "defender actions must have shape (3, 12), got (3, 10)")
    refused(lambda: dfd.step(np.zeros((4, 12), np.int64)), "defender actions must have shape (3, 12), got (4, 12)")
    for env in (joint, train):
        refused(lambda: env.step(t.zeros((E, 10), dtype=t.int64, device=dev), good2), "attacker actions must have shape (3,), got (3, 10)")
        refused(lambda: env.step(good1, t.zeros((E, 10), dtype=t.int64, device=dev)), "defender actions must have shape (3, 12), got (3, 10)")
        refused(lambda: env.step([0] * 4, [[0] * 12] * E), "attacker actions must have shape (3,), got (4,)")
        refused(lambda: env.step(good1, np.zeros(12, np.int32)), "defender actions must have shape (3, 12), got (12,)")
    t.cuda.synchronize(dev)
    for c, b in zip(clocks, before):
        assert t.equal(c, b), "a refused call stepped a wrapper's clock"
    for e in (att, md, train.att):
        e.close()


# info entries that are persistent buffers of the engine or the wrapper, not part of a step's alternating output set
PERSISTENT_INFO = {"a": ("network_availability", "step_count", "dones"), "d": ()}


# no flag, count, length, reward or return a step writes has this byte in every position (0xAB: a flag of 171, a negative count, -1.2e-12)
POISON = 0xAB


def returned_tensors(side, out):
    """the tensors of one side's step tuple that belong to that step (not the observation: the wrapper's persistent buffers)"""
    _, r, term, trunc, info = out
    named = {"reward": r, "terminated": term, "truncated": trunc}
    named.update({"info." + k: v for k, v in info.items() if k not in PERSISTENT_INFO[side]})
    return named


@pytest.mark.parametrize("E", SIZES)
def test_outputs_stand_until_the_turn_after_next(E):
    """Eager: what turn 1 returned is unchanged after turn 2, and is the memory turn 3 writes — every element of it, shown by poisoning it
    before turn 3 — (turn 4 writes turn 2's).  use_graph: every turn returns the same objects."""
    import torch as t
    rng = np.random.default_rng(E + 3)

    def attacker_rig(**kw):
        env = attacker(E, discrete=True, **kw)
        return "a", (lambda turn: [env.step(attacker_actions(env, rng, turn))]), env.close

    def defender_rig(**kw):
        att, dfd = pair(E, True, dict(kw))

        def step(turn):
            att.step(attacker_actions(att, rng, turn))
            return [dfd.step(defender_actions(rng, dfd, att.topo.n_nodes))]
        return "d", step, att.close

    def two_agent_rig(name):
        env = two_agent(name, *pair(E, name == "training"))
        return "ad", (lambda turn: list(env.step(attacker_actions(env.att, rng, turn), defender_actions(rng, env.dfd, env.att.topo.n_nodes)))), env.att.close

    eager = [("attacker fields", lambda: attacker_rig()), ("attacker packed", lambda: attacker_rig(observation_format="packed")),
             ("defender dense", lambda: defender_rig()), ("defender packed", lambda: defender_rig(observation_format="packed")),
             ("joint", lambda: two_agent_rig("joint")), ("training", lambda: two_agent_rig("training"))]
    for ctx, make in eager:
        sides, step, close = make()
        outs = [[returned_tensors(s, o) for s, o in zip(sides, step(1))]]
        kept = [{k: v.clone() for k, v in side.items()} for side in outs[0]]
        outs += [[returned_tensors(s, o) for s, o in zip(sides, step(turn))] for turn in (2,)]
        for s, side in enumerate(outs[0]):
            for k, v in side.items():
                assert t.equal(v, kept[s][k]), f"{ctx} E={E}: {sides[s]} {k} of turn 1 changed under turn 2"
        for side in outs[0]:                                         # turn 3 has to overwrite every element of what turn 1 returned
            for v in side.values():
                v.view(t.uint8).fill_(POISON)
        outs += [[returned_tensors(s, o) for s, o in zip(sides, step(turn))] for turn in (3, 4)]
        for s, side in enumerate(outs[0]):
            for k, v in side.items():
                stale = (v.view(t.uint8).reshape(E, -1) == POISON).all(dim=1)
                assert not bool(stale.any()), f"{ctx} E={E}: {sides[s]} {k} of turn 1 was not rewritten by turn 3 in envs {stale.nonzero().flatten().tolist()}"
        for s in range(len(sides)):
            assert outs[0][s].keys() == outs[1][s].keys() == outs[2][s].keys() == outs[3][s].keys()
            for k in outs[0][s]:
                first, second, third, fourth = (outs[i][s][k] for i in range(4))
                assert first.data_ptr() != second.data_ptr(), f"{ctx} E={E}: {sides[s]} {k}: consecutive turns share memory"
                assert third.data_ptr() == first.data_ptr() and third.shape == first.shape and third.dtype == first.dtype, \
                    f"{ctx} E={E}: {sides[s]} {k}: turn 3 does not write turn 1's tensor"
                assert fourth.data_ptr() == second.data_ptr(), f"{ctx} E={E}: {sides[s]} {k}: turn 4 does not write turn 2's tensor"
        close()
    graphs = [("attacker use_graph", lambda: attacker_rig(use_graph=True)),
              ("attacker packed use_graph", lambda: attacker_rig(use_graph=True, observation_format="packed")),
              ("defender use_graph", lambda: defender_rig(use_graph=True))]
    for ctx, make in graphs:
        sides, step, close = make()
        outs = [returned_tensors(sides, step(turn)[0]) for turn in (1, 2, 3)]
        for k in outs[0]:
            assert outs[0][k] is outs[1][k] is outs[2][k], f"{ctx} E={E}: {k} is not one object from turn to turn"
        close()


@pytest.mark.parametrize("E", SIZES)
def test_joint_and_separate_turns_mix_on_one_pair(E):
    """Pair A alternates a joint turn with a separate `att.step` / `dfd.step` turn, pair B steps separately throughout (parking the
    defender's turn of an env whose attacker step ended it, as the joint turn does): every output, observation and counter agrees after
    every turn.  The defender's output set moves inside the wrapper on either path, so neither overwrites what the other just returned."""
    import torch as t
    att_a, dfd_a = pair(E, False, max_timesteps=40)
    att_b, dfd_b = pair(E, False, max_timesteps=40)
    joint = two_agent("joint", att_a, dfd_a)
    dev, rng = att_a.engine.device, np.random.default_rng(E + 4)
    previous = None
    for turn in range(1, TURNS + 1):
        a1 = t.as_tensor(attacker_actions(att_b, rng, turn), device=dev)
        a2 = defender_actions(rng, dfd_b, att_b.topo.n_nodes)
        out_b = att_b.step(a1)
        parked = ((out_b[2] != 0) | (out_b[3] != 0)).cpu().numpy()
        a2_parked = a2.copy()
        a2_parked[parked, 0] = -2
        dout_b = dfd_b.step(t.as_tensor(a2_parked, device=dev))
        if turn % 2 == 1:
            out_a, dout_a = joint.step(a1.clone(), t.as_tensor(a2, device=dev))
        else:
            out_a = att_a.step(a1.clone())
            dout_a = dfd_a.step(t.as_tensor(a2_parked, device=dev))
        now = snapshot(att_a, dfd_a, out_a, dout_a)
        assert_same(snapshot(att_b, dfd_b, out_b, dout_b), now, f"E={E} turn {turn}")
        if previous is not None:                                   # the turn before, returned by the other path, still stands
            tensors, values = previous
            for k in ("d.reward", "d.terminated", "d.truncated", "a.rewards", "a.terminated", "a.truncated"):
                np.testing.assert_array_equal(bits(tensors[k]), values[k], err_msg=f"E={E} turn {turn}: {k} of the turn before")
        previous = ({"a.rewards": out_a[1], "a.terminated": out_a[2], "a.truncated": out_a[3], "d.reward": dout_a[1], "d.terminated": dout_a[2],
                     "d.truncated": dout_a[3]}, now)
    att_a.close()
    att_b.close()


def test_a_bound_call_after_close_raises_and_launches_nothing():
    import torch as t
    from marlon_amd.engine import McbsError
    E = 3
    att, dfd = pair(E, False)
    joint = two_agent("joint", att, dfd)
    att_t, dfd_t = pair(E, True)
    train = two_agent("training", att_t, dfd_t)
    packed = attacker(E, discrete=True, observation_format="packed")
    att_p, dfd_p = pair(E, True, dict(observation_format="packed"))
    dev = att.engine.device
    a1, a2 = t.zeros(E, dtype=t.int64, device=dev), t.zeros((E, 12), dtype=t.int64, device=dev)
    att.step(a1), dfd.step(a2), joint.step(a1, a2), train.step(a1, a2), packed.step(a1), att_p.step(a1), dfd_p.step(a2)
    t.cuda.synchronize(dev)
    calls = {"wrapper_step_call": (att, att._calls, (a1,)), "wrapper_step_packed_call": (packed, packed._calls, (a1,)),
             "two_agent_step_call": (att, joint._calls, (a1, a2)), "two_agent_train_step_call": (att_t, train._calls, (a1, a2)),
             "defender_wrapper_step_call": (att, {0: dfd._ring[dfd._slot][3]}, (a2,)),
             "defender_wrapper_step_packed_call": (att_p, {0: dfd_p._ring[dfd_p._slot][3]}, (a2,))}
    clocks = {name: (owner.timesteps, owner.timesteps.clone()) for name, (owner, _, _) in calls.items()}
    dclocks = [(d.timesteps, d.timesteps.clone()) for d in (dfd, dfd_t, dfd_p)]
    for e in (att, att_t, packed, att_p):
        e.close()
    for name, (owner, cached, args) in calls.items():
        assert len(cached) >= 1, name
        for call in cached.values():
            with pytest.raises(McbsError):
                call(*[x.data_ptr() for x in args])
    for env, args in ((att, (a1,)), (dfd, (a2,)), (joint, (a1, a2)), (train, (a1, a2)), (packed, (a1,)), (dfd_p, (a2,))):
        with pytest.raises(McbsError):
            env.step(*args)
    t.cuda.synchronize(dev)
    for name, (clock, was) in clocks.items():
        assert t.equal(clock, was), f"{name}: a call on a closed engine stepped the attacker's clock"
    for clock, was in dclocks:
        assert t.equal(clock, was), "a call on a closed engine stepped a defender's clock"
