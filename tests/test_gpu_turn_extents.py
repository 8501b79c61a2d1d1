"""The byte widths behind the "no written array may share a byte" checks of the packed wrapper step and of the two-agent training
turn (mcbs_attacker_wrapper_step_packed, mcbs_two_agent_train_step): for an array X of the caller's blocks and a moving array M of the
same call, both carved out of ONE allocation,

* M laid over the last bytes of X is refused — MCBS_EINVAL, a message that names both, the batch's state untouched — and
* M laid directly behind the last byte of X is accepted, and the call computes what a twin with ordinary separate buffers computes.

A width one element too small would accept the first placement, one too large would refuse the second.  68 envs: one full 64-env
workgroup and a partial one, and a multiple of 4, so that the end of every per-env array is an address an int32 array may start at."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_packed_step import EINVAL, _actions, _pack, _twins
from tests.test_gpu_two_agent import same_state
from tests.test_gpu_two_agent_training import DKEYS, make_pair

pytestmark = pytest.mark.gpu

E = 68
# (member, bytes per env) as include/mcbs.h types them; n_done (one int32 for the batch) is in no check
W_ARRAYS = (("invalid", 1), ("reward", 4), ("terminated", 1), ("timesteps", 4), ("valid_action_count", 8), ("invalid_action_count", 8),
            ("episode_returns", 8), ("last_cyber_reward", 4), ("has_cyber_reward", 1), ("rewards", 4), ("truncated", 1), ("dones", 1),
            ("episode_return_out", 8), ("episode_length_out", 4), ("executed", 1))
INFO_ARRAYS = (("network_availability", 8), ("step_count", 4), ("truncated", 1), ("out_of_bound", 1), ("raw_reward", 4))


def _w_tensors(env):
    """the tensors behind the attacker wrapper's current mcbs_wrapper_buffers, by member (AttackerVecEnv._wrapper_buffers)"""
    return dict(invalid=env._invalid, reward=env.engine.reward, terminated=env._terminated_out, timesteps=env.timesteps,
                valid_action_count=env.valid_action_count, invalid_action_count=env.invalid_action_count, episode_returns=env.episode_returns,
                last_cyber_reward=env.last_cyber_reward, has_cyber_reward=env.has_cyber_reward, rewards=env._rewards, truncated=env._truncated,
                dones=env._dones, episode_return_out=env._ret_out, episode_length_out=env._len_out, executed=env._executed)


def _zero_outputs(env):
    """both output sets of a wrapper and the engine's own outputs to zero: an element a step leaves alone then reads the same on both sides"""
    import torch
    for _ in range(2):
        o, _, _ = env._next_output_set()
        for v in o.values():
            v.zero_()
    env.engine.reward.zero_()
    for v in env.engine.info.values():
        v.zero_()
    torch.cuda.synchronize()


def _raw_bytes(x):
    import torch
    return x.contiguous().view(-1).view(torch.uint8)


def test_packed_step_refuses_the_last_bytes_of_every_array_and_accepts_the_byte_behind():
    """Chain-4 (6 nodes, 6 credentials), Discrete, auto_reset: packed_terminal against each of the 15 arrays of `w` and the 5 of `info`."""
    import torch
    from marlon_amd._abi import InfoBuffers, WrapperBuffers
    from marlon_amd.samples import chainpattern
    T = 7
    twin, packed = _twins(chainpattern.new_environment(4), E, maximum_node_count=6, maximum_total_credentials=6, discrete=True, max_timesteps=T)
    eng, lib, dev = packed.engine, packed.engine.lib, packed.engine.device
    _zero_outputs(twin)
    _zero_outputs(packed)
    W = packed.packed_observation.shape[1]
    handle = packed._packing_handle()
    g = torch.Generator(device=dev).manual_seed(3)
    ended = 0
    for step, (struct, name, width) in enumerate([("w",) + a for a in W_ARRAYS] + [("info",) + a for a in INFO_ARRAYS]):
        ctx = f"{struct}->{name}"
        _, wb, _ = packed._next_output_set()
        own = _w_tensors(packed)[name] if struct == "w" else eng.info[name]
        assert own.element_size() == width and own.numel() == E, ctx
        nbytes = E * width
        block = torch.zeros(nbytes + E * W * 4, dtype=torch.uint8, device=dev)       # X, then room for the terminal rows directly behind it
        block[:nbytes] = _raw_bytes(own)
        wb2, info2 = WrapperBuffers.from_buffer_copy(wb), InfoBuffers.from_buffer_copy(eng._info_struct)
        setattr(wb2 if struct == "w" else info2, name, block.data_ptr())
        a = _actions(twin, g, step, T)

        def call(term):
            rc = lib.mcbs_attacker_wrapper_step_packed(eng._h, None, a.data_ptr(), packed._rows.data_ptr(), C.byref(info2), handle.ptr,
                                                       packed.packed_observation.data_ptr(), term, packed._packed_fresh.data_ptr(), W, C.byref(wb2),
                                                       packed.invalid_action_reward_modifier, T, 1, eng._stream())
            return rc, lib.mcbs_last_error()

        before = eng.get_state()
        rc, msg = call(block.data_ptr() + nbytes - 4)                                 # its first four bytes are X's last four
        assert rc == EINVAL and b"overlaps" in msg and msg.endswith(ctx.encode()) and b"packed_terminal" in msg, (ctx, rc, msg)
        assert same_state(before, eng.get_state()), ctx + ": a refused call changed the batch"
        rc, msg = call(block.data_ptr() + nbytes)                                     # directly behind X's last byte
        assert rc == 0, (ctx, msg)
        twin.step(a)
        torch.cuda.synchronize()
        moved = block[:nbytes].clone().view(own.dtype)
        got_w, got_info = _w_tensors(packed), dict(eng.info)
        (got_w if struct == "w" else got_info)[name] = moved
        for k, want in _w_tensors(twin).items():
            assert torch.equal(_raw_bytes(got_w[k]), _raw_bytes(want)), f"{ctx}: w->{k} differs from the twin's"
        for k, want in twin.engine.info.items():
            assert torch.equal(_raw_bytes(got_info[k]), _raw_bytes(want)), f"{ctx}: info->{k} differs from the twin's"
        assert torch.equal(packed.packed_observation, twin.observation_packed()), ctx + ": packed observation"
        assert torch.equal(packed._rows, twin._rows), ctx + ": decoded rows"
        done = twin._dones != 0
        term = block[nbytes:].view(torch.int32).view(E, W)
        assert torch.equal(term[done], _pack(twin, twin._terminal)[done]), ctx + ": terminal rows of the envs that ended"
        assert not bool(term[~done].any()), ctx + ": a terminal row of an env that did not end was written"
        ended += int(done.sum())
        own.copy_(moved)                                                              # the wrapper's own tensor carries the state on
    assert ended > E, "too few episodes ended for the terminal rows to mean anything"
    for x, y in zip(eng.get_state(), twin.engine.get_state()):
        assert np.array_equal(x, y)
    packed.close(); twin.close()


class _TrainingSide:
    """One ToyCtf batch with a learned defender and every block of a raw mcbs_two_agent_train_step call, arrays by their message name"""

    def __init__(self, att_T, def_T):
        import torch as t
        self.att, self.dfd = make_pair("toyctf", E, 12, 10, True, att_T, def_T)
        att, eng = self.att, self.att.engine
        dev = eng.device
        att.reset()
        self.dfd.reset()
        _zero_outputs(att)
        mk = lambda dt: t.zeros(E, dtype=dt, device=dev)
        self.cfg = (-1.0, -5000.0, 200.0, 0.6, 5000.0, 1, def_T)
        self.arrays = {"defender_obs->" + k: v for k, v in eng.alloc_defender_obs().items()}
        dw = dict(valid=t.uint8, availability=t.float64, evicted=t.uint8, timesteps=t.int32, valid_action_count=t.int64, invalid_action_count=t.int64,
                  has_breached_sla=t.uint8, prev_availability=t.float64, reward=t.float64, terminated=t.uint8, truncated=t.uint8, breached=t.uint8, won=t.uint8)
        self.arrays.update({"dw->" + k: mk(dt) for k, dt in dw.items()})
        self.arrays["dw->prev_availability"].fill_(1.0)
        tr = dict(attacker_reset_request=t.uint8, defender_return=t.float64, attacker_valid_out=t.int64, attacker_invalid_out=t.int64,
                  defender_return_out=t.float64, defender_length_out=t.int32, defender_valid_out=t.int64, defender_invalid_out=t.int64, defender_dones=t.uint8)
        self.arrays.update({"tr->" + k: mk(dt) for k, dt in tr.items()})
        self.arrays.update({"tr->terminal_" + k: v for k, v in eng.alloc_defender_obs().items()})
        self.arrays.update({"tr->fresh_" + k: self.dfd.observation[k][0].clone() for k in DKEYS})      # the defender's view of a fresh env
        self.obs = eng.obs_struct(att._obs)
        self.keep = eng.row_copies([(att._obs[k], att._terminal[k]) for k in att._obs])
        self.fresh = eng.row_copies([(att._reset_rows[k], att._obs[k]) for k in att._obs], one_row_src=True)

    def current(self):
        """every array of the caller's blocks by its message name, `w` as the attacker wrapper's current output set has it"""
        seen = dict(self.arrays)
        seen.update({"w->" + k: v for k, v in _w_tensors(self.att).items()})
        seen.update({"info->" + k: v for k, v in self.att.engine.info.items()})
        return seen

    def turn(self, a1, a2, moved=None):
        """One raw call on the current output set -> (rc, message, what it wrote by name); moved: {message name: device address} in place of
        the side's own array"""
        import torch as t
        from marlon_amd._abi import (TRAINING_FIELDS, DefenderObs, DefenderWrapperBuffers, DefenderWrapperCfg, InfoBuffers, WrapperBuffers,
                                     training_buffers)
        att, eng = self.att, self.att.engine
        seen = self.current()
        ptr = {k: v.data_ptr() for k, v in seen.items()}
        ptr.update(moved or {})
        wb2 = WrapperBuffers.from_buffer_copy(att._wb)
        for k, _ in W_ARRAYS:
            setattr(wb2, k, ptr["w->" + k])
        info = InfoBuffers(**{k: ptr["info->" + k] for k in eng.info})
        dob = DefenderObs(**{k: ptr["defender_obs->" + k] for k in DKEYS})
        dwb = DefenderWrapperBuffers(**{k: ptr["dw->" + k] for k, _ in DefenderWrapperBuffers._fields_ if not k.startswith("attacker_")},
                                     attacker_has_cyber_reward=ptr["w->has_cyber_reward"], attacker_last_cyber_reward=ptr["w->last_cyber_reward"])
        tb = training_buffers(**{k: ptr["tr->" + k] for k in TRAINING_FIELDS})
        cfg = DefenderWrapperCfg(*self.cfg)
        rc = eng.lib.mcbs_two_agent_train_step(eng._h, None, a1.data_ptr(), att._rows.data_ptr(), C.byref(info), C.byref(self.obs), C.byref(wb2),
                                               att.invalid_action_reward_modifier, att.max_timesteps, C.byref(self.keep), C.byref(self.fresh),
                                               a2.data_ptr(), C.byref(dob), C.byref(dwb), C.byref(cfg), C.byref(tb), eng._stream())
        t.cuda.synchronize(eng.device)
        for k, v in att._obs.items():
            seen["obs->" + k] = v
            seen["terminal obs->" + k] = att._terminal[k]
        seen["decoded"] = att._rows
        return rc, eng.lib.mcbs_last_error().decode(), seen


def test_training_turn_refuses_the_last_bytes_of_an_array_and_accepts_the_byte_behind():
    """ToyCtf with a learned defender, bounds of 12 nodes and 10 credentials: tr->defender_return_out against one array each of `w`, `info`,
    `dw`, `defender_obs`, the terminal group of `tr` and the fresh rows of `tr` — every per-struct list, the widths that depend on the
    node and service counts included."""
    import torch as t
    MOVING = "tr->defender_return_out"
    side, twin = _TrainingSide(3, 4), _TrainingSide(3, 4)
    att, dev = side.att, side.att.engine.device
    N = att.topo.n_nodes
    g = t.Generator(device=dev).manual_seed(11)
    rng = np.random.default_rng(12)
    resets = np.zeros(2, np.int64)
    # (array, its bytes as include/mcbs.h sizes it)
    for name, width in (("w->episode_returns", 8 * E), ("info->network_availability", 8 * E), ("dw->prev_availability", 8 * E),
                        ("defender_obs->incoming_firewall_status", 6 * N * E), ("tr->terminal_outgoing_firewall_status", 6 * N * E),
                        ("tr->fresh_incoming_firewall_status", 6 * N)):
        a1 = twin.att.mask_logits(t.rand((E, att.discrete_n), generator=g, device=dev), fill=-1.0).argmax(dim=1)
        a2 = t.as_tensor((rng.random((E, 12)) * side.dfd.nvec).astype(np.int64), device=dev)
        att._next_output_set()                                            # the output set this turn writes, refused call and accepted one alike
        twin.att._next_output_set()
        own = side.current()[name]
        nbytes = own.numel() * own.element_size()
        one_row = name.startswith("tr->fresh_")
        assert nbytes == width, name
        pad = (-nbytes) % 8                                               # X ends where a double array may start (the fresh row: moved up to there)
        block = t.zeros(pad + nbytes + 8 * E, dtype=t.uint8, device=dev)
        assert (block.data_ptr() + pad) % 16 == 0 or one_row
        block[pad:pad + nbytes] = _raw_bytes(own)
        end = block.data_ptr() + pad + nbytes
        block[pad + nbytes:] = _raw_bytes(side.arrays[MOVING])
        before = att.engine.get_state()
        rc, msg, _ = side.turn(a1, a2, {name: block.data_ptr() + pad, MOVING: end - (1 if one_row else 4)})
        assert rc == EINVAL and "overlaps" in msg and name in msg and MOVING in msg, (name, rc, msg)
        assert same_state(before, att.engine.get_state()), name + ": a refused call changed the batch"
        rc, msg, got = side.turn(a1, a2, {name: block.data_ptr() + pad, MOVING: end})
        assert rc == 0, (name, msg)
        rc, msg, want = twin.turn(a1, a2)
        assert rc == 0, msg
        got[name] = block[pad:pad + nbytes].clone().view(own.dtype)
        got[MOVING] = block[pad + nbytes:].clone().view(t.float64)
        assert got.keys() == want.keys()
        for k in want:
            assert t.equal(_raw_bytes(got[k]), _raw_bytes(want[k])), f"{name}: {k} differs from the twin's"
        own.view(-1).copy_(got[name].view(-1))                            # the side's own tensors carry the state on
        side.arrays[MOVING].copy_(got[MOVING])
        resets += [int((want["w->dones"] != 0).sum()), int((want["tr->defender_dones"] != 0).sum())]
    assert (resets > 0).all(), f"no episode ended on one side: {resets}"
    for x, y in zip(att.engine.get_state(), twin.att.engine.get_state()):
        assert np.array_equal(x, y)
    side.att.close(); twin.att.close()
