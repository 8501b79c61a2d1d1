"""Every kernel path at the capacity limits of the topology format (include/mcbs.h MCBS_MAX_*): 32 ports, 60 properties, 32 local ids
and 32 vulnerability slots per node, 64 and 255 vulnerability columns, 256 credential strings, 256 / 257 / 1 024 credential triples,
1 023 credentials by one action, packed node rows of exactly 32 bits and one or two bits more, connect rows on each side of the fused
observation writers' three length thresholds.  The topologies are marlon_amd/samples/capacity.py's; scripts and references come from
tests/capacity.py (recorded once per case with the CPU oracle, shared, never changed); tests/test_capacity_script.py proves on the CPU
that they reach the bit positions these tests are about.

What is compared, bit for bit (integers, or fp64 computed in the oracle's order; availability as uint64 views): per step reward,
terminated and the five info outputs; at checkpoints and at the end the canonical state from get_state; on every k-th step every
observation field and the flat Discrete mask, into buffers pre-filled with a sentinel.  Every cell asserts eng.variant(), so that a
dispatch change cannot empty it."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from tests import capacity
from tests.test_gpu_packed_lists import _multidiscrete, _same_state

pytestmark = pytest.mark.gpu

INFO = (("network_availability", "availability"), ("step_count", "step_count"), ("truncated", "truncated"), ("out_of_bound", "oob"),
        ("raw_reward", "raw_reward"))
FIELDS = list(capacity.OBS_FIELDS)
SENTINEL = 5


def _engine(ref, monkeypatch=None, env=(), want=None, **spec_over):
    """A BatchEngine on the case's topology created under the developer switches `env`; asserts the variant it dispatches to."""
    from marlon_amd import engine
    for k in env:
        monkeypatch.setenv(k, "1")
    eng = engine.BatchEngine(ref.topo, dataclasses.replace(ref.spec, **spec_over))
    for k in env:
        monkeypatch.delenv(k)
    v = eng.variant()
    expect = dict(capacity.expected_variant(ref.topo, ref.spec))
    if "MCBS_NO_PACKED_SETS" in env:
        expect["packed"] = 0
    expect.update(want or {})
    assert {k: v[k] for k in expect} == expect, f"{ref.name}: the batch dispatches to {v}, the test expects {expect}"
    return eng


def _discrete(oo, E):
    return np.concatenate([oo["mask_connect"].reshape(E, -1), oo["mask_local"].reshape(E, -1), oo["mask_remote"].reshape(E, -1)], axis=1)


def _assert_outputs(eng, ref, t, ctx, info=True):
    np.testing.assert_array_equal(eng.reward.double().cpu().numpy(), ref.out["reward"][t], err_msg=f"{ctx}: reward")
    np.testing.assert_array_equal(eng.terminated.cpu().numpy(), ref.out["terminated"][t], err_msg=f"{ctx}: terminated")
    for mine, theirs in INFO:
        got, want = eng.info[mine].cpu().numpy(), ref.out[theirs][t]
        if not info:
            assert not got.any(), f"{ctx}: info {mine} was written without being requested"
            continue
        if mine == "network_availability":
            got, want = got.view(np.uint64), want.view(np.uint64)
        np.testing.assert_array_equal(got.astype(np.float64) if mine == "raw_reward" else got, want, err_msg=f"{ctx}: info {mine}")


def _assert_obs(obs, oo, E, ctx, A=None):
    for f in FIELDS:
        if f in obs:
            np.testing.assert_array_equal(obs[f].cpu().numpy(), oo[f], err_msg=f"{ctx}: observation {f}")
    if "mask_discrete" in obs:
        m = obs["mask_discrete"].cpu().numpy()
        A = m.shape[1] if A is None else A
        np.testing.assert_array_equal(m[:, :A], _discrete(oo, E), err_msg=f"{ctx}: mask_discrete")
        assert (m[:, A:] == SENTINEL).all(), f"{ctx}: mask_discrete was written past its row"


def _replay(ref, eng, launch, fields=None, what="", stride=0, limit=None):
    """The case's script through one entry point: 'info' (mcbs_step with the five info buffers), 'lean' (mcbs_step without),
    'many' (mcbs_step_many, 25 steps per launch), 'observe' (mcbs_step_observe on the steps the reference holds an observation for)."""
    torch = eng.torch
    E, T = ref.spec.n_envs, ref.script.shape[0] if limit is None else limit
    acts = torch.as_tensor(ref.script[:T], dtype=torch.int32, device=eng.device).contiguous()
    what = f"{ref.name} {what or launch}"
    if launch == "many":
        for t0 in range(0, T, 25):
            t1 = min(T, t0 + 25)
            r, d = eng.step_many(acts[t0:t1])
            np.testing.assert_array_equal(r.double().cpu().numpy(), ref.out["reward"][t0:t1], err_msg=f"{what}: rewards of steps {t0}..{t1 - 1}")
            np.testing.assert_array_equal(d.cpu().numpy(), ref.out["terminated"][t0:t1], err_msg=f"{what}: terminated of steps {t0}..{t1 - 1}")
            if t1 - 1 in ref.states:
                _same_state(eng.get_state(), ref.states[t1 - 1], f"{what}: state after step {t1 - 1}")
        return
    if stride:
        eng.set_mask_discrete_stride(stride)
    A = eng.discrete_action_count()
    obs = None
    if launch == "observe":
        obs = eng.alloc_obs(fields if fields is not None else FIELDS + ["mask_discrete"])
    compared = 0
    for t in range(T):
        ctx = f"{what}, step {t}"
        if launch == "observe" and t in ref.obs:
            for v in obs.values():
                v.fill_(SENTINEL)
            eng.step_observe(acts[t], obs)
            _assert_outputs(eng, ref, t, ctx)
            _assert_obs(obs, ref.obs[t], E, ctx, A)
            compared += 1
        else:
            info = launch != "lean"
            rc = eng.lib.mcbs_step(eng._h, acts[t].data_ptr(), eng.reward.data_ptr(), eng.terminated.data_ptr(),
                                   C.byref(eng._info_struct) if info else None, eng._stream())
            assert rc == 0, eng.lib.mcbs_last_error().decode()
            _assert_outputs(eng, ref, t, ctx, info)
        if t in ref.states:
            _same_state(eng.get_state(), ref.states[t], f"{ctx}: state")
    assert launch != "observe" or compared >= 4, f"{what}: only {compared} observations compared"


# ------------------------------------------------------------------------------------------------ row_limits, 6 nodes, no defender
@pytest.mark.parametrize("launch", ["info", "lean", "many", "observe"])
@pytest.mark.parametrize("E", [1, 67, 130])
def test_row_limits_step_launches(E, launch):
    """32 ports / 60 properties / 32 local ids / 32 slots on the general layout at one word per set: bit 31 of the firewall and listen
    masks, of attacked_ever / attacked_since, of the local mask; property 59 under the tags."""
    ref = capacity.reference(f"limits:{E}")
    eng = _engine(ref, want=dict(coop=0, defender_kind=0))
    assert not eng.step_is_lean(False), "only packed batches have the lean launch: here both calls take the full argument list"
    _replay(ref, eng, launch)
    eng.close()


@pytest.mark.parametrize("switch", ["MCBS_QUAD_OBS", "MCBS_NO_QUAD_OBS"])
@pytest.mark.parametrize("E", [1, 67, 130])
def test_row_limits_observation_kernels(E, switch, monkeypatch):
    """obs_quad_kernel (four envs per wavefront) and obs_small_kernel (a wavefront per env) with every mask field, dense and with
    128-byte-strided Discrete rows; obs_tiny_kernel (no mask field) through mcbs_observe against the oracle's observation of the state.
    Limitation: mcbs_batch_variant does not report which observation kernel a call takes, so this cell cannot assert it.  What it can do
    is assert the inputs of launch_obs_inner's `groups_ok` (at most 16 nodes, node and credential bounds of at most 16, at most 15
    triples, no random-events defender), under which MCBS_QUAD_OBS=1 takes obs_quad_kernel, MCBS_NO_QUAD_OBS=1 obs_small_kernel and a
    call without mask fields obs_tiny_kernel; a change of that condition itself would go unnoticed here."""
    from oracle.oracle import Oracle
    ref = capacity.reference(f"limits:{E}")
    h = capacity.header_counts(ref.topo)
    assert h["n_nodes"] <= 16 and h["n_triples"] <= 15 and ref.spec.maximum_node_count <= 16 and ref.spec.maximum_total_credentials <= 16 \
        and ref.spec.defender is None, "the preconditions of the four-envs-per-wavefront and the sixteen-lanes-per-env kernels"
    eng = _engine(ref, monkeypatch, env=(switch,))
    _replay(ref, eng, "observe", what=switch)
    eng.close()
    eng = _engine(ref, monkeypatch, env=(switch,))
    A = eng.discrete_action_count()
    _replay(ref, eng, "observe", what=f"{switch}, strided rows", stride=(A + 127) // 128 * 128, limit=40)
    eng.close()
    # no mask field: sixteen lanes per env
    over = dict(auto_reset=False, attacker_goal=None, max_episode_steps=0)          # no env ends: the rows of both stay comparable
    eng = _engine(ref, monkeypatch, env=(switch,), **over)
    orc = Oracle(ref.topo, dataclasses.replace(ref.spec, **over))
    small = FIELDS[:5]
    for t in range(30):
        orc.step(ref.script[t])
        eng.step(ref.script[t])
    obs = eng.alloc_obs(small)
    for v in obs.values():
        v.fill_(SENTINEL)
    eng.observe(obs)
    oo = orc.observe(orc.alloc_obs(small))
    _assert_obs(obs, oo, E, f"{ref.name}: mcbs_observe without mask fields after 30 steps")
    eng.close()


@pytest.mark.parametrize("E", [1, 67, 130])
def test_row_limits_masks_logits_and_features(E):
    """pack_action_mask / unpack_action_mask / mask_logits / apply_packed_mask against the oracle's mask, encode_features against
    FeatureLayout.encode_host of the oracle's observation, masked_categorical's allowed count against the mask's population."""
    from marlon_amd.features import FeatureLayout
    ref = capacity.reference(f"limits:{E}")
    eng = _engine(ref)
    torch = eng.torch
    A = eng.discrete_action_count()
    N, Cm, P, L, R = 8, 16, 32, 32, 8
    assert A == N * N * P * Cm + N * L + N * N * R
    layout = FeatureLayout(ref.topo, ref.spec)
    handle = eng.feature_layout(layout)
    obs = eng.alloc_obs(FIELDS)
    acts = torch.as_tensor(ref.script, dtype=torch.int32, device=eng.device)
    compared = compared_rows = sampled_rows = 0
    for t in range(ref.script.shape[0]):
        if t not in ref.obs:
            eng.step(acts[t])
            continue
        eng.step_observe(acts[t], obs)
        oo = ref.obs[t]
        want = _discrete(oo, E).astype(bool)
        ctx = f"{ref.name}, step {t}"
        # An env that ended on this step was re-initialised after its observation was written: the digest still describes the observed
        # state, but the local block of a rebuilt mask is read through the env's live discovery list (mcbs.h, mcbs_mask_logits).  Its
        # row is defined again after the next observation; here it is left out.
        live = (ref.out["terminated"][t] == 0) & (ref.out["truncated"][t] == 0)
        compared_rows += int(live.sum())
        bits = eng.pack_action_mask()
        W = eng.packed_mask_words()[0]
        packed = np.packbits(np.pad(want, ((0, 0), (0, W * 32 - A))), axis=1, bitorder="little").view("<i4")
        np.testing.assert_array_equal(bits.cpu().numpy()[:, :W][live], packed[live], err_msg=f"{ctx}: pack_action_mask")
        np.testing.assert_array_equal(eng.unpack_action_mask(bits).cpu().numpy()[live], want[live], err_msg=f"{ctx}: unpack_action_mask")
        for apply in ("digest", "bits"):
            logits = torch.full((E, A + 3), 2.5, dtype=torch.float32, device=eng.device)
            eng.mask_logits(logits, fill=-7.0) if apply == "digest" else eng.apply_packed_mask(bits, logits, fill=-7.0)
            got = logits.cpu().numpy()
            np.testing.assert_array_equal(got[:, :A][live], np.where(want, np.float32(2.5), np.float32(-7.0))[live], err_msg=f"{ctx}: masked logits ({apply})")
            assert (got[:, A:] == 2.5).all(), f"{ctx}: logits past the action count were written ({apply})"
        cat = eng.masked_categorical(None, mode="sample", seed=3, step=t)          # the live form: the mask rebuilt from the digest
        np.testing.assert_array_equal(cat.n_allowed.cpu().numpy()[live], want.sum(axis=1)[live], err_msg=f"{ctx}: masked_categorical allowed count")
        picked = cat.actions.cpu().numpy()
        some = live & want.any(axis=1)          # (an out-of-bound action leaves a blank observation: its mask allows nothing, n_allowed is 0)
        sampled_rows += int(some.sum())
        assert want[np.arange(E), np.clip(picked, 0, A - 1)][some].all() and (picked[some] >= 0).all() and (picked[some] < A).all(), \
            f"{ctx}: masked_categorical sampled a masked action"
        feats = eng.encode_features(handle, {k: obs[k] for k in FIELDS[:5]})
        np.testing.assert_array_equal(feats.cpu().numpy(), layout.encode_host({k: oo[k] for k in FIELDS[:5]}), err_msg=f"{ctx}: encode_features")
        compared += 1
    assert compared >= 8 and compared_rows >= 6 * E and sampled_rows >= 5 * E, "the masks of most rows are compared"
    _same_state(eng.get_state(), ref.final, f"{ref.name}: final state")
    handle.close()
    eng.close()


@pytest.mark.parametrize("discrete", [False, True], ids=["multidiscrete", "discrete"])
@pytest.mark.parametrize("E", [1, 67, 130])
def test_row_limits_attacker_vec_env(E, discrete):
    """AttackerVecEnv (three launches per step on this layout), MultiDiscrete rows and Discrete indices (decoded on the device): the
    engine state, the observation fields and the materialised Discrete mask equal the oracle's after every scripted step."""
    from marlon_amd import model
    from marlon_amd.samples import capacity as samples
    from oracle.oracle import Oracle
    ref = capacity.reference(f"limits:{E}")
    spec = ref.spec
    wr = _vec_env(samples.row_limits(model), spec, discrete)
    assert wr.engine.variant()["packed"] == 0 and wr.engine.wrapper_step_launches(True) == 3
    torch = wr.engine.torch
    N, Cm, P, L, R = 8, 16, 32, 32, 8
    orc = Oracle(ref.topo, wr.spec)
    orc.reset()                                                    # the wrapper's constructor began episode 1
    oo = orc.alloc_obs(FIELDS)
    pol = capacity.endings.Policy(ref.topo, wr.spec, seed=5)
    skipped = intercepted = 0
    for t in range(60):
        before = orc.get_state()
        rows, valid, bad = _wrapper_rows(pol.rows(before), before, N, L, R, P, Cm)
        skipped += int(bad.sum())
        intercepted += int((~valid).sum())
        if discrete:
            k, a1, a2, a3, a4 = rows.astype(np.int64).T
            act = np.where(k == 2, ((a1 * N + a2) * P + a3) * Cm + a4,
                           np.where(k == 0, N * N * P * Cm + a1 * L + a2, N * N * P * Cm + N * L + (a1 * N + a2) * R + a3))
        else:
            act = _multidiscrete(rows)
        wr.step(torch.as_tensor(act, device=wr.engine.device))
        played = rows.copy()
        played[~valid, 0] = 3                                       # MCBS_ACTION_SKIP: an intercepted action is not played
        orc.step(played, obs=oo)
        ctx = f"{ref.name} wrapper ({'Discrete' if discrete else 'MultiDiscrete'}), step {t}"
        np.testing.assert_array_equal(wr._invalid.cpu().numpy() != 0, ~valid, err_msg=f"{ctx}: interception")
        _same_state(wr.engine.get_state(), orc.get_state(), ctx)
        for f in FIELDS[:5]:
            np.testing.assert_array_equal(wr._obs[f].cpu().numpy().reshape(E, -1)[valid], oo[f].reshape(E, -1)[valid], err_msg=f"{ctx}: observation {f}")
        np.testing.assert_array_equal(wr.action_masks().cpu().numpy()[valid], _discrete(oo, E).astype(bool)[valid], err_msg=f"{ctx}: action_masks")
    assert intercepted + skipped < 60 * E // 2, "most scripted actions are played"
    wr.close()


def _wrapper_rows(rows, state, N, L, R, P, Cm):
    """(rows inside the wrapper's action space, the wrapper's validity of each, which rows had to be replaced).  A row outside the
    MultiDiscrete bounds becomes a plain local exploit; a source or target past the discovered nodes is what the wrapper intercepts
    (attack_wrapper.py:286-308): such an action is not played at all."""
    rows = rows.astype(np.int64)
    bad = (rows[:, 0] > 2) | (rows[:, 1] >= N) | (rows[:, 2] >= np.where(rows[:, 0] == 0, L, N)) | \
          (rows[:, 3] >= np.where(rows[:, 0] == 1, R, P)) | (rows[:, 4] >= Cm) | (rows < 0).any(axis=1)
    rows[bad] = (0, 0, 0, 0, 0)
    rows[rows[:, 0] == 0, 3:] = 0
    rows[rows[:, 0] == 1, 4] = 0
    nd = state[0]["n_discovered"].astype(np.int64)
    valid = (rows[:, 1] < nd) & ((rows[:, 0] == 0) | (rows[:, 2] < nd))
    return rows.astype(np.int32), valid, bad


def _vec_env(environment, spec, discrete, **kw):
    from marlon_amd.wrappers import AttackerVecEnv
    return AttackerVecEnv(environment, spec.n_envs, maximum_total_credentials=spec.maximum_total_credentials,
                          maximum_node_count=spec.maximum_node_count, attacker_goal=None, discrete=discrete, auto_reset=True,
                          seed=spec.seed, env_id_base=spec.env_id_base, max_timesteps=10 ** 6, **kw)          # (no goal, no bound: no env ends)


# ------------------------------------------------------------------------------------------------ row_limits with defenders, R bounds
@pytest.mark.parametrize("launch", ["info", "many", "observe"])
@pytest.mark.parametrize("name", ["limits:67:scan", "limits:67:ere", "limits:67:R40", "limits:67:R223"])
def test_row_limits_defenders_and_remote_bounds(name, launch):
    """ScanAndReimage (Philox; re-images clear bit 31 of attacked_since), ExternalRandomEvents at L = 32, R = 32 (column 63 of the
    presence masks), and 40 / 223 remote ids (72 / 255 vulnerability columns: past the random-events tables, at the format's bound)."""
    ref = capacity.reference(name)
    kind = {"scan": 1, "ere": 3}.get(name.split(":")[2], 0)
    eng = _engine(ref, want=dict(coop=0, defender_kind=kind))
    _replay(ref, eng, launch)
    eng.close()


@pytest.mark.parametrize("R", [33, 40, 223])
def test_random_events_refused_beyond_64_columns(R):
    from marlon_amd import engine
    ref = capacity.reference("limits:67:R40")
    topo = capacity.topology("limits", 6, 32, R)
    with pytest.raises(ValueError, match=r"\(-1\).*carries no ExternalRandomEvents tables"):        # MCBS_EINVAL
        engine.BatchEngine(topo, dataclasses.replace(ref.spec, defender=("random_events",)))


def test_topology_refused_one_column_past_the_bound():
    """A blob with 256 vulnerability columns (flatten refuses to write one: its bound is lifted here) is refused by
    mcbs_topology_create with MCBS_ELIMIT."""
    from marlon_amd import engine, flatten, model
    from marlon_amd.samples import capacity as samples
    ref = capacity.reference("limits:67:R40")
    bound = flatten.MAX_COLUMNS
    flatten.MAX_COLUMNS = 1 << 20
    try:
        topo = flatten.flatten(samples.row_limits(model, n_remote=224))
    finally:
        flatten.MAX_COLUMNS = bound
    with pytest.raises(engine.McbsError, match=r"\(-2\).*exceeds an engine limit"):
        engine.BatchEngine(topo, ref.spec)


@pytest.mark.parametrize("fused", [True, False], ids=["fused_obs", "separate_obs"])
def test_row_limits_learned_defender(fused, monkeypatch):
    """defender_step / defender_observe with firewall actions on the managed rules of port 0 (RDP) and port 31 (sudo), with the
    observation written by the turn kernel and by the separate launch."""
    ref = capacity.reference("limits:67:external")
    eng = _engine(ref, monkeypatch, env=() if fused else ("MCBS_NO_FUSED_DEFENDER_OBS",), want=dict(defender_kind=2, fused_defender_obs=int(fused)))
    assert [int(x) for x in ref.topo.header()["rule_port"][:6]] == [0, 255, 255, 255, 255, 31], "RDP is port 0 and sudo port 31"
    torch = eng.torch
    d = ref.defender
    dobs = eng.alloc_defender_obs()
    acts = torch.as_tensor(ref.script, dtype=torch.int32, device=eng.device)
    fw_acted = 0
    for t in range(ref.script.shape[0]):
        ctx = f"{ref.name} ({'fused' if fused else 'separate'} observation), step {t}"
        eng.step(acts[t])
        _assert_outputs(eng, ref, t, ctx)
        for v in dobs.values():
            v.fill_(9)
        if t % 2 == 0:
            v, av, ev = eng.defender_step(d["actions"][t], dobs)
        else:
            v, av, ev = eng.defender_step(d["actions"][t])
            eng.defender_observe(dobs)
        np.testing.assert_array_equal(v.cpu().numpy(), d["valid"][t], err_msg=f"{ctx}: valid")
        np.testing.assert_array_equal(av.cpu().numpy().view(np.uint64), d["availability"][t].view(np.uint64), err_msg=f"{ctx}: availability")
        np.testing.assert_array_equal(ev.cpu().numpy(), d["evicted"][t], err_msg=f"{ctx}: evicted")
        for k, want in d["obs"][t].items():
            np.testing.assert_array_equal(dobs[k].cpu().numpy(), want, err_msg=f"{ctx}: defender observation {k}")
        fw_acted += int(np.isin(d["actions"][t][:, 0], (1, 2)).sum())
        if t in ref.states:
            _same_state(eng.get_state(), ref.states[t], f"{ctx}: state")
    assert fw_acted > 100
    assert any((o["outgoing_firewall_status"].reshape(67, 6, 6)[:, :, 5] == 0).any() for o in d["obs"]), "an outgoing sudo (port 31) rule is blocked"
    assert any((o["incoming_firewall_status"].reshape(67, 6, 6)[:, 2, 5] == 1).any() for o in d["obs"]), "node 2's blocked port 31 is opened again"
    eng.close()


@pytest.mark.parametrize("fused", [True, False], ids=["fused_obs", "separate_obs"])
def test_row_limits_defender_vec_env(fused, monkeypatch):
    """DefenderVecEnv.step (mcbs_defender_wrapper_step: defender_turn_post_kernel<1>, the turn and the reward shaping in one launch, the
    observation fused into it or a launch of its own) next to AttackerVecEnv(learned_defender=True) on the limits topology, 67 envs:
    validity, availability bits, eviction, shaped reward bits, flags, counters and the four observation arrays against the oracle's
    turn plus the float64 NumPy shaping (tests/capacity.py defender_vec_env_reference, the protocol of
    test_gpu_defender_layouts.py::test_defender_vec_env_shaping_against_numpy), the engine state every 10th turn.  Firewall actions
    toggle the managed rules of port 0 and port 31; re-images clear rows whose attacked_since holds bit 31."""
    from marlon_amd.wrappers import AttackerVecEnv, DefenderVecEnv
    from tests.test_gpu_defender_layouts import DEF_KEYS
    ref = capacity.defender_vec_env_reference()
    E, c = capacity.VEC_E, capacity.VEC_SHAPING
    if not fused:
        monkeypatch.setenv("MCBS_NO_FUSED_DEFENDER_OBS", "1")
    att = AttackerVecEnv(ref["topo"], E, max_timesteps=capacity.VEC_MAXT_A, learned_defender=True, materialize_masks=False,
                         **capacity.vec_env_kwargs())
    monkeypatch.delenv("MCBS_NO_FUSED_DEFENDER_OBS", raising=False)
    dfd = DefenderVecEnv(att, max_timesteps=capacity.VEC_MAXT_D, invalid_action_reward=c["invalid_action_penalty"],
                         reset_on_constraint_broken=False, loss_reward=c["loss_reward"], sla_worsening_penalty_scale=c["sla_worsening_penalty_scale"])
    v = att.engine.variant()
    want = dict(defender_kind=2, packed=0, wide=0, words_per_set=1, fused_defender_obs=int(fused))
    assert {k: v[k] for k in want} == want, f"the batch dispatches to {v}"
    assert bytes(att.spec.to_cfg()) == bytes(dataclasses.replace(ref["spec"], device=att.spec.device).to_cfg()), "the oracle played another spec"
    assert (att.nvec == capacity.ATTACKER_NVEC).all() and (dfd.nvec == capacity.DEFENDER_NVEC(6)).all()
    torch = att.torch
    mask = lambda m: torch.as_tensor(m.astype(np.uint8), device=att.engine.device)          # noqa: E731
    for t, st in enumerate(ref["steps"]):
        ctx = f"limits DefenderVecEnv ({'fused' if fused else 'separate'} observation), turn {t}"
        obs, r, term, trunc, info = att.step(st["a"])
        np.testing.assert_array_equal(r.double().cpu().numpy(), st["reward"], err_msg=ctx + ": attacker reward")
        np.testing.assert_array_equal(term.cpu().numpy(), st["terminated"], err_msg=ctx + ": attacker terminated")
        np.testing.assert_array_equal(info["invalid_action"].cpu().numpy(), ~st["valid"], err_msg=ctx + ": interception")
        if st["a_done"].any():                           # a new episode of both agents: the defender wrapper's state too
            dfd.reset(mask(st["a_done"]))
        dobs, dr, dterm, dtrunc, dinfo = dfd.step(st["da"])
        od = st["od"]
        np.testing.assert_array_equal(dinfo["valid_action"].cpu().numpy(), od["valid"] != 0, err_msg=ctx + ": valid")
        np.testing.assert_array_equal(dinfo["network_availability"].cpu().numpy().view(np.uint64), od["availability"].view(np.uint64),
                                      err_msg=ctx + ": availability bits")
        np.testing.assert_array_equal(dr.cpu().numpy().view(np.uint64), st["exp_r"].view(np.uint64), err_msg=ctx + ": shaped reward bits")
        np.testing.assert_array_equal(dterm.cpu().numpy() != 0, st["exp_term"], err_msg=ctx + ": terminated")
        np.testing.assert_array_equal(dtrunc.cpu().numpy() != 0, st["exp_trunc"], err_msg=ctx + ": truncated")
        np.testing.assert_array_equal(dinfo["sla_breached"].cpu().numpy(), st["exp_breached"], err_msg=ctx + ": sla_breached")
        np.testing.assert_array_equal(dinfo["defender_won"].cpu().numpy(), od["evicted"] != 0, err_msg=ctx + ": defender_won")
        np.testing.assert_array_equal(dfd.valid_action_count.cpu().numpy(), st["n_valid"], err_msg=ctx + ": valid count")
        np.testing.assert_array_equal(dfd.invalid_action_count.cpu().numpy(), st["n_invalid"], err_msg=ctx + ": invalid count")
        for k in DEF_KEYS:
            np.testing.assert_array_equal(dobs[k].cpu().numpy(), st["obs"][k], err_msg=f"{ctx}: defender observation {k}")
        if st["state"] is not None:
            _same_state(att.engine.get_state(), st["state"], ctx + ": state")
        if st["d_done"].any():
            dfd.reset(mask(st["d_done"]))
    att.close()


# ------------------------------------------------------------------------------------------------ observation bounds
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("nmax", [8, 16])
@pytest.mark.parametrize("bounds", capacity.BOUNDS, ids=lambda b: f"{b[0]}x{b[1]}")
def test_connect_row_lengths_at_the_fused_writers_thresholds(bounds, nmax, strided):
    """RL = P * Cmax = 512, 1 024 (64 chunks), 1 056, 1 036 (the 1 040-byte pattern area exactly full), 1 040 (four bytes too long for
    it: the fused writers must leave it to the region kernels), 1 064, and 504 / 520 (no multiples of 16; 63 and 65 periods: the period
    writer and the dword writer): each side of RL / 16 <= 64, RL / gcd(RL, 16) <= 64 and RL + 4 <= 1 040 in launch_obs_inner."""
    P, C_ = bounds
    ref = capacity.reference(f"bounds:{P}x{C_}:{nmax}")
    eng = _engine(ref)
    A = eng.discrete_action_count()
    assert A == nmax * nmax * P * C_ + nmax * 32 + nmax * nmax * 8
    _replay(ref, eng, "observe", what="strided rows" if strided else "dense rows", stride=(A + 127) // 128 * 128 if strided else 0)
    eng.close()


# ------------------------------------------------------------------------------------------------ rings of 66 and 130 nodes
@pytest.mark.parametrize("defender", ["none", "scan"])
@pytest.mark.parametrize("E", [33, 67])
@pytest.mark.parametrize("n_nodes", [66, 130])
def test_cooperative_kernel_and_one_lane_twin(n_nodes, E, defender, monkeypatch):
    """The same 32-slot rows stepped by mcbs_step_coop.hip (G = 2 lanes per env at 66 nodes, G = 4 at 130: its own copy of the row code,
    `1u << slot` included) and, under MCBS_NO_COOP=1, by the one-lane kernel: each against the oracle, hence against each other."""
    ref = capacity.reference(f"limits:{E}:n{n_nodes}" + (":scan" if defender == "scan" else ""))
    G = 2 if n_nodes == 66 else 4
    for env, coop in (((), 1), (("MCBS_NO_COOP",), 0)):
        eng = _engine(ref, monkeypatch, env=env, want=dict(coop=coop, words_per_set=G, wide=0, packed=0))
        _replay(ref, eng, "info", what="cooperative" if coop else "one lane")
        eng.close()
        eng = _engine(ref, monkeypatch, env=env, want=dict(coop=coop))
        _replay(ref, eng, "many", what="cooperative, step_many" if coop else "one lane, step_many")
        eng.close()


# ------------------------------------------------------------------------------------------------ packed-row budget
@pytest.mark.parametrize("E", [1, 65, 130])
@pytest.mark.parametrize("edge", capacity.PACKED_EDGES, ids=lambda e: f"{e[0]}x{e[1]}")
def test_packed_row_budget_edges(edge, E, monkeypatch):
    """n_props + 4 + 2 * slots = 32 (packed: the top property bit touches the tags, the top slot of attacked_since is bit 31 of the
    4-byte row) and 33 / 34 (general).  Lean and full mcbs_step, step_many and step_observe, auto-reset at 7 steps; the packed cases
    again under MCBS_NO_PACKED_SETS=1."""
    p, s = edge
    ref = capacity.reference(f"packed:{p}x{s}:{E}")
    packed = int(p + 4 + 2 * s <= 32)
    twins = [()] + ([("MCBS_NO_PACKED_SETS",)] if packed else [])
    for env in twins:
        is_packed = packed and not env
        for launch in ("lean", "info", "many", "observe"):
            eng = _engine(ref, monkeypatch, env=env, want=dict(packed=int(is_packed), defender_kind=0))
            assert eng.step_is_lean(False) == bool(is_packed) and not eng.step_is_lean(True)
            _replay(ref, eng, launch, what=f"{launch}{' (general twin)' if env else ''}")
            eng.close()


@pytest.mark.parametrize("fused", [True, False], ids=["one_launch", "three_launches"])
@pytest.mark.parametrize("edge", capacity.PACKED_EDGES, ids=lambda e: f"{e[0]}x{e[1]}")
def test_packed_row_budget_edges_wrapper(edge, fused, monkeypatch):
    """The attacker wrapper's step in one launch (packed batches; MCBS_NO_FUSED_WRAPPER=1: three) on the packed-row edges."""
    from marlon_amd import model
    from marlon_amd.samples import capacity as samples
    from oracle.oracle import Oracle
    p, s = edge
    E = 65
    ref = capacity.reference(f"packed:{p}x{s}:{E}")
    packed = int(p + 4 + 2 * s <= 32)
    if not fused:
        monkeypatch.setenv("MCBS_NO_FUSED_WRAPPER", "1")
    wr = _vec_env(samples.packed_edge(model, p, s), ref.spec, False, materialize_masks=False)
    monkeypatch.delenv("MCBS_NO_FUSED_WRAPPER", raising=False)
    assert wr.engine.variant()["packed"] == packed
    assert wr.engine.wrapper_step_launches(False) == (1 if packed and fused else 3)
    torch = wr.engine.torch
    orc = Oracle(ref.topo, wr.spec)
    orc.reset()                                                    # the wrapper's constructor began episode 1
    oo = orc.alloc_obs(FIELDS[:5])
    pol = capacity.endings.Policy(ref.topo, wr.spec, seed=5)
    for t in range(40):
        before = orc.get_state()
        rows, valid, _ = _wrapper_rows(pol.rows(before), before, 16, s, s, 4, 15)
        wr.step(torch.as_tensor(_multidiscrete(rows), device=wr.engine.device))
        played = rows.copy()
        played[~valid, 0] = 3
        orc.step(played, obs=oo)
        ctx = f"{ref.name} wrapper ({'one launch' if fused else 'three launches'}), step {t}"
        np.testing.assert_array_equal(wr._invalid.cpu().numpy() != 0, ~valid, err_msg=f"{ctx}: interception")
        _same_state(wr.engine.get_state(), orc.get_state(), ctx)
        for f in FIELDS[:5]:
            np.testing.assert_array_equal(wr._obs[f].cpu().numpy().reshape(E, -1)[valid], oo[f].reshape(E, -1)[valid], err_msg=f"{ctx}: observation {f}")
    wr.close()


# ------------------------------------------------------------------------------------------------ credential limits
@pytest.mark.parametrize("launch", ["info", "many", "observe"])
@pytest.mark.parametrize("name", ["creds:256", "creds:257", "creds:1024", "creds:257:scan", "creds:1024:scan"])
def test_credential_limits(name, launch):
    """256 triples (four words per set, the last narrow count), 257 (wide, TW = 5) and 1 024 (TW = 16) with 256 credential strings: the
    top bit of word 3 of the gathered-strings set, the 10-bit new-credentials field at 1 023, the u16 cache list at 1 024 entries;
    observation (leaked_credentials with K = 1 023 rows, a 2.6 MB connect mask per env at 1 024) on every 10th step."""
    ref = capacity.reference(name)
    eng = _engine(ref, want=dict(coop=0, defender_kind=1 if name.endswith(":scan") else 0))
    _replay(ref, eng, launch)
    eng.close()


@pytest.mark.parametrize("nt", [256, 257, 1024])
def test_credential_limits_state_round_trip(nt):
    """get_state -> set_state -> get_state is the identity with a full cache, and the batch continues from it as the oracle does."""
    ref = capacity.reference(f"creds:{nt}")
    T = ref.script.shape[0]
    t_full = max(t for t in ref.states if t < T - 1 and (ref.states[t][0]["n_creds"] == nt).any())
    full = ref.states[t_full]
    assert (full[0]["n_creds"] == nt).any(), "a full cache at the checkpoint"
    eng = _engine(ref)
    eng.set_state(*full)
    _same_state(eng.get_state(), full, f"{ref.name}: set_state -> get_state")
    torch = eng.torch
    for t in range(t_full + 1, T):
        eng.step(torch.as_tensor(ref.script[t], dtype=torch.int32, device=eng.device))
        _assert_outputs(eng, ref, t, f"{ref.name} continued from set_state, step {t}")
    _same_state(eng.get_state(), ref.final, f"{ref.name}: final state after the round trip")
    eng.close()
