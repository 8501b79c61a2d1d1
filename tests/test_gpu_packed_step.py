"""AttackerVecEnv(observation_format="packed"): the one-launch wrapper step that writes each env's observation as the bit-packed row of
features.ObservationPacking itself (mcbs_attacker_wrapper_step_packed, marlon_amd/csrc/mcbs_wrapper_fused.hip
wrapper_fused_packed_kernel), against the int32 one-launch step followed by mcbs_pack_observation — the same bytes by the route a packing
trainer took before — against the traces of the reference's own wrappers (attack_wrapper.py:255-372, action_masking.py:112-142), and
the mode's consumers and refusals."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import parity
from tests.test_gpu_facades import WRAP

pytestmark = pytest.mark.gpu

FIELDS = ["scalars", "leaked_credentials", "credential_cache_matrix", "discovered_nodes_properties", "nodes_privilegelevel"]
COUNTERS = ("timesteps", "valid_action_count", "invalid_action_count", "episode_returns", "last_cyber_reward", "has_cyber_reward")
EINVAL = -1


def _case(case):
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.samples import chainpattern, toy_ctf
    if case == "chain10_discrete":
        return chainpattern.new_environment(10), dict(maximum_node_count=12, maximum_total_credentials=12, discrete=True, max_timesteps=40)
    if case == "toyctf_defender_multidiscrete":
        return toy_ctf.new_environment(), dict(maximum_node_count=12, maximum_total_credentials=10, discrete=False, max_timesteps=35,
                                               attacker_goal=ce.AttackerGoal(own_atleast=6, own_atleast_percent=1.0),
                                               defender_constraint=ce.DefenderConstraint(0.8),
                                               defender_agent=ce.ScanAndReimageCompromisedMachines(0.6, 2, 5), seed=31)
    if case == "chain4_discrete_graph":
        return chainpattern.new_environment(4), dict(maximum_node_count=6, maximum_total_credentials=6, discrete=True, max_timesteps=25, use_graph=True)
    assert case == "toyctf_learned_defender"
    return toy_ctf.new_environment(), dict(maximum_node_count=12, maximum_total_credentials=10, discrete=True, max_timesteps=30, learned_defender=True)


def _twins(env0, E, **kw):
    """-> (int32-mode one-launch wrapper, packed-mode wrapper) on the same batch settings"""
    from marlon_amd.wrappers import AttackerVecEnv
    twin = AttackerVecEnv(env0, E, materialize_masks=False, **kw)
    packed = AttackerVecEnv(env0, E, materialize_masks=False, observation_format="packed", **kw)
    assert twin.engine.wrapper_step_launches(False) == 1 and packed.observation_format == "packed"
    return twin, packed


def _as_multidiscrete(env, a):
    """The Discrete index a [E] as MultiDiscrete(10) rows (attack_wrapper.py:206-227); an index outside the space stays outside."""
    import torch
    N, Cm = env.spec.maximum_node_count, env.spec.maximum_total_credentials
    M, ML = env._mask_split[0], env._mask_split[1]
    L, R, P = ML // N, (env.discrete_n - M - ML) // (N * N), M // (N * N * Cm)
    md = torch.zeros((a.shape[0], 10), dtype=torch.int64, device=a.device)
    is_c, is_l = a < M, (a >= M) & (a < M + ML)
    is_r = ~is_c & ~is_l
    md[:, 0] = torch.where(is_c, 2, torch.where(is_l, 0, 1))
    rel = torch.where(is_c, a, torch.where(is_l, a - M, a - M - ML))
    md[:, 1] = torch.where(is_l, rel // L, 0); md[:, 2] = torch.where(is_l, rel % L, 0)
    md[:, 3] = torch.where(is_r, rel // (N * R), 0); md[:, 4] = torch.where(is_r, (rel // R) % N, 0); md[:, 5] = torch.where(is_r, rel % R, 0)
    md[:, 6] = torch.where(is_c, rel // (N * P * Cm), 0); md[:, 7] = torch.where(is_c, (rel // (P * Cm)) % N, 0)
    md[:, 8] = torch.where(is_c, (rel // Cm) % P, 0); md[:, 9] = torch.where(is_c, rel % Cm, 0)
    return md


def _actions(twin, g, t, T, every=7):
    """Masked-random actions from the twin's digests, with intercepted ones (an undiscovered node index) on every `every`-th step and on
    the truncating step, and one negative index."""
    import torch
    E, dev = twin.num_envs, twin.engine.device
    scores = torch.rand((E, twin.discrete_n), generator=g, device=dev)
    a = twin.mask_logits(scores, fill=-1.0).argmax(dim=1)
    if t % every == 3 or (t + 1) % T == 0:
        a[::9] = twin.discrete_n - 1
    negative = t % every == 5
    if negative:
        a[E // 2] = -1
    if not twin.discrete:
        a = _as_multidiscrete(twin, a)
        if negative:
            a[E // 2] = torch.tensor([0, -1, 0, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int64, device=dev)
    return a


def _pack(env, fields):
    return env.engine.pack_observation(env._packing_handle(), {k: fields[k] for k in FIELDS})


def _twin_run(case, E, steps, stream_ctx=None, full=True):
    import torch
    from tests.test_gpu_parity import _compare_states
    env0, kw = _case(case)
    twin, packed = _twins(env0, E, **kw)
    dev = twin.engine.device
    g = torch.Generator(device=dev).manual_seed(5)
    T = kw["max_timesteps"]
    assert torch.equal(packed.observation["packed"], twin.observation_packed()), "reset observation"
    ended = 0
    prev_term = packed.terminal_packed_observation.clone()
    for t in range(steps):
        a = _actions(twin, g, t, T)
        o1, r1, te1, tr1, i1 = packed.step(a.clone())
        o2, r2, te2, tr2, i2 = twin.step(a)
        ctx = f"{case} E={E} step {t}"
        assert set(o1) == {"packed"} and o1["packed"] is packed.packed_observation
        assert torch.equal(packed.packed_observation, twin.observation_packed()), ctx + " packed observation"
        done = (te1 | tr1) != 0
        want_term = _pack(twin, twin._terminal)
        assert torch.equal(packed.terminal_packed_observation[done], want_term[done]), ctx + " terminal rows of the envs that ended"
        assert torch.equal(packed.terminal_packed_observation[~done], prev_term[~done]), ctx + " terminal rows of the other envs moved"
        prev_term = packed.terminal_packed_observation.clone()
        assert torch.equal(packed.terminal_observation["packed"], packed.terminal_packed_observation)
        assert torch.equal(r1, r2) and torch.equal(te1, te2) and torch.equal(tr1, tr2), ctx + " rewards / flags"
        if full:
            assert set(i1) == set(i2)
            for k in i1:
                assert torch.equal(i1[k], i2[k]), f"{ctx} info {k}"
            for k in COUNTERS:
                assert torch.equal(getattr(packed, k), getattr(twin, k)), f"{ctx} wrapper counter {k}"
            assert torch.equal(packed._rows, twin._rows), ctx + " decoded rows"
            logits = torch.rand((E, twin.discrete_n), generator=g, device=dev)
            assert torch.equal(packed.mask_logits(logits.clone(), -1.0), twin.mask_logits(logits.clone(), -1.0)), ctx + " mask_logits (digests)"
            if t % 30 == 29:
                _compare_states(packed.engine.get_state(), twin.engine.get_state(), ctx)
        ended += int(done.sum())
    if stream_ctx is not None:
        stream_ctx.synchronize()
    packed.close(); twin.close()
    return ended


@pytest.mark.parametrize("E", [1000, 1, 64, 65])
@pytest.mark.parametrize("case", ["chain10_discrete", "toyctf_defender_multidiscrete", "toyctf_learned_defender", "chain4_discrete_graph"])
def test_packed_step_equals_the_int32_step_packed_afterwards(case, E):
    """Two wrappers on the same masked-random actions for 90 steps, intercepted actions (on the truncating step too), undiscovered and
    negative indices included: the rows the packed step writes are, bit for bit, mcbs_pack_observation of what the int32 one-launch step
    writes; terminal rows move only for the envs that ended; rewards, flags, infos, counters, decoded rows, digests and the canonical
    state agree.  E = 1000 leaves the last workgroup partly empty; 1, 64 and 65 sit around one workgroup."""
    ended = _twin_run(case, E, 90)
    assert ended > E // 2


def test_packed_terminal_row_of_an_intercepted_last_action_is_the_one_that_stands():
    """Every env intercepted on the truncating step, under a defender that re-images everything (the scenario of
    test_terminal_observation_of_an_intercepted_last_action_is_the_one_that_stands): the packed terminal row is the row that stood — the
    kernel's one read-back — not a pack of a fresh look at the state the defender has changed since."""
    import torch
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.samples import chainpattern
    E, T = 600, 14
    kw = dict(maximum_node_count=12, maximum_total_credentials=12, discrete=True, max_timesteps=T, attacker_goal=ce.AttackerGoal(own_atleast_percent=1.0),
              defender_constraint=ce.DefenderConstraint(0.0), defender_agent=ce.ScanAndReimageCompromisedMachines(1.0, 12, 1), seed=5)
    twin, packed = _twins(chainpattern.new_environment(10), E, **kw)
    dev = twin.engine.device
    g = torch.Generator(device=dev).manual_seed(2)
    for t in range(T):
        if t < T - 1:
            scores = torch.rand((E, twin.discrete_n), generator=g, device=dev)
            a = twin.mask_logits(scores, fill=-1.0).argmax(dim=1)
        else:
            a = torch.full((E,), twin.discrete_n - 1, dtype=torch.int64, device=dev)     # intercepted in every env; this step truncates
            standing = packed.packed_observation.clone()
            fresh_look = _pack(twin, twin.engine.observe(twin.engine.alloc_obs(FIELDS)))
        out = packed.step(a.clone())
        twin.step(a)
        assert torch.equal(packed.packed_observation, twin.observation_packed()), f"step {t}"
    never_ended = (packed.timesteps == 0) & (out[3] != 0)                             # truncated by this step (counters just cleared)
    assert bool(out[4]["invalid_action"].all()) and int(never_ended.sum()) > E // 2
    got = packed.terminal_packed_observation
    assert torch.equal(got[never_ended], standing[never_ended]), "the terminal row is not the row that stood"
    assert torch.equal(got[never_ended], _pack(twin, twin._terminal)[never_ended])
    assert int(((got != fresh_look).any(dim=1) & never_ended).sum()) > 0, "vacuous: no env's state moved on behind its standing observation"
    fresh = packed._packed_fresh[0]
    assert torch.equal(packed.packed_observation[never_ended], fresh.expand(int(never_ended.sum()), -1))
    packed.close(); twin.close()


def _clamped(packing, z, prefix, t):
    """The trace's five fields at step t (None: unindexed), every value clamped to its code by the packing rule"""
    vals = np.concatenate([np.asarray(z[prefix + k] if t is None else z[prefix + k][t]).reshape(-1).astype(np.int64) for k in FIELDS])
    codes = np.asarray(packing.valid_codes)
    return np.where((vals >= 0) & (vals < codes), vals, codes)


def _unpacked(packing, rows):
    got = packing.unpack_host(rows.cpu().numpy())
    return np.concatenate([np.asarray(got[k]).reshape(len(rows), -1).astype(np.int64) for k in FIELDS], axis=1)


@pytest.mark.parametrize("name", WRAP)
def test_packed_step_reproduces_reference_wrapper_traces(name):
    """The traces of the reference's own AttackerEnvWrapper / MaskedDiscreteAttackerWrapper through a packed-mode wrapper: at every step
    the unpacked row is the trace's observation clamped by the packing rule; so are terminal rows and the rows after an auto-reset."""
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd._abi import RNG_TAPE
    from marlon_amd.wrappers import AttackerVecEnv
    z = np.load(os.path.join(parity.GOLDEN, name + ".npz"))
    sj = json.loads(bytes(z["spec_json"]).decode())
    d = sj["defender"]
    env = AttackerVecEnv(parity.topology_for(name[len("wrap_"):]), 1, maximum_node_count=sj["maximum_node_count"],
                         maximum_total_credentials=sj["maximum_total_credentials"], attacker_goal=ce.AttackerGoal(**sj["attacker_goal"]),
                         defender_constraint=ce.DefenderConstraint(sj["maintain_sla"]),
                         defender_agent=None if d is None else ce.ScanAndReimageCompromisedMachines(d[1], d[2], d[3]),
                         max_timesteps=sj["max_timesteps"], discrete=sj["discrete"], rng_kind=RNG_TAPE, materialize_masks=False,
                         observation_format="packed")
    pk = env.observation_packing()
    assert np.array_equal(_unpacked(pk, env.reset()["packed"])[0], _clamped(pk, z, "first_", None)), name + " reset"
    resets = 0
    for t in range(len(z["reward"])):
        ctx = f"{name} step {t}"
        if z["tape"].size:
            env.engine.set_draw_tape(z["tape"][t:t + 1])
        obs, r, te, tr, info = env.step(np.asarray(z["action"][t]).reshape((1,) if sj["discrete"] else (1, 10)))
        assert float(r[0]) == z["reward"][t] and bool(te[0] | tr[0]) == bool(z["terminated"][t] or z["truncated"][t]), ctx
        assert bool(info["invalid_action"][0]) == bool(z["invalid"][t]), ctx + " interception"
        if te[0] or tr[0]:
            assert np.array_equal(_unpacked(pk, env.terminal_packed_observation)[0], _clamped(pk, z, "", t)), ctx + " terminal row"
            assert np.array_equal(_unpacked(pk, obs["packed"])[0], _clamped(pk, z, "after_reset_", resets)), ctx + " row after the auto-reset"
            resets += 1
        else:
            assert np.array_equal(_unpacked(pk, obs["packed"])[0], _clamped(pk, z, "", t)), ctx
    assert resets == int(z["was_reset"].sum()) > 0
    env.close()


def test_packed_step_runs_the_reference_winning_script():
    """The reference's 57-action Chain-10 script (cyberbattle_env_test.py:41-114) as MultiDiscrete rows through a packed-mode wrapper and
    its int32 twin: rows equal, nothing is clamped (every value in range), and the discovered-node count reaches the top of its range."""
    import torch
    from marlon_amd.samples import chainpattern
    z = np.load(os.path.join(parity.GOLDEN, "chain10_script.npz"))
    twin, packed = _twins(chainpattern.new_environment(10), 3, maximum_node_count=12, maximum_total_credentials=12, discrete=False, max_timesteps=2000)
    pk = packed.observation_packing()
    top_nodes = top_creds = 0
    for t in range(56):
        kind, a, b, c, d = (int(v) for v in z["actions"][t])
        first, count = {0: (1, 2), 1: (3, 3), 2: (6, 4)}[kind]      # (l_src, l_vuln) / (r_src, r_tgt, r_vuln) / (c_src, c_tgt, c_port, c_cred)
        md = [kind, 0, 0, 0, 0, 0, 0, 0, 0, 0]
        md[first:first + count] = (a, b, c, d)[:count]
        act = torch.tensor([md] * 3, dtype=torch.int64, device=twin.engine.device)
        o1, r1, te1, tr1, _ = packed.step(act.clone())
        o2, r2, te2, tr2, _ = twin.step(act)
        assert torch.equal(r1, r2) and torch.equal(te1, te2) and bool(te1[0]) == (t == 55), f"script step {t}"
        assert torch.equal(o1["packed"], twin.observation_packed()), f"script step {t}"
        rows = packed.terminal_packed_observation if t == 55 else o1["packed"]
        fields = twin._terminal if t == 55 else twin.observation_fields
        want = np.concatenate([fields[k].cpu().numpy().reshape(3, -1) for k in FIELDS], axis=1)
        assert np.array_equal(_unpacked(pk, rows), want), f"script step {t}: a value was clamped"
        top_nodes, top_creds = max(top_nodes, int(want[0, 6])), max(top_creds, int(want[0, 5]))
    codes = np.asarray(pk.valid_codes)
    assert top_nodes == codes[6] - 1 == 12, "discovered_node_count did not reach the top of its range"
    # credential_cache_length: Chain-10 leaks 11 credentials in all (one per link), the script collects every one, and the bound of 12 leaves
    # the count's last code (12) unreachable for this topology: 11 is the top the script can reach
    assert top_creds == 11 == codes[5] - 2, "credential_cache_length did not reach the 11 credentials Chain-10 has"
    packed.close(); twin.close()


@pytest.mark.parametrize("topology", ["chain4", "toyctf", "tiny"])
def test_packed_step_over_observation_bounds(topology):
    """The bounds of test_one_launch_wrapper_step_over_observation_bounds — rows of 3 .. 16 nodes, 1 .. 16 cache rows, property words
    that end inside a word, counts of every width: the packed rows against the int32 twin's."""
    import torch
    from marlon_amd.samples import chainpattern, tinytoy, toy_ctf
    make = {"chain4": lambda: chainpattern.new_environment(4), "toyctf": toy_ctf.new_environment, "tiny": tinytoy.new_environment}[topology]
    n, c = {"chain4": (6, 5), "toyctf": (10, 5), "tiny": (3, 1)}[topology]
    E, T = 203, 12
    tried = set()
    for nm, cm in ((n, c), (n + 1, c + 1), (n + 2, c + 4), (9, 7), (11, 3), (13, 11), (14, 6), (15, 13), (16, 16), (16, c), (n, 16)):
        nm, cm = max(nm, n), max(cm, c)
        if (nm, cm) in tried:
            continue
        tried.add((nm, cm))
        twin, packed = _twins(make(), E, maximum_node_count=nm, maximum_total_credentials=cm, discrete=True, max_timesteps=T)
        g = torch.Generator(device=twin.engine.device).manual_seed(nm * 31 + cm)
        for t in range(30):
            a = _actions(twin, g, t, T, every=5)
            packed.step(a.clone())
            twin.step(a)
            ctx = f"{topology} bounds ({nm}, {cm}) step {t}"
            assert torch.equal(packed.packed_observation, twin.observation_packed()), ctx + " packed observation"
        packed.close(); twin.close()
    assert len(tried) >= 8


def test_packed_step_writes_nothing_else():
    """Rows wider than W_obs keep their poison from word W_obs on, in live and terminal rows; without auto_reset no terminal row is ever
    written; an env that is neither stepped nor ended keeps its row bit for bit."""
    import torch
    from marlon_amd.samples import chainpattern
    from marlon_amd.wrappers import AttackerVecEnv
    E, T, POISON, MARK = 300, 9, -0x21124211, 0x1234567
    kw = dict(maximum_node_count=12, maximum_total_credentials=12, discrete=True, max_timesteps=T)
    for auto_reset in (True, False):
        twin, packed = _twins(chainpattern.new_environment(10), E, auto_reset=auto_reset, **kw)
        dev, W = twin.engine.device, packed.packed_observation.shape[1]
        live = torch.full((E, W + 3), POISON, dtype=torch.int32, device=dev)
        live[:, :W] = packed.packed_observation
        term = torch.full((E, W + 3), POISON, dtype=torch.int32, device=dev)
        g = torch.Generator(device=dev).manual_seed(9)
        ever_done = torch.zeros(E, dtype=torch.bool, device=dev)
        for t in range(2 * T + 3):
            a = _actions(twin, g, t, T)
            stands = None
            if t == 4:                                           # every env intercepted (the last node index is not discovered yet), none ends:
                a = torch.full((E,), twin.discrete_n - 1, dtype=torch.int64, device=dev)
                live[:, :W] = MARK                               # whatever the rows hold must stand
                stands = live.clone()
            _, wb, _ = packed._next_output_set()
            call = packed.engine.wrapper_step_packed_call(True, packed._rows, packed._packing_handle(), live, term, packed._packed_fresh, wb,
                                                          packed.invalid_action_reward_modifier, T, auto_reset)
            call(a.data_ptr())
            _, r2, te2, tr2, i2 = twin.step(a)
            ctx = f"auto_reset={auto_reset} step {t}"
            assert torch.equal(packed._rewards, r2) and torch.equal(packed._truncated, tr2), ctx
            done = (te2 | tr2) != 0
            assert bool((live[:, W:] == POISON).all()) and bool((term[:, W:] == POISON).all()), ctx + " words beyond W_obs were written"
            if stands is not None:
                assert bool(i2["invalid_action"].all()) and not bool(done.any())
                assert torch.equal(live, stands), ctx + " an env that was neither stepped nor ended lost its row"
                live[:, :W] = twin.observation_packed()         # (the twin's rows stood too)
            else:
                assert torch.equal(live[:, :W], twin.observation_packed()), ctx
            if auto_reset:
                ever_done |= done
                assert bool((term[~ever_done] == POISON).all()), ctx + " a terminal row of an env that never ended was written"
                assert torch.equal(term[done][:, :W], _pack(twin, twin._terminal)[done]), ctx
            else:
                assert bool((term == POISON).all()), ctx + " terminal rows written without auto_reset"
        assert auto_reset is False or int(ever_done.sum()) > E // 2
        packed.close(); twin.close()


def test_packed_mode_consumers_equal_the_int32_twin():
    """features(), features(include_masks=True) and first_layer() in fp32 and bf16, and a rollout buffer over 8 steps with its
    advantages and one minibatch encoded through the row index: the same bits as the int32 twin gives."""
    import torch
    env0, kw = _case("chain10_discrete")
    E = 257
    twin, packed = _twins(env0, E, **kw)
    dev = twin.engine.device
    g = torch.Generator(device=dev).manual_seed(17)
    bufs = [twin.rollout_buffer(8, pack_observations=True), packed.rollout_buffer(8)]
    assert set(bufs[1].observations) == {"packed"} and bufs[1].observations["packed"].shape == bufs[0].observations["packed"].shape
    F = packed.feature_layout().width
    weight = torch.randn((33, F), generator=g, device=dev)
    bias = torch.randn((33,), generator=g, device=dev)
    starts = torch.ones(E, dtype=torch.uint8, device=dev)
    for t in range(8):
        for env, buf in zip((twin, packed), bufs):
            env.observation_packed(out=buf.observations["packed"][buf.pos])
        a = _actions(twin, g, t + 30, kw["max_timesteps"])
        bits = twin.action_masks_packed().clone()
        assert torch.equal(bits, packed.action_masks_packed())
        values = torch.rand(E, generator=g, device=dev)
        log_prob = torch.rand(E, generator=g, device=dev)
        outs = [env.step(a.clone()) for env in (twin, packed)]
        for buf, (o, r, te, tr, info) in zip(bufs, outs):
            buf.add(None, a, r, starts, values, log_prob, bits=bits)
        starts = (outs[0][2] | outs[0][3]).clone()
        for dt in (torch.float32, torch.bfloat16):
            assert torch.equal(packed.features(dtype=dt), twin.features(dtype=dt)), f"step {t} features {dt}"
            assert torch.equal(packed.features(dtype=dt, include_masks=True), twin.features(dtype=dt, include_masks=True)), f"step {t} features + masks {dt}"
            w, b = weight.to(dt), bias.to(dt)
            assert torch.equal(packed.first_layer(w, b, dtype=dt), twin.first_layer(w, b, dtype=dt)), f"step {t} first_layer {dt}"
    last_values = torch.rand(E, generator=g, device=dev)
    for buf in bufs:
        buf.compute_returns_and_advantage(last_values, starts)
    assert torch.equal(bufs[0].observations["packed"], bufs[1].observations["packed"]) and torch.equal(bufs[0].advantages, bufs[1].advantages)
    batches = [next(iter(buf.get(64, generator=torch.Generator(device=dev).manual_seed(3)))) for buf in bufs]
    assert torch.equal(batches[0].index, batches[1].index)
    rows = [env.encode_features_packed(buf.observations["packed"].view(8 * E, -1), index=b.index, dtype=torch.bfloat16)
            for env, buf, b in zip((twin, packed), bufs, batches)]
    assert torch.equal(rows[0], rows[1]) and rows[0].shape[0] == 64
    packed.close(); twin.close()


def test_packed_step_refusals():
    """Library level: a batch of more than 16 nodes, a random-events batch, row_words < W_obs, a packing of another geometry, missing
    terminal / fresh rows under auto_reset, aliased arrays — MCBS_EINVAL with a message, nothing launched, the batch steps afterwards.
    Python level: materialize_masks=True, observation_fields, rollout_buffer(pack_observations=False), TwoAgentVecEnv, MarlonVecEnv."""
    import torch
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.features import ObservationPacking
    from marlon_amd.samples import chainpattern, toy_ctf
    from marlon_amd.vecenv import MarlonVecEnv
    from marlon_amd.wrappers import AttackerVecEnv, DefenderVecEnv, TwoAgentVecEnv
    E = 70
    kw = dict(maximum_node_count=12, maximum_total_credentials=12, discrete=True, max_timesteps=20)
    twin, packed = _twins(chainpattern.new_environment(10), E, **kw)
    dev = twin.engine.device
    eng, lib = packed.engine, packed.engine.lib
    W = packed.packed_observation.shape[1]
    a = torch.zeros(E, dtype=torch.int64, device=dev)
    _, wb, _ = packed._next_output_set()
    before = packed.packed_observation.clone()

    def raw(e, handle, live=None, term=0, fresh=0, row_words=W, md=None, disc=0, auto_reset=1, rows=None, bufs=wb):
        live = packed.packed_observation.data_ptr() if live is None else live
        term = packed.terminal_packed_observation.data_ptr() if term == 0 else term
        fresh = packed._packed_fresh.data_ptr() if fresh == 0 else fresh
        disc = a.data_ptr() if disc == 0 else disc
        rows = (packed._rows if rows is None else rows).data_ptr()
        rc = lib.mcbs_attacker_wrapper_step_packed(e._h, md, disc, rows, C.byref(e._info_struct), handle.ptr, live, term, fresh, row_words, C.byref(bufs),
                                                   -1.0, 20, auto_reset, e._stream())
        return rc, lib.mcbs_last_error()

    def refused(got, text):
        rc, msg = got
        assert rc == EINVAL and text in msg, (rc, msg)

    handle = packed._packing_handle()
    refused(raw(eng, handle, row_words=W - 1), b"shorter")
    refused(raw(eng, handle, term=None), b"packed_terminal")
    refused(raw(eng, handle, fresh=None), b"packed_fresh")
    refused(raw(eng, handle, md=a.data_ptr()), b"exactly one action encoding")
    refused(raw(eng, handle, disc=None), b"exactly one action encoding")
    refused(raw(eng, handle, term=packed.packed_observation.data_ptr()), b"overlaps")
    refused(raw(eng, handle, term=packed.packed_observation.data_ptr() + 4 * W * (E - 1)), b"overlaps")
    refused(raw(eng, handle, fresh=packed.packed_observation.data_ptr() + 8), b"overlaps")
    refused(raw(eng, handle, rows=packed.packed_observation.view(-1)), b"overlaps")
    # arrays of `w` and `info`, written by the same launch: the decoded rows laid onto one of them (1 400 bytes from its first byte; which
    # array of the list the message names depends on what the allocator put behind it)
    refused(raw(eng, handle, rows=packed.episode_returns), b"overlaps")
    refused(raw(eng, handle, rows=eng.info["network_availability"]), b"overlaps")
    # a packing built for another geometry (ToyCtf @12/10 on the Chain-10 batch)
    other = AttackerVecEnv(toy_ctf.new_environment(), E, maximum_node_count=12, maximum_total_credentials=10, discrete=True, materialize_masks=False)
    refused(raw(eng, other._packing_handle()), b"another device or geometry")
    # batches whose wrapper step is not one launch: more than 16 nodes; the random-events defender
    outside = [(chainpattern.new_environment(100), dict(maximum_node_count=102, maximum_total_credentials=102, discrete=True, materialize_masks=False)),
               (toy_ctf.new_environment(), dict(maximum_node_count=12, maximum_total_credentials=10, discrete=True, materialize_masks=False,
                                                defender_agent=ce.ExternalRandomEvents()))]
    for env0, okw in outside:
        big = AttackerVecEnv(env0, E, **okw)
        assert big.engine.wrapper_step_launches(False) == 3
        h = big.engine.observation_packing(ObservationPacking(big.topo, big.spec))
        Wb = h.words
        live, term = (torch.zeros((E, Wb), dtype=torch.int32, device=dev) for _ in range(2))
        fresh = torch.zeros(Wb, dtype=torch.int32, device=dev)
        big._next_output_set()
        refused(raw(big.engine, h, live=live.data_ptr(), term=term.data_ptr(), fresh=fresh.data_ptr(), row_words=Wb, rows=big._rows, bufs=big._wb),
                b"not one launch")
        big.step(torch.zeros(E, dtype=torch.int64, device=dev))                         # still steps
        with pytest.raises(ValueError, match="not one launch"):
            AttackerVecEnv(env0, E, observation_format="packed", **okw)
        big.close()
    other.close()
    torch.cuda.synchronize()
    assert torch.equal(packed.packed_observation, before), "a refused call wrote"
    # Python level
    with pytest.raises(ValueError, match="materialize_masks=False"):
        AttackerVecEnv(chainpattern.new_environment(10), E, observation_format="packed", **kw)
    with pytest.raises(ValueError, match="observation_format"):
        AttackerVecEnv(chainpattern.new_environment(10), E, materialize_masks=False, observation_format="bits", **kw)
    with pytest.raises(RuntimeError, match="unpack_observation"):
        packed.observation_fields
    with pytest.raises(ValueError, match="pack_observations=False"):
        packed.rollout_buffer(4, pack_observations=False)
    with pytest.raises(ValueError, match="observation_format='fields'"):
        MarlonVecEnv(packed)
    joint = AttackerVecEnv(toy_ctf.new_environment(), E, maximum_node_count=12, maximum_total_credentials=10, discrete=True, learned_defender=True,
                           auto_reset=False, materialize_masks=False, observation_format="packed")
    assert not TwoAgentVecEnv.supported(joint)
    with pytest.raises(ValueError, match="observation_format='fields'"):
        TwoAgentVecEnv(joint, DefenderVecEnv(joint))
    joint.step(torch.zeros(E, dtype=torch.int64, device=dev))
    joint.close()
    # ... and the batch still steps, equal to its twin
    for t in range(3):
        o1 = packed.step(a.clone())
        twin.step(a)
        assert torch.equal(o1[0]["packed"], twin.observation_packed())
    unpacked = packed.unpack_observation(packed.packed_observation)
    for k in FIELDS:
        assert torch.equal(unpacked[k], twin.observation_fields[k])
    packed.close(); twin.close()


def test_packed_steps_on_a_side_stream():
    """The twin run for 20 steps inside torch.cuda.stream(side), actions produced and results compared on that stream, no synchronise
    in between."""
    import torch
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ended = _twin_run("chain10_discrete", 1000, 20, stream_ctx=side)
    assert ended >= 0
