"""The mask kernels' OWN-list instantiations (OwnListDiscovery, marlon_amd/csrc/mcbs_logits.hip; launched once a training turn has
stepped the batch) on observations that outlive a defender-side reset.

130 Chain-10 envs play the reference's winning script under `TwoAgentTrainVecEnv`, each with its own delay (tests/training_script.py;
tests/test_training_script_host.py checks the schedule without a GPU).  At turn 50 the defender's timeout re-initialises every env
under the attacker's standing observation: the digest's own discovery order (node 2 at index 1, ..., node 1 last) then differs from
the live list of the fresh env ([0, none, ...]) at every owned index >= 1, on 122 of the 130 envs; on 36 an owned node sits at index
>= 8, in the second list word; 4 envs have not acted, their digest is still the list-less one `reset()` wrote.  Every kernel that
rebuilds the mask from the digest — pack, mask_logits in every launch variant, the key store, both categorical heads in their live
form, the feature rows' mask columns — is compared with the masks the reference recorded for the script step each env stands at,
at turn 30 (live digests that carry a list), 50 (stale), 51 (all fresh) and 57 (live again); a second geometry, 13/13 (odd A, the
local block off a word boundary), at turn 50; and `collect_rollouts` storing keys next to bits over the same schedule.

On the MI355X the three tests take 2.7 s, 0.07 s and 0.04 s; at turn 50 the device shows 122 envs whose mask the live list would get
wrong (36 with an owned index >= 8, 4 that never acted), at 13/13 122 as well, and 60 of 64 in row 50 of the rollout buffers
("Two-agent training turn")."""
import numpy as np
import pytest

from tests import categorical_ref as cr
from tests import linear_head_ref as lr
from tests import training_script as ts
from tests.test_gpu_categorical import _check_modes, _composite, _within
from tests.test_gpu_linear_categorical import _assert_same, _bounded, _linear
from tests.test_gpu_mask_geometry import VARIANTS, _masked_logits_check
from tests.test_gpu_packed_masks import SENTINEL, check_pack, pack_host
from tests.test_gpu_two_agent_training import make_pair

pytestmark = pytest.mark.gpu

E = 130
CHECK_TURNS = (30, 50, 51, 57)


@pytest.fixture(scope="module")
def script():
    return ts.Script()


def pair(script, n_envs, N, C):
    """`make_pair` on Chain-10 with the script's own goal, SLA and rewards; attacker timeout 300, defender timeout 50."""
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.wrappers import TwoAgentTrainVecEnv
    sj = script.spec_json
    att, dfd = make_pair("chain10", n_envs, N, C, True, ts.ATTACKER_TIMEOUT, ts.DEFENDER_TIMEOUT, goal=ce.AttackerGoal(**sj["attacker_goal"]),
                         defender_constraint=ce.DefenderConstraint(maintain_sla=sj["maintain_sla"]), winning_reward=sj["winning_reward"],
                         losing_reward=sj["losing_reward"],
                         maximum_discoverable_credentials_per_action=sj["maximum_discoverable_credentials_per_action"])
    assert TwoAgentTrainVecEnv.supported(att), f"the library does not serve Chain-10 at {N}/{C} with a training turn"
    assert att.discrete_n == script.geometry(N, C).total
    return att, dfd, TwoAgentTrainVecEnv(att, dfd)


def rows_equal(x, want, ctx, rows=None):
    got = x.cpu().numpy()
    want = np.asarray(want).reshape((len(want),) + got.shape[1:])
    if rows is not None:
        got, want = got[rows], want[rows]
    np.testing.assert_array_equal(got, want, err_msg=ctx)


def play_turn(script, sched, att, train, turn, N, C):
    """One turn of the schedule, then: the request bytes are the schedule's, every env holds exactly the recorded observation of the
    script step the schedule names (the do-nothing defender disturbed nothing), and so do the terminal rows where an episode ended."""
    import torch as t
    dev = att.engine.device
    (_, _, _, _, info), _ = train.step(t.as_tensor(sched.actions[turn - 1], device=dev), t.as_tensor(ts.defender_noop(sched.E), device=dev))
    ctx = f"{N}/{C} turn {turn}"
    rows_equal(train.attacker_reset_request, sched.request[turn - 1], ctx + ": request bytes")
    rows_equal(info["dones"], sched.dones[turn - 1].astype(np.uint8), ctx + ": attacker dones")
    want = script.observation(sched.held[turn - 1], N, C)
    for k, v in att.observation_fields.items():
        rows_equal(v, want[k], f"{ctx}: observation {k}")
    ended = sched.dones[turn - 1] & (sched.terminal[turn - 1] != ts.UNKNOWN)
    if ended.any():
        term = script.observation(np.where(ended, sched.terminal[turn - 1], ts.RESET), N, C)
        for k in want:
            rows_equal(att._terminal[k], term[k], f"{ctx}: terminal observation {k}", rows=ended)


# ------------------------------------------------------------------------------------------------------------------ the checks
def dev_bits(att, mask):
    import torch as t
    return t.as_tensor(pack_host(mask).view(np.int32)).to(att.engine.device)


def check_packed(att, script, sched, turn, mask, N, C, ctx):
    """pack_action_mask (fresh buffer, padded rows, offset view) and unpack; where observations stand over re-initialised envs the
    result must DIFFER from the mask the live list would give on every env the host test counted.  -> the number of such envs."""
    import torch as t
    got = check_pack(att.engine, pack_host(mask), ctx)
    assert t.equal(att.unpack_action_mask(got).cpu(), t.as_tensor(mask)), f"{ctx}: unpack"
    assert t.equal(att.action_masks_packed(), got), f"{ctx}: action_masks_packed"
    held = sched.held[turn - 1]
    differs = (mask != script.live_list_mask(held, N, C)).any(axis=1) & sched.stale(turn)
    W = pack_host(mask).shape[1]
    g = got.cpu().numpy().view(np.uint32)[:, :W]
    seen = (g != pack_host(script.live_list_mask(held, N, C))).any(axis=1) & sched.stale(turn)
    np.testing.assert_array_equal(seen, differs, err_msg=f"{ctx}: envs whose packed mask differs from the live-list mask")
    return int(seen.sum())


def check_keys(att, script, sched, turn, mask, N, C, ctx, g):
    """The stored key words are the host mirror's on the expected count, owned bits and script order; they expand (with and without a
    shuffled index) to the expected mask; words past Wk of a padded buffer stay untouched."""
    import torch as t
    from marlon_amd import mask_keys
    eng, dev = att.engine, att.engine.device
    Wk, (W, row_words) = eng.mask_key_words(), eng.packed_mask_words()
    want_bits = pack_host(mask)
    keys = att.action_mask_keys()
    assert tuple(keys.shape) == (sched.E, Wk) and Wk == mask_keys.key_words(att.topo, att.spec)
    want_keys = mask_keys.keys_from_state(*script.key_state(sched.held[turn - 1], att.topo), att.topo, att.spec)
    np.testing.assert_array_equal(keys.cpu().numpy().view(np.uint32), want_keys, err_msg=f"{ctx}: key words vs the host mirror")
    np.testing.assert_array_equal(mask_keys.expand_host(want_keys, att.topo, att.spec), want_bits, err_msg=f"{ctx}: host mirror vs the recorded masks")
    bits = att.expand_mask_keys(keys)
    assert tuple(bits.shape) == (sched.E, row_words)
    b = bits.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(b[:, :W], want_bits, err_msg=f"{ctx}: expand(store())")
    assert not b[:, W:].any()
    index = t.randperm(sched.E, generator=g, device=dev)
    shuffled = att.expand_mask_keys(keys, index).cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(shuffled[:, :W], want_bits[index.cpu().numpy()], err_msg=f"{ctx}: expand through a shuffled index")
    padded = t.full((sched.E, Wk + 4), SENTINEL, dtype=t.int32, device=dev)
    att.action_mask_keys(out=padded)
    assert t.equal(padded[:, :Wk], keys) and bool((padded[:, Wk:] == SENTINEL).all()), f"{ctx}: words past Wk were written"
    wide = t.full((sched.E, Wk + 3), SENTINEL, dtype=t.int32, device=dev)
    att.action_mask_keys(out=wide[:, 1:Wk + 1])
    assert t.equal(wide[:, 1:Wk + 1], keys) and bool((wide[:, 0] == SENTINEL).all()) and bool((wide[:, Wk + 1:] == SENTINEL).all()), f"{ctx}: offset view"


def check_categorical(att, mask, turn, ctx, g):
    """sample_masked (given uniforms, 0 and 0.99999994 among them), argmax, evaluate_masked on the host-packed expected bits, fp32
    and bf16, through test_gpu_categorical._check_modes with its own bounds; sample_masked_uniform."""
    import torch as t
    dev = att.engine.device
    n, A = mask.shape
    bits = dev_bits(att, mask)
    base = t.randn((n, A), generator=g, device=dev, dtype=t.float32) * 4.0
    u = t.rand(n, generator=g, device=dev, dtype=t.float32)
    u[0], u[1] = 0.0, 0.99999994
    K = mask.sum(1)
    for dt in (t.float32, t.bfloat16):
        logits = base.to(dt)
        ref = cr.CategoricalRef(mask, logits.cpu().double().numpy())

        def run(mode, **kw):
            if mode == "evaluate":
                return att.evaluate_masked(bits, logits, kw["actions"])
            return att.sample_masked(logits, seed=0, step=0, deterministic=mode == "argmax", uniforms=kw.get("uniforms"))
        _check_modes(run, ref, mask, logits, u, f"{ctx} {dt}")
    r = att.sample_masked_uniform(seed=31, step=turn)
    ref0 = cr.CategoricalRef(mask, None)
    a = r.actions.cpu().numpy()
    assert mask[np.arange(n), a].all(), f"{ctx}: sample_masked_uniform drew an action outside the mask"
    np.testing.assert_array_equal(a, ref0.sample(cr.philox_u24(31, np.arange(n), turn)), err_msg=f"{ctx}: uniform law")
    np.testing.assert_array_equal(r.n_allowed.cpu().numpy(), K, err_msg=f"{ctx}: uniform n_allowed")
    _within(r.log_prob.cpu().numpy(), -np.log(K), 0.0, f"{ctx} uniform log_prob", rounded=True)
    _within(r.entropy.cpu().numpy(), ref0.entropy, 0.0, f"{ctx} uniform entropy", rounded=True)


def check_linear(att, mask, ctx, g):
    """sample_masked_from_latent, H = 64, fp32 and bf16: on exact inputs bit for bit evaluate_masked_from_latent and the packed form
    on the host-packed expected bits; on general inputs within the fp64 bounds of tests/test_gpu_linear_categorical.py."""
    import torch as t
    eng, dev = att.engine, att.engine.device
    n, A = mask.shape
    H = 64
    bits = dev_bits(att, mask)
    rows = np.arange(n)
    u = t.rand(n, generator=g, device=dev)
    u[0], u[1] = 0.0, 0.99999994
    u24 = cr.u24_of_uniforms(u.cpu().numpy())
    exact = lr.exact_inputs(n, A, H, np.random.default_rng(7))
    for dt in (t.float32, t.bfloat16):
        latent, weight, bias = (t.as_tensor(x, device=dev).to(dt) for x in exact)
        for kw in (dict(deterministic=False, uniforms=u), dict(deterministic=True)):
            mode = "argmax" if kw["deterministic"] else "sample"
            live = att.sample_masked_from_latent(latent, weight, bias, seed=0, step=0, **kw)
            packed = eng.masked_linear_categorical(latent, weight, bias, bits=bits, mode=mode, uniforms=kw.get("uniforms"))
            _assert_same(live, packed, f"{ctx} {dt} exact inputs {mode}: live vs packed on the expected bits")
            _assert_same(att.evaluate_masked_from_latent(bits, latent, weight, bias, live.actions), live, f"{ctx} {dt} exact inputs {mode}: evaluate")
            _assert_same(live, att.sample_masked(_linear(latent, weight, bias), seed=0, step=0, **kw), f"{ctx} {dt} exact inputs {mode}: F.linear's logits")
        np.testing.assert_array_equal(live.n_allowed.cpu().numpy(), mask.sum(1), err_msg=f"{ctx} {dt}: n_allowed")
        # general inputs
        latent = t.randn((n, H), generator=g, device=dev).to(dt)
        weight = (t.randn((A, H), generator=g, device=dev) / H ** 0.5).to(dt)
        bias = t.randn(A, generator=g, device=dev).to(dt)
        x64 = lr.logits64(latent, weight, bias)
        delta = lr.dot_bound(latent, weight, bias, mask)
        ref = cr.CategoricalRef(mask, x64)
        assert (ref.K > 0).all()
        norm, ent_c = _composite(mask, _linear(latent.cpu(), weight.cpu(), bias.cpu()))
        ent_err = float(np.abs(ent_c - ref.entropy).max())
        ent_extra = 4.0 * delta * np.maximum(1.0, np.log(ref.K))
        comp_lp = lambda a: float(np.abs(norm[t.arange(n), t.as_tensor(a)].double().numpy() - ref.log_prob(a)).max())
        what = f"{ctx} {dt} general inputs"
        r = att.sample_masked_from_latent(latent, weight, bias, seed=0, step=0, deterministic=True)
        a = r.actions.cpu().numpy()
        np.testing.assert_array_equal(r.n_allowed.cpu().numpy(), ref.K, err_msg=f"{what} n_allowed")
        assert mask[rows, a].all(), f"{what}: argmax is not allowed"
        assert np.all(ref.m - x64[rows, a] <= 2.0 * delta), f"{what}: argmax further than 2 delta from the maximum"
        _bounded(r.log_prob.cpu().numpy(), ref.log_prob(a), comp_lp(a), 2.0 * delta, f"{what} argmax log_prob")
        _bounded(r.entropy.cpu().numpy(), ref.entropy, ent_err, ent_extra, f"{what} entropy")
        r = att.sample_masked_from_latent(latent, weight, bias, seed=0, step=0, uniforms=u)
        a = r.actions.cpu().numpy()
        assert mask[rows, a].all(), f"{what}: a sampled action is not allowed"
        lo, hi = ref.cdf_interval(a)
        widen = (ref.K + 16) * 2.0 ** -23 + np.expm1(2.0 * delta)
        uu = u24 * 2.0 ** -24
        assert ((lo - widen <= uu) & (uu < hi + widen)).all(), f"{what}: sampled outside the CDF interval"
        _bounded(r.log_prob.cpu().numpy(), ref.log_prob(a), comp_lp(a), 2.0 * delta, f"{what} sample log_prob")
        _bounded(r.entropy.cpu().numpy(), ref.entropy, ent_err, ent_extra, f"{what} sample entropy")
        _assert_same(att.evaluate_masked_from_latent(bits, latent, weight, bias, r.actions), r, f"{what}: evaluate on the expected bits")


def check_features(att, mask, ctx):
    import torch as t
    live = att.features(include_masks=True)
    want = att.encode_features(att.observation_fields, bits=dev_bits(att, mask))
    assert live.shape == want.shape and t.equal(live.view(t.int32), want.view(t.int32)), f"{ctx}: features(include_masks=True)"
    assert int(live.sum()) >= int(mask.sum()) > 0


# ------------------------------------------------------------------------------------------------------------------ the tests
def test_chain10_script_under_the_training_turn(script):
    import torch as t
    N = C = 12
    att, dfd, train = pair(script, E, N, C)
    sched = ts.Schedule(script, script.geometry(N, C), E, max(CHECK_TURNS))
    g = t.Generator(device=att.engine.device).manual_seed(50)
    seen = {}
    for turn in range(1, max(CHECK_TURNS) + 1):
        play_turn(script, sched, att, train, turn, N, C)
        if turn not in CHECK_TURNS:
            continue
        ctx = f"turn {turn}"
        held = sched.held[turn - 1]
        mask = script.expected_mask(held, N, C)
        seen[turn] = check_packed(att, script, sched, turn, mask, N, C, ctx)
        _masked_logits_check(att.engine, mask, g, ctx)
        check_keys(att, script, sched, turn, mask, N, C, ctx, g)
        check_categorical(att, mask, turn, ctx, g)
        check_linear(att, mask, ctx, g)
        check_features(att, mask, ctx)
        print(f"{ctx}: envs at script steps {sorted(set(held.tolist()))[:3]} .. {int(held.max())}, K up to {int(mask.sum(1).max())}, "
              f"{int((script.deepest_owned_index(held) >= 1).sum())} with an owned index >= 1, {seen[turn]} whose live list would give another mask; "
              f"mask_logits variants: {[v[0] for v in VARIANTS]} and the dense fp32 tensor")
    held = sched.held[49]
    deep = int(((script.deepest_owned_index(held) >= 8) & sched.stale(50)).sum())
    never = int((~sched.acted[49]).sum())
    print(f"turn 50 on the device: {seen[50]} envs distinguish the own list from the live one, {deep} of them at an owned index >= 8, {never} never acted")
    assert seen[50] >= 100 and deep >= 20 and never >= 2
    assert seen[30] == seen[51] == seen[57] == 0             # (no observation stands over a re-initialised env at those turns)
    att.close()


def test_second_geometry_13x13(script):
    """A = 17 979: fp32 rows on 4-byte and bf16 rows on 2-byte boundaries only, the local block from bit 8 of a word; the same schedule
    with the waiting action at node index 12; pack, mask_logits and the keys at turn 50."""
    import torch as t
    N = C = 13
    att, dfd, train = pair(script, E, N, C)
    A = att.discrete_n
    assert A == 17979 and script.geometry(N, C).connect_size % 32 == 8
    sched = ts.Schedule(script, script.geometry(N, C), E, 50)
    g = t.Generator(device=att.engine.device).manual_seed(13)
    for turn in range(1, 51):
        play_turn(script, sched, att, train, turn, N, C)
    mask = script.expected_mask(sched.held[49], N, C)
    seen = check_packed(att, script, sched, 50, mask, N, C, "13/13 turn 50")
    _masked_logits_check(att.engine, mask, g, "13/13 turn 50")
    check_keys(att, script, sched, 50, mask, N, C, "13/13 turn 50", g)
    print(f"13/13 turn 50 on the device: {seen} envs distinguish the own list from the live one; mask_logits variants: {[v[0] for v in VARIANTS]} "
          f"and the dense fp32 tensor (rows on 4-byte boundaries)")
    assert seen >= 100
    att.close()


def test_rollouts_store_the_stale_masks_as_keys_and_as_bits(script):
    """Two pairs of 64 envs play the schedule through simulate.collect_rollouts for 52 steps, one buffer storing mask keys, the other
    packed masks: the keys expand to the other buffer's bits row for row, and row 50 — the masks the attackers held before turn 51,
    standing over re-initialised envs — is the host-packed expected one."""
    import torch as t
    from marlon_amd.simulate import collect_rollouts
    n, T, N, C = 64, 52, 12, 12
    sched = ts.Schedule(script, script.geometry(N, C), n, T)
    bufs = []
    for storage in ("keys", "bits"):
        att, dfd, train = pair(script, n, N, C)
        dev = att.engine.device
        ba, bd = att.rollout_buffer(T, mask_storage=storage), dfd.rollout_buffer(T)
        acts = t.as_tensor(sched.actions, device=dev)
        noop = t.as_tensor(ts.defender_noop(n), device=dev)
        step = {"a": 0}

        def pa(env):
            step["a"] += 1
            return acts[step["a"] - 1]
        dones = collect_rollouts(train, pa, lambda env: noop, ba, bd, T)
        assert step["a"] == T and ba.full
        np.testing.assert_array_equal(dones[0].cpu().numpy() != 0, sched.dones[T - 1])
        np.testing.assert_array_equal(ba.actions.cpu().numpy().reshape(T, n), sched.actions)
        bufs.append((att, ba))
    (att_k, kb), (att_b, bb) = bufs
    W, row_words = att_k.engine.packed_mask_words()
    assert kb.mask_bits is None and bb.mask_keys is None
    expanded = att_k.expand_mask_keys(kb.mask_keys.view(T * n, -1)).view(T, n, row_words)
    assert t.equal(expanded, bb.mask_bits), "expand(mask_keys) != mask_bits"
    got = bb.mask_bits.cpu().numpy().view(np.uint32)[:, :, :W]
    for row in range(T):                                     # row t: what the attackers held before turn t + 1
        held = sched.held_before(row + 1)
        np.testing.assert_array_equal(got[row], pack_host(script.expected_mask(held, N, C)), err_msg=f"buffer row {row}")
    assert sched.stale(50).all()
    held = sched.held_before(51)
    differs = (got[50] != pack_host(script.live_list_mask(held, N, C))).any(axis=1)
    print(f"rollout row 50: {int(differs.sum())} of {n} stored masks differ from what the live list would give")
    assert differs.sum() >= 48
    att_k.close()
    att_b.close()
