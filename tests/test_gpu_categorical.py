"""mcbs_masked_categorical / mcbs_masked_categorical_packed (the masked categorical head, include/mcbs.h) against the fp64
restatement tests/categorical_ref.py on the oracle's masks, and against torch's fp32 composite
`Categorical(logits=where(mask, logits, -1e8))` for the error bound.

Error bound of log_prob and entropy: the kernel's largest absolute error against fp64 may not exceed 4 x the largest error of torch's
fp32 CPU composite against fp64 on the same inputs, plus one fp32 ulp of the value (4 x: the summation order differs).  Measured on
the MI355X: see DESIGN.md section 7."""
import functools

import numpy as np
import pytest

from tests import categorical_ref as cr
from tests import parity

pytestmark = pytest.mark.gpu

SMALL = ["scalars", "leaked_credentials", "credential_cache_matrix", "discovered_nodes_properties", "nodes_privilegelevel"]
TRACES = ["chain10_mix_s3", "toyctf_defender_s11", "random24_defender_s51"]


def _composite(mask, logits_cpu):
    """torch fp32 on the CPU from where(mask, logits, -1e8): (normalised logits [n, A], entropy [n]) as fp64 arrays."""
    import torch
    tm = torch.as_tensor(mask)
    dist = torch.distributions.Categorical(logits=torch.where(tm, logits_cpu.float(), torch.tensor(-1e8)))
    norm = dist.logits
    ent = -(torch.where(tm, norm * dist.probs, torch.zeros(()))).sum(-1)
    return norm, ent.double().numpy()


def _within(got, want, comp_err, what, rounded=False):
    """|got - want| <= 4 * comp_err + one fp32 ulp of the value; returns the kernel's largest error.  rounded (the uniform law: no
    composite, the value is a single -log K): "equal to 1 ulp" is read as at most one fp32 step away from the correctly rounded fp32 value."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if rounded:
        want = want.astype(np.float32).astype(np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    comp_err = np.broadcast_to(np.asarray(comp_err, dtype=np.float64), err.shape)
    print(f"{what}: kernel max abs error {err.max():.3e}, fp32 composite {comp_err.max():.3e}")
    bound = 4.0 * comp_err + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    worst = int(np.argmax(err - bound))
    assert np.all(err <= bound), f"{what}: row {worst}: error {err[worst]:.3e} > bound {bound[worst]:.3e} (value {want[worst]!r})"
    return float(err.max())


def _check_modes(run, ref, mask, logits, u, what, comp=None):
    """All three modes of one call site against the restatement.  run(mode, **kw) -> MaskedCategorical; logits: the device tensor (or
    None); u: device float32 uniforms [n].  Returns (kernel error, composite error) of log_prob and of the entropy."""
    import torch
    n, A = mask.shape
    rows = np.arange(n)
    figures = {}
    # The composite's error is taken over the rows WITH allowed actions only, and that figure bounds every row.  On a blank row torch's
    # fp32 composite normalises logits that are all -1e8 (one ulp there is 8) and is off by up to 0.5: counting that in would let any
    # log_prob pass, so the blank rows (-log A, entropy 0) are held to what the other rows' composite achieves.
    nz = ref.K > 0
    if logits is not None:
        norm, ent_c = comp if comp is not None else _composite(mask, logits.cpu())
        ent_err = float(np.abs(ent_c - ref.entropy)[nz].max()) if nz.any() else 0.0
    else:
        norm, ent_err = None, 0.0

    def comp_lp_err(actions):
        if norm is None or not nz.any():
            return 0.0
        c = norm[torch.arange(n), torch.as_tensor(actions)].double().numpy()
        return float(np.abs(c - ref.log_prob(actions))[nz].max())

    before = None if logits is None else logits.clone()
    # ARGMAX: exact, the lowest index among equal logits
    r = run("argmax")
    np.testing.assert_array_equal(r.n_allowed.cpu().numpy(), ref.K, err_msg=f"{what} n_allowed")
    a = r.actions.cpu().numpy()
    np.testing.assert_array_equal(a, ref.argmax, err_msg=f"{what} argmax")
    figures["argmax_lp"] = (_within(r.log_prob.cpu().numpy(), ref.log_prob(a), comp_lp_err(a), f"{what} argmax log_prob", norm is None), comp_lp_err(a))
    figures["entropy"] = (_within(r.entropy.cpu().numpy(), ref.entropy, ent_err, f"{what} entropy", norm is None), ent_err)
    # SAMPLE with explicit uniforms: allowed, and inside the fp64 CDF interval of the action widened by (K + 16) * 2^-23
    r = run("sample", uniforms=u)
    a = r.actions.cpu().numpy()
    u24 = cr.u24_of_uniforms(u.cpu().numpy())
    uu = u24 * 2.0 ** -24
    np.testing.assert_array_equal(r.n_allowed.cpu().numpy(), ref.K, err_msg=f"{what} sample n_allowed")
    blank = ref.K == 0
    np.testing.assert_array_equal(a[blank], (u24[blank] * A) >> 24, err_msg=f"{what} blank rows")
    assert np.all((a >= 0) & (a < A)) and mask[rows[~blank], a[~blank]].all(), f"{what}: a sampled action is not allowed"
    if logits is None:
        np.testing.assert_array_equal(a, ref.sample(u24), err_msg=f"{what} uniform law")
    else:
        lo, hi = ref.cdf_interval(a)
        delta = (ref.K + 16) * 2.0 ** -23
        ok = (lo - delta <= uu) & (uu < hi + delta)
        assert ok[~blank].all(), f"{what}: rows {np.nonzero(~ok & ~blank)[0][:8]} sampled outside their CDF interval"
    figures["sample_lp"] = (_within(r.log_prob.cpu().numpy(), ref.log_prob(a), comp_lp_err(a), f"{what} sample log_prob", norm is None), comp_lp_err(a))
    _within(r.entropy.cpu().numpy(), ref.entropy, ent_err, f"{what} sample entropy", norm is None)
    # EVALUATE of the sampled actions: the same numbers, bit for bit; and two identical calls agree bitwise
    e1 = run("evaluate", actions=r.actions)
    e2 = run("evaluate", actions=r.actions)
    for x, y, z in zip(e1[1:], e2[1:], r[1:]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), z.view(torch.int32)), f"{what}: not bitwise reproducible"
    r2 = run("sample", uniforms=u)
    assert torch.equal(r2.actions, r.actions) and torch.equal(r2.log_prob.view(torch.int32), r.log_prob.view(torch.int32))
    if before is not None:
        assert torch.equal(logits.view(torch.int16 if logits.dtype == torch.bfloat16 else torch.int32),
                           before.view(torch.int16 if logits.dtype == torch.bfloat16 else torch.int32)), f"{what}: logits were modified"
    return figures


@functools.lru_cache(maxsize=None)
def _live_run(trace):
    """Test 1 for one trace; returns the K values seen and the error figures."""
    import torch
    from marlon_amd import engine
    from marlon_amd._abi import RNG_PHILOX
    from oracle.oracle import Oracle
    _, sj = parity.load_trace(trace)
    topo = parity.topology_for(trace)
    E = 1024 if topo.n_nodes <= 12 else 256
    mk = lambda n, base: parity.spec_from_json(sj, n_envs=n, auto_reset=True, rng_kind=RNG_PHILOX, seed=17, max_episode_steps=60, env_id_base=base)
    spec = mk(E, 0)
    eng = engine.BatchEngine(topo, spec)
    upper = engine.BatchEngine(topo, mk(E // 2, E // 2))         # the upper half of the batch as a shard of its own
    orc = Oracle(topo, spec)
    A = eng.discrete_action_count()
    obs, obs_u = eng.alloc_obs(SMALL), upper.alloc_obs(SMALL)
    g = torch.Generator(device=eng.device).manual_seed(2)
    seen = {"K0": 0, "K64": 0, "K2048": 0, "Kmax": 0, "figures": []}
    T = 41
    # Forty steps of random play never reach the late game (largest K seen on the MI355X: 322 / 309 / 98 on the three traces), and rows
    # with thousands of allowed actions are what the kernel's loops must be tested on: 32 envs of the Chain-10 batch play the
    # reference's own winning script (tests/golden/chain10_script.npz, same spec: K = 2 478 after 28 steps, 5 383 after 41).
    script = None
    if trace == "chain10_mix_s3":
        script = torch.as_tensor(parity.load_trace("chain10_script")[0]["actions"][:T], device=eng.device)
    for t in range(T):
        a = eng.sample_actions(t % 5 != 4, seed=9, step=t)       # every fifth step uniform over the bounds: out-of-bound actions blank the observation
        au = upper.sample_actions(t % 5 != 4, seed=9, step=t)
        assert torch.equal(au, a[E // 2:])
        if script is not None:                                   # the last 32 envs play the winning script (see below)
            a[E - 32:] = script[t]
            au[E // 2 - 32:] = script[t]
        check = t % 7 == 6 or t == T - 1
        oo = orc.alloc_obs(SMALL + ["mask_local", "mask_remote", "mask_connect"]) if check else None
        if check:
            eng.step_observe(a, obs)
            upper.step_observe(au, obs_u)
        else:
            eng.step(a)
            upper.step(au)
        orc.step(a.cpu().numpy(), obs=oo)
        if not check:
            continue
        for f in SMALL:
            np.testing.assert_array_equal(obs[f].cpu().numpy(), oo[f], err_msg=f"{trace} step {t} obs {f}")
        mask = np.concatenate([oo["mask_connect"].reshape(E, -1), oo["mask_local"].reshape(E, -1), oo["mask_remote"].reshape(E, -1)], axis=1) != 0
        assert mask.shape == (E, A)
        K = mask.sum(1)
        seen["K0"] += int((K == 0).sum()); seen["K64"] += int((K > 64).sum()); seen["K2048"] += int((K > 2048).sum())
        seen["Kmax"] = max(seen["Kmax"], int(K.max()))
        base = torch.randn((E, A), generator=g, device=eng.device, dtype=torch.float32) * 4.0
        u = torch.rand(E, generator=g, device=eng.device, dtype=torch.float32)
        u[0], u[1] = 0.0, 0.99999994
        for dt in (torch.float32, torch.bfloat16):
            logits = base.to(dt)
            ref = cr.CategoricalRef(mask, logits.cpu().double().numpy())
            what = f"{trace} step {t} {dt}"
            fig = _check_modes(lambda mode, **kw: eng.masked_categorical(logits, mode=mode, **kw), ref, mask, logits, u, what)
            seen["figures"].append((what, fig))
            # SAMPLE keyed by Philox (seed, env_id_base + e, step) == SAMPLE with the u the host derives from the documented keying
            u24 = cr.philox_u24(123456789012, np.arange(E), t)
            uh = torch.as_tensor((u24 * 2.0 ** -24).astype(np.float32), device=eng.device)
            rk = eng.masked_categorical(logits, mode="sample", seed=123456789012, step=t)
            ru = eng.masked_categorical(logits, mode="sample", uniforms=uh)
            assert torch.equal(rk.actions, ru.actions) and torch.equal(rk.log_prob.view(torch.int32), ru.log_prob.view(torch.int32)), what
            r_up = upper.masked_categorical(logits[E // 2:], mode="sample", seed=123456789012, step=t)      # a view: rows E/2 .. E of the same buffer
            assert torch.equal(r_up.actions, rk.actions[E // 2:]) and torch.equal(r_up.n_allowed, rk.n_allowed[E // 2:]), f"{what}: shard"
            assert torch.equal(r_up.log_prob.view(torch.int32), rk.log_prob[E // 2:].view(torch.int32))
            r_other = eng.masked_categorical(logits, mode="sample", seed=123456789012, step=t + 1)
            assert not torch.equal(r_other.actions, rk.actions), f"{what}: the step does not key the draw"
        # an offset view: rows neither 16-byte aligned nor a multiple of four long, in a wider buffer
        wide = torch.zeros((E, A + 3), device=eng.device, dtype=torch.float32)
        view = wide[:, 1:A + 1]
        view.copy_(base)
        rv = eng.masked_categorical(view, mode="sample", uniforms=u)
        rb = eng.masked_categorical(base, mode="sample", uniforms=u)
        assert torch.equal(rv.actions, rb.actions) and torch.equal(rv.log_prob.view(torch.int32), rb.log_prob.view(torch.int32))
    eng.close(); upper.close()
    return seen


@pytest.mark.parametrize("trace", TRACES)
def test_live_form_against_oracle_mask(trace):
    seen = _live_run(trace)
    print(trace, {k: v for k, v in seen.items() if k != "figures"})
    for what, fig in seen["figures"]:
        print(what, {k: (f"{a:.3e}", f"{b:.3e}") for k, (a, b) in fig.items()})


def test_live_runs_cover_blank_medium_and_large_rows():
    """The three traces together must have shown rows with K = 0, K > 64 and K > 2 048: otherwise the kernel's loops are untested."""
    seen = [_live_run(t) for t in TRACES]
    print({t: {k: v for k, v in s.items() if k != "figures"} for t, s in zip(TRACES, seen)})
    assert sum(s["K0"] for s in seen) > 0, "no blank row"
    assert sum(s["K64"] for s in seen) > 0, "no row with K > 64"
    assert sum(s["K2048"] for s in seen) > 0, "no row with K > 2048"


# ---------------------------------------------------------------------------------------------------------------- packed form
def _chain4_engine(n_envs=64, **kw):
    from marlon_amd import engine
    from marlon_amd._abi import EnvSpec
    from marlon_amd.flatten import flatten
    from marlon_amd.samples import chainpattern
    topo = flatten(chainpattern.new_environment(4))
    return engine.BatchEngine(topo, EnvSpec(n_envs=n_envs, maximum_node_count=6, maximum_total_credentials=6,
                                            attacker_goal=dict(own_atleast_percent=1.0), **kw))


def _synthetic_masks(A, n=64):
    """64 hand-made rows: the listed corner cases first, random densities after."""
    rng = np.random.default_rng(11)
    mask = np.zeros((n, A), dtype=bool)
    mask[0, 0] = True                                    # only bit 0
    mask[1, A - 1] = True                                # only bit A-1
    mask[2, :] = True                                    # all A bits
    # row 3: no bits
    mask[4, ::2] = True                                  # alternating bits
    mask[5, 1::2] = True
    w0 = np.arange(0, A, 32)
    mask[6, np.minimum(w0 + (7 * (w0 // 32)) % 32, A - 1)] = True     # one bit per word
    mask[7, [3, 4, 5]] = True                            # +-80 next to 0 (logits below)
    mask[8, [31, 32, 63, 64, A - 2]] = True              # word boundaries
    for i in range(9, n):
        mask[i] = rng.random(A) < rng.random() ** 3
    return mask


def _pack(mask, row_words, garbage_tail=False):
    n, A = mask.shape
    W = (A + 31) // 32
    m = np.zeros((n, row_words * 32), dtype=np.uint64)
    m[:, :A] = mask
    if garbage_tail:
        m[:, A:W * 32] = 1                               # bits at or beyond A in word W-1: to be ignored
    words = (m.reshape(n, row_words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    if garbage_tail:
        words[:, W:] = 0xDEADBEEF                        # words beyond W are not the mask's
    return words.view(np.int32)


def test_packed_form_on_synthetic_masks():
    import torch
    eng = _chain4_engine()
    dev = eng.device
    A = eng.discrete_action_count()
    W, row_words = eng.packed_mask_words()
    assert A == 1830 and W == 58 and A % 32 != 0
    n = 64
    mask = _synthetic_masks(A, n)
    g = torch.Generator(device=dev).manual_seed(4)
    base = torch.randn((n, A), generator=g, device=dev) * 4.0
    base[7, 3], base[7, 4], base[7, 5] = 80.0, 0.0, -80.0      # only the max subtraction keeps these finite
    base[8, [31, 32, 63, 64, A - 2]] = 2.5                     # all equal: the lowest index
    u = torch.rand(n, generator=g, device=dev)
    u[0], u[1], u[2] = 0.0, 0.99999994, 0.99999994
    # bits: rows of W + 6 words with garbage in the tail bits and beyond W; and clean dense rows of exactly row_words
    bits_wide = torch.as_tensor(_pack(mask, W + 6, garbage_tail=True), device=dev)
    bits_clean = torch.as_tensor(_pack(mask, row_words), device=dev)
    for dt in (torch.float32, torch.bfloat16):
        # logits: a view offset by one element with row_stride > A and sentinels around it
        wide = torch.full((n, A + 7), 7.0, device=dev, dtype=dt)
        logits = wide[:, 1:A + 1]
        logits.copy_(base.to(dt))
        ref = cr.CategoricalRef(mask, logits.cpu().double().numpy())
        comp = _composite(mask, logits.cpu())
        what = f"packed {dt}"
        _check_modes(lambda mode, **kw: eng.masked_categorical(logits, bits=bits_wide, mode=mode, **kw), ref, mask, logits, u, what, comp)
        assert bool((wide[:, 0] == 7.0).all()) and bool((wide[:, A + 1:] == 7.0).all()), "sentinels touched"
        r_wide = eng.masked_categorical(logits, bits=bits_wide, mode="sample", uniforms=u)
        r_clean = eng.masked_categorical(logits.contiguous(), bits=bits_clean, mode="sample", uniforms=u)
        for x, y in zip(r_wide, r_clean):
            assert torch.equal(x, y) or torch.equal(x.view(torch.int32), y.view(torch.int32)), "tail bits / row strides change the result"
        lp7 = r_wide.log_prob[7].item()
        assert np.isfinite(lp7) and np.isfinite(r_wide.entropy[7].item())
        # EVALUATE: allowed and disallowed actions inside the range against the fp32 torch composite (rtol 2^-22), -1 and A -> NaN
        norm = comp[0]
        rng = np.random.default_rng(12)
        acts = rng.integers(0, A, n)
        acts[0], acts[1], acts[2], acts[3] = 0, 0, A - 1, 5          # allowed, disallowed, allowed, blank row
        acts[9], acts[10] = -1, A
        bad = torch.zeros(1, dtype=torch.int32, device=dev) + 5      # increased, not zeroed
        ta = torch.as_tensor(acts, device=dev)
        r = eng.masked_categorical(logits, bits=bits_wide, mode="evaluate", actions=ta, bad_actions=bad)
        assert int(bad.item()) == 7 and torch.equal(ta.cpu(), torch.as_tensor(acts)), "bad_actions must rise by exactly 2"
        lp = r.log_prob.cpu().numpy().astype(np.float64)
        assert np.isnan(lp[9]) and np.isnan(lp[10])
        inside = np.ones(n, dtype=bool)
        inside[[9, 10]] = False
        rows = np.arange(n)[inside]
        want = norm[torch.as_tensor(rows), torch.as_tensor(acts[inside])].double().numpy()
        on = mask[rows, acts[inside]]
        assert on.any() and (~on).any()
        # (blank rows are left to the restatement below: there the composite itself normalises logits that are all -1e8 and is off by
        # up to half an ulp of 1e8 = 4, far more than the -log A it should give)
        live = ref.K[rows] > 0
        assert (~on & live).sum() > 20
        np.testing.assert_allclose(lp[inside][~on & live], want[~on & live], rtol=2.0 ** -22, err_msg=f"{what}: disallowed actions")
        ref_lp = ref.log_prob(acts)
        comp_err = float(np.abs(want - ref_lp[inside])[on].max())              # (an allowed action: the row is not blank)
        _within(lp[inside][on], ref_lp[inside][on], comp_err, f"{what} evaluate allowed")
        np.testing.assert_allclose(lp[inside][~on], ref_lp[inside][~on], rtol=2.0 ** -22)
        nzr = ref.K > 0
        _within(r.entropy.cpu().numpy()[inside], ref.entropy[inside], float(np.abs(comp[1] - ref.entropy)[nzr].max()), f"{what} evaluate entropy")
    # the uniform law on the same rows
    ref0 = cr.CategoricalRef(mask, None)
    _check_modes(lambda mode, **kw: eng.masked_categorical(None, bits=bits_wide, mode=mode, **kw), ref0, mask, None, u, "packed uniform")
    # Philox keyed by the row index
    rk = eng.masked_categorical(base, bits=bits_clean, mode="sample", seed=77, step=3)
    uh = torch.as_tensor((cr.philox_u24(77, np.arange(n), 3) * 2.0 ** -24).astype(np.float32), device=dev)
    ru = eng.masked_categorical(base, bits=bits_clean, mode="sample", uniforms=uh)
    assert torch.equal(rk.actions, ru.actions)
    # n_rows = 0
    r0 = eng.masked_categorical(base[:0], bits=bits_clean[:0], mode="sample")
    assert all(x.shape == (0,) for x in r0)
    eng.close()


def test_packed_form_more_rows_than_one_grid():
    """One grid covers 4 * 65 536 rows: rows beyond are reached by the stride loop.  The 64 synthetic rows tiled; ARGMAX and EVALUATE do
    not depend on the row key, so every tile must repeat the first bit for bit."""
    import torch
    eng = _chain4_engine()
    dev = eng.device
    A = eng.discrete_action_count()
    W, row_words = eng.packed_mask_words()
    mask = _synthetic_masks(A)
    reps = 4 * 65536 // 64 + 3
    n = reps * 64
    bits = torch.as_tensor(_pack(mask, row_words), device=dev).repeat(reps, 1)
    g = torch.Generator(device=dev).manual_seed(4)
    logits = (torch.randn((64, A), generator=g, device=dev) * 4.0).to(torch.bfloat16).repeat(reps, 1)
    r = eng.masked_categorical(logits, bits=bits, mode="argmax")
    ref = cr.CategoricalRef(mask, logits[:64].cpu().double().numpy())
    np.testing.assert_array_equal(r.actions[:64].cpu().numpy(), ref.argmax)
    np.testing.assert_array_equal(r.n_allowed[-64:].cpu().numpy(), ref.K)
    for x in r:
        assert torch.equal(x.view(reps, 64), x[:64].expand(reps, 64)), "a tile differs from the first"
    e = eng.masked_categorical(logits, bits=bits, mode="evaluate", actions=r.actions)
    assert torch.equal(e.log_prob.view(torch.int32), r.log_prob.view(torch.int32))
    s = eng.masked_categorical(None, bits=bits, mode="sample", seed=5, step=1)
    u24 = cr.philox_u24(5, np.arange(n - 64, n), 1)
    np.testing.assert_array_equal(s.actions[-64:].cpu().numpy(), cr.CategoricalRef(mask, None).sample(u24))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- wrappers
def test_rollout_buffer_pattern_evaluates_bit_for_bit():
    """Chain-10 @ 12/12, 512 envs: packed masks, sampled actions and log_prob stored for 8 steps; evaluate_masked on a shuffled minibatch
    returns the stored log_prob bit for bit (same kernel, same order)."""
    import torch
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.samples import chainpattern
    from marlon_amd.wrappers import AttackerVecEnv
    E, T = 512, 8
    env = AttackerVecEnv(chainpattern.new_environment(10), E, maximum_node_count=12, maximum_total_credentials=12,
                         attacker_goal=ce.AttackerGoal(own_atleast_percent=1.0), max_timesteps=50, discrete=True, materialize_masks=False)
    dev = env.engine.device
    A = env.discrete_n
    W, row_words = env.engine.packed_mask_words()
    g = torch.Generator(device=dev).manual_seed(8)
    buf = torch.zeros((T, E, row_words), dtype=torch.int32, device=dev)
    logits = torch.empty((T, E, A), dtype=torch.bfloat16, device=dev)
    acts = torch.zeros((T, E), dtype=torch.int64, device=dev)
    lps = torch.zeros((T, E), dtype=torch.float32, device=dev)
    ents = torch.zeros((T, E), dtype=torch.float32, device=dev)
    for t in range(T):
        env.action_masks_packed(out=buf[t])
        logits[t] = (torch.randn((E, A), generator=g, device=dev) * 3.0).to(torch.bfloat16)
        r = env.sample_masked(logits[t], seed=3, step=t)
        acts[t], lps[t], ents[t] = r.actions, r.log_prob, r.entropy
        _, _, _, _, info = env.step(r.actions)
        assert not bool(info["invalid_action"].any()), f"step {t}: a sampled action was not valid"
    perm = torch.randperm(T * E, generator=torch.Generator().manual_seed(1))[:2048].to(dev)
    mb_bits = buf.view(T * E, row_words)[perm]
    mb_logits = logits.view(T * E, A)[perm]
    r = env.evaluate_masked(mb_bits, mb_logits, acts.view(-1)[perm])
    assert torch.equal(r.log_prob.view(torch.int32), lps.view(-1)[perm].view(torch.int32))
    assert torch.equal(r.entropy.view(torch.int32), ents.view(-1)[perm].view(torch.int32))
    assert bool(torch.isfinite(r.log_prob).all()) and bool((r.n_allowed > 0).all())
    env.close()


def test_uniform_law_live():
    """logits=None: exactly the ((u24 * K) >> 24)-th set bit of the oracle's mask, log_prob = -log K to one ulp; and a lean wrapper that
    steps with sample_masked_uniform never reports an invalid action."""
    import torch
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd import engine
    from marlon_amd._abi import RNG_PHILOX
    from marlon_amd.samples import chainpattern
    from marlon_amd.wrappers import AttackerVecEnv
    from oracle.oracle import Oracle
    trace = "chain10_mix_s3"
    _, sj = parity.load_trace(trace)
    topo = parity.topology_for(trace)
    E = 512
    spec = parity.spec_from_json(sj, n_envs=E, auto_reset=True, rng_kind=RNG_PHILOX, seed=17, max_episode_steps=60, env_id_base=4096)
    eng = engine.BatchEngine(topo, spec)
    orc = Oracle(topo, spec)
    obs = eng.alloc_obs(SMALL)
    for t in range(20):
        a = eng.sample_actions(t % 5 != 4, seed=9, step=t)
        if t % 6 != 5:
            eng.step(a)
            orc.step(a.cpu().numpy())
            continue
        oo = orc.alloc_obs(SMALL + ["mask_local", "mask_remote", "mask_connect"])
        eng.step_observe(a, obs)
        orc.step(a.cpu().numpy(), obs=oo)
        mask = np.concatenate([oo["mask_connect"].reshape(E, -1), oo["mask_local"].reshape(E, -1), oo["mask_remote"].reshape(E, -1)], axis=1) != 0
        ref = cr.CategoricalRef(mask, None)
        r = eng.masked_categorical(None, mode="sample", seed=31, step=t)
        u24 = cr.philox_u24(31, 4096 + np.arange(E), t)                 # keyed by the global env id
        np.testing.assert_array_equal(r.actions.cpu().numpy(), ref.sample(u24))
        np.testing.assert_array_equal(r.n_allowed.cpu().numpy(), ref.K)
        want = np.where(ref.K > 0, -np.log(np.maximum(ref.K, 1)), -np.log(mask.shape[1]))
        lp = r.log_prob.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(lp - want) <= np.spacing(np.abs(want).astype(np.float32))), "log_prob != -log K to one ulp"
        ent = r.entropy.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(ent - ref.entropy) <= np.spacing(np.abs(ref.entropy).astype(np.float32)))
    eng.close()
    lean = AttackerVecEnv(chainpattern.new_environment(10), 512, maximum_node_count=12, maximum_total_credentials=12,
                          attacker_goal=ce.AttackerGoal(own_atleast_percent=1.0), max_timesteps=25, discrete=True, materialize_masks=False)
    for t in range(30):
        r = lean.sample_masked_uniform(seed=2, step=t)
        _, _, _, _, info = lean.step(r.actions)
        assert not bool(info["invalid_action"].any()), f"step {t}"
    lean.close()


def test_refusals():
    """The stale-digest sequence of test_mask_logits_refuses_stale_digests: the live form raises with the same messages, the packed form
    works throughout; ExternalRandomEvents batches refuse the live form; wrong dtype / shape / device raise ValueError."""
    import torch
    from marlon_amd import engine
    eng = _chain4_engine()
    dev = eng.device
    A = eng.discrete_action_count()
    W, row_words = eng.packed_mask_words()
    logits = torch.zeros((64, A), device=dev)
    bits = torch.full((64, row_words), 0x55555555, dtype=torch.int32, device=dev)
    small = eng.alloc_obs(["scalars", "nodes_privilegelevel"])

    def packed_ok():
        r = eng.masked_categorical(logits, bits=bits, mode="argmax")
        assert bool((r.actions == 0).all()) and bool((r.n_allowed == (A + 1) // 2).all())

    with pytest.raises(engine.McbsError, match="no observation"):
        eng.masked_categorical(logits)
    packed_ok()
    eng.observe(small)
    eng.masked_categorical(logits)
    for t in range(5):
        eng.step(eng.sample_actions(True, seed=1, step=t))
    eng.masked_categorical(logits)                           # steps do not invalidate: the mask is the LAST OBSERVATION's by definition
    m = torch.zeros(64, dtype=torch.uint8, device=dev)
    m[::3] = 1
    eng.reset(m)
    with pytest.raises(engine.McbsError, match="reset by mask"):
        eng.masked_categorical(logits)
    packed_ok()
    eng.observe(small, env_mask=m)
    eng.masked_categorical(logits)
    hdr, nodes, order, cache = eng.get_state()
    eng.set_state(hdr, nodes, order, cache)
    with pytest.raises(engine.McbsError, match="no observation"):
        eng.masked_categorical(logits)
    packed_ok()
    eng.observe(small)
    eng.masked_categorical(logits)
    eng.reset()
    with pytest.raises(engine.McbsError, match="no observation"):
        eng.masked_categorical(None)
    packed_ok()
    eng.observe(small)
    # argument checks
    acts = torch.zeros(64, dtype=torch.int64, device=dev)
    for bad_call in (
        lambda: eng.masked_categorical(logits.double()),
        lambda: eng.masked_categorical(logits.half()),
        lambda: eng.masked_categorical(logits[:, :A - 1]),
        lambda: eng.masked_categorical(logits[:32]),
        lambda: eng.masked_categorical(logits.cpu()),
        lambda: eng.masked_categorical(logits.t().contiguous().t()),
        lambda: eng.masked_categorical(logits, mode="mean"),
        lambda: eng.masked_categorical(logits, mode="evaluate"),
        lambda: eng.masked_categorical(logits, mode="evaluate", actions=acts.int()),
        lambda: eng.masked_categorical(logits, mode="evaluate", actions=acts[:5]),
        lambda: eng.masked_categorical(logits, mode="sample", actions=acts),
        lambda: eng.masked_categorical(logits, uniforms=torch.zeros(64, dtype=torch.float64, device=dev)),
        lambda: eng.masked_categorical(logits, uniforms=torch.zeros(63, device=dev)),
        lambda: eng.masked_categorical(logits, bits=bits.long()),
        lambda: eng.masked_categorical(logits, bits=bits[:, :W - 1]),
        lambda: eng.masked_categorical(logits, bits=bits[:10]),
        lambda: eng.masked_categorical(logits, bits=bits.cpu()),
        lambda: eng.masked_categorical(logits, out=(acts.int(), None, None, None)),
        lambda: eng.masked_categorical(logits, mode="evaluate", actions=acts, bad_actions=torch.zeros(1, device=dev)),
    ):
        with pytest.raises(ValueError):
            bad_call()
    eng.close()
    ere = _chain4_engine(defender=("random_events",))
    small = ere.alloc_obs(["scalars", "nodes_privilegelevel"])
    ere.observe(small)
    with pytest.raises(engine.McbsError, match=r"\(-5\).*ExternalRandomEvents"):
        ere.masked_categorical(logits)
    r = ere.masked_categorical(logits, bits=bits, mode="argmax")       # the packed form serves every defender kind
    assert bool((r.actions == 0).all())
    ere.close()
