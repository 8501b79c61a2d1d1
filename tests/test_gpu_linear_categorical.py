"""mcbs_masked_linear_categorical / _packed (the masked action head from the latent, include/mcbs.h): the head computes the allowed
logits itself from the policy's latent and action_net's weight and bias.

Two kinds of checks.  On tests/linear_head_ref.exact_inputs every dot product is exact in fp32 in any order, so the fused call must be
BIT FOR BIT masked_categorical on torch.nn.functional.linear's logits (tests 1, 2): this pins everything after the logits to the
already-tested head.  On general inputs the dot product is inexact and its order differs from a GEMM's: the outputs are held to the fp64
restatement (tests/categorical_ref.py on tests/linear_head_ref.logits64) within bounds derived from delta, the row's dot_bound:
  log_prob   the existing rule (4 x the error of torch's fp32 CPU composite F.linear -> where -> Categorical, plus one fp32 ulp) + 2 delta
  entropy    the existing rule + 4 delta max(1, log K)
  ARGMAX     the returned action's fp64 logit within 2 delta of the fp64 maximum
  SAMPLE     allowed, and u inside the action's fp64 CDF interval widened by (K + 16) 2^-23 + expm1(2 delta)
bfloat16: the head widens bf16 inputs exactly and computes in float32, so the logits buffer it must reproduce is F.linear on the widened
values (tests/test_linear_head_ref.py).  Measured on the MI355X: see DESIGN.md section 7."""
import functools

import numpy as np
import pytest

from tests import categorical_ref as cr
from tests import linear_head_ref as lr
from tests import parity
from tests.test_gpu_categorical import _chain4_engine, _composite, _pack, _synthetic_masks

pytestmark = pytest.mark.gpu

SMALL = ["scalars", "leaked_credentials", "credential_cache_matrix", "discovered_nodes_properties", "nodes_privilegelevel"]


def _bits_equal(x, y):
    import torch
    if x.dtype == torch.float32:
        return torch.equal(x.view(torch.int32), y.view(torch.int32))
    return torch.equal(x, y)


def _assert_same(got, want, what):
    for name, x, y in zip(("actions", "log_prob", "entropy", "n_allowed"), got, want):
        if not _bits_equal(x, y):
            bad = (x != y).nonzero().flatten()[:8].tolist()
            raise AssertionError(f"{what}: {name} differs in rows {bad}: {x[bad].tolist()} != {y[bad].tolist()}")


def _linear(latent, weight, bias):
    """The logits buffer the fused head stands for: F.linear in float32 on the exactly widened inputs, on their device."""
    import torch.nn.functional as F
    return F.linear(latent.float(), weight.float(), None if bias is None else bias.float())


def _exact_on(dev, dt, n, A, H, seed):
    import torch
    latent, weight, bias = lr.exact_inputs(n, A, H, np.random.default_rng(seed))
    return tuple(torch.as_tensor(x, device=dev).to(dt) for x in (latent, weight, bias))


# ------------------------------------------------------------------------------------------------ 1. exact inputs, packed, bitwise
@pytest.mark.parametrize("H", [1, 3, 64, 65, 200])
def test_exact_inputs_packed_bitwise(H):
    import torch
    eng = _chain4_engine()
    dev = eng.device
    A = eng.discrete_action_count()
    W, row_words = eng.packed_mask_words()
    n = 64
    mask = _synthetic_masks(A, n)
    K = mask.sum(1)
    assert K[3] == 0 and K[0] == 1 and K[2] == A and A > 512 and (K > 512).sum() >= 2, "rows without, with one, with all and with more allowed actions than the stash"
    bits = torch.as_tensor(_pack(mask, W + 6, garbage_tail=True), device=dev)      # a set tail word with garbage beyond A, junk words beyond W
    g = torch.Generator(device=dev).manual_seed(4)
    u = torch.rand(n, generator=g, device=dev)
    u[0], u[1], u[2] = 0.0, 0.99999994, 0.99999994
    rng = np.random.default_rng(5)
    for dt in (torch.float32, torch.bfloat16):
        latent, weight, bias = _exact_on(dev, dt, n, A, H, 40 + H)
        logits = _linear(latent, weight, bias)
        np.testing.assert_array_equal(logits.double().cpu().numpy(), lr.logits64(latent, weight, bias), err_msg="F.linear is not exact on exact_inputs")
        for b in (bias, None):
            lg = logits if b is not None else _linear(latent, weight, None)
            what = f"H={H} {dt} bias={'yes' if b is not None else 'none'}"
            for mode in ("argmax", "sample"):
                got = eng.masked_linear_categorical(latent, weight, b, bits=bits, mode=mode, uniforms=u if mode == "sample" else None)
                want = eng.masked_categorical(lg, bits=bits, mode=mode, uniforms=u if mode == "sample" else None)
                _assert_same(got, want, f"{what} {mode}")
            acts = want.actions.clone()                                             # the sampled actions, some replaced by arbitrary ones
            swap = torch.as_tensor(rng.random(n) < 0.5, device=dev)
            acts[swap] = torch.as_tensor(rng.integers(0, A, n), device=dev)[swap]
            got = eng.masked_linear_categorical(latent, weight, b, bits=bits, mode="evaluate", actions=acts)
            want = eng.masked_categorical(lg, bits=bits, mode="evaluate", actions=acts)
            _assert_same(got, want, f"{what} evaluate")
            on = torch.as_tensor(mask[np.arange(n), acts.cpu().numpy()])
            assert bool(on.any()) and bool((~on).any())
        np.testing.assert_array_equal(got.n_allowed.cpu().numpy(), K)
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. exact inputs through the live form
@functools.lru_cache(maxsize=None)
def _live_run(trace):
    """Random play (on Chain-10 the last 32 envs play the reference's winning script: K in the thousands) with the live form checked at
    a few steps against sample_masked(F.linear(...)), the packed form on action_masks' packed words, and two shards of the batch."""
    import torch
    from marlon_amd import engine
    from marlon_amd._abi import RNG_PHILOX
    _, sj = parity.load_trace(trace)
    topo = parity.topology_for(trace)
    E = 128 if topo.n_nodes <= 12 else 32
    mk = lambda n, base: parity.spec_from_json(sj, n_envs=n, auto_reset=True, rng_kind=RNG_PHILOX, seed=17, max_episode_steps=60, env_id_base=base)
    eng = engine.BatchEngine(topo, mk(E, 0))
    upper = engine.BatchEngine(topo, mk(E // 2, E // 2))         # the upper half of the batch as a shard of its own
    dev = eng.device
    A = eng.discrete_action_count()
    obs, obs_u = eng.alloc_obs(SMALL), upper.alloc_obs(SMALL)
    H = 64
    g = torch.Generator(device=dev).manual_seed(2)
    script = torch.as_tensor(parity.load_trace("chain10_script")[0]["actions"], device=dev) if trace == "chain10_mix_s3" else None
    T = 29 if script is not None else 15
    layers = {dt: _exact_on(dev, dt, E, A, H, 7) for dt in (torch.float32, torch.bfloat16)}
    seen = {"Kmax": 0, "K0": 0, "checked": 0, "A": A}
    for t in range(T):
        a = eng.sample_actions(t % 5 != 4, seed=9, step=t)       # every fifth step uniform over the bounds: out-of-bound actions blank the observation
        au = upper.sample_actions(t % 5 != 4, seed=9, step=t)
        if script is not None:
            a[E - 32:] = script[t]
            au[E // 2 - 32:] = script[t]
        if not (t % 7 == 6 or t == T - 1):
            eng.step(a)
            upper.step(au)
            continue
        eng.step_observe(a, obs)
        upper.step_observe(au, obs_u)
        bits = eng.pack_action_mask()
        u = torch.rand(E, generator=g, device=dev)
        u[0], u[1] = 0.0, 0.99999994
        for dt, (latent, weight, bias) in layers.items():
            what = f"{trace} step {t} {dt}"
            logits = _linear(latent, weight, bias)
            for kw in (dict(mode="sample", uniforms=u), dict(mode="argmax"), dict(mode="sample", seed=123456789012, step=t)):
                live = eng.masked_linear_categorical(latent, weight, bias, **kw)
                _assert_same(live, eng.masked_categorical(logits, **kw), f"{what} live {kw['mode']}")
                _assert_same(eng.masked_linear_categorical(latent, weight, bias, bits=bits, **kw), live, f"{what} packed == live {kw['mode']}")
            # Philox keyed by the global env id: the upper shard draws what the whole batch draws for those envs; the step keys the draw
            r_up = upper.masked_linear_categorical(latent[E // 2:], weight, bias, mode="sample", seed=123456789012, step=t)
            _assert_same(r_up, tuple(x[E // 2:] for x in live), f"{what} shard")
            other = eng.masked_linear_categorical(latent, weight, bias, mode="sample", seed=123456789012, step=t + 1)
            assert not torch.equal(other.actions, live.actions), f"{what}: the step does not key the draw"
            ev = eng.masked_linear_categorical(latent, weight, bias, bits=bits, mode="evaluate", actions=live.actions)
            _assert_same(ev, live, f"{what} evaluate of the sampled actions")
        Kt = live.n_allowed
        seen["Kmax"] = max(seen["Kmax"], int(Kt.max()))
        seen["K0"] += int((Kt == 0).sum())
        seen["checked"] += 1
    eng.close(); upper.close()
    return seen


@pytest.mark.parametrize("trace", ["chain10_mix_s3", "toyctf_defender_s11", "random24_defender_s51"])
def test_exact_inputs_live_bitwise(trace):
    """random24 (A = 186 120: 5 817 mask words) is here for the words beyond the kernel's word cache, whose logits are never stashed."""
    seen = _live_run(trace)
    print(trace, seen)
    assert seen["checked"] >= 2
    if trace == "chain10_mix_s3":
        assert seen["Kmax"] > 2048, "the scripted envs should have shown rows beyond the stash"
    if trace == "random24_defender_s51":
        assert seen["A"] > 512 * 32


# ------------------------------------------------------------------------------------------------ 3. general inputs: the dot product
def _general_on(dev, dt, n, A, H, seed, layout):
    """randn latent, randn / sqrt(H) weights, randn bias in the given layout: "dense", or "offset" — rows longer than H in buffers whose
    views start one element in (unaligned rows, strides that are no multiple of 16 bytes)."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    latent = torch.randn((n, H), generator=g, device=dev).to(dt)
    weight = (torch.randn((A, H), generator=g, device=dev) / H ** 0.5).to(dt)
    bias = torch.randn(A, generator=g, device=dev).to(dt)
    if layout == "offset":
        lw = torch.full((n, H + 6), 9.0, device=dev, dtype=dt)
        ww = torch.full((A, H + 3), 9.0, device=dev, dtype=dt)
        bw = torch.full((A + 2,), 9.0, device=dev, dtype=dt)
        lw[:, 1:H + 1], ww[:, 1:H + 1], bw[1:A + 1] = latent, weight, bias
        return lw[:, 1:H + 1], ww[:, 1:H + 1], bw[1:A + 1], (lw, ww, bw)
    return latent, weight, bias, None


def _bounded(got, want, comp_err, extra, what):
    """|got - want| <= 4 * comp_err + one fp32 ulp of the value + extra (per row); prints and returns the largest error."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    bound = 4.0 * comp_err + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + extra
    worst = int(np.argmax(err - bound))
    print(f"{what}: kernel max abs error {err.max():.3e}, fp32 composite {comp_err:.3e}, smallest bound {bound.min():.3e}, "
          f"closest row {worst}: error {err[worst]:.3e} of bound {bound[worst]:.3e}")
    assert np.all(err <= bound), f"{what}: row {worst}: error {err[worst]:.3e} > bound {bound[worst]:.3e} (value {want[worst]!r})"
    return float(err.max())


@pytest.mark.parametrize("layout", ["dense", "offset"])
@pytest.mark.parametrize("H", [64, 37])
def test_general_inputs_against_fp64(H, layout):
    import torch
    eng = _chain4_engine()
    dev = eng.device
    A = eng.discrete_action_count()
    W, row_words = eng.packed_mask_words()
    n = 64
    mask = _synthetic_masks(A, n)
    rows = np.arange(n)
    bits = torch.as_tensor(_pack(mask, row_words), device=dev)
    g = torch.Generator(device=dev).manual_seed(6)
    u = torch.rand(n, generator=g, device=dev)
    u[0], u[1], u[2] = 0.0, 0.99999994, 0.99999994
    u24 = cr.u24_of_uniforms(u.cpu().numpy())
    uu = u24 * 2.0 ** -24
    for dt in (torch.float32, torch.bfloat16):
        latent, weight, bias, wide = _general_on(dev, dt, n, A, H, 60 + H, layout)
        if wide is not None:
            assert weight.data_ptr() % 16 != 0 and latent.data_ptr() % 16 != 0
        keep = [x.clone() for x in (wide or (latent, weight, bias))]
        x64 = lr.logits64(latent, weight, bias)
        delta = lr.dot_bound(latent, weight, bias, mask)
        ref = cr.CategoricalRef(mask, x64)
        nz = ref.K > 0
        norm, ent_c = _composite(mask, _linear(latent.cpu(), weight.cpu(), bias.cpu()))         # torch fp32 on the CPU: F.linear -> where -> Categorical
        ent_err = float(np.abs(ent_c - ref.entropy)[nz].max())
        ent_extra = 4.0 * delta * np.maximum(1.0, np.log(np.maximum(ref.K, 1)))
        comp_lp = lambda a: float(np.abs(norm[torch.arange(n), torch.as_tensor(a)].double().numpy() - ref.log_prob(a))[nz].max())
        what = f"H={H} {layout} {dt}"
        print(f"{what}: delta {delta[nz].min():.3e} .. {delta.max():.3e}")
        run = lambda mode, **kw: eng.masked_linear_categorical(latent, weight, bias, bits=bits, mode=mode, **kw)
        # ARGMAX: its fp64 logit within 2 delta of the fp64 maximum
        r = run("argmax")
        np.testing.assert_array_equal(r.n_allowed.cpu().numpy(), ref.K, err_msg=f"{what} n_allowed")
        a = r.actions.cpu().numpy()
        assert np.all(a[~nz] == 0) and mask[rows[nz], a[nz]].all(), f"{what}: argmax is not allowed"
        gap = ref.m - x64[rows, a]
        print(f"{what} argmax: largest fp64 gap to the maximum {gap[nz].max():.3e}, rows not at the fp64 arg max {int((a != ref.argmax)[nz].sum())}")
        assert np.all(gap[nz] <= 2.0 * delta[nz]), f"{what}: argmax further than 2 delta from the maximum"
        _bounded(r.log_prob.cpu().numpy(), ref.log_prob(a), comp_lp(a), 2.0 * delta, f"{what} argmax log_prob")
        _bounded(r.entropy.cpu().numpy(), ref.entropy, ent_err, ent_extra, f"{what} entropy")
        # SAMPLE
        r = run("sample", uniforms=u)
        a = r.actions.cpu().numpy()
        np.testing.assert_array_equal(r.n_allowed.cpu().numpy(), ref.K)
        np.testing.assert_array_equal(a[~nz], (u24[~nz] * A) >> 24, err_msg=f"{what} blank rows")
        assert np.all((a >= 0) & (a < A)) and mask[rows[nz], a[nz]].all(), f"{what}: a sampled action is not allowed"
        lo, hi = ref.cdf_interval(a)
        widen = (ref.K + 16) * 2.0 ** -23 + np.expm1(2.0 * delta)
        ok = (lo - widen <= uu) & (uu < hi + widen)
        assert ok[nz].all(), f"{what}: rows {np.nonzero(~ok & nz)[0][:8]} sampled outside their CDF interval"
        _bounded(r.log_prob.cpu().numpy(), ref.log_prob(a), comp_lp(a), 2.0 * delta, f"{what} sample log_prob")
        _bounded(r.entropy.cpu().numpy(), ref.entropy, ent_err, ent_extra, f"{what} sample entropy")
        # EVALUATE of arbitrary actions inside the range: allowed ones to the bound, disallowed ones to rtol 2^-22 of -1e8 - m - log Z
        acts = np.random.default_rng(12).integers(0, A, n)
        acts[0], acts[2] = 0, A - 1
        e = run("evaluate", actions=torch.as_tensor(acts, device=dev))
        on = mask[rows, acts]
        lp, want = e.log_prob.cpu().numpy().astype(np.float64), ref.log_prob(acts)
        assert on.sum() > 5 and (~on & nz).sum() > 5
        np.testing.assert_allclose(lp[~on], want[~on], rtol=2.0 ** -22, err_msg=f"{what}: disallowed actions")
        _bounded(lp[on], want[on], comp_lp(np.where(on, acts, ref.argmax)), 2.0 * delta[on], f"{what} evaluate allowed")
        for x, k in zip(wide or (latent, weight, bias), keep):
            assert torch.equal(x.view(torch.int16 if dt == torch.bfloat16 else torch.int32), k.view(torch.int16 if dt == torch.bfloat16 else torch.int32)), \
                f"{what}: an input was modified"
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. invariance and reproducibility
def test_invariance_and_reproducibility():
    import torch
    eng = _chain4_engine()
    dev = eng.device
    A = eng.discrete_action_count()
    W, row_words = eng.packed_mask_words()
    n = 64
    mask = _synthetic_masks(A, n)
    bits = torch.as_tensor(_pack(mask, row_words), device=dev)
    g = torch.Generator(device=dev).manual_seed(9)
    u = torch.rand(n, generator=g, device=dev)
    perm = torch.randperm(n, generator=g, device=dev)
    for dt in (torch.float32, torch.bfloat16):
        for H in (64, 37):
            what = f"H={H} {dt}"
            latent, weight, bias, _ = _general_on(dev, dt, n, A, H, 80 + H, "dense")
            keep = [x.clone() for x in (latent, weight, bias)]
            run = lambda **kw: eng.masked_linear_categorical(latent, weight, bias, bits=bits, **kw)
            # two identical calls; sample, then evaluate what was sampled
            s1, s2 = run(mode="sample", seed=77, step=3), run(mode="sample", seed=77, step=3)
            _assert_same(s1, s2, f"{what}: two identical calls")
            _assert_same(run(mode="evaluate", actions=s1.actions), s1, f"{what}: sample then evaluate")
            # the same values in other layouts: one element in (unaligned), longer strides (a weight stride of H + 3 elements puts
            # aligned and unaligned weight rows into one call), and padded to aligned strides
            su = run(mode="sample", uniforms=u)
            au = run(mode="argmax")
            for pad_l, pad_w, off in ((6, 3, 1), (8, 8, 0), (2, 1, 0), (5, 7, 2)):
                lw = torch.full((n, H + pad_l), 9.0, device=dev, dtype=dt)
                ww = torch.full((A, H + pad_w), 9.0, device=dev, dtype=dt)
                bw = torch.full((A + 3,), 9.0, device=dev, dtype=dt)
                lv, wv, bv = lw[:, off:off + H], ww[:, off:off + H], bw[off:off + A]
                lv.copy_(latent); wv.copy_(weight); bv.copy_(bias)
                lay = f"{what} layout pad {pad_l}/{pad_w} offset {off}"
                _assert_same(eng.masked_linear_categorical(lv, wv, bv, bits=bits, mode="sample", uniforms=u), su, lay)
                _assert_same(eng.masked_linear_categorical(lv, wv, bv, bits=bits, mode="argmax"), au, lay)
                assert bool((lw[:, off + H:] == 9.0).all()) and bool((ww[:, off + H:] == 9.0).all()), "sentinels touched"
            # a row placed at another row index, with its uniform number
            sp = eng.masked_linear_categorical(latent[perm], weight, bias, bits=bits[perm], mode="sample", uniforms=u[perm])
            _assert_same(sp, tuple(x[perm] for x in su), f"{what}: rows permuted")
            for x, k in zip((latent, weight, bias), keep):
                assert torch.equal(x.view(torch.int16 if dt == torch.bfloat16 else torch.int32), k.view(torch.int16 if dt == torch.bfloat16 else torch.int32)), \
                    f"{what}: an input was modified"
    # preallocated outputs are the ones returned
    out = (torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    r = eng.masked_linear_categorical(latent, weight, bias, bits=bits, mode="sample", uniforms=u, out=out)
    assert all(x is y for x, y in zip(r, out))
    _assert_same(r, su, "out=")
    eng.close()


def test_more_rows_than_one_grid():
    """One grid covers 4 * 65 536 rows: rows beyond are reached by the stride loop.  The whole call equals the same rows in two halves."""
    import torch
    eng = _chain4_engine()
    dev = eng.device
    A = eng.discrete_action_count()
    W, row_words = eng.packed_mask_words()
    mask = _synthetic_masks(A)
    mask[2, 600:] = False                                # keep the tiled work small: no row with all 1 830 actions
    reps = 4 * 65536 // 64 + 3
    n = reps * 64
    H = 8
    bits = torch.as_tensor(_pack(mask, row_words), device=dev).repeat(reps, 1)
    g = torch.Generator(device=dev).manual_seed(4)
    latent = torch.randn((n, H), generator=g, device=dev)
    weight = torch.randn((A, H), generator=g, device=dev) / H ** 0.5
    bias = torch.randn(A, generator=g, device=dev)
    u = torch.rand(n, generator=g, device=dev)
    whole = eng.masked_linear_categorical(latent, weight, bias, bits=bits, mode="sample", uniforms=u)
    h = n // 2
    halves = [eng.masked_linear_categorical(latent[s], weight, bias, bits=bits[s], mode="sample", uniforms=u[s]) for s in (slice(0, h), slice(h, n))]
    _assert_same(whole, tuple(torch.cat([a, b]) for a, b in zip(*halves)), "whole == two halves")
    assert torch.equal(whole.n_allowed.view(reps, 64), whole.n_allowed[:64].expand(reps, 64))
    np.testing.assert_array_equal(whole.n_allowed[-64:].cpu().numpy(), mask.sum(1))
    ev = eng.masked_linear_categorical(latent, weight, bias, bits=bits, mode="evaluate", actions=whole.actions)
    _assert_same(ev, whole, "evaluate of the sampled actions")
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_c_abi_refusals():
    """Every MCBS_EINVAL (-1) / MCBS_ESTATE (-5) case of the two entry points, through ctypes."""
    import torch
    eng = _chain4_engine()
    dev = eng.device
    lib = eng.lib
    A = eng.discrete_action_count()
    W, row_words = eng.packed_mask_words()
    n, H = 64, 16
    latent = torch.zeros((n, H), device=dev)
    weight = torch.zeros((A, H), device=dev)
    bias = torch.zeros(A, device=dev)
    bits = torch.full((n, row_words), 0x55555555, dtype=torch.int32, device=dev)
    acts = torch.full((n,), -7, dtype=torch.int64, device=dev)
    lp = torch.full((n,), 3.0, device=dev)

    def packed(bits_ptr=bits.data_ptr(), words=row_words, rows=n, lat=latent.data_ptr(), ls=H, wt=weight.data_ptr(), ws=H, b=bias.data_ptr(), h=H,
               dtype=0, mode=1, a=acts.data_ptr(), l=lp.data_ptr()):
        return lib.mcbs_masked_linear_categorical_packed(eng._h, bits_ptr, words, rows, lat, ls, wt, ws, b, h, dtype, mode, a, l, None, None, None, 0, 0,
                                                         None, None)

    def live(lat=latent.data_ptr(), ls=H, wt=weight.data_ptr(), ws=H, h=H, dtype=0, mode=1):
        return lib.mcbs_masked_linear_categorical(eng._h, lat, ls, wt, ws, bias.data_ptr(), h, dtype, mode, acts.data_ptr(), lp.data_ptr(), None, None, None,
                                                  0, 0, None, None)

    def err():
        return lib.mcbs_last_error().decode()

    for kw, word in ((dict(h=0), "H 0"), (dict(h=513, ls=513, ws=513), "H 513"), (dict(ls=H - 1), "latent_row_stride"), (dict(ws=H - 1), "weight_row_stride"),
                     (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"), (dict(lat=None), "latent and weight"), (dict(wt=None), "latent and weight"),
                     (dict(words=W - 1), "bits_row_words"), (dict(bits_ptr=None), "bits"), (dict(mode=3), "mode"), (dict(a=None), "actions"),
                     (dict(l=None), "log_prob")):
        assert packed(**kw) == -1 and word in err(), (kw, err())
    torch.cuda.synchronize()
    assert bool((acts == -7).all()) and bool((lp == 3.0).all()), "a refused call wrote its outputs"
    assert packed(rows=0) == 0 and packed(rows=0, lat=None, h=0) == 0                  # n_rows == 0 is a no-op
    assert lib.mcbs_masked_linear_categorical_packed(None, None, 0, 0, None, 0, None, 0, None, 0, 0, 0, None, None, None, None, None, 0, 0, None, None) == -1
    torch.cuda.synchronize()
    assert bool((acts == -7).all())
    assert packed() == 0                                                               # and the accepted call: zero layer, argmax = lowest allowed action
    torch.cuda.synchronize()
    assert bool((acts == 0).all())
    # the live form: MCBS_ESTATE as for mcbs_masked_categorical, MCBS_EINVAL for its arguments once the digest is usable
    assert live() == -5 and "no observation" in err()
    small = eng.alloc_obs(["scalars", "nodes_privilegelevel"])
    eng.observe(small)
    assert live() == 0
    for kw, word in ((dict(h=0), "H 0"), (dict(h=513, ls=513, ws=513), "H 513"), (dict(ls=H - 1), "latent_row_stride"), (dict(ws=H - 1), "weight_row_stride"),
                     (dict(dtype=2), "dtype"), (dict(lat=None), "latent and weight"), (dict(wt=None), "latent and weight"), (dict(mode=-1), "mode")):
        assert live(**kw) == -1 and word in err(), (kw, err())
    m = torch.zeros(n, dtype=torch.uint8, device=dev)
    m[::3] = 1
    eng.reset(m)
    assert live() == -5 and "reset by mask" in err()
    assert packed() == 0                                                               # the packed form needs no digest
    eng.close()
    ere = _chain4_engine(defender=("random_events",))
    ere.observe(ere.alloc_obs(["scalars", "nodes_privilegelevel"]))
    assert lib.mcbs_masked_linear_categorical(ere._h, latent.data_ptr(), H, weight.data_ptr(), H, None, H, 0, 1, acts.data_ptr(), lp.data_ptr(), None, None,
                                              None, 0, 0, None, None) == -5 and "ExternalRandomEvents" in err()
    r = ere.masked_linear_categorical(latent, weight, bits=bits, mode="argmax")         # the packed form serves every defender kind
    assert bool((r.actions == 0).all())
    ere.close()


def test_python_refusals_and_bad_actions():
    import torch
    from marlon_amd import engine
    eng = _chain4_engine()
    dev = eng.device
    A = eng.discrete_action_count()
    W, row_words = eng.packed_mask_words()
    n, H = 64, 16
    g = torch.Generator(device=dev).manual_seed(1)
    latent = torch.randn((n, H), generator=g, device=dev)
    weight = torch.randn((A, H), generator=g, device=dev)
    bias = torch.randn(A, generator=g, device=dev)
    bits = torch.full((n, row_words), 0x55555555, dtype=torch.int32, device=dev)
    acts = torch.zeros(n, dtype=torch.int64, device=dev)
    with pytest.raises(engine.McbsError, match="no observation"):
        eng.masked_linear_categorical(latent, weight, bias)
    eng.observe(eng.alloc_obs(["scalars", "nodes_privilegelevel"]))
    eng.masked_linear_categorical(latent, weight, bias)
    for bad_call in (
        lambda: eng.masked_linear_categorical(latent.cpu(), weight, bias),
        lambda: eng.masked_linear_categorical(latent, weight.cpu(), bias),
        lambda: eng.masked_linear_categorical(latent, weight, bias.cpu()),
        lambda: eng.masked_linear_categorical(latent.bfloat16(), weight, bias),
        lambda: eng.masked_linear_categorical(latent, weight.bfloat16(), bias),
        lambda: eng.masked_linear_categorical(latent, weight, bias.bfloat16()),
        lambda: eng.masked_linear_categorical(latent.double(), weight.double(), bias.double()),
        lambda: eng.masked_linear_categorical(latent.half(), weight.half(), bias.half()),
        lambda: eng.masked_linear_categorical(latent, weight[:A - 1], bias),
        lambda: eng.masked_linear_categorical(latent, torch.cat([weight, weight[:1]]), bias),
        lambda: eng.masked_linear_categorical(latent, weight[:, :H - 1], bias),
        lambda: eng.masked_linear_categorical(latent, weight, bias[:A - 1]),
        lambda: eng.masked_linear_categorical(latent, weight, torch.cat([bias, bias])[::2]),
        lambda: eng.masked_linear_categorical(latent.t().contiguous().t(), weight, bias),
        lambda: eng.masked_linear_categorical(latent, weight.t().contiguous().t(), bias),
        lambda: eng.masked_linear_categorical(latent[:32], weight, bias),
        lambda: eng.masked_linear_categorical(latent[:, :0], weight[:, :0], bias),
        lambda: eng.masked_linear_categorical(torch.zeros((n, 513), device=dev), torch.zeros((A, 513), device=dev), bias),
        lambda: eng.masked_linear_categorical(None, weight, bias),
        lambda: eng.masked_linear_categorical(latent, None, bias),
        lambda: eng.masked_linear_categorical(latent, weight, bias, mode="mean"),
        lambda: eng.masked_linear_categorical(latent, weight, bias, mode="evaluate"),
        lambda: eng.masked_linear_categorical(latent, weight, bias, mode="evaluate", actions=acts.int()),
        lambda: eng.masked_linear_categorical(latent, weight, bias, mode="sample", actions=acts),
        lambda: eng.masked_linear_categorical(latent, weight, bias, uniforms=torch.zeros(n - 1, device=dev)),
        lambda: eng.masked_linear_categorical(latent, weight, bias, bits=bits.long()),
        lambda: eng.masked_linear_categorical(latent, weight, bias, bits=bits[:, :W - 1]),
        lambda: eng.masked_linear_categorical(latent, weight, bias, bits=bits[:10]),
        lambda: eng.masked_linear_categorical(latent, weight, bias, out=(acts.int(), None, None, None)),
        lambda: eng.masked_linear_categorical(latent, weight, bias, mode="evaluate", actions=acts, bad_actions=torch.zeros(1, device=dev)),
    ):
        with pytest.raises(ValueError):
            bad_call()
    # EVALUATE with actions -1 and A: NaN, and bad_actions rises by exactly 2 (it is not zeroed)
    a = torch.as_tensor(np.random.default_rng(3).integers(0, A, n), device=dev)
    a[9], a[10] = -1, A
    bad = torch.zeros(1, dtype=torch.int32, device=dev) + 5
    r = eng.masked_linear_categorical(latent, weight, bias, bits=bits, mode="evaluate", actions=a, bad_actions=bad)
    assert int(bad.item()) == 7
    lp = r.log_prob.cpu().numpy()
    assert np.isnan(lp[9]) and np.isnan(lp[10]) and np.isfinite(np.delete(lp, [9, 10])).all()
    assert int(a[9]) == -1 and int(a[10]) == A
    r0 = eng.masked_linear_categorical(latent[:0], weight, bias, bits=bits[:0], mode="sample")
    assert all(x.shape == (0,) for x in r0)
    eng.close()


def test_wrapper_surface():
    """AttackerVecEnv.sample_masked_from_latent / evaluate_masked_from_latent and MarlonVecEnv's pass-throughs: a rollout that never
    builds logits steps without an invalid action, and the stored log_prob comes back bit for bit from a shuffled minibatch."""
    import torch
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.samples import chainpattern
    from marlon_amd.vecenv import MarlonVecEnv
    from marlon_amd.wrappers import AttackerVecEnv
    E, T, H = 128, 6, 64
    env = AttackerVecEnv(chainpattern.new_environment(10), E, maximum_node_count=12, maximum_total_credentials=12,
                         attacker_goal=ce.AttackerGoal(own_atleast_percent=1.0), max_timesteps=50, discrete=True, materialize_masks=False)
    dev = env.engine.device
    A = env.discrete_n
    W, row_words = env.engine.packed_mask_words()
    g = torch.Generator(device=dev).manual_seed(8)
    weight = (torch.randn((A, H), generator=g, device=dev) / 8.0).bfloat16()
    bias = torch.randn(A, generator=g, device=dev).bfloat16()
    buf = torch.zeros((T, E, row_words), dtype=torch.int32, device=dev)
    lat = torch.zeros((T, E, H), dtype=torch.bfloat16, device=dev)
    acts = torch.zeros((T, E), dtype=torch.int64, device=dev)
    lps = torch.zeros((T, E), device=dev)
    ents = torch.zeros((T, E), device=dev)
    for t in range(T):
        env.action_masks_packed(out=buf[t])
        lat[t] = torch.randn((E, H), generator=g, device=dev).bfloat16()
        r = env.sample_masked_from_latent(lat[t], weight, bias, seed=3, step=t)
        d = env.sample_masked_from_latent(lat[t], weight, bias, seed=3, step=t, deterministic=True)
        assert torch.equal(d.n_allowed, r.n_allowed) and bool((d.log_prob >= r.log_prob).all())
        acts[t], lps[t], ents[t] = r.actions, r.log_prob, r.entropy
        _, _, _, _, info = env.step(r.actions)
        assert not bool(info["invalid_action"].any()), f"step {t}: a sampled action was not valid"
    perm = torch.randperm(T * E, generator=torch.Generator().manual_seed(1))[:512].to(dev)
    r = env.evaluate_masked_from_latent(buf.view(T * E, row_words)[perm], lat.view(T * E, H)[perm], weight, bias, acts.view(-1)[perm])
    assert torch.equal(r.log_prob.view(torch.int32), lps.view(-1)[perm].view(torch.int32))
    assert torch.equal(r.entropy.view(torch.int32), ents.view(-1)[perm].view(torch.int32))
    assert bool(torch.isfinite(r.log_prob).all()) and bool((r.n_allowed > 0).all())
    # against the materialised logits: the same distribution to rounding.  Both the kernel's and the GEMM's logits are within delta of the
    # exact ones, log p moves by at most twice what the logits move by: 4 delta, plus an ulp of either value
    logits = _linear(lat[T - 1], weight, bias)
    m = env.evaluate_masked(buf[T - 1], logits, acts[T - 1])
    delta = lr.dot_bound(lat[T - 1], weight, bias, env.unpack_action_mask(buf[T - 1]).cpu().numpy())
    diff = (m.log_prob - lps[T - 1]).abs().double().cpu().numpy()
    print(f"log_prob against evaluate_masked on F.linear's logits: max difference {diff.max():.3e}, smallest bound {4 * delta.min():.3e}")
    assert np.all(diff <= 4.0 * delta + 2.0 * np.spacing(np.abs(lps[T - 1].cpu().numpy())))
    env.close()
    for name in ("sample_masked_from_latent", "evaluate_masked_from_latent"):
        assert callable(getattr(MarlonVecEnv, name))
