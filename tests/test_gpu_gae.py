"""mcbs_gae (generalized advantage estimation over a whole [T, E] rollout in one launch, include/mcbs.h) against tests/gae_ref.py's
NumPy float32 restatement of Stable-Baselines3's loop: advantages and returns BIT FOR BIT (compared as int32), on every T from 1 to 40
(the tail, exactly one block and a block boundary of every candidate block length 4 / 8 / 16) and E in {1, 63, 64, 65, 193}, plus
[128, 4099]; start densities 0 / 0.1 / 1, four (gamma, lambda) pairs, with and without the truncation bootstrap, with and without the
returns output, -0.0 rewards, flag bytes other than 1, strided [T, :E] views of sentinel-filled buffers, and the refusals.  Finite inputs
only: NaN payloads are not promised."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests.gae_ref import gae_f32

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
COEFFS = ((0.99, 0.95), (1.0, 1.0), (0.9, 0.0), (0.0, 0.5))
DENSITIES = (0.0, 0.1, 1.0)
COMBOS = list(itertools.product(DENSITIES, COEFFS, (False, True)))      # 24: (density, (gamma, lambda), bootstrap)
# extra row stride (elements beyond E) of rewards, values, episode_starts, bootstrap, advantages, returns: all different
PADS = dict(rewards=3, values=5, episode_starts=9, bootstrap=1, advantages=7, returns=2)

_ENGINE = []


def _engine():
    """A Chain-4 batch of 64 envs: it only owns the device for these calls."""
    if not _ENGINE:
        from marlon_amd import engine
        from marlon_amd._abi import EnvSpec
        from marlon_amd.flatten import flatten
        from marlon_amd.samples import chainpattern
        topo = flatten(chainpattern.new_environment(4))
        _ENGINE.append(engine.BatchEngine(topo, EnvSpec(n_envs=64, maximum_node_count=6, maximum_total_credentials=6,
                                                        attacker_goal=dict(own_atleast_percent=1.0))))
    return _ENGINE[0]


def _case(T, E, density, seed, neg_zero=False):
    """Finite inputs: rewards 5 N(0,1), values 3 N(0,1), starts of the given density, mixed last_dones, a sparse bootstrap."""
    rng = np.random.default_rng(seed)
    r = (5.0 * rng.standard_normal((T, E))).astype(np.float32)
    v = (3.0 * rng.standard_normal((T, E))).astype(np.float32)
    if neg_zero:                                        # -0.0 rewards (next to +0.0 values, where the sign can reach the output)
        z = rng.random((T, E)) < 0.2
        r[z] = -0.0
        v[z & (rng.random((T, E)) < 0.5)] = 0.0
    s = (rng.random((T, E)) < density).astype(np.uint8)
    lv = (3.0 * rng.standard_normal(E)).astype(np.float32)
    ld = (rng.random(E) < 0.5).astype(np.uint8)
    b = np.where(rng.random((T, E)) < 0.1, 3.0 * rng.standard_normal((T, E)), 0.0).astype(np.float32)
    return dict(rewards=r, values=v, episode_starts=s, last_values=lv, last_dones=ld, bootstrap=b)


def _framed(T, E, pad, offset, dtype, dev, fill=SENTINEL):
    """A [T, E] view at element `offset` with row stride E + pad inside a sentinel-filled buffer -> (buffer, view)."""
    import torch
    stride = E + pad
    buf = torch.full((offset + T * stride + 9,), fill, dtype=dtype, device=dev)
    return buf, buf[offset:offset + T * stride].view(T, stride)[:, :E]


def _frame_untouched(buf, T, E, pad, offset, fill=SENTINEL):
    stride = E + pad
    rows = buf[offset:offset + T * stride].view(T, stride)
    return bool((buf[:offset] == fill).all()) and bool((rows[:, E:] == fill).all()) and bool((buf[offset + T * stride:] == fill).all())


def _run(case, gamma, lam, bootstrap, strided=True, offset=0, want_returns=True, flag_bytes=None):
    """One call on `case`: every [T, E] array a view of its own sentinel-filled buffer (strided) or dense; checks that no input changed
    and that nothing outside the frames was written; -> (advantages, returns or None) as int32 NumPy arrays."""
    import torch
    eng = _engine()
    dev = eng.device
    T, E = case["rewards"].shape
    bufs, views = {}, {}
    for k in ("rewards", "values", "episode_starts", "bootstrap", "advantages", "returns"):
        dtype = torch.uint8 if k == "episode_starts" else torch.float32
        pad = PADS[k] if strided else 0
        bufs[k], views[k] = _framed(T, E, pad, offset if strided else 0, dtype, dev)
        if k in case:
            src = case[k]
            if k == "episode_starts" and flag_bytes is not None:
                src = np.where(src != 0, flag_bytes[0], 0).astype(np.uint8)
            views[k].copy_(torch.from_numpy(src))
    ld = case["last_dones"]
    if flag_bytes is not None:
        ld = np.where(ld != 0, flag_bytes[1], 0).astype(np.uint8)
    lv_t, ld_t = torch.from_numpy(case["last_values"]).to(dev), torch.from_numpy(ld).to(dev)
    before = {k: bufs[k].clone() for k in ("rewards", "values", "episode_starts", "bootstrap")}
    lv0, ld0 = lv_t.clone(), ld_t.clone()
    boot = views["bootstrap"] if bootstrap else None
    if want_returns:
        adv, ret = eng.gae(views["rewards"], views["values"], views["episode_starts"], lv_t, ld_t, gamma, lam, bootstrap=boot,
                           advantages=views["advantages"], returns=views["returns"])
        assert adv is views["advantages"] and ret is views["returns"]
    else:                                               # the C level's nullable `returns`
        from marlon_amd._abi import GaeIO
        st = lambda k: views[k].stride(0) if T > 1 else E
        io = GaeIO(views["rewards"].data_ptr(), views["values"].data_ptr(), views["episode_starts"].data_ptr(),
                   boot.data_ptr() if bootstrap else None, lv_t.data_ptr(), ld_t.data_ptr(), views["advantages"].data_ptr(), None, T, E,
                   st("rewards"), st("values"), st("episode_starts"), st("bootstrap") if bootstrap else 0, st("advantages"), 0, gamma, lam)
        assert eng.lib.mcbs_gae(eng._h, C.byref(io), eng._stream()) == 0, eng.lib.mcbs_last_error()
    torch.cuda.synchronize()
    for k, b in before.items():
        assert torch.equal(bufs[k], b), f"input {k} was modified"
    assert torch.equal(lv_t, lv0) and torch.equal(ld_t, ld0)
    pad = lambda k: PADS[k] if strided else 0
    off = offset if strided else 0
    assert _frame_untouched(bufs["advantages"], T, E, pad("advantages"), off), "advantages: written outside [T, :E]"
    if want_returns:
        assert _frame_untouched(bufs["returns"], T, E, pad("returns"), off), "returns: written outside [T, :E]"
    else:
        assert bool((bufs["returns"] == SENTINEL).all()), "returns written although NULL"
    adv = views["advantages"].contiguous().cpu().numpy().view(np.int32)
    ret = views["returns"].contiguous().cpu().numpy().view(np.int32) if want_returns else None
    return adv, ret


def _reference(case, gamma, lam, bootstrap):
    adv, ret = gae_f32(case["rewards"], case["values"], case["episode_starts"], case["last_values"], case["last_dones"], gamma, lam,
                       bootstrap=case["bootstrap"] if bootstrap else None)
    return adv.view(np.int32), ret.view(np.int32)


@pytest.mark.parametrize("E", [1, 63, 64, 65, 193])
def test_bit_exact_on_every_small_shape(E):
    """T = 1 .. 40; the (density, coefficients, bootstrap) combination rotates with T and E so that all 24 occur for every E; runs
    without bootstrap carry -0.0 rewards; odd T start at an odd element offset; every third run leaves `returns` out."""
    shift = [1, 63, 64, 65, 193].index(E) * 5
    seen = set()
    for T in range(1, 41):
        combo = (T - 1 + shift) % len(COMBOS)
        density, (gamma, lam), bootstrap = COMBOS[combo]
        seen.add(combo)
        case = _case(T, E, density, seed=1000 * E + T, neg_zero=not bootstrap)
        want_returns = T % 3 != 0
        adv, ret = _run(case, gamma, lam, bootstrap, offset=T % 2, want_returns=want_returns)
        wadv, wret = _reference(case, gamma, lam, bootstrap)
        assert np.array_equal(adv, wadv), f"advantages differ at T={T} E={E} combo={COMBOS[combo]}: {int((adv != wadv).sum())} elements"
        if want_returns:
            assert np.array_equal(ret, wret), f"returns differ at T={T} E={E} combo={COMBOS[combo]}"
    assert len(seen) == len(COMBOS)


@pytest.mark.parametrize("bootstrap", [False, True])
def test_bit_exact_on_many_blocks_and_workgroups(bootstrap):
    """[128, 4099]: 65 workgroups, the last with three lanes; strided, dense and a second call give the same bits."""
    case = _case(128, 4099, 0.1, seed=77, neg_zero=not bootstrap)
    wadv, wret = _reference(case, 0.99, 0.95, bootstrap)
    adv, ret = _run(case, 0.99, 0.95, bootstrap, offset=1)
    assert np.array_equal(adv, wadv) and np.array_equal(ret, wret)
    adv2, ret2 = _run(case, 0.99, 0.95, bootstrap, offset=1)
    assert np.array_equal(adv, adv2) and np.array_equal(ret, ret2)
    dadv, dret = _run(case, 0.99, 0.95, bootstrap, strided=False)
    assert np.array_equal(adv, dadv) and np.array_equal(ret, dret)


def test_any_nonzero_byte_is_a_flag():
    """episode_starts bytes of 2 and last_dones bytes of 255 where the reference has 1."""
    for T, E, density in ((19, 65, 0.1), (16, 64, 1.0), (33, 193, 0.3)):
        case = _case(T, E, density, seed=5 + T)
        wadv, wret = _reference(case, 0.99, 0.95, True)
        for flags in ((2, 255), (255, 2), (128, 1)):
            adv, ret = _run(case, 0.99, 0.95, True, flag_bytes=flags)
            assert np.array_equal(adv, wadv) and np.array_equal(ret, wret), flags


def test_negative_zero_reward_keeps_its_sign_without_bootstrap():
    """A -0.0 reward reaches the output as -0.0 where the rest of the step is -0.0 too (next value negative, next step a start, value
    +0.0, running advantage negative); adding gamma * 0 to it first would give +0.0.  With a bootstrap array the reference does add."""
    T, E = 3, 65
    case = _case(T, E, 1.0, seed=3)
    case["rewards"][2], case["values"][2] = -5.0, -1.0
    case["last_dones"][:] = 1
    case["rewards"][1], case["values"][1] = -0.0, 0.0
    case["bootstrap"][:] = 0.0
    adv, ret = _run(case, 0.99, 0.95, False)
    wadv, wret = _reference(case, 0.99, 0.95, False)
    assert np.array_equal(adv, wadv) and np.array_equal(ret, wret)
    assert (adv[1].view(np.uint32) == 0x80000000).all() and (wadv[1].view(np.uint32) == 0x80000000).all()
    adv_b, ret_b = _run(case, 0.99, 0.95, True)
    wadv_b, wret_b = _reference(case, 0.99, 0.95, True)
    assert np.array_equal(adv_b, wadv_b) and np.array_equal(ret_b, wret_b)


def _dense_args(T=6, E=65):
    import torch
    eng = _engine()
    case = _case(T, E, 0.1, seed=9)
    t = {k: torch.from_numpy(v).to(eng.device) for k, v in case.items()}
    return eng, case, t


def test_c_level_refusals():
    """Every refusal include/mcbs.h lists returns MCBS_EINVAL (-1) with a message naming the argument; nothing is launched."""
    import torch
    from marlon_amd._abi import GaeIO
    eng, case, t = _dense_args()
    T, E = case["rewards"].shape
    adv, ret = torch.full((T, E), SENTINEL, device=eng.device), torch.full((T, E), SENTINEL, device=eng.device)
    wide = torch.zeros((T, 2 * E + 8), device=eng.device)

    def io(**kw):
        a = dict(rewards=t["rewards"].data_ptr(), values=t["values"].data_ptr(), episode_starts=t["episode_starts"].data_ptr(),
                 bootstrap=t["bootstrap"].data_ptr(), last_values=t["last_values"].data_ptr(), last_dones=t["last_dones"].data_ptr(),
                 advantages=adv.data_ptr(), returns=ret.data_ptr(), n_steps=T, n_envs=E, rewards_stride=E, values_stride=E,
                 episode_starts_stride=E, bootstrap_stride=E, advantages_stride=E, returns_stride=E, gamma=0.99, gae_lambda=0.95)
        a.update(kw)
        return GaeIO(**a)

    def refused(word, **kw):
        rc = eng.lib.mcbs_gae(eng._h, C.byref(io(**kw)), eng._stream())
        msg = eng.lib.mcbs_last_error()
        assert rc == -1 and word.encode() in msg, (kw, rc, msg)

    assert eng.lib.mcbs_gae(None, C.byref(io()), None) == -1 and b"null" in eng.lib.mcbs_last_error()
    assert eng.lib.mcbs_gae(eng._h, None, None) == -1 and b"null" in eng.lib.mcbs_last_error()
    for name in ("rewards", "values", "episode_starts", "last_values", "last_dones", "advantages"):
        refused(name, **{name: None})
    for name in ("rewards", "values", "episode_starts", "bootstrap", "advantages", "returns"):
        refused(name + "_stride", **{name + "_stride": E - 1})
    for bad in (float("nan"), float("inf"), -0.01, 1.01):
        refused("gamma", gamma=bad)
        refused("gae_lambda", gae_lambda=bad)
    for name in ("rewards", "values", "episode_starts", "bootstrap"):
        refused(name, advantages=t[name].data_ptr())
        refused(name, returns=t[name].data_ptr())
    # the two [E] rows: an output whose extent covers them
    refused("last_values", advantages=t["last_values"].data_ptr(), n_steps=1)
    refused("last_dones", returns=t["last_dones"].data_ptr(), n_steps=1, n_envs=16)
    refused("returns", returns=adv.data_ptr())
    refused("returns", returns=adv.data_ptr() + 4 * (E - 1), returns_stride=E)                      # shifted by less than a row
    refused("rewards", rewards=wide.data_ptr(), rewards_stride=2 * E + 8, advantages=wide.data_ptr() + 4 * (E - 1), advantages_stride=2 * E + 8)
    torch.cuda.synchronize()
    assert bool((adv == SENTINEL).all()) and bool((ret == SENTINEL).all())
    # accepted: rows of equal stride interleaved in one buffer, bootstrap NULL, returns NULL, and the plain call
    ok = io(rewards=wide.data_ptr(), rewards_stride=2 * E + 8, advantages=wide.data_ptr() + 4 * E, advantages_stride=2 * E + 8, bootstrap=None,
            bootstrap_stride=0, returns=None, returns_stride=0)
    assert eng.lib.mcbs_gae(eng._h, C.byref(ok), eng._stream()) == 0, eng.lib.mcbs_last_error()
    assert eng.lib.mcbs_gae(eng._h, C.byref(io()), eng._stream()) == 0, eng.lib.mcbs_last_error()
    # a no-op needs no pointers at all
    assert eng.lib.mcbs_gae(eng._h, C.byref(GaeIO(n_steps=0, n_envs=E)), eng._stream()) == 0
    assert eng.lib.mcbs_gae(eng._h, C.byref(GaeIO(n_steps=T, n_envs=0)), eng._stream()) == 0
    torch.cuda.synchronize()
    wadv, wret = _reference(case, 0.99, 0.95, True)
    assert np.array_equal(adv.cpu().numpy().view(np.int32), wadv) and np.array_equal(ret.cpu().numpy().view(np.int32), wret)


def test_method_refusals_and_empty_shapes():
    import torch
    from marlon_amd.engine import McbsError
    eng, case, t = _dense_args()
    T, E = case["rewards"].shape
    r, v, s, lv, ld, b = (t[k] for k in ("rewards", "values", "episode_starts", "last_values", "last_dones", "bootstrap"))
    adv, ret = eng.gae(r, v, s, lv, ld, 0.99, 0.95)                                                 # outputs allocated
    assert adv.shape == (T, E) and ret.shape == (T, E) and adv.dtype == torch.float32
    wadv, wret = _reference(case, 0.99, 0.95, False)
    assert np.array_equal(adv.cpu().numpy().view(np.int32), wadv) and np.array_equal(ret.cpu().numpy().view(np.int32), wret)
    transposed = r.t().contiguous().t()                                                             # [T, E] with strides (1, T)
    assert transposed.shape == r.shape and transposed.stride(1) != 1
    for bad in (
        lambda: eng.gae(r.double(), v, s, lv, ld, 0.99, 0.95),
        lambda: eng.gae(r, v.double(), s, lv, ld, 0.99, 0.95),
        lambda: eng.gae(r.cpu(), v, s, lv, ld, 0.99, 0.95),
        lambda: eng.gae(r, v, s.cpu(), lv, ld, 0.99, 0.95),
        lambda: eng.gae(r, v[:, :E - 1], s, lv, ld, 0.99, 0.95),
        lambda: eng.gae(r, v[:T - 1], s, lv, ld, 0.99, 0.95),
        lambda: eng.gae(r[0], v[0], s[0], lv, ld, 0.99, 0.95),
        lambda: eng.gae(r, v, s.int(), lv, ld, 0.99, 0.95),
        lambda: eng.gae(r, v, s.bool(), lv, ld, 0.99, 0.95),
        lambda: eng.gae(r, v, s.float(), lv, ld, 0.99, 0.95),
        lambda: eng.gae(transposed, v, s, lv, ld, 0.99, 0.95),
        lambda: eng.gae(r, v, s, lv, ld, 0.99, 0.95, advantages=transposed.clone().t().contiguous().t()),
        lambda: eng.gae(r, v, s, lv[:E - 1], ld, 0.99, 0.95),
        lambda: eng.gae(r, v, s, lv.double(), ld, 0.99, 0.95),
        lambda: eng.gae(r, v, s, lv, ld.float(), 0.99, 0.95),
        lambda: eng.gae(r, v, s, lv, ld.cpu(), 0.99, 0.95),
        lambda: eng.gae(r, v, s, lv, ld, 0.99, 0.95, bootstrap=b.double()),
        lambda: eng.gae(r, v, s, lv, ld, 0.99, 0.95, bootstrap=b[:, :E - 1]),
        lambda: eng.gae(r, v, s, lv, ld, 0.99, 0.95, advantages=adv.double()),
        lambda: eng.gae(r, v, s, lv, ld, 0.99, 0.95, returns=ret[:T - 1]),
        lambda: eng.gae(r, v, s, lv, ld, 0.99, 0.95, returns=ret.cpu()),
    ):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(McbsError, match="overlap"):
        eng.gae(r, v, s, lv, ld, 0.99, 0.95, advantages=r)
    with pytest.raises(McbsError, match="overlap"):
        eng.gae(r, v, s, lv, ld, 0.99, 0.95, advantages=adv, returns=adv)
    with pytest.raises(McbsError, match="gamma"):
        eng.gae(r, v, s, lv, ld, 1.5, 0.95)
    for Tn, En in ((0, E), (T, 0)):
        a0, r0 = eng.gae(r[:Tn, :En], v[:Tn, :En], s[:Tn, :En], lv[:En], ld[:En], 0.99, 0.95)
        assert a0.shape == (Tn, En) and r0.shape == (Tn, En)
    torch.cuda.synchronize()
