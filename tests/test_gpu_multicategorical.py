"""mcbs_multicategorical (the MultiDiscrete head, include/mcbs.h) against the fp64 restatement tests/multicategorical_ref.py, and against
torch's fp32 composite — split -> Categorical per dimension -> sums — for the error bound.

Error bound of log_prob and entropy (the rule of tests/test_gpu_categorical.py::_within): the kernel's largest absolute error against fp64
may not exceed 4 x the largest error of torch's fp32 CPU composite against fp64 on the same inputs, plus one fp32 ulp of the value (4 x:
the summation order differs).  A float32 restatement of the header's order on the CPU stays at <= 0.26 of that bound for every shape here.
Measured on the MI355X: see DESIGN.md section 7."""
import numpy as np
import pytest

from tests import multicategorical_ref as mr

pytestmark = pytest.mark.gpu

NAMES = list(mr.NVECS)
DTYPES = ["float32", "bfloat16"]


def _n_rows(name):
    """Row counts of a shape: none a multiple of any rows-per-workgroup; the widest shape (16 rows per workgroup) needs fewer."""
    return (1, 63, 65, 130) if name == "wider_than_lds" else (1, 63, 65, 1000)


def _inputs(name, dtype_name, n=None, scale=4.0):
    import torch
    nvec = mr.NVECS[name]
    n = max(_n_rows(name)) if n is None else n
    rng = np.random.default_rng(1000 * NAMES.index(name) + DTYPES.index(dtype_name))
    values = torch.as_tensor((rng.standard_normal((n, sum(nvec))) * scale).astype(np.float32)).to(getattr(torch, dtype_name))
    u = torch.as_tensor(rng.random((n, len(nvec)), dtype=np.float32))
    return nvec, values, u


def _in_interval(ref, a, u24, what):
    """Every component's u lies inside the component's fp64 CDF interval widened by (nvec[d] + 16) * 2^-23."""
    lo, hi = ref.cdf_interval(a)
    uu = u24 * 2.0 ** -24
    delta = (np.asarray(ref.nvec)[None, :] + 16) * 2.0 ** -23
    ok = (lo - delta <= uu) & (uu < hi + delta)
    assert ok.all(), f"{what}: (row, dimension) {np.argwhere(~ok)[:8].tolist()} sampled outside their CDF interval"


def _same(x, y, what):
    import torch
    for name, p, q in zip(("actions", "log_prob", "entropy"), x, y):
        same = torch.equal(p, q) if p.dtype == torch.int64 else torch.equal(p.view(torch.int32), q.view(torch.int32))
        assert same, f"{what}: {name} differs"


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_modes_against_the_restatement(name, dtype_name):
    import torch
    eng = mr.shared_engine()
    dev = eng.device
    nvec, values, u_cpu = _inputs(name, dtype_name)
    n, A = values.shape
    x32 = values.float().numpy()
    ref = mr.MultiCategoricalRef(nvec, x32)
    logits, u = values.to(dev), u_cpu.to(dev)
    before = logits.clone()
    what = f"{name} {dtype_name}"

    # ARGMAX: exact, the lowest index among equal logits
    r = eng.multicategorical(logits, nvec, mode="argmax")
    a = r.actions.cpu().numpy()
    np.testing.assert_array_equal(a, ref.argmax, err_msg=f"{what} argmax")
    lp_c, ent_c, _ = mr.composite(nvec, x32, a, torch.float32)
    mr.within(r.log_prob.cpu().numpy(), ref.log_prob(a), lp_c, f"{what} argmax log_prob")
    mr.within(r.entropy.cpu().numpy(), ref.entropy, ent_c, f"{what} entropy")

    # SAMPLE with explicit uniforms: in range, inside the CDF interval
    s = eng.multicategorical(logits, nvec, mode="sample", uniforms=u)
    a = s.actions.cpu().numpy()
    assert ref.in_range(a).all(), f"{what}: a sampled component is out of range"
    _in_interval(ref, a, mr.u24_of_uniforms(u_cpu.numpy()), what)
    mr.within(s.log_prob.cpu().numpy(), ref.log_prob(a), mr.composite(nvec, x32, a, torch.float32)[0], f"{what} sample log_prob")
    assert torch.equal(s.entropy.view(torch.int32), r.entropy.view(torch.int32)), f"{what}: the entropy depends on the mode"

    # bitwise: EVALUATE of the sampled actions, two identical calls, fewer rows, other layouts
    _same(eng.multicategorical(logits, nvec, mode="evaluate", actions=s.actions), s, f"{what} evaluate")
    _same(eng.multicategorical(logits, nvec, mode="sample", uniforms=u), s, f"{what} second call")
    for k in _n_rows(name)[:-1]:
        part = eng.multicategorical(logits[:k], nvec, mode="sample", uniforms=u[:k])
        _same(part, [x[:k] for x in s], f"{what} first {k} rows")
    k = 65
    dt = logits.dtype
    buf, view = mr.framed(k, A, A + 3, 1, dt, dev)                   # row stride A + 3, one element into a sentinel-filled buffer
    view.copy_(logits[:k])
    snapshot = buf.clone()
    _same(eng.multicategorical(view, nvec, mode="sample", uniforms=u[:k]), [x[:k] for x in s], f"{what} framed")
    _same(eng.multicategorical(view, nvec, mode="evaluate", actions=s.actions[:k].contiguous()), [x[:k] for x in s], f"{what} framed evaluate")
    assert torch.equal(mr.bits_of(buf), mr.bits_of(snapshot)) and mr.frame_untouched(buf, k, A, A + 3, 1), f"{what}: the frame was touched"
    for offset in (1, 2, 3, 5):                                       # dense rows that start off a 16-byte boundary
        flat = torch.full((offset + k * A + 9,), mr.SENTINEL, dtype=dt, device=dev)
        dense = flat[offset:offset + k * A].view(k, A)
        dense.copy_(logits[:k])
        _same(eng.multicategorical(dense, nvec, mode="sample", uniforms=u[:k]), [x[:k] for x in s], f"{what} dense rows at element {offset}")
    assert torch.equal(mr.bits_of(logits), mr.bits_of(before)), f"{what}: logits were modified"


@pytest.mark.parametrize("name", NAMES)
def test_philox_keying_and_shards(name):
    """uniforms=None: every component's u is the restatement's Philox number, at row keys from 0 and from 2^32 + 5; rows [a, b) called on
    their own with row_key_base = a are rows [a, b) of the whole call."""
    import torch
    eng = mr.shared_engine()
    nvec, values, _ = _inputs(name, "float32", n=65)
    ref = mr.MultiCategoricalRef(nvec, values.numpy())
    logits = values.to(eng.device)
    seed, step = 0x1234567800000011, (1 << 40) + 9
    lo, hi = 17, 50
    for base in (0, 2 ** 32 + 5):
        r = eng.multicategorical(logits, nvec, mode="sample", seed=seed, step=step, row_key_base=base)
        a = r.actions.cpu().numpy()
        assert ref.in_range(a).all()
        _in_interval(ref, a, mr.philox_u24(seed, base + np.arange(65), step, len(nvec)), f"{name} keys from {base}")
        part = eng.multicategorical(logits[lo:hi], nvec, mode="sample", seed=seed, step=step, row_key_base=base + lo)
        _same(part, [x[lo:hi] for x in r], f"{name} rows [{lo}, {hi}) keyed from {base + lo}")
        _same(eng.multicategorical(logits, nvec, mode="sample", seed=seed, step=step, row_key_base=base), r, f"{name} second call")
    other = eng.multicategorical(logits, nvec, mode="sample", seed=seed, step=step + 1, row_key_base=0)
    if sum(nvec) > len(nvec) + 6:
        assert not torch.equal(other.actions, r.actions)


@pytest.mark.parametrize("name", NAMES)
def test_uniform_law(name):
    """logits=None: the integer rule exactly; log_prob / entropy within one fp32 step of the rounded fp64 value."""
    import torch
    eng = mr.shared_engine()
    nvec, _, u_cpu = _inputs(name, "float32", n=65)
    D = len(nvec)
    ref = mr.MultiCategoricalRef(nvec, None, n=65)
    r = eng.multicategorical(None, nvec, mode="sample", uniforms=u_cpu.to(eng.device))
    a = r.actions.cpu().numpy()
    np.testing.assert_array_equal(a, ref.sample(mr.u24_of_uniforms(u_cpu.numpy())))
    mr.within(r.log_prob.cpu().numpy(), ref.log_prob(a), None, f"{name} uniform log_prob", rounded=True)
    mr.within(r.entropy.cpu().numpy(), ref.entropy, None, f"{name} uniform entropy", rounded=True)
    seed, step, base = 77, 3, 2 ** 32 + 5
    out = (torch.empty((65, D), dtype=torch.int64, device=eng.device), None, None)
    k = eng.multicategorical(None, nvec, mode="sample", seed=seed, step=step, row_key_base=base, out=out)
    assert k.actions is out[0]
    np.testing.assert_array_equal(k.actions.cpu().numpy(), ref.sample(mr.philox_u24(seed, base + np.arange(65), step, D)))
    e = eng.multicategorical(None, nvec, mode="evaluate", actions=k.actions)
    assert torch.equal(e.log_prob.view(torch.int32), k.log_prob.view(torch.int32))
    z = eng.multicategorical(None, nvec, mode="argmax", out=out)
    assert not bool(z.actions.any())


def test_first_and_last_index_with_nonzero_probability():
    """uniforms of 0 and 1 - 2^-24: the first and the last index whose probability is not zero (dimensions with -inf logits in front and
    behind; 40 choices span two blocks of the sums)."""
    import torch
    eng = mr.shared_engine()
    nvec = [4, 7, 1, 12, 40]
    D, A, n = len(nvec), sum(nvec), 63
    rng = np.random.default_rng(8)
    x = rng.uniform(-1.0, 1.0, (n, A)).astype(np.float32)
    first, last = np.zeros((n, D), dtype=np.int64), np.zeros((n, D), dtype=np.int64)
    off = 0
    for d, w in enumerate(nvec):
        for i in range(n):
            f = int(rng.integers(0, w))
            l = int(rng.integers(f, w))
            if w > 1:
                x[i, off:off + f] = -np.inf
                x[i, off + l + 1:off + w] = -np.inf
            first[i, d], last[i, d] = (f, l) if w > 1 else (0, 0)
        off += w
    for dt in (torch.float32, torch.bfloat16):
        logits = torch.as_tensor(x).to(dt).to(eng.device)
        zero = torch.zeros((n, D), device=eng.device)
        top = torch.full((n, D), 1.0 - 2.0 ** -24, device=eng.device)
        np.testing.assert_array_equal(eng.multicategorical(logits, nvec, uniforms=zero).actions.cpu().numpy(), first)
        np.testing.assert_array_equal(eng.multicategorical(logits, nvec, uniforms=top).actions.cpu().numpy(), last)
        np.testing.assert_array_equal(eng.multicategorical(logits, nvec, uniforms=top + 1.0).actions.cpu().numpy(), last)      # clamped to 2^24 - 1
        r = eng.multicategorical(logits, nvec, uniforms=top)
        assert bool(torch.isfinite(r.log_prob).all()) and bool(torch.isfinite(r.entropy).all())


def test_edge_rows():
    import torch
    eng = mr.shared_engine()
    dev = eng.device
    nvec = [3, 12, 5]
    A = sum(nvec)
    x = np.random.default_rng(9).standard_normal((7, A)).astype(np.float32) * 4.0
    x[0] = 0.5                                           # all equal: arg max 0, entropy sum log nvec[d]
    x[1, 3:15] = 0.0
    x[1, 7] = 80.0                                       # exp(-80) = 1.8e-35 next to exp(0)
    x[5, 3:15] = 0.0
    x[5, 7] = 120.0                                      # exp(-120) underflows to 0 in float32: no term of the entropy
    x[2, 3:15] = -np.inf
    x[2, 9] = -2.0                                       # one finite logit in its dimension
    x[4] = x[3]                                          # row 4 is row 3 with a NaN logit
    clean = torch.as_tensor(x)
    ref = mr.MultiCategoricalRef(nvec, x)
    r = eng.multicategorical(clean.to(dev), nvec, mode="argmax")
    a = r.actions.cpu().numpy()
    np.testing.assert_array_equal(a, ref.argmax)
    assert not a[0].any() and a[1, 1] == 4 and a[5, 1] == 4 and a[2, 1] == 6
    lp_c, ent_c, _ = mr.composite(nvec, x, a, torch.float32)
    mr.within(r.log_prob.cpu().numpy(), ref.log_prob(a), lp_c, "edge rows log_prob")
    mr.within(r.entropy.cpu().numpy(), ref.entropy, ent_c, "edge rows entropy")
    ent = r.entropy.cpu().numpy().astype(np.float64)
    bound = 4.0 * np.abs(ent_c - ref.entropy).max() + mr.ulp(ref.entropy)
    assert abs(ent[0] - np.log(3 * 12 * 5)) <= bound[0]
    for i in (1, 5):
        assert np.isfinite(ent[i]) and ent[i] >= -bound[i]
    # a NaN logit: every sampled component of its row stays in range, the other rows are what they were
    u = torch.rand((7, 3), generator=torch.Generator().manual_seed(1)).to(dev)
    base = eng.multicategorical(clean.to(dev), nvec, uniforms=u)
    for dt in (torch.float32, torch.bfloat16):
        for col in (0, 5, A - 1):
            bad = clean.clone()
            bad[4, col] = float("nan")
            for mode in ("sample", "argmax"):
                got = eng.multicategorical(bad.to(dt).to(dev), nvec, mode=mode, uniforms=u if mode == "sample" else None)
                g = got.actions.cpu().numpy()
                assert ((g >= 0) & (g < np.asarray(nvec))).all(), f"NaN at column {col}, {mode}: a component left its range"
                if dt == torch.float32 and mode == "sample":
                    keep = [0, 1, 2, 3, 5, 6]
                    _same([t[keep] for t in got], [t[keep] for t in base], f"NaN at column {col}: another row changed")


def test_evaluate_counts_rows_with_a_component_out_of_range():
    import torch
    eng = mr.shared_engine()
    dev = eng.device
    nvec, values, u = _inputs("defender_toyctf", "float32", n=65)
    logits = values.to(dev)
    s = eng.multicategorical(logits, nvec, uniforms=u.to(dev))
    acts = s.actions.clone()
    acts[5, 3] = -1
    acts[40, 0] = nvec[0]
    acts[64, 11] = nvec[11]
    acts[64, 2] = -7                                     # two components of one row: one row
    count = torch.full((1,), 5, dtype=torch.int32, device=dev)
    e = eng.multicategorical(logits, nvec, mode="evaluate", actions=acts, bad_actions=count)
    assert int(count.item()) == 5 + 3
    eng.multicategorical(logits, nvec, mode="evaluate", actions=acts, bad_actions=count)
    assert int(count.item()) == 5 + 6                    # increased, not zeroed
    bad = torch.zeros(65, dtype=torch.bool)
    bad[[5, 40, 64]] = True
    lp = e.log_prob.cpu()
    assert bool(torch.isnan(lp[bad]).all())
    assert torch.equal(lp[~bad].view(torch.int32), s.log_prob.cpu()[~bad].view(torch.int32))
    assert torch.equal(e.entropy.view(torch.int32), s.entropy.view(torch.int32)), "the entropy of such a row is still the row's"
    eng.multicategorical(logits, nvec, mode="evaluate", actions=s.actions, bad_actions=count)
    assert int(count.item()) == 5 + 6


def test_refusals():
    import torch
    from marlon_amd import engine
    eng = mr.shared_engine()
    dev = eng.device
    refused = (engine.McbsError, ValueError)
    logits = torch.zeros((4, 40), device=dev)
    with pytest.raises(refused, match="n_dims"):
        eng.multicategorical(logits, [])
    with pytest.raises(refused, match="n_dims"):
        eng.multicategorical(logits, [2] * 17)
    with pytest.raises(refused, match=r"nvec\[1\]"):
        eng.multicategorical(logits, [3, 0, 2])
    with pytest.raises(refused, match=r"nvec\[0\]"):
        eng.multicategorical(None, [65537])              # (the uniform law: no row of logits that wide is needed)
    with pytest.raises(refused):
        eng.multicategorical(logits[:, :9], [5, 5])      # rows narrower than A
    with pytest.raises(refused, match="step"):
        eng.multicategorical(logits, [5, 5], step=2 ** 48)
    with pytest.raises(refused):
        eng.multicategorical(logits, [5, 5], mode="mean")
    ok = eng.multicategorical(logits, [5, 5], step=2 ** 48 - 1)
    assert bool(((ok.actions >= 0) & (ok.actions < 5)).all())

    # the C entry point itself: each refusal is MCBS_EINVAL (-1) with a message that names the argument
    import ctypes as C
    acts = torch.zeros((4, 2), dtype=torch.int64, device=dev)
    lp = torch.zeros(4, device=dev)
    nv = (C.c_uint32 * 17)(*([5, 5] + [1] * 15))

    def raw(nvec=nv, D=2, rows=4, logits_p=logits.data_ptr(), dtype=0, stride=40, mode=0, acts_p=acts.data_ptr(), lp_p=lp.data_ptr(), step=0):
        return eng.lib.mcbs_multicategorical(eng._h, nvec, D, rows, logits_p, dtype, stride, mode, acts_p, lp_p, None, None, 0, step, 0, None, None)

    torch.cuda.synchronize()
    assert raw() == 0
    for what, kw, word in (("D = 0", dict(D=0), b"n_dims"), ("D = 17", dict(D=17), b"n_dims"), ("nvec NULL", dict(nvec=None), b"nvec"),
                           ("nvec entry 0", dict(nvec=(C.c_uint32 * 2)(5, 0)), b"nvec[1]"), ("row_stride", dict(stride=9), b"row_stride"),
                           ("step", dict(step=2 ** 48), b"step"), ("mode", dict(mode=3), b"mode"), ("dtype", dict(dtype=2), b"dtype"),
                           ("actions NULL", dict(acts_p=None), b"actions"), ("log_prob NULL", dict(lp_p=None), b"log_prob")):
        rc = raw(**kw)
        assert rc == -1, f"{what}: {rc}"
        assert word in eng.lib.mcbs_last_error(), (what, eng.lib.mcbs_last_error())
    assert raw(rows=0, logits_p=None, acts_p=None, lp_p=None) == 0
    assert raw(logits_p=None, stride=0, dtype=9) == 0    # the uniform law ignores dtype and row_stride
    torch.cuda.synchronize()
    # the method's own argument checks
    u = torch.zeros((4, 2), device=dev)
    for bad_call in (
        lambda: eng.multicategorical(logits.double(), [5, 5]),
        lambda: eng.multicategorical(logits.cpu(), [5, 5]),
        lambda: eng.multicategorical(logits.t().contiguous().t(), [5, 5]),
        lambda: eng.multicategorical(logits, [5, 5], mode="evaluate"),
        lambda: eng.multicategorical(logits, [5, 5], mode="evaluate", actions=acts.int()),
        lambda: eng.multicategorical(logits, [5, 5], mode="evaluate", actions=acts[:, :1]),
        lambda: eng.multicategorical(logits, [5, 5], actions=acts),
        lambda: eng.multicategorical(logits, [5, 5], uniforms=u[:, :1]),
        lambda: eng.multicategorical(logits, [5, 5], uniforms=u.double()),
        lambda: eng.multicategorical(logits, [5, 5], out=(acts, lp)),
        lambda: eng.multicategorical(logits, [5, 5], out=(acts, lp[:3], None)),
        lambda: eng.multicategorical(logits, [5, 5], mode="evaluate", actions=acts, bad_actions=torch.zeros(1, device=dev)),
    ):
        with pytest.raises(ValueError):
            bad_call()
    empty = eng.multicategorical(logits[:0], [5, 5])
    assert empty.actions.shape == (0, 2) and empty.log_prob.shape == (0,)


def _toyctf_pair(n_envs, env_id_base=0, **kw):
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.wrappers import AttackerVecEnv, DefenderVecEnv
    from tests import parity
    att = AttackerVecEnv(parity.topology_for("toyctf"), n_envs, maximum_node_count=12, maximum_total_credentials=10,
                         attacker_goal=ce.AttackerGoal(own_atleast=6), defender_constraint=ce.DefenderConstraint(0.6), losing_reward=-5000.0,
                         max_timesteps=50, learned_defender=True, env_id_base=env_id_base, **kw)
    return att, DefenderVecEnv(att, max_timesteps=50, invalid_action_reward=-1, loss_reward=-5000.0)


def test_wrappers_sample_step_and_shard():
    import torch
    att, dfd = _toyctf_pair(64)
    dev = att.engine.device
    assert list(dfd.nvec) == mr.NVECS["defender_toyctf"]
    g = torch.Generator(device=dev).manual_seed(2)
    logits = torch.randn((64, int(dfd.nvec.sum())), generator=g, device=dev) * 2.0
    r = dfd.sample_actions(logits, seed=11, step=4)
    assert r.actions.shape == (64, 12) and r.actions.dtype == torch.int64
    a = r.actions.cpu().numpy()
    assert ((a >= 0) & (a < dfd.nvec)).all()
    att.step(att.sample_uniform(seed=3, step=0).actions)
    obs, reward, terminated, truncated, info = dfd.step(r.actions)                      # accepted as it is
    assert reward.shape == (64,) and info["valid_action"].shape == (64,)
    e = dfd.evaluate_actions(logits, r.actions)
    assert torch.equal(e.log_prob.view(torch.int32), r.log_prob.view(torch.int32))
    top = dfd.sample_actions(logits, seed=11, step=4, deterministic=True)
    ref = mr.MultiCategoricalRef(dfd.nvec, logits.cpu().numpy())
    np.testing.assert_array_equal(top.actions.cpu().numpy(), ref.argmax)
    uni = dfd.sample_uniform(seed=11, step=5)
    np.testing.assert_array_equal(uni.actions.cpu().numpy(),
                                  mr.MultiCategoricalRef(dfd.nvec, None, n=64).sample(mr.philox_u24(11, np.arange(64), 5, 12)))
    dfd.step(uni.actions)
    # the attacker's MultiDiscrete action through the same head
    la = torch.randn((64, int(att.nvec.sum())), generator=g, device=dev)
    ra = att.sample_actions(la, seed=11, step=4)
    assert ra.actions.shape == (64, 10) and ((ra.actions.cpu().numpy() >= 0) & (ra.actions.cpu().numpy() < att.nvec)).all()
    att.step(ra.actions)
    att.step(att.sample_uniform(seed=3, step=0).actions)
    assert torch.equal(att.evaluate_actions(la, ra.actions).log_prob.view(torch.int32), ra.log_prob.view(torch.int32))
    # two shards of 32 envs draw what the 64 envs drew
    for base in (0, 32):
        s_att, s_dfd = _toyctf_pair(32, env_id_base=base)
        part = s_dfd.sample_actions(logits[base:base + 32], seed=11, step=4)
        _same(part, [x[base:base + 32] for x in r], f"shard at env {base}")
        pu = s_dfd.sample_uniform(seed=11, step=5)
        assert torch.equal(pu.actions, uni.actions[base:base + 32])
        s_att.close()
    att.close()


def test_discrete_attacker_names_the_masked_head():
    import torch
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.samples import chainpattern
    from marlon_amd.wrappers import AttackerVecEnv
    env = AttackerVecEnv(chainpattern.new_environment(4), 64, maximum_node_count=6, maximum_total_credentials=6,
                         attacker_goal=ce.AttackerGoal(own_atleast_percent=1.0), max_timesteps=50, discrete=True, materialize_masks=False)
    logits = torch.zeros((64, int(env.nvec.sum())), device=env.engine.device)
    acts = torch.zeros((64, 10), dtype=torch.int64, device=env.engine.device)
    for call in (lambda: env.sample_actions(logits, 0, 0), lambda: env.sample_uniform(0, 0), lambda: env.evaluate_actions(logits, acts)):
        with pytest.raises(RuntimeError, match="sample_masked.*evaluate_masked"):
            call()
    env.close()
