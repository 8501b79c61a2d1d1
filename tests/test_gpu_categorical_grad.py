"""mcbs_masked_categorical_grad (the backward pass of the masked categorical head, include/mcbs.h) against the fp64 closed form
tests/categorical_grad_ref.py, and against torch's fp32 autograd through `Categorical(logits=where(mask, logits, -1e8))` for the error
bound.

Error bound (the rule of test_gpu_categorical.py): over the allowed entries, the kernel's largest absolute error against fp64 may not
exceed 4 x the largest error of torch's fp32 CPU autograd composite against fp64 on the same inputs (taken on logits.float()), plus one
ulp of the value in the output dtype (float32, or bfloat16 for bfloat16 logits).  Masked entries, all-zero rows and rows whose action
lies outside [0, A) are +0.0 bit for bit.  Measured on the MI355X: see DESIGN.md section 7."""
import functools

import numpy as np
import pytest

from tests import categorical_grad_ref as gr

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


def _chain4_engine(n_envs=64, **kw):
    from marlon_amd import engine
    from marlon_amd._abi import EnvSpec
    from marlon_amd.flatten import flatten
    from marlon_amd.samples import chainpattern
    topo = flatten(chainpattern.new_environment(4))
    return engine.BatchEngine(topo, EnvSpec(n_envs=n_envs, maximum_node_count=6, maximum_total_credentials=6,
                                            attacker_goal=dict(own_atleast_percent=1.0), **kw))


def _ulp(want, bf16):
    u = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return u * 65536.0 if bf16 else u                    # bfloat16 keeps 8 of float32's 24 significand bits


def _within(got, want, comp, sel, what, bf16=False):
    """|got - want| <= 4 * (largest |comp - want| over sel) + one ulp of the value, over the entries sel; prints both figures."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)[sel]
    comp_err = float(np.abs(comp - want)[sel].max())
    print(f"{what}: kernel max abs error {err.max():.3e}, fp32 composite {comp_err:.3e}, ratio {err.max() / max(comp_err, 1e-300):.2f}")
    bound = 4.0 * comp_err + _ulp(want[sel], bf16)
    worst = int(np.argmax(err - bound))
    assert np.all(err <= bound), f"{what}: entry {worst}: error {err[worst]:.3e} > bound {bound[worst]:.3e} (value {want[sel][worst]!r})"


def _bits_of(x):
    import torch
    return x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def _framed(n, A, stride, offset, dtype, dev):
    """A [n, A] view at element `offset` with row stride `stride` inside a sentinel-filled buffer -> (buffer, view)."""
    import torch
    buf = torch.full((offset + n * stride + 9,), SENTINEL, dtype=dtype, device=dev)
    return buf, buf[offset:offset + n * stride].view(n, stride)[:, :A]


def _frame_untouched(buf, n, A, stride, offset):
    rows = buf[offset:offset + n * stride].view(n, stride)
    return bool((buf[:offset] == SENTINEL).all()) and bool((rows[:, A:] == SENTINEL).all()) and bool((buf[offset + n * stride:] == SENTINEL).all())


# output layouts (element offset, row stride - A): A = 1830, so a stride of A + 6 makes float32 rows 16-byte and bfloat16 rows 8-byte
# aligned at offset 0, A + 2 makes bfloat16 rows 16-byte aligned; the odd offsets take the element-store path
LAYOUTS = {"float32": ((0, 6), (1, 6), (3, 6)), "bfloat16": ((0, 2), (0, 6), (1, 6), (5, 6))}


@functools.lru_cache(maxsize=None)
def _synthetic_run(dtype_name, poison):
    """Test 1 / 2 for one dtype: every layout and both forms of bits checked against each other; returns the first output (device),
    and the inputs.  poison: NaN / +Inf / -Inf written into the logits under every clear mask bit."""
    import torch
    eng = _chain4_engine()
    dev = eng.device
    dt = getattr(torch, dtype_name)
    A = eng.discrete_action_count()
    W, row_words = eng.packed_mask_words()
    assert A == 1830 and W == 58
    n = 64
    mask, base, actions, g_lp, g_H = gr.synthetic_inputs(A, n)
    actions = actions.copy()
    actions[9], actions[10] = -1, A
    values = torch.as_tensor(base).to(dt)
    if poison:
        bad = torch.tensor([float("nan"), float("inf"), float("-inf")], dtype=dt)[torch.arange(n * A).view(n, A) % 3]
        values = torch.where(torch.as_tensor(mask), values, bad)
    # logits: a view offset by one element with row_stride > A; and aligned rows of the output's stride for the whole-group loads
    lbuf, logits = _framed(n, A, A + 7, 1, dt, dev)
    logits.copy_(values)
    bits_wide = torch.as_tensor(gr.pack(mask, W + 6, garbage_tail=True), device=dev)
    bits_clean = torch.as_tensor(gr.pack(mask, row_words), device=dev)
    ta, tl, th = (torch.as_tensor(x, device=dev) for x in (actions, g_lp, g_H))
    before = [x.clone() for x in (lbuf, bits_wide, bits_clean, ta)]
    first = None
    for offset, pad in LAYOUTS[dtype_name]:
        aligned = torch.full((n, A + pad), SENTINEL, dtype=dt, device=dev)
        aligned[:, :A] = values
        for bits in (bits_wide, bits_clean):
            for lg in ((logits, aligned[:, :A]) if offset == 0 else (logits,)):
                buf, out = _framed(n, A, A + pad, offset, dt, dev)
                got = eng.masked_categorical_grad(lg, bits, ta, tl, th, out=out)
                assert got.data_ptr() == out.data_ptr()
                what = f"{dtype_name} offset {offset} stride A+{pad}"
                assert _frame_untouched(buf, n, A, A + pad, offset), f"{what}: sentinels touched"
                buf2, out2 = _framed(n, A, A + pad, offset, dt, dev)
                eng.masked_categorical_grad(lg, bits, ta, tl, th, out=out2)
                assert torch.equal(_bits_of(buf), _bits_of(buf2)), f"{what}: two calls differ"
                if first is None:
                    first = out.contiguous()
                assert torch.equal(_bits_of(out.contiguous()), _bits_of(first)), f"{what}: the layout or the garbage bits change the result"
    for x, y in zip((lbuf, bits_wide, bits_clean, ta), before):
        assert torch.equal(_bits_of(x) if x.is_floating_point() else x, _bits_of(y) if y.is_floating_point() else y), "an input was modified"
    eng.close()
    return first, mask, values, actions, g_lp, g_H


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_synthetic_rows(dtype_name):
    import torch
    first, mask, values, actions, g_lp, g_H = _synthetic_run(dtype_name, False)
    n, A = mask.shape
    got = first.cpu()
    x32 = values.float().numpy()
    want = gr.closed_form(mask, x32, actions, g_lp, g_H)
    inside = (actions >= 0) & (actions < A)
    comp = np.zeros_like(want)
    comp[inside] = gr.composite_grad(mask[inside], x32[inside], actions[inside], g_lp[inside], g_H[inside], torch.float32)
    sel = mask & inside[:, None]
    _within(got.double().numpy(), want, comp, sel, f"synthetic rows {dtype_name}", bf16=dtype_name == "bfloat16")
    zero = ~sel
    assert zero[3].all() and zero[9].all() and zero[10].all() and zero[1, 0]
    assert not _bits_of(got)[torch.as_tensor(zero)].any(), "a masked entry, the blank row or a row with an action outside [0, A) is not +0.0"


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_masked_logits_never_matter(dtype_name):
    """NaN, +Inf and -Inf under every clear bit: the output is bit for bit that of the clean logits."""
    import torch
    clean = _synthetic_run(dtype_name, False)[0]
    poisoned, _, values, *_ = _synthetic_run(dtype_name, True)
    assert not bool(torch.isfinite(values.float()).all())
    assert torch.equal(_bits_of(poisoned), _bits_of(clean))


def test_optional_gradients():
    import torch
    eng = _chain4_engine()
    dev = eng.device
    A = eng.discrete_action_count()
    W, row_words = eng.packed_mask_words()
    mask, base, actions, g_lp, g_H = gr.synthetic_inputs(A)
    n = mask.shape[0]
    logits = torch.as_tensor(base, device=dev)
    bits = torch.as_tensor(gr.pack(mask, row_words), device=dev)
    ta, tl, th = (torch.as_tensor(x, device=dev) for x in (actions, g_lp, g_H))
    zeros = torch.zeros(n, device=dev)
    for dt in (torch.float32, torch.bfloat16):
        lg = logits.to(dt)
        run = lambda a, b: _bits_of(eng.masked_categorical_grad(lg, bits, ta, a, b))
        assert torch.equal(run(tl, None), run(tl, zeros))
        assert torch.equal(run(None, th), run(zeros, th))
        assert bool(run(tl, None).any()) and bool(run(None, th).any())
        assert not torch.equal(run(tl, th), run(tl, None)) and not torch.equal(run(tl, th), run(None, th))
        out = torch.full((n, A + 3), SENTINEL, dtype=dt, device=dev)
        eng.masked_categorical_grad(lg, bits, ta, None, None, out=out)
        assert not bool(_bits_of(out[:, :A]).any()), "no incoming gradient: every element below A must have been written with +0.0"
        assert bool((out[:, A:] == SENTINEL).all())
    eng.close()


@pytest.mark.parametrize("nodes,A_want,W_want", [(12, 14172, 443), (14, 19278, 603)])
def test_wide_rows(nodes, A_want, W_want):
    """Chain-10 @ 12/12 (A = 14 172: 443 mask words, 7 blocks of 64, all of them inside the wavefront's LDS cache of 512 words) and
    @ 14/12 (A = 19 278: 603 words, so the words beyond the cache are read from memory again in sweep 2 and in the store phase).
    Rows padded to a whole number of 16-byte groups, so groups of logits are loaded whole; dense [n, A] rows must give the same bits."""
    import torch
    from marlon_amd import engine
    from marlon_amd._abi import EnvSpec
    from marlon_amd.flatten import flatten
    from marlon_amd.samples import chainpattern
    eng = engine.BatchEngine(flatten(chainpattern.new_environment(10)),
                             EnvSpec(n_envs=64, maximum_node_count=nodes, maximum_total_credentials=12, attacker_goal=dict(own_atleast_percent=1.0)))
    dev = eng.device
    A = eng.discrete_action_count()
    W, row_words = eng.packed_mask_words()
    assert (A, W) == (A_want, W_want) and (W > 512) == (nodes == 14)
    n = 64
    rng = np.random.default_rng(31)
    mask = rng.random((n, A)) < (rng.random((n, 1)) ** 2)
    mask[0, :] = True
    mask[1, :] = False
    mask[1, (W - 1) * 32 + 3] = True                     # a single bit, in the last word
    mask[2, :] = False
    logits = (rng.standard_normal((n, A)) * 4.0).astype(np.float32)
    actions = np.array([np.flatnonzero(mask[i])[rng.integers(0, mask[i].sum())] if mask[i].any() else 0 for i in range(n)], dtype=np.int64)
    actions[3] = int(np.flatnonzero(~mask[3])[-1])       # not allowed, near the row's end
    g_lp, g_H = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    bits = torch.as_tensor(gr.pack(mask, row_words), device=dev)
    stride = (A + 3) // 4 * 4
    padded = torch.zeros((n, stride), device=dev)
    padded[:, :A] = torch.as_tensor(logits)
    out = torch.full((n, stride), SENTINEL, device=dev)
    args = (bits, torch.as_tensor(actions, device=dev), torch.as_tensor(g_lp, device=dev), torch.as_tensor(g_H, device=dev))
    eng.masked_categorical_grad(padded[:, :A], *args, out=out[:, :A])
    assert bool((out[:, A:] == SENTINEL).all())
    dense = eng.masked_categorical_grad(padded[:, :A].contiguous(), *args)
    assert torch.equal(_bits_of(dense), _bits_of(out[:, :A].contiguous())), "padded and dense rows differ"
    got = dense.cpu()
    want = gr.closed_form(mask, logits, actions, g_lp, g_H)
    comp = gr.composite_grad(mask, logits, actions, g_lp, g_H, torch.float32)
    _within(got.double().numpy(), want, comp, mask, f"wide rows float32 A={A}")
    assert not _bits_of(got)[torch.as_tensor(~mask)].any()
    eng.close()


def test_more_rows_than_one_grid():
    """One grid covers 4 * 65 536 rows: rows beyond are reached by the stride loop.  The 64 synthetic rows tiled: every tile must repeat
    the first bit for bit."""
    import torch
    eng = _chain4_engine()
    dev = eng.device
    A = eng.discrete_action_count()
    W, row_words = eng.packed_mask_words()
    mask, base, actions, g_lp, g_H = gr.synthetic_inputs(A)
    reps = 4 * 65536 // 64 + 3
    bits = torch.as_tensor(gr.pack(mask, row_words), device=dev).repeat(reps, 1)
    logits = torch.as_tensor(base, device=dev).to(torch.bfloat16).repeat(reps, 1)
    ta, tl, th = (torch.as_tensor(x, device=dev).repeat(reps) for x in (actions, g_lp, g_H))
    got = _bits_of(eng.masked_categorical_grad(logits, bits, ta, tl, th)).view(reps, 64 * A)
    one = _bits_of(eng.masked_categorical_grad(logits[:64], bits[:64], ta[:64], tl[:64], th[:64])).view(1, 64 * A)
    assert bool(one.any())
    assert bool((got == one).all()), "a tile differs from the first"
    eng.close()


def test_autograd_end_to_end():
    """A Linear(32, A) policy head, 256 stored rows of a short rollout, the PPO loss: the gradients of weight and bias through
    evaluate_masked(differentiable=True) against the same loss through the composite (fp64 on the CPU; the fp32 composite on the CPU
    sets the bound)."""
    import torch
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.samples import chainpattern
    from marlon_amd.wrappers import AttackerVecEnv
    E, T, F = 64, 4, 32
    env = AttackerVecEnv(chainpattern.new_environment(4), E, maximum_node_count=6, maximum_total_credentials=6,
                         attacker_goal=ce.AttackerGoal(own_atleast_percent=1.0), max_timesteps=50, discrete=True, materialize_masks=False)
    dev = env.engine.device
    A = env.discrete_n
    W, row_words = env.engine.packed_mask_words()
    torch.manual_seed(5)
    head = torch.nn.Linear(F, A).to(dev)
    g = torch.Generator(device=dev).manual_seed(6)
    feats = torch.randn((T, E, F), generator=g, device=dev)
    buf = torch.zeros((T, E, row_words), dtype=torch.int32, device=dev)
    acts = torch.zeros((T, E), dtype=torch.int64, device=dev)
    lps = torch.zeros((T, E), device=dev)
    with torch.no_grad():
        for t in range(T):
            env.action_masks_packed(out=buf[t])
            r = env.sample_masked(head(feats[t]), seed=3, step=t)
            acts[t], lps[t] = r.actions, r.log_prob
            env.step(r.actions)
    n = T * E
    x, bits, actions = feats.view(n, F), buf.view(n, row_words), acts.view(n)
    old_lp = lps.view(n) + 0.1 * torch.randn(n, generator=g, device=dev)
    adv = torch.randn(n, generator=g, device=dev)
    mask = env.unpack_action_mask(bits)
    assert bool(mask.any(1).all()) and bool(mask[torch.arange(n, device=dev), actions].all())

    def loss_of(lp, ent, old, a):
        return -(torch.exp(lp - old) * a).mean() - 0.01 * ent.mean()

    def composite(dtype):
        """weight.grad, bias.grad of the loss through where -> Categorical on the CPU in `dtype`."""
        lin = torch.nn.Linear(F, A).to(dtype)
        lin.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in head.state_dict().items()})
        tm = mask.cpu()
        dist = torch.distributions.Categorical(logits=torch.where(tm, lin(x.cpu().to(dtype)), torch.tensor(-1e8, dtype=dtype)))
        ent = -(torch.where(tm, dist.logits * dist.probs, torch.zeros((), dtype=dtype))).sum(-1)
        loss_of(dist.log_prob(actions.cpu()), ent, old_lp.cpu().to(dtype), adv.cpu().to(dtype)).backward()
        return lin.weight.grad.double().numpy(), lin.bias.grad.double().numpy()

    logits = head(x)
    r = env.evaluate_masked(bits, logits, actions, differentiable=True)
    plain = env.evaluate_masked(bits, logits.detach(), actions)
    assert r.log_prob.requires_grad and r.entropy.requires_grad and not r.n_allowed.requires_grad and not plain.log_prob.requires_grad
    for a, b in zip(r[1:], plain[1:]):
        assert torch.equal(a.detach().view(torch.int32), b.view(torch.int32)), "differentiable=True changes the forward's numbers"
    loss_of(r.log_prob, r.entropy, old_lp, adv).backward()
    want, c32 = composite(torch.float64), composite(torch.float32)
    for name, got, w, c in (("weight.grad", head.weight.grad, want[0], c32[0]), ("bias.grad", head.bias.grad, want[1], c32[1])):
        _within(got.cpu().double().numpy(), w, c, np.ones(w.shape, dtype=bool), f"end to end {name}")
    # a loss of one output alone backpropagates (the other's incoming gradient is absent)
    for pick in (1, 2):
        head.zero_grad()
        env.evaluate_masked(bits, head(x), actions, differentiable=True)[pick].sum().backward()
        assert bool(torch.isfinite(head.weight.grad).all()) and bool(head.weight.grad.any())
    with pytest.raises(ValueError):
        env.evaluate_masked(bits, head(x), actions, differentiable=True, out=(None, None, None, None))
    env.close()


def test_refusals():
    import ctypes as C

    import torch
    from marlon_amd import engine
    eng = _chain4_engine()
    dev = eng.device
    A = eng.discrete_action_count()
    W, row_words = eng.packed_mask_words()
    n = 8
    logits = torch.zeros((n, A), device=dev)
    bits = torch.full((n, row_words), 0x55555555, dtype=torch.int32, device=dev)
    acts = torch.zeros(n, dtype=torch.int64, device=dev)
    g = torch.ones(n, device=dev)
    out = torch.empty((n, A), device=dev)
    ok = eng.masked_categorical_grad(logits, bits, acts, g, g, out=out)
    assert ok is out and bool(torch.isfinite(out).all()) and bool(out.any())

    # the C entry point itself: each refusal is MCBS_EINVAL (-1)
    def raw(bits_p=bits.data_ptr(), words=row_words, rows=n, logits_p=logits.data_ptr(), dtype=0, stride=A, acts_p=acts.data_ptr(),
            out_p=out.data_ptr(), out_stride=A):
        return eng.lib.mcbs_masked_categorical_grad(eng._h, bits_p, words, rows, logits_p, dtype, stride, acts_p, g.data_ptr(), None, out_p, out_stride, None)

    torch.cuda.synchronize()
    assert raw() == 0
    for what, rc in (("bits NULL", raw(bits_p=None)), ("logits NULL", raw(logits_p=None)), ("actions NULL", raw(acts_p=None)),
                     ("grad_logits NULL", raw(out_p=None)), ("dtype", raw(dtype=2)), ("bits_row_words", raw(words=W - 1)),
                     ("row_stride", raw(stride=A - 1)), ("grad_row_stride", raw(out_stride=A - 1)),
                     ("in place", raw(out_p=logits.data_ptr())), ("overlap", raw(out_p=logits.data_ptr() + 4 * (A - 1)))):
        assert rc == -1, f"{what}: {rc}"
        assert eng.lib.mcbs_last_error()
    assert raw(rows=0, bits_p=None, logits_p=None, acts_p=None, out_p=None) == 0
    torch.cuda.synchronize()
    # rows of the same stride interleaved in one buffer do not overlap
    both = torch.zeros((n, 2 * A), device=dev)
    eng.masked_categorical_grad(both[:, :A], bits, acts, g, g, out=both[:, A:])
    assert bool(both[:, A:].any()) and not bool(both[:, :A].any())
    with pytest.raises(engine.McbsError, match=r"\(-1\).*overlap"):
        eng.masked_categorical_grad(both[:, :A], bits, acts, g, g, out=both[:, 1:A + 1])
    with pytest.raises(engine.McbsError, match=r"\(-1\).*overlap"):
        eng.masked_categorical_grad(logits, bits, acts, g, g, out=logits)
    # the method's own argument checks
    for bad_call in (
        lambda: eng.masked_categorical_grad(None, bits, acts, g, g),
        lambda: eng.masked_categorical_grad(logits.double(), bits, acts, g, g),
        lambda: eng.masked_categorical_grad(logits.half(), bits, acts, g, g),
        lambda: eng.masked_categorical_grad(logits[:, :A - 1], bits, acts, g, g),
        lambda: eng.masked_categorical_grad(logits[:4], bits, acts, g, g),
        lambda: eng.masked_categorical_grad(logits.cpu(), bits, acts, g, g),
        lambda: eng.masked_categorical_grad(logits.t().contiguous().t(), bits, acts, g, g),
        lambda: eng.masked_categorical_grad(logits, None, acts, g, g),
        lambda: eng.masked_categorical_grad(logits, bits.long(), acts, g, g),
        lambda: eng.masked_categorical_grad(logits, bits[:, :W - 1], acts, g, g),
        lambda: eng.masked_categorical_grad(logits, bits.cpu(), acts, g, g),
        lambda: eng.masked_categorical_grad(logits, bits, None, g, g),
        lambda: eng.masked_categorical_grad(logits, bits, acts.int(), g, g),
        lambda: eng.masked_categorical_grad(logits, bits, acts[:5], g, g),
        lambda: eng.masked_categorical_grad(logits, bits, acts, g.double(), g),
        lambda: eng.masked_categorical_grad(logits, bits, acts, g, g[:5]),
        lambda: eng.masked_categorical_grad(logits, bits, acts, g, g, out=out.bfloat16()),
        lambda: eng.masked_categorical_grad(logits, bits, acts, g, g, out=out[:, :A - 1]),
        lambda: eng.masked_categorical_grad(logits, bits, acts, g, g, out=out[:4]),
        lambda: eng.masked_categorical_grad(logits, bits, acts, g, g, out=out.cpu()),
    ):
        with pytest.raises(ValueError):
            bad_call()
    expect = eng.masked_categorical_grad(logits, bits, acts, g, g)
    empty = eng.masked_categorical_grad(logits[:0], bits[:0], acts[:0], g[:0], g[:0])
    assert empty.shape == (0, A) and empty.dtype == logits.dtype
    eng.close()
    ere = _chain4_engine(defender=("random_events",))   # the batch only supplies the device and A: every defender kind is served
    served = ere.masked_categorical_grad(logits, bits, acts, g, g)
    assert torch.equal(served, expect)
    ere.close()
