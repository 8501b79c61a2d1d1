"""mcbs_masked_linear_categorical_grad (the backward pass of the masked action head from the latent, include/mcbs.h) against the fp64
closed form and the error bound of tests/linear_head_grad_ref.py, against mcbs_masked_categorical_grad for g bit for bit, and through
torch's autograd (BatchEngine.masked_linear_evaluate, evaluate_masked_from_latent(differentiable=True)).

The bound holds for any order of the three sums (linear_head_grad_ref's docstring); an entry whose bound is 0 — a dead row, an action no
live row allows — must be +0.0 bit for bit.  Sums of a single term are compared bit for bit with the rounded product added to +0.0:
the header's chains start at +0.0, so a product of -0.0 (a zero latent entry times a negative g) comes out as +0.0.
Measured on the MI355X: see DESIGN.md section 7."""
import functools

import numpy as np
import pytest

from tests import categorical_grad_ref as gr
from tests import linear_head_grad_ref as lg
from tests import linear_head_ref as lhr

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
OUTS = ("grad_latent", "grad_weight", "grad_bias")
ROW_BLOCK = 512


def _chain4_engine(n_envs=64, **kw):
    from marlon_amd import engine
    from marlon_amd._abi import EnvSpec
    from marlon_amd.flatten import flatten
    from marlon_amd.samples import chainpattern
    topo = flatten(chainpattern.new_environment(4))
    return engine.BatchEngine(topo, EnvSpec(n_envs=n_envs, maximum_node_count=6, maximum_total_credentials=6,
                                            attacker_goal=dict(own_atleast_percent=1.0), **kw))


def _chain10_engine(nodes):
    from marlon_amd import engine
    from marlon_amd._abi import EnvSpec
    from marlon_amd.flatten import flatten
    from marlon_amd.samples import chainpattern
    return engine.BatchEngine(flatten(chainpattern.new_environment(10)),
                              EnvSpec(n_envs=64, maximum_node_count=nodes, maximum_total_credentials=12, attacker_goal=dict(own_atleast_percent=1.0)))


def _i32(x):
    import torch
    return x.contiguous().view(torch.int32)


def _on_device(eng, c, dt, row_words=None, garbage_tail=False, with_bias=True):
    """A case of linear_head_grad_ref (NumPy) as the device arguments of masked_linear_categorical_grad, in call order."""
    import torch
    dev = eng.device
    W, rw = eng.packed_mask_words()
    bits = torch.as_tensor(gr.pack(c["mask"], row_words or rw, garbage_tail=garbage_tail), device=dev)
    lat, wt, b = (torch.as_tensor(c[k], device=dev).to(dt) for k in ("latent", "weight", "bias"))
    return [lat, wt, b if with_bias else None, bits] + [torch.as_tensor(c[k], device=dev) for k in ("actions", "g_lp", "g_H")]


@functools.lru_cache(maxsize=None)
def _reference(A, H, exact, bf16, n=64):
    """The case, its fp64 closed form, its bound and the fp32 CPU composite's error, computed once and shared (read-only)."""
    import torch
    c = lg.case(A, H, exact, n=n, bf16=bf16)
    want = lg.closed_form(**c)
    bound = lg.bounds(exact=exact, **c)
    comp = lg.composite_grads(dtype=torch.float32, **c)
    comp_err = {k: float(np.abs(comp[k] - want[k]).max()) for k in OUTS}
    return c, want, bound, comp_err


def _check_bound(got, want, bound, comp_err, what):
    """Every entry of the three outputs within its bound, +0.0 bit for bit where the bound is 0; prints the worst error / bound and the
    ratio of the largest error to the fp32 composite's.  -> the worst error / bound."""
    import torch
    worst = 0.0
    for k, g in zip(OUTS, got):
        assert g.dtype == torch.float32, (what, k)
        g64 = g.double().cpu().numpy()
        assert np.isfinite(g64).all(), (what, k)
        err = np.abs(g64 - want[k])
        zero = bound[k] == 0.0
        assert not _i32(g).cpu().numpy()[zero].any(), f"{what} {k}: an entry without a term is not +0.0"
        ratio = float((err[~zero] / bound[k][~zero]).max()) if (~zero).any() else 0.0
        ce = comp_err.get(k) if comp_err else None
        vs = f", {err.max() / max(ce, 1e-300):.2f} x the fp32 composite's error {ce:.2e}" if ce is not None else ""
        print(f"{what} {k}: max abs error {err.max():.3e}, worst error / bound {ratio:.3f}{vs}")
        i = int(np.argmax(err - bound[k]))
        assert np.all(err <= bound[k]), f"{what} {k}: entry {i}: error {err.flat[i]:.3e} > bound {bound[k].flat[i]:.3e}"
        worst = max(worst, ratio)
    return worst


# ------------------------------------------------------------------------------------------------ 1. g is the logits-gradient kernel's
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
@pytest.mark.parametrize("H", [3, 64])
def test_g_is_the_logits_gradient_kernels(H, dtype_name, with_bias):
    """Every action is allowed in at most one row, so every sum over rows has one term or none: grad_bias[a] is g_{i,a} itself and
    grad_weight[a, h] the rounded product g * l_{i,h}.  On exact_inputs F.linear's logits are exact and equal the kernel's x, so g must
    be what mcbs_masked_categorical_grad writes for those logits in float32."""
    import torch
    eng = _chain4_engine()
    dev = eng.device
    dt = getattr(torch, dtype_name)
    A = eng.discrete_action_count()
    n = 64
    rng = np.random.default_rng(40 + H)
    mask = np.zeros((n, A), dtype=bool)
    mask[0, :600] = True                                 # more than the 512 logits the row pass keeps in LDS
    mask[1, 700] = True                                  # one action
    mask[2, 800:841] = True
    mask[5, A - 3:] = True                               # the last word
    mask[40, 900:1500:7] = True
    assert mask.sum(0).max() == 1
    actions = np.zeros(n, dtype=np.int64)
    actions[0], actions[1], actions[2], actions[5], actions[40] = 17, 3, 805, A - 1, 907      # row 1: not allowed, so g = -g_lp p
    actions[7] = 9                                       # a blank row
    g_lp, g_H = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    latent, weight, bias = lhr.exact_inputs(n, A, H, rng)
    c = dict(mask=mask, latent=latent, weight=weight, bias=bias, actions=actions, g_lp=g_lp, g_H=g_H)
    args = _on_device(eng, c, dt, with_bias=with_bias)
    lat, wt, b, bits, ta, tl, th = args
    logits = torch.nn.functional.linear(lat.float(), wt.float(), b.float() if with_bias else None)
    gl = eng.masked_categorical_grad(logits, bits, ta, tl, th).cpu().numpy()          # float32 [n, A]: g, zeros elsewhere
    got = eng.masked_linear_categorical_grad(*args)
    row_of = mask.argmax(0)                              # the one row that allows a (0 where none does: its g there is 0)
    g = gl[row_of, np.arange(A)]
    allowed = mask.any(0)
    assert not gl[:, ~allowed].any() and np.count_nonzero(g) >= 600
    zero = np.float32(0.0)
    np.testing.assert_array_equal(got.grad_bias.cpu().numpy().view(np.int32), (g + zero).view(np.int32))
    want_w = (g[:, None] * latent[row_of]).astype(np.float32) + zero                 # one rounding: what fmaf(g, l, +0.0) gives
    np.testing.assert_array_equal(got.grad_weight.cpu().numpy().view(np.int32), want_w.view(np.int32))
    assert not got.grad_weight.cpu().numpy().view(np.int32)[~allowed].any() and not got.grad_bias.cpu().numpy().view(np.int32)[~allowed].any()
    want_l1 = (g[700] * weight[700]).astype(np.float32) + zero
    assert g[700] == -g_lp[1]
    np.testing.assert_array_equal(got.grad_latent[1].cpu().numpy().view(np.int32), want_l1.view(np.int32))
    dead = ~lg.live_rows(mask, actions)
    assert dead.sum() == n - 5 and not _i32(got.grad_latent).cpu().numpy()[dead].any()
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. against fp64 within the bound
@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
@pytest.mark.parametrize("H", [1, 3, 64, 65, 200])
def test_against_fp64_within_the_bound(H, exact, dtype_name):
    import torch
    eng = _chain4_engine()
    A = eng.discrete_action_count()
    assert A == 1830 and eng.packed_mask_words()[0] == 58
    bf16 = dtype_name == "bfloat16"
    c, want, bound, comp_err = _reference(A, H, exact, bf16)
    got = eng.masked_linear_categorical_grad(*_on_device(eng, c, getattr(torch, dtype_name)))
    _check_bound(got, want, bound, comp_err, f"H={H} {'exact' if exact else 'general'} {dtype_name}")
    live = lg.live_rows(c["mask"], c["actions"])
    assert not live[3] and not live[9] and not live[10] and not _i32(got.grad_latent).cpu().numpy()[~live].any()
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. masked values never matter
@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_masked_values_never_matter(dtype_name):
    """NaN, +Inf and -Inf in the weight rows and the bias of actions no row allows: every output is bit for bit that of clean values."""
    import torch
    eng = _chain4_engine()
    A = eng.discrete_action_count()
    dt = getattr(torch, dtype_name)
    c = dict(lg.case(A, 64, exact=False))
    never = np.arange(A) % 7 == 3
    never[A - 1] = True
    c["mask"] = c["mask"] & ~never[None, :]
    c["actions"] = np.where(never[np.clip(c["actions"], 0, A - 1)], 0, c["actions"])
    args = _on_device(eng, c, dt)
    clean = eng.masked_linear_categorical_grad(*args)
    poison = torch.tensor([float("nan"), float("inf"), float("-inf")], dtype=dt, device=eng.device)
    idx = torch.as_tensor(np.flatnonzero(never), device=eng.device)
    wt, b = args[1].clone(), args[2].clone()
    wt[idx] = poison[(torch.arange(idx.numel() * 64, device=eng.device) % 3).view(-1, 64)]
    b[idx] = poison[torch.arange(idx.numel(), device=eng.device) % 3]
    dirty = eng.masked_linear_categorical_grad(args[0], wt, b, *args[3:])
    for k, x, y in zip(OUTS, clean, dirty):
        assert bool(torch.isfinite(y).all()), k
        assert torch.equal(_i32(x), _i32(y)), f"{k}: a value under a clear mask bit reached the output"
    assert bool(clean.grad_bias.any()) and not _i32(clean.grad_weight)[idx].any() and not _i32(clean.grad_bias)[idx].any()
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. reproducibility and invariance
def _framed(rows, cols, stride, offset, dtype, dev):
    """A [rows, cols] view at element `offset` with row stride `stride` inside a sentinel-filled buffer -> (buffer, view)."""
    import torch
    buf = torch.full((offset + rows * stride + 9,), SENTINEL, dtype=dtype, device=dev)
    return buf, buf[offset:offset + rows * stride].view(rows, stride)[:, :cols]


def _frame_untouched(buf, rows, cols, stride, offset):
    body = buf[offset:offset + rows * stride].view(rows, stride)
    return bool((buf[:offset] == SENTINEL).all()) and bool((body[:, cols:] == SENTINEL).all()) and bool((buf[offset + rows * stride:] == SENTINEL).all())


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
@pytest.mark.parametrize("H", [64, 65])
def test_reproducible_and_invariant(H, dtype_name):
    import torch
    eng = _chain4_engine()
    dev = eng.device
    A = eng.discrete_action_count()
    W, row_words = eng.packed_mask_words()
    dt = getattr(torch, dtype_name)
    c, want, bound, comp_err = _reference(A, H, False, dtype_name == "bfloat16")
    n = 64
    args = _on_device(eng, c, dt)
    lat, wt, b, bits, ta, tl, th = args
    inputs_before = [x.clone() for x in args]
    base = eng.masked_linear_categorical_grad(*args)

    def same(got, what):
        for k, x, y in zip(OUTS, base, got):
            if y is not None:
                assert torch.equal(_i32(x), _i32(y)), f"{what}: {k} differs"

    same(eng.masked_linear_categorical_grad(*args), "a second call")
    # garbage in the tail bits of word W-1 and junk words beyond W
    junk = torch.as_tensor(gr.pack(c["mask"], W + 6, garbage_tail=True), device=dev)
    same(eng.masked_linear_categorical_grad(lat, wt, b, junk, ta, tl, th), "garbage tail bits and junk words")
    # offset and strided inputs and outputs inside sentinel frames
    for off_in, off_out, pad in ((1, 3, 5), (0, 0, 4), (3, 1, 2)):
        lbuf, lat2 = _framed(n, H, H + pad, off_in, dt, dev)
        wbuf, wt2 = _framed(A, H, H + pad + 1, off_in, dt, dev)
        lat2.copy_(lat)
        wt2.copy_(wt)
        frames = [_framed(n, H, H + pad, off_out, torch.float32, dev), _framed(A, H, H + pad + 2, off_out, torch.float32, dev)]
        gb = torch.full((A + 2,), SENTINEL, device=dev)
        got = eng.masked_linear_categorical_grad(lat2, wt2, b, bits, ta, tl, th, out=(frames[0][1], frames[1][1], gb[1:A + 1]))
        same(got, f"frames {off_in}/{off_out}/{pad}")
        assert _frame_untouched(frames[0][0], n, H, H + pad, off_out) and _frame_untouched(frames[1][0], A, H, H + pad + 2, off_out)
        assert float(gb[0]) == SENTINEL and float(gb[A + 1]) == SENTINEL
        assert _frame_untouched(lbuf, n, H, H + pad, off_in) and _frame_untouched(wbuf, A, H, H + pad + 1, off_in)
    # a poisoned workspace, larger than asked for
    need = eng.masked_linear_categorical_grad_workspace(n, H)
    assert need > 0
    for fill in (0xFF, 0x7F):
        ws = torch.full((need + 64,), fill, dtype=torch.uint8, device=dev)
        same(eng.masked_linear_categorical_grad(*args, workspace=ws), f"workspace filled with {fill:#x}")
    # any subset of the outputs
    for want_k in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True), (True, False, True)):
        got = eng.masked_linear_categorical_grad(*args, want=want_k)
        assert [x is not None for x in got] == list(want_k)
        same(got, f"want={want_k}")
    for x, y in zip(args, inputs_before):
        assert torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x, y.view(torch.int16) if y.dtype == torch.bfloat16 else y), "an input was modified"
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. row blocks
def _tiled_case(A, H, n):
    c = lg.case(A, H, exact=False)
    reps = (n + 63) // 64
    return {k: np.concatenate([v] * reps)[:n] if k in ("mask", "latent", "actions", "g_lp", "g_H") else v for k, v in c.items()}


def test_row_blocks_within_the_bound():
    """2 blocks and 3 rows: the synthetic rows tiled, every action's sums cross the block boundary."""
    import torch
    eng = _chain4_engine()
    A = eng.discrete_action_count()
    n, H = 2 * ROW_BLOCK + 3, 64
    c = _tiled_case(A, H, n)
    want = lg.closed_form(**c)
    bound = lg.bounds(**c)
    got = eng.masked_linear_categorical_grad(*_on_device(eng, c, torch.float32))
    _check_bound(got, want, bound, None, f"{n} rows")
    eng.close()


def test_first_block_alone_when_the_rest_is_blank():
    """Rows from the second block on with all-zero masks add nothing: grad_weight and grad_bias are bit for bit those of the first block."""
    import torch
    eng = _chain4_engine()
    A = eng.discrete_action_count()
    n, H = 2 * ROW_BLOCK + 3, 65
    c = _tiled_case(A, H, n)
    c["mask"] = c["mask"].copy()
    c["mask"][ROW_BLOCK:] = False
    args = _on_device(eng, c, torch.bfloat16)
    full = eng.masked_linear_categorical_grad(*args)
    first = eng.masked_linear_categorical_grad(*[x[:ROW_BLOCK] if i in (0, 3, 4, 5, 6) else x for i, x in enumerate(args)])
    assert torch.equal(_i32(full.grad_weight), _i32(first.grad_weight)) and torch.equal(_i32(full.grad_bias), _i32(first.grad_bias))
    assert torch.equal(_i32(full.grad_latent[:ROW_BLOCK]), _i32(first.grad_latent)) and not _i32(full.grad_latent[ROW_BLOCK:]).any()
    assert bool(first.grad_weight.any())
    eng.close()


def test_more_rows_than_one_grid():
    """The row pass's grid covers 4 * 65 536 rows, the stride loop reaches the rest.  The 64 synthetic rows tiled: every tile of grad_latent
    repeats the first bit for bit; every full row block holds the same 8 tiles, so grad_weight / grad_bias are the first block's partial p
    added up in block order, ((p + p) + p) + ... + the partial of the last 3 tiles, bit for bit."""
    import torch
    eng = _chain4_engine()
    dev = eng.device
    A = eng.discrete_action_count()
    H = 3
    reps = 4 * 65536 // 64 + 3
    n = reps * 64
    c = lg.case(A, H, exact=False)
    a64 = _on_device(eng, c, torch.float32)
    args = [x.repeat(reps, 1) if x.dim() == 2 and i != 1 else (x.repeat(reps) if i in (4, 5, 6) else x) for i, x in enumerate(a64)]
    got = eng.masked_linear_categorical_grad(*args)
    one = eng.masked_linear_categorical_grad(*a64)
    assert bool(one.grad_latent.any())
    assert bool((_i32(got.grad_latent).view(reps, 64 * H) == _i32(one.grad_latent).view(1, 64 * H)).all()), "a tile of grad_latent differs from the first"
    head = lambda k: [x[:k] if i in (0, 3, 4, 5, 6) else x for i, x in enumerate(args)]
    p = eng.masked_linear_categorical_grad(*head(ROW_BLOCK))
    last = eng.masked_linear_categorical_grad(*head(n % ROW_BLOCK))
    assert n % ROW_BLOCK == 3 * 64
    for k in ("grad_weight", "grad_bias"):
        s = getattr(p, k).clone()
        for _ in range(n // ROW_BLOCK - 1):
            s = s + getattr(p, k)
        s = s + getattr(last, k)
        assert torch.equal(_i32(getattr(got, k)), _i32(s)), f"{k}: the block partials were not added in block order"
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. wide rows
def test_wide_rows():
    """Chain-10 @ 14 nodes: A = 19 278, 603 mask words — beyond the 512 words a wavefront caches — with allowed actions in the last words."""
    import torch
    eng = _chain10_engine(14)
    A = eng.discrete_action_count()
    W, row_words = eng.packed_mask_words()
    assert (A, W) == (19278, 603)
    n, H = 64, 16
    rng = np.random.default_rng(31)
    mask = rng.random((n, A)) < (rng.random((n, 1)) ** 3) * 0.2
    mask[0, :] = True
    mask[1, :] = False
    mask[1, (W - 1) * 32 + 3] = True                     # a single bit, in the last word
    mask[2, :] = False
    mask[4, :] = False
    mask[4, 512 * 32 - 2:] = True                        # across the end of the cache to the last action
    actions = np.array([np.flatnonzero(mask[i])[rng.integers(0, mask[i].sum())] if mask[i].any() else 0 for i in range(n)], dtype=np.int64)
    actions[3] = int(np.flatnonzero(~mask[3])[-1])       # not allowed, near the row's end
    actions[4] = A - 1
    latent, weight, bias = lg.general_inputs(n, A, H, rng)
    c = dict(mask=mask, latent=latent, weight=weight, bias=bias, actions=actions, g_lp=rng.standard_normal(n).astype(np.float32),
             g_H=rng.standard_normal(n).astype(np.float32))
    want = lg.closed_form(**c)
    bound = lg.bounds(**c)
    got = eng.masked_linear_categorical_grad(*_on_device(eng, c, torch.float32))
    _check_bound(got, want, bound, None, f"wide rows A={A}")
    assert bool(got.grad_bias[A - 1] != 0)
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. autograd end to end
def test_autograd_end_to_end():
    """The PPO loss through evaluate_masked_from_latent(differentiable=True): the forward's numbers bit for bit, the three .grad within the
    bound of the closed form fed the incoming gradients autograd handed the node; next to it the composite path on the device, F.linear +
    evaluate_masked(differentiable=True), for the printed comparison."""
    import inspect
    import torch
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.samples import chainpattern
    from marlon_amd.vecenv import MarlonVecEnv
    from marlon_amd.wrappers import AttackerVecEnv
    E, T, F = 64, 4, 32
    env = AttackerVecEnv(chainpattern.new_environment(4), E, maximum_node_count=6, maximum_total_credentials=6,
                         attacker_goal=ce.AttackerGoal(own_atleast_percent=1.0), max_timesteps=50, discrete=True, materialize_masks=False)
    eng = env.engine
    dev = eng.device
    A = env.discrete_n
    W, row_words = eng.packed_mask_words()
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
            r = env.sample_masked_from_latent(feats[t], head.weight, head.bias, seed=3, step=t)
            acts[t], lps[t] = r.actions, r.log_prob
            env.step(r.actions)
    n = T * E
    bits, actions = buf.view(n, row_words), acts.view(n)
    old_lp = lps.view(n) + 0.1 * torch.randn(n, generator=g, device=dev)
    adv = torch.randn(n, generator=g, device=dev)
    mask = env.unpack_action_mask(bits).cpu().numpy()

    def loss_of(lp, ent):
        return -(adv * torch.exp(lp - old_lp)).mean() - 0.01 * ent.mean()

    calls = []
    inner = eng.masked_linear_categorical_grad

    def recording(*a, **kw):
        calls.append((a, kw))
        return inner(*a, **kw)

    eng.masked_linear_categorical_grad = recording

    def fused(dt, only_latent=False, use_entropy=True):
        lat = feats.view(n, F).to(dt).clone().requires_grad_(True)
        w = head.weight.detach().to(dt).clone().requires_grad_(not only_latent)
        b = head.bias.detach().to(dt).clone().requires_grad_(not only_latent)
        r = env.evaluate_masked_from_latent(bits, lat, w, b, actions, differentiable=True)
        incoming = {}
        r.log_prob.register_hook(lambda gr_: incoming.__setitem__("g_lp", gr_.clone()))
        if use_entropy:
            r.entropy.register_hook(lambda gr_: incoming.__setitem__("g_H", gr_.clone()))
        loss_of(r.log_prob, r.entropy if use_entropy else torch.zeros(n, device=dev)).backward()
        return lat, w, b, r, incoming

    # ---- float32: forward bit for bit, gradients within the bound
    lat, w, b, r, incoming = fused(torch.float32)
    plain = env.evaluate_masked_from_latent(bits, lat.detach(), w.detach(), b.detach(), actions)
    assert r.log_prob.requires_grad and r.entropy.requires_grad and not r.n_allowed.requires_grad and not plain.log_prob.requires_grad
    for x, y in zip(r[1:], plain[1:]):
        assert torch.equal(x.detach().view(torch.int32), y.view(torch.int32)), "differentiable=True changes the forward's numbers"
    assert torch.equal(plain.log_prob.view(torch.int32), lps.view(n).view(torch.int32)), "the update does not see the rollout's log_prob bit for bit"
    c = dict(mask=mask, latent=lat.detach().cpu().numpy(), weight=w.detach().cpu().numpy(), bias=b.detach().cpu().numpy(),
             actions=actions.cpu().numpy(), g_lp=incoming["g_lp"].cpu().numpy(), g_H=incoming["g_H"].cpu().numpy())
    want, bound = lg.closed_form(**c), lg.bounds(**c)
    # the composite path on the device, for the comparison
    lat_c, w_c, b_c = (x.detach().clone().requires_grad_(True) for x in (lat, w, b))
    rc = env.evaluate_masked(bits, torch.nn.functional.linear(lat_c, w_c, b_c), actions, differentiable=True)
    loss_of(rc.log_prob, rc.entropy).backward()
    comp_err = {k: float(np.abs(x.grad.double().cpu().numpy() - want[k]).max()) for k, x in zip(OUTS, (lat_c, w_c, b_c))}
    _check_bound((lat.grad, w.grad, b.grad), want, bound, comp_err, "end to end float32 (composite: F.linear + evaluate_masked on the device)")
    assert calls[-1][1]["want"] == (True, True, True)

    # ---- an unused entropy arrives as None
    lat1, w1, b1, _, inc1 = fused(torch.float32, use_entropy=False)
    a, kw = calls[-1]
    assert a[5] is not None and a[6] is None and "g_H" not in inc1
    assert bool(torch.isfinite(w1.grad).all()) and bool(w1.grad.any())

    # ---- requires_grad on the latent alone: no action pass, the same latent.grad
    lat2, w2, b2, _, _ = fused(torch.float32, only_latent=True)
    assert calls[-1][1]["want"] == (True, False, False)
    assert w2.grad is None and b2.grad is None
    assert torch.equal(lat2.grad.view(torch.int32), lat.grad.view(torch.int32))

    # ---- bfloat16 parameters get bfloat16 gradients: the float32 result rounded once
    lat3, w3, b3, r3, inc3 = fused(torch.bfloat16)
    assert lat3.grad.dtype == w3.grad.dtype == b3.grad.dtype == torch.bfloat16
    c3 = dict(mask=mask, latent=lat3.detach().float().cpu().numpy(), weight=w3.detach().float().cpu().numpy(), bias=b3.detach().float().cpu().numpy(),
              actions=actions.cpu().numpy(), g_lp=inc3["g_lp"].float().cpu().numpy(), g_H=inc3["g_H"].float().cpu().numpy())
    want3, bound3 = lg.closed_form(**c3), lg.bounds(**c3)
    for k, x in zip(OUTS, (lat3, w3, b3)):
        err = np.abs(x.grad.double().cpu().numpy() - want3[k])
        tol = bound3[k] * (1.0 + 2.0 ** -8) + 2.0 ** -8 * np.abs(want3[k]) + 1e-40      # one rounding to bfloat16's 8 significant bits
        assert np.all(err <= tol), f"bfloat16 {k}: {err.max():.3e}"
        assert not x.grad.view(torch.int16).cpu().numpy()[bound3[k] == 0.0].any()

    # ---- the surface
    del eng.masked_linear_categorical_grad
    with pytest.raises(ValueError):
        env.evaluate_masked_from_latent(bits, lat.detach(), w.detach(), b.detach(), actions, differentiable=True, out=(None, None, None, None))
    assert "differentiable" in inspect.signature(MarlonVecEnv.evaluate_masked_from_latent).parameters
    assert "differentiable" in inspect.signature(AttackerVecEnv.evaluate_masked_from_latent).parameters
    ev = eng.masked_linear_evaluate(lat.detach().requires_grad_(True), w.detach(), None, bits, actions)      # no bias
    ev.entropy.sum().backward()
    env.close()


# ------------------------------------------------------------------------------------------------ 8. refusals, workspace, n_rows == 0
def test_c_abi_refusals_and_empty_call():
    """Every MCBS_EINVAL (-1) case through ctypes; a refused call writes nothing; n_rows == 0 writes +0.0 to grad_weight / grad_bias."""
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
    acts = torch.zeros(n, dtype=torch.int64, device=dev)
    g_lp = torch.ones(n, device=dev)
    gl = torch.full((n, H), SENTINEL, device=dev)
    gw = torch.full((A, H), SENTINEL, device=dev)
    gb = torch.full((A,), SENTINEL, device=dev)
    need = lib.mcbs_masked_linear_categorical_grad_workspace(eng._h, n, H)
    assert need == eng.masked_linear_categorical_grad_workspace(n, H) and need >= 32 * n + ROW_BLOCK // ROW_BLOCK * W * 32 * (H + 1) * 4
    assert lib.mcbs_masked_linear_categorical_grad_workspace(eng._h, 0, H) == 0
    assert lib.mcbs_masked_linear_categorical_grad_workspace(eng._h, n, 0) == 0 and lib.mcbs_masked_linear_categorical_grad_workspace(eng._h, n, 513) == 0
    assert lib.mcbs_masked_linear_categorical_grad_workspace(eng._h, ROW_BLOCK + 1, H) > lib.mcbs_masked_linear_categorical_grad_workspace(eng._h, ROW_BLOCK, H) + 32
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)

    def call(bits_ptr=bits.data_ptr(), words=row_words, rows=n, lat=latent.data_ptr(), ls=H, wt=weight.data_ptr(), wst=H, b=bias.data_ptr(), h=H, dtype=0,
             a=acts.data_ptr(), o_l=gl.data_ptr(), o_ls=H, o_w=gw.data_ptr(), o_ws=H, o_b=gb.data_ptr(), wsp=ws.data_ptr(), wsb=need):
        return lib.mcbs_masked_linear_categorical_grad(eng._h, bits_ptr, words, rows, lat, ls, wt, wst, b, h, dtype, a, g_lp.data_ptr(), None,
                                                       o_l, o_ls, o_w, o_ws, o_b, wsp, wsb, None)

    def err():
        return lib.mcbs_last_error().decode()

    for kw, word in ((dict(h=0), "H 0"), (dict(h=513, ls=513, wst=513, o_ls=513, o_ws=513), "H 513"), (dict(ls=H - 1), "latent_row_stride"),
                     (dict(wst=H - 1), "weight_row_stride"), (dict(o_ls=H - 1), "grad_latent_row_stride"), (dict(o_ws=H - 1), "grad_weight_row_stride"),
                     (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"), (dict(lat=None), "must not be NULL"), (dict(wt=None), "must not be NULL"),
                     (dict(bits_ptr=None), "must not be NULL"), (dict(a=None), "must not be NULL"), (dict(words=W - 1), "bits_row_words"),
                     (dict(o_l=None, o_w=None, o_b=None), "all NULL"), (dict(wsp=None), "workspace"), (dict(wsb=need - 1), "workspace"),
                     (dict(o_l=latent.data_ptr()), "overlaps"), (dict(o_w=weight.data_ptr()), "overlaps"), (dict(o_b=bias.data_ptr()), "overlaps"),
                     (dict(o_b=gw.data_ptr() + 4), "overlaps"), (dict(o_l=ws.data_ptr()), "overlaps"), (dict(o_b=g_lp.data_ptr()), "overlaps"),
                     (dict(wsp=bits.data_ptr()), "overlaps")):
        assert call(**kw) == -1 and word in err(), (kw, err())
    assert lib.mcbs_masked_linear_categorical_grad(None, None, 0, 0, None, 0, None, 0, None, 0, 0, None, None, None, None, 0, None, 0, None, None, 0, None) == -1
    torch.cuda.synchronize()
    assert bool((gl == SENTINEL).all()) and bool((gw == SENTINEL).all()) and bool((gb == SENTINEL).all()), "a refused call wrote its outputs"
    # n_rows == 0: grad_weight and grad_bias are cleared, grad_latent has no rows; no workspace needed
    assert call(rows=0, wsp=None, wsb=0) == 0
    torch.cuda.synchronize()
    assert not gw.view(torch.int32).any() and not gb.view(torch.int32).any() and bool((gl == SENTINEL).all())
    # the accepted call: a zero layer, every second action allowed, action 0 chosen, g_lp = 1: g = [a == 0] - 1 / K
    assert call() == 0
    torch.cuda.synchronize()
    K = (A + 1) // 2
    assert not gl.view(torch.int32).any() and not gw.view(torch.int32).any()
    gbn = gb.cpu().numpy()
    assert not gbn[1::2].any() and abs(gbn[0] - n * (1.0 - 1.0 / K)) < 1e-3 and np.allclose(gbn[2::2], -n / K, rtol=1e-5)
    eng.close()


def test_python_refusals_and_workspace_size():
    import torch
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
    ones = torch.ones(n, device=dev)
    f = eng.masked_linear_categorical_grad
    ok = f(latent, weight, bias, bits, acts, ones, ones)
    assert [tuple(x.shape) for x in ok] == [(n, H), (A, H), (A,)] and all(x.dtype == torch.float32 for x in ok)
    for bad_call in (
        lambda: f(latent.cpu(), weight, bias, bits, acts),
        lambda: f(latent, weight.bfloat16(), bias, bits, acts),
        lambda: f(latent.double(), weight.double(), bias.double(), bits, acts),
        lambda: f(latent, weight[:A - 1], bias, bits, acts),
        lambda: f(latent, weight[:, :H - 1], bias, bits, acts),
        lambda: f(latent, weight, bias[:A - 1], bits, acts),
        lambda: f(latent[:32], weight, bias, bits, acts),
        lambda: f(latent.t().contiguous().t(), weight, bias, bits, acts),
        lambda: f(torch.zeros((n, 513), device=dev), torch.zeros((A, 513), device=dev), bias, bits, acts),
        lambda: f(latent, weight, bias, None, acts),
        lambda: f(latent, weight, bias, bits.long(), acts),
        lambda: f(latent, weight, bias, bits[:, :W - 1], acts),
        lambda: f(latent, weight, bias, bits, acts.int()),
        lambda: f(latent, weight, bias, bits, acts[:10]),
        lambda: f(latent, weight, bias, bits, acts, ones.double()),
        lambda: f(latent, weight, bias, bits, acts, ones, ones[:3]),
        lambda: f(latent, weight, bias, bits, acts, out=(None, None)),
        lambda: f(latent, weight, bias, bits, acts, out=(torch.zeros((n, H), dtype=torch.bfloat16, device=dev), None, None)),
        lambda: f(latent, weight, bias, bits, acts, out=(torch.zeros((n, H - 1), device=dev), None, None)),
        lambda: f(latent, weight, bias, bits, acts, out=(None, torch.zeros((A - 1, H), device=dev), None)),
        lambda: f(latent, weight, bias, bits, acts, out=(None, None, torch.zeros(2 * A, device=dev)[::2])),
        lambda: f(latent, weight, bias, bits, acts, want=(False, False, False)),
        lambda: f(latent, weight, bias, bits, acts, want=(True, True)),
        lambda: f(latent, weight, bias, bits, acts, workspace=torch.zeros(16, dtype=torch.uint8, device=dev)),
        lambda: f(latent, weight, bias, bits, acts, workspace=torch.zeros(1 << 22, device=dev)),
    ):
        with pytest.raises(ValueError):
            bad_call()
    from marlon_amd import engine
    with pytest.raises(engine.McbsError, match="overlaps"):
        f(latent, weight, bias, bits, acts, out=(latent, None, None))
    e0 = f(latent[:0], weight, bias, bits[:0], acts[:0])
    assert e0.grad_latent.shape == (0, H) and not e0.grad_weight.view(torch.int32).any() and not e0.grad_bias.view(torch.int32).any()
    eng.close()
    # the headline minibatch: 16 384 rows of Chain-10's 14 172 actions at H = 64 need less than a quarter of one float32 [n, A] tensor
    big = _chain10_engine(12)
    assert big.discrete_action_count() == 14172
    need = big.masked_linear_categorical_grad_workspace(16384, 64)
    print(f"workspace for 16 384 x 14 172 at H = 64: {need / 1e6:.1f} MB")
    assert 0 < need < 232_000_000 and need < 16384 * 14172 * 4 // 4
    big.close()
