"""mcbs_multicategorical_grad (the backward pass of the MultiDiscrete head, include/mcbs.h) against the fp64 closed form of
tests/multicategorical_ref.py, and against torch's fp32 autograd through split -> Categorical -> log_prob.sum / entropy.sum for the bound.

Error bound (the rule of tests/test_gpu_categorical_grad.py::_within): the kernel's largest absolute error against fp64 may not exceed
4 x the largest error of torch's fp32 CPU autograd composite against fp64 on the same inputs (taken on logits.float()), plus one ulp of
the value in the output dtype (float32, or bfloat16 for bfloat16 logits).  A float32 restatement of the header's order on the CPU stays at
<= 0.20 of that bound for every shape here.  Measured on the MI355X: see DESIGN.md section 7."""
import numpy as np
import pytest

from tests import multicategorical_ref as mr

pytestmark = pytest.mark.gpu

NAMES = list(mr.NVECS)
DTYPES = ["float32", "bfloat16"]
N_ROWS = (1, 65, 300)


def _inputs(name, dtype_name, n):
    import torch
    nvec = mr.NVECS[name]
    rng = np.random.default_rng(77 + 1000 * NAMES.index(name) + DTYPES.index(dtype_name))
    values = torch.as_tensor((rng.standard_normal((n, sum(nvec))) * 4.0).astype(np.float32)).to(getattr(torch, dtype_name))
    actions = np.stack([rng.integers(0, w, n) for w in nvec], axis=1).astype(np.int64)
    return nvec, values, actions, rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_gradient_against_the_closed_form(name, dtype_name):
    import torch
    eng = mr.shared_engine()
    dev = eng.device
    n = 130 if name == "wider_than_lds" else max(N_ROWS)
    rows = (1, 65, n)
    nvec, values, actions, g_lp, g_H = _inputs(name, dtype_name, n)
    A, bf16 = sum(nvec), dtype_name == "bfloat16"
    actions[7, 0] = -1                                   # rows with a component outside its range: +0.0 throughout
    actions[66, len(nvec) - 1] = nvec[-1]
    inside = np.ones(n, dtype=bool)
    inside[[7, 66]] = False
    x32 = values.float().numpy()
    ref = mr.MultiCategoricalRef(nvec, x32)
    logits = values.to(dev)
    before = logits.clone()
    ta, tl, th = (torch.as_tensor(x, device=dev) for x in (actions, g_lp, g_H))
    safe = np.where(ref.in_range(actions), actions, 0)
    what = f"{name} {dtype_name}"
    sel = np.broadcast_to(inside[:, None], (n, A))
    first = {}
    for tag, a, b in (("both", g_lp, g_H), ("log_prob only", g_lp, None), ("entropy only", None, g_H)):
        got = eng.multicategorical_grad(logits, nvec, ta, None if a is None else tl, None if b is None else th)
        assert got.shape == (n, A) and got.dtype == logits.dtype
        want = ref.grad(actions, a, b)
        comp = mr.composite(nvec, x32, safe, torch.float32, a, b)[2]
        mr.within(got.float().cpu().numpy(), want, comp, f"{what} gradient ({tag})", sel=sel, bf16=bf16)
        assert not bool(mr.bits_of(got)[torch.as_tensor(~inside)].any()), f"{what}: a row with a component out of range is not +0.0"
        ones = [int(ref.off[d]) for d, w in enumerate(nvec) if w == 1]
        assert not bool(mr.bits_of(got)[:, ones].any()), f"{what}: a dimension of one choice has a gradient"
        first[tag] = got
    zeros = torch.zeros(n, device=dev)
    assert torch.equal(mr.bits_of(eng.multicategorical_grad(logits, nvec, ta, tl, zeros)), mr.bits_of(first["log_prob only"]))
    assert not bool(mr.bits_of(eng.multicategorical_grad(logits, nvec, ta)).any()), f"{what}: no incoming gradient must give +0.0 everywhere"

    # bitwise: two calls, fewer rows, a sentinel frame (stride A + 5, one element in), dense rows off a 16-byte boundary
    got = first["both"]
    assert torch.equal(mr.bits_of(eng.multicategorical_grad(logits, nvec, ta, tl, th)), mr.bits_of(got)), f"{what}: two calls differ"
    for k in rows[:-1]:
        part = eng.multicategorical_grad(logits[:k], nvec, ta[:k], tl[:k], th[:k])
        assert torch.equal(mr.bits_of(part), mr.bits_of(got[:k])), f"{what}: the first {k} rows differ"
    k = 65
    buf, out = mr.framed(k, A, A + 5, 1, logits.dtype, dev)
    ret = eng.multicategorical_grad(logits[:k], nvec, ta[:k], tl[:k], th[:k], out=out)
    assert ret.data_ptr() == out.data_ptr()
    assert mr.frame_untouched(buf, k, A, A + 5, 1), f"{what}: an element outside [0, A) of a row was written"
    assert torch.equal(mr.bits_of(out.contiguous()), mr.bits_of(got[:k])), f"{what}: the framed call differs from the dense one"
    lbuf, lview = mr.framed(k, A, A + 3, 1, logits.dtype, dev)
    lview.copy_(logits[:k])
    assert torch.equal(mr.bits_of(eng.multicategorical_grad(lview, nvec, ta[:k], tl[:k], th[:k])), mr.bits_of(got[:k])), f"{what}: framed logits"
    for offset in (1, 3):
        flat = torch.full((offset + k * A + 9,), mr.SENTINEL, dtype=logits.dtype, device=dev)
        dense = flat[offset:offset + k * A].view(k, A)
        eng.multicategorical_grad(logits[:k], nvec, ta[:k], tl[:k], th[:k], out=dense)
        assert torch.equal(mr.bits_of(dense), mr.bits_of(got[:k])), f"{what}: dense output at element {offset}"
        assert bool((flat[:offset] == mr.SENTINEL).all()) and bool((flat[offset + k * A:] == mr.SENTINEL).all()), f"{what}: written past the rows"
    assert torch.equal(mr.bits_of(logits), mr.bits_of(before)), f"{what}: logits were modified"


def test_infinite_logits_and_underflow():
    """-inf logits next to a finite one and an exp that underflows: the product term is exactly 0 there, the gradient finite."""
    import torch
    eng = mr.shared_engine()
    nvec = [3, 12, 5]
    x = np.random.default_rng(5).standard_normal((4, 20)).astype(np.float32)
    x[0, 3:15] = -np.inf
    x[0, 9] = 1.0
    x[1, 3:15] = 0.0
    x[1, 4] = 120.0
    x[2, 0] = -np.inf
    actions = np.array([[0, 6, 1], [1, 1, 0], [1, 3, 4], [2, 11, 2]], dtype=np.int64)
    g_lp, g_H = np.array([1.0, -2.0, 0.5, 3.0], dtype=np.float32), np.array([0.25, 1.0, -1.0, 2.0], dtype=np.float32)
    ref = mr.MultiCategoricalRef(nvec, x)
    dev = eng.device
    got = eng.multicategorical_grad(torch.as_tensor(x, device=dev), nvec, torch.as_tensor(actions, device=dev), torch.as_tensor(g_lp, device=dev),
                                    torch.as_tensor(g_H, device=dev))
    want = ref.grad(actions, g_lp, g_H)
    comp = mr.composite(nvec, np.maximum(x, -1e30), actions, torch.float32, g_lp, g_H)[2]     # (autograd through -inf logits gives NaN)
    mr.within(got.cpu().numpy(), want, comp, "infinite logits", sel=np.isfinite(x))
    g = got.cpu()
    assert not bool(g.view(torch.int32)[0, [3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14]].any()) and not bool(g.view(torch.int32)[2, 0].any())
    assert not bool(g.view(torch.int32)[1, [3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14]].any()), "an exp that underflows leaves a term"


def test_refusals():
    import ctypes as C

    import torch
    from marlon_amd import engine
    eng = mr.shared_engine()
    dev = eng.device
    nvec, A, n = [5, 5], 10, 8
    logits = torch.randn((n, A), device=dev)
    acts = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    g = torch.ones(n, device=dev)
    out = torch.empty((n, A), device=dev)
    ok = eng.multicategorical_grad(logits, nvec, acts, g, g, out=out)
    assert ok is out and bool(torch.isfinite(out).all()) and bool(out.any())
    nv = (C.c_uint32 * 17)(*([5, 5] + [1] * 15))

    def raw(nvec_p=nv, D=2, rows=n, logits_p=logits.data_ptr(), dtype=0, stride=A, acts_p=acts.data_ptr(), out_p=out.data_ptr(), out_stride=A):
        return eng.lib.mcbs_multicategorical_grad(eng._h, nvec_p, D, rows, logits_p, dtype, stride, acts_p, g.data_ptr(), None, out_p, out_stride, None)

    torch.cuda.synchronize()
    assert raw() == 0
    for what, kw, word in (("nvec NULL", dict(nvec_p=None), b"nvec"), ("D = 0", dict(D=0), b"n_dims"), ("D = 17", dict(D=17), b"n_dims"),
                           ("nvec entry 0", dict(nvec_p=(C.c_uint32 * 2)(0, 5)), b"nvec[0]"), ("logits NULL", dict(logits_p=None), b"logits"),
                           ("actions NULL", dict(acts_p=None), b"actions"), ("grad_logits NULL", dict(out_p=None), b"grad_logits"),
                           ("dtype", dict(dtype=2), b"dtype"), ("row_stride", dict(stride=A - 1), b"row_stride"),
                           ("grad_row_stride", dict(out_stride=A - 1), b"grad_row_stride"), ("in place", dict(out_p=logits.data_ptr()), b"overlap"),
                           ("overlap", dict(out_p=logits.data_ptr() + 4 * (A - 1)), b"overlap")):
        rc = raw(**kw)
        assert rc == -1, f"{what}: {rc}"
        assert word in eng.lib.mcbs_last_error(), (what, eng.lib.mcbs_last_error())
    assert raw(rows=0, logits_p=None, acts_p=None, out_p=None) == 0
    torch.cuda.synchronize()
    # rows of the same stride interleaved in one buffer do not overlap
    both = torch.zeros((n, 2 * A), device=dev)
    both[:, :A] = logits
    eng.multicategorical_grad(both[:, :A], nvec, acts, g, g, out=both[:, A:])
    expect = eng.multicategorical_grad(logits, nvec, acts, g, g)
    assert torch.equal(both[:, A:].contiguous().view(torch.int32), expect.view(torch.int32)) and torch.equal(both[:, :A], logits)
    with pytest.raises(engine.McbsError, match=r"\(-1\).*overlap"):
        eng.multicategorical_grad(both[:, :A], nvec, acts, g, g, out=both[:, 1:A + 1])
    with pytest.raises(engine.McbsError, match=r"\(-1\).*overlap"):
        eng.multicategorical_grad(logits, nvec, acts, g, g, out=logits)
    for bad_call in (
        lambda: eng.multicategorical_grad(None, nvec, acts, g, g),
        lambda: eng.multicategorical_grad(logits.double(), nvec, acts, g, g),
        lambda: eng.multicategorical_grad(logits[:, :A - 1], nvec, acts, g, g),
        lambda: eng.multicategorical_grad(logits.cpu(), nvec, acts, g, g),
        lambda: eng.multicategorical_grad(logits, nvec, None, g, g),
        lambda: eng.multicategorical_grad(logits, nvec, acts.int(), g, g),
        lambda: eng.multicategorical_grad(logits, nvec, acts[:5], g, g),
        lambda: eng.multicategorical_grad(logits, nvec, acts[:, 0], g, g),
        lambda: eng.multicategorical_grad(logits, nvec, acts, g.double(), g),
        lambda: eng.multicategorical_grad(logits, nvec, acts, g, g[:5]),
        lambda: eng.multicategorical_grad(logits, nvec, acts, g, g, out=out.bfloat16()),
        lambda: eng.multicategorical_grad(logits, nvec, acts, g, g, out=out[:, :A - 1]),
        lambda: eng.multicategorical_grad(logits, nvec, acts, g, g, out=out[:4]),
    ):
        with pytest.raises(ValueError):
            bad_call()
    empty = eng.multicategorical_grad(logits[:0], nvec, acts[:0], g[:0], g[:0])
    assert empty.shape == (0, A) and empty.dtype == logits.dtype


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_differentiable_evaluate(dtype_name):
    """evaluate_actions(differentiable=True): (w1 * log_prob + w2 * entropy).sum().backward() fills logits.grad with exactly what
    multicategorical_grad returns for g_lp = w1, g_H = w2; the forward values are those of the plain call, bit for bit."""
    import torch
    from tests.test_gpu_multicategorical import _toyctf_pair
    att, dfd = _toyctf_pair(64)
    dev = att.engine.device
    nvec = [int(v) for v in dfd.nvec]
    n = 150                                              # any n stored rows
    g = torch.Generator(device=dev).manual_seed(3)
    logits = (torch.randn((n, sum(nvec)), generator=g, device=dev) * 3.0).to(getattr(torch, dtype_name)).requires_grad_(True)
    actions = dfd.engine.multicategorical(logits.detach(), nvec, seed=1, step=2).actions
    w1, w2 = torch.randn(n, generator=g, device=dev), torch.randn(n, generator=g, device=dev)
    r = dfd.evaluate_actions(logits, actions, differentiable=True)
    plain = dfd.evaluate_actions(logits.detach(), actions)
    assert r.log_prob.requires_grad and r.entropy.requires_grad and not plain.log_prob.requires_grad
    for a, b in zip(r[1:], plain[1:]):
        assert torch.equal(a.detach().view(torch.int32), b.view(torch.int32)), "differentiable=True changes the forward's numbers"
    (w1 * r.log_prob + w2 * r.entropy).sum().backward()
    want = dfd.engine.multicategorical_grad(logits.detach(), nvec, actions, w1, w2)
    assert torch.equal(mr.bits_of(logits.grad), mr.bits_of(want))
    # a loss of one output alone backpropagates (the other's incoming gradient is absent)
    for pick, (a, b) in ((1, (w1, None)), (2, (None, w2))):
        logits.grad = None
        (dfd.evaluate_actions(logits, actions, differentiable=True)[pick] * (w1 if pick == 1 else w2)).sum().backward()
        assert torch.equal(mr.bits_of(logits.grad), mr.bits_of(dfd.engine.multicategorical_grad(logits.detach(), nvec, actions, a, b)))
    with pytest.raises(ValueError):
        dfd.evaluate_actions(logits, actions, differentiable=True, out=(None, None, None))
    # the attacker's MultiDiscrete head goes the same way
    la = torch.randn((n, int(att.nvec.sum())), generator=g, device=dev, requires_grad=True)
    aa = att.engine.multicategorical(la.detach(), att.nvec, seed=1, step=2).actions
    att.evaluate_actions(la, aa, differentiable=True).log_prob.sum().backward()
    assert torch.equal(la.grad.view(torch.int32), att.engine.multicategorical_grad(la.detach(), att.nvec, aa, torch.ones(n, device=dev)).view(torch.int32))
    att.close()
