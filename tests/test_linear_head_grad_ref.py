"""tests/linear_head_grad_ref.py — the fp64 closed form and the error bound the GPU tests of mcbs_masked_linear_categorical_grad use —
pinned to torch on the CPU: the closed form against fp64 autograd through F.linear -> where -> Categorical, and the fp32 composite inside
the bound on every input set of the GPU tests (the 64 synthetic rows at A = 1830, H in {1, 3, 64, 65, 200}, exact and general layers,
fp32 and bf16-rounded values).

fp64 tolerance: that of tests/test_categorical_grad_ref.py for an entry of g, A * 2^-53 * scale, plus the bound's own sensitivity term
for the fp64 rounding of the logits (torch's GEMM and NumPy's sum in different orders), carried through the three sums with their fp64
rounding (gamma in fp64)."""
import numpy as np
import pytest

from tests import linear_head_grad_ref as lg
from tests import linear_head_ref as lhr

A = 1830
HS = (1, 3, 64, 65, 200)
OUTS = ("grad_latent", "grad_weight", "grad_bias")


def test_case_covers_the_listed_rows():
    c = lg.case(A, 64, exact=False)
    K = c["mask"].sum(1)
    assert K[3] == 0 and K[0] == 1 and K[2] == A and (K > 512).sum() >= 3            # blank, one action, all, beyond the kernel's stash
    assert c["actions"][9] == -1 and c["actions"][10] == A and not c["mask"][1, c["actions"][1]]
    live = lg.live_rows(c["mask"], c["actions"])
    assert not live[3] and not live[9] and not live[10] and live.sum() == 53           # (some random rows are blank too)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
@pytest.mark.parametrize("H", HS)
def test_closed_form_is_fp64_autograd(H, exact):
    import torch
    c = lg.case(A, H, exact)
    want = lg.composite_grads(dtype=torch.float64, **c)
    got = lg.closed_form(**c)
    mask, g_lp, g_H = c["mask"], c["g_lp"].astype(np.float64), c["g_H"].astype(np.float64)
    scale = max(np.abs(g_lp).max(), np.abs(g_H).max() * 2.0 * np.log(A))
    u64 = 2.0 ** -53
    delta64 = lhr.dot_bound(c["latent"], c["weight"], c["bias"], mask) * 2.0 ** -29       # the fp32 bound's gamma is (H + 1) 2^-24
    p, q, ent = lg._row_terms(mask, got["x"], g_lp, g_H)
    t = np.where(mask, A * u64 * scale + 2.1 * delta64[:, None] * (np.abs(q) + p * np.abs(g_H)[:, None] * (ent[:, None] + 2.0)), 0.0)
    L, Wt, absg = np.abs(lhr.to64(c["latent"])), np.abs(lhr.to64(c["weight"])), np.abs(got["g"])
    tol = dict(grad_latent=t @ Wt + (A + 1) * u64 * (absg @ Wt), grad_weight=t.T @ L + 65 * u64 * (absg.T @ L),
               grad_bias=t.sum(0) + 65 * u64 * absg.sum(0))
    for k in OUTS:
        err = np.abs(got[k] - want[k])
        print(f"H={H} {'exact' if exact else 'general'} {k}: closed form against fp64 autograd: max abs error {err.max():.3e}")
        assert np.all(err <= tol[k]), k


@pytest.mark.parametrize("bf16", [False, True], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
@pytest.mark.parametrize("H", HS)
def test_fp32_composite_stays_within_the_bound(H, exact, bf16):
    """The bound holds for any summation order, so torch's own fp32 path has to sit inside it; prints the worst error / bound."""
    import torch
    c = lg.case(A, H, exact, bf16=bf16)
    want = lg.closed_form(**c)
    bound = lg.bounds(exact=exact, **c)
    comp = lg.composite_grads(dtype=torch.float32, **c)
    for k in OUTS:
        err = np.abs(comp[k] - want[k])
        zero = bound[k] == 0.0
        assert not comp[k][zero].any(), f"{k}: the fp32 composite is not 0 where the bound is"
        ratio = float((err[~zero] / bound[k][~zero]).max())
        print(f"H={H} {'exact' if exact else 'general'} {'bf16' if bf16 else 'fp32'} {k}: fp32 composite worst error / bound {ratio:.3f} "
              f"(E_g {bound['E_g']:.2e})")
        assert ratio <= 1.0, k


def test_bound_is_zero_exactly_where_nothing_contributes():
    c = lg.case(A, 3, exact=True)
    bound = lg.bounds(exact=True, **c)
    live = lg.live_rows(c["mask"], c["actions"])
    assert np.array_equal(bound["grad_latent"].any(axis=1), live)
    allowed = (c["mask"] & live[:, None]).any(axis=0)
    assert np.array_equal(bound["grad_bias"] > 0.0, allowed)
    assert not bound["grad_weight"][~allowed].any()
