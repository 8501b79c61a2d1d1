"""tests/categorical_grad_ref.py — the fp64 closed form the GPU tests of mcbs_masked_categorical_grad compare against — pinned to
torch's fp64 autograd through `Categorical(logits=where(mask, logits, -1e8))`: log_prob(actions) and the entropy with the masked terms
zeroed, fed separate random incoming gradients, on the 64 synthetic rows at A = 1830 (the 4-node chain's action count).

Bound: the closed form and autograd both work in fp64 on sums of at most A terms of magnitude <= max(|g_lp|, |g_H| * |log p + H|), so
they may differ by A * 2^-53 times that scale (2e-13 * scale); measured: 1.8e-15."""
import numpy as np
import pytest

from tests import categorical_grad_ref as gr

A = 1830


@pytest.fixture(scope="module")
def inputs():
    return gr.synthetic_inputs(A)


def test_inputs_cover_the_listed_cases(inputs):
    mask, logits, actions, g_lp, g_H = inputs
    assert mask.shape == (64, A) and logits.dtype == np.float32
    K = mask.sum(1)
    assert K[3] == 0 and K[2] == A and K[0] == 1 and K[1] == 1
    on = mask[np.arange(64), actions]
    assert on[0] and not on[1] and not on[3] and np.array_equal(on[4:], K[4:] > 0)      # (a random row may be blank too)
    assert tuple(logits[7, 3:6]) == (80.0, 0.0, -80.0) and len(set(logits[8, [31, 32, 63, 64, A - 2]])) == 1
    assert np.all(g_lp != 0) and np.all(g_H != 0)


def test_closed_form_is_fp64_autograd(inputs):
    import torch
    mask, logits, actions, g_lp, g_H = inputs
    want = gr.composite_grad(mask, logits, actions, g_lp, g_H, torch.float64)
    got = gr.closed_form(mask, logits, actions, g_lp, g_H)
    scale = max(np.abs(g_lp).max(), np.abs(g_H).max() * 2.0 * np.log(A))
    err = np.abs(got - want).max()
    print(f"closed form against fp64 autograd: max abs error {err:.3e}")
    assert err <= A * 2.0 ** -53 * scale
    # each output alone (the other incoming gradient absent = zeros)
    z = np.zeros_like(g_lp)
    assert np.abs(gr.closed_form(mask, logits, actions, g_lp, None) - gr.composite_grad(mask, logits, actions, g_lp, z, torch.float64)).max() <= A * 2.0 ** -53 * scale
    assert np.abs(gr.closed_form(mask, logits, actions, None, g_H) - gr.composite_grad(mask, logits, actions, z, g_H, torch.float64)).max() <= A * 2.0 ** -53 * scale
    assert not gr.closed_form(mask, logits, actions).any()


def test_autograd_is_exactly_zero_where_the_closed_form_says_so(inputs):
    """Masked entries, the blank row and a chosen action that is not allowed get exactly 0 from torch, in fp64 and in fp32; a chosen
    action that is not allowed still pushes the allowed ones down."""
    import torch
    mask, logits, actions, g_lp, g_H = inputs
    for dt in (torch.float64, torch.float32):
        g = gr.composite_grad(mask, logits, actions, g_lp, g_H, dt)
        assert not g[~mask].any(), dt
        assert not g[3].any() and g[1, 0] == 0.0, dt
    only_lp = gr.closed_form(mask, logits, actions, g_lp, None)
    assert only_lp[1, A - 1] == -g_lp[1] and not only_lp[1, :A - 1].any()      # row 1: the one allowed action has p = 1
    assert not only_lp[0].any()                                                 # row 0: the chosen action is the only one: 1 - p = 0


def test_actions_outside_the_range_give_a_zero_row(inputs):
    mask, logits, actions, g_lp, g_H = inputs
    a = actions.copy()
    a[9], a[10] = -1, A
    g = gr.closed_form(mask, logits, a, g_lp, g_H)
    assert not g[9].any() and not g[10].any() and g[11].any()
