"""tests/linear_head_ref.py against torch on the CPU: the error bound holds for torch's own fp32 linear layer, and on exact_inputs
torch.nn.functional.linear IS the fp64 result, so a GPU test may take it as the logits buffer the fused head must reproduce bit for bit.

bfloat16: the head widens bf16 inputs exactly and works in float32, so "the bf16 F.linear" it is compared with is F.linear on the widened
values (a bf16 OUTPUT would round the exact dot product to 8 bits)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import linear_head_ref as lr


@pytest.mark.parametrize("H", [1, 7, 64, 65, 512])
def test_fp32_linear_stays_within_dot_bound(H):
    g = torch.Generator().manual_seed(H)
    n, A = 48, 700
    latent = torch.randn((n, H), generator=g)
    weight = torch.randn((A, H), generator=g) / H ** 0.5
    bias = torch.randn(A, generator=g)
    want = lr.logits64(latent, weight, bias)
    np.testing.assert_array_equal(want, latent.double().numpy() @ weight.double().numpy().T + bias.double().numpy())
    got = F.linear(latent, weight, bias).double().numpy()
    mask = np.ones((n, A), dtype=bool)
    delta = lr.dot_bound(latent, weight, bias, mask)
    err = np.abs(got - want).max(axis=1)
    print(f"H={H}: fp32 F.linear max error {err.max():.3e}, bound {delta.min():.3e} .. {delta.max():.3e}")
    assert np.all(err <= delta) and np.all(delta > 0)
    # the bound is the maximum over the allowed actions only, and 0 for a row without any
    mask[:, A // 2:] = False
    mask[3] = False
    d2 = lr.dot_bound(latent, weight, bias, mask)
    assert d2[3] == 0.0 and np.all(d2 <= delta)
    assert np.all(np.abs(got - want)[:, :A // 2].max(axis=1)[mask.any(1)] <= d2[mask.any(1)])
    # without a bias
    np.testing.assert_array_equal(lr.logits64(latent, weight), latent.double().numpy() @ weight.double().numpy().T)


@pytest.mark.parametrize("H", [1, 3, 64, 65, 200])
def test_exact_inputs_make_every_order_exact(H):
    rng = np.random.default_rng(100 + H)
    n, A = 32, 900
    latent, weight, bias = lr.exact_inputs(n, A, H, rng)
    assert latent.dtype == weight.dtype == bias.dtype == np.float32
    assert np.abs(latent).max() <= 2 and np.abs(weight).max() <= 1 and np.abs(bias).max() <= 1
    assert np.all(latent * 8 == np.round(latent * 8)) and np.all(weight * 16 == np.round(weight * 16)) and np.all(bias * 16 == np.round(bias * 16))
    tl, tw, tb = torch.as_tensor(latent), torch.as_tensor(weight), torch.as_tensor(bias)
    want = lr.logits64(tl, tw, tb)
    assert np.all(want * 128 == np.round(want * 128)) and np.abs(want).max() < 512
    got32 = F.linear(tl, tw, tb)
    np.testing.assert_array_equal(got32.double().numpy(), want)
    # bf16 storage holds the same values; widened, the layer gives the same bits
    bl, bw, bb = tl.bfloat16(), tw.bfloat16(), tb.bfloat16()
    assert torch.equal(bl.float(), tl) and torch.equal(bw.float(), tw) and torch.equal(bb.float(), tb)
    np.testing.assert_array_equal(lr.logits64(bl, bw, bb), want)
    got16 = F.linear(bl.float(), bw.float(), bb.float())
    assert torch.equal(got16.view(torch.int32), got32.view(torch.int32))
    # any order: reversed and pairwise sums of the fp32 products
    prod = latent[:, None, :] * weight[None, :, :]
    np.testing.assert_array_equal((np.cumsum(prod[..., ::-1], axis=-1, dtype=np.float32)[..., -1] + bias).astype(np.float64), want)
    np.testing.assert_array_equal((prod.sum(axis=-1, dtype=np.float32) + bias).astype(np.float64), want)
