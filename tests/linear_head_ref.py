"""fp64 NumPy restatement of the linear layer in front of the masked action head (include/mcbs.h "masked action head from the latent"):
the logits `latent @ weight.T + bias` a policy's action_net would produce, the forward error bound of an fp32 dot product, and inputs
on which every dot product is exact in fp32 whatever the order of its sum.  tests/test_linear_head_ref.py pins them to torch on the CPU."""
import numpy as np

U = 2.0 ** -24                      # unit roundoff of float32


def to64(x) -> np.ndarray:
    """A NumPy array or a torch tensor (float32 / bfloat16 / float64, any device) as fp64, exactly."""
    if hasattr(x, "detach"):
        x = x.detach().double().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def logits64(latent, weight, bias=None) -> np.ndarray:
    """fp64 `latent @ weight.T + bias` on the values as given (bf16 inputs are widened exactly): [n, A]."""
    x = to64(latent) @ to64(weight).T
    return x if bias is None else x + to64(bias)[None, :]


def dot_bound(latent, weight, bias, mask) -> np.ndarray:
    """Per row delta = gamma * max over the ALLOWED actions a of (|b_a| + sum_h |latent_h| |W_ah|), gamma = (H+1)u / (1 - (H+1)u): the
    standard forward bound of an fp32 dot product of length H plus one addition, valid for any summation order, fused or not.  A row
    without allowed actions gets 0."""
    L, Wt = np.abs(to64(latent)), np.abs(to64(weight))
    H = L.shape[1]
    gamma = (H + 1) * U / (1.0 - (H + 1) * U)
    mag = L @ Wt.T
    if bias is not None:
        mag = mag + np.abs(to64(bias))[None, :]
    return gamma * np.where(np.asarray(mask, dtype=bool), mag, 0.0).max(axis=1)


def exact_inputs(n: int, A: int, H: int, rng):
    """(latent [n, H], weight [A, H], bias [A]) as float32: latent entries multiples of 2^-3 in [-2, 2], weights and bias multiples of
    2^-4 in [-1, 1], H <= 200.  Every product is a multiple of 2^-7 and every partial sum stays below 2^9 (200 * 2 + 1 < 512), so it has
    at most 16 significant bits: every dot product is exact in fp32 in any order, and every input is exact in bf16 storage (at most 6
    significant bits)."""
    assert 1 <= H <= 200
    latent = rng.integers(-16, 17, size=(n, H)).astype(np.float32) / np.float32(8.0)
    weight = rng.integers(-16, 17, size=(A, H)).astype(np.float32) / np.float32(16.0)
    bias = rng.integers(-16, 17, size=A).astype(np.float32) / np.float32(16.0)
    return latent, weight, bias
