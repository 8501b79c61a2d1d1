"""fp64 NumPy closed form of the gradient of the masked action head from the latent (include/mcbs.h "masked action head from the latent:
gradient"), its error bound, and the torch composite it restates: autograd through F.linear -> where(mask, logits, -1e8) -> Categorical
for log_prob(actions) and MaskableCategorical's entropy.  tests/test_linear_head_grad_ref.py pins the closed form to the composite in fp64
and shows the fp32 composite inside the bound; tests/test_gpu_linear_categorical_grad.py holds the kernels to the same bound.

Closed form: x = logits64(latent, weight, bias); g = categorical_grad_ref.closed_form(mask, x, ...) [n, A];
    grad_latent = g @ W,  grad_weight = g.T @ L,  grad_bias = g.sum(0).

Error bound, valid for ANY order of the three sums.  With
    E_g      the largest error over the allowed entries of live rows of torch's fp32 CPU autograd with respect to the logits
             (categorical_grad_ref.composite_grad(..., torch.float32) on float32(x)) against the closed form on the same float32(x),
    delta_i  linear_head_ref.dot_bound: what the fp32 logits of row i may be off by (0 on exact_inputs),
    q_ia     the product term of g: p_a * (-g_lp - g_H * (log p_a + H)),
    B_ia     = 4 E_g + ulp32(g_ia) + 2.1 delta_i (|q_ia| + p_ia |g_H,i| (H_i + 2))   for allowed entries of live rows, else 0
             (the first two terms are the project's accepted rule for the logits gradient; the third is the first-order sensitivity of g
             to a perturbation of every logit of the row by at most delta: |d log p| <= 2 delta, |d p| <= 2 delta p, |d H| <= 2 delta (H + 1)),
    gamma_k  = k u / (1 - k u), u = 2^-24: k roundings of a sum of k - 1 products,
the bounds are
    grad_latent: B @ |W|   + gamma_{K_i + 1} (|g| @ |W|)
    grad_weight: B.T @ |L| + gamma_{n_a + 1} (|g|.T @ |L|)        n_a = the live rows that allow a
    grad_bias:   B.sum(0)  + gamma_{n_a + 1} |g|.sum(0)
and an entry whose bound is 0 (a dead row, an action no live row allows) must be exactly +0.0."""
import numpy as np

from tests import categorical_grad_ref as cgr
from tests import linear_head_ref as lhr

U = lhr.U


def _gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def live_rows(mask, actions):
    """Rows that contribute: at least one allowed action and the chosen action inside [0, A)."""
    mask = np.asarray(mask, dtype=bool)
    actions = np.asarray(actions)
    return mask.any(axis=1) & (actions >= 0) & (actions < mask.shape[1])


def closed_form(mask, latent, weight, bias, actions, g_lp=None, g_H=None):
    """-> dict(x, g, grad_latent, grad_weight, grad_bias), all float64, from the values as given (bf16 inputs widen exactly)."""
    L, Wt = lhr.to64(latent), lhr.to64(weight)
    x = lhr.logits64(latent, weight, bias)
    g = cgr.closed_form(mask, x, actions, g_lp, g_H)
    return dict(x=x, g=g, grad_latent=g @ Wt, grad_weight=g.T @ L, grad_bias=g.sum(axis=0))


def _row_terms(mask, x, g_lp, g_H):
    """Per entry: p, the product term q, and per row the entropy, in fp64 (0 outside the mask)."""
    n, A = mask.shape
    p, q, ent = np.zeros((n, A)), np.zeros((n, A)), np.zeros(n)
    for i in range(n):
        S = np.flatnonzero(mask[i])
        if S.size == 0:
            continue
        d = x[i, S] - x[i, S].max()
        ex = np.exp(d)
        Z = ex.sum()
        pi = ex / Z
        logp = d - np.log(Z)
        on = ex > 0.0
        ent[i] = -(pi[on] * logp[on]).sum()
        p[i, S] = pi
        q[i, S] = np.where(on, pi * (-g_lp[i] - g_H[i] * (logp + ent[i])), 0.0)
    return p, q, ent


def logits_grad_error(mask, x, actions, g_lp, g_H):
    """E_g: the largest error over the allowed entries of live rows of torch's fp32 CPU autograd with respect to the logits against the
    closed form, both on float32(x)."""
    import torch
    mask = np.asarray(mask, dtype=bool)
    live = live_rows(mask, actions)
    if not live.any():
        return 0.0
    x32 = np.asarray(x, dtype=np.float64).astype(np.float32)[live]
    a, gl, gh = np.asarray(actions)[live], np.asarray(g_lp)[live], np.asarray(g_H)[live]
    want = cgr.closed_form(mask[live], x32, a, gl, gh)
    comp = cgr.composite_grad(mask[live], x32, a, gl, gh, torch.float32)
    return float(np.abs(comp - want)[mask[live]].max())


def bounds(mask, latent, weight, bias, actions, g_lp=None, g_H=None, exact=False):
    """-> dict(grad_latent, grad_weight, grad_bias) of the error bounds above (float64, the outputs' shapes), and "E_g".
    exact: the inputs are linear_head_ref.exact_inputs, every logit is exact in fp32 in any order: delta = 0."""
    mask = np.asarray(mask, dtype=bool)
    n, A = mask.shape
    g_lp = np.zeros(n) if g_lp is None else np.asarray(g_lp, dtype=np.float64)
    g_H = np.zeros(n) if g_H is None else np.asarray(g_H, dtype=np.float64)
    L, Wt = np.abs(lhr.to64(latent)), np.abs(lhr.to64(weight))
    ref = closed_form(mask, latent, weight, bias, actions, g_lp, g_H)
    x, g = ref["x"], ref["g"]
    live = live_rows(mask, actions)
    sel = mask & live[:, None]
    E_g = logits_grad_error(mask, x, actions, g_lp, g_H)
    delta = np.zeros(n) if exact else lhr.dot_bound(latent, weight, bias, mask)
    p, q, ent = _row_terms(mask, x, g_lp, g_H)
    ulp = np.spacing(np.abs(g).astype(np.float32)).astype(np.float64)
    B = 4.0 * E_g + ulp + 2.1 * delta[:, None] * (np.abs(q) + p * np.abs(g_H)[:, None] * (ent[:, None] + 2.0))
    B = np.where(sel, B, 0.0)
    absg = np.abs(g)
    K = sel.sum(axis=1)
    n_a = sel.sum(axis=0)
    return dict(E_g=E_g,
                grad_latent=B @ Wt + _gamma(K + 1)[:, None] * (absg @ Wt),
                grad_weight=B.T @ L + _gamma(n_a + 1)[:, None] * (absg.T @ L),
                grad_bias=B.sum(axis=0) + _gamma(n_a + 1) * absg.sum(axis=0))


def composite_grads(mask, latent, weight, bias, actions, g_lp, g_H, dtype):
    """torch autograd on the CPU in `dtype`: the gradients with respect to latent, weight and bias of sum(g_lp * log_prob(actions) +
    g_H * entropy) through F.linear -> where(mask, logits, -1e8) -> Categorical, as float64 arrays.  Rows whose action lies outside
    [0, A) contribute nothing (the kernel's rule); bias None: grad_bias is what a zero bias would receive."""
    import torch
    mask = np.asarray(mask, dtype=bool)
    n, A = mask.shape
    actions = np.asarray(actions, dtype=np.int64)
    inside = (actions >= 0) & (actions < A)
    tm = torch.as_tensor(mask)
    lat = torch.as_tensor(lhr.to64(latent)).to(dtype).requires_grad_(True)
    w = torch.as_tensor(lhr.to64(weight)).to(dtype).requires_grad_(True)
    b = (torch.zeros(A, dtype=dtype) if bias is None else torch.as_tensor(lhr.to64(bias)).to(dtype)).requires_grad_(True)
    x = torch.nn.functional.linear(lat, w, b)
    dist = torch.distributions.Categorical(logits=torch.where(tm, x, torch.tensor(-1e8, dtype=dtype)))
    lp = dist.log_prob(torch.as_tensor(np.where(inside, actions, 0)))
    ent = -(torch.where(tm, dist.logits * dist.probs, torch.zeros((), dtype=dtype))).sum(-1)
    keep = torch.as_tensor(inside).to(dtype)
    loss = (lp * torch.as_tensor(np.asarray(g_lp)).to(dtype) * keep).sum() + (ent * torch.as_tensor(np.asarray(g_H)).to(dtype) * keep).sum()
    loss.backward()
    return dict(grad_latent=lat.grad.double().numpy(), grad_weight=w.grad.double().numpy(), grad_bias=b.grad.double().numpy())


def general_inputs(n, A, H, rng):
    """(latent, weight, bias) float32: randn latent, 4 randn / sqrt(H) weight, randn bias — logits of the spread of synthetic_inputs."""
    latent = rng.standard_normal((n, H)).astype(np.float32)
    weight = (4.0 * rng.standard_normal((A, H)) / np.sqrt(H)).astype(np.float32)
    bias = rng.standard_normal(A).astype(np.float32)
    return latent, weight, bias


def case(A, H, exact, n=64, bf16=False, seed=5):
    """One input set of the GPU tests: the 64 synthetic rows' masks, actions (two of them outside [0, A)) and incoming gradients, with
    exact_inputs or general_inputs for the layer.  bf16: the layer's values rounded to bfloat16 (still float32 arrays).
    -> dict(mask, latent, weight, bias, actions, g_lp, g_H)."""
    mask, _, actions, g_lp, g_H = cgr.synthetic_inputs(A, n)
    actions = actions.copy()
    actions[9], actions[10] = -1, A
    rng = np.random.default_rng(seed + 131 * H + (7 if exact else 0))
    latent, weight, bias = lhr.exact_inputs(n, A, H, rng) if exact else general_inputs(n, A, H, rng)
    if bf16:
        import torch
        latent, weight, bias = (torch.as_tensor(v).bfloat16().float().numpy() for v in (latent, weight, bias))
    return dict(mask=mask, latent=latent, weight=weight, bias=bias, actions=actions, g_lp=g_lp, g_H=g_H)
