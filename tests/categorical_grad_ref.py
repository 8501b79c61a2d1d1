"""fp64 NumPy closed form of the gradient of the masked categorical head (include/mcbs.h "masked categorical head: gradient"), from the
allowed entries only, and the torch composite it restates: autograd through `Categorical(logits=where(mask, logits, -1e8))` for
`log_prob(actions)` and MaskableCategorical's entropy with the masked terms zeroed.  tests/test_categorical_grad_ref.py pins the closed
form to the composite in fp64; tests/test_gpu_categorical_grad.py measures the kernel against the closed form and bounds its error by
the fp32 composite's."""
import numpy as np


def synthetic_masks(A, n=64):
    """The 64 hand-made rows of test_gpu_categorical._synthetic_masks: the listed corner cases first, random densities after."""
    rng = np.random.default_rng(11)
    mask = np.zeros((n, A), dtype=bool)
    mask[0, 0] = True                                    # only bit 0
    mask[1, A - 1] = True                                # only bit A-1
    mask[2, :] = True                                    # all A bits
    # row 3: no bits
    mask[4, ::2] = True                                  # alternating bits
    mask[5, 1::2] = True
    w0 = np.arange(0, A, 32)
    mask[6, np.minimum(w0 + (7 * (w0 // 32)) % 32, A - 1)] = True     # one bit per word
    mask[7, [3, 4, 5]] = True                            # +-80 next to 0 (synthetic_inputs)
    mask[8, [31, 32, 63, 64, A - 2]] = True              # word boundaries
    for i in range(9, n):
        mask[i] = rng.random(A) < rng.random() ** 3
    return mask


def pack(mask, row_words, garbage_tail=False):
    """Rows of `row_words` int32 words, bit a of a row = bit (a & 31) of word a >> 5; garbage_tail: ones in the bits of word W-1 from A
    on and 0xDEADBEEF in the words from W on (both are not the mask's)."""
    n, A = mask.shape
    W = (A + 31) // 32
    m = np.zeros((n, row_words * 32), dtype=np.uint64)
    m[:, :A] = mask
    if garbage_tail:
        m[:, A:W * 32] = 1
    words = (m.reshape(n, row_words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    if garbage_tail:
        words[:, W:] = 0xDEADBEEF
    return words.view(np.int32)


def synthetic_inputs(A, n=64):
    """-> (mask [n, A] bool, logits [n, A] float32 = randn * 4, actions [n] int64, g_lp [n] float32, g_H [n] float32).  Row 7 holds
    80 / 0 / -80 (only the max subtraction keeps these finite), row 8 equal logits.  Actions: an allowed one wherever the row has any;
    row 1 action 0, which is not allowed; row 3 (blank) action 5."""
    mask = synthetic_masks(A, n)
    rng = np.random.default_rng(21)
    logits = (rng.standard_normal((n, A)) * 4.0).astype(np.float32)
    logits[7, 3], logits[7, 4], logits[7, 5] = 80.0, 0.0, -80.0
    logits[8, [31, 32, 63, 64, A - 2]] = 2.5
    actions = np.zeros(n, dtype=np.int64)
    for i in range(n):
        on = np.flatnonzero(mask[i])
        actions[i] = on[rng.integers(0, on.size)] if on.size else 5
    actions[0], actions[1], actions[2] = 0, 0, A - 1     # allowed, not allowed, allowed
    assert not mask[1, 0] and not mask[3].any()
    g_lp = rng.standard_normal(n).astype(np.float32)
    g_H = rng.standard_normal(n).astype(np.float32)
    return mask, logits, actions, g_lp, g_H


def closed_form(mask, logits, actions, g_lp=None, g_H=None):
    """grad_logits [n, A] float64.  For the allowed set S of row i, p the softmax over S, H its entropy, c = actions[i]:
    a in S: p_a * (-g_lp - g_H * (log p_a + H)) + (a == c ? g_lp : 0), the product being 0 where p_a underflows; a not in S: 0; an
    all-zero row or c outside [0, A): the whole row 0.  g_lp / g_H = None: zeros."""
    mask = np.asarray(mask, dtype=bool)
    x = np.asarray(logits, dtype=np.float64)
    n, A = mask.shape
    g_lp = np.zeros(n) if g_lp is None else np.asarray(g_lp, dtype=np.float64)
    g_H = np.zeros(n) if g_H is None else np.asarray(g_H, dtype=np.float64)
    out = np.zeros((n, A), dtype=np.float64)
    for i in range(n):
        S = np.flatnonzero(mask[i])
        c = int(actions[i])
        if S.size == 0 or c < 0 or c >= A:
            continue
        d = x[i, S] - x[i, S].max()
        ex = np.exp(d)
        Z = ex.sum()
        p = ex / Z
        logp = d - np.log(Z)
        live = ex > 0.0
        H = -(p[live] * logp[live]).sum()
        out[i, S] = np.where(live, p * (-g_lp[i] - g_H[i] * (logp + H)), 0.0)
        if mask[i, c]:
            out[i, c] += g_lp[i]
    return out


def composite_grad(mask, logits, actions, g_lp, g_H, dtype):
    """torch autograd on the CPU in `dtype` (torch.float64 / torch.float32): the gradient with respect to the logits of
    sum(g_lp * log_prob(actions) + g_H * entropy) through where(mask, logits, -1e8) -> Categorical, as a float64 array [n, A].
    Actions must lie inside [0, A)."""
    import torch
    tm = torch.as_tensor(np.asarray(mask, dtype=bool))
    x = torch.as_tensor(np.asarray(logits)).to(dtype).clone().requires_grad_(True)
    dist = torch.distributions.Categorical(logits=torch.where(tm, x, torch.tensor(-1e8, dtype=dtype)))
    lp = dist.log_prob(torch.as_tensor(np.asarray(actions, dtype=np.int64)))
    ent = -(torch.where(tm, dist.logits * dist.probs, torch.zeros((), dtype=dtype))).sum(-1)
    (lp * torch.as_tensor(np.asarray(g_lp)).to(dtype)).sum().backward(retain_graph=True)
    (ent * torch.as_tensor(np.asarray(g_H)).to(dtype)).sum().backward()
    return x.grad.double().numpy()
