"""fp64 NumPy restatement of the MultiDiscrete head (include/mcbs.h "MultiDiscrete head"): what Stable-Baselines3's
MultiCategoricalDistribution gives for a MultiDiscrete(nvec) action — `split` the row of logits by nvec, a Categorical per segment,
log_prob and entropy summed over the segments — with the arg max (lowest index among equal logits), the inverse-CDF sample in ascending
index order, the CDF interval of an action, the closed-form gradient and the documented Philox keying.
tests/test_multicategorical_ref.py pins it to torch's fp64 composite and fp64 autograd."""
import numpy as np

from tests.categorical_ref import M32, philox4x32_10

PHILOX_DOMAIN = 0x3C47E6A1          # MCBS_MULTICATEGORICAL_PHILOX_DOMAIN
MAX_DIMS = 16                       # MCBS_MAX_ACTION_DIMS

# the shapes every test of the head runs: the issue's list, and one row too wide for the kernel's LDS staging (A = 8 320 > 8 192 floats)
NVECS = {
    "defender_toyctf": [5, 10, 10, 6, 2, 10, 6, 2, 10, 3, 10, 3],
    "attacker_chain10": [3, 12, 5, 12, 12, 2, 12, 12, 8, 12],
    "ones_and_seven": [1, 1, 7, 1],
    "one_dimension": [9],
    "sixteen_mixed": [1, 2, 3, 5, 2, 1, 7, 4, 11, 2, 6, 1, 9, 2, 13, 8],
    "defender_256": [5, 256, 256, 6, 2, 256, 6, 2, 256, 3, 256, 3],
    "credentials_1000": [3, 1000, 4],
    "wider_than_lds": [520] * 16,
}


def philox_counter_key(seed: int, row_key: int, step: int, d: int):
    """The documented keying of dimension d: counter = (k_lo, k_hi, step_lo, step_hi | ((d >> 2) << 16)), key = (seed_lo ^ DOMAIN,
    seed_hi); the dimension takes word d & 3 of the block."""
    return ([row_key & M32, (row_key >> 32) & M32, step & M32, ((step >> 32) & M32) | ((d >> 2) << 16)],
            [(seed & M32) ^ PHILOX_DOMAIN, (seed >> 32) & M32])


def philox_u24(seed: int, row_keys, step: int, n_dims: int) -> np.ndarray:
    """u24 [n, D] of every (row key, dimension): the top 24 bits of word d & 3 of block d >> 2."""
    rk = np.asarray(row_keys, dtype=np.uint64)
    out = np.zeros((rk.size, n_dims), dtype=np.int64)
    for blk in range((n_dims + 3) // 4):
        hi = ((step >> 32) & M32) | (blk << 16)
        ctr = np.stack([rk & np.uint64(M32), rk >> np.uint64(32), np.full_like(rk, step & M32), np.full_like(rk, hi)], axis=1)
        words = philox4x32_10(ctr, philox_counter_key(seed, 0, step, 0)[1])
        for d in range(4 * blk, min(n_dims, 4 * blk + 4)):
            out[:, d] = (words[:, d & 3] >> np.uint32(8)).astype(np.int64)
    return out


def u24_of_uniforms(u) -> np.ndarray:
    """u24 = min(2^24 - 1, floor(uniforms * 2^24)) of float32 uniforms."""
    return np.minimum(2 ** 24 - 1, np.floor(np.asarray(u, dtype=np.float32).astype(np.float64) * 2.0 ** 24)).astype(np.int64)


class MultiCategoricalRef:
    """nvec: D dimension widths; logits: [n, >= A] of any float type (taken to fp64 as they are), or None with n rows of the uniform law."""

    def __init__(self, nvec, logits=None, n=None):
        self.nvec = nv = [int(v) for v in nvec]
        self.D, self.A = len(nv), sum(nv)
        self.off = np.concatenate([[0], np.cumsum(nv)[:-1]]).astype(np.int64)
        self.uniform = logits is None
        self.n = n = int(n) if logits is None else np.asarray(logits).shape[0]
        x = np.zeros((n, self.A)) if logits is None else np.asarray(logits)[:, :self.A].astype(np.float64)
        self.x = x
        self.m, self.Z, self.H = np.zeros((n, self.D)), np.zeros((n, self.D)), np.zeros((n, self.D))
        self.argmax = np.zeros((n, self.D), dtype=np.int64)
        self.logp = np.zeros((n, self.A))                # log p of every (dimension, index)
        self.cdf = np.zeros((n, self.A))                 # cumulative probability up to and including the index, within its dimension
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            for d, (o, w) in enumerate(zip(self.off, nv)):
                seg = x[:, o:o + w]
                m = seg.max(axis=1)
                dd = seg - m[:, None]
                e = np.exp(dd)
                Z = e.sum(axis=1)
                T = np.where(e > 0, dd * e, 0.0).sum(axis=1)
                self.m[:, d], self.Z[:, d] = m, Z
                self.H[:, d] = np.log(Z) - T / Z
                self.argmax[:, d] = np.argmax(seg, axis=1)       # the first of equal maxima
                self.logp[:, o:o + w] = dd - np.log(Z)[:, None]
                self.cdf[:, o:o + w] = np.cumsum(e, axis=1) / Z[:, None]
        self.entropy = self.H.sum(axis=1)

    def in_range(self, actions) -> np.ndarray:
        a = np.asarray(actions, dtype=np.int64).reshape(self.n, self.D)
        return (a >= 0) & (a < np.asarray(self.nvec)[None, :])

    def log_prob(self, actions) -> np.ndarray:
        """sum over d of log p of the row's components; NaN for a row with a component outside its range."""
        a = np.asarray(actions, dtype=np.int64).reshape(self.n, self.D)
        ok = self.in_range(a)
        cols = np.where(ok, a, 0) + self.off[None, :]
        lp = np.take_along_axis(self.logp, cols, axis=1).sum(axis=1)
        return np.where(ok.all(axis=1), lp, np.nan)

    def sample(self, u24) -> np.ndarray:
        """Per dimension: inverse CDF in ascending index order at u = u24 * 2^-24 (the first index whose cumulative probability exceeds u,
        the last index if none does); logits=None: (u24 * nvec[d]) >> 24."""
        u24 = np.asarray(u24, dtype=np.int64).reshape(self.n, self.D)
        out = np.zeros((self.n, self.D), dtype=np.int64)
        for d, (o, w) in enumerate(zip(self.off, self.nvec)):
            if self.uniform:
                out[:, d] = (u24[:, d] * w) >> 24
            else:
                u = u24[:, d].astype(np.float64) * 2.0 ** -24
                out[:, d] = np.minimum((self.cdf[:, o:o + w] <= u[:, None]).sum(axis=1), w - 1)
        return out

    def cdf_interval(self, actions):
        """(F(a - 1), F(a)) per (row, dimension) for components inside their range (F(-1) = 0); NaN elsewhere."""
        a = np.asarray(actions, dtype=np.int64).reshape(self.n, self.D)
        ok = self.in_range(a)
        cols = np.where(ok, a, 0) + self.off[None, :]
        hi = np.take_along_axis(self.cdf, cols, axis=1)
        prev = np.take_along_axis(self.cdf, np.maximum(cols - 1, 0), axis=1)
        lo = np.where(np.where(ok, a, 0) > 0, prev, 0.0)
        return np.where(ok, lo, np.nan), np.where(ok, hi, np.nan)

    def grad(self, actions, g_lp=None, g_H=None) -> np.ndarray:
        """The closed form: grad[i, off_d + a] = p (-g_lp - g_H (log p + H_d)) + (a == c_d ? g_lp : 0), the product term 0 where p is 0;
        a row with a component outside its range is zero throughout.  None = zeros."""
        a = np.asarray(actions, dtype=np.int64).reshape(self.n, self.D)
        g_lp = np.zeros(self.n) if g_lp is None else np.asarray(g_lp, dtype=np.float64)
        g_H = np.zeros(self.n) if g_H is None else np.asarray(g_H, dtype=np.float64)
        ok = self.in_range(a).all(axis=1)
        out = np.zeros((self.n, self.A))
        with np.errstate(invalid="ignore"):
            for d, (o, w) in enumerate(zip(self.off, self.nvec)):
                lq = self.logp[:, o:o + w]
                p = np.exp(lq)
                prod = np.where(p > 0, p * (-g_lp[:, None] - g_H[:, None] * (lq + self.H[:, d:d + 1])), 0.0)
                hit = np.arange(w)[None, :] == a[:, d:d + 1]
                out[:, o:o + w] = prod + np.where(hit, g_lp[:, None], 0.0)
        out[~ok] = 0.0
        return out


def composite(nvec, logits, actions=None, dtype=None, g_lp=None, g_H=None):
    """SB3's composite in torch on the CPU in `dtype`: split -> Categorical per dimension -> log_prob(actions).sum, entropy.sum.
    -> (log_prob or None, entropy, grad or None) as fp64 NumPy; grad = autograd of (g_lp * log_prob + g_H * entropy).sum() (None = zeros)."""
    import torch
    x = torch.as_tensor(np.asarray(logits)).to(dtype).clone()
    want_grad = g_lp is not None or g_H is not None
    x.requires_grad_(want_grad)
    dists = [torch.distributions.Categorical(logits=s) for s in torch.split(x, [int(v) for v in nvec], dim=1)]
    ent = torch.stack([q.entropy() for q in dists], dim=1).sum(dim=1)
    lp = None
    if actions is not None:
        a = torch.as_tensor(np.asarray(actions, dtype=np.int64))
        lp = torch.stack([q.log_prob(c) for q, c in zip(dists, torch.unbind(a, dim=1))], dim=1).sum(dim=1)
    grad = None
    if want_grad:
        loss = torch.zeros((), dtype=dtype)
        if g_lp is not None:
            loss = loss + (torch.as_tensor(np.asarray(g_lp)).to(dtype) * lp).sum()
        if g_H is not None:
            loss = loss + (torch.as_tensor(np.asarray(g_H)).to(dtype) * ent).sum()
        loss.backward()
        grad = x.grad.double().numpy()
    return (None if lp is None else lp.detach().double().numpy()), ent.detach().double().numpy(), grad


# ---- plumbing shared by the GPU tests of the head (tests/test_gpu_multicategorical*.py) ----
SENTINEL = 7.0
_ENGINE = []


def chain4_engine(n_envs=64, **kw):
    """The engine of tests/test_gpu_categorical_grad.py::_chain4_engine (Chain-4, 64 envs): the head takes only its device from it."""
    from marlon_amd import engine
    from marlon_amd._abi import EnvSpec
    from marlon_amd.flatten import flatten
    from marlon_amd.samples import chainpattern
    topo = flatten(chainpattern.new_environment(4))
    return engine.BatchEngine(topo, EnvSpec(n_envs=n_envs, maximum_node_count=6, maximum_total_credentials=6,
                                            attacker_goal=dict(own_atleast_percent=1.0), **kw))


def shared_engine():
    """One engine for all tests of a process (they only launch the head's kernels through it)."""
    if not _ENGINE:
        _ENGINE.append(chain4_engine())
    return _ENGINE[0]


def bits_of(x):
    import torch
    return x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def framed(n, A, stride, offset, dtype, dev):
    """A [n, A] view at element `offset` with row stride `stride` inside a sentinel-filled buffer -> (buffer, view)."""
    import torch
    buf = torch.full((offset + n * stride + 9,), SENTINEL, dtype=dtype, device=dev)
    return buf, buf[offset:offset + n * stride].view(n, stride)[:, :A]


def frame_untouched(buf, n, A, stride, offset):
    rows = buf[offset:offset + n * stride].view(n, stride)
    return bool((buf[:offset] == SENTINEL).all()) and bool((rows[:, A:] == SENTINEL).all()) and bool((buf[offset + n * stride:] == SENTINEL).all())


def ulp(want, bf16=False):
    u = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return u * 65536.0 if bf16 else u                    # bfloat16 keeps 8 of float32's 24 significand bits


def within(got, want, comp, what, sel=None, bf16=False, rounded=False):
    """The rule of tests/test_gpu_categorical.py::_within and tests/test_gpu_categorical_grad.py::_within: over the entries sel,
    |got - want| <= 4 x (the largest |comp - want|) + one ulp of the value in the output dtype; prints both figures.  rounded (the
    uniform law: no composite): at most one float32 step from the correctly rounded float32 of want."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    sel = np.ones(want.shape, dtype=bool) if sel is None else sel
    if rounded:
        want = want.astype(np.float32).astype(np.float64)
    assert np.isfinite(got[sel]).all(), what
    err = np.abs(got - want)[sel]
    comp_err = 0.0 if comp is None else float(np.abs(np.asarray(comp, dtype=np.float64) - want)[sel].max())
    ratio = f"{err.max() / comp_err:.2f}" if comp_err > 0.0 else "n/a"
    print(f"{what}: kernel max abs error {err.max():.3e}, fp32 composite {comp_err:.3e}, ratio {ratio}")
    bound = 4.0 * comp_err + ulp(want[sel], bf16)
    worst = int(np.argmax(err - bound))
    assert np.all(err <= bound), f"{what}: entry {worst}: error {err[worst]:.3e} > bound {bound[worst]:.3e} (value {want[sel][worst]!r})"
