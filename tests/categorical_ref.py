"""fp64 NumPy restatement of the masked categorical head (include/mcbs.h "masked categorical head"): what
`torch.distributions.Categorical(logits=where(mask, logits, -1e8))` gives for log_prob, MaskableCategorical's entropy with the masked
terms zeroed, the arg max, and the inverse-CDF sample in ascending action order — computed from the ALLOWED entries only (rows of
186 120 actions stay cheap), with K = 0 (uniform over all A, entropy 0) and logits=None (uniform over the allowed actions).
tests/test_categorical_ref.py pins it to torch's fp64 composite and its Philox keying to the oracle's Philox."""
import numpy as np

PHILOX_DOMAIN = 0xCA7E6041          # MCBS_CATEGORICAL_PHILOX_DOMAIN
FILL = float(np.float32(-1e8))      # the reference's `where(mask, logits, -1e8)`
M32 = 0xFFFFFFFF


def philox_counter_key(seed: int, row_key: int, step: int):
    """The documented keying: counter = (key_lo, key_hi, step_lo, step_hi), key = (seed_lo ^ DOMAIN, seed_hi)."""
    return ([row_key & M32, (row_key >> 32) & M32, step & M32, (step >> 32) & M32], [(seed & M32) ^ PHILOX_DOMAIN, (seed >> 32) & M32])


def philox4x32_10(ctr, key) -> np.ndarray:
    """Philox4x32-10 on arrays of counters [n, 4] and one key (2,): -> uint32 [n, 4]."""
    c = np.array(ctr, dtype=np.uint64).reshape(-1, 4).copy()
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[:, 0]
        p1 = np.uint64(0xCD9E8D57) * c[:, 2]
        n0 = (p1 >> np.uint64(32)) ^ c[:, 1] ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c[:, 3] ^ np.uint64(k1)
        c = np.stack([n0, p1 & np.uint64(M32), n2, p0 & np.uint64(M32)], axis=1)
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c.astype(np.uint32)


def philox_u24(seed: int, row_keys, step: int) -> np.ndarray:
    """u24 of every row key: the top 24 bits of word 0 of the row's one Philox block."""
    rk = np.asarray(row_keys, dtype=np.uint64)
    ctr = np.stack([rk & np.uint64(M32), rk >> np.uint64(32), np.full_like(rk, step & M32), np.full_like(rk, (step >> 32) & M32)], axis=1)
    return (philox4x32_10(ctr, philox_counter_key(seed, 0, step)[1])[:, 0] >> np.uint32(8)).astype(np.int64)


def u24_of_uniforms(u) -> np.ndarray:
    """u24 = min(2^24 - 1, floor(uniforms * 2^24)) of float32 uniforms."""
    return np.minimum(2 ** 24 - 1, np.floor(np.asarray(u, dtype=np.float32).astype(np.float64) * 2.0 ** 24)).astype(np.int64)


class CategoricalRef:
    """mask: bool [n, A]; logits: [n, A] of any float type (taken to fp64 as they are) or None."""

    def __init__(self, mask, logits=None):
        mask = np.asarray(mask, dtype=bool)
        self.mask = mask
        self.n, self.A = n, A = mask.shape
        self.uniform = logits is None
        self.logits = None if logits is None else np.asarray(logits)
        rows, cols = np.nonzero(mask)                    # row-major: ascending actions within a row
        self.rows, self.cols = rows, cols
        self.K = K = np.bincount(rows, minlength=n).astype(np.int64)
        self.start = np.concatenate([[0], np.cumsum(K)[:-1]]).astype(np.int64)
        nz = K > 0
        seg = self.start[nz]
        x = np.zeros(rows.size) if logits is None else self.logits[rows, cols].astype(np.float64)
        self.m = np.zeros(n)
        self.Z = np.ones(n)
        T = np.zeros(n)
        self.argmax = np.zeros(n, dtype=np.int64)        # K = 0: action 0
        if rows.size:
            self.m[nz] = np.maximum.reduceat(x, seg)
            d = x - self.m[rows]
            e = np.exp(d)
            self.Z[nz] = np.add.reduceat(e, seg)
            T[nz] = np.add.reduceat(np.where(e > 0, d * e, 0.0), seg)
            self.argmax[nz] = np.minimum.reduceat(np.where(d == 0.0, cols, A), seg)       # the lowest index among equal logits
            cum = np.cumsum(e)
            self.cdf = (cum - (cum[self.start[rows]] - e[self.start[rows]])) / self.Z[rows]   # per allowed entry: cumulative probability up to and including it
            self.x = x
        else:
            self.cdf, self.x = np.zeros(0), np.zeros(0)
        self.logZ = np.log(self.Z)
        self.entropy = np.where(nz, self.logZ - T / self.Z, 0.0)                          # K = 0: entropy 0

    def log_prob(self, actions) -> np.ndarray:
        """log p of one action per row: allowed (x - m) - log Z, not allowed (-1e8 - m) - log Z, outside [0, A) NaN; K = 0: -log A."""
        a = np.asarray(actions, dtype=np.int64)
        out = np.full(self.n, np.nan)
        ok = (a >= 0) & (a < self.A)
        r = np.nonzero(ok)[0]
        on = self.mask[r, a[r]]
        x = np.where(on, 0.0 if self.uniform else self.logits[r, a[r]].astype(np.float64), FILL)
        out[r] = np.where(self.K[r] > 0, (x - self.m[r]) - self.logZ[r], -np.log(float(self.A)))
        return out

    def sample(self, u24) -> np.ndarray:
        """Inverse CDF in ascending action order at u = u24 * 2^-24: the first allowed action whose cumulative probability exceeds u (the
        last allowed one if none does); logits=None: the ((u24 * K) >> 24)-th allowed action; K = 0: (u24 * A) >> 24."""
        u24 = np.asarray(u24, dtype=np.int64)
        out = np.zeros(self.n, dtype=np.int64)
        for i in range(self.n):
            K, s = int(self.K[i]), int(self.start[i])
            if K == 0:
                out[i] = (int(u24[i]) * self.A) >> 24
            elif self.uniform:
                out[i] = self.cols[s + ((int(u24[i]) * K) >> 24)]
            else:
                j = int(np.searchsorted(self.cdf[s:s + K], float(u24[i]) * 2.0 ** -24, side="right"))
                out[i] = self.cols[s + min(j, K - 1)]
        return out

    def cdf_interval(self, actions):
        """(F(a-), F(a)) per row for ALLOWED actions a (a- = the previous allowed action, F = 0 before the first); NaN elsewhere."""
        a = np.asarray(actions, dtype=np.int64)
        lo, hi = np.full(self.n, np.nan), np.full(self.n, np.nan)
        for i in range(self.n):
            K, s = int(self.K[i]), int(self.start[i])
            if K == 0 or not (0 <= a[i] < self.A) or not self.mask[i, a[i]]:
                continue
            j = int(np.searchsorted(self.cols[s:s + K], a[i]))
            hi[i] = self.cdf[s + j]
            lo[i] = self.cdf[s + j - 1] if j else 0.0
        return lo, hi
