"""tests/categorical_ref.py — the fp64 restatement the GPU tests of the masked categorical head compare against — pinned to the
reference's semantics without SB3: `torch.distributions.Categorical(logits=torch.where(mask, logits, -1e8))` in fp64 for log_prob,
MaskableCategorical's `-(where(mask, logits_norm * probs, 0)).sum(-1)` for the entropy, argmax for the deterministic action; and its
Philox keying (include/mcbs.h) to the oracle's Philox4x32-10."""
import os
import re

import numpy as np

from tests import categorical_ref as cr

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOL = 1e-12


def _cases():
    rng = np.random.default_rng(5)
    n, A = 48, 203
    mask = rng.random((n, A)) < rng.random((n, 1)) * 0.6
    mask[0] = False                                      # an all-false row: uniform over all A, entropy 0
    mask[1] = True
    mask[2] = False
    mask[2, A - 1] = True                                # a single allowed action
    mask[3] = False
    mask[3, [0, 7, 64]] = True
    logits = rng.standard_normal((n, A)) * 4.0
    logits[3, [0, 7, 64]] = 1.5                          # equal logits: the lowest index wins
    logits[4, mask[4]] += 80.0 * np.sign(rng.standard_normal(int(mask[4].sum())))
    return mask, logits


def test_restatement_equals_torch_fp64_composite():
    import torch
    mask, logits = _cases()
    n, A = mask.shape
    ref = cr.CategoricalRef(mask, logits)
    tm, tl = torch.as_tensor(mask), torch.as_tensor(logits, dtype=torch.float64)
    dist = torch.distributions.Categorical(logits=torch.where(tm, tl, torch.tensor(-1e8, dtype=torch.float64)))
    norm, probs = dist.logits, dist.probs
    ent = -(torch.where(tm, norm * probs, torch.zeros((), dtype=torch.float64))).sum(-1)
    np.testing.assert_allclose(ref.entropy, ent.numpy(), rtol=TOL, atol=TOL)
    assert ref.entropy[0] == 0.0 and ref.K[0] == 0
    # The all-false row: torch normalises logits that are all -1e8, i.e. forms -1e8 - (-1e8 + log A) at magnitude 1e8, where one fp64 ulp is
    # 2^-26 = 1.5e-8: the composite's own rounding there, not the restatement's (-log A exactly) — that row is held to 2^-26, every
    # other row to 1e-12.
    atol = np.full(n, TOL)
    atol[0] = 2.0 ** -26
    for a in range(A):                                   # every action of every row, allowed or not
        acts = np.full(n, a)
        want = dist.log_prob(torch.as_tensor(acts)).numpy()
        got = ref.log_prob(acts)
        assert np.all(np.abs(got - want) <= atol + TOL * np.abs(want)), f"action {a}: {np.abs(got - want).max()}"
    np.testing.assert_allclose(ref.log_prob(np.zeros(n, dtype=np.int64))[0], -np.log(A), rtol=TOL)
    np.testing.assert_array_equal(ref.argmax, torch.where(tm, tl, torch.tensor(-1e8, dtype=torch.float64)).argmax(-1).numpy())
    assert ref.argmax[3] == 0 and ref.argmax[0] == 0
    assert np.isnan(ref.log_prob(np.full(n, -1))).all() and np.isnan(ref.log_prob(np.full(n, A))).all()


def test_restatement_sample_is_the_inverse_cdf_in_action_order():
    import torch
    mask, logits = _cases()
    n, A = mask.shape
    ref = cr.CategoricalRef(mask, logits)
    probs = torch.distributions.Categorical(logits=torch.where(torch.as_tensor(mask), torch.as_tensor(logits), torch.tensor(-1e8, dtype=torch.float64))).probs.numpy()
    cdf = np.cumsum(probs, axis=1)
    rng = np.random.default_rng(6)
    for u24 in (np.zeros(n, dtype=np.int64), np.full(n, 2 ** 24 - 1), rng.integers(0, 2 ** 24, n), rng.integers(0, 2 ** 24, n)):
        a = ref.sample(u24)
        u = u24 * 2.0 ** -24
        for i in range(n):
            if ref.K[i] == 0:
                assert a[i] == (int(u24[i]) * A) >> 24
                continue
            assert mask[i, a[i]]
            before = cdf[i, a[i]] - probs[i, a[i]]
            assert before - 1e-12 <= u[i] < cdf[i, a[i]] + 1e-12 or (a[i] == np.nonzero(mask[i])[0][-1] and u[i] >= before - 1e-12)
        lo, hi = ref.cdf_interval(a)
        ok = ref.K > 0
        assert np.all(lo[ok] <= hi[ok]) and np.all(np.abs(hi[ok] - cdf[np.arange(n)[ok], a[ok]]) < 1e-12)


def test_restatement_uniform_law_and_blank_rows():
    mask, _ = _cases()
    n, A = mask.shape
    ref = cr.CategoricalRef(mask, None)
    K = mask.sum(1)
    nz = K > 0
    np.testing.assert_allclose(ref.entropy[nz], np.log(K[nz]), rtol=TOL, atol=TOL)
    assert ref.entropy[0] == 0.0
    rng = np.random.default_rng(7)
    u24 = rng.integers(0, 2 ** 24, n)
    a = ref.sample(u24)
    for i in range(n):
        want = np.flatnonzero(mask[i])[(int(u24[i]) * int(K[i])) >> 24] if K[i] else (int(u24[i]) * A) >> 24
        assert a[i] == want
    lp = ref.log_prob(a)
    np.testing.assert_allclose(lp[nz], -np.log(K[nz]), rtol=TOL)
    np.testing.assert_allclose(lp[~nz], -np.log(A), rtol=TOL)
    first_off = np.array([int(np.flatnonzero(~mask[i])[0]) if not mask[i].all() else 0 for i in range(n)])
    off = nz & ~mask[np.arange(n), first_off]
    np.testing.assert_allclose(ref.log_prob(first_off)[off], -1e8 - np.log(K[off]), rtol=TOL)
    assert np.array_equal(cr.u24_of_uniforms(np.float32([0.0, 0.5, 0.99999994, 1.0, 2 ** -24])), [0, 2 ** 23, 2 ** 24 - 1, 2 ** 24 - 1, 1])


def test_philox_keying_matches_the_header_and_the_oracles_philox():
    from marlon_amd import engine
    from oracle.oracle import philox4x32_10
    text = open(os.path.join(REPO, "include", "mcbs.h")).read()
    m = re.search(r"#define MCBS_CATEGORICAL_PHILOX_DOMAIN\s+(0x[0-9A-Fa-f]+)u", text)
    assert m and int(m.group(1), 16) == cr.PHILOX_DOMAIN == engine.CATEGORICAL_PHILOX_DOMAIN != 0x5A17ACED
    assert "counter = (key_lo, key_hi, step_lo, step_hi)" in text and "key = (seed_lo ^ MCBS_CATEGORICAL_PHILOX_DOMAIN, seed_hi)" in text
    for name, val in (("SAMPLE", 0), ("ARGMAX", 1), ("EVALUATE", 2)):
        assert re.search(rf"#define MCBS_CATEGORICAL_{name}\s+{val}\b", text) and engine.CATEGORICAL_MODES[name.lower()] == val
    cases = [(0, 0, 0), (9, 5, 3), (0x123456789ABCDEF, (1 << 40) + 77, (1 << 33) + 5), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32)]
    for seed, row, step in cases:
        ctr, key = cr.philox_counter_key(seed, row, step)
        assert ctr == [row & 0xFFFFFFFF, row >> 32, step & 0xFFFFFFFF, step >> 32]
        assert key == [(seed & 0xFFFFFFFF) ^ cr.PHILOX_DOMAIN, seed >> 32]
        want = philox4x32_10(ctr, key)
        np.testing.assert_array_equal(cr.philox4x32_10([ctr], key)[0], want)
        assert cr.philox_u24(seed, [row], step)[0] == int(want[0]) >> 8
    rows = np.arange(1000, 1064)
    many = cr.philox_u24(17, rows, 4)
    for r in (0, 31, 63):
        ctr, key = cr.philox_counter_key(17, int(rows[r]), 4)
        assert many[r] == int(philox4x32_10(ctr, key)[0]) >> 8
    assert 0 <= many.min() and many.max() < 2 ** 24 and len(set(many.tolist())) > 60
