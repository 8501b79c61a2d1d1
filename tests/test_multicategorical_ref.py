"""Pins tests/multicategorical_ref.py (the fp64 restatement the GPU tests of the MultiDiscrete head compare against) to torch's fp64
composite — split -> Categorical per dimension -> log_prob.sum / entropy.sum — and to fp64 autograd, its Philox keying to a counter built
by hand, and the Python ABI layer to the two entry points and two constants of include/mcbs.h.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import multicategorical_ref as mr
from tests.categorical_ref import philox4x32_10

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _inputs(nvec, n=37, scale=4.0, seed=0):
    rng = np.random.default_rng(seed)
    A = sum(nvec)
    logits = rng.standard_normal((n, A)) * scale
    actions = np.stack([rng.integers(0, w, n) for w in nvec], axis=1).astype(np.int64)
    return logits, actions, rng.standard_normal(n), rng.standard_normal(n)


@pytest.mark.parametrize("name", [k for k in mr.NVECS if k != "wider_than_lds"])
def test_restatement_equals_the_fp64_composite(name):
    import torch
    nvec = mr.NVECS[name]
    logits, actions, g_lp, g_H = _inputs(nvec)
    ref = mr.MultiCategoricalRef(nvec, logits)
    lp, ent, grad = mr.composite(nvec, logits, actions, torch.float64, g_lp, g_H)
    assert np.abs(ref.log_prob(actions) - lp).max() <= 1e-12
    assert np.abs(ref.entropy - ent).max() <= 1e-12
    assert np.abs(ref.grad(actions, g_lp, g_H) - grad).max() <= 1e-12
    for a, b in ((g_lp, None), (None, g_H)):
        assert np.abs(ref.grad(actions, a, b) - mr.composite(nvec, logits, actions, torch.float64, a, b)[2]).max() <= 1e-12
    assert not ref.grad(actions).any()
    # the arg max is torch's per segment; a dimension of one choice contributes nothing
    parts = torch.split(torch.as_tensor(logits), nvec, dim=1)
    assert np.array_equal(ref.argmax, torch.stack([p.argmax(dim=1) for p in parts], dim=1).numpy())
    for d, w in enumerate(nvec):
        if w == 1:
            assert not ref.H[:, d].any() and not ref.logp[:, ref.off[d]].any() and not ref.grad(actions, g_lp, g_H)[:, ref.off[d]].any()


def test_ties_bad_actions_and_infinities():
    nvec = [3, 4, 1]
    x = np.zeros((3, 8))
    x[1, 3:7] = [-np.inf, 2.0, 2.0, -np.inf]
    ref = mr.MultiCategoricalRef(nvec, x)
    assert np.array_equal(ref.argmax, [[0, 0, 0], [0, 1, 0], [0, 0, 0]])            # the lowest index among equal logits
    assert np.allclose(ref.entropy, [np.log(3) + np.log(4), np.log(3) + np.log(2), np.log(3) + np.log(4)])
    lp = ref.log_prob([[0, 0, 0], [0, 4, 0], [-1, 0, 0]])
    assert np.isclose(lp[0], -np.log(12)) and np.isnan(lp[1]) and np.isnan(lp[2])
    g = ref.grad([[0, 0, 0], [2, 1, 0], [0, 0, 1]], np.ones(3), np.ones(3))
    assert np.isfinite(g).all() and not g[2].any() and g[1, 3] == 0.0 and g[1, 6] == 0.0 and not g[:, 7].any()


def test_sampling_and_intervals():
    nvec = [4, 1, 6]
    logits, *_ = _inputs(nvec, n=50, seed=3)
    logits[0, :4] = [-np.inf, 0.0, 0.0, -np.inf]
    ref = mr.MultiCategoricalRef(nvec, logits)
    rng = np.random.default_rng(4)
    u24 = rng.integers(0, 2 ** 24, (50, 3))
    u24[0], u24[1] = 0, 2 ** 24 - 1
    a = ref.sample(u24)
    assert ref.in_range(a).all() and not a[:, 1].any()
    lo, hi = ref.cdf_interval(a)
    u = u24 * 2.0 ** -24
    assert ((lo <= u) & (u < hi) | (a == np.asarray(nvec) - 1) & (u >= hi)).all()
    assert a[0, 0] == 1 and a[1, 2] == 5                 # the first / last index with nonzero probability
    uni = mr.MultiCategoricalRef(nvec, None, n=50)
    assert np.array_equal(uni.sample(u24), (u24 * np.asarray(nvec)) >> 24)
    assert np.allclose(uni.entropy, np.log(24)) and np.allclose(uni.log_prob(uni.sample(u24)), -np.log(24))
    assert np.array_equal(mr.u24_of_uniforms([0.0, 0.5, 1.0 - 2.0 ** -24, 1.0]), [0, 2 ** 23, 2 ** 24 - 1, 2 ** 24 - 1])


def test_philox_keying_against_a_counter_built_by_hand():
    seed, step = 0x0123456789ABCDEF, (1 << 47) + 12345
    keys = np.array([0, 7, 2 ** 32 + 5], dtype=np.uint64)
    got = mr.philox_u24(seed, keys, step, 16)
    assert got.shape == (3, 16) and (got >= 0).all() and (got < 2 ** 24).all()
    for d in (0, 3, 4, 15):
        for j, k in enumerate(int(v) for v in keys):
            ctr = [k & 0xFFFFFFFF, k >> 32, step & 0xFFFFFFFF, (step >> 32) | ((d // 4) << 16)]
            key = [(seed & 0xFFFFFFFF) ^ 0x3C47E6A1, seed >> 32]
            assert (ctr, key) == mr.philox_counter_key(seed, k, step, d)
            assert got[j, d] == int(philox4x32_10([ctr], key)[0, d % 4]) >> 8
    assert len({tuple(r) for r in got.T}) == 16          # sixteen dimensions, sixteen different numbers per row
    assert mr.PHILOX_DOMAIN not in (0xCA7E6041, 0x5A17ACED)


def test_abi_declares_the_entry_points_and_constants():
    """The header's two constants and two prototypes as the Python layer states them (fails before the MultiDiscrete head exists)."""
    import ctypes as C

    from marlon_amd import _abi, engine
    text = open(os.path.join(REPO, "include", "mcbs.h")).read()
    assert _abi.MCBS_MAX_ACTION_DIMS == int(re.search(r"#define MCBS_MAX_ACTION_DIMS (\d+)", text).group(1)) == mr.MAX_DIMS
    assert _abi.MCBS_MULTICATEGORICAL_PHILOX_DOMAIN == int(re.search(r"#define MCBS_MULTICATEGORICAL_PHILOX_DOMAIN (0x[0-9A-Fa-f]+)u", text).group(1), 16) \
        == mr.PHILOX_DOMAIN
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    ctype = {"const mcbs_batch*": C.c_void_p, "const uint32_t*": C.POINTER(C.c_uint32), "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
             "const void*": C.c_void_p, "int32_t": C.c_int32, "size_t": C.c_size_t, "int64_t*": C.c_void_p, "const int64_t*": C.c_void_p,
             "float*": C.c_void_p, "const float*": C.c_void_p, "uint32_t*": C.c_void_p, "void*": C.c_void_p}
    for name in ("mcbs_multicategorical", "mcbs_multicategorical_grad"):
        restype, argtypes = _abi.PROTOTYPES[name]
        assert restype is C.c_int
        params = re.search(r"int\s+%s\((.*?)\);" % name, code, flags=re.S).group(1)
        declared = [" ".join(p.split()[:-1]) if len(p.split()) > 1 and not p.split()[-1].endswith("*") else " ".join(p.split())
                    for p in params.split(",")]
        assert [ctype[t] for t in declared] == argtypes, name
        assert name in engine.EXPORTS
    lib = engine.load_library()
    assert lib.mcbs_multicategorical.argtypes == _abi.PROTOTYPES["mcbs_multicategorical"][1]
    # refusals that need no GPU: a null batch
    assert lib.mcbs_multicategorical(None, None, 0, 0, None, 0, 0, 0, None, None, None, None, 0, 0, 0, None, None) == -1
    assert b"batch" in lib.mcbs_last_error()
    assert lib.mcbs_multicategorical_grad(None, None, 0, 0, None, 0, 0, None, None, None, None, 0, None) == -1
