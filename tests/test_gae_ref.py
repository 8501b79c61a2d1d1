"""tests/gae_ref.py — the float32 restatement of Stable-Baselines3's GAE loop the GPU tests of mcbs_gae compare against, and its float64
twin — pinned without a GPU: a hand-worked case, bit equality with a torch CPU float32 loop of the same expressions, an error bound
against float64, the lambda = 1 and lambda = 0 special cases; then the C ABI of mcbs_gae as far as a GPU-less host can see it."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests.gae_ref import gae_f32, gae_f64

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F = np.float32


def _inputs(T, E, density, seed, bootstrap=False):
    rng = np.random.default_rng(seed)
    r = (5.0 * rng.standard_normal((T, E))).astype(F)
    v = (3.0 * rng.standard_normal((T, E))).astype(F)
    s = (rng.random((T, E)) < density).astype(np.uint8)
    lv = (3.0 * rng.standard_normal(E)).astype(F)
    ld = (rng.random(E) < max(density, 0.3) if density < 1 else np.ones(E, bool)).astype(np.uint8)
    b = None
    if bootstrap:
        b = np.where(rng.random((T, E)) < 0.1, 3.0 * rng.standard_normal((T, E)), 0.0).astype(F)
    return r, v, s, lv, ld, b


def test_hand_worked_case():
    """T = 3, E = 2, gamma = 0.5, lambda = 0.5 (every product exact in float32); env 1 starts a new episode at t = 1 and is done at the
    end, env 0 runs through and bootstraps from last_values."""
    r = np.array([[1, 2], [3, 4], [5, 6]], F)
    v = np.array([[8, 4], [2, 16], [4, 8]], F)
    s = np.array([[1, 1], [0, 1], [0, 0]], np.uint8)
    lv, ld = np.array([16, 99], F), np.array([0, 1], np.uint8)
    # env 0: t=2: delta = 5 + .5*16 - 4 = 9,  adv = 9
    #        t=1: delta = 3 + .5*4 - 2 = 3,   adv = 3 + .25*9 = 5.25
    #        t=0: delta = 1 + .5*2 - 8 = -6,  adv = -6 + .25*5.25 = -4.6875
    # env 1: t=2: done after it: delta = 6 - 8 = -2, adv = -2
    #        t=1: delta = 4 + .5*8 - 16 = -8, adv = -8 + .25*(-2) = -8.5
    #        t=0: step 1 starts an episode: delta = 2 - 4 = -2, adv = -2
    want = np.array([[-4.6875, -2], [5.25, -8.5], [9, -2]], F)
    adv, ret = gae_f32(r, v, s, lv, ld, 0.5, 0.5)
    assert adv.dtype == F and ret.dtype == F
    assert np.array_equal(adv, want) and np.array_equal(ret, want + v)
    a64, r64 = gae_f64(r, v, s, lv, ld, 0.5, 0.5)
    assert a64.dtype == np.float64 and np.array_equal(a64, want) and np.array_equal(r64, want + v)
    # the truncation bootstrap: env 0 truncated at t = 1 with a terminal value of 4 -> its reward there becomes 3 + .5*4 = 5
    b = np.zeros((3, 2), F)
    b[1, 0] = 4
    adv_b, _ = gae_f32(r, v, s, lv, ld, 0.5, 0.5, bootstrap=b)
    assert adv_b[1, 0] == F(7.25) and adv_b[0, 0] == F(-6 + 0.25 * 7.25) and np.array_equal(adv_b[:, 1], want[:, 1]) and adv_b[2, 0] == 9
    # any nonzero byte is a flag
    adv_f, _ = gae_f32(r, v, s * 255, lv, ld * 2, 0.5, 0.5)
    assert np.array_equal(adv_f, want)


def _torch_loop(r, v, s, lv, ld, gamma, lam, b):
    """The same expressions on torch CPU float32 tensors."""
    r, v, lv = torch.from_numpy(r.copy()), torch.from_numpy(v), torch.from_numpy(lv)
    s, ld = torch.from_numpy((s != 0).astype(F)), torch.from_numpy((ld != 0).astype(F))
    if b is not None:
        r = r + gamma * torch.from_numpy(b)
    T = r.shape[0]
    adv = torch.zeros_like(r)
    last = 0
    for t in reversed(range(T)):
        nnt, nv = (1.0 - ld, lv) if t == T - 1 else (1.0 - s[t + 1], v[t + 1])
        delta = r[t] + gamma * nv * nnt - v[t]
        last = delta + gamma * lam * nnt * last
        adv[t] = last
    return adv.numpy(), (adv + v).numpy()


@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)])
@pytest.mark.parametrize("bootstrap", [False, True])
def test_bit_equal_to_torch_cpu_float32(gamma, lam, bootstrap):
    for density in (0.0, 0.1, 1.0):
        r, v, s, lv, ld, b = _inputs(300, 7, density, seed=11, bootstrap=bootstrap)
        adv, ret = gae_f32(r, v, s, lv, ld, gamma, lam, bootstrap=b)
        tadv, tret = _torch_loop(r, v, s, lv, ld, gamma, lam, b)
        assert np.array_equal(adv.view(np.int32), tadv.view(np.int32)) and np.array_equal(ret.view(np.int32), tret.view(np.int32))


def _bound(T, r, v, adv64):
    return 8 * T * 2.0 ** -24 * (np.abs(r).max() + 2 * np.abs(v).max() + np.abs(adv64).max())


@pytest.mark.parametrize("T", [37, 300, 2048])
@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)])
def test_error_bound_against_float64(T, gamma, lam):
    """|gae_f32 - gae_f64| <= 8 T 2^-24 (max|r| + 2 max|v| + max|adv64|): each step adds a few roundings of terms no larger than the
    bracket, and the recurrence never amplifies them (gamma * lambda <= 1)."""
    for density in (0.0, 0.01, 0.1, 1.0):
        r, v, s, lv, ld, _ = _inputs(T, 5, density, seed=T)
        a32, r32 = gae_f32(r, v, s, lv, ld, gamma, lam)
        a64, r64 = gae_f64(r, v, s, lv, ld, gamma, lam)
        bound = _bound(T, r, v, a64)
        assert np.abs(a32 - a64).max() <= bound and np.abs(r32 - r64).max() <= bound, (density, np.abs(a32 - a64).max(), bound)


def test_lambda_one_is_the_discounted_return():
    T, E, gamma = 300, 5, 0.99
    r, v, s, lv, ld, _ = _inputs(T, E, 0.0, seed=5)
    ld[:] = 0
    adv, _ = gae_f32(r, v, s, lv, ld, gamma, 1.0)
    g = lv.astype(np.float64)
    want = np.zeros((T, E))
    for t in reversed(range(T)):
        g = r[t].astype(np.float64) + gamma * g
        want[t] = g
    a64, _ = gae_f64(r, v, s, lv, ld, gamma, 1.0)
    assert np.abs(adv.astype(np.float64) + v - want).max() <= _bound(T, r, v, a64)


def test_lambda_zero_is_the_td_error():
    T, E, gamma = 40, 6, 0.9
    r, v, s, lv, ld, _ = _inputs(T, E, 0.1, seed=6)
    adv, _ = gae_f32(r, v, s, lv, ld, gamma, 0.0)
    nv = np.concatenate([v[1:], lv[None]])
    nnt = F(1) - np.concatenate([s[1:], ld[None]]).astype(F)
    assert np.array_equal(adv, r + F(gamma) * nv * nnt - v)


# ---------------------------------------------------------------- the C ABI, as far as a GPU-less host sees it
def test_gae_io_mirror_matches_header():
    """mcbs_gae_io: the ctypes mirror has the header's members in the header's order with matching types, and the size they imply."""
    from marlon_amd._abi import GaeIO
    text = open(os.path.join(REPO, "include", "mcbs.h")).read()
    body = re.search(r"typedef struct mcbs_gae_io \{(.*?)\} mcbs_gae_io;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = re.findall(r"([\w ]+?\*?)\s*(\w+);", body)
    members = [(ty.strip(), n) for ty, n in members]
    assert len(members) == 18
    ctype = {"const float*": C.c_void_p, "const uint8_t*": C.c_void_p, "float*": C.c_void_p, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
             "double": C.c_double}
    assert [n for _, n in members] == [n for n, _ in GaeIO._fields_]
    assert [ctype[ty] for ty, _ in members] == [ty for _, ty in GaeIO._fields_]
    assert C.sizeof(GaeIO) == sum(C.sizeof(ctype[ty]) for ty, _ in members) == 144      # (every member is 8 bytes wide: no padding)


def test_gae_refuses_null_arguments_without_gpu():
    from marlon_amd import engine
    from marlon_amd._abi import GaeIO
    lib = engine.load_library()
    assert lib.mcbs_gae(None, None, None) == -1 and b"null" in lib.mcbs_last_error()
    assert lib.mcbs_gae(None, C.byref(GaeIO()), None) == -1 and b"mcbs_gae" in lib.mcbs_last_error()
    assert "mcbs_gae" in engine.EXPORTS


def test_rollout_module_imports_without_gpu():
    """Fresh interpreter: importing the buffer module pulls in neither torch nor the native library."""
    import subprocess
    code = ("import sys; import marlon_amd.rollout as r; assert 'torch' not in sys.modules; "
            "assert r.RolloutBatch._fields == ('index', 'observations', 'actions', 'old_values', 'old_log_prob', 'advantages', 'returns', "
            "'mask_bits'); assert callable(r.DeviceRolloutBuffer.compute_returns_and_advantage); print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
    from marlon_amd.wrappers import AttackerVecEnv
    assert callable(AttackerVecEnv.rollout_buffer)
