"""The host mirrors of the first layer from the observation (include/mcbs.h "first layer from the observation"):
FeatureLayout.first_layer_host / first_layer_grad_host of marlon_amd/features.py, on observations the CPU oracle produced.

Yardstick: `restate` of tests/test_feature_layout.py (torch one_hot per element, cat) followed by a float64 matmul, and torch's float64
autograd of torch.nn.functional.linear on those one-hot rows.  The mirrors sum in float32 in the contract's fixed order, so they differ
from float64 by rounding only:
  forward   m = n_elements float32 additions in one chain: |got - want| <= gamma_m * (|b| + sum |w_selected|), gamma_m = m u / (1 - m u),
            u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2; the bound holds for any order of the sum)
  gradient  a column's sum has as many terms as rows select it: the additions that start a block at +0.0, and those of an empty block's
            partial, are exact, so at most m - 1 round; the bound is taken with m = the rows that select the column (all rows: the bias)
On integer weights / gradients in [-8, 8] every partial sum is an integer far below 2^24: every order gives the same float, and the
comparison is bitwise."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from marlon_amd.features import FeatureLayout
from marlon_amd.samples import chainpattern, toy_ctf
from tests.test_feature_layout import ARRAYS, dims, key_classes, public_obs, restate, stepped_observation

U = 2.0 ** -24
CASES = {"chain10": (12, 12), "toyctf": (12, 10)}
_cache = {}


def gamma(m):
    m = np.asarray(m, dtype=np.float64)
    return m * U / (1.0 - m * U)


def observation(name):
    """(topo, spec, the oracle's fields, the wrapper's keys) after 60 valid random steps of 8 envs, made once"""
    if name not in _cache:
        N, C = CASES[name]
        env = chainpattern.new_environment(10) if name == "chain10" else toy_ctf.new_environment()
        topo, spec, oo = stepped_observation(env, N, C, 60)
        obs = public_obs(oo)
        assert obs["discovered_node_count"].max() > 1 and (oo["nodes_privilegelevel"] > 0).any()      # the run left the reset state
        _cache[name] = (topo, spec, {k: oo[k] for k in ["scalars"] + ARRAYS}, obs)
    return _cache[name]


def one_hot_rows(topo, spec, obs, reference_counts=False):
    """-> (float64 [n, F] one-hot rows by the restatement, its out-of-range count)"""
    classes, mask_sizes = key_classes(*dims(topo, spec), reference_counts)
    x, bad = restate(obs, classes, mask_sizes, sorted(classes))
    return x.double().numpy(), bad


def weights(F, H, seed, exact):
    rng = np.random.default_rng(seed)
    if exact:
        return rng.integers(-8, 9, (F, H)).astype(np.float32), rng.integers(-8, 9, H).astype(np.float32)
    return rng.standard_normal((F, H)).astype(np.float32), rng.standard_normal(H).astype(np.float32)


@pytest.mark.parametrize("H", [1, 3, 64])
@pytest.mark.parametrize("name", ["chain10", "toyctf"])
def test_first_layer_host_equals_the_float64_restatement(name, H):
    topo, spec, fields, obs = observation(name)
    lay = FeatureLayout(topo, spec)
    x, bad = one_hot_rows(topo, spec, obs)
    assert bad == 0 and x.shape[1] == lay.width and (x.sum(axis=1) == lay.n_elements).all()
    w, b = weights(lay.width, H, 1, exact=False)
    want = x @ w.astype(np.float64) + b.astype(np.float64)
    bound = gamma(lay.n_elements) * (x @ np.abs(w).astype(np.float64) + np.abs(b).astype(np.float64))
    for o in (obs, fields):                                          # the wrapper's keys and the engine's fields encode alike
        got, got_bad = lay.first_layer_host(o, w, b, return_out_of_range=True)
        assert got.dtype == np.float32 and got.shape == want.shape and got_bad == 0
        err = np.abs(got.astype(np.float64) - want)
        print(f"{name} H={H}: max error {err.max():.3e}, smallest bound {bound.min():.3e}")
        assert (err <= bound).all()
    # without a bias the chain starts at +0.0
    got0 = lay.first_layer_host(obs, w)
    assert (np.abs(got0.astype(np.float64) - x @ w.astype(np.float64)) <= gamma(lay.n_elements) * (x @ np.abs(w).astype(np.float64))).all()
    # exact inputs: bitwise, also against torch's float32 linear
    w, b = weights(lay.width, H, 2, exact=True)
    want = (x @ w.astype(np.float64) + b.astype(np.float64)).astype(np.float32)
    got = lay.first_layer_host(obs, w, b)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    lin = TF.linear(torch.from_numpy(x).float(), torch.from_numpy(w).t().contiguous(), torch.from_numpy(b)).numpy()
    assert np.array_equal(got.view(np.uint32), lin.view(np.uint32))


def test_bfloat16_rounding_is_torchs():
    topo, spec, fields, obs = observation("chain10")
    lay = FeatureLayout(topo, spec)
    w, b = weights(lay.width, 16, 3, exact=False)
    w = torch.from_numpy(w).bfloat16().float().numpy()               # bfloat16 weights as the float32 values they widen to
    f32 = lay.first_layer_host(obs, w, b)
    bf = lay.first_layer_host(obs, w, b, out_dtype="bfloat16")
    assert bf.dtype == np.float32 and np.array_equal(bf, torch.from_numpy(f32).bfloat16().float().numpy())
    assert not np.array_equal(bf, f32)
    with pytest.raises(ValueError, match="out_dtype"):
        lay.first_layer_host(obs, w, b, out_dtype=np.float16)
    # ties go to even, a NaN stays a NaN
    from marlon_amd.features import _round_to_bfloat16
    ties = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x7FC00001, 0xFF800000], dtype=np.uint32).view(np.float32)
    assert np.array_equal(_round_to_bfloat16(ties).view(np.uint32)[:3], np.array([0x3F800000, 0x3F820000, 0x3F810000], dtype=np.uint32))
    assert np.isnan(_round_to_bfloat16(ties)[3]) and _round_to_bfloat16(ties)[4] == -np.inf


@pytest.mark.parametrize("name", ["chain10", "toyctf"])
def test_first_layer_grad_host_equals_float64_autograd(name):
    topo, spec, fields, obs = observation(name)
    lay = FeatureLayout(topo, spec)
    x8, _ = one_hot_rows(topo, spec, obs)
    index = np.array([(5 * i + i // 8) % 8 for i in range(21)])       # 21 rows of the 8: blocks of 4 leave a short last block
    x = x8[index]
    H, F, n = 5, lay.width, len(index)
    for exact in (False, True):
        rng = np.random.default_rng(7)
        g = rng.integers(-8, 9, (n, H)).astype(np.float32) if exact else rng.standard_normal((n, H)).astype(np.float32)
        wt = torch.zeros((H, F), dtype=torch.float64, requires_grad=True)
        bt = torch.zeros(H, dtype=torch.float64, requires_grad=True)
        TF.linear(torch.from_numpy(x), wt, bt).backward(torch.from_numpy(g).double())
        want_w, want_b = wt.grad.t().numpy(), bt.grad.numpy()
        for row_block in (4, 512):
            got_w, got_b = lay.first_layer_grad_host(obs, g, H, row_block=row_block, index=index)
            assert got_w.dtype == got_b.dtype == np.float32 and got_w.shape == (F, H) and got_b.shape == (H,)
            if exact:
                assert np.array_equal(got_w.view(np.uint32), want_w.astype(np.float32).view(np.uint32))
                assert np.array_equal(got_b.view(np.uint32), want_b.astype(np.float32).view(np.uint32))
                continue
            rows_per_column = x.sum(axis=0)                          # m of every column
            bound_w = gamma(rows_per_column)[:, None] * (x.T @ np.abs(g).astype(np.float64))
            assert (np.abs(got_w.astype(np.float64) - want_w) <= bound_w).all()
            assert (np.abs(got_b.astype(np.float64) - want_b) <= gamma(n) * np.abs(g).astype(np.float64).sum(axis=0)).all()
            unselected = rows_per_column == 0
            assert unselected.any() and not got_w[unselected].any() and not np.signbit(got_w[unselected]).any()       # exactly +0.0
        # the dense form: no index, the 8 rows themselves
        got_w, got_b = lay.first_layer_grad_host(fields, g[:8], H, row_block=3)
        wt.grad = bt.grad = None
        TF.linear(torch.from_numpy(x8), wt, bt).backward(torch.from_numpy(g[:8]).double())
        g8 = np.abs(g[:8]).astype(np.float64)
        assert (np.abs(got_w.astype(np.float64) - wt.grad.t().numpy()) <= gamma(x8.sum(axis=0))[:, None] * (x8.T @ g8)).all()
        assert (np.abs(got_b.astype(np.float64) - bt.grad.numpy()) <= gamma(8) * g8.sum(axis=0)).all()
    with pytest.raises(ValueError, match="grad_out"):
        lay.first_layer_grad_host(obs, g, H + 1)


def test_single_terms_and_negative_zero():
    """a sum with one term is that term added to +0.0: -0.0 comes out as +0.0; a -0.0 bias stays -0.0 where nothing is added to it"""
    topo, spec, fields, obs = observation("chain10")
    lay = FeatureLayout(topo, spec)
    g = np.full((8, 2), -0.0, dtype=np.float32)
    gw, gb = lay.first_layer_grad_host(obs, g, 2)
    assert not np.signbit(gw).any() and not np.signbit(gb).any() and not gw.any()
    out = lay.first_layer_host(obs, np.zeros((lay.width, 2), np.float32), np.full(2, -0.0, np.float32), index=np.array([-1, 8]))
    assert np.signbit(out).all()                                     # rows outside the storage: the bias alone


def test_out_of_range_values_and_index_rows():
    topo, spec, oo = stepped_observation(chainpattern.new_environment(10), 12, 12, 40, E=4)
    N = 12
    obs = {k: np.array(v) for k, v in public_obs(oo).items()}
    obs["discovered_node_count"][0] = N                      # the full count: class N of N + 1, beyond Discrete(N)
    obs["nodes_privilegelevel"][1, 3] = -1                   # negative
    obs["credential_cache_matrix"][2, 5] = 1000              # too large
    obs["leaked_credentials"][3, 1] = 12                     # cache index C of Discrete(C)
    for reference_counts, bad_want in ((True, 4), (False, 3)):
        lay = FeatureLayout(topo, spec, reference_counts=reference_counts)
        x, bad = one_hot_rows(topo, spec, obs, reference_counts)
        assert bad == bad_want
        w, b = weights(lay.width, 4, 5, exact=True)
        got, got_bad = lay.first_layer_host(obs, w, b, return_out_of_range=True)
        assert got_bad == bad_want
        assert np.array_equal(got, (x @ w.astype(np.float64) + b).astype(np.float32))      # an out-of-range element adds nothing
        # rows through an index; -1 and 4 lie outside the 4 stored rows: the bias alone, every element counted
        index = np.array([3, -1, 0, 4, 3])
        got, got_bad = lay.first_layer_host(obs, w, b, index=index, return_out_of_range=True)
        inside = np.array([True, False, True, False, True])
        per_row = lay.n_elements - x.sum(axis=1)                     # out-of-range elements of every stored row
        assert got_bad == 2 * lay.n_elements + int(per_row[[3, 0, 3]].sum())
        assert np.array_equal(got[inside], (x[[3, 0, 3]] @ w.astype(np.float64) + b).astype(np.float32))
        assert np.array_equal(got[~inside], np.broadcast_to(b, (2, 4)))
        assert np.array_equal(lay.first_layer_host(obs, w, None, index=index)[~inside], np.zeros((2, 4), np.float32))
        # the gradient: rows outside the storage reach grad_bias only
        g = np.random.default_rng(9).integers(-8, 9, (5, 4)).astype(np.float32)
        gw, gb = lay.first_layer_grad_host(obs, g, 4, row_block=2, index=index)
        assert np.array_equal(gb, g.sum(axis=0)) and np.array_equal(gw, (x[[3, 0, 3]].T @ g[inside].astype(np.float64)).astype(np.float32))


def test_layouts_with_mask_columns_are_refused():
    topo, spec, fields, obs = observation("chain10")
    lay = FeatureLayout(topo, spec, include_masks=True)
    with pytest.raises(ValueError, match="include_masks"):
        lay.first_layer_host(obs, np.zeros((lay.width, 2), np.float32))
    with pytest.raises(ValueError, match="include_masks"):
        lay.first_layer_grad_host(obs, np.zeros((8, 2), np.float32), 2)
    with pytest.raises(ValueError, match="weight_t"):
        FeatureLayout(topo, spec).first_layer_host(obs, np.zeros((3, 2), np.float32))
