"""mcbs_first_layer_grad (include/mcbs.h "first layer from the observation", marlon_amd/csrc/mcbs_first_layer.hip) through
BatchEngine.first_layer_grad and the autograd node behind AttackerVecEnv.encode_first_layer[_packed](differentiable=True).

Yardstick: FeatureLayout.first_layer_grad_host — NumPy float32, block partials of 512 rows in ascending row order, added in ascending
block order — which tests/test_first_layer_ref.py holds to torch's float64 autograd; the kernel states the same order, so the comparison
is bit for bit.  Against float64 autograd of torch.nn.functional.linear on the one-hot rows the bound is gamma_m * sum |g| with m = the
rows that select the column (all rows: the bias), gamma_m = m u / (1 - m u), u = 2^-24: at most m - 1 of a column's additions round."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_features import expected
from tests.test_gpu_first_layer import SENTINEL, Envs, bits, case, params

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
HS = [1, 3, 64, 65, 200]
NS = [1, 511, 512, 513, 1100]


@pytest.fixture(scope="module", autouse=True)
def _close_envs():
    yield
    for env in Envs.cache.values():
        env.close()
    Envs.cache.clear()
    Envs.data.clear()


def repeating_index(E, n, seed):
    """n rows over the E stored ones: every row is used, in no order"""
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.randperm(E, generator=g), torch.randint(0, E, (max(n - E, 0),), generator=g)])[:n]


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("name", ["chain10", "toyctf"])
def test_gradients_equal_host_mirror(name, H):
    """grad_weight_t and grad_bias, each alone and together, for row counts around the block length, from the packed source through a
    repeating index and from the dense source on the gathered rows: the host mirror's bits; columns no row selects are exactly +0.0."""
    import torch
    env, fields, host, lay, packed = case(name)
    eng, h, pk = env.engine, env._feature_handle(False, False), env._packing_handle()
    E, F = env.num_envs, lay.width
    for n in NS:
        idx = repeating_index(E, n, n + H)
        g = torch.randn((n, H), generator=torch.Generator().manual_seed(n))
        want_w, want_b = lay.first_layer_grad_host(host, g.numpy(), H, index=idx.numpy())
        gd, idxd = g.to(eng.device), idx.to(eng.device)
        ctx = f"{name} H={H} n={n}"
        both = eng.first_layer_grad(h, gd, packing=pk, packed=packed, index=idxd)
        assert tuple(both.grad_weight_t.shape) == (F, H) and tuple(both.grad_bias.shape) == (H,), ctx
        assert np.array_equal(bits(both.grad_weight_t), bits(want_w)), ctx + " grad_weight_t"
        assert np.array_equal(bits(both.grad_bias), bits(want_b)), ctx + " grad_bias"
        only_w = eng.first_layer_grad(h, gd, packing=pk, packed=packed, index=idxd, want=(True, False))
        only_b = eng.first_layer_grad(h, gd, packing=pk, packed=packed, index=idxd, want=(False, True))
        assert only_w.grad_bias is None and only_b.grad_weight_t is None
        assert torch.equal(only_w.grad_weight_t, both.grad_weight_t) and torch.equal(only_b.grad_bias, both.grad_bias), ctx
        gathered = {k: v[idxd].contiguous() for k, v in fields.items()}
        dense = eng.first_layer_grad(h, gd, obs=gathered)
        assert torch.equal(dense.grad_weight_t, both.grad_weight_t) and torch.equal(dense.grad_bias, both.grad_bias), ctx + " dense"
        unselected = torch.as_tensor(want_w == 0).all(dim=1)
        assert bool(unselected.any()) and not bits(both.grad_weight_t)[unselected.numpy()].any(), ctx + ": an unselected column is not +0.0"


@pytest.mark.parametrize("name", ["chain10", "toyctf"])
def test_gradients_against_float64_autograd(name):
    import torch
    import torch.nn.functional as TF
    env, fields, host, lay, packed = case(name)
    eng, h, pk = env.engine, env._feature_handle(False, False), env._packing_handle()
    E, F, H, n = env.num_envs, lay.width, 64, 1100
    idx = repeating_index(E, n, 3)
    x = expected(env.topo, env.spec, fields)[0].double()[idx]        # the one-hot rows, by the restatement
    g = torch.randn((n, H), generator=torch.Generator().manual_seed(8))
    w = torch.zeros((H, F), dtype=torch.float64, requires_grad=True)
    b = torch.zeros(H, dtype=torch.float64, requires_grad=True)
    TF.linear(x, w, b).backward(g.double())
    got = eng.first_layer_grad(h, g.to(eng.device), packing=pk, packed=packed, index=idx.to(eng.device))
    m = x.sum(dim=0)
    bound_w = (m * U / (1 - m * U)).unsqueeze(1) * (x.t() @ g.double().abs())
    err_w = (got.grad_weight_t.double().cpu() - w.grad.t()).abs()
    err_b = (got.grad_bias.double().cpu() - b.grad).abs()
    bound_b = n * U / (1 - n * U) * g.double().abs().sum(dim=0)
    print(f"{name}: grad_weight_t max error {float(err_w.max()):.3e}, grad_bias max error {float(err_b.max()):.3e} (bound min {float(bound_b.min()):.3e})")
    assert bool((err_w <= bound_w).all()) and bool((err_b <= bound_b).all())
    # integer gradients: every order gives the same float
    gi = torch.randint(-8, 9, (n, H), generator=torch.Generator().manual_seed(9)).float()
    w.grad = b.grad = None
    TF.linear(x, w, b).backward(gi.double())
    got = eng.first_layer_grad(h, gi.to(eng.device), packing=pk, packed=packed, index=idx.to(eng.device))
    assert torch.equal(got.grad_weight_t.cpu(), w.grad.t().float()) and torch.equal(got.grad_bias.cpu(), b.grad.float())


def test_write_discipline():
    """Write-only outputs with padded strides in poisoned buffers, a poisoned and an oversized workspace, two calls: the same bits, and
    nothing past H or outside the rows is touched.  Rows outside the storage reach grad_bias only; no rows at all: +0.0 everywhere."""
    import torch
    env, fields, host, lay, packed = case("chain10")
    eng, h, pk = env.engine, env._feature_handle(False, False), env._packing_handle()
    E, F, H, n = env.num_envs, lay.width, 65, 700
    idx = repeating_index(E, n, 1)
    idx[5], idx[600] = -1, E                                         # two rows outside the storage
    g = torch.randn((n, H), generator=torch.Generator().manual_seed(2))
    want_w, want_b = lay.first_layer_grad_host(host, g.numpy(), H, index=idx.numpy())
    gd, idxd = g.to(eng.device), idx.to(eng.device)
    gpad = torch.full((n, H + 3), SENTINEL, dtype=torch.float32, device=eng.device)
    gpad[:, :H] = gd
    need = eng.first_layer_grad_workspace(h, n, H)
    assert need == 2 * (F + 1) * H * 4
    for poison in (float("nan"), -1e30):
        ws = torch.empty(need + 64, dtype=torch.uint8, device=eng.device)
        ws.view(torch.float32).fill_(poison)
        gw = torch.full((F + 2, H + 7), poison, dtype=torch.float32, device=eng.device)
        gb = torch.full((H,), poison, dtype=torch.float32, device=eng.device)
        r = eng.first_layer_grad(h, gpad[:, :H], packing=pk, packed=packed, index=idxd, out=(gw[1:F + 1, :H], gb), workspace=ws)
        assert r.grad_weight_t.data_ptr() == gw[1].data_ptr() and r.grad_bias.data_ptr() == gb.data_ptr()
        assert np.array_equal(bits(r.grad_weight_t), bits(want_w)) and np.array_equal(bits(gb), bits(want_b))
        rest = torch.ones_like(gw, dtype=torch.bool)
        rest[1:F + 1, :H] = False
        left = gw[rest]
        assert bool(torch.isnan(left).all()) if poison != poison else bool((left == poison).all())
    again = eng.first_layer_grad(h, gd, packing=pk, packed=packed, index=idxd)
    assert np.array_equal(bits(again.grad_weight_t), bits(want_w)) and np.array_equal(bits(again.grad_bias), bits(want_b))
    # the bias sums every row, the weights only those inside the storage
    inside = ((idx >= 0) & (idx < E))
    assert np.array_equal(bits(again.grad_bias), bits(lay.first_layer_grad_host(host, g.numpy(), H, index=idx.clamp(0, E - 1).numpy())[1]))
    assert not np.array_equal(bits(want_w), bits(lay.first_layer_grad_host(host, g.numpy(), H, index=idx.clamp(0, E - 1).numpy())[0]))
    assert int(inside.sum()) == n - 2
    # no rows
    none = eng.first_layer_grad(h, gd[:0], packing=pk, packed=packed, index=idxd[:0])
    assert eng.first_layer_grad_workspace(h, 0, H) == 0
    assert not bits(none.grad_weight_t).any() and not bits(none.grad_bias).any() and tuple(none.grad_weight_t.shape) == (F, H)


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_autograd_end_to_end(dtype_name):
    """encode_first_layer_packed(differentiable=True), a scalar loss and .backward(): weight.grad [H, F] and bias.grad [H] in the
    parameters' dtype equal the direct calls; the dense form likewise; the forward's bits are the plain call's."""
    import torch
    env, fields, host, lay, packed = case("toyctf")
    eng, h, pk = env.engine, env._feature_handle(False, False), env._packing_handle()
    dtype = getattr(torch, dtype_name)
    E, F, H, n = env.num_envs, lay.width, 64, 600
    idx = repeating_index(E, n, 4).to(eng.device)
    wt, b, _, _ = params(env, F, H, dtype, 21)
    weight = wt.t().contiguous().requires_grad_(True)                # torch's Linear.weight [H, F]
    bias = b.clone().requires_grad_(True)
    coef = torch.randn((n, H), generator=torch.Generator().manual_seed(6)).to(eng.device)
    out = env.encode_first_layer_packed(packed, weight, bias, index=idx, differentiable=True)
    assert out.requires_grad and out.dtype == torch.float32 and tuple(out.shape) == (n, H)
    assert torch.equal(out.detach(), env.encode_first_layer_packed(packed, weight, bias, index=idx))
    (out * coef).sum().backward()
    direct = eng.first_layer_grad(h, coef, packing=pk, packed=packed, index=idx)
    assert weight.grad.dtype == dtype and tuple(weight.grad.shape) == (H, F) and bias.grad.dtype == dtype and tuple(bias.grad.shape) == (H,)
    assert torch.equal(weight.grad, direct.grad_weight_t.t().to(dtype)) and torch.equal(bias.grad, direct.grad_bias.to(dtype))
    # an output in the parameters' dtype sends a gradient of that dtype back: cast to float32 before the kernel
    weight.grad = bias.grad = None
    out = env.encode_first_layer_packed(packed, weight, bias, index=idx, dtype=dtype, differentiable=True, weight_t=wt)
    assert out.dtype == dtype
    (out.float() * coef).sum().backward()
    direct = eng.first_layer_grad(h, coef.to(dtype).float(), packing=pk, packed=packed, index=idx)
    assert torch.equal(weight.grad, direct.grad_weight_t.t().to(dtype)) and torch.equal(bias.grad, direct.grad_bias.to(dtype))
    # the dense form, without a bias; only the weight asks for a gradient
    weight.grad = None
    gathered = {k: v[idx].contiguous() for k, v in fields.items()}
    out = env.encode_first_layer(gathered, weight, None, differentiable=True)
    (out * coef).sum().backward()
    direct = eng.first_layer_grad(h, coef, obs=gathered, want=(True, False))
    assert torch.equal(weight.grad, direct.grad_weight_t.t().to(dtype))
    # torch's own composite on the feature rows agrees to rounding (float32 parameters: the bound of the float64 test, twice over)
    if dtype == torch.float32:
        w2 = weight.detach().clone().requires_grad_(True)
        x = env.encode_features_packed(packed, index=idx)
        (torch.nn.functional.linear(x, w2) * coef).sum().backward()
        m = x.sum(dim=0).double()
        bound = 2 * (m * U / (1 - m * U)).unsqueeze(0) * (coef.double().abs().t() @ x.double())
        assert bool(((w2.grad.double() - weight.grad.double()).abs() <= bound).all())


def test_refusals():
    import torch
    from marlon_amd._abi import ObsBuffers
    env, fields, host, lay, packed = case("chain10")
    eng, lib = env.engine, env.engine.lib
    h, hm, pk = env._feature_handle(False, False), env._feature_handle(True, False), env._packing_handle()
    E, F, H = env.num_envs, lay.width, 16
    g = torch.randn((E, H), device=eng.device)
    gw = torch.full((F, H), SENTINEL, dtype=torch.float32, device=eng.device)
    gb = torch.full((H,), SENTINEL, dtype=torch.float32, device=eng.device)
    need = eng.first_layer_grad_workspace(h, E, H)
    ws = torch.zeros(need, dtype=torch.uint8, device=eng.device)
    ob = ObsBuffers(**{k: v.data_ptr() for k, v in fields.items()})
    st = eng._stream()

    def call(handle=h, obs=None, packing=pk.ptr, p=packed.data_ptr(), words=packed.stride(0), index=None, m=E, n=E, go=g.data_ptr(), gs=H, hh=H,
             w=gw.data_ptr(), wstride=H, bias=gb.data_ptr(), work=ws.data_ptr(), wbytes=need):
        return lib.mcbs_first_layer_grad(eng._h, handle.ptr, obs, packing, p, words, index, m, n, go, gs, hh, w, wstride, bias, work, wbytes, st)

    def refused(rc, word):
        assert rc == -1 and word in lib.mcbs_last_error(), (rc, lib.mcbs_last_error())

    refused(call(handle=hm), b"include_masks")
    refused(call(hh=0), b"H 0")
    refused(call(hh=513), b"H 513")
    refused(call(gs=H - 1), b"grad_out_row_stride")
    refused(call(wstride=H - 1), b"grad_weight_row_stride")
    refused(call(w=None, bias=None), b"both NULL")
    refused(call(go=None), b"grad_out")
    refused(call(obs=C.byref(ob)), b"either obs")
    refused(call(packing=None, p=None), b"either obs")
    refused(call(p=None), b"NULL")
    refused(call(words=pk.words - 1), b"packed_row_words")
    refused(call(m=E - 1), b"no index")
    refused(call(work=None), b"workspace")
    refused(call(wbytes=need - 1), b"workspace")
    refused(call(w=g.data_ptr()), b"overlaps")
    refused(call(bias=g.data_ptr()), b"overlaps")
    refused(call(work=packed.data_ptr()), b"overlaps")
    refused(call(bias=gw.data_ptr()), b"overlaps")
    refused(call(w=ws.data_ptr()), b"overlaps")
    refused(call(handle=Envs.get("toyctf")._feature_handle(False, False)), b"geometry")
    assert lib.mcbs_first_layer_grad_workspace(eng._h, hm.ptr, E, H) == 0 and lib.mcbs_first_layer_grad_workspace(eng._h, h.ptr, E, 513) == 0
    assert lib.mcbs_first_layer_grad_workspace(None, h.ptr, E, H) == 0
    torch.cuda.synchronize()
    assert bool((gw == SENTINEL).all()) and bool((gb == SENTINEL).all())
    assert call() == 0 and call(obs=C.byref(ob), packing=None, p=None, words=0, m=0) == 0
    torch.cuda.synchronize()
    assert not bool((gw == SENTINEL).any())
    # the Python layer
    with pytest.raises(ValueError, match="mask columns"):
        eng.first_layer_grad(hm, g, obs=fields)
    with pytest.raises(ValueError, match="grad_out"):
        eng.first_layer_grad(h, g.double(), obs=fields)
    with pytest.raises(ValueError, match="grad_out"):
        eng.first_layer_grad(h, g[:-1], obs=fields)
    with pytest.raises(ValueError, match="no gradient"):
        eng.first_layer_grad(h, g, obs=fields, want=(False, False))
    with pytest.raises(ValueError, match="workspace"):
        eng.first_layer_grad(h, g, obs=fields, workspace=ws[:-1])
    with pytest.raises(ValueError, match="grad_weight_t"):
        eng.first_layer_grad(h, g, obs=fields, out=(gw[:-1], None))
    with pytest.raises(ValueError, match="grad_bias"):
        eng.first_layer_grad(h, g, obs=fields, out=(None, gb[:-1]))
