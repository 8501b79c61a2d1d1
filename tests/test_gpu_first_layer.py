"""mcbs_first_layer / mcbs_first_layer_packed (include/mcbs.h "first layer from the observation", marlon_amd/csrc/mcbs_first_layer.hip)
through BatchEngine.first_layer and AttackerVecEnv.first_layer / encode_first_layer / encode_first_layer_packed.

Yardstick: FeatureLayout.first_layer_host — NumPy float32, one accumulator per output, the elements in row order — which
tests/test_first_layer_ref.py holds to a float64 restatement.  The kernel states the same order, so every comparison with it is bit
for bit; on integer weights in [-8, 8] every order gives the same float and torch.nn.functional.linear on features() is the yardstick."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_features import BOUNDS, FIELDS, Stepped, _environment, assert_left_reset_state, expected, host_obs

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
HS = [1, 3, 64, 65, 200, 512]
NS = [1, 63, 64, 65, 320]


class Envs(Stepped):
    """the 320 envs stepped 300 times of tests/test_gpu_features.py, a cache of this module's own"""
    cache = {}
    data = {}


@pytest.fixture(scope="module", autouse=True)
def _close_envs():
    yield
    for env in Envs.cache.values():
        env.close()
    Envs.cache.clear()
    Envs.data.clear()


def case(name):
    """-> (env, device fields, the same on the host under the wrapper's keys, layout, packed rows [E, W_obs]); every field has left its
    reset state"""
    if name not in Envs.data:
        env = Envs.get(name)
        fields = {k: env._obs[k] for k in FIELDS}
        want, bad, where = expected(env.topo, env.spec, fields)
        assert bad == 0
        assert_left_reset_state(want, where)
        Envs.data[name] = (env, fields, host_obs(fields)[0], env.feature_layout(), env.observation_packed().clone())
    return Envs.data[name]


def params(env, F, H, dtype, seed, exact=False, bias=True):
    """-> (weight_t [F, H] and bias [H] on the device in `dtype`, the float32 values they hold on the host)"""
    import torch
    g = torch.Generator().manual_seed(seed)
    if exact:
        w, b = torch.randint(-8, 9, (F, H), generator=g).float(), torch.randint(-8, 9, (H,), generator=g).float()
    else:
        w, b = torch.randn((F, H), generator=g), torch.randn((H,), generator=g)
    w, b = w.to(dtype), b.to(dtype)
    return (w.to(env.engine.device), b.to(env.engine.device) if bias else None, w.float().numpy(), b.float().numpy() if bias else None)


def bits(x):
    """a float32 / bfloat16 device or host tensor, or a float32 array, as the uint32 patterns of its float32 values"""
    if not isinstance(x, np.ndarray):
        x = x.detach().float().cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def out_name(dtype):
    import torch
    return "bfloat16" if dtype == torch.bfloat16 else np.float32


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("name", ["chain10", "toyctf"])
def test_forward_equals_host_mirror(name, H):
    """General random weights, fp32 and bf16 weights x fp32 and bf16 output, every row count, the dense source, the packed source and
    the packed source through a permuting and a repeating index: the host mirror's bits."""
    import torch
    env, fields, host, lay, packed = case(name)
    eng, h, pk = env.engine, env._feature_handle(False, False), env._packing_handle()
    E, F = env.num_envs, lay.width
    gen = torch.Generator().manual_seed(H)
    perm = torch.randperm(E, generator=gen)
    rep = torch.randint(0, E, (E,), generator=gen)
    for wdt in (torch.float32, torch.bfloat16):
        wt, b, wt_host, b_host = params(env, F, H, wdt, 100 + H)
        for odt in (torch.float32, torch.bfloat16):
            want = lay.first_layer_host(host, wt_host, b_host, out_dtype=out_name(odt))
            want_perm = lay.first_layer_host(host, wt_host, b_host, out_dtype=out_name(odt), index=perm.numpy())
            want_rep = lay.first_layer_host(host, wt_host, b_host, out_dtype=out_name(odt), index=rep.numpy())
            oor = torch.zeros(1, dtype=torch.int32, device=eng.device)
            for n in NS:
                ctx = f"{name} H={H} {wdt} -> {odt} n={n}"
                got = eng.first_layer(h, wt, b, obs={k: v[:n] for k, v in fields.items()}, dtype=odt, out_of_range=oor)
                assert got.dtype == odt and tuple(got.shape) == (n, H), ctx
                assert np.array_equal(bits(got), bits(want[:n])), ctx + " dense"
                got = eng.first_layer(h, wt, b, packing=pk, packed=packed[:n], dtype=odt, out_of_range=oor)
                assert np.array_equal(bits(got), bits(want[:n])), ctx + " packed"
                for idx, w_idx, label in ((perm, want_perm, "permuting"), (rep, want_rep, "repeating")):
                    got = eng.first_layer(h, wt, b, packing=pk, packed=packed, index=idx[:n].to(eng.device), dtype=odt, out_of_range=oor)
                    assert tuple(got.shape) == (n, H) and np.array_equal(bits(got), bits(w_idx[:n])), f"{ctx} {label} index"
            assert int(oor) == 0
    # without a bias the chain starts at +0.0
    wt, _, wt_host, _ = params(env, F, H, torch.float32, 7, bias=False)
    assert np.array_equal(bits(eng.first_layer(h, wt, obs=fields)), bits(lay.first_layer_host(host, wt_host)))


def test_odd_observation_bounds():
    """Chain-10 at 13/13 (the bounds of tests/golden/chain10_bounds13x13_s92.npz): another row layout, element counts and packing."""
    import torch
    from marlon_amd.wrappers import AttackerVecEnv
    env = AttackerVecEnv(_environment("chain10"), 65, maximum_node_count=13, maximum_total_credentials=13, discrete=True, seed=3,
                         materialize_masks=False)
    g = torch.Generator(device=env.engine.device).manual_seed(2)
    for _ in range(80):
        m = env.unpack_action_mask(env.action_masks_packed())
        scores = torch.rand(m.shape, generator=g, device=m.device)
        env.step(torch.where(m, scores, torch.full_like(scores, -1.0)).argmax(dim=1))
    fields = {k: env._obs[k] for k in FIELDS}
    host, lay = host_obs(fields)[0], env.feature_layout()
    assert lay.width != 1012 and bool((fields["nodes_privilegelevel"] > 0).any())
    for H, wdt in ((64, torch.float32), (5, torch.bfloat16)):
        wt, b, wt_host, b_host = params(env, lay.width, H, wdt, H)
        want = lay.first_layer_host(host, wt_host, b_host)
        assert np.array_equal(bits(env.first_layer(wt.t().contiguous(), b)), bits(want))
        assert np.array_equal(bits(env.encode_first_layer_packed(env.observation_packed(), None, b, weight_t=wt)), bits(want))
    env.close()


def test_table_wider_than_any_staging():
    """Chain-100 at 102/102, 64 envs: 17 302 columns (4.5 MB of weights at H = 65), elements of 102 classes next to elements of 3 —
    slabs of every fill, H across two 64-lane chunks; the gradient's wavefronts own more columns than their LDS holds."""
    import torch
    from marlon_amd import engine, flatten
    from marlon_amd._abi import EnvSpec
    from marlon_amd.features import FeatureLayout, ObservationPacking
    from marlon_amd.samples import chainpattern
    topo = flatten.flatten(chainpattern.new_environment(100))
    E = 64
    spec = EnvSpec(n_envs=E, maximum_node_count=102, maximum_total_credentials=102, auto_reset=True, seed=1)
    eng = engine.BatchEngine(topo, spec)
    obs = eng.alloc_obs(FIELDS)
    for t in range(120):
        a = eng.sample_actions(True, seed=3, step=t)
        if t == 119:
            eng.step_observe(a, obs)
        else:
            eng.step(a)
    lay = FeatureLayout(topo, spec)
    H = 65
    assert lay.width * H * 4 > 4 * 160 * 1024 and max(n for _, _, n in lay.groups) > 100
    h, pk = eng.feature_layout(lay), eng.observation_packing(ObservationPacking(topo, spec))
    host = host_obs(obs)[0]
    g = torch.Generator().manual_seed(5)
    w = torch.randn((lay.width, H), generator=g)
    b = torch.randn((H,), generator=g)
    want = lay.first_layer_host(host, w.numpy(), b.numpy())
    oor = torch.zeros(1, dtype=torch.int32, device=eng.device)
    got = eng.first_layer(h, w.to(eng.device), b.to(eng.device), obs=obs, out_of_range=oor)
    assert np.array_equal(bits(got), bits(want)) and int(oor) == 0
    packed = eng.pack_observation(pk, obs)
    got = eng.first_layer(h, w.to(eng.device), b.to(eng.device), packing=pk, packed=packed, out_of_range=oor)
    assert np.array_equal(bits(got), bits(want)) and int(oor) == 0
    grad = torch.randn((E, H), generator=g)
    want_w, want_b = lay.first_layer_grad_host(host, grad.numpy(), H)
    got = eng.first_layer_grad(h, grad.to(eng.device), obs=obs)
    assert np.array_equal(bits(got.grad_weight_t), bits(want_w)) and np.array_equal(bits(got.grad_bias), bits(want_b))
    h.close()
    pk.close()
    eng.close()


def test_elements_wider_than_a_slab():
    """Chain-4 at 6/130: the credential elements have 130 and 131 classes, more columns than one slab of the forward kernel stages, so
    their selected column is read from memory; forward and gradient, both sources."""
    import torch
    from marlon_amd.samples import chainpattern
    from marlon_amd.wrappers import AttackerVecEnv
    env = AttackerVecEnv(chainpattern.new_environment(4), 65, maximum_node_count=6, maximum_total_credentials=130, discrete=True, seed=4,
                         materialize_masks=False)
    g = torch.Generator(device=env.engine.device).manual_seed(3)
    for _ in range(40):
        m = env.unpack_action_mask(env.action_masks_packed())
        scores = torch.rand(m.shape, generator=g, device=m.device)
        env.step(torch.where(m, scores, torch.full_like(scores, -1.0)).argmax(dim=1))
    fields = {k: env._obs[k] for k in FIELDS}
    host, lay = host_obs(fields)[0], env.feature_layout()
    assert max(n for _, _, n in lay.groups) == 131 and bool((fields["scalars"][:, 5] > 0).any())
    eng, h, pk = env.engine, env._feature_handle(False, False), env._packing_handle()
    packed = env.observation_packed()
    for H, wdt in ((65, torch.float32), (3, torch.bfloat16)):
        wt, b, wt_host, b_host = params(env, lay.width, H, wdt, H)
        want = lay.first_layer_host(host, wt_host, b_host)
        assert np.array_equal(bits(eng.first_layer(h, wt, b, obs=fields)), bits(want))
        assert np.array_equal(bits(eng.first_layer(h, wt, b, packing=pk, packed=packed)), bits(want))
        grad = torch.randn((65, H), generator=torch.Generator().manual_seed(H))
        want_w, want_b = lay.first_layer_grad_host(host, grad.numpy(), H)
        for source in (dict(obs=fields), dict(packing=pk, packed=packed)):
            got = eng.first_layer_grad(h, grad.to(eng.device), **source)
            assert np.array_equal(bits(got.grad_weight_t), bits(want_w)) and np.array_equal(bits(got.grad_bias), bits(want_b))
    env.close()


@pytest.mark.parametrize("name", ["chain10", "toyctf"])
def test_exact_inputs_equal_torch_linear(name):
    """Integer weights and bias in [-8, 8]: every partial sum is exact, so torch.nn.functional.linear on features() gives the same bits
    in whatever order it sums; through the wrapper's three entry points and the VecEnv adapter."""
    import torch
    import torch.nn.functional as TF
    from marlon_amd.vecenv import MarlonVecEnv
    env, fields, host, lay, packed = case(name)
    for H in (3, 64, 200):
        wt, b, _, _ = params(env, lay.width, H, torch.float32, H, exact=True)
        weight = wt.t().contiguous()                                 # torch's Linear.weight [H, F]
        want = TF.linear(env.features(), weight, b)
        assert torch.equal(env.first_layer(weight, b), want)
        assert torch.equal(env.first_layer(weight, b, weight_t=wt), want)
        assert torch.equal(env.encode_first_layer(fields, weight, b), want)
        assert torch.equal(env.encode_first_layer_packed(packed, weight, b), want)
        assert torch.equal(MarlonVecEnv(env, numpy_outputs=False).first_layer(weight, b), want)
        # policy_net[0] and value_net[0] in one call: the weights concatenated into [2H, F]
        w2, b2, _, _ = params(env, lay.width, H, torch.float32, H + 1, exact=True)
        both = env.first_layer(torch.cat([weight, w2.t()]), torch.cat([b, b2]))
        assert torch.equal(both[:, :H], want) and torch.equal(both[:, H:], TF.linear(env.features(), w2.t().contiguous(), b2))
        # bfloat16 end to end: the exact integer sum rounded once
        want16 = TF.linear(env.features(dtype=torch.bfloat16), weight.bfloat16(), b.bfloat16())
        assert torch.equal(env.first_layer(weight.bfloat16(), b.bfloat16(), dtype=torch.bfloat16), want16)
    # the reference's class counts: two columns fewer
    layr = env.feature_layout(reference_counts=True)
    wt, b, _, _ = params(env, layr.width, 16, torch.float32, 1, exact=True)
    assert torch.equal(env.first_layer(None, b, weight_t=wt, reference_counts=True), TF.linear(env.features(reference_counts=True), wt.t(), b))


def test_out_discipline():
    """out= with padded row strides and rows that start on odd elements: elements from H up to the stride, and the rows around the call,
    keep their sentinel; weights whose rows lie further apart than H read the same."""
    import torch
    env, fields, host, lay, packed = case("chain10")
    eng, h = env.engine, env._feature_handle(False, False)
    E, F = env.num_envs, lay.width
    for H in (3, 64, 65):
        for wdt in (torch.float32, torch.bfloat16):
            wt, b, wt_host, b_host = params(env, F, H, wdt, 3 * H)
            wide = torch.full((F, H + 5), SENTINEL, dtype=wdt, device=eng.device)
            wide[:, :H] = wt
            for odt in (torch.float32, torch.bfloat16):
                want = lay.first_layer_host(host, wt_host, b_host, out_dtype=out_name(odt))
                for stride, offset in ((H, 0), (H + 1, 0), (H + 2 + H % 2, 1), (H + 61, 3)):
                    buf = torch.full(((E + 2) * stride + offset,), SENTINEL, dtype=odt, device=eng.device)
                    rows = buf[offset:].view(E + 2, stride)
                    got = eng.first_layer(h, wide[:, :H], b, obs=fields, out=rows[1:E + 1, :H])
                    ctx = f"H={H} {wdt} -> {odt} stride {stride} offset {offset}"
                    assert got.data_ptr() == rows[1].data_ptr() and tuple(got.shape) == (E, H), ctx
                    assert np.array_equal(bits(got), bits(want)), ctx
                    r = rows.float().cpu()
                    assert (r[1:E + 1, H:] == SENTINEL).all(), ctx + ": elements past H were written"
                    assert (r[0] == SENTINEL).all() and (r[E + 1] == SENTINEL).all() and (buf[:offset] == SENTINEL).all(), ctx
            assert bool((wide[:, H:] == SENTINEL).all())


def test_out_of_range_values_and_index_bounds():
    """Injected negative and too-large values select nothing and are counted (the counter is INCREASED); an index outside the storage
    reads nothing: that row is the bias alone (+0.0 without one) and counts every element."""
    import torch
    env, fields, host, lay, packed = case("toyctf")
    eng, h, pk = env.engine, env._feature_handle(False, False), env._packing_handle()
    E, F, H = env.num_envs, lay.width, 64
    bad_fields = {k: v.clone() for k, v in fields.items()}
    bad_fields["scalars"][0, 6] = 99
    bad_fields["scalars"][1, 3] = -1
    bad_fields["scalars"][2, 0] = 2 ** 31 - 1
    bad_fields["leaked_credentials"][3].fill_(-5)
    bad_fields["credential_cache_matrix"][4:9, 2, 1] = 8 + 65536
    bad_fields["nodes_privilegelevel"][E - 1] = 4
    bad_fields["nodes_privilegelevel"][E - 2, 0] = -(2 ** 31)
    bad_host = host_obs(bad_fields)[0]
    wt, b, wt_host, b_host = params(env, F, H, torch.float32, 4)
    want, bad = lay.first_layer_host(bad_host, wt_host, b_host, return_out_of_range=True)
    assert bad > 30 and bad == expected(env.topo, env.spec, bad_fields)[1]
    oor = torch.full((1,), 1000, dtype=torch.int32, device=eng.device)
    assert np.array_equal(bits(eng.first_layer(h, wt, b, obs=bad_fields, out_of_range=oor)), bits(want)) and int(oor) == 1000 + bad
    bad_packed = eng.pack_observation(pk, bad_fields)
    assert np.array_equal(bits(eng.first_layer(h, wt, b, packing=pk, packed=bad_packed, out_of_range=oor)), bits(want))
    assert int(oor) == 1000 + 2 * bad
    # H over two chunks counts once
    wt2, b2, wt2_host, b2_host = params(env, F, 130, torch.float32, 5)
    oor.zero_()
    got = eng.first_layer(h, wt2, b2, obs=bad_fields, out_of_range=oor)
    assert np.array_equal(bits(got), bits(lay.first_layer_host(bad_host, wt2_host, b2_host))) and int(oor) == bad
    # reference_counts: a full count selects nothing
    hr, layr = env._feature_handle(False, True), env.feature_layout(reference_counts=True)
    full = {k: v.clone() for k, v in fields.items()}
    full["scalars"][:5, 6] = env.spec.maximum_node_count
    full["scalars"][:3, 5] = env.spec.maximum_total_credentials
    wr, br, wr_host, br_host = params(env, layr.width, 8, torch.float32, 6)
    want_r, bad_r = layr.first_layer_host(host_obs(full)[0], wr_host, br_host, return_out_of_range=True)
    assert bad_r >= 8
    oor.zero_()
    assert np.array_equal(bits(eng.first_layer(hr, wr, br, obs=full, out_of_range=oor)), bits(want_r)) and int(oor) == bad_r
    # index bounds
    index = torch.tensor([5, -1, 0, E, E - 1, 2 ** 40, -(2 ** 62), 7], dtype=torch.int64)
    inside = ((index >= 0) & (index < E)).numpy()
    for bias, bias_host in ((b, b_host), (None, None)):
        want_i, bad_i = lay.first_layer_host(host, wt_host, bias_host, index=index.numpy(), return_out_of_range=True)
        assert bad_i == int((~inside).sum()) * lay.n_elements
        oor.zero_()
        got = eng.first_layer(h, wt, bias, packing=pk, packed=packed, index=index.to(eng.device), out_of_range=oor)
        assert np.array_equal(bits(got), bits(want_i)) and int(oor) == bad_i
        alone = np.broadcast_to(bias_host if bias is not None else np.zeros(H, np.float32), (int((~inside).sum()), H))
        assert np.array_equal(bits(got)[~inside], bits(alone))


def test_a_row_does_not_depend_on_its_place():
    """The same bits whatever the row's position in the launch — rows computed alone, in short calls at odd offsets and as part of 320 —
    and across two calls."""
    import torch
    env, fields, host, lay, packed = case("chain10")
    eng, h, pk = env.engine, env._feature_handle(False, False), env._packing_handle()
    E = env.num_envs
    for H, wdt in ((64, torch.float32), (200, torch.bfloat16)):
        wt, b, _, _ = params(env, lay.width, H, wdt, 11)
        whole = eng.first_layer(h, wt, b, obs=fields)
        assert torch.equal(eng.first_layer(h, wt, b, obs=fields), whole)
        assert torch.equal(eng.first_layer(h, wt, b, packing=pk, packed=packed), whole)
        for r in (0, 1, 63, 64, 200, E - 1):
            alone = eng.first_layer(h, wt, b, obs={k: v[r:r + 1] for k, v in fields.items()})
            assert torch.equal(alone[0], whole[r]), (H, r)
            idx = torch.tensor([r], dtype=torch.int64, device=eng.device)
            assert torch.equal(eng.first_layer(h, wt, b, packing=pk, packed=packed, index=idx)[0], whole[r]), (H, r)
        part = eng.first_layer(h, wt, b, obs={k: v[37:37 + 70] for k, v in fields.items()})
        assert torch.equal(part, whole[37:37 + 70])


def test_graph_capture():
    """One launch, no host synchronisation: captured with torch.cuda.graph, one replay equals the eager result."""
    import torch
    env, fields, host, lay, packed = case("toyctf")
    eng, h, pk = env.engine, env._feature_handle(False, False), env._packing_handle()
    E, H = env.num_envs, 64
    wt, b, _, _ = params(env, lay.width, H, torch.float32, 12)
    idx = torch.randperm(E, generator=torch.Generator().manual_seed(1)).to(eng.device)
    eager = eng.first_layer(h, wt, b, obs=fields).clone()
    eager_packed = eng.first_layer(h, wt, b, packing=pk, packed=packed, index=idx).clone()
    out = torch.zeros((E, H), dtype=torch.float32, device=eng.device)
    out_packed = torch.zeros((E, H), dtype=torch.float32, device=eng.device)
    oor = torch.zeros(1, dtype=torch.int32, device=eng.device)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.first_layer(h, wt, b, obs=fields, out=out, out_of_range=oor)
        eng.first_layer(h, wt, b, packing=pk, packed=packed, index=idx, out=out_packed, out_of_range=oor)
    out.zero_()
    out_packed.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(out_packed, eager_packed) and int(oor) == 0


def test_refusals():
    """Every refusal of the contract through the C ABI (MCBS_EINVAL with a message, nothing written) and what the Python layer
    refuses before the call."""
    import torch
    from marlon_amd._abi import ObsBuffers
    env, fields, host, lay, packed = case("chain10")
    eng, lib = env.engine, env.engine.lib
    h, hm, pk = env._feature_handle(False, False), env._feature_handle(True, False), env._packing_handle()
    E, F, H = env.num_envs, lay.width, 16
    wt, b, _, _ = params(env, F, H, torch.float32, 1)
    out = torch.full((E, H + 4), SENTINEL, dtype=torch.float32, device=eng.device)
    ob = ObsBuffers(**{k: v.data_ptr() for k, v in fields.items()})
    st = eng._stream()

    def dense(handle=h, obs=ob, n=E, w=wt.data_ptr(), ws=H, bias=b.data_ptr(), wd=0, hh=H, o=out.data_ptr(), od=0, os_=H + 4):
        return lib.mcbs_first_layer(eng._h, handle.ptr, C.byref(obs), n, w, ws, bias, wd, hh, o, od, os_, None, st)

    def from_packed(handle=h, packing=pk.ptr, p=packed.data_ptr(), words=packed.stride(0), index=None, m=E, n=E, w=wt.data_ptr(), o=out.data_ptr()):
        return lib.mcbs_first_layer_packed(eng._h, handle.ptr, packing, p, words, index, m, n, w, H, b.data_ptr(), 0, H, o, 0, H + 4, None, st)

    def refused(rc, word):
        assert rc == -1 and word in lib.mcbs_last_error(), (rc, lib.mcbs_last_error())

    refused(dense(handle=hm), b"include_masks")
    refused(from_packed(handle=hm), b"include_masks")
    refused(dense(hh=0), b"H 0")
    refused(dense(hh=513), b"H 513")
    refused(dense(ws=H - 1), b"weight_row_stride")
    refused(dense(os_=H - 1), b"out_row_stride")
    refused(dense(wd=2), b"dtype")
    refused(dense(od=2), b"dtype")
    refused(dense(od=-1), b"dtype")
    refused(dense(w=None), b"NULL")
    refused(dense(o=None), b"NULL")
    refused(dense(obs=ObsBuffers(**{k: v.data_ptr() for k, v in fields.items() if k != "nodes_privilegelevel"})), b"nodes_privilegelevel")
    assert lib.mcbs_first_layer(eng._h, h.ptr, None, E, wt.data_ptr(), H, None, 0, H, out.data_ptr(), 0, H + 4, None, st) == -1
    assert lib.mcbs_first_layer(None, h.ptr, C.byref(ob), E, wt.data_ptr(), H, None, 0, H, out.data_ptr(), 0, H + 4, None, st) == -1
    refused(from_packed(p=None), b"null")
    refused(from_packed(packing=None), b"null")
    refused(from_packed(words=pk.words - 1), b"packed_row_words")
    refused(from_packed(m=E - 1), b"no index")
    other = Envs.get("toyctf")
    refused(dense(handle=other._feature_handle(False, False)), b"geometry")
    refused(from_packed(packing=other._packing_handle().ptr), b"geometry")
    # an output sharing a byte with an input
    refused(dense(o=wt.data_ptr()), b"overlaps")
    refused(dense(o=fields["scalars"].data_ptr()), b"overlaps")
    refused(dense(o=b.data_ptr()), b"overlaps")
    refused(from_packed(o=packed.data_ptr()), b"overlaps")
    # a layout that gives a value more classes than the packing has codes
    from marlon_amd.features import ObservationPacking
    small = ObservationPacking(env.topo, env.spec)
    small.valid_codes = small.valid_codes.copy()
    small.valid_codes[0] -= 1                                       # 12 codes instead of 13: the same 4 bits, the same words
    narrow = eng.observation_packing(small)
    refused(from_packed(packing=narrow.ptr), b"valid codes")
    narrow.close()
    assert dense(n=0) == 0 and from_packed(n=0) == 0                # no rows: success without a launch
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    # the Python layer
    with pytest.raises(ValueError, match="mask columns"):
        eng.first_layer(hm, wt, b, obs=fields)
    with pytest.raises(ValueError, match="either obs"):
        eng.first_layer(h, wt, b)
    with pytest.raises(ValueError, match="either obs"):
        eng.first_layer(h, wt, b, obs=fields, packing=pk, packed=packed)
    with pytest.raises(ValueError, match="packing="):
        eng.first_layer(h, wt, b, packed=packed)
    with pytest.raises(ValueError, match="weight_t"):
        eng.first_layer(h, wt[:-1], b, obs=fields)
    with pytest.raises(ValueError, match="weight_t"):
        eng.first_layer(h, wt.double(), b, obs=fields)
    with pytest.raises(ValueError, match="bias"):
        eng.first_layer(h, wt, b.bfloat16(), obs=fields)
    with pytest.raises(ValueError, match="at most 512"):
        eng.first_layer(h, torch.zeros((F, 513), device=eng.device), obs=fields)
    with pytest.raises(ValueError, match="out"):
        eng.first_layer(h, wt, b, obs=fields, out=out[:, :H - 1])
    with pytest.raises(ValueError, match="out"):
        eng.first_layer(h, wt, b, obs=fields, dtype=torch.float16)
    with pytest.raises(ValueError, match="index"):
        eng.first_layer(h, wt, b, packing=pk, packed=packed, index=torch.zeros(4, dtype=torch.int32, device=eng.device))
    with pytest.raises(ValueError, match="out="):
        env.encode_first_layer(fields, wt.t().contiguous(), b, out=out[:, :H], differentiable=True)
