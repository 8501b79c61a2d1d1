"""mcbs_encode_features (include/mcbs.h "feature encoder", marlon_amd/csrc/mcbs_features.hip) through BatchEngine.encode_features and
AttackerVecEnv.features / encode_features.

Yardstick: `restate` of tests/test_feature_layout.py — torch.nn.functional.one_hot per element and torch.cat on the observation tensors
copied to the host, class counts computed in the test from the reference's spaces.  Neither FeatureLayout.encode_host nor the kernel
produces an expected value.  Values are exactly 0 and 1 in every dtype, so every comparison is exact equality."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.test_feature_layout import ARRAYS, MASKS, SCALARS, dims, key_classes, restate

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ["scalars"] + ARRAYS
SENTINEL = 7.0
BOUNDS = {"chain10": (12, 12), "toyctf": (12, 10)}


def _environment(name):
    from marlon_amd.samples import chainpattern, toy_ctf
    return chainpattern.new_environment(10) if name == "chain10" else toy_ctf.new_environment()


def _dtypes():
    import torch
    return {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def host_obs(fields, masks=None):
    """device observation fields (+ the bool Discrete mask [n, A] in connect | local | remote order) -> the wrapper's keys on the host"""
    sc = fields["scalars"].cpu().numpy()
    n = sc.shape[0]
    out = {k: sc[:, i] for i, k in enumerate(SCALARS)}
    out.update({k: fields[k].cpu().numpy().reshape(n, -1) for k in ARRAYS})
    return out, (None if masks is None else masks.cpu().numpy())


def expected(topo, spec, fields, masks=None, reference_counts=False, keys=None):
    """-> (float32 CPU tensor [n, F], out-of-range count, key -> (first column, class counts or None, columns)) by the one_hot / cat
    restatement"""
    N, Cm, K, L, R, P, NP = dims(topo, spec)
    classes, mask_sizes = key_classes(N, Cm, K, L, R, P, NP, reference_counts)
    obs, m = host_obs(fields, masks)
    if m is not None:
        M, ML = mask_sizes["connect"], mask_sizes["local_vulnerability"]
        obs.update(connect=m[:, :M], local_vulnerability=m[:, M:M + ML], remote_vulnerability=m[:, M + ML:])
    keys = keys or sorted(list(classes) + (MASKS if m is not None else []))
    want, bad = restate(obs, classes, mask_sizes, keys)
    where, col = {}, 0
    for k in keys:
        w = mask_sizes[k] if k in mask_sizes else sum(classes[k])
        where[k] = (col, classes.get(k), w)
        col += w
    return want, bad, where


def assert_left_reset_state(want, where):
    """the expected rows hold a 1 outside class 0 in each of the five int32 fields (a run that never left the reset state cannot pass)"""
    def beyond_class0(k):
        c0, widths, _ = where[k]
        keep = np.ones(sum(widths), bool)
        keep[np.cumsum([0] + widths[:-1])] = False
        return bool(want[:, c0:c0 + sum(widths)][:, keep].any())
    assert any(beyond_class0(k) for k in SCALARS), "scalars"
    for k in ARRAYS:
        assert beyond_class0(k), k


class Stepped:
    """One AttackerVecEnv per (topology, mask mode) stepped with masked uniformly random Discrete actions, built once per module."""
    cache = {}

    @classmethod
    def get(cls, name, materialize=True, E=320, steps=300):
        key = (name, materialize)
        if key not in cls.cache:
            import torch
            from marlon_amd.wrappers import AttackerVecEnv
            N, Cm = BOUNDS[name]
            env = AttackerVecEnv(_environment(name), E, maximum_node_count=N, maximum_total_credentials=Cm, discrete=True, seed=5,
                                 materialize_masks=materialize)
            g = torch.Generator(device=env.engine.device).manual_seed(11)
            # `steps` steps, then on until the observation of some env reports leaked credentials (leaked_credentials holds the LAST
            # action's leaks only, so most steps show none): the rule looks at the observation alone, and both mask modes stop alike
            for t in range(steps + 200):
                if t >= steps and bool(env._obs["leaked_credentials"].any()):
                    break
                m = env.action_masks() if materialize else env.unpack_action_mask(env.action_masks_packed())
                scores = torch.rand(m.shape, generator=g, device=m.device)
                env.step(torch.where(m, scores, torch.full_like(scores, -1.0)).argmax(dim=1))
            cls.cache[key] = env
        return cls.cache[key]


@pytest.fixture(scope="module", autouse=True)
def _close_envs():
    yield
    for env in Stepped.cache.values():
        env.close()
    Stepped.cache.clear()


def _fields(env):
    return {k: env._obs[k] for k in FIELDS}


@pytest.mark.parametrize("dt", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("name", ["chain10", "toyctf"])
def test_features_equal_one_hot_restatement(name, dt):
    """At least 300 valid random steps of 320 envs, then features() in both count modes: equal to the restatement, out_of_range stays 0 with
    the default layout, the returned rows are a view of rows padded to whole 128-byte lines."""
    import torch
    env = Stepped.get(name)
    dtype = _dtypes()[dt]
    want, bad, where = expected(env.topo, env.spec, _fields(env))
    assert bad == 0
    assert_left_reset_state(want, where)
    oor = torch.zeros(1, dtype=torch.int32, device=env.engine.device)
    got = env.features(dtype=dtype, out_of_range=oor)
    lay = env.feature_layout()
    assert got.dtype == dtype and tuple(got.shape) == (env.num_envs, lay.width) == tuple(want.shape)
    assert (got.stride(0) * got.element_size()) % 128 == 0 and got.data_ptr() % 128 == 0
    assert torch.equal(got.float().cpu(), want)
    assert int(oor) == 0
    assert {k: v[0] for k, v in where.items()} == {k: v[0] for k, v in lay.segments.items()}
    want_r, bad_r, _ = expected(env.topo, env.spec, _fields(env), reference_counts=True)
    oor.zero_()
    got_r = env.features(dtype=dtype, reference_counts=True, out_of_range=oor)
    assert tuple(got_r.shape) == tuple(want_r.shape) == (env.num_envs, lay.width - 2)
    assert torch.equal(got_r.float().cpu(), want_r) and int(oor) == bad_r


@pytest.mark.parametrize("materialize", [True, False])
@pytest.mark.parametrize("name", ["chain10", "toyctf"])
def test_features_with_masks(name, materialize):
    """include_masks=True: the three masks as 0 / 1 columns, from the mask packed on the device, in both materialize_masks modes; the
    restatement is fed with action_masks() — for the lean env (whose action_masks() raises) that of the materialising env, which took
    the same actions from the same seed and holds the same observation."""
    import torch
    env = Stepped.get(name, materialize)
    full = Stepped.get(name, True)
    assert all(torch.equal(env._obs[k], full._obs[k]) for k in FIELDS)
    masks = full.action_masks()
    want, bad, where = expected(env.topo, env.spec, _fields(env), masks)
    assert bad == 0
    for k in MASKS:                                          # every mask key allows something somewhere
        assert want[:, where[k][0]:where[k][0] + where[k][2]].any(), k
    for dt, dtype in _dtypes().items():
        oor = torch.zeros(1, dtype=torch.int32, device=env.engine.device)
        got = env.features(dtype=dtype, include_masks=True, out_of_range=oor)
        assert tuple(got.shape) == tuple(want.shape) and torch.equal(got.float().cpu(), want), dt
        assert int(oor) == 0


def _strides(F, itemsize):
    line = 128 // itemsize
    return {"dense": F, "padded": (F + line - 1) // line * line, "odd": F + 1 if (F + 1) % 2 else F + 2, "plus2": F + 2, "plus4": F + 4}


@pytest.mark.parametrize("reference_counts", [False, True])
@pytest.mark.parametrize("dt", ["fp32", "fp16", "bf16"])
def test_row_strides_and_sentinels(dt, reference_counts):
    """Dense rows, rows padded to whole lines, an odd stride in elements (4-byte aligned fp32 rows, 2-byte aligned 16-bit rows) and
    strides of F + 2 / F + 4 (the 8- and 4-byte store widths): equal to the restatement; elements from F up to the stride, the rows
    after the last and the row before the first keep their sentinel.  Without and with mask columns."""
    import torch
    env = Stepped.get("chain10")
    dtype = _dtypes()[dt]
    E = env.num_envs
    for include_masks in (False, True):
        masks = env.action_masks() if include_masks else None
        want, _, _ = expected(env.topo, env.spec, _fields(env), masks, reference_counts=reference_counts)
        F = want.shape[1]
        for label, stride in _strides(F, torch.empty((), dtype=dtype).element_size()).items():
            buf = torch.full((E + 2, stride), SENTINEL, dtype=dtype, device=env.engine.device)
            got = env.features(out=buf[1:E + 1, :F], include_masks=include_masks, reference_counts=reference_counts)
            ctx = f"{dt} {label} stride {stride} masks={include_masks}"
            assert got.data_ptr() == buf[1].data_ptr() and tuple(got.shape) == (E, F), ctx
            b = buf.float().cpu()
            assert torch.equal(b[1:E + 1, :F], want), ctx
            assert (b[1:E + 1, F:] == SENTINEL).all(), ctx + ": elements past F were written"
            assert (b[0] == SENTINEL).all() and (b[E + 1] == SENTINEL).all(), ctx + ": a row outside the call was written"


@pytest.mark.parametrize("n", [1, 63, 257, 320])
def test_any_number_of_rows(n):
    """encode_features on the first n rows of the observation (and of the packed masks): equal to the restatement of those rows; the
    rows after them keep their sentinel."""
    import torch
    env = Stepped.get("chain10")
    fields = {k: v[:n] for k, v in _fields(env).items()}
    bits = env.action_masks_packed()
    for masks in (None, env.action_masks()[:n]):
        want, _, _ = expected(env.topo, env.spec, fields, masks)
        F = want.shape[1]
        buf = torch.full((n + 1, F), SENTINEL, dtype=torch.float32, device=env.engine.device)
        got = env.encode_features(fields, bits=None if masks is None else bits[:n], out=buf[:n])
        assert tuple(got.shape) == (n, F) and torch.equal(got.cpu(), want)
        assert (buf[n] == SENTINEL).all()
        half = env.encode_features(fields, bits=None if masks is None else bits[:n], dtype=torch.bfloat16)
        assert torch.equal(half.float().cpu(), want)


def test_shuffled_gather_from_a_rollout_store():
    """A [T, E, ...] store of observations and packed masks filled over T steps; a shuffled minibatch gathered from it encodes to the
    features taken live at those steps (with mask columns), and the named-scalar form of the observation encodes the same."""
    import torch
    from marlon_amd.wrappers import AttackerVecEnv
    E, T = 96, 12
    env = AttackerVecEnv(_environment("toyctf"), E, maximum_node_count=12, maximum_total_credentials=10, discrete=True, seed=9,
                         materialize_masks=False)
    dev = env.engine.device
    g = torch.Generator(device=dev).manual_seed(4)
    W, row_words = env.engine.packed_mask_words()
    F = env.feature_layout(include_masks=True).width
    store = {k: torch.zeros((T,) + tuple(v.shape), dtype=v.dtype, device=dev) for k, v in _fields(env).items()}
    bits = torch.zeros((T, E, row_words), dtype=torch.int32, device=dev)
    live = torch.zeros((T, E, F), dtype=torch.float32, device=dev)
    for t in range(T):
        for k in FIELDS:
            store[k][t] = env._obs[k]
        env.action_masks_packed(out=bits[t])
        env.features(out=live[t], include_masks=True)
        m = env.unpack_action_mask(bits[t])
        scores = torch.rand(m.shape, generator=g, device=dev)
        for _ in range(4):                                   # four steps between stored ones: the stored rows differ
            env.step(torch.where(m, scores, torch.full_like(scores, -1.0)).argmax(dim=1))
            m = env.unpack_action_mask(env.action_masks_packed())
            scores = torch.rand(m.shape, generator=g, device=dev)
    assert not torch.equal(live[0], live[T - 1])
    idx = torch.randperm(T * E, generator=torch.Generator().manual_seed(1))[:257].to(dev)
    tt, ee = idx // E, idx % E
    gathered = {k: store[k][tt, ee] for k in FIELDS}
    got = env.encode_features(gathered, bits=bits[tt, ee])
    assert tuple(got.shape) == (257, F) and torch.equal(got, live[tt, ee])
    want, bad, _ = expected(env.topo, env.spec, gathered, env.unpack_action_mask(bits[tt, ee]))
    assert bad == 0 and torch.equal(got.cpu(), want)
    named = {k: gathered[k] for k in ARRAYS}
    named.update({k: gathered["scalars"][:, i] for i, k in enumerate(SCALARS)})
    assert torch.equal(env.encode_features(named, bits=bits[tt, ee]), got)
    env.close()


def test_chain10_winning_script_fills_the_reference_counts():
    """The reference's winning Chain-10 script at bounds 12/12 ends with discovered_node_count = 12 = N and credential_cache_length =
    11: under reference_counts=True (Discrete(N), as the reference declares it) the full count is an all-zero group and is counted,
    under the default it is class N."""
    import torch
    from marlon_amd import engine, flatten
    from marlon_amd._abi import EnvSpec
    from marlon_amd.features import FeatureLayout
    z = np.load(os.path.join(GOLDEN, "chain10_script.npz"))
    E = 4
    topo = flatten.flatten(_environment("chain10"))
    spec = EnvSpec(n_envs=E, maximum_node_count=12, maximum_total_credentials=12)
    eng = engine.BatchEngine(topo, spec)
    obs = eng.alloc_obs(FIELDS)
    for t in range(56):
        a = torch.as_tensor(np.repeat(z["actions"][t:t + 1], E, axis=0), device=eng.device)
        r, d = eng.step_observe(a, obs) if t == 55 else eng.step(a)
    assert bool(d.all())
    sc = obs["scalars"].cpu().numpy()
    assert (sc[:, 6] == 12).all() and (sc[:, 5] == 11).all()
    for reference_counts in (True, False):
        lay = FeatureLayout(topo, spec, reference_counts=reference_counts)
        h = eng.feature_layout(lay)
        oor = torch.zeros(1, dtype=torch.int32, device=eng.device)
        got = eng.encode_features(h, obs, out_of_range=oor).cpu()
        want, bad, where = expected(topo, spec, obs, reference_counts=reference_counts)
        assert torch.equal(got, want) and int(oor) == bad == (E if reference_counts else 0)
        c0, widths, _ = where["discovered_node_count"]
        assert widths == [12 if reference_counts else 13]
        if reference_counts:
            assert not got[:, c0:c0 + 12].any()
        else:
            assert (got[:, c0 + 12] == 1).all() and (got[:, c0:c0 + 13].sum(dim=1) == 1).all()
        l0 = where["credential_cache_length"][0]
        assert (got[:, l0 + 11] == 1).all()
        h.close()
    eng.close()


def test_random_events_and_learned_defender_batches():
    """No digest is read: an ExternalRandomEvents batch and a learned-defender batch encode like any other.  With mask columns the
    random-events wrapper packs the materialised mask itself (mcbs_pack_action_mask refuses such batches); without materialised masks
    it raises."""
    import torch
    from marlon_amd import cyberbattle_env as ce
    from marlon_amd.wrappers import AttackerVecEnv
    E = 64
    for kind in ("random_events", "learned"):
        kw = dict(defender_agent=ce.ExternalRandomEvents()) if kind == "random_events" else dict(learned_defender=True)
        env = AttackerVecEnv(_environment("toyctf"), E, maximum_node_count=12, maximum_total_credentials=10, discrete=True, seed=3, **kw)
        g = torch.Generator(device=env.engine.device).manual_seed(2)
        for _ in range(40):
            m = env.action_masks()
            scores = torch.rand(m.shape, generator=g, device=m.device)
            env.step(torch.where(m, scores, torch.full_like(scores, -1.0)).argmax(dim=1))
        want, bad, _ = expected(env.topo, env.spec, _fields(env))
        assert bad == 0 and torch.equal(env.features().cpu(), want), kind
        want_m, _, _ = expected(env.topo, env.spec, _fields(env), env.action_masks())
        got_m = env.features(include_masks=True, dtype=torch.float16)
        assert torch.equal(got_m.float().cpu(), want_m), kind
        env.close()
    lean = AttackerVecEnv(_environment("toyctf"), 8, maximum_node_count=12, maximum_total_credentials=10, discrete=True,
                          defender_agent=ce.ExternalRandomEvents(), materialize_masks=False)
    want, _, _ = expected(lean.topo, lean.spec, _fields(lean))
    assert torch.equal(lean.features().cpu(), want)
    with pytest.raises(RuntimeError, match="materialize"):
        lean.features(include_masks=True)
    lean.close()


def test_out_of_range_counts_add_up():
    """Rows edited to hold negative and too-large values: the groups are all zero, everything else equals the restatement, the
    counter is INCREASED by exactly the restatement's count on every call, nothing outside [row, F) is written."""
    import torch
    env = Stepped.get("toyctf")
    fields = {k: v.clone() for k, v in _fields(env).items()}
    E = env.num_envs
    fields["scalars"][0, 6] = 99
    fields["scalars"][1, 3] = -1
    fields["scalars"][2, 0] = 2 ** 31 - 1
    fields["leaked_credentials"][3].fill_(-5)
    fields["credential_cache_matrix"][4:9, 2, 1] = 8 + 65536          # the class bits of a descriptor must not alias a larger value
    fields["discovered_nodes_properties"][9, 1, :] = 3
    fields["nodes_privilegelevel"][E - 1] = 4
    fields["nodes_privilegelevel"][E - 2, 0] = -(2 ** 31)
    want, bad, _ = expected(env.topo, env.spec, fields)
    assert bad > 30
    F = want.shape[1]
    oor = torch.full((1,), 1000, dtype=torch.int32, device=env.engine.device)
    for dtype, calls in ((torch.float32, 1), (torch.bfloat16, 2)):
        buf = torch.full((E + 1, F + 3), SENTINEL, dtype=dtype, device=env.engine.device)
        got = env.encode_features(fields, out=buf[:E], out_of_range=oor)
        assert tuple(got.shape) == (E, F) and torch.equal(got.float().cpu(), want)
        assert int(oor) == 1000 + calls * bad
        b = buf.float().cpu()
        assert (b[:E, F:] == SENTINEL).all() and (b[E] == SENTINEL).all()
    # the same values are in range or not depending on the layout's class counts: a caller-ordered layout with fewer keys
    keys = ["nodes_privilegelevel", "probe_result"]
    h = env.engine.feature_layout(env.feature_layout(keys=keys))
    want_k, bad_k, _ = expected(env.topo, env.spec, fields, keys=keys)
    oor.zero_()
    sub = {k: fields[k] for k in ("scalars", "nodes_privilegelevel")}            # the other fields are not read: they may be left out
    assert torch.equal(env.engine.encode_features(h, sub, out_of_range=oor).cpu(), want_k) and int(oor) == bad_k == 12 + 1 + 1
    with pytest.raises(Exception, match="credential_cache_matrix|leaked|discovered"):
        env.engine.encode_features(env._feature_handle(False, False), sub)
    h.close()


def test_refusals_launch_nothing():
    """Narrow rows, NULL bits with mask columns, an unknown dtype, a layout of another geometry: MCBS_EINVAL with a message, the output
    untouched; malformed layouts are refused when they are created."""
    import torch
    from marlon_amd._abi import ObsBuffers
    env = Stepped.get("chain10")
    eng, lib = env.engine, env.engine.lib
    plain, masked = env._feature_handle(False, False), env._feature_handle(True, False)
    F, Fm = plain.width, masked.width
    E = env.num_envs
    out = torch.full((E, Fm + 8), SENTINEL, dtype=torch.float32, device=eng.device)
    bits = env.action_masks_packed()
    ob = ObsBuffers(**{k: v.data_ptr() for k, v in _fields(env).items()})
    st = eng._stream()

    def call(handle, bits_ptr, words, dtype, stride, n=E):
        return lib.mcbs_encode_features(eng._h, handle.ptr, C.byref(ob), bits_ptr, words, out.data_ptr(), dtype, stride, n, None, st)

    assert call(plain, None, 0, 0, F - 1) == -1 and b"shorter" in lib.mcbs_last_error()
    assert call(masked, bits.data_ptr(), bits.stride(0), 0, Fm - 1) == -1 and b"shorter" in lib.mcbs_last_error()
    assert call(masked, None, 0, 0, Fm) == -1 and b"bits is NULL" in lib.mcbs_last_error()
    assert call(masked, bits.data_ptr(), 10, 0, Fm) == -1 and b"bits_row_words" in lib.mcbs_last_error()
    assert call(plain, None, 0, 3, F) == -1 and b"dtype" in lib.mcbs_last_error()
    assert call(plain, None, 0, -1, F) == -1 and b"dtype" in lib.mcbs_last_error()
    other = Stepped.get("toyctf")
    assert call(other._feature_handle(False, False), None, 0, 0, Fm) == -1 and b"geometry" in lib.mcbs_last_error()
    assert call(plain, None, 0, 0, F, n=0) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    # the Python layer refuses what the C side cannot see: a view narrower than F, a missing bits tensor, a wrong dtype
    with pytest.raises(ValueError, match="contiguous rows"):
        eng.encode_features(plain, _fields(env), out=out[:, :F - 1])
    with pytest.raises(ValueError, match="bits"):
        eng.encode_features(masked, _fields(env))
    with pytest.raises(ValueError, match="float32, bfloat16 or float16"):
        eng.encode_features(plain, _fields(env), dtype=torch.float64)
    # layouts: a source index beyond the row, classes that do not count up, overlapping mask ranges, bits beyond the action count
    h = C.c_void_p()
    V = env.feature_layout().values_per_row

    def create(desc, ranges=()):
        d = np.asarray(desc, np.uint32)
        r = np.asarray(ranges, np.uint32).reshape(-1, 3)
        return lib.mcbs_feature_layout_create(eng._h, d.ctypes.data if d.size else None, d.size, r.ctypes.data if r.size else None, r.shape[0], C.byref(h))

    first = 1 << 31
    assert create([first | (V << 16)]) == -1 and b"reads value" in lib.mcbs_last_error()
    assert create([first, 2]) == -1 and b"continue" in lib.mcbs_last_error()
    assert create([1]) == -1
    assert create([first | 1]) == -1 and b"starts an element" in lib.mcbs_last_error()
    assert create([first, 1], [(0, 4, 0), (2, 4, 8)]) == -1
    assert create([first, 1], [(2, 4, eng.discrete_action_count() - 3)]) == -1 and b"Discrete actions" in lib.mcbs_last_error()
    assert create([first, 1], [(3, 4, 0)]) == -1
    assert create([], []) == -1
    assert create([first, 1], [(0, 1, 0)] * 4) == -1
    assert create([first, 1], [(1, 3, 5)]) == 0 and lib.mcbs_feature_layout_width(h) == 5
    lib.mcbs_feature_layout_destroy(h)


def test_side_stream_equals_default_stream():
    import torch
    env = Stepped.get("chain10")
    a = env.features(include_masks=True).clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=env.engine.device)
    with torch.cuda.stream(side):
        b = env.features(include_masks=True, dtype=torch.float32)
        c = env.features(dtype=torch.bfloat16)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(c.float(), env.features())


def test_env_method_reaches_features():
    """MarlonVecEnv.env_method("features", ...) reaches AttackerVecEnv.features like the wrapper's other methods."""
    import torch
    from marlon_amd.vecenv import MarlonVecEnv
    env = Stepped.get("toyctf")
    venv = MarlonVecEnv(env, numpy_outputs=False)
    res = venv.env_method("features", dtype=torch.float16)
    assert len(res) == env.num_envs and torch.equal(res[0].float(), env.features())
    assert venv.env_method("feature_layout", indices=0)[0].width == env.features().shape[1]


def test_large_topology_takes_the_unstaged_path():
    """A topology whose descriptor table and rows exceed the LDS budget (Chain-100 at 102/102: 30 000 columns, 59 KB of values per four
    rows) runs the variant that reads descriptors, values and bits from memory: equal to the restatement, with mask columns on a few
    rows (the Discrete space has 9.6 M actions)."""
    import torch
    from marlon_amd import engine, flatten
    from marlon_amd._abi import EnvSpec
    from marlon_amd.features import FeatureLayout
    from marlon_amd.samples import chainpattern
    topo = flatten.flatten(chainpattern.new_environment(100))
    E = 6
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
    assert (len(lay.descriptors) + 4 * lay.values_per_row) * 4 > 48 * 1024
    h = eng.feature_layout(lay)
    want, bad, where = expected(topo, spec, obs)
    assert bad == 0
    oor = torch.zeros(1, dtype=torch.int32, device=eng.device)
    for dtype in (torch.float32, torch.float16):
        got = eng.encode_features(h, obs, dtype=dtype, out_of_range=oor)
        assert torch.equal(got.float().cpu(), want)
    assert int(oor) == 0
    h.close()
    # with mask columns: two rows, bits packed on the device, the restatement fed with the unpacked bool mask
    laym = FeatureLayout(topo, spec, include_masks=True)
    hm = eng.feature_layout(laym)
    bits = eng.pack_action_mask()[:2]
    sub = {k: v[:2] for k, v in obs.items()}
    wantm, _, _ = expected(topo, spec, sub, eng.unpack_action_mask(bits))
    gotm = eng.encode_features(hm, sub, bits=bits, dtype=torch.bfloat16)
    assert tuple(gotm.shape) == tuple(wantm.shape) and torch.equal(gotm.float().cpu(), wantm)
    hm.close()
    eng.close()
