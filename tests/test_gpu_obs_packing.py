"""Packed observations on the device (include/mcbs.h "packed observations", marlon_amd/csrc/mcbs_obs_packing.hip) through
BatchEngine.pack_observation / unpack_observation / encode_features_packed and AttackerVecEnv.observation_packed / unpack_observation /
encode_features_packed / rollout_buffer(pack_observations=True).

Yardsticks: the restatement of the packed format written in tests/test_obs_packing_layout.py (class counts from the reference's spaces,
bit_length widths, no straddling, a plain loop over values) and `expected()` of tests/test_gpu_features.py (one_hot / cat on the int32
fields copied to the host).  Neither ObservationPacking.pack_host nor a kernel produces an expected value.  Every comparison is exact."""
import numpy as np
import pytest

from tests.test_feature_layout import MASKS
from tests.test_gpu_features import FIELDS, SENTINEL, Stepped, _dtypes, _fields, assert_left_reset_state, expected
from tests.test_obs_packing_layout import flat_values, restate_format, restate_pack

pytestmark = pytest.mark.gpu

WORD_SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _close_envs():
    yield
    for env in Stepped.cache.values():
        env.close()
    Stepped.cache.clear()


def host_fields(fields):
    return {k: v.cpu().numpy() for k, v in fields.items()}


def restated_rows(env, fields):
    """-> (uint32 [n, W_obs], count of out-of-range values, the format) of device fields by the restatement"""
    fmt = restate_format(env.topo, env.spec)
    codes, _, word, shift, words, _ = fmt
    want, bad = restate_pack(flat_values(host_fields(fields)), codes, word, shift, words)
    return want, bad, fmt


def as_u32(t):
    return t.cpu().numpy().view(np.uint32)


def shuffled_index(n_source, n, seed, device):
    """n row numbers of n_source: a permutation's start, then repeats of rows already drawn"""
    import torch
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(n_source, generator=g)
    idx = torch.cat([perm, perm[:7], perm[3:4].repeat(5)])[:n] if n > n_source else torch.cat([perm[:n - 9], perm[:9]])
    return idx.to(device)


@pytest.mark.parametrize("name", ["chain10", "toyctf"])
def test_pack_equals_the_restated_format(name):
    """The live observation after at least 300 random steps, packed: bit for bit the restatement; out= into the middle step of a
    [3, E, W_obs + 5] buffer changes only that step's first W_obs words; 1, 63, 65 and 320 rows through sliced fields."""
    import torch
    env = Stepped.get(name)
    E = env.num_envs
    feat, bad_f, where = expected(env.topo, env.spec, _fields(env))
    assert bad_f == 0
    assert_left_reset_state(feat, where)
    want, bad, fmt = restated_rows(env, _fields(env))
    W = fmt[4]
    assert bad == 0 and W == {"chain10": 18, "toyctf": 14}[name] == env.observation_packing().words
    oor = torch.zeros(1, dtype=torch.int32, device=env.engine.device)
    got = env.observation_packed(out_of_range=oor)
    assert got.dtype == torch.int32 and tuple(got.shape) == (E, W)
    assert np.array_equal(as_u32(got), want) and int(oor) == 0
    buf = torch.full((3, E, W + 5), WORD_SENTINEL, dtype=torch.int32, device=env.engine.device)
    ret = env.observation_packed(out=buf[1])
    assert ret.data_ptr() == buf[1].data_ptr()
    b = as_u32(buf)
    assert np.array_equal(b[1, :, :W], want)
    assert (b[1, :, W:] == WORD_SENTINEL).all() and (b[0] == WORD_SENTINEL).all() and (b[2] == WORD_SENTINEL).all()
    h = env._packing_handle()
    for n in (1, 63, 65, 320):
        out = torch.full((n + 1, W), WORD_SENTINEL, dtype=torch.int32, device=env.engine.device)
        env.engine.pack_observation(h, {k: v[:n] for k, v in _fields(env).items()}, out=out[:n])
        o = as_u32(out)
        assert np.array_equal(o[:n], want[:n]) and (o[n] == WORD_SENTINEL).all(), n


@pytest.mark.parametrize("name", ["chain10", "toyctf"])
def test_unpack_returns_the_fields(name):
    """unpack(pack(obs)) is the five fields exactly (every value in range); with an index that permutes, repeats and is shorter / longer
    than E it is index_select of them; a subset of fields through out=."""
    import torch
    env = Stepped.get(name)
    E = env.num_envs
    fields = _fields(env)
    packed = env.observation_packed()
    back = env.unpack_observation(packed)
    assert list(back) == FIELDS
    for k in FIELDS:
        assert back[k].dtype == torch.int32 and back[k].shape == fields[k].shape and torch.equal(back[k], fields[k]), k
    wide = torch.full((E, packed.shape[1] + 3), WORD_SENTINEL, dtype=torch.int32, device=packed.device)
    wide[:, :packed.shape[1]] = packed
    for n in (E + 12, 131):
        idx = shuffled_index(E, n, 5, packed.device)
        assert idx.shape[0] == n and len(set(idx.tolist())) < n
        got = env.unpack_observation(wide, index=idx)
        for k in FIELDS:
            assert got[k].shape[0] == n and torch.equal(got[k], fields[k].index_select(0, idx)), k
    only = {"nodes_privilegelevel": torch.full_like(fields["nodes_privilegelevel"], -3)}
    env.engine.unpack_observation(env._packing_handle(), packed, out=only)
    assert torch.equal(only["nodes_privilegelevel"], fields["nodes_privilegelevel"])


@pytest.mark.parametrize("dt", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("name", ["chain10", "toyctf"])
def test_packed_features_equal_one_hot_restatement(name, dt):
    """encode_features_packed on the packed live observation in both count modes: the restatement's rows and out-of-range count, and
    bit for bit what encode_features gives on the int32 fields."""
    import torch
    env = Stepped.get(name)
    dtype = _dtypes()[dt]
    packed = env.observation_packed()
    for reference_counts in (False, True):
        want, bad, _ = expected(env.topo, env.spec, _fields(env), reference_counts=reference_counts)
        oor = torch.zeros(1, dtype=torch.int32, device=env.engine.device)
        got = env.encode_features_packed(packed, dtype=dtype, reference_counts=reference_counts, out_of_range=oor)
        assert got.dtype == dtype and tuple(got.shape) == tuple(want.shape)
        assert (got.stride(0) * got.element_size()) % 128 == 0
        assert torch.equal(got.float().cpu(), want) and int(oor) == bad
        assert bad == 0 or reference_counts
        assert torch.equal(got, env.encode_features(_fields(env), dtype=dtype, reference_counts=reference_counts))


@pytest.mark.parametrize("materialize", [True, False])
@pytest.mark.parametrize("name", ["chain10", "toyctf"])
def test_packed_features_with_masks(name, materialize):
    """With the three masks as columns, bits packed on the device in both materialize_masks modes (the restatement is fed with the
    materialising env's action_masks(), which took the same actions from the same seed)."""
    import torch
    env = Stepped.get(name, materialize)
    full = Stepped.get(name, True)
    assert all(torch.equal(env._obs[k], full._obs[k]) for k in FIELDS)
    want, bad, where = expected(env.topo, env.spec, _fields(env), full.action_masks())
    assert bad == 0
    for k in MASKS:
        assert want[:, where[k][0]:where[k][0] + where[k][2]].any(), k
    packed, bits = env.observation_packed(), env.action_masks_packed()
    for dt, dtype in _dtypes().items():
        got = env.encode_features_packed(packed, bits=bits, dtype=dtype)
        assert tuple(got.shape) == tuple(want.shape) and torch.equal(got.float().cpu(), want), dt


def test_packed_features_in_a_custom_key_order():
    import torch
    env = Stepped.get("toyctf")
    keys = ["nodes_privilegelevel", "remote_vulnerability", "credential_cache_matrix", "discovered_node_count", "connect", "leaked_credentials"]
    from marlon_amd.features import FeatureLayout
    h = env.engine.feature_layout(FeatureLayout(env.topo, env.spec, keys=keys, include_masks=True))
    want, bad, _ = expected(env.topo, env.spec, _fields(env), env.action_masks(), keys=keys)
    oor = torch.zeros(1, dtype=torch.int32, device=env.engine.device)
    got = env.engine.encode_features_packed(h, env._packing_handle(), env.observation_packed(), bits=env.action_masks_packed(), out_of_range=oor)
    assert torch.equal(got.cpu(), want) and int(oor) == bad == 0
    h.close()


@pytest.mark.parametrize("dt", ["fp32", "fp16", "bf16"])
def test_packed_features_row_offsets_and_strides(dt):
    """out= whose rows all start one element off an even boundary (16-bit rows on an odd 2-byte boundary, fp32 rows 4-byte aligned
    and no more), and rows padded to whole lines: equal to the restatement; every element from F up to the stride and before / after the
    rows keeps its sentinel.  Without and with mask columns."""
    import torch
    env = Stepped.get("chain10")
    dtype = _dtypes()[dt]
    E = env.num_envs
    item = torch.empty((), dtype=dtype).element_size()
    packed, bits = env.observation_packed(), env.action_masks_packed()
    for include_masks in (False, True):
        want, _, _ = expected(env.topo, env.spec, _fields(env), env.action_masks() if include_masks else None)
        F = want.shape[1]
        line = 128 // item
        even = F + 2 + F % 2                                 # with an offset of one element every row starts on an odd element
        for label, stride, offset in (("odd offset", even, 1), ("padded", (F + line - 1) // line * line, 0)):
            flat = torch.full(((E + 2) * stride + offset,), SENTINEL, dtype=dtype, device=env.engine.device)
            rows = flat[offset:].view(E + 2, stride)
            assert all((rows[r].data_ptr() // item) % 2 == (1 if label == "odd offset" else 0) for r in (1, 2, E))
            got = env.encode_features_packed(packed, bits=bits if include_masks else None, out=rows[1:E + 1, :F])
            ctx = f"{dt} {label} masks={include_masks}"
            assert got.data_ptr() == rows[1].data_ptr() and tuple(got.shape) == (E, F), ctx
            b = rows.float().cpu()
            assert torch.equal(b[1:E + 1, :F], want), ctx
            assert (b[1:E + 1, F:] == SENTINEL).all(), ctx + ": elements past F were written"
            assert (b[0] == SENTINEL).all() and (b[E + 1] == SENTINEL).all() and (flat[:offset].float() == SENTINEL).all(), ctx


@pytest.mark.parametrize("name", ["chain10", "toyctf"])
def test_packed_features_through_an_index(name):
    """index permutes, repeats and is shorter / longer than the stored rows; packed and bits are both read at index[i] (their rows
    wider than needed): the restatement of the index_selected fields, bitwise encode_features on them."""
    import torch
    env = Stepped.get(name)
    E = env.num_envs
    fields = _fields(env)
    packed, bits, masks = env.observation_packed(), env.action_masks_packed(), env.action_masks()
    for n, with_masks, dtype in ((E + 12, True, torch.float32), (131, True, torch.bfloat16), (131, False, torch.float16)):
        idx = shuffled_index(E, n, n, packed.device)
        sel = {k: v.index_select(0, idx).contiguous() for k, v in fields.items()}
        want, bad, _ = expected(env.topo, env.spec, sel, masks.index_select(0, idx) if with_masks else None)
        oor = torch.zeros(1, dtype=torch.int32, device=packed.device)
        got = env.encode_features_packed(packed, bits=bits if with_masks else None, index=idx, dtype=dtype, out_of_range=oor)
        assert tuple(got.shape) == tuple(want.shape) and torch.equal(got.float().cpu(), want) and int(oor) == bad == 0
        ref = env.encode_features(sel, bits=bits.index_select(0, idx) if with_masks else None, dtype=dtype)
        assert torch.equal(got, ref)


def test_injected_out_of_range_values():
    """-1, n_s and 2^31 - 1 written into chosen elements of each of the five fields of a copy: packed as the code n_s and counted;
    the features show those groups all zero with their neighbours intact, rows and count as the int32 path gives them."""
    import torch
    env = Stepped.get("toyctf")
    fields = {k: v.clone() for k, v in _fields(env).items()}
    E = env.num_envs
    codes, _, word, shift, words, shapes = restate_format(env.topo, env.spec)
    off = np.cumsum([0] + [int(np.prod(shapes[k])) for k in FIELDS])
    # (field, row, flat element of the row, kind of bad value)
    spots = [("scalars", 0, 6, "n"), ("scalars", 1, 3, "neg"), ("scalars", 2, 0, "max"),
             ("leaked_credentials", 3, 5, "n"), ("leaked_credentials", 3, 6, "neg"), ("leaked_credentials", 4, 0, "max"),
             ("credential_cache_matrix", 5, 4, "neg"), ("credential_cache_matrix", 5, 7, "n"), ("credential_cache_matrix", E - 1, 1, "max"),
             ("discovered_nodes_properties", 9, 15, "n"), ("discovered_nodes_properties", 9, 17, "max"), ("discovered_nodes_properties", 10, 0, "neg"),
             ("nodes_privilegelevel", E - 1, 11, "n"), ("nodes_privilegelevel", E - 2, 0, "neg"), ("nodes_privilegelevel", 7, 5, "max")]
    for k, r, e, kind in spots:
        n_s = int(codes[off[FIELDS.index(k)] + e])
        fields[k][r].view(-1)[e] = {"n": n_s, "neg": -1, "max": 2 ** 31 - 1}[kind]
    want_words, bad_pack, _ = restated_rows(env, fields)
    assert bad_pack == len(spots)
    h = env._packing_handle()
    oor = torch.full((1,), 100, dtype=torch.int32, device=env.engine.device)
    packed = env.engine.pack_observation(h, fields, out_of_range=oor)
    assert np.array_equal(as_u32(packed), want_words) and int(oor) == 100 + len(spots)
    back = env.unpack_observation(packed)
    clean = _fields(env)
    for k, r, e, _ in spots:
        assert int(back[k][r].view(-1)[e]) == int(codes[off[FIELDS.index(k)] + e]), (k, r, e)
        back[k][r].view(-1)[e] = clean[k][r].view(-1)[e]
    assert all(torch.equal(back[k], clean[k]) for k in FIELDS)              # every other value is intact
    want, bad, _ = expected(env.topo, env.spec, fields)
    assert bad == len(spots)
    foor = torch.zeros(1, dtype=torch.int32, device=env.engine.device)
    got = env.encode_features_packed(packed, out_of_range=foor)
    assert torch.equal(got.cpu(), want) and int(foor) == bad
    ioor = torch.zeros(1, dtype=torch.int32, device=env.engine.device)
    assert torch.equal(got, env.encode_features(fields, out_of_range=ioor)) and int(ioor) == bad
    # the groups are all zero and nothing else changed: ones = elements - injected, row by row
    lay = env.feature_layout()
    ones = got.sum(dim=1).cpu()
    per_row = np.zeros(E, np.int64)
    for _, r, _, _ in spots:
        per_row[r] += 1
    assert np.array_equal(ones.numpy().astype(np.int64), lay.n_elements - per_row)


def test_index_outside_the_stored_rows_gives_zero_rows():
    """-1 and n_source_rows among valid entries of the index: a defined result of the bounds check — those rows all zero, out_of_range
    grown by n_elements each, every other row correct; unpack returns such a row as out-of-range codes.  (The stored rows are a slice
    from the middle of a larger allocation that holds other rows before and after it.)"""
    import torch
    env = Stepped.get("chain10")
    m = 200
    live, live_bits = env.observation_packed(), env.action_masks_packed()
    packed, bits = torch.cat([live[-8:], live])[8:8 + m], torch.cat([live_bits[-8:], live_bits])[8:8 + m]
    idx = torch.tensor([5, -1, 0, m, m - 1, 17, -1, 5], dtype=torch.int64, device=packed.device)
    valid = ((idx >= 0) & (idx < m)).cpu()
    safe = idx.clamp(0, m - 1)
    sel = {k: v[:m].index_select(0, safe).contiguous() for k, v in _fields(env).items()}
    lay = env.feature_layout(include_masks=True)
    want, bad, _ = expected(env.topo, env.spec, sel, env.action_masks()[:m].index_select(0, safe))
    want[~valid] = 0
    oor = torch.full((1,), 3, dtype=torch.int32, device=packed.device)
    buf = torch.full((len(idx) + 1, lay.width + 4), SENTINEL, dtype=torch.float32, device=packed.device)
    got = env.encode_features_packed(packed, bits=bits, index=idx, out=buf[:len(idx)], out_of_range=oor)
    assert torch.equal(got.cpu(), want)
    assert bad == 0 and int(oor) == 3 + int((~valid).sum()) * lay.n_elements
    b = buf.cpu()
    assert (b[:len(idx), lay.width:] == SENTINEL).all() and (b[len(idx)] == SENTINEL).all()
    codes, _, _, _, _, shapes = restate_format(env.topo, env.spec)
    back = env.unpack_observation(packed, index=idx)
    flat = flat_values(host_fields(back))
    assert np.array_equal(flat[valid.numpy()], flat_values(host_fields(sel))[valid.numpy()])
    assert (flat[~valid.numpy()] == codes).all()


def test_refusals():
    """Rows narrower than W_obs, a wrong dtype, row counts that differ, an index on the host or of another dtype, a missing field:
    refused by the Python layer; short rows, a NULL field, more rows than stored without an index, a layout with more classes than the
    packing has codes and malformed code counts by the C ABI."""
    import ctypes as C
    import torch
    from marlon_amd._abi import ObsBuffers
    env = Stepped.get("chain10")
    eng, lib, h = env.engine, env.engine.lib, env._packing_handle()
    W, E = h.words, env.num_envs
    packed = env.observation_packed()
    with pytest.raises(ValueError, match="contiguous rows"):
        eng.pack_observation(h, _fields(env), out=torch.zeros((E, W - 1), dtype=torch.int32, device=eng.device))
    with pytest.raises(ValueError, match="contiguous rows"):
        eng.pack_observation(h, _fields(env), out=torch.zeros((E, W), dtype=torch.int64, device=eng.device))
    with pytest.raises(ValueError, match="rows"):
        eng.pack_observation(h, _fields(env), out=torch.zeros((E - 1, W), dtype=torch.int32, device=eng.device))
    with pytest.raises(ValueError, match="all five"):
        eng.pack_observation(h, {k: v for k, v in _fields(env).items() if k != "scalars"})
    with pytest.raises(ValueError, match="int64"):
        env.unpack_observation(packed, index=torch.zeros(4, dtype=torch.int32, device=eng.device))
    with pytest.raises(ValueError, match="int64"):
        env.encode_features_packed(packed, index=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="bits"):
        env.encode_features_packed(packed, bits=env.action_masks_packed()[:E - 1])
    with pytest.raises(ValueError, match="contiguous rows"):
        env.encode_features_packed(packed[:, :W - 1])
    ob = ObsBuffers(**{k: v.data_ptr() for k, v in _fields(env).items()})
    st = eng._stream()
    out = torch.full((E, W), WORD_SENTINEL, dtype=torch.int32, device=eng.device)
    assert lib.mcbs_pack_observation(eng._h, h.ptr, C.byref(ob), out.data_ptr(), W - 1, E, None, st) == -1 and b"shorter" in lib.mcbs_last_error()
    assert lib.mcbs_pack_observation(eng._h, h.ptr, C.byref(ObsBuffers(scalars=_fields(env)["scalars"].data_ptr())), out.data_ptr(), W, E, None, st) == -1
    assert b"NULL" in lib.mcbs_last_error()
    assert lib.mcbs_unpack_observation(eng._h, h.ptr, packed.data_ptr(), W, None, E, E + 1, C.byref(ob), st) == -1 and b"no index" in lib.mcbs_last_error()
    other = Stepped.get("toyctf")
    assert lib.mcbs_pack_observation(eng._h, other._packing_handle().ptr, C.byref(ob), out.data_ptr(), W, E, None, st) == -1
    assert b"geometry" in lib.mcbs_last_error()
    torch.cuda.synchronize()
    assert bool((out == WORD_SENTINEL).all())
    V = env.observation_packing().values_per_row
    hh = C.c_void_p()
    codes = np.asarray(env.observation_packing().valid_codes, np.uint32)

    def create(c):
        c = np.ascontiguousarray(c, np.uint32)
        return lib.mcbs_obs_packing_create(eng._h, c.ctypes.data, c.size, C.byref(hh))

    assert create(codes[:V - 1]) == -1 and b"values of a row" in lib.mcbs_last_error()
    bad = codes.copy()
    bad[3] = 0
    assert create(bad) == -2
    bad[3] = 65537
    assert create(bad) == -2
    # a packing with fewer valid codes than the layout has classes cannot serve it
    small = codes.copy()
    small[0] = 2
    assert create(small) == 0
    lay = env._feature_handle(False, False)
    feats = torch.empty((E, lay.width), dtype=torch.float32, device=eng.device)
    assert lib.mcbs_encode_features_packed(eng._h, lay.ptr, hh, packed.data_ptr(), W, None, 0, None, E, feats.data_ptr(), 0, lay.width, E, None, st) == -1
    assert b"valid codes" in lib.mcbs_last_error()
    lib.mcbs_obs_packing_destroy(hh)
    big = np.full(V, 65536, np.uint32)                       # 17 bits each: one value per word, the format's widest field
    assert create(big) == 0 and lib.mcbs_obs_packing_words(hh) == V
    lib.mcbs_obs_packing_destroy(hh)


@pytest.mark.parametrize("credentials,staged", [(102, True), (800, False)])
def test_large_layout_round_trips_and_encodes(credentials, staged):
    """Chain-100 at 102/102 (1 761 values, 145 words a row, 30 000 one-hot columns), stepped as the int32 encoder's large-topology test,
    and at 102/800 (3 157 values: four rows of decoded values no longer fit the encoder's LDS budget, it decodes per column instead):
    pack equals the restatement and round-trips, the packed encoder equals the one_hot restatement in fp32 and fp16; at 102/102 also
    with mask columns on two rows, read through an index."""
    import torch
    from marlon_amd import engine, flatten
    from marlon_amd._abi import EnvSpec
    from marlon_amd.features import FeatureLayout, ObservationPacking
    from marlon_amd.samples import chainpattern
    topo = flatten.flatten(chainpattern.new_environment(100))
    E = 6
    spec = EnvSpec(n_envs=E, maximum_node_count=102, maximum_total_credentials=credentials, auto_reset=True, seed=1)
    eng = engine.BatchEngine(topo, spec)
    obs = eng.alloc_obs(FIELDS)
    for t in range(120):
        a = eng.sample_actions(True, seed=3, step=t)
        if t == 119:
            eng.step_observe(a, obs)
        else:
            eng.step(a)
    codes, _, word, shift, words, _ = restate_format(topo, spec)
    assert (4 * len(codes) * 4 <= 48 * 1024) == staged
    want_words, bad_pack = restate_pack(flat_values(host_fields(obs)), codes, word, shift, words)
    hp = eng.observation_packing(ObservationPacking(topo, spec))
    assert hp.words == words and bad_pack == 0 and (words == 145 or not staged)
    packed = eng.pack_observation(hp, obs)
    assert np.array_equal(as_u32(packed), want_words)
    back = eng.unpack_observation(hp, packed)
    assert all(torch.equal(back[k], obs[k]) for k in FIELDS)
    h = eng.feature_layout(FeatureLayout(topo, spec))
    want, bad, _ = expected(topo, spec, obs)
    assert bad == 0
    oor = torch.zeros(1, dtype=torch.int32, device=eng.device)
    for dtype in (torch.float32, torch.float16):
        got = eng.encode_features_packed(h, hp, packed, dtype=dtype, out_of_range=oor)
        assert torch.equal(got.float().cpu(), want)
    assert int(oor) == 0
    h.close()
    if not staged:                                           # (67 M Discrete actions a row: no mask columns here)
        hp.close()
        eng.close()
        return
    hm = eng.feature_layout(FeatureLayout(topo, spec, include_masks=True))
    bits = eng.pack_action_mask()[:2]
    wantm, _, _ = expected(topo, spec, {k: v[:2] for k, v in obs.items()}, eng.unpack_action_mask(bits))
    idx = torch.tensor([1, 0], dtype=torch.int64, device=eng.device)
    gotm = eng.encode_features_packed(hm, hp, packed[:2], bits=bits, index=idx, dtype=torch.bfloat16)
    assert tuple(gotm.shape) == tuple(wantm.shape) and torch.equal(gotm.float().cpu(), wantm[[1, 0]])
    hm.close()
    hp.close()
    eng.close()


def test_rollout_buffer_with_packed_observations():
    """rollout_buffer(4, pack_observations=True) on 320 Chain-10 envs filled in place over four steps next to an unpacked buffer filled
    from the same steps: for every minibatch of get(256), encode_features_packed(storage, bits=storage, index=batch.index) equals
    encode_features of the unpacked buffer's rows at the same index, and batch.observations["packed"] is the storage at index."""
    import torch
    from marlon_amd.samples import chainpattern
    from marlon_amd.wrappers import AttackerVecEnv
    E, T = 320, 4
    env = AttackerVecEnv(chainpattern.new_environment(10), E, maximum_node_count=12, maximum_total_credentials=12, discrete=True, seed=2,
                         materialize_masks=False)
    dev = env.engine.device
    buf = env.rollout_buffer(T, pack_observations=True)
    plain = env.rollout_buffer(T)
    W = env.observation_packing().words
    assert list(buf.observations) == ["packed"] and tuple(buf.observations["packed"].shape) == (T, E, W)
    assert buf.observations["packed"].dtype == torch.int32 and sorted(plain.observations) == sorted(FIELDS)
    g = torch.Generator(device=dev).manual_seed(6)
    zeros = torch.zeros(E, device=dev)
    for t in range(T):
        for _ in range(25):                                  # steps between stored ones: the stored rows differ
            m = env.unpack_action_mask(env.action_masks_packed())
            scores = torch.rand(m.shape, generator=g, device=dev)
            env.step(torch.where(m, scores, torch.full_like(scores, -1.0)).argmax(dim=1))
        env.observation_packed(out=buf.observations["packed"][buf.pos])
        env.action_masks_packed(out=buf.mask_bits[buf.pos])
        rewards = torch.rand(E, generator=g, device=dev)
        buf.add(None, zeros.long(), rewards, zeros, zeros, zeros)
        plain.add(env.observation_fields, zeros.long(), rewards, zeros, zeros, zeros, bits=buf.mask_bits[t])
    assert not torch.equal(buf.observations["packed"][0], buf.observations["packed"][T - 1])
    for b in (buf, plain):
        b.compute_returns_and_advantage(zeros, zeros)
    storage, bits = buf.observations["packed"].view(T * E, -1), buf.mask_bits.view(T * E, -1)
    gen = torch.Generator(device=dev).manual_seed(8)
    seen = 0
    for batch in buf.get(256, generator=gen):
        n = batch.index.shape[0]
        seen += n
        assert torch.equal(batch.observations["packed"], storage.index_select(0, batch.index))
        x = env.encode_features_packed(storage, bits=bits, index=batch.index, dtype=torch.bfloat16)
        sel = {k: v.view((T * E,) + tuple(v.shape[2:])).index_select(0, batch.index) for k, v in plain.observations.items()}
        want = env.encode_features(sel, bits=plain.mask_bits.view(T * E, -1).index_select(0, batch.index), dtype=torch.bfloat16)
        assert tuple(x.shape) == (n, env.feature_layout(include_masks=True).width) and torch.equal(x, want)
    assert seen == T * E
    env.close()
