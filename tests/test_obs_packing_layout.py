"""marlon_amd/features.py ObservationPacking on the host: the packed row format of include/mcbs.h "packed observations" (valid codes,
bit widths, words and shifts) against a restatement written here from the class counts of the reference's spaces, `pack_host` /
`unpack_host` against that restatement, and the C ABI's refusals without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from marlon_amd import engine, flatten
from marlon_amd._abi import EnvSpec
from marlon_amd.samples import chainpattern, toy_ctf
from tests.test_feature_layout import ARRAYS, SCALARS, dims, key_classes

FIELDS = ["scalars"] + ARRAYS
CASES = {"chain10": (lambda: chainpattern.new_environment(10), 12, 12), "toyctf": (toy_ctf.new_environment, 12, 10),
         "chain100": (lambda: chainpattern.new_environment(100), 102, 102)}
NEW_SYMBOLS = ["mcbs_obs_packing_create", "mcbs_obs_packing_destroy", "mcbs_obs_packing_words", "mcbs_pack_observation",
               "mcbs_unpack_observation", "mcbs_encode_features_packed"]


def case(name):
    make, N, Cm = CASES[name]
    topo = flatten.flatten(make())
    return topo, EnvSpec(n_envs=1, maximum_node_count=N, maximum_total_credentials=Cm)


def restate_format(topo, spec):
    """-> (valid codes, bits, word, shift, words, field shapes) of a row's values in source order: the class counts of the reference's
    spaces with C + 1 and N + 1 codes for the two counts, bit_length bits each, placed from bit 0 of word 0 without straddling a word."""
    N, Cm, K, L, R, P, NP = dims(topo, spec)
    classes, _ = key_classes(N, Cm, K, L, R, P, NP, False)
    codes = [classes[k][0] for k in SCALARS] + [n for k in ARRAYS for n in classes[k]]
    bits, word, shift = [], [], []
    w = s = 0
    for n in codes:
        b = n.bit_length()
        if s + b > 32:
            w, s = w + 1, 0
        bits.append(b)
        word.append(w)
        shift.append(s)
        s += b
    shapes = {"scalars": (7,), "leaked_credentials": (K, 4), "credential_cache_matrix": (Cm, 2), "discovered_nodes_properties": (N, NP),
              "nodes_privilegelevel": (N,)}
    return np.array(codes), np.array(bits), np.array(word), np.array(shift), w + (1 if s else 0), shapes


def flat_values(obs):
    """dict of the five fields [n, ...] -> int64 [n, V] in source order"""
    n = len(obs["scalars"])
    return np.concatenate([np.asarray(obs[k]).reshape(n, -1).astype(np.int64) for k in FIELDS], axis=1)


def restate_pack(values, codes, word, shift, words):
    """int64 [n, V] -> (uint32 [n, words], values stored as their out-of-range code) in a plain loop"""
    out = np.zeros((values.shape[0], words), dtype=np.uint64)
    bad = 0
    for r in range(values.shape[0]):
        for i, v in enumerate(values[r]):
            ok = 0 <= v < codes[i]
            bad += not ok
            out[r, word[i]] |= np.uint64(int(v if ok else codes[i]) << int(shift[i]))
    return out.astype(np.uint32), bad


def random_rows(rng, codes, shapes, n):
    vals = rng.integers(0, 1 << 30, size=(n, len(codes))) % codes
    out, o = {}, 0
    for k in FIELDS:
        ln = int(np.prod(shapes[k]))
        out[k] = vals[:, o:o + ln].reshape((n,) + shapes[k]).astype(np.int32)
        o += ln
    return out, vals


@pytest.mark.parametrize("name", list(CASES))
def test_layout_equals_the_restated_format(name):
    from marlon_amd.features import ObservationPacking
    topo, spec = case(name)
    codes, bits, word, shift, words, _ = restate_format(topo, spec)
    p = ObservationPacking(topo, spec)
    for got, want in ((p.valid_codes, codes), (p.bits, bits), (p.word, word), (p.shift, shift)):
        assert len(got) == len(want) == p.values_per_row and np.array_equal(np.asarray(got), want)
    assert p.words == words
    if name != "chain100":
        assert words == {"chain10": 18, "toyctf": 14}[name]
    assert (shift + bits <= 32).all() and (2 ** bits > codes).all()            # no straddling, a spare code everywhere


@pytest.mark.parametrize("name", ["chain10", "toyctf"])
def test_pack_host_round_trips_and_clamps(name):
    from marlon_amd.features import ObservationPacking
    topo, spec = case(name)
    codes, bits, word, shift, words, shapes = restate_format(topo, spec)
    p = ObservationPacking(topo, spec)
    rng = np.random.default_rng(7)
    obs, vals = random_rows(rng, codes, shapes, 9)
    packed = p.pack_host(obs)
    want, bad = restate_pack(vals, codes, word, shift, words)
    assert bad == 0 and packed.dtype == np.uint32 and packed.shape == (9, words) and np.array_equal(packed, want)
    back = p.unpack_host(packed)
    for k in FIELDS:
        assert back[k].dtype == np.int32 and back[k].shape == obs[k].shape and np.array_equal(back[k], obs[k]), k
    assert np.array_equal(p.unpack_host(packed.view(np.int32))["scalars"], obs["scalars"])       # the device tensors' dtype
    # padding bits are zero (nothing outside the fields' bits is set), and so are a field's bits above its code (it reads below n_s)
    used = np.zeros(words, dtype=np.uint64)
    for i in range(len(codes)):
        used[word[i]] |= np.uint64(((1 << int(bits[i])) - 1) << int(shift[i]))
    assert not (packed.astype(np.uint64) & ~used).any()
    assert (flat_values(back) < codes).all()
    # -1, n_s and 2^31 - 1 come back as n_s, in every value position; the neighbours are intact
    for v_bad in (-1, None, 2 ** 31 - 1):
        edited = vals.copy()
        pos = np.arange(0, len(codes), 3)
        edited[0, pos] = codes[pos] if v_bad is None else v_bad
        o, eo = 0, {}
        for k in FIELDS:
            ln = int(np.prod(shapes[k]))
            eo[k] = edited[:, o:o + ln].reshape((9,) + shapes[k]).astype(np.int32)
            o += ln
        pk = p.pack_host(eo)
        want, bad = restate_pack(edited, codes, word, shift, words)
        assert bad == len(pos) and np.array_equal(pk, want)
        got = flat_values(p.unpack_host(pk))
        expect = vals.copy()
        expect[0, pos] = codes[pos]
        assert np.array_equal(got, expect)


@pytest.mark.parametrize("reference_counts", [False, True])
def test_features_of_unpacked_rows_equal_features_of_the_rows(reference_counts):
    """encode_host(unpack_host(pack_host(x))) == encode_host(x), rows and out-of-range count, on rows holding full counts (in range only
    without reference_counts) and injected -1 / n_s / 2^31 - 1."""
    from marlon_amd.features import FeatureLayout, ObservationPacking
    topo, spec = case("chain10")
    codes, _, _, _, _, shapes = restate_format(topo, spec)
    p = ObservationPacking(topo, spec)
    lay = FeatureLayout(topo, spec, reference_counts=reference_counts)
    obs, _ = random_rows(np.random.default_rng(3), codes, shapes, 12)
    obs["scalars"][:, 5:7] %= 12                             # (the random rows hold no full count of their own)
    obs["scalars"][0, 5] = 12                                # credential_cache_length = C: class C of C + 1, beyond Discrete(C)
    obs["scalars"][1, 6] = 12                                # discovered_node_count = N
    obs["scalars"][2, 3] = -1
    obs["leaked_credentials"][3, 2, 1] = 12                  # cache index C of Discrete(C): the out-of-range code itself
    obs["credential_cache_matrix"][4, 1, 0] = 2 ** 31 - 1
    obs["discovered_nodes_properties"][5, 7, 2] = 3
    obs["nodes_privilegelevel"][6, 11] = -7
    want, bad = lay.encode_host(obs, return_out_of_range=True)
    got, got_bad = lay.encode_host(p.unpack_host(p.pack_host(obs)), return_out_of_range=True)
    assert bad == got_bad == (7 if reference_counts else 5)
    assert np.array_equal(got, want)


def test_header_and_exports_name_the_packing():
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mcbs.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mcbs_[a-z_]+)\s*\(", text))
    lib = engine.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared and name in engine.EXPORTS and hasattr(lib, name), name


def test_entry_points_refuse_null_arguments_without_a_gpu():
    lib = engine.load_library()
    h = C.c_void_p()
    codes = np.ones(4, np.uint32)
    assert lib.mcbs_obs_packing_create(None, codes.ctypes.data, 4, C.byref(h)) == -1 and b"null" in lib.mcbs_last_error()
    assert lib.mcbs_obs_packing_create(None, None, 0, None) == -1
    assert lib.mcbs_obs_packing_words(None) == 0
    lib.mcbs_obs_packing_destroy(None)
    assert lib.mcbs_pack_observation(None, None, None, None, 0, 0, None, None) == -1 and b"null" in lib.mcbs_last_error()
    assert lib.mcbs_unpack_observation(None, None, None, 0, None, 0, 0, None, None) == -1 and b"null" in lib.mcbs_last_error()
    assert lib.mcbs_encode_features_packed(None, None, None, None, 0, None, 0, None, 0, None, 0, 0, 0, None, None) == -1
    assert b"null" in lib.mcbs_last_error()
