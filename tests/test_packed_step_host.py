"""The host side of the packed wrapper step (mcbs_attacker_wrapper_step_packed, marlon_amd/csrc/mcbs_wrapper_fused.hip): the word table
`ObservationPacking.word_first` — the values of a packed word are one contiguous run of the descriptor table — against a restatement
of the placement rule of include/mcbs.h "packed observations", and the row sizes the step accepts for every bound the one-launch step
is tested under."""
import numpy as np
import pytest

from marlon_amd import flatten
from marlon_amd._abi import EnvSpec
from marlon_amd.samples import chainpattern, tinytoy, toy_ctf
from tests.test_obs_packing_layout import restate_format

CASES = {"chain10": (lambda: chainpattern.new_environment(10), 12, 12), "toyctf": (toy_ctf.new_environment, 12, 10),
         "tiny": (tinytoy.new_environment, 3, 1), "chain4": (lambda: chainpattern.new_environment(4), 6, 6)}


def restate_word_first(codes):
    """First value index of every word, then V: values are placed in source order from bit 0 of word 0, bit_length(n) bits each, and one
    that does not fit in what is left of a word opens the next."""
    first, used = [], 32                              # (no word is open before the first value)
    for s, n in enumerate(codes):
        b = int(n).bit_length()
        if used + b > 32:
            first.append(s)
            used = 0
        used += b
    return first + [len(codes)]


@pytest.mark.parametrize("name", list(CASES))
def test_word_first_equals_the_restated_placement(name):
    from marlon_amd.features import ObservationPacking
    make, N, Cm = CASES[name]
    topo = flatten.flatten(make())
    spec = EnvSpec(n_envs=1, maximum_node_count=N, maximum_total_credentials=Cm)
    codes, bits, word, shift, words, _ = restate_format(topo, spec)
    p = ObservationPacking(topo, spec)
    V = p.values_per_row
    wf = np.asarray(p.word_first)
    assert wf.tolist() == restate_word_first(codes) and len(wf) == p.words + 1 == words + 1
    # the runs partition range(V) in order ...
    assert wf[0] == 0 and wf[-1] == V and (np.diff(wf) > 0).all()
    assert np.concatenate([np.arange(wf[w], wf[w + 1]) for w in range(p.words)]).tolist() == list(range(V))
    # ... and every value's word is the run it lies in
    for w in range(p.words):
        assert (np.asarray(p.word)[wf[w]:wf[w + 1]] == w).all(), f"{name}: word {w}"
        assert int(np.asarray(p.bits)[wf[w]:wf[w + 1]].sum()) <= 32
    assert (np.searchsorted(wf, np.arange(V), side="right") - 1 == np.asarray(p.word)).all()


@pytest.mark.parametrize("topology", ["chain4", "toyctf", "tiny"])
def test_rows_stay_within_the_room_the_step_keeps(topology):
    """Every (maximum_node_count, maximum_total_credentials) that test_one_launch_wrapper_step_over_observation_bounds steps: the packed
    row fits the LDS room of the packed step (include/mcbs.h: W_obs <= 128 words, W_obs + 1 + V <= 896 table entries)."""
    from marlon_amd.features import PACKED_STEP_MAX_WORDS, PACKED_STEP_TABLE_ENTRIES, ObservationPacking
    assert (PACKED_STEP_MAX_WORDS, PACKED_STEP_TABLE_ENTRIES) == (128, 896)
    make = {"chain4": lambda: chainpattern.new_environment(4), "toyctf": toy_ctf.new_environment, "tiny": tinytoy.new_environment}[topology]
    n, c = {"chain4": (6, 5), "toyctf": (10, 5), "tiny": (3, 1)}[topology]
    topo = flatten.flatten(make())
    tried = set()
    for nm, cm in ((n, c), (n + 1, c + 1), (n + 2, c + 4), (9, 7), (11, 3), (13, 11), (14, 6), (15, 13), (16, 16), (16, c), (n, 16)):
        nm, cm = max(nm, n), max(cm, c)
        if (nm, cm) in tried:
            continue
        tried.add((nm, cm))
        p = ObservationPacking(topo, EnvSpec(n_envs=1, maximum_node_count=nm, maximum_total_credentials=cm))
        assert p.words <= PACKED_STEP_MAX_WORDS and p.words + 1 + p.values_per_row <= PACKED_STEP_TABLE_ENTRIES, (topology, nm, cm, p.words)
        assert p.fits_packed_step
    assert len(tried) >= 8
