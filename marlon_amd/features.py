"""The policy's input features: the layout of the float row that Stable-Baselines3's "MultiInputPolicy" builds from the attacker
wrapper's Dict observation (preprocess_obs + CombinedExtractor; marlon/baseline_models/ppo/train.py:79, ppo_multi/train_marl_multi.py:275).

Every key of the observation becomes a run of columns — a `Discrete(n)` a one-hot of n, every element of a `MultiDiscrete(nvec)` a
one-hot of its own width, a `MultiBinary` its values as 0.0 / 1.0 — and the runs are concatenated in key order into one `[n, F]` row.
`FeatureLayout` describes that row for a topology and its observation bounds; `mcbs_encode_features` (marlon_amd/csrc/mcbs_features.hip)
writes it on the device in one launch from the descriptors this class builds, `encode_host` is the same encoding in NumPy.
`ObservationPacking` is the host mirror of the packed row format (include/mcbs.h "packed observations"): the same source values as bit
fields, what a rollout buffer stores per step and `mcbs_encode_features_packed` reads at update time.
`DefenderObservationPacking` is the same for the learned defender's four MultiBinary fields: one bit per element, in the column order
of `DefenderVecEnv.features()` (include/mcbs.h "packed defender observations").

Pure Python / NumPy: importable without a GPU and without the native library.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np

from ._abi import EnvSpec
from .flatten import FlatTopology

SCALAR_KEYS = ["newly_discovered_nodes_count", "lateral_move", "customer_data_found", "probe_result", "escalation",
               "credential_cache_length", "discovered_node_count"]
ARRAY_KEYS = ["leaked_credentials", "credential_cache_matrix", "discovered_nodes_properties", "nodes_privilegelevel"]
MASK_KEYS = ["connect", "local_vulnerability", "remote_vulnerability"]     # MaskedDiscreteAttackerWrapper's order (the packed bits')
# the int32 fields of mcbs_obs_buffers in the struct's order: a row's source values are these, flattened, one after the other
OBS_FIELDS = ["scalars", "leaked_credentials", "credential_cache_matrix", "discovered_nodes_properties", "nodes_privilegelevel"]

MAX_SOURCE, MAX_CLASSES = 1 << 15, 1 << 16        # what a 32-bit column descriptor holds (class 16 bits, source index 15, first flag 1)
FIRST = 1 << 31
# the LDS room mcbs_attacker_wrapper_step_packed keeps (include/mcbs.h): W_obs words for the fresh row, W_obs + 1 + V table entries
PACKED_STEP_MAX_WORDS, PACKED_STEP_TABLE_ENTRIES = 128, 896


class FeatureLayout:
    """Feature row of the attacker observation of `topo` under `spec`'s bounds.

    keys: the observation keys in the order of their column runs; default: every key sorted by name — how a `gymnasium.spaces.Dict`
        built from a plain dict orders its keys (gymnasium is not a dependency here, so this is stated, not checked: pass `keys` to
        impose another order or to leave keys out).
    include_masks: also the three action masks `connect`, `local_vulnerability`, `remote_vulnerability` (observation keys in the
        reference's spaces), copied as 0 / 1 from the bit-packed Discrete mask (`mcbs_pack_action_mask`'s format).
    reference_counts: the reference declares `credential_cache_length` as `Discrete(maximum_total_credentials)` and
        `discovered_node_count` as `Discrete(maximum_node_count)` (cyberbattle_env.py:307-309) although both counts REACH their bound
        (Chain-10 has 12 nodes at maximum_node_count = 12), where `one_hot` raises.  By default the two therefore get one class more
        than declared; `reference_counts=True` gives the reference's widths exactly, and a full count then encodes as an all-zero
        group and is counted as out of range.

    Class counts (N = maximum_node_count, C = maximum_total_credentials, K = maximum_discoverable_credentials_per_action, P = ports,
    NP = properties; cyberbattle_env.py:262-320, attack_wrapper.py:164-204): newly_discovered_nodes_count N+1; lateral_move,
    customer_data_found 2; probe_result 3; escalation 4; credential_cache_length C+1 (C); discovered_node_count N+1 (N);
    leaked_credentials K x (2, C, N, P); credential_cache_matrix C x (N, P); discovered_nodes_properties N*NP x 3;
    nodes_privilegelevel N x 4; the masks N*N*P*C, N*L and N*N*R single columns.

    A value outside [0, classes) leaves its group all zero (and never touches a neighbour); `encode_host(..., return_out_of_range=True)`
    and the device encoder's `out_of_range` count such elements.

    width: F.  segments: key -> (first column, columns).  groups: one (key, source index, classes) per one-hot element in row order.
    descriptors / mask_ranges: what `mcbs_feature_layout_create` takes (include/mcbs.h)."""

    def __init__(self, topo: FlatTopology, spec: EnvSpec, keys: Optional[Iterable[str]] = None, include_masks: bool = False,
                 reference_counts: bool = False):
        N, C, K = spec.maximum_node_count, spec.maximum_total_credentials, spec.maximum_discoverable_credentials_per_action
        L, R, P, NP = len(topo.local_vulnerabilities), len(topo.remote_vulnerabilities), len(topo.ports), len(topo.properties)
        self.N, self.C, self.K, self.L, self.R, self.P, self.NP = N, C, K, L, R, P, NP
        self.include_masks, self.reference_counts = bool(include_masks), bool(reference_counts)
        self.field_len = [7, K * 4, C * 2, N * NP, N]
        self.field_off = [int(x) for x in np.concatenate([[0], np.cumsum(self.field_len)[:-1]])]
        self.values_per_row = int(sum(self.field_len))
        scalar_classes = [N + 1, 2, 2, 3, 4, C if reference_counts else C + 1, N if reference_counts else N + 1]
        o = self.field_off
        # key -> [(source index, classes)] in element order
        elements: Dict[str, List[Tuple[int, int]]] = {k: [(i, scalar_classes[i])] for i, k in enumerate(SCALAR_KEYS)}
        elements["leaked_credentials"] = [(o[1] + 4 * k + j, n) for k in range(K) for j, n in enumerate((2, C, N, P))]
        elements["credential_cache_matrix"] = [(o[2] + 2 * c + j, n) for c in range(C) for j, n in enumerate((N, P))]
        elements["discovered_nodes_properties"] = [(o[3] + i, 3) for i in range(N * NP)]
        elements["nodes_privilegelevel"] = [(o[4] + i, 4) for i in range(N)]
        M, ML, MR = N * N * P * C, N * L, N * N * R
        self.discrete_n = M + ML + MR
        mask_bits = {"connect": (0, M), "local_vulnerability": (M, ML), "remote_vulnerability": (M + ML, MR)}
        known = list(elements) + (MASK_KEYS if include_masks else [])
        self.keys = sorted(known) if keys is None else list(keys)
        if len(set(self.keys)) != len(self.keys):
            raise ValueError("a key is listed twice")
        for k in self.keys:
            if k not in known:
                raise ValueError(f"unknown observation key {k!r}" + (" (the action masks need include_masks=True)" if k in MASK_KEYS else ""))
        self.segments: Dict[str, Tuple[int, int]] = {}
        self.groups: List[Tuple[str, int, int]] = []
        desc: List[int] = []
        ranges: List[Tuple[int, int, int]] = []
        col = 0
        for k in self.keys:
            if k in mask_bits:
                b0, n = mask_bits[k]
                if n:
                    ranges.append((col, n, b0))
                self.segments[k] = (col, n)
                col += n
                continue
            first = col
            for src, n in elements[k]:
                if n < 1 or n > MAX_CLASSES or src >= MAX_SOURCE:
                    raise ValueError(f"{k}: {n} classes / source value {src} do not fit a column descriptor "
                                     f"(at most {MAX_CLASSES} classes, {MAX_SOURCE} int32 values per observation row)")
                self.groups.append((k, src, n))
                desc.extend((FIRST if c == 0 else 0) | (src << 16) | c for c in range(n))
                col += n
            self.segments[k] = (first, col - first)
        self.width = col
        self.n_elements = len(self.groups)
        self.descriptors = np.asarray(desc, dtype=np.uint32)
        self.mask_ranges = np.asarray(ranges, dtype=np.uint32).reshape(-1, 3)
        self.mask_columns = int(self.mask_ranges[:, 1].sum()) if len(ranges) else 0
        self.mask_words = (self.discrete_n + 31) // 32         # words of a packed mask row (mcbs_pack_action_mask)

    def padded_width(self, itemsize: int) -> int:
        """F rounded up so that a row is a whole number of 128-byte lines: the row stride the wrappers allocate."""
        per_line = 128 // itemsize
        return (self.width + per_line - 1) // per_line * per_line

    # -- host encoding --
    def _values(self, obs: dict) -> np.ndarray:
        """[n, values_per_row] int64: the row's source values from a dict holding either the engine's fields (`scalars` [n, 7], ...) or
        the wrapper's public keys (the seven named counts [n] instead of `scalars`)."""
        if "scalars" in obs:
            sc = np.asarray(obs["scalars"]).reshape(-1, 7)
        else:                                         # a named count the layout leaves out may be absent: it reads as zero
            present = [k for k in SCALAR_KEYS + ARRAY_KEYS if k in obs]
            if not present:
                raise KeyError("observation holds none of the layout's keys")
            n = np.asarray(obs[present[0]]).shape[0]
            absent = [k for k in SCALAR_KEYS if k not in obs and k in self.segments]
            if absent:
                raise KeyError(f"observation lacks {absent}")
            sc = np.stack([np.asarray(obs[k]).reshape(n) if k in obs else np.zeros(n, np.int64) for k in SCALAR_KEYS], axis=1)
        n = sc.shape[0]
        parts = [sc.astype(np.int64)]
        for k, ln in zip(ARRAY_KEYS, self.field_len[1:]):
            if k in obs:
                parts.append(np.asarray(obs[k]).reshape(n, ln).astype(np.int64))
            elif k in self.segments:
                raise KeyError(f"observation lacks {k!r}")
            else:
                parts.append(np.zeros((n, ln), np.int64))
        return np.concatenate(parts, axis=1)

    def encode_host(self, obs: dict, dtype=np.float32, return_out_of_range: bool = False):
        """The feature rows [n, F] of a dict of host arrays with a leading row axis (the engine's fields or the wrapper's public
        observation keys; with mask columns also `connect` / `local_vulnerability` / `remote_vulnerability`, any shape after the row
        axis, non-zero = allowed).  With return_out_of_range: (rows, number of elements whose value lay outside [0, classes))."""
        vals = self._values(obs)
        n = vals.shape[0]
        out = np.zeros((n, self.width), dtype=dtype)
        rows = np.arange(n)
        bad = 0
        col = {k: c0 for k, (c0, _) in self.segments.items()}
        for k, src, ncls in self.groups:
            v = vals[:, src]
            ok = (v >= 0) & (v < ncls)
            out[rows[ok], col[k] + v[ok]] = 1
            bad += int((~ok).sum())
            col[k] += ncls
        for k in self.keys:
            if k in MASK_KEYS:
                c0, w = self.segments[k]
                out[:, c0:c0 + w] = (np.asarray(obs[k]).reshape(n, w) != 0)
        return (out, bad) if return_out_of_range else out

    # -- the first layer from the observation (include/mcbs.h "first layer from the observation") on the host --
    def _selected_columns(self, obs: dict, index=None):
        """-> (cols int64 [n, n_elements]: the column each element of each row selects, in row order, -1 where its value lies outside its
        classes; out-of-range count).  index: output row i is row index[i] of obs; an index outside the rows selects nothing and counts
        every element."""
        if self.mask_columns or any(k in MASK_KEYS for k in self.keys):
            raise ValueError("the first-layer calls serve layouts without mask columns (include_masks is out of scope)")
        vals = self._values(obs)
        inside = None
        if index is not None:
            index = np.asarray(index, dtype=np.int64)
            inside = (index >= 0) & (index < vals.shape[0])
            vals = vals[np.where(inside, index, 0)]
        cols = np.full((vals.shape[0], self.n_elements), -1, dtype=np.int64)
        col = 0
        for e, (_, src, ncls) in enumerate(self.groups):              # row order: the groups' columns follow each other
            v = vals[:, src]
            ok = (v >= 0) & (v < ncls)
            if inside is not None:
                ok &= inside
            cols[ok, e] = col + v[ok]
            col += ncls
        return cols, int((cols < 0).sum())

    def first_layer_host(self, obs: dict, weight_t, bias=None, out_dtype=np.float32, index=None, return_out_of_range: bool = False):
        """mcbs_first_layer[_packed] in NumPy float32, operation for operation in the contract's order: for every row ONE accumulator
        that starts at the bias (+0.0 without one) and takes one float32 add per element, in row order, of the weight column the
        element's value selects — torch.nn.functional.linear(encode_host(obs), weight_t.T, bias) summed in that order.
        weight_t [F, H] and bias [H]: float32 arrays (bfloat16 weights as the float32 values they widen to).  out_dtype: np.float32, or
        "bfloat16" for the result rounded to nearest even to bfloat16 and returned as the float32 values that holds.  index: as the
        packed form's (a row outside obs comes out as the bias alone, every element of it counted).  -> [n, H] float32, with
        return_out_of_range also the number of elements that selected nothing."""
        cols, bad = self._selected_columns(obs, index)
        w = np.ascontiguousarray(weight_t, dtype=np.float32)
        if w.ndim != 2 or w.shape[0] != self.width:
            raise ValueError(f"weight_t must be [{self.width}, H], got {w.shape}")
        n, H = cols.shape[0], w.shape[1]
        acc = np.zeros((n, H), dtype=np.float32)
        if bias is not None:
            acc[:] = np.asarray(bias, dtype=np.float32).reshape(1, H)  # acc STARTS at the bias (a -0.0 stays -0.0)
        for e in range(self.n_elements):
            ok = cols[:, e] >= 0
            acc[ok] = acc[ok] + w[cols[ok, e]]
        if out_dtype in ("bfloat16", "bf16"):
            acc = _round_to_bfloat16(acc)
        elif np.dtype(out_dtype) != np.float32:
            raise ValueError("out_dtype must be np.float32 or 'bfloat16'")
        return (acc, bad) if return_out_of_range else acc

    def first_layer_grad_host(self, obs: dict, grad_out, H: int, row_block: int = 512, index=None):
        """mcbs_first_layer_grad in NumPy float32, operation for operation in the contract's order -> (grad_weight_t [F, H], grad_bias
        [H]).  The rows are cut into blocks of row_block; a block's partial of (column c, h) starts at +0.0 and does s = s + grad_out[i, h]
        over the block's rows, in ascending i, whose element selects c (the bias row: over all of them); the result is the partials added
        in ascending block order starting from partial 0.  A row whose index lies outside obs contributes to grad_bias only."""
        cols, _ = self._selected_columns(obs, index)
        g = np.ascontiguousarray(grad_out, dtype=np.float32)
        n, F = cols.shape[0], self.width
        if g.shape != (n, H):
            raise ValueError(f"grad_out must be [{n}, {H}], got {g.shape}")
        total = np.zeros((F + 1, H), dtype=np.float32)
        for b0 in range(0, n, row_block):
            part = np.zeros((F + 1, H), dtype=np.float32)
            for i in range(b0, min(b0 + row_block, n)):
                c = cols[i]
                c = np.append(c[c >= 0], F)                           # a row's columns are distinct: one add each
                part[c] = part[c] + g[i]
            total = part if b0 == 0 else total + part
        return total[:F], total[F]


def _round_to_bfloat16(x: np.ndarray) -> np.ndarray:
    """float32 -> the float32 values of x rounded to nearest even to bfloat16 (a NaN stays a quiet NaN): the device's rule restated"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (u >> 16) | 0x40, (u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return (r << 16).astype(np.uint32).view(np.float32).reshape(x.shape)


class ObservationPacking:
    """The packed row format of the attacker observation of `topo` under `spec`'s bounds (include/mcbs.h "packed observations"): the
    host mirror of what `mcbs_pack_observation` writes and `mcbs_unpack_observation` / `mcbs_encode_features_packed` read.

    A row's source values are the V int32 values of the five fields (`OBS_FIELDS`), flattened in that order.  Value s has
    `valid_codes[s]` = n_s valid codes 0 .. n_s - 1: the class count `FeatureLayout(topo, spec)` gives it with reference_counts=False
    (the two counts keep C + 1 and N + 1 codes, so a packed row serves either feature layout).  It occupies `bits[s]` =
    n_s.bit_length() bits — always one spare code at least — at bit `shift[s]` of word `word[s]`: fields follow each other in source
    order from bit 0 of word 0, and one that does not fit in what is left of a word starts the next (no field straddles a word; unused
    bits are 0).  The stored code is v where 0 <= v < n_s, and n_s — the out-of-range code — for anything else; unpacking returns
    the code.  `words`: the uint32 words of a row.  `word_first` [words + 1]: the values of word w are the contiguous run
    word_first[w] .. word_first[w + 1] - 1 (the mirror of the table mcbs_obs_packing_create uploads for the packed wrapper step).

    valid_codes, bits, word, shift: int arrays [V].  Pure NumPy."""

    def __init__(self, topo: FlatTopology, spec: EnvSpec):
        lay = FeatureLayout(topo, spec)
        self.field_len, self.field_off, self.values_per_row = lay.field_len, lay.field_off, lay.values_per_row
        self.field_shape = [(7,), (lay.K, 4), (lay.C, 2), (lay.N, lay.NP), (lay.N,)]
        codes = np.zeros(self.values_per_row, dtype=np.int64)
        for _, src, n in lay.groups:
            codes[src] = n
        if (codes < 1).any() or (codes > MAX_CLASSES).any():
            raise ValueError(f"a source value has no element or more than {MAX_CLASSES} classes")
        self.valid_codes = codes
        self.bits = np.array([int(n).bit_length() for n in codes], dtype=np.int64)
        self.word = np.zeros_like(codes)
        self.shift = np.zeros_like(codes)
        w = s = 0
        first = [0]
        for i, b in enumerate(self.bits):
            if s + b > 32:
                w, s = w + 1, 0
                first.append(i)
            self.word[i], self.shift[i] = w, s
            s += int(b)
        self.words = w + (1 if s else 0)
        self.word_first = np.array(first[:self.words] + [self.values_per_row], dtype=np.int64)

    @property
    def fits_packed_step(self) -> bool:
        """Whether the one-launch wrapper step can write these rows itself (mcbs_attacker_wrapper_step_packed keeps the fresh row and both
        tables in LDS)."""
        return self.words <= PACKED_STEP_MAX_WORDS and self.words + 1 + self.values_per_row <= PACKED_STEP_TABLE_ENTRIES

    def _fields(self, vals: np.ndarray) -> dict:
        n = vals.shape[0]
        return {k: vals[:, o:o + ln].reshape((n,) + shp).astype(np.int32)
                for k, o, ln, shp in zip(OBS_FIELDS, self.field_off, self.field_len, self.field_shape)}

    def pack_host(self, obs: dict) -> np.ndarray:
        """uint32 [n, words] of a dict of the five int32 fields with a leading row axis (`scalars` [n, 7], ... in any trailing shape)."""
        vals = np.concatenate([np.asarray(obs[k]).reshape(len(obs["scalars"]), ln).astype(np.int64)
                               for k, ln in zip(OBS_FIELDS, self.field_len)], axis=1)
        code = np.where((vals >= 0) & (vals < self.valid_codes), vals, self.valid_codes).astype(np.uint64)
        out = np.zeros((vals.shape[0], self.words), dtype=np.uint64)
        for i in range(self.values_per_row):                     # (fields of a word do not overlap: adding is OR-ing)
            out[:, self.word[i]] += code[:, i] << np.uint64(self.shift[i])
        return out.astype(np.uint32)

    def unpack_host(self, packed) -> dict:
        """The five int32 fields (codes) of uint32 / int32 rows [n, >= words]."""
        p = np.asarray(packed)
        p = (p.view(np.uint32) if p.dtype == np.int32 else p.astype(np.uint32)).astype(np.uint64)
        vals = (p[:, self.word] >> self.shift.astype(np.uint64)) & ((np.uint64(1) << self.bits.astype(np.uint64)) - np.uint64(1))
        return self._fields(vals.astype(np.int64))


DEFENDER_KEYS = ("incoming_firewall_status", "infected_nodes", "outgoing_firewall_status", "services_status")     # sorted key order


class DefenderObservationPacking:
    """The packed row of the learned defender's observation of `topo` (include/mcbs.h "packed defender observations"): the host mirror
    of what `mcbs_defender_observe_packed` / `mcbs_pack_defender_observation` write and `mcbs_unpack_defender_observation` /
    `mcbs_encode_defender_features` read.

    With N nodes and S services a row has `width` = F = 6N + N + 6N + S columns: the four MultiBinary fields in sorted key order
    (`DEFENDER_KEYS`, the column order of `DefenderVecEnv.features()`): incoming_firewall_status column 6n + k, infected_nodes 6N + n,
    outgoing_firewall_status 7N + 6n + k, services_status 13N + s.  `fields[key]` = (offset, size) of each.  Column c is bit c & 31 of
    word c >> 5 of `words` = ceil(F / 32) uint32 words; bits at or past F are zero, always.
    Packing rule: a bit is set where the dense element is NOT ZERO (`v != 0`; the observation only ever holds 0 and 1); unpacking gives
    int8 0 / 1.  Pure NumPy."""

    def __init__(self, topo: FlatTopology):
        N, S = int(topo.n_nodes), int(topo.header()["n_services"])
        self.n_nodes, self.n_services = N, S
        sizes = (6 * N, N, 6 * N, S)
        self.fields = {}
        c = 0
        for k, n in zip(DEFENDER_KEYS, sizes):
            self.fields[k] = (c, n)
            c += n
        self.width = c
        self.words = (c + 31) // 32

    def pack_host(self, obs: dict) -> np.ndarray:
        """uint32 [n, words] of a dict of the four fields with a leading row axis (any trailing shape, any integer or bool dtype)."""
        n = len(np.asarray(obs[DEFENDER_KEYS[0]]))
        bits = np.zeros((n, self.words * 32), dtype=np.uint64)
        for k, (off, size) in self.fields.items():
            bits[:, off:off + size] = np.asarray(obs[k]).reshape(n, size) != 0
        shifts = np.arange(32, dtype=np.uint64)
        return (bits.reshape(n, self.words, 32) << shifts).sum(axis=2).astype(np.uint32)       # (distinct bits: adding is OR-ing)

    def unpack_host(self, rows) -> dict:
        """The four int8 fields (0 / 1, [n, size] each) of uint32 / int32 rows [n, >= words]."""
        p = np.asarray(rows)
        p = (p.view(np.uint32) if p.dtype == np.int32 else p.astype(np.uint32))[:, :self.words]
        bits = ((p[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(p.shape[0], self.words * 32).astype(np.int8)
        return {k: bits[:, off:off + size].copy() for k, (off, size) in self.fields.items()}
