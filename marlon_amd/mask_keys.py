"""Host mirror of the action-mask keys (include/mcbs.h "action-mask keys"; the kernels are marlon_amd/csrc/mcbs_mask_keys.hip).

A key row holds what the Discrete action mask of one observation is a function of: the effective discovered-node count and the
cached-credential count (word 0), the owned-source bits by discovery index (ceil(Nk / 32) words) and the node id at every discovery
index (ceil(Nk / 4) words, one byte each), Nk = min(maximum_node_count, the topology's node count).  NumPy only: this module states the
format and the malformed-key rule for tests and tools; the product path is the device's (engine.store_mask_keys / expand_mask_keys).
"""
from __future__ import annotations

import numpy as np


def key_node_bound(topo, spec) -> int:
    """Nk: the discovery indices a key can describe."""
    return min(int(spec.maximum_node_count), int(topo.n_nodes))


def key_words(topo, spec) -> int:
    """Wk = 1 + ceil(Nk / 32) + ceil(Nk / 4)."""
    nk = key_node_bound(topo, spec)
    return 1 + (nk + 31) // 32 + (nk + 3) // 4


def keys_from_state(headers, nodes, order, topo, spec, blank=None) -> np.ndarray:
    """Key rows uint32 [E, Wk] of the observation a state record (`_abi.split_state`: headers [E], nodes [E, N], discovery order [E, N])
    gives.  blank: bool [E], the rows whose observation is the blank one (their effective count is 0); None takes the state's
    out-of-bound flag (`last_oob`), as the observation does."""
    nk, wk = key_node_bound(topo, spec), key_words(topo, spec)
    nb = (nk + 31) // 32
    E = headers.shape[0]
    blank = headers["last_oob"] != 0 if blank is None else np.asarray(blank, dtype=bool)
    count = np.where(blank, 0, np.minimum(headers["n_discovered"].astype(np.int64), nk))
    live = np.arange(nk)[None, :] < count[:, None]                                        # [E, Nk]: index below the effective count
    ids = np.where(live, order[:, :nk].astype(np.int64), 0)
    owned = live & (np.take_along_axis(nodes["installed"], ids, axis=1) != 0)
    keys = np.zeros((E, wk), dtype=np.uint32)
    keys[:, 0] = count.astype(np.uint32) | (headers["n_creds"].astype(np.uint32) << np.uint32(16))
    own_bits = np.zeros((E, 32 * nb), dtype=bool)
    own_bits[:, :nk] = owned
    keys[:, 1:1 + nb] = np.packbits(own_bits, axis=1, bitorder="little").view("<u4")
    id_bytes = np.zeros((E, 4 * (wk - 1 - nb)), dtype=np.uint8)
    id_bytes[:, :nk] = ids
    keys[:, 1 + nb:] = id_bytes.view("<u4")
    return keys


def expand_host(keys, topo, spec) -> np.ndarray:
    """Key rows [n, >= Wk] -> packed masks uint32 [n, W] in mcbs_pack_action_mask's format (connect | local | remote, bit a = bit a & 31
    of word a >> 5, tail bits zero).  Malformed keys follow the device's rule: a count above Nk acts as Nk, owned-source bits at or
    beyond the count are ignored, a node id at or above the topology's node count contributes no local bits, the credential count
    is used as it stands."""
    keys = np.ascontiguousarray(np.asarray(keys)).view(np.uint32)
    nk, wk = key_node_bound(topo, spec), key_words(topo, spec)
    nb = (nk + 31) // 32
    if keys.ndim != 2 or keys.shape[1] < wk:
        raise ValueError(f"keys must be [n, >= {wk}] words")
    n = keys.shape[0]
    N, C = int(spec.maximum_node_count), int(spec.maximum_total_credentials)
    P, L, R = len(topo.ports), len(topo.local_vulnerabilities), len(topo.remote_vulnerabilities)
    count = np.minimum((keys[:, 0] & 0xFFFF).astype(np.int64), nk)
    creds = (keys[:, 0] >> 16).astype(np.int64)
    live = np.arange(nk)[None, :] < count[:, None]                                        # [n, Nk]
    own_k = np.unpackbits(np.ascontiguousarray(keys[:, 1:1 + nb]).view(np.uint8), axis=1, bitorder="little")[:, :nk] != 0
    ids = np.ascontiguousarray(keys[:, 1 + nb:wk]).view(np.uint8)[:, :nk].astype(np.int64)
    table = topo.node_table()["local_mask"].astype(np.uint32)
    lmask = np.where(ids < topo.n_nodes, table[np.minimum(ids, topo.n_nodes - 1)], 0)
    own = np.zeros((n, N), dtype=bool)                                                    # by discovery index, up to the node bound N
    own[:, :nk] = own_k & live
    disc = np.arange(N)[None, :] < count[:, None]
    lm = np.zeros((n, N), dtype=np.uint32)
    lm[:, :nk] = lmask
    pair = own[:, :, None] & disc[:, None, :]                                             # [n, s, t]
    cred_on = np.arange(C)[None, :] < creds[:, None]                                      # [n, c]
    connect = np.broadcast_to(pair[:, :, :, None, None] & cred_on[:, None, None, None, :], (n, N, N, P, C))
    local = own[:, :, None] & (((lm[:, :, None] >> np.arange(L, dtype=np.uint32)[None, None, :]) & 1) != 0)
    remote = np.broadcast_to(pair[:, :, :, None], (n, N, N, R))
    mask = np.concatenate([connect.reshape(n, -1), local.reshape(n, -1), remote.reshape(n, -1)], axis=1)
    A = mask.shape[1]
    W = (A + 31) // 32
    out = np.zeros((n, 4 * W), dtype=np.uint8)
    b = np.packbits(mask, axis=1, bitorder="little")
    out[:, :b.shape[1]] = b
    return out.view("<u4")
