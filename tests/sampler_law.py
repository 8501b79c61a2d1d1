"""The random agent's law, restated in float64 from the reference's procedure, and the statistics the sampler tests share.

`valid_law` is CyberBattleEnv.sample_valid_action (cyberbattle_env.py:959-1047) as a distribution over the Discrete action indices of
MaskedDiscreteAttackerWrapper (`connect | local | remote`, action_masking.py:72-136):

  * kind uniform over {local, remote} while the credential cache is empty, else over {local, remote, connect} (:969-981);
  * source uniform over the external indices of the nodes with privilege >= LocalUser (`__get__owned_nodes_indices`).  The reference
    takes them from every node of the network (actions.py:317-319) and looks each one up in the discovery list, the kernel walks the
    discovery list: the two agree when every such node is discovered, which this helper asserts for each state it is given.  It models
    LIVE privilege levels (what the kernel reads), not the reference's `__owned_nodes_indices_cache`;
  * target uniform over [0, n_discovered), vulnerability / port uniform over their bound, credential uniform over [0, n_creds);
  * the whole action redrawn until the action mask allows it (:1043-1046): law(a) = q(a) * mask(a) / Z, Z = sum of q * mask.

The mask is built here from the state by the reference's rule (`mask_indices`, cyberbattle_env.py:643-677): sources are the DISCOVERED
nodes with the agent installed; such a source may use the local vulnerabilities it has (its own or the library's), any remote
vulnerability and any (port, cached credential) against any discovered node.  tests cross-check it against Oracle.observe.

`uniform_law` is the valid=0 law: kind uniform over 3, every component uniform over its DECLARED bound.

Nothing here is tuned on the code under test: the chi-square bound is the 1 - 1e-9 quantile, bins are merged until each expects at
least MIN_EXPECTED = 50 draws, and a state is only used when the sampler's 64 redraws cannot plausibly run out (`exhaustion_bound`).
"""
from __future__ import annotations

import math
from statistics import NormalDist

import numpy as np

MIN_EXPECTED = 50.0
FALSE_ALARM = 1e-9
REDRAWS = 64


class Geometry:
    """Bounds of the Discrete action space: N = maximum_node_count, C = maximum_total_credentials, L / R / P from the topology."""

    def __init__(self, topo, spec):
        self.N, self.C = int(spec.maximum_node_count), int(spec.maximum_total_credentials)
        self.L, self.R, self.P = len(topo.local_vulnerabilities), len(topo.remote_vulnerabilities), len(topo.ports)
        self.connect_size = self.N * self.N * self.P * self.C
        self.local_size = self.N * self.L
        self.remote_size = self.N * self.N * self.R
        self.total = self.connect_size + self.local_size + self.remote_size

    def encode(self, rows):
        """Engine rows [.., 5] (kind 0 local / 1 remote / 2 connect) -> Discrete indices, int64 (numpy or torch)."""
        k, a, b, c, d = (rows[..., i] for i in range(5))
        if not isinstance(rows, np.ndarray):                     # torch
            k, a, b, c, d = (x.long() for x in (k, a, b, c, d))
            where = __import__("torch").where
        else:
            k, a, b, c, d = (x.astype(np.int64) for x in (k, a, b, c, d))
            where = np.where
        con = ((a * self.N + b) * self.P + c) * self.C + d
        loc = self.connect_size + a * self.L + b
        rem = self.connect_size + self.local_size + (a * self.N + b) * self.R + c
        return where(k == 2, con, where(k == 0, loc, rem))

    def decode(self, idx: int):
        """MaskedDiscreteAttackerWrapper._decode (action_masking.py:107-136) with Python integers -> engine row (kind, a, b, c, d)."""
        a = int(idx)
        if a < 0 or a >= self.total:
            raise ValueError(f"Invalid discrete action: {a}")
        if a < self.connect_size:
            cred = a % self.C
            a //= self.C
            port = a % self.P
            a //= self.P
            return (2, a // self.N, a % self.N, port, cred)
        if a < self.connect_size + self.local_size:
            a -= self.connect_size
            return (0, a // self.L, a % self.L, 0, 0)
        a -= self.connect_size + self.local_size
        vuln = a % self.R
        a //= self.R
        return (1, a // self.N, a % self.N, vuln, 0)


def env_state(state, e: int = 0) -> dict:
    """One env of a get_state() record (Oracle or BatchEngine) as plain lists."""
    hdr, nodes, order, _ = state
    nd = int(hdr["n_discovered"][e])
    return dict(n_discovered=nd, n_creds=int(hdr["n_creds"][e]), order=[int(x) for x in order[e][:nd]],
                installed=[int(x) for x in nodes["installed"][e]], privilege=[int(x) for x in nodes["privilege"][e]])


def _grid(*sizes):
    return [g.reshape(-1) for g in np.meshgrid(*[np.arange(s, dtype=np.int64) for s in sizes], indexing="ij")]


def _rows_for(geo: Geometry, st: dict, sources, kinds):
    """Rows (kind, src, ., ., .) x every in-range completion, for the given external source indices."""
    nd, nc = st["n_discovered"], st["n_creds"]
    out = []
    src = np.asarray(sources, np.int64)
    for kind in kinds:
        if kind == 0:
            s, v = _grid(len(src), geo.L)
            out.append(np.stack([np.zeros_like(s), src[s], v, np.zeros_like(s), np.zeros_like(s)], 1))
        elif kind == 1:
            s, t, v = _grid(len(src), nd, geo.R)
            out.append(np.stack([np.ones_like(s), src[s], t, v, np.zeros_like(s)], 1))
        else:
            s, t, p, c = _grid(len(src), nd, geo.P, nc)
            out.append(np.stack([np.full_like(s, 2), src[s], t, p, c], 1))
    return np.concatenate(out) if out else np.zeros((0, 5), np.int64)


def mask_indices(topo, geo: Geometry, st: dict) -> np.ndarray:
    """Sorted Discrete indices the reference's action mask allows in this state (cyberbattle_env.py:643-677)."""
    lmask = topo.node_table()["local_mask"]
    sources = [i for i, n in enumerate(st["order"]) if st["installed"][n]]
    rows = _rows_for(geo, st, sources, (0, 1, 2))
    keep = np.ones(len(rows), bool)
    loc = rows[:, 0] == 0
    node = np.asarray(st["order"], np.int64)[rows[loc, 1]]
    keep[loc] = (lmask[node].astype(np.int64) >> rows[loc, 2]) & 1 == 1
    return np.sort(geo.encode(rows[keep]))


def valid_law(topo, geo: Geometry, st: dict) -> dict:
    """The law of sample_valid_action in this state: dict(idx sorted int64 [S], p float64 [S] summing to 1, rows [S,5], Z)."""
    assert geo.L > 0 and geo.R > 0 and geo.P > 0
    nd, nc = st["n_discovered"], st["n_creds"]
    by_priv = {n for n, p in enumerate(st["privilege"]) if p >= 1}
    assert by_priv <= set(st["order"]), "a node with privilege >= LocalUser is not discovered: reference and kernel enumerate differently"
    owned = [i for i, n in enumerate(st["order"]) if st["privilege"][n] >= 1]
    assert owned, "no owned node: sample_valid_action has nothing to choose from"
    kinds = (0, 1, 2) if nc else (0, 1)
    rows = _rows_for(geo, st, owned, kinds)
    per_kind = {0: 1.0 / geo.L, 1: 1.0 / (nd * geo.R), 2: 1.0 / (nd * geo.P * nc) if nc else 0.0}
    q = np.asarray([per_kind[k] for k in (0, 1, 2)], np.float64)[rows[:, 0]] / (len(kinds) * len(owned))
    assert abs(q.sum() - 1.0) < 1e-12
    idx = geo.encode(rows)
    allowed = np.isin(idx, mask_indices(topo, geo, st))
    Z = float(q[allowed].sum())
    o = np.argsort(idx[allowed])
    return dict(idx=idx[allowed][o], p=q[allowed][o] / Z, rows=rows[allowed][o], Z=Z)


def uniform_law(geo: Geometry) -> np.ndarray:
    """valid=0: kind uniform over 3, every component uniform over its declared bound; probability of each of the geo.total indices."""
    p = np.empty(geo.total, np.float64)
    p[:geo.connect_size] = 1.0 / (3.0 * geo.connect_size)
    p[geo.connect_size:geo.connect_size + geo.local_size] = 1.0 / (3.0 * geo.local_size)
    p[geo.connect_size + geo.local_size:] = 1.0 / (3.0 * geo.remote_size)
    return p


def exhaustion_bound(Z: float, draws: int) -> float:
    """Expected number of draws whose 64 redraws are all refused: draws * (1 - Z)^64."""
    return draws * (1.0 - Z) ** REDRAWS


def chi2_quantile(df: int, tail: float = FALSE_ALARM) -> float:
    """The 1 - tail quantile of chi-square(df): scipy when present, else Wilson-Hilferty (df = 278: 443.5 and 443.9)."""
    try:
        from scipy.stats import chi2
        return float(chi2.isf(tail, df))
    except ImportError:
        z = -NormalDist().inv_cdf(tail)
        return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3


def merge_bins(expected: np.ndarray, observed: np.ndarray, min_expected: float = MIN_EXPECTED):
    """Merge neighbouring bins, in index order, until each expects at least min_expected; the tail joins the last group."""
    e_out, o_out, e_acc, o_acc = [], [], 0.0, 0
    for e, o in zip(expected.tolist(), observed.tolist()):
        e_acc += e
        o_acc += o
        if e_acc >= min_expected:
            e_out.append(e_acc)
            o_out.append(o_acc)
            e_acc, o_acc = 0.0, 0
    if e_acc > 0.0 or o_acc:
        assert e_out, "fewer than min_expected draws expected over the whole support"
        e_out[-1] += e_acc
        o_out[-1] += o_acc
    return np.asarray(e_out, np.float64), np.asarray(o_out, np.float64)


def pearson(p: np.ndarray, counts: np.ndarray):
    """(chi-square, degrees of freedom, bound) of observed counts against the law p over the same bins (counts.sum() draws)."""
    n = float(counts.sum())
    e, o = merge_bins(p * n, counts)
    assert e.min() >= MIN_EXPECTED and len(e) >= 2
    stat = float(((o - e) ** 2 / e).sum())
    return stat, len(e) - 1, chi2_quantile(len(e) - 1)


def independence(p: np.ndarray, first: np.ndarray, second: np.ndarray):
    """Contingency chi-square of pairs (first[i], second[i]) of bin numbers against the product law p x p: (stat, df, bound).
    Bins are merged on the marginal first so that every CELL expects at least MIN_EXPECTED pairs."""
    n = len(first)
    need = math.sqrt(MIN_EXPECTED / n)                       # marginal weight g with g * g * n >= MIN_EXPECTED
    group = np.zeros(len(p), np.int64)
    weights, acc, g = [], 0.0, 0
    for i, pi in enumerate(p.tolist()):
        group[i] = g
        acc += pi
        if acc >= need:
            weights.append(acc)
            acc, g = 0.0, g + 1
    if acc > 0.0:
        assert weights
        group[group == g] = g - 1
        weights[-1] += acc
    w = np.asarray(weights, np.float64)
    G = len(w)
    assert G >= 2
    e = np.outer(w, w) * n
    assert e.min() >= MIN_EXPECTED * (1 - 1e-12)
    o = np.bincount(group[first] * G + group[second], minlength=G * G).reshape(G, G).astype(np.float64)
    return float(((o - e) ** 2 / e).sum()), G * G - 1, chi2_quantile(G * G - 1)


def agreement_bound(p_equal: float, n: int, tail: float = FALSE_ALARM) -> int:
    """Smallest m with P(Binomial(n, p_equal) > m) <= tail: how many of n independent pairs may agree."""
    try:
        from scipy.stats import binom
        return int(binom.isf(tail, n, p_equal))
    except ImportError:                                      # Bernstein: P(X - np >= t) <= exp(-t^2 / (2 (np(1-p) + t/3)))
        v, lg = n * p_equal * (1 - p_equal), math.log(1.0 / tail)
        t = lg / 3.0 + math.sqrt(lg * lg / 9.0 + 2.0 * v * lg)
        return int(math.ceil(n * p_equal + t))
