"""Scripted episodes that END, written with the CPU oracle: the inputs of tests/test_endings_script.py (do they reach what they
claim?) and tests/test_gpu_episode_endings.py (does every step-kernel layout end them as the oracle does?).

`case(name)` (name = "<topology>-<spec>", cached per process) returns a Case: the flattened topology, the EnvSpec, an action script
[T, E, 5] int32 and the oracle's outputs of every step.  The script is written by a host policy that reads the ORACLE's state
(get_state and the topology's local masks and credential triples), never the device sampler, so the CPU test proves reachability
without a GPU and every entry point replays the same rows.  About 10 % of the rows are uniform over the declared bounds and about 2 %
carry a node index past the discovered nodes (the out-of-bound path: it never ends by goal, it can truncate).

Next to the oracle that records the outputs runs a SHADOW oracle with auto_reset off, reset by hand (Oracle.reset(i) begins the next
episode exactly as the auto-reset does: same episode index, same Philox keys).  Its state after an ending step is the terminal state,
not the reset image, so the owned count, the availability and the cumulative reward the goals compared can be read back: `derive()`
restates the goals (cyberbattle_env.py:1080-1116, 1162-1169) from them, the second opinion the classifier `reason()` is checked with.

The hidden counter `owned` of the kernels is followed the same way.  Within one step the attacker acts before the defender, so per
step  ups = nodes newly owned,  downs = nodes re-imaged,  peak = owned before + ups.  A node that was running and not owned before the
step and is being re-imaged after it was owned in between (ScanAndReimage only re-images infected nodes): it counts in both.

Parameters chosen from a pilot run are chosen from the ORACLE alone.  The truncation bound of `mixed` (a step count at which a first
episode wins) and the reward goal R (a cumulative reward some env holds exactly on the step before it wins) come from the pilot's
first episodes, which do not depend on the parameter, so what the pilot shows happens again in the case.  k of `percent` (an owned
count enough envs exceed) needs no such exactness and is taken over the whole pilot.

The weighted cases (WEIGHT_SPECS, further down) use the same machinery on topologies with unequal SLA weights, for
tests/test_gpu_availability_weights.py: there the availability itself, the project's only floating point, is what is under test.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

E = 203                    # not a multiple of 64, 32 or 16: the last wavefront and the last G-lane group are partial
T_MAX = 160                # most steps of a script
WIN, LOSE = 4321.5, -77.25  # exact in fp32, distinct from any raw reward and from 0
SCAN = ("scan_and_reimage", 0.5, 2, 3)
SCAN_AVAIL = ("scan_and_reimage", 0.9, 3, 2)
REASONS = ("goal", "sla", "evicted", "truncated")
TOPOLOGIES = ("toyctf", "random24", "random100", "random129", "ad6")
SPECS = ("mixed", "updown", "frozen", "reward", "reward_def", "sla", "lowavail", "sla_evict", "pct_eq", "pct_below", "pct_above")
# the reasons each spec is meant to produce (at least 8 envs each, tests/test_endings_script.py)
MEANT = {"mixed": ("goal", "evicted", "truncated"), "updown": ("goal", "evicted", "truncated"), "frozen": ("goal", "truncated"), "reward": ("goal",),
         "reward_def": ("goal",), "sla": ("sla",), "lowavail": ("goal",), "sla_evict": ("sla",), "pct_eq": ("goal",),
         "pct_below": ("goal",), "pct_above": ("goal",)}
RANDOM_NET_SEED = {24: 5, 100: 7, 129: 7}      # (24, seed 7) leaves the attacker on one node


# SLA weights by node (and by service) index, cycled.  dyadic: unequal, and every sum of them exact in fp64 in any order.
# odd: the non-dyadic weights of tests/test_gpu_defender_layouts.py::_weighted_topology (sums depend on the order).
WEIGHT_KINDS = ("dyadic", "odd")
NODE_WEIGHTS = {"dyadic": (1.0, 2.0, 0.5, 4.0, 0.25, 1.5, 3.0, 0.75, 8.0), "odd": (0.1, 0.3, 0.7, 1.9, 2.3, 0.6, 1.1, 3.3, 0.35)}
SERVICE_WEIGHTS = (0.3, 0.6, 1.7, 0.9, 0.1, 2.2, 1.3)


@functools.lru_cache(maxsize=None)
def topology(name: str, weights: str = "uniform"):
    """The flattened topology with every node re-imagable (the defender can evict the attacker).  weights: "uniform" (the samples' own SLA
    weights), "dyadic" or "odd" (NODE_WEIGHTS cycled over the nodes; odd: SERVICE_WEIGHTS cycled over the services too; dyadic: a
    stopped service weighs 1 + the node's running services, which makes the node's share (1 + running) / (1 + total) exactly 1/2)."""
    from marlon_amd import flatten as F, model
    from marlon_amd.samples import active_directory, kitchen_sink, random_net, toy_ctf
    if name == "toyctf":
        env = toy_ctf.new_environment()
    elif name == "sink":
        env = kitchen_sink.new_environment()
    elif name == "ad6":
        env = active_directory.new_random_environment(6)
    else:
        n = int(name[6:])
        env = random_net.build(model, n, RANDOM_NET_SEED[n])
    for _, info in env.nodes():
        info.reimagable = True
    return F.flatten(reweigh(env, weights))


def reweigh(env, weights: str):
    """Set the SLA weights of a model environment in place (see topology); returns it."""
    k = 0
    for i, (_, info) in enumerate(env.nodes()):
        if weights == "uniform":
            break
        info.sla_weight = NODE_WEIGHTS[weights][i % len(NODE_WEIGHTS[weights])]
        running = sum(1.0 for s in info.services if s.running)
        for s in info.services:
            s.sla_weight = SERVICE_WEIGHTS[k % len(SERVICE_WEIGHTS)] if weights == "odd" else (1.0 if s.running else 1.0 + running)
            k += 1
    return env


def make_spec(topo, **over):
    from marlon_amd._abi import RNG_PHILOX, EnvSpec
    kw = dict(n_envs=E, maximum_node_count=topo.n_nodes, maximum_total_credentials=max(1, len(topo.triples)),
              maximum_discoverable_credentials_per_action=max(8, int(topo.header()["max_leak_per_action"])),
              winning_reward=WIN, losing_reward=LOSE, auto_reset=True, max_episode_steps=60, rng_kind=RNG_PHILOX, seed=4242,
              env_id_base=500)
    kw.update(over)
    return EnvSpec(**kw)


def owned_count(state) -> np.ndarray:
    """get_nodes_with_atleast_privilegelevel(LocalUser) per env, from the privileges of a get_state() record."""
    return (state[1]["privilege"] >= 1).sum(axis=1).astype(np.int64)


class Policy:
    """Rows [E, 5] from the oracle's state.  Source: a random node with the agent installed.  Then a connect with a random cached
    credential to that credential's own node and port, a local exploit the source's static local mask has, or a remote exploit on a
    random discovered node (one not owned, if there is one).  Two candidates are drawn per env and the second is taken when the first
    was already played in this episode.  Every call draws arrays of the same shapes, so an env's rows depend on its own state and draws
    only.  stall: the share of envs that open an episode with an out-of-bound row (the defender then scans on the first played step)."""
    SLOTS = 2048

    def __init__(self, topo, spec, seed: int, stall: float = 0.0):
        from marlon_amd import flatten as F
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.N, self.Nmax, self.Cmax = topo.n_nodes, int(spec.maximum_node_count), int(spec.maximum_total_credentials)
        self.L, self.R, self.P = len(topo.local_vulnerabilities), len(topo.remote_vulnerabilities), len(topo.ports)
        self.local_mask = topo.node_table()["local_mask"].astype(np.int64)
        tr = topo.section("triple", F.TRIPLE_DT, len(topo.triples)) if len(topo.triples) else np.zeros(1, F.TRIPLE_DT)
        self.tr_node, self.tr_port = tr["node"].astype(np.int64), tr["port"].astype(np.int64)
        self.tried = np.zeros((spec.n_envs, self.SLOTS), bool)
        self.stall = stall

    def _candidate(self, nd, nc, disc, onode, inst, priv, cache):
        rng, n_envs, N = self.rng, onode.shape[0], self.N
        ar = np.arange(n_envs)
        src = np.argmax(np.where(inst, rng.random((n_envs, N)), -1.0), axis=1)   # external index of a random installed node (0 if none)
        bits = ((self.local_mask[onode[ar, src]][:, None] >> np.arange(max(1, self.L))[None, :]) & 1) != 0
        lv = np.argmax(np.where(bits, rng.random(bits.shape), -1.0), axis=1)
        score = np.where(disc, rng.random((n_envs, N)) + (priv == 0), -1.0)       # a discovered node, one not owned first
        tgt = np.argmax(score, axis=1)
        rv = rng.integers(0, max(1, self.R), n_envs)
        ci = np.minimum((rng.random(n_envs) * nc).astype(np.int64), np.maximum(nc - 1, 0))
        trip = np.minimum(cache[ar, ci].astype(np.int64), len(self.tr_node) - 1)
        hit = (onode == self.tr_node[trip][:, None]) & disc
        ctgt = np.argmax(hit, axis=1)
        fresh = hit.any(axis=1) & (nc > 0) & (priv[ar, ctgt] == 0)              # the credential opens a node not owned yet
        u = rng.random(n_envs)
        connect = (nc > 0) & ((fresh & (u < 0.3)) | (u < 0.1))
        local = ~connect & bits.any(axis=1) & (u < 0.85)
        out = np.zeros((n_envs, 5), np.int32)
        out[:, 0] = np.where(connect, 2, np.where(local, 0, 1))
        out[:, 1] = src
        out[:, 2] = np.where(connect, ctgt, np.where(local, lv, tgt))
        out[:, 3] = np.where(connect, self.tr_port[trip], np.where(local, 0, rv))
        out[:, 4] = np.where(connect, ci, 0)
        return out

    def rows(self, state) -> np.ndarray:
        hdr, nodes, order, cache = state
        rng, n_envs, N = self.rng, order.shape[0], self.N
        ar = np.arange(n_envs)
        nd = hdr["n_discovered"].astype(np.int64)
        nc = np.minimum(hdr["n_creds"].astype(np.int64), self.Cmax)
        disc = np.arange(N)[None, :] < nd[:, None]
        onode = np.where(disc, order, 0).astype(np.int64)                       # [E, N] node at each external index
        inst = (np.take_along_axis(nodes["installed"], onode, 1) != 0) & disc
        priv = np.where(disc, np.take_along_axis(nodes["privilege"], onode, 1), 0)
        opening = hdr["step_count"] == 0
        self.tried[opening] = False
        first, second = (self._candidate(nd, nc, disc, onode, inst, priv, cache) for _ in range(2))
        slot = lambda r: (r.astype(np.int64) * np.array([7919, 104729, 1299709, 15485863, 32452843])).sum(axis=1) % self.SLOTS
        out = np.where(self.tried[ar, slot(first)][:, None], second, first)
        self.tried[ar, slot(out)] = True
        # ~10 % uniform over the declared bounds, ~2 % with a node index past the discovered nodes
        uni = np.stack([rng.integers(0, 3, n_envs), rng.integers(0, self.Nmax, n_envs), rng.integers(0, self.Nmax, n_envs),
                        rng.integers(0, max(self.L, self.R, self.P, 1), n_envs), rng.integers(0, self.Cmax, n_envs)], axis=1).astype(np.int32)
        pick = rng.random(n_envs)
        out = np.where((pick < 0.10)[:, None], uni, out)
        far = ((pick >= 0.10) & (pick < 0.12)) | (opening & (rng.random(n_envs) < self.stall))
        out[far, 0] = np.where(out[far, 0] == 2, 1, out[far, 0])                  # (a connect checks its credential first)
        out[far, 1] = np.where(rng.random(n_envs) < 0.5, nd, self.Nmax + 3)[far]
        return out


OUT_KEYS = ("reward", "raw_reward", "terminated", "truncated", "oob", "step_count", "availability")


@dataclass
class Case:
    name: str
    topo: object
    spec: object
    actions: np.ndarray                      # [T, E, 5] int32
    out: dict                                # OUT_KEYS -> [T, E], the oracle's outputs
    live: np.ndarray                         # [T, E] bool: the env was stepped (False: ended and frozen, auto_reset off)
    reset_at: int                            # frozen: before this step the ended envs are reset by hand (-1: never)
    reset_mask: np.ndarray                   # [E] uint8
    shadow_equal: bool                       # the shadow oracle returned the same outputs and, where compared, the same state
    owned_after: np.ndarray                  # [T, E] owned nodes after the step, before any reset
    cum_before: np.ndarray                   # [T, E] cumulative reward before the step
    peak: np.ndarray                         # [T, E] owned before + nodes newly owned (the counter's highest value in the step)
    ups: np.ndarray                          # [T, E] nodes newly owned in the step
    downs: np.ndarray                        # [T, E] nodes re-imaged in the step
    had_two: np.ndarray                      # [T, E] the counter reached 2 or more at an EARLIER step of this episode
    up_down_up: np.ndarray                   # [T, E] by this step the episode saw: counter >= 2, then a re-image, then (a later step) a node owned
    params: dict = field(default_factory=dict)
    imaging: np.ndarray = None               # [T, E, N] bool, weighted cases only: the node is being re-imaged at the step's defender tick

    @property
    def ended(self) -> np.ndarray:
        return self.live & ((self.out["terminated"] != 0) | (self.out["truncated"] != 0))

    def reasons(self) -> np.ndarray:
        """[T, E] of '' or a reason, from the classifier."""
        r = np.stack([reason({k: v[t] for k, v in self.out.items()}, self.spec) for t in range(self.actions.shape[0])])
        return np.where(self.live, r, "")

    def envs_by_reason(self) -> dict:
        """reason -> (number of distinct envs it ended at least once, number of endings)."""
        r = self.reasons()
        return {k: (int((r == k).any(axis=0).sum()), int((r == k).sum())) for k in REASONS}


def has_defender(spec) -> bool:
    return spec.defender is not None and spec.defender[0] in ("scan_and_reimage", "random_events")


def reason(out: dict, spec) -> np.ndarray:
    """Per env, why the step ended the episode ('' if it did not), from one step's outputs alone."""
    term, trunc = out["terminated"] != 0, out["truncated"] != 0
    lost = term & (out["reward"] == spec.losing_reward)
    sla = term & (out["reward"] == spec.winning_reward) & has_defender(spec) & (out["availability"] < spec.maintain_sla)
    return np.where(trunc, "truncated", np.where(lost, "evicted", np.where(sla, "sla", np.where(term, "goal", ""))))


def derive(case: Case) -> np.ndarray:
    """[T, E] reasons from the shadow oracle's terminal state: the goals restated (env.py:1080-1116, 1162-1169)."""
    s, g = case.spec, case.spec.attacker_goal
    N = case.topo.n_nodes
    d = has_defender(s)
    av, owned = case.out["availability"], case.owned_after
    goal = np.zeros(av.shape, bool)
    if g is not None:
        goal = ~(case.cum_before < float(g.get("reward", 0.0))) & ~(owned < int(g.get("own_atleast", 0))) & \
               ~(owned.astype(np.float64) / float(N) < float(g.get("own_atleast_percent", 1.0)))
        if d:
            goal &= ~(av >= float(g.get("low_availability", 1.0)))
    broken = (av < s.maintain_sla) if d else np.zeros(av.shape, bool)
    evicted = (owned == 0) if s.defender_goal_eviction else np.zeros(av.shape, bool)
    play = case.out["oob"] == 0
    done = play & (goal | broken | evicted)
    trunc = ~done & (s.max_episode_steps > 0) & (case.out["step_count"] >= s.max_episode_steps)
    r = np.where(play & broken, "sla", np.where(play & goal, "goal", np.where(done, "evicted", np.where(trunc, "truncated", ""))))
    return np.where(case.live, r, "")


def _same_state(a, b) -> bool:
    """Two get_state() records, field by field (padding aside)."""
    for x, y in zip(a, b):
        if x.dtype.names:
            if not all(np.array_equal(x[f], y[f]) for f in x.dtype.names if not f.startswith("pad")):
                return False
        elif not np.array_equal(x, y):
            return False
    return True


def run(name: str, topo, spec, n_steps: int, reset_at: int = -1, policy_seed: int = 11, stall: float = 0.0, params=None,
        record_imaging: bool = False) -> Case:
    """Write the script with the oracle and record it.  record_imaging: keep, per step, the nodes not running before the step and still
    not running after it.  The availability a step reports is taken at its tick, after the nodes whose re-imaging is over came back and
    before the step's scan re-images others: those nodes are the ones missing from the sum."""
    import dataclasses
    from oracle.oracle import Oracle
    orc = Oracle(topo, spec)
    shadow = Oracle(topo, dataclasses.replace(spec, auto_reset=False))
    pol = Policy(topo, spec, policy_seed, stall)
    n_envs = spec.n_envs
    acts = np.zeros((n_steps, n_envs, 5), np.int32)
    out = {k: [] for k in OUT_KEYS}
    rec = {k: [] for k in ("live", "owned_after", "cum_before", "peak", "ups", "downs", "had_two", "up_down_up")}
    over = np.zeros(n_envs, bool)
    reset_mask = np.zeros(n_envs, np.uint8)
    two, down, again = (np.zeros(n_envs, bool) for _ in range(3))
    imaging = []
    same = True
    before = shadow.get_state()
    fresh = [x.copy() for x in before]
    for t in range(n_steps):
        if t == reset_at:
            reset_mask = over.astype(np.uint8)
            for i in np.flatnonzero(over):
                orc.reset(int(i))
                shadow.reset(int(i))
            two[over] = down[over] = again[over] = False
            over[:] = False
            before = shadow.get_state()
        if t % 20 == 0 or t == reset_at:
            same &= _same_state(orc.get_state(), before)           # the policy reads the recording oracle's state
        a = pol.rows(before)
        acts[t] = a
        o = orc.step(a)
        o2 = shadow.step(a)
        after = shadow.get_state()
        same &= all(np.array_equal(o[k].view(np.uint8), o2[k].view(np.uint8)) for k in OUT_KEYS)
        for k in OUT_KEYS:
            out[k].append(o[k])
        lv = ~over
        if record_imaging:
            imaging.append((before[1]["running"][:, :topo.n_nodes] == 0) & (after[1]["running"][:, :topo.n_nodes] == 0))
        pb, pa = before[1]["privilege"] >= 1, after[1]["privilege"] >= 1
        between = ~pb & ~pa & (before[1]["running"] != 0) & (after[1]["running"] == 0)     # owned and re-imaged within the step
        up = np.where(lv, (~pb & pa).sum(axis=1) + between.sum(axis=1), 0)
        dn = np.where(lv, (pb & ~pa).sum(axis=1) + between.sum(axis=1), 0)
        pk = owned_count(before) + up
        rec["had_two"].append(two.copy())
        again |= down & (up > 0)                                    # `down` holds re-images of EARLIER steps here
        rec["up_down_up"].append(again.copy())
        two |= lv & (pk >= 2)
        down |= two & (dn > 0)
        for k, v in (("live", lv), ("owned_after", owned_count(after)), ("cum_before", before[0]["cum_reward"].copy()), ("peak", pk),
                     ("ups", up), ("downs", dn)):
            rec[k].append(v)
        end = lv & ((o["terminated"] != 0) | (o["truncated"] != 0))
        after_episode = after[0]["episode"].copy()
        if spec.auto_reset:
            for i in np.flatnonzero(end):
                shadow.reset(int(i))
            two[end] = down[end] = again[end] = False
            before = after
            for x, x0 in zip(before, fresh):                     # a reset env is the initial record again, one episode later
                x[end] = x0[end]
            before[0]["episode"][end] = after_episode[end] + 1
        else:
            over |= end
            before = after
    same &= _same_state(orc.get_state(), before)
    return Case(name, topo, spec, acts, {k: np.stack(v) for k, v in out.items()}, reset_at=reset_at, reset_mask=reset_mask,
                shadow_equal=bool(same), params=dict(params or {}), imaging=np.stack(imaging) if record_imaging else None,
                **{k: np.stack(v) for k, v in rec.items()})


def first_episode(c: Case) -> np.ndarray:
    """[T, E] bool: the step belongs to the env's first episode."""
    e = c.ended
    return np.cumsum(e, axis=0) - e == 0


MIXED_GOAL = dict(own_atleast=2, own_atleast_percent=0.0, low_availability=2.0)
PILOT_STEPS = 64


def updown_settings(topo_name: str, N: int) -> tuple:
    """(defender, max_episode_steps) of `updown`: ScanAndReimage(0.5, max(2, N // 8), 3) and 25 steps.  With 2 draws per scan a re-image
    of one of two owned nodes among 100 happens about once in 150 steps; the capacity grows with the topology so that it stays about
    once in 25.  On ToyCtf the third node is a long chain of exploits away: detection probability 0.1 and 150 steps, or nobody wins."""
    p, steps = (0.1, 150) if topo_name == "toyctf" else (0.5, 25)
    return ("scan_and_reimage", p, max(2, N // 8), 3), steps


@functools.lru_cache(maxsize=None)
def pilot(topo_name: str, kind: str) -> Case:
    """A run whose first episodes do not depend on the parameter being chosen (the goal or the bound is out of reach in it)."""
    topo = topology(topo_name)
    if kind == "mixed":          # no truncation bound
        spec = make_spec(topo, attacker_goal=dict(MIXED_GOAL), defender=SCAN, maintain_sla=0.0, max_episode_steps=0)
    elif kind == "reward":       # reward goal out of reach, no defender
        spec = make_spec(topo, attacker_goal=dict(reward=1e300, own_atleast_percent=0.0), defender=None)
    elif kind == "reward_def":
        spec = make_spec(topo, attacker_goal=dict(reward=1e300, own_atleast_percent=0.0), defender=SCAN)
    else:                        # percent: share out of reach
        spec = make_spec(topo, attacker_goal=dict(own_atleast_percent=2.0, low_availability=2.0), defender=SCAN)
    return run(f"{topo_name}-pilot-{kind}", topo, spec, PILOT_STEPS)


def _mixed_bound(topo_name: str) -> int:
    """The step count in [4, 60] at which most first episodes of the pilot win: `done` and the truncation bound then coincide."""
    p = pilot(topo_name, "mixed")
    win = first_episode(p) & (p.reasons() == "goal")
    steps = p.out["step_count"][win]
    counts = np.bincount(steps[(steps >= 4) & (steps <= 60)], minlength=61)
    assert counts.max() > 0, f"{topo_name}: no first episode wins between step 4 and 60"
    return int(np.argmax(counts))


def _reward_goal(topo_name: str, kind: str) -> float:
    """R in [20, 200] held exactly, on the step before the first crossing, by the most envs of the pilot's first episodes."""
    p = pilot(topo_name, kind)
    first = first_episode(p)
    best, best_n = None, -1
    for v in np.unique(p.cum_before[first]):
        if not 20.0 <= v <= 200.0:
            continue
        crossed = first & (p.cum_before >= v) & (p.out["oob"] == 0)
        t0 = np.argmax(crossed, axis=0)
        cols = np.flatnonzero(crossed.any(axis=0))
        n = int((p.cum_before[t0[cols], cols] == v).sum())
        if n > best_n:
            best, best_n = float(v), n
    assert best is not None, f"{topo_name}: no cumulative reward between 20 and 200"
    return best


def _percent_k(topo_name: str) -> int:
    """The largest k such that at least 24 envs of the pilot own k + 1 nodes at the end of some step."""
    p = pilot(topo_name, "percent")
    most = np.where(p.live, p.owned_after, 0).max(axis=0)
    ks = [k for k in range(1, p.topo.n_nodes) if int((most >= k + 1).sum()) >= 24]
    assert ks, f"{topo_name}: fewer than 24 envs own 2 nodes"
    return ks[-1]


def percent_values(k: int, N: int) -> dict:
    """own_atleast_percent and the owned count it needs: k/N and the double below it need k, the double above it k + 1."""
    x = k / N
    return {"pct_eq": (x, k), "pct_below": (float(np.nextafter(x, 0.0)), k), "pct_above": (float(np.nextafter(x, 1.0)), k + 1)}


def needed_owned(pct: float, N: int) -> int:
    """Smallest owned count j that the reference's `owned / N < percent` (two doubles) lets through: the correctly rounded double of the
    rational j / N, taken from fractions.Fraction and not from a floating-point division, is not below pct."""
    return next(j for j in range(N + 2) if float(Fraction(j, N)) >= pct)


def near_one(N: int) -> float:
    """A threshold just below 1: availability moves by about 1/N per re-imaged node, so one stopped node already crosses it."""
    return 1.0 - 0.05 / N


# steps per spec: the long ones need room for evictions (rare at 100 nodes) and, frozen, for a second part after the reset by hand
STEPS = {"mixed": 160, "updown": 160, "frozen": 160, "reward": 80, "reward_def": 120, "sla": 80, "lowavail": 80, "sla_evict": 80,
         "pct_eq": 100, "pct_below": 100, "pct_above": 100}
assert max(STEPS.values()) <= T_MAX


# ---- availability sums under non-uniform SLA weights (tests/test_gpu_availability_weights.py) ----
# "<topology>-<spec>_<weight kind>": every node re-imagable, ScanAndReimage as in SCAN_AVAIL, eviction ends nothing (a re-imaged entry
# node would end the episode before a second node is missing from the sum), a goal out of reach, truncation (weighted_settings).
#   avail    maintain_sla = 0: no ending depends on the availability; the episodes truncate and restart inside the script
#   sla_eq   maintain_sla = an availability v that first episodes of `avail` attain below full.  The goal is `availability < maintain_sla`:
#            equality does not end the episode
#   sla_up   maintain_sla = the next double above v: the same steps do end
# v comes from the oracle alone: `avail` is the pilot, its first episodes are those of sla_eq and sla_up up to the step that ends them
# (the threshold is read by nothing before that), so an env that meets v on its first played step at or below v, in the pilot, ends
# there under sla_up and plays on under sla_eq.  Only steps count whose sum a kernel on another branch gets wrong (`discriminating`).
WEIGHT_SPECS = tuple(f"{s}_{k}" for k in WEIGHT_KINDS for s in ("avail", "sla_eq", "sla_up"))
WEIGHT_TOPOLOGIES = ("sink", "random24", "random100", "random129", "ad6")   # the packed cell: see weighted_settings
WEIGHT_STEPS = 120
WEIGHT_EPISODE = 40
WEIGHT_GOAL = dict(own_atleast_percent=2.0, low_availability=2.0)


def weighted_settings(topo_name: str) -> dict:
    """ToyCtf's attacker rarely holds a second node (a long chain of exploits away), so hardly more than the entry node is ever missing
    from the sum (3 different sets in 120 steps): the packed cell plays the kitchen-sink topology instead (6 nodes, a stopped service,
    packed like ToyCtf) under a defender that detects less often, so that the attacker gets to hold several nodes before it loses them.
    Beyond 64 nodes 3 draws every 2nd step seldom hit two owned nodes in different 64-bit words while both are down (39 steps among
    100 nodes): there the defender scans on every step and the episodes last 60 steps."""
    if topo_name == "sink":
        defender, bound = ("scan_and_reimage", 0.3, 2, 2), WEIGHT_EPISODE
    elif topology(topo_name).n_nodes > 64:
        defender, bound = ("scan_and_reimage", 0.9, 3, 1), 60
    else:
        defender, bound = SCAN_AVAIL, WEIGHT_EPISODE
    return dict(attacker_goal=dict(WEIGHT_GOAL), defender=defender, defender_goal_eviction=False, max_episode_steps=bound)


def availability_sums(c: Case) -> dict:
    """sums_of(c.topo, c.imaging): [T, E] restatements of a weighted case's availability."""
    return sums_of(c.topo, c.imaging)


def sums_of(topo, im: np.ndarray) -> dict:
    """fp64 restatements of the availability from the avail_term column of the flattened topology and im [..., N] bool, the nodes being
    re-imaged:
    order    the sum over the running nodes in node order, divided by total_sla_weight (on_attacker_step_taken, actions.py:728-745)
    sub_seq  full_sum minus the terms of the nodes being re-imaged, one by one in node order, divided likewise
    sub_sum  full_sum minus (the sum of those terms in node order), divided likewise
    uniform  full_sum minus (their number times the first node's term), divided likewise
    and n, the number of nodes being re-imaged."""
    h = topo.header()
    term = topo.node_table()["avail_term"].astype(np.float64)
    full, total = float(h["full_sum"]), float(h["total_sla_weight"])
    order = np.zeros(im.shape[:-1], np.float64)
    seq = np.full(im.shape[:-1], full, np.float64)
    part = np.zeros(im.shape[:-1], np.float64)
    for n in range(topo.n_nodes):
        order = order + np.where(im[..., n], 0.0, term[n])
        seq = seq - np.where(im[..., n], term[n], 0.0)
        part = part + np.where(im[..., n], term[n], 0.0)
    n_im = im.sum(axis=-1)
    return dict(order=order / total, sub_seq=seq / total, sub_sum=(full - part) / total, uniform=(full - n_im * term[0]) / total, n=n_im)


def compared(c: Case) -> np.ndarray:
    """[T, E] bool: played steps that do not end their episode (the pairs the restatement is compared on)."""
    return c.live & (c.out["oob"] == 0) & ~c.ended


def _bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def discriminating(c: Case) -> np.ndarray:
    """[T, E] bool: a node is being re-imaged and the kernel branches the topology must NOT take give other bits than the node-order sum:
    the uniform shortcut, and for an order-dependent topology both ways of subtracting from full_sum."""
    return discriminating_of(c.topo, c.imaging)


def discriminating_of(topo, im: np.ndarray) -> np.ndarray:
    s = sums_of(topo, im)
    d = (s["n"] > 0) & (_bits(s["uniform"]) != _bits(s["order"]))
    if int(topo.header()["avail_any_order"]) == 0:
        d &= (_bits(s["sub_seq"]) != _bits(s["order"])) & (_bits(s["sub_sum"]) != _bits(s["order"]))
    return d


def sla_candidates(p: Case, v: float) -> np.ndarray:
    """Envs of the pilot whose first episode meets v exactly on its first played step at or below v, on a discriminating step."""
    play = first_episode(p) & p.live & (p.out["oob"] == 0)
    low = play & (p.out["availability"] <= v)
    t0 = np.argmax(low, axis=0)
    cols = np.flatnonzero(low.any(axis=0))
    hit = (p.out["availability"][t0[cols], cols] == v) & discriminating(p)[t0[cols], cols]
    return cols[hit]


@functools.lru_cache(maxsize=None)
def _sla_value(topo_name: str, kind: str) -> float:
    """The availability below full that the most envs of the pilot meet as sla_candidates do."""
    p = case(f"{topo_name}-avail_{kind}")
    play = first_episode(p) & p.live & (p.out["oob"] == 0) & discriminating(p)
    values, counts = np.unique(p.out["availability"][play], return_counts=True)
    best, best_n = None, 0
    for v in values[np.argsort(-counts)][:40]:                      # (the most frequent values: a value few steps show ends few envs)
        n = sla_candidates(p, float(v)).size
        if n > best_n:
            best, best_n = float(v), n
    assert best is not None, f"{topo_name} {kind}: no first episode of the pilot shows a discriminating availability"
    return best


def _weighted_case(name: str, topo_name: str, spec_name: str) -> Case:
    base, kind = spec_name.rsplit("_", 1)
    topo = topology(topo_name, kind)
    params = {}
    sla = 0.0
    if base != "avail":
        v = _sla_value(topo_name, kind)
        sla = v if base == "sla_eq" else float(np.nextafter(v, np.inf))
        params["v"] = v
    spec = make_spec(topo, maintain_sla=sla, **weighted_settings(topo_name))
    return run(name, topo, spec, WEIGHT_STEPS, params=params, record_imaging=True)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    topo_name, spec_name = name.split("-")
    if spec_name in WEIGHT_SPECS:
        return _weighted_case(name, topo_name, spec_name)
    topo = topology(topo_name)
    N = topo.n_nodes
    params, reset_at, stall = {}, -1, 0.0
    n_steps = STEPS[spec_name]
    if spec_name in ("mixed", "frozen"):
        m = _mixed_bound(topo_name)
        params["bound"] = m
        spec = make_spec(topo, attacker_goal=dict(MIXED_GOAL), defender=SCAN, maintain_sla=0.0, max_episode_steps=m,
                         auto_reset=spec_name == "mixed")
        if spec_name == "frozen":                  # every env has ended by step m: two idle thirds would compare nothing
            n_steps = 3 * m + 6
            reset_at = 2 * n_steps // 3
    elif spec_name == "updown":
        # `mixed` ends an episode the moment two nodes are owned at the end of a step, so there the counter never comes down and goes
        # up again between steps.  Three nodes to win and a defender that re-images often: it sits at 2, falls to 1, rises again.
        defender, bound = updown_settings(topo_name, N)
        spec = make_spec(topo, attacker_goal=dict(MIXED_GOAL, own_atleast=3), defender=defender, maintain_sla=0.0, max_episode_steps=bound)
    elif spec_name in ("reward", "reward_def"):
        R = _reward_goal(topo_name, spec_name)
        params["R"] = R
        spec = make_spec(topo, attacker_goal=dict(reward=R, own_atleast_percent=0.0), defender=SCAN if spec_name == "reward_def" else None)
    elif spec_name == "sla":
        spec = make_spec(topo, attacker_goal=dict(own_atleast_percent=1.0), defender=SCAN_AVAIL, maintain_sla=near_one(N), defender_goal_eviction=False)
    elif spec_name == "lowavail":
        spec = make_spec(topo, attacker_goal=dict(own_atleast_percent=0.0, low_availability=near_one(N)), defender=SCAN_AVAIL, maintain_sla=0.0,
                         defender_goal_eviction=False)
    elif spec_name == "sla_evict":
        # The availability a step compares is the one from before that step's scan, so a re-image shows one step later, and with a scan
        # every 2nd step that step has no scan: SLA and eviction cannot meet on a step while the SLA is only just breakable.  Here it is
        # out of reach (every played step breaks it) and half of the envs open an episode with an out-of-bound row, which skips the
        # defender: their first played step is step 2, a scan step, and the scan may evict on it.  The win must take precedence.
        spec = make_spec(topo, attacker_goal=dict(own_atleast_percent=1.0), defender=SCAN_AVAIL, maintain_sla=1.5)
        stall = 0.5
    else:
        k = _percent_k(topo_name)
        pct, need = percent_values(k, N)[spec_name]
        params.update(k=k, need=need)
        spec = make_spec(topo, attacker_goal=dict(own_atleast_percent=pct, low_availability=2.0), defender=SCAN)
    return run(name, topo, spec, n_steps, reset_at=reset_at, stall=stall, params=params)
