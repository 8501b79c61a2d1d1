"""The reference's winning Chain-10 script (tests/golden/chain10_script.npz: 56 engine rows at bounds 12/12, with the observation and
the three mask fields recorded after every step, and the same for a fresh env under `reset_*`) as a schedule for one batch under
`TwoAgentTrainVecEnv`, in numpy.  Env e waits d_e = e % PERIOD turns with an action the wrapper intercepts, then plays script steps
0, 1, 2, ... one per turn, and starts over (wait d_e, then step 0) whenever its attacker episode ends; the defender plays an action
that changes nothing.  The defender's timeout then re-initialises every env under the attacker's standing observation at once, and
the envs stand at script steps spread over the whole script when it does: the discovery order of the observation (node 2 at index 1,
node 1 last) differs from a fresh env's at every owned index >= 1, which is what the own-list mask kernels are held to
(tests/test_gpu_training_masks.py).  tests/test_training_script_host.py checks the schedule itself without a GPU.

Nothing here is computed by the library: masks and observations are the recorded ones, zero-padded to larger bounds."""
from __future__ import annotations

import json
import os

import numpy as np

from tests.sampler_law import Geometry

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ["scalars", "leaked_credentials", "credential_cache_matrix", "discovered_nodes_properties", "nodes_privilegelevel"]
MASKS = ["mask_connect", "mask_local", "mask_remote"]            # the Discrete order
PERIOD = 52
ATTACKER_TIMEOUT, DEFENDER_TIMEOUT = 300, 50
RESET, UNKNOWN = -1, -2                                           # "script step" of the reset observation / of an observation nobody recorded


def defender_noop(E: int) -> np.ndarray:
    """[E, 12] rows of DefenderVecEnv's MultiDiscrete space: kind 3 (stop_service) on node 0, service 0 — valid or not, the reference's
    stop_service has no effect on the environment (defender.py:45-48), and an invalid action changes nothing either."""
    a = np.zeros((E, 12), np.int64)
    a[:, 0] = 3
    return a


class Script:
    def __init__(self):
        z = np.load(os.path.join(GOLDEN, "chain10_script.npz"))
        self.spec_json = json.loads(bytes(z["spec_json"]).decode())
        assert (self.spec_json["maximum_node_count"], self.spec_json["maximum_total_credentials"]) == (12, 12) and self.spec_json["defender"] is None
        self.rows = z["actions"].astype(np.int64)                 # [56, 5] engine rows (kind, a, b, c, d)
        self.n_steps = len(self.rows)
        self.terminated = z["terminated"] != 0
        assert self.terminated.tolist() == [False] * (self.n_steps - 1) + [True]
        # index s + 1 = after script step s; index 0 = a fresh env (so that the RESET index -1 selects row 0 after + 1)
        cat = lambda k: np.concatenate([z["reset_" + k][None], z[k]])
        self.fields = {k: cat(k) for k in FIELDS}
        self.masks = {k: cat(k) for k in MASKS}
        fresh = np.full((1, 12), 0xFFFF, np.int64)
        fresh[0, 0] = 0
        self.order = np.concatenate([fresh, z["order"].astype(np.int64)])                    # node id at every discovery index, 0xFFFF beyond the count
        self.n_disc = np.concatenate([[1], z["n_order"]]).astype(np.int64)
        self.n_creds = np.concatenate([[0], z["n_cache"]]).astype(np.int64)
        assert (self.n_disc == self.fields["scalars"][:, 6]).all() and (self.n_creds == self.fields["scalars"][:, 5]).all()
        self.owned = self.fields["nodes_privilegelevel"] > 0                                 # by discovery index
        assert not (self.owned & (np.arange(12)[None, :] >= self.n_disc[:, None])).any()
        self.L, self.R, self.P = z["mask_local"].shape[2], z["mask_remote"].shape[3], z["mask_connect"].shape[3]

    # ---- geometry ----
    def geometry(self, N: int = 12, C: int = 12) -> Geometry:
        from marlon_amd._abi import EnvSpec
        from tests import parity
        g = Geometry(parity.topology_for("chain10_script"), EnvSpec(maximum_node_count=N, maximum_total_credentials=C))
        assert (g.L, g.R, g.P) == (self.L, self.R, self.P)
        return g

    def wait_action(self, geo: Geometry) -> int:
        """The local action (node index maximum_node_count - 1, vulnerability 0): beyond the discovered range of every standing state
        (the wrapper intercepts it: the observation and its digest stand, the wrapper's clocks tick), and never inside a recorded mask."""
        return int(geo.encode(np.array([0, geo.N - 1, 0, 0, 0], np.int64)))

    # ---- what an env holds, from the index of the script step it stands at (RESET: the fresh observation) ----
    @staticmethod
    def _pad(x, shape):
        out = np.zeros((x.shape[0],) + tuple(shape), x.dtype)
        out[(slice(None),) + tuple(slice(0, n) for n in x.shape[1:])] = x
        return out

    def observation(self, held, N: int = 12, C: int = 12) -> dict:
        """The five int32 observation fields [n, ...] of the script steps `held`, zero-padded to bounds N / C."""
        i = np.asarray(held) + 1
        assert (i >= 0).all()
        f = {k: v[i] for k, v in self.fields.items()}
        f["credential_cache_matrix"] = self._pad(f["credential_cache_matrix"], (C, 2))
        f["discovered_nodes_properties"] = self._pad(f["discovered_nodes_properties"], (N, f["discovered_nodes_properties"].shape[2]))
        f["nodes_privilegelevel"] = self._pad(f["nodes_privilegelevel"], (N,))
        return f

    def _mask_fields(self, held, N, C):
        i = np.asarray(held) + 1
        assert (i >= 0).all()
        return (self._pad(self.masks["mask_connect"][i], (N, N, self.P, C)), self._pad(self.masks["mask_local"][i], (N, self.L)),
                self._pad(self.masks["mask_remote"][i], (N, N, self.R)))

    def expected_mask(self, held, N: int = 12, C: int = 12) -> np.ndarray:
        """bool [n, A] in connect | local | remote order (oracle_mask of tests/test_gpu_packed_masks.py) from the recorded mask fields."""
        n = len(np.asarray(held))
        return np.concatenate([m.reshape(n, -1) for m in self._mask_fields(held, N, C)], axis=1) != 0

    def live_list_mask(self, held, N: int = 12, C: int = 12) -> np.ndarray:
        """The mask a kernel would build for the standing observations `held` from the discovery list of a RE-INITIALISED env
        ([0, 0xFFFF, ...]: no node at any index >= 1): the expected mask with the local row of every owned index >= 1 zeroed."""
        n = len(np.asarray(held))
        connect, local, remote = self._mask_fields(held, N, C)
        own = self._pad(self.owned[np.asarray(held) + 1], (N,))
        local = local.copy()
        local[:, 1:][own[:, 1:]] = 0
        return np.concatenate([m.reshape(n, -1) for m in (connect, local, remote)], axis=1) != 0

    def deepest_owned_index(self, held) -> np.ndarray:
        own = self.owned[np.asarray(held) + 1]
        return np.where(own.any(axis=1), own.shape[1] - 1 - np.argmax(own[:, ::-1], axis=1), -1)

    def key_state(self, held, topo):
        """(headers, nodes, order) as marlon_amd.mask_keys.keys_from_state takes them: the expected counts, the owned bits (as the
        installed flags of the nodes the script's order names) and the script's discovery order."""
        i = np.asarray(held) + 1
        n = len(i)
        hdr = np.zeros(n, dtype=[("last_oob", np.uint8), ("n_discovered", np.int64), ("n_creds", np.int64)])
        hdr["n_discovered"], hdr["n_creds"] = self.n_disc[i], self.n_creds[i]
        order = self.order[i]
        installed = np.zeros((n, topo.n_nodes), np.uint8)
        for j in range(order.shape[1]):
            on = self.owned[i][:, j]
            installed[np.flatnonzero(on), order[on, j]] = 1
        return hdr, {"installed": installed}, np.where(order == 0xFFFF, 0, order)


class Schedule:
    """Per turn t = 1 .. turns (row t - 1) and env: `actions` (Discrete), `held` (the script step whose observation and mask the env
    holds after the turn, RESET for the fresh ones), `request` (the attacker's reset_request byte after the turn), `dones` (the
    attacker's), `terminal` (the script step of the terminal observation where dones, UNKNOWN where nobody recorded it), `played`
    (the script step the action is, -1 for the waiting action), `acted` (the env's digest was written by a turn: a live step or an
    episode end since reset())."""

    def __init__(self, script: Script, geo: Geometry, E: int, turns: int, period: int = PERIOD, attacker_timeout: int = ATTACKER_TIMEOUT,
                 defender_timeout: int = DEFENDER_TIMEOUT):
        self.script, self.geo, self.E, self.turns = script, geo, E, turns
        self.delay = np.arange(E) % period
        wait_a = script.wait_action(geo)
        script_a = geo.encode(script.rows)
        rows = script.rows
        # the nodes an action names must lie inside the live env's discovered range, or the wrapper intercepts it
        first = rows[:, 1]
        second = np.where(rows[:, 0] == 0, 0, rows[:, 2])
        need = np.maximum(first, second) + 1
        shape = (turns, E)
        self.actions, self.held, self.played = np.zeros(shape, np.int64), np.zeros(shape, np.int64), np.zeros(shape, np.int64)
        self.request, self.dones, self.acted = np.zeros(shape, bool), np.zeros(shape, bool), np.zeros(shape, bool)
        self.terminal = np.full(shape, UNKNOWN, np.int64)
        held = np.full(E, RESET)                   # the observation the attacker holds
        live = np.full(E, RESET)                   # the script step the ENV stands at (differs from held after a defender-side reset)
        wait, ptr = self.delay.copy(), np.zeros(E, np.int64)
        a_clock, d_clock = np.zeros(E, np.int64), np.zeros(E, np.int64)
        request, acted = np.zeros(E, bool), np.zeros(E, bool)
        for t in range(turns):
            done = np.zeros(E, bool)
            for e in range(E):
                nd = int(script.n_disc[live[e] + 1])
                if wait[e] > 0 or ptr[e] >= script.n_steps:
                    wait[e] -= wait[e] > 0
                    s, executed = -1, False
                    self.actions[t, e] = wait_a
                    assert geo.N - 1 >= nd, "the waiting action would reach the engine: the env has discovered every index"
                else:
                    s = int(ptr[e])
                    ptr[e] += 1
                    self.actions[t, e] = script_a[s]
                    executed = need[s] <= nd
                self.played[t, e] = s
                a_clock[e] += 1
                in_sync = executed and live[e] == s - 1
                if executed and not in_sync and not request[e]:
                    raise NotImplementedError(f"turn {t + 1} env {e}: script step {s} on an env at step {live[e]} with no request pending: not recorded")
                terminated = bool(in_sync and script.terminated[s] and not request[e])
                after = s if in_sync else (held[e] if not executed else UNKNOWN)            # the observation of this step
                if in_sync:
                    live[e] = s
                done[e] = terminated or request[e] or a_clock[e] >= attacker_timeout
                if done[e]:
                    self.terminal[t, e] = after
                    held[e] = live[e] = RESET
                    a_clock[e], wait[e], ptr[e] = 0, self.delay[e], 0
                elif executed:
                    held[e] = after
                acted[e] |= executed or done[e]
            notify = done & ~request
            d_clock += 1
            done2 = (d_clock >= defender_timeout) | notify
            d_clock[done2] = 0
            live[done2] = RESET                    # the env is re-initialised; the attacker's observation stands
            request = done2 & ~notify
            self.held[t], self.request[t], self.dones[t], self.acted[t] = held, request, done, acted

    def held_before(self, turn: int) -> np.ndarray:
        """What the attacker holds when it chooses the action of turn `turn` (1-based)."""
        return self.held[turn - 2] if turn >= 2 else np.full(self.E, RESET)

    def stale(self, turn: int) -> np.ndarray:
        """bool [E]: after turn `turn` the env was re-initialised under an observation that stands (a request is pending)."""
        return self.request[turn - 1].copy()
