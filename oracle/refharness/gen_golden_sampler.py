"""Histograms of the UNMODIFIED reference's sample_valid_action in fixed states -> tests/golden/sampler_histograms.json.

Run in the build container only (needs the reference):   python oracle/refharness/gen_golden_sampler.py

For each state the imported reference env (no defender) is reset with a fixed seed, walked to the state by `walk` actions it samples
itself (sample_valid_action, recorded: the fixture's `script` reproduces the state on any stepper), and then asked DRAWS times for
sample_valid_action() without stepping.  Both generators it draws from are seeded the way gen_golden.py seeds them: `env.np_random` by
reset(seed=...), `env.action_space.union_np_random` by assignment.  Recorded: the script and the count of every drawn action (data
only, a few KB).  tests/test_sampler_law.py replays the script through the CPU oracle, computes the law with tests/sampler_law.py and
runs its goodness-of-fit test on these counts.

DRAWS is large enough that every action of every state's support expects well over 50 draws (the rarest, a connect action of the
ToyCtf mid-episode state, has probability about 1/1500); the test asserts that from the law before it looks at the counts.  The
reference rebuilds its action mask in Python loops on every call: the recipe takes a few minutes.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import ref_loader  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
DRAWS = 400_000


def to_action_dict(a):
    return {0: {"local_vulnerability": np.array(a[1:3])}, 1: {"remote_vulnerability": np.array(a[1:4])}, 2: {"connect": np.array(a[1:5])}}[a[0]]


def from_action_dict(d):
    if "local_vulnerability" in d:
        v = d["local_vulnerability"]
        return [0, int(v[0]), int(v[1]), 0, 0]
    if "remote_vulnerability" in d:
        v = d["remote_vulnerability"]
        return [1, int(v[0]), int(v[1]), int(v[2]), 0]
    v = d["connect"]
    return [2, int(v[0]), int(v[1]), int(v[2]), int(v[3])]


def histogram(name, topology, make_env, spec, seed, walk, need_owned):
    env = make_env()
    env.action_space.union_np_random = np.random.Generator(np.random.PCG64(seed + 1))
    obs, info = env.reset(seed=seed)
    script = []
    for _ in range(walk):
        a = from_action_dict(env.sample_valid_action())
        obs, _, done, _, info = env.step(to_action_dict(a))
        assert not done, f"{name}: the walk ended the episode"
        script.append(a)
    owned = int((np.asarray(obs["nodes_privilegelevel"]) >= 1).sum()) if walk else 1
    n_creds = int(obs["credential_cache_length"]) if walk else 0
    assert owned >= need_owned and (n_creds > 0) == (walk > 0), f"{name}: {owned} owned nodes, {n_creds} cached credentials"
    counts = {}
    for _ in range(DRAWS):
        a = tuple(from_action_dict(env.sample_valid_action()))
        counts[a] = counts.get(a, 0) + 1
    print(f"{name:24s} walk={walk:3d} owned={owned} creds={n_creds} distinct actions={len(counts)} min count={min(counts.values())}")
    return dict(name=name, topology=topology, spec=spec, seed=seed, script=script, owned=owned, n_creds=n_creds, draws=DRAWS,
                counts=[list(k) + [counts[k]] for k in sorted(counts)])


def main():
    ref = ref_loader.load()
    AG = ref.env.AttackerGoal
    sp_c4 = dict(maximum_node_count=6, maximum_total_credentials=6, maximum_discoverable_credentials_per_action=5)
    sp_t = dict(maximum_node_count=12, maximum_total_credentials=10, maximum_discoverable_credentials_per_action=5)

    def chain4():
        return ref.CyberBattleChain(size=4, attacker_goal=AG(own_atleast_percent=1.0), throws_on_invalid_actions=False,
                                    maximum_node_count=6, maximum_total_credentials=6)

    def toyctf():
        return ref.CyberBattleToyCtf(attacker_goal=AG(own_atleast_percent=1.0), throws_on_invalid_actions=False,
                                     maximum_node_count=12, maximum_total_credentials=10)

    states = [
        histogram("chain4_reset", "chain4", chain4, sp_c4, 301, 0, 1),
        histogram("chain4_mid", "chain4", chain4, sp_c4, 302, CHAIN4_WALK, 3),
        histogram("toyctf_reset", "toyctf", toyctf, sp_t, 303, 0, 1),
        histogram("toyctf_mid", "toyctf", toyctf, sp_t, 304, TOYCTF_WALK, 3),
    ]
    path = os.path.join(GOLDEN, "sampler_histograms.json")
    with open(path, "w") as f:
        json.dump(dict(states=states), f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{path}: {os.path.getsize(path) / 1024:.1f} KiB")


# walk lengths: the first at which the seeded walk owns >= 3 nodes with a non-empty cache (asserted above)
CHAIN4_WALK = 125
TOYCTF_WALK = 305

if __name__ == "__main__":
    main()
