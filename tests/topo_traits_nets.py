"""Topology traits (MCBS_TOPO_*, include/mcbs.h) computed from a sample's model objects, independently of marlon_amd/flatten.py and of the
native library, and the hand-made networks of tests/test_topo_traits.py and tests/test_gpu_step_narrow.py: a base network of four nodes
with no trait at all and five variants that each switch on exactly one."""
from marlon_amd import model as m
from marlon_amd._abi import (TOPO_ESCALATION, TOPO_LATERAL_EXPLOIT, TOPO_MULTI_LEAK, TOPO_PRECONDITION, TOPO_PROBE, TOPO_WIDE_ROWS)

TRAIT_NAMES = {TOPO_ESCALATION: "escalation", TOPO_LATERAL_EXPLOIT: "lateral-move exploit", TOPO_PRECONDITION: "precondition",
               TOPO_PROBE: "probe", TOPO_MULTI_LEAK: "multi-entry leak", TOPO_WIDE_ROWS: "more than 12 nodes"}
# what the narrow lean step kernel still handles (marlon_amd/csrc/mcbs_step.hip kNarrowStepCan): a topology with any other trait
# takes the general lean kernel.  ("At most 12 nodes" was measured not to pay and is not assumed: profiles/step_topo_traits.md.)
NARROW_CAN = TOPO_PROBE | TOPO_WIDE_ROWS


def traits_of(env) -> int:
    """From the model objects: every vulnerability a node can be attacked with (the library's entries shadow the node's own,
    actions.py:342-345), its outcome's class, its precondition over the node's properties and each of the 16 sets of privilege tags."""
    nodes = list(env.nodes())
    t = TOPO_WIDE_ROWS if len(nodes) > 12 else 0
    tag_sets = [{f"privilege_{k}" for k in range(4) if s >> k & 1} for s in range(16)]
    for _, info in nodes:
        vulns = dict(info.vulnerabilities)
        vulns.update(env.vulnerability_library)
        for v in vulns.values():
            o = v.outcome
            if isinstance(o, m.PrivilegeEscalation):
                t |= TOPO_ESCALATION
            elif isinstance(o, m.LateralMove):
                t |= TOPO_LATERAL_EXPLOIT
            elif isinstance(o, m.ProbeSucceeded):
                t |= TOPO_PROBE
            elif isinstance(o, m.LeakedCredentials) and len(o.credentials) > 1:
                t |= TOPO_MULTI_LEAK
            elif isinstance(o, m.LeakedNodesId) and len(o.nodes) > 1:
                t |= TOPO_MULTI_LEAK
            if not all(v.precondition.expression.evaluate(set(info.properties) | tags) for tags in tag_sets):
                t |= TOPO_PRECONDITION
    return t


def _vuln(kind, outcome, pre="true", cost=1.0):
    return m.VulnerabilityInfo(description="", type=m.VulnerabilityType.LOCAL if kind == "local" else m.VulnerabilityType.REMOTE,
                               outcome=outcome, precondition=m.Precondition(pre), cost=cost)


def handmade(which: str) -> m.Environment:
    """client (agent installed) -> web -> db, plus a vault nobody names.  The client's history names web; web's page source (remote)
    leaks web's SSH credential; once owned, web's shell history names db and its key file holds db's SSH credential.  Every exploit of
    the base network leaks ONE entry, has no precondition, and none escalates, moves laterally or probes: no trait.
    `which`: base | escalation | lateral | precondition | leak2 | nodes13 — the base plus the one rule the name says."""
    assert which in HANDMADE
    client_v = {"History": _vuln("local", m.LeakedNodesId(["web"]))}
    web_v = {"PageSource": _vuln("remote", m.LeakedCredentials([m.CachedCredential("web", "SSH", "web-pw")])),
             "ShellHistory": _vuln("local", m.LeakedNodesId(["db"])),
             "KeyFile": _vuln("local", m.LeakedCredentials([m.CachedCredential("db", "SSH", "db-pw")]), cost=2.0)}
    db_v = {"PageSource": _vuln("remote", m.ExploitFailed(), cost=3.0)}
    if which == "escalation":
        web_v["Sudo"] = _vuln("local", m.AdminEscalation())
    elif which == "lateral":
        db_v["Hop"] = _vuln("remote", m.LateralMove())
    elif which == "precondition":
        db_v["Dump"] = _vuln("local", m.LeakedNodesId(["vault"]), pre="Windows")      # db is a Linux machine: false there
    elif which == "leak2":
        web_v["ShellHistory"] = _vuln("local", m.LeakedNodesId(["db", "vault"]))
    nodes = {
        "client": m.NodeInfo(services=[], value=0, properties=["Windows"], vulnerabilities=client_v, agent_installed=True, reimagable=False),
        "web": m.NodeInfo(services=[m.ListeningService("HTTPS"), m.ListeningService("SSH", allowedCredentials=["web-pw"])], value=100,
                          properties=["Linux"], vulnerabilities=web_v),
        "db": m.NodeInfo(services=[m.ListeningService("SSH", allowedCredentials=["db-pw"])], value=500, properties=["Linux"], vulnerabilities=db_v),
        "vault": m.NodeInfo(services=[m.ListeningService("HTTPS")], value=1000, properties=["Linux"], vulnerabilities={}),
    }
    if which == "nodes13":
        for k in range(9):
            nodes[f"spare{k}"] = m.NodeInfo(services=[m.ListeningService("HTTPS")], value=10 + k, properties=["Linux"], vulnerabilities={})
        db_v["PageSource"] = _vuln("remote", m.LeakedNodesId(["spare8"]), cost=3.0)   # the thirteenth node's row: the fourth row vector
    ids = m.infer_constants_from_nodes(list(nodes.items()), {})
    return m.Environment(network=m.create_network(nodes), vulnerability_library={}, identifiers=ids)


# name -> the one trait it switches on (0: none)
HANDMADE = {"base": 0, "escalation": TOPO_ESCALATION, "lateral": TOPO_LATERAL_EXPLOIT, "precondition": TOPO_PRECONDITION,
            "leak2": TOPO_MULTI_LEAK, "nodes13": TOPO_WIDE_ROWS}


def describe(t: int) -> str:
    return " + ".join(n for b, n in TRAIT_NAMES.items() if t & b) or "none"

