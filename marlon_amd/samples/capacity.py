"""Synthetic topologies that sit ON the capacity limits of the topology format (include/mcbs.h MCBS_MAX_*, flatten.MAX_*).

Not reference topologies: they exist so that every bit position the kernels' fields are sized for is reached by a test
(tests/capacity.py, tests/test_gpu_capacity_limits.py) and by golden traces captured from the reference on these very networks
(tests/golden/limits_*.npz, credlimits257_*.npz).  Every builder takes the model module to build with, like random_net.build:
marlon_amd.model here, the reference's simulation.model in oracle/refharness.

  row_limits         32 ports, 60 properties, 32 local ids, 32 vulnerability slots per node: bit 31 of the port masks, of the local
                     mask and of the attacked-ever / attacked-since words; property bit 59 right below the four privilege tags.
  packed_edge        at most 16 nodes and 15 credentials with n_props + 4 + 2 * slots on either side of the 32-bit packed-row budget.
  credential_limits  256 credential strings and up to 1 024 (node, port, credential) triples, leaked in scrambled slices and,
                     optionally, 1 023 of them by one action.
"""
from __future__ import annotations


def _allow_all(m, ports, block_in=()):
    A, B = m.RulePermission.ALLOW, m.RulePermission.BLOCK
    return m.FirewallConfiguration(incoming=[m.FirewallRule(p, B if p in block_in else A) for p in ports],
                                   outgoing=[m.FirewallRule(p, A) for p in ports])


def _vuln(m, kind, outcome, cost, pre=None):
    kw = dict(description="", type=kind, outcome=outcome, cost=float(cost))
    if pre is not None:
        kw["precondition"] = m.Precondition(pre)
    return m.VulnerabilityInfo(**kw)


def row_limits(m, n_nodes: int = 6, n_ports: int = 32, n_props: int = 60, n_local: int = 32, n_remote: int = 8, slots: int = 32):
    """A ring n000 -> n001 -> ... of nodes that all carry `slots` vulnerabilities: slots - 2 local ones (the FIRST slots - 2 local ids on
    even nodes, the LAST on odd ones, so local id 0 and local id n_local - 1 both occur) and the first and the last remote id.

    * local outcomes cycle through LeakedNodesId (the next node), LeakedCredentials (the next node's credential, on the last port for
      even slots and the first port for odd ones; on the last port only in rings of more than 64 nodes) and ProbeSucceeded (the node's own highest properties); local slot 1 escalates
      (Admin on even nodes, System on odd ones), so the tags are written right above property n_props - 1;
    * every node listens on the first and the last port; every node allows every port both ways except node 2, whose incoming rules
      block the last port (a connect there is refused by bit n_ports - 1 of the firewall mask and succeeds through port 0);
    * every node owns property n_props - 1 except node 3; the last local vulnerability of a node requires that property, so it holds
      everywhere but on node 3 (an odd node: there it is local id n_local - 1 that fails);
    * the first remote id leaks the next node, the last one the node's mirror image n_nodes - 1 - i (with more than 64 nodes: a node whose bit
      lies in another word of the node sets)."""
    LOCAL, REMOTE = m.VulnerabilityType.LOCAL, m.VulnerabilityType.REMOTE
    assert 3 <= slots <= n_local + 2 and n_remote >= 2 and n_nodes >= 4 and n_ports >= 3
    # the first and the last port carry names the learned defender manages (LearningDefender.firewall_rule_list): its firewall actions
    # then reach bit 0 and bit n_ports - 1 of the port masks
    ports = ["RDP"] + [f"P{i:02d}" for i in range(1, n_ports - 1)] + ["sudo"]
    props = [f"p{i:02d}" for i in range(n_props)]
    loc = [f"L{i:02d}" for i in range(n_local)]
    rem = [f"R{i:03d}" for i in range(n_remote)]
    names = [f"n{i:03d}" for i in range(n_nodes)]
    top = props[-1]
    two_ports = n_nodes <= 64          # larger rings: one triple per node, so that 130 nodes stay below the 256 triples of the narrow sets
    nodes = {}
    for i, name in enumerate(names):
        nxt, far = names[(i + 1) % n_nodes], names[n_nodes - 1 - i]
        own = props[i::n_nodes]
        if top not in own and i != 3:
            own = own + [top]
        own_local = loc[:slots - 2] if i % 2 == 0 else loc[n_local - (slots - 2):]
        vul = {}
        for j, vid in enumerate(own_local):
            k = (i + j) % 3
            if j == 1:
                out = m.AdminEscalation() if i % 2 == 0 else m.SystemEscalation()
            elif k == 0:
                out = m.LeakedNodesId([nxt])
            elif k == 1:
                out = m.LeakedCredentials([m.CachedCredential(nxt, ports[0] if j % 2 and two_ports else ports[-1], f"k{i:03d}")])
            else:
                out = m.ProbeSucceeded([own[-1 - (j % len(own))]])
            vul[vid] = _vuln(m, LOCAL, out, 1 + j % 3, top if j == len(own_local) - 1 else None)
        vul[rem[0]] = _vuln(m, REMOTE, m.LeakedNodesId([nxt]), 2)
        vul[rem[-1]] = _vuln(m, REMOTE, m.LeakedNodesId([far]), 2)
        key = f"k{(i - 1) % n_nodes:03d}"
        nodes[name] = m.NodeInfo(
            services=[m.ListeningService(ports[-1], allowedCredentials=[key]), m.ListeningService(ports[0], allowedCredentials=[key])],
            value=10 * (i % 11), agent_installed=(i == 0), reimagable=(i != 0), properties=own,
            firewall=_allow_all(m, ports, block_in=(ports[-1],) if i == 2 else ()), vulnerabilities=vul)
    ids = m.Identifiers(properties=props, ports=ports, local_vulnerabilities=loc, remote_vulnerabilities=rem)
    return m.Environment(network=m.create_network(nodes), vulnerability_library={}, identifiers=ids)


def packed_edge(m, n_props: int, slots: int, n_nodes: int = 16):
    """16 nodes, 15 credential triples, n_props properties and `slots` vulnerabilities on every node: n_props + 4 + 2 * slots is the
    width of a packed node row.  Slot s of node i is, by (i + s) % 4: a local leak of the next three nodes' credentials, a local probe of
    the node's highest property (property n_props - 1, the bit below the tags), a local Admin escalation, a remote leak of the next two
    node ids.  With one slot per node the attacker gets as far as the fourth node; the row formats are exercised all the same."""
    LOCAL, REMOTE = m.VulnerabilityType.LOCAL, m.VulnerabilityType.REMOTE
    assert 4 <= n_nodes <= 16 and slots >= 1
    ports = ["P0", "P1", "P2", "P3"]
    props = [f"p{i:02d}" for i in range(n_props)]
    names = [f"n{i:02d}" for i in range(n_nodes)]

    def cred(j):                                     # the one credential of node j (j = 1 .. n_nodes - 1): n_nodes - 1 <= 15 triples
        j = 1 + (j - 1) % (n_nodes - 1)
        return m.CachedCredential(names[j], ports[-1], f"k{j:02d}")

    nodes = {}
    for i, name in enumerate(names):
        own = sorted({props[i % n_props], props[-1]})
        vul = {}
        for s in range(slots):
            k = (i + s) % 4
            if k == 0:
                vul[f"L{s:02d}"] = _vuln(m, LOCAL, m.LeakedCredentials([cred(i + d) for d in (1, 2, 3)]), 1 + s)
            elif k == 1:
                vul[f"L{s:02d}"] = _vuln(m, LOCAL, m.ProbeSucceeded([own[-1]]), 1 + s)
            elif k == 2:
                vul[f"L{s:02d}"] = _vuln(m, LOCAL, m.AdminEscalation(), 1 + s)
            else:
                vul[f"R{s:02d}"] = _vuln(m, REMOTE, m.LeakedNodesId([names[(i + 1) % n_nodes], names[(i + 2) % n_nodes]]), 1 + s)
        nodes[name] = m.NodeInfo(
            services=[m.ListeningService(ports[-1], allowedCredentials=[f"k{i:02d}"])] if i else [],
            value=5 * i, agent_installed=(i == 0), reimagable=(i != 0), properties=own, firewall=_allow_all(m, ports), vulnerabilities=vul)
    ids = m.Identifiers(properties=props, ports=ports, local_vulnerabilities=[f"L{s:02d}" for s in range(slots)],
                        remote_vulnerabilities=[f"R{s:02d}" for s in range(slots)])
    return m.Environment(network=m.create_network(nodes), vulnerability_library={}, identifiers=ids)


def credential_triple(k: int, others: int = 8, n_ports: int = 32, n_strings: int = 256):
    """(node index among the servers, port index, credential string index) of triple k."""
    return k % others, (k // others) % n_ports, (k % 256 + k // 256) % n_strings


def credential_limits(m, n_triples: int, n_strings: int = 256, others: int = 8, n_ports: int = 32, n_leaks: int = 12, leak_all: bool = False):
    """A client and `others` servers.  The client's local vulnerabilities Leak00 .. leak every triple in scrambled slices (cache positions and
    triple ids then differ) and Seq00 .. the same triples in order;
    leak_all adds LeakAll, one action that leaks min(n_triples, 1 023) triples at once.  Server s listens on every port one of its
    triples names and accepts that triple's string there, so every cached credential opens its node."""
    LOCAL, REMOTE = m.VulnerabilityType.LOCAL, m.VulnerabilityType.REMOTE
    ports = [f"P{i:02d}" for i in range(n_ports)]
    names = [f"s{i}" for i in range(others)]
    tr = []
    for k in range(n_triples):
        n, p, c = credential_triple(k, others, n_ports, n_strings)
        tr.append((names[n], ports[p], f"c{c:03d}"))
    assert len(set(tr)) == n_triples, "the triples must be distinct"
    mult = 7 if n_triples % 7 else 5
    order = [(k * mult + 3) % n_triples for k in range(n_triples)]
    assert len(set(order)) == n_triples
    # triple ids are handed out in order of first appearance (flatten): the Seq vulnerabilities come first and name the triples in order,
    # which pins id k to triple k; the Leak vulnerabilities name the same triples in the scrambled order
    vul = {"Find": _vuln(m, LOCAL, m.LeakedNodesId(list(names[:2])), 1)}
    per = -(-n_triples // n_leaks)
    seqs, leaks = [], []
    for j in range(n_leaks):
        if j * per < n_triples:
            seqs.append(f"Seq{j:02d}")
            vul[seqs[-1]] = _vuln(m, LOCAL, m.LeakedCredentials([m.CachedCredential(*tr[k]) for k in range(j * per, min(n_triples, (j + 1) * per))]), 2)
    for j in range(n_leaks):
        part = order[j * per:(j + 1) * per]
        if part:
            leaks.append(f"Leak{j:02d}")
            vul[leaks[-1]] = _vuln(m, LOCAL, m.LeakedCredentials([m.CachedCredential(*tr[k]) for k in part]), 1)
    if leak_all:
        vul["LeakAll"] = _vuln(m, LOCAL, m.LeakedCredentials([m.CachedCredential(*tr[k]) for k in range(min(n_triples, 1023))]), 3)
    nodes = {"client": m.NodeInfo(services=[], value=0, properties=["CLIENT"], agent_installed=True, reimagable=False,
                                  firewall=_allow_all(m, ports), vulnerabilities=vul)}
    by = {}
    for n, p, c in tr:
        by.setdefault(n, {}).setdefault(p, []).append(c)
    for i, n in enumerate(names):
        scan = {"Scan": _vuln(m, REMOTE, m.LeakedNodesId(list(names[:2])), 1)} if i == 0 else {}
        nodes[n] = m.NodeInfo(services=[m.ListeningService(p, allowedCredentials=cs) for p, cs in by.get(n, {}).items()], value=10 * i + 5,
                              properties=["SRV"], firewall=_allow_all(m, ports), vulnerabilities=scan)
    ids = m.Identifiers(properties=["CLIENT", "SRV"], ports=ports, local_vulnerabilities=["Find"] + seqs + leaks + (["LeakAll"] if leak_all else []),
                        remote_vulnerabilities=["Scan"])
    return m.Environment(network=m.create_network(nodes), vulnerability_library={}, identifiers=ids)
