"""The contract of po_layout_bubblechains_all (include/phasm_overlap.h) as plain Python, the scheme the
kernels use run synchronously, the direct cases and the loader of tests/golden/bubblechain_all_cases.npz.

``definition`` restates the reference's sequential walk (build_bubblechains, phasm/assembly_graph.py:594-652) on the arrays of
``cyclic_utils.scheme_all`` and makes it RING-AWARE: the first two tiers of starts walk the path chains as the reference
does; what is left unvisited lies on rings of links, and each ring is walked ONCE ROUND from its lowest-ranked entrance (the
reference starts its third tier at an arbitrary entrance and stops one bubble short).  ``scheme`` reaches the same the way the
device does (phasm_amd.cyclic.HostSuperbubblesAll.layout_bubblechains_all: bubblechains.hip.h with the election of
ringchains.hip.h)."""
import os

import numpy as np

import bubblechain_utils as bu
import components_utils as cu
import cyclic_utils as cy
import partition_utils as pu
import reduce_utils as ru
import superbubble_utils as su
from phasm_amd import cyclic

GOLDEN_FILE = os.path.join(ru.GOLDEN, "bubblechain_all_cases.npz")
DIGEST_ABOVE = bu.DIGEST_ABOVE
CONTIG_DIGEST_ABOVE = 400        # edges: above, a contig record of this golden holds a digest of its arrays
NONE = bu.NONE
ARRAY_KEYS = bu.ARRAY_KEYS
STAT_KEYS = bu.STAT_KEYS + ("n_ring_chains", "n_ring_bubbles", "n_cyclic_bubbles")
SCHEME_KEYS = ("n_ring_rounds", "n_root_runs", "n_split_levels")


def ring_rounds(n_top):
    """Rounds of the election: ceil(log2(n_top)) + 1."""
    return bu.log2_ceil(n_top) + 1


# ---- the reference's walk, ring-aware -----------------------------------------------------------------------------------------

def definition(edges, order, min_nodes=1, sb=None):
    """edges: rows that start with (u, v); order: the graph's nodes in node order; sb: ``cyclic_utils.scheme_all`` of them.
    The shape of ``bubblechain_utils.definition``; ``stats`` gains the ring counts."""
    if sb is None:
        sb = cy.scheme_all(cu.uv_of(edges).tolist(), order)
    order, eu, ev, sb, rank = bu._inputs(edges, order, sb)
    top = [i for i, nested in enumerate(sb["b_nested"].tolist()) if not nested]
    bubbles = {rank[int(sb["b_entrance"][i])]: rank[int(sb["b_exit"][i])] for i in top}
    sets = su.node_sets(sb, order)
    nodes_of = {rank[int(sb["b_entrance"][i])]: [rank[x] for x in sets[i]] for i in top}
    entrances, exits = sorted(bubbles), set(bubbles.values())
    assert len(exits) == len(bubbles), "a node exits two top-level bubbles"
    visited, chains, rings = set(), [], []

    def walk(start, ring):
        head, pos, num_bubbles, last = start, {}, 0, NONE
        while start in bubbles and not (num_bubbles and ring and start == head):
            bubble_exit = bubbles[start]
            for x in nodes_of[start]:
                if x not in pos or x == start:       # (an exit that enters the next bubble lies at that one's position)
                    pos[x] = num_bubbles
            visited.update(nodes_of[start])
            start, last = bubble_exit, bubble_exit
            num_bubbles += 1
        chains.append((head, last, num_bubbles, pos))
        return num_bubbles

    for s in entrances:                          # the reference's first two tiers: an entrance that no top-level bubble exits
        if s not in exits:
            walk(s, False)
    for s in entrances:                          # ascending: the first unvisited entrance of a ring is its lowest
        if s not in visited:
            rings.append(walk(s, True))
            assert chains[-1][1] == s, "a ring does not close"
    assert all(s in visited for s in entrances)
    res = bu._result(order, eu, ev, sb, chains, min_nodes)
    res["stats"].update({"n_ring_chains": len(rings), "n_ring_bubbles": sum(rings), "n_cyclic_bubbles": sb["stats"]["n_cyclic_bubbles"]})
    return res


# ---- the device's scheme, run synchronously -------------------------------------------------------------------------------

def as_result(stats, out):
    """What HostSuperbubblesAll.layout_bubblechains_all / the device returns in the shape of ``definition``."""
    node_chain, node_bubble, edge_chain, table = out
    word = lambda a: np.where(np.asarray(a) == 0xFFFFFFFF, NONE, np.asarray(a).astype(np.int64))   # noqa: E731
    return {"node_chain": word(node_chain), "node_bubble": word(node_bubble), "edge_chain": word(edge_chain),
            "c_first": table["first_entrance"].astype(np.int64), "c_last": table["last_exit"].astype(np.int64),
            "c_bubbles": table["n_bubbles"].astype(np.int64), "c_nodes": table["n_nodes"].astype(np.int64),
            "c_edges": table["n_edges"].astype(np.int64), "stats": dict(stats)}


def scheme(edges, order, min_nodes=1):
    host = cyclic.HostSuperbubblesAll(cu.uv_of(edges).tolist() if len(edges) else [], order)
    out = host.layout_bubblechains_all(None, min_nodes)
    return as_result(host.bubblechain_all_stats(), out)


def is_ring(res, j):
    return int(res["c_first"][j]) == int(res["c_last"][j])


# ---- direct cases: edges (u, v), an explicit node order, min_nodes ----------------------------------------------------------

def ring_of_trivial(k, at=0):
    """A plain ring of k nodes: every edge is a trivial bubble."""
    ids = [at + 2 * i for i in range(k)]
    return ids, pu._ring(ids)


def direct_inputs():
    """(name, order, edges, n_ids or None, min_nodes): every direct case of cyclic_utils with min_nodes 1, then the shapes this
    stage is about.  Nodes are even ids."""
    D = cy._diamond
    cases = [(name, order, edges, n_ids, 1) for name, order, edges, n_ids in cy.direct_inputs()]
    new = []
    o, e = cy.ring_of_diamonds(2)
    new.append(("ring_of_2_diamonds", o, e, 1))                                  # 6 nodes: the smallest ring
    for k in (3, 4, 5, 8, 15, 16, 17):                                            # both sides of the powers of two
        o, e = cy.ring_of_diamonds(k)
        new.append(("ring_of_%d_bubbles_scrambled" % k, pu._scrambled(o, k), e, 1))
        o, e = ring_of_trivial(k)
        new.append(("plain_ring_of_%d_descending" % k, o[::-1], e, 1))
    o, e = cy.ring_of_diamonds(4)
    new.append(("ring_lowest_rank_is_an_interior_node", [o[4], o[7]] + [x for x in o if x not in (o[4], o[7])], e, 1))
    # a ring beside a path chain in one graph.  (Never in one weak component: every in-edge of a ring's entrance comes from the
    # bubble it exits and every out-edge goes into the bubble it enters, so the nodes of a ring chain are closed under edges.)
    ro, re_ = cy.ring_of_diamonds(3)
    path = D(100, 102, 104, 106) + D(106, 108, 110, 112)
    po = [100 + 2 * i for i in range(7)]
    new.append(("ring_beside_a_path_chain", po + ro, path + re_, 1))
    o1, e1 = cy.ring_of_diamonds(2)
    o2, e2 = cy.ring_of_diamonds(3, 100)
    new.append(("two_rings_joined_by_a_bridge", o2 + o1 + [50], e1 + [(0, 50), (50, 100)] + e2, 1))   # (the bridge opens both)
    nested = [(0, 2), (0, 10), (10, 12), (8, 12), (12, 14), (14, 0)] + D(2, 4, 6, 8)
    new.append(("ring_with_a_nested_bubble", [14, 12] + [x for x in range(0, 12, 2)], nested, 1))
    o, e = cy.ring_of_diamonds(2)
    new.append(("ring_dropped_by_min_nodes", o + po, e + path, 7))               # the ring has 6 nodes, the path chain 7
    new.append(("ring_kept_path_chain_dropped", po + ro, path + re_, 8))         # the ring has 9 nodes
    return cases + [("rc_" + name, order, edges, None, min_nodes) for name, order, edges, min_nodes in new]


# ---- golden file ---------------------------------------------------------------------------------------------------

def record_of(res, edges):
    """The golden record of one application: the stats and the arrays, or above DIGEST_ABOVE edges their digest."""
    rec = {k: int(res["stats"][k]) for k in STAT_KEYS}
    arrays = bu._canonical(res, edges)
    if rec["n_edges"] > DIGEST_ABOVE:
        rec["sha256"] = cu.digest(*arrays)
    else:
        for k, a in zip(ARRAY_KEYS, arrays):
            rec["a_" + k] = a.tolist()
    return rec


def check_against_record(res, rec, edges, keys=STAT_KEYS):
    """A ``definition``-shaped result (of any producer, on ``edges`` in its own order) against one golden record."""
    assert {k: int(res["stats"][k]) for k in keys} == {k: rec[k] for k in keys}
    arrays = bu._canonical(res, edges)
    if "sha256" in rec:
        assert cu.digest(*arrays) == rec["sha256"]
    else:
        for k, a in zip(ARRAY_KEYS, arrays):
            assert a.tolist() == list(rec["a_" + k]), k


def save_golden(obj):
    cu.save_golden(obj, GOLDEN_FILE)


_GOLDEN = []


def load_golden():
    if not _GOLDEN:
        _GOLDEN.append(cu.load_golden(GOLDEN_FILE))
    return _GOLDEN[0]
