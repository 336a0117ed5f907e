"""``po_layout_superbubbles_all`` in plain Python: the superbubbles of a whole graph, the cyclic partitions included, by the
scheme the device runs (phasm_amd/csrc/cyclic.hip.h), one step after the other.

It is for machines without a GPU and for the tests.  It is no fallback: nothing here picks it on its own.

The scheme.  SPLITTING a node x keeps its out-edges on ``x_out`` (a source, the rank of x) and moves ALL its in-edges to a new
rank ``x_in`` (a sink).  A level finds the SCCs of the current flat graph and splits one root per non-singleton SCC -- its
lowest-ranked node with an in-edge from outside the SCC, else its lowest-ranked node with an out-edge to outside, else (a
ROOTLESS SCC: a whole weak component) the root this run was given -- until a level finds singletons only.  The flat graph
is then acyclic but for self-loops, and the stage of section 3.9j runs on it: longest-path levels, the two dominator trees,
the pairs t = ipdom(s) with idom(t) = s, the enclosing bubbles, the discards, the labels.  A pair whose two ends are the two
copies of one node and a pair (s, t) with an edge t -> s seed the discards next to the self-loops.  A rootless SCC is run
with its lowest rank first and, unless that root is CERTIFIED (alone it leaves no cycle in its SCC), with the nodes of one
shortest cycle through it in turn, up to the first certified one; the runs are merged."""
from typing import List

import numpy as np

NONE = -1
SB_ENTRANCE, SB_EXIT, SB_NESTED, SB_SELF_LOOP = 1, 2, 4, 8
STAT_KEYS = ("n_nodes", "n_edges", "n_bubbles", "n_nested", "n_cyclic_bubbles", "n_split", "n_split_levels", "n_rootless", "n_root_runs",
             "n_certified", "n_edge_filtered")


def _sccs(n: int, succ: List[List[int]]) -> List[int]:
    """low[r] = the lowest rank of r's SCC (Tarjan, iterative)."""
    index, link, on, stack, low, counter = [-1] * n, [0] * n, [False] * n, [], [-1] * n, 0
    for s in range(n):
        if index[s] >= 0:
            continue
        work = [(s, 0)]
        while work:
            v, k = work.pop()
            if k == 0:
                index[v] = link[v] = counter
                counter += 1
                stack.append(v)
                on[v] = True
            if k < len(succ[v]):
                w = succ[v][k]
                work.append((v, k + 1))
                if index[w] < 0:
                    work.append((w, 0))
                elif on[w]:
                    link[v] = min(link[v], index[w])
                continue
            if link[v] == index[v]:
                members = []
                while True:
                    w = stack.pop()
                    on[w] = False
                    members.append(w)
                    if w == v:
                        break
                m = min(members)
                for w in members:
                    low[w] = m
            if work:
                u = work[-1][0]
                link[u] = min(link[u], link[v])
    return low


def _levels(n: int, eu: List[int], ev: List[int]) -> List[int]:
    """Longest-path levels of a DAG: 1 where no edge enters."""
    indeg, succ = [0] * n, [[] for _ in range(n)]
    for a, b in zip(eu, ev):
        indeg[b] += 1
        succ[a].append(b)
    lvl, todo = [1] * n, [r for r in range(n) if indeg[r] == 0]
    for v in todo:
        for c in succ[v]:
            lvl[c] = max(lvl[c], lvl[v] + 1)
            indeg[c] -= 1
            if indeg[c] == 0:
                todo.append(c)
    if len(todo) != n:
        raise RuntimeError("internal: the flat graph of po_layout_superbubbles_all is not acyclic")
    return lvl


def _tree(n: int, lvl: List[int], towards_root: List[List[int]]):
    """Immediate dominators under the virtual root ``n``, level by level; a rank without a neighbour on the root's side
    hangs on the root."""
    idom, depth = [NONE] * n + [n], [0] * (n + 1)
    for v in sorted(range(n), key=lambda r: lvl[r]):
        d = NONE if towards_root[v] else n
        for p in towards_root[v]:
            if d == NONE:
                d = p
                continue
            a, b = d, p
            while a != b:
                if depth[a] >= depth[b]:
                    a = idom[a]
                else:
                    b = idom[b]
            d = a
        idom[v], depth[v] = d, depth[d] + 1
    return idom


class HostSuperbubblesAll:
    """``edges``: rows that start with (u, v); ``node_order``: the graph's nodes in node order.  ``layout_superbubbles_all``
    returns what ``ExactOverlapper.layout_superbubbles_all`` returns; ``superbubble_all_stats()`` the integer stats of
    ``po_get_superbubble_all_stats`` (no batches, no times)."""

    def __init__(self, edges, node_order):
        self.order = [int(x) for x in node_order]
        rank = {x: r for r, x in enumerate(self.order)}
        if len(rank) != len(self.order):
            raise ValueError("po_layout_superbubbles_all: the node order repeats a node")
        try:
            self.eu = [rank[int(e[0])] for e in edges]
            self.ev = [rank[int(e[1])] for e in edges]
        except KeyError:
            raise ValueError("po_layout_superbubbles_all: an edge has an end that is not in the node order")
        self.stats = {}
        self.roots_of_runs = []          # per run: {lowest rank of a rootless SCC: the root it was given}
        self.situations = {}             # what the runs met (the golden's generator asserts that each occurs)

    def node_order(self) -> np.ndarray:
        return np.asarray(self.order, dtype=np.uint32)

    # ---- one run: the levelled loop, the stage of section 3.9j on the flat graph, the back-mapping ----------------------

    def _run(self, root_of: dict, scc0: List[int]):
        n0, eu, ev = len(self.order), self.eu, self.ev
        split, levels, uncertain = [], 0, set()
        while True:
            if levels > n0 + 1:
                raise RuntimeError("internal: po_layout_superbubbles_all reached its bound of n_order + 2 split levels")
            copy_of = {x: n0 + i for i, x in enumerate(sorted(split))}
            nf = n0 + len(split)
            fv = [copy_of.get(b, b) for b in ev]
            succ = [[] for _ in range(nf)]
            for a, b in zip(eu, fv):
                succ[a].append(b)
            low = _sccs(nf, succ)
            size = {}
            for r in range(nf):
                size[low[r]] = size.get(low[r], 0) + 1
            if levels == 1:
                uncertain = {scc0[r] for r in range(n0) if size[low[r]] > 1}
            r_in, re_out = {}, {}
            for a, b in zip(eu, fv):
                if low[a] != low[b]:
                    if size[low[b]] > 1:
                        r_in[low[b]] = min(r_in.get(low[b], b), b)
                    if size[low[a]] > 1:
                        re_out[low[a]] = min(re_out.get(low[a], a), a)
            chosen = []
            for c, k in size.items():
                if k > 1:
                    x = r_in.get(c, re_out.get(c, root_of.get(c, c) if levels == 0 else c))
                    chosen.append(x)
            if not chosen:
                break
            split.extend(chosen)
            levels += 1
        orig = list(range(n0)) + sorted(split)
        # the stage of section 3.9j on the flat graph: every rank is real, a self-loop only marks its rank
        loop = [False] * nf
        parents, children, du, dv = [[] for _ in range(nf)], [[] for _ in range(nf)], [], []
        for a, b in zip(eu, fv):
            if a == b:
                loop[a] = True
                continue
            parents[b].append(a)
            children[a].append(b)
            du.append(a)
            dv.append(b)
        lvl_f, lvl_b = _levels(nf, du, dv), _levels(nf, dv, du)
        idom, ipdom = _tree(nf, lvl_f, parents), _tree(nf, lvl_b, children)
        exit_of = {s: ipdom[s] for s in range(nf) if ipdom[s] != nf and idom[ipdom[s]] == s}
        encl = [NONE] * (nf + 1)
        for v in sorted(range(nf), key=lambda r: lvl_f[r]):
            d = idom[v]
            if d != nf:
                encl[v] = d if d in exit_of and exit_of[d] != v else encl[d]
        dead, filtered = set(), set()
        for s, t in exit_of.items():                      # the two copies of one node
            if orig[s] == orig[t]:
                dead.add(s)
        for a, b in zip(eu, ev):                          # (s, t) with an edge t -> s
            if b in exit_of and orig[exit_of[b]] == a and a != b:
                filtered.add(b)
        dead |= filtered
        for v in range(nf):
            if loop[v]:
                if v in exit_of:
                    dead.add(v)
                if idom[v] != nf and exit_of.get(idom[v]) == v:
                    dead.add(idom[v])
                if encl[v] != NONE:
                    dead.add(encl[v])
        while True:
            more = {encl[s] for s in dead if encl[s] != NONE} - dead
            if not more:
                break
            dead |= more
        pairs = {s: orig[t] for s, t in exit_of.items() if s not in dead}
        was_split = set(split)
        self.situations["split_entrance"] += sum(1 for s in pairs if s in was_split)
        self.situations["split_exit"] += sum(1 for s in pairs if exit_of[s] >= n0)
        inside_of = {v: encl[v] for v in range(n0) if encl[v] != NONE and encl[v] not in dead}
        total = {s: 0 for s in pairs}
        for v, s in inside_of.items():
            total[s] += 1
        for s in sorted(pairs, key=lambda r: -lvl_f[r]):
            if s in inside_of:
                total[inside_of[s]] += total[s]
        return pairs, inside_of, total, filtered, len(split), levels, uncertain

    def _shortest_cycles(self, roots):
        """Per root x: the nodes behind x on one shortest cycle through it, forward -- breadth-first distances from x, the
        lowest-ranked parent one step nearer, walked back from the lowest-ranked last node."""
        n0 = len(self.order)
        is_root = set(roots)
        dist, din = [NONE] * n0, {}
        for x in roots:
            dist[x] = 0
        frontier, d = list(roots), 0
        while frontier:
            d += 1
            nxt = []
            for u in frontier:
                for k in self._succ[u]:
                    if k in is_root:
                        din.setdefault(k, d)
                    elif dist[k] == NONE:
                        dist[k] = d
                        nxt.append(k)
            frontier = nxt
        par, pin = [NONE] * n0, {}
        for a, b in zip(self.eu, self.ev):
            if dist[a] == NONE:
                continue
            if b in is_root:
                if din[b] == dist[a] + 1:
                    pin[b] = min(pin.get(b, a), a)
            elif dist[b] == dist[a] + 1:
                par[b] = a if par[b] == NONE else min(par[b], a)
        out = {}
        for x in roots:
            back, v = [], pin[x]
            for _ in range(din[x] - 1):
                back.append(v)
                v = par[v]
            if v != x:
                raise RuntimeError("internal: the cycle walk of po_layout_superbubbles_all does not close")
            out[x] = back[::-1]
        return out

    def layout_superbubbles_all(self, graph=None, n_nodes=None):
        n0, eu, ev = len(self.order), self.eu, self.ev
        succ = [[] for _ in range(n0)]
        for a, b in zip(eu, ev):
            succ[a].append(b)
        self._succ = succ
        scc0 = _sccs(n0, succ)
        size = {}
        for r in range(n0):
            size[scc0[r]] = size.get(scc0[r], 0) + 1
        rooted = set()
        for a, b in zip(eu, ev):
            if scc0[a] != scc0[b]:
                rooted.add(scc0[a])
                rooted.add(scc0[b])
        rootless = sorted(c for c, k in size.items() if k > 1 and c not in rooted)
        m_exit, m_inside, m_size, m_total, m_filtered = {}, {}, {}, {}, set()
        n_split = n_levels = n_runs = 0
        root_of, cycles, done, certified = {}, None, set(), set()
        self.roots_of_runs = []
        self.situations = {"split_entrance": 0, "split_exit": 0, "inside_from_a_later_run": 0}
        while n0:                         # (an empty order: nothing runs)
            n_runs += 1
            self.roots_of_runs.append({c: root_of.get(c, c) for c in rootless})
            pairs, inside_of, total, filtered, k_split, k_levels, uncertain = self._run(root_of, scc0)
            n_split, n_levels = max(n_split, k_split), max(n_levels, k_levels)
            m_filtered |= filtered
            for s, t in pairs.items():
                m_exit[s], m_total[s] = t, total[s]
            for v, s in inside_of.items():
                if v not in m_size or total[s] < m_size[v]:
                    self.situations["inside_from_a_later_run"] += n_runs > 1
                    m_inside[v], m_size[v] = s, total[s]
            for c in rootless:
                if c not in done and c not in uncertain:
                    done.add(c)
                    certified.add(c)
            todo = [c for c in rootless if c not in done]
            if todo and cycles is None:
                cycles = self._shortest_cycles(todo)
            for c in todo:
                if n_runs > len(cycles[c]):       # the end of the cycle
                    done.add(c)
                else:
                    root_of[c] = cycles[c][n_runs - 1]
            if all(c in done for c in rootless):
                break
        order = self.order
        node_exit, node_inside = np.full(n0, 0xFFFFFFFF, np.uint32), np.full(n0, 0xFFFFFFFF, np.uint32)
        flags = np.zeros(n0, np.uint8)
        for a, b in zip(eu, ev):
            if a == b:
                flags[a] |= SB_SELF_LOOP
        for s, t in m_exit.items():
            node_exit[s] = order[t]
            flags[s] |= SB_ENTRANCE | (SB_NESTED if s in m_inside else 0)
            flags[t] |= SB_EXIT
        for v, s in m_inside.items():
            node_inside[v] = order[s]
        ent = sorted(m_exit)
        table = np.zeros(len(ent), dtype=[("entrance", "<u4"), ("exit", "<u4"), ("n_inside", "<u4"), ("nested", "<u4")])
        for i, s in enumerate(ent):
            table[i] = (order[s], order[m_exit[s]], m_total[s], int(s in m_inside))
        self.stats = {"n_nodes": n0, "n_edges": len(eu), "n_bubbles": len(ent), "n_nested": sum(1 for s in ent if s in m_inside),
                      "n_cyclic_bubbles": sum(1 for s in ent if size[scc0[s]] > 1), "n_split": n_split, "n_split_levels": n_levels,
                      "n_rootless": len(rootless), "n_root_runs": n_runs, "n_certified": len(certified),
                      "n_edge_filtered": len(m_filtered)}
        return node_exit, node_inside, flags, table

    def superbubble_all_stats(self) -> dict:
        return dict(self.stats)

    # ---- the bubble chains behind these superbubbles, ring chains included ----------------------

    def layout_bubblechains_all(self, graph=None, min_nodes: int = 1, n_nodes=None):
        """``po_layout_bubblechains_all`` by the device's scheme (bubblechains.hip.h with ringchains.hip.h between the heads
        and the ranking), on ranks: the top-level entrances, their links, the heads; one leader per RING of links -- the
        doubling election, run synchronously for exactly ceil(log2(n_top)) + 1 rounds; the ranking from every head and
        leader; head and position of every rank; the sums, the ``min_nodes`` filter, the numbering by head rank.  Returns
        what ``ExactOverlapper.layout_bubblechains_all`` returns; ``bubblechain_all_stats()`` the integer stats."""
        if not 1 <= int(min_nodes) <= 0xFFFFFFFF:
            raise ValueError("po_layout_bubblechains_all: bad parameters")
        node_exit, node_inside, flags, sb_table = self.layout_superbubbles_all()
        sb = dict(self.stats)
        n0, eu, ev, order = len(self.order), self.eu, self.ev, self.order
        rank = {x: r for r, x in enumerate(order)}
        none = 0xFFFFFFFF
        exit_of = [rank[int(t)] if int(t) != none else NONE for t in node_exit]
        inside = [rank[int(s)] if int(s) != none else NONE for s in node_inside]
        top = [exit_of[r] != NONE and inside[r] == NONE for r in range(n0)]
        nxt, pred = [NONE] * n0, [NONE] * n0
        for r in range(n0):
            if top[r]:
                pred[exit_of[r]] = r
                if top[exit_of[r]]:
                    nxt[r] = exit_of[r]
        head = [top[r] and pred[r] == NONE for r in range(n0)]
        n_top, n_path_heads = sum(top), sum(head)
        # the election: ptr = pred of a linked top-level entrance, else the rank itself; mn = the rank
        ring, rounds = [False] * n0, 0
        if n_top and sb["n_cyclic_bubbles"]:
            ptr = [pred[r] if top[r] and pred[r] != NONE else r for r in range(n0)]
            mn = list(range(n0))
            rounds = max(n_top - 1, 0).bit_length() + 1
            for _ in range(rounds):
                mn = [min(mn[r], mn[ptr[r]]) for r in range(n0)]
                ptr = [ptr[ptr[r]] for r in range(n0)]
            for r in range(n0):
                if mn[r] == r and top[r] and not head[r] and not head[ptr[r]]:
                    ring[r] = True
            for r in range(n0):
                head[r] = head[r] or ring[r]
        n_heads = sum(head)
        if n_heads != n_path_heads + sum(ring) or (n_top and not n_heads):
            raise RuntimeError("internal: the heads and ring leaders of po_layout_bubblechains_all do not add up")
        # the ranking: every top-level entrance reaches its head along pred (a leader's link in is cut)
        home, pos, last = [NONE] * n0, [NONE] * n0, {}
        for hd in range(n0):
            if not head[hd]:
                continue
            s, k = hd, 0
            while True:
                if k > n_top:
                    raise RuntimeError("internal: the ranking of po_layout_bubblechains_all reached its bound")
                home[s], pos[s] = hd, k
                t = nxt[s]
                if t == NONE or t == hd:
                    last[hd] = exit_of[s]
                    break
                s, k = t, k + 1
        if any(top[r] and home[r] == NONE for r in range(n0)):
            raise RuntimeError("internal: a node of po_layout_bubblechains_all reached no head")
        nhead, npos = [NONE] * n0, [NONE] * n0
        cb, cn, ce = [0] * n0, [0] * n0, [0] * n0
        for r in range(n0):
            if top[r]:
                s = r
            elif pred[r] != NONE:                     # a last exit: the bubble it exits
                s = pred[r]
            else:
                s = inside[r]
                while s != NONE and inside[s] != NONE:   # the outermost holder
                    s = inside[s]
            if s == NONE:
                continue
            if not top[s] or home[s] == NONE:
                raise RuntimeError("internal: a node of po_layout_bubblechains_all reached no head")
            nhead[r], npos[r] = home[s], pos[s]
            cn[home[s]] += 1
            cb[home[s]] += top[r]
        for a, b in zip(eu, ev):
            if nhead[a] != NONE and nhead[a] == nhead[b]:
                ce[nhead[a]] += 1
        kept = [r for r in range(n0) if head[r] and cn[r] >= min_nodes]
        number = {r: i for i, r in enumerate(kept)}
        node_chain, node_bubble = np.full(n0, none, np.uint32), np.full(n0, none, np.uint32)
        for r in range(n0):
            if nhead[r] in number:
                node_chain[r], node_bubble[r] = number[nhead[r]], npos[r]
        edge_chain = np.full(len(eu), none, np.uint32)
        for e, (a, b) in enumerate(zip(eu, ev)):
            if node_chain[a] == node_chain[b]:
                edge_chain[e] = node_chain[a]
        table = np.zeros(len(kept), dtype=[("first_entrance", "<u4"), ("last_exit", "<u4"), ("n_bubbles", "<u4"), ("n_nodes", "<u4"),
                                           ("n_edges", "<u8")])
        for i, r in enumerate(kept):
            table[i] = (order[r], order[last[r]], cb[r], cn[r], ce[r])
        self.chain_stats = {"n_nodes": n0, "n_edges": len(eu), "n_bubbles": sb["n_bubbles"], "n_top": n_top, "n_chains": len(kept),
                            "n_short": n_heads - len(kept), "n_chain_nodes": sum(cn[r] for r in kept),
                            "n_chain_edges": sum(ce[r] for r in kept), "n_invalid": 0, "n_ring_chains": sum(ring),
                            "n_ring_bubbles": sum(cb[r] for r in range(n0) if ring[r]), "n_cyclic_bubbles": sb["n_cyclic_bubbles"],
                            "max_chain_bubbles": max([cb[r] for r in range(n0) if head[r]], default=0), "n_ring_rounds": rounds,
                            "n_root_runs": sb["n_root_runs"], "n_split_levels": sb["n_split_levels"]}
        return node_chain, node_bubble, edge_chain, table

    def bubblechain_all_stats(self) -> dict:
        return dict(self.chain_stats)
