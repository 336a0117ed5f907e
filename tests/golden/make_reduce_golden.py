#!/usr/bin/env python3
"""Generate tests/golden/reduce_cases.npz by EXECUTING the reference's own functions.

Runs only where the reference checkout is present (/root/reference); the output is committed.  Every case is GFA2
text that goes through what `phasm layout` does up to the symmetry pass (phasm/cli/assembler.py:56-159):

    reads, E lines -> LocalAlignment -> filters            (as tests/golden/make_layout_golden.py)
    phasm.assembly_graph.build_assembly_graph(la_iter)      -> the stage-1 edges WITH attributes
    removal of every filtered read in both orientations
    phasm.assembly_graph.remove_transitive_edges(g, fuzz)   -> flag 1
    g.remove_edges_from(...)
    phasm.assembly_graph.make_symmetric(g)                  -> flag 2

The installed networkx (3.x) cannot run the reference's AssemblyGraph (1.x calls: ``add_edge(u, v, attr_dict)``,
assignment to ``g.adj[v]``, ``edges_iter``), so the module's ``AssemblyGraph`` name is pointed at ``StandInGraph``
below -- ordered dicts of ordered dicts with a predecessor map, offering just the calls those functions make.  The
functions themselves are imported and run, not restated.

Per-branch totals: the reference logs every elimination at DEBUG level; a handler counts the records by the source
line that wrote them (step 2, step 3 "smallest", step 3 "< fuzz"), for neighbours of the node in work.  What it does not log (skipped w, tied weights) is
counted by tests/reduce_utils.py, whose three logged totals must equal the reference's here.

After the first 73 cases come the ones that vary the out-degree (dense lines, hubs of exact degrees, staggered hubs), and
for a few cases a SECOND PASS: the same three calls run again on the graph the first run left ("second_pass" in the
file, beside the cases, as is every case's largest out-degree: the records of the first cases stay as they were)."""
import io
import json
import logging
import os
import sys
from collections import OrderedDict

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))            # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

import phasm.assembly_graph as ag  # noqa: E402  (reference)
from phasm.filter import ContainedReads, MaxOverhang, MinOverlapLength, MinReadLength  # noqa: E402  (reference)
from phasm.io import gfa  # noqa: E402  (reference)

import reduce_utils as ru  # noqa: E402


class StandInGraph:
    """The networkx 1.x surface the reference's graph functions use, on insertion-ordered dicts."""

    def __init__(self, data=None, **attr):
        self.graph = dict(attr)
        self.adj = OrderedDict()
        self.pred = {}
        self.sequence_src = None

    edge_len = property(lambda self: self.graph.get("edge_len", "weight"))
    overlap_len = property(lambda self: self.graph.get("overlap_len", "overlap_len"))

    def _node(self, n):
        if n not in self.adj:
            self.adj[n] = OrderedDict()
            self.pred[n] = {}

    def add_edge(self, u, v, attr_dict=None, **attr):
        self._node(u)
        self._node(v)
        data = self.adj[u].get(v)
        if data is None:                       # a known edge keeps its place; its attributes are updated
            data = self.adj[u][v] = {}
            self.pred[v][u] = data
        data.update(attr_dict or {})
        data.update(attr)

    def __iter__(self):
        return iter(self.adj)

    def __getitem__(self, n):
        return self.adj[n]

    def __contains__(self, n):
        return n in self.adj

    def __len__(self):
        return len(self.adj)

    def out_degree(self, n):
        return len(self.adj[n])

    def degree(self, n):
        return len(self.adj[n]) + len(self.pred[n])

    def number_of_nodes(self):
        return len(self.adj)

    def number_of_edges(self):
        return sum(len(nb) for nb in self.adj.values())

    def sort_adjacency_lists(self, reverse=False, weight="weight"):
        for n in self.adj:
            self.adj[n] = OrderedDict(sorted(self.adj[n].items(), key=lambda kv: kv[1][weight], reverse=reverse))

    def edges_iter(self, data=False):
        for u, nb in self.adj.items():
            for v, d in nb.items():
                yield (u, v, d) if data else (u, v)

    def has_edge(self, u, v):
        return u in self.adj and v in self.adj[u]

    def remove_edges_from(self, ebunch):
        for e in ebunch:
            u, v = e[0], e[1]
            if self.has_edge(u, v):
                del self.adj[u][v]
                del self.pred[v][u]

    def remove_node(self, n):
        for v in list(self.adj[n]):
            del self.pred[v][n]
        for u in list(self.pred[n]):
            del self.adj[u][n]
        del self.adj[n]
        del self.pred[n]


ag.AssemblyGraph = StandInGraph
KEPT_MAX = 3000
FULL_STAGE1_MAX = 400   # larger cases keep a digest of their stage-1 edges (the file stays below 1 MiB)
STEP_LINES = {240: "step2_eliminations", 250: "step3_first", 254: "step3_fuzz"}   # logger.debug calls of remove_transitive_edges


# the read sets that vary the out-degree: (reads, fuzz values, branches counted from the reference's log, second pass)
# (a second pass = (fuzz of the first, fuzz of the second); with a larger second fuzz it finds something to remove)
DENSE = [(260, [0, 150, 1000], True, [(150, 150), (0, 1000)]), (450, [0, 150, 1000], True, []), (600, [150, 0], False, [])]
HUB_DEGREES = [63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2049]

NODE_LINE = 218   # "Processing node %s ...": names the node v the records after it belong to


class BranchCounter(logging.Handler):
    """Counts the eliminations of NEIGHBOURS of the node in work.  (The reference's node_state map is shared between
    nodes, so it also "eliminates" -- and logs -- nodes that are no neighbours of v and whose state nobody reads.)"""

    def __init__(self, g):
        super().__init__(logging.DEBUG)
        self.g = g
        self.v = None
        self.counts = {v: 0 for v in STEP_LINES.values()}

    def emit(self, record):
        if record.funcName != "remove_transitive_edges":
            return
        if record.lineno == NODE_LINE:
            self.v = record.args[0]
        elif record.lineno in STEP_LINES and record.args[0] in self.g[self.v]:
            self.counts[STEP_LINES[record.lineno]] += 1


def stage1_graph(text, params):
    reads = gfa.gfa2_parse_segments(io.StringIO(text))
    node_index = {}
    for i, name in enumerate(reads):                       # dict order = S line order (names are distinct here)
        node_index[name + "+"] = 2 * i
        node_index[name + "-"] = 2 * i + 1
    filters = [ContainedReads()]
    if params["min_read_length"]:
        filters.append(MinReadLength(params["min_read_length"]))
    if params["min_overlap_length"]:
        filters.append(MinOverlapLength(params["min_overlap_length"]))
    filters.append(MaxOverhang(params["max_overhang_abs"], params["max_overhang_rel"]))
    la_iter = map(gfa.gfa2_line_to_la(reads), (l for l in io.StringIO(text) if l.startswith("E")))
    g = ag.build_assembly_graph(filter(lambda la: all(f(la) for f in filters), la_iter))
    for f in filters:                                      # every filtered read leaves in both orientations
        for read in f.nodes_to_remove:
            for strand in "+-":
                node = read.with_orientation(strand)
                if node in g:
                    g.remove_node(node)
    return g, node_index


def edge_list(g, node_index):
    return [[node_index[str(u)], node_index[str(v)], int(d[g.edge_len]), int(d[g.overlap_len])] for u, v, d in g.edges_iter(data=True)]


def run_case(name, text, params, fuzzes, full_stage1, source, totals, count_branches, second_pass=(), second=None, max_deg=None):
    log = logging.getLogger("phasm.assembly_graph")
    out = dict(source, name=name, params=params)
    results = {}
    flag_sets = []
    for fuzz in fuzzes:
        g, node_index = stage1_graph(text, params)         # (a fresh graph per fuzz: the functions change it)
        stage1 = edge_list(g, node_index)                  # insertion order, before the adjacency lists are sorted
        counter = BranchCounter(g)
        if count_branches:
            log.addHandler(counter)
            log.setLevel(logging.DEBUG)
        transitive = ag.remove_transitive_edges(g, fuzz)
        log.removeHandler(counter)
        log.setLevel(logging.WARNING)
        g.remove_edges_from(transitive)
        before = {(node_index[str(u)], node_index[str(v)]) for u, v in g.edges_iter()}
        n_asym = ag.make_symmetric(g)
        kept = {(node_index[str(u)], node_index[str(v)]) for u, v in g.edges_iter()}
        tset = {(node_index[str(u)], node_index[str(v)]) for u, v in transitive}
        assert len(tset) == len(transitive) and n_asym == len(before) - len(kept)
        s1 = np.asarray(stage1, dtype=np.int64).reshape(-1, 4)
        flags = np.array([1 if (u, v) in tset else (0 if (u, v) in kept else 2) for u, v in s1[:, :2].tolist()], dtype=np.uint8)
        order = np.lexsort((s1[:, 1], s1[:, 0])) if len(s1) else np.empty(0, dtype=np.int64)
        results[str(fuzz)] = {"n_transitive": len(tset), "n_asymmetric": int(n_asym), "n_kept": len(kept),
                              "flags_by_uv": ru.pack_flags(flags[order]),
                              "kept_sha256": ru.edge_digest(ru.sort_edges(s1[flags == 0]))}
        if len(kept) <= KEPT_MAX:
            results[str(fuzz)]["kept"] = ru.sort_edges(s1[flags == 0]).tolist()
        flag_sets.append(flags.tobytes())
        # the restatement on the same edges: equal flags, and equal totals for the branches the reference logs
        counts = ru.new_counts()
        mine = ru.reduce_edges(s1, fuzz, counts=counts)
        assert np.array_equal(mine, flags), (name, fuzz)
        if count_branches:
            for k, v in counter.counts.items():
                assert counts[k] == v, (name, fuzz, k, counts[k], v)
            for k, v in counts.items():
                totals[k] += v
        for fuzz2 in [f2 for f1, f2 in second_pass if f1 == fuzz]:
            # the same three calls once more (length fuzz ``fuzz2``) on the graph they left, whose adjacency lists stand
            # in the first pass's sorted order; flags per kept edge of the first pass, by (u, v)
            if g is None:
                g, _ = stage1_graph(text, params)
                g.remove_edges_from(ag.remove_transitive_edges(g, fuzz))
                ag.make_symmetric(g)
            transitive2 = ag.remove_transitive_edges(g, fuzz2)
            g.remove_edges_from(transitive2)
            n_asym2 = ag.make_symmetric(g)
            kept2 = {(node_index[str(u)], node_index[str(v)]) for u, v in g.edges_iter()}
            tset2 = {(node_index[str(u)], node_index[str(v)]) for u, v in transitive2}
            g = None
            k1 = ru.sort_edges(s1[flags == 0])
            flags2 = np.array([1 if (u, v) in tset2 else (0 if (u, v) in kept2 else 2) for u, v in k1[:, :2].tolist()], dtype=np.uint8)
            assert tset2 <= kept and kept2 <= kept and n_asym2 == int((flags2 == 2).sum())
            second.append({"case": name, "fuzz": fuzz, "fuzz2": fuzz2, "n_in": len(k1), "n_transitive": len(tset2),
                           "n_asymmetric": int(n_asym2), "n_kept": len(kept2), "flags_by_uv": ru.pack_flags(flags2),
                           "kept_sha256": ru.edge_digest(k1[flags2 == 0])})
            # the restatement: the kept edges with the rank they had in the first pass
            keep_idx = np.flatnonzero(flags == 0)
            mine2 = ru.reduce_edges(s1[keep_idx], fuzz2, rank=keep_idx)
            assert np.array_equal(mine2[np.lexsort((s1[keep_idx, 1], s1[keep_idx, 0]))], flags2), (name, fuzz, fuzz2)
            print("%-28s second pass F%d -> F%d: %d/%d/%d" % (name, fuzz, fuzz2, len(tset2), n_asym2, len(kept2)))
    if len(set(flag_sets)) > 1:
        totals["fuzz_sensitive_cases"] += 1
    totals["edges_weight_le0"] += int((s1[:, 2] <= 0).sum()) if len(s1) else 0
    out["n_stage1"] = len(s1)
    if max_deg is not None:
        max_deg[name] = int(np.bincount(s1[:, 0]).max()) if len(s1) else 0
    if full_stage1 and len(s1) <= FULL_STAGE1_MAX:
        out["stage1"] = s1.tolist()
    else:
        out["stage1_sha256"] = ru.edge_digest(ru.sort_edges(s1))
    out["results"] = results
    print("%-28s stage-1 %7d  " % (name, len(s1)) +
          "  ".join("F%s: %d/%d/%d" % (f, r["n_transitive"], r["n_asymmetric"], r["n_kept"]) for f, r in results.items()))
    return out


def main():
    import layout_utils as lu
    totals = dict(ru.new_counts(), fuzz_sensitive_cases=0, edges_weight_le0=0)
    cases, max_deg = [], {}
    default = ru.DEFAULT_PARAMS
    for lad, seed, fuzzes in [("ladder_small", None, [1000, 10]), ("ladder_varlen", None, [1000, 10]),
                              ("ladder_varlen", 7, [1000]), ("ladder_cfg1_mini", None, [1000, 10]),
                              ("ladder_cfg2_mini", None, [1000, 10]), ("cfg2_1k", None, [1000, 10])]:
        src = {"ladder": lad, "shuffle_seed": seed}
        name = lad + ("" if seed is None else "_shuffled%d" % seed)
        cases.append(run_case(name, ru.case_text(src), default, fuzzes, False, src, totals, False, max_deg=max_deg))
    for c in lu.load_cases():
        if c["digests"]:
            continue
        cases.append(run_case("layout_" + c["name"], c["text"], c["params"], [1000, 10, 0], True, {"layout_case": c["name"]}, totals, True, max_deg=max_deg))
    big_fuzz = 10 ** 6
    for seed in range(12):
        src = {"synth": {"kind": "line", "seed": 100 + seed, "n": 24 + 4 * seed}}
        src["text_sha256"] = ru.text_digest(ru.case_text(src))
        cases.append(run_case("line_%d" % (100 + seed), ru.case_text(src), default, [0, 150, 1000, big_fuzz], True, src, totals, True, max_deg=max_deg))
    src = {"synth": {"kind": "hub", "seed": 5}}
    src["text_sha256"] = ru.text_digest(ru.case_text(src))
    cases.append(run_case("hub_5200", ru.case_text(src), default, [1000, 0], True, src, totals, False, max_deg=max_deg))
    # (everything above is as the file first had it; what follows varies the out-degree: DESIGN.md section 3.9b)
    second = []

    def synth(name, kw, fuzzes, counted, second_pass=()):
        src = {"synth": kw, "counted": counted}
        src["text_sha256"] = ru.text_digest(ru.case_text(src))
        cases.append(run_case(name, ru.case_text(src), default, fuzzes, True, src, totals, counted, second_pass, second, max_deg))

    for n, fuzzes, counted, twice in DENSE:
        synth("dense_%d" % n, {"kind": "line", "seed": 300 + n, "n": n, "span": 1200, "n_false": n // 9}, fuzzes, counted, twice)
    for deg in HUB_DEGREES:
        synth("hub_%d" % deg, {"kind": "hub", "seed": deg, "n_nb": deg, "n_cross": 200}, [0, 1000], True, [(0, 0), (0, 1000)] if deg == 1025 else [])
    synth("stagger_1100", {"kind": "stagger", "seed": 11}, [0, 150, 1000], True, [(0, 0), (150, 150), (0, 1000)])
    # tied weights whose order -- the rank the first pass hands on -- decides the second pass (reduce_utils.tie_case)
    synth("tie_8", {"kind": "tie", "seed": 2}, [0, 150], True, [(0, 150), (0, 0), (150, 150)])
    for name in ("line_105", "line_108"):       # a second pass of two of the first cases, recorded beside them
        c = next(x for x in cases if x["name"] == name)
        scrap = dict(ru.new_counts(), fuzz_sensitive_cases=0, edges_weight_le0=0)
        again = run_case(name, ru.case_text(c), default, [0, 150], True, {}, scrap, False, [(150, 150), (0, 150), (0, 1000)], second)
        assert all(again["results"][f] == c["results"][f] for f in ("0", "150"))
    path = ru.GOLDEN_FILE
    ru.save_golden({"branch_totals": totals, "cases": cases, "second_pass": second, "max_out_degree": max_deg}, path)
    print("totals", totals)
    print("wrote", path, len(cases), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
