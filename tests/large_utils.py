"""The cases of po_phase_large (include/phasm_overlap.h) and the loader of tests/golden/large_cases.npz.

A CASE is a dict: ``name``; the graph as ``order`` (node ids) and ``edges`` ([u, v, weight], in edge order); ``max_paths`` (what
``po_phase_paths`` lists up to); ``bubble`` (the index of the large bubble in the table); ``node_reads`` (``[node, [read ids]]``
pairs: a merged node has several, any other node one); ``ploidy`` (= n_best); the relevant reads as the arrays of
``phasing.RelevantReads`` (``b_reads`` global ids ascending, ``overlap_max``, ``aln_off``, ``aln_b`` local ids, ``aln_a0``,
``aln_a1``); and, from the generator, ``ref`` = ``{"scores": [...], "best": [...]}`` by the reference's ``phase_large_bubble``.
The one case with ``walk`` holds the inputs of a whole synthetic walk (tests/walk_utils.py ``synth``) instead of a graph of
its own: graph, node reads and relevant reads follow from it."""
import os

import numpy as np

import components_utils as cu
import paths_utils as pp
import phase_utils as pu
import reduce_utils as ru
import walk_product_utils as wp
import walk_utils as wu
from phasm_amd import phasing

GOLDEN_FILE = os.path.join(ru.GOLDEN, "large_cases.npz")
CHUNK = 256          # LG_CHUNK of phasm_amd/csrc/large.hip.h: interior slots of a path staged in LDS at a time
REL_KEYS = ("b_reads", "overlap_max", "aln_off", "aln_b", "aln_a0", "aln_a1")


# ---- graphs -------------------------------------------------------------------------------------------------------------------

class Builder:
    """Edges of a chain of bubbles over node ids handed out in order."""

    def __init__(self):
        self.edges, self.n = [], 0

    def node(self):
        self.n += 1
        return self.n - 1

    def diamond(self, s):
        a, b, t = self.node(), self.node(), self.node()
        self.edges += [(s, a), (s, b), (a, t), (b, t)]
        return t

    def large(self, s, k, arm=1, bypass=False, nested=False, lanes=1):
        """``lanes`` times s -> x0, k diamonds in series, xk -> t; an arm of ``arm`` nodes from s to t (0: none); ``bypass``: the
        edge s -> t (``"first"``: ahead of the arm); ``nested``: one arm of the first diamond is a diamond itself.
        lanes * (2^k or 3 * 2^(k-1)) + (arm > 0) + bypass paths."""
        ends = []
        for _ in range(lanes):
            x = self.node()
            self.edges.append((s, x))
            for i in range(k):
                if nested and i == 0:
                    a, a1, a2, a3, b, t = (self.node() for _ in range(6))
                    self.edges += [(x, a), (x, b), (a, a1), (a, a2), (a1, a3), (a2, a3), (a3, t), (b, t)]
                    x = t
                else:
                    x = self.diamond(x)
            ends.append(x)
        t = self.node()
        self.edges += [(x, t) for x in ends]
        if bypass == "first":
            self.edges.append((s, t))
        if arm:
            zs = [self.node() for _ in range(arm)]
            self.edges += list(zip([s] + zs, zs + [t]))
        if bypass and bypass != "first":
            self.edges.append((s, t))
        return t


def graph_case(name, build, bubble=0, permute=None, **rel_spec):
    b = Builder()
    build(b)
    edges = pp._w(b.edges)
    order = pp.first_seen(edges)
    if permute is not None:
        edges = [edges[i] for i in np.random.default_rng(permute).permutation(len(edges))]
    return dict(name=name, order=order, edges=[list(e) for e in edges], max_paths=1 << 20, bubble=bubble, rel_spec=rel_spec)


def host_paths(case) -> "phasing.HostResidentPaths":
    """The bubbles of the case's graph with every path on the host, behind the interface of a ``DevicePaths``."""
    if "walk" in case:
        order, edges = wp.node_order(case["walk"]), wu.edges_of(case["walk"])
    else:
        order, edges = case["order"], case["edges"]
    return phasing.HostResidentPaths(phasing.HostPaths(edges, order).phase_paths(None, case["max_paths"]))


def graph_inputs(case):
    """(node order, edges with weights) of the case's graph."""
    if "walk" in case:
        return wp.node_order(case["walk"]), [list(e) for e in wu.edges_of(case["walk"])]
    return list(case["order"]), [list(e) for e in case["edges"]]


def reads_of_node(case):
    if "walk" in case:
        return wp.reads_of_node(case["walk"])
    table = {int(n): [int(r) for r in rs] for n, rs in case["node_reads"]}
    return lambda x: table[int(x)]


def rel_of(case) -> phasing.RelevantReads:
    u32, i32 = (lambda v: np.asarray(v, dtype=np.uint32)), (lambda v: np.asarray(v, dtype=np.int32))
    R = len(case["overlap_max"])
    return phasing.RelevantReads(u32([]), u32(np.arange(R)), i32(case["overlap_max"]), u32(case["aln_off"]), u32(case["aln_b"]),
                                 i32(case["aln_a0"]), i32(case["aln_a1"]), u32(case["b_reads"]), 0, False)


# ---- the relevant reads of a graph case ---------------------------------------------------------------------------------------

def fill(case, seed):
    """``node_reads`` and the relevant reads of a graph case from a seed.  ``rel_spec``: R; n_b (the b reads are the interior
    reads named plus reads outside the bubble up to this number); ploidy; merged (every how-manieth interior node holds
    three reads); unnamed (every how-manieth interior node has reads no alignment names: alternately reads that are b reads
    without an alignment and reads that are no b reads at all); outside_only (every alignment names a read outside the
    bubble: S0 >= E everywhere); quiet_last (the nodes of the last diamond are unnamed: every path has a twin with the same
    per-read terms); favour_last (every read aligns widely to the first node of the last path)."""
    spec = dict(R=40, n_b=None, ploidy=2, merged=5, unnamed=7, outside_only=False, quiet_last=False, favour_last=False)
    spec.update(case["rel_spec"])
    rng = np.random.default_rng(seed)
    hp = host_paths(dict(case, node_reads=[]))
    b = case["bubble"]
    inside, paths = hp.interior_of(b), hp.paths_of(b)
    node_reads = {n: [1000 + n] for n in case["order"]}
    quiet, absent = set(), set()
    for j, n in enumerate(inside):
        if spec["merged"] and j % spec["merged"] == 2:
            node_reads[n] = [1000 + n, 5000 + n, 9000 + n]
        if spec["unnamed"] and j % spec["unnamed"] == 3:
            (quiet if (j // spec["unnamed"]) % 2 == 0 else absent).add(n)
    if spec["quiet_last"]:
        last_exit = paths[0][-2]                                   # the node before the exit on the diamond route
        quiet |= {p[-3] for p in paths if len(p) >= 3 and p[-2] == last_exit}
    named = [r for n in inside if n not in quiet and n not in absent for r in node_reads[n]]
    present = sorted(r for n in inside if n not in absent for r in node_reads[n])
    n_b = spec["n_b"] if spec["n_b"] is not None else len(present) + 3
    assert n_b > len(present), (case["name"], n_b, len(present))
    outside = [20000 + i for i in range(n_b - len(present))]
    b_reads = sorted(present + outside)
    local = {r: i for i, r in enumerate(b_reads)}
    pool = [local[r] for r in (outside if spec["outside_only"] else named + outside[:2])]
    R = spec["R"]
    om = rng.integers(400, 5000, size=R).tolist()
    aln = []
    for r in range(R):
        mine = []
        for _ in range(int(rng.integers(0 if R > 4 and r % 9 == 4 else 1, 4))):
            a0 = int(rng.integers(0, max(om[r] - 50, 1)))
            mine.append((int(pool[int(rng.integers(0, len(pool)))]), a0, a0 + int(rng.integers(20, 1500))))
        if spec["favour_last"]:
            mine.append((local[node_reads[paths[-1][1]][0]], 0, om[r]))
        aln.append(mine)
    if len(paths[0]) > CHUNK + 2 or len(paths[-1]) > CHUNK + 2:      # a long path: reads that only its nodes past the first chunk hold
        long_path = max(paths, key=len)
        for r in range(0, R, 3):
            node = long_path[CHUNK + 5 + r % 20]
            if node_reads[node][0] in local:
                aln[r].append((local[node_reads[node][0]], 1, om[r] - 1 - r))
    case = dict(case)
    case.pop("rel_spec")
    case.update(seed=int(seed), ploidy=spec["ploidy"], node_reads=[[int(n), node_reads[n]] for n in case["order"]], b_reads=b_reads,
                overlap_max=om, aln_off=np.cumsum([0] + [len(a) for a in aln]).tolist(), aln_b=[t[0] for a in aln for t in a],
                aln_a0=[t[1] for a in aln for t in a], aln_a1=[t[2] for a in aln for t in a])
    return case


def read_terms(case, path):
    """The per-read terms of a path's score, by the loops of ``phase_large_bubble`` (phasing.py:649-667) on local ids."""
    reads_of, local = reads_of_node(case), {int(r): i for i, r in enumerate(case["b_reads"])}
    mine = {local[r] for n in path[1:-1] for r in reads_of(n) if r in local}
    out = []
    for r in range(len(case["overlap_max"])):
        lo, hi = case["aln_off"][r], case["aln_off"][r + 1]
        f = pu._overlap(list(zip(case["aln_b"][lo:hi], case["aln_a0"][lo:hi], case["aln_a1"][lo:hi])), case["overlap_max"][r], mine)
        out.append(0.0 if f is None else f)
    return out


def definition(case):
    """``(scores, best)`` by those loops: the per-read terms added in read order, divided by R; the stable descending sort."""
    paths = host_paths(case).paths_of(case["bubble"])
    R = len(case["overlap_max"])
    scores = []
    for p in paths:
        s = 0.0
        for f in read_terms(case, p):
            if f:
                s += f
        scores.append(s / R)
    return scores, sorted(range(len(paths)), key=lambda p: scores[p], reverse=True)[:case["ploidy"]]


def margins_hold(case, scores):
    """Any two of the best ploidy + 1 scores are more than 4 table_tol apart, or equal by construction: the same per-read terms,
    whose sum has the same bits in any FIXED order."""
    R = len(case["overlap_max"])
    paths = host_paths(case).paths_of(case["bubble"])
    top = sorted(range(len(scores)), key=lambda p: scores[p], reverse=True)[:case["ploidy"] + 1]
    for i, p in enumerate(top):
        for q in top[:i]:
            if abs(scores[p] - scores[q]) * R > 4 * pu.table_tol(max(scores[p], scores[q]) * R, R):
                continue
            if read_terms(case, paths[p]) != read_terms(case, paths[q]):
                return False
    return True


def twin_scores(case, want_scores=True):
    """``(best, best_scores, scores)`` of the numpy twin (``phasing.HostResidentPaths.score_large``)."""
    return host_paths(case).score_large(case["bubble"], rel_of(case), reads_of_node(case), case["ploidy"], want_scores=want_scores)


def check_scores(got, case):
    R = len(case["overlap_max"])
    want = case["ref"]["scores"]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert abs(g - w) * R <= pu.table_tol(w * R, R), (g, w)


# ---- the cases ----------------------------------------------------------------------------------------------------------------

def _chain(b):
    """A diamond, a 65-path bubble, a 66-path bubble with a bypass, a diamond: the large bubbles are bubbles 1 and 2."""
    t = b.diamond(b.node())
    t = b.large(t, 6)
    t = b.large(t, 6, bypass=True)
    b.diamond(t)


def specs():
    one = lambda **kw: (lambda b: b.large(b.node(), **kw))   # noqa: E731
    return [
        graph_case("p3_n_best_8_r1", one(k=1), R=1, ploidy=8, n_b=32, merged=0, unnamed=0),
        graph_case("p64_r256", one(k=5, arm=0, lanes=2), R=256),
        graph_case("p65_r255", one(k=6), R=255, n_b=65),
        graph_case("p66_bypass_r257", one(k=6, bypass=True), R=257),
        graph_case("p66_bypass_first", one(k=6, bypass="first"), R=12, n_b=33),
        graph_case("p257", one(k=8), R=40, ploidy=3),
        graph_case("p33_r2049", one(k=5), R=2049),
        graph_case("p65_r2048", one(k=6), R=2048, ploidy=4),
        graph_case("long_path_300", one(k=6, arm=300), R=40),
        graph_case("all_zero", one(k=6), R=30, outside_only=True),
        graph_case("tie_for_first", one(k=6), R=50, quiet_last=True, unnamed=0),
        graph_case("winner_last", one(k=6), R=50, favour_last=True),
        graph_case("second_of_four", _chain, bubble=1, R=33),
        graph_case("third_of_four", _chain, bubble=2, R=33),
        graph_case("nested", one(k=6, nested=True), R=45),
        graph_case("permuted", one(k=6, nested=True, bypass=True), R=45, permute=77),
    ]


WALK_NAME = "walk_65_between_two"


def walk_inputs(seed):
    """A synthetic walk whose chain has a 65-path bubble between two ordinary ones (``walk_utils.synth``)."""
    w = wu.synth(seed, params=wu._params(max_bubble_size=10), paths=[2, 65, 2], depth=1, span=[8, 24, 8], window=2)
    w["name"] = WALK_NAME
    return w


def walk_case(walk):
    """The case of the walk's large bubble: the relevant reads as ``phase_chain`` collects them at a large bubble (all aligning
    reads, nothing before it) through ``phasing.HostIndex``."""
    case = dict(name=walk["name"], walk=walk, max_paths=1 << 20, bubble=1, ploidy=walk["params"]["ploidy"])
    hp = host_paths(case)
    bubbles = phasing.chain_bubbles_input(hp, 0, wp.reads_of_node(walk))
    src = phasing.HostIndex(wu.lengths_of(walk))
    rel = phasing.relevant_reads(src, src.phase_index(wu.rows_of(walk)), bubbles[1]["interior_reads"], [], [], bubbles[1]["preds"], True, 0)
    case.update(b_reads=rel.b_reads.tolist(), overlap_max=rel.overlap_max.tolist(), aln_off=rel.aln_off.tolist(), aln_b=rel.aln_b.tolist(),
                aln_a0=rel.aln_a0.tolist(), aln_a1=rel.aln_a1.tolist())
    return case


def build(spec, first_seed=1):
    """The case of a spec: the first seed at which the margins hold on the definition's numbers."""
    for seed in range(first_seed, first_seed + 200):
        case = fill(spec, seed)
        if margins_hold(case, definition(case)[0]):
            return case
    raise AssertionError("no seed gives %s its margins" % spec["name"])


# ---- golden file --------------------------------------------------------------------------------------------------------------

def save_golden(obj):
    cu.save_golden(obj, GOLDEN_FILE)


_GOLDEN = []


def load_golden():
    if not _GOLDEN:
        _GOLDEN.append(cu.load_golden(GOLDEN_FILE))
    return _GOLDEN[0]


def cases():
    return load_golden()["cases"]


# ---- what the device tests share ----------------------------------------------------------------------------------------------

def device_graph(order, edges):
    """(handle, graph result) of a graph through po_graph_from_edges, on a handle with one segment per two node ids."""
    from phasm_amd.overlapper import ExactOverlapper
    ov = ExactOverlapper()
    for i in range(((max([int(x) for x in order] + [1]) | 1) + 1) // 2):
        ov.add_segment("s%d" % i, 1000 + i % 97)
    e = np.asarray([[u, v, w, 17] for u, v, w in edges], dtype=np.int64).reshape(-1, 4)
    return ov, ov.graph_from_edges(e, order)


def simple_rel(inside, R, seed):
    """Relevant reads over a bubble of which only the interior nodes are at hand: node n holds read 1000 + n, every read
    has one to three alignments to interior reads.  ``(RelevantReads, reads_of_node)``."""
    rng = np.random.default_rng(seed)
    b_reads = sorted(1000 + int(n) for n in inside)
    om = rng.integers(400, 5000, size=R)
    count = rng.integers(1, 4, size=R)
    n_aln = int(count.sum())
    a0 = rng.integers(0, 350, size=n_aln)
    u32, i32 = (lambda v: np.asarray(v, dtype=np.uint32)), (lambda v: np.asarray(v, dtype=np.int32))
    rel = phasing.RelevantReads(u32([]), u32(np.arange(R)), i32(om), u32(np.concatenate([[0], np.cumsum(count)])),
                                u32(rng.integers(0, len(b_reads), size=n_aln)), i32(a0), i32(a0 + rng.integers(20, 1500, size=n_aln)),
                                u32(b_reads), 0, False)
    return rel, (lambda n: [1000 + int(n)])
