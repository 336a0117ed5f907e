"""The resident route through one step of the walk (po_walk_relevant, po_walk_step_resident, po_walk_prev_copy; DESIGN.md section
3.9w) against the route through host lists and arrays (po_phase_relevant + po_walk_step), on one handle: every golden walk of
tests/golden/walk_cases.npz by both routes with every gather, every (cand, ext, rl), the stats, histories, read sets and the two
previous sets equal, twice on the same walk objects; two walks back to back on one handle in both orders; a synthetic walk past
what the goldens reach; the contract's edges; one step with 530 000 new reads in b_reads; and the `phase` command by both
routes."""
import ctypes

import numpy as np
import pytest

import large_utils as lu
import phase_utils as pu
import relevant_utils as ru
import resident_utils as rsu
import walk_product_utils as wp
import walk_utils as wu
from phasm_amd import phasing
from phasm_amd.overlapper import ExactOverlapper

pytestmark = pytest.mark.gpu

WALKS = wu.load_golden()["walks"]
NAMES = [w["name"] for w in WALKS]
FRESH = {"ploidy": 2, "n_cands": 1, "depth": 0, "start_of_block": 1, "n_block_reads": 0}


def named(name):
    return next(w for w in WALKS if w["name"] == name)


def lists(triple):
    return [x.tolist() for x in triple[:2]] + [triple[2].tobytes()]


@pytest.mark.parametrize("name", NAMES)
def test_every_golden_walk_by_both_routes_on_one_handle(name):
    walk = named(name)
    k = walk["params"]["ploidy"]
    ov = rsu.handle_for(walk)
    index = rsu.indexed(ov, walk)
    dw_host, dw_res = ov.phase_walk(k), ov.phase_walk(k)
    got, blocks, raw = rsu.both_routes(walk, ov, index, dw_host, dw_res)
    wu.same_trace(got, walk, walk, optional=wp.OPTIONAL)                   # ... and so the reference's recorded phase()
    wp.check_blocks(blocks, got)
    # a second time on the same walk objects: what the first walk left is un-mapped and cleared at the first device call
    dw_host.reset()
    dw_res.reset()
    assert dw_res.info() == dict(FRESH, ploidy=k) and dw_res.prev_sets() == ([], [])
    again, _, raw_again = rsu.both_routes(walk, ov, index, dw_host, dw_res)
    assert raw_again == raw and again[2] == got[2]
    dw_res.close()
    dw_host.close()
    index.free()
    ov.close()


@pytest.mark.parametrize("order", [("grow_words", "break_and_shrink"), ("break_and_shrink", "grow_words")], ids="_then_".join)
def test_two_walks_back_to_back_on_one_handle_and_one_walk_object(order):
    """The map, the two sets and the rows grow, shrink to a handful of reads and grow again on ONE walk object of the resident
    route: every step byte-equal to the same walk by the host route on a fresh handle."""
    walks = [named(n) for n in order]
    fresh = []
    for walk in walks:
        ov = rsu.handle_for(walk)
        index = rsu.indexed(ov, walk)
        dw = ov.phase_walk(2)
        raw = []
        got, _ = rsu.run_chain(walk, ov, ov, index, dw, False, raw=raw)
        wu.same_trace(got, walk, walk, optional=wp.OPTIONAL)
        fresh.append((raw, got[2]["cands"]))
        dw.close()
        index.free()
        ov.close()
    ovs = ExactOverlapper()
    ru.add_reads(ovs, walks[0]["lengths"] + walks[1]["lengths"])
    dw = ovs.phase_walk(2)
    for walk, shift, (want, cands) in zip(walks, [0, 2 * len(walks[0]["lengths"])], fresh):
        moved = rsu.shifted(walk, shift)
        index = rsu.indexed(ovs, moved)
        dw.reset()
        raw = []
        got, _ = rsu.run_chain(moved, ovs, ovs, index, dw, True, raw=raw)
        assert raw == want, "%s after %s on one walk object: the bytes of a step differ from those on a fresh handle" % (walk["name"], order[0])
        assert [[[x - shift for x in s] for s in c["read_sets"]] for c in got[2]["cands"]] == [c["read_sets"] for c in cands]
        index.free()
    dw.close()
    ovs.close()


def test_a_long_walk_equals_the_host_array_route_and_the_host_walk():
    walk = rsu.long_walk()                                # (the properties and the margins: on the host, before the device)
    assert rsu.long_properties(walk) is None and wu.margins_hold(walk) is None
    ov = rsu.handle_for(walk)
    index = rsu.indexed(ov, walk)
    dw_host, dw_res = ov.phase_walk(2), ov.phase_walk(2)
    got, blocks, raw = rsu.both_routes(walk, ov, index, dw_host, dw_res, bubbles=walk["bubbles"])
    src, sc = phasing.HostIndex(wu.lengths_of(walk)), phasing.HostScorer()
    hw = phasing.HostWalk(sc, 2)
    want, host_blocks = rsu.run_chain(walk, sc, src, src.phase_index(wu.rows_of(walk)), hw, True, bubbles=walk["bubbles"])
    assert [s["arm"] for s in got[0]] == [s["arm"] for s in want[0]] and "retry" in [s["arm"] for s in got[0]]
    assert [(s.get("surv_cand"), s.get("surv_ext")) for s in got[0]] == [(s.get("surv_cand"), s.get("surv_ext")) for s in want[0]]
    assert [(b.haplotypes, b.read_sets, b.tie, b.include_last) for b in blocks] == [(b.haplotypes, b.read_sets, b.tie, b.include_last) for b in host_blocks]
    info = dw_res.info()
    assert info == hw.info() and dw_res.prev_sets() == hw.prev_sets()
    assert max(s["n_b"] for s in got[0]) > 256
    everyone = list(range(info["n_cands"]))
    assert dw_res.history(everyone).tolist() == hw.history(everyone).tolist() and dw_res.read_sets(everyone) == hw.read_sets(everyone)
    for w in (dw_res, dw_host):
        w.close()
    index.free()
    ov.close()


class Live:
    """``grow_words`` on one handle with a walk of each route, advanced over the first ``n`` bubbles in lock-step."""

    def __init__(self, n):
        self.walk = named("grow_words")
        self.p = self.walk["params"]
        self.ov = rsu.handle_for(self.walk)
        self.index = rsu.indexed(self.ov, self.walk)
        self.host, self.res = self.ov.phase_walk(2), self.ov.phase_walk(2)
        self.levels = phasing.prune_levels(self.p["prune_factor"], self.p["prune_step_size"], self.p["max_prune_rounds"])
        self.prev_graph, self.prev_aligning = set(), set()
        self.bubbles = wp.recorded_bubbles(self.walk)
        expand = wp.reads_of_node(self.walk)
        self.path_reads = [[[r for x in path[1:-1] for r in expand(x)] for path in b["paths"]] for b in self.bubbles]
        for i in range(n):
            g = self.gather(i)
            assert lists(self.res.step_resident(g, *self.step_args(i))) == lists(self.host_step(i))
            g.close()

    def step_args(self, i, start=None):
        start = self.res.start_of_block if start is None else start
        return (self.path_reads[i], start, self.p["threshold"], self.p["min_spanning_reads"], self.levels, self.p["max_candidates"])

    def gather(self, i, **kw):
        b = self.bubbles[i]
        return self.res.relevant(self.ov, self.index, b["interior_reads"], b["preds"], self.res.start_of_block, self.p["min_spanning_reads"], **kw)

    def host_rel(self, i, prev_graph=None):
        b = self.bubbles[i]
        return phasing.relevant_reads(self.ov, self.index, b["interior_reads"], sorted(self.prev_graph if prev_graph is None else prev_graph),
                                      sorted(self.prev_aligning), b["preds"], self.host.start_of_block, self.p["min_spanning_reads"])

    def host_step(self, i, **kw):
        rel = self.host_rel(i)
        out = self.host.step(rel, *self.step_args(i, self.host.start_of_block), **kw)
        if kw.get("advance", True) and len(out[2]):
            self.prev_graph |= set(self.bubbles[i]["interior_reads"])
            self.prev_aligning |= set(rel.cur_aligning.tolist())
        return out

    def same_state(self):
        n = self.res.info()["n_cands"]
        assert self.res.info() == self.host.info() and self.res.prev_sets() == (sorted(self.prev_graph), sorted(self.prev_aligning))
        for cands in ([0], [n - 1, 0], list(range(n))):
            assert self.res.history(cands).tolist() == self.host.history(cands).tolist() and self.res.read_sets(cands) == self.host.read_sets(cands)
        assert self.res.best() == self.host.best()

    def close(self):
        self.res.close()
        self.host.close()
        self.index.free()
        self.ov.close()


def test_a_peek_then_the_advance_and_a_cap_of_one_and_other_calls_in_between():
    """On one gather: a peek changes nothing, the advancing call with ``cap`` = 1 brings one entry home and takes the whole list
    over; between the gather and its step ``po_phase_branch`` and ``po_phase_relevant`` run at other sizes on the handle."""
    t = Live(2)
    big = next(c for c in pu.load_golden()["cases"] if c["name"] == "nb33_r64")
    for i in (2, 3):
        g = t.gather(i)
        assert rsu.rel_bytes(g.fetch()) == rsu.rel_bytes(t.host_rel(i))
        pu.check_result(pu.result_of(t.ov, big), big["ref"], big)             # (the handle's phase scratch at another size)
        t.host_rel(0, prev_graph=[])                                          # (the handle's gather scratch at another size)
        before = (t.res.info(), t.res.prev_sets(), t.res.read_sets([0]))
        peek = t.res.step_resident(g, *t.step_args(i), advance=False)
        assert (t.res.info(), t.res.prev_sets(), t.res.read_sets([0])) == before and t.ov.walk_stats()["advanced"] == 0
        t.host_rel(0, prev_graph=[])
        got = t.res.step_resident(g, *t.step_args(i), cap=1)
        st = rsu.counts(t.ov.walk_stats())
        want = t.host_step(i)
        assert lists(peek) == lists(want) and len(want[0]) > 1
        assert len(got[0]) == 1 and (got[0][0], got[1][0]) == (want[0][0], want[1][0]) and got[2].tobytes() == want[2][:1].tobytes()
        assert st == rsu.counts(t.ov.walk_stats()) and st["advanced"] == 1 and st["n_cands_out"] == len(want[0])
        t.same_state()
        g.close()
    t.close()


def test_a_stale_gather_and_the_other_route_inside_a_block_are_refused():
    t = Live(1)
    g1 = t.gather(1)
    # the five mismatches and the pointers, on a live gather: each refused with the state as it was
    before = (t.res.info(), t.res.prev_sets())
    with pytest.raises(ValueError, match="start_of_block is not the walk's"):
        t.res.step_resident(g1, *t.step_args(1, start=True))
    for field, sentence in (("n_relevant", "n_reads is not the number of relevant reads of the gather"),
                            ("n_b", "n_b is not the number of b reads of the gather")):
        keep = getattr(g1, field)
        setattr(g1, field, keep + 1)
        with pytest.raises(ValueError, match=sentence):
            t.res.step_resident(g1, *t.step_args(1))
        setattr(g1, field, keep)
    other = t.ov.phase_walk(3)
    with pytest.raises(ValueError, match="the gather belongs to another walk"):
        other.step_resident(g1, *t.step_args(1, start=True))
    other.close()
    with pytest.raises(ValueError, match="a path names a read the handle does not hold"):
        t.res.step_resident(g1, [[len(t.ov)]] + t.path_reads[1][1:], *t.step_args(1)[1:])
    with pytest.raises(ValueError, match="every other array must be NULL"):
        raw_step(t, g1, overlap_max=True)
    with pytest.raises(ValueError, match="n_cands is not the number of candidates the walk holds"):
        raw_step(t, g1, n_cands=t.res.info()["n_cands"] + 1)
    with pytest.raises(ValueError, match="the ploidy is not the walk's"):
        raw_step(t, g1, ploidy=3)
    assert (t.res.info(), t.res.prev_sets()) == before
    # the next gather makes this one stale, for the copy and for the step
    g2 = t.gather(1)
    for call in (g1.fetch, lambda: t.res.step_resident(g1, *t.step_args(1))):
        with pytest.raises(ValueError, match="the gather is stale"):
            call()
    # one route per block: po_walk_step on the resident walk, po_walk_relevant / po_walk_step_resident on the host walk
    with pytest.raises(ValueError, match="po_walk_step: the block advanced by po_walk_step_resident"):
        t.res.step(g2.fetch(), *t.step_args(1))
    with pytest.raises(ValueError, match="po_walk_relevant: the block advanced by po_walk_step"):
        t.host.relevant(t.ov, t.index, t.bubbles[1]["interior_reads"], t.bubbles[1]["preds"], False, 3)
    assert lists(t.res.step_resident(g2, *t.step_args(1))) == lists(t.host_step(1))
    with pytest.raises(ValueError, match="the gather was made at another depth of the walk"):
        t.res.step_resident(g2, *t.step_args(2))
    t.same_state()
    # after a reset either walk takes the other route: a read of the old block gets a new id
    t.res.reset()
    t.host.reset()
    with pytest.raises(ValueError, match="the gather is stale"):              # (it did not fall back: the reset took it)
        t.res.step_resident(g2, *t.step_args(1))
    t.res, t.host = t.host, t.res
    t.prev_graph, t.prev_aligning = set(), set()
    assert t.res.prev_sets() == ([], []) and t.host.prev_sets() == ([], [])
    for i in (1, 0):
        g = t.gather(i)
        assert lists(t.res.step_resident(g, *t.step_args(i))) == lists(t.host_step(i))
        t.same_state()
        g.close()
    # a gather outlives its walk as a stale result, and a walk its gather
    g = t.gather(2)
    t.res.close()
    with pytest.raises(ValueError, match="the gather is stale"):
        g.fetch()
    g.close()
    t.res = t.ov.phase_walk(2)
    t.close()


def raw_step(t, g, overlap_max=False, n_cands=None, ploidy=2):
    """One po_walk_step_resident call through ctypes, with what ``DeviceWalk.step_resident`` cannot get wrong."""
    from phasm_amd import _lib
    from phasm_amd.overlapper import _check
    path_off, path_ids, lv = np.asarray([0, 1, 2], np.uint32), np.asarray([0, 1], np.uint32), np.asarray(t.levels, np.float64)
    keep = np.zeros(4, np.int32)
    prm = _lib.PoPhaseParams(ploidy, 2, t.res.info()["n_cands"] if n_cands is None else n_cands, g.n_relevant, g.n_b, 0, 3, 1, 90, len(lv),
                             1e-4, 0, 0)
    inp = _lib.PoPhaseInput(keep.ctypes.data if overlap_max else None, None, None, None, None, path_off.ctypes.data, path_ids.ctypes.data,
                            None, None, lv.ctypes.data)
    n = ctypes.c_uint64(9)
    st = _lib.load().po_walk_step_resident(t.ov._h, t.res._ptr, g._ptr, ctypes.byref(prm), ctypes.byref(inp), 1, None, None, None, 0,
                                           ctypes.byref(n))
    assert st != 0 and n.value == 0
    _check(t.ov._h, st)


def test_a_gather_that_fell_back_is_stepped_after_the_reset():
    t = Live(2)
    b = t.bubbles[2]
    g = t.res.relevant(t.ov, t.index, b["interior_reads"], b["preds"], False, 10 ** 6)     # (never that many spanning reads)
    assert g.fell_back
    for w in (t.res, t.host):
        w.reset()
    t.prev_graph, t.prev_aligning = set(), set()
    rel = phasing.relevant_reads(t.ov, t.index, b["interior_reads"], [], [], b["preds"], True, 0)
    assert rsu.rel_bytes(g.fetch())[:8] == rsu.rel_bytes(rel)[:8]
    args = (t.path_reads[2], True, t.p["threshold"], 0, t.levels, t.p["max_candidates"])
    assert lists(t.res.step_resident(g, *args)) == lists(t.host.step(rel, *args))
    t.prev_graph, t.prev_aligning = set(b["interior_reads"]), set(rel.cur_aligning.tolist())
    t.same_state()
    t.res.reset()
    with pytest.raises(ValueError, match="the gather is stale"):              # (one reset, not two)
        t.res.step_resident(g, *args)
    g.close()
    t.close()


def test_without_prev_graph_at_a_large_bubble_then_score_large():
    """The gather of a large bubble behind a phased block: prev_graph counts as empty, prev_aligning still counts the spanning
    reads; ``score_large`` on the fetched arrays gives what it gives on po_phase_relevant's."""
    case = next(c for c in lu.cases() if "walk" in c)
    walk = case["walk"]
    p = walk["params"]
    order, edges = lu.graph_inputs(case)
    ov = rsu.handle_for(walk)                                                 # (the walk's reads: the graph's nodes are among them)
    graph = ov.graph_from_edges(np.asarray([[u, v, w, 17] for u, v, w in edges], dtype=np.int64).reshape(-1, 4), order)
    paths = ov.phase_paths_resident(graph, case["max_paths"])
    graph.free()
    index = rsu.indexed(ov, walk)
    bubbles = phasing.chain_bubbles_input(paths, 0, wp.reads_of_node(walk), resident_above=64)
    assert bubbles[1]["paths"] is None and bubbles[1]["n_paths"] == 65
    dw = ov.phase_walk(p["ploidy"])
    b0, big = bubbles[0], bubbles[1]
    g0 = dw.relevant(ov, index, b0["interior_reads"], b0["preds"], True, p["min_spanning_reads"])
    expand = wp.reads_of_node(walk)
    first = dw.step_resident(g0, [[r for x in path[1:-1] for r in expand(x)] for path in b0["paths"]], True, p["threshold"],
                             p["min_spanning_reads"], phasing.prune_levels(p["prune_factor"], p["prune_step_size"], p["max_prune_rounds"]),
                             p["max_candidates"])
    assert len(first[0]) and dw.info()["depth"] == 1
    prev_graph, prev_aligning = dw.prev_sets()
    assert prev_graph == sorted(set(b0["interior_reads"])) and prev_aligning == g0.fetch().cur_aligning.tolist()
    g = dw.relevant(ov, index, big["interior_reads"], big["preds"], True, 0, without_prev_graph=True)
    want = phasing.relevant_reads(ov, index, big["interior_reads"], [], prev_aligning, big["preds"], True, 0)
    with_prev = phasing.relevant_reads(ov, index, big["interior_reads"], prev_graph, prev_aligning, big["preds"], True, 0)
    rel = g.fetch()
    assert rsu.rel_bytes(rel) == rsu.rel_bytes(want) and g.n_spanning == want.n_spanning > 0 and len(with_prev.b_reads) > g.n_b
    assert dw.prev_sets() == (prev_graph, prev_aligning)                      # (a gather changes neither set)
    a = big["scorer"].score_large(rel, expand, p["ploidy"], want_scores=True)
    b = big["scorer"].score_large(want, expand, p["ploidy"], want_scores=True)
    assert a[0] == b[0] and a[0][0] == int(case["ref"]["best"][0]) and a[2].tobytes() == b[2].tobytes()
    dw.close()
    paths.close()
    index.free()
    ov.close()


def test_one_step_past_one_capped_grid():
    """530 000 reads in b_reads, all new to the block, one candidate, ploidy 1, two paths, a handful of alignments: the
    grid-stride loops of the new kernels and the prefix sum over more than one window, against the host-array route."""
    n_seg, n_cur = 265_100, 530_000
    ov = ExactOverlapper()
    for i in range(n_seg):
        ov.add_segment("s%d" % i, 900)
    n_ids = len(ov)
    assert n_ids == 2 * n_seg
    out = [n_ids - 1, n_ids - 2, n_ids - 7]                                   # three reads outside the graph
    rows = [(out[0], 0, 10, 400, 0, 390), (out[0], 31, 300, 700, 5, 405), (out[0], 64, 600, 890, 0, 290), (out[1], 265_000, 0, 500, 100, 600),
            (n_cur - 1, out[1], 20, 420, 400, 800), (out[2], 32, 50, 450, 0, 400), (out[2], 529_999 - 64, 400, 800, 0, 400), (63, out[2], 0, 99, 700, 799)]
    res = ov.result_from_rows(ru.rows_array(rows))
    index = ov.phase_index(res)
    res.free()
    cur = list(range(n_cur))
    path_reads = [list(range(0, n_cur, 2)), list(range(1, n_cur, 2)) + [n_ids - 3]]     # (the last one is no b read: dropped)
    host, resw = ov.phase_walk(1), ov.phase_walk(1)
    rel = phasing.relevant_reads(ov, index, cur, [], [], [], True, 0)
    g = resw.relevant(ov, index, cur, [], True, 0)
    assert g.n_b == n_cur and g.n_alignments == 8 and rsu.rel_bytes(g.fetch()) == rsu.rel_bytes(rel)
    want = host.step(rel, path_reads, True, 0.0, 0, [], 0)
    st_host = rsu.counts(ov.walk_stats())
    got = resw.step_resident(g, path_reads, True, 0.0, 0, [], 0)
    st = rsu.counts(ov.walk_stats())
    assert lists(got) == lists(want) and len(want[0]) == 2
    assert st == st_host and st["n_new_reads"] == n_cur and st["words_per_slot"] == (n_cur + 31) // 32 and st["advanced"] == 1
    assert resw.info() == host.info() and resw.info()["n_block_reads"] == n_cur
    assert resw.read_sets([0, 1]) == host.read_sets([0, 1]) and resw.read_sets([1]) == [[path_reads[1][:-1]]]
    prev_graph, prev_aligning = resw.prev_sets()
    assert prev_graph == cur and prev_aligning == rel.cur_aligning.tolist()
    # a second step in the block: every read is known now and keeps its id; then the reset un-maps all of them
    g2 = resw.relevant(ov, index, cur[:1000], [], False, 0)
    rel2 = phasing.relevant_reads(ov, index, cur[:1000], prev_graph, prev_aligning, [], False, 0)
    assert rsu.rel_bytes(g2.fetch()) == rsu.rel_bytes(rel2)
    assert lists(resw.step_resident(g2, path_reads, False, 0.0, 0, [], 0)) == lists(host.step(rel2, path_reads, False, 0.0, 0, [], 0))
    assert rsu.counts(ov.walk_stats())["n_new_reads"] == 0 and resw.read_sets([0]) == host.read_sets([0])
    resw.reset()
    host.reset()
    g3 = resw.relevant(ov, index, [529_999 - 64, 64, 64], [], True, 0)       # (a duplicate in cur_graph counts once)
    rel3 = phasing.relevant_reads(ov, index, [529_999 - 64, 64, 64], [], [], [], True, 0)
    assert rsu.rel_bytes(g3.fetch()) == rsu.rel_bytes(rel3) and g3.n_b == 2
    assert lists(resw.step_resident(g3, [[64], [529_999 - 64]], True, 0.0, 0, [], 0)) == lists(host.step(rel3, [[64], [529_999 - 64]], True, 0.0, 0, [], 0))
    assert rsu.counts(ov.walk_stats())["n_new_reads"] == 2 and resw.read_sets([0, 1]) == host.read_sets([0, 1])
    assert resw.prev_sets() == ([64, 529_999 - 64], rel3.cur_aligning.tolist())
    for w in (resw, host):
        w.close()
    index.free()
    ov.close()


def phase_argv(p):
    return ["phase", "-p", str(p["ploidy"]), "-s", str(p["min_spanning_reads"]), "-b", str(p["max_bubble_size"]), "-t", repr(p["threshold"]),
            "-d", repr(p["prune_factor"]), "-c", str(p["max_candidates"]), "-r", str(p["max_prune_rounds"]), "-S", repr(p["prune_step_size"]),
            "--seed", "7", "-o"]


@pytest.mark.parametrize("name", ["ploidy3_rounds", "merged_nodes", "chain_with_a_65_path_bubble"])
def test_phase_end_to_end_by_both_routes(name, tmp_path):
    """`phase` on the files of a recorded chain: the resident route (the command's own) and ``--host-sets`` write the same bytes,
    and they are the recorded haplotypes (where a block ends in a tie of candidates that differ in the order of their slots,
    its sequences are compared as a sorted list)."""
    from phasm_amd import cli
    if name == "chain_with_a_65_path_bubble":
        walk = next(c for c in lu.cases() if "walk" in c)["walk"]
        hp = lu.host_paths(next(c for c in lu.cases() if "walk" in c))
        src, sc = phasing.HostIndex(wu.lengths_of(walk)), phasing.HostScorer()
        p, turns = walk["params"], []
        list(phasing.phase_chain(sc, src, src.phase_index(wu.rows_of(walk)),
                                 phasing.chain_bubbles_input(hp, 0, wp.reads_of_node(walk), resident_above=64), wp.reads_of_node(walk),
                                 p["ploidy"], p["min_spanning_reads"], p["max_bubble_size"], p["threshold"], p["prune_factor"], p["max_candidates"],
                                 p["max_prune_rounds"], p["prune_step_size"], walk=phasing.HostWalk(sc, p["ploidy"]), choose=wp.first,
                                 on_step=turns.append, resident=True))
        recorded = dict(walk, trace=[{"yields": t["yields"]} for t in turns[:-1]], final={"yields": turns[-1]["yields"]})
    else:
        walk = recorded = named(name)
    p = walk["params"]
    fasta, aln, graph, node_name = wp.write_chain_files(walk, str(tmp_path))
    out, out_host = str(tmp_path / "out.fasta"), str(tmp_path / "out_host.fasta")
    assert cli.main(phase_argv(p) + [out, fasta, aln, graph]) == 0
    assert cli.main(phase_argv(p) + [out_host, "--host-sets", fasta, aln, graph]) == 0
    with open(out, "rb") as a, open(out_host, "rb") as b:
        written = a.read()
        assert written and written == b.read()
    got, want = wp.read_fasta_entries(out), wp.expected_fasta(recorded, graph, node_name)
    assert [n for n, _ in got] == [n for n, _ in want] and len(want) >= p["ploidy"]
    if name == "ploidy3_rounds":
        assert got == want
    else:
        block = lambda entries: sorted((n.rsplit(".", 1)[0], s) for n, s in entries)   # noqa: E731
        assert block(got) == block(want)
        assert name == "merged_nodes" or [n for n, _ in got].count("chain0.largebubble1") == 1
