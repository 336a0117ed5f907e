"""The resident route of the walk without a GPU: all golden walks of tests/golden/walk_cases.npz (the reference's own
``phase()``) through ``phasing.phase_chain(resident=True)`` on ``HostScorer`` / ``HostIndex`` / ``HostWalk`` -- the loop keeps no
previous sets of its own and asks ``walk.relevant`` / ``walk.step_resident`` / ``walk.prev_sets``.  It must yield the same blocks
and the same ``on_step`` traces as ``resident=False``, and so as the recording; after every turn the walk's two sets are those
the other loop holds.  Also the contract's edges on the host statement: one live gather, one route per block, a peek."""
import pytest

import resident_utils as rsu
import walk_product_utils as wp
import walk_utils as wu
from phasm_amd import phasing

WALKS = wu.load_golden()["walks"]
NAMES = [w["name"] for w in WALKS]


def host(walk):
    src = phasing.HostIndex(wu.lengths_of(walk))
    return phasing.HostScorer(), src, src.phase_index(wu.rows_of(walk))


def test_the_golden_walks_are_the_eleven_with_53_steps():
    assert len(WALKS) == 11 and sum(len(w["trace"]) for w in WALKS) == 53


@pytest.mark.parametrize("name", NAMES)
def test_the_resident_loop_on_the_host_equals_the_other_loop_and_the_walk(name):
    walk = next(w for w in WALKS if w["name"] == name)
    sc, src, index = host(walk)
    k = walk["params"]["ploidy"]
    raw_host, raw_res, sets = [], [], []
    want, want_blocks = rsu.run_chain(walk, sc, src, index, phasing.HostWalk(sc, k), False, raw=raw_host)
    hw = phasing.HostWalk(sc, k)
    got, blocks = rsu.run_chain(walk, sc, src, index, hw, True, raw=raw_res, sets=sets)
    assert got[0] == want[0], "%s: the on_step traces differ" % name          # every key of every turn, exactly
    assert got[1] == want[1] and got[2] == want[2]
    assert blocks == want_blocks and raw_res == raw_host
    wu.same_trace(got, walk, walk, optional=wp.OPTIONAL)                       # ... and so the reference's recorded phase()
    wp.check_blocks(blocks, got)
    assert sets == rsu.loop_sets(want[0], wp.recorded_bubbles(walk))
    assert list(hw.prev_sets()) == [walk["state"]["prev_graph"], walk["state"]["prev_aligning"]]


def test_without_on_step_the_arrays_stay_where_they_are():
    """No trace asked for: ``fetch()`` is called at the large arm alone, and the blocks are the same."""
    fetched = []

    class Counting(phasing.HostWalk):
        def relevant(self, *a, **kw):
            g = super().relevant(*a, **kw)
            inner = g.fetch
            g.fetch = lambda: (fetched.append(1), inner())[1]
            return g

    for walk in WALKS:
        sc, src, index = host(walk)
        p, k = walk["params"], walk["params"]["ploidy"]
        args = (sc, src, index, wp.recorded_bubbles(walk), wp.reads_of_node(walk), k, p["min_spanning_reads"], p["max_bubble_size"],
                wu.param(p["threshold"]), wu.param(p["prune_factor"]), p["max_candidates"], p["max_prune_rounds"], p["prune_step_size"])
        want = list(phasing.phase_chain(*args, walk=phasing.HostWalk(sc, k), choose=wp.first))
        del fetched[:]
        got = list(phasing.phase_chain(*args, walk=Counting(sc, k), choose=wp.first, resident=True))
        assert got == want
        assert len(fetched) == sum(s["arm"] == "large" for s in walk["trace"]), walk["name"]


def first_two(walk):
    sc, src, index = host(walk)
    b0, b1 = wp.recorded_bubbles(walk)[:2]
    return sc, src, index, b0, b1, [list(p[1:-1]) for p in b0["paths"]], [list(p[1:-1]) for p in b1["paths"]]


def test_a_peek_then_the_advance_on_one_gather_and_the_stale_ones():
    walk = next(w for w in WALKS if w["name"] == "straight")
    sc, src, index, b0, b1, paths0, paths1 = first_two(walk)
    hw = phasing.HostWalk(sc, 2)
    assert hw.prev_sets() == ([], [])
    g0 = hw.relevant(src, index, b0["interior_reads"], b0["preds"], True, 3)
    before = (hw.info(), hw.prev_sets())
    peek = hw.step_resident(g0, paths0, True, 1e-3, 3, advance=False)
    assert (hw.info(), hw.prev_sets()) == before and len(peek[0])
    took = hw.step_resident(g0, paths0, True, 1e-3, 3)
    assert [x.tolist() for x in took] == [x.tolist() for x in peek] and hw.info()["depth"] == 1
    assert hw.prev_sets() == (sorted(set(b0["interior_reads"])), g0.fetch().cur_aligning.tolist())
    with pytest.raises(ValueError, match="the gather was made at another depth of the walk"):
        hw.step_resident(g0, paths1, False, 1e-3, 3)
    g1 = hw.relevant(src, index, b1["interior_reads"], b1["preds"], False, 3)
    with pytest.raises(ValueError, match="the gather is stale"):
        g0.fetch()
    with pytest.raises(ValueError, match="the gather is stale"):
        hw.step_resident(g0, paths1, False, 1e-3, 3)
    # one route per block: the host-array step is refused inside a resident block, and the other way round after a reset
    with pytest.raises(ValueError, match="the two routes do not mix before po_walk_reset"):
        hw.step(g1.fetch(), paths1, False, 1e-3, 3)
    hw.reset()
    assert hw.prev_sets() == ([], [])
    with pytest.raises(ValueError, match="the gather is stale"):              # (it did not fall back: the reset took it)
        hw.step_resident(g1, paths1, True, 1e-3, 3)
    rel = phasing.relevant_reads(src, index, b0["interior_reads"], [], [], b0["preds"], True, 3)
    hw.step(rel, paths0, True, 1e-3, 3)
    with pytest.raises(ValueError, match="the two routes do not mix before po_walk_reset"):
        hw.relevant(src, index, b1["interior_reads"], b1["preds"], False, 3)
    hw.reset()
    hw.relevant(src, index, b1["interior_reads"], b1["preds"], True, 3).close()


def test_a_gather_that_fell_back_is_stepped_after_the_reset():
    walk = next(w for w in WALKS if w["name"] == "straight")
    sc, src, index, b0, b1, paths0, paths1 = first_two(walk)
    hw = phasing.HostWalk(sc, 2)
    hw.step_resident(hw.relevant(src, index, b0["interior_reads"], b0["preds"], True, 3), paths0, True, 1e-3, 3)
    g = hw.relevant(src, index, b1["interior_reads"], b1["preds"], False, 10 ** 6)     # (never that many spanning reads)
    assert g.fell_back
    hw.reset()
    want = phasing.relevant_reads(src, index, b1["interior_reads"], [], [], b1["preds"], True, 0)
    assert g.fetch().b_reads.tolist() == want.b_reads.tolist() and g.fetch().rel_reads.tolist() == want.rel_reads.tolist()
    other = phasing.HostWalk(sc, 2)
    a = hw.step_resident(g, paths1, True, 1e-3, 0)
    b = other.step(want, paths1, True, 1e-3, 0)
    assert [x.tolist() for x in a] == [x.tolist() for x in b] and hw.read_sets([0]) == other.read_sets([0])
    hw.reset()
    with pytest.raises(ValueError, match="the gather is stale"):              # (one reset, not two)
        hw.step_resident(g, paths1, True, 1e-3, 0)
