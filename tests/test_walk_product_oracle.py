"""The product's walk without a GPU: every golden walk of tests/golden/walk_cases.npz (the reference's own ``phase()``) through
``phasing.phase_chain`` on ``HostScorer`` / ``HostIndex`` / ``HostWalk`` with ``choose`` = the first of the list -- arms, ``broke``,
``fell_back``, ``n_cands_in``, survivors, every yield, the final prune and the end state equal the recording.  The bubbles go in
twice: as recorded, and as ``chain_bubbles_input`` builds them from ``HostPaths`` on the walk's edges."""
import math

import numpy as np
import pytest

import walk_product_utils as wp
import walk_utils as wu
from phasm_amd import phasing

WALKS = wu.load_golden()["walks"]
NAMES = [w["name"] for w in WALKS]


def host(walk):
    src = phasing.HostIndex(wu.lengths_of(walk))
    return phasing.HostScorer(), src, src.phase_index(wu.rows_of(walk))


@pytest.mark.parametrize("how", ["recorded", "built"])
@pytest.mark.parametrize("name", NAMES)
def test_phase_chain_on_the_host_equals_the_walk(name, how):
    walk = next(w for w in WALKS if w["name"] == name)
    bubbles = wp.recorded_bubbles(walk) if how == "recorded" else wp.built_bubbles(walk)
    if how == "built":
        for got, want in zip(bubbles, wp.recorded_bubbles(walk)):
            assert (got["entrance"], got["exit"], [list(p) for p in got["paths"]], got["preds"]) == \
                   (want["entrance"], want["exit"], want["paths"], want["preds"])
            assert sorted(got["interior_reads"]) == sorted(want["interior_reads"]) and sorted(got["interior_nodes"]) == sorted(want["interior_nodes"])
        assert len(bubbles) == len(walk["bubbles"])
    sc, src, index = host(walk)
    hw = phasing.HostWalk(sc, walk["params"]["ploidy"])
    raw, by_branch = [], []
    got, blocks = wp.run_product(walk, sc, src, index, hw, bubbles=bubbles, raw=raw)
    wu.same_trace(got, walk, walk, optional=wp.OPTIONAL)
    wp.check_blocks(blocks, got)
    assert got[2]["n_cands"] == walk["state"]["n_cands"] and got[2]["cands"] == walk["state"]["cands"]
    # the same scorer through bubble_from_relevant: the same bytes at every step
    wu.run_arrays(walk, sc, src, index, raw=by_branch)
    assert raw == by_branch


def one_bubble(aln_read, om=100):
    """A chain of one bubble with two one-read paths (reads 2 and 4) between reads 0 and 6, and one read outside the graph (8)
    that aligns to ``aln_read`` over bases 10..60."""
    lengths = [3000, 3000, 3000, 3000, om]
    src = phasing.HostIndex(np.repeat(lengths, 2))
    index = src.phase_index(np.asarray([[8, aln_read, 10, 60, 0, 50]]))
    bubbles = [{"entrance": 0, "exit": 6, "paths": [(0, 2, 6), (0, 4, 6)], "interior_nodes": [2, 4], "interior_reads": [2, 4], "preds": []}]
    return src, index, bubbles


def test_a_start_of_block_bubble_that_keeps_nothing_raises():
    src, index, bubbles = one_bubble(2)
    sc = phasing.HostScorer()
    with pytest.raises(ValueError, match=r"bubble 0 \(0 \.\. 6\) keeps no candidate even as the start of a block"):
        list(phasing.phase_chain(sc, src, index, bubbles, lambda x: [x], 2, 0, 4, 10.0, 0.1, walk=phasing.HostWalk(sc, 2), choose=wp.first))
    blocks = list(phasing.phase_chain(sc, src, index, bubbles, lambda x: [x], 2, 0, 4, 1e-3, 0.1, walk=phasing.HostWalk(sc, 2), choose=wp.first))
    assert len(blocks) == 1 and blocks[0].include_last and blocks[0].haplotypes[0][0] == 0 and blocks[0].haplotypes[0][-1] == 6


def test_best_returns_everyone_at_its_early_returns():
    sc = phasing.HostScorer()
    hw = phasing.HostWalk(sc, 2)
    assert hw.best() == ([0], -math.inf)                                  # a fresh walk
    src, index, bubbles = one_bubble(2)
    rel = phasing.relevant_reads(src, index, [2, 4], [], [], [], True, 0)
    cand, ext, rl = hw.step(rel, [[2], [4]], True, 0.0, 0, levels=[0.0], max_candidates=1)
    assert len(rl) == 1 and hw.info()["n_cands"] == 1 and hw.best()[0] == [0] and hw.best()[1] == rl[0]   # one candidate
    hw.reset()
    far = phasing.relevant_reads(src, index, [2, 4], [], [], [], True, 0)
    far.aln_a0[:], far.aln_a1[:] = 70, 60                                 # no overlap: every rl is -inf, threshold 0 keeps them
    cand, ext, rl = hw.step(far, [[2], [4]], True, 0.0, 0)
    assert len(rl) == 3 and all(x == -math.inf for x in rl) and hw.best() == ([0, 1, 2], -math.inf)


def test_a_peek_leaves_the_walk_as_it_was():
    walk = next(w for w in WALKS if w["name"] == "straight")
    sc, src, index = host(walk)
    hw = phasing.HostWalk(sc, 2)
    b = wp.recorded_bubbles(walk)[0]
    rel = phasing.relevant_reads(src, index, b["interior_reads"], [], [], b["preds"], True, 3)
    path_reads = [list(p[1:-1]) for p in b["paths"]]
    first = hw.step(rel, path_reads, True, 1e-3, 3)
    assert hw.info()["depth"] == 1
    b = wp.recorded_bubbles(walk)[1]
    rel = phasing.relevant_reads(src, index, b["interior_reads"], wp.recorded_bubbles(walk)[0]["interior_reads"], rel.cur_aligning.tolist(),
                                 b["preds"], False, 3)
    everyone = list(range(hw.info()["n_cands"]))
    before = (hw.info(), hw.history(everyone).tolist(), hw.read_sets(everyone))
    peek = hw.step(rel, [list(p[1:-1]) for p in b["paths"]], False, 1e-3, 3, advance=False)
    assert len(peek[0]) and (hw.info(), hw.history(everyone).tolist(), hw.read_sets(everyone)) == before and len(first[0]) == len(everyone)
    with pytest.raises(ValueError, match="start_of_block is not the walk's"):
        hw.step(rel, path_reads, True, 1e-3, 3)
