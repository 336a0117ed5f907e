"""The walk of a bubble chain with the candidates resident on the device (po_walk_*): every golden walk
through ``phasing.phase_chain`` on an ``ExactOverlapper`` with a ``DeviceWalk``, held to tests/golden/walk_cases.npz (the
reference's own ``phase()``) and, step by step and byte for byte, to the ``po_phase_branch`` route of tests/walk_utils.py
(``run_arrays``) on the same handle and index.  Sizes up, down and up again on one handle and ONE walk object (the stale-row check
of the ping-pong pair); a synthetic walk past what the goldens reach (a block of 20 and more bubbles, 8 and more words per slot,
100 and more candidates, a new_block in the middle) against ``run_arrays`` and ``HostWalk``; histories and read sets of one, two
and all candidates, a ``cap`` below the list at a step that advances, and ``po_phase_branch`` at a larger size between the
steps of a live walk."""
import numpy as np
import pytest

import phase_utils as pu
import walk_product_utils as wp
import walk_utils as wu
from phasm_amd import phasing
from phasm_amd.overlapper import ExactOverlapper
from test_gpu_walk import handle_for, indexed, shifted

pytestmark = pytest.mark.gpu

WALKS = wu.load_golden()["walks"]
NAMES = [w["name"] for w in WALKS]


def named(name):
    return next(w for w in WALKS if w["name"] == name)


def product_bytes(walk, ov, index, dw, bubbles=None):
    raw = []
    got, blocks = wp.run_product(walk, ov, ov, index, dw, bubbles=bubbles, raw=raw)
    return got, blocks, raw


@pytest.mark.parametrize("name", NAMES)
def test_every_golden_walk_on_a_device_walk(name):
    walk = named(name)
    ov = handle_for(walk)
    index = indexed(ov, walk)
    dw = ov.phase_walk(walk["params"]["ploidy"])
    got, blocks, raw = product_bytes(walk, ov, index, dw)
    wu.same_trace(got, walk, walk, optional=wp.OPTIONAL)
    wp.check_blocks(blocks, got)
    # the po_phase_branch route on the same handle and index: the same bytes at every step
    by_branch = []
    wu.run_arrays(walk, ov, ov, index, raw=by_branch)
    assert raw and raw == by_branch
    # a second time on the same walk object
    dw.reset()
    again, _, raw_again = product_bytes(walk, ov, index, dw)
    assert raw_again == raw and again[2] == got[2]
    dw.close()
    index.free()
    ov.close()


@pytest.mark.parametrize("order", [("grow_words", "break_and_shrink"), ("break_and_shrink", "grow_words")], ids="_then_".join)
def test_two_walks_back_to_back_on_one_handle_and_one_walk_object(order):
    """Rows that grow, shrink to a handful of reads and grow again in the same ping-pong pair: every step byte-equal to the
    walk on a fresh handle."""
    walks = [named(n) for n in order]
    fresh = []
    for walk in walks:
        ov = handle_for(walk)
        index = indexed(ov, walk)
        dw = ov.phase_walk(2)
        got, _, raw = product_bytes(walk, ov, index, dw)
        wu.same_trace(got, walk, walk, optional=wp.OPTIONAL)
        fresh.append((raw, got[2]["cands"]))
        dw.close()
        index.free()
        ov.close()
    ovs = ExactOverlapper()
    import relevant_utils as ru
    ru.add_reads(ovs, walks[0]["lengths"] + walks[1]["lengths"])
    dw = ovs.phase_walk(2)
    for walk, shift, (want, cands) in zip(walks, [0, 2 * len(walks[0]["lengths"])], fresh):
        moved = shifted(walk, shift)
        index = indexed(ovs, moved)
        dw.reset()
        got, _, raw = product_bytes(moved, ovs, index, dw)
        assert raw == want, "%s after %s on one walk object: the bytes of a step differ from those on a fresh handle" % (walk["name"], order[0])
        assert [[[x - shift for x in s] for s in c["read_sets"]] for c in got[2]["cands"]] == [c["read_sets"] for c in cands]
        index.free()
    dw.close()
    ovs.close()


# ---- a walk past what the goldens reach ------------------------------------------------------------------------------------------

LONG = dict(paths=[2] * 27, depth=6, span=12, window=3, noise=0.15, cuts=(5,), link=False)


def long_walk():
    """The first seed whose walk shows the sizes asked for on the HOST route, with the margins of ``walk_utils.margins_hold``
    (no log_rl within 4 tol of the threshold, of a prune level or of a tie), so that host and device decide alike.  The prune
    factor is a constant CALLABLE: every step then peeks first, which records the kept lists the margins are checked on."""
    params = wu._params(threshold=1e-3, prune_factor=["step", 0, 0.29, 0.29], max_candidates=120)
    for seed in range(1, 9):
        w = wu.synth(seed, params, **LONG)
        w["name"] = "long_%d" % seed
        w["bubbles"] = wp.built_bubbles(w)
        src = phasing.HostIndex(wu.lengths_of(w))
        w["trace"], w["final"], w["state"] = wu.run_arrays(w, phasing.HostScorer(), src, src.phase_index(wu.rows_of(w)))
        if properties(w) is None and wu.margins_hold(w) is None:
            return w
    raise AssertionError("no seed gives the walk")


def properties(w):
    """None when one block of the walk has 20 advanced bubbles, 8 words per slot at its end and 100 candidates at some step, and
    a new_block lies in the middle; else what is missing."""
    blocks, cur = [], []
    for s in w["trace"]:
        if s["broke"] or s["arm"] == "retry":
            blocks.append(cur)
            cur = []
        if s["arm"] == "advanced":
            cur.append(s)
    blocks.append(cur)
    if len(blocks) < 2 or not blocks[0]:
        return "no new_block in the middle"
    for blk in blocks:
        reads = set()
        for s in blk:
            reads |= set(w["bubbles"][s["bubble"]]["interior_reads"])
        if len(blk) >= 20 and (len(reads) + 31) // 32 >= 8 and max(s["n_cands_in"] for s in blk) >= 100:
            return None
    return "no block of 20 bubbles, 8 words and 100 candidates"


def test_a_long_walk_equals_the_branch_route_and_the_host_walk():
    walk = long_walk()                                    # (the properties and the margins: on the host, before the device)
    assert properties(walk) is None and wu.margins_hold(walk) is None
    ov = handle_for(walk)
    index = indexed(ov, walk)
    dw = ov.phase_walk(2)
    got, blocks, raw = product_bytes(walk, ov, index, dw, bubbles=walk["bubbles"])
    by_branch = []
    wu.run_arrays(walk, ov, ov, index, raw=by_branch)
    assert raw and raw == by_branch
    src = phasing.HostIndex(wu.lengths_of(walk))
    sc = phasing.HostScorer()
    hw = phasing.HostWalk(sc, 2)
    want, host_blocks = wp.run_product(walk, sc, src, src.phase_index(wu.rows_of(walk)), hw, bubbles=walk["bubbles"])
    assert [s["arm"] for s in got[0]] == [s["arm"] for s in want[0]]
    assert [(s.get("surv_cand"), s.get("surv_ext")) for s in got[0]] == [(s.get("surv_cand"), s.get("surv_ext")) for s in want[0]]
    assert [(b.haplotypes, b.read_sets, b.tie, b.include_last) for b in blocks] == [(b.haplotypes, b.read_sets, b.tie, b.include_last) for b in host_blocks]
    info = dw.info()
    assert info == hw.info() and info["depth"] >= 20 and ov.walk_stats()["words_per_slot"] >= 8
    everyone = list(range(info["n_cands"]))
    assert dw.history(everyone).tolist() == hw.history(everyone).tolist() and dw.read_sets(everyone) == hw.read_sets(everyone)
    assert dw.best()[0] == hw.best()[0]
    dw.close()
    index.free()
    ov.close()


def test_histories_read_sets_a_small_cap_and_a_larger_branch_call_in_between():
    """``grow_words`` step by step on a DeviceWalk and a HostWalk side by side (the golden's margins make both decide alike):
    only ONE entry of every step comes home, yet the state takes the whole list; between the steps ``po_phase_branch`` runs at
    a larger size on the same handle; histories and read sets of one, two and all candidates agree after every step."""
    walk = named("grow_words")
    p = walk["params"]
    big = next(c for c in pu.load_golden()["cases"] if c["name"] == "nb33_r64")
    ov = handle_for(walk)
    index = indexed(ov, walk)
    dw, sc = ov.phase_walk(2), phasing.HostScorer()
    hw = phasing.HostWalk(sc, 2)
    src = phasing.HostIndex(wu.lengths_of(walk))
    host_index = src.phase_index(wu.rows_of(walk))
    levels = phasing.prune_levels(p["prune_factor"], p["prune_step_size"], p["max_prune_rounds"])
    prev_graph, prev_aligning = set(), set()
    expand = wp.reads_of_node(walk)
    for b in wp.recorded_bubbles(walk):
        start = hw.start_of_block
        assert dw.start_of_block == start
        args = (b["interior_reads"], sorted(prev_graph), sorted(prev_aligning), b["preds"], start, p["min_spanning_reads"])
        rel = phasing.relevant_reads(ov, index, *args)
        path_reads = [[r for x in path[1:-1] for r in expand(x)] for path in b["paths"]]
        step = (path_reads, start, p["threshold"], p["min_spanning_reads"], levels, p["max_candidates"])
        want = hw.step(phasing.relevant_reads(src, host_index, *args), *step)
        before = dw.info()
        peek = dw.step(rel, *step, advance=False)
        assert dw.info() == before and [x.tolist() for x in peek[:2]] == [x.tolist() for x in want[:2]]
        got = dw.step(rel, *step, cap=1)
        assert len(got[0]) == 1 and (got[0][0], got[1][0]) == (want[0][0], want[1][0]) and got[2].tobytes() == peek[2][:1].tobytes()
        assert dw.info() == hw.info() and len(want[0]) > 1
        st = ov.walk_stats()
        assert (st["advanced"], st["n_cands_out"], st["depth"], st["n_block_reads"]) == (1, len(want[0]), hw.info()["depth"], hw.info()["n_block_reads"])
        pu.check_result(pu.result_of(ov, big), big["ref"], big)           # (the handle's phase scratch at another size)
        n = dw.info()["n_cands"]
        for cands in ([0], [n - 1, 0], list(range(n))):
            assert dw.history(cands).tolist() == hw.history(cands).tolist()
            assert dw.read_sets(cands) == hw.read_sets(cands)
        assert dw.best()[0] == hw.best()[0] and abs(dw.best()[1] - hw.best()[1]) <= pu.tol(hw.best()[1], 2, len(rel.rel_reads))
        with pytest.raises(ValueError, match="a candidate is not below"):
            dw.history([n])
        prev_graph |= set(b["interior_reads"])
        prev_aligning |= set(rel.cur_aligning.tolist())
    assert dw.info()["depth"] == len(walk["bubbles"])
    dw.reset()
    assert dw.info() == {"ploidy": 2, "n_cands": 1, "depth": 0, "start_of_block": 1, "n_block_reads": 0}
    assert dw.read_sets([0]) == [[[], []]] and dw.best() == ([0], -np.inf)
    dw.close()
    index.free()
    ov.close()


@pytest.mark.parametrize("name", ["ploidy3_rounds", "merged_nodes"])
def test_phase_end_to_end_writes_the_recorded_haplotypes(name, tmp_path):
    """`phase` on the files of a golden walk: the FASTA is what ``HostSpeller`` spells for the recorded yields.  The first
    walk (two new_blocks, ploidy 3) has no tie of more than one candidate, so the seed decides nothing; ``merged_nodes`` (F lines) ends in a tie of two
    candidates that differ in the order of their slots, so there the sequences of a block are compared as a sorted list."""
    from phasm_amd import cli
    walk = named(name)
    p = walk["params"]
    fasta, aln, graph, node_name = wp.write_chain_files(walk, str(tmp_path))
    out = str(tmp_path / "out.fasta")
    assert cli.main(["phase", "-p", str(p["ploidy"]), "-s", str(p["min_spanning_reads"]), "-b", str(p["max_bubble_size"]), "-t",
                     repr(p["threshold"]), "-d", repr(p["prune_factor"]), "-c", str(p["max_candidates"]), "-r", str(p["max_prune_rounds"]),
                     "-S", repr(p["prune_step_size"]), "--seed", "7", "-o", out, fasta, aln, graph]) == 0
    got, want = wp.read_fasta_entries(out), wp.expected_fasta(walk, graph, node_name)
    assert [n for n, _ in got] == [n for n, _ in want] and len(want) >= p["ploidy"]
    if name == "merged_nodes":
        block = lambda entries: sorted((n.rsplit(".", 1)[0], s) for n, s in entries)   # noqa: E731
        assert block(got) == block(want)
    else:
        assert got == want
