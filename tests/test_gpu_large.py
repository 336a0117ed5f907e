"""po_phase_large on the device (``ExactOverlapper.phase_paths_resident`` -> ``DevicePaths.score_large``) against
tests/golden/large_cases.npz -- the reference's ``phase_large_bubble``, run unmodified by tests/golden/make_large_golden.py: the
best list exactly, every score within ``table_tol``; for the bubbles of up to 64 paths the scores byte for byte those of
``score_paths`` through po_phase_branch on the same handle; the ranged path copy against po_paths_copy; a bubble with more paths
than k_lg_score has workgroups against the numpy twin; a bubble of 65 536 paths of which only the winner comes home; and the
`phase` command on a chain with a 65-path bubble between two ordinary ones."""
import os
import re

import numpy as np
import pytest
import torch

import large_utils as lu
import phase_utils as pu
import walk_product_utils as wp
import walk_utils as wu
from phasm_amd import phasing

pytestmark = pytest.mark.gpu

CASES = lu.cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_cases_through_po_phase_large(case):
    order, edges = lu.graph_inputs(case)
    ov, g = lu.device_graph(order, edges)
    home = ov.phase_paths(g, case["max_paths"])                     # everything on the host, through po_paths_copy
    paths = ov.phase_paths_resident(g, case["max_paths"])
    g.free()
    b, rel, reads_of = case["bubble"], lu.rel_of(case), lu.reads_of_node(case)
    assert paths.bubbles.tobytes() == home.bubbles.tobytes() and paths.bubble_path_off.tolist() == home.bubble_path_off.tolist()
    assert paths.inside_nodes.tolist() == home.inside_nodes.tolist() and paths.pred_weight.tolist() == home.pred_weight.tolist()
    for x in range(len(home)):
        assert paths.paths_of(x) == home.paths_of(x) and paths.interior_of(x) == home.interior_of(x) and paths.preds_of(x) == home.preds_of(x)
    n_listed = len(home.path_off) - 1
    for first, count in ((0, n_listed), (1, n_listed - 1), (n_listed - 1, 1), (n_listed // 2, min(3, n_listed - n_listed // 2)), (n_listed, 0)):
        off, nodes = paths._range(first, count)
        lo, hi = int(home.path_off[first]), int(home.path_off[first + count])
        assert (off + lo).tolist() == home.path_off[first:first + count + 1].tolist() and nodes.tolist() == home.path_nodes[lo:hi].tolist()
    best, best_scores, scores = paths.score_large(b, rel, reads_of, case["ploidy"], want_scores=True)
    st = paths.large_stats()
    lu.check_scores(scores.tolist(), case)
    assert best == case["ref"]["best"] and best_scores.tolist() == [scores[p] for p in best]
    assert paths.path_of(b, best[0]) == home.paths_of(b)[best[0]]
    assert (st["n_paths"], st["n_inside"], st["n_reads"]) == (len(scores), len(home.interior_of(b)), len(case["overlap_max"]))
    assert st["max_path_nodes"] == max(len(p) for p in home.paths_of(b))
    again, again_scores, none = paths.score_large(b, rel, reads_of, case["ploidy"])
    assert again == best and again_scores.tobytes() == best_scores.tobytes() and none is None
    if len(scores) <= 64:
        bubble = phasing.bubble_from_relevant(rel, 1, [[r for n in p[1:-1] for r in reads_of(n)] for p in home.paths_of(b)], [[[]]])
        assert scores.tobytes() == phasing.score_paths(ov, bubble).tobytes()
    print("%s: %d paths, %d reads: %.3f ms (intervals %.3f, score %.3f, best %.3f)" % (
        case["name"], st["n_paths"], st["n_reads"], st["ms_total"], st["ms_intervals"], st["ms_score"], st["ms_best"]))
    paths.close()
    ov.close()


def grid_cap():
    """The most workgroups k_lg_score is launched with, as the library's source states it: a number per compute unit."""
    src = open(os.path.join(wu.ROOT, "phasm_amd", "csrc", "c_api.hip")).read()
    per_cu = int(re.search(r"uint32_t large_grid_cap\(const po_handle\* h\) \{ return \(uint32_t\)h->n_cu \* (\d+); \}", src).group(1))
    return per_cu * torch.cuda.get_device_properties(0).multi_processor_count


def series_bubble(k, bypass, lanes=1):
    b = lu.Builder()
    b.large(b.node(), k, arm=0, bypass=bypass, lanes=lanes)
    edges = lu.pp._w(b.edges)
    return lu.pp.first_seen(edges), [list(e) for e in edges]


def test_more_paths_than_workgroups_against_the_twin():
    order, edges = series_bubble(13, True)                           # 8 193 paths, one of them without an interior
    ov, g = lu.device_graph(order, edges)
    paths = ov.phase_paths_resident(g, 1 << 20)
    g.free()
    n_paths = int(paths.bubbles["n_paths"][0])
    assert len(paths) == 1 and n_paths == 8193 > grid_cap()
    rel, reads_of = lu.simple_rel(paths.interior_of(0), 257, 5)
    best, best_scores, scores = paths.score_large(0, rel, reads_of, 8, want_scores=True)
    twin = phasing.HostResidentPaths(phasing.HostPaths(edges, order).phase_paths(None, 1 << 20))
    want_best, _, want = twin.score_large(0, rel, reads_of, 8, want_scores=True)
    assert len(scores) == 8193 and scores[-1] == 0.0 and twin.paths_of(0)[-1] == (order[0], paths.bubbles["exit"][0])
    worst = max(abs(g_ - w) * 257 / pu.table_tol(w * 257, 257) for g_, w in zip(scores.tolist(), want.tolist()))
    assert worst <= 1.0, worst
    top = sorted(want.tolist(), reverse=True)[:9]
    if all((a - b_) * 257 > 4 * pu.table_tol(a * 257, 257) for a, b_ in zip(top, top[1:])):
        assert best == want_best
    assert best == phasing.best_paths(scores, 8) and best_scores.tolist() == [scores[p] for p in best]
    paths.close()
    ov.close()


def test_65536_paths_of_which_the_winner_comes_home():
    order, edges = series_bubble(15, False, lanes=2)                 # two lanes of 15 diamonds in series between one pair of ends
    ov, g = lu.device_graph(order, edges)
    paths = ov.phase_paths_resident(g, 1 << 20)
    g.free()
    inside = paths.interior_of(0)
    assert int(paths.bubbles["n_paths"][0]) == 65536 and len(paths.path_nodes) == 0 and paths.n_listed_paths == 65536
    rel, reads_of = lu.simple_rel(inside, 64, 9)
    best, best_scores, none = paths.score_large(0, rel, reads_of, 4)
    st = paths.large_stats()
    assert none is None and len(best) == 4 == len(set(best)) and all(0 <= p < 65536 for p in best)
    assert (st["n_paths"], st["n_inside"], st["n_reads"], st["max_path_nodes"]) == (65536, len(inside), 64, 2 + 1 + 2 * 15)
    assert best_scores.tolist() == sorted(best_scores.tolist(), reverse=True)
    # the winner's score from its node tuple alone, by the numpy twin
    winner = paths.path_of(0, best[0])
    node_off, node_ids = phasing.large_node_lists(rel, inside, reads_of)
    want = phasing.host_score_large(rel, node_off, node_ids, inside, [winner])[0]
    assert winner[0] == order[0] and len(winner) == 33 and abs(best_scores[0] - want) * 64 <= pu.table_tol(want * 64, 64)
    # once more on the same handle: the same bits, and the best list is the stable descending order of all the scores
    again, again_scores, scores = paths.score_large(0, rel, reads_of, 4, want_scores=True)
    _, _, third = paths.score_large(0, rel, reads_of, 4, want_scores=True)
    assert again == best and again_scores.tobytes() == best_scores.tobytes() and scores.tobytes() == third.tobytes()
    assert best == phasing.best_of_scores(scores, 4) and best_scores.tolist() == scores[best].tolist()
    print("65 536 paths, 64 reads: %.3f ms (intervals %.3f, score %.3f, best %.3f)" % (st["ms_total"], st["ms_intervals"], st["ms_score"], st["ms_best"]))
    paths.close()
    ov.close()


def test_phase_end_to_end_with_a_65_path_bubble(tmp_path):
    """`phase` on the files of the golden's walk: a ``largebubble`` entry with the sequence ``HostSpeller`` spells for the
    reference's winner, between the haploblocks the host walk yields; with ``--max-listed-paths 64`` the command names the option."""
    from phasm_amd import cli
    case = next(c for c in CASES if "walk" in c)
    walk = case["walk"]
    p = walk["params"]
    hp = lu.host_paths(case)
    src, sc = phasing.HostIndex(wu.lengths_of(walk)), phasing.HostScorer()
    turns = []
    blocks = list(phasing.phase_chain(sc, src, src.phase_index(wu.rows_of(walk)),
                                      phasing.chain_bubbles_input(hp, 0, wp.reads_of_node(walk), resident_above=64), wp.reads_of_node(walk),
                                      p["ploidy"], p["min_spanning_reads"], p["max_bubble_size"], p["threshold"], p["prune_factor"],
                                      p["max_candidates"], p["max_prune_rounds"], p["prune_step_size"], walk=phasing.HostWalk(sc, p["ploidy"]),
                                      choose=wp.first, on_step=turns.append))
    assert [b.from_large_bubble for b in blocks] == [False, True, False]
    assert blocks[1].haplotypes[0] == list(hp.paths_of(1)[case["ref"]["best"][0]])            # the reference's winner
    recorded = dict(walk, trace=[{"yields": t["yields"]} for t in turns[:-1]], final={"yields": turns[-1]["yields"]})
    fasta, aln, graph, node_name = wp.write_chain_files(walk, str(tmp_path))
    out = str(tmp_path / "out.fasta")
    argv = ["phase", "-p", str(p["ploidy"]), "-s", str(p["min_spanning_reads"]), "-b", str(p["max_bubble_size"]), "-t", repr(p["threshold"]),
            "-d", repr(p["prune_factor"]), "-c", str(p["max_candidates"]), "-r", str(p["max_prune_rounds"]), "-S", repr(p["prune_step_size"]),
            "--seed", "7", "-o"]
    assert cli.main(argv + [out, fasta, aln, graph]) == 0
    got, want = wp.read_fasta_entries(out), wp.expected_fasta(recorded, graph, node_name)
    assert [n for n, _ in got] == [n for n, _ in want] and [n for n, _ in got].count("chain0.largebubble1") == 1
    assert dict(got)["chain0.largebubble1"] == dict(want)["chain0.largebubble1"]
    block = lambda entries: sorted((n.rsplit(".", 1)[0], s) for n, s in entries)   # noqa: E731  (a tie of two candidates: slots in either order)
    assert block(got) == block(want)
    with pytest.raises(SystemExit, match="bubble 1 has 65 paths, more than --max-listed-paths 64"):
        cli.main(argv + [str(tmp_path / "none.fasta"), "--max-listed-paths", "64", fasta, aln, graph])
