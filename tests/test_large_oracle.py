"""The numpy twin of po_phase_large (``phasing.HostResidentPaths.score_large``: the decomposition over the interior nodes, the
stable descending tie rule) against tests/golden/large_cases.npz -- the reference's ``phase_large_bubble``, run unmodified by
tests/golden/make_large_golden.py -- and, cut to 64 paths, against ``score_paths(HostScorer(), ...)``, the route through the
table of po_phase_branch; and the large arm of ``phase_chain`` at a bubble whose paths are not on the host."""
import numpy as np
import pytest

import large_utils as lu
import phase_utils as pu
import walk_product_utils as wp
import walk_utils as wu
from phasm_amd import phasing

CASES = lu.cases()
IDS = [c["name"] for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_twin_equals_the_reference(case):
    best, best_scores, scores = lu.twin_scores(case)
    lu.check_scores(scores.tolist(), case)
    assert best == case["ref"]["best"] and best_scores.tolist() == [scores[p] for p in best]
    assert best == phasing.best_paths(scores, case["ploidy"])
    again, _, none = lu.twin_scores(case, want_scores=False)
    assert again == best and none is None
    st = lu.host_paths(case)
    st.score_large(case["bubble"], lu.rel_of(case), lu.reads_of_node(case), 1)
    assert st.large_stats()["n_paths"] == len(scores) and st.large_stats()["n_reads"] == len(case["overlap_max"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cut_to_64_paths_the_twin_equals_the_table_route(case):
    hp, rel, reads_of = lu.host_paths(case), lu.rel_of(case), lu.reads_of_node(case)
    paths = hp.paths_of(case["bubble"])[:64]
    inside = hp.interior_of(case["bubble"])
    node_off, node_ids = phasing.large_node_lists(rel, inside, reads_of)
    got = phasing.host_score_large(rel, node_off, node_ids, inside, paths)
    bubble = phasing.bubble_from_relevant(rel, 1, [[r for n in p[1:-1] for r in reads_of(n)] for p in paths], [[[]]])
    want = phasing.score_paths(phasing.HostScorer(), bubble)
    R = len(case["overlap_max"])
    assert len(got) == len(want) == len(paths)
    for g, w in zip(got.tolist(), want.tolist()):
        assert abs(g - w) * R <= pu.table_tol(w * R, R), (g, w)


def test_the_cases_cover_what_the_kernel_branches_on():
    by = {c["name"]: c for c in CASES}
    assert {1, 255, 256, 257, 2048, 2049} <= {len(c["overlap_max"]) for c in CASES}
    assert {32, 33, 65} <= {len(c["b_reads"]) for c in CASES} and {64, 65, 66, 257} <= {len(c["ref"]["scores"]) for c in CASES}
    assert max(len(p) for p in lu.host_paths(by["long_path_300"]).paths_of(0)) - 2 > lu.CHUNK
    assert set(by["all_zero"]["ref"]["scores"]) == {0.0} and by["all_zero"]["ref"]["best"] == [0, 1]
    tie = by["tie_for_first"]["ref"]
    assert tie["scores"][tie["best"][0]] == tie["scores"][tie["best"][1]] and tie["best"][0] < tie["best"][1]
    assert by["winner_last"]["ref"]["best"][0] == len(by["winner_last"]["ref"]["scores"]) - 1
    assert len(by["p3_n_best_8_r1"]["ref"]["best"]) == 3 and by["p3_n_best_8_r1"]["ploidy"] == 8
    for name in ("second_of_four", "third_of_four"):
        assert int(lu.host_paths(by[name]).bubble_path_off[by[name]["bubble"]]) != 0
    assert any(a1 > om for c in CASES for r, om in enumerate(c["overlap_max"])
               for a1 in c["aln_a1"][c["aln_off"][r]:c["aln_off"][r + 1]])
    assert any(len(rs) > 1 for n, rs in by["p65_r255"]["node_reads"])


def test_bad_arguments_of_the_twin():
    case = CASES[0]
    hp = lu.host_paths(case)
    with pytest.raises(ValueError, match="n_best must be 1 to 8"):
        hp.score_large(case["bubble"], lu.rel_of(case), lu.reads_of_node(case), 9)
    empty = phasing.RelevantReads(*(np.zeros(0, np.uint32),) * 2, np.zeros(0, np.int32), np.zeros(1, np.uint32), np.zeros(0, np.uint32),
                                  np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint32))
    with pytest.raises(ZeroDivisionError):
        hp.score_large(case["bubble"], empty, lu.reads_of_node(case), 1)
    with pytest.raises(ValueError, match="no listed path"):
        hp.path_of(case["bubble"], 10**6)


# ---- phase_chain at a bubble whose paths are not on the host ----------------------------------------------------------------------

class StubScorer:
    """A bubble's scorer that answers from a list and notes what it was asked."""

    def __init__(self, best, scores, paths):
        self.best, self.scores, self.paths, self.asked, self.fetched = best, scores, paths, [], []

    def score_large(self, rel, reads_of_node, n_best, want_scores=False):
        self.asked.append((len(rel.rel_reads), n_best, want_scores))
        return self.best[:n_best], np.asarray([self.scores[p] for p in self.best[:n_best]]), (np.asarray(self.scores) if want_scores else None)

    def path_of(self, p):
        self.fetched.append(p)
        return self.paths[p]


def walk_and_bubbles():
    case = next(c for c in CASES if "walk" in c)
    walk = case["walk"]
    hp = lu.host_paths(case)
    return case, walk, hp


def run_chain(walk, bubbles, **kw):
    p = walk["params"]
    src = phasing.HostIndex(wu.lengths_of(walk))
    sc = phasing.HostScorer()
    turns = []
    blocks = list(phasing.phase_chain(sc, src, src.phase_index(wu.rows_of(walk)), bubbles, wp.reads_of_node(walk), p["ploidy"],
                                      p["min_spanning_reads"], p["max_bubble_size"], p["threshold"], p["prune_factor"], p["max_candidates"],
                                      p["max_prune_rounds"], p["prune_step_size"], walk=phasing.HostWalk(sc, p["ploidy"]), choose=wp.first,
                                      on_step=turns.append, **kw))
    return blocks, turns


def test_phase_chain_asks_the_scorer_of_a_bubble_without_paths():
    case, walk, hp = walk_and_bubbles()
    listed = phasing.chain_bubbles_input(hp, 0, wp.reads_of_node(walk))
    paths = listed[1]["paths"]
    stub = StubScorer(case["ref"]["best"], case["ref"]["scores"], paths)
    bubbles = [listed[0], {k: v for k, v in listed[1].items() if k != "paths"}, listed[2]]
    bubbles[1].update(n_paths=len(paths), scorer=stub)
    blocks, turns = run_chain(walk, bubbles)
    large = [t for t in turns if t.get("arm") == "large"]
    assert len(large) == 1 and large[0]["bubble"] == 1 and large[0]["best"] == case["ref"]["best"] and large[0]["winner"] == case["ref"]["best"][0]
    assert "scores" not in large[0]
    assert stub.asked == [(len(case["overlap_max"]), walk["params"]["ploidy"], False)] and stub.fetched == [case["ref"]["best"][0]]
    block = next(b for b in blocks if b.from_large_bubble)
    winner = paths[case["ref"]["best"][0]]
    assert block.haplotypes == [list(winner), []] and block.read_sets == [sorted(wu.node_reads(walk, winner[1:-1])), []]
    # with the scores asked for, and with "paths": None in place of no key
    bubbles[1]["paths"] = None
    stub.asked, stub.fetched = [], []
    _, turns = run_chain(walk, bubbles, large_scores=True)
    large = [t for t in turns if t.get("arm") == "large"]
    assert large[0]["scores"] == case["ref"]["scores"] and stub.asked[0][2] is True
    # the blocks around the large bubble are those of the walk that has every path on the host
    resident = phasing.chain_bubbles_input(hp, 0, wp.reads_of_node(walk), resident_above=64)
    assert resident[1]["paths"] is None and resident[1]["n_paths"] == 65 and resident[0]["paths"] == listed[0]["paths"]
    got, _ = run_chain(walk, resident)
    assert [b.haplotypes for b in got] == [b.haplotypes for b in blocks] and [b.read_sets for b in got] == [b.read_sets for b in blocks]
    assert len(got) == 3 and [b.from_large_bubble for b in got] == [False, True, False]


def test_a_bubble_without_paths_that_is_not_large_names_itself():
    case, walk, hp = walk_and_bubbles()
    bubbles = phasing.chain_bubbles_input(hp, 0, wp.reads_of_node(walk), resident_above=64)
    p = dict(walk["params"], max_bubble_size=100)
    with pytest.raises(ValueError, match="bubble 1 .* has 65 paths that are not on the host"):
        run_chain(dict(walk, params=p), bubbles)
