"""tests/diamond_utils.py -- the sequential statement of po_layout_diamonds, the round scheme the kernels use and the
composition of the whole cleaning chain -- against every application of tests/golden/diamond_cases.npz, which the
reference's own remove_diamond_tips (and, for the chain, its remove_transitive_edges / remove_tips / make_symmetric /
clean_graph around it) produced (tests/golden/make_diamond_golden.py)."""
import numpy as np
import pytest

import diamond_utils as du
import reduce_utils as ru
import tips_utils as tu
from test_tips_oracle import REDUCE, stage1

GOLDEN = du.load_golden()
CASES = GOLDEN["cases"]
TEXT_CASES = [c for c in CASES if not c.get("direct")]
_TEXT = {}


def case_stage1(c):
    """(rows, node lengths, stage-1 edges in insertion order) of a text case: the cases of tips_cases.npz through the
    cache of tests/test_tips_oracle.py, the union cases of this file on their own."""
    if c.get("synth", {}).get("kind") != "union":
        return stage1(c)
    if c["name"] not in _TEXT:
        import layout_utils as lu
        from oracle import layout_oracle as lo
        from phasm_amd.io import gfa
        _, lengths, rows = gfa.read_gfa2_rows(du.case_text(c).splitlines(True))
        L = lu.node_lengths(lengths)
        got = lo.layout_sequential(rows, L, **c["params"])["edges"]
        _TEXT[c["name"]] = (rows, L, np.array([[u, v, w, o] for (u, v), (w, o) in got.items()], dtype=np.int64).reshape(-1, 4))
    return _TEXT[c["name"]]


def reduce_flags(c, s1):
    """Flags of the reduction at the stage fuzz per stage-1 edge, in the order of s1: the reference's own where
    reduce_cases.npz records them, else the restatement that file pins."""
    rc = REDUCE.get(c.get("reduce_case"))
    if rc is not None and str(du.STAGE_FUZZ) in rc["results"]:
        o = tu.by_uv(s1)
        f = np.zeros(len(s1), dtype=np.uint8)
        f[o] = ru.unpack_flags(rc["results"][str(du.STAGE_FUZZ)]["flags_by_uv"], len(s1))
        return f
    return ru.reduce_edges(s1, du.STAGE_FUZZ)


def input_edges(c, r):
    """The edges one recorded application started from, ordered by (u, v) as the golden's flags are."""
    if c.get("direct"):
        e = np.asarray(c["edges"], dtype=np.int64).reshape(-1, 4)
    else:
        e = case_stage1(c)[2]
        if r["stage"] == "b":
            e = e[reduce_flags(c, e) == 0]
            f, left, _ = tu.remove_tips(e, c["order"], du.STAGE_L, du.STAGE_B)
            assert left == r["order_before"]
            e = e[f == 0]
    e = e[tu.by_uv(e)]
    assert len(e) == r["n_in"]
    return e


def check(e, rec):
    flags, left, st = du.remove_diamond_tips(e, rec["order_before"])
    assert np.array_equal(flags, ru.unpack_flags(rec["flags"], len(e)))
    assert left == rec["order_left"]
    assert (st["n_candidates"], st["n_diamonds"], st["n_nodes"], st["n_edges_out"]) == \
           (rec["n_candidates"], rec["n_diamonds"], rec["n_nodes"], rec["n_kept"])
    assert st["n_nodes_removed"] == 2 * rec["n_diamonds"] and st["n_edges_in"] - st["n_edges_out"] == 3 * rec["n_diamonds"]
    assert ru.edge_digest(e[flags == 0]) == rec["kept_sha256"]
    worst = 0
    for seed in (4, 5):                  # candidates in two scrambled orders (the generator used three others)
        rf, rounds = du.remove_diamond_tips_rounds(e, rec["order_before"], seed)
        assert np.array_equal(rf, flags)
        worst = max(worst, rounds)
    assert (worst > 0) == (rec["n_candidates"] > 0) and worst <= GOLDEN["branch_totals"]["max_rounds"]
    rev, _, _ = du.remove_diamond_tips(e, rec["order_before"][::-1])
    assert (not np.array_equal(rev, flags)) == rec["order_sensitive"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_statement_and_round_scheme_equal_the_reference(case):
    assert [r["stage"] for r in case["results"]] == (["a"] if case.get("direct") else ["a", "b"])
    for r in case["results"]:
        check(input_edges(case, r), r)


@pytest.mark.parametrize("case", TEXT_CASES, ids=[c["name"] for c in TEXT_CASES])
def test_the_restated_chain_equals_the_reference(case):
    s1 = case_stage1(case)[2]
    removed_by, kept, left, stats = du.clean_chain(s1, case["order"], reduce_flags=reduce_flags(case, s1))
    ch = case["chain"]
    assert np.array_equal(removed_by[tu.by_uv(s1)], case["removed_by"])
    assert left == ch["order_left"] and len(kept) == ch["n_kept"] and len(s1) == ch["n_stage1"]
    assert ru.edge_digest(ru.sort_edges(kept)) == ch["kept_sha256"]
    counts = du.chain_counts(stats)
    assert counts == {k: ch[k] for k in counts}
    # the second tip block counts the nodes the diamonds isolated, and starts from the order the diamonds left
    assert stats[3]["n_nodes"] == stats[2]["n_nodes"] - stats[2]["n_nodes_removed"] == len(case["results"][1]["order_left"])


def test_every_branch_is_taken():
    totals = GOLDEN["branch_totals"]
    assert set(du.BRANCHES) <= set(totals)
    for k, v in totals.items():
        assert v > 0, k
    # what the text cases bring on their own
    assert GOLDEN["text_totals"]["diamonds"] >= 784 and GOLDEN["text_totals"]["order_sensitive_cases"] >= 3
    assert sum(r["n_candidates"] for c in TEXT_CASES for r in c["results"]) >= 1197
    sensitive = {c["name"] for c in TEXT_CASES if c["results"][1]["order_sensitive"]}
    assert {"reduced_hub_1023", "reduced_hub_1025", "reduced_stagger_1100"} <= sensitive
    every = [c["name"] for c in TEXT_CASES if set(range(1, 11)) <= set(c["removed_by"].tolist())]
    assert len(every) == totals["chains_with_every_code"] > 0


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def test_the_shared_predecessor_depends_on_the_node_order():
    """Z->Q, Q->E1, Q->E2, X->P, P->E1, R->E2, R->Y: E1 first takes E1 and P, which leaves Q with one out-edge -- a pred1
    for E2, whose R is a gt1: Q and E2 go too.  E2 first finds Q and R both gt1, and only E1's diamond is one."""
    got = {}
    for name in ("direct_q_e1_first", "direct_q_e2_first"):
        c = by_name(name)
        r = c["results"][0]
        e = input_edges(c, r)
        f = ru.unpack_flags(r["flags"], len(e))
        got[name] = {(int(u), int(v)): int(x) for (u, v), x in zip(e[:, :2].tolist(), f) if x}
        assert r["order_sensitive"]
    assert got["direct_q_e1_first"] == {(2, 4): 1, (10, 4): 1, (8, 10): 2, (2, 6): 1, (12, 6): 1, (0, 2): 2}
    assert got["direct_q_e2_first"] == {(2, 4): 1, (10, 4): 1, (8, 10): 2}


@pytest.mark.parametrize("name,diamonds,rounds", [("fan_2", 1, 2), ("fan_3", 2, 3), ("fan_64", 63, 64), ("fan_65", 64, 65),
                                                  ("fan_3_last_gt1", 3, 3), ("fan_65_last_gt1", 65, 65), ("fan_3_last_none", 2, 2)])
def test_a_fan_settles_one_end_node_per_round(name, diamonds, rounds):
    """K end nodes on one hub: each diamond takes one of the hub's out-edges, so the last end node finds the hub with
    out-degree 1 -- no gt1 (its own chain is a pred1 too), or, where its other predecessor is a gt1, a pred1 that goes."""
    r = by_name("direct_" + name)["results"][0]
    assert (r["n_diamonds"], r["rounds"]) == (diamonds, rounds)


@pytest.mark.parametrize("name,candidates,diamonds", [
    ("pp_is_gt1", 1, 1), ("pp_is_gt1_node0_pred1", 1, 1), ("both_pred1", 1, 0), ("both_gt1", 1, 0), ("pred1_in0", 1, 0),
    ("pred1_in2", 1, 0), ("gt1_self_loop", 1, 1), ("pp_two_cycle", 1, 1), ("pred_is_mirror", 1, 1), ("pred1_is_mirror", 1, 1),
    ("empty", 0, 0), ("nodes_without_edges", 0, 0), ("no_candidates", 0, 0)])
def test_direct_shapes(name, candidates, diamonds):
    c = by_name("direct_" + name)
    r = c["results"][0]
    assert (r["n_candidates"], r["n_diamonds"]) == (candidates, diamonds)
    assert len(r["order_left"]) == len(c["order"]) - 2 * diamonds


def test_removed_by_composes_the_four_flag_arrays():
    got = du.compose_removed_by([[0, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0], [1, 2, 3, 0, 0, 0, 0, 0, 0], [1, 2, 0, 0, 0, 0], [1, 2, 3, 0]])
    assert got.tolist() == [3, 1, 2, 4, 5, 6, 7, 8, 9, 10, 0]
