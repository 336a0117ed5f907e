"""tests/tips_utils.py -- the sequential statement of po_layout_tips, the round scheme the kernels use and the
node-order rule of po_layout_edges -- against every case of tests/golden/tips_cases.npz, which the reference's own
remove_incoming_tips / remove_outgoing_tips / make_symmetric / clean_graph produced (tests/golden/make_tips_golden.py)."""
import numpy as np
import pytest

import layout_utils as lu
import reduce_utils as ru
import tips_utils as tu
from oracle import layout_oracle as lo
from phasm_amd.io import gfa

GOLDEN = tu.load_golden()
CASES = GOLDEN["cases"]
REDUCE = {c["name"]: c for c in ru.load_golden()["cases"]}
_STAGE1 = {}
ROUNDS_MAX_CANDIDATES = 700


def stage1(c):
    """(rows, node lengths, stage-1 edges in insertion order) of a text case, once per case."""
    if c["name"] not in _STAGE1:
        names, lengths, rows = gfa.read_gfa2_rows(tu.case_text(c).splitlines(True))
        L = lu.node_lengths(lengths)
        got = lo.layout_sequential(rows, L, **c["params"])["edges"]
        s1 = np.array([[u, v, w, o] for (u, v), (w, o) in got.items()], dtype=np.int64).reshape(-1, 4)
        _STAGE1[c["name"]] = (rows, L, s1)
    return _STAGE1[c["name"]]


def input_edges(c, r):
    """The edges one recorded application started from, ordered by (u, v) as the golden's flags are."""
    if c.get("direct"):
        e = np.asarray(c["edges"], dtype=np.int64).reshape(-1, 4)
    else:
        e = stage1(c)[2]
        if r["fuzz"] is not None:        # the reduction as the reduce goldens record it (the reference's own)
            rc = REDUCE[c["reduce_case"]] if "reduce_case" in c else None
            o = tu.by_uv(e)
            if rc is not None:
                f = ru.unpack_flags(rc["results"][str(r["fuzz"])]["flags_by_uv"], len(e))
            else:
                f = ru.reduce_edges(e, r["fuzz"])[o]
            e = e[o][f == 0]
    e = e[tu.by_uv(e)]
    assert len(e) == r["n_in"]
    return e


def check(e, order, L, B, rec, flags_key="flags", left_key="order_left"):
    flags, left, st = tu.remove_tips(e, order, L, B)
    assert np.array_equal(flags, ru.unpack_flags(rec[flags_key], len(e)))
    assert left == rec[left_key]
    want = rec if flags_key == "flags" else rec["second"]
    for k in ("n_in_tip_edges", "n_out_tip_edges", "n_asymmetric", "n_isolated_nodes", "n_candidates_in", "n_candidates_out", "n_nodes"):
        assert st[k] == want[k], k
    assert st["n_edges_out"] == want["n_kept"] and ru.edge_digest(e[flags == 0]) == want["kept_sha256"]
    # the round scheme, candidates in two scrambled orders.  (In plain Python a round costs a walk per unresolved
    # candidate, and the hubs settle one candidate per round: the generator held the scheme to those cases when it wrote
    # the file, and tests/test_tips_host_emulation.py runs the kernels themselves on them.)
    if st["n_candidates_in"] + st["n_candidates_out"] <= ROUNDS_MAX_CANDIDATES:
        for seed in (3, 4):
            rf, r_in, r_out = tu.remove_tips_rounds(e, order, L, B, seed)
            assert np.array_equal(rf, np.where(flags == 3, 0, flags))
            assert max(r_in, r_out) <= GOLDEN["branch_totals"]["max_rounds"]
    return e[flags == 0], left


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_statement_and_round_scheme_equal_the_reference(case):
    for r in case["results"]:
        e = input_edges(case, r)
        kept, left = check(e, case["order"], r["L"], r["B"], r)
        if "second" in r:                # applied to its own output, with the reference's default of 5000 bases
            assert r["second"]["B"] == tu.DEFAULT_B and r["second"]["n_in"] == len(kept)
            check(kept, left, r["second"]["L"], r["second"]["B"], r, "flags2", "order_left2")


TEXT_CASES = [c for c in CASES if not c.get("direct")]


@pytest.mark.parametrize("case", TEXT_CASES, ids=[c["name"] for c in TEXT_CASES])
def test_node_order_rule_equals_the_reference_graph_order(case):
    rows, L, s1 = stage1(case)
    order = tu.node_order(rows.tolist(), L, **case["params"])
    assert order == case["order"]
    assert set(s1[:, :2].reshape(-1).tolist()) <= set(order)


def test_every_branch_is_taken_and_some_nodes_own_no_edge():
    for k, v in GOLDEN["branch_totals"].items():
        assert v > 0, k
    assert set(tu.BRANCHES) <= set(GOLDEN["branch_totals"])
    edgeless = 0
    for c in TEXT_CASES:
        s1 = stage1(c)[2]
        edgeless += len(set(c["order"]) - set(s1[:, :2].reshape(-1).tolist())) > 0
    assert edgeless > 10                 # nodes that entered through a row to a read found contained later


def test_the_shared_junction_depends_on_the_row_order():
    """a0 -> a1 -> J and b0 -> J: chain A first takes (a0, a1), (a1, J) and their mirrors and leaves b0 -> J; chain B
    first takes (b0, J) and its mirror only."""
    got = {}
    for name in ("junction_a_first", "junction_b_first"):
        c = next(x for x in CASES if x["name"] == name)
        r = c["results"][0]
        e = input_edges(c, r)
        f = ru.unpack_flags(r["flags"], len(e))
        got[name] = {(int(u), int(v)): int(x) for (u, v), x in zip(e[:, :2].tolist(), f) if x}
        assert r["order_sensitive"]
    assert got["junction_a_first"] == {(0, 2): 1, (2, 6): 1, (3, 1): 2, (7, 3): 2}
    assert got["junction_b_first"] == {(4, 6): 1, (7, 5): 2}
    assert sum(c["results"][0]["order_sensitive"] for c in CASES) >= 5


def test_the_selfish_cases_bring_self_loops_flips_and_two_cycles_through_stage_1():
    """Reads aligned with themselves and with their own reverse strand, from GFA text: the shapes a tip walk could
    return through, in the cases the device runs (tests/test_gpu_tips.py)."""
    cases = [c for c in TEXT_CASES if c["name"].startswith("selfish_")]
    assert len(cases) >= 3
    for c in cases:
        uv = {(int(u), int(v)) for u, v in stage1(c)[2][:, :2].tolist()}
        assert sum(u == v for u, v in uv) >= 4                                  # (x, x) and (x^1, x^1)
        assert sum(u == v ^ 1 for u, v in uv) >= 2                              # (x, x^1), its own twin
        assert sum((v, u) in uv and u >> 1 != v >> 1 for u, v in uv) >= 4       # x -> y -> x
        assert any(r["n_in_tip_edges"] and r["n_out_tip_edges"] for r in c["results"])


def test_comb_teeth_meet_the_base_bound_at_every_length_bound():
    """One-edge teeth of B - 1, B and B + 1 bases: at L = 1 and L = 4 the first two go and the third stays; at L = 0
    nothing is a tip."""
    for L, want in ((0, 0), (1, 1), (4, 1)):
        c = next(x for x in CASES if x["name"] == "comb_%d" % L)
        r = c["results"][0]
        e = input_edges(c, r)
        f = ru.unpack_flags(r["flags"], len(e))
        for w, gone in ((tu.DEFAULT_B - 1, want), (tu.DEFAULT_B, want), (tu.DEFAULT_B + 1, 0)):
            teeth = f[e[:, 2] == w]
            assert len(teeth) == 4 and (teeth != 0).all() == bool(gone) and (teeth != 0).any() == bool(gone), (L, w)


@pytest.mark.parametrize("argv", [["-t", "-1"], ["-t", str(2**32)], ["--max-tip-length-bases", str(2**31)], ["-t", "four"]])
def test_cli_rejects_tip_bounds_that_do_not_fit(argv, capsys):
    from phasm_amd import cli
    with pytest.raises(SystemExit) as err:
        cli.main(["layout-edges", "overlaps.gfa", "--remove-tips"] + argv)
    assert err.value.code == 2 and "layout-edges: error: argument" in capsys.readouterr().err
