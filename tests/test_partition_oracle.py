"""tests/partition_utils.py -- the plain statement of po_layout_partition (Tarjan plus the rules) and the device's scheme run
synchronously -- against every application of tests/golden/partition_cases.npz (tests/golden/make_partition_golden.py: the
reference's partition_graph, unmodified, per weakly connected component of the reference's graphs at two stages and of the
direct cases), and ``layout.superbubble_partitions`` on outputs shaped as the device returns them."""
import numpy as np
import pytest

import components_utils as cu
import partition_utils as pu
from phasm_amd import _lib, layout
from test_components_oracle import CASES as COMPONENT_CASES, stage_inputs as component_stage_inputs

GOLDEN = pu.load_golden()
CASES = GOLDEN["cases"]
DIRECT = {name: (order, edges, n_ids) for name, order, edges, n_ids in pu.direct_inputs()}
_COMPONENTS = {c["name"]: c for c in COMPONENT_CASES}


def stage_inputs(case):
    """{stage: (edges [n, >=2], node order, n_ids)} of a golden case: a direct case's own, or the graphs of the text case at
    (b) after the cleaning chain and (c) after the merge, as tests/test_components_oracle.py rebuilds them."""
    name = case["name"]
    if case.get("direct"):
        order, edges, _ = DIRECT[name[len("direct_"):]]
        return {"a": (np.asarray(edges, dtype=np.int64).reshape(-1, 2), list(order), case["results"][0]["n_ids"])}
    return {k: v for k, v in component_stage_inputs(_COMPONENTS[name]).items() if k in ("b", "c")}


def check_input(edges, order, rec):
    e = cu.uv_of(edges)
    assert cu.digest(order, e[pu.by_uv(edges)]) == rec["in_sha256"], "the input differs from the generator's"


def as_device(res, weak, order, edges):
    """The restatement's arrays in the dataclasses the device route fills."""
    table = np.zeros(len(res["first_node"]), dtype=_lib.SCC_DTYPE)
    for k in _lib.SCC_DTYPE.names:
        table[k] = res[k]
    rank = {n: r for r, n in enumerate(order)}
    scc_of_edge = np.asarray([res["node_scc"][rank[int(u)]] for u in cu.uv_of(edges)[:, 0]], dtype=np.uint32)
    sccs = layout.StrongComponents(np.asarray(order, dtype=np.uint32), res["node_scc"].astype(np.uint32), res["node_flags"].astype(np.uint8),
                                   res["edge_class"].astype(np.uint8), scc_of_edge, table, {})
    ctable = np.zeros(len(weak["first_node"]), dtype=_lib.COMPONENT_DTYPE)
    for k in _lib.COMPONENT_DTYPE.names:
        ctable[k] = weak[k]
    comps = layout.Components(np.asarray(order, dtype=np.uint32), weak["node_component"].astype(np.uint32),
                              weak["edge_component"].astype(np.uint32), ctable, {})
    return sccs, comps


def test_one_parametrised_case_per_golden_case():
    text = [c["name"] for c in COMPONENT_CASES if not c.get("direct")]
    assert [c["name"] for c in CASES] == text + ["direct_" + n for n in DIRECT]
    t = GOLDEN["totals"]
    assert all(t[k] > 0 for k in t if k != "digest_records"), t   # every class, every flag bit, >= 2 iterations, trim after a peel


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_statement_and_device_scheme_equal_the_golden(case):
    stages = stage_inputs(case)
    assert [r["stage"] for r in case["results"]] == (["a"] if case.get("direct") else ["b", "c"])
    for r in case["results"]:
        edges, order, n_ids = stages[r["stage"]]
        check_input(edges, order, r)
        assert r["n_ids"] == n_ids
        weak = cu.weak_components(edges, order)
        plain, sync = pu.partition(edges, order), pu.partition_rounds(edges, order)
        for res in (plain, sync):
            pu.check_against_record(res, pu.reference_partitions(res, weak, edges, order), edges, r)
            rank = {n: i for i, n in enumerate(order)}
            # the numbering: SCC i starts at the i-th lowest-ranked first node, which is its lowest-ranked member
            first = [rank[int(f)] for f in res["first_node"]]
            assert first == sorted(first)
            assert all(first[c] <= i for i, c in enumerate(res["node_scc"].tolist()))
        st = sync["stats"]
        assert {k: st[k] for k in ("n_trimmed", "n_outer", "n_trim_rounds", "n_forward_rounds", "n_backward_rounds")} == \
               {k: r[k] for k in ("n_trimmed", "n_outer", "n_trim_rounds", "n_forward_rounds", "n_backward_rounds")}
        assert st["n_outer"] <= max(len(order), 0) and sum(st["n_class"]) == len(edges)
        # layout.superbubble_partitions on the same arrays gives the reference's partitions
        sccs, comps = as_device(plain, weak, order, edges)
        parts = layout.superbubble_partitions(sccs, comps)
        assert len(parts) == weak["stats"]["n_components"] and all(p[-1].acyclic and not any(q.acyclic for q in p[:-1]) for p in parts)
        pu.check_against_record(plain, pu.device_partitions(parts, edges), edges, r)


def test_the_shapes_the_direct_cases_are_about():
    by = {c["name"][len("direct_"):]: c["results"][0] for c in CASES if c.get("direct")}
    assert by["empty"]["n_sccs"] == 0 and by["empty"]["n_partitions"] == 0
    assert by["one_self_loop_alone"]["p_sources"] == [0] and by["one_self_loop_alone"]["n_class"] == [0, 1, 0, 0, 0]   # sourceless
    assert by["two_cycles_joined_by_an_edge"]["n_class"][4] == 1
    assert by["cycle_bridge_cycle"]["n_outer"] == 2 and by["cycle_bridge_path_cycle"]["n_trimmed"] == 3   # (the rest of the bridge)
    assert by["six_cycles_ascending"]["n_outer"] == 6 and by["six_cycles_descending"]["n_outer"] == 1
    assert by["every_node_in_a_cycle"]["p_n_nodes"] == [3, 0, 2, 0]               # both acyclic partitions are empty
    assert by["k8_both_directions"]["max_scc_edges"] == 56
    for tag in ("ascending", "descending", "scrambled"):
        assert by["path_1025_" + tag]["n_trim_rounds"] == 514 and by["path_1025_" + tag]["n_forward_rounds"] == 0
    for n in (257, 1025):
        for tag in ("ascending", "scrambled"):
            assert by["ring_%d_%s" % (n, tag)]["n_forward_rounds"] == n == by["ring_%d_%s" % (n, tag)]["n_backward_rounds"]
    assert by["two_cycles_2050"]["n_sccs"] == 2050 == by["two_cycles_2050"]["n_nonsingleton_sccs"]
    assert sum(1 for n in by if n.startswith("random_200_")) == 10


def test_an_edge_end_outside_the_node_order_is_refused_by_the_statement():
    with pytest.raises(ValueError):
        pu.partition([(0, 2), (2, 4)], [0, 2])
