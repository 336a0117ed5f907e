"""Paths, interior and exit predecessors of every top-level bubble on the device (po_phase_paths, ExactOverlapper.phase_paths,
phasing.bubble_paths) against tests/golden/paths_cases.npz -- held by its generator to the reference's find_superbubbles and
superbubble_nodes, to networkx.all_simple_paths and to predecessors_iter -- and against ``paths_utils.scheme`` on the device's
own edge order.  Exact integers throughout.  Every case goes through po_graph_from_edges on a handle with one segment per two
node ids, so the merged-node ids of a walk (ids behind the reads) are plain node ids here and need no mapping back."""
import numpy as np
import pytest
import torch

import paths_utils as pp
import walk_utils as wu
from phasm_amd import _lib, phasing
from test_gpu_components import segments
from test_paths_oracle import BY_NAME, CASES, WALKS

pytestmark = pytest.mark.gpu


def graph_of(order, edges):
    n_ids = (max([int(x) for x in order] + [-1]) | 1) + 1
    ov = segments(max(n_ids, 2))
    e = np.asarray([[u, v, w, 17] for u, v, w in edges], dtype=np.int64).reshape(-1, 4)
    return ov, ov.graph_from_edges(e, order)


def device_edges(g):
    rows = g.rows()
    return [[int(r["u"]), int(r["v"]), int(r["weight"])] for r in rows]


def call_bytes(bp):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (bp.bubbles, bp.inside_off, bp.inside_nodes, bp.pred_off, bp.pred_node,
                                                                 bp.pred_weight, bp.bubble_path_off, bp.path_off, bp.path_nodes))


def check_paths(ov, g, max_paths, want):
    """One call on the graph result ``g`` against the expected result; returns the BubblePaths and the bytes of the call."""
    before, order = g.rows().tobytes(), g.node_order()
    bp = phasing.bubble_paths(ov, g, max_paths)
    st = ov.paths_stats()
    got = pp.result_of(bp, st)
    pp.same(got, want)                                                                   # the golden
    pp.same(got, pp.scheme(device_edges(g), order.tolist(), max_paths))                  # the restatement, on the device's own edge order
    assert st["n_stray_edges"] == 0 and st["n_invalid"] == 0
    assert st["n_count_rounds"] == want["stats"]["n_count_rounds"] <= max(want["b_inside"].tolist() + [-2]) + 2
    assert st["n_batches"] >= -(-st["n_count_rounds"] // 8)
    assert bp.bubbles.dtype == _lib.BUBBLE_PATHS_DTYPE and bp.inside_off.dtype == np.uint64 and bp.path_nodes.dtype == np.uint32
    assert g.rows().tobytes() == before and g.node_order().tobytes() == order.tobytes()  # the inputs stay as they were
    print("%d bubbles, %d listed paths, %d path nodes, %d rounds: %.3f ms (chains %.3f, count %.3f, list %.3f)" % (
        st["n_bubbles"], st["n_listed_paths"], st["n_path_nodes"], st["n_count_rounds"], st["ms_total"], st["ms_chains"], st["ms_count"],
        st["ms_list"]))
    return bp, call_bytes(bp)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_cases_through_graph_from_edges(case):
    order, edges, max_paths = pp.case_inputs(case)
    ov, g = graph_of(order, edges)
    assert g.node_order().tolist() == order and device_edges(g) == edges
    check_paths(ov, g, max_paths, pp.result_of_record(case["result"]))
    g.free()
    ov.close()


@pytest.mark.parametrize("case", WALKS, ids=[c["name"] for c in WALKS])
def test_every_walk_as_phase_computed_it(case):
    walk = wu.load_golden()["walks"][case["walk"]]
    order, edges, max_paths = pp.case_inputs(case)
    ov, g = graph_of(order, edges)
    bp = phasing.bubble_paths(ov, g, max_paths)
    visited = bp.chain_bubbles(0)
    assert [int(bp.bubbles["entrance"][b]) for b in visited] == [x["entrance"] for x in walk["bubbles"]]
    size = walk["params"]["max_bubble_size"]
    for b, want in zip(visited, walk["bubbles"]):
        assert int(bp.bubbles["exit"][b]) == want["exit"]
        assert [list(p) for p in bp.paths_of(b)] == want["paths"]
        assert bp.interior_of(b) == sorted(want["interior_nodes"], key=order.index)
        assert [list(p) for p in bp.preds_of(b)] == want["preds"]
        assert bp.is_large(b, size) == (len(want["paths"]) > size)
    # the decision from the counts alone: nothing listed
    counted = ov.phase_paths(g, 0)
    assert counted.bubbles["n_paths"].tolist() == bp.bubbles["n_paths"].tolist() and len(counted.path_nodes) == 0
    assert [counted.is_large(b, size) for b in visited] == [len(x["paths"]) > size for x in walk["bubbles"]]
    g.free()
    ov.close()


def test_three_calls_and_a_fresh_handle_give_identical_bytes():
    for name in ("direct_su_sb_random_dag_200_seed3", "direct_one_bubble_129_paths", "walk_break_and_shrink"):
        case = BY_NAME[name]
        order, edges, max_paths = pp.case_inputs(case)
        seen = []
        for calls in (3, 1):
            ov, g = graph_of(order, edges)
            seen += [check_paths(ov, g, max_paths, pp.result_of_record(case["result"]))[1] for _ in range(calls)]
            g.free()
            ov.close()
        assert len(seen) == 4 and all(s == seen[0] for s in seen)


def test_the_call_takes_turns_with_the_stages_before_it():
    small, large = BY_NAME["direct_nested_in_nested"], BY_NAME["direct_su_sb_random_digraph_200_seed4"]
    ov = segments(400)
    graphs = []
    for case in (small, large):
        order, edges, _ = pp.case_inputs(case)
        graphs.append(ov.graph_from_edges(np.asarray([[u, v, w, 17] for u, v, w in edges], dtype=np.int64), order))
    first = {}
    for turn in range(2):
        for k, (case, g) in enumerate(((small, graphs[0]), (large, graphs[1]), (small, graphs[0]))):
            sb = ov.layout_superbubbles(g)
            _, data = check_paths(ov, g, case["max_paths"], pp.result_of_record(case["result"]))
            bc = ov.layout_bubblechains(g)
            assert [a.tobytes() for a in ov.layout_superbubbles(g)] == [a.tobytes() for a in sb]
            assert [a.tobytes() for a in ov.layout_bubblechains(g)] == [a.tobytes() for a in bc]
            assert first.setdefault(case["name"], data) == data
            assert int((sb[3]["nested"] == 0).sum()) == ov.paths_stats()["n_bubbles"]
    for g in graphs:
        g.free()
    ov.close()


def test_an_empty_graph_null_outputs_and_an_edge_outside_the_order():
    import ctypes
    lib = _lib.load()
    ov = segments(8)
    g = ov.graph_from_edges(np.zeros((0, 4), dtype=np.int64), [])
    bp = ov.phase_paths(g, 10)
    assert len(bp) == 0 and bp.inside_off.tolist() == bp.pred_off.tolist() == bp.bubble_path_off.tolist() == bp.path_off.tolist() == [0]
    assert ov.paths_stats()["n_bubbles"] == 0
    g.free()
    # nodes without a bubble: sizes 0, one offset each
    g = ov.graph_from_edges(np.asarray([[0, 2, 5, 17], [0, 4, 6, 17]]), [0, 2, 4])
    bp = ov.phase_paths(g, 10)
    assert len(bp) == 0 and bp.path_off.tolist() == [0] and ov.paths_stats()["n_nodes"] == 3
    g.free()
    # every output may be NULL; the sizes stand
    g = ov.graph_from_edges(np.asarray([[0, 2, 5, 17], [0, 4, 6, 17], [2, 6, 7, 17], [4, 6, 8, 17]]), [0, 2, 4, 6])
    r = ctypes.c_void_p()
    prm = _lib.PoPathsParams(10, 0)
    assert lib.po_phase_paths(ov._h, g._ptr, ctypes.byref(prm), ctypes.byref(r)) == _lib.PO_OK
    dims = _lib.PoPathsDims()
    assert lib.po_paths_sizes(r, ctypes.byref(dims)) == _lib.PO_OK
    assert dims.as_dict() == {"n_bubbles": 1, "n_inside_nodes": 2, "n_preds": 2, "n_listed_paths": 2, "n_path_nodes": 6}
    assert lib.po_paths_copy(r, *[None] * 9) == _lib.PO_OK
    nodes = np.zeros(6, dtype=np.uint32)
    assert lib.po_paths_copy(r, *[None] * 8, nodes.ctypes.data_as(ctypes.c_void_p)) == _lib.PO_OK and nodes.tolist() == [0, 2, 6, 0, 4, 6]
    lib.po_result_free(r)
    # params NULL: counts only
    assert lib.po_phase_paths(ov._h, g._ptr, None, ctypes.byref(r)) == _lib.PO_OK
    assert lib.po_paths_sizes(r, ctypes.byref(dims)) == _lib.PO_OK and dims.n_listed_paths == 0 and dims.n_bubbles == 1
    lib.po_result_free(r)
    g.free()
    ov.close()


def test_capacity_is_refused_from_the_counts_alone():
    case = BY_NAME["direct_unlisted_62"]
    order, edges, _ = pp.case_inputs(case)
    ov, g = graph_of(order, edges)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    with pytest.raises(OverflowError, match="paths to list in one call"):
        ov.phase_paths(g, 2**62 + 1)
    # nothing the size of a listing was allocated: a handle's first workspaces at the most
    assert free_before - torch.cuda.mem_get_info()[0] < (1 << 30)
    st = ov.paths_stats()
    assert st["max_paths_seen"] == 2**62 + 1 and st["n_unlisted"] == 0 and st["n_listed_paths"] == 0
    # the same handle goes on
    check_paths(ov, g, case["max_paths"], pp.result_of_record(case["result"]))
    g.free()
    ov.close()


# ---- past one capped grid ---------------------------------------------------------------------------------------------------

def capped_grid_threads():
    """The threads of one capped grid: what the listed paths must exceed for the stride loop of the walk to wrap."""
    return 8 * 256 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("layout", ["copy_major", "interleaved"])
def test_listed_paths_past_one_capped_grid(layout):
    cases = [BY_NAME[n] for n in pp.UNION_NAMES]
    assert all(c["max_paths"] <= 200 for c in cases)
    per_copy = sum(c["result"]["stats"]["n_listed_paths"] for c in cases)
    copies = capped_grid_threads() // per_copy + 2
    order, edges, want = pp.union_of(cases, copies, layout)
    assert len(want["path_off"]) - 1 > capped_grid_threads()
    ov = segments(int(order.max()) + 2)
    g = ov.graph_from_edges(np.concatenate([edges, np.full((len(edges), 1), 17)], axis=1), order)
    bp = ov.phase_paths(g, 200)
    st = ov.paths_stats()
    got = pp.result_of(bp, st)
    for k in pp.ARRAY_KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert st["n_listed_paths"] == copies * per_copy and st["n_stray_edges"] == 0 and st["n_bubbles"] == len(want["b_entrance"])
    assert st["max_paths_seen"] == 129 and st["n_path_nodes"] == len(want["path_nodes"])
    print("%s: %d copies, %d bubbles, %d listed paths, %d path nodes: %.3f ms (chains %.3f, count %.3f, list %.3f)" % (
        layout, copies, st["n_bubbles"], st["n_listed_paths"], st["n_path_nodes"], st["ms_total"], st["ms_chains"], st["ms_count"], st["ms_list"]))
    g.free()
    ov.close()
