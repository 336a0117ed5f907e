"""What a rejected po_layout_* call says and leaves behind.  The entry points build their messages from the stage's name,
so every sentence is written out here as the header's callers have always seen it, not taken from the library's source.
A rejected call returns PO_ERR_INVALID, leaves ``*out`` null and the caller's flag buffer alone, and a handle that has
rejected calls computes the same bytes afterwards as before (the goldens of tests/golden/merge_cases.npz).

Every rejection here is turned away by the checks in front of the call, before a result is allocated: no fault is
provoked, so the clean-up of a driver that fails half way (synchronise, release, delete) is not reached by this file."""
import ctypes

import numpy as np
import pytest

import diamond_utils as du
import merge_utils as mu
import reduce_utils as ru
import tips_utils as tu
from phasm_amd import _lib
from phasm_amd.overlapper import ExactOverlapper

EDGE_RESULT_4 = "an edge result (po_layout_edges, po_layout_reduce, po_layout_tips, po_layout_diamonds)"
CLEANED_AGAIN = ": a merged graph (po_layout_merge) cannot be cleaned again"
# stage -> (its parameter block with a given reserved word, "needs ..." sentence, sentence for a merged graph)
STAGES = {
    "po_layout_reduce": (lambda rsv: _lib.PoReduceParams(1000, rsv), "po_layout_reduce needs a po_layout_edges result",
                         "po_layout_reduce" + CLEANED_AGAIN),
    "po_layout_tips": (lambda rsv: _lib.PoTipsParams(4, 5000, rsv),
                       "po_layout_tips needs an edge result (po_layout_edges, po_layout_reduce, po_layout_tips)",
                       "po_layout_tips" + CLEANED_AGAIN),
    "po_layout_diamonds": (lambda rsv: _lib.PoDiamondParams(rsv), "po_layout_diamonds needs " + EDGE_RESULT_4,
                           "po_layout_diamonds" + CLEANED_AGAIN),
    "po_layout_merge": (lambda rsv: _lib.PoMergeParams(rsv), "po_layout_merge needs " + EDGE_RESULT_4,
                        "po_layout_merge: the graph is merged already"),
}
FILL = 0xAB


def rejected(ov, name, result, params, message):
    """One call of an edge-producing entry point that must be turned away with ``message``."""
    lib = _lib.load()
    out = ctypes.c_void_p()
    flags = np.full(64, FILL, dtype=np.uint8)
    status = getattr(lib, name)(ov._h, result._ptr, ctypes.byref(params), flags.ctypes.data_as(ctypes.c_void_p), ctypes.byref(out))
    assert status == _lib.PO_ERR_INVALID, name
    assert out.value is None, name
    assert lib.po_last_error(ov._h).decode() == message
    assert (flags == FILL).all(), name


def coverage_rejected(ov, graph, rows, reserved, message):
    lib = _lib.load()
    out = np.full(64, FILL, dtype=np.uint8)
    prm = _lib.PoCoverageParams(reserved)
    status = lib.po_layout_coverage(ov._h, graph._ptr, rows._ptr, ctypes.byref(prm), out.ctypes.data_as(ctypes.c_void_p))
    assert status == _lib.PO_ERR_INVALID
    assert lib.po_last_error(ov._h).decode() == message
    assert (out == FILL).all()


def segment_handle(name):
    ov = ExactOverlapper()
    ov.add_segment(name, 10)
    return ov, ov.result_from_rows(np.zeros((0, 6), dtype=np.int64))


def test_checks_in_front_of_the_device_keep_their_sentences():
    """A result of another handle, then a non-zero reserved word: both are turned away before the device is looked for."""
    mine, my_rows = segment_handle("x")
    other, other_rows = segment_handle("y")
    layout = lambda rsv: _lib.PoLayoutParams(0, 0, 1000, rsv, 0.8)   # noqa: E731
    rejected(mine, "po_layout_edges", other_rows, layout(0), "po_layout_edges: the rows belong to another handle")
    rejected(mine, "po_layout_edges", my_rows, layout(1), "po_layout_edges: bad parameters")
    for name, (params, _, _) in STAGES.items():
        rejected(mine, name, other_rows, params(0), name + ": the edges belong to another handle")
        rejected(mine, name, my_rows, params(1), name + ": bad parameters")
    coverage_rejected(mine, other_rows, other_rows, 0, "po_layout_coverage: a result belongs to another handle")
    coverage_rejected(mine, my_rows, other_rows, 0, "po_layout_coverage: a result belongs to another handle")
    coverage_rejected(mine, my_rows, my_rows, 1, "po_layout_coverage: bad parameters")
    for r in (my_rows, other_rows):
        r.free()
    mine.close()
    other.close()


@pytest.mark.gpu
def test_a_row_result_and_a_merged_graph_are_turned_away():
    """One segment, no rows: a row result, an empty edge result and an empty merged graph without a kernel of any size."""
    ov, rows = segment_handle("x")
    empty, _ = ov.layout_edges(rows)
    merged = ov.layout_merge(empty)
    assert len(ov) == 2 and len(empty) == 0 and len(merged) == 0
    for name, (params, needs, again) in STAGES.items():
        rejected(ov, name, rows, params(0), needs)
        rejected(ov, name, merged, params(0), again)
    for r in (merged, empty, rows):
        r.free()
    ov.close()


# the smallest golden case (by edges of its stage-1 graph) whose cleaned graph still merges into paths: every stage of the
# chain has edges to work on
CASE = min((c for c in mu.load_golden()["cases"] if not c.get("direct") and c["results"][1]["n_merged"]),
           key=lambda c: c["results"][0]["n_edges_in"])


def chain(ov, edges_res):
    """reduce -> tips -> diamonds -> tips -> merge at the CLI defaults, as tests/test_gpu_merge.py cleans a graph.
    Returns (every byte the calls gave back, the merged graph's pieces for the golden record)."""
    steps = (lambda r: ov.layout_reduce(r, du.STAGE_FUZZ, want_flags=True),
             lambda r: ov.layout_tips(r, du.STAGE_L, du.STAGE_B, want_flags=True),
             lambda r: ov.layout_diamonds(r, want_flags=True),
             lambda r: ov.layout_tips(r, du.STAGE_L, tu.DEFAULT_B, want_flags=True),
             lambda r: ov.layout_merge(r, want_flags=True))
    seen, cur = [], edges_res
    for k, step in enumerate(steps):
        before = cur.rows()
        nxt, flags = step(cur)
        seen += [flags.tobytes(), nxt.rows().tobytes(), nxt.node_order().tobytes()]
        if k == len(steps) - 1:
            tables = nxt.merged_paths()
            seen += [t.tobytes() for t in tables]
            final = (before, cur.node_order().tolist(), flags, nxt.rows(), nxt.node_order().tolist(), tables)
        if cur is not edges_res:
            cur.free()
        cur = nxt
    cur.free()
    return seen, final


@pytest.mark.gpu
def test_rejected_calls_leave_the_handle_as_it_was(tmp_path):
    p = tmp_path / "in.gfa"
    p.write_text(mu.case_text(CASE))
    ov = ExactOverlapper()
    _, rows = ov.add_gfa(str(p))
    edges_res, _ = ov.layout_edges(rows, **CASE["params"])
    first, final = chain(ov, edges_res)
    # one rejection per stage, each for another reason, with results of other calls alive on the handle
    other, other_rows = segment_handle("y")
    merged = ov.layout_merge(edges_res)
    rejected(ov, "po_layout_reduce", edges_res, STAGES["po_layout_reduce"][0](1), "po_layout_reduce: bad parameters")
    rejected(ov, "po_layout_tips", merged, STAGES["po_layout_tips"][0](0), STAGES["po_layout_tips"][2])
    rejected(ov, "po_layout_diamonds", rows, STAGES["po_layout_diamonds"][0](0), STAGES["po_layout_diamonds"][1])
    rejected(ov, "po_layout_merge", other_rows, STAGES["po_layout_merge"][0](0), "po_layout_merge: the edges belong to another handle")
    merged.free()
    other_rows.free()
    other.close()
    second, _ = chain(ov, edges_res)
    assert first == second
    # ... and they are the golden's: the merge of the cleaned graph, as tests/test_gpu_merge.py holds it to its record.
    # (merge_cases.npz records the merge alone.  The bytes of reduce, tips and diamonds are held to the first run here;
    # their own goldens are those of test_gpu_reduce.py, test_gpu_tips.py and test_gpu_diamond.py.  The merge's input is
    # their output, so its record -- order_before, flags per input edge -- pins the cleaned graph too.)
    rec = CASE["results"][1]
    before, order_before, flags, got, order, (offsets, members, prefix, lengths) = final
    edge_array = lambda e: np.stack([e["u"], e["v"], e["weight"], e["overlap_len"]], 1).astype(np.int64).reshape(-1, 4)   # noqa: E731
    assert order_before == rec["order_before"] and len(ov) == rec["n_ids"]
    assert np.array_equal(flags[tu.by_uv(edge_array(before))], ru.unpack_flags(rec["flags"], len(before)))
    assert flags.any()
    assert ru.edge_digest(ru.sort_edges(edge_array(got))) == rec["kept_sha256"]
    for a, key in ((offsets, "offsets"), (members, "members"), (prefix, "prefix"), (lengths, "lengths")):
        assert a.tolist() == rec[key].tolist(), key
    assert order == du.minus(order_before, rec["members"].tolist()) + [rec["n_ids"] + k for k in range(rec["n_merged"])]
    for r in (edges_res, rows):
        r.free()
    ov.close()
