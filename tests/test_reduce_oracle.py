"""The plain-Python statement of po_layout_reduce's contract (tests/reduce_utils.py) against the golden cases that
the reference's own remove_transitive_edges / make_symmetric produced (tests/golden/reduce_cases.npz, made by
tests/golden/make_reduce_golden.py), the fixture conditions of that file, and the host side of the new C ABI calls.
Everything is exact equality of integers."""
import ctypes

import numpy as np
import pytest

import layout_utils as lu
import reduce_utils as ru
from oracle import layout_oracle as lo
from phasm_amd import _lib
from phasm_amd.io import gfa
from phasm_amd.overlapper import ExactOverlapper

GOLDEN = ru.load_golden()
CASES = GOLDEN["cases"]
# the cases whose branches the generator counted (reference's debug log): every inline case
COUNTED = [c for c in CASES if "layout_case" in c or c.get("synth", {}).get("kind") == "line"]


def stage1_in_insertion_order(c):
    """Stage-1 edges of a case from the layout oracle, every adjacency list in the order the reference's OrderedDict
    holds it (first writer first), checked against what the reference's build_assembly_graph gave the generator."""
    names, lengths, rows = gfa.read_gfa2_rows(ru.case_text(c).splitlines(True))
    got = lo.layout_sequential(rows, lu.node_lengths(lengths), **c["params"])["edges"]
    arr = np.array([[u, v, w, o] for (u, v), (w, o) in got.items()], dtype=np.int64).reshape(-1, 4)
    assert len(arr) == c["n_stage1"]
    want = ru.case_stage1(c)
    if want is None:
        assert ru.edge_digest(ru.sort_edges(arr)) == c["stage1_sha256"]
    else:
        assert ru.sort_edges(arr).tolist() == ru.sort_edges(want).tolist()        # weight and overlap_len included
        for u in set(arr[:, 0].tolist()):                                         # ... and the order per source node
            assert arr[arr[:, 0] == u][:, 1].tolist() == want[want[:, 0] == u][:, 1].tolist()
    return arr


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_equals_the_reference_on_every_golden_case(case):
    s1 = stage1_in_insertion_order(case)
    order = np.lexsort((s1[:, 1], s1[:, 0])) if len(s1) else np.empty(0, dtype=np.int64)
    for fuzz, exp in case["results"].items():
        flags = ru.reduce_edges(s1, int(fuzz))
        assert np.array_equal(flags[order], ru.unpack_flags(exp["flags_by_uv"], len(s1))), fuzz
        assert int((flags == 1).sum()) == exp["n_transitive"]
        assert int((flags == 2).sum()) == exp["n_asymmetric"]
        kept = ru.sort_edges(s1[flags == 0])
        assert len(kept) == exp["n_kept"] and ru.edge_digest(kept) == exp["kept_sha256"]
        if "kept" in exp:
            assert kept.tolist() == exp["kept"]


def test_the_fixtures_reach_every_branch():
    """A condition on the golden file: every branch of the contract is taken somewhere, by the reference's own count.

    ``edges_weight_le0`` is the exception, and it is 0 by arithmetic, not by the choice of seeds: build_assembly_graph
    adds edges for OVERLAP_AB / OVERLAP_BA rows only, and classify() (phasm/alignments.py:248-258) returns OVERLAP_AB
    only when astart > bstart and la - aend < lb - bend (anything else is one of the two containments), so both
    weights of the row, astart - bstart and (lb - bend) - (la - aend), are >= 1; OVERLAP_BA likewise.  No E line, from
    whatever producer, gives a stage-1 edge of weight <= 0 (the generator tries: 48 random-coordinate cases)."""
    t = GOLDEN["branch_totals"]
    for k in ru.BRANCHES + ("fuzz_sensitive_cases",):
        assert t[k] > 0, k
    assert t["edges_weight_le0"] == 0
    # the totals are those of the restatement on the counted cases (the generator held them to the reference's log)
    counts = ru.new_counts()
    sensitive = 0
    for c in CASES:
        s1 = stage1_in_insertion_order(c) if c in COUNTED else None
        seen = set()
        for fuzz, exp in c["results"].items():
            seen.add(exp["flags_by_uv"])
            if s1 is not None:
                ru.reduce_edges(s1, int(fuzz), counts=counts)
        sensitive += len(seen) > 1
    assert counts == {k: t[k] for k in ru.BRANCHES}
    assert sensitive == t["fuzz_sensitive_cases"]
    assert max(c["n_stage1"] for c in CASES if c.get("synth", {}).get("kind") == "hub") > 2 * 5000
    assert {"0", "1000000"} <= {f for c in CASES for f in c["results"]}


def test_restatement_on_a_node_subset_equals_the_whole():
    c = next(x for x in CASES if x["name"] == "line_105")
    s1 = stage1_in_insertion_order(c)
    whole = ru.reduce_edges(s1, 150)
    nodes = sorted(set(s1[:, 0].tolist()))[::3]
    part = ru.reduce_edges(s1, 150, nodes=nodes)
    sel = np.isin(s1[:, 0], nodes)
    assert (part[~sel] == 255).all()
    assert np.array_equal(part[sel] == 1, whole[sel] == 1)


def test_flag_packing_round_trip():
    f = np.array([0, 1, 2, 0, 2, 2, 1], dtype=np.uint8)
    assert np.array_equal(ru.unpack_flags(ru.pack_flags(f), len(f)), f)


# ---- the C ABI: host side ---------------------------------------------------------------------------------------

def test_reduce_symbols_are_exported_and_bound():
    lib = _lib.load()
    names = [s[0] for s in _lib.SYMBOLS]
    for name in ("po_layout_reduce", "po_get_reduce_stats"):
        assert name in names and hasattr(lib, name)
    assert ctypes.sizeof(_lib.PoReduceParams) == 8 and ctypes.sizeof(_lib.PoReduceStats) == 64
    assert lib.po_abi_version() == 4      # additive change


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001
        return False


def test_reduce_argument_checks_and_no_cpu_fallback():
    lib = _lib.load()
    ov, other = ExactOverlapper(), ExactOverlapper()
    for o in (ov, other):
        o.add_segment("a", 100)
        o.add_segment("b", 100)
    rows = ov.result_from_rows(np.array([[0, 2, 40, 100, 0, 60]], dtype=np.int64))
    out = ctypes.c_void_p()
    good = _lib.PoReduceParams(1000, 0)
    call = lambda h, res, prm: lib.po_layout_reduce(h, res, ctypes.byref(prm) if prm is not None else None, None, ctypes.byref(out))
    assert call(None, rows._ptr, good) == _lib.PO_ERR_INVALID
    assert call(ov._h, None, good) == _lib.PO_ERR_INVALID
    assert call(ov._h, rows._ptr, None) == _lib.PO_ERR_INVALID
    assert lib.po_layout_reduce(ov._h, rows._ptr, ctypes.byref(good), None, None) == _lib.PO_ERR_INVALID
    assert call(other._h, rows._ptr, good) == _lib.PO_ERR_INVALID                       # a result of another handle
    assert call(ov._h, rows._ptr, _lib.PoReduceParams(1000, 1)) == _lib.PO_ERR_INVALID   # reserved
    assert call(ov._h, rows._ptr, _lib.PoReduceParams(-1, 0)) == _lib.PO_ERR_INVALID     # negative fuzz
    # good arguments: without a GPU there is nothing to fall back to; with one, a row result is not an edge result
    assert call(ov._h, rows._ptr, good) == (_lib.PO_ERR_INVALID if _have_gpu() else _lib.PO_ERR_HIP)
    assert not out.value
    with pytest.raises(ValueError):
        ov.layout_reduce(rows, length_fuzz=-5)
    st = _lib.PoReduceStats()
    assert lib.po_get_reduce_stats(ov._h, ctypes.byref(st)) == _lib.PO_OK and st.n_edges_in == 0
    assert lib.po_get_reduce_stats(None, ctypes.byref(st)) == _lib.PO_ERR_INVALID
    rows.free()
    ov.close()
    other.close()


def test_cli_knows_the_reference_option_names():
    from phasm_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["layout-edges", "--help"])
    assert e.value.code == 0
    import inspect
    from phasm_amd import layout
    for fn in (layout.layout_from_gfa, layout.layout_from_daligner, layout.layout_from_overlaps):
        p = inspect.signature(fn).parameters
        assert p["reduce"].default is False and p["length_fuzz"].default == 1000
