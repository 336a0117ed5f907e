"""The plain-Python statement of po_layout_reduce's contract (tests/reduce_utils.py) against the golden cases that
the reference's own remove_transitive_edges / make_symmetric produced (tests/golden/reduce_cases.npz, made by
tests/golden/make_reduce_golden.py), the fixture conditions of that file, and the host side of the new C ABI calls.
Everything is exact equality of integers."""
import ctypes
import functools
import hashlib
import json

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
# (the cases added for their out-degrees say so themselves)
COUNTED = [c for c in CASES if c.get("counted", "layout_case" in c or c.get("synth", {}).get("kind") == "line")]
BY_NAME = {c["name"]: c for c in CASES}
N_FIRST = 73          # the cases the file had before the out-degree cases came
FIRST_SHA256 = "d3f51c4dcf2bd3952b6370d2ef84b5dd21dc794a9d207858f8d040549ccd5d3f"


@functools.lru_cache(maxsize=None)
def stage1_of(name):
    """(stage-1 edges in insertion order, their (u, v) order): computed once per case, shared, never written to."""
    s1 = stage1_in_insertion_order(BY_NAME[name])
    order = np.lexsort((s1[:, 1], s1[:, 0])) if len(s1) else np.empty(0, dtype=np.int64)
    s1.setflags(write=False)
    order.setflags(write=False)
    return s1, order


@functools.lru_cache(maxsize=None)
def restated(name, fuzz):
    """(flags, branch counts) of the restatement: computed once per (case, fuzz), shared between the tests."""
    counts = ru.new_counts()
    flags = ru.reduce_edges(stage1_of(name)[0], fuzz, counts=counts)
    flags.setflags(write=False)
    return flags, counts


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
    s1, order = stage1_of(case["name"])
    for fuzz, exp in case["results"].items():
        flags = restated(case["name"], int(fuzz))[0]
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
        seen = set()
        for fuzz, exp in c["results"].items():
            seen.add(exp["flags_by_uv"])
            if c in COUNTED:
                for k, n in restated(c["name"], int(fuzz))[1].items():
                    counts[k] += n
        sensitive += len(seen) > 1
    assert counts == {k: t[k] for k in ru.BRANCHES}
    assert sensitive == t["fuzz_sensitive_cases"]
    assert max(c["n_stage1"] for c in CASES if c.get("synth", {}).get("kind") == "hub") > 2 * 5000
    assert {"0", "1000000"} <= {f for c in CASES for f in c["results"]}
    # the out-degrees the kernels branch on (a wave strides over adj[w] by 64; the states leave LDS above 1024)
    degrees = set()
    for c in CASES[N_FIRST:]:
        degrees |= set(np.bincount(stage1_of(c["name"])[0][:, 0]).tolist())
    assert {63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2049} <= degrees
    prof = {n: ru.degree_profile(stage1_of(n)[0], f) for n, f in (("dense_260", 0), ("dense_450", 0), ("stagger_1100", 0))}
    # nodes with 129..1023 out-edges that have a neighbour w with len(adj[w]) > 64
    assert prof["dense_260"]["mid_long_w"] + prof["dense_450"]["mid_long_w"] >= 100
    # a node above 1024 with a neighbour w above 1024, more than 64 of whose targets are its neighbours
    assert prof["stagger_1100"]["wide_pairs"] >= 1
    # (v, w) with len(adj[w]) > 128 whose walk over adj[w] accepts at least one entry and stops before the end
    assert prof["stagger_1100"]["partial_walks"] >= 1 and prof["dense_450"]["partial_walks"] >= 1


def test_the_first_cases_are_as_they_were():
    """The cases added later leave the records of the first 73 alone: the digest below was taken from the file as it
    stood before them (canonical JSON of load_golden()["cases"][:73])."""
    text = json.dumps(CASES[:N_FIRST], sort_keys=True, separators=(",", ":"))
    assert hashlib.sha256(text.encode()).hexdigest() == FIRST_SHA256
    assert len(CASES) > N_FIRST


def test_the_golden_file_is_small_enough_to_commit():
    import os
    assert os.path.getsize(ru.GOLDEN_FILE) < 1 << 20


SECOND = GOLDEN["second_pass"]


def second_pass_flags(rec, rank_of):
    """Flags of the second pass by (u, v); rank_of(keep) -> the rank given to the kept edges (keep = their indices in
    the first pass's insertion order, ascending)."""
    s1, _ = stage1_of(rec["case"])
    keep = np.flatnonzero(restated(rec["case"], rec["fuzz"])[0] == 0)
    kept = s1[keep]
    flags = ru.reduce_edges(kept, rec["fuzz2"], rank=rank_of(keep))
    return flags[np.lexsort((kept[:, 1], kept[:, 0]))]


def test_a_second_pass_depends_on_the_rank_the_first_hands_on():
    """A condition on the golden file: at least one recorded second pass comes out differently when the kept edges are
    given another order than the one they had in the first pass -- reversed, none at all (every rank 0), or their
    (u, v) order.  Without such a record a kept result with a wrong or missing hidden rank would pass every test."""
    rec = next(r for r in SECOND if r["case"] == "tie_8" and (r["fuzz"], r["fuzz2"]) == (0, 150))
    want = ru.unpack_flags(rec["flags_by_uv"], rec["n_in"])
    assert rec["n_transitive"] > 0
    assert np.array_equal(second_pass_flags(rec, lambda keep: keep), want)
    s1, _ = stage1_of("tie_8")
    for wrong in (lambda keep: -keep, lambda keep: np.zeros(len(keep), dtype=np.int64),
                  lambda keep: np.argsort(np.lexsort((s1[keep, 1], s1[keep, 0])))):
        assert not np.array_equal(second_pass_flags(rec, wrong), want)


@pytest.mark.parametrize("rec", SECOND, ids=["%s-F%d-F%d" % (r["case"], r["fuzz"], r["fuzz2"]) for r in SECOND])
def test_restatement_of_a_second_pass_equals_the_reference(rec):
    """Reducing the kept edges again: the reference ran its three calls a second time on the graph the first pass left
    (adjacency lists in the first pass's order), the restatement takes the kept edges with their first-pass rank."""
    s1, _ = stage1_of(rec["case"])
    keep = np.flatnonzero(restated(rec["case"], rec["fuzz"])[0] == 0)
    kept = s1[keep]
    assert len(kept) == rec["n_in"]
    flags = ru.reduce_edges(kept, rec["fuzz2"], rank=keep)
    order = np.lexsort((kept[:, 1], kept[:, 0]))
    assert np.array_equal(flags[order], ru.unpack_flags(rec["flags_by_uv"], len(kept)))
    assert (int((flags == 1).sum()), int((flags == 2).sum())) == (rec["n_transitive"], rec["n_asymmetric"])
    assert ru.edge_digest(ru.sort_edges(kept[flags == 0])) == rec["kept_sha256"]


def test_restatement_on_a_node_subset_equals_the_whole():
    s1 = stage1_of("line_105")[0]
    whole = restated("line_105", 150)[0]
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
