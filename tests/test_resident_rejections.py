"""Every rejection of po_walk_relevant, po_walk_step_resident and po_walk_prev_copy (include/phasm_overlap.h) that needs no live
gather, through ctypes, on a machine without a GPU: each is PO_ERR_INVALID with its sentence, decided on the host before the
device is touched, and leaves outputs and state as they were.  (The rejections that need a live gather -- a stale one, the
mismatches of sizes and state, the other route inside a block -- are in tests/test_gpu_resident.py: a gather needs the device.)"""
import ctypes

import numpy as np
import pytest

from phasm_amd import _lib
from phasm_amd._lib import PoPhaseInput, PoPhaseParams, PoRelevantInput, PoWalkInfo, PoWalkRelevantParams

LIB = _lib.load()
SEQS = ((b"a", b"ACGTACGTAC"), (b"b", b"TTGACCATGA"), (b"c", b"GGATCCATTA"), (b"d", b"CATTAGGACC"))
FRESH = {"ploidy": 2, "n_cands": 1, "depth": 0, "start_of_block": 1, "n_block_reads": 0}


def arr(values, dtype=np.uint32):
    return np.ascontiguousarray(values, dtype=dtype)


@pytest.fixture()
def handle():
    h = ctypes.c_void_p()
    assert LIB.po_create(ctypes.byref(h)) == 0
    for name, seq in SEQS:                                                            # read ids 0..3
        assert LIB.po_add_sequence(h, name, len(name), seq, len(seq)) == 0
    assert LIB.po_num_sequences(h) == 4
    yield h
    LIB.po_destroy(h)


@pytest.fixture()
def walk(handle):
    w = ctypes.c_void_p()
    assert LIB.po_walk_create(handle, 2, ctypes.byref(w)) == 0
    yield w
    LIB.po_result_free(w)


@pytest.fixture()
def rows(handle):
    r = ctypes.c_void_p()
    assert LIB.po_result_from_rows(handle, None, 0, ctypes.byref(r)) == 0
    yield r
    LIB.po_result_free(r)


def info(w):
    out = PoWalkInfo()
    assert LIB.po_walk_info_get(w, ctypes.byref(out)) == 0
    return out.as_dict()


def said(handle):
    return LIB.po_last_error(handle).decode()


class Gather:
    """One po_walk_relevant call that only lacks a real index (which needs the device), to be spoilt."""

    def __init__(self):
        self.cur, self.pred, self.plen = arr([0, 2]), arr([1]), arr([5000], np.int32)
        self.prm = PoWalkRelevantParams(0, 3, 0, 0)
        self.inp = PoRelevantInput(self.cur.ctypes.data, 2, None, 0, None, 0, self.pred.ctypes.data, self.plen.ctypes.data, 1)


def gather_refused(handle, w, index, g, sentence, walk_of=None):
    out = ctypes.c_void_p(1)
    st = LIB.po_walk_relevant(handle, w, index, ctypes.byref(g.prm), ctypes.byref(g.inp), ctypes.byref(out))
    assert st == _lib.PO_ERR_INVALID, st
    assert sentence in said(handle), said(handle)
    assert not out.value and info(walk_of or w) == FRESH


def spoil(what):
    g = Gather()
    g.keep = arr([1, 3])
    if what == "reserved":
        g.prm.reserved = 1
    elif what == "mode":
        g.prm.mode = 2
    elif what == "prev_graph":
        g.inp.prev_graph, g.inp.n_prev_graph = g.keep.ctypes.data, 2
    elif what == "prev_graph_pointer":
        g.inp.prev_graph = g.keep.ctypes.data
    elif what == "prev_aligning":
        g.inp.prev_aligning, g.inp.n_prev_aligning = g.keep.ctypes.data, 2
    elif what == "prev_aligning_count":
        g.inp.n_prev_aligning = 1
    elif what == "missing":
        g.inp.cur_graph = None
    elif what == "cur_id":
        g.cur[1] = 4
    elif what == "pred_id":
        g.pred[0] = 2**31
    return g


@pytest.mark.parametrize("what,sentence", [
    ("reserved", "po_walk_relevant: bad parameters"), ("mode", "po_walk_relevant: the mode must be 0 (spanning) or 1 (all)"),
    ("prev_graph", "prev_graph and prev_aligning must be NULL with count 0"),
    ("prev_graph_pointer", "prev_graph and prev_aligning must be NULL with count 0"),
    ("prev_aligning", "prev_graph and prev_aligning must be NULL with count 0"),
    ("prev_aligning_count", "prev_graph and prev_aligning must be NULL with count 0"),
    ("missing", "po_walk_relevant: a list is missing"), ("cur_id", "po_walk_relevant: a list names a read the handle does not hold"),
    ("pred_id", "po_walk_relevant: a list names a read the handle does not hold")])
def test_the_gather_refuses(handle, walk, rows, what, sentence):
    gather_refused(handle, walk, rows, spoil(what), sentence)


def test_the_gather_refuses_missing_arguments(handle, walk, rows):
    g = Gather()
    out = ctypes.c_void_p(1)
    assert LIB.po_walk_relevant(handle, walk, rows, ctypes.byref(g.prm), ctypes.byref(g.inp), None) == _lib.PO_ERR_INVALID
    assert "po_walk_relevant: no room for the result" in said(handle)
    for args, sentence in (((None, rows, ctypes.byref(g.prm), ctypes.byref(g.inp)), "no walk"),
                           ((walk, None, ctypes.byref(g.prm), ctypes.byref(g.inp)), "no index"),
                           ((walk, rows, None, ctypes.byref(g.inp)), "no parameters"),
                           ((walk, rows, ctypes.byref(g.prm), None), "no parameters")):
        out = ctypes.c_void_p(1)
        assert LIB.po_walk_relevant(handle, *args, ctypes.byref(out)) == _lib.PO_ERR_INVALID and not out.value
        assert "po_walk_relevant: " + sentence in said(handle)
    assert info(walk) == FRESH


def test_a_walk_or_an_index_of_another_handle_or_of_another_kind(handle, walk, rows):
    other = ctypes.c_void_p()
    assert LIB.po_create(ctypes.byref(other)) == 0
    for name, seq in SEQS:
        assert LIB.po_add_sequence(other, name, len(name), seq, len(seq)) == 0
    far = ctypes.c_void_p()
    assert LIB.po_result_from_rows(other, None, 0, ctypes.byref(far)) == 0
    gather_refused(other, walk, far, Gather(), "po_walk_relevant: the walk belongs to another handle")
    gather_refused(handle, walk, far, Gather(), "po_walk_relevant: the index belongs to another handle")
    LIB.po_result_free(far)
    LIB.po_destroy(other)
    gather_refused(handle, rows, rows, Gather(), "po_walk_relevant: needs the result of po_walk_create", walk_of=walk)
    gather_refused(handle, walk, rows, Gather(), "po_walk_relevant: needs the result of po_phase_index")
    gather_refused(handle, walk, walk, Gather(), "po_walk_relevant: needs the result of po_phase_index")


class Step:
    """The arguments of one po_walk_step_resident call on a fresh walk of ploidy 2 with two paths."""

    def __init__(self):
        self.path_off, self.path_ids, self.levels = arr([0, 1, 3]), arr([0, 1, 2]), arr([-1.0], np.float64)
        self.prm = PoPhaseParams(2, 2, 1, 2, 3, 1, 0, 1, 500, 1, 1e-3, 0, 0)
        self.inp = PoPhaseInput(None, None, None, None, None, self.path_off.ctypes.data, self.path_ids.ctypes.data, None, None,
                                self.levels.ctypes.data)


def step_refused(handle, w, rel, sentence, walk_of=None, prm=True, inp=True):
    c = Step()
    cand, ext, rl = np.full(8, 77, np.uint32), np.full(8, 77, np.uint32), np.full(8, 7.5)
    n = ctypes.c_uint64(99)
    st = LIB.po_walk_step_resident(handle, w, rel, ctypes.byref(c.prm) if prm else None, ctypes.byref(c.inp) if inp else None, 1,
                                   cand.ctypes.data, ext.ctypes.data, rl.ctypes.data, 8, ctypes.byref(n))
    assert st == _lib.PO_ERR_INVALID, st
    assert sentence in said(handle), said(handle)
    assert n.value == 0 and set(cand.tolist()) == {77} and set(ext.tolist()) == {77} and set(rl.tolist()) == {7.5}
    assert info(walk_of) == FRESH


def test_the_step_refuses_what_is_no_gather_or_no_walk(handle, walk, rows):
    c = Step()
    assert LIB.po_walk_step_resident(handle, walk, rows, ctypes.byref(c.prm), ctypes.byref(c.inp), 1, None, None, None, 0, None) == _lib.PO_ERR_INVALID
    assert "po_walk_step_resident: no room for the number of entries" in said(handle)
    step_refused(handle, None, rows, "po_walk_step_resident: no walk", walk_of=walk)
    step_refused(handle, walk, None, "po_walk_step_resident: no gather", walk_of=walk)
    step_refused(handle, walk, rows, "po_walk_step_resident: no parameters", walk_of=walk, prm=False)
    step_refused(handle, walk, rows, "po_walk_step_resident: no parameters", walk_of=walk, inp=False)
    step_refused(handle, rows, rows, "po_walk_step_resident: needs the result of po_walk_create", walk_of=walk)
    step_refused(handle, walk, rows, "po_walk_step_resident: needs the result of po_walk_relevant", walk_of=walk)
    step_refused(handle, walk, walk, "po_walk_step_resident: needs the result of po_walk_relevant", walk_of=walk)
    other = ctypes.c_void_p()
    assert LIB.po_create(ctypes.byref(other)) == 0
    step_refused(other, walk, rows, "po_walk_step_resident: the walk belongs to another handle", walk_of=walk)
    LIB.po_destroy(other)


def test_the_previous_sets_of_a_fresh_walk_need_no_device(handle, walk, rows):
    ids, n = np.full(4, 77, np.uint32), ctypes.c_uint64(9)
    for which in (0, 1):
        n.value = 9
        assert LIB.po_walk_prev_copy(walk, which, ids.ctypes.data, 4, ctypes.byref(n)) == 0
        assert n.value == 0 and set(ids.tolist()) == {77}
    assert LIB.po_walk_reset(walk) == 0
    assert LIB.po_walk_prev_copy(walk, 1, None, 0, ctypes.byref(n)) == 0 and n.value == 0
    n.value = 9
    assert LIB.po_walk_prev_copy(walk, 2, ids.ctypes.data, 4, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    assert "po_walk_prev_copy: which must be 0 (prev_graph) or 1 (prev_aligning)" in said(handle) and n.value == 0
    assert LIB.po_walk_prev_copy(walk, 0, ids.ctypes.data, 4, None) == _lib.PO_ERR_INVALID
    assert "po_walk_prev_copy: no room for the number of ids" in said(handle)
    assert LIB.po_walk_prev_copy(rows, 0, ids.ctypes.data, 4, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    assert "po_walk_prev_copy needs the result of po_walk_create" in said(handle)
    assert LIB.po_walk_prev_copy(None, 0, ids.ctypes.data, 4, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    assert set(ids.tolist()) == {77} and info(walk) == FRESH


def test_po_relevant_copy_still_refuses_a_walk(handle, walk):
    assert LIB.po_relevant_copy(walk, *[None] * 8) == _lib.PO_ERR_INVALID
    assert "po_relevant_copy needs the result of po_phase_relevant" in said(handle)
