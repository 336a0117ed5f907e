"""Every rejection of the po_walk_* calls (include/phasm_overlap.h), through ctypes, on a machine without a GPU: each is
PO_ERR_INVALID with its sentence, decided on the host before the device is touched, and leaves outputs and state as they were.
Creating, resetting and asking a walk that has not advanced need no device either."""
import ctypes

import numpy as np
import pytest

from phasm_amd import _lib
from phasm_amd._lib import PoPhaseInput, PoPhaseParams, PoWalkInfo

LIB = _lib.load()


def arr(values, dtype):
    return np.ascontiguousarray(values, dtype=dtype)


class Call:
    """One valid po_walk_step call on a fresh walk of ploidy 2 -- two reads, three b reads, two paths -- to be spoilt."""

    def __init__(self):
        self.om, self.aln_off = arr([100, 90], np.int32), arr([0, 2, 3], np.uint32)
        self.aln_b, self.a0, self.a1 = arr([0, 2, 1], np.uint32), arr([5, 7, 9], np.int32), arr([50, 60, 70], np.int32)
        self.path_off, self.path_ids = arr([0, 1, 3], np.uint32), arr([0, 1, 2], np.uint32)
        self.levels = arr([-1.0], np.float64)
        self.b_reads = arr([4, 9, 12], np.uint32)
        self.prm = PoPhaseParams(2, 2, 1, 2, 3, 1, 0, 1, 500, 1, 1e-3, 0, 0)
        self.inp = PoPhaseInput(*[a.ctypes.data for a in (self.om, self.aln_off, self.aln_b, self.a0, self.a1, self.path_off, self.path_ids)],
                                None, None, self.levels.ctypes.data)
        self.b_ptr = self.b_reads.ctypes.data


@pytest.fixture()
def handle():
    h = ctypes.c_void_p()
    assert LIB.po_create(ctypes.byref(h)) == 0
    yield h
    LIB.po_destroy(h)


@pytest.fixture()
def walk(handle):
    w = ctypes.c_void_p()
    assert LIB.po_walk_create(handle, 2, ctypes.byref(w)) == 0
    yield w
    LIB.po_result_free(w)


def info(w):
    out = PoWalkInfo()
    assert LIB.po_walk_info_get(w, ctypes.byref(out)) == 0
    return out.as_dict()


FRESH = {"ploidy": 2, "n_cands": 1, "depth": 0, "start_of_block": 1, "n_block_reads": 0}


def refused(handle, w, call, sentence, walk_of=None):
    cand, ext, rl = np.full(8, 77, np.uint32), np.full(8, 77, np.uint32), np.full(8, 7.5)
    n = ctypes.c_uint64(99)
    st = LIB.po_walk_step(handle, w, ctypes.byref(call.prm), ctypes.byref(call.inp), call.b_ptr, 1, cand.ctypes.data, ext.ctypes.data,
                          rl.ctypes.data, 8, ctypes.byref(n))
    assert st == _lib.PO_ERR_INVALID, st
    assert sentence in LIB.po_last_error(handle).decode(), LIB.po_last_error(handle)
    assert n.value == 0 and set(cand.tolist()) == {77} and set(ext.tolist()) == {77} and set(rl.tolist()) == {7.5}
    assert info(walk_of or w) == FRESH


def test_a_fresh_walk_needs_no_device(handle, walk):
    assert info(walk) == FRESH and LIB.po_result_count(walk) == 0
    out, n, top = np.zeros(4, np.uint32), ctypes.c_uint64(), ctypes.c_double()
    assert LIB.po_walk_best(walk, out.ctypes.data, 4, ctypes.byref(n), ctypes.byref(top)) == 0
    assert n.value == 1 and out[0] == 0 and top.value == -np.inf
    zero = arr([0], np.uint32)
    assert LIB.po_walk_history(walk, zero.ctypes.data, 1, None) == 0
    off, n_ids = np.full(3, 9, np.uint64), ctypes.c_uint64(5)
    assert LIB.po_walk_read_sets(walk, zero.ctypes.data, 1, off.ctypes.data, None, 0, ctypes.byref(n_ids)) == 0
    assert off.tolist() == [0, 0, 0] and n_ids.value == 0
    assert LIB.po_walk_reset(walk) == 0 and info(walk) == FRESH


@pytest.mark.parametrize("ploidy", [0, 9, 2**31])
def test_create_refuses_a_ploidy_outside_1_to_8(handle, ploidy):
    w = ctypes.c_void_p(1)
    assert LIB.po_walk_create(handle, ploidy, ctypes.byref(w)) == _lib.PO_ERR_INVALID and not w.value
    assert "the ploidy must be 1 to 8" in LIB.po_last_error(handle).decode()


def test_a_walk_of_another_handle_or_of_the_wrong_kind(handle, walk):
    other = ctypes.c_void_p()
    assert LIB.po_create(ctypes.byref(other)) == 0
    refused(other, walk, Call(), "the walk belongs to another handle")
    LIB.po_destroy(other)
    rows = ctypes.c_void_p()
    assert LIB.po_result_from_rows(handle, None, 0, ctypes.byref(rows)) == 0
    refused(handle, rows, Call(), "needs the result of po_walk_create", walk_of=walk)
    for fn, args in ((LIB.po_walk_reset, ()), (LIB.po_walk_info_get, (ctypes.byref(PoWalkInfo()),)),
                     (LIB.po_walk_best, (None, 0, ctypes.byref(ctypes.c_uint64()), None)), (LIB.po_walk_history, (None, 0, None)),
                     (LIB.po_walk_read_sets, (None, 0, None, None, 0, ctypes.byref(ctypes.c_uint64())))):
        assert fn(rows, *args) == _lib.PO_ERR_INVALID
        assert "needs the result of po_walk_create" in LIB.po_last_error(handle).decode()
    LIB.po_result_free(rows)
    # ... and the calls that want rows, an index or a graph refuse a walk
    out = ctypes.c_void_p()
    assert LIB.po_phase_index(handle, walk, ctypes.byref(out)) == _lib.PO_ERR_INVALID


def spoil(what):
    c = Call()
    zero = arr([0, 0, 0], np.uint32)
    c.keep = zero
    if what == "set_off":
        c.inp.set_off = zero.ctypes.data
    elif what == "set_ids":
        c.inp.set_ids = zero.ctypes.data
    elif what == "n_cands":
        c.prm.n_cands = 2
    elif what == "start":
        c.prm.start_of_block = 0
    elif what == "ploidy":
        c.prm.ploidy = 3
    elif what == "no_b_reads":
        c.b_ptr = None
    elif what in ("equal", "descending"):
        c.b_reads[:] = [4, 4, 12] if what == "equal" else [4, 12, 9]
    elif what == "reserved":
        c.prm.reserved = 1
    elif what == "threshold":
        c.prm.threshold = -1.0
    elif what == "paths":
        c.prm.n_paths = 65
    elif what == "missing":
        c.inp.path_off = None
    elif what == "offsets":
        c.aln_off[:] = [0, 3, 2]
    elif what == "local_id":
        c.path_ids[2] = 3
    elif what == "levels":
        c.inp.levels = None
    return c


@pytest.mark.parametrize("what,sentence", [
    ("set_off", "set_off and set_ids must be NULL"), ("set_ids", "set_off and set_ids must be NULL"),
    ("n_cands", "n_cands is not the number of candidates the walk holds"), ("start", "start_of_block is not the walk's"),
    ("ploidy", "the ploidy is not the walk's"), ("no_b_reads", "b_reads is missing"), ("equal", "b_reads is not strictly ascending"),
    ("descending", "b_reads is not strictly ascending"),
    # ... and po_phase_branch's own, under this call's name
    ("reserved", "po_walk_step: bad parameters"), ("threshold", "po_walk_step: bad parameters"),
    ("paths", "po_walk_step: the number of paths must be 1 to 64"), ("missing", "po_walk_step: an input array is missing"),
    ("offsets", "po_walk_step: the offsets of the alignments do not start at 0 or decrease"),
    ("local_id", "po_walk_step: a local read id is not below n_b"), ("levels", "po_walk_step: an input array is missing")])
def test_step_refuses(handle, walk, what, sentence):
    refused(handle, walk, spoil(what), sentence)


def test_step_refuses_missing_arguments(handle, walk):
    c = Call()
    n = ctypes.c_uint64(5)
    assert LIB.po_walk_step(handle, walk, ctypes.byref(c.prm), ctypes.byref(c.inp), c.b_ptr, 1, None, None, None, 0, None) == _lib.PO_ERR_INVALID
    assert "no room for the number of entries" in LIB.po_last_error(handle).decode()
    assert LIB.po_walk_step(handle, None, ctypes.byref(c.prm), ctypes.byref(c.inp), c.b_ptr, 1, None, None, None, 0, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    assert "no walk" in LIB.po_last_error(handle).decode() and n.value == 0
    assert LIB.po_walk_step(handle, walk, None, ctypes.byref(c.inp), c.b_ptr, 1, None, None, None, 0, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    assert "no parameters" in LIB.po_last_error(handle).decode()
    assert info(walk) == FRESH


def test_a_candidate_past_the_list_is_refused(handle, walk):
    one = arr([1], np.uint32)
    assert LIB.po_walk_history(walk, one.ctypes.data, 1, None) == _lib.PO_ERR_INVALID
    assert "a candidate is not below the number the walk holds" in LIB.po_last_error(handle).decode()
    n = ctypes.c_uint64(3)
    assert LIB.po_walk_read_sets(walk, one.ctypes.data, 1, None, None, 0, ctypes.byref(n)) == _lib.PO_ERR_INVALID and n.value == 0
    assert LIB.po_walk_read_sets(walk, None, 1, None, None, 0, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    assert LIB.po_walk_best(walk, None, 0, None, None) == _lib.PO_ERR_INVALID
    assert LIB.po_walk_read_sets(walk, None, 0, None, None, 0, None) == _lib.PO_ERR_INVALID
