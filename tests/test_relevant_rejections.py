"""What a rejected po_phase_index / po_phase_relevant call says and leaves behind: every PO_ERR_INVALID path with its sentence
written out and no result -- all of them checked on the host before the device is touched, so they are held here without a GPU;
a VALID po_phase_index call without a GPU returns PO_ERR_HIP (an index, and so a valid po_phase_relevant call, cannot exist
there)."""
import ctypes

import numpy as np
import pytest

import relevant_utils as ru
from phasm_amd import _lib, phasing
from phasm_amd.overlapper import ExactOverlapper
from test_components_rejections import _have_gpu

NAME = "po_phase_relevant: "


def handle(n_seg=4):
    ov = ExactOverlapper()
    ru.add_reads(ov, [100] * n_seg)
    return ov


def some_rows(ov):
    return ov.result_from_rows(ru.rows_array([(0, 2, 1, 10, 2, 11), (4, 6, 1, 10, 2, 11)]))


def call(ov, index_ptr, want_out=True, want_params=True, want_input=True, mode=0, reserved=0, reserved2=0, cur=(0,), prev_graph=(),
         prev_aligning=(), pred=(), pred_len=(), drop=()):
    lib = _lib.load()
    arrays = {"cur": np.asarray(cur, np.uint32), "prev_graph": np.asarray(prev_graph, np.uint32),
              "prev_aligning": np.asarray(prev_aligning, np.uint32), "pred": np.asarray(pred, np.uint32), "pred_len": np.asarray(pred_len, np.int32)}
    p = lambda k: None if k in drop or not len(arrays[k]) else arrays[k].ctypes.data   # noqa: E731
    prm = _lib.PoRelevantParams(mode, 1, reserved, reserved2)
    inp = _lib.PoRelevantInput(p("cur"), len(cur), p("prev_graph"), len(prev_graph), p("prev_aligning"), len(prev_aligning), p("pred"),
                               p("pred_len"), len(pred))
    out = ctypes.c_void_p(0x77)
    status = lib.po_phase_relevant(ov._h, index_ptr, ctypes.byref(prm) if want_params else None, ctypes.byref(inp) if want_input else None,
                                   ctypes.byref(out) if want_out else None)
    return status, lib.po_last_error(ov._h).decode(), out.value


def rejected(ov, index_ptr, message, want_out=True, **kw):
    status, said, out = call(ov, index_ptr, want_out=want_out, **kw)
    assert status == _lib.PO_ERR_INVALID and said == message, said
    assert out == (None if want_out else 0x77)          # no result


def test_relevant_checks_in_front_of_the_device_keep_their_sentences():
    ov, other = handle(), handle()
    rows, foreign = some_rows(ov), some_rows(other)
    r = rows._ptr                                        # (a row result stands where the index goes: its kind is checked last)
    rejected(ov, r, NAME + "no room for the result", want_out=False)
    rejected(ov, None, NAME + "no index")
    rejected(ov, r, NAME + "no parameters", want_params=False)
    rejected(ov, r, NAME + "no parameters", want_input=False)
    rejected(ov, r, NAME + "bad parameters", reserved=1)
    rejected(ov, r, NAME + "bad parameters", reserved2=7)
    rejected(ov, r, NAME + "the mode must be 0 (spanning) or 1 (all)", mode=2)
    for key, kw in (("cur", {}), ("prev_graph", {"prev_graph": (1,)}), ("prev_aligning", {"prev_aligning": (1,)}),
                    ("pred", {"pred": (1,), "pred_len": (5,)}), ("pred_len", {"pred": (1,), "pred_len": (5,)})):
        rejected(ov, r, NAME + "a list is missing", drop=(key,), **kw)
    for kw in ({"cur": (8,)}, {"prev_graph": (0, 8)}, {"prev_aligning": (0xFFFFFFFF,)}, {"pred": (8,), "pred_len": (5,)}):
        rejected(ov, r, NAME + "a list names a read the handle does not hold", **kw)
    rejected(ov, foreign._ptr, NAME + "the index belongs to another handle")
    rejected(ov, r, NAME + "needs the result of po_phase_index")
    lib = _lib.load()
    out = ctypes.c_void_p()
    assert lib.po_phase_relevant(None, None, None, None, ctypes.byref(out)) == _lib.PO_ERR_INVALID
    # the index call and the read-outs
    assert lib.po_phase_index(ov._h, None, ctypes.byref(out)) == _lib.PO_ERR_INVALID
    assert lib.po_phase_index(ov._h, r, None) == _lib.PO_ERR_INVALID
    out = ctypes.c_void_p(0x77)
    assert lib.po_phase_index(ov._h, foreign._ptr, ctypes.byref(out)) == _lib.PO_ERR_INVALID and out.value is None
    assert lib.po_last_error(ov._h).decode() == "po_phase_index: the rows belong to another handle"
    n = ctypes.c_uint64(77)
    assert lib.po_phase_index_copy(r, None, None, 0, None) == _lib.PO_ERR_INVALID
    assert lib.po_last_error(ov._h).decode() == "po_phase_index_copy: no room for the number of entries"
    assert lib.po_phase_index_copy(r, None, None, 0, ctypes.byref(n)) == _lib.PO_ERR_INVALID and n.value == 0
    assert lib.po_last_error(ov._h).decode() == "po_phase_index_copy needs the result of po_phase_index"
    d = _lib.PoRelevantDims()
    assert lib.po_relevant_sizes(r, ctypes.byref(d)) == _lib.PO_ERR_INVALID
    assert lib.po_last_error(ov._h).decode() == "po_relevant_sizes needs the result of po_phase_relevant"
    assert lib.po_relevant_copy(r, *[None] * 8) == _lib.PO_ERR_INVALID
    assert lib.po_last_error(ov._h).decode() == "po_relevant_copy needs the result of po_phase_relevant"
    assert lib.po_relevant_sizes(None, ctypes.byref(d)) == _lib.PO_ERR_INVALID and lib.po_relevant_sizes(r, None) == _lib.PO_ERR_INVALID
    xs, rs = _lib.PoPhaseIndexStats(), _lib.PoRelevantStats()
    assert lib.po_get_phase_index_stats(ov._h, None) == _lib.PO_ERR_INVALID and lib.po_get_relevant_stats(ov._h, None) == _lib.PO_ERR_INVALID
    assert lib.po_get_phase_index_stats(ov._h, ctypes.byref(xs)) == _lib.PO_OK and xs.n_keys == 0
    assert lib.po_get_relevant_stats(ov._h, ctypes.byref(rs)) == _lib.PO_OK and rs.n_relevant == 0
    assert ctypes.sizeof(_lib.PoRelevantParams) == 16 and ctypes.sizeof(_lib.PoRelevantInput) == 72
    assert ctypes.sizeof(_lib.PoRelevantDims) == 48 and ctypes.sizeof(_lib.PoRelevantStats) == 64 and ctypes.sizeof(_lib.PoPhaseIndexStats) == 48
    assert _lib.ALIGNMENT_DTYPE.itemsize == 16 and phasing.ALIGNMENT_DTYPE == _lib.ALIGNMENT_DTYPE
    with pytest.raises(ValueError, match="32 bits"):
        ov.phase_relevant(rows, [0], mode=-1)
    with pytest.raises(ValueError, match="needs the result of po_phase_index"):
        ov.phase_relevant(rows, [0])
    for x in (rows, foreign):
        x.free()
    ov.close()
    other.close()


def test_the_host_index_refuses_what_the_library_refuses():
    host = phasing.HostIndex([100] * 8)
    with pytest.raises(ValueError, match="a row names a read the handle does not hold"):
        host.phase_index(np.array([[0, 8, 1, 2, 3, 4]]))
    index = host.phase_index(np.array([[0, 2, 1, 2, 3, 4]]))
    with pytest.raises(ValueError, match="a list names a read the handle does not hold"):
        host.phase_relevant(index, [8])
    with pytest.raises(ValueError, match="the mode must be 0"):
        host.phase_relevant(index, [0], mode=2)


def test_a_valid_index_call_needs_a_gpu():
    """No CPU fallback: without a GPU the valid call fails loudly and leaves no result; with one it succeeds."""
    ov = handle()
    rows = some_rows(ov)
    out = ctypes.c_void_p(0x77)
    status = _lib.load().po_phase_index(ov._h, rows._ptr, ctypes.byref(out))
    if _have_gpu():
        assert status == _lib.PO_OK and out.value
        _lib.load().po_result_free(out)
    else:
        assert status == _lib.PO_ERR_HIP and out.value is None and "no HIP device" in _lib.load().po_last_error(ov._h).decode()
    rows.free()
    ov.close()
