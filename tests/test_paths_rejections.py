"""What a rejected po_phase_paths call says and leaves behind: every PO_ERR_INVALID path in front of the device with its
sentence written out, *out NULL; without a GPU a call that passes them returns PO_ERR_HIP.  (An edge end outside the node
order is refused behind the ranks, on the device: below under the gpu mark and, for the kernels,
tests/test_paths_host_emulation.py.)"""
import ctypes

import numpy as np
import pytest

from phasm_amd import _lib
from test_components_rejections import _have_gpu, from_edges, three_segments
from test_layout_rejections import segment_handle


def paths_call(ov, graph_ptr, max_paths=4, reserved=0, want_out=True):
    lib = _lib.load()
    out = ctypes.c_void_p(77)
    prm = _lib.PoPathsParams(max_paths, reserved)
    status = lib.po_phase_paths(ov._h, graph_ptr, ctypes.byref(prm), ctypes.byref(out) if want_out else None)
    return status, lib.po_last_error(ov._h).decode(), out.value


def paths_rejected(ov, graph, message, reserved=0, want_out=True):
    status, said, out = paths_call(ov, graph._ptr, 4, reserved, want_out)
    assert status == _lib.PO_ERR_INVALID and said == message
    assert out == (None if want_out else 77)


def test_paths_checks_in_front_of_the_device_keep_their_sentences():
    mine, my_rows = segment_handle("x")
    other, other_rows = segment_handle("y")
    paths_rejected(mine, my_rows, "po_phase_paths: no room for the result", want_out=False)
    paths_rejected(mine, other_rows, "po_phase_paths: the graph belongs to another handle")
    paths_rejected(mine, my_rows, "po_phase_paths: bad parameters", reserved=1)
    paths_rejected(mine, my_rows, "po_phase_paths needs an edge result, a merged graph or a po_graph_from_edges result")
    with pytest.raises(ValueError, match="needs an edge result"):
        mine.phase_paths(my_rows, 4)
    with pytest.raises(ValueError, match="64 bits"):
        mine.phase_paths(my_rows, 1 << 64)
    lib = _lib.load()
    out = ctypes.c_void_p()
    assert lib.po_phase_paths(None, my_rows._ptr, None, ctypes.byref(out)) == _lib.PO_ERR_INVALID
    status, said, _ = paths_call(mine, None)
    assert status == _lib.PO_ERR_INVALID and said == "po_phase_paths: no graph"
    # the accessors turn away a result of another kind
    dims = _lib.PoPathsDims()
    assert lib.po_paths_sizes(my_rows._ptr, ctypes.byref(dims)) == _lib.PO_ERR_INVALID
    assert lib.po_last_error(mine._h).decode() == "po_paths_sizes needs the result of po_phase_paths"
    assert lib.po_paths_copy(my_rows._ptr, *[None] * 9) == _lib.PO_ERR_INVALID
    assert lib.po_last_error(mine._h).decode() == "po_paths_copy needs the result of po_phase_paths"
    assert lib.po_paths_sizes(None, ctypes.byref(dims)) == _lib.PO_ERR_INVALID and lib.po_paths_copy(None, *[None] * 9) == _lib.PO_ERR_INVALID
    st = _lib.PoPathsStats()
    assert lib.po_get_paths_stats(mine._h, None) == _lib.PO_ERR_INVALID
    assert lib.po_get_paths_stats(mine._h, ctypes.byref(st)) == _lib.PO_OK and st.n_bubbles == 0 and st.n_batches == 0
    assert ctypes.sizeof(_lib.PoPathsStats) == 12 * 8 + 2 * 4 + 4 * 4 and _lib.BUBBLE_PATHS_DTYPE.itemsize == 40
    assert ctypes.sizeof(_lib.PoPathsParams) == 16 and ctypes.sizeof(_lib.PoPathsDims) == 40
    for r in (my_rows, other_rows):
        r.free()
    mine.close()
    other.close()


@pytest.mark.skipif(_have_gpu(), reason="checks the no-GPU failure mode")
def test_valid_calls_fail_loudly_without_a_gpu():
    ov = three_segments()
    status, _, out = from_edges(ov, [(0, 2)], [0, 2])          # (no graph result without a device ...)
    assert status == _lib.PO_ERR_HIP and out.value is None
    rows = ov.result_from_rows(np.zeros((0, 6), dtype=np.int64))
    status, _, out = paths_call(ov, rows._ptr)                 # (... and a row result is turned away first)
    assert status == _lib.PO_ERR_INVALID and out is None
    with pytest.raises(Exception):
        ov.phase_paths(rows, 4)
    rows.free()
    ov.close()


@pytest.mark.gpu
def test_the_checks_behind_the_device():
    ov = three_segments()
    g = ov.graph_from_edges(np.asarray([[0, 2, 100, 17], [2, 4, 101, 17]]), [4, 2, 0])
    paths_rejected(ov, g, "po_phase_paths: bad parameters", reserved=3)
    bp = ov.phase_paths(g, 4)
    assert bp.bubbles.tolist() == [(0, 2, 0, 0, 0, _lib.PATHS_BARE, 1, 2), (2, 4, 0, 1, 0, _lib.PATHS_BARE, 1, 2)]
    assert bp.paths_of(0) == [(0, 2)] and bp.paths_of(1) == [(2, 4)] and bp.preds_of(1) == [(2, 101)] and bp.interior_of(0) == []
    assert ov.paths_stats()["n_bare"] == 2 and ov.paths_stats()["n_stray_edges"] == 0
    # a graph is no result of po_phase_paths
    lib = _lib.load()
    dims = _lib.PoPathsDims()
    assert lib.po_paths_sizes(g._ptr, ctypes.byref(dims)) == _lib.PO_ERR_INVALID
    g.free()
    ov.close()
