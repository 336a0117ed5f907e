"""What a rejected po_layout_superbubbles_all call says and leaves behind: every PO_ERR_INVALID path in front of the device
with its sentence written out, the outputs untouched; without a GPU a call that passes them returns PO_ERR_HIP.  An edge
end outside the node order never reaches the call through po_graph_from_edges, which refuses the graph and writes nothing;
behind the ranks the call counts such an edge as its siblings do (n_invalid, ranked_open), and the plain-Python statement
raises."""
import ctypes

import numpy as np
import pytest

from phasm_amd import _lib, cyclic
from test_components_rejections import FILL, _have_gpu, from_edges, three_segments
from test_layout_rejections import segment_handle


def all_call(ov, graph_ptr, reserved=0, want_count=True):
    lib = _lib.load()
    bufs = [np.full(64, FILL, dtype=np.uint8) for _ in range(4)]
    n = ctypes.c_uint64(77)
    prm = _lib.PoSuperbubbleAllParams(reserved)
    status = lib.po_layout_superbubbles_all(ov._h, graph_ptr, ctypes.byref(prm), *[b.ctypes.data_as(ctypes.c_void_p) for b in bufs],
                                            ctypes.byref(n) if want_count else None)
    return status, lib.po_last_error(ov._h).decode(), bufs, n.value


def all_rejected(ov, graph, message, reserved=0, want_count=True):
    status, said, bufs, n = all_call(ov, graph._ptr, reserved, want_count)
    assert status == _lib.PO_ERR_INVALID and said == message
    assert all((b == FILL).all() for b in bufs)
    assert n == (0 if want_count else 77)


def test_checks_in_front_of_the_device_keep_their_sentences():
    mine, my_rows = segment_handle("x")
    other, other_rows = segment_handle("y")
    all_rejected(mine, my_rows, "po_layout_superbubbles_all: no room for the number of superbubbles", want_count=False)
    all_rejected(mine, other_rows, "po_layout_superbubbles_all: the graph belongs to another handle")
    all_rejected(mine, my_rows, "po_layout_superbubbles_all: bad parameters", reserved=1)
    all_rejected(mine, my_rows, "po_layout_superbubbles_all needs an edge result, a merged graph or a po_graph_from_edges result")
    lib = _lib.load()
    n = ctypes.c_uint64()
    assert lib.po_layout_superbubbles_all(mine._h, None, None, None, None, None, None, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    assert lib.po_layout_superbubbles_all(None, my_rows._ptr, None, None, None, None, None, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    st = _lib.PoSuperbubbleAllStats()
    assert lib.po_get_superbubble_all_stats(mine._h, None) == _lib.PO_ERR_INVALID
    assert lib.po_get_superbubble_all_stats(mine._h, ctypes.byref(st)) == _lib.PO_OK and st.n_bubbles == 0 and st.n_root_runs == 0
    assert ctypes.sizeof(_lib.PoSuperbubbleAllStats) == 120 and ctypes.sizeof(_lib.PoSuperbubbleAllParams) == 4
    assert lib.po_abi_version() == 4
    for r in (my_rows, other_rows):
        r.free()
    mine.close()
    other.close()


def test_an_edge_end_outside_the_node_order_writes_nothing():
    ov = three_segments()
    status, said, out = from_edges(ov, [(0, 2), (2, 4)], [0, 2])
    assert status == _lib.PO_ERR_INVALID and said == "po_graph_from_edges: an edge has an end that is not in the node order"
    assert out.value is None                                    # no graph result: nothing the call could be given
    with pytest.raises(ValueError, match="an edge has an end that is not in the node order"):
        cyclic.HostSuperbubblesAll([(0, 2), (2, 4)], [0, 2])
    with pytest.raises(ValueError, match="repeats a node"):
        cyclic.HostSuperbubblesAll([(0, 2)], [0, 2, 0])
    ov.close()


@pytest.mark.skipif(_have_gpu(), reason="checks the no-GPU failure mode")
def test_valid_calls_fail_loudly_without_a_gpu():
    ov = three_segments()
    status, _, out = from_edges(ov, [(0, 2)], [0, 2])          # (no graph result without a device ...)
    assert status == _lib.PO_ERR_HIP and out.value is None
    rows = ov.result_from_rows(np.zeros((0, 6), dtype=np.int64))
    status, _, bufs, n = all_call(ov, rows._ptr)               # (... and a row result is turned away first)
    assert status == _lib.PO_ERR_INVALID and n == 0
    with pytest.raises(Exception):
        ov.layout_superbubbles_all(rows, 0)
    rows.free()
    ov.close()


@pytest.mark.gpu
def test_the_checks_behind_the_device():
    ov = three_segments()
    g = ov.graph_from_edges(np.asarray([[0, 2, 100, 17], [2, 4, 100, 17], [4, 0, 100, 17]]), [4, 2, 0])
    all_rejected(ov, g, "po_layout_superbubbles_all: bad parameters", reserved=3)
    node_exit, node_inside, flags, table = ov.layout_superbubbles_all(g)
    assert table.tolist() == [(4, 0, 0, 0), (2, 4, 0, 0), (0, 2, 0, 0)] and node_exit.tolist() == [0, 4, 2]
    assert node_inside.tolist() == [_lib.NO_NODE] * 3 and flags.tolist() == [_lib.SB_ENTRANCE | _lib.SB_EXIT] * 3
    g.free()
    ov.close()
