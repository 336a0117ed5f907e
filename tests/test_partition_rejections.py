"""What a rejected po_layout_partition call says and leaves behind: every PO_ERR_INVALID path with its sentence written out,
the outputs untouched.  The checks come in front of the device, so they are held here without a GPU."""
import ctypes

import numpy as np
import pytest

from phasm_amd import _lib
from test_components_rejections import FILL, _have_gpu, three_segments
from test_layout_rejections import segment_handle


def partition_call(ov, graph_ptr, reserved=0, want_count=True):
    lib = _lib.load()
    bufs = [np.full(64, FILL, dtype=np.uint8) for _ in range(4)]
    n = ctypes.c_uint64(77)
    prm = _lib.PoPartitionParams(reserved)
    status = lib.po_layout_partition(ov._h, graph_ptr, ctypes.byref(prm), *[b.ctypes.data_as(ctypes.c_void_p) for b in bufs],
                                     ctypes.byref(n) if want_count else None)
    return status, lib.po_last_error(ov._h).decode(), bufs, n.value


def partition_rejected(ov, graph, message, reserved=0, want_count=True):
    status, said, bufs, n = partition_call(ov, graph._ptr, reserved, want_count)
    assert status == _lib.PO_ERR_INVALID and said == message
    assert all((b == FILL).all() for b in bufs)
    assert n == (0 if want_count else 77)


def test_partition_checks_in_front_of_the_device_keep_their_sentences():
    mine, my_rows = segment_handle("x")
    other, other_rows = segment_handle("y")
    partition_rejected(mine, my_rows, "po_layout_partition: no room for the number of strongly connected components", want_count=False)
    partition_rejected(mine, other_rows, "po_layout_partition: the graph belongs to another handle")
    partition_rejected(mine, my_rows, "po_layout_partition: bad parameters", reserved=1)
    partition_rejected(mine, my_rows, "po_layout_partition needs an edge result, a merged graph or a po_graph_from_edges result")
    lib = _lib.load()
    n = ctypes.c_uint64()
    assert lib.po_layout_partition(mine._h, None, None, None, None, None, None, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    assert lib.po_layout_partition(None, my_rows._ptr, None, None, None, None, None, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    for r in (my_rows, other_rows):
        r.free()
    mine.close()
    other.close()


def test_the_stats_struct_is_the_header_s():
    # 15 64-bit counts, 5 32-bit counts, 4 times, padded to the alignment of the counts; the table entry is 24 bytes
    assert ctypes.sizeof(_lib.PoPartitionStats) == 160 and _lib.PoPartitionStats.n_invalid.offset == 112
    assert _lib.PoPartitionStats.n_outer.offset == 120 and _lib.PoPartitionStats.ms_total.offset == 152
    assert _lib.SCC_DTYPE.itemsize == 24 and (_lib.PART_R_IN, _lib.PART_RE_OUT, _lib.PART_START, _lib.PART_SINK) == (1, 2, 4, 8)
    ov = three_segments()
    assert ov.partition_stats()["n_class"] == [0] * 5 and ov.partition_stats()["n_sccs"] == 0
    ov.close()


@pytest.mark.skipif(_have_gpu(), reason="checks the no-GPU failure mode")
def test_a_row_result_is_turned_away_before_the_device_is_asked_for():
    ov = three_segments()
    rows = ov.result_from_rows(np.zeros((0, 6), dtype=np.int64))
    status, said, _, _ = partition_call(ov, rows._ptr)
    assert status == _lib.PO_ERR_INVALID and said.startswith("po_layout_partition needs")
    rows.free()
    ov.close()


@pytest.mark.gpu
def test_bad_parameters_on_a_graph_that_the_call_takes():
    ov = three_segments()
    g = ov.graph_from_edges(np.asarray([[0, 2, 100, 17], [2, 0, 100, 17], [2, 4, 100, 17]]), [4, 2, 0])
    partition_rejected(ov, g, "po_layout_partition: bad parameters", reserved=3)
    nodes, flags, classes, table = ov.layout_partition(g)
    assert nodes.tolist() == [0, 1, 1] and classes.tolist() == [0, 0, 3] and table.tolist() == [(4, 1, 0, 1, 0), (2, 2, 2, 0, 1)]
    assert flags.tolist() == [_lib.PART_R_IN | _lib.PART_SINK, _lib.PART_RE_OUT, 0]
    g.free()
    ov.close()
