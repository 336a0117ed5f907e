"""What a rejected po_layout_contigs call says and leaves behind: every PO_ERR_INVALID path in front of the device with its
sentence written out, the outputs untouched; without a GPU a call that passes them returns PO_ERR_HIP.  (An edge end outside
the node order is refused behind the ranks, on the device: tests/test_gpu_contigs.py and, for the kernels,
tests/test_contigs_host_emulation.py.)"""
import ctypes

import numpy as np
import pytest

from phasm_amd import _lib
from test_components_rejections import FILL, _have_gpu, from_edges, three_segments
from test_layout_rejections import segment_handle


def contigs_call(ov, graph_ptr, min_len=5000, min_nodes=1, reserved=0, want_count=True, exclude=None):
    lib = _lib.load()
    bufs = [np.full(64 * 24, FILL, dtype=np.uint8) for _ in range(3)]
    n = ctypes.c_uint64(77)
    prm = _lib.PoContigParams(min_len, min_nodes, reserved)
    status = lib.po_layout_contigs(ov._h, graph_ptr, ctypes.byref(prm), exclude.ctypes.data_as(ctypes.c_void_p) if exclude is not None else None,
                                   *[b.ctypes.data_as(ctypes.c_void_p) for b in bufs], ctypes.byref(n) if want_count else None)
    return status, lib.po_last_error(ov._h).decode(), bufs, n.value


def contigs_rejected(ov, graph, message, want_count=True, **kw):
    status, said, bufs, n = contigs_call(ov, graph._ptr, want_count=want_count, **kw)
    assert status == _lib.PO_ERR_INVALID and said == message
    assert all((b == FILL).all() for b in bufs)
    assert n == (0 if want_count else 77)


def test_contigs_checks_in_front_of_the_device_keep_their_sentences():
    mine, my_rows = segment_handle("x")
    other, other_rows = segment_handle("y")
    contigs_rejected(mine, my_rows, "po_layout_contigs: no room for the number of contigs", want_count=False)
    contigs_rejected(mine, other_rows, "po_layout_contigs: the graph belongs to another handle")
    contigs_rejected(mine, my_rows, "po_layout_contigs: bad parameters", reserved=1)
    contigs_rejected(mine, my_rows, "po_layout_contigs: bad parameters", min_nodes=0)
    contigs_rejected(mine, my_rows, "po_layout_contigs: bad parameters", min_nodes=0, exclude=np.zeros(8, dtype=np.uint8))
    contigs_rejected(mine, my_rows, "po_layout_contigs needs an edge result, a merged graph or a po_graph_from_edges result")
    contigs_rejected(mine, my_rows, "po_layout_contigs needs an edge result, a merged graph or a po_graph_from_edges result", min_len=0)
    with pytest.raises(ValueError, match="bad parameters"):
        mine.layout_contigs(my_rows, 5000, 0, None, 0)
    with pytest.raises(ValueError, match="32 bits"):
        mine.layout_contigs(my_rows, 5000, 1 << 32, None, 0)
    with pytest.raises(ValueError, match="64 bits"):
        mine.layout_contigs(my_rows, 1 << 64, 1, None, 0)
    with pytest.raises(ValueError, match="64 bits"):
        mine.layout_contigs(my_rows, -1, 1, None, 0)
    with pytest.raises(ValueError, match="one entry per node"):
        mine.layout_contigs(my_rows, 5000, 1, [1, 0, 1], 2)
    lib = _lib.load()
    n = ctypes.c_uint64()
    assert lib.po_layout_contigs(mine._h, None, None, None, None, None, None, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    assert lib.po_layout_contigs(None, my_rows._ptr, None, None, None, None, None, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    st = _lib.PoContigStats()
    assert lib.po_get_contig_stats(mine._h, None) == _lib.PO_ERR_INVALID
    assert lib.po_get_contig_stats(mine._h, ctypes.byref(st)) == _lib.PO_OK and st.n_contigs == 0 and st.n_batches == 0
    assert ctypes.sizeof(_lib.PoContigStats) == 168 and _lib.CONTIG_DTYPE.itemsize == 24 and ctypes.sizeof(_lib.PoContigParams) == 16
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
    status, _, bufs, n = contigs_call(ov, rows._ptr)           # (... and a row result is turned away first)
    assert status == _lib.PO_ERR_INVALID and n == 0
    with pytest.raises(Exception):
        ov.layout_contigs(rows, 5000, 1, None, 0)
    rows.free()
    ov.close()


@pytest.mark.gpu
def test_the_checks_behind_the_device():
    ov = three_segments()
    g = ov.graph_from_edges(np.asarray([[0, 2, 100, 17], [2, 4, 100, 17]]), [4, 2, 0])
    contigs_rejected(ov, g, "po_layout_contigs: bad parameters", reserved=3)
    contigs_rejected(ov, g, "po_layout_contigs: bad parameters", min_nodes=0)
    lengths = ov.lengths()
    # the path 0 -> 2 -> 4 is one bubble chain: with its nodes excluded the one start is blocked
    edge_contig, edge_pos, table = ov.layout_contigs(g, 0)
    assert len(table) == 0 and edge_contig.tolist() == edge_pos.tolist() == [_lib.NO_NODE] * 2
    st = ov.contig_stats()
    assert (st["n_chains"], st["n_excluded"], st["n_blocked"], st["n_uncovered_edges"]) == (1, 3, 1, 2)
    edge_contig, edge_pos, table = ov.layout_contigs(g, 0, exclude=[0, 0, 0])
    assert table.tolist() == [(0, 4, 3, 0, 200 + int(lengths[2]))] and edge_contig.tolist() == [0, 0] and edge_pos.tolist() == [0, 1]
    edge_contig, edge_pos, table = ov.layout_contigs(g, 200 + int(lengths[2]) + 1, exclude=[0, 0, 0])
    assert len(table) == 0 and ov.contig_stats()["n_short_paths"] == 1
    g.free()
    ov.close()
