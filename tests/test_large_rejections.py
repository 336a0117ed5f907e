"""What a rejected po_phase_large or po_paths_copy_paths call says and leaves behind: every PO_ERR_INVALID path with its sentence
written out, in the order the header lists them, *n_best_out 0 and the outputs untouched.  The checks that need a paths result
(which only a device makes) stand under the gpu mark; without a GPU a call that passes the others returns PO_ERR_HIP."""
import ctypes

import numpy as np
import pytest

import paths_utils as pp
from phasm_amd import _lib
from test_components_rejections import _have_gpu, three_segments
from test_layout_rejections import segment_handle

FILL = 0x5A


def valid(n_nodes=0):
    """The arrays of a small valid call: two relevant reads, three alignments, ``n_nodes`` interior nodes of one read each."""
    u32, i32 = (lambda v: np.asarray(v, dtype=np.uint32)), (lambda v: np.asarray(v, dtype=np.int32))
    return {"overlap_max": i32([900, 800]), "aln_off": u32([0, 2, 3]), "aln_b": u32([0, 1, 2]), "aln_a0": i32([5, 50, 7]),
            "aln_a1": i32([300, 400, 500]), "node_off": u32(np.arange(n_nodes + 1)), "node_ids": u32(np.arange(n_nodes) % 3),
            "n_nodes": n_nodes, "bubble": 0, "n_reads": 2, "n_b": 3, "n_best": 2, "reserved": 0}


def large_call(ov, paths_ptr, a, want=("params", "input", "best", "scores", "n")):
    lib = _lib.load()
    prm = _lib.PoLargeParams(a["bubble"], a["n_reads"], a["n_b"], a["n_best"], a["reserved"])
    ptr = lambda x: None if x is None or not len(x) else x.ctypes.data   # noqa: E731
    inp = _lib.PoLargeInput(*[ptr(a[k]) for k in ("overlap_max", "aln_off", "aln_b", "aln_a0", "aln_a1", "node_off", "node_ids")], a["n_nodes"])
    best, best_scores = np.full(8, FILL, dtype=np.uint64), np.full(8, float(FILL))
    n = ctypes.c_uint32(77)
    status = lib.po_phase_large(ov._h, paths_ptr, ctypes.byref(prm) if "params" in want else None, ctypes.byref(inp) if "input" in want else None,
                                best.ctypes.data if "best" in want else None, best_scores.ctypes.data if "scores" in want else None, None,
                                ctypes.byref(n) if "n" in want else None)
    untouched = bool((best == FILL).all() and (best_scores == float(FILL)).all())
    return status, lib.po_last_error(ov._h).decode(), n.value, untouched


def rejected(ov, result, message, want=("params", "input", "best", "scores", "n"), **change):
    a = valid(change.pop("n_nodes", 0))
    a.update(change)
    status, said, n, untouched = large_call(ov, result._ptr if result is not None else None, a, want)
    assert status == _lib.PO_ERR_INVALID and said == message, (status, said)
    assert n == (0 if "n" in want else 77) and untouched


def host_checks(ov, result):
    """The rejections that need no paths result, in the header's order."""
    u32 = lambda v: np.asarray(v, dtype=np.uint32)   # noqa: E731
    rejected(ov, result, "po_phase_large: no room for the number of best paths", want=("params", "input", "best", "scores"))
    rejected(ov, None, "po_phase_large: no paths result")
    rejected(ov, result, "po_phase_large: no parameters", want=("input", "best", "scores", "n"))
    rejected(ov, result, "po_phase_large: no parameters", want=("params", "best", "scores", "n"))
    rejected(ov, result, "po_phase_large: no room for the best paths", want=("params", "input", "scores", "n"))
    rejected(ov, result, "po_phase_large: no room for the best paths", want=("params", "input", "best", "n"))
    rejected(ov, result, "po_phase_large: bad parameters", reserved=1)
    rejected(ov, result, "po_phase_large: n_best must be 1 to 8", n_best=0)
    rejected(ov, result, "po_phase_large: n_best must be 1 to 8", n_best=9)
    rejected(ov, result, "po_phase_large: there must be at least one relevant read", n_reads=0)
    for key in ("overlap_max", "aln_off", "node_off", "aln_b", "aln_a0", "aln_a1"):
        rejected(ov, result, "po_phase_large: an input array is missing", **{key: None})
    rejected(ov, result, "po_phase_large: an input array is missing", n_nodes=2, node_ids=None)
    rejected(ov, result, "po_phase_large: the offsets of the alignments do not start at 0 or decrease", aln_off=u32([1, 2, 3]))
    rejected(ov, result, "po_phase_large: the offsets of the alignments do not start at 0 or decrease", aln_off=u32([0, 3, 2]))
    rejected(ov, result, "po_phase_large: the offsets of the interior nodes do not start at 0 or decrease", n_nodes=2, node_off=u32([1, 1, 2]))
    rejected(ov, result, "po_phase_large: the offsets of the interior nodes do not start at 0 or decrease", n_nodes=2, node_off=u32([0, 2, 1]))
    rejected(ov, result, "po_phase_large: a local read id is not below n_b", aln_b=u32([0, 3, 2]))
    rejected(ov, result, "po_phase_large: a local read id is not below n_b", n_nodes=2, node_ids=u32([0, 3]))
    rejected(ov, result, "po_phase_large: a local read id is not below n_b", n_b=2)


def test_large_checks_in_front_of_the_device_keep_their_sentences():
    mine, my_rows = segment_handle("x")
    host_checks(mine, my_rows)
    rejected(mine, my_rows, "po_phase_large needs the result of po_phase_paths")
    lib = _lib.load()
    assert large_call(mine, my_rows._ptr, valid())[0] == _lib.PO_ERR_INVALID
    prm, inp, n = _lib.PoLargeParams(), _lib.PoLargeInput(), ctypes.c_uint32()
    assert lib.po_phase_large(None, my_rows._ptr, ctypes.byref(prm), ctypes.byref(inp), None, None, None, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    # the ranged copy turns away a result of another kind
    nodes = ctypes.c_uint64(77)
    assert lib.po_paths_copy_paths(my_rows._ptr, 0, 0, None, None, 0, ctypes.byref(nodes)) == _lib.PO_ERR_INVALID and nodes.value == 0
    assert lib.po_last_error(mine._h).decode() == "po_paths_copy_paths needs the result of po_phase_paths"
    assert lib.po_paths_copy_paths(my_rows._ptr, 0, 0, None, None, 0, None) == _lib.PO_ERR_INVALID
    assert lib.po_last_error(mine._h).decode() == "po_paths_copy_paths: no room for the number of nodes"
    assert lib.po_paths_copy_paths(None, 0, 0, None, None, 0, ctypes.byref(nodes)) == _lib.PO_ERR_INVALID
    st = _lib.PoLargeStats()
    assert lib.po_get_large_stats(mine._h, None) == _lib.PO_ERR_INVALID
    assert lib.po_get_large_stats(mine._h, ctypes.byref(st)) == _lib.PO_OK and st.n_paths == 0 and st.ms_total == 0.0
    assert ctypes.sizeof(_lib.PoLargeParams) == 20 and ctypes.sizeof(_lib.PoLargeInput) == 64 and ctypes.sizeof(_lib.PoLargeStats) == 48
    my_rows.free()
    mine.close()


@pytest.mark.skipif(_have_gpu(), reason="checks the no-GPU failure mode")
def test_python_layer_without_a_gpu():
    ov = three_segments()
    rows = ov.result_from_rows(np.zeros((0, 6), dtype=np.int64))
    with pytest.raises(Exception):
        ov.phase_paths_resident(rows, 4)
    with pytest.raises(ValueError, match="64 bits"):
        ov.phase_paths_resident(rows, 1 << 64)
    assert ov.large_stats()["n_paths"] == 0
    rows.free()
    ov.close()


@pytest.mark.gpu
def test_the_checks_that_need_a_paths_result():
    from test_gpu_paths import graph_of
    edges = pp._w(pp.many_paths(3))                        # 9 paths, 11 interior nodes
    ov, g = graph_of(pp.first_seen(edges), edges)
    other, other_rows = segment_handle("y")
    listed, counted = ov.phase_paths_resident(g, 16), ov.phase_paths_resident(g, 4)
    g.free()
    n_inside = int(listed.bubbles["n_inside"][0])
    host_checks(ov, listed)
    rejected(other, listed, "po_phase_large: the paths result belongs to another handle")
    rejected(ov, listed, "po_phase_large: bubble 1 is not below the 1 bubbles of the result", bubble=1, n_nodes=n_inside)
    rejected(ov, counted, "po_phase_large: the paths of bubble 0 were not listed (more than max_paths)", n_nodes=n_inside)
    rejected(ov, listed, "po_phase_large: n_nodes is 3, bubble 0 has %d interior nodes" % n_inside, n_nodes=3)
    status, said, n, _ = large_call(ov, listed._ptr, dict(valid(n_inside)))
    assert status == _lib.PO_OK and n == 2, said
    # the ranged copy: a range past the listed paths, too small a cap (which still says how many nodes there are)
    lib = _lib.load()
    nodes = ctypes.c_uint64(77)
    assert lib.po_paths_copy_paths(listed._ptr, 8, 2, None, None, 0, ctypes.byref(nodes)) == _lib.PO_ERR_INVALID and nodes.value == 0
    assert lib.po_last_error(ov._h).decode() == "po_paths_copy_paths: paths 8 .. 8 + 2 end past the 9 listed paths"
    assert lib.po_paths_copy_paths(listed._ptr, 10, 0, None, None, 0, ctypes.byref(nodes)) == _lib.PO_ERR_INVALID
    room = np.full(64, 0xEE, dtype=np.uint32)
    assert lib.po_paths_copy_paths(listed._ptr, 0, 9, None, room.ctypes.data, 5, ctypes.byref(nodes)) == _lib.PO_ERR_CAPACITY
    want = listed.paths_of(0)
    assert nodes.value == sum(len(p) for p in want) and (room == 0xEE).all()
    assert lib.po_last_error(ov._h).decode() == "po_paths_copy_paths: the paths hold %d nodes, there is room for 5" % nodes.value
    off = np.zeros(1, dtype=np.uint64) + 9
    assert lib.po_paths_copy_paths(listed._ptr, 9, 0, off.ctypes.data, None, 0, ctypes.byref(nodes)) == _lib.PO_OK and off[0] == 0 and nodes.value == 0
    with pytest.raises(ValueError, match="not listed"):
        counted.paths_of(0)
    with pytest.raises(ValueError, match="no listed path"):
        listed.path_of(0, 9)
    listed.close()
    counted.close()
    with pytest.raises(ValueError, match="closed"):
        listed.paths_of(0)
    other_rows.free()
    other.close()
    ov.close()
