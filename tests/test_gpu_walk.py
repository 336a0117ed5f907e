"""Whole walks of a bubble chain on the device: both routes of tests/walk_utils.py on a real ``ExactOverlapper`` -- one handle and
one index per walk -- held step by step to tests/golden/walk_cases.npz (the reference's own ``phase()``).  Every walk runs twice
on its handle with equal bytes for (cand, ext, rl) at every step; the two walks whose sizes go up (``grow_words``) and up, then
down to a handful of reads (``break_and_shrink``) run back to back on ONE handle, in both orders, and every step's bytes must be
those of the same walk on a fresh handle: scratch of a larger call that leaked into a smaller one would show here.
``phase_stats()`` and ``relevant_stats()`` are held to the trace's counts at every step."""
import pytest

import relevant_utils as ru
import walk_utils as wu
from phasm_amd.overlapper import ExactOverlapper

pytestmark = pytest.mark.gpu

WALKS = wu.load_golden()["walks"]
NAMES = [w["name"] for w in WALKS]
ARRAYS_OPTIONAL = ("kept_cand", "kept_ext", "kept_rl")


def indexed(ov, walk):
    res = ov.result_from_rows(ru.rows_array(wu.rows_of(walk)))
    index = ov.phase_index(res)
    res.free()
    return index


def handle_for(walk):
    ov = ExactOverlapper()
    ru.add_reads(ov, walk["lengths"])
    return ov


def check_stats(walk, steps):
    for got, want in zip(steps, walk["trace"]):
        rel, ph = wu.expected_stats(walk, want)
        st = got["relevant_stats"]
        assert {k: int(st[k]) for k in rel} == rel, (walk["name"], want["bubble"])
        if ph is not None:
            st = got["phase_stats"]
            assert {k: int(st[k]) for k in ph} == ph, (walk["name"], want["bubble"])


@pytest.mark.parametrize("name", NAMES)
def test_both_routes_on_the_device_equal_the_walk(name):
    walk = next(w for w in WALKS if w["name"] == name)
    ov = handle_for(walk)
    index = indexed(ov, walk)
    first, second, kept, kept_again = [], [], [], []
    got = wu.run_arrays(walk, ov, ov, index, raw=first)
    wu.same_trace(got, walk, walk, optional=ARRAYS_OPTIONAL)
    check_stats(walk, got[0])
    wu.same_trace(wu.run_integration(walk, ov, ov, index, raw=kept), walk, walk, optional=("best",))
    # a second time on the same handle and index: the same bytes at every step
    wu.run_arrays(walk, ov, ov, index, raw=second)
    wu.run_integration(walk, ov, ov, index, raw=kept_again)
    assert first and first == second and kept and kept == kept_again
    index.free()
    ov.close()


@pytest.mark.parametrize("order", [("grow_words", "break_and_shrink"), ("break_and_shrink", "grow_words")], ids="_then_".join)
def test_two_walks_back_to_back_on_one_handle(order):
    """Sizes up, down and up again on one handle: every step of every walk byte-equal to the walk on a fresh handle."""
    walks = [next(w for w in WALKS if w["name"] == n) for n in order]
    fresh = []
    for walk in walks:
        ov = handle_for(walk)
        index = indexed(ov, walk)
        raw = []
        wu.same_trace(wu.run_arrays(walk, ov, ov, index, raw=raw), walk, walk, optional=ARRAYS_OPTIONAL)
        wu.run_integration(walk, ov, ov, index, raw=raw)
        fresh.append(raw)
        index.free()
        ov.close()
    # one handle holds the reads of both walks, the second walk's behind the first's (its ids shifted: the ranks, and with
    # them the local ids of every bubble, stay); one scratch arena then serves the calls of both walks
    ovs = ExactOverlapper()
    ru.add_reads(ovs, walks[0]["lengths"] + walks[1]["lengths"])
    shifts = [0, 2 * len(walks[0]["lengths"])]
    for walk, shift, want in zip(walks, shifts, fresh):
        moved = shifted(walk, shift)
        index = indexed(ovs, moved)
        raw = []
        got = wu.run_arrays(moved, ovs, ovs, index, raw=raw)
        assert [s["arm"] for s in got[0]] == [s["arm"] for s in walk["trace"]]
        wu.run_integration(moved, ovs, ovs, index, raw=raw)
        assert raw == want, "%s after %s on one handle: the bytes of a step differ from those on a fresh handle" % (walk["name"], order[0])
        index.free()
    ovs.close()


def shifted(walk, shift):
    """The walk with every oriented read id moved up by ``shift`` (merged node ids move with the reads)."""
    if shift == 0:
        return walk
    n = wu.n_ids_of(walk)
    total = shift + n
    move = lambda x: x + shift if x < n else total + (x - n)   # noqa: E731
    out = dict(walk)
    out["n_seg"] = total // 2
    out["lengths"] = [1] * (shift // 2) + list(walk["lengths"])
    rows = wu.rows_of(walk).copy()
    rows[:, :2] += shift
    out["rows_flat"] = rows.reshape(-1).tolist()
    out["merged"] = [dict(m, reads=[move(r) for r in m["reads"]]) for m in walk["merged"]]
    out["bubbles"] = [dict(b, entrance=move(b["entrance"]), exit=move(b["exit"]), paths=[[move(x) for x in p] for p in b["paths"]],
                           interior_nodes=[move(x) for x in b["interior_nodes"]], interior_reads=[move(x) for x in b["interior_reads"]],
                           preds=[[move(p), e] for p, e in b["preds"]]) for b in walk["bubbles"]]
    return out
