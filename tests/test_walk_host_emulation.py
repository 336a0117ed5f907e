"""The kernels of the resident walk compiled for the HOST (tools/walk_host_emu.cpp: one lane per wave, threads one after
another) under AddressSanitizer + UBSan, launched as run_walk_step, run_walk_best and run_walk_history of c_api.hip launch them,
checked without a GPU.  They are fed the survivors and the path sets of every golden walk, over block-stable read ids; the rows
after every advance, the trace-back of every candidate and the tie set must equal ``HostWalk``.  The program is a stand-alone
executable run as a subprocess; every loop is bounded."""
import subprocess

import pytest

import emu_utils
import walk_product_utils as wp
import walk_utils as wu
from phasm_amd import phasing

WALKS = wu.load_golden()["walks"]
emu = emu_utils.emu_fixture("walk")


def events_and_snapshots(walk):
    """The walk through ``phase_chain`` on a ``HostWalk``: the text of the emulator's events, and after every event what the
    HostWalk holds (candidates, read sets over block-stable ids as bit rows, histories, the tie set)."""
    p = walk["params"]
    k = p["ploidy"]
    src, sc = phasing.HostIndex(wu.lengths_of(walk)), phasing.HostScorer()
    hw = phasing.HostWalk(sc, k)
    bubbles = wp.recorded_bubbles(walk)
    expand = wp.reads_of_node(walk)
    stable, text, snaps = {}, [str(k)], []

    def snapshot():
        n = hw.info()["n_cands"]
        depth = hw.info()["depth"]
        W = max(1, (len(stable) + 31) // 32) if depth else 0
        rows = []
        for sets in hw.read_sets(range(n)) if depth else []:
            for s in sets:
                words = [0] * W
                for r in s:
                    words[stable[r] >> 5] |= 1 << (stable[r] & 31)
                rows.append(words)
        snaps.append((n, W, depth, rows, hw.history(range(n)).tolist() if depth else [], hw.best()[0]))

    def on_step(s):
        if s.get("final"):
            return
        if s["broke"]:
            stable.clear()
            text.append("R")
            snaps.append((1, 0, 0, [], [], [0]))
        if s["arm"] == "advanced" and s["surv_cand"]:
            b = bubbles[s["bubble"]]
            for r in sorted(set(s["aln_y"]) | set(b["interior_reads"]) | set(stable)):     # (ascending, as b_reads is)
                stable.setdefault(r, len(stable))
            assert s["n_b"] == len(stable)
            paths = [[stable[r] for x in path[1:-1] for r in expand(x)] for path in b["paths"]]
            text.append("A %d %d %d" % (len(paths), len(stable), len(s["surv_cand"])))
            text.extend("%d %s" % (len(ids), " ".join(map(str, ids))) for ids in paths)
            text.extend("%d %d %s" % (c, e, float(x).hex()) for c, e, x in zip(s["surv_cand"], s["surv_ext"], s["surv_rl"]))
            snapshot()
        if s["arm"] == "retry":
            stable.clear()
            text.append("R")
            snapshot()

    list(phasing.phase_chain(sc, src, src.phase_index(wu.rows_of(walk)), bubbles, expand, k, p["min_spanning_reads"], p["max_bubble_size"],
                             wu.param(p["threshold"]), wu.param(p["prune_factor"]), p["max_candidates"], p["max_prune_rounds"],
                             p["prune_step_size"], walk=hw, choose=wp.first, on_step=on_step))
    return "\n".join(text) + "\n", snaps


@pytest.mark.parametrize("name", [w["name"] for w in WALKS])
def test_host_compiled_kernels_equal_the_host_walk(emu, name):
    walk = next(w for w in WALKS if w["name"] == name)
    text, snaps = events_and_snapshots(walk)
    assert snaps
    out = subprocess.run([emu], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    assert len(lines) == 4 * len(snaps) + 1, lines[:2]
    for j, (n, W, depth, rows, hist, tie) in enumerate(snaps):
        head, got_rows, got_hist, got_tie = lines[4 * j:4 * j + 4]
        assert [int(x) for x in head.split()] == [n, W, depth], (j, head)
        assert [[int(x, 16) for x in g.split()] for g in got_rows.split(";")[:-1]] == rows, j
        assert [[int(x) for x in g.split()] for g in got_hist.split(";")[:-1]] == hist, j
        assert [int(x) for x in got_tie.split()] == tie, j


def test_an_event_the_library_would_refuse_ends_the_program(emu):
    for text in ("9\n", "2\nA 2 4 1\n1 0\n1 1\n1 0 0x0p+0\n", "2\nA 2 4 1\n1 0\n1 9\n0 0 0x0p+0\n", "2\nX\n"):
        assert subprocess.run([emu], input=text, capture_output=True, text=True, timeout=120).returncode == 1
