"""The k_rs_ kernels of phasm_amd/csrc/resident.hip.h compiled for the HOST (tools/resident_host_emu.cpp, one lane per wave)
under AddressSanitizer + UBSan, launched as the library launches them: on the gathers and steps of every golden walk of
tests/golden/walk_cases.npz as ``phase_chain(resident=True)`` makes them on a ``HostWalk``, and on hand-made events -- new and
known reads interleaved in b_reads, a peek before an advance, a reset and a read of the old block coming back, blocks of 31 to 65
reads, the read ids at the word borders and the last one, a path read outside b_reads, duplicates in cur_graph.  After every event
the translation, stable_of, global_of and both previous sets are those of the rule ``po_walk_step`` applies on the host and of
``HostWalk``.  An event the library would refuse ends the program with status 1."""
import subprocess

import pytest

import emu_utils
import walk_product_utils as wp
import walk_utils as wu
from phasm_amd import phasing

emu = emu_utils.emu_fixture("resident")
WALKS = wu.load_golden()["walks"]
NONE = 0xFFFFFFFF


def text_of(n_ids, events):
    out = [str(n_ids)]
    for e in events:
        if e == "R":
            out.append("R")
            continue
        lists = [e["cur"], e["ca"], e["b"], e["aln_b"]]
        out.append("S %d " % e["advance"] + " ".join("%d %s" % (len(x), " ".join(map(str, x))) for x in lists) +
                   " %d " % len(e["paths"]) + " ".join("%d %s" % (len(p), " ".join(map(str, p))) for p in e["paths"]))
    return "\n".join(out) + "\n"


class Model:
    """The state the events must leave, by the rule of ``run_walk_step``: a read known to the block keeps its id, the reads of
    b_reads new to it get n_block + their rank among the new ones, in the order of b_reads."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.stable, self.order, self.prev_graph, self.prev_aligning = {}, [], set(), set()

    def event(self, e):
        fresh = [g for g in e["b"] if g not in self.stable]
        xl = {g: self.stable.get(g, len(self.order) + (fresh.index(g) if g in fresh else 0)) for g in e["b"]}
        out = {"n_new": len(fresh), "nb": len(self.order) + len(fresh), "xl": [xl[g] for g in e["b"]],
               "aln_b": [xl[e["b"][x]] for x in e["aln_b"]], "pids": [xl.get(g, NONE) for p in e["paths"] for g in p]}
        if e["advance"]:
            for g in fresh:
                self.stable[g] = len(self.order)
                self.order.append(g)
            self.prev_graph |= set(e["cur"])
            self.prev_aligning |= set(e["ca"])
        out.update(global_of=list(self.order), stable_of=sorted(self.stable.items()), prev_graph=sorted(self.prev_graph),
                   prev_aligning=sorted(self.prev_aligning))
        return out


def run(emu, n_ids, events):
    res = subprocess.run([emu], input=text_of(n_ids, events), capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    lines = res.stdout.split("\n")
    got, at = [], 0
    for e in events:
        if e == "R":
            assert lines[at] == "reset"
            got.append(None)
            at += 1
            continue
        ints = [[int(x) for x in lines[at + j].split()] for j in (0, 1, 2, 3, 4, 6, 7)]
        pairs = [tuple(int(v) for v in x.split(":")) for x in lines[at + 5].split()]
        got.append({"n_new": ints[0][0], "nb": ints[0][1], "xl": ints[1], "aln_b": ints[2], "pids": ints[3], "global_of": ints[4][1:],
                    "stable_of": pairs, "prev_graph": ints[5], "prev_aligning": ints[6], "n_block": ints[4][0]})
        at += 8
    assert lines[at:] == [""]
    return got


def check(emu, n_ids, events, host_states=None):
    model, got = Model(), run(emu, n_ids, events)
    n = 0
    for e, g in zip(events, got):
        if e == "R":
            model.reset()
            continue
        want = model.event(e)
        assert g.pop("n_block") == len(want["global_of"])
        assert g == want, (n, e)
        if host_states is not None:           # ... and HostWalk's own: the block reads and the two sets after this step
            block, sets = host_states[n]
            assert set(g["global_of"]) == block and (g["prev_graph"], g["prev_aligning"]) == sets
        n += 1
    return got


class Recording(phasing.HostWalk):
    """A ``HostWalk`` that notes every step of the resident route as an event of the emulator, and what it holds afterwards."""

    def __init__(self, scorer, ploidy, events, states):
        self.events, self.states = events, states
        super().__init__(scorer, ploidy)

    def reset(self):
        super().reset()
        self.events.append("R")

    def step_resident(self, rel, path_reads, *args, **kw):
        out = super().step_resident(rel, path_reads, *args, **kw)
        r = rel.rel
        self.events.append({"advance": self._stats["advanced"], "cur": [int(x) for x in rel.cur_graph], "ca": r.cur_aligning.tolist(),
                            "b": r.b_reads.tolist(), "aln_b": r.aln_b.tolist(), "paths": [[int(x) for x in p] for p in path_reads]})
        self.states.append((set(self._block), self.prev_sets()))
        return out


def test_the_events_of_every_golden_walk(emu):
    n_steps = 0
    for walk in WALKS:
        src, sc = phasing.HostIndex(wu.lengths_of(walk)), phasing.HostScorer()
        p, events, states = walk["params"], [], []
        hw = Recording(sc, p["ploidy"], events, states)
        del events[:]                                                          # (the reset of the constructor)
        list(phasing.phase_chain(sc, src, src.phase_index(wu.rows_of(walk)), wp.recorded_bubbles(walk), wp.reads_of_node(walk), p["ploidy"],
                                 p["min_spanning_reads"], p["max_bubble_size"], wu.param(p["threshold"]), wu.param(p["prune_factor"]),
                                 p["max_candidates"], p["max_prune_rounds"], p["prune_step_size"], walk=hw, choose=wp.first, resident=True))
        assert any(e != "R" for e in events), walk["name"]
        check(emu, wu.n_ids_of(walk), events, states)
        n_steps += sum(e != "R" for e in events)
    assert n_steps >= 53 - sum(s["arm"] in ("large", "skipped") for w in WALKS for s in w["trace"])


def event(b, advance=1, cur=None, ca=None, aln_b=None, paths=None):
    b = sorted(b)
    return {"advance": advance, "cur": list(b if cur is None else cur), "ca": list(b if ca is None else ca), "b": b,
            "aln_b": list(range(len(b)))[::-1] if aln_b is None else aln_b, "paths": [b[::2], b[1::2]] if paths is None else paths}


def test_new_and_known_reads_interleaved_a_peek_and_a_reset(emu):
    n_ids = 200
    first = event([5, 9, 40, 41, 100])
    # new reads between, before and behind the known ones; the peek numbers them as the advancing call does
    mixed = [2, 5, 7, 9, 39, 40, 41, 42, 100, 150]
    peek = event(mixed, advance=0, cur=[2, 7, 39, 42, 150], ca=[2, 3, 7, 150, 199])
    took = dict(peek, advance=1)
    back = event([9, 41, 160], cur=[9, 41, 160])                              # after the reset: reads of the old block come back
    events = [first, peek, peek, took, "R", back, "R", "R", event([41], paths=[[41], [9]])]
    got = check(emu, n_ids, events)
    assert got[1]["xl"] == got[3]["xl"] == [5, 0, 6, 1, 7, 2, 3, 8, 4, 9] and got[1]["n_new"] == 5 and got[1]["global_of"] == [5, 9, 40, 41, 100]
    assert got[1]["prev_aligning"] == [5, 9, 40, 41, 100] and got[3]["prev_aligning"] == [2, 3, 5, 7, 9, 40, 41, 100, 150, 199]
    assert got[5]["xl"] == [0, 1, 2] and got[5]["stable_of"] == [(9, 0), (41, 1), (160, 2)] and got[5]["prev_graph"] == [9, 41, 160]
    assert got[8]["pids"] == [0, NONE] and got[8]["stable_of"] == [(41, 0)]


@pytest.mark.parametrize("size", [31, 32, 33, 63, 64, 65])
def test_blocks_at_the_word_borders(emu, size):
    n_ids = 131
    border = [0, 31, 32, 63, 64, n_ids - 1]
    rest = [x for x in range(1, n_ids - 1) if x not in border]
    block = sorted(border + rest[:size - len(border)])
    assert len(block) == size
    half = block[::2]
    events = [event(half), event(block, cur=block + block[:3]),                # (duplicates in cur_graph count once)
              event(border, advance=0, paths=[[0, 31, 1, 130], [32, 63, 64, 129, 2]]),      # (path reads outside b_reads are dropped)
              event(block + [rest[-1]], cur=[rest[-1]])]
    got = check(emu, n_ids, events)
    assert got[1]["nb"] == size and got[1]["n_new"] == size - len(half) and got[3]["nb"] == size + 1
    assert got[2]["n_new"] == 0 and got[2]["pids"].count(NONE) == sum(x not in border for x in [1, 130, 129, 2])
    assert got[1]["prev_graph"] == block and sorted(got[3]["global_of"]) == sorted(block + [rest[-1]])


@pytest.mark.parametrize("what", ["id", "order", "local", "paths", "outside", "advance", "event"])
def test_an_event_the_library_would_refuse_ends_with_status_1(emu, what):
    e = event([3, 8, 20])
    text = None
    if what == "id":
        e["paths"] = [[3], [50]]
    elif what == "order":
        e["b"] = [3, 20, 8]
    elif what == "local":
        e["aln_b"] = [0, 3]
    elif what == "paths":
        e["paths"] = [[3]] * 65
    elif what == "outside":
        e["cur"] = [3, 8]
    elif what == "advance":
        e["advance"] = 2
    else:
        text = "50\nX\n"
    res = subprocess.run([emu], input=text or text_of(50, [e]), capture_output=True, text=True, timeout=60)
    assert res.returncode == 1, (res.returncode, res.stderr[-2000:])
