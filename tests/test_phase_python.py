"""The Python layer of po_phase_branch without a GPU: ``pack_bubble`` round trips, the functions of ``phasm_amd.phasing`` on the
host scorer against the goldens, and ``device_phaser`` (integration/phasm/phasing_device.py) on the host scorer against
stand-in objects shaped like the reference's."""
import math
import os
import sys
from collections import deque, namedtuple
from itertools import combinations_with_replacement, product

import numpy as np
import pytest

import phase_utils as pu
from phasm_amd import phasing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "integration", "phasm"))
from phasing_device import device_phaser  # noqa: E402

CASES = pu.load_golden()["cases"]
Info = namedtuple("Info", "alignments overlap_max")


class Aln:
    """An alignment object as the reference's: ``.arange`` and ``.get_oriented_reads()``."""

    def __init__(self, a, b, arange):
        self.a, self.b, self.arange = a, b, arange

    def get_oriented_reads(self):
        return self.a, self.b


class Merged:
    def __init__(self, name, reads):
        self.name, self.reads = name, reads

    def __hash__(self):
        return hash(self.name)

    def __eq__(self, other):
        return isinstance(other, Merged) and other.name == self.name


def objects_of(case, as_objects):
    """Stand-ins for a case: reads are strings, local id b is "b<b>"; every path and every non-empty read set also holds a read
    that no alignment names."""
    aln, paths, sets = pu._lists(case)
    rel = {}
    for r in range(case["R"]):
        a = "r%d" % r
        las = [Aln(a, "b%d" % b, (a0, a1)) if as_objects else ("b%d" % b, a0, a1) for b, a0, a1 in aln[r]]
        rel[a] = Info(las, case["overlap_max"][r])
    node_paths = []
    for p, ids in enumerate(paths):
        ids = sorted(ids)
        nodes = ["b%d" % i for i in ids]
        if len(nodes) >= 2:
            nodes = [Merged("m%d" % p, nodes[:2])] + nodes[2:]
        node_paths.append(("entrance", *nodes, "via%d" % p, "exit"))
    read_sets = [[{"b%d" % x for x in s} | ({"stray"} if s else set()) for s in c] for c in sets]
    return node_paths, read_sets, rel


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["R"] <= 300])
def test_pack_bubble_round_trips(name):
    case = next(c for c in CASES if c["name"] == name)
    for as_objects in (False, True):
        node_paths, read_sets, rel = objects_of(case, as_objects)
        b = phasing.pack_bubble(node_paths, read_sets, rel)
        assert (b.ploidy, b.n_paths, b.n_cands, b.n_reads) == (case["k"], case["P"], case["C"], case["R"])
        assert b.n_b == len(b.b_reads) == len(set(case["aln_b"])) and "stray" not in b.b_reads
        assert not any(r.startswith("via") for r in b.b_reads)
        back = lambda ids: {int(b.b_reads[i][1:]) for i in ids}   # noqa: E731
        aln, paths, sets = pu._lists(case)
        named = set(case["aln_b"])
        for p in range(b.n_paths):
            assert back(b.path_reads(p)) == paths[p] & named
        for c in range(b.n_cands):
            for i in range(b.ploidy):
                assert back(b.set_reads(c, i)) == sets[c][i] & named
        assert b.overlap_max.tolist() == case["overlap_max"] and b.aln_off.tolist() == case["aln_off"]
        assert [int(b.b_reads[i][1:]) for i in b.aln_b] == case["aln_b"]
        assert b.aln_a0.tolist() == case["aln_a0"] and b.aln_a1.tolist() == case["aln_a1"]
        # another numbering of the reads, the same result
        again = dict(case, n_b=b.n_b)
        for key in pu.INPUT_KEYS:
            again[key] = getattr(b, key).tolist()
        pu.check_result(pu.scheme(again), case["ref"], case)


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_the_phasing_functions_on_the_host_scorer_equal_the_golden(name):
    case = next(c for c in CASES if c["name"] == name)
    hs, b, ref = phasing.HostScorer(), pu.bubble_of(case), case["ref"]
    cand, ext, rl = phasing.branch(hs, b, case["start"], case["threshold"], case["min_span"])
    assert cand.dtype == ext.dtype == np.uint32 and rl.dtype == np.float64
    assert cand.tolist() == ref["kept_cand"] and ext.tolist() == ref["kept_ext"]
    st = hs.phase_stats()
    n_tuples = math.comb(case["P"] + case["k"] - 1, case["k"]) if case["start"] else case["P"] ** case["k"]
    assert st["n_extensions"] == case["C"] * n_tuples and st["n_kept"] == st["n_survivors"] == len(rl) and st["level_used"] == -1
    for c, e in zip(cand.tolist(), ext.tolist()):
        digits = phasing.ext_digits(e, case["P"], case["k"])
        assert pu.ext_id(digits, case["P"]) == e and (not case["start"] or list(digits) == sorted(digits))
    pr = case["prune"]
    if pr is not None and not pu.level_zero(case):
        sc, se, sr = phasing.branch_and_prune(hs, b, case["start"], case["threshold"], case["min_span"], pr["factor"], pr["step"],
                                              pr["max_candidates"], pr["max_rounds"])
        assert sc.tolist() == [ref["kept_cand"][j] for j in ref["surv"]] and se.tolist() == [ref["kept_ext"][j] for j in ref["surv"]]
        st = hs.phase_stats()
        assert st["n_survivors"] == len(ref["surv"]) and st["n_kept"] == len(ref["kept_rl"])
        assert st["level_used"] == len(ref["levels"]) - 1
        if ref["levels"]:
            assert st["level_counts"][st["level_used"]] == len(ref["surv"])
    if case["R"]:
        scores = phasing.score_paths(hs, b)
        assert phasing.best_paths(scores, 1)[0] == ref["winner"] and len(phasing.best_paths(scores, case["k"])) == min(case["k"], case["P"])
    else:
        with pytest.raises(ZeroDivisionError):
            phasing.score_paths(hs, b)
    few = hs.phase_branch(b, case["start"], case["min_span"], case["threshold"], cap=1)
    assert len(few[0]) == min(1, len(ref["kept_rl"])) and hs.phase_stats()["n_kept"] == len(ref["kept_rl"])


def test_enumeration_orders_are_those_of_itertools():
    for P, k in ((3, 2), (2, 3), (4, 1), (3, 4)):
        b = phasing.bubble_from_arrays(k, [10], [[(0, 0, 5)]], [[0]] + [[] for _ in range(P - 1)], [[[] for _ in range(k)]])
        hs = phasing.HostScorer()
        for start, it in ((False, product(range(P), repeat=k)), (True, combinations_with_replacement(range(P), k))):
            _, ext, _ = hs.phase_branch(b, start)
            assert [phasing.ext_digits(e, P, k) for e in ext.tolist()] == list(it)


# ---- device_phaser on stand-ins shaped like the reference's classes ---------------------------------------------------

class StandInSet:
    """HaplotypeSet (phasm/phasing.py:58-108) as far as branch and prune use it."""

    def __init__(self, ploidy, copy_from=None):
        self.ploidy = ploidy
        self.haplotypes = [deque(copy_from.haplotypes[i]) if copy_from else deque() for i in range(ploidy)]
        self.read_sets = [set(copy_from.read_sets[i]) if copy_from else set() for i in range(ploidy)]
        self.log_rl = -math.inf

    def extend(self, extensions, ext_read_sets):
        new = StandInSet(self.ploidy, copy_from=self)
        for i, (extension, reads) in enumerate(zip(extensions, ext_read_sets)):
            nodes = new.haplotypes[i]
            nodes.extend(extension[1:] if nodes and nodes[-1] == extension[0] else extension)
            new.read_sets[i].update(reads)
        return new


class StandInPhaser:
    """BubbleChainPhaser as far as the subclass touches it; its own ``branch`` is the reference's loop, restated."""
    calls = 0

    def get_all_reads(self, nodes):
        for node in nodes:
            yield from (node.reads if isinstance(node, Merged) else (node,))

    def branch(self, possible_paths, relevant_reads):
        StandInPhaser.calls += 1
        return "inherited"


class Log:
    outfile = None


def test_device_phaser_rebuilds_the_kept_sets_in_the_reference_order():
    for case in CASES:
        if case["R"] > 300:
            continue
        node_paths, read_sets, rel = objects_of(case, True)
        ph = device_phaser(StandInPhaser, phasing.HostScorer())()
        ph.ploidy, ph.start_of_block, ph.min_spanning_reads = case["k"], bool(case["start"]), case["min_span"]
        ph.threshold = (lambda n, t=case["threshold"]: t) if case["C"] % 2 else case["threshold"]     # (a callable, as the reference allows)
        ph.debug_data_log = Log()
        ph.candidate_sets = []
        for c, sets in enumerate(read_sets):
            hs = StandInSet(case["k"])
            for i in range(case["k"]):
                hs.haplotypes[i].append("cand%d" % c)
                hs.read_sets[i] |= sets[i]
            ph.candidate_sets.append(hs)
        kept = ph.branch(node_paths, rel)
        ref = case["ref"]
        assert [int(hs.haplotypes[0][0][4:]) for hs in kept] == ref["kept_cand"]
        index = {p: j for j, p in enumerate(node_paths)}
        assert [pu.ext_id([index[tuple(list(h)[1:])] for h in hs.haplotypes], case["P"]) for hs in kept] == ref["kept_ext"]
        assert all(pu.same_rl(hs.log_rl, w, case["k"], case["R"]) for hs, w in zip(kept, ref["kept_rl"]))
        for hs, c, e in zip(kept, ref["kept_cand"], ref["kept_ext"]):
            digits = phasing.ext_digits(e, case["P"], case["k"])
            for i, d in enumerate(digits):
                assert hs.read_sets[i] == read_sets[c][i] | set(ph.get_all_reads(node_paths[d][1:-1]))
    assert StandInPhaser.calls == 0


def test_device_phaser_leaves_a_debug_run_to_the_inherited_branch():
    ph = device_phaser(StandInPhaser, phasing.HostScorer())()
    ph.debug_data_log = Log()
    ph.debug_data_log.outfile = object()
    before = StandInPhaser.calls
    assert ph.branch([("s", "x", "t")], {}) == "inherited" and StandInPhaser.calls == before + 1
    assert type(ph).__name__ == "DeviceStandInPhaser"
