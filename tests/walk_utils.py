"""Whole walks of a bubble chain through the phase device calls (po_phase_index, po_phase_relevant, po_phase_branch): the
inputs of the walks, a recorder of what a phaser does step by step, a stand-in phaser whose loop restates the reference's
``phase()``, the two routes that are held to the recorded trace, and the loader of tests/golden/walk_cases.npz.

The walk itself -- the loop of ``phase()``, ``new_block`` and the final ``prune(.., 1.0)`` (phasm/phasing.py:182-364) -- is no
part of the product.  It lives here, test-side, so that the suite can carry state from bubble to bubble:
read sets that grow, ``prev_graph_reads`` / ``prev_aligning_reads`` that accumulate and are reset, local read ids that change at
every bubble, sizes that go up and down on one handle.

A WALK is a dict: ``params`` (the arguments of ``BubbleChainPhaser.__init__``; a callable is ``["step", n0, below, from_n0]``),
``lengths`` per segment -- segment i has the oriented reads 2i and 2i + 1 --, the rows ``(a, b, astart, aend, bstart, bend)`` in
``rows_flat``, the graph as ``edges_flat`` (u, v, edge_len) over node ids, ``merged`` (node id 2 * n_seg + j: its reads, prefix
lengths and length), and -- recorded from the reference -- ``bubbles`` (entrance, exit, paths as node lists, interior reads, the
exit's predecessors with their edge lengths), ``trace`` (one dict per turn of the loop), ``final`` and ``state``.

A STEP of a trace: ``bubble``, ``start`` (start_of_block on entry), ``state_in`` (digest of candidates, prev sets and flag on
entry), ``arm`` ("advanced", "retry", "skipped", "large"), ``broke`` (new_block ran before the relevant reads were collected),
``fell_back`` (... because too few reads span), ``cur_aligning``, ``n_spanning``, the relevant reads as in tests/relevant_utils.py
(``rel_reads overlap_max aln_off aln_y aln_a0 aln_a1``), ``n_b``, ``n_cands_in``, the kept list ``kept_cand kept_ext kept_rl``,
``prune_factor`` (the number ``prune`` used; None where the list had fewer than two entries), the survivors ``surv_cand surv_ext
surv_rl``, ``yields`` (kind, include_last, the tie set as places in the list that was pruned, the haplotypes as node lists) and at
a large bubble ``winner`` (the reference's first path), ``best`` and ``scores`` (by ``large_scores``)."""
import contextlib
import math
import os
import random
import sys
from collections import deque, namedtuple

import numpy as np

import components_utils as cu
import phase_utils as pu
import reduce_utils as ru
import relevant_utils as rel_u
from phasm_amd import phasing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_FILE = os.path.join(ru.GOLDEN, "walk_cases.npz")
NODE_LEN = 3000
REL_KEYS = ("rel_reads", "overlap_max", "aln_off", "aln_y", "aln_a0", "aln_a1")
EXACT_KEYS = ("bubble", "start", "state_in", "arm", "broke", "fell_back", "cur_aligning", "n_spanning") + REL_KEYS + (
    "n_b", "n_cands_in", "n_kept", "kept_cand", "kept_ext", "prune_factor", "surv_cand", "surv_ext", "winner", "best")


def device_phaser_factory():
    sys.path.insert(0, os.path.join(ROOT, "integration", "phasm"))
    try:
        import phasing_device
    finally:
        sys.path.pop(0)
    return phasing_device.device_phaser


# ---- parameters ----------------------------------------------------------------------------------------------------------------

def param(spec):
    """A number, or the callable of the count that ``["step", n0, below, from_n0]`` stands for."""
    if isinstance(spec, (list, tuple)):
        kind, n0, below, above = spec
        assert kind == "step"
        return lambda n: below if n < n0 else above
    return spec


def resolve(spec, n):
    f = param(spec)
    return f(n) if callable(f) else f


def phaser_arguments(params):
    """The keyword arguments of ``BubbleChainPhaser.__init__`` behind the graph."""
    p = dict(params)
    p["threshold"], p["prune_factor"] = param(p["threshold"]), param(p["prune_factor"])
    return p


def prune_spec(params, factor):
    return {"factor": factor, "step": params["prune_step_size"], "max_candidates": params["max_candidates"],
            "max_rounds": params["max_prune_rounds"]}


# ---- the inputs of a walk, from a seed -----------------------------------------------------------------------------------------

def _params(ploidy=2, min_spanning_reads=3, max_bubble_size=4, threshold=1e-3, prune_factor=0.1, max_candidates=500, max_prune_rounds=9,
            prune_step_size=0.1):
    return dict(ploidy=ploidy, min_spanning_reads=min_spanning_reads, max_bubble_size=max_bubble_size, threshold=threshold,
                prune_factor=prune_factor, max_candidates=max_candidates, max_prune_rounds=max_prune_rounds, prune_step_size=prune_step_size)


def synth(seed, params, paths, depth=2, span=6, window=3, noise=0.1, cuts=(), weak=(), isolated=(), bare=(), link=True,
          merged_interior=(), merged_pred=(), twins=(), extra_graph=0):
    """A chain of len(paths) bubbles, bubble b with paths[b] paths of ``depth`` (a number or one per bubble) interior reads,
    ``k`` true haplotypes that each follow one path per bubble, and per bubble ``span`` reads outside the graph that follow one
    haplotype over up to ``window`` bubbles and align to its interior reads (with probability ``noise`` to another path's).

    ``cuts``: bubbles no read crosses into.  ``weak``: cuts that three reads cross with alignments of a dozen bases.  ``isolated``:
    bubbles whose interior aligns to reads of their own alone; the other reads pass over them.  ``bare``: bubbles whose interior
    reads have no row at all.  ``link``: rows between an entrance or exit and the interior reads beside it.  ``merged_interior``
    / ``merged_pred``: (bubble, path) whose interior reads but the last / whose interior reads all sit in one merged node.
    ``twins``: bubbles whose paths 0 and 1 are two merged nodes over the same reads.  ``extra_graph``: interior reads added to
    every path of every bubble beyond ``depth`` that no read outside the graph aligns to."""
    rng = np.random.default_rng(seed)
    k, N = params["ploidy"], len(paths)
    depths = [depth] * N if isinstance(depth, int) else list(depth)
    spans = [span] * N if isinstance(span, int) else list(span)
    lengths, rows, edges, merged = [], [], [], []

    def segment(length):
        lengths.append(int(length))
        i = len(lengths) - 1
        return 2 * i + (i % 3 == 1)                       # one orientation per segment, a third of them the reverse one

    def row(a, b, a0, a1, b0, b1):
        rows.append((a, b, a0, a1, b0, b1) if rng.random() < 0.67 else (b, a, b0, b1, a0, a1))

    ends = [segment(NODE_LEN) for _ in range(N + 1)]
    # (later bubbles get the lower ids: a read's rank among the b reads, its local id, then changes at every bubble)
    reads_of = [[[segment(NODE_LEN) for _ in range(depths[b] + extra_graph)] for _ in range(paths[b])] for b in reversed(range(N))][::-1]
    for b in twins:
        reads_of[b][1] = list(reads_of[b][0])
    edge_len = [[2500 + int(rng.integers(0, 300)) for _ in range(paths[b])] for b in range(N)]
    n_real = len(lengths)                                  # (the reads outside the graph come behind)
    pending = []                                           # merged nodes get their ids when the segments are all known

    def node_list(b, p):
        rs = reads_of[b][p]
        if b in twins and p < 2 or (b, p) in merged_pred:
            pending.append((rs, b, p))
            return [("m", len(pending) - 1)]
        if (b, p) in merged_interior and len(rs) >= 2:
            pending.append((rs[:-1], b, p))
            return [("m", len(pending) - 1), rs[-1]]
        return list(rs)

    node_paths = [[node_list(b, p) for p in range(paths[b])] for b in range(N)]
    first = [int(rng.integers(0, paths[b])) for b in range(N)]
    hap = [[(first[b] + h) % paths[b] for b in range(N)] for h in range(k)]
    blocked = set(cuts) | set(weak)

    def align(s, t, b, p, short=False):
        rs = reads_of[b][p][:depths[b]]
        d = len(rs)
        step = 500 // d
        for j, g in enumerate(rs):
            last = j == len(reads_of[b][p]) - 1
            if short and j != int(rng.integers(0, d)) and d > 1:
                continue
            if not short and not last and rng.random() > 0.85:
                continue
            a0 = t * 600 + 40 + j * step + int(rng.integers(0, 10))
            a1 = a0 + (12 if short else step + int(rng.integers(5, 40)))
            b0 = edge_len[b][p] - ((t + 1) * 600 + int(rng.integers(0, 60))) if last else int(rng.integers(0, 100))
            row(s, g, a0, a1, b0, b0 + a1 - a0)

    for b in range(N):
        if b in bare:
            continue
        for p in range(paths[b]):
            if b in twins and p == 1:
                continue
            rs = reads_of[b][p]
            for x, y in zip(rs, rs[1:]):
                row(x, y, 2000, NODE_LEN, 0, 1000)
            if link and b not in isolated:
                row(ends[b], rs[0], 2000, NODE_LEN, 0, 1000)
                row(rs[-1], ends[b + 1], 2000, NODE_LEN, 0, 1000)
    for b0 in range(N):
        if b0 in bare:
            continue
        for i in range(spans[b0]):
            h = i % k
            w = 1 if b0 in isolated else 1 + int(rng.integers(0, window))
            covered = [b0]
            for b in range(b0 + 1, N):
                if len(covered) == w or b in blocked:
                    break
                if b not in isolated and b not in bare:
                    covered.append(b)
            s = segment(600 * len(covered) + 200)
            for t, b in enumerate(covered):
                p = hap[h][b]
                if rng.random() < noise and paths[b] > 1:
                    p = (p + 1 + int(rng.integers(0, paths[b] - 1))) % paths[b]
                align(s, t, b, p)
    for b in weak:
        for i in range(3):
            s = segment(1400)
            align(s, 0, b - 1, int(rng.integers(0, paths[b - 1])), short=True)
            align(s, 1, b, int(rng.integers(0, paths[b])), short=True)
    n_ids = 2 * len(lengths)
    name = lambda x: n_ids + x[1] if isinstance(x, tuple) else x   # noqa: E731
    for j, (rs, b, p) in enumerate(pending):
        merged.append({"reads": list(rs), "prefix_lengths": [700 + 10 * j] * (len(rs) - 1), "length": NODE_LEN + 700 * (len(rs) - 1)})
    for b in range(N):
        for p in range(paths[b]):
            nodes = [ends[b]] + [name(x) for x in node_paths[b][p]] + [ends[b + 1]]
            for u, v in zip(nodes, nodes[1:]):
                edges.append((u, v, edge_len[b][p] if v == ends[b + 1] else 1500 + int(rng.integers(0, 300))))
    return {"params": params, "seed": int(seed), "n_seg": len(lengths), "lengths": lengths, "rows_flat": [int(v) for r in rows for v in r],
            "edges_flat": [int(v) for e in edges for v in e], "merged": merged, "n_graph_segments": n_real}


# name -> (arguments of synth, the arms and situations the walk must show); see ``situations``
SPECS = {
    "straight": (dict(params=_params(), paths=[2] * 5, depth=2, span=6, window=3),
                 ("advanced", "clipped_by_two_preds", "spans_three_bubbles")),
    "grow_words": (dict(params=_params(threshold=1e-4, prune_factor=0.02, max_candidates=90), paths=[2] * 5, depth=6, extra_graph=1,
                        span=[54, 16, 16, 16, 16], window=3, noise=0.15),
                   ("advanced", "nb_below_32", "nb_past_32", "nb_past_64", "relevant_past_64", "cands_past_64", "cut_by_max_candidates")),
    "break_and_shrink": (dict(params=_params(threshold=1e-4, prune_factor=0.02, max_candidates=90), paths=[2] * 8, depth=[6] * 5 + [1] * 3,
                              extra_graph=1, span=[16] * 5 + [8] * 3, window=3, noise=0.15, cuts=(5,), link=False),
                         ("advanced", "fell_back", "nb_past_64", "nb_below_8_after_a_break", "two_small_bubbles_follow")),
    "retry": (dict(params=_params(threshold=["step", 8, 0.5, 1e-3]), paths=[2] * 4, depth=2, span=6, window=3),
              ("advanced", "retry")),
    "skipped": (dict(params=_params(min_spanning_reads=0), paths=[2] * 5, depth=2, span=8, window=3, bare=(0,), isolated=(3,)),
                ("advanced", "skipped_at_a_start_with_relevant_reads", "skipped_in_the_middle_state_kept")),
    "large_first": (dict(params=_params(max_bubble_size=3), paths=[4, 2, 2], depth=1, span=8, window=2),
                    ("advanced", "large_at_the_start")),
    "large_middle": (dict(params=_params(max_bubble_size=3), paths=[2, 2, 4, 2], depth=1, span=8, window=2),
                     ("advanced", "large_behind_phased_bubbles")),
    "ploidy3_rounds": (dict(params=_params(ploidy=3, threshold=1e-4, prune_factor=0.05, max_candidates=6, max_prune_rounds=12),
                            paths=[3, 4, 3, 2], depth=1, span=12, window=3, noise=0.2),
                       ("advanced", "retry", "several_prune_rounds_at_two_bubbles", "four_paths")),
    "callables": (dict(params=_params(threshold=["step", 12, 1e-3, 1e-2], prune_factor=["step", 5, 0.05, 0.3]), paths=[2] * 4, depth=2,
                       span=6, window=3),
                  ("advanced", "both_sides_of_the_threshold_step", "both_sides_of_the_factor_step")),
    "merged_nodes": (dict(params=_params(), paths=[2] * 3, depth=3, span=8, window=3, merged_interior=((0, 0), (1, 1)), merged_pred=((1, 0), (2, 1))),
                     ("advanced", "merged_interior", "merged_pred")),
    "twins": (dict(params=_params(), paths=[3, 2, 2, 2], depth=2, span=8, window=2, twins=(0, 3), cuts=(2,)),
              ("advanced", "fell_back", "tie_at_a_new_block", "tie_at_the_end")),
}


def inputs(name, seed):
    w = synth(seed, **SPECS[name][0])
    w["name"] = name
    return w


INPUT_KEYS = ("params", "seed", "n_seg", "lengths", "rows_flat", "edges_flat", "merged", "n_graph_segments", "name")


# ---- a walk's pieces -------------------------------------------------------------------------------------------------------------

def n_ids_of(walk):
    return 2 * walk["n_seg"]


def rows_of(walk):
    return np.asarray(walk["rows_flat"], dtype=np.int64).reshape(-1, 6)


def edges_of(walk):
    return np.asarray(walk["edges_flat"], dtype=np.int64).reshape(-1, 3).tolist()


def lengths_of(walk):
    return np.repeat(np.asarray(walk["lengths"], dtype=np.int64), 2)


def node_reads(walk, nodes):
    """``get_all_reads``: the reads of a list of node ids."""
    n = n_ids_of(walk)
    out = []
    for x in nodes:
        out += walk["merged"][x - n]["reads"] if x >= n else [x]
    return out


def plain_preds(walk, bubble):
    n = n_ids_of(walk)
    return [(int(p), int(e)) for p, e in bubble["preds"] if p < n]


def digest_state(start, prev_graph, prev_aligning, cands):
    """``cands``: (haplotypes as node id lists, read sets as id collections) per candidate."""
    flat = [int(bool(start)), -3] + sorted(prev_graph) + [-3] + sorted(prev_aligning) + [-3]
    for hist, sets in cands:
        for h, s in zip(hist, sets):
            flat += list(h) + [-1] + sorted(s) + [-2]
    return cu.digest(flat)[:16]


def extended(hist, sets, ext_paths, ext_reads):
    """``HaplotypeSet.extend`` (phasm/phasing.py:85-108) on ids."""
    new_h, new_s = [], []
    for h, s, path, reads in zip(hist, sets, ext_paths, ext_reads):
        h, path = list(h), list(path)
        new_h.append(h + (path[1:] if h and h[-1] == path[0] else path))
        new_s.append(set(s) | set(reads))
    return new_h, new_s


def _overlap(las, om, reads):
    return pu._overlap(las, om, reads)


def large_scores(walk, step):
    """The score of every path of a large bubble, by the loops of ``phase_large_bubble`` (phasing.py:641-672)."""
    b = walk["bubbles"][step["bubble"]]
    R = len(step["rel_reads"])
    scores = []
    for path in b["paths"]:
        reads = set(node_reads(walk, path[1:-1]))
        s = 0.0
        for r in range(R):
            lo, hi = step["aln_off"][r], step["aln_off"][r + 1]
            f = _overlap(list(zip(step["aln_y"][lo:hi], step["aln_a0"][lo:hi], step["aln_a1"][lo:hi])), step["overlap_max"][r], reads)
            if f is not None:
                s += f
        scores.append(s / R)
    return scores


# ---- the recorder: what a phaser does, step by step -----------------------------------------------------------------------------

class Recorder:
    """Wraps the methods of one phaser object (the reference's ``BubbleChainPhaser`` or a stand-in) and notes what goes in and
    comes out.  ``ident(node)``: the node id of a read or merged node.  ``set_class``: the class of the haplotype sets, whose
    ``extend`` is wrapped while recording so that every new set knows its parent and its extension."""

    def __init__(self, ph, walk, bubbles, ident, set_class):
        self.ph, self.walk, self.bubbles, self.ident, self.set_class = ph, walk, bubbles, ident, set_class
        self.by_interior = {frozenset(b["interior_nodes"]): i for i, b in enumerate(bubbles)}
        self.steps, self.final, self.cur = [], None, None
        self.pruned, self.tie, self.branched = None, None, None
        for name in ("get_aligning_reads", "get_relevant_read_info", "branch", "prune", "new_block", "phase_large_bubble"):
            setattr(ph, name, getattr(self, "_" + name)(getattr(ph, name)))

    # -- plumbing
    def ids(self, nodes):
        return [self.ident(n) for n in nodes]

    def cands(self, sets):
        return [([self.ids(h) for h in hs.haplotypes], [self.ids(s) for s in hs.read_sets]) for hs in sets]

    def state(self):
        ph = self.ph
        return digest_state(ph.start_of_block, self.ids(ph.prev_graph_reads), self.ids(ph.prev_aligning_reads), self.cands(ph.candidate_sets))

    @contextlib.contextmanager
    def recording(self):
        cls, rec = self.set_class, self
        orig_extend, orig_choice = cls.extend, random.choice

        def extend(hs, extensions, ext_read_sets):
            new = orig_extend(hs, extensions, ext_read_sets)
            new._parent, new._ext = hs, tuple(extensions)
            return new

        def choice(seq):
            seq = list(seq)
            place = {id(hs): j for j, hs in enumerate(rec.pruned)}
            rec.tie = [place[id(hs)] for hs in seq]
            return seq[0]

        cls.extend, random.choice = extend, choice
        try:
            yield self
        finally:
            cls.extend, random.choice = orig_extend, orig_choice

    def run(self, *phase_args):
        with self.recording():
            for hs, include_last in self.ph.phase(*phase_args):
                self.on_yield(hs, include_last)
        ph = self.ph
        state = {"start": int(ph.start_of_block), "prev_graph": sorted(self.ids(ph.prev_graph_reads)),
                 "prev_aligning": sorted(self.ids(ph.prev_aligning_reads)), "digest": self.state(), "n_cands": len(ph.candidate_sets),
                 "cands": [{"haplotypes": h, "read_sets": [sorted(s) for s in sets]} for h, sets in self.cands(ph.candidate_sets)]}
        for s in self.steps:
            s["fell_back"] = int(bool(s["broke"]) and s["arm"] != "large")
        return self.steps, self.final or {"yields": []}, state

    def on_yield(self, hs, include_last):
        y = {"include_last": int(bool(include_last)), "tie": self.tie, "haplotypes": [self.ids(h) for h in hs.haplotypes],
             "read_sets": [sorted(self.ids(s)) for s in hs.read_sets]}
        if include_last:
            y["kind"] = "final"
            self.final = {"yields": [y], "prune_in": len(self.pruned)}
        else:
            y["kind"] = "new_block" if self.tie is not None else "large"
            self.cur["yields"].append(y)
        self.tie = None

    # -- the wrappers
    def _get_aligning_reads(self, orig):
        def wrapper(nodes):
            nodes = list(nodes)
            ph = self.ph
            state = self.state()
            out = orig(nodes)
            self.cur = {"bubble": self.by_interior[frozenset(self.ids(nodes))], "start": int(ph.start_of_block), "state_in": state, "arm": "skipped",
                        "broke": 0, "yields": [], "cur_aligning": sorted(self.ids(out)), "n_spanning": len(set(ph.prev_aligning_reads) & set(out))}
            self.steps.append(self.cur)
            return out
        return wrapper

    def _get_relevant_read_info(self, orig):
        def wrapper(relevant_reads, cur_bubble_graph_reads, bubble_exit):
            out = orig(relevant_reads, cur_bubble_graph_reads, bubble_exit)
            assert set(out) == set(relevant_reads)
            by_id = {self.ident(r): v for r, v in out.items()}
            s = self.cur
            s.update({k: [] for k in REL_KEYS})
            s["aln_off"] = [0]
            for r in sorted(by_id):
                las, om = by_id[r][0], by_id[r][1]
                for y, a0, a1 in sorted((self.ident(la.get_oriented_reads()[1]), int(la.arange[0]), int(la.arange[1])) for la in las):
                    s["aln_y"].append(y)
                    s["aln_a0"].append(a0)
                    s["aln_a1"].append(a1)
                s["aln_off"].append(len(s["aln_y"]))
                s["rel_reads"].append(r)
                s["overlap_max"].append(int(om))
            s["n_b"] = len(set(self.ids(cur_bubble_graph_reads)) | set(self.ids(self.ph.prev_graph_reads)))
            return out
        return wrapper

    def _branch(self, orig):
        def wrapper(possible_paths, relevant_reads):
            ph, s = self.ph, self.cur
            entry = list(ph.candidate_sets)
            place = {id(hs): c for c, hs in enumerate(entry)}
            index = {tuple(self.ids(p)): j for j, p in enumerate(possible_paths)}
            assert [list(p) for p in index] == self.bubbles[s["bubble"]]["paths"]
            s["n_cands_in"] = len(entry)
            out = orig(possible_paths, relevant_reads)
            s["kept_cand"] = [place[id(hs._parent)] for hs in out]
            s["kept_ext"] = [pu.ext_id([index[tuple(self.ids(p))] for p in hs._ext], len(index)) for hs in out]
            s["kept_rl"] = [float(hs.log_rl) for hs in out]
            s["n_kept"] = len(out)
            s["arm"] = "advanced"
            self.branched = out
            return out
        return wrapper

    def _prune(self, orig):
        def wrapper(candidate_sets, prune_factor):
            given = list(candidate_sets)
            out = orig(candidate_sets, prune_factor)
            self.pruned = given
            if candidate_sets is self.branched:
                s = self.cur
                place = {id(hs): j for j, hs in enumerate(given)}
                at = [place[id(hs)] for hs in out]
                s["prune_factor"] = None if len(given) < 2 else float(prune_factor(len(given)) if callable(prune_factor) else prune_factor)
                s["surv_cand"], s["surv_ext"] = [s["kept_cand"][j] for j in at], [s["kept_ext"][j] for j in at]
                s["surv_rl"] = [s["kept_rl"][j] for j in at]
                self.branched = None
            return out
        return wrapper

    def _new_block(self, orig):
        def wrapper():
            s = self.cur
            if "rel_reads" not in s:
                s["broke"] = 1
            elif s["arm"] == "advanced":
                s["arm"] = "retry"
            return orig()
        return wrapper

    def _phase_large_bubble(self, orig):
        def wrapper(possible_paths, relevant_reads):
            out = orig(possible_paths, relevant_reads)
            s = self.cur
            index = {tuple(self.ids(p)): j for j, p in enumerate(possible_paths)}
            s["arm"] = "large"
            s["winner"] = index[tuple(self.ids(out.haplotypes[0]))]
            return out
        return wrapper


# ---- stand-ins shaped like the reference's classes --------------------------------------------------------------------------------

class StandInRead:
    """What the reference's OrientedRead is to the methods at hand: hashable, with a length."""

    def __init__(self, ident, length):
        self.ident, self.length = ident, length

    def __len__(self):
        return self.length

    def __hash__(self):
        return hash(self.ident)

    def __eq__(self, other):
        return isinstance(other, StandInRead) and self.ident == other.ident

    def __repr__(self):
        return "read%d" % self.ident


class StandInMerged(StandInRead):
    """MergedReads: ``reads`` and ``prefix_lengths``; never a key of the alignments."""

    def __init__(self, ident, length, reads, prefix_lengths):
        super().__init__(ident, length)
        self.reads, self.prefix_lengths = reads, prefix_lengths


class StandInGraph:
    """What ``get_relevant_read_info`` asks of the assembly graph, for every exit of the chain."""
    edge_len = "weight"

    def __init__(self):
        self.preds = {}                          # exit -> {pred: edge_len}, in the recorded order

    def predecessors_iter(self, node):
        return iter(self.preds[node])

    def __getitem__(self, pred):
        return {x: {self.edge_len: d[pred]} for x, d in self.preds.items() if pred in d}


class StandInSet:
    """HaplotypeSet (phasm/phasing.py:58-108)."""

    def __init__(self, ploidy, copy_from=None):
        self.ploidy = ploidy
        self.haplotypes = [deque(copy_from.haplotypes[i]) if copy_from else deque() for i in range(ploidy)]
        self.read_sets = [set(copy_from.read_sets[i]) if copy_from else set() for i in range(ploidy)]
        self.log_rl = -math.inf
        self.from_large_bubble = False

    def extend(self, extensions, ext_read_sets):
        new = StandInSet(self.ploidy, copy_from=self)
        for i, (extension, reads) in enumerate(zip(extensions, ext_read_sets)):
            nodes = new.haplotypes[i]
            nodes.extend(extension[1:] if nodes and nodes[-1] == extension[0] else extension)
            new.read_sets[i].update(reads)
        return new


StandInBubble = namedtuple("StandInBubble", "entrance exit paths interior")


class StandInWalker:
    """BubbleChainPhaser as far as a walk touches it.  ``phase()`` restates the loop of the reference (phasm/phasing.py:182-341)
    over the recorded bubbles: what ``find_superbubbles``, ``networkx.all_simple_paths`` and ``superbubble_nodes`` gave is read
    from the golden.  ``branch``, ``get_aligning_reads`` and ``get_relevant_read_info`` are what ``device_phaser`` replaces:
    here they raise."""

    def __init__(self, g, bubbles, ploidy, min_spanning_reads, max_bubble_size, threshold, prune_factor, max_candidates, max_prune_rounds,
                 prune_step_size):
        self.g, self.chain, self.ploidy = g, bubbles, ploidy
        self.start_of_block = True                                                   # phasing.py:125-142
        self.prev_aligning_reads, self.prev_graph_reads = set(), set()
        self.min_spanning_reads, self.max_bubble_size = min_spanning_reads, max_bubble_size
        self.threshold, self.prune_factor = threshold, prune_factor
        self.max_candidates, self.max_prune_rounds, self.prune_step_size = max_candidates, max_prune_rounds, prune_step_size
        self.candidate_sets = [StandInSet(self.ploidy)]
        self.debug_data_log = None

    def phase(self):
        for bubble in self.chain:
            again = True
            while again:                                                             # ("try again at the same bubble", :320-332)
                again = False
                exit_, possible_paths, interior_nodes = bubble.exit, list(bubble.paths), bubble.interior
                cur_bubble_graph_reads = set(self.get_all_reads(interior_nodes))    # :231-234
                cur_bubble_aligning_reads = self.get_aligning_reads(interior_nodes)
                if len(possible_paths) > self.max_bubble_size:                      # :242-259
                    if not self.start_of_block:
                        yield self.new_block()
                    rel_read_info = self.get_relevant_read_info(cur_bubble_aligning_reads, cur_bubble_graph_reads, exit_)
                    yield (self.phase_large_bubble(possible_paths, rel_read_info), False)
                    continue
                spanning_reads = (self.prev_aligning_reads & cur_bubble_aligning_reads)   # :263-264
                if (len(spanning_reads) < self.min_spanning_reads and not self.start_of_block):   # :266-275
                    yield self.new_block()
                relevant_reads = (spanning_reads if not self.start_of_block else cur_bubble_aligning_reads)   # :283-286
                rel_read_info = self.get_relevant_read_info(relevant_reads, cur_bubble_graph_reads, exit_)
                total_relevant_la = 0                                               # :288-290
                for read_alignments, _ in rel_read_info.values():
                    total_relevant_la += len(read_alignments)
                if total_relevant_la == 0:                                          # :299-305
                    continue
                new_haplotype_sets = self.branch(possible_paths, rel_read_info)     # :307-309
                new_haplotype_sets = self.prune(new_haplotype_sets, self.prune_factor)
                if new_haplotype_sets:                                              # :311-319
                    self.candidate_sets = new_haplotype_sets
                    self.prev_graph_reads.update(cur_bubble_graph_reads)
                    self.prev_aligning_reads.update(cur_bubble_aligning_reads)
                    self.start_of_block = False
                else:                                                               # :320-332
                    yield self.new_block()
                    again = True
        if not self.start_of_block:                                                 # :335-339
            self.candidate_sets = self.prune(self.candidate_sets, 1.0)
            yield random.choice(self.candidate_sets), True

    def new_block(self):                                                            # :343-364
        best_candidates = self.prune(self.candidate_sets, 1.0)
        random_best = random.choice(best_candidates)
        self.candidate_sets = [StandInSet(self.ploidy)]
        self.prev_graph_reads = set()
        self.prev_aligning_reads = set()
        self.start_of_block = True
        return random_best, False

    def prune(self, candidate_sets, prune_factor):
        """``phase_utils.prune_definition`` on the sets' log_rl (phasing.py:482-539)."""
        if len(candidate_sets) < 2:
            return candidate_sets
        if callable(prune_factor):
            prune_factor = prune_factor(len(candidate_sets))
        spec = {"factor": prune_factor, "step": self.prune_step_size, "max_candidates": self.max_candidates, "max_rounds": self.max_prune_rounds}
        return [candidate_sets[j] for j in pu.prune_definition([hs.log_rl for hs in candidate_sets], spec)]

    def get_all_reads(self, nodes):                                                 # :552-562
        for node in nodes:
            if isinstance(node, StandInMerged):
                for read in node.reads:
                    yield read
            else:
                yield node

    def phase_large_bubble(self, possible_paths, relevant_reads):
        """The set the reference returns at a large bubble: the best-scored path in slot 0, the first of equals.  The score is
        ``phase_utils._overlap`` summed over the relevant reads (the common division by their number left out); the mapping is
        read the way the reference's method reads it -- ``info.alignments``, ``info.overlap_max``, ``la.get_oriented_reads()``,
        ``la.arange`` -- so what ``device_phaser`` hands to the inherited method must offer exactly that."""
        interiors = [set(self.get_all_reads(path[1:-1])) for path in possible_paths]
        reads = [([(la.get_oriented_reads()[1], la.arange[0], la.arange[1]) for la in info.alignments], info.overlap_max)
                 for info in relevant_reads.values()]
        totals = [sum(f for f in (pu._overlap(las, om, interior) for las, om in reads) if f is not None) for interior in interiors]
        winner = max(range(len(totals)), key=lambda p: (totals[p], -p))
        hs = StandInSet(self.ploidy)
        hs.haplotypes[0].extend(possible_paths[winner])
        hs.read_sets[0] |= interiors[winner]
        hs.from_large_bubble = True
        return hs

    def branch(self, possible_paths, relevant_reads):
        raise AssertionError("the inherited method ran")

    def get_aligning_reads(self, nodes):
        raise AssertionError("the inherited method ran")

    def get_relevant_read_info(self, relevant_reads, cur_bubble_graph_reads, bubble_exit):
        raise AssertionError("the inherited method ran")


def stand_ins(walk):
    """(node id -> stand-in object, the graph, the chain of StandInBubble) of a recorded walk."""
    n = n_ids_of(walk)
    nodes = {i: StandInRead(i, int(ln)) for i, ln in enumerate(lengths_of(walk).tolist())}
    for j, m in enumerate(walk["merged"]):
        nodes[n + j] = StandInMerged(n + j, m["length"], [nodes[r] for r in m["reads"]], list(m["prefix_lengths"]))
    g = StandInGraph()
    chain = []
    for b in walk["bubbles"]:
        g.preds[nodes[b["exit"]]] = {nodes[p]: e for p, e in b["preds"]}
        chain.append(StandInBubble(nodes[b["entrance"]], nodes[b["exit"]], [tuple(nodes[x] for x in p) for p in b["paths"]],
                                   [nodes[x] for x in b["interior_nodes"]]))
    return nodes, g, chain


# ---- the two routes ----------------------------------------------------------------------------------------------------------------

def run_integration(walk, scorer, source, index, walker=StandInWalker, raw=None):
    """The walk through ``device_phaser(StandInWalker, scorer, index=..., read_id=..., source=...)``: all three replaced methods
    of integration/phasm/phasing_device.py under the restated loop.  Returns (steps, final, state) as the recorder notes them.
    ``raw`` (a list) receives the bytes of every kept list."""
    nodes, g, chain = stand_ins(walk)
    read_id = {r: i for i, r in nodes.items() if i < n_ids_of(walk)}
    cls = device_phaser_factory()(walker, scorer, index=index, read_id=read_id, source=source)
    ph = cls(g, chain, **phaser_arguments(walk["params"]))
    rec = Recorder(ph, walk, walk["bubbles"], lambda x: x.ident, StandInSet)
    out = rec.run()
    if raw is not None:
        for s in rec.steps:
            if "kept_rl" in s:
                raw.append((len(raw), np.asarray(s["kept_cand"], np.uint32).tobytes(), np.asarray(s["kept_ext"], np.uint32).tobytes(),
                            np.asarray(s["kept_rl"], np.float64).tobytes()))
    return out


def _new_block(cands, params):
    """``new_block`` on (hist, sets, rl) candidates: the yield and the tie set."""
    keep = pu.prune_definition([c[2] for c in cands], prune_spec(params, 1.0))
    hist, sets, _ = cands[keep[0]]
    return {"kind": "new_block", "include_last": 0, "tie": keep, "haplotypes": [list(h) for h in hist], "read_sets": [sorted(s) for s in sets]}, keep


def run_arrays(walk, scorer, source, index, raw=None, translate=None, keep_prev_graph=False, sort_kept=False):
    """The walk through ``phasing.relevant_reads`` -> ``bubble_from_relevant`` -> ``branch_and_prune`` (at a large bubble
    ``score_paths`` and ``best_paths``; with a callable prune factor ``branch`` first), the candidates carried as (path history,
    read-id sets, log_rl).  ``raw`` (a list) receives the bytes of every (cand, ext, rl) the scorer returned.  The last three
    arguments break the route on purpose, for the tests of these tests."""
    p = walk["params"]
    k = p["ploidy"]
    fresh = lambda: [([[] for _ in range(k)], [set() for _ in range(k)], -math.inf)]   # noqa: E731
    cands, prev_graph, prev_aligning, start = fresh(), set(), set(), True
    steps, i, last_bubble = [], 0, None
    while i < len(walk["bubbles"]):
        b = walk["bubbles"][i]
        paths = b["paths"]
        path_reads = [node_reads(walk, path[1:-1]) for path in paths]
        s = {"bubble": i, "start": int(start), "state_in": digest_state(start, prev_graph, prev_aligning, [c[:2] for c in cands]),
             "arm": "skipped", "broke": 0, "fell_back": 0, "yields": []}
        steps.append(s)
        large = len(paths) > p["max_bubble_size"]
        rel = phasing.relevant_reads(source, index, b["interior_reads"], [] if large else sorted(prev_graph), sorted(prev_aligning),
                                     plain_preds(walk, b), start or large, 0 if large else p["min_spanning_reads"])
        as_result = rel_u.result_of_relevant(rel)
        s.update({key: as_result[key] for key in REL_KEYS + ("cur_aligning", "n_spanning")})
        s["n_b"] = len(rel.b_reads)
        stats = getattr(source, "relevant_stats", None)
        if stats is not None:
            s["relevant_stats"] = stats()
        if (large and not start) or rel.fell_back:
            y, _ = _new_block(cands, p)
            s["yields"].append(y)
            s["broke"], s["fell_back"] = 1, int(rel.fell_back)
            cands, start = fresh(), True
            prev_aligning = set()
            if not keep_prev_graph:
                prev_graph = set()
        if large:
            bubble = phasing.bubble_from_relevant(rel, k, path_reads, [[[] for _ in range(k)]])
            scores = phasing.score_paths(scorer, bubble)
            s["scores"] = scores.tolist()
            s["best"] = phasing.best_paths(scores, k)
            s["winner"] = s["best"][0]
            s["arm"] = "large"
            s["yields"].append({"kind": "large", "include_last": 0, "tie": None, "haplotypes": [list(paths[s["winner"]])] + [[] for _ in range(k - 1)],
                                "read_sets": [sorted(set(path_reads[s["winner"]]))] + [[] for _ in range(k - 1)]})
            i += 1
            continue
        if len(rel.aln_b) == 0:
            i += 1
            continue
        if translate is not None and last_bubble is not None:
            bubble = translate(rel, last_bubble, k, path_reads, [c[1] for c in cands])
        else:
            bubble = phasing.bubble_from_relevant(rel, k, path_reads, [c[1] for c in cands])
        last_bubble = bubble
        R = len(rel.rel_reads)
        threshold = resolve(p["threshold"], R)
        s["n_cands_in"] = len(cands)
        factor = p["prune_factor"]
        if callable(param(factor)):
            cand, ext, rl = phasing.branch(scorer, bubble, start, threshold, p["min_spanning_reads"])
            s["kept_cand"], s["kept_ext"], s["kept_rl"] = cand.tolist(), ext.tolist(), rl.tolist()
            if raw is not None:
                raw.append((len(raw), cand.tobytes(), ext.tobytes(), rl.tobytes()))
            factor = resolve(factor, len(rl)) if len(rl) >= 2 else 0.0
        cand, ext, rl = phasing.branch_and_prune(scorer, bubble, start, threshold, p["min_spanning_reads"], factor, p["prune_step_size"],
                                                 p["max_candidates"], p["max_prune_rounds"])
        if raw is not None:
            raw.append((len(raw), cand.tobytes(), ext.tobytes(), rl.tobytes()))
        st = scorer.phase_stats()
        s["phase_stats"] = st
        s["n_kept"] = int(st["n_kept"])
        s["prune_factor"] = None if s["n_kept"] < 2 else float(factor)
        s["surv_cand"], s["surv_ext"], s["surv_rl"] = cand.tolist(), ext.tolist(), rl.tolist()
        s["arm"] = "advanced"
        if len(rl):
            order = range(len(rl))
            if sort_kept:
                order = sorted(order, key=lambda j: -s["surv_rl"][j])
            new = []
            for j in order:
                digits = phasing.ext_digits(s["surv_ext"][j], len(paths), k)
                hist, sets, _ = cands[s["surv_cand"][j]]
                h2, s2 = extended(hist, sets, [paths[d] for d in digits], [path_reads[d] for d in digits])
                new.append((h2, s2, s["surv_rl"][j]))
            cands = new
            prev_graph |= set(b["interior_reads"])
            prev_aligning |= set(s["cur_aligning"])
            start = False
            i += 1
        else:
            y, _ = _new_block(cands, p)
            s["yields"].append(y)
            s["arm"] = "retry"
            cands, prev_graph, prev_aligning, start = fresh(), set(), set(), True
    final = {"yields": []}
    if not start:
        n_in = len(cands)
        keep = pu.prune_definition([c[2] for c in cands], prune_spec(p, 1.0))
        cands = [cands[j] for j in keep]
        final = {"prune_in": n_in, "yields": [{"kind": "final", "include_last": 1, "tie": keep, "haplotypes": [list(h) for h in cands[0][0]],
                                                "read_sets": [sorted(x) for x in cands[0][1]]}]}
    state = {"start": int(start), "prev_graph": sorted(prev_graph), "prev_aligning": sorted(prev_aligning), "n_cands": len(cands),
             "digest": digest_state(start, prev_graph, prev_aligning, [c[:2] for c in cands]),
             "cands": [{"haplotypes": [list(h) for h in c[0]], "read_sets": [sorted(x) for x in c[1]]} for c in cands]}
    return steps, final, state


def stale_translation(rel, last_bubble, k, path_reads, read_sets):
    """A broken ``bubble_from_relevant``: the candidates' read sets go through the PREVIOUS bubble's id map."""
    good = phasing.bubble_from_relevant(rel, k, path_reads, read_sets)
    old = {r: j for j, r in enumerate(last_bubble.b_reads)}
    good.set_off, good.set_ids = phasing._csr([sorted({old[x] for x in s if x in old and old[x] < good.n_b}) for c in read_sets for s in c])
    return good


class LeakyWalker(StandInWalker):
    """A broken walker: ``new_block`` leaves ``prev_graph_reads`` as it is."""

    def new_block(self):
        kept = self.prev_graph_reads
        out = super().new_block()
        self.prev_graph_reads = kept
        return out


class SortingWalker(StandInWalker):
    """A broken walker: the survivors become the candidates sorted by log_rl."""

    def prune(self, candidate_sets, prune_factor):
        out = super().prune(candidate_sets, prune_factor)
        return sorted(out, key=lambda hs: -hs.log_rl) if prune_factor != 1.0 else out


# ---- comparison ------------------------------------------------------------------------------------------------------------------

def _same_yield(got, want, where):
    for key in ("kind", "include_last", "tie", "haplotypes", "read_sets"):
        assert got[key] == want[key], "%s: yield differs in %s: %r != %r" % (where, key, got[key], want[key])


def same_trace(got, want, walk, optional=()):
    """(steps, final, state) of a route against the recorded walk: everything exactly but log_rl (``phase_utils.tol``) and the
    path scores (``phase_utils.table_tol``).  Keys in ``optional`` may be missing from ``got``."""
    steps, final, state = got
    k = walk["params"]["ploidy"]
    for n, (g, w) in enumerate(zip(steps, want["trace"])):
        where = "%s step %d (bubble %d)" % (walk["name"], n, w["bubble"])
        for key in EXACT_KEYS:
            if key in w and not (key in optional and key not in g):
                assert key in g, "%s: no %s" % (where, key)
                assert g[key] == w[key], "%s: %s differs: %r != %r" % (where, key, g[key], w[key])
            elif key not in w:
                assert key not in g, "%s: %s where the reference has none" % (where, key)
        R = len(w.get("rel_reads", ()))
        for key in ("kept_rl", "surv_rl"):
            if key in w and not (key in optional and key not in g):
                assert len(g[key]) == len(w[key]) and all(pu.same_rl(a, b, k, R) for a, b in zip(g[key], w[key])), "%s: %s differs" % (where, key)
        if "scores" in g:
            assert all(abs(a - b) * R <= pu.table_tol(b * R, R) for a, b in zip(g["scores"], w["scores"])), "%s: scores differ" % where
        assert len(g["yields"]) == len(w["yields"]), "%s: the yields differ" % where
        for a, b in zip(g["yields"], w["yields"]):
            _same_yield(a, b, where)
    assert len(steps) == len(want["trace"]), "%s: %d steps, the reference took %d" % (walk["name"], len(steps), len(want["trace"]))
    assert len(final["yields"]) == len(want["final"]["yields"]) and final.get("prune_in") == want["final"].get("prune_in"), \
        "%s: the final prune differs" % walk["name"]
    for a, b in zip(final["yields"], want["final"]["yields"]):
        _same_yield(a, b, walk["name"] + " final")
    for key in ("start", "prev_graph", "prev_aligning", "n_cands", "digest", "cands"):
        assert state[key] == want["state"][key], "%s: the state after the walk differs in %s" % (walk["name"], key)


def expected_stats(walk, w):
    """What ``relevant_stats()`` and ``phase_stats()`` must say after the calls of one recorded step."""
    k, P = walk["params"]["ploidy"], len(walk["bubbles"][w["bubble"]]["paths"])
    rel = {"n_cur_aligning": len(w["cur_aligning"]), "n_spanning": w["n_spanning"], "fell_back": w["fell_back"], "n_relevant": len(w["rel_reads"]),
           "n_alignments": len(w["aln_y"]), "n_b": w["n_b"]}
    ph = None
    if "n_kept" in w:
        start_now = w["start"] or w["broke"]
        n_tuples = math.comb(P + k - 1, k) if start_now else P ** k
        ph = {"n_extensions": w["n_cands_in"] * n_tuples, "n_kept": w["n_kept"], "n_survivors": len(w["surv_cand"])}
    return rel, ph


# ---- the trace's own consistency: every branch step as a one-bubble case of phase_utils ---------------------------------------------

def branch_cases(walk):
    """Replays the recorded trace -- the candidates rebuilt from the survivors' (cand, ext), the state digests checked on the
    way -- and yields (step, case) for every step with a ``branch``: the bubble re-packed as a case of tests/phase_utils.py with
    the recorded lists as its ``ref``."""
    p = walk["params"]
    k = p["ploidy"]
    fresh = lambda: [([[] for _ in range(k)], [set() for _ in range(k)])]   # noqa: E731
    cands, prev_graph, prev_aligning, start = fresh(), set(), set(), True
    for w in walk["trace"]:
        b = walk["bubbles"][w["bubble"]]
        assert w["state_in"] == digest_state(start, prev_graph, prev_aligning, cands) and w["start"] == int(start)
        if w["broke"]:
            cands, prev_graph, prev_aligning, start = fresh(), set(), set(), True
        if "n_b" in w:
            assert w["n_b"] == len(set(b["interior_reads"]) | prev_graph)
        if "kept_cand" not in w:
            continue
        paths = b["paths"]
        path_reads = [node_reads(walk, path[1:-1]) for path in paths]
        R = len(w["rel_reads"])
        named = sorted(set(w["aln_y"]))
        local = {y: j for j, y in enumerate(named)}
        aln = [[(local[w["aln_y"][j]], w["aln_a0"][j], w["aln_a1"][j]) for j in range(w["aln_off"][r], w["aln_off"][r + 1])] for r in range(R)]
        ids = lambda reads: [local[x] for x in reads if x in local]   # noqa: E731
        bubble = phasing.bubble_from_arrays(k, w["overlap_max"], aln, [ids(r) for r in path_reads], [[ids(x) for x in c[1]] for c in cands],
                                            len(named))
        case = {"k": k, "P": len(paths), "C": len(cands), "R": R, "n_b": len(named), "start": int(start), "min_span": p["min_spanning_reads"],
                "threshold": float(resolve(p["threshold"], R)),
                "prune": None if w["prune_factor"] is None else prune_spec(p, w["prune_factor"])}
        for key in pu.INPUT_KEYS:
            case[key] = getattr(bubble, key).tolist()
        place = {ce: j for j, ce in enumerate(zip(w["kept_cand"], w["kept_ext"]))}
        case["ref"] = {"kept_cand": w["kept_cand"], "kept_ext": w["kept_ext"], "kept_rl": w["kept_rl"],
                       "surv": [place[ce] for ce in zip(w["surv_cand"], w["surv_ext"])], "scores": None, "winner": None}
        assert len(place) == len(w["kept_cand"]) and w["n_cands_in"] == len(cands)
        yield w, case
        if w["arm"] == "advanced":
            new = []
            for c, e in zip(w["surv_cand"], w["surv_ext"]):
                digits = phasing.ext_digits(e, len(paths), k)
                new.append(extended(cands[c][0], cands[c][1], [paths[d] for d in digits], [path_reads[d] for d in digits]))
            cands = new
            prev_graph |= set(b["interior_reads"])
            prev_aligning |= set(w["cur_aligning"])
            start = False
        else:
            assert w["arm"] == "retry" and not w["surv_cand"]
            cands, prev_graph, prev_aligning, start = fresh(), set(), set(), True


def margins_hold(walk):
    """The margin conditions of ``phase_utils.conditions_hold`` at every step of a recorded walk: no log_rl within 4 tol of the
    threshold, none within 4 tol of a prune level the loop consulted, the path scores of a large bubble apart where the choice
    falls; and at every ``prune(.., 1.0)`` -- ``new_block`` and the end -- every entry either EQUAL to the greatest or more than
    4 tol below it (equal entries come from identical inputs: twin paths).  Returns the reason it does not hold, or None."""
    k = walk["params"]["ploidy"]
    last_rl, R_last = None, 0
    for w, case in branch_cases(walk):
        all_rl, levels = [], []
        d = dict(pu.definition(case, all_rl), scores=None, winner=None)
        pu.check_result(d, case["ref"], case)
        pu.prune_definition(d["kept_rl"], case["prune"], levels)
        if not pu.conditions_hold(case, [x[2] for x in all_rl], case["ref"]["kept_rl"], levels, None):
            return "step at bubble %d: a log_rl within 4 tol of the threshold or of a prune level" % w["bubble"]
    for w in walk["trace"]:
        R = len(w.get("rel_reads", ()))
        for y in w["yields"]:
            if y["kind"] == "new_block" and last_rl and not _clear_tie(last_rl, k, R_last):
                return "new_block at bubble %d: a near tie" % w["bubble"]
        if w["arm"] == "advanced":
            last_rl, R_last = w["surv_rl"], R
        elif w["arm"] == "retry" or w["broke"]:
            last_rl = None
        if w["arm"] == "large":
            top = sorted(w["scores"], reverse=True)[:k + 1]
            if any((a - b) * R <= 4 * pu.table_tol(a * R, R) for a, b in zip(top, top[1:])):
                return "large bubble %d: two path scores within 4 tol" % w["bubble"]
    if walk["final"]["yields"] and last_rl and not _clear_tie(last_rl, k, R_last):
        return "the final prune: a near tie"
    return None


def _clear_tie(rls, k, R):
    best = max(rls)
    return all(x == best or not math.isfinite(x) or best - x > 4 * pu.tol(x, k, R) for x in rls)


def situations(walk):
    """The situations a recorded walk shows (the second entry of SPECS names those it must)."""
    out = set()
    p, trace, bubbles = walk["params"], walk["trace"], walk["bubbles"]
    n = n_ids_of(walk)
    for j, w in enumerate(trace):
        out.add(w["arm"])
        b = bubbles[w["bubble"]]
        if w["fell_back"]:
            out.add("fell_back")
            if w["n_b"] < 8 and any(t.get("n_b", 0) > 64 for t in trace[:j]):
                out.add("nb_below_8_after_a_break")
                if [t["arm"] for t in trace[j + 1:j + 3]] == ["advanced", "advanced"] and all(t["n_b"] < 32 for t in trace[j + 1:j + 3]):
                    out.add("two_small_bubbles_follow")
        if "n_b" in w and w["arm"] != "skipped":
            out.add("nb_below_32" if w["n_b"] < 32 else "nb_past_64" if w["n_b"] > 64 else "nb_past_32")
        if len(w.get("rel_reads", ())) > 64:
            out.add("relevant_past_64")
        if w.get("n_cands_in", 0) > 64:
            out.add("cands_past_64")
        if w["arm"] == "advanced" and len(w["surv_cand"]) < w["n_kept"] and w["prune_factor"] is not None:
            levels = []
            pu.prune_definition(w["kept_rl"], prune_spec(p, w["prune_factor"]), levels)
            if len(levels) > 1:
                out.add("cut_by_max_candidates")
        if len(b["paths"]) == 4 and w["arm"] != "large":
            out.add("four_paths")
        if w["arm"] == "large":
            out.add("large_at_the_start" if j == 0 else "large_behind_phased_bubbles" if w["broke"] and j >= 2 else "large")
        if w["arm"] == "skipped":
            if w["start"] and w["rel_reads"] and not w["aln_y"]:
                out.add("skipped_at_a_start_with_relevant_reads")
            if not w["start"] and j + 1 < len(trace) and trace[j + 1]["state_in"] == w["state_in"]:
                out.add("skipped_in_the_middle_state_kept")
        if "rel_reads" in w and len(plain_preds(walk, b)) >= 2:
            lens = lengths_of(walk)
            if any(om < lens[r] for r, om in zip(w["rel_reads"], w["overlap_max"])):
                out.add("clipped_by_two_preds")
        if callable(param(p["threshold"])) and "rel_reads" in w:
            out.add("threshold_below_the_step" if len(w["rel_reads"]) < p["threshold"][1] else "threshold_from_the_step")
        if callable(param(p["prune_factor"])) and w.get("prune_factor") is not None:
            out.add("factor_below_the_step" if w["n_kept"] < p["prune_factor"][1] else "factor_from_the_step")
        if any(x >= n for path in b["paths"] for x in path[1:-1]) and w["arm"] == "advanced":
            out.add("merged_interior")
        if any(x >= n for x, _ in b["preds"]) and w["arm"] == "advanced":
            out.add("merged_pred")
        for y in w["yields"]:
            if y["kind"] == "new_block" and len(y["tie"]) > 1:
                out.add("tie_at_a_new_block")
    if sum(1 for t in trace if t["arm"] == "advanced" and t["prune_factor"] is not None and _rounds(t, p) >= 3) >= 2:
        out.add("several_prune_rounds_at_two_bubbles")
    if {"threshold_below_the_step", "threshold_from_the_step"} <= out:
        out.add("both_sides_of_the_threshold_step")
    if {"factor_below_the_step", "factor_from_the_step"} <= out:
        out.add("both_sides_of_the_factor_step")
    for y in walk["final"]["yields"]:
        if len(y["tie"]) > 1:
            out.add("tie_at_the_end")
    # a read outside the graph whose alignments reach three bubbles
    rows = rows_of(walk)
    home = {}
    for i, b in enumerate(bubbles):
        for r in b["interior_reads"]:
            home[r] = i
    reach = {}
    for a, b_, *_ in rows.tolist():
        for x, y in ((a, b_), (b_, a)):
            if y in home and x not in home:
                reach.setdefault(x, set()).add(home[y])
    if any(len(v) >= 3 for v in reach.values()):
        out.add("spans_three_bubbles")
    return out


def _rounds(t, p):
    levels = []
    pu.prune_definition(t["kept_rl"], prune_spec(p, t["prune_factor"]), levels)
    return len(levels)


# ---- golden file -----------------------------------------------------------------------------------------------------------------

PACKED = ("bubbles", "trace", "final", "state")


def _pack(o, pool):
    """Every list of more than 8 integers becomes a slice of ``pool``: one array per walk instead of one per list."""
    if isinstance(o, dict):
        return {k: _pack(v, pool) for k, v in o.items()}
    if isinstance(o, list) and len(o) > 8 and all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) for x in o):
        pool += [int(x) for x in o]
        return {"__slice__": [len(pool) - len(o), len(o)]}
    if isinstance(o, list):
        return [_pack(v, pool) for v in o]
    return o


def _unpack(o, pool):
    if isinstance(o, dict):
        if set(o) == {"__slice__"}:
            return pool[o["__slice__"][0]:o["__slice__"][0] + o["__slice__"][1]]
        return {k: _unpack(v, pool) for k, v in o.items()}
    if isinstance(o, list):
        return [_unpack(v, pool) for v in o]
    return o


def save_golden(obj):
    walks = []
    for w in obj["walks"]:
        pool = []
        packed = dict(w)
        for key in PACKED:
            packed[key] = _pack(w[key], pool)
        packed["pool"] = pool + [0] * 9               # (long enough to be stored as an array whatever the walk)
        walks.append(packed)
    cu.save_golden(dict(obj, walks=walks), GOLDEN_FILE)


_GOLDEN = []


def load_golden():
    if not _GOLDEN:
        obj = cu.load_golden(GOLDEN_FILE)
        for w in obj["walks"]:
            pool = w.pop("pool")
            for key in PACKED:
                w[key] = _unpack(w[key], pool)
        _GOLDEN.append(obj)
    return _GOLDEN[0]
