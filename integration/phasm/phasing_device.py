"""``BubbleChainPhaser.branch`` on the device, for a process that runs the reference's `phasm phase` with this package.

    from phasm.phasing import BubbleChainPhaser
    from phasm.phasing_device import device_phaser
    phaser = device_phaser(BubbleChainPhaser, ExactOverlapper())(g, ploidy, ...)     # then phaser.phase(alignments) as before

The subclass replaces ``branch`` alone: it packs the bubble (``phasm_amd.phasing.pack_bubble``), has ``po_phase_branch`` score
and filter every extension of every candidate set, and rebuilds the kept ``HaplotypeSet``s with the class's own ``extend``, in
the order of the inherited method.  ``prune`` then runs unchanged on that list, as do the bubble walk, ``new_block`` and
everything else.  With a debug data file set the inherited ``branch`` runs: the device returns no per-read probabilities.

With an alignment index the subclass also replaces ``get_aligning_reads`` and ``get_relevant_read_info``:

    index = ov.phase_index(rows)                         # once; rows: the E lines as a row result (po_add_gfa)
    phaser = device_phaser(BubbleChainPhaser, ov, index=index, read_id=read_id)(g, ploidy, ...)

``read_id`` maps a read object to its oriented id on the handle (a dict or a callable).  Both methods then go through
``po_phase_relevant``; ``get_relevant_read_info`` returns ``{read: RelevantReadInfo(list of (b read, a0, a1), overlap_max)}``, which
``pack_bubble`` accepts.  The inherited ``phase_large_bubble`` reads the same mapping (phasm/phasing.py:649-662), so the info
also has ``.alignments`` and ``.overlap_max`` and every triple ``.arange`` and ``.get_oriented_reads()``, as the reference's
``RelevantReadInfo`` and ``LocalAlignment`` have.  Without ``index`` and ``read_id`` nothing changes."""
from collections import namedtuple

from phasm_amd import phasing

RelevantReadInfo = namedtuple("RelevantReadInfo", "alignments overlap_max")


class Alignment(tuple):
    """``(b read, a0, a1)`` of a relevant read, with what the reference's loops ask of a ``LocalAlignment``."""

    def __new__(cls, a, b, a0, a1):
        self = super().__new__(cls, (b, a0, a1))
        self.a = a
        return self

    arange = property(lambda self: (self[1], self[2]))

    def get_oriented_reads(self):
        return self.a, self[0]


def device_phaser(phaser_class, scorer, index=None, read_id=None, source=None):
    """A subclass of ``phaser_class`` (the reference's ``BubbleChainPhaser``) whose ``branch`` runs on ``scorer`` (an
    ``ExactOverlapper``, or a ``phasm_amd.phasing.HostScorer``).  With ``index`` and ``read_id`` the relevant reads come from
    ``source.phase_relevant`` (``source``: the ``ExactOverlapper`` or ``HostIndex`` the index belongs to; default: ``scorer``)."""
    if (index is None) != (read_id is None):
        raise ValueError("index and read_id go together")
    if index is not None:
        return _with_relevant(device_phaser(phaser_class, scorer), source if source is not None else scorer, index, read_id)

    class DevicePhaser(phaser_class):
        phase_scorer = scorer

        def branch(self, possible_paths, relevant_reads):
            if getattr(getattr(self, "debug_data_log", None), "outfile", None):
                return super().branch(possible_paths, relevant_reads)
            possible_paths = list(possible_paths)
            if not possible_paths or not self.candidate_sets:
                return []
            threshold = self.threshold(len(relevant_reads)) if callable(self.threshold) else self.threshold
            bubble = phasing.pack_bubble(possible_paths, [hs.read_sets for hs in self.candidate_sets], relevant_reads,
                                         expand=lambda node: self.get_all_reads([node]))
            cand, ext, rl = phasing.branch(self.phase_scorer, bubble, self.start_of_block, threshold, self.min_spanning_reads)
            path_reads = [set(self.get_all_reads(p[1:-1])) for p in possible_paths]
            out = []
            for c, e, r in zip(cand.tolist(), ext.tolist(), rl.tolist()):
                digits = phasing.ext_digits(e, len(possible_paths), self.ploidy)
                new_set = self.candidate_sets[c].extend(tuple(possible_paths[d] for d in digits), [path_reads[d] for d in digits])
                new_set.log_rl = r
                out.append(new_set)
            return out

    DevicePhaser.__name__ = "Device" + phaser_class.__name__
    return DevicePhaser


def _with_relevant(base, source, index, read_id):
    to_id = read_id if callable(read_id) else read_id.__getitem__

    class IndexedPhaser(base):
        relevant_source = source
        alignment_index = index

        def _read_of(self, reads):
            """oriented id -> the caller's read object, for the reads at hand and every read the caller's mapping knows."""
            back = getattr(self, "_id_to_read", None)
            if back is None:
                back = self._id_to_read = {}
                if not callable(read_id):
                    back.update((i, r) for r, i in read_id.items())
            for r in reads:
                back.setdefault(to_id(r), r)
            return back

        def get_aligning_reads(self, nodes):
            cur = list(self.get_all_reads(nodes))
            if not cur:
                return set()
            back = self._read_of(cur)
            rel = phasing.relevant_reads(self.relevant_source, self.alignment_index, [to_id(r) for r in cur], start_of_block=True)
            return {back[int(x)] for x in rel.cur_aligning}

        def get_relevant_read_info(self, relevant_reads, cur_bubble_graph_reads, bubble_exit):
            relevant_reads = list(relevant_reads)
            cur = list(cur_bubble_graph_reads)
            if not relevant_reads or not cur:
                return {r: RelevantReadInfo([], len(r)) for r in relevant_reads}
            prev = list(self.prev_graph_reads)
            preds = [(p, self.g[p][bubble_exit][self.g.edge_len]) for p in self.g.predecessors_iter(bubble_exit)
                     if not hasattr(p, "prefix_lengths")]                       # (a MergedReads predecessor yields len(read))
            back = self._read_of(cur + prev + relevant_reads + [p for p, _ in preds])
            # mode 0 with the wanted reads as prev_aligning: the relevant reads are those of them that align to the bubble
            rel = phasing.relevant_reads(self.relevant_source, self.alignment_index, [to_id(r) for r in cur], [to_id(r) for r in prev],
                                         [to_id(r) for r in relevant_reads], [(to_id(p), int(e)) for p, e in preds], False, 0)
            out = {back[int(x)]: RelevantReadInfo([Alignment(back[int(x)], back[b], a0, a1) for b, a0, a1 in rel.alignments_of(j)],
                                                  int(rel.overlap_max[j])) for j, x in enumerate(rel.rel_reads)}
            missing = [r for r in relevant_reads if r not in out]
            if missing:
                raise ValueError("get_relevant_read_info: %d reads that do not align to the bubble" % len(missing))
            return out

    IndexedPhaser.__name__ = base.__name__
    return IndexedPhaser
