"""``BubbleChainPhaser.branch`` on the device, for a process that runs the reference's `phasm phase` with this package.

    from phasm.phasing import BubbleChainPhaser
    from phasm.phasing_device import device_phaser
    phaser = device_phaser(BubbleChainPhaser, ExactOverlapper())(g, ploidy, ...)     # then phaser.phase(alignments) as before

The subclass replaces ``branch`` alone: it packs the bubble (``phasm_amd.phasing.pack_bubble``), has ``po_phase_branch`` score
and filter every extension of every candidate set, and rebuilds the kept ``HaplotypeSet``s with the class's own ``extend``, in
the order of the inherited method.  ``prune`` then runs unchanged on that list, as do the bubble walk, ``new_block`` and
everything else.  With a debug data file set the inherited ``branch`` runs: the device returns no per-read probabilities."""
from phasm_amd import phasing


def device_phaser(phaser_class, scorer):
    """A subclass of ``phaser_class`` (the reference's ``BubbleChainPhaser``) whose ``branch`` runs on ``scorer`` (an
    ``ExactOverlapper``, or a ``phasm_amd.phasing.HostScorer``)."""

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
