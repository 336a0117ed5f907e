"""ctypes binding of libphasm_overlap.so (include/phasm_overlap.h).

There is no fallback: if the shared library is missing this raises ImportError, and the
library itself fails with PO_ERR_HIP when no GPU is usable.  (``cffi`` is not installed in the
target image, hence ctypes.)
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PHASM_LIB") or os.path.join(HERE, "libphasm_overlap.so")  # PHASM_LIB: dev override

PO_OK, PO_ERR_INVALID, PO_ERR_NOMEM, PO_ERR_HIP, PO_ERR_CAPACITY = range(5)

ROW_DTYPE = np.dtype([("a_idx", "<u4"), ("b_idx", "<u4"), ("astart", "<i4"),
                      ("aend", "<i4"), ("bstart", "<i4"), ("bend", "<i4")])


CAND_DTYPE = np.dtype([("a_idx", "<u4"), ("p", "<u4"), ("b_idx", "<u4"), ("type", "<u4")])


EDGE_DTYPE = np.dtype([("u", "<u4"), ("v", "<u4"), ("weight", "<i4"), ("overlap_len", "<i4")])
# po_edge_coverage
COVERAGE_DTYPE = np.dtype([("read_length_sum", "<u8"), ("path_length", "<i8")])
# po_component
COMPONENT_DTYPE = np.dtype([("first_node", "<u4"), ("n_nodes", "<u4"), ("n_edges", "<u8")])
# po_scc
SCC_DTYPE = np.dtype([("first_node", "<u4"), ("n_nodes", "<u4"), ("n_edges", "<u8"), ("n_r_in", "<u4"), ("n_re_out", "<u4")])
# PO_PART_*: the bits of po_layout_partition's flag byte per node
PART_R_IN, PART_RE_OUT, PART_START, PART_SINK = 1, 2, 4, 8
# po_superbubble
SUPERBUBBLE_DTYPE = np.dtype([("entrance", "<u4"), ("exit", "<u4"), ("n_inside", "<u4"), ("nested", "<u4")])
# PO_SB_*: the bits of po_layout_superbubbles' flag byte per node; PO_NO_NODE
SB_ENTRANCE, SB_EXIT, SB_NESTED, SB_SELF_LOOP = 1, 2, 4, 8
NO_NODE = 0xFFFFFFFF
# po_bubblechain
BUBBLECHAIN_DTYPE = np.dtype([("first_entrance", "<u4"), ("last_exit", "<u4"), ("n_bubbles", "<u4"), ("n_nodes", "<u4"), ("n_edges", "<u8")])
# po_bubble_paths; PO_PATHS_*
BUBBLE_PATHS_DTYPE = np.dtype([("entrance", "<u4"), ("exit", "<u4"), ("chain", "<u4"), ("position", "<u4"), ("n_inside", "<u4"),
                               ("flags", "<u4"), ("n_paths", "<u8"), ("n_path_nodes", "<u8")])
PATHS_BARE, PATHS_UNLISTED, PATHS_SATURATED = 1, 2, 4
PATHS_MANY = 0xFFFFFFFFFFFFFFFF
# po_contig
CONTIG_DTYPE = np.dtype([("first_node", "<u4"), ("last_node", "<u4"), ("n_nodes", "<u4"), ("first_edge", "<u4"), ("length", "<i8")])


class PoLayoutParams(ctypes.Structure):
    _fields_ = [("min_read_length", ctypes.c_uint32), ("min_overlap_length", ctypes.c_uint32),
                ("max_overhang_abs", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("max_overhang_rel", ctypes.c_double)]


class PoLayoutStats(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_uint64), ("n_type", ctypes.c_uint64 * 4), ("n_short", ctypes.c_uint64),
                ("n_min_overlap", ctypes.c_uint64), ("n_overhang", ctypes.c_uint64), ("n_pass", ctypes.c_uint64),
                ("n_contained_reads", ctypes.c_uint64), ("n_edges", ctypes.c_uint64),
                ("ms_classify", ctypes.c_float), ("ms_dedupe", ctypes.c_float), ("ms_emit", ctypes.c_float),
                ("ms_total", ctypes.c_float)]

    def as_dict(self) -> dict:
        d = {name: getattr(self, name) for name, _ in self._fields_}
        d["n_type"] = list(self.n_type)
        return d


class PoReduceParams(ctypes.Structure):
    _fields_ = [("length_fuzz", ctypes.c_int32), ("reserved", ctypes.c_uint32)]


class PoReduceStats(ctypes.Structure):
    _fields_ = [("n_edges_in", ctypes.c_uint64), ("n_transitive", ctypes.c_uint64), ("n_asymmetric", ctypes.c_uint64),
                ("n_edges_out", ctypes.c_uint64), ("max_out_degree", ctypes.c_uint64),
                ("ms_csr", ctypes.c_float), ("ms_mark", ctypes.c_float), ("ms_symmetric", ctypes.c_float),
                ("ms_emit", ctypes.c_float), ("ms_total", ctypes.c_float)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoTipsParams(ctypes.Structure):
    _fields_ = [("max_tip_len", ctypes.c_uint32), ("max_tip_len_bases", ctypes.c_int32), ("reserved", ctypes.c_uint32)]


class PoTipsStats(ctypes.Structure):
    _fields_ = [("n_edges_in", ctypes.c_uint64), ("n_in_tip_edges", ctypes.c_uint64), ("n_out_tip_edges", ctypes.c_uint64),
                ("n_asymmetric", ctypes.c_uint64), ("n_edges_out", ctypes.c_uint64), ("n_nodes", ctypes.c_uint64),
                ("n_isolated_nodes", ctypes.c_uint64), ("n_candidates_in", ctypes.c_uint64), ("n_candidates_out", ctypes.c_uint64),
                ("n_rounds_in", ctypes.c_uint64), ("n_rounds_out", ctypes.c_uint64),
                ("ms_setup", ctypes.c_float), ("ms_incoming", ctypes.c_float), ("ms_outgoing", ctypes.c_float),
                ("ms_symmetric", ctypes.c_float), ("ms_emit", ctypes.c_float), ("ms_total", ctypes.c_float)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoDiamondParams(ctypes.Structure):
    _fields_ = [("reserved", ctypes.c_uint32)]


class PoDiamondStats(ctypes.Structure):
    _fields_ = [("n_edges_in", ctypes.c_uint64), ("n_edges_out", ctypes.c_uint64), ("n_nodes", ctypes.c_uint64),
                ("n_nodes_removed", ctypes.c_uint64), ("n_candidates", ctypes.c_uint64), ("n_diamonds", ctypes.c_uint64),
                ("n_rounds", ctypes.c_uint64), ("n_invalid", ctypes.c_uint64),
                ("ms_setup", ctypes.c_float), ("ms_rounds", ctypes.c_float), ("ms_emit", ctypes.c_float), ("ms_total", ctypes.c_float)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoMergeParams(ctypes.Structure):
    _fields_ = [("reserved", ctypes.c_uint32)]


class PoMergeStats(ctypes.Structure):
    _fields_ = [("n_edges_in", ctypes.c_uint64), ("n_edges_out", ctypes.c_uint64), ("n_nodes", ctypes.c_uint64),
                ("n_merged", ctypes.c_uint64), ("n_nodes_merged", ctypes.c_uint64), ("max_path_nodes", ctypes.c_uint64),
                ("n_self_loops", ctypes.c_uint64), ("n_cycle_nodes", ctypes.c_uint64), ("n_rounds", ctypes.c_uint64),
                ("n_overflow", ctypes.c_uint64), ("n_invalid", ctypes.c_uint64),
                ("ms_links", ctypes.c_float), ("ms_rank", ctypes.c_float), ("ms_number", ctypes.c_float), ("ms_emit", ctypes.c_float),
                ("ms_total", ctypes.c_float)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoCoverageParams(ctypes.Structure):
    _fields_ = [("reserved", ctypes.c_uint32)]


class PoCoverageStats(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_uint64), ("n_edges", ctypes.c_uint64), ("n_nodes", ctypes.c_uint64), ("n_pairs", ctypes.c_uint64),
                ("max_set", ctypes.c_uint64), ("n_zero_path", ctypes.c_uint64), ("n_invalid", ctypes.c_uint64),
                ("ms_sets", ctypes.c_float), ("ms_edges", ctypes.c_float), ("ms_total", ctypes.c_float)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoComponentsParams(ctypes.Structure):
    _fields_ = [("reserved", ctypes.c_uint32)]


class PoComponentsStats(ctypes.Structure):
    _fields_ = [("n_nodes", ctypes.c_uint64), ("n_edges", ctypes.c_uint64), ("n_components", ctypes.c_uint64),
                ("n_singletons", ctypes.c_uint64), ("max_component_nodes", ctypes.c_uint64), ("max_component_edges", ctypes.c_uint64),
                ("n_invalid", ctypes.c_uint64), ("n_rounds", ctypes.c_uint32), ("n_batches", ctypes.c_uint32),
                ("ms_rounds", ctypes.c_float), ("ms_label", ctypes.c_float), ("ms_total", ctypes.c_float)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoPartitionParams(ctypes.Structure):
    _fields_ = [("reserved", ctypes.c_uint32)]


class PoPartitionStats(ctypes.Structure):
    _fields_ = [("n_nodes", ctypes.c_uint64), ("n_edges", ctypes.c_uint64), ("n_sccs", ctypes.c_uint64),
                ("n_nonsingleton_sccs", ctypes.c_uint64), ("n_singletons", ctypes.c_uint64), ("n_self_loops", ctypes.c_uint64),
                ("max_scc_nodes", ctypes.c_uint64), ("max_scc_edges", ctypes.c_uint64), ("n_trimmed", ctypes.c_uint64),
                ("n_class", ctypes.c_uint64 * 5), ("n_invalid", ctypes.c_uint64), ("n_outer", ctypes.c_uint32),
                ("n_trim_rounds", ctypes.c_uint32), ("n_forward_rounds", ctypes.c_uint32), ("n_backward_rounds", ctypes.c_uint32),
                ("n_batches", ctypes.c_uint32),
                ("ms_ranks", ctypes.c_float), ("ms_rounds", ctypes.c_float), ("ms_label", ctypes.c_float), ("ms_total", ctypes.c_float)]

    def as_dict(self) -> dict:
        d = {name: getattr(self, name) for name, _ in self._fields_}
        d["n_class"] = list(self.n_class)
        return d


class PoSuperbubbleParams(ctypes.Structure):
    _fields_ = [("reserved", ctypes.c_uint32)]


class PoSuperbubbleStats(ctypes.Structure):
    _fields_ = [("n_nodes", ctypes.c_uint64), ("n_edges", ctypes.c_uint64), ("n_p_nodes", ctypes.c_uint64), ("n_p_edges", ctypes.c_uint64),
                ("n_bubbles", ctypes.c_uint64), ("n_nested", ctypes.c_uint64), ("n_self_loop_nodes", ctypes.c_uint64),
                ("n_discarded", ctypes.c_uint64), ("n_invalid", ctypes.c_uint64), ("n_levels_forward", ctypes.c_uint32),
                ("n_levels_backward", ctypes.c_uint32), ("n_scc_rounds", ctypes.c_uint32), ("n_level_rounds", ctypes.c_uint32),
                ("n_discard_rounds", ctypes.c_uint32), ("n_batches", ctypes.c_uint32),
                ("ms_partition", ctypes.c_float), ("ms_levels", ctypes.c_float), ("ms_dominators", ctypes.c_float),
                ("ms_label", ctypes.c_float), ("ms_total", ctypes.c_float)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoSuperbubbleAllParams(ctypes.Structure):
    _fields_ = [("reserved", ctypes.c_uint32)]


class PoSuperbubbleAllStats(ctypes.Structure):
    _fields_ = [("n_nodes", ctypes.c_uint64), ("n_edges", ctypes.c_uint64), ("n_invalid", ctypes.c_uint64), ("n_bubbles", ctypes.c_uint64),
                ("n_nested", ctypes.c_uint64), ("n_cyclic_bubbles", ctypes.c_uint64), ("n_split", ctypes.c_uint64),
                ("n_rootless", ctypes.c_uint64), ("n_certified", ctypes.c_uint64), ("n_edge_filtered", ctypes.c_uint64),
                ("n_split_levels", ctypes.c_uint32), ("n_root_runs", ctypes.c_uint32), ("n_scc_rounds", ctypes.c_uint32),
                ("n_batches", ctypes.c_uint32), ("ms_ranks", ctypes.c_float), ("ms_split", ctypes.c_float), ("ms_bubbles", ctypes.c_float),
                ("ms_merge", ctypes.c_float), ("ms_total", ctypes.c_float)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoBubblechainParams(ctypes.Structure):
    _fields_ = [("min_nodes", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class PoBubblechainStats(ctypes.Structure):
    _fields_ = [("n_nodes", ctypes.c_uint64), ("n_edges", ctypes.c_uint64), ("n_bubbles", ctypes.c_uint64), ("n_top", ctypes.c_uint64),
                ("n_chains", ctypes.c_uint64), ("n_short", ctypes.c_uint64), ("n_chain_nodes", ctypes.c_uint64),
                ("n_chain_edges", ctypes.c_uint64), ("n_invalid", ctypes.c_uint64), ("max_chain_bubbles", ctypes.c_uint32),
                ("n_nest_rounds", ctypes.c_uint32), ("n_chain_rounds", ctypes.c_uint32), ("n_batches", ctypes.c_uint32),
                ("ms_superbubbles", ctypes.c_float), ("ms_chains", ctypes.c_float), ("ms_label", ctypes.c_float),
                ("ms_total", ctypes.c_float)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoBubblechainAllStats(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in (
                    "n_nodes", "n_edges", "n_bubbles", "n_top", "n_chains", "n_short", "n_chain_nodes", "n_chain_edges", "n_invalid",
                    "n_ring_chains", "n_ring_bubbles", "n_cyclic_bubbles")] + \
               [(name, ctypes.c_uint32) for name in ("max_chain_bubbles", "n_nest_rounds", "n_chain_rounds", "n_batches", "n_ring_rounds",
                                                     "n_root_runs", "n_split_levels", "reserved")] + \
               [(name, ctypes.c_float) for name in ("ms_superbubbles", "ms_chains", "ms_label", "ms_total")]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoContigParams(ctypes.Structure):
    _fields_ = [("min_contig_len", ctypes.c_uint64), ("min_nodes", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class PoContigStats(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in (
                    "n_nodes", "n_edges", "n_invalid", "n_excluded", "n_root_starts", "n_late_starts", "n_blocked", "n_covered_edges",
                    "n_uncovered_edges", "n_paths", "n_short_paths", "n_isolated", "n_short_isolated", "n_contigs", "max_path_nodes",
                    "n_chains")] + \
               [(name, ctypes.c_uint32) for name in ("n_path_rounds", "n_cover_rounds", "n_batches", "reserved")] + \
               [(name, ctypes.c_float) for name in ("ms_ranks", "ms_bubblechains", "ms_paths", "ms_cover", "ms_label", "ms_total")]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoPhaseParams(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint32) for name in (
                    "ploidy", "n_paths", "n_cands", "n_reads", "n_b", "start_of_block", "min_spanning_reads", "prune", "max_candidates",
                    "n_levels")] + \
               [("threshold", ctypes.c_double), ("reserved", ctypes.c_uint32), ("reserved2", ctypes.c_uint32)]


class PoPhaseInput(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in (
                    "overlap_max", "aln_off", "aln_b", "aln_a0", "aln_a1", "path_off", "path_ids", "set_off", "set_ids", "levels")]


class PoPhaseStats(ctypes.Structure):
    _fields_ = [("n_extensions", ctypes.c_uint64), ("n_kept", ctypes.c_uint64), ("n_survivors", ctypes.c_uint64),
                ("level_counts", ctypes.c_uint64 * 16), ("max_rl", ctypes.c_double), ("level_used", ctypes.c_int32),
                ("n_levels", ctypes.c_uint32)] + \
               [(name, ctypes.c_float) for name in ("ms_intervals", "ms_table", "ms_extend", "ms_filter", "ms_prune", "ms_total")]

    def as_dict(self) -> dict:
        d = {name: getattr(self, name) for name, _ in self._fields_}
        d["level_counts"] = list(self.level_counts)
        return d


ALIGNMENT_DTYPE = np.dtype([("b", np.uint32), ("a0", np.int32), ("a1", np.int32), ("seq", np.uint32)])


class PoPhaseIndexStats(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in ("n_rows", "n_keys", "max_degree", "n_invalid")] + \
               [(name, ctypes.c_float) for name in ("ms_insert", "ms_fill", "ms_place", "ms_total")]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoRelevantParams(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint32) for name in ("mode", "min_spanning_reads", "reserved", "reserved2")]


class PoWalkRelevantParams(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint32) for name in ("mode", "min_spanning_reads", "without_prev_graph", "reserved")]


class PoRelevantInput(ctypes.Structure):
    _fields_ = [("cur_graph", ctypes.c_void_p), ("n_cur_graph", ctypes.c_uint64), ("prev_graph", ctypes.c_void_p),
                ("n_prev_graph", ctypes.c_uint64), ("prev_aligning", ctypes.c_void_p), ("n_prev_aligning", ctypes.c_uint64),
                ("pred_read", ctypes.c_void_p), ("pred_edge_len", ctypes.c_void_p), ("n_pred", ctypes.c_uint64)]


class PoRelevantDims(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in ("n_cur_aligning", "n_spanning", "n_relevant", "n_alignments", "n_b")] + \
               [("fell_back", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class PoRelevantStats(ctypes.Structure):
    _fields_ = PoRelevantDims._fields_ + [(name, ctypes.c_float) for name in ("ms_mark", "ms_lists", "ms_alignments", "ms_total")]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class PoSpellInput(ctypes.Structure):
    _fields_ = [("n_seqs", ctypes.c_uint64), ("n_pieces", ctypes.c_uint64), ("seq_off", ctypes.c_void_p), ("piece_read", ctypes.c_void_p),
                ("piece_take", ctypes.c_void_p)]


class PoSpellStats(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in ("n_seqs", "n_pieces", "n_bytes", "n_patched")] + \
               [("device_ms", ctypes.c_float), ("reserved", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class PoPathsParams(ctypes.Structure):
    _fields_ = [("max_paths", ctypes.c_uint64), ("reserved", ctypes.c_uint32)]


class PoPathsDims(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in ("n_bubbles", "n_inside_nodes", "n_preds", "n_listed_paths", "n_path_nodes")]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoPathsStats(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in (
                    "n_nodes", "n_edges", "n_invalid", "n_bubbles", "n_bare", "n_unlisted", "n_saturated", "n_listed_paths", "n_path_nodes",
                    "max_paths_seen", "max_path_nodes", "n_stray_edges")] + \
               [(name, ctypes.c_uint32) for name in ("n_count_rounds", "n_batches")] + \
               [(name, ctypes.c_float) for name in ("ms_chains", "ms_count", "ms_list", "ms_total")]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoLargeParams(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint32) for name in ("bubble", "n_reads", "n_b", "n_best", "reserved")]


class PoLargeInput(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ("overlap_max", "aln_off", "aln_b", "aln_a0", "aln_a1", "node_off", "node_ids")] + \
               [("n_nodes", ctypes.c_uint32)]


class PoLargeStats(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in ("n_paths", "n_inside", "n_reads", "max_path_nodes")] + \
               [(name, ctypes.c_float) for name in ("ms_intervals", "ms_score", "ms_best", "ms_total")]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoWalkInfo(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint32) for name in ("ploidy", "n_cands", "depth", "start_of_block")] + [("n_block_reads", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoWalkStats(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in ("n_cands_in", "n_cands_out", "depth", "n_block_reads", "n_new_reads")] + \
               [("words_per_slot", ctypes.c_uint32), ("advanced", ctypes.c_uint32)] + \
               [(name, ctypes.c_float) for name in ("ms_bits", "ms_advance", "ms_total", "ms_resident")]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoNodeOrderStats(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_uint64), ("ms_first_contained", ctypes.c_float), ("ms_rank", ctypes.c_float),
                ("ms_total", ctypes.c_float)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoStats(ctypes.Structure):
    _fields_ = [
        ("bits_per_base", ctypes.c_uint32), ("kmer", ctypes.c_uint32),
        ("paired", ctypes.c_uint32), ("wide_index", ctypes.c_uint32),
        ("n_reads", ctypes.c_uint64), ("n_eligible", ctypes.c_uint64),
        ("total_bases", ctypes.c_uint64), ("shard_bases", ctypes.c_uint64),
        ("n_tiles", ctypes.c_uint64), ("n_candidates", ctypes.c_uint64),
        ("n_verified", ctypes.c_uint64), ("n_rows", ctypes.c_uint64),
        ("sum_overlap_bases", ctypes.c_uint64), ("verify_bytes_algo", ctypes.c_uint64),
        ("ms_index", ctypes.c_float), ("ms_scan_count", ctypes.c_float),
        ("ms_scan_fill", ctypes.c_float), ("ms_verify", ctypes.c_float),
        ("ms_select", ctypes.c_float), ("ms_emit", ctypes.c_float),
        ("ms_total", ctypes.c_float), ("ms_upload", ctypes.c_float),
        ("ms_scan_probe", ctypes.c_float), ("ms_verify_kernel", ctypes.c_float),
        ("verify_bytes_exec", ctypes.c_uint64), ("dp_steps", ctypes.c_uint64), ("dp_stopped", ctypes.c_uint64),
        ("max_diff", ctypes.c_uint32), ("band", ctypes.c_uint32), ("index_reused", ctypes.c_uint32),
        ("dp_lanes", ctypes.c_uint32), ("upload_bytes", ctypes.c_uint64),
        ("streamed", ctypes.c_uint32), ("n_deferred", ctypes.c_uint32),
        ("fused_tail", ctypes.c_uint32), ("tail_fallback", ctypes.c_uint32),
        ("n_predicted", ctypes.c_uint32), ("home_record_bytes", ctypes.c_uint32),
    ]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


# every symbol include/phasm_overlap.h declares: (name, restype, argtypes)
_P = ctypes.c_void_p
SYMBOLS = [
    ("po_abi_version", ctypes.c_int, []),
    ("po_create", ctypes.c_int, [ctypes.POINTER(_P)]),
    ("po_destroy", None, [_P]),
    ("po_set_device", ctypes.c_int, [_P, ctypes.c_int]),
    ("po_add_sequence", ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]),
    ("po_add_fasta", ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]),
    ("po_num_sequences", ctypes.c_uint32, [_P]),
    ("po_get_id", ctypes.c_int, [_P, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]),
    ("po_get_length", ctypes.c_uint32, [_P, ctypes.c_uint32]),
    ("po_upload", ctypes.c_int, [_P]),
    ("po_invalidate", ctypes.c_int, [_P]),
    ("po_upload_piece", ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                       ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int)]),
    ("po_upload_assemble", ctypes.c_int, [_P, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]),
    ("po_upload_piece_part", ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                            ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int)]),
    ("po_upload_assemble_parts", ctypes.c_int, [_P, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32]),
    ("po_overlaps", ctypes.c_int, [_P, ctypes.c_uint32, ctypes.POINTER(_P)]),
    ("po_overlaps_to_host", ctypes.c_int, [_P, ctypes.c_uint32, ctypes.POINTER(_P)]),
    ("po_overlaps_ex", ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_P)]),
    ("po_overlaps_shard", ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_P)]),
    ("po_candidates_shard", ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_P)]),
    ("po_expand", ctypes.c_int, [_P, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(_P)]),
    ("po_candidates_shard_into", ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                               ctypes.c_uint64, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(_P)]),
    ("po_index_slice_build", ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                            ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)]),
    ("po_index_chunk_bytes", ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    ("po_index_slice_export", ctypes.c_int, [_P, ctypes.c_void_p, ctypes.c_uint64]),
    ("po_candidates_shard_indexed", ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                                                   ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                                   ctypes.POINTER(ctypes.c_int), ctypes.POINTER(_P)]),
    ("po_overlaps_shard_indexed", ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                                                 ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(_P)]),
    ("po_shard_range", ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
    ("po_result_count", ctypes.c_uint64, [_P]),
    ("po_result_rows", ctypes.c_void_p, [_P]),
    ("po_result_rows_range", ctypes.c_void_p, [_P, ctypes.c_uint64, ctypes.c_uint64]),
    ("po_result_device_rows", ctypes.c_void_p, [_P]),
    ("po_result_copy_to_device", ctypes.c_int, [_P, ctypes.c_void_p]),
    ("po_result_copy_prefix_to_device", ctypes.c_int, [_P, ctypes.c_void_p, ctypes.c_uint64]),
    ("po_result_free", None, [_P]),
    ("po_write_gfa_edges", ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]),
    ("po_write_gfa_segments", ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]),
    ("po_add_segment", ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32]),
    ("po_result_from_rows", ctypes.c_int, [_P, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(_P)]),
    ("po_add_gfa", ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(_P)]),
    ("po_layout_edges", ctypes.c_int, [_P, _P, ctypes.POINTER(PoLayoutParams), ctypes.c_void_p, ctypes.POINTER(_P)]),
    ("po_get_layout_stats", ctypes.c_int, [_P, ctypes.POINTER(PoLayoutStats)]),
    ("po_layout_reduce", ctypes.c_int, [_P, _P, ctypes.POINTER(PoReduceParams), ctypes.c_void_p, ctypes.POINTER(_P)]),
    ("po_get_reduce_stats", ctypes.c_int, [_P, ctypes.POINTER(PoReduceStats)]),
    ("po_layout_tips", ctypes.c_int, [_P, _P, ctypes.POINTER(PoTipsParams), ctypes.c_void_p, ctypes.POINTER(_P)]),
    ("po_get_tips_stats", ctypes.c_int, [_P, ctypes.POINTER(PoTipsStats)]),
    ("po_layout_diamonds", ctypes.c_int, [_P, _P, ctypes.POINTER(PoDiamondParams), ctypes.c_void_p, ctypes.POINTER(_P)]),
    ("po_get_diamond_stats", ctypes.c_int, [_P, ctypes.POINTER(PoDiamondStats)]),
    ("po_layout_merge", ctypes.c_int, [_P, _P, ctypes.POINTER(PoMergeParams), ctypes.c_void_p, ctypes.POINTER(_P)]),
    ("po_get_merge_stats", ctypes.c_int, [_P, ctypes.POINTER(PoMergeStats)]),
    ("po_result_merged_paths", ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p,
                                              ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    ("po_layout_coverage", ctypes.c_int, [_P, _P, _P, ctypes.POINTER(PoCoverageParams), ctypes.c_void_p]),
    ("po_get_coverage_stats", ctypes.c_int, [_P, ctypes.POINTER(PoCoverageStats)]),
    ("po_layout_components", ctypes.c_int, [_P, _P, ctypes.POINTER(PoComponentsParams), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.POINTER(ctypes.c_uint64)]),
    ("po_get_components_stats", ctypes.c_int, [_P, ctypes.POINTER(PoComponentsStats)]),
    ("po_layout_partition", ctypes.c_int, [_P, _P, ctypes.POINTER(PoPartitionParams), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    ("po_get_partition_stats", ctypes.c_int, [_P, ctypes.POINTER(PoPartitionStats)]),
    ("po_layout_superbubbles", ctypes.c_int, [_P, _P, ctypes.POINTER(PoSuperbubbleParams), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    ("po_get_superbubble_stats", ctypes.c_int, [_P, ctypes.POINTER(PoSuperbubbleStats)]),
    ("po_layout_superbubbles_all", ctypes.c_int, [_P, _P, ctypes.POINTER(PoSuperbubbleAllParams), ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    ("po_get_superbubble_all_stats", ctypes.c_int, [_P, ctypes.POINTER(PoSuperbubbleAllStats)]),
    ("po_layout_bubblechains", ctypes.c_int, [_P, _P, ctypes.POINTER(PoBubblechainParams), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    ("po_get_bubblechain_stats", ctypes.c_int, [_P, ctypes.POINTER(PoBubblechainStats)]),
    ("po_layout_bubblechains_all", ctypes.c_int, [_P, _P, ctypes.POINTER(PoBubblechainParams), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    ("po_get_bubblechain_all_stats", ctypes.c_int, [_P, ctypes.POINTER(PoBubblechainAllStats)]),
    ("po_layout_contigs_all", ctypes.c_int, [_P, _P, ctypes.POINTER(PoContigParams), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    ("po_layout_contigs", ctypes.c_int, [_P, _P, ctypes.POINTER(PoContigParams), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    ("po_get_contig_stats", ctypes.c_int, [_P, ctypes.POINTER(PoContigStats)]),
    ("po_phase_branch", ctypes.c_int, [_P, ctypes.POINTER(PoPhaseParams), ctypes.POINTER(PoPhaseInput), ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    ("po_get_phase_stats", ctypes.c_int, [_P, ctypes.POINTER(PoPhaseStats)]),
    ("po_phase_index", ctypes.c_int, [_P, _P, ctypes.POINTER(_P)]),
    ("po_phase_index_copy", ctypes.c_int, [_P, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    ("po_get_phase_index_stats", ctypes.c_int, [_P, ctypes.POINTER(PoPhaseIndexStats)]),
    ("po_phase_relevant", ctypes.c_int, [_P, _P, ctypes.POINTER(PoRelevantParams), ctypes.POINTER(PoRelevantInput), ctypes.POINTER(_P)]),
    ("po_relevant_sizes", ctypes.c_int, [_P, ctypes.POINTER(PoRelevantDims)]),
    ("po_relevant_copy", ctypes.c_int, [_P] + [ctypes.c_void_p] * 8),
    ("po_get_relevant_stats", ctypes.c_int, [_P, ctypes.POINTER(PoRelevantStats)]),
    ("po_spell", ctypes.c_int, [_P, ctypes.POINTER(PoSpellInput), ctypes.POINTER(_P)]),
    ("po_spell_sizes", ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    ("po_spell_copy", ctypes.c_int, [_P, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    ("po_get_spell_stats", ctypes.c_int, [_P, ctypes.POINTER(PoSpellStats)]),
    ("po_phase_paths", ctypes.c_int, [_P, _P, ctypes.POINTER(PoPathsParams), ctypes.POINTER(_P)]),
    ("po_paths_sizes", ctypes.c_int, [_P, ctypes.POINTER(PoPathsDims)]),
    ("po_paths_copy", ctypes.c_int, [_P] + [ctypes.c_void_p] * 9),
    ("po_get_paths_stats", ctypes.c_int, [_P, ctypes.POINTER(PoPathsStats)]),
    ("po_phase_large", ctypes.c_int, [_P, _P, ctypes.POINTER(PoLargeParams), ctypes.POINTER(PoLargeInput), ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]),
    ("po_get_large_stats", ctypes.c_int, [_P, ctypes.POINTER(PoLargeStats)]),
    ("po_paths_copy_paths", ctypes.c_int, [_P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                           ctypes.POINTER(ctypes.c_uint64)]),
    ("po_walk_create", ctypes.c_int, [_P, ctypes.c_uint32, ctypes.POINTER(_P)]),
    ("po_walk_reset", ctypes.c_int, [_P]),
    ("po_walk_info_get", ctypes.c_int, [_P, ctypes.POINTER(PoWalkInfo)]),
    ("po_walk_step", ctypes.c_int, [_P, _P, ctypes.POINTER(PoPhaseParams), ctypes.POINTER(PoPhaseInput), ctypes.c_void_p, ctypes.c_uint32,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    ("po_walk_best", ctypes.c_int, [_P, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]),
    ("po_walk_history", ctypes.c_int, [_P, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    ("po_walk_read_sets", ctypes.c_int, [_P, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                         ctypes.POINTER(ctypes.c_uint64)]),
    ("po_get_walk_stats", ctypes.c_int, [_P, ctypes.POINTER(PoWalkStats)]),
    ("po_walk_relevant", ctypes.c_int, [_P, _P, _P, ctypes.POINTER(PoWalkRelevantParams), ctypes.POINTER(PoRelevantInput), ctypes.POINTER(_P)]),
    ("po_walk_step_resident", ctypes.c_int, [_P, _P, _P, ctypes.POINTER(PoPhaseParams), ctypes.POINTER(PoPhaseInput), ctypes.c_uint32,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    ("po_walk_prev_copy", ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    ("po_graph_from_edges", ctypes.c_int, [_P, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(_P)]),
    ("po_result_node_order", ctypes.c_int, [_P, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    ("po_get_node_order_stats", ctypes.c_int, [_P, ctypes.POINTER(PoNodeOrderStats)]),
    ("po_get_stats", ctypes.c_int, [_P, ctypes.POINTER(PoStats)]),
    ("po_last_error", ctypes.c_char_p, [_P]),
    ("po_debug_fault_backtrace", ctypes.c_int, [ctypes.c_int]),
    ("po_debug_store_words", ctypes.c_uint64, [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    ("po_debug_expand_packed", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                                              ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64]),
    ("po_debug_expand_records", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                               ctypes.c_void_p, ctypes.c_uint64]),
    ("po_debug_host_ranges", ctypes.c_uint64, [ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint64]),
    ("po_debug_pointer_info", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                             ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
]

_lib = None


def _preload_torch_hip_runtime() -> None:
    """One HIP runtime per process.  PyTorch wheels bundle their own ``libamdhip64.so`` (SONAME
    ``libamdhip64.so.7``) and link to it by its unversioned file name, so a process that loads this
    library first (bound to /opt/rocm's copy) and torch afterwards ends up with two runtimes, and the second
    one finds no device.  Loading torch's copy first -- by path, without importing torch -- makes both bind
    to the same one, whatever the import order."""
    import importlib.util
    if os.environ.get("PHASM_HIP_RUNTIME") == "system":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(path):
        try:
            ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def load() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _preload_torch_hip_runtime()
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s not found: build it with `python -m phasm_amd.build` (hipcc, gfx950). "
                "phasm_amd has no CPU fallback." % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, restype, argtypes in SYMBOLS:
            fn = getattr(lib, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = lib
    return _lib
