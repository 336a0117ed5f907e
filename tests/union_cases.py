"""The small cases that tests/test_union_rules.py (CPU) and tests/test_gpu_union_scale.py (device) replicate: drawn from the
generators and direct inputs the stage utils already have, structurally different, and small -- the chain stages launch per
level or round, so nothing here has more than a few dozen levels."""
import numpy as np

import bubblechain_utils as bcu
import contig_utils as ctu
import coverage_utils as cu
import merge_utils as mu
import reduce_utils as ru
import tips_utils as tu

MIN_CONTIG_LEN = 60


def alternating(n_cases, per_case):
    """The case of every copy: A, B, C, A, B, C, ... with ``per_case`` copies of each."""
    return list(range(n_cases)) * per_case


def row_cases():
    """(names, segment lengths, rows): tips on tips and diamonds; self-loops, own-twin edges and 2-cycles; every tip length
    at both bounds; transitive edges and rows written one way only; a ring with a tail; rows one strand only, duplicates,
    contained reads and overhangs; segments of length 0."""
    return [tu.tangle_case(3), tu.selfish_case(2), tu.comb_case(), ru.line_case(1), mu.lasso_case(20, 6), cu.mix_case(1), cu.zero_case(1)]


GRAPH_NAMES = ("sb_nesting_depth_3", "sb_self_loop_inside_nesting_depth_3", "sb_nested_with_the_outer_one_discarded",
               "sb_two_diamonds_sharing_a_node", "sb_out_edge_into_a_cycle", "sb_in_edge_from_a_cycle", "sb_path_17_scrambled",
               "sb_branches_1_2_5", "sb_self_loop_on_the_exit", "bc_two_chains_heads_descending", "bc_head_with_and_without_in_edges",
               "bc_diamond_edge_diamond_fork", "bc_nesting_depth_3_inside_a_chain_member", "nodes_without_edges", "two_cycle")


def _weighted(uv, seed):
    return [(u, v, w, 50 + (7 * i) % 40) for i, (u, v, w) in enumerate(ctu._weights(uv, seed))]


def graph_cases():
    """(order, edges (u, v, weight, overlap_len)) for the stages that take any graph: nesting, discarded bubbles, chains of
    several bubbles, cycles beside bubbles, self-loops, a scrambled path, nodes without edges."""
    by_name = {c[0]: c for c in bcu.direct_inputs()}
    return [([int(x) for x in by_name[n][1]], _weighted(by_name[n][2], i)) for i, n in enumerate(GRAPH_NAMES)]


CONTIG_NAMES = ("lasso", "ring_with_a_spur_out", "blocked_root_start_with_a_tree_behind", "blocked_late_start_beside_an_open_sibling",
                "path_through_a_stretch_of_excluded_nodes", "every_node_excluded", "self_loop_as_head_edge", "self_loop_on_an_in_degree_1_node",
                "two_cycle_entered_from_outside", "isolated_nodes_at_and_below_the_minimum", "ring_40")


def contig_cases():
    """(order, edges (u, v, weight, overlap_len), {node: length}, excluded nodes): late starts, blocked starts, rings, self-loops,
    isolated nodes on both sides of MIN_CONTIG_LEN."""
    by_name = {c[0]: c for c in ctu.direct_inputs()}
    return [(by_name[n][1], [(u, v, w, 77) for u, v, w in by_name[n][2]], by_name[n][3], by_name[n][4]) for n in CONTIG_NAMES]


def contig_union_inputs(U, cases, nseq):
    """(length, excluded) per node of the union's order."""
    lengths = U.gather([[c[2][n] for n in c[0]] for c in cases], *nseq)
    exclude = U.gather([[int(n in set(c[3])) for n in c[0]] for c in cases], *nseq)
    return lengths, exclude


def segment_lengths(U, cases, default=1000):
    """One length per segment of a graph union (segment i of copy c is base[c] / 2 + i): the case's own where it names one."""
    per_case = []
    for k, c in enumerate(cases):
        l = np.full(int(U.n_ids[k]) // 2, default, dtype=np.int64)
        if len(c) > 2:
            for n, x in c[2].items():
                l[n >> 1] = x
        per_case.append(l)
    return np.concatenate([per_case[k] for k in U.case_of.tolist()]) if U.R else np.zeros(0, np.int64)
