"""``phasm overlap`` on the MI355X path.

Counterpart of ``overlap(args)`` in the reference CLI (/root/reference/phasm/cli/assembler.py:29-50,
parser at :436-452): same positional FASTA argument, ``-l/--min-length`` (default 1000),
``-o/--output`` (default stdout), and byte-identical ``H`` / ``S`` / ``E`` lines for identical
rows -- all ``S`` lines first, then the ``E`` lines.  Row order differs from the reference
(whose order is an artefact of ``std::unordered_map`` iteration, overlapper.cpp:30,:68) and is
not specified here either: the ``E`` lines come in the order the device emits the rows, which
depends on the path a call takes (strand-paired 2-bit reads, 8-bit reads, pieces).

    python -m phasm_amd.cli overlap reads.fasta -l 1000 -o overlaps.gfa

``layout-edges`` is the first stage of ``phasm layout`` (assembler.py:52-139, options :469-489) on the
same device: read the overlap file, classify and filter the alignments, drop contained reads, and
write the assembly graph as it stands before graph cleaning, in the reference's own graph format
(``gfa2_write_graph``, phasm/io/gfa.py:283-327: one ``S`` line per read that still has an edge, one
``E * u v weight len(u) 0 overlap_len *`` line per edge).

    python -m phasm_amd.cli layout-edges overlaps.gfa -o graph.gfa

``daligner2gfa`` is the other producer of the overlap file (``phasm-convert daligner2gfa``,
/root/reference/phasm/cli/convert.py:65-133, options :146-183): DBdump + LAdump text in, the same GFA2 lines out.
``layout-edges --las`` takes the two dumps directly and skips the text in between.

    python -m phasm_amd.cli daligner2gfa -o overlaps.gfa reads.dbdump alignments.ladump
    python -m phasm_amd.cli layout-edges reads.dbdump --las alignments.ladump -o graph.gfa
"""
from __future__ import annotations

import argparse
import logging
import sys
from typing import Optional

import numpy as np

from .io import daligner, gfa
from .io.fasta import read_fasta, reverse_complement
from .overlapper import ExactOverlapper
from . import layout as layout_mod

logger = logging.getLogger("phasm_amd")


def _seconds_since_process_start() -> float:
    """Wall time since the kernel started this process (interpreter start and imports included), from /proc."""
    import os
    try:
        with open("/proc/self/stat") as f:
            start_ticks = int(f.read().rsplit(")", 1)[1].split()[19])
        with open("/proc/uptime") as f:
            up = float(f.read().split()[0])
        return up - start_ticks / os.sysconf("SC_CLK_TCK")
    except (OSError, ValueError, IndexError):
        return float("nan")


def overlap(args) -> int:
    import time
    marks = [("process start -> overlap() entered (interpreter, imports)", _seconds_since_process_start())]
    t_prev = [time.perf_counter()]

    def mark(what):
        now = time.perf_counter()
        marks.append((what, now - t_prev[0]))
        t_prev[0] = now

    args.output.write(gfa.gfa_header())
    overlapper = ExactOverlapper(device=getattr(args, "device", None))
    mark("library loaded, handle made")
    logger.info("Packing reads and searching for pairwise overlaps on the GPU...")
    if isinstance(args.fasta_input, (str, bytes)) and not getattr(args, "python_ingest", False):
        # native parse + reverse complement + 2-bit pack in one pass (po_add_fasta)
        overlapper.add_fasta(args.fasta_input, both_strands=True)
        mark("FASTA parsed, reverse-complemented, packed (the device comes up beside it)")
        try:
            args.output.fileno()
            overlapper.write_gfa_segments(args.output)       # S lines formatted in C, straight to the descriptor
        except (AttributeError, OSError, ValueError):
            ids, lens = overlapper.ids(), overlapper.lengths()
            for i in range(0, len(ids), 2):
                args.output.write(gfa.gfa_line("S", ids[i][:-1], int(lens[i]), "*"))
    else:
        for name, seq in read_fasta(args.fasta_input):
            args.output.write(gfa.gfa_line("S", name, len(seq), "*"))
            overlapper.add_sequence(name + "+", seq)
            overlapper.add_sequence(name + "-", reverse_complement(seq))
    mark("S lines")
    max_diff = int(getattr(args, "max_diff", 0) or 0)
    if max_diff > 0:
        # beyond the reference (which is exact, assembler.py:436-439): banded seed-extension DP, po_overlaps_ex
        res = overlapper.overlaps_ex_result(args.min_length, max_diff, int(getattr(args, "band", 0) or 0))
    else:
        res = overlapper.overlaps_to_host_result(args.min_length)   # rows travel to the host while later chunks are computed
    mark("the overlap call (upload, kernels, rows home)")
    logger.info("Writing %d overlaps to GFA2...", len(res))
    try:
        try:
            args.output.fileno()
            native = True
        except (AttributeError, OSError, ValueError):
            native = False
        if native:
            n = res.write_gfa_edges(args.output)       # formatted in C, straight to the descriptor
        else:
            n = gfa.write_edges(args.output, res.rows(), overlapper.ids())
    finally:
        res.free()
    mark("E lines formatted and written")
    args.output.flush()
    if not getattr(args, "leave_handle_to_exit", False):
        overlapper.close()
    mark("flush + handle closed")
    if getattr(args, "timing", False):
        import json
        sys.stderr.write("PHASM_CLI_TIMING " + json.dumps({k: round(v, 4) for k, v in marks}) + "\n")
    logger.info("Done.")
    return n


def write_stage1_graph(out, ids, lengths, edges_arr, edges_res=None) -> int:
    """The graph after stage 1 in the format of gfa2_write_graph (phasm/io/gfa.py:283-327): S lines of the reads
    that still have an edge, then one ``E * u v weight len(u) 0 overlap_len *`` line per edge (written natively
    from the device result when ``out`` is a real file)."""
    import numpy as np
    out.write(gfa.gfa_header())
    e = edges_arr
    used = np.zeros(len(ids) // 2, dtype=bool)
    used[e["u"] >> 1] = True
    used[e["v"] >> 1] = True
    for i in np.flatnonzero(used).tolist():
        out.write(gfa.gfa_line("S", ids[2 * i][:-1], int(lengths[2 * i]), "*"))
    if edges_res is not None:
        try:
            out.fileno()
            return edges_res.write_gfa_edges(out)
        except (AttributeError, OSError, ValueError):
            pass
    lu = np.asarray(lengths)[e["u"]]
    chunk = 1 << 18
    for lo in range(0, len(e), chunk):
        sl = slice(lo, lo + chunk)
        out.write("".join("E\t*\t%s\t%s\t%d\t%d\t0\t%d\t*\n" % t for t in
                          zip([ids[u] for u in e["u"][sl].tolist()], [ids[v] for v in e["v"][sl].tolist()],
                              e["weight"][sl].tolist(), lu[sl].tolist(), e["overlap_len"][sl].tolist())))
    return len(e)


def _load_translations(path):
    """-T of daligner2gfa (convert.py:69-76): a JSON object {dump id: name}; a missing file is ignored with a
    warning (the reference's warning line itself fails on an undefined attribute, :75-76)."""
    import json
    import os
    if not path:
        return None
    if not os.path.isfile(path):
        logger.warning("Translations file '%s' does not exist, ignoring.", path)
        return None
    with open(path) as f:
        return json.load(f)


def daligner2gfa(args) -> int:
    las = sys.stdin if args.las_input in (None, "-") else open(args.las_input)
    try:
        with open(args.db_input) as db:
            n_s, n_e = daligner.write_gfa(args.out, db, las, args.with_sequences, args.with_trace_points,
                                          _load_translations(args.translations))
    finally:
        if las is not sys.stdin:
            las.close()
    logger.info("Wrote %d reads and %d local alignments.", n_s, n_e)
    return n_e


def _int_in(lo: int, hi: int):
    """argparse type: an integer in [lo, hi] (what the library's 32-bit parameters hold)."""
    def parse(text: str) -> int:
        try:
            value = int(text)
        except ValueError:
            raise argparse.ArgumentTypeError("%r is not an integer" % text)
        if not lo <= value <= hi:
            raise argparse.ArgumentTypeError("%d is not in [%d, %d]" % (value, lo, hi))
        return value
    return parse


def _write_coverage(graphml, g) -> None:
    """The log line of the coverage and, with --graphml, the file (assembler.py:208-209)."""
    if g.coverage_stats is None:
        return
    cs = g.coverage_stats
    logger.info("Average coverage of %d edges from %d (node, aligning read) pairs; largest set %d reads.",
                cs["n_edges"], cs["n_pairs"], cs["max_set"])
    if graphml is not None:
        layout_mod.write_graphml(graphml, g)


def layout_edges(args) -> int:
    ov = ExactOverlapper(device=getattr(args, "device", None))
    try:
        if getattr(args, "las", None):
            with open(args.gfa_file) as db, open(args.las) as las:
                rows = layout_mod.load_daligner(ov, db, las, _load_translations(getattr(args, "translations", None)))
            nseg = len(ov) // 2
        else:
            nseg, rows = ov.add_gfa(args.gfa_file)
        logger.info("Read %d reads and %d local alignments from the GFA2 file.", nseg, len(rows))
        graphml = getattr(args, "graphml", None)
        coverage = getattr(args, "coverage", False) or graphml is not None
        try:
            edges, _removed = ov.layout_edges(rows, args.min_read_length, args.min_overlap_length,
                                              args.max_overhang_abs, args.max_overhang_rel)
        finally:
            if not coverage:
                rows.free()   # (the coverage reads every row again: with it they live until it is done)
        st = ov.layout_stats()
        logger.info("%d contained reads removed; %d alignments pass the filters; graph has %d edges.",
                    st["n_contained_reads"], st["n_pass"], st["n_edges"])
        try:
            merge = getattr(args, "merge", False)
            clean = getattr(args, "clean", False) or merge
            if clean or getattr(args, "transitive_reduction", False):
                # assembler.py:145-159: remove_transitive_edges, remove_edges_from, make_symmetric
                kept = ov.layout_reduce(edges, args.length_fuzz)
                edges.free()
                edges = kept
                rs = ov.reduce_stats()
                logger.info("Removing %d transitive edges...", rs["n_transitive"])
                logger.info("Removed %d asymmetric edges; graph has %d edges.", rs["n_asymmetric"], rs["n_edges_out"])
            if clean or getattr(args, "remove_tips", False):
                # assembler.py:161-171: remove_tips, make_symmetric, clean_graph
                # (one device call does all three, so the reference's two progress lines come before it)
                logger.info("Removing tips...")
                logger.info("Removing isolated nodes...")
                kept = ov.layout_tips(edges, args.max_tip_length, args.max_tip_length_bases)
                edges.free()
                edges = kept
                ts = ov.tips_stats()
                logger.info("Removed %d tip edges, %d isolated nodes, %d asymmetric edges.",
                            ts["n_in_tip_edges"] + ts["n_out_tip_edges"], ts["n_isolated_nodes"], ts["n_asymmetric"])
            if clean or getattr(args, "remove_diamond_tips", False):
                # assembler.py:173-174: remove_diamond_tips (no symmetry pass, no clean_graph)
                kept = ov.layout_diamonds(edges)
                edges.free()
                edges = kept
                logger.info("Removed %d diamond tips", ov.diamond_stats()["n_diamonds"])
            if clean:
                # assembler.py:176-182: remove_tips(g, max_tip_length) -- the base bound is the function's default --,
                # make_symmetric, clean_graph; the counts are this block's own
                logger.info("Removing tips (stage 2)...")
                kept = ov.layout_tips(edges, args.max_tip_length, 5000)
                edges.free()
                edges = kept
                ts = ov.tips_stats()
                logger.info("Removed %d tip edges, %d isolated nodes, %d asymmetric edges.",
                            ts["n_in_tip_edges"] + ts["n_out_tip_edges"], ts["n_isolated_nodes"], ts["n_asymmetric"])
            if merge:
                # assembler.py:184-186 and the file of :195-212 (gfa2_write_graph): S lines in node order, F lines behind
                # a merged node's S line, E lines in the result's own order
                logger.info("Merging unambiguous paths...")
                if coverage:   # assembler.py:190-193, on the merged graph while it is still on the device
                    logger.info("Calculating average coverage for each edge...")
                g = layout_mod.merge_unambiguous_paths(ov, edges, coverage_rows=rows if coverage else None)
                logger.info("Merged %d nodes.", g.merge_stats["n_nodes_merged"])
                _write_coverage(graphml, g)
                return layout_mod.write_merged_graph(args.output, g)
            if coverage:
                logger.info("Calculating average coverage for each edge...")
                g = layout_mod.AssemblyEdges(edges.rows(), None, ov.ids(), st)
                _write_coverage(graphml, layout_mod._coverage_into(g, ov, edges, rows))
            return write_stage1_graph(args.output, ov.ids(), ov.lengths(), edges.rows(), edges)
        finally:
            edges.free()
            if coverage:
                rows.free()
    finally:
        ov.close()


def chain_components(args) -> int:
    """The start of `phasm chain` (assembler.py:231-310): the graph file's weakly connected components, one file each."""
    from . import layout
    allowed, formats = {"gfa1", "gfa2", "graphml"}, []
    for file_format in args.format.split(","):
        file_format = file_format.strip()
        if file_format in allowed:
            formats.append(file_format)
        else:
            logger.warning("File format '%s' not recognised, ignoring.", file_format)
    if not formats:
        logger.critical("No valid file formats specified.")
        sys.exit(1)
    logger.info("Reconstructing assembly graph...")
    contigs = getattr(args, "contigs", False)
    g = layout.chain_components(args.graph_gfa, device=args.device, partitions=args.partitions, superbubbles=args.superbubbles,
                                bubblechains=args.bubblechains or contigs, min_nodes=args.min_nodes, contigs=contigs,
                                min_length=args.min_length, cyclic=getattr(args, "cyclic", False))
    logger.info("Enumerate weakly connected components in the graph...")
    n = layout.write_component_graphs(args.output_dir, g, formats)
    for parts in g.partitions or ():
        for part in parts:   # (find_superbubbles, phasm/bubbles.py:402-409, logs this line per partition)
            logger.info("Partition with %d nodes with in-degree 0, %d nodes with out-degree 0, acyclic: %s", part.num_sources,
                        part.num_sinks, part.acyclic)
    if g.superbubbles is not None:
        import numpy as np
        entrances = g.superbubbles.table["entrance"].astype(np.int64)
        comp_of = np.zeros(int(g.components.node_order.max()) + 1 if len(g.components.node_order) else 0, dtype=np.int64)
        comp_of[g.components.node_order] = g.components.component_of_node
        per = np.bincount(comp_of[entrances], minlength=len(g.components))
        top = np.bincount(comp_of[entrances[g.superbubbles.table["nested"] == 0]], minlength=len(g.components))
        for i in range(len(g.components)):
            logger.info("Connected component %d: %d superbubbles in its acyclic partition, %d of them not nested.", i, per[i], top[i])
        if g.superbubbles_all is not None:   # (a superbubble lies in one partition: those the acyclic call lacks lie in an SCC)
            every = g.superbubbles_all.table["entrance"].astype(np.int64)
            per_all = np.bincount(comp_of[every], minlength=len(g.components))
            for i in range(len(g.components)):
                logger.info("Connected component %d: %d superbubbles in all its partitions, %d of them in non-singleton SCCs.", i,
                            per_all[i], per_all[i] - per[i])
    if getattr(args, "as_chain", False):   # (the last line of `phasm chain`, assembler.py:308-310)
        logger.info("Built %d bubblechains and %d contigs from %d weakly connected components.",
                    sum(len(x) for x in g.component_chains), sum(len(x) for x in g.component_contigs), n)
    else:
        logger.info("Wrote %d weakly connected components.", n)
    return 0


def bubble_paths_lines(graph, paths, max_bubble_size: int, listing: bool):
    """The lines of ``bubble-paths``: one per top-level bubble -- chain, position, entrance, exit, interior nodes, paths, and
    the arm ``phase()`` would take (``bare``: the walk of the chain ends here; ``large``: more than ``max_bubble_size`` paths,
    ``phase_large_bubble``; ``branch``) --, with ``listing`` behind each listed bubble its paths by segment name."""
    from .phasing import paths_text
    yield "#chain\tposition\tentrance\texit\tinterior_nodes\tpaths\tarm\n"
    for b in range(len(paths)):
        row = paths.bubbles[b]
        arm = "bare" if paths.is_bare(b) else "large" if paths.is_large(b, max_bubble_size) else "branch"
        yield "%d\t%d\t%s\t%s\t%d\t%s\t%s\n" % (row["chain"], row["position"], graph.node_name(int(row["entrance"])),
                                               graph.node_name(int(row["exit"])), row["n_inside"], paths_text(row["n_paths"]), arm)
        if listing and paths.is_listed(b):
            for j, p in enumerate(paths.paths_of(b)):
                yield "P\t%d\t%d\t%d\t%s\n" % (row["chain"], row["position"], j, ",".join(graph.node_name(n) for n in p))


def bubble_paths(args) -> int:
    """What ``BubbleChainPhaser.phase()`` computes per bubble before it looks at a read, for every top-level bubble of a graph
    file in one device call: the paths are counted there, and listed only with --list and only up to MAX_BUBBLE_SIZE."""
    from . import layout
    graph, paths, stats = layout.graph_file_bubble_paths(args.graph_gfa, args.max_bubble_size if args.list else 0, device=args.device)
    logger.info("%d top-level bubbles (%d bare, %d with more than %d paths); %d paths listed; %.3f ms on the device.", stats["n_bubbles"],
                stats["n_bare"], sum(paths.is_large(b, args.max_bubble_size) for b in range(len(paths))), args.max_bubble_size,
                stats["n_listed_paths"], stats["ms_total"])
    args.output.writelines(bubble_paths_lines(graph, paths, args.max_bubble_size, args.list))
    return len(paths)


def spell_contigs(args) -> int:
    """Per graph file one FASTA entry, named after the file: what the no-bubble branch of the reference's ``phase`` writes
    (phasm/cli/assembler.py:368-383).  The reads go on the handle once, all files are spelled in one device call."""
    from . import spelling
    graphs = []
    for path in args.graph_gfa:
        with open(path) as f:
            graphs.append((path, gfa.read_graph_gfa(f)))
    overlapper = ExactOverlapper(device=getattr(args, "device", None))
    overlapper.add_fasta(args.fasta_input, both_strands=True)
    reads_of = spelling.ReadMap.of(overlapper)
    piece_lists = []
    for path, gf in graphs:
        try:
            piece_lists.append(spelling.contig_pieces(gf, reads_of))
        except (ValueError, KeyError) as e:
            raise SystemExit("%s: %s (a graph with bubbles needs `phase`)" % (path, e.args[0] if e.args else e))
    logger.info("Spelling %d contigs of %d pieces on the GPU...", len(piece_lists), sum(map(len, piece_lists)))
    seqs = spelling.spell_pieces(overlapper, piece_lists)
    for (path, _), seq in zip(graphs, seqs):
        args.output.write(b">" + spelling.contig_name(path).encode("utf-8") + b"\n" + seq + b"\n")
    args.output.flush()
    overlapper.close()
    return len(seqs)


class PhasingError(Exception):
    """What the reference's ``BubbleChainPhaser`` raises for a graph it cannot start on (phasm/phasing.py:172-192)."""


def phase_chain_of(gf, paths) -> Optional[int]:
    """The chain ``phase()`` walks on graph file ``gf`` with the bubbles ``paths`` (a ``phasing.BubblePaths``): None when no
    top-level bubble has an interior (the no-bubble branch); else the chain whose first entrance is the one node of
    in-degree 0 -- anything else is a ``PhasingError`` with the reference's sentence."""
    if all(paths.is_bare(b) for b in range(len(paths))):
        return None
    heads = {int(v) for v in gf.edges[:, 1].tolist()}
    starts = [int(n) for n in gf.node_order if int(n) not in heads]
    if len(starts) > 1:
        raise PhasingError("There are multiple nodes with in-degree 0, not sure what the start point is.")
    table = paths.bubbles
    first = [b for b in range(len(paths)) if starts and int(table["position"][b]) == 0 and int(table["entrance"][b]) == starts[0]
             and not paths.is_bare(b)]
    if not first:
        raise PhasingError("Unexpected starting point '%s', this is not a bubble entrance" % (gf.node_name(starts[0]) if starts else None))
    return int(table["chain"][first[0]])


def phase_entries(base: str, blocks):
    """``(name, node path, include_last)`` of every FASTA entry of a phased subgraph: ``{base}.haploblock{i}.{j}`` for every
    haplotype of block i, ``{base}.largebubble{i}`` for the first haplotype of a large bubble's block alone."""
    for i, block in enumerate(blocks):
        for j, haplotype in enumerate(block.haplotypes):
            if block.from_large_bubble:
                yield "%s.largebubble%d" % (base, i), haplotype, block.include_last
                break
            yield "%s.haploblock%d.%d" % (base, i, j), haplotype, block.include_last


HOST_PATHS = 64                  # a bubble of up to this many paths comes to the host: what the branch arm can score in one call
MAX_LISTED_PATHS = 1 << 20       # --max-listed-paths: the paths of a larger bubble are not listed at all


def _subgraph_bubble_paths(path, device, max_listed=MAX_LISTED_PATHS):
    """(graph file, DevicePaths) of a subgraph, to be closed: every bubble of up to ``max_listed`` paths is listed and stays on
    the device; the walk fetches the paths of the bubbles of up to 64 paths and scores the larger ones where they are."""
    from . import layout
    graph, paths, _ = layout.graph_file_device_paths(path, max(int(max_listed), HOST_PATHS), device=device)
    return graph, paths


def phase(args) -> int:
    """`phasm phase` (phasm/cli/assembler.py:331-418): per subgraph either the one contig of a graph without bubbles, or the
    haploblocks of its bubble chain -- the walk of ``phasing.phase_chain`` with the candidate sets resident on the device.
    The reads go on the handle once; the alignments are indexed there once, when the first subgraph with bubbles needs them;
    all sequences of a subgraph are spelled in one device call.  The paths of a subgraph's bubbles stay on the device
    (``--max-listed-paths`` caps what is listed): those of a bubble of up to 64 paths come home for the branch arm, a larger
    bubble is scored where its paths are (``po_phase_large``) and only the winner comes home.  The walk takes the resident
    route: the previous sets and the relevant reads of a bubble stay on the device between the gather and
    the step; ``--host-sets`` takes the route through host lists and arrays, with the same output."""
    import random
    from . import phasing, spelling
    if not 1 <= args.ploidy <= 8:
        raise SystemExit("phase: the ploidy must be 1 to 8")
    choose = random.Random(args.seed).choice
    overlapper = ExactOverlapper(device=args.device)
    overlapper.add_fasta(args.reads_fasta, both_strands=True)
    reads_of = spelling.ReadMap.of(overlapper)
    index, n_entries = None, 0
    max_listed = int(getattr(args, "max_listed_paths", MAX_LISTED_PATHS))
    for path in args.subgraphs:
        try:
            gf, paths = _subgraph_bubble_paths(path, args.device, **({} if max_listed == MAX_LISTED_PATHS else {"max_listed": max_listed}))
        except OverflowError as e:
            raise SystemExit("%s: %s (lower --max-listed-paths)" % (path, e))
        try:
            base = spelling.contig_name(path)
            try:
                chain = phase_chain_of(gf, paths)
            except PhasingError as e:
                raise SystemExit("%s: %s" % (path, e))
            if chain is None:
                logger.info("%s: no bubbles, a simple contig path of %d nodes.", path, len(gf.node_order))
                names, pieces = [base], [spelling.contig_pieces(gf, reads_of)]
            else:
                if index is None:
                    with open(args.alignments_gfa) as f:
                        seg_names, _, rows = gfa.read_gfa2_rows(f)
                    to_read = np.asarray([reads_of[name + sign] for name in seg_names for sign in "+-"], dtype=np.int64)
                    if len(rows):
                        rows[:, 0], rows[:, 1] = to_read[rows[:, 0]], to_read[rows[:, 1]]
                    res = overlapper.result_from_rows(rows)
                    index = overlapper.phase_index(res)
                    res.free()

                def node_reads(n, gf=gf):
                    seg = int(n) >> 1
                    return [reads_of[r] for r in gf.fragments[seg][0]] if seg in gf.fragments else [reads_of[gf.node_name(n)]]

                for b in paths.chain_bubbles(chain):
                    if not paths.is_listed(b) and int(paths.bubbles["n_paths"][b]) > max(max_listed, HOST_PATHS):
                        raise SystemExit("%s: bubble %d has %s paths, more than --max-listed-paths %d: they were not listed" %
                                         (path, b, phasing.paths_text(paths.bubbles["n_paths"][b]), max_listed))
                try:
                    bubbles = phasing.chain_bubbles_input(paths, chain, node_reads, is_merged=lambda n, gf=gf: (int(n) >> 1) in gf.fragments,
                                                          **({"resident_above": HOST_PATHS} if hasattr(paths, "score_large") else {}))
                except ValueError as e:
                    raise SystemExit("%s: %s" % (path, e))
                for i, b in enumerate(bubbles):
                    if b.get("paths") is None and b["n_paths"] <= args.max_bubble_size:
                        raise SystemExit("%s: bubble %d (%s .. %s) has %d paths: more than the 64 the branch arm takes, and no large bubble "
                                         "with --max-bubble-size %d" % (path, i, gf.node_name(b["entrance"]), gf.node_name(b["exit"]),
                                                                        b["n_paths"], args.max_bubble_size))
                logger.info("%s: a bubble chain of %d bubbles, ploidy %d.", path, len(bubbles), args.ploidy)
                walk = overlapper.phase_walk(args.ploidy)
                try:
                    blocks = list(phasing.phase_chain(overlapper, overlapper, index, bubbles, node_reads, args.ploidy, args.min_spanning_reads,
                                                      args.max_bubble_size, args.threshold, args.prune_factor, args.max_candidates,
                                                      args.max_prune_rounds, args.prune_step_size, walk=walk, choose=choose,
                                                      resident=not getattr(args, "host_sets", False)))
                finally:
                    walk.close()
                entries = list(phase_entries(base, blocks))
                names = [e[0] for e in entries]
                pieces = [spelling.path_pieces(gf, nodes, reads_of, include_last) for _, nodes, include_last in entries]
        finally:
            if hasattr(paths, "close"):
                paths.close()
        for name, seq in zip(names, spelling.spell_pieces(overlapper, pieces)):
            args.output.write(b">" + name.encode("utf-8") + b"\n" + seq + b"\n")
        n_entries += len(names)
    args.output.flush()
    if index is not None:
        index.free()
    overlapper.close()
    return n_entries


def main(argv=None) -> int:
    parser = argparse.ArgumentParser(prog="phasm-amd", description="MI355X-native PHASM overlap step")
    parser.add_argument("-v", "--verbose", action="count", default=0)
    sub = parser.add_subparsers(dest="command")
    p = sub.add_parser("overlap", help="Find pairwise exact overlaps between reads in a FASTA file.")
    p.add_argument("-l", "--min-length", type=int, default=1000,
                   help="Minimum overlap length (default: 1000)")
    p.add_argument("-o", "--output", type=argparse.FileType("w"), default=sys.stdout,
                   help="Output file (default: stdout)")
    p.add_argument("--device", type=int, default=None, help="HIP device ordinal (default 0)")
    p.add_argument("--python-ingest", action="store_true", help="parse the FASTA in Python instead of po_add_fasta")
    p.add_argument("--timing", action="store_true", help="print the command's stage times as one JSON line on stderr")
    p.add_argument("--leave-handle-to-exit", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("--max-diff", type=int, default=0,
                   help="(extension beyond the exact reference) accept overlaps with up to this many differences: banded "
                        "seed-extension DP on the GPU; 0 = exact, the reference's behaviour (default)")
    p.add_argument("--band", type=int, default=8, help="with --max-diff: diagonals each side of the anchor's diagonal (<= 30; default 8)")
    p.add_argument("fasta_input", help="FASTA file with reads")
    p.set_defaults(func=overlap)
    # option names and defaults of `phasm layout`, assembler.py:469-489
    q = sub.add_parser("layout-edges", help="Stage 1 of `phasm layout`: filter the alignments of an overlap file and "
                                            "write the assembly graph before graph cleaning.")
    q.add_argument("-l", "--min-read-length", type=int, default=0)
    q.add_argument("-s", "--min-overlap-length", type=int, default=0)
    q.add_argument("-a", "--max-overhang-abs", type=int, default=1000)
    q.add_argument("-r", "--max-overhang-rel", type=float, default=0.8)
    q.add_argument("-o", "--output", type=argparse.FileType("w"), default=sys.stdout)
    q.add_argument("--transitive-reduction", action="store_true",
                   help="also remove the transitive edges and make the graph symmetric (the first two operations of "
                        "graph cleaning, `phasm layout` stage 2) before writing it")
    q.add_argument("-F", "--length-fuzz", type=int, default=1000,
                   help="with --transitive-reduction: length fuzz of the transitive reduction (default: 1000)")
    q.add_argument("--remove-tips", action="store_true",
                   help="also remove short tips, make the graph symmetric and drop the isolated nodes (the next three "
                        "operations of graph cleaning; after the transitive reduction when both are given)")
    q.add_argument("-t", "--max-tip-length", type=_int_in(0, 2**32 - 1), default=4,
                   help="with --remove-tips: maximum number of edges of a tip (default: 4)")
    q.add_argument("--max-tip-length-bases", type=_int_in(-2**31, 2**31 - 1), default=5000,
                   help="with --remove-tips: maximum length of a tip in bases (default: 5000)")
    q.add_argument("--remove-diamond-tips", action="store_true",
                   help="also remove the diamond tips (the call between the two tip blocks of graph cleaning; after "
                        "--remove-tips when both are given)")
    q.add_argument("--clean", action="store_true",
                   help="graph cleaning as `phasm layout` runs it up to the merging of paths: transitive reduction, tips, "
                        "diamond tips, tips again; -F, -t and --max-tip-length-bases apply (the last to the first tip "
                        "block only, as in the reference)")
    q.add_argument("--merge", action="store_true",
                   help="graph cleaning as --clean, then merge the unambiguous paths and write the graph file of `phasm "
                        "layout`: S lines in node order, F lines for the reads of every merged node, E lines")
    q.add_argument("--coverage", action="store_true",
                   help="also calculate the average coverage of every edge of the graph the command ends with (the last "
                        "computation of `phasm layout` before it writes the graph), from every alignment of the input")
    q.add_argument("--graphml", type=argparse.FileType("w"), default=None, metavar="FILE",
                   help="also write the graph as GraphML with the edge attributes weight, overlap_len and avg_coverage "
                        "(implies --coverage)")
    q.add_argument("--device", type=int, default=None)
    q.add_argument("--las", default=None, metavar="LADUMP",
                   help="read the positional file as DBdump text and the alignments from this LAdump text")
    q.add_argument("-T", "--translations", default=None, help="with --las: JSON map of dump ids to read names")
    q.add_argument("gfa_file", help="GFA2 file with the reads (S lines) and their pairwise alignments (E lines)")
    q.set_defaults(func=layout_edges)
    # option names of `phasm-convert daligner2gfa`, convert.py:146-183
    c = sub.add_parser("daligner2gfa", help="Convert DAZZ_DB DBdump and DALIGNER LAdump text to a GFA2 overlap file.")
    c.add_argument("-s", "--with-sequences", action="store_true", default=False)
    c.add_argument("-t", "--with-trace-points", type=int, default=None, metavar="SPACING")
    c.add_argument("-T", "--translations", type=str, default=None, metavar="TRANSLATION_FILE")
    c.add_argument("-o", "--out", type=argparse.FileType("w"), default=sys.stdout)
    c.add_argument("db_input", help="DBdump text")
    c.add_argument("las_input", nargs="?", default=None, help="LAdump text (default: stdin)")
    c.set_defaults(func=daligner2gfa)
    # option names of `phasm chain`, assembler.py
    k = sub.add_parser("chain-components", help="The first step of `phasm chain`: the weakly connected components of a graph "
                                                "file written by `layout-edges --merge`, one file per component.")
    k.add_argument("-f", "--format", default="gfa2", help="comma separated: gfa1, gfa2, graphml (default: gfa2)")
    k.add_argument("-o", "--output-dir", required=True)
    k.add_argument("--device", type=int, default=None)
    k.add_argument("--bubblechains", action="store_true",
                   help="also build the bubble chains of every component: component{i}.bubblechain{j}.* and the node attribute "
                        "bubblechain in component{i}.graphml")
    k.add_argument("--min-nodes", type=int, default=1, help="with --bubblechains: drop chains with fewer nodes (default: 1)")
    k.add_argument("--contigs", action="store_true",
                   help="also build the contigs outside the bubble chains: component{i}.contig{j}.* and the edge attribute contig "
                        "in component{i}.graphml (implies --bubblechains)")
    k.add_argument("-l", "--min-length", type=_int_in(0, 2**63 - 1), default=5000,
                   help="with --contigs: drop contigs shorter than this many bases (default: 5000)")
    k.add_argument("--superbubbles", action="store_true",
                   help="also log, per component, the number of superbubbles of its acyclic partition")
    k.add_argument("--cyclic", action="store_true",
                   help="with --superbubbles: also log, per component, the superbubbles of all its partitions, the cyclic ones included; "
                        "with --bubblechains / --contigs: build them on those superbubbles, so a circular component is one ring chain")
    k.add_argument("--partitions", action="store_true",
                   help="also log, per component, the partitions superbubble detection starts with (strongly connected components)")
    k.add_argument("graph_gfa", help="the graph file (S, F and E lines)")
    k.set_defaults(func=chain_components)
    # `phasm chain` itself, with its own arguments (assembler.py): chain-components --bubblechains --contigs
    m = sub.add_parser("chain", help="`phasm chain`: per weakly connected component of a graph file its bubble chains and the "
                                     "contigs outside them, one file each, then the component's own.")
    m.add_argument("-l", "--min-length", type=_int_in(0, 2**63 - 1), default=5000,
                   help="minimum length of a contig outside the bubble chains (default: 5000)")
    m.add_argument("-f", "--format", default="gfa2", help="comma separated: gfa1, gfa2, graphml (default: gfa2)")
    m.add_argument("-o", "--output-dir", required=True)
    m.add_argument("--device", type=int, default=None)
    m.add_argument("--cyclic", action="store_true",
                   help="build the chains on the superbubbles of all partitions, the cyclic ones included: a circular component is one "
                        "ring chain that holds all its bubbles (the reference stops one bubble short of closing the ring)")
    m.add_argument("graph_gfa", help="the graph file (S, F and E lines)")
    m.set_defaults(func=chain_components, bubblechains=True, contigs=True, min_nodes=1, superbubbles=False, partitions=False, as_chain=True)
    sc = sub.add_parser("spell-contigs", help="Per graph file that is one simple path (or one node) its sequence as one FASTA entry "
                                              "named after the file: the no-bubble branch of `phasm phase`.  The line format is "
                                              "this tool's own (`>name`, then the sequence on ONE line): the reference writes through "
                                              "dinopy, whose line width is not pinned here.")
    sc.add_argument("-o", "--output", type=argparse.FileType("wb"), required=True, help="the FASTA file to write")
    sc.add_argument("--device", type=int, default=None)
    sc.add_argument("fasta_input", help="the reads (FASTA); both strands go on the handle, as `overlap` adds them")
    sc.add_argument("graph_gfa", nargs="+", help="graph files (S, F and E lines), each one simple path or a single node")
    sc.set_defaults(func=spell_contigs)
    # -b as `phasm phase` names it (assembler.py)
    bp = sub.add_parser("bubble-paths", help="Per top-level bubble of a graph file what `phasm phase` computes before it looks at a "
                                             "read: chain, position, entrance, exit, interior nodes, the number of simple paths, "
                                             "and the arm phase() would take, as TSV.")
    bp.add_argument("-b", "--max-bubble-size", type=_int_in(0, 2**64 - 1), default=10,
                    help="a bubble with more paths is `large` and its paths are not listed (default: 10)")
    bp.add_argument("--list", action="store_true", help="also the paths of every bubble that is not large, by segment name (P lines)")
    bp.add_argument("-o", "--output", type=argparse.FileType("w"), default=sys.stdout)
    bp.add_argument("--device", type=int, default=None)
    bp.add_argument("graph_gfa", help="the graph file (S, F and E lines)")
    bp.set_defaults(func=bubble_paths)
    # option names and defaults of `phasm phase`, assembler.py:572-656 (-D is not offered: the device returns no per-read
    # probabilities)
    ph = sub.add_parser("phase", help="`phasm phase`: phase the bubble chain of every subgraph and write the sequence of every "
                                      "haplotype of every haploblock as FASTA (`>name`, then the sequence on ONE line); a subgraph "
                                      "without bubbles gives the entry `spell-contigs` writes.")
    ph.add_argument("-p", "--ploidy", type=int, required=True, help="the ploidy level (1 to 8)")
    ph.add_argument("-s", "--min-spanning-reads", type=_int_in(0, 2**32 - 1), default=3,
                    help="fewer spanning reads between two bubbles start a new haploblock (default: 3)")
    ph.add_argument("-b", "--max-bubble-size", type=_int_in(0, 2**32 - 1), default=10,
                    help="a bubble with more simple paths is phased on its own (default: 10)")
    ph.add_argument("-t", "--threshold", type=float, default=1e-3, help="minimum relative likelihood of a candidate (default: 1e-3)")
    ph.add_argument("-d", "--prune-factor", type=float, default=0.1, help="prune candidates below this factor of the best (default: 0.1)")
    ph.add_argument("-c", "--max-candidates", type=_int_in(0, 2**32 - 1), default=500, help="candidates to prune down to (default: 500)")
    ph.add_argument("-r", "--max-prune-rounds", type=_int_in(0, 1024), default=9, help="maximum number of pruning rounds (default: 9)")
    ph.add_argument("-S", "--prune-step-size", type=float, default=0.1, help="raise of the prune factor per round (default: 0.1)")
    ph.add_argument("-o", "--output", type=argparse.FileType("wb"), required=True, help="the FASTA file to write")
    ph.add_argument("--max-listed-paths", type=_int_in(1, 2**30 - 1), default=MAX_LISTED_PATHS,
                    help="the paths of a bubble are listed on the device, and the bubble can be phased, only up to this many: a cap on "
                         "device memory (default: 2^20)")
    ph.add_argument("--device", type=int, default=None)
    ph.add_argument("--host-sets", action="store_true",
                    help="keep prev_graph_reads / prev_aligning_reads and the relevant reads of every bubble on the host (po_phase_relevant + "
                         "po_walk_step) instead of on the device (po_walk_relevant + po_walk_step_resident); the output is the same")
    ph.add_argument("--seed", type=int, default=None, help="seed of the choice among equally likely candidates (default: unseeded)")
    ph.add_argument("reads_fasta", help="the reads (FASTA); both strands go on the handle, as `overlap` adds them")
    ph.add_argument("alignments_gfa", help="the GFA2 file with all pairwise local alignments")
    ph.add_argument("subgraphs", nargs="+", help="the bubble chain / contig graph files (S, F and E lines)")
    ph.set_defaults(func=phase)
    args = parser.parse_args(argv)
    if not getattr(args, "func", None):    args = parser.parse_args(argv)
    if not getattr(args, "func", None):
        parser.print_help()
        return 1
    logging.basicConfig(level=[logging.WARNING, logging.INFO, logging.DEBUG][min(args.verbose, 2)],
                        stream=sys.stderr)
    args.func(args)
    for name in ("output", "out", "graphml"):   # (the command may end with os._exit: nothing may be left in a Python buffer)
        f = getattr(args, name, None)
        if f is not None and f not in (sys.stdout, sys.stderr):
            f.close()
        elif f is not None:
            f.flush()
    return 0


def _run_as_command() -> None:
    """The command ends when its output is on disk: the handle's device buffers, the page-locked pools and the GPU runtime
    are left to the operating system (giving 600 MB of page-locked and device memory back buffer by buffer, and unloading
    the runtime, took 0.15 s of the `overlap` command's 0.8 s)."""
    import os
    argv = sys.argv[1:]
    if argv and argv[0] == "overlap" and "--keep-teardown" not in argv:
        argv = ["overlap", "--leave-handle-to-exit"] + argv[1:]
    else:
        argv = [a for a in argv if a != "--keep-teardown"]
    rc = 1
    try:
        rc = main(argv)
        sys.stdout.flush()
        sys.stderr.flush()
    except SystemExit as e:
        raise e
    except BaseException:
        import traceback
        traceback.print_exc()
        sys.stderr.flush()
        os._exit(1)
    os._exit(rc)


if __name__ == "__main__":
    _run_as_command()
