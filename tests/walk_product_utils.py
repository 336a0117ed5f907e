"""The product's walk (``phasing.phase_chain`` on a ``DeviceWalk`` or a ``HostWalk``) as a route of tests/walk_utils.py: the
(steps, final, state) that ``walk_utils.same_trace`` holds to a recorded walk, the bytes of every step call, and the bubbles of a
walk as ``phasing.chain_bubbles_input`` builds them from ``HostPaths``."""
import walk_utils as wu
from phasm_amd import phasing

# what phase_chain does not know without extra device work, or knows only where it had to peek
OPTIONAL = ("state_in", "kept_cand", "kept_ext", "kept_rl")


def first(seq):
    return seq[0]


def reads_of_node(walk):
    n = wu.n_ids_of(walk)
    return lambda x: walk["merged"][x - n]["reads"] if x >= n else [x]


def recorded_bubbles(walk):
    """The bubbles as the golden holds them, the merged predecessors left out (they are no key of the alignments)."""
    return [dict(b, preds=wu.plain_preds(walk, b)) for b in walk["bubbles"]]


def node_order(walk):
    """The nodes of the walk's graph in the order its edges first name them."""
    order = []
    for u, v, _ in wu.edges_of(walk):
        for x in (u, v):
            if x not in order:
                order.append(x)
    return order


def built_bubbles(walk):
    """The bubbles of the walk's one chain from its edges: ``HostPaths`` -> ``chain_bubbles_input``."""
    hp = phasing.HostPaths(wu.edges_of(walk), node_order(walk))
    return phasing.chain_bubbles_input(hp.phase_paths(None, 64), 0, reads_of_node(walk))


def haplotypes_of(walk_obj, cands, bubbles, block_bubbles, k):
    out = []
    for hist in walk_obj.history(cands).tolist():
        haps = [[] for _ in range(k)]
        for i, e in zip(block_bubbles, hist):
            paths = bubbles[i]["paths"]
            for h, d in zip(haps, phasing.ext_digits(e, len(paths), k)):
                path = list(paths[d])
                h.extend(path[1:] if h and h[-1] == path[0] else path)
        out.append(haps)
    return out


def run_product(walk, scorer, source, index, walk_obj, bubbles=None, raw=None, choose=first):
    """The walk through ``phase_chain``.  Returns (steps, final, state) in the shape of ``walk_utils.run_arrays`` and the blocks;
    ``raw`` (a list) receives the bytes of every (cand, ext, rl) a step call returned."""
    p = walk["params"]
    k = p["ploidy"]
    bubbles = recorded_bubbles(walk) if bubbles is None else bubbles
    turns = []
    blocks = list(phasing.phase_chain(scorer, source, index, bubbles, reads_of_node(walk), k, p["min_spanning_reads"], p["max_bubble_size"],
                                      wu.param(p["threshold"]), wu.param(p["prune_factor"]), p["max_candidates"], p["max_prune_rounds"],
                                      p["prune_step_size"], walk=walk_obj, choose=choose, on_step=turns.append))
    assert turns and turns[-1].get("final") and not any(t.get("final") for t in turns[:-1])
    steps, last = turns[:-1], turns[-1]
    for s in steps:
        for cand, ext, rl in s.pop("steps"):
            if raw is not None:
                raw.append((len(raw), cand.tobytes(), ext.tobytes(), rl.tobytes()))
    final = {"yields": last["yields"]}
    if "prune_in" in last:
        final["prune_in"] = last["prune_in"]
    info = walk_obj.info()
    start = bool(info["start_of_block"])
    tie = last["yields"][0]["tie"] if last["yields"] else list(range(info["n_cands"]))
    haps = haplotypes_of(walk_obj, tie, bubbles, last["block_bubbles"], k)
    sets = walk_obj.read_sets(tie)
    cands = [{"haplotypes": h, "read_sets": s} for h, s in zip(haps, sets)]
    state = {"start": int(start), "prev_graph": last["prev_graph"], "prev_aligning": last["prev_aligning"], "n_cands": len(cands),
             "digest": wu.digest_state(start, last["prev_graph"], last["prev_aligning"], [(c["haplotypes"], c["read_sets"]) for c in cands]),
             "cands": cands}
    return (steps, final, state), blocks


def check_blocks(blocks, got):
    """The blocks the generator yielded are the yields the turns noted, in order."""
    steps, final, _ = got
    noted = [y for s in steps for y in s["yields"]] + final["yields"]
    assert len(blocks) == len(noted)
    for b, y in zip(blocks, noted):
        assert (b.haplotypes, b.read_sets, int(b.include_last), b.tie) == (y["haplotypes"], y["read_sets"], y["include_last"], y["tie"])
        assert b.from_large_bubble == (y["kind"] == "large")


# ---- a walk as the files `phase` reads ---------------------------------------------------------------------------------------------

def sequences_of(walk):
    """One random sequence per segment (upper-case ACGT), from the walk's seed."""
    import numpy as np
    rng = np.random.default_rng(walk["seed"] + 1000)
    return [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(n)).tobytes()) for n in walk["lengths"]]


def write_chain_files(walk, folder, stem="chain0"):
    """reads.fasta (segment i as ``s<i>``: its strands are the oriented reads 2i and 2i + 1), alignments.gfa (the walk's rows)
    and <stem>.gfa (the walk's graph: S lines, F lines for the merged nodes, E lines in edge order).  Returns the three paths
    and ``name(node)``."""
    import os
    n = wu.n_ids_of(walk)
    seg = lambda x: "s%d%s" % (x >> 1, "+-"[x & 1])                        # noqa: E731
    name = lambda x: seg(x) if x < n else "m%d+" % (x - n)                # noqa: E731
    length = lambda x: walk["lengths"][x >> 1] if x < n else walk["merged"][x - n]["length"]   # noqa: E731
    fasta, aln, graph = (os.path.join(folder, f) for f in ("reads.fasta", "alignments.gfa", stem + ".gfa"))
    with open(fasta, "wb") as f:
        for i, s in enumerate(sequences_of(walk)):
            f.write(b">s%d\n%s\n" % (i, s))
    with open(aln, "w") as f:
        f.write("H\tVN:Z:2.0\n")
        for i, ln in enumerate(walk["lengths"]):
            f.write("S\ts%d\t%d\t*\n" % (i, ln))
        for a, b, a0, a1, b0, b1 in wu.rows_of(walk).tolist():
            f.write("E\t*\t%s\t%s\t%d\t%d\t%d\t%d\t*\n" % (seg(a), seg(b), a0, a1, b0, b1))
    with open(graph, "w") as f:
        f.write("H\tVN:Z:2.0\n")
        seen = set()
        for x in node_order(walk):
            if name(x)[:-1] in seen:
                continue
            seen.add(name(x)[:-1])
            f.write("S\t%s\t%d\t*\n" % (name(x)[:-1], length(x)))
            if x >= n:
                m = walk["merged"][x - n]
                cur, total = 0, sum(m["prefix_lengths"])
                for k, r in enumerate(m["reads"]):
                    p = m["prefix_lengths"][k] if k < len(m["prefix_lengths"]) else None
                    f.write("F\t%s\t%s\t%d\t%d\t0\t%d\t*\n" % (name(x)[:-1], seg(r), cur, cur + p if p else m["length"], p if p else m["length"] - total))
                    cur += p or 0
        for u, v, w in wu.edges_of(walk):
            f.write("E\t*\t%s\t%s\t%d\t%d\t0\t%d\t*\n" % (name(u), name(v), w, length(u), length(u) - w))
    return fasta, aln, graph, name


def expected_fasta(walk, graph_path, name, stem="chain0"):
    """The entries `phase` must write for the walk's recorded yields, spelled by ``HostSpeller``: [(name, sequence)]."""
    from phasm_amd import spelling
    from phasm_amd.io import gfa
    with open(graph_path) as f:
        gf = gfa.read_graph_gfa(f)
    node_of = {gf.node_name(x): x for x in gf.node_order}
    seqs, ids, both = sequences_of(walk), [], []
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    for i, s in enumerate(seqs):
        ids += ["s%d+" % i, "s%d-" % i]
        both += [s, s.translate(comp)[::-1]]
    hs = spelling.HostSpeller(both, ids)
    reads_of = spelling.ReadMap.of(hs)
    yields = [y for s in walk["trace"] for y in s["yields"]] + walk["final"]["yields"]
    out = []
    for i, y in enumerate(yields):
        for j, hap in enumerate(y["haplotypes"]):
            nodes = [node_of[name(x)] for x in hap]
            seq = spelling.spell_pieces(hs, [spelling.path_pieces(gf, nodes, reads_of, bool(y["include_last"]))])[0]
            if y["kind"] == "large":
                out.append(("%s.largebubble%d" % (stem, i), seq))
                break
            out.append(("%s.haploblock%d.%d" % (stem, i, j), seq))
    return out


def read_fasta_entries(path):
    with open(path, "rb") as f:
        lines = f.read().split(b"\n")
    assert lines[-1] == b"" and len(lines) % 2 == 1
    return [(lines[i][1:].decode(), lines[i + 1]) for i in range(0, len(lines) - 1, 2)]
