"""The `phase` command as far as it needs no GPU: its arguments, the two ``PhasingError`` exits of the reference on a graph
the walk cannot start on (with the bubbles from ``HostPaths``), the no-bubble decision, and the names of the FASTA entries of a
list of blocks."""
import pytest

import walk_product_utils as wp
import walk_utils as wu
from phasm_amd import cli, phasing
from phasm_amd.io import gfa
from phasm_amd.phasing import Haploblock


def graph_and_paths(lines):
    gf = gfa.read_graph_gfa(lines)
    return gf, phasing.HostPaths(gf.edges.tolist(), gf.node_order).phase_paths(None, 64)


def lines_of(edges, nodes=None):
    nodes = nodes or sorted({x for e in edges for x in e})
    return ["S\t%s\t100\t*\n" % x for x in nodes] + ["E\t*\t%s+\t%s+\t60\t100\t0\t40\t*\n" % (u, v) for u, v in edges]


BUBBLE = [("a", "b"), ("a", "c"), ("b", "d"), ("c", "d")]


def test_the_chain_of_a_graph_that_starts_with_a_bubble():
    gf, paths = graph_and_paths(lines_of(BUBBLE + [("d", "e"), ("d", "f"), ("e", "g"), ("f", "g")]))
    chain = cli.phase_chain_of(gf, paths)
    assert chain == 0 and [int(paths.bubbles["entrance"][b]) for b in paths.chain_bubbles(chain)] == [0, 6]


def test_no_bubble_with_an_interior_is_the_contig_branch():
    gf, paths = graph_and_paths(lines_of([("a", "b"), ("b", "c")]))
    assert cli.phase_chain_of(gf, paths) is None


def test_two_nodes_of_in_degree_0():
    gf, paths = graph_and_paths(lines_of(BUBBLE + [("e", "a"), ("f", "a")]))
    with pytest.raises(cli.PhasingError, match="There are multiple nodes with in-degree 0, not sure what the start point is."):
        cli.phase_chain_of(gf, paths)


def test_a_start_that_is_no_bubble_entrance():
    # e -> f -> a is no chain of bubbles: f has one way in and one way out, the pair (e, f) has no interior and is dropped
    gf, paths = graph_and_paths(lines_of([("e", "x"), ("e", "y"), ("x", "z"), ("y", "z"), ("x", "w"), ("z", "a")] + BUBBLE, "abcdexyzw"))
    with pytest.raises(cli.PhasingError, match="Unexpected starting point 'e\\+', this is not a bubble entrance"):
        cli.phase_chain_of(gf, paths)


def test_the_exit_of_the_command_names_the_file(tmp_path, monkeypatch):
    graph = tmp_path / "component0.bubblechain0.gfa"
    graph.write_text("".join(lines_of(BUBBLE + [("e", "a"), ("f", "a")])))
    (tmp_path / "reads.fasta").write_text("")
    monkeypatch.setattr(cli, "_subgraph_bubble_paths", lambda path, device: graph_and_paths(open(path)))

    class NoDevice:
        def __init__(self, device=None):
            pass

        def add_fasta(self, path, both_strands=True):
            return 0

        def ids(self):
            return []

        def lengths(self):
            return []

    monkeypatch.setattr(cli, "ExactOverlapper", NoDevice)
    with pytest.raises(SystemExit, match="bubblechain0.gfa: There are multiple nodes with in-degree 0"):
        cli.main(["phase", "-p", "2", "-o", str(tmp_path / "out.fasta"), str(tmp_path / "reads.fasta"), "none.gfa", str(graph)])
    with pytest.raises(SystemExit, match="the ploidy must be 1 to 8"):
        cli.main(["phase", "-p", "9", "-o", str(tmp_path / "out.fasta"), str(tmp_path / "reads.fasta"), "none.gfa", str(graph)])


@pytest.mark.parametrize("argv", [["phase", "-o", "x", "r", "a", "g"], ["phase", "-p", "2", "r", "a", "g"], ["phase", "-p", "2", "-o", "x", "r", "a"],
                                  ["phase", "-p", "2", "-s", "-1", "-o", "x", "r", "a", "g"], ["phase", "-p", "2", "-D", "d", "-o", "x", "r", "a", "g"]])
def test_argument_errors(argv, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2


def test_the_defaults_are_the_reference_s(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(cli, "phase", lambda args: seen.update(vars(args)))
    monkeypatch.chdir(tmp_path)
    cli.main(["phase", "-p", "2", "-o", "out.fasta", "r", "a", "g1", "g2"])
    assert {k: seen[k] for k in ("ploidy", "min_spanning_reads", "max_bubble_size", "threshold", "prune_factor", "max_candidates",
                                 "max_prune_rounds", "prune_step_size", "seed", "subgraphs")} == \
        {"ploidy": 2, "min_spanning_reads": 3, "max_bubble_size": 10, "threshold": 1e-3, "prune_factor": 0.1, "max_candidates": 500,
         "max_prune_rounds": 9, "prune_step_size": 0.1, "seed": None, "subgraphs": ["g1", "g2"]}


def test_the_names_of_the_entries():
    blocks = [Haploblock([[1, 2], [1, 3]], [[], []], False, False, -1.0, [0]), Haploblock([[4, 5], []], [[], []], False, True, 0.0, None),
              Haploblock([[6, 7], [6, 8]], [[], []], True, False, -2.0, [0, 1])]
    assert list(cli.phase_entries("chain3", blocks)) == [
        ("chain3.haploblock0.0", [1, 2], False), ("chain3.haploblock0.1", [1, 3], False), ("chain3.largebubble1", [4, 5], False),
        ("chain3.haploblock2.0", [6, 7], True), ("chain3.haploblock2.1", [6, 8], True)]


def test_the_entries_of_a_golden_walk_from_a_host_walk(tmp_path):
    """The blocks of ``phase_chain`` on a ``HostWalk`` over the files of a golden walk, through the command's own naming and
    ``spelling.path_pieces``: the entries ``expected_fasta`` spells from the recording."""
    from phasm_amd import spelling
    walk = next(w for w in wu.load_golden()["walks"] if w["name"] == "ploidy3_rounds")
    fasta, aln, graph, node_name = wp.write_chain_files(walk, str(tmp_path))
    gf, paths = graph_and_paths(open(graph))
    assert cli.phase_chain_of(gf, paths) == 0
    src = phasing.HostIndex(wu.lengths_of(walk))
    sc = phasing.HostScorer()
    got, blocks = wp.run_product(walk, sc, src, src.phase_index(wu.rows_of(walk)), phasing.HostWalk(sc, 3))
    to_file = {x: n for n, x in ((n, next(y for y in wp.node_order(walk) if node_name(y) == gf.node_name(n))) for n in gf.node_order)}
    want = wp.expected_fasta(walk, graph, node_name)
    entries = list(cli.phase_entries("chain0", blocks))
    assert [e[0] for e in entries] == [n for n, _ in want]
    both, ids = [], []
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    for i, s in enumerate(wp.sequences_of(walk)):
        ids += ["s%d+" % i, "s%d-" % i]
        both += [s, s.translate(comp)[::-1]]
    hs = spelling.HostSpeller(both, ids)
    reads_of = spelling.ReadMap.of(hs)
    seqs = spelling.spell_pieces(hs, [spelling.path_pieces(gf, [to_file[x] for x in nodes], reads_of, last) for _, nodes, last in entries])
    assert seqs == [s for _, s in want]
