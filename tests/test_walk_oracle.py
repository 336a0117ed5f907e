"""Whole walks of a bubble chain without a GPU: the two routes of tests/walk_utils.py -- ``device_phaser`` on a stand-in walker,
and the plain chain ``relevant_reads`` -> ``bubble_from_relevant`` -> ``branch_and_prune`` -- on the numpy ``HostScorer`` and
``HostIndex``, held step by step to tests/golden/walk_cases.npz, which make_walk_golden.py recorded from the reference's own
``phase()``.  Also the trace's own consistency (every recorded ``branch`` step, re-packed as a one-bubble case, passes
``phase_utils.definition``), and three broken walks that the comparison must notice."""
import re

import pytest

import phase_utils as pu
import walk_utils as wu
from phasm_amd import phasing

GOLDEN = wu.load_golden()
WALKS = GOLDEN["walks"]
NAMES = [w["name"] for w in WALKS]


def host(walk):
    src = phasing.HostIndex(wu.lengths_of(walk))
    return phasing.HostScorer(), src, src.phase_index(wu.rows_of(walk))


def test_the_walks_are_the_specs():
    assert NAMES == list(wu.SPECS)
    for w in WALKS:
        spec = wu.inputs(w["name"], w["seed"])
        for key in wu.INPUT_KEYS:
            assert w[key] == spec[key], (w["name"], key)
        assert len(w["bubbles"]) <= 8 and set(wu.SPECS[w["name"]][1]) <= wu.situations(w)
        assert wu.margins_hold(w) is None
    assert sum(1 + ("kept_cand" in s) for w in WALKS for s in w["trace"]) < 150


@pytest.mark.parametrize("name", NAMES)
def test_every_branch_step_passes_the_single_bubble_definition(name):
    walk = next(w for w in WALKS if w["name"] == name)
    n = 0
    for step, case in wu.branch_cases(walk):
        got = dict(pu.definition(case), scores=None, winner=None)
        pu.check_result(got, case["ref"], case)
        n += 1
    assert n == sum("kept_cand" in s for s in walk["trace"])


@pytest.mark.parametrize("name", NAMES)
def test_the_integration_route_on_the_host_equals_the_walk(name):
    walk = next(w for w in WALKS if w["name"] == name)
    wu.same_trace(wu.run_integration(walk, *host(walk)), walk, walk, optional=("best",))


@pytest.mark.parametrize("name", NAMES)
def test_the_array_route_on_the_host_equals_the_walk(name):
    walk = next(w for w in WALKS if w["name"] == name)
    wu.same_trace(wu.run_arrays(walk, *host(walk)), walk, walk, optional=("kept_cand", "kept_ext", "kept_rl"))


BROKEN = {
    "candidate read sets translated with the previous bubble's id map": lambda w: wu.run_arrays(w, *host(w), translate=wu.stale_translation),
    "prev_graph not cleared in new_block (arrays)": lambda w: wu.run_arrays(w, *host(w), keep_prev_graph=True),
    "prev_graph not cleared in new_block (walker)": lambda w: wu.run_integration(w, *host(w), walker=wu.LeakyWalker),
    "the kept list sorted by rl before it becomes the candidates (arrays)": lambda w: wu.run_arrays(w, *host(w), sort_kept=True),
    "the kept list sorted by rl before it becomes the candidates (walker)": lambda w: wu.run_integration(w, *host(w), walker=wu.SortingWalker),
}


@pytest.mark.parametrize("what", list(BROKEN))
def test_a_broken_walk_is_noticed(what):
    """The comparison is only worth what it refuses: each of these breaks must fail it on at least one walk, and it must be
    ``same_trace`` that refuses -- its messages name the walk and the step, the final prune or the state after the walk."""
    failed = []
    for walk in WALKS:
        got = BROKEN[what](walk)                       # (the broken route itself must run through)
        try:
            wu.same_trace(got, walk, walk, optional=("best", "kept_cand", "kept_ext", "kept_rl"))
        except AssertionError as exc:
            assert re.match(r"%s( step \d+ \(bubble \d+\)| final)?: " % walk["name"], str(exc)), str(exc)
            failed.append(walk["name"])
    assert failed, what
    if "prev_graph" in what:
        assert "break_and_shrink" in failed
