"""po_phase_branch on the device against tests/golden/phase_cases.npz (the reference's own branch, prune and
phase_large_bubble): the kept list, the survivors and their order exactly, log_rl within ``tol``, the table within its
tolerance, two calls on one input bit for bit the same -- through ``phasm_amd.phasing`` (``branch``, ``branch_and_prune``,
``score_paths``) and ``device_phaser`` on a real handle.  One case lies past the capped grid of 524 288 threads; its
expectation is the scheme's, which tests/test_phase_oracle.py pins to the same goldens."""
import math
import os
import sys

import numpy as np
import pytest

import phase_utils as pu
from phasm_amd import phasing
from phasm_amd.overlapper import ExactOverlapper

pytestmark = pytest.mark.gpu

CASES = pu.load_golden()["cases"]


@pytest.fixture(scope="module")
def ov():
    h = ExactOverlapper()
    yield h
    h.close()


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_device_equals_the_golden(ov, name):
    case = next(c for c in CASES if c["name"] == name)
    ref, k, P, C, R = case["ref"], case["k"], case["P"], case["C"], case["R"]
    got = pu.result_of(ov, case)            # branch, branch_and_prune, score_paths
    pu.check_result(got, ref, case)
    assert got["surv_rl"] == [got["kept_rl"][j] for j in got["surv"]]
    b = pu.bubble_of(case)
    cand, ext, rl, table = ov.phase_branch(b, case["start"], case["min_span"], case["threshold"], want_table=True)
    st = ov.phase_stats()
    n_tuples = math.comb(P + k - 1, k) if case["start"] else P ** k
    assert st["n_extensions"] == C * n_tuples and st["n_kept"] == st["n_survivors"] == len(ref["kept_rl"]) and st["level_used"] == -1
    if len(rl):
        assert st["max_rl"] == rl.max()
    want = phasing.HostScorer().table(b).reshape(-1)
    assert table.shape == want.shape and all(abs(g - w) <= pu.table_tol(w, R) for g, w in zip(table.tolist(), want.tolist()))
    # the same input, the same bits
    cand2, ext2, rl2, table2 = ov.phase_branch(b, case["start"], case["min_span"], case["threshold"], want_table=True)
    assert cand2.tobytes() == cand.tobytes() and ext2.tobytes() == ext.tobytes() and rl2.tobytes() == rl.tobytes()
    assert table2.tobytes() == table.tobytes()
    pr = case["prune"]
    if pr is not None and not pu.level_zero(case):
        phasing.branch_and_prune(ov, b, case["start"], case["threshold"], case["min_span"], pr["factor"], pr["step"], pr["max_candidates"],
                                 pr["max_rounds"])
        st = ov.phase_stats()
        assert st["n_kept"] == len(ref["kept_rl"]) and st["n_survivors"] == len(ref["surv"])
        assert st["level_used"] == len(ref["levels"]) - 1
        if ref["levels"]:
            assert st["level_used"] >= 16 or st["level_counts"][st["level_used"]] == len(ref["surv"])


def test_cap_smaller_than_the_count(ov):
    from test_phase_rejections import FILL, phase_call
    from phasm_amd import _lib
    case = next(c for c in CASES if c["name"] == "twins_zero_thr")           # 128 kept, room for 64
    ref = case["ref"]
    status, _, bufs, n = phase_call(ov, case)
    assert status == _lib.PO_OK and n == len(ref["kept_rl"]) == 128
    assert bufs[0].view(np.uint32)[:64].tolist() == ref["kept_cand"][:64] and (bufs[0][256:] == FILL).all()
    assert bufs[1].view(np.uint32)[:64].tolist() == ref["kept_ext"][:64] and (bufs[1][256:] == FILL).all()
    assert all(pu.same_rl(g, w, case["k"], case["R"]) for g, w in zip(bufs[2].view(np.float64).tolist(), ref["kept_rl"][:64]))
    few = ov.phase_branch(pu.bubble_of(case), case["start"], cap=5)
    assert few[0].tolist() == ref["kept_cand"][:5] and ov.phase_stats()["n_kept"] == 128
    none = ov.phase_branch(pu.bubble_of(case), case["start"], cap=0)
    assert len(none[0]) == 0 and ov.phase_stats()["n_kept"] == 128


def test_past_the_capped_grid(ov):
    case = pu.build(pu.BIG_SPEC)
    assert case["C"] * case["P"] ** case["k"] == 530000
    want = pu.scheme(case)
    got = pu.result_of(ov, case)
    pu.check_result(got, want, case)
    assert len(want["kept_rl"]) > 1000 and 0 < len(want["surv"]) < len(want["kept_rl"])
    # with threshold 0 every extension id comes out, in id order
    b = pu.bubble_of(case)
    cand, ext, rl = ov.phase_branch(b, False)
    assert len(rl) == 530000 and (cand.astype(np.int64) * 10000 + ext == np.arange(530000)).all()
    full, _ = pu.scheme_all_rl(case)
    flat = full.reshape(-1)
    assert np.array_equal(np.isfinite(rl), np.isfinite(flat))
    fin = np.isfinite(flat)
    assert (np.abs(rl[fin] - flat[fin]) <= (case["k"] * case["R"] + 16) * pu.EPS * np.maximum(1.0, np.abs(flat[fin]))).all()


def test_device_phaser_on_a_real_handle(ov):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "integration", "phasm"))
    from phasing_device import device_phaser
    from test_phase_python import Log, StandInPhaser, StandInSet, objects_of
    for name in ("nb33_r64", "p10_k3_start", "k8_p2", "c65"):
        case = next(c for c in CASES if c["name"] == name)
        node_paths, read_sets, rel = objects_of(case, True)
        ph = device_phaser(StandInPhaser, ov)()
        ph.ploidy, ph.start_of_block, ph.min_spanning_reads = case["k"], bool(case["start"]), case["min_span"]
        ph.threshold, ph.debug_data_log, ph.candidate_sets = case["threshold"], Log(), []
        for c, sets in enumerate(read_sets):
            hs = StandInSet(case["k"])
            for i in range(case["k"]):
                hs.haplotypes[i].append("cand%d" % c)
                hs.read_sets[i] |= sets[i]
            ph.candidate_sets.append(hs)
        kept = ph.branch(node_paths, rel)
        ref = case["ref"]
        index = {p: j for j, p in enumerate(node_paths)}
        assert [int(hs.haplotypes[0][0][4:]) for hs in kept] == ref["kept_cand"]
        assert [pu.ext_id([index[tuple(list(h)[1:])] for h in hs.haplotypes], case["P"]) for hs in kept] == ref["kept_ext"]
        assert all(pu.same_rl(hs.log_rl, w, case["k"], case["R"]) for hs, w in zip(kept, ref["kept_rl"]))
