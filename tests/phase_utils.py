"""The contract of po_phase_branch (include/phasm_overlap.h) as plain Python, the scheme the kernels
use, the direct cases and the loader of tests/golden/phase_cases.npz.

``definition`` restates the loops of the reference on local read ids: ``generate_new_hsets`` and ``calculate_rl``
(phasm/phasing.py:435-480, 564-631) -- per candidate set and extension every relevant read and every alignment --, ``prune``
(phasing.py:482-539) and the scoring of ``phase_large_bubble`` (phasing.py:633-685).  ``scheme`` is the table decomposition the
device uses, vectorised in numpy: ``phasm_amd.phasing.HostScorer``, the host scorer of the Python layer.

A CASE is a dict: the sizes ``k P C R n_b``, ``start`` (start of a block), ``min_span``, ``threshold`` (linear), ``prune`` (None or
``{"factor", "step", "max_candidates", "max_rounds"}``) and the arrays of ``po_phase_input`` as lists.  A RESULT is a dict:
``kept_cand / kept_ext / kept_rl`` (the list ``branch`` returns), ``surv`` (the places in the kept list of what ``prune`` left),
``levels`` (log10 of the factors the loop reached), ``scores`` (per path, None when there are no reads) and ``winner``."""
import math
import os
from itertools import combinations_with_replacement, product

import numpy as np

import components_utils as cu
import reduce_utils as ru
from phasm_amd import phasing

GOLDEN_FILE = os.path.join(ru.GOLDEN, "phase_cases.npz")
EPS = 2.0 ** -52
SITUATIONS = ("read_without_alignments", "overlap_max_zero", "overlap_max_negative", "overlap_max_below_every_start",
              "all_zero_sum_kept_at_threshold_0", "all_zero_sum_dropped_at_positive_threshold", "multiplicity_2", "multiplicity_3",
              "multiplicity_k", "two_paths_with_one_interior", "empty_candidate_set", "read_set_shares_reads_with_a_path",
              "too_few_spanning_reads", "no_pruning", "one_prune_round", "several_prune_rounds_down_to_max_candidates",
              "stopped_by_max_prune_rounds", "level_above_0_empties_the_list", "fewer_than_2_entries", "maximum_minus_inf",
              "prune_level_of_exactly_0")
INPUT_KEYS = ("overlap_max", "aln_off", "aln_b", "aln_a0", "aln_a1", "path_off", "path_ids", "set_off", "set_ids")


def tol(rl, k, R):
    """|rl - reference| allowed: a sum of k*R non-negative float64 quotients in any order, one division, two log10 within
    2 ulp each, one addition: (k*R + 16) * 2^-52 * max(1, |rl|).  Infinite values must be equal."""
    return (k * R + 16) * EPS * max(1.0, abs(rl)) if math.isfinite(rl) else 0.0


def table_tol(s, R):
    return (R + 2) * EPS * max(1.0, abs(s))


def same_rl(got, want, k, R):
    return got == want if not (math.isfinite(got) and math.isfinite(want)) else abs(got - want) <= tol(want, k, R)


def bubble_of(case) -> phasing.PackedBubble:
    u32 = lambda x: np.asarray(x, dtype=np.uint32)   # noqa: E731
    i32 = lambda x: np.asarray(x, dtype=np.int32)    # noqa: E731
    return phasing.PackedBubble(case["k"], case["P"], case["C"], case["R"], case["n_b"], i32(case["overlap_max"]), u32(case["aln_off"]),
                                u32(case["aln_b"]), i32(case["aln_a0"]), i32(case["aln_a1"]), u32(case["path_off"]), u32(case["path_ids"]),
                                u32(case["set_off"]), u32(case["set_ids"]))


def ext_id(ext, P):
    x = 0
    for d in ext:
        x = x * P + d
    return x


def _lists(case):
    k, P, C, R = case["k"], case["P"], case["C"], case["R"]
    aln = [[(case["aln_b"][j], case["aln_a0"][j], case["aln_a1"][j]) for j in range(case["aln_off"][r], case["aln_off"][r + 1])]
           for r in range(R)]
    paths = [set(case["path_ids"][case["path_off"][p]:case["path_off"][p + 1]]) for p in range(P)]
    sets = [[set(case["set_ids"][case["set_off"][c * k + i]:case["set_off"][c * k + i + 1]]) for i in range(k)] for c in range(C)]
    return aln, paths, sets


def _overlap(las, om, reads):
    start, end = 2 ** 63 - 1, 0
    for b, a0, a1 in las:
        if b in reads:
            start = min(start, a0)
            end = max(end, min(om, a1))
    return (end - start) / om if start < end else None


def calculate_rl(case, aln, hap_sets, ext_sets, ext, num_possible_sets):
    """calculate_rl, phasing.py:564-631, with the reference's order of operations."""
    k, R = case["k"], case["R"]
    if R < case["min_span"]:
        return -math.inf
    p_sr = 0.0
    for r in range(R):
        read_prob = 0.0
        for hap, extra in zip(hap_sets, ext_sets):
            f = _overlap(aln[r], case["overlap_max"][r], hap | extra)
            if f is not None:
                read_prob += f
        read_prob /= k
        p_sr += read_prob
    p_sr /= R
    p_sr = -math.inf if p_sr == 0.0 else math.log10(p_sr)
    counts = {}
    for d in ext:
        counts[d] = counts.get(d, 0) + 1
    coeff, total = 1.0, 0
    for m in counts.values():
        total += m
        coeff *= float(math.comb(total, m))
    return p_sr + math.log10(coeff / num_possible_sets)


def prune_definition(rls, prune, trace=None):
    """prune, phasing.py:482-539, on the list of log_rl: the places that survive; ``trace`` receives the log10 levels used."""
    keep = list(range(len(rls)))
    if len(rls) < 2 or prune is None:
        return keep
    factor = prune["factor"]
    if factor <= 0.0:
        return keep
    level = math.log10(factor)
    best = max(rls)
    if best == -math.inf:
        return keep
    if trace is not None:
        trace.append(level)
    keep = [j for j in keep if rls[j] - best >= level]
    rounds = 1
    while len(keep) > prune["max_candidates"] and rounds < prune["max_rounds"] and factor < 1.0:
        factor += prune["step"]
        level = math.log10(factor)
        if trace is not None:
            trace.append(level)
        keep = [j for j in keep if rls[j] - best >= level]
        rounds += 1
    return keep


def definition(case, all_rl=None):
    """The RESULT of a case by the reference's loops.  ``all_rl`` (a list) receives (cand, ext id, rl) of EVERY extension."""
    k, P, C, R = case["k"], case["P"], case["C"], case["R"]
    aln, paths, sets = _lists(case)
    thr = -math.inf if case["threshold"] == 0.0 else math.log10(case["threshold"])
    out = {"kept_cand": [], "kept_ext": [], "kept_rl": []}
    for c in range(C):
        it = combinations_with_replacement(range(P), k) if case["start"] else product(range(P), repeat=k)
        for ext in it:
            rl = calculate_rl(case, aln, sets[c], [paths[d] for d in ext], ext, P ** k)
            if all_rl is not None:
                all_rl.append((c, ext_id(ext, P), rl))
            if rl >= thr:
                out["kept_cand"].append(c)
                out["kept_ext"].append(ext_id(ext, P))
                out["kept_rl"].append(rl)
    levels = []
    out["surv"] = prune_definition(out["kept_rl"], case.get("prune"), levels)
    out["levels"] = levels
    out["scores"], out["winner"] = None, None
    if R:
        scores = []
        for p in range(P):
            s = 0.0
            for r in range(R):
                f = _overlap(aln[r], case["overlap_max"][r], paths[p])
                if f is not None:
                    s += f
            scores.append(s / R)
        out["scores"] = scores
        out["winner"] = sorted(range(P), key=lambda p: scores[p], reverse=True)[0]
    return out


def call_scorer(scorer, case, pruned):
    """(cand, ext, rl) of a case from a scorer of phasm_amd.phasing -- the kept list, or with ``pruned`` the survivors."""
    b = bubble_of(case)
    pr = case.get("prune")
    if pruned and pr is not None:
        return phasing.branch_and_prune(scorer, b, case["start"], case["threshold"], case["min_span"], pr["factor"], pr["step"],
                                        pr["max_candidates"], pr["max_rounds"])
    return phasing.branch(scorer, b, case["start"], case["threshold"], case["min_span"])


def result_of(scorer, case):
    """The RESULT of a case from a scorer: two calls (kept list, survivors) and the path scores."""
    cand, ext, rl = call_scorer(scorer, case, False)
    out = {"kept_cand": cand.tolist(), "kept_ext": ext.tolist(), "kept_rl": rl.tolist()}
    sc, se, sr = call_scorer(scorer, case, True)
    place = {(c, e): j for j, (c, e) in enumerate(zip(out["kept_cand"], out["kept_ext"]))}
    out["surv"] = [place[(c, e)] for c, e in zip(sc.tolist(), se.tolist())]
    out["surv_rl"] = sr.tolist()
    st = scorer.phase_stats()
    out["level_used"] = st["level_used"]
    out["scores"], out["winner"] = None, None
    if case["R"]:
        scores = phasing.score_paths(scorer, bubble_of(case))
        out["scores"] = scores.tolist()
        out["winner"] = phasing.best_paths(scores, 1)[0]
    return out


def scheme(case):
    return result_of(phasing.HostScorer(), case)


def scheme_all_rl(case):
    """rl of every extension id [C, P^k] and the listed mask [P^k], by the scheme (threshold 0, no pruning)."""
    b = bubble_of(case)
    P, k = case["P"], case["k"]
    cand, ext, rl = phasing.HostScorer().phase_branch(b, False, case["min_span"], 0.0)
    full = np.full((case["C"], P ** k), np.nan)
    full[cand, ext] = rl
    digits = np.stack(np.unravel_index(np.arange(P ** k), (P,) * k), axis=1)
    listed = np.all(digits[:, 1:] >= digits[:, :-1], axis=1) if case["start"] else np.ones(P ** k, dtype=bool)
    return full, listed


def check_result(got, want, case, exact_rl=False):
    """A RESULT (of the scheme, the host emulation or the device) against another (the reference's): lists and order exactly,
    rl within tol, scores within the table's tolerance."""
    k, R = case["k"], case["R"]
    assert got["kept_cand"] == list(want["kept_cand"]) and got["kept_ext"] == list(want["kept_ext"])
    for g, w in zip(got["kept_rl"], want["kept_rl"]):
        assert (g == w) if exact_rl else same_rl(g, w, k, R), (g, w)
    if level_zero(case):
        # a level of exactly 0: the greatest entry survives, every survivor is within tol of the greatest
        if len(want["kept_rl"]) >= 2 and max(want["kept_rl"]) != -math.inf:
            best = max(got["kept_rl"])
            assert got["kept_rl"].index(best) in got["surv"]
            assert all(abs(got["kept_rl"][j] - best) <= tol(best, k, R) for j in got["surv"])
    else:
        assert got["surv"] == list(want["surv"])
    if want["scores"] is None:
        assert got["scores"] is None
    else:
        assert got["winner"] == want["winner"]
        for g, w in zip(got["scores"], want["scores"]):
            assert abs(g - w) * R <= table_tol(w * R, R), (g, w)


def level_zero(case):
    pr = case.get("prune")
    return pr is not None and any(x == 0.0 for x in phasing.prune_levels(pr["factor"], pr["step"], pr["max_rounds"]))


def conditions_hold(case, rls_all, kept_rl, levels_used, scores):
    """The three conditions on a case's own numbers: no rl within 4 tol of log10(threshold); no rl - max within 4 tol of a prune
    level the loop consults (a level of exactly 0 aside: ``level_zero``); the two best path scores more than 4 tol apart."""
    k, R = case["k"], case["R"]
    if case["threshold"] > 0.0:
        thr = math.log10(case["threshold"])
        if any(math.isfinite(x) and abs(x - thr) <= 4 * tol(x, k, R) for x in rls_all):
            return False
    if levels_used and kept_rl:
        best = max(kept_rl)
        for level in levels_used:
            if level == 0.0:
                continue
            if any(math.isfinite(x) and abs((x - best) - level) <= 4 * tol(x, k, R) for x in kept_rl):
                return False
    if scores is not None and len(scores) > 1:
        a, b = sorted(scores, reverse=True)[:2]
        if (a - b) * R <= 4 * table_tol(a * R, R):
            return False
    return True


def situations(case, res, rls_all):
    """The situations of SITUATIONS a case shows (``res``: its RESULT, ``rls_all``: (cand, ext, rl) of every extension)."""
    k, P, C, R = case["k"], case["P"], case["C"], case["R"]
    aln, paths, sets = _lists(case)
    out = set()
    om = case["overlap_max"]
    for r in range(R):
        if not aln[r]:
            out.add("read_without_alignments")
        if om[r] == 0:
            out.add("overlap_max_zero")
        if om[r] < 0:
            out.add("overlap_max_negative")
        if aln[r] and 0 < om[r] < min(a[1] for a in aln[r]):
            out.add("overlap_max_below_every_start")
    zero = [rl for _, _, rl in rls_all if rl == -math.inf]
    if R >= case["min_span"] and zero:
        out.add("all_zero_sum_kept_at_threshold_0" if case["threshold"] == 0.0 else "all_zero_sum_dropped_at_positive_threshold")
    if R < case["min_span"]:
        out.add("too_few_spanning_reads")
    # a path repeated in an enumerated extension: k times in (p, .., p); 2 or 3 times beside another path when P >= 2
    if k == 2 or (k >= 3 and P >= 2):
        out.add("multiplicity_2")
    if k == 3 or (k >= 4 and P >= 2):
        out.add("multiplicity_3")
    if k >= 2:
        out.add("multiplicity_k")
    if any(paths[p] == paths[q] for p in range(P) for q in range(p)):
        out.add("two_paths_with_one_interior")
    if any(not s for c in sets for s in c):
        out.add("empty_candidate_set")
    if any(s & p for c in sets for s in c for p in paths):
        out.add("read_set_shares_reads_with_a_path")
    pr, n = case.get("prune"), len(res["kept_rl"])
    if pr is None:
        out.add("no_pruning")
    elif n < 2:
        out.add("fewer_than_2_entries")
    elif max(res["kept_rl"]) == -math.inf:
        out.add("maximum_minus_inf")
    elif pr["factor"] > 0.0:
        used = res["levels"]
        if level_zero(case) and 0.0 in used:
            out.add("prune_level_of_exactly_0")
        if len(used) == 1:
            out.add("one_prune_round")
        if len(used) > 1 and len(res["surv"]) <= pr["max_candidates"]:
            out.add("several_prune_rounds_down_to_max_candidates")
        if len(used) == pr["max_rounds"] and len(res["surv"]) > pr["max_candidates"]:
            out.add("stopped_by_max_prune_rounds")
        if used and used[-1] > 0.0 and not res["surv"]:
            out.add("level_above_0_empties_the_list")
    return out


# ---- the direct cases ------------------------------------------------------------------------------------------------

def random_case(seed, k, P, C, R, n_b, start, threshold=0.0, min_span=0, prune=None, odd_reads=True, twin_paths=False, max_aln=4):
    """A bubble from a seed.  ``odd_reads``: where R allows, read 0 has no alignment, read 1 overlap_max 0, read 2 a negative
    one, read 3 one below every arange[0].  ``twin_paths``: the last path has the interior of the first.  Candidate 0 has empty
    read sets; every other candidate draws its sets from all local ids, so they share reads with the paths."""
    rng = np.random.default_rng(seed)
    om = rng.integers(400, 5000, size=R).tolist()
    aln = []
    for r in range(R):
        n = int(rng.integers(1, max_aln + 1))
        mine = []
        for _ in range(n):
            a0 = int(rng.integers(0, max(om[r] - 50, 1)))
            mine.append((int(rng.integers(0, n_b)), a0, a0 + int(rng.integers(20, 1500))))
        aln.append(mine)
    if odd_reads:
        if R > 4:
            aln[0] = []
        if R > 5:
            om[1] = 0
        if R > 6:
            om[2] = -int(rng.integers(1, 300))
        if R > 7:
            aln[3] = [(b, a0 + 2, a1 + 2) for b, a0, a1 in aln[3]]
            om[3] = min(a[1] for a in aln[3]) - 1
    paths = [sorted(set(rng.integers(0, n_b, size=int(rng.integers(1, 4))).tolist())) for _ in range(P)]
    if P >= 3 and not twin_paths:
        paths[1] = []                                       # a path without interior reads
    if twin_paths and P >= 2:
        paths[P - 1] = list(paths[0])
    sets = []
    for c in range(C):
        sets.append([[] if c == 0 or rng.random() < 0.2 else sorted(set(rng.integers(0, n_b, size=int(rng.integers(1, 5))).tolist()))
                     for _ in range(k)])
    b = phasing.bubble_from_arrays(k, om, aln, paths, sets, n_b)
    case = {"k": k, "P": P, "C": C, "R": R, "n_b": n_b, "start": int(bool(start)), "min_span": int(min_span),
            "threshold": float(threshold), "prune": prune}
    for key in INPUT_KEYS:
        case[key] = getattr(b, key).tolist()
    return case


def _pr(factor, step=0.1, max_candidates=500, max_rounds=9):
    return {"factor": factor, "step": step, "max_candidates": max_candidates, "max_rounds": max_rounds}


# name -> arguments of random_case (without the seed).  The shapes: n_b at the bitset word edges 1, 31, 32, 33, 65; R at the
# wave, workgroup and tile edges 0, 1, 2, 63, 64, 65, 257 and 2049 (the tile of k_ph_table holds 2048); k 1, 2, 3, 4, 8; P 1, 2,
# 10, 64; C 1, 2, 65; both block modes; the prune cases.
SPECS = {
    "nb1_k1_p1": dict(k=1, P=1, C=1, R=1, n_b=1, start=0),
    "nb31_r2": dict(k=2, P=2, C=2, R=2, n_b=31, start=0, threshold=0.01),
    "nb32_r63": dict(k=2, P=3, C=2, R=63, n_b=32, start=1, threshold=0.001),
    "nb33_r64": dict(k=3, P=3, C=2, R=64, n_b=33, start=0, threshold=0.002, prune=_pr(0.1, max_candidates=40)),
    "nb65_r65": dict(k=3, P=2, C=2, R=65, n_b=65, start=1, prune=_pr(0.3, max_candidates=3)),
    "r0_dead": dict(k=2, P=2, C=2, R=0, n_b=4, start=0, min_span=1, prune=_pr(0.1)),
    "r3_below_min_span": dict(k=2, P=3, C=1, R=3, n_b=8, start=0, min_span=4, threshold=0.001),
    "r257_k4": dict(k=4, P=3, C=2, R=257, n_b=40, start=0, threshold=0.0005, prune=_pr(0.2, max_candidates=30)),
    "r2049_past_the_tile": dict(k=2, P=2, C=2, R=2049, n_b=70, start=0, prune=_pr(0.5, max_candidates=2), max_aln=2),
    "k8_p2": dict(k=8, P=2, C=2, R=12, n_b=10, start=0, threshold=1e-6, prune=_pr(0.1, max_candidates=20)),
    "k8_p2_start": dict(k=8, P=2, C=1, R=12, n_b=10, start=1),
    "p10_k2": dict(k=2, P=10, C=3, R=20, n_b=33, start=0, threshold=0.0004, twin_paths=True, prune=_pr(0.05, 0.05, 15, 30)),
    "p10_k3_start": dict(k=3, P=10, C=2, R=9, n_b=20, start=1, prune=_pr(0.1, max_candidates=25)),
    "p64_k1": dict(k=1, P=64, C=2, R=10, n_b=65, start=0, threshold=0.0006),
    "p64_k2": dict(k=2, P=64, C=1, R=6, n_b=64, start=1, prune=_pr(0.1, 0.1, 50, 4)),
    "c65": dict(k=2, P=2, C=65, R=9, n_b=12, start=0, threshold=0.01, prune=_pr(0.1, 0.1, 10, 9)),
    "twins_zero_thr": dict(k=3, P=4, C=2, R=10, n_b=9, start=0, twin_paths=True),
    "zero_sum_positive_thr": dict(k=2, P=3, C=2, R=10, n_b=30, start=0, threshold=1e-9),
    "prune_none_factor_0": dict(k=2, P=3, C=2, R=9, n_b=9, start=0, prune=_pr(0.0)),
    "prune_one_round": dict(k=2, P=4, C=2, R=11, n_b=12, start=0, prune=_pr(0.1, max_candidates=1000)),
    "prune_max_rounds": dict(k=3, P=4, C=2, R=11, n_b=12, start=0, prune=_pr(0.01, 0.01, 1, 3)),
    "prune_passes_1": dict(k=3, P=4, C=2, R=11, n_b=12, start=0, prune=_pr(0.15, 0.2, 0, 20)),
    "prune_above_0_empties": dict(k=2, P=4, C=2, R=11, n_b=12, start=0, prune=_pr(0.7, 0.45, 0, 9)),
    "prune_one_entry": dict(k=1, P=1, C=1, R=5, n_b=4, start=0, prune=_pr(0.5), odd_reads=False),
    "prune_level_0": dict(k=2, P=3, C=2, R=9, n_b=9, start=0, prune=_pr(1.0, max_candidates=1)),
}
# more of the same at small sizes: ploidy 1..4, 1..5 paths, both modes, three thresholds (the shapes of the probe of DESIGN 3.9n)
for _i in range(40):
    SPECS["probe_%02d" % _i] = dict(k=1 + _i % 4, P=1 + (_i * 7) % 5, C=1 + _i % 3, R=5 + (_i * 5) % 23, n_b=3 + (_i * 11) % 40,
                                     start=_i % 2, threshold=(0.0, 1e-3, 0.05)[_i % 3],
                                     prune=None if _i % 4 == 0 else _pr(0.1 + 0.1 * (_i % 3), 0.1, 1 + _i % 7, 2 + _i % 8))
# past the capped grid of 524 288 threads: 530 000 extension ids (its expectation is the scheme's, which the goldens pin)
BIG_SPEC = dict(k=4, P=10, C=53, R=40, n_b=50, start=0, threshold=2e-6, prune=_pr(0.3, 0.1, 500, 9))


def build(spec, first_seed=1):
    """The case of a spec: the first seed at which the three conditions hold on the scheme's numbers."""
    for seed in range(first_seed, first_seed + 200):
        case = random_case(seed, **spec)
        full, listed = scheme_all_rl(case)
        rls_all = full[:, listed].reshape(-1).tolist()
        thr = -math.inf if case["threshold"] == 0.0 else math.log10(case["threshold"])
        kept = [x for x in rls_all if x >= thr]
        levels = []
        prune_definition(kept, case["prune"], levels)
        scores = None
        if case["R"]:
            scores = phasing.score_paths(phasing.HostScorer(), bubble_of(case)).tolist()
        if conditions_hold(case, rls_all, kept, levels, scores):
            case["seed"] = seed
            return case
    raise AssertionError("no seed satisfies the conditions for %r" % (spec,))


# ---- golden file -----------------------------------------------------------------------------------------------------

def save_golden(obj):
    cu.save_golden(obj, GOLDEN_FILE)


_GOLDEN = []


def load_golden():
    if not _GOLDEN:
        _GOLDEN.append(cu.load_golden(GOLDEN_FILE))
    return _GOLDEN[0]
