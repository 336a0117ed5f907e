"""Loaders for the committed golden vectors (tests/golden/, made by make_golden.py from the
compiled reference).  Each case is ``(name, [seq bytes...], min_length, expected_rows)`` with
expected_rows a lexicographically sorted (n,6) int64 array of
``(a_idx, b_idx, astart, aend, bstart, bend)``."""
import hashlib
import json
import os

import numpy as np

from phasm_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rows(x):
    return np.asarray(x, dtype=np.int64).reshape(-1, 6)


def sha(seqs):
    h = hashlib.sha256()
    for s in seqs:
        h.update(len(s).to_bytes(4, "little"))
        h.update(s)
    return h.hexdigest()


def json_cases(fname):
    with open(os.path.join(GOLDEN, fname)) as f:
        cases = json.load(f)
    return [(c["name"], [s.encode("latin-1") for s in c["reads"]], c["min_length"], _rows(c["rows"]))
            for c in cases]


def repeats_cases():
    z = np.load(os.path.join(GOLDEN, "repeats.npz"))
    cat = z["cat"].tobytes()
    lens = z["lens"]
    offs = np.concatenate([[0], np.cumsum(lens)])
    seqs = [cat[offs[i]:offs[i + 1]] for i in range(len(lens))]
    assert sha(seqs) == str(z["sha256"])
    return [("repeats_m%d" % m, seqs, int(m), _rows(z["rows_m%d" % m])) for m in z["min_lengths"]]


LADDER_NAMES = ["ladder_small", "ladder_varlen", "ladder_cfg1_mini", "ladder_cfg2_mini",
                "ladder_cfg4_noise", "ladder_lownoise", "cfg1_full", "cfg2_1k", "cfg3_1k", "cfg5_1k"]


def ladder_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = synth.SynthConfig(**json.loads(str(z["config"])))
    seqs = [s for _, s in synth.oriented(synth.generate_reads(cfg))]
    # the generator is seeded; the hash proves these are the reads the reference saw
    assert sha(seqs) == str(z["sha256"]), "synthetic generator drifted from the golden inputs"
    return name, seqs, int(z["min_length"]), _rows(z["rows"])


def all_small_cases():
    return json_cases("toy_cases.json") + json_cases("adversarial.json")


def random_small_inputs(n_cases=60, seed=99):
    """Seeded random read sets (substrings of a random genome, half of them with their reverse complement) and a
    min_length each: the inputs of live_random.npz."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_cases):
        glen = int(rng.integers(50, 400))
        genome = bytes(b"ACGT"[i] for i in rng.integers(0, 4, size=glen))
        reads = []
        for _ in range(int(rng.integers(2, 30))):
            ln = int(rng.integers(1, min(120, glen)))
            st = int(rng.integers(0, glen - ln + 1))
            r = genome[st:st + ln]
            reads.append(r)
            if rng.random() < 0.5:
                reads.append(r.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1])
        out.append((reads, int(rng.integers(1, 40))))
    return out


def random_small_cases():
    """random_small_inputs() with the reference's rows for each (tests/golden/live_random.npz)."""
    z = np.load(os.path.join(GOLDEN, "live_random.npz"))
    cases = []
    for t, (reads, m) in enumerate(random_small_inputs(int(z["n_cases"]), int(z["seed"]))):
        assert sha(reads) == str(z["sha256_%d" % t]) and m == int(z["min_length_%d" % t]), "random inputs drifted from the golden"
        cases.append(("random%d" % t, reads, m, _rows(z["rows_%d" % t])))
    return cases


# read sets the ladder does not cover: config-2 density on a seed of its own, and a variable-length diploid set with
# containments (stored in the ladder's format, loaded with ladder_case)
FRESH_CASES = {
    "fresh_cfg2_700": (dict(synth.scaled(synth.CONFIGS["cfg2"], 700).__dict__, seed=4242), 1000),
    "fresh_varlen_500": (dict(n_reads=500, read_len=6000, genome_len=150_000, ploidy=2, snp=0.004, seed=909,
                              len_sd=2500.0, len_min=800, len_max=15000), 600),
}


def fresh_config(name):
    kw, m = FRESH_CASES[name]
    return synth.SynthConfig(**kw), m
