#!/usr/bin/env python3
"""Developer probe: po_spell over repeated calls, from one process on the GPU -- what DESIGN.md section 3.9q records.

    python tools/spell_probe.py [--repeat 21]
        contig50k     a synthetic path of 50 000 pieces over 15 kb reads with takes around 1 000: the shape of a config-2 contig
        pieces600k    the call of tests/test_gpu_spell.py past one capped grid: 600 000 pieces with takes 0 .. 33, ~10 MB

Per input: the median, minimum and maximum of the device time (po_spell_stats.device_ms: upload of the pieces, scan, decode,
patch) and of the whole call (ExactOverlapper.spell: the device time, the copy of the bytes to the host and the split into
Python bytes objects); the device time as a fraction of what writing the output bytes alone takes at the measured HBM rate
(a device-to-device copy moves 4.9 TB/s, read + write, so 2.45 TB/s of writes); and, on a host core of
the same machine, two points of comparison: ``slice_join`` -- ``b"".join(seq[:take] ...)`` over upper-cased reads held in a
dict, which is all the reference's sequence_for_path does once its cache is warm (tests/golden/make_spell_golden.py --time
runs the reference itself) -- and HostSpeller (numpy).  Nothing here is asserted anywhere.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from phasm_amd import spelling, synth  # noqa: E402
from phasm_amd.overlapper import ExactOverlapper  # noqa: E402

HBM_WRITE_BYTES_PER_MS = 2.45e9   # half of the measured 4.9 TB/s of a device-to-device copy


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def contig_call(n_pieces=50_000, seed=5):
    cfg = synth.SynthConfig(n_reads=300, read_len=15000, genome_len=400_000, seed=seed)
    reads = synth.oriented(synth.generate_reads(cfg))
    rng = np.random.default_rng(seed)
    piece_read = rng.integers(0, len(reads), n_pieces).astype(np.uint32)
    piece_take = np.clip(np.rint(rng.normal(1000, 150, n_pieces)), 0, 15000).astype(np.uint32)
    return reads, np.asarray([0, n_pieces], dtype=np.uint64), piece_read, piece_take


def probe(reads, seq_off, piece_read, piece_take, repeat):
    ov = ExactOverlapper(device=0)
    for name, seq in reads:
        ov.add_sequence(name, seq)
    dev, wall, got = [], [], None
    for i in range(max(1, repeat) + 1):
        t0 = time.perf_counter()
        got = ov.spell(seq_off, piece_read, piece_take)
        ms = 1e3 * (time.perf_counter() - t0)
        if i:                                              # (one call outside the samples: upload, workspaces)
            wall.append(ms)
            dev.append(ov.spell_stats()["device_ms"])
    st = ov.spell_stats()
    ov.close()
    upper = {i: s.upper() for i, (_, s) in enumerate(reads)}
    t0 = time.perf_counter()
    joined = b"".join(upper[r][:t] for r, t in zip(piece_read.tolist(), piece_take.tolist()))
    ms_join = 1e3 * (time.perf_counter() - t0)
    hs = spelling.HostSpeller([s for _, s in reads])
    t0 = time.perf_counter()
    want = hs.spell(seq_off, piece_read, piece_take)
    ms_host = 1e3 * (time.perf_counter() - t0)
    assert got == want and b"".join(got) == joined
    floor = st["n_bytes"] / HBM_WRITE_BYTES_PER_MS
    return {"stats": {k: v for k, v in st.items() if k != "device_ms"}, "device_ms": spread(dev), "call_ms": spread(wall),
            "ms_hbm_write_floor": round(floor, 5), "floor_over_device": round(floor / statistics.median(dev), 4),
            "ms_slice_join_host": round(ms_join, 3), "ms_host_speller": round(ms_host, 3)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeat", type=int, default=21, help="calls per measurement; medians, minima and maxima are reported")
    args = ap.parse_args(argv)
    import spell_utils as su
    out = {"repeat": max(1, args.repeat)}
    out["contig50k"] = probe(*contig_call(), args.repeat)
    out["pieces600k"] = probe(*su.big_call(), args.repeat)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
