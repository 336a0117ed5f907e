"""Every PHASM_* switch that selects a kernel, a row order, a buffer or a sync path, run where it acts, with the rows held
against the golden rows and the switch shown to have acted.

One table: each entry names the switch and its value, the input, the entry point, and the proof -- a po_stats field that
differs from the call without the switch, a stderr trace line, a host range the library did (not) pin, or the thread count
of a child process.  Some switches leave no trace inside the process (PHASM_VERIFY_STAGED=0 launches the unstaged
k_verify_a, PHASM_SELECT_KERNEL=1 the separate k_select_local): their proof is the kernel trace of a profiled run of this
module (`rocprofv3 --kernel-trace --stats -- python -m pytest tests/test_gpu_switches.py -m gpu`); the entry says which
kernel to look for.  tests/test_switch_inventory.py makes sure no switch is left without a test."""
import functools
import os
import re
import sys

import numpy as np
import pytest

import checker as ck
import golden_utils as gu
from oracle import overlap_oracle as oo   # row helpers only
from phasm_amd.overlapper import ExactOverlapper

pytestmark = pytest.mark.gpu

STREAM = {"PHASM_STREAM": "1", "PHASM_STREAM_CUTS": "250,500,750", "PHASM_VERIFY_ORDER": "1"}


@functools.lru_cache(maxsize=None)
def case(name):
    """(reads, min_length, golden rows); name "x_sc" is ladder x soft-masked (8 bits per base, tests/test_bytemode_host.py)."""
    base = name[:-3] if name.endswith("_sc") else name
    _, seqs, m, want = gu.ladder_case(base)
    if name.endswith("_sc"):
        seqs = [s.swapcase() for s in seqs]
    return tuple(seqs), m, want


def _sorted(arr):
    return oo.sort_rows(oo.struct_to_rows(arr))


# ---- entry points: (ov, m) -> [(rows, stats) per call]

def whole(ov, m):
    return [(_sorted(ov.overlaps_array(m)), ov.stats()) for _ in range(2)]


def shards(ov, m):
    out = []
    for _ in range(2):
        parts = [ov.overlaps_shard_array(m, k, 3) for k in range(3)]
        out.append((_sorted(np.concatenate(parts)), ov.stats()))
    return out


def to_host(ov, m, calls=3):
    out = []
    for _ in range(calls):
        ov.invalidate()
        res = ov.overlaps_to_host_result(m)
        out.append((_sorted(res.rows_view()), ov.stats()))
        res.free()
    return out


def cands_into(ov, m):
    """po_candidates_shard_into straight into a caller's buffer, then into one too small (the spare-buffer branch), then
    po_candidates_shard (no destination); expanded, the candidates of every form are the rows."""
    import torch
    from phasm_amd.dist import _result_to_tensor
    dev = torch.device("cuda", 0)
    out = []
    for cap in (1 << 22, 1, None):
        parts, written = [], []
        for k in range(3):
            if cap is None:
                res, w = ov.candidates_result(m, k, 3), False
            else:
                dst = torch.empty((cap, 4), dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                res, w = ov.candidates_result_into(m, k, 3, dst.data_ptr(), cap)
            if w:
                parts.append(dst[:len(res)].clone())
            else:
                parts.append(_result_to_tensor(res, 4, dev))
            written.append(w)
            res.free()
        merged = torch.cat(parts, dim=0).contiguous()
        res = ov.expand_result(merged.data_ptr(), merged.shape[0])
        st = dict(ov.stats(), written=sum(written))
        out.append((_sorted(res.rows()), st))
        res.free()
    return out


def tuples(ov, m):
    from phasm_amd import overlapper
    overlapper._PYT[:] = [False, None]   # (the tuple builder is looked up once per process: look again under this switch)
    try:
        tup = ov.overlaps(m)
        st = dict(ov.stats(), pytuples=overlapper._pytuples() is not None)
    finally:
        overlapper._PYT[:] = [False, None]
    ids = {s: i for i, s in enumerate(ov.ids())}
    rows = np.array([(ids[a], ids[b], s, e, bs, be) for a, b, s, e, bs, be in tup], dtype=np.int64).reshape(-1, 6)
    return [(oo.sort_rows(rows), st)]


# ---- proofs: (switched calls, control calls, switched stderr, control stderr, extra) -> None (assert)

def stat(field, fn, calls=None):
    def proof(sw, ctl, err_sw, err_ctl, extra):
        idx = range(len(sw)) if calls is None else calls
        for i in idx:
            assert fn(sw[i][1][field], ctl[i][1][field]), "%s: call %d switched %r, control %r" % (field, i, sw[i][1][field], ctl[i][1][field])
    proof.what = "po_stats.%s" % field
    return proof


def trace(pattern, fn):
    def proof(sw, ctl, err_sw, err_ctl, extra):
        a, b = len(re.findall(pattern, err_sw, re.M)), len(re.findall(pattern, err_ctl, re.M))
        assert fn(a, b), "trace %r: %d lines with the switch, %d without" % (pattern, a, b)
    proof.what = "stderr %r" % pattern
    return proof


def pieces(n):
    def proof(sw, ctl, err_sw, err_ctl, extra):
        got = [int(x) for x in re.findall(r"^\[stream\] (\d+) pieces queued", err_sw, re.M)]
        ctl_n = [int(x) for x in re.findall(r"^\[stream\] (\d+) pieces queued", err_ctl, re.M)]
        assert got and all(p == n for p in got) and ctl_n and all(p > n for p in ctl_n), (got, ctl_n)
    proof.what = "stderr [stream] pieces queued"
    return proof


def kernel(name):
    def proof(sw, ctl, err_sw, err_ctl, extra):
        pass   # (no in-process signal: the kernel trace of the profiled run shows the launch)
    proof.what = "kernel trace: %s" % name
    proof.kernel_only = True
    return proof


def registered_stores(fn):
    def proof(sw, ctl, err_sw, err_ctl, extra):
        assert fn(extra["pins_sw"], extra["pins_ctl"]), (extra["pins_sw"], extra["pins_ctl"])
    proof.what = "host stores registered with the runtime while the handle is open (po_debug_host_ranges, kind 2)"
    return proof


def never_predicts(sw, ctl, err_sw, err_ctl, extra):
    assert all(st["n_predicted"] == 0 for _, st in sw), [st["n_predicted"] for _, st in sw]
    assert any(st["n_predicted"] > 0 for _, st in ctl), [st["n_predicted"] for _, st in ctl]


never_predicts.what = "po_stats.n_predicted: 0 with the switch, > 0 without"

DIFFERENT = lambda a, b: a != b   # noqa: E731

# (id, environment, input, entry point, proof)
TABLE = [
    ("verify_unstaged_whole_2bit", {"PHASM_VERIFY_STAGED": "0"}, "ladder_varlen", whole, kernel("k_verify_a<2, false, false>")),
    ("verify_unstaged_shards_2bit", {"PHASM_VERIFY_STAGED": "0"}, "ladder_varlen", shards, kernel("k_verify_a<2, true, false>")),
    ("verify_unstaged_streamed", dict(STREAM, PHASM_VERIFY_STAGED="0"), "cfg2_1k", to_host, kernel("k_verify_a<2, false, false, true>")),
    ("verify_unstaged_whole_8bit", {"PHASM_VERIFY_STAGED": "0"}, "ladder_varlen_sc", whole, kernel("k_verify_a<8, false, false>")),
    ("verify_unstaged_shards_8bit", {"PHASM_VERIFY_STAGED": "0"}, "ladder_varlen_sc", shards, kernel("k_verify_a<8, false, false>")),
    ("verify_unstaged_to_host_8bit", {"PHASM_VERIFY_STAGED": "0", "PHASM_HOST_CHUNKS": "3"}, "ladder_cfg2_mini_sc", to_host,
     kernel("k_verify_a<8, false, false>")),
    ("select_kernel_shards", {"PHASM_SELECT_KERNEL": "1"}, "ladder_varlen", shards, kernel("k_select_local")),
    ("select_kernel_streamed", dict(STREAM, PHASM_SELECT_KERNEL="1"), "cfg2_1k", to_host, kernel("k_select_local")),
    ("select_kernel_wide", {"PHASM_SELECT_KERNEL": "1", "PHASM_INDEX": "wide"}, "cfg3_1k", whole, kernel("k_select_local")),
    ("select_kernel_wide_8bit", {"PHASM_SELECT_KERNEL": "1", "PHASM_INDEX": "wide"}, "ladder_varlen_sc", whole, kernel("k_select_local")),
    ("piece_reset", dict(STREAM, PHASM_PIECE_RESET="1"), "cfg2_1k", to_host, kernel("k_call_reset once per piece: 12 launches in 3 calls, 3 without the switch")),
    ("sync_count", dict(STREAM, PHASM_SYNC_COUNT="1"), "cfg2_1k", to_host, never_predicts),
    ("stream_lead2", dict(STREAM, PHASM_STREAM_LEAD2="1", PHASM_INDEX="wide"), "cfg3_1k", to_host, stat("upload_bytes", DIFFERENT, [0])),
    ("late_index", dict(STREAM, PHASM_LATE_INDEX="1"), "cfg2_1k", to_host, stat("upload_bytes", DIFFERENT)),
    ("no_index_reuse_whole", {"PHASM_NO_INDEX_REUSE": "1"}, "ladder_varlen", whole, stat("index_reused", lambda a, b: a == 0 and b == 1, [1])),
    ("no_index_reuse_streamed", dict(STREAM, PHASM_NO_INDEX_REUSE="1"), "cfg2_1k", to_host,
     stat("index_reused", lambda a, b: a == 0 and b == 1)),
    ("stream_max_pieces_2", {"PHASM_STREAM": "1", "PHASM_STREAM_MAX_PIECES": "2", "PHASM_STREAM_TRACE": "1"}, "big_pairs", to_host,
     pieces(2)),
    ("stream_sync", dict(STREAM, PHASM_STREAM_SYNC="1"), "cfg2_1k", to_host, never_predicts),
    ("no_kit_pool", {"PHASM_NO_KIT_POOL": "1", "PHASM_ALLOC_TRACE": "1"}, "ladder_varlen", whole,
     trace(r"^\[init\] streams and events made", lambda a, b: a > b)),
    ("no_pin", {"PHASM_NO_PIN": "1"}, "cfg2_1k", whole, registered_stores(lambda a, b: a == 0 and b > 0)),
    ("no_pool", {"PHASM_NO_POOL": "1", "PHASM_STREAM": "0", "PHASM_ALLOC_TRACE": "1"}, "big_pairs", to_host,
     trace(r"^\[alloc\] result pool", lambda a, b: a == 0 and b > 0)),
    # (a handle that takes a device kit from the pool skips the device start where this acts: no kit for either side)
    ("no_warm", {"PHASM_NO_WARM": "1", "PHASM_NO_KIT_POOL": "1"}, "cfg2_1k", to_host, kernel("k_fill_u32: fewer launches at device start")),
    ("no_pytuples", {"PHASM_NO_PYTUPLES": "1"}, "ladder_varlen", tuples, stat("pytuples", lambda a, b: a is False and b is True)),
]

# Switches with no signal inside the process: neither a statistic, a trace line nor a kernel launch changes.  Their entries
# check rows only and prove nothing about the switch; tests/test_switch_inventory.py lists each of them as an explicit,
# reasoned exemption instead of counting it as covered.  (id, environment, input, entry point, why there is no proof)
ROWS_ONLY = [
    ("compact_sync", {"PHASM_COMPACT_SYNC": "1"}, "ladder_cfg2_mini", cands_into,
     "only makes the host wait for the candidate count before the compaction, which writes to the same places"),
    ("home_spin_0", {"PHASM_HOME_SPIN": "0", "PHASM_HOST_CHUNKS": "2"}, "cfg2_1k", to_host,
     "only makes the host pool's helper threads sleep at once instead of spinning first"),
    ("no_arena", {"PHASM_NO_ARENA": "1", "PHASM_NO_KIT_POOL": "1"}, "ladder_varlen", whole,
     "only gives small device buffers a hipMalloc each instead of a slice of a 64 MB chunk"),
]


def switch_of(env):
    """The switch an entry is about: its first variable that is not part of the entry's setting (streaming, host chunks,
    index flavour, traces, no device kit)."""
    return next(k for k in env if k not in STREAM and k not in ("PHASM_HOST_CHUNKS", "PHASM_INDEX") and not k.endswith("_TRACE"))


def proven_switches():
    """Switches this module shows to act: every TABLE entry's, and PHASM_HOME_THREADS (test_home_threads_in_a_fresh_process)."""
    return {switch_of(env) for _, env, _, _, _ in TABLE} | {"PHASM_HOME_THREADS"}


def rows_only_switches():
    return {switch_of(env) for _, env, _, _, _ in ROWS_ONLY}


@functools.lru_cache(maxsize=None)
def big_pairs():
    """480 strand pairs of 400 kb reads tiled along a random genome with 20 kb overlaps: 48 MB of packed even reads, three
    streamed pieces by default.  Its rows follow from the tiling: read 2k is tile k, read 2k + 1 its reverse complement.
    Tile k's last 20 kb are tile k + 1's first (row 2k -> 2k + 2), so the reverse complement of tile k + 1 ends with the
    first 20 kb of the reverse complement of tile k (row 2k + 3 -> 2k + 1).  Nothing else of 5 kb or more recurs."""
    rng = np.random.default_rng(77)
    step, ln = 380_000, 400_000
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=480 * step + ln - step)].tobytes()
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    seqs = []
    for k in range(480):
        r = genome[k * step:k * step + ln]
        seqs += [r, r.translate(comp)[::-1]]
    o = ln - step
    rows = [(2 * k, 2 * k + 2, step, ln, 0, o) for k in range(479)] + [(2 * k + 3, 2 * k + 1, step, ln, 0, o) for k in range(479)]
    return tuple(seqs), 5000, oo.sort_rows(np.array(rows, dtype=np.int64))


def _run(env, name, entry, monkeypatch, capfd):
    seqs, m, want = big_pairs() if name == "big_pairs" else case(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ov = ExactOverlapper()
    for i, s in enumerate(seqs):
        ov.add_sequence("r%d" % i, s)
    try:
        out = entry(ov, m)
        pins = sum(1 for _, _, kind, live in ck.host_ranges() if kind == 2 and live)
    finally:
        ov.close()
        for k in env:
            monkeypatch.delenv(k)
    err = capfd.readouterr().err
    for i, (rows, st) in enumerate(out):
        ck.assert_same_rows(rows, want, seqs if name != "big_pairs" else None, m, "%s, call %d" % (name, i))
    return out, err, pins


@pytest.mark.parametrize("sid,env,name,entry,proof", TABLE, ids=[t[0] for t in TABLE])
def test_switch(sid, env, name, entry, proof, monkeypatch, capfd):
    if "PHASM_NO_KIT_POOL" in env:   # (a handle closed before leaves its device kit in the pool for the next one)
        ExactOverlapper(device=0).close()
    sw, err_sw, pins_sw = _run(env, name, entry, monkeypatch, capfd)
    if "PHASM_NO_KIT_POOL" in env:
        ExactOverlapper(device=0).close()
    # the same call without the switch (the other variables of the entry kept)
    key = switch_of(env)
    ctl_env = {k: v for k, v in env.items() if k != key}
    ctl, err_ctl, pins_ctl = _run(ctl_env, name, entry, monkeypatch, capfd)
    if env.get("PHASM_STREAM") == "1":
        assert all(st["streamed"] == 1 for _, st in sw + ctl), [st["streamed"] for _, st in sw + ctl]
    if name.endswith("_sc"):
        assert all(st["bits_per_base"] == 8 for _, st in sw), sid
    proof(sw, ctl, err_sw, err_ctl, {"pins_sw": pins_sw, "pins_ctl": pins_ctl})


@pytest.mark.parametrize("sid,env,name,entry,why", ROWS_ONLY, ids=[t[0] for t in ROWS_ONLY])
def test_switch_rows_only(sid, env, name, entry, why, monkeypatch, capfd):
    """Golden rows with a switch that leaves no signal (ROWS_ONLY): the path runs and gives the right rows, no more."""
    if "PHASM_NO_KIT_POOL" in env:
        ExactOverlapper(device=0).close()
    out, _, _ = _run(env, name, entry, monkeypatch, capfd)
    if env.get("PHASM_STREAM") == "1":
        assert all(st["streamed"] == 1 for _, st in out), [st["streamed"] for _, st in out]


def test_every_entry_names_its_proof():
    for sid, env, name, entry, proof in TABLE:
        assert proof.what and switch_of(env).startswith("PHASM_"), sid
    proven = proven_switches()
    for sid, env, name, entry, why in ROWS_ONLY:
        assert why.strip() and switch_of(env) not in proven, sid
    for must in ("PHASM_VERIFY_STAGED", "PHASM_SELECT_KERNEL", "PHASM_PIECE_RESET", "PHASM_SYNC_COUNT",
                 "PHASM_STREAM_LEAD2", "PHASM_LATE_INDEX", "PHASM_NO_INDEX_REUSE", "PHASM_STREAM_MAX_PIECES",
                 "PHASM_STREAM_SYNC", "PHASM_NO_KIT_POOL", "PHASM_NO_PIN", "PHASM_NO_POOL", "PHASM_NO_WARM"):
        assert must in proven, must


_THREADS_CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import golden_utils as gu
from oracle import overlap_oracle as oo
from phasm_amd.overlapper import ExactOverlapper
# the host pool started on its own, before anything brings the GPU runtime (and its threads) up: po_debug_expand_records
# of no records runs through the pool without a device
import ctypes
from phasm_amd import _lib
from phasm_amd._lib import ROW_DTYPE
lib = _lib.load()
before = set(os.listdir("/proc/self/task"))
out = np.zeros(2, dtype=ROW_DTYPE)
lens = np.ones(1, dtype=np.uint32)
assert lib.po_debug_expand_records(None, 0, lens.ctypes.data_as(ctypes.c_void_p), 1, 0, out.ctypes.data_as(ctypes.c_void_p), 0) == 0
added = set(os.listdir("/proc/self/task")) - before
print("THREADS %%d" %% len(added), flush=True)
# golden rows through the same pool
_, seqs, m, want = gu.ladder_case("cfg2_1k")
ov = ExactOverlapper(device=0)
for i, s in enumerate(seqs):
    ov.add_sequence("r%%d" %% i, s)
for _ in range(2):
    res = ov.overlaps_to_host_result(m)
    assert np.array_equal(oo.sort_rows(oo.struct_to_rows(res.rows_view())), want)
    res.free()
assert ov.stats()["home_record_bytes"] > 0
ov.close()
print("ROWS OK")
"""


def test_home_threads_in_a_fresh_process(tmp_path):
    """PHASM_HOME_THREADS is read once, when the process's host pool starts (c_api.hip home::pool): one child per value,
    started by the checker process.  The pool is started by the host-only record expansion before the GPU runtime is up,
    so the threads it adds are the pool's alone: exactly the number asked for.  Golden rows through that pool in each."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "home_threads.py"
    script.write_text(_THREADS_CHILD % {"root": root, "tests": os.path.join(root, "tests")})
    counts = {}
    for n in ("1", "2"):
        env = dict(os.environ, PHASM_HOME_THREADS=n, PHASM_HOST_CHUNKS="2")
        rc, stdout, stderr = ck.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
        assert rc == 0 and "THREADS" in stdout and "ROWS OK" in stdout, stdout[-2000:] + stderr[-3000:]
        counts[n] = int(re.search(r"THREADS (\d+)", stdout).group(1))
    assert counts == {"1": 1, "2": 2}, counts
