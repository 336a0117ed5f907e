"""Every PHASM_* environment switch the library reads must be exercised by some test, or be a diagnostic switch named on
the allow-list below with its reason.  A switch that selects a kernel, a row order, a buffer or a sync path is code the
library ships: a new one comes with a test (tests/test_gpu_switches.py is the table for such switches).

tests/test_gpu_switches.py is read through its tables, not its text: a switch counts there only when an entry proves that it
acted.  Its rows-only entries (switches with no signal in the process) count only as the explicit exemptions listed in
ROWS_ONLY_EXEMPT below."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")

# name -> reason.  Only switches that trace or time may stand here.
ALLOWED_UNTESTED = {
    "PHASM_ALLOC_TRACE": "trace only: prints each device / pinned allocation and init step to stderr",
    "PHASM_FASTA_TRACE": "trace only: prints the FASTA ingest steps to stderr",
    "PHASM_HOME_TRACE": "trace only: prints when each piece's rows reach the host",
    "PHASM_STREAM_TRACE": "trace only: prints the streamed step's host-clock marks",
    "PHASM_PHASE_EVENTS": "timing only: which phase events are recorded for the ms_* statistics",
}
# the allow-list is for diagnostics: anything else may not hide there
_DIAGNOSTIC = re.compile(r"_TRACE$|^PHASM_PHASE_EVENTS$")

# switches whose only test checks rows, because nothing in the process shows whether they acted (test_gpu_switches.py
# ROWS_ONLY): name -> why no test can prove more.  Not coverage: an exemption, stated one by one.
ROWS_ONLY_EXEMPT = {
    "PHASM_COMPACT_SYNC": "adds a host wait before the candidate compaction; rows, statistics and kernel launches are unchanged",
    "PHASM_HOME_SPIN": "changes how long host pool threads spin before sleeping; nothing else changes",
    "PHASM_NO_ARENA": "changes how small device buffers are allocated; rows, statistics and kernel launches are unchanged",
}

_READ = re.compile(r"""(?:getenv|environ\.get|environ\[|environ\.setdefault)\(?\s*["'](PHASM_[A-Z0-9_]+)["']""")


def switches_read_by_the_library():
    names = set()
    files = glob.glob(os.path.join(ROOT, "phasm_amd", "csrc", "*")) + glob.glob(os.path.join(ROOT, "phasm_amd", "*.py"))
    for path in files:
        with open(path, encoding="utf-8", errors="replace") as f:
            names.update(_READ.findall(f.read()))
    return names


def test_the_scan_finds_the_known_switches():
    names = switches_read_by_the_library()
    # (a few that are read in different ways: C getenv, os.environ.get, inside an if with an assignment)
    for known in ("PHASM_VERIFY_STAGED", "PHASM_SELECT_KERNEL", "PHASM_HOME_THREADS", "PHASM_LIB", "PHASM_NO_PYTUPLES",
                  "PHASM_STREAM", "PHASM_INDEX"):
        assert known in names, known
    assert len(names) >= 50


def covered_switches():
    """Names a test file (other than this one and the switch table) names as a whole word, plus the switches the switch
    table proves to act."""
    import test_gpu_switches as table
    text = ""
    for path in glob.glob(os.path.join(TESTS, "test_*.py")):
        if os.path.basename(path) not in (os.path.basename(__file__), "test_gpu_switches.py"):
            with open(path, encoding="utf-8") as f:
                text += f.read()
    names = switches_read_by_the_library()
    # a name counts only as a whole word (PHASM_STREAM must not be satisfied by PHASM_STREAM_SYNC)
    return {n for n in names if re.search(r"\b%s\b" % n, text)} | table.proven_switches()


def test_every_path_switch_is_named_by_a_test():
    names = switches_read_by_the_library()
    covered = covered_switches()
    untested = sorted(n for n in names if n not in covered and n not in ALLOWED_UNTESTED and n not in ROWS_ONLY_EXEMPT)
    assert not untested, "switches read by the library that no test proves: %s" % untested


def test_rows_only_exemptions_match_the_switch_table():
    import test_gpu_switches as table
    rows_only = table.rows_only_switches()
    # every rows-only switch is exempted here by name, and nothing is exempted that a test proves or the table lacks
    assert set(ROWS_ONLY_EXEMPT) == rows_only - covered_switches(), (sorted(ROWS_ONLY_EXEMPT), sorted(rows_only))
    names = switches_read_by_the_library()
    for n, reason in ROWS_ONLY_EXEMPT.items():
        assert n in names and reason.strip(), n


def test_allow_list_holds_only_diagnostic_switches_that_exist():
    names = switches_read_by_the_library()
    for n, reason in ALLOWED_UNTESTED.items():
        assert _DIAGNOSTIC.search(n), "%s is not a diagnostic switch and needs a test" % n
        assert n in names, "%s is on the allow-list but the library no longer reads it" % n
        assert reason.strip()
