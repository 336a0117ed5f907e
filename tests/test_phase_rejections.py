"""What a rejected po_phase_branch call says and leaves behind: every PO_ERR_INVALID path with its sentence written out, the
outputs untouched -- all of them checked on the host before the device is touched, so they are held here without a GPU; a
VALID call without a GPU returns PO_ERR_HIP."""
import ctypes

import numpy as np
import pytest

import phase_utils as pu
from phasm_amd import _lib
from phasm_amd.overlapper import ExactOverlapper
from test_components_rejections import FILL, _have_gpu

NAME = "po_phase_branch: "


def valid():
    return next(c for c in pu.load_golden()["cases"] if c["name"] == "nb31_r2")


def phase_call(ov, case, want_count=True, want_params=True, drop=(), n_levels=0, **over):
    """The raw call on the arrays of ``case`` with the sizes overridden by ``over`` and the arrays named in ``drop`` NULL."""
    lib = _lib.load()
    size = dict(ploidy=case["k"], n_paths=case["P"], n_cands=case["C"], n_reads=case["R"], n_b=case["n_b"], threshold=case["threshold"],
                reserved=0, reserved2=0)
    size.update(over)
    dtypes = dict(overlap_max=np.int32, aln_a0=np.int32, aln_a1=np.int32)
    arrays = {k: np.asarray(case[k], dtype=dtypes.get(k, np.uint32)) for k in pu.INPUT_KEYS}
    arrays["levels"] = np.full(max(n_levels, 1), -1.0)
    prm = _lib.PoPhaseParams(size["ploidy"], size["n_paths"], size["n_cands"], size["n_reads"], size["n_b"], case["start"], case["min_span"],
                             int(n_levels > 0), 5, n_levels, size["threshold"], size["reserved"], size["reserved2"])
    inp = _lib.PoPhaseInput(*[None if k in drop or not len(arrays[k]) else arrays[k].ctypes.data for k in pu.INPUT_KEYS + ("levels",)])
    bufs = [np.full(64 * 8, FILL, dtype=np.uint8) for _ in range(4)]
    n = ctypes.c_uint64(77)
    status = lib.po_phase_branch(ov._h, ctypes.byref(prm) if want_params else None, ctypes.byref(inp),
                                 *[b.ctypes.data_as(ctypes.c_void_p) for b in bufs[:3]], 64, bufs[3].ctypes.data_as(ctypes.c_void_p),
                                 ctypes.byref(n) if want_count else None)
    return status, lib.po_last_error(ov._h).decode(), bufs, n.value


def phase_rejected(ov, case, message, want_count=True, **kw):
    status, said, bufs, n = phase_call(ov, case, want_count=want_count, **kw)
    assert status == _lib.PO_ERR_INVALID and said == message, said
    assert all((b == FILL).all() for b in bufs)
    assert n == (0 if want_count else 77)


def test_phase_checks_in_front_of_the_device_keep_their_sentences():
    ov, case = ExactOverlapper(), valid()
    phase_rejected(ov, case, NAME + "no room for the number of entries", want_count=False)
    phase_rejected(ov, case, NAME + "no parameters", want_params=False)
    phase_rejected(ov, case, NAME + "bad parameters", reserved=1)
    phase_rejected(ov, case, NAME + "bad parameters", reserved2=7)
    phase_rejected(ov, case, NAME + "bad parameters", threshold=-0.5)
    phase_rejected(ov, case, NAME + "bad parameters", threshold=float("nan"))
    phase_rejected(ov, case, NAME + "bad parameters", n_levels=1025)
    phase_rejected(ov, case, NAME + "the ploidy must be 1 to 8", ploidy=0)
    phase_rejected(ov, case, NAME + "the ploidy must be 1 to 8", ploidy=9)
    phase_rejected(ov, case, NAME + "the number of paths must be 1 to 64", n_paths=0)
    phase_rejected(ov, case, NAME + "the number of paths must be 1 to 64", n_paths=65)
    phase_rejected(ov, case, NAME + "there must be at least one candidate set", n_cands=0)
    phase_rejected(ov, case, NAME + "too many extensions for one call", n_paths=64, ploidy=8)            # P^k alone
    phase_rejected(ov, case, NAME + "too many extensions for one call", n_cands=2 ** 29)                 # C * P^k = 2^31
    for key in ("overlap_max", "aln_off", "path_off", "set_off", "aln_b", "aln_a0", "aln_a1", "path_ids", "set_ids"):
        phase_rejected(ov, case, NAME + "an input array is missing", drop=(key,))
    phase_rejected(ov, case, NAME + "an input array is missing", drop=("levels",), n_levels=2)
    for key, what in (("aln_off", "alignments"), ("path_off", "paths"), ("set_off", "read sets")):
        bad = dict(case)
        bad[key] = list(case[key])
        bad[key][0] = 1
        phase_rejected(ov, bad, NAME + "the offsets of the %s do not start at 0 or decrease" % what)
        bad[key] = list(case[key])
        bad[key][-1] = bad[key][-2] - 1 if bad[key][-2] else 0xFFFFFFFF
        if bad[key][-2]:
            phase_rejected(ov, bad, NAME + "the offsets of the %s do not start at 0 or decrease" % what)
    for key in ("aln_b", "path_ids", "set_ids"):
        bad = dict(case)
        bad[key] = list(case[key])
        bad[key][-1] = case["n_b"]
        phase_rejected(ov, bad, NAME + "a local read id is not below n_b")
    phase_rejected(ov, case, NAME + "a local read id is not below n_b", n_b=1)
    lib = _lib.load()
    n = ctypes.c_uint64()
    assert lib.po_phase_branch(None, None, None, None, None, None, 0, None, ctypes.byref(n)) == _lib.PO_ERR_INVALID
    st = _lib.PoPhaseStats()
    assert lib.po_get_phase_stats(ov._h, None) == _lib.PO_ERR_INVALID
    assert lib.po_get_phase_stats(ov._h, ctypes.byref(st)) == _lib.PO_OK and st.n_extensions == 0 and st.n_kept == 0
    assert ctypes.sizeof(_lib.PoPhaseParams) == 56 and ctypes.sizeof(_lib.PoPhaseInput) == 80 and ctypes.sizeof(_lib.PoPhaseStats) == 192
    with pytest.raises(ValueError, match="lengths its sizes give"):
        b = pu.bubble_of(case)
        b.n_reads += 1
        ov.phase_branch(b, False)
    with pytest.raises(ValueError, match="32 bits"):
        ov.phase_branch(pu.bubble_of(case), False, min_spanning_reads=-1)
    with pytest.raises(ValueError, match="ploidy must be 1 to 8"):
        b = pu.bubble_of(case)
        b.ploidy, b.n_cands = 16, 1
        b.set_off = np.zeros(17, dtype=np.uint32)
        b.set_ids = b.set_ids[:0]
        ov.phase_branch(b, False)
    ov.close()


@pytest.mark.skipif(_have_gpu(), reason="checks the no-GPU failure mode")
def test_a_valid_call_fails_loudly_without_a_gpu():
    ov, case = ExactOverlapper(), valid()
    status, said, bufs, n = phase_call(ov, case)
    assert status == _lib.PO_ERR_HIP and "no HIP device" in said and n == 0
    assert all((b == FILL).all() for b in bufs)
    with pytest.raises(Exception, match="no HIP device"):
        ov.phase_branch(pu.bubble_of(case), False)
    ov.close()
