"""Per-bin evaluation spectra of the broadband stream (apvast.enable_evaluation_spectra): what can be checked without a GPU -- the
method's signature and its refusals (they come before any library call), the accessor's message, the two state rows, and the
declarations of the new C ABI entries."""
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from test_cpu_broadband_evaluation import ROOT, NoLibrary, bare


def test_method_signature():
    from ap_vast_unofficial_amd.apvast import apvast
    assert list(inspect.signature(apvast.enable_evaluation_spectra).parameters) == ["self"]
    # the pinned ones stay
    p = inspect.signature(apvast.enable_evaluation).parameters
    assert list(p) == ["self", "validation_rir_A", "validation_rir_B", "ranks"]


def test_refusals_come_before_the_library():
    rv = np.ones((5, 2, 3))
    sub = bare(mode="subband")
    sub._bb_evaluation = (rv, rv, [1])
    with pytest.raises(RuntimeError, match=r"evaluation_spectra=True to the constructor"):
        sub.enable_evaluation_spectra()
    ap = bare()
    with pytest.raises(RuntimeError, match=r"after enable_evaluation\(\)"):
        ap.enable_evaluation_spectra()
    ap._bb_evaluation = (rv, rv, [1])
    ap._bb_evaluation_spectra = True
    with pytest.raises(RuntimeError, match="already"):
        ap.enable_evaluation_spectra()
    assert isinstance(ap._eng, NoLibrary) and not sub.__dict__.get("_bb_evaluation_spectra")


def test_accepted_call_reaches_the_library_once():
    calls = []

    class Recorder:
        def bb_set_evaluation_spectra(self):
            calls.append("set")

    rv = np.ones((5, 2, 3))
    ap = bare()
    ap._bb_evaluation = (rv, rv, [1, 3])
    ap._eng = Recorder()
    assert not ap.__dict__.get("_bb_evaluation_spectra")
    ap.enable_evaluation_spectra()
    assert calls == ["set"] and ap._bb_evaluation_spectra is True
    with pytest.raises(RuntimeError, match="already"):
        ap.enable_evaluation_spectra()
    assert calls == ["set"]
    ap._hops = 0
    assert ap.evaluation_spectra() is None                  # no hop since the switch, and no library call to find that out


def test_accessor_names_the_method_in_broadband_mode():
    rv = np.ones((5, 2, 3))
    ap = bare()
    with pytest.raises(RuntimeError, match=r"no evaluation stage.*enable_evaluation\(\)"):
        ap.evaluation_spectra()
    ap._bb_evaluation = (rv, rv, [1])
    with pytest.raises(RuntimeError, match=r"no evaluation spectra: call enable_evaluation_spectra\(\)"):
        ap.evaluation_spectra()
    # a stray subband attribute does not switch the broadband accessor on
    ap._evaluation_spectra = True
    with pytest.raises(RuntimeError, match=r"enable_evaluation_spectra\(\)"):
        ap.evaluation_spectra()
    sub = bare(mode="subband")
    sub._evaluation = (rv, rv, [1])
    with pytest.raises(RuntimeError, match=r"no evaluation spectra: pass evaluation_spectra=True$"):
        sub.evaluation_spectra()


def test_state_rows_follow_the_method():
    from ap_vast_unofficial_amd.apvast import apvast
    rows = [r for r in apvast._STATE_ROWS if r.key in apvast._EVALSPEC_STATE]
    assert [r.key for r in rows] == ["evaluation_spectra", "evaluation_ring"]
    flags = lambda **kw: [bool(f(SimpleNamespace(**kw))) for r in rows for f in (r.accepts, r.reports or r.accepts)]
    stage = (None, None, [1])
    assert all(flags(mode="broadband", _evaluation=None, _bb_evaluation=stage, _bb_evaluation_spectra=True))
    assert not any(flags(mode="broadband", _evaluation=None, _bb_evaluation=stage, _bb_evaluation_spectra=False))
    assert not any(flags(mode="broadband", _evaluation=None, _bb_evaluation=stage))
    assert not any(flags(mode="broadband", _evaluation=None, _bb_evaluation=None, _bb_evaluation_spectra=True))
    assert not any(flags(mode="broadband", _evaluation=None, _bb_evaluation=None))
    assert not any(flags(mode="broadband", _evaluation_spectra=True))
    assert not any(flags(mode="subband", _evaluation=None, _evaluation_spectra=False, _bb_evaluation=stage, _bb_evaluation_spectra=True))
    # the subband rows are what they were
    assert all(flags(mode="subband", _evaluation=stage, _evaluation_spectra=True))
    assert not any(flags(mode="subband", _evaluation=stage, _evaluation_spectra=False))
    rv = np.ones((5, 2, 3))
    ap = bare()
    ap._bb_evaluation = (rv, rv, [1, 3])
    ap._bb_evaluation_spectra = True
    ap.block_size, ap._K = 32, 17
    assert {r.key: r.shape(ap) for r in rows} == {"evaluation_spectra": (2, 7, 17, 3), "evaluation_ring": (2, 5, 3, 32)}
    # the key set of the class is unchanged
    assert apvast._EVALSPEC_STATE == ("evaluation_spectra", "evaluation_ring")


def test_abi_declared_and_exported():
    from ap_vast_unofficial_amd import _capi
    text = open(os.path.join(ROOT, "include", "apvast_hip.h")).read()
    assert re.search(r"int\s+apv_bb_set_evaluation_spectra\(apv_handle\* h, int32_t on\);", text)
    assert re.search(r"int\s+apv_eval_spectra_hops\(apv_handle\* h, const double\* d_pressure, double\* d_tail, int32_t N, int32_t H, "
                     r"int32_t Z, int32_t E,\s+int32_t Mv, int32_t n_hops, int32_t hops_per_launch, double\* d_totals\);", text)
    assert re.search(r"#define\s+APV_ABI_VERSION\s+2\b", text)
    names = ("apv_bb_set_evaluation_spectra", "apv_eval_spectra_hops")
    src = inspect.getsource(_capi.load)
    for name in names:
        assert name in _capi.EXPORTS
        assert f"lib.{name}.argtypes" in src
    for name in ("bb_set_evaluation_spectra", "eval_spectra_hops"):
        assert hasattr(_capi.Engine, name)
    p = inspect.signature(_capi.Engine.eval_spectra_hops).parameters
    assert list(p) == ["self", "p", "tail", "N", "H", "totals", "hops_per_launch"]
    assert p["totals"].default is None and p["hops_per_launch"].default == 0
    mk = open(os.path.join(ROOT, "ap_vast_unofficial_amd", "csrc", "Makefile")).read()
    assert "kernels_bbevalspec.hip" in mk
    internal = open(os.path.join(ROOT, "ap_vast_unofficial_amd", "csrc", "apv_internal.h")).read()
    assert "apv_launch_bbspec_hops" in internal and "APV_BBSPEC_SCRATCH_BYTES" in internal
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "apv_bb_set_evaluation_spectra" in doc and "apv_eval_spectra_hops" in doc
