"""Evaluation stage of the broadband stream (apvast.enable_evaluation): what can be checked without a GPU -- the method's argument
checks (they run before any library call), the shared checker's unchanged subband messages, the state rows, and the declarations
of the new C ABI entries."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class NoLibrary:
    """stands where the engine would: any use of it is a library call the checks were to come before"""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the argument checks were through")


def bare(mode="broadband", ranks=(1, 2, 3), L=2):
    """an object as far as the argument checks look at it, without an engine"""
    from ap_vast_unofficial_amd.apvast import apvast
    ap = apvast.__new__(apvast)
    ap.__dict__.update(mode=mode, number_of_srcs=L, _ranks=list(ranks), _eng=NoLibrary(), run_A=True, run_B=True,
                       _evaluation=None, _bb_evaluation=None, _bb_eval_hops=0)
    return ap


def test_method_signature():
    from ap_vast_unofficial_amd.apvast import apvast
    p = inspect.signature(apvast.enable_evaluation).parameters
    assert list(p) == ["self", "validation_rir_A", "validation_rir_B", "ranks"] and p["ranks"].default is None


def test_argument_checks_come_before_the_library():
    rv = np.ones((5, 2, 3))
    ap = bare()
    with pytest.raises(ValueError, match="both or neither"):
        ap.enable_evaluation(rv, None)
    with pytest.raises(ValueError, match="both or neither"):
        ap.enable_evaluation(None, rv)
    with pytest.raises(ValueError, match="one shape"):
        ap.enable_evaluation(rv, np.ones((5, 2, 4)))
    with pytest.raises(ValueError, match="one shape"):
        ap.enable_evaluation(np.ones((5, 6)), np.ones((5, 6)))
    with pytest.raises(ValueError, match="L = 2 loudspeakers"):
        ap.enable_evaluation(np.ones((5, 3, 3)), np.ones((5, 3, 3)))
    with pytest.raises(ValueError, match="L = 2 loudspeakers"):
        ap.enable_evaluation(np.ones((0, 2, 3)), np.ones((0, 2, 3)))
    for bad in (np.nan, np.inf):
        nf = rv.copy()
        nf[2, 1, 0] = bad
        with pytest.raises(ValueError, match="must be finite"):
            ap.enable_evaluation(rv, nf)
        with pytest.raises(ValueError, match="must be finite"):
            ap.enable_evaluation(nf, rv)
    with pytest.raises(ValueError, match="Pv <= 20465"):
        ap.enable_evaluation(np.ones((20466, 2, 1)), np.ones((20466, 2, 1)))
    for bad in ([], [0], [4], [2, 1], [1, 1], [1.5], [True], 2, "12"):
        with pytest.raises(ValueError, match="strictly ascending"):
            ap.enable_evaluation(rv, rv, bad)
    # the MATLAB dialect emits the entries of number_of_eigenvectors: a rank between them is not emitted
    m = bare(ranks=(1, 6, 12))
    for bad in ([2], [1, 5], [12, 6], [6, 6], [13]):
        with pytest.raises(ValueError, match=r"ranks the object emits: \[1, 6, 12\]"):
            m.enable_evaluation(rv, rv, bad)
    assert ap._bb_evaluation is None and m._bb_evaluation is None
    for name in ("evaluation_hops", "evaluation_totals", "predicted_pressure", "reset_evaluation"):
        with pytest.raises(RuntimeError, match=r"no evaluation stage.*enable_evaluation\(\)"):
            getattr(ap, name)()


def test_subband_object_and_second_call():
    rv = np.ones((5, 2, 3))
    with pytest.raises(RuntimeError, match="validation_rir_A and validation_rir_B .*to the constructor"):
        bare(mode="subband").enable_evaluation(rv, rv)
    ap = bare()
    ap._bb_evaluation = (rv, rv, [1])
    with pytest.raises(RuntimeError, match="already"):
        ap.enable_evaluation(rv, rv)


def test_accepted_arguments_reach_the_library_once():
    calls = []

    class Recorder:
        def bb_set_evaluation(self, a, b, r):
            calls.append((a, b, r))

    rv = np.arange(30.0).reshape(5, 2, 3)
    ap = bare(ranks=(1, 6, 12))
    ap._eng = Recorder()
    ap.enable_evaluation(rv, rv.astype(np.float32), [6, 12])
    (a, b, r), = calls
    assert a.dtype == b.dtype == np.float64 and a is not rv and r == [6, 12]
    assert ap._eval_dims() == (2, 2, 5, 3)
    ap2 = bare()
    ap2._eng = Recorder()
    ap2.enable_evaluation(rv, rv)
    assert calls[-1][2] == [1, 2, 3]                       # None: every emitted rank


def test_shared_checker_keeps_the_subband_messages():
    from ap_vast_unofficial_amd.apvast import apvast
    rv = np.ones((5, 2, 3))
    chk = apvast._check_evaluation
    assert chk(None, None, None, 2, 2, "subband") is None and chk(None, None, None, 2, 2, "broadband") is None
    with pytest.raises(ValueError, match="evaluation_ranks needs validation_rir_A"):
        chk(None, None, [1], 2, 2, "subband")
    with pytest.raises(ValueError, match="a subband keyword: broadband mode has no evaluation stage"):
        chk(rv, rv, None, 2, 2, "broadband")
    with pytest.raises(ValueError, match="go together: both or neither"):
        chk(rv, None, None, 2, 2, "subband")
    with pytest.raises(ValueError, match=r"must have one shape \(Pv, L, Mv\), got \(5, 2, 3\) and \(5, 2, 4\)"):
        chk(rv, np.ones((5, 2, 4)), None, 2, 2, "subband")
    with pytest.raises(ValueError, match=r"with L = 4 loudspeakers \(the constructor's\) and Pv, Mv >= 1, got \(5, 2, 3\)"):
        chk(rv, rv, None, 4, 2, "subband")
    for bad in ([], [0], [3], [2, 1], [1, 1], [1.5], [True], 2, "12"):
        with pytest.raises(ValueError, match="evaluation_ranks must be None or a strictly ascending list of ranks within 1..number_of_eigenvectors"):
            chk(rv, rv, bad, 2, 2, "subband")
    a, b, r = chk(rv, rv, (np.int64(2),), 2, 2, "subband")
    assert r == [2] and type(r[0]) is int and a is not rv and a.dtype == np.float64


def test_state_rows_follow_the_method():
    from types import SimpleNamespace
    from ap_vast_unofficial_amd.apvast import apvast
    rows = [r for r in apvast._STATE_ROWS if r.key in apvast._EVAL_STATE]
    assert len(rows) == 2
    flags = lambda **kw: [bool(f(SimpleNamespace(**kw))) for r in rows for f in (r.accepts, r.reports or r.accepts)]
    assert not any(flags(mode="broadband", _evaluation=None, _bb_evaluation=None))
    assert not any(flags(mode="broadband", _evaluation=None))
    assert all(flags(mode="broadband", _evaluation=None, _bb_evaluation=(None, None, [1])))
    assert not any(flags(mode="subband", _evaluation=None, _bb_evaluation=(None, None, [1])))
    rv = np.ones((5, 2, 3))
    ap = bare()
    ap._bb_evaluation = (rv, rv, [1, 3])
    shapes = {r.key: r.shape(ap) for r in rows}
    assert shapes == {"evaluation_history": (2, 3, 4, 2), "evaluation_totals": (2, 7, 3)}


def test_abi_declared_and_exported():
    from ap_vast_unofficial_amd import _capi
    text = open(os.path.join(ROOT, "include", "apvast_hip.h")).read()
    assert re.search(r"int\s+apv_bb_set_evaluation\(apv_handle\* h, int32_t Pv, int32_t Mv, const double\* h_rvA, const double\* h_rvB, "
                     r"int32_t n_ranks,\s+const int32_t\* ranks\);", text)
    assert re.search(r"int\s+apv_bb_reset_evaluation\(apv_handle\* h\);", text)
    assert re.search(r"int\s+apv_eval_energies\(apv_handle\* h, const double\* d_p, int32_t Z, int32_t E, int32_t H, int32_t Mv, "
                     r"int32_t n_hops, double\* d_record,\s+double\* d_totals\);", text)
    for name in ("apv_bb_set_evaluation", "apv_bb_reset_evaluation", "apv_eval_energies"):
        assert name in _capi.EXPORTS
    src = inspect.getsource(_capi.load)
    for name in ("apv_bb_set_evaluation", "apv_bb_reset_evaluation", "apv_eval_energies"):
        assert f"lib.{name}.argtypes" in src
    for name in ("bb_set_evaluation", "bb_reset_evaluation", "eval_energies"):
        assert hasattr(_capi.Engine, name)
    mk = open(os.path.join(ROOT, "ap_vast_unofficial_amd", "csrc", "Makefile")).read()
    assert "kernels_bbeval.hip" in mk
    internal = open(os.path.join(ROOT, "ap_vast_unofficial_amd", "csrc", "apv_internal.h")).read()
    assert "apv_launch_bbeval_energies" in internal and "apv_launch_bbeval_advance" in internal
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "apv_bb_set_evaluation" in doc and "apv_eval_energies" in doc
