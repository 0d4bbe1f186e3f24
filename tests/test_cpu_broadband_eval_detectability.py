"""Detectability stage of the broadband stream (apvast.enable_evaluation_detectability): what can be checked without a GPU -- the
method's signature and its refusals (they come before any library call), the accessors' messages, the state row, the
declarations and exports of the new C ABI entries, and the metrics on a broadband-shaped dict."""
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from test_cpu_broadband_evaluation import ROOT, NoLibrary, bare


def test_method_signature():
    from ap_vast_unofficial_amd.apvast import apvast
    assert list(inspect.signature(apvast.enable_evaluation_detectability).parameters) == ["self"]
    # the pinned ones stay
    assert list(inspect.signature(apvast.enable_evaluation_spectra).parameters) == ["self"]
    assert inspect.signature(apvast.__init__).parameters["evaluation_detectability"].default is False
    with pytest.raises(ValueError, match="evaluation_detectability is a subband keyword: broadband mode has no evaluation stage"):
        apvast._check_evaluation_detectability(True, False, "broadband")


def test_refusals_come_before_the_library():
    rv = np.ones((5, 2, 3))
    sub = bare(mode="subband")
    sub._bb_evaluation, sub._bb_evaluation_spectra = (rv, rv, [1]), True
    with pytest.raises(RuntimeError, match=r"evaluation_detectability=True to the constructor"):
        sub.enable_evaluation_detectability()
    ap = bare()
    with pytest.raises(RuntimeError, match=r"after enable_evaluation_spectra\(\)"):
        ap.enable_evaluation_detectability()
    ap._bb_evaluation = (rv, rv, [1])
    with pytest.raises(RuntimeError, match=r"after enable_evaluation_spectra\(\)"):
        ap.enable_evaluation_detectability()
    ap._bb_evaluation_spectra = True
    ap._bb_evaluation_detectability = True
    with pytest.raises(RuntimeError, match="already"):
        ap.enable_evaluation_detectability()
    assert isinstance(ap._eng, NoLibrary) and not sub.__dict__.get("_bb_evaluation_detectability")


class Recorder:
    def __init__(self):
        self.calls = []

    def bb_set_evaluation_detectability(self, tables):
        self.calls.append(tables)


def switchable(block_size, sampling_rate, **kw):
    rv = np.ones((5, 2, 3))
    ap = bare()
    ap.__dict__.update(_bb_evaluation=(rv, rv, [1, 3]), _bb_evaluation_spectra=True, _eng=Recorder(), block_size=block_size,
                       sampling_rate=sampling_rate, _fullscale_db_spl=94.0, perceptual=False, detectability_model=None, **kw)
    return ap


def test_accepted_call_reaches_the_library_once():
    from ap_vast_unofficial_amd.perceptual import PerceptualTables
    ap = switchable(96, 48000)
    ap.enable_evaluation_detectability()
    tb = ap.detectability_model
    assert ap._eng.calls == [tb] and isinstance(tb, PerceptualTables) and tb.G2.shape == (49, 44)
    assert ap._bb_evaluation_detectability is True and ap._detect_hops == 0
    with pytest.raises(RuntimeError, match="already"):
        ap.enable_evaluation_detectability()
    assert len(ap._eng.calls) == 1
    ap._hops = 0
    assert ap.evaluation_detectability() is None and ap.evaluation_detectability_hops() is None
    ap._hops = 3                                             # hops before the switch, none since: still no library call
    assert ap.evaluation_detectability() is None and ap.evaluation_detectability_hops() is None
    # with the design weighting on, the object's own tables are the ones that go down
    model = PerceptualTables(96, 48000, 94.0)
    ap = switchable(96, 48000, model=model)
    ap.perceptual = True
    ap.enable_evaluation_detectability()
    assert ap._eng.calls == [model] and ap.detectability_model is model


@pytest.mark.parametrize("n,fs,exc", [(32, 8000, ValueError), (64, 48000, RuntimeError)])
def test_uncalibrated_block_raises_what_the_tables_raise(n, fs, exc):
    ap = switchable(n, fs)
    with pytest.raises(exc):
        ap.enable_evaluation_detectability()
    assert ap._eng.calls == [] and ap.detectability_model is None and not ap.__dict__.get("_bb_evaluation_detectability")


def test_accessors_name_the_method_in_broadband_mode():
    rv = np.ones((5, 2, 3))
    ap = bare()
    for f in (ap.evaluation_detectability, ap.evaluation_detectability_hops):
        with pytest.raises(RuntimeError, match=r"no evaluation stage.*enable_evaluation\(\)"):
            f()
    ap._bb_evaluation, ap._bb_evaluation_spectra = (rv, rv, [1]), True
    ap._evaluation_detectability = True                      # a stray subband attribute does not switch the broadband accessors on
    for f in (ap.evaluation_detectability, ap.evaluation_detectability_hops):
        with pytest.raises(RuntimeError, match=r"no detectabilities: call enable_evaluation_detectability\(\)"):
            f()
    sub = bare(mode="subband")
    sub._evaluation = (rv, rv, [1])
    sub._bb_evaluation_detectability = True
    with pytest.raises(RuntimeError, match=r"no detectabilities: pass evaluation_detectability=True$"):
        sub.evaluation_detectability()


def test_state_row_follows_the_method():
    from ap_vast_unofficial_amd.apvast import apvast
    rows = [r for r in apvast._STATE_ROWS if r.key in apvast._EVALDETECT_STATE]
    assert [r.key for r in rows] == ["evaluation_detectability"]
    flags = lambda **kw: [bool(f(SimpleNamespace(**kw))) for r in rows for f in (r.accepts, r.reports or r.accepts)]
    stage = (None, None, [1])
    on = dict(mode="broadband", _evaluation=None, _bb_evaluation=stage, _bb_evaluation_spectra=True, _bb_evaluation_detectability=True)
    assert all(flags(**on))
    for off in ("_bb_evaluation_spectra", "_bb_evaluation_detectability"):
        assert not any(flags(**dict(on, **{off: False})))
        assert not any(flags(**{k: v for k, v in on.items() if k != off}))
    assert not any(flags(**dict(on, _bb_evaluation=None)))
    assert not any(flags(mode="broadband", _evaluation_detectability=True))
    assert not any(flags(**dict(on, mode="subband", _evaluation_detectability=False)))
    # the subband row is what it was
    assert all(flags(mode="subband", _evaluation_detectability=True))
    assert not any(flags(mode="subband", _evaluation_detectability=False))
    rv = np.ones((5, 2, 3))
    ap = bare()
    ap.__dict__.update(_bb_evaluation=(rv, rv, [1, 3]), _bb_evaluation_spectra=True, _bb_evaluation_detectability=True)
    assert {r.key: r.shape(ap) for r in rows} == {"evaluation_detectability": (2, 13, 3)}
    assert apvast._EVALDETECT_STATE == ("evaluation_detectability",)


def test_abi_declared_and_exported():
    from ap_vast_unofficial_amd import _capi
    text = open(os.path.join(ROOT, "include", "apvast_hip.h")).read()
    assert re.search(r"int\s+apv_bb_set_evaluation_detectability\(apv_handle\* h, int32_t n_channels, const double\* h_G2, "
                     r"double Cs, double Ca, double Leff\);", text)
    assert re.search(r"int\s+apv_eval_detect_hops\(apv_handle\* h, const void\* d_spec, int32_t n_hops, int32_t hops_per_launch, "
                     r"int32_t N, int32_t Z, int32_t E,\s+int32_t Mv, int32_t n_channels, const double\* h_G2, double Cs, double Ca, "
                     r"double Leff, double\* d_hops,\s+double\* d_totals\);", text)
    assert re.search(r"#define\s+APV_ABI_VERSION\s+2\b", text) and _capi.ABI_VERSION == 2
    lib = _capi.load()
    src = inspect.getsource(_capi.load)
    for name in ("apv_bb_set_evaluation_detectability", "apv_eval_detect_hops"):
        assert name in _capi.EXPORTS and hasattr(lib, name)
        assert f"lib.{name}.argtypes" in src
    for name in ("bb_set_evaluation_detectability", "eval_detect_hops"):
        assert hasattr(_capi.Engine, name)
    p = inspect.signature(_capi.Engine.eval_detect_hops).parameters
    assert list(p) == ["self", "spec", "tables", "Z", "E", "totals", "hops_per_launch"]
    assert p["totals"].default is None and p["hops_per_launch"].default is None
    internal = open(os.path.join(ROOT, "ap_vast_unofficial_amd", "csrc", "apv_internal.h")).read()
    assert "apv_launch_eval_detect_hops" in internal and "BbSpecDetectArgs" in internal
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "apv_bb_set_evaluation_detectability" in doc and "apv_eval_detect_hops" in doc


def test_detectability_metrics_on_a_broadband_dict():
    """what evaluation_detectability() returns after 4 hops of a broadband object with Z = 2, E = 2, Mv = 3"""
    from ap_vast_unofficial_amd.evaluation import detectability_metrics
    rng = np.random.default_rng(3)
    tot = {"hops": 4}
    for key in ("error", "leak"):
        tot[key] = rng.random((2, 2, 3)) * 8
        tot[key + "_max"] = tot[key] / 2
        tot[key + "_audible"] = rng.integers(0, 5, (2, 2, 3)).astype(np.int64)
    m = detectability_metrics(tot)
    assert sorted(m) == ["error_audible_share", "error_mean", "leak_audible_share", "leak_mean"]
    for key in ("error", "leak"):
        assert m[key + "_mean"].shape == m[key + "_audible_share"].shape == (2, 2)
        assert np.allclose(m[key + "_mean"], tot[key].mean(axis=-1) / 4, rtol=1e-15)
        assert np.allclose(m[key + "_audible_share"], tot[key + "_audible"].mean(axis=-1) / 4, rtol=1e-15)
        assert np.all(m[key + "_audible_share"] <= 1.0)
    with pytest.raises(ValueError):
        detectability_metrics(dict(tot, hops=0))
