"""Detectability stage of the subband stream (apvast(..., evaluation_detectability=True)): what can be checked without a GPU --
the keyword, the ABI's declarations, the NumPy helper of tests/detectability_oracle.py (its two orders of summation and the
condition its bound must meet) and evaluation.detectability_metrics."""
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import detectability_oracle as do

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# block, hop, sampling rate, channels of the model: the smallest blocks the tables calibrate at
SIZES = [(96, 24, 48000, 44), (136, 40, 16000, 34), (96, 32, 14000, 32), (192, 96, 3000, 19)]


def tables_of(n, fs):
    from ap_vast_unofficial_amd.perceptual import PerceptualTables
    return PerceptualTables(n, fs, 94.0)


def test_keyword_position_default_and_validation():
    from ap_vast_unofficial_amd.apvast import apvast
    params = inspect.signature(apvast.__init__).parameters
    p = params["evaluation_detectability"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    names = list(params)
    assert names[-1] == "statistics_hops" and names.index("evaluation_detectability") == names.index("evaluation_spectra") + 1
    r = np.zeros((10, 2, 2))
    rv = np.ones((5, 2, 3))
    mk = lambda **kw: apvast(256, r, r, 16, 4, 0, 0, 2, 1.0, 512, 128, perceptual=False, **kw)
    # all of it before the engine is created: none of these needs a GPU or the library
    with pytest.raises(ValueError, match="needs evaluation_spectra=True"):
        mk(evaluation_detectability=True)
    with pytest.raises(ValueError, match="needs evaluation_spectra=True"):
        mk(evaluation_detectability=True, validation_rir_A=rv, validation_rir_B=rv)
    with pytest.raises(ValueError, match="a subband keyword"):
        mk(evaluation_detectability=True, mode="broadband")
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError, match="evaluation_detectability must be a bool"):
            mk(evaluation_detectability=bad, evaluation_spectra=True, validation_rir_A=rv, validation_rir_B=rv)
    assert apvast._check_evaluation_detectability(False, False, "broadband") is False
    assert apvast._check_evaluation_detectability(np.True_, True, "subband") is True


def test_uncalibrated_block_raises_what_the_tables_raise():
    from ap_vast_unofficial_amd.apvast import apvast
    r = np.zeros((10, 2, 2))
    rv = np.ones((5, 2, 3))
    with pytest.raises(ValueError, match="block size too small for the calibration"):
        apvast(32, r, r, 8, 4, 0, 0, 2, 1.0, 128, 16, perceptual=False, validation_rir_A=rv, validation_rir_B=rv,
               evaluation_spectra=True, evaluation_detectability=True)


def test_state_key_and_accessors():
    from ap_vast_unofficial_amd.apvast import apvast
    assert apvast._EVALDETECT_STATE == ("evaluation_detectability",)
    others = (apvast._SB_STATE + apvast._BB_STATE + apvast._LIVE_STATE + apvast._WIN_STATE + apvast._FORGET_STATE + apvast._FIR_STATE
              + apvast._EVAL_STATE + apvast._EVALSPEC_STATE)
    assert not set(apvast._EVALDETECT_STATE) & set(others)
    # get_state and set_state take the key only in subband mode and behind the object's own keyword
    rows = [r for r in apvast._STATE_ROWS if r.key in apvast._EVALDETECT_STATE]
    flags = lambda **kw: [bool(f(SimpleNamespace(**kw))) for r in rows for f in (r.accepts, r.reports or r.accepts)]
    assert len(rows) == len(apvast._EVALDETECT_STATE)
    assert not any(flags(mode="subband", _evaluation_detectability=False))
    assert all(flags(mode="subband", _evaluation_detectability=True))
    assert not any(flags(mode="broadband", _evaluation_detectability=True))
    assert callable(apvast.evaluation_detectability) and callable(apvast.evaluation_detectability_hops)


def test_abi_declared_and_exported():
    from ap_vast_unofficial_amd import _capi
    text = open(os.path.join(ROOT, "include", "apvast_hip.h")).read()
    assert re.search(r"int\s+apv_stream_set_evaluation_detectability\(apv_handle\* h, int32_t n_channels, const double\* h_G2, "
                     r"double Cs, double Ca, double Leff\);", text)
    assert re.search(r"int\s+apv_eval_detect_step\(apv_handle\* h, const void\* d_spec, int32_t N, int32_t Z, int32_t E, int32_t Mv, "
                     r"int32_t n_channels,\s+const double\* h_G2, double Cs, double Ca, double Leff, double\* d_hop, "
                     r"double\* d_totals\);", text)
    assert int(re.search(r"#define APV_ABI_VERSION (\d+)", text).group(1)) == 2 and _capi.ABI_VERSION == 2
    lib = _capi.load()
    for name in ("apv_stream_set_evaluation_detectability", "apv_eval_detect_step"):
        assert name in _capi.EXPORTS and hasattr(lib, name)
    assert inspect.signature(_capi.Engine.__init__).parameters["evaluation_detectability"].default is None
    for name in ("set_evaluation_detectability", "eval_detect_step"):
        assert hasattr(_capi.Engine, name)
    mk = open(os.path.join(ROOT, "ap_vast_unofficial_amd", "csrc", "Makefile")).read()
    assert "kernels_evaldetect.hip" in mk
    internal = open(os.path.join(ROOT, "ap_vast_unofficial_amd", "csrc", "apv_internal.h")).read()
    assert "apv_launch_eval_detect" in internal


@pytest.mark.parametrize("n,h,fs,c", SIZES)
def test_helper_sum_orders_agree(n, h, fs, c):
    """the curve form (the device's order) equals the channel-power form (the reference's evaluateDetectability) to 1e-12"""
    tb = tables_of(n, fs)
    assert tb.n_channels == c
    rng = np.random.default_rng(n + fs)
    for amp, ratio in ((1.0, 0.0), (1e-3, -30.0), (1e-6, -60.0)):
        D, _, T, X = do.white_noise_case(tb, n, rng, amp, ratio)
        D2 = do.detectability_channel_form(tb, T, X, n)
        assert np.all(D > 0) and np.all(np.abs(D - D2) <= 1e-12 * D), (amp, ratio)
    # a silent masker: the threshold in quiet
    X = np.fft.rfft(rng.standard_normal((3, n)), axis=-1)
    Dq = do.detectability(do.curve(tb, None, n), X, n)
    assert np.all(np.abs(Dq - do.detectability_channel_form(tb, None, X, n)) <= 1e-12 * Dq)
    assert np.all(np.abs(Dq - do.detectability(do.curve(tb, np.zeros_like(X), n), X, n)) <= 1e-15 * Dq)


@pytest.mark.parametrize("n,h,fs,c", SIZES)
def test_helper_bound_stays_far_below_the_value(n, h, fs, c):
    """the condition every GPU test asserts of its own data: the bound is below 1e-10 of the value, so it cannot hide a failure.
    Windowed white noise over amplitudes 1e-6 .. 1 and disturbance-to-masker ratios -60 .. 0 dB"""
    tb = tables_of(n, fs)
    rng = np.random.default_rng(7 * n + fs)
    worst = 0.0
    for amp in (1e-6, 1e-4, 1e-2, 1.0):
        for ratio in (-60.0, -40.0, -20.0, 0.0):
            D, bound, _, _ = do.white_noise_case(tb, n, rng, amp, ratio)
            worst = max(worst, float((bound / D).max()))
            assert np.all(bound < 1e-10 * D), (amp, ratio, worst)
            assert np.all(do.bound_given(n // 2 + 1, c, D) <= bound)
    print(f"N={n} Fs={fs}: largest bound / D {worst:.3e}")


def test_model_constants_agree_with_the_tables():
    """what the 4e-6 cross-check of the GPU stream test rests on"""
    from oracle.perceptual import Model
    for n, h, fs, c in SIZES:
        tb, m = tables_of(n, fs), Model(n, fs)
        ot = do.from_model(m)
        assert ot.G2.shape == tb.G2.shape == (n // 2 + 1, c)
        assert abs(ot.Cs / tb.Cs - 1) < 1e-6 and abs(ot.Ca / tb.Ca - 1) < 1e-6 and ot.Leff == tb.Leff
        # the helper's curve is Model.squared_weighting_curve on the scaled spectrum
        S = np.fft.rfft(np.random.default_rng(n).standard_normal(n))
        w2 = np.asarray(do.curve(ot, S, n), dtype=np.float64)
        assert np.allclose(w2, m.squared_weighting_curve(np.sqrt(2) / n * S), rtol=1e-12, atol=0)


def test_detectability_metrics():
    from ap_vast_unofficial_amd.evaluation import detectability_metrics
    tot = {"error": np.array([[[2.0, 4.0], [8.0, 0.0]]]), "leak": np.array([[[1.0, 1.0], [0.0, 6.0]]]),
           "error_max": np.zeros((1, 2, 2)), "leak_max": np.zeros((1, 2, 2)),
           "error_audible": np.array([[[1, 3], [4, 0]]]), "leak_audible": np.array([[[0, 0], [0, 2]]]), "hops": 4}
    m = detectability_metrics(tot)
    assert sorted(m) == ["error_audible_share", "error_mean", "leak_audible_share", "leak_mean"]
    assert np.array_equal(m["error_mean"], [[0.75, 1.0]]) and np.array_equal(m["leak_mean"], [[0.25, 0.75]])
    assert np.array_equal(m["error_audible_share"], [[0.5, 0.5]]) and np.array_equal(m["leak_audible_share"], [[0.0, 0.25]])
    with pytest.raises(ValueError):
        detectability_metrics(dict(tot, hops=0))
