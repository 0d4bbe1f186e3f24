"""Per-bin evaluation spectra (apvast(..., evaluation_spectra=True)): what can be checked without a GPU -- the two host functions
evaluation.spectral_metrics and evaluation.third_octave_bands, the keyword's validation (it runs before any engine exists), the
state keys and the C ABI's declarations."""
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_spectra(Z=2, E=3, Mv=5, K=17, seed=0):
    rng = np.random.default_rng(seed)
    return {"bright": rng.random((Z, E, Mv, K)) + 0.1, "dark": rng.random((Z, E, Mv, K)) + 0.1,
            "error": rng.random((Z, E, Mv, K)) + 0.1, "target": rng.random((Z, Mv, K)) + 0.1}


def test_spectral_metrics_per_bin():
    from ap_vast_unofficial_amd.evaluation import spectral_metrics
    s = random_spectra()
    m = spectral_metrics(s)
    assert m["contrast_db"].shape == m["nmse"].shape == (2, 3, 17)
    c = 10 * np.log10(s["bright"].sum(axis=2) / s["dark"].sum(axis=2))
    n = s["error"].sum(axis=2) / s["target"].sum(axis=1)[:, None, :]
    assert np.allclose(m["contrast_db"], c, rtol=1e-13, atol=0) and np.allclose(m["nmse"], n, rtol=1e-13, atol=0)


def test_spectral_metrics_one_band_is_the_weighted_ratio():
    from ap_vast_unofficial_amd.evaluation import spectral_metrics
    s = random_spectra(K=17)
    ck = np.full(17, 2.0)
    ck[0] = ck[16] = 1.0
    m = spectral_metrics(s, bands=[(0, 17)])
    assert m["contrast_db"].shape == m["nmse"].shape == (2, 3, 1)
    c = 10 * np.log10((s["bright"].sum(axis=2) * ck).sum(axis=-1) / (s["dark"].sum(axis=2) * ck).sum(axis=-1))
    n = (s["error"].sum(axis=2) * ck).sum(axis=-1) / (s["target"].sum(axis=1) * ck).sum(axis=-1)[:, None]
    assert np.allclose(m["contrast_db"][..., 0], c, rtol=1e-13, atol=0) and np.allclose(m["nmse"][..., 0], n, rtol=1e-13, atol=0)
    # two bands that split the bins: inner bins alone carry weight 2, which cancels in the ratios
    m2 = spectral_metrics(s, bands=[(1, 4), (4, 16)])
    n2 = s["error"].sum(axis=2)[..., 1:4].sum(axis=-1) / s["target"].sum(axis=1)[..., 1:4].sum(axis=-1)[:, None]
    assert m2["nmse"].shape == (2, 3, 2) and np.allclose(m2["nmse"][..., 0], n2, rtol=1e-13, atol=0)


def test_spectral_metrics_vanishing_target_at_one_microphone():
    from ap_vast_unofficial_amd.evaluation import spectral_metrics
    s = random_spectra()
    s["target"][:, 2, 5] = 0.0                           # one microphone's target vanishes in bin 5, the sum does not
    m = spectral_metrics(s)
    assert np.isfinite(m["nmse"]).all()
    assert np.allclose(m["nmse"][:, :, 5], s["error"][..., 5].sum(axis=2) / s["target"][..., 5].sum(axis=1)[:, None], rtol=1e-13, atol=0)
    assert np.isfinite(spectral_metrics(s, bands=[(4, 7)])["nmse"]).all()


@pytest.mark.parametrize("bands", [[], [(3, 3)], [(5, 2)], [(-1, 4)], [(0, 18)], [(0.0, 4)], [(True, 4)], [(1, 2, 3)], 7, [5]])
def test_spectral_metrics_bad_bands(bands):
    from ap_vast_unofficial_amd.evaluation import spectral_metrics
    with pytest.raises(ValueError):
        spectral_metrics(random_spectra(), bands=bands)


def test_third_octave_bands():
    from ap_vast_unofficial_amd.evaluation import spectral_metrics, third_octave_bands
    fs, N = 48000, 2048
    K = N // 2 + 1
    centres, bands = third_octave_bands(fs, N)
    assert len(centres) == len(bands) > 20
    assert all(isinstance(k0, int) and isinstance(k1, int) and 0 <= k0 < k1 <= K for k0, k1 in bands)
    assert all(bands[i][1] <= bands[i + 1][0] for i in range(len(bands) - 1))          # ascending, no overlap
    ratio = centres[1:] / centres[:-1]
    steps = np.round(3 * np.log2(ratio))
    assert np.all(steps >= 1) and np.allclose(ratio, 2.0 ** (steps / 3), rtol=1e-12, atol=0)
    dense = centres >= 400.0                             # from here on every band holds a bin: neighbours are 2^(1/3) apart
    assert np.all(steps[dense[:-1]] == 1)
    i = int(np.argmin(np.abs(centres - 1000.0)))
    assert abs(centres[i] - 1000.0) < 1e-9
    f = np.arange(K) * fs / N
    inside = np.nonzero((f >= 1000.0 * 2 ** (-1 / 6)) & (f < 1000.0 * 2 ** (1 / 6)))[0]
    assert bands[i] == (int(inside[0]), int(inside[-1]) + 1)
    for fc, (k0, k1) in zip(centres, bands):             # every band: exactly the bins inside its edges
        assert np.all(f[k0:k1] >= fc * 2 ** (-1 / 6) * (1 - 1e-12)) and np.all(f[k0:k1] < fc * 2 ** (1 / 6) * (1 + 1e-12))
    c2, b2 = third_octave_bands(fs, N, f_min=200.0, f_max=4000.0)
    assert c2[0] >= 200.0 and c2[-1] <= 4000.0 and len(c2) == len(b2) == 13
    assert spectral_metrics(random_spectra(K=K), bands=bands)["nmse"].shape == (2, 3, len(bands))
    with pytest.raises(ValueError):
        third_octave_bands(fs, 255)
    with pytest.raises(ValueError):
        third_octave_bands(fs, N, f_min=0.0)


def test_keyword_signature_and_validation():
    from ap_vast_unofficial_amd.apvast import apvast
    p = inspect.signature(apvast).parameters["evaluation_spectra"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    r = np.zeros((10, 2, 2))
    rv = np.ones((5, 2, 3))
    mk = lambda **kw: apvast(256, r, r, 16, 4, 0, 0, 2, 1.0, 512, 128, perceptual=False, **kw)
    # all of it before the engine is created: none of these needs a GPU or the library
    with pytest.raises(ValueError, match="needs validation_rir_A and validation_rir_B"):
        mk(evaluation_spectra=True)
    with pytest.raises(ValueError, match="a subband keyword"):
        mk(evaluation_spectra=True, mode="broadband")
    with pytest.raises(ValueError, match="a subband keyword"):
        mk(evaluation_spectra=True, validation_rir_A=rv, validation_rir_B=rv, mode="broadband")
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError, match="must be a bool"):
            mk(evaluation_spectra=bad, validation_rir_A=rv, validation_rir_B=rv)
    assert apvast._check_evaluation_spectra(False, None, "broadband") is False
    assert apvast._check_evaluation_spectra(np.True_, (rv, rv, [1]), "subband") is True


def test_state_keys_and_accessor():
    from ap_vast_unofficial_amd.apvast import apvast
    assert apvast._EVALSPEC_STATE == ("evaluation_spectra", "evaluation_ring")
    others = (apvast._SB_STATE + apvast._BB_STATE + apvast._LIVE_STATE + apvast._WIN_STATE + apvast._FORGET_STATE + apvast._FIR_STATE
              + apvast._EVAL_STATE)
    assert not set(apvast._EVALSPEC_STATE) & set(others)
    # get_state and set_state take the keys only in subband mode and behind the object's own keyword
    rows = [r for r in apvast._STATE_ROWS if r.key in apvast._EVALSPEC_STATE]
    flags = lambda **kw: [bool(f(SimpleNamespace(**kw))) for r in rows for f in (r.accepts, r.reports or r.accepts)]
    assert len(rows) == len(apvast._EVALSPEC_STATE)
    assert not any(flags(mode="subband", _evaluation_spectra=False))
    assert all(flags(mode="subband", _evaluation_spectra=True))
    assert not any(flags(mode="broadband", _evaluation_spectra=True))
    assert callable(apvast.evaluation_spectra)


def test_abi_declared_and_exported():
    from ap_vast_unofficial_amd import _capi
    text = open(os.path.join(ROOT, "include", "apvast_hip.h")).read()
    assert re.search(r"int\s+apv_stream_set_evaluation_spectra\(apv_handle\* h, int32_t on\);", text)
    assert re.search(r"int\s+apv_eval_spectrum_step\(apv_handle\* h, const double\* d_pressure, double\* d_ring, int32_t ring_off, "
                     r"int32_t N, int32_t H, int32_t Z,\s+int32_t E, int32_t Mv, double\* d_totals\);", text)
    assert int(re.search(r"#define APV_ABI_VERSION (\d+)", text).group(1)) == 2
    for name in ("apv_stream_set_evaluation_spectra", "apv_eval_spectrum_step"):
        assert name in _capi.EXPORTS
    assert inspect.signature(_capi.Engine.__init__).parameters["evaluation_spectra"].default is False
    for name in ("set_evaluation_spectra", "eval_spectrum_step"):
        assert hasattr(_capi.Engine, name)
    mk = open(os.path.join(ROOT, "ap_vast_unofficial_amd", "csrc", "Makefile")).read()
    assert "kernels_evalspec.hip" in mk
    internal = open(os.path.join(ROOT, "ap_vast_unofficial_amd", "csrc", "apv_internal.h")).read()
    assert "apv_launch_eval_spectra" in internal
