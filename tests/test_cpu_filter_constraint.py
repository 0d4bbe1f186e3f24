"""Filter-length constraint of the subband stream (constrain_filter_length): what can be checked without a GPU -- the oracle
helper, the keyword's validation, and the C ABI's declarations and exports."""
import inspect
import os
import re

import numpy as np
import pytest

from constraint_oracle import ConstrainedForgettingOracle, ConstrainedSubbandOracle, project
from oracle.subband_stream import SubbandStreamOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synth_rirs(P, L, M, seed):
    rng = np.random.default_rng(seed)
    env = np.exp(-np.arange(P) / (P / 6.0))[:, None, None]
    return (rng.standard_normal((P, L, M)) * env * 1e-3, rng.standard_normal((P, L, M)) * env * 1e-3)


ARGS = (32, *synth_rirs(24, 4, 6, 1), 3, 1, 2, [1, 2], 1.0)


def _run(orc, x, hops, H):
    return [orc.process(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H]) for h in range(hops)]


def test_projection_is_a_projection():
    rng = np.random.default_rng(0)
    N, J = 60, 7
    w = rng.standard_normal((N // 2 + 1, 2, 3)) + 1j * rng.standard_normal((N // 2 + 1, 2, 3))
    w1, taps = project(w, N, J)
    w2, taps2 = project(w1, N, J)
    assert taps.shape == (J, 2, 3)
    assert np.abs(w2 - w1).max() < 1e-14 * np.abs(w1).max() and np.abs(taps2 - taps).max() < 1e-14 * np.abs(taps).max()
    assert np.abs(np.fft.irfft(w1, N, axis=0)[J:]).max() < 1e-15 * np.abs(taps).max()
    full, _ = project(w, N, N)                       # J = N: only the imaginary parts of bins 0 and N/2 go
    assert np.abs(full[1:-1] - w[1:-1]).max() < 1e-14 * np.abs(w).max()
    assert np.abs(full[[0, -1]].imag).max() == 0.0 and np.abs(full[[0, -1]].real - w[[0, -1]].real).max() < 1e-14 * np.abs(w).max()


def test_helper_with_all_taps_is_the_plain_oracle_and_few_taps_are_not():
    """J = N leaves every output where it was (1e-12 of the peak: an irfft / rfft pair on the filters); J = 8 of 32 moves them."""
    H, hops = 16, 6
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    plain = _run(SubbandStreamOracle(*ARGS, hop_size=H), x, hops, H)
    full = _run(ConstrainedSubbandOracle(*ARGS, hop_size=H, filter_taps=32), x, hops, H)
    orc = ConstrainedSubbandOracle(*ARGS, hop_size=H, filter_taps=8)
    cut = _run(orc, x, hops, H)
    peak = max(np.abs(p[0]).max() for p in plain)
    assert max(np.abs(f[0] - p[0]).max() for f, p in zip(full, plain)) < 1e-12 * peak
    # the constraint changes what the mode computes: a build that ignores the keyword cannot pass the GPU tests
    assert max(np.abs(c[0] - p[0]).max() for c, p in zip(cut, plain)) > 0.01 * peak
    for q in (2, 3):                                 # the target paths are untouched
        assert all(np.array_equal(c[q], p[q]) for c, p in zip(cut, plain))
    for z in range(2):
        assert orc.w_time[z].shape == (2, 8, 4)
        g = np.fft.irfft(orc.w[z], 32, axis=0)       # (N, nV, L)
        assert np.abs(g[8:]).max() < 1e-15 * np.abs(g).max()
        assert np.abs(g[:8].transpose(1, 0, 2) - orc.w_time[z]).max() < 1e-15 * np.abs(g).max()


def test_helper_combines_with_window_and_forgetting():
    H, hops = 16, 5
    x = np.random.default_rng(3).standard_normal((2, hops * H))
    a = _run(ConstrainedSubbandOracle(*ARGS, hop_size=H, filter_taps=8, stat_hops=3), x, hops, H)
    b = _run(ConstrainedForgettingOracle(*ARGS, hop_size=H, filter_taps=8, beta=0.9), x, hops, H)
    c = _run(ConstrainedSubbandOracle(*ARGS, hop_size=H, filter_taps=8), x, hops, H)
    assert np.array_equal(a[0][0], c[0][0]) and np.array_equal(b[0][0], c[0][0])          # one hop in: the same statistics
    assert not np.array_equal(a[-1][0], c[-1][0]) and not np.array_equal(b[-1][0], c[-1][0])
    with pytest.raises(ValueError, match="filter_taps"):
        ConstrainedSubbandOracle(*ARGS, hop_size=H, filter_taps=33)


def test_keyword_signature_and_validation():
    from ap_vast_unofficial_amd.apvast import apvast
    p = inspect.signature(apvast.__init__).parameters["constrain_filter_length"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert "w_time_A" in apvast._LAZY and "w_time_B" in apvast._LAZY
    r = np.zeros((10, 2, 2))
    mk = lambda J, delay, **kw: apvast(256, r, r, J, delay, 0, 0, 2, 1.0, 512, 128, perceptual=False, **kw)
    for bad in (1, 0, "yes", None, 1.0):             # a bool, nothing else
        with pytest.raises(ValueError, match="constrain_filter_length must be a bool"):
            mk(16, 4, constrain_filter_length=bad)
    for J in (0, -3, 257, 2.5):                      # 1 <= filter_length <= block_size
        with pytest.raises(ValueError, match="filter_length must be an int in 1..block_size"):
            mk(J, 0, constrain_filter_length=True)
    for J, delay in ((16, 16), (16, 40), (1, 1)):    # modeling_delay < filter_length
        with pytest.raises(ValueError, match="modeling_delay must be below filter_length"):
            mk(J, delay, constrain_filter_length=True)
    with pytest.raises(ValueError, match="constrain_filter_length is a subband keyword"):
        mk(16, 4, constrain_filter_length=True, mode="broadband")
    # all of it before the engine is created: none of the above needed a GPU.  Off, filter_length stays unchecked as it was
    assert apvast._check_constrain_filter_length(False, 0, 256, 300, "subband") is False
    assert apvast._check_constrain_filter_length(True, 256, 256, 255, "subband") is True
    assert apvast._check_constrain_filter_length(np.bool_(True), 1, 256, 0, "subband") is True


def test_abi_declared_and_exported():
    from ap_vast_unofficial_amd import _capi
    text = open(os.path.join(ROOT, "include", "apvast_hip.h")).read()
    assert re.search(r"int\s+apv_stream_set_filter_taps\(apv_handle\* h, int32_t J\);", text)
    assert re.search(r"int\s+apv_constrain_filters\(apv_handle\* h, void\* d_w, int32_t n_bins, int32_t nV, int32_t L, int32_t N, "
                     r"int32_t J, void\* d_taps\);", text)
    assert "g[J:] = 0" in text and "w_time_A" in text
    assert int(re.search(r"#define APV_ABI_VERSION (\d+)", text).group(1)) == 2
    lib = _capi.load()
    for name in ("apv_stream_set_filter_taps", "apv_constrain_filters"):
        assert hasattr(lib, name) and name in _capi.EXPORTS
    assert inspect.signature(_capi.Engine.__init__).parameters["filter_taps"].default == 0
    assert hasattr(_capi.Engine, "constrain_filters")
    mk = open(os.path.join(ROOT, "ap_vast_unofficial_amd", "csrc", "Makefile")).read()
    assert "kernels_constrain.hip" in mk
