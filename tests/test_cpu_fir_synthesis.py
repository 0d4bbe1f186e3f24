"""FIR synthesis of the constrained subband stream (synthesis="fir"): what can be checked without a GPU -- the NumPy helper, the
keyword's validation (it runs before any engine exists), the defaults, and the C ABI's declarations and exports."""
import inspect
import os
import re

import numpy as np
import pytest

from fir_synthesis_oracle import FirStreamReference, fir_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_helper_is_the_definition():
    rng = np.random.default_rng(0)
    V, J, L, H = 2, 5, 3, 7
    gp, gc = rng.standard_normal((V, J, L)), rng.standard_normal((V, J, L))
    x = rng.standard_normal(J - 1 + H)
    y, S = fir_reference(x, gp, gc, H)
    assert y.shape == S.shape == (V, H, L)
    for v in range(V):
        for l in range(L):
            for t in range(H):
                a = (t + 1) / H
                yp = sum(gp[v, j, l] * x[J - 1 + t - j] for j in range(J))
                yc = sum(gc[v, j, l] * x[J - 1 + t - j] for j in range(J))
                assert abs(y[v, t, l] - ((1 - a) * yp + a * yc)) < 1e-14
                s = sum((abs(gp[v, j, l]) + abs(gc[v, j, l])) * abs(x[J - 1 + t - j]) for j in range(J))
                assert abs(S[v, t, l] - s) < 1e-14 and abs(y[v, t, l]) <= s
    # equal taps: the plain linear convolution; the last sample of a hop takes the current taps alone
    y, _ = fir_reference(x, gc, gc, H)
    for v in range(V):
        for l in range(L):
            assert np.abs(y[v, :, l] - np.convolve(x, gc[v, :, l])[J - 1:J - 1 + H]).max() < 1e-14
    y, _ = fir_reference(x, gp, gc, H)
    yc, _ = fir_reference(x, gc, gc, H)
    assert np.abs(y[:, -1] - yc[:, -1]).max() < 1e-15


def test_stream_reference_is_a_time_varying_convolution():
    """constant taps from the first hop on: after the fade-in of hop 0 the stream is np.convolve of the whole signal; the target
    paths are the delayed inputs"""
    rng = np.random.default_rng(1)
    V, J, L, H, hops, d, ref = 2, 11, 3, 4, 6, 2, 1               # J - 1 > 2 H: the history spans more than two hops
    g = rng.standard_normal((V, J, L))
    x = rng.standard_normal((2, hops * H))
    r = FirStreamReference(J, H, L, V, d, ref, run_B=False)
    outs = [r.hop(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H], [g, None])[0] for h in range(hops)]
    assert all(o[1] is None for o in outs)
    y = np.concatenate([np.stack(o[0]) for o in outs], axis=1)    # (V, hops H, L)
    for v in range(V):
        for l in range(L):
            full = np.convolve(x[0], g[v, :, l])[:hops * H]
            assert np.abs(y[v, H:, l] - full[H:]).max() < 1e-13
            a = (np.arange(H) + 1) / H
            assert np.abs(y[v, :H, l] - a * full[:H]).max() < 1e-13
    for q, sig in ((2, 0), (3, 1)):
        t = np.concatenate([o[q][0] for o in outs])
        assert np.array_equal(t[d:, ref], x[sig, :hops * H - d]) and not t[:d].any()
        assert not np.delete(t, ref, axis=1).any()


def test_keyword_signature_and_validation():
    from ap_vast_unofficial_amd.apvast import apvast
    p = inspect.signature(apvast).parameters["synthesis"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "wola"
    r = np.zeros((10, 2, 2))
    mk = lambda **kw: apvast(256, r, r, 16, 4, 0, 0, 2, 1.0, 512, 128, perceptual=False, **kw)
    # all of it before the engine is created: none of these needs a GPU
    with pytest.raises(ValueError, match="synthesis='fir' is a subband keyword"):
        mk(synthesis="fir", mode="broadband")
    with pytest.raises(ValueError, match="needs constrain_filter_length=True"):
        mk(synthesis="fir")
    with pytest.raises(ValueError, match="needs constrain_filter_length=True"):
        mk(synthesis="fir", constrain_filter_length=False)
    for bad in ("FIR", "ola", "", None, 1, True):
        with pytest.raises(ValueError, match="synthesis must be 'wola'"):
            mk(synthesis=bad, constrain_filter_length=True)
    assert apvast._check_synthesis("wola", False, "broadband") == "wola"
    assert apvast._check_synthesis("fir", True, "subband") == "fir"
    assert "fir_synthesis_taps" in apvast._FIR_STATE and "fir_synthesis_history" in apvast._FIR_STATE
    assert not set(apvast._FIR_STATE) & set(apvast._SB_STATE + apvast._BB_STATE)


def test_abi_declared_and_exported():
    from ap_vast_unofficial_amd import _capi
    text = open(os.path.join(ROOT, "include", "apvast_hip.h")).read()
    assert re.search(r"#define APV_SYNTH_WOLA 0\n#define APV_SYNTH_FIR 1\n", text)
    assert re.search(r"int\s+apv_stream_set_synthesis\(apv_handle\* h, int32_t mode\);", text)
    assert re.search(r"int\s+apv_fir_synthesis\(apv_handle\* h, const void\* d_x, const void\* d_taps_prev, const void\* d_taps_cur, "
                     r"int32_t nV, int32_t L,\s+int32_t J, int32_t H, void\* d_out\);", text)
    assert int(re.search(r"#define APV_ABI_VERSION (\d+)", text).group(1)) == 2
    lib = _capi.load()
    for name in ("apv_stream_set_synthesis", "apv_fir_synthesis"):
        assert hasattr(lib, name) and name in _capi.EXPORTS
    assert _capi.SYNTHESIS == {"wola": 0, "fir": 1}
    assert inspect.signature(_capi.Engine.__init__).parameters["synthesis"].default == "wola"
    assert hasattr(_capi.Engine, "fir_synthesis") and hasattr(_capi.Engine, "set_synthesis")
    mk = open(os.path.join(ROOT, "ap_vast_unofficial_amd", "csrc", "Makefile")).read()
    assert "kernels_firsynth.hip" in mk
