"""Exponentially forgetting statistics of the subband stream (statistics_forgetting): what can be checked without a GPU -- the
forgetting oracle helper, the keyword's validation, and the C ABI's declaration and export."""
import inspect
import os
import re

import numpy as np
import pytest

from forgetting_oracle import ForgettingSubbandOracle
from oracle import subband
from windowed_oracle import WindowedSubbandOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synth_rirs(P, L, M, seed):
    rng = np.random.default_rng(seed)
    env = np.exp(-np.arange(P) / (P / 6.0))[:, None, None]
    return (rng.standard_normal((P, L, M)) * env * 1e-3, rng.standard_normal((P, L, M)) * env * 1e-3)


def _run(orc, x, hops, H):
    return [orc.process(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H]) for h in range(hops)]


ARGS = (256, *synth_rirs(200, 8, 16, 1), 12, 2, 5, [1, 2, 3, 4], 1.0)


def test_helper_beta_one_is_the_unfilled_window():
    """beta = 1, 5 hops: the stack is that of a window of 8 hops that has not filled (scaling by 1.0 is exact)."""
    H, hops = 128, 5
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    fg = _run(ForgettingSubbandOracle(*ARGS, hop_size=H, beta=1.0), x, hops, H)
    win = _run(WindowedSubbandOracle(*ARGS, hop_size=H, stat_hops=8), x, hops, H)
    for f, w in zip(fg, win):
        for q in range(4):
            assert np.array_equal(f[q], w[q])


def test_helper_statistics_are_the_recursion():
    """beta = 0.5: forgetting_statistics against R <- beta R + G formed hop by hop, and the outputs differ from one block's."""
    H, hops, beta = 128, 6, 0.5
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    orc = ForgettingSubbandOracle(*ARGS, hop_size=H, beta=beta)
    one = WindowedSubbandOracle(*ARGS, hop_size=H, stat_hops=1)
    acc = [None, None]
    moved = 0.0
    for h in range(hops):
        sl = slice(h * H, (h + 1) * H)
        a, b = orc.process(x[0, sl], x[1, sl]), one.process(x[0, sl], x[1, sl])
        moved = max(moved, np.abs(a[0] - b[0]).max() / np.abs(b[0]).max())
        for z in range(2):
            G = subband.correlate(*orc.window_hops[z][-1])
            acc[z] = G if acc[z] is None else tuple(beta * o + g for o, g in zip(acc[z], G))
            for got, ref in zip(orc.forgetting_statistics(z), acc[z]):
                assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max(), (h, z)
    # forgetting changes what the mode computes: a build that ignores the keyword cannot pass the GPU tests
    assert moved > 0.01


def test_keyword_signature_and_validation():
    from ap_vast_unofficial_amd.apvast import apvast
    params = inspect.signature(apvast.__init__).parameters
    p = params["statistics_forgetting"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert list(params)[-1] != "statistics_forgetting"
    r = np.zeros((10, 2, 2))
    for bad in (0, -0.1, 1.5, float("nan"), "x", True):
        with pytest.raises(ValueError, match="statistics_forgetting"):
            apvast(256, r, r, 16, 4, 0, 0, 2, 1.0, 512, 128, perceptual=False, statistics_forgetting=bad)
    with pytest.raises(ValueError, match="statistics_forgetting"):
        apvast(256, r, r, 16, 4, 0, 0, 2, 1.0, 512, 128, perceptual=False, mode="broadband", statistics_forgetting=0.9)
    with pytest.raises(ValueError, match="statistics_forgetting"):
        apvast(256, r, r, 16, 4, 0, 0, 2, 1.0, 512, 128, perceptual=False, statistics_forgetting=0.9, statistics_hops=3)


def test_abi_declared_and_exported():
    from ap_vast_unofficial_amd import _capi
    text = open(os.path.join(ROOT, "include", "apvast_hip.h")).read()
    assert re.search(r"int\s+apv_stream_set_stat_forgetting\(apv_handle\* h, double beta\);", text)
    assert re.search(r"replaces:[^/]*apvast\.py:329-364 \*/\s*int\s+apv_stream_set_stat_forgetting", text)
    assert int(re.search(r"#define APV_ABI_VERSION (\d+)", text).group(1)) == 2
    assert hasattr(_capi.load(), "apv_stream_set_stat_forgetting")
    assert "apv_stream_set_stat_forgetting" in _capi.EXPORTS
    assert "stat_forgetting" in inspect.signature(_capi.Engine.__init__).parameters
