"""Statistics window of the subband stream (statistics_hops): what can be checked without a GPU -- the windowed oracle helper,
the keyword's validation, and the C ABI's declaration and export."""
import inspect
import os
import re

import numpy as np
import pytest

from oracle.subband_stream import SubbandStreamOracle
from windowed_oracle import WindowedSubbandOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synth_rirs(P, L, M, seed):
    rng = np.random.default_rng(seed)
    env = np.exp(-np.arange(P) / (P / 6.0))[:, None, None]
    return (rng.standard_normal((P, L, M)) * env * 1e-3, rng.standard_normal((P, L, M)) * env * 1e-3)


def _run(orc, x, hops, H):
    return [orc.process(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H]) for h in range(hops)]


def test_helper_one_hop_is_the_stream_oracle_and_three_hops_differ():
    N, H, hops = 256, 128, 8
    rirA, rirB = synth_rirs(200, 8, 16, 1)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    args = (N, rirA, rirB, 12, 2, 5, [1, 2, 3, 4], 1.0)
    base = _run(SubbandStreamOracle(*args, hop_size=H), x, hops, H)
    one = _run(WindowedSubbandOracle(*args, hop_size=H, stat_hops=1), x, hops, H)
    three = _run(WindowedSubbandOracle(*args, hop_size=H, stat_hops=3), x, hops, H)
    for b, o in zip(base, one):
        for q in range(4):
            assert np.array_equal(b[q], o[q])
    # the window changes what the mode computes: a build that ignores the keyword cannot pass the GPU tests
    for q in range(2):
        peak = max(np.abs(b[q]).max() for b in base)
        diff = max(np.abs(b[q] - t[q]).max() for b, t in zip(base, three))
        print(f"zone {q}: T = 3 against T = 1 moves the outputs by {diff / peak:.3f} of the peak")
        assert diff > 0.01 * peak
    # the first hop has nothing behind it: identical whatever the window
    for q in range(4):
        assert np.array_equal(base[0][q], three[0][q])


def test_keyword_signature_and_validation():
    from ap_vast_unofficial_amd.apvast import apvast
    p = inspect.signature(apvast.__init__).parameters["statistics_hops"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 1
    assert list(inspect.signature(apvast.__init__).parameters)[-1] == "statistics_hops"
    r = np.zeros((10, 2, 2))
    for bad in (0, -1, 65, 2.5, "x"):
        with pytest.raises(ValueError, match="statistics_hops"):
            apvast(256, r, r, 16, 4, 0, 0, 2, 1.0, 512, 128, perceptual=False, statistics_hops=bad)
    with pytest.raises(ValueError, match="statistics_hops"):
        apvast(256, r, r, 16, 4, 0, 0, 2, 1.0, 512, 128, perceptual=False, mode="broadband", statistics_hops=2)


def test_auto_resolves_from_statistics_buffer_length():
    from ap_vast_unofficial_amd.apvast import apvast
    res = apvast._resolve_statistics_hops
    assert res("auto", 512, 256, 128, "subband") == 3            # cfg1: 512 samples against blocks of 256, hop 128
    assert res("auto", 1000, 1600, 800, "subband") == 1          # the reference's own test parameters
    assert res("auto", 512, 256, 128, "broadband") == 1          # accepted, means nothing there
    assert res(1, 512, 256, 128, "broadband") == 1
    assert res(64, 512, 256, 128, "subband") == 64


def test_abi_declared_and_exported():
    from ap_vast_unofficial_amd import _capi
    text = open(os.path.join(ROOT, "include", "apvast_hip.h")).read()
    assert re.search(r"int\s+apv_stream_set_stat_hops\(apv_handle\* h, int32_t n_hops\);", text)
    assert int(re.search(r"#define APV_MAX_STAT_HOPS (\d+)", text).group(1)) == 64 == _capi.MAX_STAT_HOPS
    assert re.search(r"replaces:[^/]*apvast\.py:329-364 \*/\s*int\s+apv_stream_set_stat_hops", text)
    assert int(re.search(r"#define APV_ABI_VERSION (\d+)", text).group(1)) == 2
    assert hasattr(_capi.load(), "apv_stream_set_stat_hops")
    assert "apv_stream_set_stat_hops" in _capi.EXPORTS
    assert "stat_hops" in inspect.signature(_capi.Engine.__init__).parameters
