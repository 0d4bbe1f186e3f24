"""The per-bin span of the subband stream (mu_profile, rank_profile, contrast_floor_db): what can be checked without a GPU -- the
keywords' signature and validation, the broadband refusals, the C ABI's declaration and export, and the oracle helper."""
import inspect
import os
import re

import numpy as np
import pytest

from oracle.subband_stream import SubbandStreamOracle
from span_oracle import SpanSubbandOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYWORDS = ("mu_profile", "rank_profile", "contrast_floor_db")


def synth_rirs(P, L, M, seed):
    rng = np.random.default_rng(seed)
    env = np.exp(-np.arange(P) / (P / 6.0))[:, None, None]
    return (rng.standard_normal((P, L, M)) * env * 1e-3, rng.standard_normal((P, L, M)) * env * 1e-3)


def _run(orc, x, hops, H):
    return [orc.process(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H]) for h in range(hops)]


def _make(**kw):
    from ap_vast_unofficial_amd.apvast import apvast
    r = np.zeros((10, 2, 2))
    return apvast(256, r, r, 16, 4, 0, 0, 2, 1.0, 512, 128, perceptual=False, **kw)


def test_keywords_are_keyword_only_and_statistics_hops_stays_last():
    from ap_vast_unofficial_amd.apvast import apvast
    params = inspect.signature(apvast.__init__).parameters
    for name in KEYWORDS:
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default is None
    assert list(params)[-1] == "statistics_hops"
    for name in ("mu_profile", "rank_profile", "contrast_floor_db", "span_rank_A", "span_rank_B", "span_contrast_A", "span_contrast_B"):
        assert isinstance(getattr(apvast, name), property)


@pytest.mark.parametrize("bad", [np.ones(128), np.ones((3, 129)), np.ones((2, 128)), -np.ones(129), np.full(129, np.nan),
                                 np.full(129, np.inf), np.ones(129, dtype=bool), np.array(["x"] * 129)])
def test_mu_profile_validation(bad):
    with pytest.raises(ValueError, match="mu_profile"):
        _make(mu_profile=bad)


@pytest.mark.parametrize("bad", [np.ones(128, dtype=int), np.zeros(129, dtype=int), np.full(129, 3), np.ones(129),
                                 np.ones(129, dtype=bool), np.full((2, 129), -1)])
def test_rank_profile_validation(bad):
    # two loudspeakers: caps are integers in 1..2
    with pytest.raises(ValueError, match="rank_profile"):
        _make(rank_profile=bad)


# (-4000 dB and 4000 dB are finite floats whose 10^(dB / 10) is not a positive, finite double: 0 would mean "no floor" to the library)
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), True, "3", [3.0], -4000.0, 4000.0])
def test_contrast_floor_validation(bad):
    with pytest.raises(ValueError, match="contrast_floor_db"):
        _make(contrast_floor_db=bad)


@pytest.mark.parametrize("kw", [dict(mu_profile=np.ones(129)), dict(rank_profile=np.ones(129, dtype=int)), dict(contrast_floor_db=3.0)])
def test_broadband_refuses_the_keywords(kw):
    name = next(iter(kw))
    with pytest.raises(ValueError, match=f"{name} is a subband keyword"):
        _make(mode="broadband", **kw)


def test_abi_declared_and_exported():
    from ap_vast_unofficial_amd import _capi
    text = open(os.path.join(ROOT, "include", "apvast_hip.h")).read()
    assert re.search(r"int\s+apv_set_span\(apv_handle\* h, const double\* h_mu_profile, const int32_t\* h_rank_cap, double contrast_floor\);", text)
    assert re.search(r"int\s+apv_get_span\(apv_handle\* h, int32_t zone, int32_t\* h_rank, double\* h_contrast\);", text)
    assert int(re.search(r"#define APV_ABI_VERSION (\d+)", text).group(1)) == 2
    lib = _capi.load()
    for name in ("apv_set_span", "apv_get_span"):
        assert hasattr(lib, name) and name in _capi.EXPORTS
    assert inspect.signature(_capi.Engine.__init__).parameters["span"].default is None
    assert list(inspect.signature(_capi.Engine.set_span).parameters)[1:] == ["mu_profile", "rank_cap", "contrast_floor_db"]


@pytest.fixture(scope="module")
def stream_inputs():
    N, H, hops = 256, 128, 6
    rirA, rirB = synth_rirs(200, 8, 16, 1)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    return N, H, hops, (N, rirA, rirB, 5, 1, 2, list(range(1, 9)), 1.0), x


def test_helper_without_a_span_is_the_stream_oracle(stream_inputs):
    N, H, hops, args, x = stream_inputs
    base_orc, span_orc = SubbandStreamOracle(*args, hop_size=H), SpanSubbandOracle(*args, hop_size=H)
    base, plain = _run(base_orc, x, hops, H), _run(span_orc, x, hops, H)
    for b, o in zip(base, plain):
        for q in range(4):
            assert np.array_equal(b[q], o[q])
    for z in range(2):
        assert np.array_equal(base_orc.w[z], span_orc.w[z]) and np.array_equal(base_orc.lam[z], span_orc.lam[z])


def test_helper_contrast_curve_is_monotone_and_the_span_changes_the_outputs(stream_inputs):
    N, H, hops, args, x = stream_inputs
    K, L = N // 2 + 1, 8
    base = _run(SubbandStreamOracle(*args, hop_size=H), x, hops, H)
    orc = SpanSubbandOracle(*args, hop_size=H, mu_profile=np.geomspace(1.0, 10.0, K), rank_cap=np.linspace(8, 1, K).round().astype(int),
                            floor_db=5.0)
    got = _run(orc, x, hops, H)
    phi = 10.0 ** 0.5
    for z in range(2):
        c, lam = orc.span_contrast[z], orc.lam[z]
        # a weighted mean of a descending sequence: it never rises (up to the rounding of the two running sums)
        assert (np.diff(c, axis=1) <= 1e-12 * lam[:, :1]).all()
        assert (c[:, 0] <= lam[:, 0] * (1 + 1e-12)).all() and (c[:, -1] >= lam[:, -1] - 1e-12 * lam[:, 0]).all()
        f = np.maximum(np.cumprod(c >= phi, axis=1).sum(axis=1), 1)
        s = np.minimum(orc.rank_cap[z], f)
        # (the helper compares num >= phi den, not the quotient: equal off the rounding of one division)
        assert (orc.span_rank[z] == np.minimum(8, s)).mean() > 0.99
        assert 1 <= orc.span_rank[z].min() and orc.span_rank[z].max() <= 8
        # slots above the bin's rank repeat it
        w = orc.w[z]
        for k in (0, K // 2, K - 1):
            sk = orc.span_rank[z][k]
            for t in range(sk, 8):
                assert np.array_equal(w[k, t], w[k, sk - 1])
    # the span changes what the mode computes: a build that ignores the keywords cannot pass the GPU tests
    for q in range(2):
        peak = max(np.abs(b[q]).max() for b in base)
        diff = max(np.abs(b[q] - t[q]).max() for b, t in zip(base, got))
        assert diff > 0.01 * peak
