"""The rank choice by the contrast at validation microphones (validation_floor_db): what can be checked without a
GPU -- the keyword's signature and validation, the refusals, the C ABI's declaration and export, the transfer functions, and the
oracle helper (tests/validation_span_oracle.py) on hand-made curves."""
import inspect
import os
import re

import numpy as np
import pytest

from effort_oracle import EffortConstrainedOracle, EffortForgettingOracle, EffortSubbandOracle
from validation_span_oracle import (ValidationConstrainedOracle, ValidationForgettingOracle, ValidationSubbandOracle, choose, decide,
                                    energies, transfer, validation_span)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = tuple(f"validation_{q}_{z}" for q in ("bright", "dark", "source", "rank") for z in "AB")
K = 129


def _make(**kw):
    from ap_vast_unofficial_amd.apvast import apvast
    r = np.zeros((10, 2, 2))
    return apvast(256, r, r, 16, 4, 0, 0, 2, 1.0, 512, 128, perceptual=False, **kw)


RV = dict(validation_rir_A=np.ones((5, 2, 3)), validation_rir_B=np.ones((5, 2, 3)))


# ---- the keyword ----
def test_keyword_is_keyword_only_and_optional():
    from ap_vast_unofficial_amd.apvast import apvast
    params = inspect.signature(apvast.__init__).parameters
    assert params["validation_floor_db"].kind is inspect.Parameter.KEYWORD_ONLY and params["validation_floor_db"].default is None
    assert list(params)[-1] == "statistics_hops"
    for name in ("validation_floor_db",) + OUTPUTS:
        assert isinstance(getattr(apvast, name), property)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), True, "3", np.ones(128), np.ones((3, 129)), np.ones((2, 128)),
                                 np.full(129, np.nan), np.full((2, 129), np.inf), np.ones(129, dtype=bool), np.array(["x"] * 129),
                                 -4000.0, 4000.0])
def test_validation(bad):
    # (-4000 dB is a finite float whose 10^(dB / 10) is zero, which would silently mean "no floor"; +4000 dB overflows)
    with pytest.raises(ValueError, match="validation_floor_db"):
        _make(validation_floor_db=bad, **RV)


def test_check_accepts_a_float_a_row_and_a_table():
    from ap_vast_unofficial_amd.apvast import apvast
    ev = (RV["validation_rir_A"], RV["validation_rir_B"], [1, 2])
    for good in (-12.0, 3, -float("inf"), np.full(K, -6.0), np.full((2, K), -np.inf), np.linspace(-20, 20, K)):
        a = apvast._check_validation_floor_db(good, K, ev, "subband")
        assert a.shape == (2, K) and a.dtype == np.float64 and not a.flags.writeable
    a = apvast._check_validation_floor_db(np.stack([np.full(K, -12.0), np.full(K, 3.0)]), K, ev, "subband")
    assert (a[0] == -12.0).all() and (a[1] == 3.0).all()
    assert apvast._check_validation_floor_db(None, K, None, "subband") is None
    assert apvast._check_validation_floor_db(None, K, None, "broadband") is None


def test_refusals():
    with pytest.raises(ValueError, match="validation_floor_db needs validation_rir_A and validation_rir_B"):
        _make(validation_floor_db=3.0)
    with pytest.raises(ValueError, match="validation_floor_db is a subband keyword"):
        _make(mode="broadband", validation_floor_db=3.0)
    with pytest.raises(ValueError, match="a subband keyword"):
        _make(mode="broadband", validation_floor_db=3.0, **RV)


def test_abi_declared_and_exported():
    from ap_vast_unofficial_amd import _capi
    text = open(os.path.join(ROOT, "include", "apvast_hip.h")).read()
    assert re.search(r"int\s+apv_stream_set_validation_span\(apv_handle\* h, const void\* h_G_A, const void\* h_G_B, const double\* h_floor\);", text)
    assert re.search(r"int\s+apv_get_validation_span\(apv_handle\* h, int32_t zone, int32_t what, void\* h_dst\);", text)
    assert re.search(r"int\s+apv_validation_span\(apv_handle\* h, int32_t c128, int32_t K, int32_t nV, int32_t L, int32_t Mv, void\* h_w,", text)
    assert "Matlab/main.m:120-130" in text
    assert int(re.search(r"#define APV_ABI_VERSION (\d+)", text).group(1)) == 2
    lib = _capi.load()
    for name in ("apv_stream_set_validation_span", "apv_get_validation_span", "apv_validation_span"):
        assert hasattr(lib, name) and name in _capi.EXPORTS
    assert inspect.signature(_capi.Engine.__init__).parameters["validation_span"].default is None
    for name in ("set_validation_span", "validation_span", "validation_span_kernel"):
        assert callable(getattr(_capi.Engine, name))


def test_contrast_helper():
    from ap_vast_unofficial_amd.evaluation import validation_contrast_db
    c = validation_contrast_db([[10.0, 1.0, 1.0, 0.0, np.nan]], [[1.0, 10.0, 0.0, 0.0, 1.0]])
    assert c.shape == (1, 5) and c[0, 0] == 10.0 and c[0, 1] == -10.0 and c[0, 2] == np.inf and np.isnan(c[0, 3]) and np.isnan(c[0, 4])


# ---- the transfer functions ----
@pytest.mark.parametrize("Pv,N", [(9, 32), (35, 32), (1, 32), (5, 256)])
def test_transfer_against_a_direct_sum(Pv, N):
    """Pv < N, Pv = N + 3 (taps beyond the block fold back onto the bin frequencies) and Pv = 1 (constant over frequency)"""
    from ap_vast_unofficial_amd.apvast import apvast
    rng = np.random.default_rng(Pv)
    L, Mv = 3, 4
    rv = rng.standard_normal((Pv, L, Mv))
    ref = np.zeros((N // 2 + 1, Mv, L), dtype=np.complex128)
    for k in range(N // 2 + 1):
        for j in range(Pv):
            ref[k] += rv[j].T * np.exp(-2j * np.pi * j * k / N)
    scale = np.abs(rv).sum(0).T[None]                          # sum_j |rv|
    for G in (transfer(rv, N), apvast.validation_transfer(rv, N)):
        assert G.shape == ref.shape and G.dtype == np.complex128
        assert (np.abs(G - ref) <= 64 * np.finfo(np.float64).eps * scale).all()
    if Pv == 1:
        assert np.array_equal(transfer(rv, N), np.broadcast_to(rv[0].T, ref.shape))


# ---- decide on hand-made curves ----
def test_decide_all_admissible():
    src, top = decide([[4.0, 6.0, 9.0]], [[1.0, 2.0, 3.0]], 2.0)
    assert np.array_equal(src, [[0, 1, 2]]) and top[0] == 3 and src.dtype == top.dtype == np.int32


def test_decide_a_gap():
    # contrast 4, 1, 1, 5, 0.5: slots 1, 2 and 4 fall back on the admissible slot below them
    src, top = decide([[4.0, 1.0, 2.0, 5.0, 1.0]], [[1.0, 1.0, 2.0, 1.0, 2.0]], 3.0)
    assert np.array_equal(src, [[0, 0, 0, 3, 3]]) and top[0] == 4
    # the first slots inadmissible: they take the running best, later slots the admissible one
    src, top = decide([[1.0, 2.0, 9.0, 1.0]], [[1.0, 1.0, 1.0, 1.0]], 5.0)
    assert np.array_equal(src, [[0, 1, 2, 2]]) and top[0] == 3


def test_decide_none_admissible():
    # the running argmax of bright / dark; ties (2/4 = 1/2, 6/4 = 3/2) keep the smaller slot
    src, top = decide([[1.0, 2.0, 3.0, 6.0, 1.0]], [[2.0, 4.0, 2.0, 4.0, 8.0]], 100.0)
    assert np.array_equal(src, [[0, 0, 2, 2, 2]]) and top[0] == 3
    # under a finite floor a slot with dark = 0 is always admissible (bright >= phi 0), so its place in the ranking shows only
    # under phi = inf, which the library refuses and the helper takes: inf * 0 = NaN, nothing is admissible.  0/0 ranks lowest,
    # below a ratio of 0
    src, top = decide([[0.0, 0.0, 1.0, 7.0]], [[0.0, 5.0, 2.0, 2.0]], np.inf)
    assert np.array_equal(src, [[0, 1, 2, 3]])
    src, _ = decide([[0.0, 0.0]], [[5.0, 0.0]], 2.0)           # ratio 0, then 0/0: admissible (0 >= 2 * 0), the largest wins
    assert np.array_equal(src, [[0, 1]])
    src, _ = decide([[0.0, 0.0, 0.0]], [[0.0, 3.0, 0.0]], np.inf)   # inf * 0 = NaN: nothing admissible; 0/0 < 0/3, tie keeps 1
    assert np.array_equal(src, [[0, 1, 1]])
    src, _ = decide([[1.0, 2.0, 3.0]], [[4.0, 0.0, 0.0]], np.inf)   # dark = 0 < bright above 1/4; two of them tie
    assert np.array_equal(src, [[0, 1, 1]])


def test_decide_non_finite_slots():
    nan, inf = np.nan, np.inf
    # no finite slot at or below: left as it is (-1); a non-finite slot above a finite one takes that slot's source
    src, top = decide([[nan, 1.0, inf, 1.0]], [[1.0, 1.0, 1.0, nan]], 0.5)
    assert np.array_equal(src, [[-1, 1, 1, 1]]) and top[0] == 2
    src, top = decide([[nan, nan]], [[1.0, inf]], 0.5)
    assert np.array_equal(src, [[-1, -1]]) and top[0] == 0
    # no floor: every finite slot is its own source, a non-finite one is left as it is
    src, top = decide([[2.0, nan, 1.0]], [[1.0, 1.0, 9.0]], 0.0)
    assert np.array_equal(src, [[0, -1, 2]]) and top[0] == 3
    # a per-bin floor
    src, _ = decide([[1.0, 2.0], [1.0, 2.0]], [[1.0, 4.0], [1.0, 4.0]], [1.0, 0.25])
    assert np.array_equal(src, [[0, 0], [0, 1]])


def test_sources_are_fixed_points():
    """the proof case: whatever the curves, src[src[t]] = src[t], so the copies never read a slot that is written"""
    rng = np.random.default_rng(0)
    Kb, nV = 400, 9
    bright = rng.choice([0.0, 0.5, 1.0, 2.0, 3.0, np.nan, np.inf], (Kb, nV), p=[.1, .2, .2, .2, .2, .05, .05])
    dark = rng.choice([0.0, 0.5, 1.0, 2.0, 3.0, np.nan], (Kb, nV), p=[.1, .2, .2, .2, .2, .1])
    phi = rng.choice([0.0, 0.5, 1.0, 2.0, 50.0], Kb)
    src, top = decide(bright, dark, phi)
    hit = 0
    for k in range(Kb):
        for t in range(nV):
            s = src[k, t]
            assert -1 <= s <= t
            if s >= 0:
                assert src[k, s] == s, (k, t, s)
                hit += s != t
    assert hit > 100
    # so applying the copies in any order gives the same filters
    W = rng.standard_normal((Kb, nV, 3)) + 1j * rng.standard_normal((Kb, nV, 3))
    a = choose(W, src)
    b = W.copy()
    for t in reversed(range(nV)):
        for k in range(Kb):
            if src[k, t] >= 0:
                b[k, t] = b[k, src[k, t]]
    assert np.array_equal(a, b)


def test_energies_and_the_whole_stage():
    rng = np.random.default_rng(1)
    Kb, nV, L, Mv = 6, 4, 5, 3
    cn = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    W, GB, GD = cn(Kb, nV, L), cn(Kb, Mv, L), cn(Kb, Mv, L)
    bright, dark = energies(GB, GD, W)
    for k in range(Kb):
        for t in range(nV):
            assert np.isclose(bright[k, t], np.linalg.norm(GB[k] @ W[k, t]) ** 2, rtol=1e-13)
            assert np.isclose(dark[k, t], np.linalg.norm(GD[k] @ W[k, t]) ** 2, rtol=1e-13)
    phi = np.median(bright / dark)
    out, b2, d2, src, top = validation_span(W, GB, GD, phi)
    assert np.array_equal(b2, bright) and (src != np.arange(nV)).any() and (src == np.arange(nV)).any()
    for k in range(Kb):
        for t in range(nV):
            assert np.array_equal(out[k, t], W[k, src[k, t]])
    # no floor: bitwise unchanged
    out0 = validation_span(W, GB, GD, 0.0)
    assert np.array_equal(out0[0], W) and np.array_equal(out0[3], np.broadcast_to(np.arange(nV), (Kb, nV)))


# ---- the helper in the stream ----
@pytest.fixture(scope="module")
def stream_inputs():
    N, H, hops = 64, 32, 4
    rng = np.random.default_rng(3)
    env = np.exp(-np.arange(60) / 10.0)[:, None, None]
    rirA, rirB = rng.standard_normal((60, 4, 8)) * env * 1e-3, rng.standard_normal((60, 4, 8)) * env * 1e-3
    rvA, rvB = rng.standard_normal((9, 4, 5)), rng.standard_normal((9, 4, 5))
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    return N, H, hops, (N, rirA, rirB, 5, 1, 2, [1, 2, 3, 4], 1.0), x, rvA, rvB


def _run(orc, x, hops, H):
    return [orc.process(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H]) for h in range(hops)]


@pytest.mark.parametrize("pair", ["windowed", "forgetting", "constrained"])
@pytest.mark.parametrize("off", ["absent", "no floor"])
def test_off_is_identical_to_the_parents(stream_inputs, pair, off):
    N, H, hops, args, x, rvA, rvB = stream_inputs
    Kb = N // 2 + 1
    parent, child, kw = {"windowed": (EffortSubbandOracle, ValidationSubbandOracle, dict(stat_hops=2)),
                         "forgetting": (EffortForgettingOracle, ValidationForgettingOracle, dict(beta=0.9)),
                         "constrained": (EffortConstrainedOracle, ValidationConstrainedOracle, dict(filter_taps=8))}[pair]
    common = dict(hop_size=H, effort_limit=np.full((2, Kb), 0.1), **kw)
    vkw = {} if off == "absent" else dict(rv_A=rvA, rv_B=rvB, validation_floor=np.zeros((2, Kb)))
    a, b = parent(*args, **common), child(*args, **common, **vkw)
    for p, c in zip(_run(a, x, hops, H), _run(b, x, hops, H)):
        for q in range(4):
            assert np.array_equal(p[q], c[q])
    for z in range(2):
        assert np.array_equal(a.w[z], b.w[z]) and np.array_equal(a.effort[z], b.effort[z])
        if off == "absent":
            assert b.validation_bright[z] is None
        else:
            assert (b.validation_src[z] == np.arange(4)).all() and (b.validation_rank[z] == 4).all()


def test_helper_in_the_stream_chooses_and_changes_the_outputs(stream_inputs):
    N, H, hops, args, x, rvA, rvB = stream_inputs
    Kb = N // 2 + 1
    base = ValidationSubbandOracle(*args, hop_size=H, rv_A=rvA, rv_B=rvB, validation_floor=np.zeros((2, Kb)))
    ref = _run(base, x, hops, H)
    phi = [np.median(base.validation_bright[z] / base.validation_dark[z]) for z in range(2)]
    orc = ValidationSubbandOracle(*args, hop_size=H, rv_A=rvA, rv_B=rvB, validation_floor=np.stack([np.full(Kb, p) for p in phi]))
    got = _run(orc, x, hops, H)
    for z in range(2):
        src = orc.validation_src[z]
        assert (src != np.arange(4)).any() and (src == np.arange(4)).any()
        assert np.array_equal(orc.w[z], choose(orc.w_unchosen[z], src))
        assert 1 <= orc.validation_rank[z].min() and orc.validation_rank[z].max() <= 4
    # the choice changes what the mode computes: a build that ignores the keyword cannot pass the GPU tests
    for q in range(2):
        peak = max(np.abs(b[q]).max() for b in ref)
        diff = max(np.abs(b[q] - t[q]).max() for b, t in zip(ref, got))
        assert diff > 0.01 * peak
