"""The per-bin array-effort limit of the subband stream (effort_limit_db): what can be checked without a GPU -- the keyword's
signature and validation, the broadband refusal, the C ABI's declaration and export, and the oracle helper."""
import inspect
import os
import re

import numpy as np
import pytest

from effort_oracle import EffortSubbandOracle, limit_effort
from oracle.subband_stream import SubbandStreamOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("effort_A", "effort_B", "effort_rank_A", "effort_rank_B", "effort_gain_A", "effort_gain_B")


def _make(**kw):
    from ap_vast_unofficial_amd.apvast import apvast
    r = np.zeros((10, 2, 2))
    return apvast(256, r, r, 16, 4, 0, 0, 2, 1.0, 512, 128, perceptual=False, **kw)


def test_keyword_is_keyword_only_and_statistics_hops_stays_last():
    from ap_vast_unofficial_amd.apvast import apvast
    params = inspect.signature(apvast.__init__).parameters
    assert params["effort_limit_db"].kind is inspect.Parameter.KEYWORD_ONLY and params["effort_limit_db"].default is None
    assert list(params)[-2:] == ["effort_limit_db", "statistics_hops"]
    for name in ("effort_limit_db",) + OUTPUTS:
        assert isinstance(getattr(apvast, name), property)


@pytest.mark.parametrize("bad", [float("nan"), -float("inf"), True, "3", np.ones(128), np.ones((3, 129)), np.ones((2, 128)),
                                 np.full(129, np.nan), np.full((2, 129), -np.inf), np.ones(129, dtype=bool), np.array(["x"] * 129),
                                 -4000.0])
def test_validation(bad):
    # (-4000 dB is a finite float whose 10^(dB / 10) is zero: the library takes limits > 0 only)
    with pytest.raises(ValueError, match="effort_limit_db"):
        _make(effort_limit_db=bad)


def test_check_accepts_a_float_a_row_and_a_table():
    from ap_vast_unofficial_amd.apvast import apvast
    K = 129
    for good in (-12.0, 3, float("inf"), np.full(K, -6.0), np.full((2, K), np.inf), np.linspace(-20, 20, K)):
        a = apvast._check_effort_limit_db(good, K, "subband")
        assert a.shape == (2, K) and a.dtype == np.float64 and not a.flags.writeable
    a = apvast._check_effort_limit_db(np.stack([np.full(K, -12.0), np.full(K, 3.0)]), K, "subband")
    assert (a[0] == -12.0).all() and (a[1] == 3.0).all()
    assert apvast._check_effort_limit_db(None, K, "subband") is None and apvast._check_effort_limit_db(None, K, "broadband") is None


def test_broadband_refuses_the_keyword():
    with pytest.raises(ValueError, match="effort_limit_db is a subband keyword"):
        _make(mode="broadband", effort_limit_db=-12.0)


def test_abi_declared_and_exported():
    from ap_vast_unofficial_amd import _capi
    text = open(os.path.join(ROOT, "include", "apvast_hip.h")).read()
    assert re.search(r"int\s+apv_stream_set_effort_limit\(apv_handle\* h, const double\* h_limit\);", text)
    assert re.search(r"int\s+apv_get_effort\(apv_handle\* h, int32_t zone, double\* h_effort, int32_t\* h_rank, double\* h_gain\);", text)
    assert re.search(r"int\s+apv_limit_effort\(apv_handle\* h, int32_t c128, int32_t n_hops, int32_t K, int32_t nV, int32_t L, void\* h_w, "
                     r"const double\* h_limit,\s+double\* h_effort, int32_t\* h_rank, double\* h_gain\);", text)
    assert int(re.search(r"#define APV_ABI_VERSION (\d+)", text).group(1)) == 2
    lib = _capi.load()
    for name in ("apv_stream_set_effort_limit", "apv_get_effort", "apv_limit_effort"):
        assert hasattr(lib, name) and name in _capi.EXPORTS
    assert inspect.signature(_capi.Engine.__init__).parameters["effort_limit"].default is None
    assert list(inspect.signature(_capi.Engine.set_span).parameters)[1:] == ["mu_profile", "rank_cap", "contrast_floor_db"]
    for name in ("set_effort_limit", "effort", "limit_effort"):
        assert callable(getattr(_capi.Engine, name))


# ---- the oracle helper ----
def _filters(K, nV, L, seed, dtype=np.complex128):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((K, nV, L)) + 1j * rng.standard_normal((K, nV, L))).astype(dtype)


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_helper_holds_the_limit_and_leaves_admissible_slots(dtype):
    K, nV, L = 40, 6, 7
    W = _filters(K, nV, L, 0, dtype) * np.random.default_rng(1).uniform(0.2, 2.0, (K, nV, 1)).astype(np.float32)
    W = W.astype(dtype)
    E = np.random.default_rng(2).uniform(4.0, 20.0, K)
    out, e, rank, gain, src = limit_effort(W, E, list(range(1, nV + 1)))
    assert out.dtype == W.dtype and e.shape == (K, nV) and rank.shape == gain.shape == (K,) and rank.dtype == np.int32
    e_out = (out.real.astype(np.float64) ** 2 + out.imag.astype(np.float64) ** 2).sum(-1)
    eps = np.finfo(np.float64).eps if dtype == np.complex128 else np.finfo(np.float32).eps
    assert (e_out <= E[:, None] * (1 + (1e-15 if dtype == np.complex128 else 4 * eps) * L)).all()
    ok = e <= E[:, None]
    assert 0.2 < ok.mean() < 0.8                       # both kinds of slot occur
    assert np.array_equal(out[ok], W[ok])              # admissible slots are bit-identical
    # applying it twice: slots that were kept or copied are admissible and stay bit for bit, and every slot still holds the limit.
    # A scaled slot has effort E (1 + O(eps)), on either side of E, so in floating point a second pass may scale it once more or
    # take a scaled slot below it: "changes nothing" bit for bit holds where the scaling is exact
    # (test_helper_twice_is_exact_on_exact_inputs)
    again = limit_effort(out, E, list(range(1, nV + 1)))[0]
    kept = src >= 0
    assert np.array_equal(again[kept], out[kept])
    e_again = (again.real.astype(np.float64) ** 2 + again.imag.astype(np.float64) ** 2).sum(-1)
    assert (e_again <= E[:, None] * (1 + (1e-15 if dtype == np.complex128 else 4 * eps) * L)).all()
    # E = inf is the identity
    ident, _, rank_inf, gain_inf, _ = limit_effort(W, np.inf, list(range(1, nV + 1)))
    assert np.array_equal(ident, W) and (rank_inf == nV).all() and (gain_inf == 1.0).all()


def test_helper_twice_is_exact_on_exact_inputs():
    # every slot of a bin is a permutation of one integer vector times a power of two, the limit a power of four times that
    # vector's effort: efforts and gains are exact, so the scaled slots land on E itself
    rng = np.random.default_rng(5)
    K, nV, L = 30, 5, 6
    base = (rng.integers(-8, 9, (K, L)) + 1j * rng.integers(-8, 9, (K, L))).astype(np.complex128)
    base[:, 0] += 1                                     # no zero vector
    W = np.stack([np.stack([1j ** t * rng.permutation(base[k]) * 2.0 ** rng.integers(-1, 3) for t in range(nV)]) for k in range(K)])
    E = (np.abs(base) ** 2).sum(-1) * 4.0 ** rng.integers(-1, 2, K)
    ranks = [1, 2, 3, 4, 5]
    out, _, _, gain, src = limit_effort(W, E, ranks)
    assert (src < 0).any() and (src >= 0).any() and (gain != 1.0).any()
    again, e2, rank2, gain2, _ = limit_effort(out, E, ranks)
    assert np.array_equal(again, out) and (gain2 == 1.0).all() and (e2 <= E[:, None]).all()


def test_helper_takes_the_largest_admissible_slot_not_above():
    # admissible, not, admissible (effort is not monotone in the rank); then none admissible; then a non-finite top slot
    d = np.zeros((3, 3, 4), dtype=np.complex128)
    d[0, :, 0] = [1.0, 3.0, 1.5j]
    d[1, :, 1] = [4.0, 2.0, 8.0]
    d[2, :, 2] = [1.0, 1.0, np.nan]
    out, e, rank, gain, src = limit_effort(d, 4.0, [1, 2, 5])
    assert np.array_equal(src, [[0, 0, 2], [-1, 1, 1], [0, 1, -1]])
    assert np.array_equal(out[0, 1], d[0, 0]) and np.array_equal(out[0, 2], d[0, 2]) and rank[0] == 5
    assert np.allclose(out[1, 0], d[1, 0] * 0.5) and np.array_equal(out[1, 2], d[1, 1]) and rank[1] == 2 and gain[1] == 1.0
    # a slot whose effort is not finite is never admissible, never a source, and is left as it is (rank 0 when it is the top slot)
    assert rank[2] == 0 and gain[2] == 1.0 and np.isnan(out[2, 2, 2].real) and np.array_equal(out[2, :2], d[2, :2])
    # a top slot with no admissible slot below it is scaled; a slot above a non-finite one still finds the admissible slot below
    t = np.zeros((2, 3, 1), dtype=np.complex128)
    t[0, :, 0] = [3.0, 4.0, 4.0]
    t[1, :, 0] = [0.5, np.inf, 3.0]
    out, e, rank, gain, src = limit_effort(t, 1.0, [1, 2, 3])
    assert rank[0] == 3 and gain[0] == 0.25 and out[0, 2, 0] == 1.0 and np.isclose(out[0, 0, 0], 1.0)
    assert rank[1] == 1 and gain[1] == 1.0 and np.isinf(out[1, 1, 0].real) and out[1, 2, 0] == 0.5


@pytest.fixture(scope="module")
def stream_inputs():
    N, H, hops = 64, 32, 5
    rng = np.random.default_rng(3)
    env = np.exp(-np.arange(60) / 10.0)[:, None, None]
    rirA, rirB = rng.standard_normal((60, 4, 8)) * env * 1e-3, rng.standard_normal((60, 4, 8)) * env * 1e-3
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    return N, H, hops, (N, rirA, rirB, 5, 1, 2, [1, 2, 3, 4], 1.0), x


def _run(orc, x, hops, H):
    return [orc.process(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H]) for h in range(hops)]


def test_helper_without_a_limit_is_the_stream_oracle(stream_inputs):
    N, H, hops, args, x = stream_inputs
    base_orc, eff_orc = SubbandStreamOracle(*args, hop_size=H), EffortSubbandOracle(*args, hop_size=H)
    for b, o in zip(_run(base_orc, x, hops, H), _run(eff_orc, x, hops, H)):
        for q in range(4):
            assert np.array_equal(b[q], o[q])
    for z in range(2):
        assert np.array_equal(base_orc.w[z], eff_orc.w[z]) and eff_orc.effort[z] is None


def test_helper_in_the_stream_limits_and_changes_the_outputs(stream_inputs):
    N, H, hops, args, x = stream_inputs
    K, E = N // 2 + 1, 10.0 ** -1.2
    base = _run(SubbandStreamOracle(*args, hop_size=H), x, hops, H)
    orc = EffortSubbandOracle(*args, hop_size=H, effort_limit=np.full((2, K), E))
    got = _run(orc, x, hops, H)
    for z in range(2):
        w = orc.w[z]
        assert ((np.abs(w) ** 2).sum(-1) <= E * (1 + 1e-15 * 4)).all()
        assert (orc.effort[z] > E).any() and orc.effort_rank[z].max() <= 4
    # the limit changes what the mode computes: a build that ignores the keyword cannot pass the GPU tests
    for q in range(2):
        peak = max(np.abs(b[q]).max() for b in base)
        diff = max(np.abs(b[q] - t[q]).max() for b, t in zip(base, got))
        assert diff > 0.01 * peak
