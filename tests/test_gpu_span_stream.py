"""The per-bin span of the subband stream (apvast(..., mu_profile=, rank_profile=, contrast_floor_db=), apv_set_span / apv_get_span)
against tests/span_oracle.py.  Tolerances: the table TOL of tests/test_gpu_stream.py; span_rank is an integer and is compared
exactly wherever the oracle's own curve decides it (see test_floor_vs_oracle)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from evaluation_oracle import StreamEvaluation  # noqa: E402
from fir_synthesis_oracle import FirStreamReference  # noqa: E402
from span_oracle import SpanConstrainedOracle, SpanForgettingOracle, SpanSubbandOracle, span_gevd_vast  # noqa: E402
from test_gpu_stat_window import hop, same_outputs  # noqa: E402
from test_gpu_stream import TOL, check_last_hop_state, check_outputs, synth_rirs  # noqa: E402
from test_gpu_stream_evaluation import check_hop, validation_rirs  # noqa: E402

DELAY, REF_A, REF_B, MU = 5, 1, 2, 1.0
DTYPES = ["f64", "mixed", "f32"]


def make_pair(N, H, rirA, rirB, V, dtype="f64", seed=0, mu_profile=None, rank_profile=None, floor_db=None, oracle=SpanSubbandOracle,
              okw=None, **kw):
    """an apvast object with the span and the helper started from the same response buffers (RandomState(seed), as make_pair of
    tests/test_gpu_stat_window.py)"""
    from ap_vast_unofficial_amd.apvast import apvast
    P, L, M = rirA.shape
    ap = apvast(N, rirA, rirB, kw.pop("filter_length", 16), DELAY, REF_A, REF_B, V, MU, 4 * N, hop_size=H, perceptual=False, seed=seed,
                dtype=dtype, mu_profile=mu_profile, rank_profile=rank_profile, contrast_floor_db=floor_db, **kw)
    rs = np.random.RandomState(seed)
    init_r = np.stack([1e-3 * rs.randn(N, L, M) for _ in range(4)])
    init_t = np.stack([1e-3 * rs.randn(N, M) for _ in range(2)])
    orc = oracle(N, rirA, rirB, DELAY, REF_A, REF_B, list(range(1, V + 1)), MU, hop_size=H, init_response=init_r,
                 init_target_response=init_t, mu_profile=mu_profile, rank_cap=rank_profile, floor_db=floor_db, **(okw or {}))
    return ap, orc


def profiles(K, L):
    """mu rising tenfold over the bins, the cap falling from L to 1; program B's rows differ from program A's"""
    m = np.geomspace(1.0, 10.0, K)
    cap = np.linspace(L, 1, K).round().astype(int)
    return np.stack([m, m[::-1] * 0.5]), np.stack([cap, np.roll(cap, K // 3)])


def run(ap, orc, x, hops, H):
    return [hop(ap, x, h, H) for h in range(hops)], [hop(orc, x, h, H) for h in range(hops)]


def check_ranks(ap, orc):
    for z, name in enumerate("AB"):
        assert np.array_equal(getattr(ap, "span_rank_" + name), orc.span_rank[z]), name


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_profiles_vs_oracle(dtype):
    """8 x 16, N = 256, 6 hops: every hop's outputs, the last hop's spectra, w, lambda and span_rank"""
    N, H, hops, L = 256, 128, 6, 8
    rirA, rirB = synth_rirs(200, L, 16, 1)
    m, cap = profiles(N // 2 + 1, L)
    ap, orc = make_pair(N, H, rirA, rirB, L, dtype, mu_profile=m, rank_profile=cap)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    got, exp = run(ap, orc, x, hops, H)
    check_outputs(got, exp, TOL[dtype]["out"], TOL[dtype]["tgt"])
    check_last_hop_state(ap, orc, TOL[dtype], N // 2 + 1, L, 16)
    check_ranks(ap, orc)
    assert ap.span_contrast_A is None and ap.span_contrast_B is None
    assert np.array_equal(ap.mu_profile, m) and np.array_equal(ap.rank_profile, cap) and ap.contrast_floor_db is None
    ap.close()


# 2 ---------------------------------------------------------------------------------------------------------------
FLOOR_CASES = [(200, 8, 16, 1, 256, 128, 6, 5.0), (70, 16, 32, 5, 128, 64, 5, 5.0), (60, 4, 8, 3, 64, 32, 5, 3.0)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,L,M,seed,N,H,hops,floor", FLOOR_CASES)
def test_floor_vs_oracle(P, L, M, seed, N, H, hops, floor, dtype):
    """A bin is undecided if some c_v of the oracle lies within TOL[dtype]["lam"] lambda_1 of phi.  On decided bins span_rank equals
    the oracle's; on every bin it is the prefix count of the device's own curve and w is the oracle's filter at the device's rank.
    Undecided bins: at most 1 % (f64), 5 % (f32 / mixed); the oracle alone gives 0 % and at most 3.1 % (2 of 65 bins) on these inputs."""
    K = N // 2 + 1
    rirA, rirB = synth_rirs(P, L, M, seed)
    ap, orc = make_pair(N, H, rirA, rirB, L, dtype, floor_db=floor)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    run(ap, orc, x, hops, H)
    tol, phi = TOL[dtype], 10.0 ** (floor / 10.0)
    ranks = list(range(1, L + 1))
    for z, name in enumerate("AB"):
        rank, con, lam = getattr(ap, "span_rank_" + name), getattr(ap, "span_contrast_" + name), orc.lam[z]
        assert rank.shape == (K,) and rank.dtype == np.int32 and con.shape == (K, L)
        undecided = (np.abs(orc.span_contrast[z] - phi) <= tol["lam"] * lam[:, :1]).any(axis=1)
        share = (np.abs(con - orc.span_contrast[z]).max(axis=1) / lam[:, 0]).max() / tol["lam"]
        print(f"{L} x {M} {dtype} {name}: oracle ranks {orc.span_rank[z].min()}..{orc.span_rank[z].max()}, undecided "
              f"{undecided.mean():.3f}, {(rank != orc.span_rank[z]).sum()} bins off the oracle's rank, contrast at {share:.2e} of its bound")
        assert undecided.mean() <= (0.01 if dtype == "f64" else 0.05)
        assert np.array_equal(rank[~undecided], orc.span_rank[z][~undecided])
        assert np.array_equal(rank, np.maximum(np.cumprod(con >= phi, axis=1).sum(axis=1), 1))
        assert share <= 1.0
        RB, RD, r = orc.window_statistics(z)
        wr = span_gevd_vast(RB, RD, r, MU, ranks, 1e-7, None, rank, None)[0].transpose(1, 0, 2)
        err = np.linalg.norm(getattr(ap, "w_" + name) - wr, axis=-1) / np.linalg.norm(wr, axis=-1)
        assert np.median(err) < tol["w_med"] and err.max() < tol["w_max"], (name, np.median(err), err.max())
    ap.close()


# 3 ---------------------------------------------------------------------------------------------------------------
def _plain(N, H, rirA, rirB, V, dtype, mu=MU, **kw):
    from ap_vast_unofficial_amd.apvast import apvast
    return apvast(N, rirA, rirB, 16, DELAY, REF_A, REF_B, V, mu, 4 * N, hop_size=H, perceptual=False, seed=0, dtype=dtype, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_identities_with_the_plain_stream(dtype):
    N, H, hops, L = 256, 128, 5, 8
    K = N // 2 + 1
    rirA, rirB = synth_rirs(200, L, 16, 1)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    plain = _plain(N, H, rirA, rirB, L, dtype)
    ones = _plain(N, H, rirA, rirB, L, dtype, mu_profile=np.ones(K), rank_profile=np.full(K, L), contrast_floor_db=-300.0)
    scaled = _plain(N, H, rirA, rirB, L, dtype, mu=4.0)
    uniform = _plain(N, H, rirA, rirB, L, dtype, mu=8.0, mu_profile=np.full((2, K), 0.5))
    for h in range(hops):
        same_outputs(hop(plain, x, h, H), hop(ones, x, h, H))
        same_outputs(hop(scaled, x, h, H), hop(uniform, x, h, H))
    for z in "AB":
        for a, b in ((plain, ones), (scaled, uniform)):
            assert np.array_equal(getattr(a, "w_" + z), getattr(b, "w_" + z))
            assert np.array_equal(getattr(a, "lambda_" + z), getattr(b, "lambda_" + z))
        assert (getattr(ones, "span_rank_" + z) == L).all()
        assert getattr(plain, "span_rank_" + z) is None and getattr(uniform, "span_contrast_" + z) is None
    for ap in (plain, ones, scaled, uniform):
        ap.close()


@pytest.mark.parametrize("L,M,N,dtype", [(8, 16, 256, "f64"), (16, 32, 512, "f64"), (16, 32, 512, "f32"), (24, 32, 128, "f64")])
def test_process_signal_equals_hop_loop(L, M, N, dtype):
    """the chunked schedule (order 16: the hops of a chunk in one launch; other orders: hop by hop on two streams), chunk boundaries
    included, on the same schedule as the stream without the keywords"""
    H, hops, K = N // 2, 40, N // 2 + 1
    rirA, rirB = synth_rirs(200, L, M, 1)
    m, cap = profiles(K, L)
    kw = dict(mu_profile=m, rank_profile=cap, contrast_floor_db=3.0)
    a, b, c = _plain(N, H, rirA, rirB, 4, dtype, **kw), _plain(N, H, rirA, rirB, 4, dtype, **kw), _plain(N, H, rirA, rirB, 4, dtype)
    x = np.random.default_rng(7).standard_normal((2, hops * H))
    loop = [hop(a, x, h, H) for h in range(hops)]
    sig = b.process_signal(x[0], x[1])
    c.process_signal(x[0], x[1])
    assert b.signal_schedule == c.signal_schedule and sum(b.signal_schedule) == hops
    for q in range(4):
        for v in range(4):
            assert np.array_equal(np.concatenate([o[q][v] for o in loop]), sig[q][v]), (q, v)
    for z in "AB":
        assert np.array_equal(getattr(a, "w_" + z), getattr(b, "w_" + z))
        assert np.array_equal(getattr(a, "span_rank_" + z), getattr(b, "span_rank_" + z))
        assert np.array_equal(getattr(a, "span_contrast_" + z), getattr(b, "span_contrast_" + z))
        assert getattr(a, "span_rank_" + z).max() <= 4
    for ap in (a, b, c):
        ap.close()


# 4 ---------------------------------------------------------------------------------------------------------------
def test_live_assignment():
    N, H, hops, L = 256, 128, 6, 8
    K = N // 2 + 1
    rirA, rirB = synth_rirs(200, L, 16, 1)
    m, cap = profiles(K, L)
    ap, orc = make_pair(N, H, rirA, rirB, L, "f64", mu_profile=m, rank_profile=cap, floor_db=2.0)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    got, exp = [], []
    for h in range(hops):
        if h == 2:
            ap.mu_profile = m[::-1]
            orc.mu_profile = m[::-1]
            ap.mu = orc.mu = 3.0
        if h == 4:
            ap.rank_profile = cap[0][::-1]                 # (K,): both programs
            orc.rank_cap = np.stack([cap[0][::-1]] * 2)
            ap.contrast_floor_db = orc.floor_db = 6.0
        got.append(hop(ap, x, h, H))
        exp.append(hop(orc, x, h, H))
        if h in (1, 3, 5):
            check_ranks(ap, orc)
    check_outputs(got, exp, TOL["f64"]["out"], TOL["f64"]["tgt"])
    check_last_hop_state(ap, orc, TOL["f64"], K, L, 16)
    assert ap.mu == 3.0 and ap.contrast_floor_db == 6.0
    with pytest.raises(ValueError, match="rank_profile"):
        ap.rank_profile = np.full(K, L + 1)
    ap.close()
    only_mu = _plain(N, H, rirA, rirB, L, "f64", mu_profile=m)
    with pytest.raises(ValueError, match="rank_profile was not given"):
        only_mu.rank_profile = cap
    with pytest.raises(ValueError, match="contrast_floor_db was not given"):
        only_mu.contrast_floor_db = 3.0
    only_mu.close()


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["window", "forgetting", "constrained_fir"])
def test_combinations_vs_oracle(combo):
    N, H, hops, L, J = 256, 128, 6, 8, 16
    K = N // 2 + 1
    rirA, rirB = synth_rirs(200, L, 16, 1)
    m, cap = profiles(K, L)
    span = dict(mu_profile=m, rank_profile=cap, floor_db=3.0)
    if combo == "window":
        ap, orc = make_pair(N, H, rirA, rirB, L, okw=dict(stat_hops=3), statistics_hops=3, **span)
    elif combo == "forgetting":
        ap, orc = make_pair(N, H, rirA, rirB, L, oracle=SpanForgettingOracle, okw=dict(beta=0.8), statistics_forgetting=0.8, **span)
    else:
        ap, orc = make_pair(N, H, rirA, rirB, L, oracle=SpanConstrainedOracle, okw=dict(filter_taps=J), filter_length=J,
                            constrain_filter_length=True, synthesis="fir", **span)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    if combo == "constrained_fir":
        # every hop's outputs against the FIR reference fed with the helper's taps (as run_vs_oracle of tests/test_gpu_fir_synthesis.py),
        # then the projected filters of the last hop
        ref = FirStreamReference(J, H, L, L, DELAY, REF_A)
        got, exp = [], []
        for h in range(hops):
            got.append(hop(ap, x, h, H))
            hop(orc, x, h, H)
            exp.append(ref.hop(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H], orc.w_time)[0])
        exp = [tuple(np.stack(e[q]) if q < 2 else e[q][0] for q in range(4)) for e in exp]      # the shapes the stream oracles return
        check_outputs(got, exp, TOL["f64"]["out"], TOL["f64"]["tgt"])
    else:
        got, exp = run(ap, orc, x, hops, H)
    check_ranks(ap, orc)
    if combo == "constrained_fir":
        for z, name in enumerate("AB"):
            wr = orc.w[z].transpose(1, 0, 2)
            err = np.linalg.norm(getattr(ap, "w_" + name) - wr, axis=-1) / np.linalg.norm(wr, axis=-1)
            assert np.median(err) < TOL["f64"]["w_med"] and err.max() < TOL["f64"]["w_max"], (name, np.median(err), err.max())
    else:
        check_outputs(got, exp, TOL["f64"]["out"], TOL["f64"]["tgt"])
        check_last_hop_state(ap, orc, TOL["f64"], K, L, 16)
    ap.close()


def test_with_the_evaluation_stage():
    """the evaluation stage reads the hop's outputs: with a span it still predicts the pressures of what the call returned"""
    N, H, hops, L, M, Pv, Mv = 32, 16, 5, 3, 4, 9, 5
    K = N // 2 + 1
    rirA, rirB = synth_rirs(12, L, M, 1)
    rvA, rvB = validation_rirs(Pv, L, Mv)
    m, cap = profiles(K, L)
    ap, orc = make_pair(N, H, rirA, rirB, L, mu_profile=m, rank_profile=cap, floor_db=3.0, validation_rir_A=rvA, validation_rir_B=rvB)
    import test_gpu_stream_evaluation as tse
    assert (tse.L, tse.M) == (L, M)
    ev = StreamEvaluation(rvA, rvB, [1, 2, 3])
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    worst = [0.0, 0.0]
    for h in range(hops):
        out = hop(ap, x, h, H)
        hop(orc, x, h, H)
        check_hop(ap, ev.hop(out), H, Pv, worst)
    check_ranks(ap, orc)
    ap.close()


# 6 ---------------------------------------------------------------------------------------------------------------
def test_errors():
    from ap_vast_unofficial_amd._capi import ApvError
    N, H, L = 256, 128, 8
    K = N // 2 + 1
    rirA, rirB = synth_rirs(200, L, 16, 1)
    x = np.random.default_rng(99).standard_normal((2, 4 * H))
    m, cap = profiles(K, L)
    # a part added once the stream runs: refused, and the stream carries on unchanged
    ap, ref = _plain(N, H, rirA, rirB, L, "f64", mu_profile=m), _plain(N, H, rirA, rirB, L, "f64", mu_profile=m)
    for h in range(2):
        same_outputs(hop(ap, x, h, H), hop(ref, x, h, H))
    with pytest.raises(ApvError):
        ap._eng.set_span(mu_profile=m, rank_cap=cap)
    with pytest.raises(ApvError):
        ap._eng.set_span(rank_cap=cap)
    with pytest.raises(ApvError):
        ap._eng.span(2)
    for h in range(2, 4):
        same_outputs(hop(ap, x, h, H), hop(ref, x, h, H))
    assert ap.span_contrast_A is None and ap.span_rank_A.shape == (K,)
    ap.close()
    ref.close()
    # a plain stream has no span, before or after apv_stream_init
    plain = _plain(N, H, rirA, rirB, L, "f64")
    hop(plain, x, 0, H)
    with pytest.raises(ApvError):
        plain._eng.span(0)
    with pytest.raises(ApvError):
        plain._eng.set_span(mu_profile=m)
    assert plain.span_rank_A is None and plain.span_contrast_B is None
    plain.close()
