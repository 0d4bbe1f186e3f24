"""The per-bin array-effort limit of the subband stream (apvast(..., effort_limit_db=), apv_stream_set_effort_limit /
apv_get_effort) against tests/effort_oracle.py.  Tolerances: the table TOL of tests/test_gpu_stream.py.  Effort is quadratic in the
filters, so its bound is twice the filters' (2 w_max); a bin is UNDECIDED when some effort of the oracle's curve lies within that
bound of the limit, and the branch the device takes there may differ from the oracle's.  On these inputs the oracle alone gives no
undecided bin at any hop in float64 and at most 4.6 % (3 of 65 bins) on the last hop at the float32 margin."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from effort_oracle import (EffortConstrainedOracle, EffortForgettingOracle, EffortSubbandOracle, decide)  # noqa: E402
from evaluation_oracle import StreamEvaluation  # noqa: E402
from test_gpu_stat_window import hop, same_outputs  # noqa: E402
from test_gpu_stream import TOL, check_outputs, synth_rirs  # noqa: E402
from test_gpu_stream_evaluation import KEYS, check_hop, validation_rirs  # noqa: E402

DELAY, REF_A, REF_B, MU = 5, 1, 2, 1.0
DTYPES = ["f64", "mixed", "f32"]
CASES = [(200, 8, 16, 1, 256, 128, 6, -12.0), (70, 16, 32, 5, 128, 64, 5, -18.0), (60, 4, 8, 3, 64, 32, 5, -12.0)]


def lin(db):
    return 10.0 ** (np.asarray(db, dtype=np.float64) / 10.0)


def make_pair(N, H, rirA, rirB, V, dtype="f64", seed=0, limit_db=None, oracle=EffortSubbandOracle, okw=None, **kw):
    """an apvast object with the limit and the helper started from the same response buffers (RandomState(seed), as make_pair of
    tests/test_gpu_span_stream.py)"""
    from ap_vast_unofficial_amd.apvast import apvast
    P, L, M = rirA.shape
    okw = dict(okw or {})
    for name, oname in (("mu_profile", "mu_profile"), ("rank_profile", "rank_cap"), ("run_A", "run_A"), ("run_B", "run_B")):
        if name in kw:
            okw[oname] = kw[name]
    ap = apvast(N, rirA, rirB, kw.pop("filter_length", 16), DELAY, REF_A, REF_B, V, MU, 4 * N, hop_size=H, perceptual=False, seed=seed,
                dtype=dtype, effort_limit_db=limit_db, **kw)
    rs = np.random.RandomState(seed)
    init_r = np.stack([1e-3 * rs.randn(N, L, M) for _ in range(4)])
    init_t = np.stack([1e-3 * rs.randn(N, M) for _ in range(2)])
    table = None if limit_db is None else np.broadcast_to(lin(limit_db), (2, N // 2 + 1) if np.ndim(limit_db) < 2 else np.shape(limit_db))
    orc = oracle(N, rirA, rirB, DELAY, REF_A, REF_B, list(range(1, V + 1)), MU, hop_size=H, init_response=init_r,
                 init_target_response=init_t, effort_limit=table, **okw)
    return ap, orc


def undecided_bins(orc, z, dtype):
    E = orc.effort_limit[z][:, None]
    return (np.abs(orc.effort[z] / E - 1.0) <= 2 * TOL[dtype]["w_max"]).any(axis=1)


def check_zone(ap, orc, z, dtype, cap):
    """the last hop's effort outputs and filters of zone program z; returns the share of undecided bins"""
    name, tol = "AB"[z], TOL[dtype]
    eff, rank, gain, w = (getattr(ap, a + name) for a in ("effort_", "effort_rank_", "effort_gain_", "w_"))
    K, V = orc.effort[z].shape
    E, ranks = orc.effort_limit[z], list(range(1, V + 1))
    assert eff.shape == (K, V) and eff.dtype == np.float64 and rank.shape == gain.shape == (K,) and rank.dtype == np.int32
    und = undecided_bins(orc, z, dtype)
    scaled_o, scaled_d = orc.effort_gain[z] != 1.0, gain != 1.0
    lower_o = orc.effort_src[z][:, -1] != V - 1
    print(f"{dtype} {name}: undecided {und.mean():.3f}, scaled {scaled_o.mean():.2f}, lower slot {(lower_o & ~scaled_o).mean():.2f}, "
          f"closest |e/E - 1| {np.abs(orc.effort[z] / E[:, None] - 1).min():.1e}, effort at "
          f"{(np.abs(eff - orc.effort[z]) / orc.effort[z]).max() / (2 * tol['w_max']):.2e} of its bound")
    assert und.mean() <= cap
    # decided bins: the oracle's rank and branch
    assert np.array_equal(rank[~und], orc.effort_rank[z][~und])
    assert np.array_equal(scaled_d[~und], scaled_o[~und])
    # every bin: what the definition gives on the device's own curve
    src_d, rank_d, gain_d = decide(eff, E, ranks)
    assert np.array_equal(rank, rank_d)
    assert (np.abs(gain - gain_d) <= 1e-14 * gain_d).all()
    assert (np.abs(eff - orc.effort[z]) <= 2 * tol["w_max"] * orc.effort[z]).all()
    # the filters: the oracle's unlimited ones put through the device's decisions
    wu = orc.w_unlimited[z]
    wr = np.empty_like(wu)
    for k in range(K):
        for t in range(V):
            s = src_d[k, t]
            wr[k, t] = wu[k, s] if s >= 0 else wu[k, t] * np.sqrt(E[k] / orc.effort[z][k, t])
    wr = wr.transpose(1, 0, 2)
    err = np.linalg.norm(w - wr, axis=-1) / np.linalg.norm(wr, axis=-1)
    assert np.median(err) < tol["w_med"] and err.max() < tol["w_max"], (name, np.median(err), err.max())
    return und.mean()


def run_checked(ap, orc, x, hops, H, dtype, zones=(0, 1)):
    """hops of both; float64: every hop's outputs, with every bin decided at every hop"""
    got, exp = [], []
    for h in range(hops):
        got.append(hop(ap, x, h, H))
        exp.append(hop(orc, x, h, H))
        if dtype == "f64":
            for z in zones:
                assert not undecided_bins(orc, z, dtype).any(), (h, z)
    if dtype == "f64":
        check_outputs(got, exp, TOL[dtype]["out"], TOL[dtype]["tgt"])
    return got, exp


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,L,M,seed,N,H,hops,limit", CASES)
def test_limit_vs_oracle(P, L, M, seed, N, H, hops, limit, dtype):
    rirA, rirB = synth_rirs(P, L, M, seed)
    ap, orc = make_pair(N, H, rirA, rirB, L, dtype, limit_db=limit)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    run_checked(ap, orc, x, hops, H, dtype)
    for z in range(2):
        check_zone(ap, orc, z, dtype, 0.0 if dtype == "f64" else 0.05)
        # both branches run
        assert (orc.effort_gain[z] != 1.0).any() and (orc.effort_src[z][:, -1] >= 0).any()
    assert np.array_equal(ap.effort_limit_db, np.full((2, N // 2 + 1), limit))
    ap.close()


# 2 ---------------------------------------------------------------------------------------------------------------
def _plain(N, H, rirA, rirB, V, dtype, **kw):
    from ap_vast_unofficial_amd.apvast import apvast
    return apvast(N, rirA, rirB, kw.pop("filter_length", 16), DELAY, REF_A, REF_B, V, MU, 4 * N, hop_size=H, perceptual=False, seed=0,
                  dtype=dtype, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_row_per_zone_program(dtype):
    """row A -12 dB, row B +3 dB: nothing exceeds +3 dB, so program B's filters are those of the plain stream bit for bit"""
    P, L, M, seed, N, H, hops, _ = CASES[0]
    K = N // 2 + 1
    rirA, rirB = synth_rirs(P, L, M, seed)
    table = np.stack([np.full(K, -12.0), np.full(K, 3.0)])
    ap, orc = make_pair(N, H, rirA, rirB, L, dtype, limit_db=table)
    plain = _plain(N, H, rirA, rirB, L, dtype)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    for h in range(hops):
        a, p = hop(ap, x, h, H), hop(plain, x, h, H)
        hop(orc, x, h, H)
        assert np.array_equal(np.stack(a[1]), np.stack(p[1])), h
    assert (orc.effort[1] < lin(3.0)).all()
    check_zone(ap, orc, 0, dtype, 0.0 if dtype == "f64" else 0.05)
    assert np.array_equal(ap.w_B, plain.w_B) and np.array_equal(ap.lambda_B, plain.lambda_B) and np.array_equal(ap.lambda_A, plain.lambda_A)
    assert (ap.effort_rank_B == L).all() and (ap.effort_gain_B == 1.0).all() and (ap.effort_B < lin(3.0)).all()
    ap.close()
    plain.close()


def test_two_limited_rows():
    P, L, M, seed, N, H, hops, _ = CASES[0]
    K = N // 2 + 1
    rirA, rirB = synth_rirs(P, L, M, seed)
    ap, orc = make_pair(N, H, rirA, rirB, L, "f64", limit_db=np.stack([np.full(K, -12.0), np.full(K, -5.0)]))
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    run_checked(ap, orc, x, hops, H, "f64")
    for z in range(2):
        assert check_zone(ap, orc, z, "f64", 0.0) == 0.0
    assert not np.array_equal(ap.effort_rank_A, ap.effort_rank_B)
    ap.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_with_the_plain_stream(dtype):
    P, L, M, seed, N, H, hops, _ = CASES[0]
    rirA, rirB = synth_rirs(P, L, M, seed)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    plain, lim = _plain(N, H, rirA, rirB, L, dtype), _plain(N, H, rirA, rirB, L, dtype, effort_limit_db=3.0)
    assert lim.effort_A is None and lim.effort_rank_B is None and lim.effort_gain_A is None             # before the first hop
    for h in range(hops):
        same_outputs(hop(plain, x, h, H), hop(lim, x, h, H))
    for z in "AB":
        assert np.array_equal(getattr(plain, "w_" + z), getattr(lim, "w_" + z))
        assert np.array_equal(getattr(plain, "lambda_" + z), getattr(lim, "lambda_" + z))
        assert (getattr(lim, "effort_rank_" + z) == L).all() and (getattr(lim, "effort_gain_" + z) == 1.0).all()
        w = getattr(lim, "w_" + z).astype(np.complex128)
        e = (w.real ** 2 + w.imag ** 2).sum(-1).T
        assert (np.abs(getattr(lim, "effort_" + z) - e) <= 1e-13 * e).all()
        assert all(getattr(plain, a + z) is None for a in ("effort_", "effort_rank_", "effort_gain_"))
    assert plain.effort_limit_db is None
    plain.close()
    lim.close()


# 3 ---------------------------------------------------------------------------------------------------------------
def test_live_assignment():
    P, L, M, seed, N, H, hops, _ = CASES[0]
    K = N // 2 + 1
    rirA, rirB = synth_rirs(P, L, M, seed)
    ap, orc = make_pair(N, H, rirA, rirB, L, "f64", limit_db=-12.0)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    got, exp = [], []
    for h in range(hops):
        if h == 2:
            ap.effort_limit_db = -5.0
            orc.effort_limit = np.full((2, K), lin(-5.0))
        if h == 4:
            t = np.stack([np.linspace(-18.0, -6.0, K), np.full(K, np.inf)])
            ap.effort_limit_db = t
            orc.effort_limit = lin(t)
        got.append(hop(ap, x, h, H))
        exp.append(hop(orc, x, h, H))
        for z in range(2):
            assert not undecided_bins(orc, z, "f64").any(), (h, z)
            assert np.array_equal(getattr(ap, "effort_rank_" + "AB"[z]), orc.effort_rank[z]), (h, z)
    check_outputs(got, exp, TOL["f64"]["out"], TOL["f64"]["tgt"])
    for z in range(2):
        check_zone(ap, orc, z, "f64", 0.0)
    assert (ap.effort_rank_B == L).all()
    with pytest.raises(ValueError, match="effort_limit_db"):
        ap.effort_limit_db = None
    with pytest.raises(ValueError, match="effort_limit_db"):
        ap.effort_limit_db = np.full(K, np.nan)
    ap.close()
    plain = _plain(N, H, rirA, rirB, L, "f64")
    with pytest.raises(ValueError, match="effort_limit_db was not given"):
        plain.effort_limit_db = -12.0
    plain.close()


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "constrained", "fir"])
@pytest.mark.parametrize("L,M,N,dtype", [(8, 16, 256, "f64"), (16, 32, 512, "f64"), (16, 32, 512, "f32"), (24, 32, 128, "f64")])
def test_process_signal_equals_hop_loop(L, M, N, dtype, variant):
    """every schedule of the whole-signal call (order 16: the hops of a chunk in one launch; other orders: hop by hop on the back
    streams; constrained and FIR streams: their chunk schedule), chunk boundaries included, on the schedule of the stream without
    the keyword"""
    H, hops = N // 2, 40
    rirA, rirB = synth_rirs(200, L, M, 1)
    kw = {"plain": {}, "constrained": dict(constrain_filter_length=True), "fir": dict(constrain_filter_length=True, synthesis="fir")}[variant]
    a, b = (_plain(N, H, rirA, rirB, 4, dtype, effort_limit_db=-12.0, **kw) for _ in range(2))
    c = _plain(N, H, rirA, rirB, 4, dtype, **kw)
    x = np.random.default_rng(7).standard_normal((2, hops * H))
    loop = [hop(a, x, h, H) for h in range(hops)]
    sig = b.process_signal(x[0], x[1])
    c.process_signal(x[0], x[1])
    assert b.signal_schedule == c.signal_schedule and sum(b.signal_schedule) == hops
    for q in range(4):
        for v in range(len(sig[q])):
            assert np.array_equal(np.concatenate([o[q][v] for o in loop]), sig[q][v]), (q, v)
    for z in "AB":
        assert np.array_equal(getattr(a, "w_" + z), getattr(b, "w_" + z))
        for name in ("effort_", "effort_rank_", "effort_gain_"):
            assert np.array_equal(getattr(a, name + z), getattr(b, name + z)), name + z
        assert not np.array_equal(getattr(b, "w_" + z), getattr(c, "w_" + z))                  # the limit acts
    for ap in (a, b, c):
        ap.close()


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["span", "window", "forgetting", "constrained", "run_B_only"])
def test_combinations_vs_oracle(combo):
    P, L, M, seed, N, H, hops, limit = CASES[0]
    K, J = N // 2 + 1, 16
    rirA, rirB = synth_rirs(P, L, M, seed)
    zones = (0, 1)
    if combo == "span":
        m, cap = np.geomspace(1.0, 10.0, K), np.linspace(L, 1, K).round().astype(int)
        ap, orc = make_pair(N, H, rirA, rirB, L, limit_db=limit, mu_profile=np.stack([m, m[::-1] * 0.5]),
                            rank_profile=np.stack([cap, np.roll(cap, K // 3)]))
    elif combo == "window":
        ap, orc = make_pair(N, H, rirA, rirB, L, limit_db=limit, okw=dict(stat_hops=3), statistics_hops=3)
    elif combo == "forgetting":
        ap, orc = make_pair(N, H, rirA, rirB, L, limit_db=limit, oracle=EffortForgettingOracle, okw=dict(beta=0.9),
                            statistics_forgetting=0.9)
    elif combo == "constrained":
        ap, orc = make_pair(N, H, rirA, rirB, L, limit_db=limit, oracle=EffortConstrainedOracle, okw=dict(filter_taps=J),
                            filter_length=J, constrain_filter_length=True)
    else:
        ap, orc = make_pair(N, H, rirA, rirB, L, limit_db=limit, run_A=False)
        zones = (1,)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    run_checked(ap, orc, x, hops, H, "f64", zones)
    for z in zones:
        name = "AB"[z]
        assert np.array_equal(getattr(ap, "effort_rank_" + name), orc.effort_rank[z])
        assert (np.abs(getattr(ap, "effort_" + name) - orc.effort[z]) <= 2 * TOL["f64"]["w_max"] * orc.effort[z]).all()
        wr = orc.w[z].transpose(1, 0, 2)                                                    # limited (and projected)
        err = np.linalg.norm(getattr(ap, "w_" + name) - wr, axis=-1) / np.linalg.norm(wr, axis=-1)
        assert np.median(err) < TOL["f64"]["w_med"] and err.max() < TOL["f64"]["w_max"], (name, np.median(err), err.max())
    if combo == "constrained":
        for z, name in enumerate("AB"):
            tr, tg = orc.w_time[z], np.asarray(getattr(ap, "w_time_" + name))                 # the taps of the limited filters
            assert tg.shape == tr.shape and np.abs(tg - tr).max() <= TOL["f64"]["w_max"] * np.abs(tr).max()
    if combo == "run_B_only":
        assert ap.effort_A is None and ap.effort_rank_A is None and ap.effort_gain_A is None
    ap.close()


def test_with_the_evaluation_stage():
    """the evaluation stage reads the hop's outputs: with a limit it predicts the pressures of the limited filters' outputs, and its
    totals are the sums over the hops"""
    N, H, hops, L, M, Pv, Mv = 32, 16, 5, 3, 4, 9, 5
    rirA, rirB = synth_rirs(12, L, M, 1)
    rvA, rvB = validation_rirs(Pv, L, Mv)
    ap, orc = make_pair(N, H, rirA, rirB, L, limit_db=-12.0, validation_rir_A=rvA, validation_rir_B=rvB)
    import test_gpu_stream_evaluation as tse
    assert (tse.L, tse.M) == (L, M)
    ev = StreamEvaluation(rvA, rvB, [1, 2, 3])
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    worst, run = [0.0, 0.0], None
    for h in range(hops):
        out = hop(ap, x, h, H)
        hop(orc, x, h, H)
        eh = check_hop(ap, ev.hop(out), H, Pv, worst)
        run = {q: eh[q][0] for q in KEYS} if run is None else {q: run[q] + eh[q][0] for q in KEYS}
        tot = ap.evaluation_totals()
        for q in KEYS:
            assert np.array_equal(tot[q], run[q]), (h, q)
    for z, name in enumerate("AB"):
        und = undecided_bins(orc, z, "f64")
        assert np.array_equal(getattr(ap, "effort_rank_" + name)[~und], orc.effort_rank[z][~und])
        assert (orc.effort[z] > orc.effort_limit[z][:, None]).any()
    ap.close()


# 6 ---------------------------------------------------------------------------------------------------------------
def test_state_keys_and_resume():
    P, L, M, seed, N, H, hops, limit = CASES[2]
    rirA, rirB = synth_rirs(P, L, M, seed)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    plain = _plain(N, H, rirA, rirB, L, "f64")
    a, b = (_plain(N, H, rirA, rirB, L, "f64", effort_limit_db=limit) for _ in range(2))
    for h in range(3):
        hop(plain, x, h, H)
        hop(a, x, h, H)
    st = a.get_state()
    assert sorted(st) == sorted(plain.get_state())
    b.set_state(st)
    assert b.effort_A is None                                                                 # b has run no hop of its own
    for h in range(3, hops):
        same_outputs(hop(a, x, h, H), hop(b, x, h, H))
    for z in "AB":
        for name in ("w_", "effort_", "effort_rank_", "effort_gain_"):
            assert np.array_equal(getattr(a, name + z), getattr(b, name + z)), name + z
    for ap in (plain, a, b):
        ap.close()


def test_errors():
    from ap_vast_unofficial_amd._capi import ApvError
    P, L, M, seed, N, H, hops, limit = CASES[2]
    K = N // 2 + 1
    rirA, rirB = synth_rirs(P, L, M, seed)
    x = np.random.default_rng(99).standard_normal((2, 2 * H))
    # a first limit once the stream is initialised: refused, and the stream carries on unchanged
    plain, ref = _plain(N, H, rirA, rirB, L, "f64"), _plain(N, H, rirA, rirB, L, "f64")
    same_outputs(hop(plain, x, 0, H), hop(ref, x, 0, H))
    with pytest.raises(ApvError):
        plain._eng.set_effort_limit(np.ones(K))
    with pytest.raises(ApvError):
        plain._eng.effort(0)
    same_outputs(hop(plain, x, 1, H), hop(ref, x, 1, H))
    plain.close()
    ref.close()
    lim = _plain(N, H, rirA, rirB, L, "f64", effort_limit_db=limit)
    for bad in (np.zeros(K), -np.ones(K), np.full(K, np.nan)):
        with pytest.raises(ApvError):
            lim._eng.set_effort_limit(bad)
    with pytest.raises(ApvError):
        lim._eng.effort(2)
    with pytest.raises(ValueError):
        lim._eng.set_effort_limit(np.ones(K + 1))
    lim._eng.set_effort_limit(np.full((2, K), np.inf))                                       # +inf is a value like any other
    lim.close()
