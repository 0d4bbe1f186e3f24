"""Exponentially forgetting statistics of the subband stream (apvast(..., statistics_forgetting=beta),
apv_stream_set_stat_forgetting) against the forgetting CPU oracle (tests/forgetting_oracle.py).  Tolerances: the table TOL of
tests/test_gpu_stream.py throughout -- the oracle's two float64 solvers lie 2e-15 ... 2e-14 of the output peak apart on every
input used here, the rank-deficient first hops included, so the plain bounds apply as they do for the window."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from forgetting_oracle import ForgettingSubbandOracle  # noqa: E402
from test_gpu_stat_window import hop, same_outputs  # noqa: E402
from test_gpu_stream import TOL, cfg3_rirs, check_last_hop_state, check_outputs, pink, synth_rirs  # noqa: E402


def make_pair(N, H, rirA, rirB, delay, refA, refB, V, mu, beta, run_A=True, run_B=True, seed=0, dtype="f64", perceptual=None,
              sampling_rate=48000, fullscale=94.0):
    """an apvast object with statistics_forgetting = beta and the forgetting oracle started from the same response buffers"""
    from ap_vast_unofficial_amd.apvast import apvast
    P, L, M = rirA.shape
    ap = apvast(N, rirA, rirB, 16, delay, refA, refB, V, mu, 4 * N, hop_size=H, run_A=run_A, run_B=run_B,
                perceptual=perceptual is not None, seed=seed, dtype=dtype, statistics_forgetting=beta, sampling_rate=sampling_rate,
                fullscale_db_spl=fullscale)
    rs = np.random.RandomState(seed)
    init_r = np.stack([1e-3 * rs.randn(N, L, M) for _ in range(4)])
    init_t = np.stack([1e-3 * rs.randn(N, M) for _ in range(2)])
    orc = ForgettingSubbandOracle(N, rirA, rirB, delay, refA, refB, list(range(1, V + 1)), mu, hop_size=H, run_A=run_A,
                                  run_B=run_B, init_response=init_r, init_target_response=init_t, perceptual=perceptual, beta=beta)
    return ap, orc


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "mixed", "f32"])
def test_forgetting_vs_oracle(dtype):
    """8 x 16, N = 256, beta = 0.8, 8 hops: every hop's outputs, the last hop's spectra, w, lambda."""
    rirA, rirB = synth_rirs(200, 8, 16, 1)
    N, H, hops = 256, 128, 8
    ap, orc = make_pair(N, H, rirA, rirB, 12, 2, 5, 4, 1.0, 0.8, dtype=dtype)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    got = [hop(ap, x, h, H) for h in range(hops)]
    exp = [hop(orc, x, h, H) for h in range(hops)]
    check_outputs(got, exp, TOL[dtype]["out"], TOL[dtype]["tgt"])
    check_last_hop_state(ap, orc, TOL[dtype], 129, 8, 16)
    ap.close()


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_beta_one_is_the_unfilled_window_bit_for_bit(dtype):
    """statistics_forgetting = 1.0 against statistics_hops = 8 over 5 hops: the window sums oldest first with the new hop last,
    an fma with beta = 1 is that same sum, and the Gram tiles are the same code."""
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(200, 8, 16, 1)
    N, H, hops = 256, 128, 5
    mk = lambda **kw: apvast(N, rirA, rirB, 16, 12, 2, 5, 4, 1.0, 4 * N, hop_size=H, perceptual=False, seed=0, dtype=dtype, **kw)
    a, b = mk(statistics_forgetting=1.0), mk(statistics_hops=8)
    x = np.random.default_rng(3).standard_normal((2, hops * H))
    for h in range(hops):
        same_outputs(hop(a, x, h, H), hop(b, x, h, H))
        for z in "AB":
            assert np.array_equal(getattr(a, "w_" + z), getattr(b, "w_" + z)), (h, z)
            assert np.array_equal(getattr(a, "lambda_" + z), getattr(b, "lambda_" + z)), (h, z)
    a.close()
    b.close()


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,M,hops", [(64, 16, 6), (128, 64, 4)])
def test_forgetting_more_loudspeakers_than_control_points(L, M, hops):
    """Orders 64 and 128 with M < L, beta = 0.9, every hop held to the plain TOL["f64"].  The first hops hold fewer than L rows
    and the later ones geometrically weighted rows; the oracle's two float64 solvers lie 1.2e-14 (64 x 16) and 2.0e-14 (128 x 64)
    of the output peak apart over every hop, so the plain bound stands.  At order 64 no hop of such a stream may reach
    csrc/kernels_gevd64.hip (GevdParams::no_gevd64 for the life of the stream, csrc/stream.hip)."""
    rirA, rirB = synth_rirs(70, L, M, 5)
    N, H = 128, 64
    ap, orc = make_pair(N, H, rirA, rirB, 5, 1, 2, 2, 1.0, 0.9)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    got = [hop(ap, x, h, H) for h in range(hops)]
    exp = [hop(orc, x, h, H) for h in range(hops)]
    for q in range(2):
        peak = max(np.abs(e[q]).max() for e in exp)
        print(f"{L} x {M} zone {q}: per-hop output error / peak",
              ["%.1e" % (np.abs(np.stack(g[q]) - e[q]).max() / peak) for g, e in zip(got, exp)])
    check_outputs(got, exp, TOL["f64"]["out"], TOL["f64"]["tgt"])
    check_last_hop_state(ap, orc, TOL["f64"], 65, L, M)
    ap.close()


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_A,run_B", [(True, True), (True, False)])
def test_forgetting_cfg3_shape(run_A, run_B):
    """16 x 32, N = 2048, 800 taps, pink input, beta = 0.9, 5 hops: the captured hop graphs (hops 3 and later replay) and the
    order-16 explicit kernel."""
    rirA, rirB = cfg3_rirs()
    hops, H = 5, 1024
    x = pink(hops * H, 2024)
    ap, orc = make_pair(2048, H, rirA, rirB, 16, 3, 7, 8, 1.0, 0.9, run_A=run_A, run_B=run_B)
    got = [hop(ap, x, h, H) for h in range(hops)]
    exp = [hop(orc, x, h, H) for h in range(hops)]
    check_outputs(got, exp, TOL["f64"]["out"], TOL["f64"]["tgt"])
    check_last_hop_state(ap, orc, TOL["f64"], 1025, 16, 32, tuple(z for z, r in enumerate((run_A, run_B)) if r))
    ap.close()


# 5 ---------------------------------------------------------------------------------------------------------------
def test_statistics_attributes_are_the_running_sums():
    """R_*, r_* after hops 2 and 6 against the helper's forgetting_statistics (1e-12 of the largest entry); U_A through jdiag's
    contract."""
    rirA, rirB = synth_rirs(200, 8, 16, 1)
    N, H, L = 256, 128, 8
    ap, orc = make_pair(N, H, rirA, rirB, 12, 2, 5, 4, 1.0, 0.8)
    x = np.random.default_rng(99).standard_normal((2, 7 * H))
    for h in range(7):
        hop(ap, x, h, H)
        hop(orc, x, h, H)
        if h not in (2, 6):
            continue
        for z, names in enumerate((("R_A_to_A", "R_A_to_B", "r_A"), ("R_B_to_B", "R_B_to_A", "r_B"))):
            for name, ref in zip(names, orc.forgetting_statistics(z)):
                g = getattr(ap, name)
                err = np.abs(g - ref).max() / np.abs(ref).max()
                print(f"hop {h} {name}: {err:.2e}")
                assert err < 1e-12, (h, name, err)
        RB, RD, _ = orc.forgetting_statistics(0)
        U, lam = ap.U_A, ap.lambda_A
        UH = U.conj().transpose(0, 2, 1)
        assert np.abs(UH @ (RD + 1e-7 * np.eye(L)) @ U - np.eye(L)).max() < 1e-10
        assert np.abs(UH @ RB @ U - lam[:, :, None] * np.eye(L)).max() < 1e-10 * lam.max()
    ap.close()


# 6 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,M,N,dtype", [(8, 16, 256, "f64"), (8, 16, 256, "f32"), (16, 32, 512, "f64"), (16, 32, 512, "f32")])
def test_process_signal_equals_hop_loop(L, M, N, dtype):
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(200, L, M, 1)
    H, hops = N // 2, 40
    mk = lambda: apvast(N, rirA, rirB, 16, 12, 2, 5, 4, 1.0, 4 * N, hop_size=H, perceptual=False, seed=0, dtype=dtype,
                        statistics_forgetting=0.9)
    a, b = mk(), mk()
    x = np.random.default_rng(7).standard_normal((2, hops * H))
    loop = [hop(a, x, h, H) for h in range(hops)]
    sig = b.process_signal(x[0], x[1])
    for q in range(4):
        for v in range(4):
            assert np.array_equal(np.concatenate([o[q][v] for o in loop]), sig[q][v]), (q, v)
    for z in "AB":
        assert np.array_equal(getattr(a, "w_" + z), getattr(b, "w_" + z))
    a.close()
    b.close()


# 7 ---------------------------------------------------------------------------------------------------------------
def test_resume_is_bit_for_bit():
    """get_state after 3 hops -> set_state into a fresh object made with another seed, 5 more hops on both."""
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(200, 8, 16, 1)
    N, H = 256, 128
    mk = lambda seed, **kw: apvast(N, rirA, rirB, 16, 12, 2, 5, 4, 1.0, 4 * N, hop_size=H, perceptual=False, seed=seed, **kw)
    a, b = mk(0, statistics_forgetting=0.8), mk(1, statistics_forgetting=0.8)
    x = np.random.default_rng(5).standard_normal((2, 8 * H))
    for h in range(3):
        hop(a, x, h, H)
    st = a.get_state()
    assert st["statistics_forgetting_sums"].shape == (2, 129, 2 * 8 * 8 + 8)
    assert st["statistics_forgetting_sums"].dtype == np.complex128
    assert np.abs(st["statistics_forgetting_sums"]).max() > 0
    b.set_state(st)
    for h in range(3, 8):
        same_outputs(hop(a, x, h, H), hop(b, x, h, H))
    sa, sb = a.get_state(), b.get_state()
    assert sorted(sa) == sorted(sb)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    with pytest.raises(ValueError, match="statistics_forgetting_sums"):
        b.set_state({"statistics_forgetting_sums": st["statistics_forgetting_sums"][:1]})
    d = mk(0)
    assert "statistics_forgetting_sums" not in d.get_state()
    with pytest.raises(KeyError):
        d.set_state({"statistics_forgetting_sums": st["statistics_forgetting_sums"]})
    for o in (a, b, d):
        o.close()


# 8 ---------------------------------------------------------------------------------------------------------------
def test_reassigned_response_and_mu_keep_the_sums():
    """rir_A reassigned before hop 4, mu before hop 6, beta = 0.8: what has been accumulated keeps the statistics it was formed
    with, as the reference's statistics buffer keeps old samples."""
    rirA, rirB = synth_rirs(200, 8, 16, 1)
    newA = synth_rirs(200, 8, 16, 77)[0]
    N, H, hops = 256, 128, 8
    ap, orc = make_pair(N, H, rirA, rirB, 12, 2, 5, 4, 1.0, 0.8)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    got, exp = [], []
    for h in range(hops):
        if h == 4:
            ap.rir_A = newA
            orc.rir = (np.asarray(newA, float), orc.rir[1])
        if h == 6:
            ap.mu = orc.mu = 30.0
        got.append(hop(ap, x, h, H))
        exp.append(hop(orc, x, h, H))
    check_outputs(got, exp, TOL["f64"]["out"], TOL["f64"]["tgt"])
    ap.close()


# 9 ---------------------------------------------------------------------------------------------------------------
def test_forgetting_with_perceptual_weighting():
    """perceptual=True, beta = 0.8, 4 hops, at the bounds of test_window_with_perceptual_weighting."""
    from oracle.perceptual import Model
    rirA, rirB = synth_rirs(150, 4, 8, 6)
    N, H = 512, 256
    ap, orc = make_pair(N, H, rirA, rirB, 9, 1, 2, 2, 1.0, 0.8, perceptual=Model(N, 16000, 100.0), sampling_rate=16000,
                        fullscale=100.0)
    x = np.random.default_rng(5).standard_normal((2, 4 * H))
    for h in range(4):
        check_outputs([hop(ap, x, h, H)], [hop(orc, x, h, H)], 1e-6, 1e-9)
    ap.close()


# 10 --------------------------------------------------------------------------------------------------------------
def test_set_stat_forgetting_refusals():
    from ap_vast_unofficial_amd import _capi
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(60, 4, 8, 3)
    ap = apvast(128, rirA, rirB, 8, 4, 0, 0, 2, 1.0, 256, perceptual=False, seed=5, statistics_forgetting=0.5)
    x = np.random.default_rng(1).standard_normal((2, 64 * 2))
    hop(ap, x, 0, 64)
    e = ap._eng
    assert e.lib.apv_stream_set_stat_forgetting(e.h, 0.9) == _capi.ERR_ARG
    assert e.stat_forgetting == 0.5
    out = hop(ap, x, 1, 64)                                   # the stream is still running
    assert np.isfinite(np.stack(out[0])).all()
    ap.close()
    eng = _capi.Engine(4, 4, 8)
    for bad in (0.0, 1.5, float("nan")):
        assert eng.lib.apv_stream_set_stat_forgetting(eng.h, bad) == _capi.ERR_ARG
    assert eng.lib.apv_stream_set_stat_hops(eng.h, 3) == _capi.OK
    assert eng.lib.apv_stream_set_stat_forgetting(eng.h, 0.9) == _capi.ERR_ARG       # hops, then forgetting
    eng.close()
    eng = _capi.Engine(4, 4, 8)
    assert eng.lib.apv_stream_set_stat_forgetting(eng.h, 0.9) == _capi.OK
    assert eng.lib.apv_stream_set_stat_hops(eng.h, 3) == _capi.ERR_ARG               # forgetting, then hops > 1
    assert eng.lib.apv_stream_set_stat_hops(eng.h, 1) == _capi.OK
    eng.close()
