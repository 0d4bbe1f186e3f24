"""Statistics window of the subband stream (apvast(..., statistics_hops=T), apv_stream_set_stat_hops) against the windowed CPU
oracle (tests/windowed_oracle.py).  Tolerances: the table TOL of tests/test_gpu_stream.py unless a test says otherwise."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import subband  # noqa: E402  (checker only)
from test_gpu_stream import TOL, cfg3_rirs, check_last_hop_state, check_outputs, pink, synth_rirs  # noqa: E402
from windowed_oracle import WindowedSubbandOracle  # noqa: E402


def make_pair(N, H, rirA, rirB, delay, refA, refB, V, mu, T, run_A=True, run_B=True, seed=0, dtype="f64", perceptual=None,
              sampling_rate=48000, fullscale=94.0):
    """an apvast object with statistics_hops = T and the windowed oracle started from the same response buffers"""
    from ap_vast_unofficial_amd.apvast import apvast
    P, L, M = rirA.shape
    ap = apvast(N, rirA, rirB, 16, delay, refA, refB, V, mu, 4 * N, hop_size=H, run_A=run_A, run_B=run_B,
                perceptual=perceptual is not None, seed=seed, dtype=dtype, statistics_hops=T, sampling_rate=sampling_rate,
                fullscale_db_spl=fullscale)
    rs = np.random.RandomState(seed)
    init_r = np.stack([1e-3 * rs.randn(N, L, M) for _ in range(4)])
    init_t = np.stack([1e-3 * rs.randn(N, M) for _ in range(2)])
    orc = WindowedSubbandOracle(N, rirA, rirB, delay, refA, refB, list(range(1, V + 1)), mu, hop_size=H, run_A=run_A, run_B=run_B,
                                init_response=init_r, init_target_response=init_t, perceptual=perceptual, stat_hops=T)
    return ap, orc


def hop(obj, x, h, H):
    f = obj.process_input_buffers if hasattr(obj, "process_input_buffers") else obj.process
    return f(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])


def same_outputs(oa, ob):
    for q in range(4):
        assert (oa[q] is None) == (ob[q] is None)
        if oa[q] is not None:
            assert np.array_equal(np.stack(oa[q]), np.stack(ob[q])), q


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "mixed", "f32"])
def test_window_vs_oracle(dtype):
    """8 x 16, N = 256, T = 3, 8 hops: every hop's outputs (the fill phase included), the last hop's spectra, w, lambda."""
    rirA, rirB = synth_rirs(200, 8, 16, 1)
    N, H, hops = 256, 128, 8
    ap, orc = make_pair(N, H, rirA, rirB, 12, 2, 5, 4, 1.0, 3, dtype=dtype)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    got = [hop(ap, x, h, H) for h in range(hops)]
    exp = [hop(orc, x, h, H) for h in range(hops)]
    check_outputs(got, exp, TOL[dtype]["out"], TOL[dtype]["tgt"])
    check_last_hop_state(ap, orc, TOL[dtype], 129, 8, 16)
    ap.close()


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_A,run_B", [(True, True), (True, False)])
def test_window_cfg3_shape(run_A, run_B):
    """16 x 32, N = 2048, 800 taps, pink input, T = 4: the captured hop graphs and the order-16 explicit kernel."""
    rirA, rirB = cfg3_rirs()
    hops, H = 6, 1024
    x = pink(hops * H, 2024)
    ap, orc = make_pair(2048, H, rirA, rirB, 16, 3, 7, 8, 1.0, 4, run_A=run_A, run_B=run_B)
    got = [hop(ap, x, h, H) for h in range(hops)]
    exp = [hop(orc, x, h, H) for h in range(hops)]
    check_outputs(got, exp, TOL["f64"]["out"], TOL["f64"]["tgt"])
    check_last_hop_state(ap, orc, TOL["f64"], 1025, 16, 32, tuple(z for z, r in enumerate((run_A, run_B)) if r))
    ap.close()


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,M,T", [(64, 16, 6), (128, 64, 4)])
def test_window_more_loudspeakers_than_control_points(L, M, T):
    """Orders 64 and 128 with M < L, every hop held to the plain TOL["f64"] (one block alone needs the loosened
    TOL_RANK_DEFICIENT of tests/test_gpu_order128.py).

    The first hops hold fewer than L rows (64 x 16: hops 0-2 with 16, 32, 48 rows; 128 x 64: hop 0 with 64) and are rank
    deficient by construction.  No looser bound is taken for them: two float64 evaluations of the oracle itself on the same input
    (WindowedSubbandOracle with solver="jdiag" against solver="eigh", i.e. oracle.subband.update against update_vectorised)
    lie 1.8e-15 ... 1.0e-14 of the largest sample apart on the outputs of every hop of both runs, those hops included, so ten
    times that distance is below TOL["f64"]["out"] = 1e-9 and the plain bound stands.  At order 64 those hops must not reach
    csrc/kernels_gevd64.hip, whose float32 sweeps do not resolve the whitened matrix of a rank-16 pencil (first hop off by 4.7e2
    of the largest sample, status 2 in every bin, before the stream sent them to the float64 LDS kernel: win_low_rank in
    csrc/stream.hip)."""
    rirA, rirB = synth_rirs(70, L, M, 5)
    N, H, hops = 128, 64, T + 2
    ap, orc = make_pair(N, H, rirA, rirB, 5, 1, 2, 2, 1.0, T)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    got = [hop(ap, x, h, H) for h in range(hops)]
    exp = [hop(orc, x, h, H) for h in range(hops)]
    for q in range(2):
        peak = max(np.abs(e[q]).max() for e in exp)
        print(f"{L} x {M} zone {q}: per-hop output error / peak",
              ["%.1e" % (np.abs(np.stack(g[q]) - e[q]).max() / peak) for g, e in zip(got, exp)],
              "rows", [min(h + 1, T) * M for h in range(hops)])
    check_outputs(got, exp, TOL["f64"]["out"], TOL["f64"]["tgt"])
    check_last_hop_state(ap, orc, TOL["f64"], 65, L, M)
    ap.close()


def test_eigenvectors_read_in_the_fill_phase_at_order_64():
    """U_A read while the window of a 64 x 16 stream holds 16 rows: the statistics reader must solve that pencil with the float64
    LDS kernel too.  jdiag's contract U^H (R_D + 1e-7 I) U = I, held to the rounding of a backward-stable float64 solve,
    10 n eps |U|_F^2 |R_D + 1e-7 I|_F per bin (|U|^2 is of the order of 1 / 1e-7 here: the absolute 1e-10 of the full-rank tests
    does not apply)."""
    L, M, T = 64, 16, 6
    rirA, rirB = synth_rirs(70, L, M, 5)
    ap, orc = make_pair(128, 64, rirA, rirB, 5, 1, 2, 2, 1.0, T)
    x = np.random.default_rng(99).standard_normal((2, 64))
    hop(ap, x, 0, 64)
    hop(orc, x, 0, 64)
    RB, RD, _ = orc.window_statistics(0)
    U, B = ap.U_A, RD + 1e-7 * np.eye(L)
    res = np.abs(U.conj().transpose(0, 2, 1) @ B @ U - np.eye(L)).max(axis=(1, 2))
    bound = 10 * L * np.finfo(float).eps * np.linalg.norm(U, axis=(1, 2)) ** 2 * np.linalg.norm(B, axis=(1, 2))
    print(f"fill-phase U_A: residual {res.max():.2e}, bound {bound.min():.2e} .. {bound.max():.2e}")
    assert (res <= bound).all() and bound.max() < 1e-3, (res.max(), bound.max())
    ap.close()


# 4 ---------------------------------------------------------------------------------------------------------------
def test_one_hop_given_explicitly_is_the_default():
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(200, 8, 16, 1)
    N, H, hops = 256, 128, 6
    mk = lambda **kw: apvast(N, rirA, rirB, 16, 12, 2, 5, 4, 1.0, 4 * N, hop_size=H, perceptual=False, seed=0, **kw)
    a, b = mk(), mk(statistics_hops=1)
    x = np.random.default_rng(3).standard_normal((2, hops * H))
    for h in range(hops):
        same_outputs(hop(a, x, h, H), hop(b, x, h, H))
    for z in "AB":
        assert np.array_equal(getattr(a, "w_" + z), getattr(b, "w_" + z))
        assert np.array_equal(getattr(a, "lambda_" + z), getattr(b, "lambda_" + z))
    assert sorted(a.get_state()) == sorted(b.get_state()) == ["input_block", "input_history", "out_overlap", "response",
                                                              "target_response"]
    a.close()
    b.close()


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,M,N,dtype", [(8, 16, 256, "f64"), (8, 16, 256, "f32"), (16, 32, 512, "f64"), (16, 32, 512, "f32")])
def test_process_signal_equals_hop_loop(L, M, N, dtype):
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(200, L, M, 1)
    H, hops = N // 2, 40
    mk = lambda: apvast(N, rirA, rirB, 16, 12, 2, 5, 4, 1.0, 4 * N, hop_size=H, perceptual=False, seed=0, dtype=dtype,
                        statistics_hops=3)
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


# 6 ---------------------------------------------------------------------------------------------------------------
def test_statistics_attributes_are_windowed():
    """R_*, r_* after hop 2 (window of 4 not yet full) and after hop 7 against the sums formed in NumPy from the helper's spectra
    (1e-12 of the largest entry, as test_attributes_and_state of tests/test_gpu_order128.py); U_A through jdiag's contract."""
    rirA, rirB = synth_rirs(200, 8, 16, 1)
    N, H, L = 256, 128, 8
    ap, orc = make_pair(N, H, rirA, rirB, 12, 2, 5, 4, 1.0, 4)
    x = np.random.default_rng(99).standard_normal((2, 8 * H))
    for h in range(8):
        hop(ap, x, h, H)
        hop(orc, x, h, H)
        if h not in (2, 7):
            continue
        assert len(orc.window_hops[0]) == min(h + 1, 4)
        for z, names in enumerate((("R_A_to_A", "R_A_to_B", "r_A"), ("R_B_to_B", "R_B_to_A", "r_B"))):
            for name, ref in zip(names, orc.window_statistics(z)):
                g = getattr(ap, name)
                err = np.abs(g - ref).max() / np.abs(ref).max()
                print(f"hop {h} {name}: {err:.2e}")
                assert err < 1e-12, (h, name, err)
        RB, RD, _ = orc.window_statistics(0)
        U, lam = ap.U_A, ap.lambda_A
        UH = U.conj().transpose(0, 2, 1)
        assert np.abs(UH @ (RD + 1e-7 * np.eye(L)) @ U - np.eye(L)).max() < 1e-10
        assert np.abs(UH @ RB @ U - lam[:, :, None] * np.eye(L)).max() < 1e-10 * lam.max()
    ap.close()


# 7 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [5, 2])
def test_resume_is_bit_for_bit(at):
    """get_state -> set_state into a fresh object after `at` hops (2: inside the fill phase of a window of 4), 5 more on both."""
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(200, 8, 16, 1)
    N, H = 256, 128
    mk = lambda seed: apvast(N, rirA, rirB, 16, 12, 2, 5, 4, 1.0, 4 * N, hop_size=H, perceptual=False, seed=seed,
                             statistics_hops=4)
    a, b = mk(0), mk(1)
    x = np.random.default_rng(5).standard_normal((2, (at + 5) * H))
    for h in range(at):
        hop(a, x, h, H)
    st = a.get_state()
    assert st["statistics_window_fill"] == min(at, 4) and st["statistics_window"].shape == (2, 4, 129, 2 * 8 * 8 + 8)
    b.set_state(st)
    for h in range(at, at + 5):
        same_outputs(hop(a, x, h, H), hop(b, x, h, H))
    sa, sb = a.get_state(), b.get_state()
    assert sorted(sa) == sorted(sb)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    a.close()
    b.close()


# 8 ---------------------------------------------------------------------------------------------------------------
def test_reassigned_response_and_mu_keep_the_window():
    """rir_A reassigned after hop 3, mu after hop 5, T = 3: the hops already in the window keep the statistics they were formed
    with, as the reference's statistics buffer keeps old samples."""
    rirA, rirB = synth_rirs(200, 8, 16, 1)
    newA = synth_rirs(200, 8, 16, 77)[0]
    N, H, hops = 256, 128, 8
    ap, orc = make_pair(N, H, rirA, rirB, 12, 2, 5, 4, 1.0, 3)
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
def test_window_with_perceptual_weighting():
    """perceptual=True, T = 3, 4 hops, at the bounds of test_stream_perceptual_weighting (tests/test_gpu_stream.py)."""
    from oracle.perceptual import Model
    rirA, rirB = synth_rirs(150, 4, 8, 6)
    N, H = 512, 256
    ap, orc = make_pair(N, H, rirA, rirB, 9, 1, 2, 2, 1.0, 3, perceptual=Model(N, 16000, 100.0), sampling_rate=16000,
                        fullscale=100.0)
    x = np.random.default_rng(5).standard_normal((2, 4 * H))
    for h in range(4):
        check_outputs([hop(ap, x, h, H)], [hop(orc, x, h, H)], 1e-6, 1e-9)
    ap.close()


# 10 --------------------------------------------------------------------------------------------------------------
def test_set_stat_hops_refused_once_the_stream_runs():
    from ap_vast_unofficial_amd import _capi
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(60, 4, 8, 3)
    ap = apvast(128, rirA, rirB, 8, 4, 0, 0, 2, 1.0, 256, perceptual=False, seed=5, statistics_hops=2)
    x = np.random.default_rng(1).standard_normal((2, 64 * 2))
    hop(ap, x, 0, 64)
    e = ap._eng
    assert e.lib.apv_stream_set_stat_hops(e.h, 3) == _capi.ERR_ARG
    assert e.stat_hops == 2
    out = hop(ap, x, 1, 64)                                   # the stream is still running
    assert np.isfinite(np.stack(out[0])).all()
    eng = _capi.Engine(4, 4, 8)
    for bad in (0, 65):
        assert eng.lib.apv_stream_set_stat_hops(eng.h, bad) == _capi.ERR_ARG
    eng.close()
    ap.close()
