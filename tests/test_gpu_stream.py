"""GPU parity of the streaming path (class apvast, mode='subband') against the CPU oracle."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from oracle.subband_stream import SubbandStreamOracle  # noqa: E402  (checker only)


def synth_rirs(P, L, M, seed):
    rng = np.random.default_rng(seed)
    env = np.exp(-np.arange(P) / (P / 6.0))[:, None, None]
    return (rng.standard_normal((P, L, M)) * env * 1e-3, rng.standard_normal((P, L, M)) * env * 1e-3)


# Tolerances of the streaming subband composition against the float64 oracle, which always receives the UNROUNDED
# impulse responses, start buffers and inputs.  Errors are relative to the largest reference value of the run (outputs),
# of the tensor (spectra), to |w| per bin and rank (filters) and to the bin's largest eigenvalue.
#   "f64": every stage in float64 like the reference (lambda 1e-9, w 1e-7 |w|, outputs 1e-9 max|y|).
#          Measured at cfg3's shape (tools/probes/stream_err_probe.py): spectra 4e-16, w 3e-9 (median 1e-12),
#          lambda 1e-11, outputs 1e-10, target path 4e-12.
#   "mixed" / "f32": float32 FIR + FFT front-end (1e-7 on the spectra), amplified by cond(R_D) in the filters.
#          Measured: spectra 2e-7, w 1.2e-3 (median 5e-6), lambda 3e-5, outputs 3e-6.
TOL = {
    "f64": dict(spec=1e-13, w_med=1e-10, w_max=1e-7, lam=1e-9, out=1e-9, tgt=1e-11),
    "mixed": dict(spec=1e-6, w_med=5e-5, w_max=1e-2, lam=3e-4, out=5e-5, tgt=1e-5),
    "f32": dict(spec=1e-6, w_med=5e-5, w_max=1e-2, lam=3e-4, out=5e-5, tgt=1e-5),
}


def run_pair(block, hop, rirA, rirB, delay, refA, refB, V, mu, hops, run_A=True, run_B=True, seed=0, dtype="f64",
             dialect="python", x=None):
    from ap_vast_unofficial_amd.apvast import apvast
    P, L, M = rirA.shape
    ap = apvast(block, rirA, rirB, 16, delay, refA, refB, V, mu, 4 * block, hop_size=hop, run_A=run_A, run_B=run_B,
                perceptual=False, seed=seed, dtype=dtype, dialect=dialect)
    init_r = init_t = None
    if dialect == "python":
        rs = np.random.RandomState(seed)
        init_r = np.stack([1e-3 * rs.randn(block, L, M) for _ in range(4)])
        init_t = np.stack([1e-3 * rs.randn(block, M) for _ in range(2)])
    orc = SubbandStreamOracle(block, rirA, rirB, delay, refA, refB, list(range(1, V + 1)), mu, hop_size=hop, run_A=run_A,
                              run_B=run_B, init_response=init_r, init_target_response=init_t)
    H = ap.hop_size
    if x is None:
        x = np.random.default_rng(99).standard_normal((2, hops * H))
    got, exp = [], []
    for h in range(hops):
        got.append(ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H]))
        exp.append(orc.process(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H]))
    return ap, orc, got, exp


def check_outputs(got, exp, tol, tol_target=None):
    """every hop's outputs against the oracle's, relative to the largest reference sample of the run"""
    for q in range(4):
        if exp[0][q] is None:
            assert all(g[q] is None for g in got)
            continue
        scale = max(max(np.abs(e[q]).max() for e in exp), 1e-30)
        t = tol if (q < 2 or tol_target is None) else tol_target
        for h, (g, e) in enumerate(zip(got, exp)):
            ref = e[q] if q < 2 else np.broadcast_to(e[q], (len(g[q]),) + e[q].shape)
            err = np.abs(np.stack(g[q]) - ref).max()
            assert err <= t * scale, (h, q, err / scale)


def check_last_hop_state(ap, orc, tol, K, L, M, zones=(0, 1)):
    """control-point spectra (K2) and filters / eigenvalues (K5'-K10) of the last hop against the oracle's"""
    e = ap._eng
    for p in range(4):
        if (p < 2 and 0 not in zones) or (p >= 2 and 1 not in zones):
            continue
        X = e.get_state(f"spectra{p}", (K, M, L), e.sc_dtype)
        ref = orc.spectra[p].transpose(0, 2, 1)
        assert np.abs(X - ref).max() <= tol["spec"] * np.abs(ref).max(), (p, np.abs(X - ref).max() / np.abs(ref).max())
    for z in zones:
        name = "AB"[z]
        w, wr = getattr(ap, "w_" + name), orc.w[z].transpose(1, 0, 2)
        err = np.linalg.norm(w - wr, axis=-1) / np.linalg.norm(wr, axis=-1)
        assert np.median(err) < tol["w_med"] and err.max() < tol["w_max"], (name, np.median(err), err.max())
        lam, lr = getattr(ap, "lambda_" + name), orc.lam[z]
        V = w.shape[0]
        lerr = np.abs(lam[:, :V] - lr[:, :V]).max(axis=1) / lr[:, 0]
        assert lerr.max() < tol["lam"], (name, lerr.max())


@pytest.mark.parametrize("dtype", ["f64", "mixed", "f32"])
def test_stream_two_zones_vs_oracle(dtype):
    rirA, rirB = synth_rirs(200, 8, 16, 1)
    ap, orc, got, exp = run_pair(256, 128, rirA, rirB, 12, 2, 5, 4, 1.0, hops=6, dtype=dtype)
    tol = TOL[dtype]
    check_last_hop_state(ap, orc, tol, 129, 8, 16)
    check_outputs(got, exp, tol["out"], tol["tgt"])
    assert len(got[0][0]) == 4 and got[0][0][0].shape == (128, 8)
    ap.close()


# ---- BASELINE config 3 at its own shape: 16 loudspeakers x 32 control points, N = 2048, H = 1024, 800-tap RIRs --------
# This is where the order-16 register-resident kernel (two-zone launch, blockIdx.y = zone program), the 512-channel FIR
# launch and the N = 2048 transforms run under the captured hipGraph phases (reference anchors: apvast.py:153-165 the
# hop, 167-194 the FIR, 237-311 the control-point spectra, 428-506 the outputs).
def cfg3_rirs():
    rng = np.random.default_rng(99)          # synthetic RIRs (800, 16, 32) per zone, |x| <~ 1e-3
    env = (np.exp(-np.arange(800) / 120.0) * 1e-3)[:, None, None]
    return rng.standard_normal((800, 16, 32)) * env, rng.standard_normal((800, 16, 32)) * env


def pink(n, seed):
    rng = np.random.default_rng(seed)        # white noise shaped by 1/sqrt(f), DC zeroed, unit RMS
    X = np.fft.rfft(rng.standard_normal((2, n)), axis=1)
    f = np.arange(X.shape[1], dtype=float)
    f[0] = np.inf
    x = np.fft.irfft(X / np.sqrt(f), n, axis=1)
    return x / np.sqrt(np.mean(x ** 2, axis=1, keepdims=True))


@pytest.mark.parametrize("dtype,V,run_A,run_B", [("f64", 1, True, True), ("f64", 8, True, True), ("f64", 1, True, False),
                                                 ("f64", 8, False, True), ("mixed", 1, True, True), ("f32", 8, True, True)])
def test_stream_cfg3_shape_vs_oracle(dtype, V, run_A, run_B):
    rirA, rirB = cfg3_rirs()
    hops = 6
    x = pink(hops * 1024, 2024)
    ap, orc, got, exp = run_pair(2048, 1024, rirA, rirB, 16, 3, 7, V, 1.0, hops=hops, run_A=run_A, run_B=run_B,
                                 dtype=dtype, x=x)
    tol = TOL[dtype]
    zones = tuple(z for z, r in enumerate((run_A, run_B)) if r)
    check_last_hop_state(ap, orc, tol, 1025, 16, 32, zones)
    check_outputs(got, exp, tol["out"], tol["tgt"])
    assert (got[0][0] is None) == (not run_A) and (got[0][1] is None) == (not run_B)
    live = got[0][0] if run_A else got[0][1]
    assert len(live) == V and live[0].shape == (1024, 16)
    ap.close()


@pytest.mark.parametrize("dtype", ["f64", "mixed"])
def test_stream_cfg3_shape_ka1_delay(dtype):
    """KA-1 at cfg3's shape: with modeling_delay = 0 the target output on the reference loudspeaker is the input delayed by
    block_size - hop_size samples, every other channel exactly zero."""
    rirA, rirB = cfg3_rirs()
    hops, H, N = 5, 1024, 2048
    x = pink(hops * H, 7)
    ap, orc, got, exp = run_pair(N, H, rirA, rirB, 0, 5, 5, 1, 1.0, hops=hops, dtype=dtype, x=x)
    At = np.stack([g[2][0] for g in got])            # (hops, H, L)
    flat = At[:, :, 5].reshape(-1)
    assert np.abs(flat[N - H:] - x[0, : flat.size - (N - H)]).max() < (1e-13 if dtype == "f64" else 1e-5)
    assert np.abs(np.delete(At, 5, axis=2)).max() == 0.0
    ap.close()


def test_stream_target_path_is_wola_delay():
    """KA-1/KA-2: target outputs = OLA(w * circshift(w * block, d)); exact, independent of the GEVD."""
    rirA, rirB = synth_rirs(100, 4, 8, 2)
    ap, orc, got, exp = run_pair(128, 64, rirA, rirB, 0, 1, 1, 2, 1.0, hops=5)
    H, N = 64, 128
    x = np.random.default_rng(99).standard_normal((2, 5 * H))
    At = np.stack([g[2][0] for g in got])            # (hops, H, L)
    flat = At[:, :, 1].reshape(-1)
    assert np.abs(flat[N - H:] - x[0, : flat.size - (N - H)]).max() < 1e-13          # float64 end to end
    assert np.abs(np.delete(At, 1, axis=2)).max() == 0.0
    ap.close()


def test_stream_single_zone_and_errors(golden):
    g = golden("rirs_cfg1")
    rirA, rirB = g["rirA"], g["rirB"]
    from ap_vast_unofficial_amd.apvast import apvast
    with pytest.raises(RuntimeError, match="block size must be modulo 2"):
        apvast(255, rirA, rirB, 32, 16, 0, 0, 8, 1.0, 512, perceptual=False)
    with pytest.raises(RuntimeError, match="rirs of unequal size"):
        apvast(256, rirA, rirB[:, :, :7], 32, 16, 0, 0, 8, 1.0, 512, perceptual=False)
    ap, orc, got, exp = run_pair(256, 128, rirA, rirB, 16, 0, 0, 8, 1.0, hops=4, run_B=False)
    with pytest.raises(RuntimeError, match="invalid input size"):
        ap.process_input_buffers(np.zeros(100), np.zeros(100))
    assert got[0][1] is None                           # apvast.py:433-443
    # cfg1 is square (8 loudspeakers x 8 control points): the loaded dark matrix reaches cond ~ 1e5 and the eigenvalues of a
    # bin span as many decades.  Plain float64 bounds all the same: lambda 1e-9 of the bin's largest, w 1e-7 |w|
    # at every rank; the target path does not depend on the solve
    check_outputs([(None, None, g_[2], g_[3]) for g_ in got], [(None, None, e[2], e[3]) for e in exp], TOL["f64"]["tgt"])
    lam, lam_ref = ap.lambda_A, orc.lam[0]
    lerr = np.abs(lam - lam_ref).max(axis=1) / lam_ref[:, 0]
    assert lerr.max() < 1e-9, lerr.max()
    w, wr = ap.w_A, orc.w[0].transpose(1, 0, 2)
    werr = np.linalg.norm(w - wr, axis=-1) / np.linalg.norm(wr, axis=-1)
    assert werr.max() < 1e-7, werr.max()
    # outputs: the filters' 1e-7 bound carried through (measured 4e-9 of the largest sample with cond(R_D) ~ 1e5)
    check_outputs([(g_[0], None, None, None) for g_ in got], [(e[0], None, None, None) for e in exp], 5e-8)
    ap.close()


def test_state_roundtrip():
    rirA, rirB = synth_rirs(60, 4, 8, 3)
    from ap_vast_unofficial_amd.apvast import apvast
    a = apvast(128, rirA, rirB, 8, 4, 0, 0, 2, 1.0, 256, perceptual=False, seed=5)
    b = apvast(128, rirA, rirB, 8, 4, 0, 0, 2, 1.0, 256, perceptual=False, seed=6)
    x = np.random.default_rng(1).standard_normal((2, 64 * 5))
    for h in range(3):
        a.process_input_buffers(x[0, h * 64:(h + 1) * 64], x[1, h * 64:(h + 1) * 64])
    b.set_state(a.get_state())
    for h in range(3, 5):
        oa = a.process_input_buffers(x[0, h * 64:(h + 1) * 64], x[1, h * 64:(h + 1) * 64])
        ob = b.process_input_buffers(x[0, h * 64:(h + 1) * 64], x[1, h * 64:(h + 1) * 64])
        for q in range(4):
            assert np.array_equal(np.stack(oa[q]), np.stack(ob[q]))
    a.close()
    b.close()


def test_module_jdiag_dropin(golden):
    from ap_vast_unofficial_amd.apvast import jdiag
    g = golden("g2_jdiag_real")
    U, D = jdiag(g["A"][0], g["B"][0])
    assert U.dtype == np.float64 and D.shape == (12, 12)
    assert np.abs(np.diag(D) / g["lam"][0] - 1).max() < 1e-9
    assert np.abs(U.T @ (g["B"][0] + 1e-7 * np.eye(12)) @ U - np.eye(12)).max() < 1e-10
    with pytest.raises(np.linalg.LinAlgError):
        jdiag(np.eye(4), -np.eye(4))


def test_stream_non_power_of_two_block():
    """The reference's own fixture script uses blockSize = 1600 (make_python_test.m:6); here 240 = 2^4 * 3 * 5."""
    rirA, rirB = synth_rirs(90, 4, 8, 4)
    ap, orc, got, exp = run_pair(240, 120, rirA, rirB, 7, 1, 2, 2, 1.0, hops=5)
    check_outputs(got, exp, TOL["f64"]["out"], TOL["f64"]["tgt"])
    ap.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("P,block,hop", [(20, 256, 128), (200, 256, 128), (90, 240, 120)])
def test_stream_fir_direct_and_fast_convolution(P, block, hop, dtype, monkeypatch):
    """K1 (apvast.py:171-192) has two forms: the direct one on the matrix cores and, for responses of 64 taps or more, an
    overlap-save segment through the frequency domain.  Both against the oracle's lfilter (float64: spectra at 1e-13);
    with APV_FIR_DIRECT set the long responses take the direct form too, and the two forms agree to rounding."""
    rirA, rirB = synth_rirs(P, 4, 8, 11)
    K = block // 2 + 1
    runs = {}
    for form in ("default", "direct"):
        if form == "direct":
            monkeypatch.setenv("APV_FIR_DIRECT", "1")
        ap, orc, got, exp = run_pair(block, hop, rirA, rirB, 5, 1, 2, 2, 1.0, hops=5, dtype=dtype)
        check_last_hop_state(ap, orc, TOL[dtype], K, 4, 8)
        check_outputs(got, exp, TOL[dtype]["out"], TOL[dtype]["tgt"])
        runs[form] = np.stack([ap._eng.get_state(f"spectra{p}", (K, 8, 4), ap._eng.sc_dtype) for p in range(4)])
        ap.close()
    scale = np.abs(runs["direct"]).max()
    assert np.abs(runs["default"] - runs["direct"]).max() <= (1e-14 if dtype == "f64" else 1e-6) * scale


@pytest.mark.parametrize("P,block,hop,dtype", [(4800, 2048, 1024, "f64"),      # five partitions of 1024 taps
                                                (4200, 256, 128, "f64"),        # 33 partitions
                                                (9000, 256, 128, "f32")])       # 71 partitions, float32 front-end
def test_stream_partitioned_convolution(P, block, hop, dtype):
    """K1 (apvast.py:171-192) for responses too long for ONE overlap-save segment in LDS (P - 1 + H beyond 4096 doubles / 8192
    floats): uniformly partitioned, partitions of H taps in segments of 2 H samples, against the oracle's lfilter at the plain
    tolerances of the stream; the state arrays resume bit for bit (the input history is longer in this form: apv_state_bytes),
    and the whole-signal entry point returns the hop loop's samples."""
    from ap_vast_unofficial_amd.apvast import apvast
    L, M = 2, 4
    rirA, rirB = synth_rirs(P, L, M, 31)
    K = block // 2 + 1
    ap, orc, got, exp = run_pair(block, hop, rirA, rirB, 5, 1, 0, 2, 1.0, hops=7, dtype=dtype)
    e = ap._eng
    n_part = -(-P // hop)
    assert e.state_bytes("input_history0") == (n_part + 1) * hop * np.dtype(e.s_dtype).itemsize      # the partitioned form ran
    check_last_hop_state(ap, orc, TOL[dtype], K, L, M)
    check_outputs(got, exp, TOL[dtype]["out"], TOL[dtype]["tgt"])
    # resume: a second object set to this one's state continues bit for bit, per hop and through process_signal
    b = apvast(block, rirA, rirB, 16, 5, 1, 0, 2, 1.0, 4 * block, hop_size=hop, perceptual=False, seed=9, dtype=dtype)
    b.set_state(ap.get_state())
    x = np.random.default_rng(4).standard_normal((2, 5 * hop))
    ref = [ap.process_input_buffers(x[0, h * hop:(h + 1) * hop], x[1, h * hop:(h + 1) * hop]) for h in range(5)]
    sig = b.process_signal(x[0], x[1])
    for q in range(4):
        for v in range(2):
            assert np.array_equal(np.concatenate([r[q][v] for r in ref]), sig[q][v]), (q, v)
    sa, sb = ap.get_state(), b.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    ap.close()
    b.close()


@pytest.mark.parametrize("dialect", ["python", "matlab"])
def test_stream_perceptual_weighting(dialect):
    """perceptual=True: device weighting curves (perceptualModel.m:118-139, 177-190) against the independent NumPy
    restatement, then the weighted streaming path against the oracle."""
    from ap_vast_unofficial_amd.apvast import apvast
    from oracle.perceptual import Model
    rirA, rirB = synth_rirs(150, 4, 8, 6)
    N, H, L, M, V = 512, 256, 4, 8, 2
    ap = apvast(N, rirA, rirB, 16, 9, 1, 2, V, 1.0, 4 * N, hop_size=H, sampling_rate=16000, perceptual=True,
                dialect=dialect, seed=0, fullscale_db_spl=100.0)
    rs = np.random.RandomState(0)
    init_r = np.stack([1e-3 * rs.randn(N, L, M) for _ in range(4)])
    init_t = np.stack([1e-3 * rs.randn(N, M) for _ in range(2)])
    if dialect == "matlab":
        init_r[:] = 0
        init_t[:] = 0
    model = Model(N, 16000, 100.0)
    # the MATLAB dialect also loads both matrices relatively (apVast.m:552-569); the oracle run below only
    # checks the weighting curves for it
    orc = SubbandStreamOracle(N, rirA, rirB, 9, 1, 2, [1, 2], 1.0, hop_size=H,
                              init_response=init_r, init_target_response=init_t, perceptual=model,
                              normalisation=dialect)
    x = np.random.default_rng(5).standard_normal((2, 4 * H))
    for h in range(4):
        got = ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        exp = orc.process(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        for z in range(2):
            W = ap._eng.get_state(f"weights{z}", (N // 2 + 1, M), np.float64)
            assert np.abs(W - orc.weights[z]).max() < 1e-9 * np.abs(orc.weights[z]).max(), (h, z)
        if dialect == "python":
            check_outputs([got], [exp], 1e-6, 1e-9)
    assert abs(np.linalg.norm(W[:, 0]) - (1.0 if dialect == "python" else np.linalg.norm(W[:, 0]))) < 1e-5
    ap.close()


def test_g4_control_point_spectra_vs_reference(golden):
    """Fixture G4: the per-bin control-point matrices X[k] (M x L) that the subband update consumes are the spectra of
    the reference's own response buffers (apvast.py:202-203, 246-255) -- same rirs.mat, same start buffers and same
    input hops as G1; the float64 front-end against the reference's float64.  The fixture stores the spectra in complex64
    (6e-8 resolution), which is what bounds this comparison; the float32 front-end agrees to 2e-5."""
    from ap_vast_unofficial_amd.apvast import apvast
    g1, g4, rirs = golden("g1_broadband_cfg1"), golden("g4_stft_stage"), golden("rirs_cfg1")
    N, H, L, M = 256, 128, 8, 8
    ap = apvast(N, rirs["rirA"], rirs["rirB"], 32, 16, 0, 0, 8, 1.0, 512, hop_size=H, perceptual=False, seed=0)
    ap.set_state({"response": g1["init_response"], "target_response": g1["init_target_response"]})
    x = g1["x"]
    hops = list(g4["hops"])
    K = N // 2 + 1
    for h in range(max(hops) + 1):
        ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        if h in hops:
            i = hops.index(h)
            for p in range(4):
                X = ap._eng.get_state(f"spectra{p}", (K, M, L), np.complex128)         # X[k] = spectra[k].T
                ref = g4["spectra"][i, p].transpose(0, 2, 1)
                assert np.abs(X - ref).max() <= 1e-7 * np.abs(ref).max(), (h, p)
            for z in range(2):
                T = ap._eng.get_state(f"target_spectra{z}", (K, M), np.complex128)
                ref = g4["target_spectra"][i, z]
                assert np.abs(T - ref).max() <= 1e-7 * np.abs(ref).max(), (h, z)
    ap.close()


def test_stream_per_bin_attributes():
    """U_A, R_A_to_A, R_A_to_B, r_A (apvast.py:368-387) per bin in subband mode, recomputed on demand from the hop's
    control-point spectra: statistics against the oracle's, U through jdiag's contract, and w from U."""
    rirA, rirB = synth_rirs(200, 8, 16, 1)
    ap, orc, got, exp = run_pair(256, 128, rirA, rirB, 12, 2, 5, 4, 1.0, hops=3)
    from oracle import subband
    for z, (names, bright, dark) in enumerate(((("R_A_to_A", "R_A_to_B", "r_A", "U_A", "lambda_A", "w_A"), 0, 1),
                                               (("R_B_to_B", "R_B_to_A", "r_B", "U_B", "lambda_B", "w_B"), 3, 2))):
        RB, RD, r = subband.correlate(orc.spectra[bright].transpose(0, 2, 1), orc.spectra[dark].transpose(0, 2, 1),
                                      orc.target_spectra[z])
        gRB, gRD, gr, U, lam, w = (getattr(ap, n) for n in names)
        assert gRB.shape == (129, 8, 8) and U.shape == (129, 8, 8)
        for got_, ref in ((gRB, RB), (gRD, RD), (gr, r)):
            assert np.abs(got_ - ref).max() < 1e-12 * np.abs(ref).max()
        UH = U.conj().transpose(0, 2, 1)
        assert np.abs(UH @ (RD + 1e-7 * np.eye(8)) @ U - np.eye(8)).max() < 1e-8
        D = UH @ RB @ U
        assert np.abs(D - lam[:, :, None] * np.eye(8)).max() < 1e-8 * lam.max()
        coef = np.einsum("kli,kl->ki", U.conj(), r) / (lam + 1.0)
        w4 = np.einsum("kli,ki->kl", U[:, :, :4], coef[:, :4])
        assert np.abs(w4 - w[3]).max() < 1e-9 * np.abs(w4).max()
    assert len(ap.filter_spectra_A_t) == 4 and np.abs(ap.filter_spectra_A_t[0] - orc.target_filter).max() < 1e-14
    ap.close()



def _hop_loop(ap, x, h0, h1):
    H = ap.hop_size
    outs = [ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H]) for h in range(h0, h1)]
    # concatenate like main.m:58-61: per zone a list over the ranks of (n_samples, L)
    return [None if outs[0][q] is None else [np.concatenate([o[q][v] for o in outs]) for v in range(len(outs[0][q]))]
            for q in range(4)]


def test_stray_debug_variable_cannot_corrupt_a_stream():
    """APV_STFT_DEBUG switches timing aids on that make every transform wrong (tools/probes/analysis_bound.sh).  Left over in an
    environment it must not silently corrupt the outputs: without APV_STFT_DEBUG_PROBE=1 no stream can be created."""
    import subprocess
    code = ("import sys, numpy as np; sys.path.insert(0, %r)\n"
            "from ap_vast_unofficial_amd.apvast import apvast\n"
            "r = np.random.default_rng(0).standard_normal((20, 4, 8)) * 1e-3\n"
            "try:\n"
            "    apvast(128, r, r, 16, 5, 1, 2, 2, 1.0, 512, hop_size=64, perceptual=False, seed=3)\n"
            "except RuntimeError as e:\n"
            "    print('REFUSED', e)\n" % ROOT)
    env = dict(os.environ, APV_STFT_DEBUG="1")
    env.pop("APV_STFT_DEBUG_PROBE", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert "REFUSED" in out.stdout and "APV_STFT_DEBUG" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("dtype,L", [("f64", 64), ("f32", 64), ("f64", 40)])
def test_process_signal_equals_hop_loop_orders_33_to_64(dtype, L):
    """Orders 33..64 park per-bin state of the joint diagonalisation in HBM scratch (the order-64 kernel's slots, the LDS
    kernel's Cholesky factor).  The chunked whole-signal path runs the diagonalisations of consecutive hops on three streams at
    once: each back stream must park in scratch of its own, or two hops overwrite each other's bins.  Bit for bit
    against the hop loop, over a chunk boundary."""
    from ap_vast_unofficial_amd.apvast import apvast
    M = L + 8
    rirA, rirB = synth_rirs(70, L, M, 21)
    N, H = 128, 64
    mk = lambda: apvast(N, rirA, rirB, 16, 5, 1, 2, 2, 1.0, 4 * N, hop_size=H, seed=3, dtype=dtype, perceptual=False,
                        sampling_rate=16000)
    a, b = mk(), mk()
    n_hops = 21
    x = np.random.default_rng(9).standard_normal((2, n_hops * H))
    ref = _hop_loop(a, x, 0, n_hops)
    got = list(b.process_signal(x[0], x[1]))
    for q in range(4):
        for v in range(len(ref[q])):
            assert got[q][v].shape == ref[q][v].shape == (n_hops * H, L)
            assert np.array_equal(got[q][v], ref[q][v]), (q, v)
    for z in "AB":
        assert np.array_equal(getattr(a, "w_" + z), getattr(b, "w_" + z))
    a.close()
    b.close()


@pytest.mark.parametrize("dtype,run_A,run_B,perceptual,P", [("f64", True, True, False, 70), ("mixed", True, True, False, 70),
                                                            ("f32", True, False, False, 70), ("f64", False, True, True, 70),
                                                            ("f64", True, True, False, 20), ("f32", True, True, False, 20)])
def test_process_signal_equals_hop_loop(dtype, run_A, run_B, perceptual, P):
    """process_signal against the hop loop: per hop the kernels and their operands are those of process_input_buffers,
    so every sample, filter and state array must come out bit for bit: across chunk boundaries (16 hops per chunk of the
    pinned staging), ending on either set, and mixed with per-hop calls before and after.  P = 70: K1 by fast convolution
    in one segment, so the chunked driver runs (input spectra, K1 and analysis transforms of a chunk of hops in one launch
    each); P = 20: K1 in its direct form on the matrix cores, consecutive hops pipelined on three streams over two sets
    of spectra."""
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(P, 4, 8, 11)
    N, H = 128, 64
    mk = lambda: apvast(N, rirA, rirB, 16, 5, 1, 2, 2, 1.0, 4 * N, hop_size=H, run_A=run_A, run_B=run_B, seed=3,
                        dtype=dtype, perceptual=perceptual, sampling_rate=16000)
    a, b = mk(), mk()
    n_hops = 2 + 41 + 2 + 4 + 1
    x = np.random.default_rng(8).standard_normal((2, n_hops * H))
    ref = _hop_loop(a, x, 0, n_hops)
    parts = [_hop_loop(b, x, 0, 2)]
    pos = 2
    for n in (41, 0, 4):                    # 41: three chunks, ends on set 0;  4: ends on set 1 -> copied to set 0
        if n == 0:
            parts.append(_hop_loop(b, x, pos, pos + 2))
            pos += 2
            continue
        parts.append(list(b.process_signal(x[0, pos * H:(pos + n) * H], x[1, pos * H:(pos + n) * H])))
        pos += n
        # attributes and state arrays are those of the last hop of the signal
        c = mk()
        _hop_loop(c, x, 0, pos)
        sb, sc = b.get_state(), c.get_state()
        assert sb.keys() == sc.keys()
        for k in sb:
            assert np.array_equal(sb[k], sc[k]), k
        for z, run in (("A", run_A), ("B", run_B)):
            if run:
                assert np.array_equal(getattr(b, "w_" + z), getattr(c, "w_" + z))
                assert np.array_equal(getattr(b, "R_%s_to_%s" % (z, z)), getattr(c, "R_%s_to_%s" % (z, z)))
        c.close()
    parts.append(_hop_loop(b, x, pos, pos + 1))
    for q in range(4):
        if ref[q] is None:
            assert all(p[q] is None for p in parts)
            continue
        for v in range(len(ref[q])):
            got = np.concatenate([p[q][v] for p in parts])
            assert got.shape == ref[q][v].shape == (n_hops * H, 4)
            assert np.array_equal(got, ref[q][v]), (q, v)
    with pytest.raises(RuntimeError):
        b.process_signal(x[0, :H + 1], x[1, :H + 1])
    a.close()
    b.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_process_signal_into_callers_array(dtype):
    """`out=`: the samples land in the caller's array (shape / dtype as the object says) and the returned lists are slices of
    it, in its own dtype -- float32 arithmetic hands float32 back without a second copy of the signal; without `out` the
    result is float64 as the reference's; the values are the same either way.  A wrong shape or dtype is refused."""
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(70, 4, 8, 11)
    N, H = 128, 64
    mk = lambda: apvast(N, rirA, rirB, 16, 5, 1, 2, 2, 1.0, 4 * N, hop_size=H, seed=3, dtype=dtype, perceptual=False, sampling_rate=16000)
    a, b = mk(), mk()
    x = np.random.default_rng(9).standard_normal((2, 20 * H))
    buf = np.full(a.signal_output_shape(x.shape[1]), np.nan, dtype=a.signal_output_dtype)
    assert buf.dtype == (np.float64 if dtype == "f64" else np.float32)
    got = a.process_signal(x[0], x[1], out=buf)
    ref = b.process_signal(x[0], x[1])
    assert np.isfinite(buf).all()
    for q in range(4):
        for v in range(len(ref[q])):
            assert ref[q][v].dtype == np.float64
            assert got[q][v].dtype == buf.dtype
            assert np.array_equal(got[q][v].astype(np.float64), ref[q][v]), (q, v)
    assert np.shares_memory(got[0][0], buf) and np.shares_memory(got[1][1], buf)
    with pytest.raises((ValueError, RuntimeError, TypeError)):
        a.process_signal(x[0], x[1], out=np.empty((1, 2, 3), dtype=buf.dtype))
    a.close()
    b.close()


def test_process_signal_vs_oracle_cfg3_shape():
    """The pipelined path against the oracle at BASELINE configs[2]'s shape (16 loudspeakers, 32 control points,
    block 2048, 800-tap RIRs), float64 end to end."""
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = cfg3_rirs()
    N, H, L, M, V, hops = 2048, 1024, 16, 32, 2, 5
    ap = apvast(N, rirA, rirB, 16, 100, 0, 0, V, 1.0, 4 * N, hop_size=H, perceptual=False, seed=0, dtype="f64")
    rs = np.random.RandomState(0)
    init_r = np.stack([1e-3 * rs.randn(N, L, M) for _ in range(4)])
    init_t = np.stack([1e-3 * rs.randn(N, M) for _ in range(2)])
    orc = SubbandStreamOracle(N, rirA, rirB, 100, 0, 0, [1, 2], 1.0, hop_size=H, init_response=init_r,
                              init_target_response=init_t)
    x = pink(hops * H, 77)
    sig = ap.process_signal(x[0], x[1])
    exp = [orc.process(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H]) for h in range(hops)]
    got = [tuple([sig[q][v][h * H:(h + 1) * H] for v in range(V)] for q in range(4)) for h in range(hops)]
    check_outputs(got, exp, TOL["f64"]["out"], TOL["f64"]["tgt"])
    check_last_hop_state(ap, orc, TOL["f64"], N // 2 + 1, L, M)
    ap.close()
