"""Subband mode at 65..128 loudspeakers (csrc/kernels_gevd128.hip) against the float64 oracle.

Every comparison is with oracle/ except the bit-for-bit schedule check.  A ConvergenceWarning is an error here: the QL
iteration of this order must converge on every spectrum these tests build, exact clusters included.
"""
import os
import sys
import warnings

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::ap_vast_unofficial_amd._capi.ConvergenceWarning")]
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import gevd, subband  # noqa: E402  (checker only)
from oracle.subband_stream import SubbandStreamOracle  # noqa: E402
from test_gpu_stream import TOL, _hop_loop, check_last_hop_state, check_outputs, run_pair, synth_rirs  # noqa: E402

# With M < L both R_B and R_D are rank-deficient and only the loading (1e-7 I) keeps R_D definite: cond(R_D + 1e-7 I) ~ 1e9.
# The oracle agrees with scipy.linalg.eigh(A, B) on the SAME R to 7e-14 (lambda / lambda_1) and 7e-10 (w) at L = 96, 128 with
# M = L / 2, but R summed in another order (tiles of 16 control points, as the device does) moves the oracle itself by 2e-7
# (lambda) and 4e-6 (w) at those shapes: float64 rounding of R, amplified by cond(R_D).  The bounds of those cases are set from
# that measured disagreement, with a margin of ~5x.
TOL_RANK_DEFICIENT = dict(lam=1e-6, w=5e-5)
TOL_F32 = TOL["f32"]


def _cplx(rng, *s):
    return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)


def _check_update(L, M, dtype, reg_mode, reg_dark, reg_bright, ranks, seed, K=64):
    from ap_vast_unofficial_amd._capi import Engine
    rng = np.random.default_rng(seed)
    XB, XD, d = _cplx(rng, K, M, L), _cplx(rng, K, M, L), _cplx(rng, K, M)
    eng = Engine(K, L, M, ranks=ranks, mu=1.0, compute_dtype=dtype, reg_mode=reg_mode, reg_dark=reg_dark,
                 reg_bright=reg_bright)
    w, lam, st = eng.update(XB, XD, d)
    eng.close()
    RB, RD, r = subband.correlate(XB, XD, d)
    mode = gevd.REG_MODE_REL if reg_mode == 1 else gevd.REG_MODE_ABS
    wr, lr, sr = subband.gevd_vast(RB, RD, r, 1.0, list(ranks), reg_mode=mode, reg=reg_dark, reg_bright=reg_bright)
    assert (st == 0).all() and (sr == 0).all()
    lerr = (np.abs(lam - lr).max(axis=1) / lr[:, 0]).max()
    werr = (np.linalg.norm(w - wr, axis=-1) / np.linalg.norm(wr, axis=-1)).max()
    if dtype == "f32":
        tl, tw = TOL_F32["lam"], TOL_F32["w_max"]
    elif M < L:
        tl, tw = TOL_RANK_DEFICIENT["lam"], TOL_RANK_DEFICIENT["w"]
    else:
        tl, tw = 1e-9, 1e-7
    assert lerr <= tl and werr <= tw, (L, M, dtype, lerr, werr)


@pytest.mark.parametrize("L", [65, 96, 128])
@pytest.mark.parametrize("mcase", ["L+8", "2L", "L/2"])
def test_update_vs_oracle_f64(L, mcase):
    """Engine.update at K = 64: M = L + 8, 2 L, and L // 2 (an exact (L - M)-fold zero eigenvalue of R_B in every bin)."""
    M = {"L+8": L + 8, "2L": 2 * L, "L/2": L // 2}[mcase]
    ranks = (1, 2, min(L, M) // 2, min(L, M))
    _check_update(L, M, "f64", 0, 1e-7, 0.0, ranks, seed=L + M)


@pytest.mark.parametrize("L,M", [(96, 192), (128, 136)])
def test_update_vs_oracle_relative_loading(L, M):
    """REG_REL (dark loading relative to ||R_D||_2) with the MATLAB dialect's bright loading."""
    _check_update(L, M, "f64", 1, 5e-3, 1e-8 if L == 96 else 0.0, (1, 8, L), seed=3 * L)


@pytest.mark.parametrize("L,M", [(96, 104), (128, 256)])
def test_update_vs_oracle_f32_handle(L, M):
    """compute_dtype="f32": the solve still runs in float64, c64 w and f32 lambda come out."""
    _check_update(L, M, "f32", 0, 1e-7, 0.0, (1, 4, 32), seed=5 * L)


def _pencil(rng, lam, cond_b):
    """(A, B) of order n with generalised eigenvalues lam: B = G G^H with cond(B) = cond_b, A = G diag(lam) G^H."""
    n = len(lam)
    q1, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    q2, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    G = q1 @ np.diag(np.logspace(0, -0.5 * np.log10(cond_b), n)) @ q2
    A = G @ np.diag(lam) @ G.conj().T
    B = G @ G.conj().T
    return 0.5 * (A + A.conj().T), 0.5 * (B + B.conj().T)


def test_gevd_vast_prescribed_spectra():
    """gevd_vast(RB, RD, r) at n = 128 on built pairs: a 16-fold exact cluster, a geometric spectrum over 1e12, a dark matrix of
    condition 1e8, and one bin whose R_D is indefinite (status 1 there, the other bins unaffected).  w is compared at ranks
    whose gap lambda_v - lambda_{v+1} exceeds 1e-6 lambda_1 only: inside a cluster w is not unique."""
    from ap_vast_unofficial_amd._capi import Engine
    n, rng = 128, np.random.default_rng(77)
    spectra = [np.concatenate([np.linspace(10.0, 1.0, 112), np.full(16, 0.5)]),     # 16-fold cluster
               np.logspace(0, -12, n),                                               # geometric over 1e12
               rng.uniform(0.1, 10.0, n),                                            # with the dark matrix of cond 1e8
               rng.uniform(0.1, 10.0, n)]                                            # indefinite R_D
    conds = [10.0, 10.0, 1e8, 10.0]
    RB, RD = np.empty((4, n, n), complex), np.empty((4, n, n), complex)
    for k in range(4):
        RB[k], RD[k] = _pencil(rng, spectra[k], conds[k])
    RD[3] -= 2.0 * np.eye(n)                       # G G^H has eigenvalues <= 1: now indefinite
    r = rng.standard_normal((4, n)) + 1j * rng.standard_normal((4, n))
    ranks = (1, 50, 112, 128)
    eng = Engine(4, n, n, ranks=ranks, mu=1e-3, compute_dtype="f64", reg_mode=0, reg_dark=1e-12)
    w, lam, st = eng.gevd_vast(RB, RD, r, raise_on_status=False)
    eng.close()
    wr, lr, sr = subband.gevd_vast(RB, RD, r, 1e-3, list(ranks), reg=1e-12)
    assert st.tolist() == [0, 0, 0, 1] and sr.tolist() == [0, 0, 0, 1]
    assert np.all(w[3] == 0) and np.all(lam[3] == 0)
    for k in range(3):
        assert np.abs(lam[k] - lr[k]).max() <= 1e-9 * lr[k, 0], (k, np.abs(lam[k] - lr[k]).max() / lr[k, 0])
        for t, V in enumerate(ranks):
            if V < n and lr[k, V - 1] - lr[k, V] <= 1e-6 * lr[k, 0]:
                continue
            err = np.linalg.norm(w[k, t] - wr[k, t]) / np.linalg.norm(wr[k, t])
            assert err <= 1e-7, (k, V, err)
    # the cluster's 16 values themselves
    assert np.abs(lam[0, 112:] - 0.5).max() <= 1e-9 * lam[0, 0]


@pytest.mark.parametrize("L,M,V,dtype", [(96, 104, 2, "f64"), (128, 136, 2, "f64"), (96, 104, 2, "mixed"),
                                         (96, 104, 2, "f32"), (96, 104, 96, "f64")])
def test_stream_vs_oracle(L, M, V, dtype):
    """apvast subband against SubbandStreamOracle, N = 128, H = 64, P = 70, 6 hops: outputs, last-hop w, lambda, spectra.
    V = L = 96 emits every rank, the list beyond 64 going through apv_set_rank_list."""
    rirA, rirB = synth_rirs(70, L, M, L + M)
    ap, orc, got, exp = run_pair(128, 64, rirA, rirB, 5, 1, 2, V, 1.0, hops=6, dtype=dtype)
    tol = TOL[dtype]
    check_outputs(got, exp, tol["out"], tol["tgt"])
    check_last_hop_state(ap, orc, tol, 65, L, M)
    assert len(ap.filter_spectra_A_t) == V and np.asarray(ap.w_A).shape == (V, 65, L)
    ap.close()


def test_stream_rank_deficient_dark():
    """L = 128, M = 64: R_B and R_D of rank 64 in every bin, loading alone keeps R_D definite (bounds: TOL_RANK_DEFICIENT)."""
    L, M = 128, 64
    rirA, rirB = synth_rirs(70, L, M, 5)
    ap, orc, got, exp = run_pair(128, 64, rirA, rirB, 5, 1, 2, 2, 1.0, hops=6)
    tol = dict(TOL["f64"], w_med=TOL_RANK_DEFICIENT["w"], w_max=TOL_RANK_DEFICIENT["w"], lam=TOL_RANK_DEFICIENT["lam"],
               out=TOL_RANK_DEFICIENT["w"])
    check_outputs(got, exp, tol["out"], tol["tgt"])
    check_last_hop_state(ap, orc, tol, 65, L, M)
    ap.close()


def test_stream_matlab_dialect():
    """dialect="matlab" (REG_REL dark 5e-3 ||R_D||_2, bright 1e-8 ||R_B||_2): the last hop's filters and eigenvalues against the
    oracle's solve of the hop's own statistics (which test_attributes_and_state checks against the oracle's correlation)."""
    from ap_vast_unofficial_amd.apvast import apvast
    L, M = 96, 104
    rirA, rirB = synth_rirs(70, L, M, 12)
    ap = apvast(128, rirA, rirB, 16, 5, 1, 2, 3, 1.0, 512, hop_size=64, perceptual=False, dialect="matlab", dtype="f64")
    x = np.random.default_rng(4).standard_normal((2, 5 * 64))
    for h in range(5):
        ap.process_input_buffers(x[0, h * 64:(h + 1) * 64], x[1, h * 64:(h + 1) * 64])
    for RBn, RDn, rn, wn, ln in (("R_A_to_A", "R_A_to_B", "r_A", "w_A", "lambda_A"), ("R_B_to_B", "R_B_to_A", "r_B", "w_B", "lambda_B")):
        wr, lr, sr = subband.gevd_vast(getattr(ap, RBn), getattr(ap, RDn), getattr(ap, rn), 1.0, [1, 2, 3],
                                       reg_mode=gevd.REG_MODE_REL, reg=5e-3, reg_bright=1e-8)
        w = np.asarray(getattr(ap, wn)).transpose(1, 0, 2)
        lam = getattr(ap, ln)
        assert (sr == 0).all()
        assert (np.abs(lam - lr).max(axis=1) / lr[:, 0]).max() <= 1e-9
        assert (np.linalg.norm(w - wr, axis=-1) / np.linalg.norm(wr, axis=-1)).max() <= 1e-7
    ap.close()


def test_stream_perceptual():
    """perceptual=True at L = 96: device weighting + order-96 solve against the oracle (bounds of test_gpu_stream's perceptual
    case)."""
    from ap_vast_unofficial_amd.apvast import apvast
    from oracle.perceptual import Model
    L, M, N, H = 96, 104, 256, 128
    rirA, rirB = synth_rirs(100, L, M, 6)
    ap = apvast(N, rirA, rirB, 16, 9, 1, 2, 2, 1.0, 4 * N, hop_size=H, sampling_rate=16000, perceptual=True, seed=0,
                fullscale_db_spl=100.0)
    rs = np.random.RandomState(0)
    init_r = np.stack([1e-3 * rs.randn(N, L, M) for _ in range(4)])
    init_t = np.stack([1e-3 * rs.randn(N, M) for _ in range(2)])
    orc = SubbandStreamOracle(N, rirA, rirB, 9, 1, 2, [1, 2], 1.0, hop_size=H, init_response=init_r,
                              init_target_response=init_t, perceptual=Model(N, 16000, 100.0), normalisation="python")
    x = np.random.default_rng(5).standard_normal((2, 4 * H))
    for h in range(4):
        got = ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        exp = orc.process(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        check_outputs([got], [exp], 1e-6, 1e-9)
    ap.close()


@pytest.mark.parametrize("dtype", ["f64", "mixed", "f32"])
def test_process_signal_equals_hop_loop_order_128(dtype):
    """The chunked whole-signal path runs consecutive hops' diagonalisations on several back streams: each must park in
    scratch slots of its own.  Bit for bit against the hop loop at L = 128, over a chunk boundary (21 hops)."""
    from ap_vast_unofficial_amd.apvast import apvast
    L, M = 128, 136
    rirA, rirB = synth_rirs(70, L, M, 21)
    N, H = 128, 64
    mk = lambda: apvast(N, rirA, rirB, 16, 5, 1, 2, 2, 1.0, 4 * N, hop_size=H, seed=3, dtype=dtype, perceptual=False,
                        sampling_rate=16000)
    a, b = mk(), mk()
    n_hops = 21
    x = np.random.default_rng(9).standard_normal((2, n_hops * H))
    ref = _hop_loop(a, x, 0, n_hops)
    out = b.alloc_signal_output(n_hops * H)
    got = list(b.process_signal(x[0], x[1], out=out))
    for q in range(4):
        for v in range(len(ref[q])):
            assert got[q][v].shape == ref[q][v].shape == (n_hops * H, L)
            assert np.array_equal(got[q][v], ref[q][v]), (q, v)
    for z in "AB":
        assert np.array_equal(getattr(a, "w_" + z), getattr(b, "w_" + z))
    a.close()
    b.close()


def test_attributes_and_state():
    """L = 96: R_A_to_A, U_A and lambda_A of the last hop against the oracle (U through jdiag's contract at 1e-10); then a
    get_state -> set_state round trip into a fresh object gives identical next-hop outputs."""
    from ap_vast_unofficial_amd.apvast import apvast
    L, M = 96, 104
    rirA, rirB = synth_rirs(70, L, M, 31)
    ap, orc, got, exp = run_pair(128, 64, rirA, rirB, 5, 1, 2, 2, 1.0, hops=3)
    RB, RD, r = subband.correlate(orc.spectra[0].transpose(0, 2, 1), orc.spectra[1].transpose(0, 2, 1), orc.target_spectra[0])
    gRB, gRD, gr, U, lam = ap.R_A_to_A, ap.R_A_to_B, ap.r_A, ap.U_A, ap.lambda_A
    for g, ref in ((gRB, RB), (gRD, RD), (gr, r)):
        assert np.abs(g - ref).max() < 1e-12 * np.abs(ref).max()
    assert (np.abs(lam - orc.lam[0]).max(axis=1) / orc.lam[0][:, 0]).max() <= 1e-9
    UH = U.conj().transpose(0, 2, 1)
    assert np.abs(UH @ (RD + 1e-7 * np.eye(L)) @ U - np.eye(L)).max() < 1e-10
    D = UH @ RB @ U
    assert np.abs(D - lam[:, :, None] * np.eye(L)).max() < 1e-10 * lam.max()
    # state round trip
    b = apvast(128, rirA, rirB, 16, 5, 1, 2, 2, 1.0, 512, hop_size=64, perceptual=False, seed=11)
    b.set_state(ap.get_state())
    x = np.random.default_rng(12).standard_normal((2, 64))
    oa = ap.process_input_buffers(x[0], x[1])
    ob = b.process_input_buffers(x[0], x[1])
    for q in range(4):
        assert np.array_equal(np.stack(oa[q]), np.stack(ob[q]))
    ap.close()
    b.close()


def test_refusals():
    from ap_vast_unofficial_amd._capi import ApvError, Engine
    from ap_vast_unofficial_amd.apvast import apvast
    with pytest.raises(ApvError, match="1..128"):
        Engine(4, 129, 130)
    rirA, rirB = synth_rirs(20, 129, 4, 1)
    with pytest.raises(ApvError, match="1..128"):
        apvast(64, rirA, rirB, 8, 2, 0, 0, 1, 1.0, 256, perceptual=False, seed=0)
    eng = Engine(4, 96, 100, ranks=(1, 2))
    for bad in ([2, 1], [0, 3], [1, 97], list(range(1, 98))):
        with pytest.raises(ApvError):
            eng.set_rank_list(bad)
    eng.set_rank_list(list(range(1, 97)))
    assert eng.nV == 96
    eng.close()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        e64 = Engine(4, 64, 70, ranks=(1,))
        with pytest.raises(ApvError):
            e64.set_rank_list(list(range(1, 66)))
        e64.close()
