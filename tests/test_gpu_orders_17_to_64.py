"""Subband mode at orders other than 16 and below 65 against the float64 oracle: plain streams on control-point data (per-bin
eigenvalue spans of 4e3 .. 9e4, neighbours as close as 4e-6 of the largest), built pencils and structured slabs.

These orders run the LDS kernels launch_t<T, 8|16|32|64> of csrc/kernels_gevd.hip, the order-64 kernel csrc/kernels_gevd64.hip and
the float32 split update (corr_mfma_f32_kernel + float LDS kernel).  Every comparison is with oracle/; a ConvergenceWarning is an
error in this file.

Bounds
  A  plain streams                 TOL[dtype] of tests/test_gpu_stream.py.  Two float64 evaluations of the oracle (jdiag route
                                   against cholesky -> eigh) agree on these inputs to 2.7e-15 (outputs), 1.5e-14 (w), 1.7e-15 (lambda).
  B  MATLAB dialect at order 64    lambda 1e-9 of the largest, w 1e-7: tests/test_gpu_order128.py::test_stream_matlab_dialect.
  C  M < L, one block              TOL_C below: five times the distance of the oracle from itself when R is summed in the device's
                                   order at these shapes (tighter than TOL_RANK_DEFICIENT of tests/test_gpu_order128.py).
  D  built pencils                 lambda 1e-9 of the largest; w 1e-7 at ranks whose gap exceeds 1e-6 lambda_1.  The oracle lies
                                   <= 7e-14 (cluster), <= 6e-12 (1e6), <= 3e-9 (cond(B) = 1e8) from scipy.linalg.eigh(A, B); over 1e12 it
                                   carries up to 4e-8 itself at mid ranks, so only ranks 1 and n are compared there.
  E  structured slabs at 64 x 72   lambda 1e-9 of the largest, w 1e-7 outside the cluster, against update_vectorised.
"""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::ap_vast_unofficial_amd._capi.ConvergenceWarning")]
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import gevd, subband  # noqa: E402  (checker only)
from oracle.subband_stream import SubbandStreamOracle  # noqa: E402
from test_gpu_order128 import TOL_RANK_DEFICIENT, _pencil  # noqa: E402
from test_gpu_stream import TOL, check_last_hop_state, check_outputs, synth_rirs  # noqa: E402
from windowed_oracle import WindowedSubbandOracle  # noqa: E402

SEED, DELAY, REF_A, REF_B, V = 3, 5, 1, 2, 2

# C: with M < L only the loading (1e-7 I) keeps R_D definite, and float64 rounding of R is amplified by cond(R_D + 1e-7 I).  Measured on
# the CPU before the device was looked at: the oracle (cholesky -> eigh) on the inputs of C with oracle.subband.correlate summing R
# in slices of 16 rows (the device's tiles) and of 4 rows (the k of its matrix-core step) against the same oracle with R summed at once:
#   64 x 16   16 rows: identical (one tile)          4 rows: out 5.3e-11  w 1.1e-10  lambda 1.3e-11
#   40 x 24   16 rows: out 2.8e-11  w 1.8e-10  lambda 8.2e-12   4 rows: out 3.1e-11  w 2.6e-10  lambda 7.2e-12
# (outputs relative to the largest sample, w per bin and rank, lambda to the bin's largest).  The bounds are five times the largest.
TOL_C = dict(out=5 * 5.3e-11, w=5 * 2.6e-10, lam=5 * 1.3e-11)
assert TOL_C["w"] < TOL_RANK_DEFICIENT["w"] and TOL_C["lam"] < TOL_RANK_DEFICIENT["lam"]


def _inputs(L, M, H, hops):
    rirA, rirB = synth_rirs(70, L, M, 21)
    return rirA, rirB, np.random.default_rng(9).standard_normal((2, hops * H))


@functools.lru_cache(maxsize=None)
def _oracle_run(L, M, N, H, hops):
    """The oracle's stream on the inputs of test_process_signal_equals_hop_loop_orders_33_to_64, once per shape: (oracle after the
    last hop, every hop's outputs).  From order 40 on, and for M < L, the batched cholesky -> eigh evaluation (the jdiag route takes
    40 s at 64 x 72)."""
    rirA, rirB, x = _inputs(L, M, H, hops)
    rs = np.random.RandomState(SEED)
    init_r = np.stack([1e-3 * rs.randn(N, L, M) for _ in range(4)])
    init_t = np.stack([1e-3 * rs.randn(N, M) for _ in range(2)])
    args = (N, rirA, rirB, DELAY, REF_A, REF_B, list(range(1, V + 1)), 1.0)
    kw = dict(hop_size=H, init_response=init_r, init_target_response=init_t)
    orc = WindowedSubbandOracle(*args, stat_hops=1, solver="eigh", **kw) if (L >= 40 or M < L) else SubbandStreamOracle(*args, **kw)
    exp = [orc.process(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H]) for h in range(hops)]
    return orc, exp


def _stream(L, M, N, H, hops, dtype, dialect="python"):
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB, x = _inputs(L, M, H, hops)
    ap = apvast(N, rirA, rirB, 16, DELAY, REF_A, REF_B, V, 1.0, 4 * N, hop_size=H, perceptual=False, seed=SEED, dtype=dtype,
                dialect=dialect)
    got = [ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H]) for h in range(hops)]
    return ap, got


def _report(tag, ap, orc, got, exp):
    """the figures the assertions below bound, printed first (pytest -s shows them)"""
    out = max(np.abs(np.stack(g[q]) - e[q]).max() / max(np.abs(e_[q]).max() for e_ in exp) for g, e in zip(got, exp) for q in range(2))
    werr = max((np.linalg.norm(getattr(ap, "w_" + "AB"[z]) - orc.w[z].transpose(1, 0, 2), axis=-1)
                / np.linalg.norm(orc.w[z].transpose(1, 0, 2), axis=-1)).max() for z in range(2))
    lerr = max((np.abs(getattr(ap, "lambda_" + "AB"[z])[:, :V] - orc.lam[z][:, :V]).max(axis=1) / orc.lam[z][:, 0]).max() for z in range(2))
    print(f"{tag}: out {out:.1e} w {werr:.1e} lambda {lerr:.1e} not_converged {ap._eng.stream_not_converged()}")


# A -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,M,dtype", [(24, 32, "f64"),                                       # launch_t<double, 32, 256>, fused
                                       (40, 48, "f64"), (40, 48, "f32"),                      # <double, 64, 1024, spill>; <float, 64>
                                       (64, 72, "f64"), (64, 72, "mixed"), (64, 72, "f32"),   # gevd64_kernel on c128 / c64 slabs
                                       (32, 40, "f32"),                                       # split update: corr_mfma_f32_kernel<1>
                                       (12, 20, "f64")])                                      # launch_t<double, 16, 64>
def test_stream_vs_oracle(L, M, dtype):
    """N = 128, H = 64, 70-tap RIRs, V = 2, 5 hops, Python dialect: every hop's outputs, the last hop's spectra, w and lambda."""
    N, H, hops = 128, 64, 5
    orc, exp = _oracle_run(L, M, N, H, hops)
    ap, got = _stream(L, M, N, H, hops, dtype)
    _report(f"A {L} x {M} {dtype}", ap, orc, got, exp)
    tol = TOL[dtype]
    check_outputs(got, exp, tol["out"], tol["tgt"])
    check_last_hop_state(ap, orc, tol, N // 2 + 1, L, M)
    assert ap._eng.stream_not_converged() == 0
    ap.close()


# B -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _matlab_stream_errors(dtype):
    """dialect="matlab" at 64 x 72, 5 hops: the last hop's (lambda, w) errors against the oracle's solve of the hop's own statistics"""
    L, M, N, H, hops = 64, 72, 128, 64, 5
    ap, _ = _stream(L, M, N, H, hops, dtype, dialect="matlab")
    worst_l = worst_w = 0.0
    for RBn, RDn, rn, wn, ln in (("R_A_to_A", "R_A_to_B", "r_A", "w_A", "lambda_A"), ("R_B_to_B", "R_B_to_A", "r_B", "w_B", "lambda_B")):
        wr, lr, sr = subband.gevd_vast(getattr(ap, RBn), getattr(ap, RDn), getattr(ap, rn), 1.0, list(range(1, V + 1)),
                                       reg_mode=gevd.REG_MODE_REL, reg=5e-3, reg_bright=1e-8)
        w = np.asarray(getattr(ap, wn)).transpose(1, 0, 2)
        lam = getattr(ap, ln)
        assert (sr == 0).all()
        worst_l = max(worst_l, (np.abs(lam - lr).max(axis=1) / lr[:, 0]).max())
        worst_w = max(worst_w, (np.linalg.norm(w - wr, axis=-1) / np.linalg.norm(wr, axis=-1)).max())
    ap.close()
    print(f"B 64 x 72 matlab {dtype}: lambda {worst_l:.1e} w {worst_w:.1e}")
    return worst_l, worst_w


@pytest.mark.parametrize("dtype,bounds", [
    ("f64", "f64"),
    ("f32", "f32"),
    pytest.param("f32", "f64", marks=pytest.mark.xfail(strict=True, reason=(
        "measured lambda 1.3e-5 of the largest, w 1.8e-4 against the float64 bounds 1e-9 / 1e-7: the float32 handle solves and "
        "emits in float32 (eps 6e-8), so these bounds are out of the format's reach")))])
def test_stream_matlab_dialect_order_64(dtype, bounds):
    """dialect="matlab" at 64 x 72 (REG_REL dark 5e-3 ||R_D||_2, bright 1e-8 ||R_B||_2: not for kernels_gevd64.hip).  f64: the LDS
    kernel at n = 64 on fused slabs; f32: the split update with corr_mfma_f32_kernel<2> and the float LDS kernel from explicit R.
    The float64 bounds are those of test_gpu_order128.test_stream_matlab_dialect (measured: lambda 3.2e-14, w 3.7e-13).  The float32
    run is held to TOL["f32"] (lambda 3e-4, w 1e-2, as test_gpu_order128._check_update holds float32 handles; measured 1.3e-5,
    1.8e-4): that is the check of the split path.  The same run against the float64 bounds is kept beside it, expected to fail."""
    worst_l, worst_w = _matlab_stream_errors(dtype)
    tl, tw = (1e-9, 1e-7) if bounds == "f64" else (TOL["f32"]["lam"], TOL["f32"]["w_max"])
    assert worst_l <= tl and worst_w <= tw, (worst_l, worst_w)


# C -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,M", [(64, 16), (40, 24)])
def test_stream_fewer_control_points_than_loudspeakers(L, M):
    """A plain stream (one block of statistics) with M < L: R_B and R_D of rank M in every bin, the loading alone keeps R_D definite.
    At order 64 such a hop must not reach csrc/kernels_gevd64.hip (GevdParams::no_gevd64).  N = 32, H = 16, 4 hops."""
    N, H, hops = 32, 16, 4
    orc, exp = _oracle_run(L, M, N, H, hops)
    ap, got = _stream(L, M, N, H, hops, "f64")
    _report(f"C {L} x {M}", ap, orc, got, exp)
    tol = dict(TOL["f64"], w_med=TOL_C["w"], w_max=TOL_C["w"], lam=TOL_C["lam"], out=TOL_C["out"])
    check_outputs(got, exp, tol["out"], tol["tgt"])
    check_last_hop_state(ap, orc, tol, N // 2 + 1, L, M)
    assert ap._eng.stream_not_converged() == 0
    ap.close()


def test_update_fewer_control_points_than_loudspeakers():
    """Engine(17, 64, 16).update on Gaussian slabs, dark loading 1e-2: the (3, 16, 8) case of test_gpu_parity.test_update_vs_oracle at
    order 64, with that test's plain float64 bounds (the loading of 1e-2 leaves cond(R_D) at 1e4: nothing to loosen).  Eigenvalues
    beyond rank(R_B) = 16 are rounding noise and ranks above it are not emitted."""
    from ap_vast_unofficial_amd._capi import Engine
    K, L, M, ranks = 17, 64, 16, (1, 8, 16)
    rng = np.random.default_rng(1000 + K + L)
    cn = lambda *s: ((rng.standard_normal(s) + 1j * rng.standard_normal(s)) * np.sqrt(0.5)).astype(np.complex64)
    XB, XD, d = cn(K, M, L), cn(K, M, L), cn(K, M)
    eng = Engine(K, L, M, ranks=ranks, mu=0.7, compute_dtype="f64", reg_dark=1e-2)
    w, lam, status = eng.update(XB, XD, d)
    eng.close()
    w_ref, lam_ref, _ = subband.update(XB, XD, d, 0.7, list(ranks), reg=1e-2)
    lerr = (np.abs(lam[:, :M] - lam_ref[:, :M]) / lam_ref[:, :1]).max()
    werr = (np.linalg.norm(w - w_ref, axis=-1) / np.linalg.norm(w_ref, axis=-1)).max()
    print(f"C update 64 x 16: lambda {lerr:.1e} w {werr:.1e} status {status.tolist()}")
    assert not status.any()
    assert lerr <= 1e-9 and werr <= 1e-7, (lerr, werr)


# D -----------------------------------------------------------------------------------------------------------------------------
SPECTRA = ("cluster", "geometric_1e12", "geometric_1e6", "cond_b_1e6", "indefinite")


@functools.lru_cache(maxsize=None)
def _built_pencils(n):
    """One launch of Engine.gevd_vast per order on five built pairs, bin k = SPECTRA[k], and the oracle's answer."""
    from ap_vast_unofficial_amd._capi import Engine
    rng = np.random.default_rng(77 + n)
    c = n // 4
    spectra = [np.concatenate([np.linspace(10.0, 1.0, n - c), np.full(c, 0.5)]), np.logspace(0, -12, n), np.logspace(0, -6, n),
               rng.uniform(0.1, 10.0, n), rng.uniform(0.1, 10.0, n)]
    conds = [10.0, 10.0, 10.0, 1e6, 10.0]
    RB, RD = np.empty((5, n, n), complex), np.empty((5, n, n), complex)
    for k in range(5):
        RB[k], RD[k] = _pencil(rng, spectra[k], conds[k])
    RD[4] -= 2.0 * np.eye(n)                       # G G^H has eigenvalues <= 1: now indefinite
    r = rng.standard_normal((5, n)) + 1j * rng.standard_normal((5, n))
    ranks = (1, n // 2, n - c, n)
    eng = Engine(5, n, n, ranks=ranks, mu=1e-3, compute_dtype="f64", reg_mode=0, reg_dark=1e-12)
    got = eng.gevd_vast(RB, RD, r, raise_on_status=False)
    eng.close()
    return ranks, got, subband.gevd_vast(RB, RD, r, 1e-3, list(ranks), reg=1e-12)


@pytest.mark.parametrize("spectrum", SPECTRA)
@pytest.mark.parametrize("n", [24, 40, 64])
def test_gevd_vast_prescribed_spectra(n, spectrum):
    """Engine.gevd_vast on built pairs (reg_dark 1e-12, mu 1e-3), all five in one launch: an exact n/4-fold cluster at 0.5 below
    linspace(10, 1), geometric spectra over 1e12 and over 1e6, cond(B) = 1e6, and a bin whose R_D is indefinite (status 1 there,
    zeros out; the other cases are its neighbours).  Inside a cluster w is not unique: it is compared where the gap exceeds
    1e-6 lambda_1, and over 1e12 at ranks 1 and n only (the oracle itself carries up to 4e-8 at the ranks between).

    Over 1e12 with mu = 1e-3 lambda_1 the float64 LDS kernel's stop threshold of 1e-16 ||C||_F^2 left w at rank n at 1.1e-7 of the
    oracle's at n = 24 (the oracle lies 6e-14 from a direct solve of (A + mu B) w = r there), and the 16-sweep cap ended the bin at
    status 2 at n = 64: the kernel now sweeps on to 1e-20 where lambda + mu reaches below 1e-2 lambda_1, with a cap of 24."""
    ranks, (w, lam, st), (wr, lr, sr) = _built_pencils(n)
    k = SPECTRA.index(spectrum)
    if spectrum == "indefinite":
        assert st[k] == 1 and sr[k] == 1
        assert np.all(w[k] == 0) and np.all(lam[k] == 0)
        return
    lerr = np.abs(lam[k] - lr[k]).max() / lr[k, 0]
    werr = {}
    for t, Vr in enumerate(ranks):
        if spectrum == "geometric_1e12" and Vr not in (1, n):
            continue
        if Vr < n and lr[k, Vr - 1] - lr[k, Vr] <= 1e-6 * lr[k, 0]:
            continue
        werr[Vr] = np.linalg.norm(w[k, t] - wr[k, t]) / np.linalg.norm(wr[k, t])
    print(f"D n = {n} {spectrum}: status {st[k]} lambda {lerr:.1e} w", {Vr: "%.1e" % e for Vr, e in werr.items()})
    assert st[k] == 0 and sr[k] == 0
    assert lerr <= 1e-9, lerr
    assert len(werr) == (2 if spectrum == "geometric_1e12" else 4) and max(werr.values()) <= 1e-7, werr
    if spectrum == "cluster":
        assert np.abs(lam[k, n - n // 4:] - 0.5).max() <= 1e-9 * lam[k, 0]        # the cluster's values themselves


# E -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [16, 512])            # gevd64_kernel; gevd64x2_kernel (two bins per workgroup from K * zones = 512 on)
@pytest.mark.parametrize("spectrum", ["geometric", "cluster"])
def test_update_structured_slabs_order_64(K, spectrum):
    """Engine.update at 64 x 72 on the construction of test_gpu_parity.test_spectra_at_the_trust_threshold: R_D = I (orthonormal dark
    slab), R_B = 9 U diag(lam) U^H, lam geometric over 1e6 or with an exact 16-fold cluster behind a gap (the c64 rounding of the
    slabs spreads it over 1e-7)."""
    from ap_vast_unofficial_amd._capi import Engine
    L, M, ranks = 64, 72, (1, 32, 48, 64)
    rng = np.random.default_rng(11)
    lam0 = {"geometric": np.geomspace(1.0, 1e-6, L), "cluster": np.r_[np.linspace(1.0, 0.5, 48), np.full(16, 1.5e-3)]}[spectrum]
    g = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    XB = np.zeros((K, M, L), np.complex128)
    XB[:, :L] = np.sqrt(lam0)[:, None] * np.linalg.qr(g(K, L, L))[0].conj().transpose(0, 2, 1) * 3.0
    XD = np.linalg.qr(g(K, M, L))[0]
    XB, XD, d = XB.astype(np.complex64), XD.astype(np.complex64), g(K, M).astype(np.complex64)
    eng = Engine(K, L, M, ranks=ranks, mu=0.1, compute_dtype="f64", out_c128=True)
    w, lam, status = eng.update(XB, XD, d)
    eng.close()
    w_ref, lam_ref = subband.update_vectorised(XB, XD, d, 0.1, list(ranks))
    lerr = (np.abs(lam - lam_ref).max(axis=1) / lam_ref[:, 0]).max()
    gap_ok = [t for t, Vr in enumerate(ranks) if Vr == L or (lam_ref[:, Vr - 1] - lam_ref[:, Vr] > 1e-6 * lam_ref[:, 0]).all()]
    werr = (np.linalg.norm(w - w_ref, axis=-1) / np.linalg.norm(w_ref, axis=-1))[:, gap_ok].max()
    print(f"E K = {K} {spectrum}: lambda {lerr:.1e} w {werr:.1e} (ranks {[ranks[t] for t in gap_ok]}) status != 0 in {int((status != 0).sum())} bins")
    assert not status.any()
    assert len(gap_ok) == 4
    assert lerr <= 1e-9 and werr <= 1e-7, (lerr, werr)
