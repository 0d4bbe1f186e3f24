"""The float64 stages of the order-16 kernel (kernels_gevd16m.hip): the whitening products of stage 2 and the sums over the four
16-lane rows of a wave.

  row sums by lane swaps the sums over the four 16-lane rows of a wave (r = X_B^H d, ||C||_F^2, the refinement's quotients and
                         second-order terms, the sort's ranks, g = W r, the coefficients, y and w) run on v_permlane16_swap /
                         v_permlane32_swap instead of ds_bpermute, with the same additions: every output keeps its bits
                         ("Row sums by lane swaps")
  C from one real tile   tried with it and not kept (it missed the timing rule): stage 2's Hermitian C = T1 W^H (T1 = W R_B) from
                         the real tile G = Re C + Im C = T1r (Wr - Wi)^T + T1i (Wr + Wi)^T, C_ij = ((G_ij + G_ji) / 2,
                         (G_ij - G_ji) / 2), 8 f64 MFMAs for 12.  The cases below were written to catch that form going wrong
                         (`identity`, `quadrature`, `skew`) and hold for the general product that stays.

  plain       257-bin slabs, M in {1, 8, 32, 33}, c64 and c128 outputs, fused and built pairs; ranks (8,) without a lam buffer and
              (1, 8, 16) with one, against the oracle; every rank of the list bit for bit its single-rank launch
  U           jdiag_batched (the entry that returns U) against the oracle: projectors, eigenvalues, U^H (R_D + reg I) U = I
  stream      c128 slabs: a float64 stream of 16 loudspeakers x 8 microphones, 257 bins, whose filters are held against the oracle's
              on the stream's own statistics
  identity    R_D = s I with s a power of four and Gaussian-integer R_B: W = I / sqrt(s) is real diagonal and C = R_B / s exact in
              both products, so that the tile's cancellations have nothing to hide behind; lam and w to TOL, every rank bit for
              bit its single-rank launch
  quadrature  R_B with purely imaginary off-diagonals (X_B's columns alternately real and imaginary): Re C_ij is what
              G_ij + G_ji leaves after cancelling
  skew        R_D with off-diagonals of large imaginary part, so that Wi is comparable to Wr; every rank bit for bit its
              single-rank launch here and in `quadrature` too
  scale       the 2^+-160 pencils of test_gpu_leading_half_refinement.py with ranks (1, 8, 16)
  rare        a NaN bin and a zero pivot between healthy bins: status 1 and zeros there, the neighbours keep their bits

Bounds.  TOL["f64"] of tests/test_gpu_parity.py (a c64 output adds its rounding, 2^-24), and for w also max(2 x the parent's worst,
1e-10), PARENT below holding the parent commit's figures of this file (profiles/r19/new_tests_parent.log).  No mark is pinned to
a bin.

Checked on scratch builds (profiles/r19/breakit_*.log): a rows_sum2 that hands row 1's sum to row 0 fails the suite's first filter
test (tests/test_gpu_parity.py) and this file; on the build with the real tile, `w.x + w.y` in both of its B operands and the tile
without its factor 1/2 each failed this file.
Run on the MI355X box with `-m gpu`."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, ROOT]

from oracle import gevd, subband  # noqa: E402  (checker only)
from presolve_cases import cn, rel_w  # noqa: E402
from test_gpu_leading_half_refinement import _engine, _launch, _plain as _plain_8_32_33, _reg  # noqa: E402
from test_gpu_parity import TOL  # noqa: E402

L, MU, REG = 16, 0.7, 1e-7
C64 = 2.0 ** -24
LIST = (1, 8, 16)
W_FLOOR = 1e-10
K_PLAIN = 257

# the parent commit's worst w (U: projector) error per case (profiles/r19/new_tests_parent.log)
PARENT = {
    "quadrature": 4.145e-10, "quadrature/imaginary": 6.548e-11, "plain/M1/c64/fused": 3.757e-08,
    "plain/M1/c64/built": 3.757e-08, "plain/M1/c128/fused": 9.212e-14, "plain/M1/c128/built": 9.212e-14,
    "plain/M8/c64/fused": 3.932e-08, "plain/M8/c64/built": 3.932e-08, "plain/M8/c128/fused": 4.753e-12,
    "plain/M8/c128/built": 4.307e-12, "plain/M32/c64/fused": 3.946e-08, "plain/M32/c64/built": 3.946e-08,
    "plain/M32/c128/fused": 1.451e-10, "plain/M32/c128/built": 1.451e-10, "plain/M33/c64/fused": 3.618e-08,
    "plain/M33/c64/built": 3.618e-08, "plain/M33/c128/fused": 1.233e-10, "plain/M33/c128/built": 1.230e-10,
    "plain/U": 6.149e-13, "stream/c128": 4.496e-09, "identity/4^0": 6.877e-11, "identity/4^3": 6.877e-11,
    "identity/4^-5": 6.877e-11, "skew": 3.360e-10, "scale/0": 4.030e-11, "scale/+160": 4.030e-11, "scale/-160": 4.030e-11,
}


def _tight(tag, e_w):
    bw = max(2 * PARENT[tag], W_FLOOR) if tag in PARENT else None
    print(f"FIGURES {tag}: w {e_w:.3e} (bound {bw})")
    assert bw is not None, f"no parent figure for {tag}"
    assert e_w <= bw, (tag, e_w, bw)


def _lam_err(lam, lam_ref, nz=L):
    return float((np.abs(lam[:, :nz] - lam_ref[:, :nz]) / np.abs(lam_ref[:, :1])).max())


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---------------------------------------------------------------------------------------------------------------------------
# plain slabs
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain(M):
    """slabs, pairs, {rank: w_ref}, lam_ref; M = 8, 32, 33 are the slabs of test_gpu_leading_half_refinement.py"""
    if M == 1:
        rng = np.random.default_rng(6100 + M)
        slabs = cn(rng, K_PLAIN, M, L), cn(rng, K_PLAIN, M, L), cn(rng, K_PLAIN, M)
    else:
        slabs = _plain_8_32_33(M)[0]
    pairs = subband.correlate(*slabs)
    w_ref, lam_ref, st = subband.gevd_vast(*pairs, MU, list(LIST), reg=_reg(M))
    assert not st.any()
    _frozen(*slabs, *pairs, w_ref, lam_ref)
    return slabs, pairs, dict(zip(LIST, np.moveaxis(w_ref, 1, 0))), lam_ref


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "built"])
@pytest.mark.parametrize("out_c128", [False, True], ids=["c64", "c128"])
@pytest.mark.parametrize("M", [1, 8, 32, 33])
def test_plain_against_oracle(M, out_c128, fused):
    slabs, pairs, w_ref, lam_ref = _plain(M)
    args = slabs if fused else pairs
    kw = dict(M=M, out_c128=out_c128, reg=_reg(M))
    extra = 0.0 if out_c128 else C64
    nz = min(L, M)                                   # beyond rank(R_B) the eigenvalues are rounding noise
    w, lam, st = _launch(args, LIST, fused, True, **kw)
    assert not st.any(), st
    assert _lam_err(lam, lam_ref, nz) < TOL["f64"]["lam"] + extra
    if M >= L:
        assert np.abs(lam / lam_ref - 1).max() < TOL["f64"]["lam"] + extra
    worst = 0.0
    for t, V in enumerate(LIST):
        if V <= nz:
            e_w = rel_w(w[:, t], w_ref[V])
            assert e_w < TOL["f64"]["w"] + extra, (V, e_w)
            worst = max(worst, e_w)
    w8, lam8, st8 = _launch(args, (8,), fused, False, **kw)
    assert lam8 is None and not st8.any()
    assert np.array_equal(w8[:, 0], w[:, 1])
    for t in (0, 2):
        assert np.array_equal(_launch(args, LIST[t:t + 1], fused, True, **kw)[0][:, 0], w[:, t]), LIST[t]
    _tight(f"plain/M{M}/{'c128' if out_c128 else 'c64'}/{'fused' if fused else 'built'}", worst)


def _U_errors(A, B, U, lam, reg=REG):
    """worst column projector u u^H against the oracle's, relative; jdiag's invariants (test_gpu_parity.test_jdiag_batched_invariants)"""
    e_U = 0.0
    for k in range(len(A)):
        U0, lam0 = gevd.jdiag(A[k], B[k])
        Bl = B[k] + reg * np.eye(L)
        assert np.abs(U[k].conj().T @ Bl @ U[k] - np.eye(L)).max() < 1e-11
        assert np.abs(U[k].conj().T @ A[k] @ U[k] - np.diag(lam[k])).max() < 1e-10 * lam[k, 0]
        assert (np.diff(lam[k]) <= 0).all() and np.abs(lam[k] / lam0 - 1).max() < TOL["f64"]["lam"]
        for c in range(L):
            P, P0 = np.outer(U[k][:, c], U[k][:, c].conj()), np.outer(U0[:, c], U0[:, c].conj())
            e_U = max(e_U, float(np.linalg.norm(P - P0) / np.linalg.norm(P0)))
    return e_U


def test_U_against_oracle():
    RB, RD = (a[:32] for a in _plain(32)[1][:2])
    eng = _engine(1, 4, 4)
    U, lam = eng.jdiag_batched(RB, RD)
    eng.close()
    e_U = _U_errors(RB, RD, U, lam)
    assert e_U < TOL["f64"]["w"]
    _tight("plain/U", e_U)


def test_stream_c128_slabs():
    """the float64 stream hands the kernel c128 slabs: its filters against the oracle's on the statistics the stream itself reports"""
    from test_gpu_stream import run_pair, synth_rirs
    rirA, rirB = synth_rirs(200, L, 8, 5)
    V = 8
    ap, _, _, _ = run_pair(512, 256, rirA, rirB, 12, 2, 5, V, 1.0, hops=2)
    worst = 0.0
    for names in (("R_A_to_A", "R_A_to_B", "r_A", "lambda_A", "w_A"), ("R_B_to_B", "R_B_to_A", "r_B", "lambda_B", "w_B")):
        RB, RD, r, lam, w = (np.asarray(getattr(ap, n)) for n in names)
        assert RB.shape == (257, L, L)
        w_ref, lam_ref, st = subband.gevd_vast(RB, RD, r, 1.0, list(range(1, V + 1)), reg=REG)
        assert not st.any()
        assert _lam_err(lam, lam_ref, 8) < TOL["f64"]["lam"]                 # 8 microphones: rank(R_B) = 8
        for v in range(V):
            e_w = rel_w(w[v], w_ref[:, v])
            assert e_w < TOL["f64"]["w"], (names[-1], v, e_w)
            worst = max(worst, e_w)
    ap.close()
    _tight("stream/c128", worst)


# ---------------------------------------------------------------------------------------------------------------------------
# built pencils that single out the tile
# ---------------------------------------------------------------------------------------------------------------------------
BINS = 24


def _gaussian_integer_RB(rng, M=24):
    """X^H X of Gaussian-integer X (|parts| <= 7): every element an exact Gaussian integer below 2^12"""
    X = rng.integers(-7, 8, (BINS, M, L)) + 1j * rng.integers(-7, 8, (BINS, M, L))
    return np.einsum("kmi,kmj->kij", X.conj(), X)


def _check_pencil(tag, RB, RD, r, reg=0.0, mu=MU):
    """lam and w to TOL, every rank bit for bit its single-rank launch"""
    w_ref, lam_ref, st = subband.gevd_vast(RB, RD, r, mu, list(LIST), reg=reg)
    assert not st.any()
    w, lam, st = _launch((RB, RD, r), LIST, False, True, reg=reg, mu=mu)
    assert not st.any(), st
    e_l, e_w = float(np.abs(lam / lam_ref - 1).max()), rel_w(w, w_ref)
    print(f"FIGURES {tag}: lam {e_l:.3e}")
    assert e_l < TOL["f64"]["lam"]
    assert e_w < TOL["f64"]["w"], e_w
    for t, V in enumerate(LIST):
        w1, _, st1 = _launch((RB, RD, r), (V,), False, V != 8, reg=reg, mu=mu)
        assert not st1.any()
        assert np.array_equal(w1[:, 0], w[:, t]), V
    _tight(tag, e_w)


@pytest.mark.parametrize("e", [0, 3, -5])
def test_identity_dark_matrix_exact_tile(e):
    """R_D = 4^e I without loading: W = 2^-e I, and both products of stage 2 are exact on Gaussian integers"""
    rng = np.random.default_rng(1901)
    RB = _gaussian_integer_RB(rng)
    r = (rng.integers(-9, 10, (BINS, L)) + 1j * rng.integers(-9, 10, (BINS, L))).astype(np.complex128)
    s = 4.0 ** e
    _check_pencil(f"identity/4^{e}", RB, np.broadcast_to(s * np.eye(L, dtype=np.complex128), RB.shape).copy(), r, mu=MU / s)


def test_quadrature_columns():
    """columns of X_B alternately real and imaginary: R_B's off-diagonals between a real and an imaginary column are purely
    imaginary, between two of a kind purely real; R_D = I keeps C = R_B, whose real parts come out of G_ij + G_ji by cancellation.
    Then every off-diagonal purely imaginary: R_B = D + i S with S real antisymmetric."""
    rng = np.random.default_rng(1902)
    X = rng.standard_normal((BINS, 32, L)).astype(np.complex128)
    X[:, :, 1::2] *= 1j
    RB = np.einsum("kmi,kmj->kij", X.conj(), X)
    assert np.abs(RB[:, 0::2, 1::2].real).max() == 0.0 and np.abs(RB[:, 0::2, 0::2].imag).max() == 0.0
    r = rng.standard_normal((BINS, L)) + 1j * rng.standard_normal((BINS, L))
    RD = np.broadcast_to(np.eye(L, dtype=np.complex128), RB.shape).copy()
    _check_pencil("quadrature", RB, RD, r, reg=REG)
    S = rng.standard_normal((BINS, L, L))
    S = S - S.transpose(0, 2, 1)
    S *= 0.5 / np.linalg.norm(S, 2, axis=(1, 2))[:, None, None]
    RB2 = (np.eye(L) * np.geomspace(4.0, 1.0, L))[None] + 1j * S
    assert np.abs(RB2[:, ~np.eye(L, dtype=bool)].real).max() == 0.0 and (np.linalg.eigvalsh(RB2) > 0.4).all()
    _check_pencil("quadrature/imaginary", RB2, RD, r, reg=REG)


def test_dark_matrix_with_large_imaginary_off_diagonals():
    """R_D = F F^H with F unit lower triangular and purely imaginary below the diagonal: W = F^-1 has imaginary parts of the size
    of its real parts below the diagonal"""
    rng = np.random.default_rng(1903)
    F = np.eye(L) + 0.4j * np.tril(rng.standard_normal((BINS, L, L)), -1)
    RD = F @ F.conj().transpose(0, 2, 1)
    RD = 0.5 * (RD + RD.conj().transpose(0, 2, 1))
    Wm = np.linalg.inv(np.linalg.cholesky(RD))
    low = np.tril(np.ones((L, L), bool), -1)
    assert np.abs(Wm[:, low].imag).mean() > 0.5 * np.abs(Wm[:, low].real).mean()
    XB = rng.standard_normal((BINS, 32, L)) + 1j * rng.standard_normal((BINS, 32, L))
    RB = np.einsum("kmi,kmj->kij", XB.conj(), XB)
    r = rng.standard_normal((BINS, L)) + 1j * rng.standard_normal((BINS, L))
    _check_pencil("skew", RB, RD, r, reg=REG)


# ---------------------------------------------------------------------------------------------------------------------------
# scale, rare entries
# ---------------------------------------------------------------------------------------------------------------------------
K_SCALE = 64


@functools.lru_cache(maxsize=None)
def _scale_runs():
    slabs, pairs, w_ref, _ = _plain(32)
    XB, XD, d = (a[:K_SCALE] for a in slabs)
    RB, RD, r = (a[:K_SCALE] for a in pairs)
    ref = np.stack([w_ref[V][:K_SCALE] for V in LIST], 1)
    runs = {}
    for e in (0, 40, -40):
        sb, sd = 2.0 ** e, 2.0 ** -e
        kw = dict(mu=MU * sb ** 2 / sd ** 2, reg=REG * sd ** 2)
        fused = _launch(((XB * np.float32(sb)).astype(np.complex64), (XD * np.float32(sd)).astype(np.complex64), d), LIST, True, True, **kw)
        built = _launch((RB * sb ** 2, RD * sd ** 2, r * sb), LIST, False, True, **kw)
        runs[4 * e] = (fused, built, ref / sb)
    return runs


@pytest.mark.parametrize("e", [0, 160, -160], ids=["0", "+160", "-160"])
def test_scale(e):
    runs = _scale_runs()
    fused, built, w_ref = runs[e]
    worst = 0.0
    for name, (w, _, status), (_, _, status0) in (("fused", fused, runs[0][0]), ("built", built, runs[0][1])):
        assert np.array_equal(status, status0) and not status.any(), (name, status)
        e_w = rel_w(w, w_ref)
        assert e_w < TOL["f64"]["w"], (name, e_w)
        worst = max(worst, e_w)
    _tight(f"scale/{e:+d}" if e else "scale/0", worst)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "built"])
def test_nan_bin_and_zero_pivot(fused):
    """bin 3 holds a NaN, bin 8 has R_D = 0 under a zero loading: status 1 and zeros on exactly those, the others bit for bit the
    launch without them"""
    K = 12
    XB, XD, d = (a[:K].copy() for a in _plain(32)[0])
    XD[3, 2, 9] = np.nan
    XD[8] = 0
    bad = np.zeros(K, bool)
    bad[[3, 8]] = True

    def run(sel):
        args = (XB[sel], XD[sel], d[sel]) if fused else subband.correlate(XB[sel], XD[sel], d[sel])
        return _launch(args, LIST, fused, True, reg=0.0)

    w, lam, status = run(np.ones(K, bool))
    assert np.array_equal(status == 1, bad) and not status[~bad].any(), status
    assert not w[bad].any() and not lam[bad].any()
    w0, lam0, st0 = run(~bad)
    assert not st0.any()
    assert np.array_equal(w[~bad], w0) and np.array_equal(lam[~bad], lam0)
    w_ref, _, _ = subband.update(XB[~bad], XD[~bad], d[~bad], MU, list(LIST), reg=0.0)
    assert rel_w(w[~bad], w_ref) < TOL["f64"]["w"]
