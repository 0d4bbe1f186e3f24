"""The float64 whitening of the order-16 kernel (kernels_gevd16m.hip, stages 0-2) fed from registers ("Whitening from
registers"):

  T1 from registers      the first product is formed transposed, X = (W R_B)^T, and its accumulator is the A operand of the second:
                         T1 = W R_B never goes to LDS
  C from one real tile   the Hermitian C = T1 W^H from G = Re C + Im C = T1r (Wr - Wi)^T + T1i (Wr + Wi)^T (8 f64 MFMAs for 12),
                         C_ij = ((G_ij + G_ji) / 2, (G_ij - G_ji) / 2); C moves in its last digits
  R_D rows from G        on slabs the Cholesky's lanes un-mix their rows of R_D from the correlation's real tile themselves

  plain       257-bin c64 slabs, M in {1, 8, 32, 33, 40} (40: a full chunk of 32 control points and a ragged one), c64 and c128
              outputs; ranks (8,) without a lam buffer and (1, 8, 16) with one, against the oracle; every rank of the list bit for
              bit its single-rank launch; one launch with built pairs.  (c128 slabs reach the kernel through the float64 stream
              only: `stream`.)
  U           jdiag_batched (the entry that returns U) against the oracle
  stream      c128 slabs: a float64 stream of 16 loudspeakers x 8 microphones, 257 bins, hop by hop (the grouped instantiation) and
              then through process_signal (the hops instantiations), its filters held against the oracle's on the statistics the
              stream itself reports
  skew        R_D = F F^H with F purely imaginary below the diagonal: Wi is of the size of Wr, so a slip in the tile's B operands
              (Wr - Wi, Wr + Wi) or in the transposition of the first product shows at full size
  quadrature  R_B with purely imaginary off-diagonals, where Re C comes out of G_ij + G_ji by cancellation
  symmetric   R_B real symmetric: Im C comes from Wi alone
  identity    R_D = 4^e I with Gaussian-integer R_B: W is real diagonal and both products are exact.  This pencil has Wi = 0, so
              it tells nothing about the Wi terms of the tile; it checks the factor 1/2, the un-mixing and the scaling, with no
              rounding to hide behind.
  fused skew  slabs X_D = Z F^H whose R_D has large imaginary off-diagonals: a conjugated R_D (G_ij and G_ji exchanged where
              the Cholesky un-mixes its rows) cannot pass
  scale       the 2^+-160 pencils of test_gpu_leading_half_refinement.py with ranks (1, 8, 16)
  rare        a NaN bin and a zero pivot between healthy bins: status 1 and zeros there, the neighbours keep their bits

Bounds.  TOL["f64"] of tests/test_gpu_parity.py against the oracle (a c64 output adds its rounding, 2^-24); for w also
max(2 x the parent's worst, 1e-10) and for the eigenvalues max(2 x the parent's worst, 1e-13), the error taken relative to
||C||_F = |lam_ref|_2 of the bin.  PARENT holds the parent commit's figures of this file (profiles/r20/new_tests_parent.log).  No
mark is pinned to a bin.

Checked on scratch builds (profiles/r20/breakit_*.log), each of which fails this file: the first product left untransposed while
the second reads it as X^T; `w.x + w.y` in both operands of the tile; the tile without its factor 1/2; G_ij and G_ji exchanged
in the Cholesky's rows.
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

from oracle import subband  # noqa: E402  (checker only)
from presolve_cases import cn, rel_w  # noqa: E402
from test_gpu_leading_half_refinement import _engine, _launch, _reg  # noqa: E402
from test_gpu_parity import TOL  # noqa: E402
from test_gpu_whitening_real_tile import _U_errors, _gaussian_integer_RB, _plain as _plain_1_8_32_33, _scale_runs  # noqa: E402

L, MU, REG = 16, 0.7, 1e-7
C64 = 2.0 ** -24
LIST = (1, 8, 16)
W_FLOOR, LAM_FLOOR = 1e-10, 1e-13
K_PLAIN = 257
BINS = 24

# the parent commit's worst errors per case, (w or U projector, eigenvalues / ||C||_F) (profiles/r20/new_tests_parent.log)
PARENT = {
    "plain/M1/c64/fused": (3.757e-08, 5.273e-08), "plain/M1/c128/fused": (9.212e-14, 4.670e-14),
    "plain/M8/c64/fused": (3.932e-08, 4.365e-08), "plain/M8/c128/fused": (4.753e-12, 2.636e-13),
    "plain/M32/c64/fused": (3.946e-08, 4.012e-08), "plain/M32/c128/fused": (1.451e-10, 2.442e-15),
    "plain/M33/c64/fused": (3.618e-08, 4.825e-08), "plain/M33/c128/fused": (1.233e-10, 2.043e-15),
    "plain/M40/c64/fused": (3.753e-08, 3.766e-08), "plain/M40/c128/fused": (6.875e-11, 1.844e-15),
    "plain/M33/c128/built": (1.230e-10, 1.553e-15), "plain/U": (6.149e-13, None), "stream/c128/hop": (4.496e-09, 4.355e-10),
    "stream/c128/signal": (2.441e-09, 3.055e-10), "skew": (5.629e-10, 5.976e-15),
    "quadrature/imaginary": (3.862e-10, 8.188e-15), "symmetric": (6.656e-10, 5.357e-15),
    "symmetric/identity": (1.073e-10, 7.661e-16), "identity/4^0": (6.877e-11, 5.854e-16),
    "identity/4^3": (6.877e-11, 5.854e-16), "identity/4^-5": (6.877e-11, 5.854e-16), "skew/fused": (3.005e-11, 1.801e-13),
    "scale/0": (4.030e-11, None), "scale/+160": (4.030e-11, None), "scale/-160": (4.030e-11, None),
}


def _tight(*figures):
    """figures: (tag, w error[, eigenvalue error]) each; every line is printed before the first bound is applied"""
    checks = []
    for tag, e_w, e_l in ((f + (None,))[:3] for f in figures):
        pw, pl = PARENT.get(tag, (None, None))
        bw = max(2 * pw, W_FLOOR) if pw is not None else None
        bl = max(2 * pl, LAM_FLOOR) if pl is not None else None
        print(f"FIGURES {tag}: w {e_w:.3e} (bound {bw}) lam {'-' if e_l is None else format(e_l, '.3e')} (bound {bl})")
        checks.append((tag, e_w, bw, e_l, bl))
    for tag, e_w, bw, e_l, bl in checks:
        assert bw is not None, f"no parent figure for {tag}"
        assert e_w <= bw, (tag, e_w, bw)
        if e_l is not None:
            assert bl is not None, f"no parent eigenvalue figure for {tag}"
            assert e_l <= bl, (tag, e_l, bl)


def _lam_abs(lam, lam_ref):
    """worst eigenvalue error relative to ||C||_F = |lam_ref|_2 of its bin"""
    return float((np.abs(lam - lam_ref).max(axis=-1) / np.linalg.norm(lam_ref, axis=-1)).max())


def _lam_err(lam, lam_ref, nz=L):
    return float((np.abs(lam[:, :nz] - lam_ref[:, :nz]) / np.abs(lam_ref[:, :1])).max())


# ---------------------------------------------------------------------------------------------------------------------------
# plain slabs
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain(M):
    """slabs, pairs, {rank: w_ref}, lam_ref; M = 1, 8, 32, 33 are the slabs (and references) of test_gpu_whitening_real_tile.py"""
    if M != 40:
        return _plain_1_8_32_33(M)
    rng = np.random.default_rng(6100 + M)
    slabs = cn(rng, K_PLAIN, M, L), cn(rng, K_PLAIN, M, L), cn(rng, K_PLAIN, M)
    pairs = subband.correlate(*slabs)
    w_ref, lam_ref, st = subband.gevd_vast(*pairs, MU, list(LIST), reg=_reg(M))
    assert not st.any()
    for a in (*slabs, *pairs, w_ref, lam_ref):
        a.setflags(write=False)
    return slabs, pairs, dict(zip(LIST, np.moveaxis(w_ref, 1, 0))), lam_ref


def _plain_case(M, out_c128, fused):
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
    _tight((f"plain/M{M}/{'c128' if out_c128 else 'c64'}/{'fused' if fused else 'built'}", worst, _lam_abs(lam, lam_ref)))


@pytest.mark.parametrize("out_c128", [False, True], ids=["c64", "c128"])
@pytest.mark.parametrize("M", [1, 8, 32, 33, 40])
def test_slabs_against_oracle(M, out_c128):
    _plain_case(M, out_c128, True)


def test_built_pairs_against_oracle():
    _plain_case(33, True, False)


def test_U_against_oracle():
    RB, RD = (a[:32] for a in _plain(32)[1][:2])
    eng = _engine(1, 4, 4)
    U, lam = eng.jdiag_batched(RB, RD)
    eng.close()
    e_U = _U_errors(RB, RD, U, lam)
    assert e_U < TOL["f64"]["w"]
    _tight(("plain/U", e_U))


def test_stream_c128_slabs():
    """the float64 stream hands the kernel c128 slabs: its filters against the oracle's on the statistics the stream itself
    reports, after two single hops (grouped spectra) and after three more through process_signal (several hops per launch)"""
    from test_gpu_stream import run_pair, synth_rirs
    rirA, rirB = synth_rirs(200, L, 8, 5)
    V = 8
    ap, _, _, _ = run_pair(512, 256, rirA, rirB, 12, 2, 5, V, 1.0, hops=2)

    def check():
        worst_w = worst_l = 0.0
        for names in (("R_A_to_A", "R_A_to_B", "r_A", "lambda_A", "w_A"), ("R_B_to_B", "R_B_to_A", "r_B", "lambda_B", "w_B")):
            RB, RD, r, lam, w = (np.asarray(getattr(ap, n)) for n in names)
            assert RB.shape == (257, L, L)
            w_ref, lam_ref, st = subband.gevd_vast(RB, RD, r, 1.0, list(range(1, V + 1)), reg=REG)
            assert not st.any()
            assert _lam_err(lam, lam_ref, 8) < TOL["f64"]["lam"]                 # 8 microphones: rank(R_B) = 8
            worst_l = max(worst_l, _lam_abs(lam, lam_ref))
            for v in range(V):
                e_w = rel_w(w[v], w_ref[:, v])
                assert e_w < TOL["f64"]["w"], (names[-1], v, e_w)
                worst_w = max(worst_w, e_w)
        return worst_w, worst_l

    first = check()
    x = np.random.default_rng(98).standard_normal((2, 3 * ap.hop_size))
    ap.process_signal(x[0], x[1])
    second = check()
    ap.close()
    _tight(("stream/c128/hop", *first), ("stream/c128/signal", *second))


# ---------------------------------------------------------------------------------------------------------------------------
# pencils that can tell a slip
# ---------------------------------------------------------------------------------------------------------------------------
def _check_pencil(tag, RB, RD, r, reg=0.0, mu=MU):
    """lam and w to TOL, every rank bit for bit its single-rank launch; returns the case's figures for _tight"""
    w_ref, lam_ref, st = subband.gevd_vast(RB, RD, r, mu, list(LIST), reg=reg)
    assert not st.any()
    w, lam, st = _launch((RB, RD, r), LIST, False, True, reg=reg, mu=mu)
    assert not st.any(), st
    e_l, e_w = float(np.abs(lam / lam_ref - 1).max()), rel_w(w, w_ref)
    assert e_l < TOL["f64"]["lam"], e_l
    assert e_w < TOL["f64"]["w"], e_w
    for t, V in enumerate(LIST):
        w1, _, st1 = _launch((RB, RD, r), (V,), False, V != 8, reg=reg, mu=mu)
        assert not st1.any()
        assert np.array_equal(w1[:, 0], w[:, t]), V
    return tag, e_w, _lam_abs(lam, lam_ref)


def _skew_factor(rng):
    """F unit lower triangular, purely imaginary below the diagonal: W = F^-1 has imaginary parts of the size of its real parts"""
    F = np.eye(L) + 0.4j * np.tril(rng.standard_normal((BINS, L, L)), -1)
    Wm = np.linalg.inv(F)
    low = np.tril(np.ones((L, L), bool), -1)
    assert np.abs(Wm[:, low].imag).mean() > 0.5 * np.abs(Wm[:, low].real).mean()
    return F


def test_dark_matrix_with_large_imaginary_off_diagonals():
    rng = np.random.default_rng(2003)
    F = _skew_factor(rng)
    RD = F @ F.conj().transpose(0, 2, 1)
    RD = 0.5 * (RD + RD.conj().transpose(0, 2, 1))
    XB = rng.standard_normal((BINS, 32, L)) + 1j * rng.standard_normal((BINS, 32, L))
    RB = np.einsum("kmi,kmj->kij", XB.conj(), XB)
    r = rng.standard_normal((BINS, L)) + 1j * rng.standard_normal((BINS, L))
    _tight(_check_pencil("skew", RB, RD, r, reg=REG))


def test_quadrature_and_real_symmetric_bright_matrix():
    """R_B = D + i S with S real antisymmetric (every off-diagonal purely imaginary), and R_B real symmetric, each under the skew
    dark matrix, whose W mixes real and imaginary parts at full size"""
    rng = np.random.default_rng(2002)
    F = _skew_factor(rng)
    RD = F @ F.conj().transpose(0, 2, 1)
    RD = 0.5 * (RD + RD.conj().transpose(0, 2, 1))
    r = rng.standard_normal((BINS, L)) + 1j * rng.standard_normal((BINS, L))
    S = rng.standard_normal((BINS, L, L))
    S = S - S.transpose(0, 2, 1)
    S *= 0.5 / np.linalg.norm(S, 2, axis=(1, 2))[:, None, None]
    RB = (np.eye(L) * np.geomspace(4.0, 1.0, L))[None] + 1j * S
    assert np.abs(RB[:, ~np.eye(L, dtype=bool)].real).max() == 0.0 and (np.linalg.eigvalsh(RB) > 0.4).all()
    figures = [_check_pencil("quadrature/imaginary", RB, RD, r, reg=REG)]
    X = rng.standard_normal((BINS, 32, L))
    RB2 = np.einsum("kmi,kmj->kij", X, X).astype(np.complex128)
    assert np.abs(RB2.imag).max() == 0.0
    figures.append(_check_pencil("symmetric", RB2, RD, r, reg=REG))
    figures.append(_check_pencil("symmetric/identity", RB2, np.broadcast_to(np.eye(L, dtype=np.complex128), RB2.shape).copy(), r, reg=REG))
    _tight(*figures)


@pytest.mark.parametrize("e", [0, 3, -5])
def test_identity_dark_matrix_exact_products(e):
    """R_D = 4^e I without loading: W = 2^-e I and every product of the whitening is exact on Gaussian integers.  Wi = 0 here: the
    case says nothing about the Wi terms of the tile (`skew` does); it holds the factor 1/2, the un-mixing and the scaling"""
    rng = np.random.default_rng(1901)
    RB = _gaussian_integer_RB(rng)
    r = (rng.integers(-9, 10, (BINS, L)) + 1j * rng.integers(-9, 10, (BINS, L))).astype(np.complex128)
    s = 4.0 ** e
    _tight(_check_pencil(f"identity/4^{e}", RB, np.broadcast_to(s * np.eye(L, dtype=np.complex128), RB.shape).copy(), r, mu=MU / s))


def test_slabs_with_skew_dark_matrix():
    """fused: X_D = Z F^H, so that R_D = F (Z^H Z) F^H has imaginary off-diagonals of the size of the real ones: the rows of R_D the
    Cholesky's lanes un-mix from G must carry the right sign"""
    rng = np.random.default_rng(2004)
    F = _skew_factor(rng)
    XB = cn(rng, BINS, 33, L)
    XD = (cn(rng, BINS, 33, L).astype(np.complex128) @ F.conj().transpose(0, 2, 1)).astype(np.complex64)
    d = cn(rng, BINS, 33)
    RB, RD, r = subband.correlate(XB, XD, d)
    off = ~np.eye(L, dtype=bool)
    assert np.abs(RD[:, off].imag).mean() > 0.5 * np.abs(RD[:, off].real).mean()
    w_ref, lam_ref, st = subband.gevd_vast(RB, RD, r, MU, list(LIST), reg=REG)
    assert not st.any()
    w, lam, st = _launch((XB, XD, d), LIST, True, True, M=33, reg=REG)
    assert not st.any(), st
    e_w = rel_w(w, w_ref)
    assert np.abs(lam / lam_ref - 1).max() < TOL["f64"]["lam"]
    assert e_w < TOL["f64"]["w"], e_w
    wb, lamb, stb = _launch((RB, RD, r), LIST, False, True, M=33, reg=REG)      # the built pair of the same slabs
    assert not stb.any() and rel_w(w, wb) < TOL["f64"]["w"]
    _tight(("skew/fused", e_w, _lam_abs(lam, lam_ref)))


# ---------------------------------------------------------------------------------------------------------------------------
# scale, rare entries
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [0, 160, -160], ids=["0", "+160", "-160"])
def test_scale(e):
    runs = _scale_runs()                             # the launches of test_gpu_whitening_real_tile.py, shared
    fused, built, w_ref = runs[e]
    worst = 0.0
    for name, (w, _, status), (_, _, status0) in (("fused", fused, runs[0][0]), ("built", built, runs[0][1])):
        assert np.array_equal(status, status0) and not status.any(), (name, status)
        e_w = rel_w(w, w_ref)
        assert e_w < TOL["f64"]["w"], (name, e_w)
        worst = max(worst, e_w)
    # R_B grows by 2^(e/2) and R_D shrinks by it: the eigenvalues scale by 2^e, and powers of two pass through every stage
    s = 2.0 ** e
    for (_, lam, _), (_, lam0, _) in ((fused, runs[0][0]), (built, runs[0][1])):
        assert np.abs(lam / s / lam0 - 1).max() < TOL["f64"]["lam"]
    _tight((f"scale/{e:+d}" if e else "scale/0", worst))


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
