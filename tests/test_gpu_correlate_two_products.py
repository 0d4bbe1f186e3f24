"""Stage 0 of the order-16 float64 update kernel (correlate16) forms each statistic from ONE real tile,

    G = sum_m  xr_m (x) (xr_m + xi_m)  +  xi_m (x) (xi_m - xr_m)  =  Re R + (P - P^T),     P = sum_m xr_m (x) xi_m,

two matrix-core products per k-step, and takes R_ij = ((G_ij + G_ji) / 2, (G_ij - G_ji) / 2) from G and its transpose.  These tests
hold that stage where the form could go wrong; they pass on the three-product form (Re R and P accumulated apart) as well.

Exact slabs.  Gaussian integers with parts in -3..3: a term of G is at most 3 * 6 = 18 in size, a sum over M <= 65 rows of two
terms stays below 2^12, and G_ij +- G_ji is an even integer (it is 2 Re R_ij, 2 Im R_ij), so the halving is exact: both forms give
the oracle's integer statistics bit for bit, in any order of summation.  Engine.update on the slabs therefore runs the stages
after stage 0 on the very numbers that the same handle's gevd_vast is given with the oracle's R_B, R_D and r.  The two launches are
different instantiations of one kernel body (fused stage 0 / statistics loaded from memory).  Measured on the three-product build
before the change, all nine cases: the filters and the eigenvalues of the two launches are equal bit for bit
(profiles/r12/new_tests_parent.log), so that is what is asserted.  reg_dark = 1.0 is exact in the addition and keeps
cond(R_D + reg I) below about 300 even at M = 1.

Quadrature columns.  X_B is Gaussian with its odd columns i times the even ones plus 1e-3 of noise: R_ij between such a pair is
almost purely imaginary, so Re R_ij is what is left when G_ij + G_ji cancels (the NumPy model of both forms, on c64 slabs with column
scales over six decades: worst element error 5.8e-16 of sqrt(R_ii R_jj) for this form, 6.8e-16 for the three products).  X_D is
sqrt(M) times an orthonormal factor, cond(R_D) = 1.  Checked against oracle.subband at TOL of test_gpu_parity, M = 31, 32, 33.
Errors measured on the device, eigenvalues on the scale of the largest / filters, three-product build | this form:

    M = 31   1.13e-14 / 9.15e-13  |  1.13e-14 / 9.15e-13
    M = 32   8.41e-15 / 3.59e-14  |  7.97e-15 / 3.69e-14
    M = 33   7.65e-15 / 2.95e-13  |  7.92e-15 / 2.96e-13

Break-it builds (profiles/r12/new_tests_break_*.log): `xi + xr` in place of `xi - xr` (Im R lost) and a missing factor 1/2 (the
statistics doubled, the loading, mu and r not) each fail all twelve cases.
"""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

from oracle import subband  # noqa: E402  (checker only)
from test_gpu_correlation_shapes import _integer_case, _lam_err  # noqa: E402
from test_gpu_parity import TOL, cn, w_err  # noqa: E402

L = 16
RANKS = (1, 8, 16)
MU = 0.7


def _engine(*a, **kw):
    from ap_vast_unofficial_amd import Engine
    return Engine(*a, **kw)


EXACT_CASES = [(5, M) for M in (1, 4, 5, 31, 32, 33, 64, 65)] + [(257, 33)]


@pytest.mark.parametrize("K,M", EXACT_CASES)
def test_exact_slabs(K, M):
    XB, XD, d, stats = _integer_case(K, M, L)
    eng = _engine(K, L, M, ranks=RANKS, mu=MU, compute_dtype="f64", reg_dark=1.0)
    try:
        w, lam, status = eng.update(XB, XD, d)
        w2, lam2, status2 = eng.gevd_vast(*stats)
    finally:
        eng.close()
    assert not status.any() and not status2.any()
    assert np.isfinite(w2).all() and np.isfinite(lam2).all() and np.abs(w2).max() > 0
    same = np.array_equal(w, w2) and np.array_equal(lam, lam2)
    e_lam, e_w = _lam_err(lam, lam2), w_err(w, w2)
    print(f"exact K={K} M={M}: bit for bit {same}; lam {e_lam:.2e} w {e_w:.2e}; moved: w {(w != w2).sum()} of {w.size}, "
          f"lam {(lam != lam2).sum()} of {lam.size}")
    assert np.array_equal(lam, lam2)
    assert np.array_equal(w, w2)


@functools.lru_cache(maxsize=None)
def _quadrature_case(M):
    K = 3
    rng = np.random.default_rng(51000 + M)
    XB = cn(rng, K, M, L).astype(np.complex128)
    XB[:, :, 1::2] = 1j * XB[:, :, 0::2] + 1e-3 * cn(rng, K, M, L // 2)
    XB = XB.astype(np.complex64)
    d = cn(rng, K, M)
    G = rng.standard_normal((K, M, L)) + 1j * rng.standard_normal((K, M, L))
    XD = (np.sqrt(M) * np.linalg.qr(G)[0]).astype(np.complex64)
    RB = subband.correlate(XB, XD, d)[0]
    # the pairs are in quadrature: Re R_ij is a small remainder beside Im R_ij
    pair = RB[:, np.arange(0, L, 2), np.arange(1, L, 2)]
    assert (np.abs(pair.real) < 1e-2 * np.abs(pair.imag)).all()
    w, lam, st = subband.update(XB, XD, d, MU, list(RANKS), reg=1e-7)
    assert not st.any()
    for a in (XB, XD, d, w, lam):
        a.setflags(write=False)
    return XB, XD, d, w, lam


@pytest.mark.parametrize("M", (31, 32, 33))
def test_quadrature_columns(M):
    XB, XD, d, w_ref, lam_ref = _quadrature_case(M)
    eng = _engine(XB.shape[0], L, M, ranks=RANKS, mu=MU, compute_dtype="f64", reg_dark=1e-7)
    try:
        w, lam, status = eng.update(XB, XD, d)
    finally:
        eng.close()
    assert not status.any()
    e_lam, e_w = _lam_err(lam, lam_ref), w_err(w, w_ref)
    print(f"quadrature M={M}: lam {e_lam:.2e} w {e_w:.2e}")
    assert e_lam < TOL["f64"]["lam"]
    assert e_w < TOL["f64"]["w"]
