"""The shortened Sturm multisection of the float32 pre-solve (kernels_gevd16m.hip: kTpQuadSteps, the `apart` gate widened by the
multisection's own error, the spread gate read from quads 0 and 15) where it can go wrong: pairs of eigenvalues whose gap straddles
the gate's threshold, eigenvalues that sit on the grid points of a multisection in fifths (the kernel's first step was one when
these cases were chosen; it is a wave-wide step of a 65th now, whose own points tests/test_gpu_presolve_wide_step.py covers, and the
old points stay as inputs like any other), the share of bench bins that need a second refinement step against the NumPy model of
the kernel's steps, and a NaN that must fail the gate.  L = 16, explicit R_B / R_D (R_D = I, so the
whitened C is R_B / (1 + reg)), bounds as tests/test_gpu_tridiag_presolve.py applies them to its structured spectra.
Run on the MI355X box with `-m gpu`; the model's own share is checked without a GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import subband  # noqa: E402  (checker only)
from presolve_cases import (binomial_bound, check_nan_bin, refinement_marks, rel_w, with_spectrum,  # noqa: E402
                            model_second_step_share as model_share)

L, M = 16, 32
REG = 1e-7                                    # the engine's and the oracle's loading of R_D
MU, RANKS = 0.1, (1, 16)
GAPS = [1e-6, 3e-6, 7e-6, 1.2e-5, 3e-5, 1e-4, 1e-3]          # x ||C||_F
PLACES = {"bottom": 14, "middle": 7, "top": 0}               # index of the pair's larger eigenvalue, descending order
BINS_PER_CASE = 4
STEP_BINS = 1024


def pair_spectrum(gap, at):
    """geomspace(1, 0.05, 16) scaled to ||lam||_2 = 1 (= ||C||_F), eigenvalue at + 1 moved to `gap` below eigenvalue at"""
    lam = np.geomspace(1.0, 0.05, L)
    lam /= np.linalg.norm(lam)
    lam[at + 1] = lam[at] - gap
    return lam


def grid_spectra():
    """Spectra with ||lam||_2 = 1 whose eigenvalues sit on points of the first two steps of a multisection in fifths,
    lo + j (hi - lo) / 5 with [lo, hi] = [-1e-3, 1.001] ||C||_F, and at 0.  (Not all four first-step points at once: their squares
    sum to 1.2.)"""
    lo, w = -1e-3, 1.002
    g = [lo + j * w / 5 for j in range(1, 5)]
    g2 = [g[0] + j * w / 25 for j in range(1, 5)]            # second step, inside [g_1, g_2]
    out = {}
    for name, fixed in (("first_123_and_zero", [g[2], g[1], g[0], 0.0]), ("first_4_1_and_zero", [g[3], g[0], 0.0]),
                        ("second_step", [g[1], g2[2], g2[0], g[0]]), ("zero_only", [0.0])):
        fill = np.geomspace(0.15, 0.02, L - len(fixed)) * (1 + 0.01 * np.arange(L - len(fixed)))
        rest = 1.0 - float(np.sum(np.square(fixed)))
        fill *= np.sqrt(rest / np.sum(fill * fill))
        lam = np.sort(np.r_[fixed, fill])[::-1]
        assert abs(np.linalg.norm(lam) - 1) < 1e-12 and np.diff(lam).max() < -1e-4, name
        out[name] = lam
    return out


@pytest.fixture(scope="module")
def Engine():
    from ap_vast_unofficial_amd import Engine
    return Engine


def solve(Engine, RB, r):
    """(w, lam, status) of the GPU and (w, lam) of the oracle for R_B = the given matrices, R_D = I"""
    K = RB.shape[0]
    RD = np.broadcast_to(np.eye(L, dtype=np.complex128), RB.shape).copy()
    eng = Engine(K, L, M, ranks=RANKS, mu=MU, compute_dtype="f64", out_c128=True)
    w, lam, status = eng.gevd_vast(RB, RD, r, raise_on_status=False)
    eng.close()
    w_ref, lam_ref, _ = subband.gevd_vast(RB, RD, r, MU, list(RANKS))
    return w, lam, status, w_ref, lam_ref


def check(res, sel, RB, simple_top):
    w, lam, status, w_ref, lam_ref = (a[sel] for a in res)
    lam_np = np.linalg.eigvalsh(RB[sel])[:, ::-1] / (1 + REG)
    e_or = (np.abs(lam - lam_ref) / lam_ref[:, :1]).max()
    e_np = (np.abs(lam - lam_np) / lam_np[:, :1]).max()
    e_w16 = rel_w(w[:, 1:], w_ref[:, 1:])
    e_w1 = rel_w(w[:, :1], w_ref[:, :1])
    print(f"status {np.unique(status)}  lam vs oracle {e_or:.2e}  vs eigh {e_np:.2e}  w(rank 16) {e_w16:.2e}  w(rank 1) {e_w1:.2e}")
    assert not status.any(), status
    assert e_or < 1e-12 and e_np < 1e-12
    # the full-rank filter is a function of the whole pencil, defined however a close pair's vectors are chosen; it is wrong if
    # the eigenvector matrix lacks a direction
    assert e_w16 < 1e-7
    if simple_top:
        assert e_w1 < 1e-7


@pytest.fixture(scope="module")
def close_pairs(Engine):
    rng = np.random.default_rng(47)
    cases, RB = {}, []
    for gap in GAPS:
        for place, at in PLACES.items():
            cases[(gap, place)] = slice(len(RB), len(RB) + BINS_PER_CASE)
            RB += [with_spectrum(rng, pair_spectrum(gap, at)) for _ in range(BINS_PER_CASE)]
    RB = np.array(RB)
    r = rng.standard_normal((len(RB), L)) + 1j * rng.standard_normal((len(RB), L))
    return cases, RB, solve(Engine, RB, r)


@pytest.mark.gpu
@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("gap", GAPS)
def test_close_pairs(close_pairs, gap, place):
    """One pair `gap` ||C|| apart, below, at and above the `apart` threshold: a gate that is too lax would hand back a wrong
    eigenvector with status 0."""
    cases, RB, res = close_pairs
    check(res, cases[(gap, place)], RB, simple_top=place != "top")


@pytest.fixture(scope="module")
def grid_points(Engine):
    rng = np.random.default_rng(53)
    cases, RB = {}, []
    for name, lam in grid_spectra().items():
        cases[name] = slice(len(RB), len(RB) + 16)
        RB += [with_spectrum(rng, lam) for _ in range(16)]
    RB = np.array(RB)
    r = rng.standard_normal((len(RB), L)) + 1j * rng.standard_normal((len(RB), L))
    return cases, RB, solve(Engine, RB, r)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(grid_spectra()))
def test_eigenvalue_at_a_multisection_point(grid_points, name):
    """Eigenvalues on the points the first two steps of a multisection in fifths evaluate (where the kernel evaluated these very
    points, a pivot of the Sturm recurrence was at or next to zero) and an eigenvalue 0 (a singular C: the spread gate sends it to
    the double sweeps)."""
    cases, RB, res = grid_points
    check(res, cases[name], RB, simple_top=True)


@pytest.fixture(scope="module")
def model_second_step_share():
    """share of the first STEP_BINS bench-distribution bins outside the one-step guard |Z| <= 3e-5 in the NumPy model"""
    return model_share(STEP_BINS)


def test_model_second_step_share(model_second_step_share):
    assert model_second_step_share <= 0.02, model_second_step_share


@pytest.mark.gpu
def test_step_marks(Engine, model_second_step_share):
    """debug_stop = 9 marks a bin 8 if it missed the first refinement step's guard and 16 if it missed the second step's too.
    No bench bin may be left to the double sweeps, and the share that needs the second step may exceed the model's (wide step,
    NQUAD_KERNEL quad steps, best of four, 1-ulp noise on the pivots' reciprocals) by at most three standard deviations of a
    binomial count over STEP_BINS draws."""
    import bench
    XB, XD, d = bench.synth(STEP_BINS, 1234)
    status = refinement_marks(Engine, XB, XD, d, mu=1.0)
    p = model_second_step_share
    share = np.count_nonzero(status == 8) / STEP_BINS
    bound = binomial_bound(p, STEP_BINS)
    print(f"second step {share:.4f}, model {p:.4f}, bound {bound:.4f}")
    assert np.count_nonzero(status == 16) == 0
    assert share <= bound, (share, p, bound)


@pytest.mark.gpu
def test_nan_fails_the_gate(Engine):
    """A NaN in one bin's R_B (through its X_B) gives that bin a non-zero status and leaves its neighbours' results as they are
    without it: bin 29 of 64, ranks (1, 16)."""
    check_nan_bin(Engine, K=64, k0=29, ranks=RANKS)
