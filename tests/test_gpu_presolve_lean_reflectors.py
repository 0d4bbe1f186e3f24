"""The lean reflectors of the float32 pre-solve (kernels_gevd16m.hip: complex multiply-accumulates with the swap and the sign as
operand modifiers, wave sums that end in a scalar register, row selects on constant lane masks, the last reflector taken as the
sign it is) where they can go wrong.  The refinement certifies the result whatever the pre-solve delivers, so a wrong modifier or
a wrong wave sum does not give a wrong filter: it sends bins to a second refinement step or to the double sweeps.  Hence every
group is looked at twice, against the oracle and through the marks of a debug_stop = 9 run.

  last reflector   block-diagonal C whose trailing 2 x 2 block sets alpha = C'[15][14] as reflector 14 meets it: zero, real
                   negative, purely imaginary, 1e-6 ||C||
  reflector sizes  block-diagonal C with a leading dense block of order 2, 3, 5, 9, 13 and a diagonal rest: the reflectors run
                   through every number of active column slots, and meet zero columns after the block
  bench marks      the first 1 024 bench bins against the NumPy model of the kernel's steps
  NaN              one NaN bin of 64 fails the gate, its neighbours stay bit for bit

Bins as test_gpu_hermitian_reflectors.py builds them: X_D the leading identity, so that the whitening is an exact scaling and the
structure of R_B = X_B^H X_B is that of the whitened C.  Bounds as that file's.  Run on the MI355X box with `-m gpu`."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import subband  # noqa: E402  (checker only)
from presolve_cases import (binomial_bound, check_nan_bin, cn, model_second_step_share, presolve_model,  # noqa: E402
                            refinement_marks, rel_w, unitary)

K, L, M = 32, 16, 32
REG = 1e-7                                    # the engine's and the oracle's loading of R_D
MU, RANKS = 0.1, (1, 16)
LAM = np.geomspace(1.0, 0.05, L)
ALPHAS = ["zero", "real_negative", "imaginary", "tiny"]
ORDERS = [2, 3, 5, 9, 13]
STEP_BINS = 1024


@pytest.fixture(scope="module")
def Engine():
    from ap_vast_unofficial_amd import Engine
    return Engine


def identity_XD(n):
    XD = np.zeros((n, M, L), np.complex64)
    XD[:, :L] = np.eye(L)
    return XD


def last_reflector_bins(case, rng):
    """C = blockdiag(C_14, B) with C_14 of spectrum LAM[:14] and random eigenvectors, and B = T^H T for the upper triangular
    T = [[a, conj(b)], [0, c]], a = sqrt(LAM[14]), c = sqrt(LAM[15]): C[15][14] = a b.  The reflectors 0 .. 12 leave rows and
    columns 14, 15 alone (zeros times anything), reflector 13 meets an exactly zero column (gamma = 0), so reflector 14 meets
    alpha = a b / (1 + reg) as the float32 conversion of C holds it."""
    XB = np.zeros((K, M, L), np.complex128)
    a, c = np.sqrt(LAM[14]), np.sqrt(LAM[15])
    norm_c = np.linalg.norm(LAM)                                       # ||C||_F to the few per cent the tiny case needs
    for k in range(K):
        XB[k, :14, :14] = np.sqrt(LAM[:14])[:, None] * unitary(rng, 14).conj().T
        size = rng.uniform(0.05, 0.15)
        b = {"zero": 0.0, "real_negative": -size, "imaginary": (1j if k & 1 else -1j) * size,
             "tiny": 1e-6 * norm_c / a * np.exp(2j * np.pi * rng.uniform())}[case]
        XB[k, 14:16, 14:16] = [[a, np.conj(b)], [0.0, c]]               # B[1][0] = conj(T[0][1]) T[0][0] = a b
    return XB.astype(np.complex64), identity_XD(K)


def block_bins(n, rng):
    """C = blockdiag(B_n, D): B_n dense of order n with random unitary eigenvectors, D diagonal, the spectrum LAM dealt at random
    between the two.  Reflector k < n - 1 acts on n - 1 - k rows; from n - 1 on every column below the diagonal is exactly zero."""
    XB = np.zeros((K, M, L), np.complex128)
    for k in range(K):
        perm = rng.permutation(L)
        XB[k, :n, :n] = np.sqrt(LAM[perm[:n]])[:, None] * unitary(rng, n).conj().T
        XB[k, np.arange(n, L), np.arange(n, L)] = np.sqrt(LAM[perm[n:]])
    return XB.astype(np.complex64), identity_XD(K)


def whitened(XB):
    XB = XB.astype(np.complex128)
    return (XB.conj().transpose(0, 2, 1) @ XB) / (1 + REG)


def test_inputs_have_the_structure():
    """The structure is exact in the complex64 inputs themselves (runs without a GPU: it only inspects the inputs)."""
    rng = np.random.default_rng(59)
    for case in ALPHAS:
        XB, _ = last_reflector_bins(case, rng)
        C = whitened(XB)
        assert not C[:, 14:, :14].any() and not C[:, :14, 14:].any()
        al, nrm = C[:, 15, 14], np.linalg.norm(C, axis=(1, 2))
        if case == "zero":
            assert not al.any()
        elif case == "real_negative":
            assert not al.imag.any() and (al.real < -1e-3).all()
        elif case == "imaginary":
            assert not al.real.any() and (np.abs(al.imag) > 1e-3).all() and (al.imag > 0).any() and (al.imag < 0).any()
        else:
            assert np.allclose(np.abs(al) / nrm, 1e-6, rtol=0.05)
    for n in ORDERS:
        XB, _ = block_bins(n, rng)
        C = whitened(XB)
        off = C.copy()
        off[:, :n, :n] = 0
        off[:, np.arange(L), np.arange(L)] = 0
        assert not off.any() and np.abs(C[:, :n, :n]).min() > 0


def against_oracle(Engine, XB, XD, d, label):
    eng = Engine(XB.shape[0], L, M, ranks=RANKS, mu=MU, compute_dtype="f64", out_c128=True)
    w, lam_gpu, status = eng.update(XB, XD, d, raise_on_status=False)
    eng.close()
    w_ref, lam_ref, _ = subband.update(XB, XD, d, MU, list(RANKS))
    lam_err = (np.abs(lam_gpu - lam_ref) / lam_ref[:, :1]).max()
    w16_err, w1_err = rel_w(w[:, 1:], w_ref[:, 1:]), rel_w(w[:, :1], w_ref[:, :1])
    print(f"{label}: lam {lam_err:.2e}  w(rank 16) {w16_err:.2e}  w(rank 1) {w1_err:.2e}  status {np.unique(status)}")
    assert not status.any()
    assert lam_err < 1e-12
    assert w16_err < 1e-7
    assert w1_err < 1e-7            # the spectrum is simple: the leading eigenvector is defined


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALPHAS)
def test_last_reflector_against_oracle(Engine, case):
    rng = np.random.default_rng(59)
    XB, XD = last_reflector_bins(case, rng)
    against_oracle(Engine, XB, XD, cn(rng, K, M), case)


@pytest.mark.gpu
def test_last_reflector_stays_on_the_refinement(Engine):
    rng = np.random.default_rng(59)
    parts = [last_reflector_bins(case, rng) for case in ALPHAS]
    XB, XD = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    status = refinement_marks(Engine, XB, XD, cn(rng, XB.shape[0], M), mu=MU)
    assert np.count_nonzero(status == 16) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", ORDERS)
def test_reflector_sizes_against_oracle(Engine, n):
    rng = np.random.default_rng(61)
    XB, XD = block_bins(n, rng)
    against_oracle(Engine, XB, XD, cn(rng, K, M), f"leading block of order {n}")


@pytest.mark.gpu
def test_reflector_sizes_marks(Engine):
    """No bin goes to the double sweeps, and no more need a second refinement step than three standard deviations above the NumPy
    model's share on these very inputs allow."""
    rng = np.random.default_rng(61)
    parts = [block_bins(n, rng) for n in ORDERS]
    XB, XD = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    nb = XB.shape[0]
    model = presolve_model()
    C = whitened(XB)
    V, _, trust, _ = model.presolve(C, model.NSTEP_KERNEL, 4, np.random.default_rng(7))
    z = model.zmax(C, V)
    assert trust.all() and (z <= 1e-2).all()
    p = float((z > 3e-5).mean())
    status = refinement_marks(Engine, XB, XD, cn(rng, nb, M), mu=MU)
    second = np.count_nonzero(status == 8)
    bound = binomial_bound(p, nb) * nb
    print(f"second step {second} of {nb}, model share {p:.4f}, bound {bound:.2f}")
    assert np.count_nonzero(status == 16) == 0
    assert second <= bound, (second, p, bound)


@pytest.mark.gpu
def test_bench_marks(Engine):
    """The first 1 024 bench bins, as test_gpu_multisection_steps.py::test_step_marks takes them: the test that catches a broken sum
    or modifier, which would push the share outside the one-step guard far above the model's."""
    import bench
    XB, XD, d = bench.synth(STEP_BINS, 1234)
    status = refinement_marks(Engine, XB, XD, d, mu=1.0)
    p = model_second_step_share(STEP_BINS)
    share = np.count_nonzero(status == 8) / STEP_BINS
    bound = binomial_bound(p, STEP_BINS)
    print(f"second step {share:.4f}, model {p:.4f}, bound {bound:.4f}")
    assert np.count_nonzero(status == 16) == 0
    assert share <= bound, (share, p, bound)


@pytest.mark.gpu
def test_nan_fails_the_gate(Engine):
    """The wave sums that end in a scalar register and the scalar-unit compares still fail the gate for a NaN bin (bin 32 of 64),
    and its neighbours stay bit for bit."""
    check_nan_bin(Engine, K=64, k0=32, ranks=RANKS)
