"""The Hermitian reflectors of the float32 pre-solve (H = I - gamma u u^H with a real gamma, the phases of the complex sub-diagonal
put back into Q's columns) on the inputs that exercise their special values: a whitened C with an exactly zero sub-column at
reflector 0, 7 and 14 (gamma = 0), a purely real C (every phase +-1) and a C whose first sub-column is purely imaginary.  Each
against the oracle at the bounds test_gpu_presolve_chain.py uses for its structured spectra.  Run on the MI355X box with `-m gpu`."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

from oracle import subband  # noqa: E402  (checker only)
from presolve_cases import cn, refinement_marks, rel_w, unitary  # noqa: E402

K, L, M = 32, 16, 32
CASES = ["zero_column_0", "zero_column_7", "zero_column_14", "real", "imaginary_first_column"]


@pytest.fixture(scope="module")
def Engine():
    from ap_vast_unofficial_amd import Engine
    return Engine


def bins(case, rng):
    """K bins with the spectrum geomspace(1, 0.05, 16), built as pencil() of test_gpu_presolve_chain.py builds its spectra
    (X_B = sqrt(lam) U^H on the first L rows) but with X_D the leading identity, so that R_D is exactly I, the whitening is an
    exact scaling and the zeros (or the zero real / imaginary parts) of R_B = X_B^H X_B are those of the whitened C, bit for bit."""
    lam = np.geomspace(1.0, 0.05, L)
    XB = np.zeros((K, M, L), np.complex128)
    XD = np.zeros((K, M, L), np.complex128)
    XD[:, :L] = np.eye(L)
    for k in range(K):
        if case.startswith("zero_column_"):
            # block diagonal C, blocks of n and L - n: the reflectors before n stay inside the first block, and the column
            # below the sub-diagonal that reflector n - 1 meets is exactly zero
            n = int(case.rsplit("_", 1)[1]) + 1
            perm = rng.permutation(L)
            for sl, idx in ((slice(0, n), perm[:n]), (slice(n, L), perm[n:])):
                U = unitary(rng, len(idx))
                XB[k, sl, sl] = np.sqrt(lam[idx])[:, None] * U.conj().T
        elif case == "real":
            XB[k, :L] = np.sqrt(lam)[:, None] * unitary(rng, L, real=True).T
        else:
            # C = D C_real D^H with D = diag(-i, 1, ..., 1): C[j][0] = i C_real[j][0] for j > 0
            XB[k, :L] = np.sqrt(lam)[:, None] * unitary(rng, L, real=True).T
            XB[k, :L, 0] *= 1j
    return XB.astype(np.complex64), XD.astype(np.complex64)


def whitened(XB):
    XB = XB.astype(np.complex128)
    return XB.conj().transpose(0, 2, 1) @ XB


def test_inputs_have_the_structure():
    """The structure is exact in the complex64 inputs themselves (runs without a GPU too: it only inspects the inputs)."""
    rng = np.random.default_rng(43)
    for case in CASES:
        XB, XD = bins(case, rng)
        assert np.array_equal(XD[:, :L], np.broadcast_to(np.eye(L, dtype=np.complex64), (K, L, L))) and not XD[:, L:].any()
        C = whitened(XB)
        if case.startswith("zero_column_"):
            n = int(case.rsplit("_", 1)[1]) + 1
            assert not C[:, n:, :n].any() and not C[:, :n, n:].any()
        elif case == "real":
            assert not C.imag.any() and np.abs(C.real).min() > 0
        else:
            assert not C[:, 1:, 0].real.any() and np.abs(C[:, 1:, 0].imag).min() > 0


@pytest.mark.parametrize("case", CASES)
def test_special_columns_against_oracle(Engine, case):
    rng = np.random.default_rng(43)
    XB, XD = bins(case, rng)
    d = cn(rng, K, M)
    ranks = (1, 16)
    eng = Engine(K, L, M, ranks=ranks, mu=0.1, compute_dtype="f64", out_c128=True)
    w, lam_gpu, status = eng.update(XB, XD, d)
    eng.close()
    w_ref, lam_ref, _ = subband.update(XB, XD, d, 0.1, list(ranks))
    lam_err = (np.abs(lam_gpu - lam_ref) / lam_ref[:, :1]).max()
    w16_err, w1_err = rel_w(w[:, 1:], w_ref[:, 1:]), rel_w(w[:, :1], w_ref[:, :1])
    print(f"{case}: lam {lam_err:.2e}  w(rank 16) {w16_err:.2e}  w(rank 1) {w1_err:.2e}")
    assert not status.any()
    assert lam_err < 1e-12
    assert w16_err < 1e-7
    assert w1_err < 1e-7            # the spectrum is simple: the leading eigenvector is defined


def test_special_columns_stay_on_the_refinement(Engine):
    """debug_stop = 9 marks a bin by the last refinement step whose guard it missed: none of these bins misses the second
    step's limit (status 16), i.e. the pre-solve's eigenvectors are fit for the refinement."""
    rng = np.random.default_rng(43)
    parts = [bins(case, rng) for case in CASES]
    XB, XD = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    d = cn(rng, XB.shape[0], M)
    status = refinement_marks(Engine, XB, XD, d, mu=0.1)
    assert np.count_nonzero(status == 16) == 0
