"""The float32 pre-solve of the float64 order-16 kernel after its chains were shortened (Householder reflectors formed from the
quad that holds row k and moved by lane permutes, multisection with two Sturm counts per lane): every bench bin against the
oracle, the refinement guard's pass rates, and spectra with close, clustered, repeated or already diagonal structure.
Run on the MI355X box with `-m gpu`."""
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


@pytest.fixture(scope="module")
def Engine():
    from ap_vast_unofficial_amd import Engine
    return Engine


@pytest.fixture(scope="module")
def bench_bins():
    import bench
    return bench.synth(32768, 1234)


def test_all_bench_bins_against_oracle(Engine, bench_bins):
    """Every one of the 32 768 headline bins succeeds and matches the oracle to the float64 tolerances."""
    XB, XD, d = bench_bins
    K, M, L = XB.shape
    ranks = (1, 8, 16)
    eng = Engine(K, L, M, ranks=ranks, mu=1.0, compute_dtype="f64", out_c128=True)
    w, lam, status = eng.update(XB, XD, d, raise_on_status=False)
    eng.close()
    assert not status.any(), np.unique(status, return_counts=True)
    w_ref, lam_ref, _ = subband.update(XB, XD, d, 1.0, list(ranks))
    assert (np.abs(lam - lam_ref) / lam_ref[:, :1]).max() < 1e-9
    assert rel_w(w, w_ref) < 1e-7


def test_guard_pass_rates(Engine, bench_bins):
    """debug_stop = 9 marks a bin by the last refinement step whose guard it missed: at least 99.6 % of the bench bins pass the
    one-step guard (the NumPy model of the kernel's steps gives 99.68 %) and every bin passes the second step's limit."""
    XB, XD, d = bench_bins
    K = XB.shape[0]
    status = refinement_marks(Engine, XB, XD, d, mu=1.0)
    assert np.count_nonzero(status == 0) / K >= 0.996, np.count_nonzero(status) / K
    assert np.count_nonzero(status == 16) == 0


def pencil(rng, lam, K, M):
    """K bins whose whitened C has the spectrum `lam` (orthonormal X_D columns: R_D = I)"""
    L = len(lam)
    XB = np.zeros((K, M, L), np.complex128)
    XD = np.zeros((K, M, L), np.complex128)
    for k in range(K):
        XB[k, :L] = np.sqrt(lam)[:, None] * unitary(rng, L).conj().T
        XD[k] = np.linalg.qr(rng.standard_normal((M, L)) + 1j * rng.standard_normal((M, L)))[0]
    return XB.astype(np.complex64), XD.astype(np.complex64)


@pytest.mark.parametrize("spectrum", ["pairs_1e-4", "pairs_1e-6", "cluster", "double", "triple", "diagonal"])
def test_structured_spectra(Engine, spectrum):
    """Pairs 1e-4 apart (above the 1e-5 ||C|| gate: kept on the pre-solve's path), pairs 1e-6 apart, a cluster of six within
    1e-7, exact doubles and triples, and a C that is diagonal already (every reflector the identity: nothing to annihilate)."""
    rng = np.random.default_rng(41)
    K, L, M = 32, 16, 32
    base = np.geomspace(1.0, 0.05, L)
    lam = {"pairs_1e-4": np.repeat(base[::2], 2) * (1 + 1e-4 * np.tile([0, 1], L // 2)),
           "pairs_1e-6": np.repeat(base[::2], 2) * (1 + 1e-6 * np.tile([0, 1], L // 2)),
           "cluster": np.r_[base[:10], 0.3 * (1 + 1e-7 * np.arange(6))],
           "double": np.repeat(base[::2], 2),
           "triple": np.r_[np.repeat(base[:5:1], 3), 0.02],
           "diagonal": base}[spectrum]
    if spectrum == "diagonal":
        XB = np.zeros((K, M, L), np.complex64)
        XB[:, :L] = np.diag(np.sqrt(lam)).astype(np.complex64)
        XD = np.zeros((K, M, L), np.complex64)
        XD[:, :L] = np.eye(L, dtype=np.complex64)
    else:
        XB, XD = pencil(rng, lam, K, M)
    d = cn(rng, K, M)
    ranks = (1, 16)
    eng = Engine(K, L, M, ranks=ranks, mu=0.1, compute_dtype="f64", out_c128=True)
    w, lam_gpu, status = eng.update(XB, XD, d)
    eng.close()
    w_ref, lam_ref, _ = subband.update(XB, XD, d, 0.1, list(ranks))
    assert not status.any()
    assert (np.abs(lam_gpu - lam_ref) / lam_ref[:, :1]).max() < 1e-12
    # the full-rank filter is a function of the whole pencil, defined however a repeated eigenvalue's vectors are chosen
    assert rel_w(w[:, 1:], w_ref[:, 1:]) < 1e-7
    if spectrum in ("pairs_1e-4", "diagonal"):
        assert rel_w(w[:, :1], w_ref[:, :1]) < 1e-7
