"""The float32 tridiagonal pre-solve of the float64 order-16 kernel (Householder, multisection, inverse iteration) on the
bench workload and on spectra with close pairs and clusters.  Run on the MI355X box with `-m gpu`."""
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


def test_bench_bins_against_oracle(Engine, bench_bins):
    """All 32 768 bins of the headline workload succeed; a sample of them matches the oracle to the float64 tolerances."""
    XB, XD, d = bench_bins
    K, M, L = XB.shape
    ranks = (1, 8, 16)
    eng = Engine(K, L, M, ranks=ranks, mu=1.0, compute_dtype="f64", out_c128=True)
    w, lam, status = eng.update(XB, XD, d, raise_on_status=False)
    eng.close()
    assert not status.any(), np.unique(status, return_counts=True)
    sel = np.random.default_rng(5).choice(K, 2048, replace=False)
    w_ref, lam_ref, _ = subband.update(XB[sel], XD[sel], d[sel], 1.0, list(ranks))
    assert (np.abs(lam[sel] - lam_ref) / lam_ref[:, :1]).max() < 1e-9
    assert rel_w(w[sel], w_ref) < 1e-7


def test_second_refinement_step_is_rare(Engine, bench_bins):
    """debug_stop = 9 marks a bin by the last refinement step whose guard it missed (8: the first only, 16: the second): at most
    1 % of the bench bins need the second step, and none is left to the double sweeps by the second guard."""
    XB, XD, d = bench_bins
    K = XB.shape[0]
    status = refinement_marks(Engine, XB, XD, d, mu=1.0)
    second = np.count_nonzero(status) / K
    assert second <= 0.01, second
    assert np.count_nonzero(status == 16) <= K * 1e-3


@pytest.mark.parametrize("spectrum", ["close_pairs", "cluster", "double"])
def test_close_eigenvalues(Engine, spectrum):
    """Pairs of eigenvalues 1e-6 apart, a cluster of six within 1e-7, and exact doubles: inverse iteration cannot separate
    them in float32, and the refinement's guard must send such bins on (second step or double sweeps) with correct results."""
    rng = np.random.default_rng(23)
    K, L, M = 32, 16, 32
    base = np.geomspace(1.0, 0.05, L)
    lam = {"close_pairs": np.repeat(base[::2], 2) * (1 + 1e-6 * np.tile([0, 1], L // 2)),
           "cluster": np.r_[base[:10], 0.3 * (1 + 1e-7 * np.arange(6))],
           "double": np.repeat(base[::2], 2)}[spectrum]
    XB = np.zeros((K, M, L), np.complex128)
    for k in range(K):
        XB[k, :L] = np.sqrt(lam)[:, None] * unitary(rng, L).conj().T
    XD = np.zeros((K, M, L), np.complex128)
    for k in range(K):
        XD[k] = np.linalg.qr(rng.standard_normal((M, L)) + 1j * rng.standard_normal((M, L)))[0]
    XB, XD = XB.astype(np.complex64), XD.astype(np.complex64)
    d = cn(rng, K, M)
    ranks = (1, 16)
    eng = Engine(K, L, M, ranks=ranks, mu=0.1, compute_dtype="f64", out_c128=True)
    w, lam_gpu, status = eng.update(XB, XD, d)
    eng.close()
    w_ref, lam_ref, _ = subband.update(XB, XD, d, 0.1, list(ranks))
    assert not status.any()
    assert (np.abs(lam_gpu - lam_ref) / lam_ref[:, :1]).max() < 1e-12
    # the full-rank filter is a function of the whole pencil, defined however the cluster's vectors are chosen
    assert rel_w(w[:, 1:], w_ref[:, 1:]) < 1e-7
