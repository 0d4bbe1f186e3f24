"""What the tests of the float32 pre-solve of the float64 order-16 kernel share (test_gpu_tridiag_presolve.py,
test_gpu_presolve_chain.py, test_gpu_hermitian_reflectors.py, test_gpu_multisection_steps.py, test_gpu_presolve_wide_step.py):
the error measure, the random constructors, the NumPy model of the kernel's steps, the debug_stop = 9 run and the NaN-bin run.
The constructors draw from the caller's generator in a fixed order: the tests' inputs sit on thresholds of the kernel, and a
changed stream changes what is tested."""
import functools
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

L = 16


def rel_w(w, ref):
    return (np.linalg.norm(w - ref, axis=-1) / np.linalg.norm(ref, axis=-1)).max()


def cn(rng, *s):
    """complex64 noise of unit variance: the real parts are drawn first, then the imaginary parts"""
    return ((rng.standard_normal(s) + 1j * rng.standard_normal(s)) * np.sqrt(0.5)).astype(np.complex64)


def unitary(rng, n=L, real=False):
    """Q of the QR factorisation of an n x n Gaussian matrix (real parts drawn first, then the imaginary parts unless `real`)"""
    g = rng.standard_normal((n, n))
    if not real:
        g = g + 1j * rng.standard_normal((n, n))
    return np.linalg.qr(g)[0]


def with_spectrum(rng, lam):
    """a Hermitian matrix of order 16 with the eigenvalues `lam` and random eigenvectors"""
    U = unitary(rng)
    C = (U * lam) @ U.conj().T
    return 0.5 * (C + C.conj().T)


@functools.lru_cache(maxsize=None)
def presolve_model():
    """tools/probes/tridiag_presolve_model.py: the NumPy model with the kernel's steps and counts"""
    spec = importlib.util.spec_from_file_location("tridiag_presolve_model", os.path.join(ROOT, "tools", "probes", "tridiag_presolve_model.py"))
    model = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(model)
    return model


@functools.lru_cache(maxsize=None)
def model_second_step_share(step_bins):
    """share of the first step_bins bench-distribution bins outside the one-step guard |Z| <= 3e-5 in the NumPy model (wide step,
    NQUAD_KERNEL quad steps, best of four, 1-ulp noise on the pivots' reciprocals)"""
    model = presolve_model()
    C = model.make_C(step_bins)                                          # bench.synth(step_bins, 1234), whitened in float64
    V, _, trust, _ = model.presolve(C, model.NSTEP_KERNEL, 4, np.random.default_rng(7))
    z = model.zmax(C, V)
    assert trust.all() and (z <= 1e-2).all()
    return float((z > 3e-5).mean())


def refinement_marks(Engine, XB, XD, d, mu):
    """Status words of a debug_stop = 9 run, which marks a bin by the last refinement step whose guard it missed: 8 if it missed
    the first step's guard only, 16 if it missed the second step's too."""
    K, M, L_ = XB.shape
    eng = Engine(K, L_, M, ranks=(1,), mu=mu, compute_dtype="f64", out_c128=True, debug_stop=9)
    _, _, status = eng.update(XB, XD, d, raise_on_status=False)
    eng.close()
    print("status words:", dict(zip(*np.unique(status, return_counts=True))))
    assert set(np.unique(status)) <= {0, 8, 16}
    return status


def binomial_bound(p, n):
    """p plus three standard deviations of the share of a binomial count over n draws"""
    return p + 3 * np.sqrt(p * (1 - p) / n)


def check_nan_bin(Engine, K, k0, ranks):
    """A NaN in bin k0 of K bench-distribution bins (through its X_B) gives that bin a non-zero status and leaves its neighbours'
    results bit for bit as they are without it."""
    import bench
    XB, XD, d = bench.synth(K, 77)
    M = XB.shape[1]
    eng = Engine(K, L, M, ranks=ranks, mu=1.0, compute_dtype="f64", out_c128=True)
    w0, lam0, st0 = eng.update(XB, XD, d, raise_on_status=False)
    XB = XB.copy()
    XB[k0, 3, 5] = np.nan
    w1, lam1, st1 = eng.update(XB, XD, d, raise_on_status=False)
    eng.close()
    print("status of the NaN bin:", st1[k0])
    assert not st0.any()
    assert st1[k0] != 0
    others = np.arange(K) != k0
    assert not st1[others].any()
    assert np.array_equal(w1[others], w0[others]) and np.array_equal(lam1[others], lam0[others])
