"""The correlation stage R_B = X_B^H X_B, R_D = X_D^H X_D, r = X_B^H d at every chunk edge of the control-point axis M, in every
piece of device code that forms it: the stand-alone kernels of csrc/kernels_corr.hip (Engine.corr, Engine.corr_bf16) and stage 0
of the fused update kernels (Engine.update).

Part 1 is exact.  The slabs hold Gaussian integers with parts in -3..3 (exact in bf16); a product term is at most 18 in either part
and a sum over M <= 80 rows stays below 130 * 18 < 2^24, so float32, float64 and bf16-input accumulation give the integer result in
any order of summation, with or without FMA: the device must equal the complex128 oracle bit for bit, and R must equal R^H bit for
bit.  Row M - 1 and column L - 1 hold no zero, so a dropped last row or column cannot hide.

Part 2 holds the same kernels to the suite's rounding bounds on Gaussian slabs, at one ragged M per (kernel, L).

Part 4 reaches the fused stage 0.  The dark slab is sqrt(M) times an orthonormal M x L factor, so cond(R_D + reg I) = 1 to float32
rounding and the bounds speak about the kernel, not about the whitening.  Eigenvalues are compared on the scale of the bin's largest,
max_i |lam_i - ref_i| / ref_1 (the measure of test_gpu_order128._check_update and the first assertion of
test_gpu_parity.test_update_vs_oracle), in both arithmetics.  Statistics and solves of finite precision carry an absolute error of
eps ||R||, which moves every eigenvalue by that much whatever its own size, and the table below has M = L on purpose: with X_B a
Gaussian M x L slab the smallest eigenvalue is then 1e-4 .. 1e-6 of the largest, and the ratio lam_i / ref_i of the tail measures
cond(R_B), not stage 0 (the last column below: up to 10.7 TOL from rounding R to complex64 alone).  A dropped, doubled or
mis-masked row moves the LARGEST eigenvalues by about 1 / M >= 7e-3.

Float32 rows of the table, measured on the CPU before any device run (_f32_statistics_distances): the oracle as it is against the
oracle whose R_B, R_D and r were rounded to complex64 before the solve, in the measures of the test and as fractions of TOL["f32"]
(lam 1e-5, w 1e-4).  Every row is below one fifth, the largest being 0.0018 (lam) and 0.0076 (w); no M or seed had to be moved.

    kernel reached   L    M   lam / TOL   w / TOL   (max |lam_i / ref_i - 1| / TOL, not asserted)
    correlate16     16   16    0.0012     0.0008    10.729
    correlate16     16   31    0.0010     0.0015     0.011
    correlate16     16   33    0.0013     0.0072     0.006
    correlate16     16   63    0.0008     0.0014     0.003
    correlate16     16   64    0.0014     0.0076     0.003
    correlate16     16   65    0.0018     0.0024     0.004
    correlate16     16  100    0.0008     0.0013     0.002
    gevd64          64   64    0.0005     0.0017     5.921
    gevd64          64   65    0.0006     0.0006     2.414
    gevd64          64   79    0.0005     0.0009     0.055
    gevd64          64   80    0.0006     0.0009     0.054
    gevd64          64   81    0.0006     0.0039     0.057
    gevd64          64   97    0.0003     0.0009     0.013
    lds             10   17    0.0014     0.0009     0.016
    lds             24   33    0.0006     0.0006     0.019
    lds             32   33    0.0007     0.0008     0.183
    split32         32   32    0.0007     0.0041     2.940
    split32         32   34    0.0006     0.0007     0.271
    split32         32   36    0.0007     0.0005     0.057
    split32         32   38    0.0008     0.0007     0.060
    split64 (rel)   64   66    0.0005     0.0006     0.771
    split64 (rel)   64   70    0.0005     0.0035     0.122
    lds64_odd (rel) 64   65    0.0006     0.0006     2.414

On the device the float32 rows of order 64 that end in the float LDS kernel (split64, lds64_odd) come out at 7.4e-6 .. 9.5e-6 on the
eigenvalues and at 1.1e-5 .. 8.6e-5 (M = 70) on the filters, the same figures in every run: that is the float32 Jacobi iteration of
that kernel at order 64 (test_gpu_parity records 7.4e-6 for it at 64 x 128), not stage 0, whose own share is the table's.  Every
other float32 row is at most 4.4e-6 and 1.8e-5.  The bounds stay TOL.
"""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

from oracle import gevd, subband  # noqa: E402  (checker only)
from test_gpu_parity import TOL, bf16_round, cn, w_err  # noqa: E402


def _engine(*a, **kw):
    from ap_vast_unofficial_amd import Engine
    return Engine(*a, **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. exact
# ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _integer_case(K, M, L):
    """Slabs of Gaussian integers and their correlation by the complex128 oracle (shared by every handle type; read-only)."""
    rng = np.random.default_rng(100000 * K + 1000 * L + M)

    def draw(*s):
        return (rng.integers(-3, 4, s) + 1j * rng.integers(-3, 4, s)).astype(np.complex64)
    XB, XD, d = draw(K, M, L), draw(K, M, L), draw(K, M)
    for X in (XB, XD):
        X[:, M - 1, :][X[:, M - 1, :] == 0] = 3 + 3j
        X[:, :, L - 1][X[:, :, L - 1] == 0] = 3 + 3j
    d[:, M - 1][d[:, M - 1] == 0] = 3 + 3j
    assert (XB[:, M - 1] != 0).all() and (XB[:, :, L - 1] != 0).all() and (XD[:, M - 1] != 0).all() and (XD[:, :, L - 1] != 0).all()
    assert np.array_equal(bf16_round(XB), XB) and np.array_equal(bf16_round(XD), XD) and np.array_equal(bf16_round(d), d)
    ref = subband.correlate(XB, XD, d)
    for e in ref:
        assert np.array_equal(e.real, np.rint(e.real)) and np.array_equal(e.imag, np.rint(e.imag))
        assert max(np.abs(e.real).max(), np.abs(e.imag).max()) < 2 ** 24
    for a in (XB, XD, d) + ref:
        a.setflags(write=False)
    return XB, XD, d, ref


def _check_exact(got, ref, dtype):
    for g, e, name in zip(got, ref, ("R_B", "R_D", "r")):
        assert g.dtype == dtype and g.shape == e.shape, name
        bad = np.argwhere(g != e)
        assert np.array_equal(g, e), (name, len(bad), bad[:4].tolist())
    for R, name in zip(got[:2], ("R_B", "R_D")):
        assert np.array_equal(R, R.conj().transpose(0, 2, 1)), name + " is not Hermitian bit for bit"


def _exact(L, M, compute_dtype, K=3, bf16=False):
    XB, XD, d, ref = _integer_case(K, M, L)
    eng = _engine(K, L, M, compute_dtype=compute_dtype)
    try:
        got = eng.corr_bf16(XB, XD, d) if bf16 else eng.corr(XB, XD, d)
    finally:
        eng.close()
    _check_exact(got, ref, np.complex128 if compute_dtype == "f64" and not bf16 else np.complex64)


F64_MFMA = ([(16, M) for M in (1, 4, 31, 32, 33, 65)] + [(32, M) for M in (3, 33)] + [(48, M) for M in (5, 40, 64)] +
            [(64, M) for M in (1, 30, 72)])
F64_VALU = [(L, M) for L in (1, 5, 17, 33, 63) for M in (1, 7, 8, 9, 20)]
F32_MFMA = [(L, M) for L in (32, 64) for M in (8, 10, 12, 14, 16, 34, 66)]       # M / 2 = 4, 5, 6, 7, 8, 17, 33: remainders 0..3
F32_VALU = ([(L, M) for L in (32, 64) for M in (1, 6, 7, 9, 33)] +              # odd M or M < 8: not for the f32 MFMA kernel
            [(L, M) for L in (1, 5, 16, 17, 48, 63) for M in (1, 9, 24)])
BF16 = [(L, M) for L in (32, 64) for M in (16, 32, 48, 80)]


@pytest.mark.parametrize("L,M", F64_MFMA)
def test_exact_f64_mfma(L, M):
    """corr_mfma_f64_kernel<L / 16>: 32 rows per step, rows past M masked to zero; L = 48 is the nine-wave workgroup."""
    _exact(L, M, "f64")


@pytest.mark.parametrize("L,M", F64_VALU)
def test_exact_f64_valu(L, M):
    """corr_kernel<double>: 8 rows per step, L neither a power of two nor a multiple of 16 (idx / L indexing, NACC guard)."""
    _exact(L, M, "f64")


@pytest.mark.parametrize("L,M", F32_MFMA)
def test_exact_f32_mfma(L, M):
    """corr_mfma_f32_kernel<L / 32>: groups of four prefetched row pairs, then the scalar remainder loop of 0..3 pairs."""
    _exact(L, M, "f32")


@pytest.mark.parametrize("L,M", F32_VALU)
def test_exact_f32_valu(L, M):
    """corr_kernel<float>: every order, and orders 32 and 64 with M odd or below 8 (the launcher's fall-back condition)."""
    _exact(L, M, "f32")


@pytest.mark.parametrize("L,M", BF16)
def test_exact_bf16(L, M):
    """to_bf16_kernel + corr_mfma_bf16_kernel<L / 32>: 16 rows per step, one to five steps."""
    _exact(L, M, "f32", bf16=True)


def test_exact_f32_mfma_many_bins():
    """257 bins at 64 x 34: size_t bin offsets, more workgroups than two per compute unit, a ragged bin count."""
    _exact(64, 34, "f32", K=257)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. rounding: one ragged M per (kernel, L)
# ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gaussian_case(K, M, L):
    rng = np.random.default_rng(7000 + 100 * L + M)
    XB, XD, d = cn(rng, K, M, L), cn(rng, K, M, L), cn(rng, K, M)
    ref = subband.correlate(XB, XD, d)
    for a in (XB, XD, d) + ref:
        a.setflags(write=False)
    return XB, XD, d, ref


ROUNDING_F64 = [(16, 33), (32, 33), (48, 40), (64, 30)] + [(L, 9) for L in (1, 5, 17, 33, 63)]
ROUNDING_F32 = [(32, 34), (64, 34), (32, 33), (64, 33)] + [(L, 9) for L in (1, 5, 16, 17, 48, 63)]


@pytest.mark.parametrize("dtype,L,M", [("f64", L, M) for L, M in ROUNDING_F64] + [("f32", L, M) for L, M in ROUNDING_F32])
def test_rounding(dtype, L, M):
    """Gaussian slabs: 1e-12 (float64) and 3e-6 (float32) of the largest entry, the bounds of test_gpu_parity's stage tests."""
    K = 3
    XB, XD, d, ref = _gaussian_case(K, M, L)
    eng = _engine(K, L, M, compute_dtype=dtype)
    try:
        got = eng.corr(XB, XD, d)
    finally:
        eng.close()
    tol = 1e-12 if dtype == "f64" else 3e-6
    for a, b, name in zip(got, ref, ("R_B", "R_D", "r")):
        err = np.abs(a - b).max() / np.abs(b).max()
        print(f"{dtype} L={L} M={M} {name}: {err:.2e}")
        assert err <= tol, name


@pytest.mark.parametrize("L,M", [(32, 48), (64, 80)])
def test_rounding_bf16(L, M):
    """Gaussian slabs through the bf16 kernel against the oracle on bf16-rounded inputs: float32 accumulation is all that is left,
    2e-6 relative Frobenius norm per bin (the bound of test_corr_bf16_exact_on_rounded_inputs)."""
    K = 3
    XB, XD, d, _ = _gaussian_case(K, M, L)
    ref = subband.correlate(bf16_round(XB), bf16_round(XD), bf16_round(d))
    eng = _engine(K, L, M, compute_dtype="f32")
    try:
        got = eng.corr_bf16(XB, XD, d)
    finally:
        eng.close()
    for a, b, name in zip(got, ref, ("R_B", "R_D", "r")):
        rel = np.linalg.norm((a - b).reshape(K, -1), axis=1) / np.linalg.norm(b.reshape(K, -1), axis=1)
        print(f"bf16 L={L} M={M} {name}: {rel.max():.2e}")
        assert rel.max() < 2e-6, name


# ---------------------------------------------------------------------------------------------------------------------------
# 3. argument checks
# ---------------------------------------------------------------------------------------------------------------------------

def test_argument_checks():
    from ap_vast_unofficial_amd import _capi
    rng = np.random.default_rng(3)
    for L, M in ((16, 32), (32, 24)):            # order without a bf16 kernel; M no multiple of 16
        eng = _engine(2, L, M, compute_dtype="f32")
        with pytest.raises(_capi.ApvError) as ei:
            eng.corr_bf16(cn(rng, 2, M, L), cn(rng, 2, M, L), cn(rng, 2, M))
        eng.close()
        assert ei.value.code == _capi.ERR_ARG
    # a handle may have up to 128 loudspeakers; the stand-alone correlation serves 64
    eng = _engine(2, 65, 70)
    with pytest.raises(_capi.ApvError, match="1..64") as ei:
        eng.corr(cn(rng, 2, 70, 65), cn(rng, 2, 70, 65), cn(rng, 2, 70))
    eng.close()
    assert ei.value.code == _capi.ERR_ARG
    for dtype, ctype in (("f64", np.complex128), ("f32", np.complex64)):
        eng = _engine(0, 16, 32, compute_dtype=dtype)
        RB, RD, r = eng.corr(np.zeros((0, 32, 16), np.complex64), np.zeros((0, 32, 16), np.complex64), np.zeros((0, 32), np.complex64))
        eng.close()
        assert RB.shape == RD.shape == (0, 16, 16) and r.shape == (0, 16)
        assert RB.dtype == RD.dtype == r.dtype == ctype


# ---------------------------------------------------------------------------------------------------------------------------
# 4. fused stage 0 of the update kernels
# ---------------------------------------------------------------------------------------------------------------------------

MU, REG = 0.7, 1e-7
K_UPDATE = 3

# (kernel reached, handle, L, M, relative loading)
UPDATE_CASES = (
    [("correlate16", dt, 16, M, False) for dt in ("f64", "f32") for M in (16, 31, 33, 63, 64, 65, 100)] +
    [("gevd64", dt, 64, M, False) for dt in ("f64", "f32") for M in (64, 65, 79, 80, 81, 97)] +
    [("lds", "f64", L, M, False) for L, M in ((10, 15), (10, 16), (10, 17), (10, 33), (24, 33), (40, 49))] +
    [("lds", "f32", L, M, False) for L, M in ((10, 17), (24, 33), (32, 33))] +       # (32, 33): odd M must not take the split path
    [("split32", "f32", 32, M, False) for M in (32, 34, 36, 38)] +
    [("split64", "f32", 64, M, True) for M in (66, 70)] + [("lds64_odd", "f32", 64, 65, True)])
ORDER128_CASES = [(96, M) for M in (96, 97, 111, 113)]


@functools.lru_cache(maxsize=None)
def _update_case(L, M, rel):
    """Gaussian X_B and d, X_D = sqrt(M) Q with Q the orthonormal factor of a Gaussian M x L matrix; the oracle's statistics and
    solve.  Shared by the float64 and float32 handles of a shape; read-only."""
    K = K_UPDATE
    rng = np.random.default_rng(40000 + 100 * L + M)
    XB, d = cn(rng, K, M, L), cn(rng, K, M)
    G = rng.standard_normal((K, M, L)) + 1j * rng.standard_normal((K, M, L))
    XD = (np.sqrt(M) * np.linalg.qr(G)[0]).astype(np.complex64)
    RB, RD, r = subband.correlate(XB, XD, d)
    for a in (XB, XD, d, RB, RD, r):
        a.setflags(write=False)
    load = REG * (np.linalg.norm(RD, ord=2, axis=(1, 2)) if rel else np.ones(K))
    cond = max(np.linalg.cond(RD[k] + load[k] * np.eye(L)) for k in range(K))
    return XB, XD, d, (RB, RD, r), cond


def _ranks(dtype, L):
    return (1, L) if dtype == "f32" else (1, L // 2, L)          # rank L has no truncation gap


@functools.lru_cache(maxsize=None)
def _update_ref(L, M, rel, ranks):
    RB, RD, r = _update_case(L, M, rel)[3]
    w, lam, st = subband.gevd_vast(RB, RD, r, MU, list(ranks), reg_mode=gevd.REG_MODE_REL if rel else gevd.REG_MODE_ABS, reg=REG)
    assert not st.any()
    w.setflags(write=False)
    lam.setflags(write=False)
    return w, lam


def _lam_err(lam, lam_ref):
    return (np.abs(lam - lam_ref).max(axis=1) / lam_ref[:, 0]).max()


@pytest.mark.parametrize("kernel,dtype,L,M,rel", UPDATE_CASES)
def test_update_stage0(kernel, dtype, L, M, rel):
    """Engine.update against oracle.subband.update at TOL of test_gpu_parity; for float64 handles also against the same handle's
    gevd_vast on the ORACLE's statistics: the same eigen-kernel from the device's stage 0 and from the oracle's."""
    from ap_vast_unofficial_amd import _capi
    XB, XD, d, stats, cond = _update_case(L, M, rel)
    assert cond < 10, cond
    ranks = _ranks(dtype, L)
    w_ref, lam_ref = _update_ref(L, M, rel, ranks)
    tol = TOL[dtype]
    eng = _engine(K_UPDATE, L, M, ranks=ranks, mu=MU, compute_dtype=dtype, reg_dark=REG,
                  reg_mode=_capi.REG_REL if rel else _capi.REG_ABS)
    try:
        w, lam, status = eng.update(XB, XD, d)
        if dtype == "f64":
            w2, lam2, status2 = eng.gevd_vast(*stats)
    finally:
        eng.close()
    assert not status.any()
    e_lam, e_w = _lam_err(lam, lam_ref), w_err(w, w_ref)
    print(f"{kernel} {dtype} L={L} M={M}: lam {e_lam:.2e} w {e_w:.2e}")
    assert e_lam < tol["lam"]
    assert e_w < tol["w"]
    if dtype == "f64":
        e_rel = np.abs(lam / lam_ref - 1).max()
        e_lam2, e_rel2, e_w2 = _lam_err(lam, lam2), np.abs(lam / lam2 - 1).max(), w_err(w, w2)
        print(f"    lam / lam_ref - 1: {e_rel:.2e}; against gevd_vast: lam {e_lam2:.2e} ({e_rel2:.2e}) w {e_w2:.2e}")
        assert not status2.any()
        assert e_lam2 < tol["lam"]
        assert e_w2 < tol["w"]


@pytest.mark.parametrize("L,M", ORDER128_CASES)
def test_update_stage0_order128(L, M):
    """corr128 stage of kernels_gevd128.hip (16 rows per step), float64, with the measures and the bounds of
    test_gpu_order128._check_update for M >= L (1e-9 of the largest eigenvalue, 1e-7 on the filters)."""
    XB, XD, d, stats, cond = _update_case(L, M, False)
    assert cond < 10, cond
    ranks = _ranks("f64", L)
    w_ref, lam_ref = _update_ref(L, M, False, ranks)
    eng = _engine(K_UPDATE, L, M, ranks=ranks, mu=MU, compute_dtype="f64", reg_dark=REG)
    try:
        w, lam, status = eng.update(XB, XD, d)
    finally:
        eng.close()
    assert (status == 0).all()
    e_lam, e_w = _lam_err(lam, lam_ref), w_err(w, w_ref)
    print(f"order128 L={L} M={M}: lam {e_lam:.2e} w {e_w:.2e}")
    assert e_lam <= 1e-9 and e_w <= 1e-7


def _f32_statistics_distances():
    """The CPU measurement of the module docstring: per float32 row, the oracle against the oracle on complex64 statistics."""
    rows = []
    for kernel, dtype, L, M, rel in UPDATE_CASES:
        if dtype != "f32":
            continue
        ranks = _ranks(dtype, L)
        RB, RD, r = _update_case(L, M, rel)[3]
        w_ref, lam_ref = _update_ref(L, M, rel, ranks)
        c64 = [a.astype(np.complex64).astype(np.complex128) for a in (RB, RD, r)]
        w, lam, st = subband.gevd_vast(*c64, MU, list(ranks), reg_mode=gevd.REG_MODE_REL if rel else gevd.REG_MODE_ABS, reg=REG)
        rows.append((kernel, L, M, _lam_err(lam, lam_ref) / TOL["f32"]["lam"], w_err(w, w_ref) / TOL["f32"]["w"],
                     np.abs(lam / lam_ref - 1).max() / TOL["f32"]["lam"]))
    return rows


if __name__ == "__main__":
    for kernel, L, M, fl, fw, frel in _f32_statistics_distances():
        print(f"  {kernel:12s} L={L:3d} M={M:3d}  lam {fl:.4f}  w {fw:.4f}   (lam / lam_ref - 1: {frel:.3f})")
