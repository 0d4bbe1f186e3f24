#!/usr/bin/env python3
"""NumPy model of the float64 order-16 kernel's first refinement step (kernels_gevd16m.hip, stage 3), old and new, batched over
bins.  V is the float32 pre-solve's result: float32-valued, exact to `noise`.

  old   T = C V, Gram = V^H V, S = V^H T and V Z, all four in float64:
        Z_ij = (S_ij - d_j E_ij) / (d_j - d_i), Z_ii = (1 - Gram_ii) / 2, d_j = S_jj / Gram_jj, V'' = V + V Z.
  new   T = C V in float64; d_j = (v_j^H t_j) / (v_j^H v_j) and g_j = v_j^H v_j by column dot products in float64; the residual
        Rs = T - V diag(d) element by element in float64, scaled by the bin's 2^sexp and rounded to float32; P = V^H Rs as a
        float32 product with float32 accumulation; Z_ij = P_ij / (d_j - d_i), Z_ii = (1 - g_i) / 2 in float64; V Z with Z
        rounded to float32, a float32 product again; V'' = V + V Z added in float64.
  Both take the eigenvalues d_j + sum_i |Z_ij|^2 (d_j - d_i).

The float32 products are modelled as the matrix cores run them: every product a_ik b_kj exact (float32 x float32 in float64),
the sum over k rounded to float32 after every term (a chain of float32 FMAs).

    python tools/probes/mixed_refine_model.py [K]           the table of DESIGN 4.1: noise 2e-7, 2e-6, 4e-6 on K bench bins
    python tools/probes/mixed_refine_model.py gap G [K]     built pairs with one gap G ||C|| (tests/test_gpu_mixed_refinement.py):
                                                            max |Z| after the modelled pre-solve (tridiag_presolve_model.py)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tridiag_presolve_model as tp  # noqa: E402

N = 16
f32 = np.float32


def cmm32(A, B):
    """complex product of float32-valued A, B [K,16,16] with float32 accumulation: four real products per k, each sum a chain of
    float32 FMAs (the product exact, the sum rounded)"""
    Ar, Ai = A.real.astype(np.float64), A.imag.astype(np.float64)
    Br, Bi = B.real.astype(np.float64), B.imag.astype(np.float64)
    K = A.shape[0]
    re = np.zeros((K, N, N), f32)
    im = np.zeros((K, N, N), f32)
    for k in range(N):
        ar, ai = Ar[:, :, k, None], Ai[:, :, k, None]
        br, bi = Br[:, None, k, :], Bi[:, None, k, :]
        re = (re.astype(np.float64) + ar * br).astype(f32)
        re = (re.astype(np.float64) - ai * bi).astype(f32)
        im = (im.astype(np.float64) + ar * bi).astype(f32)
        im = (im.astype(np.float64) + ai * br).astype(f32)
    return re.astype(np.float64) + 1j * im.astype(np.float64)


def finish(V, Z, d):
    """V'' and the eigenvalues from Z (its diagonal included) and the Rayleigh quotients"""
    den = d[:, None, :] - d[:, :, None]
    Zo = Z.copy()
    np.einsum("kii->ki", Zo)[:] = 0
    lam = d + (np.abs(Zo) ** 2 * den).sum(1)
    return lam, np.abs(Zo).max((1, 2))


def old_step(C, V):
    V = V.astype(np.complex128)
    Vh = V.conj().transpose(0, 2, 1)
    T = C @ V
    G = Vh @ V
    S = Vh @ T
    d = np.einsum("kii->ki", S).real / np.einsum("kii->ki", G).real
    den = d[:, None, :] - d[:, :, None]
    np.einsum("kii->ki", den)[:] = 1
    Z = (S - d[:, None, :] * G) / den
    np.einsum("kii->ki", Z)[:] = 0.5 * (1 - np.einsum("kii->ki", G).real)
    lam, zmax = finish(V, Z, d)
    return V + V @ Z, lam, zmax


def new_step(C, V, use_residual=True, scale=True):
    """`use_residual` False: P = V^H T (no cancellation in float64: what the tests' first break-it build does);
    `scale` False: no 2^sexp in front of the float32 conversion (the second one)"""
    V32 = V.astype(np.complex64)
    V = V.astype(np.complex128)
    T = C @ V
    g = (np.abs(V) ** 2).sum(1)
    d = (V.conj() * T).sum(1).real / g
    Rs = T - V * d[:, None, :] if use_residual else T
    nf2 = (np.abs(C) ** 2).sum((1, 2))
    sexp = -((np.frexp(nf2)[1] - 1) // 2) if scale else np.zeros(len(C), int)
    scl = np.ldexp(1.0, sexp)[:, None, None]
    with np.errstate(over="ignore"):
        Rs32 = (Rs * scl).astype(np.complex64)
    P = cmm32(V32.conj().transpose(0, 2, 1), Rs32)
    den = d[:, None, :] - d[:, :, None]
    np.einsum("kii->ki", den)[:] = 1
    Z = P / (den * scl)
    np.einsum("kii->ki", Z)[:] = 0.5 * (1 - g)
    lam, zmax = finish(V, Z, d)
    VZ = cmm32(V32, Z.astype(np.complex64))
    return V + VZ, lam, zmax


def noisy_eigenvectors(C, noise, rng):
    """exact eigenvectors plus complex Gaussian noise of that size per element, rounded to float32"""
    _, U = np.linalg.eigh(C)
    E = rng.standard_normal(U.shape) + 1j * rng.standard_normal(U.shape)
    return (U + noise * E).astype(np.complex64)


def quality(C, V2):
    nrm = np.sqrt((np.abs(C) ** 2).sum((1, 2)))
    Vh = V2.conj().transpose(0, 2, 1)
    S = Vh @ C @ V2
    np.einsum("kii->ki", S)[:] = 0
    G = Vh @ V2 - np.eye(N)
    return (np.sqrt((np.abs(S) ** 2).sum((1, 2))) / nrm).max(), np.abs(G).max()


def table(K):
    C = tp.make_C(K)
    nrm = np.sqrt((np.abs(C) ** 2).sum((1, 2)))
    print(f"{K} bench bins; float32 products with float32 accumulation")
    print("noise    max|Z|    new V'' vs old   lam diff / ||C||   offdiag old / new      orth old / new")
    for noise in (2e-7, 2e-6, 4e-6):
        V = noisy_eigenvectors(C, noise, np.random.default_rng(5))
        Vo, lo, zo = old_step(C, V)
        Vn, ln, zn = new_step(C, V)
        ok = zo <= 3e-5                                                  # the bins the kernel's guard lets take the step
        dv = np.abs(Vn - Vo)[ok].max()
        dl = (np.abs(ln - lo) / nrm[:, None])[ok].max()
        qo, qn = quality(C[ok], Vo[ok]), quality(C[ok], Vn[ok])
        print(f"{noise:.0e}   {zo[ok].max():.2e}   {dv:.2e}         {dl:.1e}            {qo[0]:.2e} / {qn[0]:.2e}    {qo[1]:.2e} / {qn[1]:.2e}"
              f"    ({ok.mean() * 100:.2f} % inside the guard; max |Z| new {zn[ok].max():.2e})")


def gap_spectrum(gap, j=7):
    """the graded spectrum of tests/test_gpu_f64_stage_trim.py (1 ... 0.05) with eigenvalue j + 1 gap ||C||_F below eigenvalue j"""
    lam = np.geomspace(1.0, 0.05, N)
    for _ in range(3):
        lam[j + 1] = lam[j] - gap * np.linalg.norm(lam)
    return lam


def gap_bins(gap, K, seed=4205):
    """K Hermitian matrices with that spectrum and random eigenvectors (tests/presolve_cases.py with_spectrum, same draws)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(K):
        g = rng.standard_normal((N, N))
        g = g + 1j * rng.standard_normal((N, N))
        U = np.linalg.qr(g)[0]
        Cm = (U * gap_spectrum(gap)) @ U.conj().T
        out.append(0.5 * (Cm + Cm.conj().T))
    return np.array(out)


def gap_report(gap, K):
    C = gap_bins(gap, K)
    V, _, trust, _ = tp.presolve(C, tp.NSTEP_KERNEL, 4, np.random.default_rng(7))
    z = tp.zmax(C, V)
    print(f"gap {gap:g} ||C||, {K} bins: trusted {trust.mean() * 100:.1f} %, max |Z| min / median / max = {z.min():.2e} / {np.median(z):.2e} / {z.max():.2e}")
    Vo, lo, _ = old_step(C, V)
    Vn, ln, zn = new_step(C, V)
    print(f"  new V'' vs old {np.abs(Vn - Vo).max():.2e}, eigenvalues {np.abs(ln - lo).max():.1e}, max |Z| of the new step {zn.max():.2e}")
    for name, kw in (("P = V^H T", dict(use_residual=False)), ("no 2^sexp, C x 2^-160", dict(scale=False))):
        Cb = C * 2.0 ** -160 if "sexp" in name else C
        Vb, _, _ = new_step(Cb, V, **kw)
        print(f"  break-it model, {name}: V'' vs old {np.abs(Vb - Vo).max():.2e}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "gap":
        gap_report(float(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 64)
    else:
        table(int(sys.argv[1]) if len(sys.argv) > 1 else 32768)
