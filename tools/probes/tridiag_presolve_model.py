#!/usr/bin/env python3
"""NumPy model of the float32 TRIDIAGONAL pre-solve of the float64 order-16 kernel (kernels_gevd16m.hip, stage 3), batched
over bins and in the kernel's order of operations:

  1. Householder reduction of 2^sexp C to a Hermitian tridiagonal Q^H C Q in float32 by 15 Hermitian reflectors
     H = I - gamma u u^H with a real gamma (u the raw column, u_0 = alpha + alpha/|alpha| ||x||), Q accumulated as
     Q H_0 H_1 ... H_14; the sub-diagonal comes out complex, only its modulus goes on, and the phases delta_0 = 1,
     delta_{k+1} = -delta_k alpha_k/|alpha_k| scale Q's columns at the end: T = (Q diag delta)^H C (Q diag delta) is real.
     The last reflector, H_14 = diag(1, ..., 1, -1), is taken as the sign it is: column 15 of Q and delta_15 keep theirs.
     ||x|| = n^2 rsq(n^2) carries a random error of up to 1 ulp, as the bare v_rsq_f32 does (ULP_NOISE=0: correctly
     rounded); 1/|alpha| and gamma take a Newton step in the kernel.  With bare instructions for all three the share of
     bins inside the one-step guard falls from 99.70 % to 99.53 %;
  2. eigenvalues by Sturm-count multisection, q_i = (a_i - x) - e_{i-1}^2 rcp(q_{i-1}), NSTEP Sturm evaluations per lane:
     a WIDE first step (all sixteen quads search the same interval, so the 64 lanes count at lo + (l + 1) (hi - lo) / 65 and
     eigenvalue m takes the 65th that holds it: nb_m = number of lanes whose count is <= m), then NSTEP - 1 quad steps of
     NPTS points per eigenvalue (the interval shrinks NPTS + 1 times; the kernel runs 4 points, four lanes with one count
     each).  The kernel runs NSTEP_KERNEL evaluations (the refinement that follows certifies the result: DESIGN 4.1 has the
     pass rates).  SCHEME without "wide" runs NSTEP quad steps, the scheme before the wide step;
  3. eigenvectors by two inverse-iteration steps on T - lam I, unpivoted L D L^T (the Sturm recurrence at the shift), start
     vector ones + e_m, normalised after each step.  BEST OF FOUR: lane jq of the quad takes the shift
     lo + (1/8 + jq/4) (hi - lo) of the final interval, and the lane whose second step grew the normalised vector most
     (the largest squared norm before the last normalisation, compared as an integer with 3 - jq in its two lowest bits: a
     tie goes to the lowest jq) delivers the vector and the quad's eigenvalue.  SCHEME without "best4" takes the midpoint;
     two neighbouring eigenvalues whose MEASURED gap is not above apart_threshold(NSTEP) ||C|| send the bin to the double
     sweeps in the kernel (none on the bench data): 1e-5 widened by twice the multisection's own error, so that every pair
     whose true gap is under 1e-5 ||C|| goes there.  `trust` below carries this gate and the spread gate;
  4. V32 = Q X.

It prints the share of bins whose refinement matrix Z_ij = (S_ij - d_j E_ij) / (d_j - d_i), taken in float64 against the
exact C, meets the kernel's one-step guard |Z| <= 3e-5 and its second-step limit 1e-2, on bench.synth(K, 1234).

    python tools/probes/tridiag_presolve_model.py [K] [NSTEP] [NPTS] [SCHEME]

SCHEME: "wide+best4" (the kernel's), "wide", "best4" or "quad".  The token "lanczos" (as in "wide+best4+lanczos") replaces step 1
by a Lanczos reduction: the three-term recurrence from a fixed generic start vector with one full reorthogonalisation pass per
step (`lanczos` below; T comes out real and the Lanczos vectors are Q, so there is nothing to accumulate and no phases), and a
beta below LANCZOS_BETA_MIN ||C||_F fails the gate.  "+noreorth" drops the pass, "+no3term" the three-term step in front of it and
"+ones" starts from ones / 4: the variants that do not work.  That reduction was built and measured in the kernel and is not what
it runs ("The reduction's crossbar trips through LDS", has why); the scheme stays here for whoever takes it up.  The reciprocals of the L D L^T pivots carry 1-ulp noise too,
as the bare v_rcp_f32 of the kernel does, whenever the reflector scalars do (ULP_NOISE, or `rng` of presolve); RCP_NOISE=0
takes them correctly rounded (the kernel's earlier Newton step).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

f32 = np.float32
N = 16
NWIDE = 64                          # points of the wide first step: one per lane
NQUAD_KERNEL = 6                    # kTpQuadSteps of kernels_gevd16m.hip
NSTEP_KERNEL = 1 + NQUAD_KERNEL     # Sturm evaluations per lane: the wide step and the quad steps
SCHEME_KERNEL = "wide+best4"


def final_interval(nstep, scheme=SCHEME_KERNEL):
    """width of the multisection's last interval in units of ||C||: 1.002 / (65 * 5^(nstep-1)) with the wide step, 1.002 * 5^-nstep without"""
    return 1.002 / (NWIDE + 1) * 5.0 ** -(nstep - 1) if "wide" in scheme else 1.002 * 5.0 ** -nstep


def lam_err(nstep, scheme=SCHEME_KERNEL):
    """kTpLamErr: the distance from an eigenvalue to the nearest shift (an eighth of the final interval with the best of four
    shifts, half of it with the midpoint) plus the float32 floor of the Sturm count, taken as 1e-6 (the largest error where
    the interval no longer matters is 7.2e-7 on the bench bins)."""
    return (0.125 if "best4" in scheme else 0.5) * final_interval(nstep, scheme) + 1e-6


def apart_threshold(nstep, scheme=SCHEME_KERNEL):
    """kTpApart, in units of ||C||"""
    return 1e-5 + 2 * lam_err(nstep, scheme)


def make_C(K, seed=1234, reg=1e-7):
    from bench import synth
    XB, XD, _ = synth(K, seed)
    XB = XB.astype(np.complex128)
    XD = XD.astype(np.complex128)
    RB = XB.conj().transpose(0, 2, 1) @ XB
    RD = XD.conj().transpose(0, 2, 1) @ XD + reg * np.eye(N)
    W = np.linalg.inv(np.linalg.cholesky(RD))
    C = W @ RB @ W.conj().transpose(0, 2, 1)
    return 0.5 * (C + C.conj().transpose(0, 2, 1))


def ulp_noise(x, rng):
    """x with a relative error of up to one float32 ulp: v_rsq_f32 and v_rcp_f32 are good to 1 ulp, not correctly rounded."""
    if rng is None:
        return x.astype(f32)
    return (x * (f32(1) + rng.uniform(-1, 1, x.shape).astype(f32) * f32(2.0 ** -23))).astype(f32)


def tridiag(A, rng=None):
    """A: [K,16,16] complex64, Hermitian.  Returns a (diag), e (modulus of the sub-diagonal), e2 (its square, as the kernel
    takes it: the squared column norm), Q (complex64) and delta (complex64) with diag(delta)^H Q^H A Q diag(delta) = T, real.
    Hermitian reflectors H = I - gamma u u^H, gamma real; `rng`: 1-ulp noise on rsq(n^2)."""
    K = A.shape[0]
    A = A.copy()
    Q = np.broadcast_to(np.eye(N, dtype=np.complex64), A.shape).copy()
    e = np.zeros((K, N - 1), f32)
    e2 = np.zeros((K, N - 1), f32)
    delta = np.ones((K, N), np.complex64)
    for k in range(N - 1):
        # alpha and n^2 from the very column entries u is made of (taken from row k, the conjugate up to the rounding of the
        # updates, H is unitary to 1e-5 only where the column is small, and 99.56 % of the bins pass the one-step guard)
        col = A[:, k + 1:, k]
        alpha = col[:, 0].copy()
        a2 = (alpha.real * alpha.real + alpha.imag * alpha.imag).astype(f32)
        if k == N - 2:
            # the last reflector is a sign, H = diag(1, ..., 1, -1): A[15][15] stays, Q's column 15 and delta_15 both change
            # sign, and the kernel leaves both alone (delta_15 = +delta_14 phi).  No products, no update.
            n2 = np.maximum(a2, f32(1e-31))
            e[:, k] = (n2 * ulp_noise(f32(1) / np.sqrt(n2), rng)).astype(f32)
            e2[:, k] = n2
            ra = (f32(1) / np.sqrt(np.maximum(a2, f32(1e-36)))).astype(f32)
            phi = np.where(a2 > f32(1e-36), (alpha * ra).astype(np.complex64), np.complex64(1))
            delta[:, k + 1] = (delta[:, k] * phi).astype(np.complex64)
            break
        # every one of the sixteen rows adds 1e-31 (the kernel: the addend of an FMA): e2 is never zero
        n2 = (f32(16e-31) + (col.real * col.real + col.imag * col.imag).sum(1, dtype=f32)).astype(f32)
        nrm = (n2 * ulp_noise(f32(1) / np.sqrt(n2), rng)).astype(f32)
        ra = (f32(1) / np.sqrt(np.maximum(a2, f32(1e-36)))).astype(f32)     # a Newton step in the kernel
        pha = a2 > f32(1e-36)
        phi = np.where(pha, (alpha * ra).astype(np.complex64), np.complex64(1))
        den = (n2 + nrm * (a2 * ra).astype(f32)).astype(f32)
        gam = np.where(n2 > f32(4e-30), f32(1) / den, f32(0)).astype(f32)   # a Newton step in the kernel
        u = np.zeros((K, N), np.complex64)
        u[:, k + 1] = (alpha + phi * nrm).astype(np.complex64)
        u[:, k + 2:] = A[:, k + 2:, k]                                   # raw column entries: no scaling
        e[:, k] = nrm
        e2[:, k] = n2
        delta[:, k + 1] = (-delta[:, k] * phi).astype(np.complex64)
        p = np.einsum("kij,kj->ki", A, u).astype(np.complex64)           # A u (gamma applied below)
        uau = np.einsum("ki,ki->k", u.conj(), p).real.astype(f32)
        kap = (f32(-0.5) * gam * gam * uau).astype(f32)
        w = (gam[:, None] * p + kap[:, None] * u).astype(np.complex64)
        A = (A - u[:, :, None] * w.conj()[:, None, :] - w[:, :, None] * u.conj()[:, None, :]).astype(np.complex64)
        tu = (gam[:, None] * np.einsum("kij,kj->ki", Q, u)).astype(np.complex64)
        Q = (Q - tu[:, :, None] * u.conj()[:, None, :]).astype(np.complex64)
    a = np.einsum("kii->ki", A).real.astype(f32)
    return a, e, e2, Q, delta


# The start vector of the Lanczos reduction: sixteen entries of modulus 1/4 whose phases
# 2 pi frac(m^2 phi + m sqrt 2) have no symmetry an array can share (a symmetric array has eigenvectors orthogonal to ones).
_m = np.arange(N, dtype=np.float64)
LANCZOS_START = (0.25 * np.exp(2j * np.pi * ((_m * _m * 0.6180339887498949 + _m * 1.4142135623730951) % 1.0))).astype(np.complex64)
LANCZOS_BETA_MIN = 1e-6             # a beta below this (x ||C||_F) is a breakdown and fails the gate


def lanczos(A, rng=None, start=None, reorth=True, three_term=True):
    """A: [K,16,16] complex64, Hermitian.  Lanczos tridiagonalisation from the fixed start vector, in float32: w = A q_k,
    alpha_k = Re q_k^H w, w -= alpha_k q_k + beta_{k-1} q_{k-1} (the three-term step), then ONE pass against all of q_0 .. q_k
    (c = Q_k^H w, w -= Q_k c), n^2 = ||w||^2 + 16e-31, beta_k = n^2 rsq(n^2) and q_{k+1} = w rsq(n^2), the reciprocal root with
    1-ulp noise (`rng`).  Returns a, e, e2, Q, delta as tridiag does: the Lanczos vectors are Q itself, T is real with a
    positive sub-diagonal and delta is all ones.  `reorth`, `three_term`: the variants that do not work (see main)."""
    K = A.shape[0]
    q0 = LANCZOS_START if start is None else np.asarray(start, np.complex64)
    Q = np.zeros((K, N, N), np.complex64)
    Q[:, :, 0] = q0
    a = np.zeros((K, N), f32)
    e = np.zeros((K, N - 1), f32)
    e2 = np.zeros((K, N - 1), f32)
    for k in range(N):
        qk = Q[:, :, k]
        w = np.einsum("kij,kj->ki", A, qk).astype(np.complex64)
        a[:, k] = (qk.real * w.real + qk.imag * w.imag).sum(1, dtype=f32)
        if k == N - 1:
            break
        if three_term:
            w = (w - a[:, k, None] * qk).astype(np.complex64)
            if k > 0:
                w = (w - e[:, k - 1, None] * Q[:, :, k - 1]).astype(np.complex64)
        if reorth:
            Qk = Q[:, :, :k + 1]
            c = np.einsum("kij,ki->kj", Qk.conj(), w).astype(np.complex64)
            w = (w - np.einsum("kij,kj->ki", Qk, c)).astype(np.complex64)
        n2 = (f32(16e-31) + (w.real * w.real + w.imag * w.imag).sum(1, dtype=f32)).astype(f32)
        r = ulp_noise(f32(1) / np.sqrt(n2), rng)
        e[:, k] = (n2 * r).astype(f32)
        e2[:, k] = n2
        Q[:, :, k + 1] = (w * r[:, None]).astype(np.complex64)
    return a, e, e2, Q, np.ones((K, N), np.complex64)


def sturm_count(a, e2, x):
    """number of eigenvalues below x; a [K,16], e2 [K,15], x [K,...]"""
    q = (a[:, 0, None] - x).astype(f32)
    cnt = np.signbit(q).astype(np.int32)                                # the kernel counts sign bits (one popcount)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in range(1, N):
            r = (f32(1) / q).astype(f32)
            q = ((a[:, i, None] - x) - e2[:, i - 1, None] * r).astype(f32)
            cnt += np.signbit(q)
    return cnt


def multisection(a, e2, nrm, nstep, npts=4, scheme=SCHEME_KERNEL, interval=False):
    """eigenvalue m of every bin after nstep Sturm evaluations: the midpoint of its last interval, or (lo, hi) if `interval`"""
    K = a.shape[0]
    lo = np.broadcast_to((f32(-1e-3) * nrm)[:, None], (K, N)).astype(f32).copy()
    hi = np.broadcast_to((f32(1.001) * nrm)[:, None], (K, N)).astype(f32).copy()
    m = np.arange(N)
    nquad = nstep
    if "wide" in scheme and nstep > 0:
        # all quads hold the same interval: 64 points, one per lane, and nb_m = number of lanes whose count is <= m
        nquad = nstep - 1
        wd = (f32(1.002) * nrm).astype(f32)                                             # hi - lo, as the kernel forms it
        fr = (np.arange(1, NWIDE + 1).astype(f32) * f32(1 / (NWIDE + 1))).astype(f32)
        pts = (lo[:, :1] + wd[:, None] * fr).astype(f32)                                # [K,64]
        c = sturm_count(a, e2, pts)
        nb = (c[:, None, :] <= m[None, :, None]).sum(2)                                 # [K,16]
        wp = (f32(1 / (NWIDE + 1)) * wd).astype(f32)[:, None]
        lo = (lo + nb.astype(f32) * wp).astype(f32)
        hi = (lo + wp).astype(f32)
    for _ in range(nquad):
        fr = (np.arange(1, npts + 1) / (npts + 1)).astype(f32)
        pts = (lo[:, :, None] + (hi - lo)[:, :, None] * fr).astype(f32)                  # [K,16,npts]
        c = sturm_count(a, e2, pts.reshape(K, -1)).reshape(K, N, npts)
        below = c <= m[None, :, None]                                   # eigenvalue m lies above this point
        nb = below.sum(2)                                               # points at or below lam_m (monotone)
        # the kernel's form: the nb-th of the npts + 1 parts of the old interval, its ends re-formed from lo
        wp = (f32(1 / (npts + 1)) * (hi - lo)).astype(f32)
        lo = (lo + nb.astype(f32) * wp).astype(f32)
        hi = (lo + wp).astype(f32)
    if interval:
        return lo, hi
    return ((lo + hi) * f32(0.5)).astype(f32)


def inverse_iteration(a, e, lam, nrm, steps=2, tiny_rel=1e-9, rng=None, growth=False):
    """X [K,16 (row),S*16 (shift)] for lam [K, S*16]: S shifts per eigenvalue, shift c belongs to eigenvalue c // S and starts from
    ones + e_(c // S).  `growth`: also the squared norm of the last step's vector before its normalisation.  `rng`: 1-ulp noise
    on the pivots' reciprocals."""
    K, NS = lam.shape
    S = NS // N
    tiny = (f32(tiny_rel) * nrm)[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = np.empty((K, N, NS), f32)                                   # [K, i, c]
        l = np.empty((K, N - 1, NS), f32)
        rd = np.empty((K, N, NS), f32)
        q = (a[:, 0, None] - lam).astype(f32)
        for i in range(N):
            if i > 0:
                q = ((a[:, i, None] - lam) - e[:, i - 1, None] * l[:, i - 1]).astype(f32)
            q = np.where(np.abs(q) < tiny, np.where(q < 0, -tiny, tiny), q).astype(f32)
            d[:, i] = q
            rd[:, i] = ulp_noise(f32(1) / q, rng)
            if i < N - 1:
                l[:, i] = (e[:, i, None] * rd[:, i]).astype(f32)
        x = (np.ones((N, NS), f32) + (np.arange(N)[:, None] == np.arange(NS)[None, :] // S).astype(f32))[None].repeat(K, 0)
        for _ in range(steps):
            y = x.copy()
            for i in range(1, N):
                y[:, i] = (y[:, i] - l[:, i - 1] * y[:, i - 1]).astype(f32)
            z = (y * rd).astype(f32)
            for i in range(N - 2, -1, -1):
                z[:, i] = (z[:, i] - l[:, i] * z[:, i + 1]).astype(f32)
            s = (z * z).sum(1, dtype=f32).astype(f32)
            x = (z / np.sqrt(s)[:, None, :]).astype(f32)
    return (x, s) if growth else x


def best_of_four(a, e, lo, hi, nrm, rng=None):
    """(X [K,16,16], lam [K,16], winner [K,16]): lane jq of quad m shifts by lo + (1/8 + jq/4) (hi - lo); the lane with the
    largest key wins, key = the bits of the squared norm of the second step with 3 - jq in the two lowest (unsigned: a NaN wins
    and fails the gate)."""
    K = a.shape[0]
    fr = (f32(0.125) + f32(0.25) * np.arange(4).astype(f32)).astype(f32)
    lam4 = (lo[:, :, None] + (hi - lo).astype(f32)[:, :, None] * fr).astype(f32)         # [K,16,4]
    X4, s = inverse_iteration(a, e, lam4.reshape(K, 4 * N), nrm, rng=rng, growth=True)
    key = (s.reshape(K, N, 4).view(np.uint32) & np.uint32(0xFFFFFFFC)) | (np.uint32(3) - np.arange(4).astype(np.uint32))
    win = key.argmax(2)                                                                  # keys are distinct within a quad
    X = np.take_along_axis(X4.reshape(K, N, N, 4), win[:, None, :, None], 3)[..., 0]
    lam = np.take_along_axis(lam4, win[:, :, None], 2)[..., 0]
    return X, lam, win


def presolve(C, nstep, npts=4, rng=None, scheme=SCHEME_KERNEL, rcp_rng="as rng"):
    """`rng`: 1-ulp noise on rsq(n^2) of the reflectors.  `rcp_rng`: 1-ulp noise on the pivots' reciprocals of the L D L^T (the
    kernel's bare v_rcp_f32); by default a generator of its own whenever `rng` is given, None for correctly rounded ones."""
    if isinstance(rcp_rng, str):
        rcp_rng = np.random.default_rng(11) if rng is not None else None
    nf2 = (np.abs(C) ** 2).sum((1, 2))
    sexp = -(np.frexp(nf2)[1] - 1) // 2
    A = (C * np.ldexp(1.0, sexp)[:, None, None]).astype(np.complex64)
    nrm = np.sqrt(np.ldexp(nf2, 2 * sexp)).astype(f32)
    if "lanczos" in scheme:
        a, e, e2, Q, delta = lanczos(A, rng, start=np.full(N, 0.25) if "ones" in scheme else None,
                                     reorth="noreorth" not in scheme, three_term="no3term" not in scheme)
    else:
        a, e, e2, Q, delta = tridiag(A, rng)
    if "best4" in scheme:
        lo, hi = multisection(a, e2, nrm, nstep, npts, scheme, interval=True)
        X, lam, _ = best_of_four(a, e, lo, hi, nrm, rcp_rng)
    else:
        lam = multisection(a, e2, nrm, nstep, npts, scheme)
        X = inverse_iteration(a, e, lam, nrm, rng=rcp_rng)
    Q = (Q * delta[:, None, :]).astype(np.complex64)                    # the phases go back into Q's columns
    V = (Q @ X.astype(np.complex64)).astype(np.complex64)
    # the kernel's gate: spread under 1e3 (smallest and largest are eigenvalue 0 and 15: they come out sorted), every
    # neighbouring pair apart (two eigenvalues that share a final interval may win with the same shift: their gap reads <= 0),
    # nothing NaN
    with np.errstate(invalid="ignore"):
        apart = (np.diff(lam, axis=1) > f32(apart_threshold(nstep, scheme)) * nrm[:, None]).all(1)
        trust = (lam[:, 0] >= f32(1e-3) * lam[:, -1]) & apart & np.isfinite(X).all((1, 2)) & ~np.isnan(lam).any(1)
        if "lanczos" in scheme:                                         # a breakdown of the recurrence fails the gate too
            trust &= (e >= f32(LANCZOS_BETA_MIN) * nrm[:, None]).all(1)
    return V, lam, trust, (a, e, Q, A)


def zmax(C, V):
    V = V.astype(np.complex128)
    S = V.conj().transpose(0, 2, 1) @ C @ V
    G = V.conj().transpose(0, 2, 1) @ V
    E = G - np.eye(N)
    dq = np.einsum("kii->ki", S).real / np.einsum("kii->ki", G).real
    num = S - dq[:, None, :] * E
    den = dq[:, None, :] - dq[:, :, None]
    np.einsum("kii->ki", den)[:] = 1
    Z = np.abs(num / den)
    np.einsum("kii->ki", Z)[:] = 0
    return Z.max((1, 2))


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
    nstep = int(sys.argv[2]) if len(sys.argv) > 2 else NSTEP_KERNEL
    npts = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    scheme = sys.argv[4] if len(sys.argv) > 4 else SCHEME_KERNEL
    C = make_C(K)
    noise = os.environ.get("ULP_NOISE", "1") != "0"
    V, lam, trust, (a, e, Q, A) = presolve(C, nstep, npts, np.random.default_rng(7) if noise else None, scheme,
                                           np.random.default_rng(11) if noise and os.environ.get("RCP_NOISE", "1") != "0" else None)
    if "lanczos" in scheme:
        print(f"lanczos: smallest beta / ||C||_F = {(e / np.sqrt((np.abs(A.astype(np.complex128)) ** 2).sum((1, 2)))[:, None]).min():.2e}")
    # the reduction itself: (Q diag(delta))^H A (Q diag(delta)) tridiagonal and real
    T = Q.conj().transpose(0, 2, 1).astype(np.complex128) @ A.astype(np.complex128) @ Q.astype(np.complex128)
    Tm = np.zeros_like(T)
    idx = np.arange(N)
    Tm[:, idx, idx] = a
    Tm[:, idx[1:], idx[:-1]] = e
    Tm[:, idx[:-1], idx[1:]] = e
    nrm = np.sqrt((np.abs(A.astype(np.complex128)) ** 2).sum((1, 2)))
    print(f"bins {K}, scheme {scheme}: {nstep} Sturm evaluations, {npts} points per eigenvalue per quad step")
    print(f"reduction: max |Q^H A Q - T| / ||A|| = {(np.abs(T - Tm).max((1, 2)) / nrm).max():.2e}, "
          f"max |Q^H Q - I| = {np.abs(Q.conj().transpose(0, 2, 1) @ Q - np.eye(N)).max():.2e}")
    lref = np.linalg.eigvalsh(C)
    sc = nrm / np.sqrt((np.abs(C) ** 2).sum((1, 2)))
    print(f"eigenvalues: max |lam - lam_ref| / ||C|| = {(np.abs(np.sort(lam, 1) / sc[:, None] - lref).max(1) * sc / nrm).max():.2e}")
    z = zmax(C, V)
    t = trust
    gaps = np.diff(lref, axis=1).min(1) / np.sqrt((np.abs(C) ** 2).sum((1, 2)))
    print(f"trusted {t.mean() * 100:.2f} % (spread < 1e3 and measured gaps > {apart_threshold(nstep, scheme):.3g} ||C||; smallest true gap {gaps.min():.2e} ||C||, "
          f"{(gaps < 1e-5).sum()} bins under 1e-5, {(~t & (gaps >= 1e-5)).sum()} untrusted above it)")
    print(f"|Z| <= 3e-5: {(z[t] <= 3e-5).mean() * 100:.2f} % of trusted bins, <= 1e-2: {(z[t] <= 1e-2).mean() * 100:.3f} %")
    print(f"max |Z| median / p99 / max: {np.median(z[t]):.2e} / {np.quantile(z[t], 0.99):.2e} / {z[t].max():.2e}")


if __name__ == "__main__":
    main()
