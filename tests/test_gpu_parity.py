"""GPU parity: the HIP path (through the C ABI) against the CPU oracle and the golden
fixtures captured from the reference.  Run on the MI355X box with `-m gpu`."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

from oracle import gevd, subband  # noqa: E402  (checker only)

# tolerances of SURVEY.md section 8(c)
TOL = {"f64": dict(lam=1e-9, w=1e-7), "f32": dict(lam=1e-5, w=1e-4)}


def cn(rng, *s):
    return ((rng.standard_normal(s) + 1j * rng.standard_normal(s)) * np.sqrt(0.5)).astype(np.complex64)


def w_err(w, ref):
    return (np.linalg.norm(w - ref, axis=-1) / np.linalg.norm(ref, axis=-1)).max()


@pytest.fixture(scope="module")
def Engine():
    from ap_vast_unofficial_amd import Engine
    return Engine


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["g3_jdiag_c_16x32", "g3_jdiag_c_8x8", "g3_jdiag_c_64x128"])
def test_update_vs_reference_golden(Engine, golden, name, dtype):
    """Fused update == reference jdiag (apvast.py:20-36) + filter (406-414) on fixture G3."""
    g = golden(name)
    XB, XD, d = g["XB"], g["XD"], g["d"]
    K, M, L = XB.shape
    ranks = [int(v) for v in g["ranks"]]
    eng = Engine(K, L, M, ranks=ranks, mu=float(g["mu"]), compute_dtype=dtype, reg_dark=float(g["reg"]))
    w, lam, status = eng.update(XB, XD, d)
    eng.close()
    assert not status.any()
    if dtype == "f64":
        assert np.abs(lam / g["lam"] - 1).max() < TOL[dtype]["lam"]
        assert w_err(w, g["w"]) < TOL[dtype]["w"]
    else:
        # fp32 arithmetic: the perturbation bound of a whitened eigenproblem solved in float32, per bin:
        # |d lam| / lam_max <= 4 eps32 cond(R_D + reg I), ||d w|| / ||w|| <= 16 eps32 cond (floor 1e-6: the c64 outputs).  Measured
        # (tools/probes/f32_error_vs_cond.py): 0.6 and 2.9 eps32 cond at 16 x 32 (cond 31), 0.3 and 1.3 at 8 x 8 (cond 5e3).
        RD = subband.correlate(XB, XD, d)[1] + float(g["reg"]) * np.eye(L)
        bound = np.finfo(np.float32).eps * np.linalg.cond(RD)                      # per bin
        e_lam = (np.abs(lam - g["lam"]) / g["lam"][:, :1]).max(axis=1)
        e_w = (np.linalg.norm(w - g["w"], axis=-1) / np.linalg.norm(g["w"], axis=-1)).max(axis=1)
        assert (e_lam <= np.maximum(4 * bound, 1e-6)).all(), (e_lam / bound).max()
        assert (e_w <= np.maximum(16 * bound, 1e-6)).all(), (e_w / bound).max()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("K,L,M,ranks", [
    (37, 16, 32, (1, 8, 16)),       # cfg2 shape, ragged bin count
    (5, 10, 24, (1, 5, 10)),        # main.m:42 uses 10 loudspeakers
    (9, 5, 7, (2, 5)),              # odd order: the Jacobi tournament gets a bye
    (3, 32, 48, (1, 16, 32)),
    (2, 64, 128, (1, 32, 64)),      # cfg5 shape
    (4, 1, 3, (1,)),                # degenerate single loudspeaker
    (3, 16, 8, (1, 4, 8)),          # M < L: bright matrix rank deficient
])
def test_update_vs_oracle(Engine, K, L, M, ranks, dtype):
    rng = np.random.default_rng(1000 + K + L)
    XB, XD, d = cn(rng, K, M, L), cn(rng, K, M, L), cn(rng, K, M)
    reg = 1e-7 if M >= L else 1e-2      # dark matrix is singular when M < L: load it visibly
    eng = Engine(K, L, M, ranks=ranks, mu=0.7, compute_dtype=dtype, reg_dark=reg)
    w, lam, status = eng.update(XB, XD, d)
    eng.close()
    w_ref, lam_ref, _ = subband.update(XB, XD, d, 0.7, list(ranks), reg=reg)
    assert not status.any()
    nz = min(L, M)                       # beyond rank(R_B) the eigenvalues are rounding noise
    scale = lam_ref[:, :1]
    # The plain SURVEY 8(c) bounds (lambda 1e-9 / 1e-5, w 1e-7 / 1e-4) hold in every case but one.  Measured on the device
    # (tools/probes/parity_margins.py, profiles/r04/parity_margins.md): float64 lambda <= 5.0e-11 relative (order 64; <= 7.5e-14
    # below it), w <= 4.8e-8 (order 64; 1.0e-10 at 16 x 32); float32 lambda <= 7.4e-6, w <= 4.3e-6.  The exception is float32 with
    # M < L: the dark matrix is singular and loaded to cond ~ 3e3, and the float32 whitening of it leaves 7.1e-5 on the
    # eigenvalues and 0.8-1.8e-3 on the filters (tools/probes/rankdef_f32_probe.py; the two-sided sweeps the probe could select
    # before that switch was removed gave the same; float64: 8e-14 and 6e-12, inside the plain bounds).
    loose = dtype == "f32" and M < L
    assert (np.abs(lam[:, :nz] - lam_ref[:, :nz]) / scale).max() < TOL[dtype]["lam"] * (10 if loose else 1)
    if M >= L:
        assert np.abs(lam / lam_ref - 1).max() < TOL[dtype]["lam"]
    good = [t for t, V in enumerate(ranks) if V <= nz]
    assert w_err(w[:, good], w_ref[:, good]) < TOL[dtype]["w"] * (30 if loose else 1)


def test_empty_shard(Engine):
    eng = Engine(0, 16, 32)
    w, lam, status = eng.update(np.zeros((0, 32, 16), np.complex64), np.zeros((0, 32, 16), np.complex64),
                                np.zeros((0, 32), np.complex64))
    eng.close()
    assert w.shape == (0, 1, 16) and lam.shape == (0, 16) and status.shape == (0,)


def test_not_positive_definite_raises(Engine):
    """apvast.py:21/24: cholesky of a non-PD dark matrix raises LinAlgError."""
    rng = np.random.default_rng(3)
    K, L, M = 4, 8, 16
    XB, XD, d = cn(rng, K, M, L), cn(rng, K, M, L), cn(rng, K, M)
    XD[2] = 0                                   # R_D[2] = 0, and a negative load makes it indefinite
    eng = Engine(K, L, M, ranks=(1,), reg_dark=-1e-3)
    with pytest.raises(np.linalg.LinAlgError):
        eng.update(XB, XD, d)
    w, lam, status = eng.update(XB, XD, d, raise_on_status=False)
    eng.close()
    assert list(status) == [1, 1, 1, 1] or status[2] == 1


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_corr_stage(Engine, dtype):
    rng = np.random.default_rng(8)
    K, L, M = 11, 16, 32
    XB, XD, d = cn(rng, K, M, L), cn(rng, K, M, L), cn(rng, K, M)
    eng = Engine(K, L, M, compute_dtype=dtype)
    RB, RD, r = eng.corr(XB, XD, d)
    eng.close()
    RB0, RD0, r0 = subband.correlate(XB, XD, d)
    tol = 1e-12 if dtype == "f64" else 2e-6
    for a, b in ((RB, RB0), (RD, RD0), (r, r0)):
        assert np.abs(a - b).max() <= tol * np.abs(b).max()


def test_gevd_stage_from_explicit_matrices(Engine):
    rng = np.random.default_rng(9)
    K, L, M = 6, 16, 32
    XB, XD, d = cn(rng, K, M, L), cn(rng, K, M, L), cn(rng, K, M)
    RB, RD, r = subband.correlate(XB, XD, d)
    eng = Engine(K, L, M, ranks=(1, 16), mu=1.0)
    w, lam, status = eng.gevd_vast(RB, RD, r)
    eng.close()
    w_ref, lam_ref, _ = subband.gevd_vast(RB, RD, r, 1.0, [1, 16])
    assert np.abs(lam / lam_ref - 1).max() < 1e-9
    assert w_err(w, w_ref) < 1e-7


@pytest.mark.parametrize("n", [3, 12, 16, 40, 64])
def test_jdiag_batched_invariants(Engine, n):
    """KA-3: U^H (B+reg) U = I, U^H A U = diag(lam), lam descending; lam == oracle jdiag."""
    rng = np.random.default_rng(n)
    batch = 5
    Y = rng.standard_normal((batch, 2 * n, n)) + 1j * rng.standard_normal((batch, 2 * n, n))
    Z = rng.standard_normal((batch, 2 * n, n)) + 1j * rng.standard_normal((batch, 2 * n, n))
    A = np.einsum("kmi,kmj->kij", Y.conj(), Y)
    B = np.einsum("kmi,kmj->kij", Z.conj(), Z)
    eng = Engine(1, 4, 4)
    U, lam = eng.jdiag_batched(A, B)
    eng.close()
    for k in range(batch):
        Bl = B[k] + 1e-7 * np.eye(n)
        G = U[k].conj().T @ Bl @ U[k]
        D = U[k].conj().T @ A[k] @ U[k]
        assert np.abs(G - np.eye(n)).max() < 1e-11
        assert np.abs(D - np.diag(lam[k])).max() < 1e-10 * lam[k, 0]
        assert (np.diff(lam[k]) <= 0).all()
        _, lam_ref = gevd.jdiag(A[k], B[k])
        assert np.abs(lam[k] / lam_ref - 1).max() < 1e-9


def test_jdiag_real_golden(Engine, golden):
    """G2: real symmetric pairs from the reference's own jdiag."""
    g = golden("g2_jdiag_real")
    eng = Engine(1, 4, 4)
    U, lam = eng.jdiag_batched(g["A"], g["B"])
    eng.close()
    assert np.abs(lam / g["lam"] - 1).max() < 1e-9
    P = np.einsum("kic,kjc->kij", U[:, :, :3], U[:, :, :3].conj())
    assert np.abs(P.imag).max() < 1e-9
    assert np.abs(P.real - g["proj3"]).max() < 1e-8 * np.abs(g["proj3"]).max()


def test_relative_loading(Engine):
    """apvast.py:26-27 (EXPERIMENTAL_REGULARIZATION=False): B + 1e-8 ||B||_2 I."""
    rng = np.random.default_rng(21)
    K, L, M = 4, 16, 32
    XB, XD, d = cn(rng, K, M, L), cn(rng, K, M, L), cn(rng, K, M)
    from ap_vast_unofficial_amd import _capi
    eng = Engine(K, L, M, ranks=(4, 16), reg_mode=_capi.REG_REL, reg_dark=5e-3)   # MATLAB dark loading
    w, lam, status = eng.update(XB, XD, d)
    eng.close()
    w_ref, lam_ref, _ = subband.update(XB, XD, d, 1.0, [4, 16], reg_mode=gevd.REG_MODE_REL, reg=5e-3)
    # ||B||_2 by Lanczos + Sturm multisection, good to 1e-16 of the interval: the plain float64 bounds hold
    assert np.abs(lam / lam_ref - 1).max() < 1e-9
    assert w_err(w, w_ref) < 1e-7


@pytest.mark.parametrize("N,H", [(256, 128), (2048, 1024), (64, 16), (512, 128),
                                 (1600, 800),       # make_python_test.m:6 (blockSize = 2 * rirLength)
                                 (210, 70), (96, 32), (8192, 4096)])
def test_stft_roundtrip_vs_oracle(Engine, N, H):
    """Analysis (apvast.py:246-255) and synthesis+OLA (265-293) against numpy.fft in float64."""
    rng = np.random.default_rng(N)
    n_ch = 19
    x = rng.standard_normal((n_ch, N)).astype(np.float32)
    eng = Engine(1, 4, 4, block_size=N, hop_size=H)
    spec = eng.stft_analysis(x)
    win = subband.sine_window(N)
    ref = subband.analysis(x.T.astype(np.float64), win).T
    assert np.abs(spec - ref).max() < 2e-6 * np.abs(ref).max()
    ov = rng.standard_normal((n_ch, N)).astype(np.float32)
    spec_in = (ref * (1.0 + 0.1j)).astype(np.complex64)      # imag at DC/Nyquist must be ignored like irfft
    ov_new, out = eng.istft_ola(spec_in, ov)
    eng.close()
    ov_ref = subband.synthesis_ola(spec_in.T.astype(np.complex128), win, ov.T.astype(np.float64), H).T
    assert np.abs(ov_new - ov_ref).max() < 3e-6 * np.abs(ov_ref).max()
    assert np.abs(out - ov_ref[:, :H]).max() < 3e-6 * np.abs(ov_ref).max()


def test_rccl_allgather_single_rank(Engine):
    """The C-ABI communicator path (ncclCommInitRank + ncclAllGather) with world = 1."""
    rng = np.random.default_rng(5)
    K, L, M = 32, 16, 32
    XB, XD, d = cn(rng, K, M, L), cn(rng, K, M, L), cn(rng, K, M)
    eng = Engine(K, L, M, ranks=(8,), out_c128=False)
    eng.comm_init(Engine.comm_unique_id(), 0, 1)
    dXB, dXD, dd = eng.to_device(XB), eng.to_device(XD), eng.to_device(d)
    dw, dall = eng.alloc(K * L * 8), eng.alloc(K * L * 8)
    eng.update_dev(dXB, dXD, dd, dw)
    eng.allgather_filters_dev(dw, dall)
    eng.sync()
    w, wall = dw.download((K, 1, L), np.complex64), dall.download((K, 1, L), np.complex64)
    eng.close()
    assert np.array_equal(w, wall)
    w_ref, _, _ = subband.update(XB, XD, d, 1.0, [8])
    assert w_err(w, w_ref) < 3e-7


def _triu_to_full(t, n):
    R = np.zeros((n, n))
    R[np.triu_indices(n)] = t
    return R + np.triu(R, 1).T


def test_jdiag_large_broadband_golden(Engine, golden):
    """G1/G2: the reference's own broadband pair (R_A_to_A, R_A_to_B) of cfg1, n = J L = 256
    (apvast.py:380): eigenvalues, invariants and the rank-accumulated filter (apvast.py:406-414)."""
    import time
    g = golden("g1_broadband_cfg1")
    n = 256
    A, B = _triu_to_full(g["R_AA_triu"], n), _triu_to_full(g["R_AB_triu"], n)
    eng = Engine(1, 4, 4)
    t0 = time.perf_counter()
    U, lam = eng.jdiag_large(A[None], B[None])
    dt = time.perf_counter() - t0
    eng.close()
    U, lam = U[0], lam[0]
    lam_ref = g["lam"][-1, 0]
    V = 8
    assert np.abs(lam[:V] / lam_ref[:V] - 1).max() < 1e-9
    assert np.abs(lam - lam_ref).max() < 1e-9 * lam_ref[0]
    G = U.T @ (B + 1e-7 * np.eye(n)) @ U
    assert np.abs(G - np.eye(n)).max() < 1e-9
    D = U.T @ A @ U
    assert np.abs(D - np.diag(lam)).max() < 1e-9 * lam[0]
    r = g["r"][-1, 0]
    coef = (U.T @ r) / (lam + 1.0)
    for i in range(V):
        w = U[:, : i + 1] @ coef[: i + 1]
        e = g["w"][-1, 0, i]
        assert np.linalg.norm(w - e) <= 1e-7 * np.linalg.norm(e), i
    print(f"jdiag_large n=256: {dt * 1e3:.1f} ms")


@pytest.mark.parametrize("n,batch", [(65, 1), (100, 2), (257, 1), (800, 1), (2048, 1)])      # 2048: the largest order the entry point takes
def test_jdiag_large_vs_oracle(Engine, n, batch):
    rng = np.random.default_rng(n)
    Y = rng.standard_normal((batch, 3 * n, n))
    Z = rng.standard_normal((batch, 3 * n, n))
    A = np.einsum("kmi,kmj->kij", Y, Y)
    B = np.einsum("kmi,kmj->kij", Z, Z)
    eng = Engine(1, 4, 4)
    U, lam = eng.jdiag_large(A, B)
    eng.close()
    for k in range(batch):
        _, lam_ref = gevd.jdiag(A[k], B[k])
        assert np.abs(lam[k] / lam_ref - 1).max() < 1e-9
        G = U[k].T @ (B[k] + 1e-7 * np.eye(n)) @ U[k]
        assert np.abs(G - np.eye(n)).max() < 1e-10
    with pytest.raises(np.linalg.LinAlgError):
        eng2 = Engine(1, 4, 4)
        eng2.jdiag_large(np.eye(70)[None], -np.eye(70)[None])


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", [1, 17, 32, 33, 64])      # one pair of blocks (n <= 32: no look-ahead), then two (the smallest look-ahead)
def test_jdiag_large_small_orders_vs_oracle(Engine, n, batch):
    rng = np.random.default_rng(n)
    Y = rng.standard_normal((batch, 3 * n, n))
    Z = rng.standard_normal((batch, 3 * n, n))
    A = np.einsum("kmi,kmj->kij", Y, Y)
    B = np.einsum("kmi,kmj->kij", Z, Z)
    eng = Engine(1, 4, 4)
    U, lam = eng.jdiag_large(A, B)
    eng.close()
    for k in range(batch):
        _, lam_ref = gevd.jdiag(A[k], B[k])
        assert np.abs(lam[k] / lam_ref - 1).max() < 1e-9
        G = U[k].T @ (B[k] + 1e-7 * np.eye(n)) @ U[k]
        assert np.abs(G - np.eye(n)).max() < 1e-10


def _g8_pair(g):
    XB, XD, d = (g[k].astype(np.complex128) for k in ("XB", "XD", "d"))
    return XB.conj().T @ XB, XD.conj().T @ XD, XB.conj().T @ d


@pytest.mark.parametrize("tag", ["abs", "rel"])
def test_jdiag_complex_beyond_64_golden(golden, tag):
    """G8: `jdiag` on a complex Hermitian pair of order 96 against the reference's own (apvast.py:20-36 takes any order), both
    loading branches: eigenvalues 1e-9, the filters of apvast.py:406-414 built from U 1e-7, jdiag's contract on U."""
    from ap_vast_unofficial_amd import apvast as host
    g = golden("g8_jdiag_c_96")
    A, B, r = _g8_pair(g)
    n = A.shape[0]
    keep = host.EXPERIMENTAL_REGULARIZATION
    host.EXPERIMENTAL_REGULARIZATION = (tag == "abs")
    try:
        U, D = host.jdiag(A, B)
    finally:
        host.EXPERIMENTAL_REGULARIZATION = keep
    lam = np.diag(D)
    assert U.dtype == np.complex128 and D.shape == (n, n)
    assert np.abs(lam / g["lam_" + tag] - 1).max() < 1e-9
    load = 1e-7 if tag == "abs" else 1e-8 * np.linalg.norm(B, 2)
    assert np.abs(U.conj().T @ (B + load * np.eye(n)) @ U - np.eye(n)).max() < 1e-10
    assert np.abs(U.conj().T @ A @ U - D).max() < 1e-9 * lam[0]
    coef = (U.conj().T @ r) / (lam + float(g["mu"]))
    for t, V in enumerate(g["ranks"]):
        w = U[:, :V] @ coef[:V]
        assert np.linalg.norm(w - g["w_" + tag][t]) < 1e-7 * np.linalg.norm(g["w_" + tag][t])


@pytest.mark.parametrize("n,batch", [(65, 2), (200, 1), (512, 1), (1024, 1)])       # 1024: the largest (its embedding is of order 2048)
def test_jdiag_large_complex_vs_oracle(Engine, n, batch):
    rng = np.random.default_rng(n)
    Y = rng.standard_normal((batch, 2 * n, n)) + 1j * rng.standard_normal((batch, 2 * n, n))
    Z = rng.standard_normal((batch, 2 * n, n)) + 1j * rng.standard_normal((batch, 2 * n, n))
    A = np.einsum("kmi,kmj->kij", Y.conj(), Y)
    B = np.einsum("kmi,kmj->kij", Z.conj(), Z)
    eng = Engine(1, 4, 4)
    U, lam = eng.jdiag_large_complex(A, B)
    eng.close()
    for k in range(batch):
        _, lam_ref = gevd.jdiag(A[k], B[k])
        assert np.abs(lam[k] / lam_ref - 1).max() < 1e-9
        G = U[k].conj().T @ (B[k] + 1e-7 * np.eye(n)) @ U[k]
        assert np.abs(G - np.eye(n)).max() < 1e-10
        D = U[k].conj().T @ A[k] @ U[k]
        assert np.abs(D - np.diag(lam[k])).max() < 1e-9 * lam[k, 0]
    with pytest.raises(np.linalg.LinAlgError):
        eng2 = Engine(1, 4, 4)
        eng2.jdiag_large_complex(np.eye(70, dtype=complex)[None], -np.eye(70, dtype=complex)[None])


def test_jdiag_large_complex_relative_loading_batch(Engine):
    """Complex pairs of order 70 in a batch of three with the relative loading of apvast.py:26-27 (the spectral norm of the
    embedding is the norm of the complex matrix)."""
    from ap_vast_unofficial_amd import _capi
    rng = np.random.default_rng(70)
    n, batch = 70, 3
    Y = rng.standard_normal((batch, 2 * n, n)) + 1j * rng.standard_normal((batch, 2 * n, n))
    Z = rng.standard_normal((batch, 2 * n, n)) + 1j * rng.standard_normal((batch, 2 * n, n))
    A = np.einsum("kmi,kmj->kij", Y.conj(), Y)
    B = np.einsum("kmi,kmj->kij", Z.conj(), Z)
    eng = Engine(1, 4, 4, reg_mode=_capi.REG_REL, reg_dark=1e-8)
    U, lam = eng.jdiag_large_complex(A, B)
    eng.close()
    for k in range(batch):
        _, lam_ref = gevd.jdiag(A[k], B[k], reg_mode=gevd.REG_MODE_REL)
        assert np.abs(lam[k] / lam_ref - 1).max() < 1e-9
        Bl = B[k] + 1e-8 * np.linalg.norm(B[k], 2) * np.eye(n)
        assert np.abs(U[k].conj().T @ Bl @ U[k] - np.eye(n)).max() < 1e-10


def test_jdiag_large_complex_repeated_eigenvalues(Engine):
    """Eigenvalue clusters: the real embedding returns an arbitrary real basis of each eigenspace; the selection must still
    hand back n vectors that are independent over C and meet jdiag's contract.  A = B Hermitian-congruent to
    diag(3, 3, 3, 3, 2, 2, 1, ..., 1): clusters of 4, 2 and n - 6."""
    rng = np.random.default_rng(8)
    n = 72
    T = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    B = T.conj().T @ T
    d = np.ones(n)
    d[:4], d[4:6] = 3.0, 2.0
    A = T.conj().T @ np.diag(d) @ T
    eng = Engine(1, 4, 4, reg_dark=0.0)
    U, lam = eng.jdiag_large_complex(A[None], B[None])
    eng.close()
    U, lam = U[0], lam[0]
    assert np.abs(lam - d).max() < 1e-9
    assert np.abs(U.conj().T @ B @ U - np.eye(n)).max() < 1e-9
    assert np.abs(U.conj().T @ A @ U - np.diag(lam)).max() < 1e-8


@pytest.mark.parametrize("L,M", [(64, 128), (32, 48)])
def test_corr_mfma_f32_and_bf16(Engine, L, M):
    """BASELINE config 5: correlation accumulated in fp32 (exact-product f32 MFMA) and from bf16 inputs (bf16 MFMA,
    f32 accumulation) against the float64 oracle."""
    rng = np.random.default_rng(L + M)
    K = 7
    XB, XD, d = cn(rng, K, M, L), cn(rng, K, M, L), cn(rng, K, M)
    RB0, RD0, r0 = subband.correlate(XB, XD, d)
    eng = Engine(K, L, M, compute_dtype="f32")
    RB, RD, r = eng.corr(XB, XD, d)
    RBh, RDh, rh = eng.corr_bf16(XB, XD, d)
    eng.close()
    for a, b in ((RB, RB0), (RD, RD0), (r, r0)):
        assert np.abs(a - b).max() <= 3e-6 * np.abs(b).max()
    # bf16 keeps 8 significant bits per input: gate of SURVEY.md section 8(c), R rel-Frobenius <= 1e-2
    for a, b in ((RBh, RB0), (RDh, RD0), (rh, r0)):
        rel = np.linalg.norm((a - b).reshape(K, -1), axis=1) / np.linalg.norm(b.reshape(K, -1), axis=1)
        assert rel.max() < 1e-2, rel.max()
    # Hermitian by construction of the four products
    assert np.abs(RBh - RBh.conj().transpose(0, 2, 1)).max() <= 1e-5 * np.abs(RBh).max()


def bf16_round(a):
    """Real and imaginary parts of a complex array rounded to bf16 (to nearest even), as float32 values."""
    def r32(x):
        u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
        u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
        return u.astype(np.uint32).view(np.float32)
    return r32(a.real) + 1j * r32(a.imag)


def test_corr_bf16_exact_on_rounded_inputs(Engine):
    """The bf16 path is exact up to f32 accumulation once the inputs are rounded to bf16: many bins, two runs
    (a scheduling-dependent fault in an earlier build showed up in a few bins per launch only)."""
    rng = np.random.default_rng(77)
    K, L, M = 300, 64, 128
    XB, XD, d = cn(rng, K, M, L), cn(rng, K, M, L), cn(rng, K, M)
    rnd = bf16_round
    RB0, RD0, r0 = subband.correlate(rnd(XB), rnd(XD), rnd(d))
    eng = Engine(K, L, M, compute_dtype="f32")
    first = None
    for _ in range(2):
        RB, RD, r = eng.corr_bf16(XB, XD, d)
        for a, b in ((RB, RB0), (RD, RD0), (r, r0)):
            rel = np.linalg.norm((a - b).reshape(K, -1), axis=1) / np.linalg.norm(b.reshape(K, -1), axis=1)
            assert rel.max() < 2e-6, rel.max()
        if first is not None:
            assert np.array_equal(first, r)
        first = r
    eng.close()


@pytest.mark.parametrize("spectrum", ["geometric", "two_levels", "one_large"])
def test_spectra_at_the_trust_threshold(Engine, spectrum):
    """Prescribed eigenvalues spanning just under 1e3 (the widest spectrum for which the float64 order-16 kernel still uses its
    one-sided float32 pre-solve), with the small ones spread out, in a tight cluster behind a gap, or all but one: the
    pre-solve leaves the columns of the small eigenvalues orthogonal only to 1e-3 ... 3e-2 there, which the refinement and
    the guarded path have to absorb.  R_D = I (orthonormal dark slab), R_B = U diag(lam) U^H."""
    rng = np.random.default_rng(11)
    K, L, M = 48, 16, 32
    lam = {"geometric": np.geomspace(1.0, 1.5e-3, L),
           "two_levels": np.r_[np.linspace(1.0, 0.5, 8), 1.5e-3 * (1 + 1e-3 * np.arange(8))],
           "one_large": np.r_[1.0, np.linspace(2e-3, 1.5e-3, L - 1)]}[spectrum]
    ranks = {"geometric": (1, 8, 16), "two_levels": (1, 8, 16), "one_large": (1, 16)}[spectrum]
    XB = np.zeros((K, M, L), np.complex128)
    XD = np.zeros((K, M, L), np.complex128)
    for k in range(K):
        U = np.linalg.qr(rng.standard_normal((L, L)) + 1j * rng.standard_normal((L, L)))[0]
        XB[k, :L] = np.sqrt(lam)[:, None] * U.conj().T * 3.0
        XD[k] = np.linalg.qr(rng.standard_normal((M, L)) + 1j * rng.standard_normal((M, L)))[0]
    XB, XD = XB.astype(np.complex64), XD.astype(np.complex64)
    d = cn(rng, K, M)
    eng = Engine(K, L, M, ranks=ranks, mu=0.1, compute_dtype="f64", out_c128=True)
    w, lam_gpu, status = eng.update(XB, XD, d)
    eng.close()
    w_ref, lam_ref, _ = subband.update(XB, XD, d, 0.1, list(ranks))
    assert not status.any()
    assert (np.abs(lam_gpu - lam_ref) / lam_ref[:, :1]).max() < 1e-12
    e = np.linalg.norm(w - w_ref, axis=-1) / np.linalg.norm(w_ref, axis=-1)
    assert e.max() < 1e-7, (spectrum, e.max(), np.unravel_index(e.argmax(), e.shape))


def test_rank_deficient_bright_matrix_every_bin(Engine):
    """M < L at the headline order, 64 bins, float64, filters returned in complex128: eight eigenvalues of C are zero, which
    the float32 pre-solve sees as eight columns at its shift that it does not orthogonalise against each other.  The float64
    stage must notice (V^H V far from I), throw the pre-solve away and rebuild C: before it did, one bin in thirty came out
    with its LEADING eigenvector off by 4e-5 while three bins of the same shape passed (tools/probes/rankdef_f32_probe.py)."""
    K, L, M, ranks = 64, 16, 8, (1, 4, 8)
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        XB, XD, d = cn(rng, K, M, L), cn(rng, K, M, L), cn(rng, K, M)
        eng = Engine(K, L, M, ranks=ranks, mu=0.7, compute_dtype="f64", reg_dark=1e-2, out_c128=True)
        w, lam, status = eng.update(XB, XD, d)
        eng.close()
        w_ref, lam_ref, _ = subband.update(XB, XD, d, 0.7, list(ranks), reg=1e-2)
        assert not status.any()
        e = np.linalg.norm(w - w_ref, axis=-1) / np.linalg.norm(w_ref, axis=-1)
        assert e.max() < 1e-9, (seed, e.max(), np.unravel_index(e.argmax(), e.shape))
        assert (np.abs(lam[:, :M] - lam_ref[:, :M]) / lam_ref[:, :1]).max() < 1e-11


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_degenerate_spectra(Engine, dtype):
    """Edge cases of the eigen-iteration at the headline shape: an all-zero bright slab (every pivot is exactly zero:
    no rotation may be attempted on 0/0), a bright matrix proportional to the identity with an identity dark matrix
    (fully degenerate spectrum) and already-diagonal matrices (nothing to rotate); no NaN, status 0, filters as the
    oracle's."""
    L, M = 16, 32
    rng = np.random.default_rng(5)
    XB, XD, d = cn(rng, 4, M, L), cn(rng, 4, M, L), cn(rng, 4, M)
    XB[0] = 0                                            # R_B = 0: all eigenvalues 0, r = 0, w = 0
    Q = np.linalg.qr(cn(rng, M, L).astype(np.complex128))[0]
    XB[1] = (3.0 * Q).astype(np.complex64)               # R_B = 9 I
    XD[1] = np.linalg.qr(cn(rng, M, L).astype(np.complex128))[0].astype(np.complex64)     # R_D = I
    XB[2] = 0
    XB[2, :L, :] = np.diag(np.arange(1, L + 1)).astype(np.complex64)                      # diagonal R_B
    XD[2] = 0
    XD[2, :L, :] = np.diag(np.linspace(2, 3, L)).astype(np.complex64)                     # diagonal R_D
    eng = Engine(4, L, M, ranks=(1, 8, 16), mu=1.0, compute_dtype=dtype)
    w, lam, status = eng.update(XB, XD, d)
    eng.close()
    assert not status.any() and np.isfinite(w).all() and np.isfinite(lam).all()
    w_ref, lam_ref, _ = subband.update(XB, XD, d, 1.0, [1, 8, 16])
    assert np.abs(lam[0]).max() < 1e-6 and np.abs(w[0]).max() < 1e-6
    # sixteen eigenvalues inside a 1e-7-wide cluster (c64 rounding of the orthonormal columns): the sweep criterion is
    # relative to ||C||, so the members are resolved to a fraction of the cluster width, not to 1e-9
    assert np.abs(lam[1] / lam_ref[1] - 1).max() < max(TOL[dtype]["lam"] * 10, 1e-7)
    assert np.abs(lam[2:] / lam_ref[2:] - 1).max() < TOL[dtype]["lam"] * 10
    # degenerate eigenvalues: only the full-rank filter (and the projector it implies) is unique
    assert w_err(w[1:2, 2], w_ref[1:2, 2]) < TOL[dtype]["w"] * 10
    assert w_err(w[2:, :], w_ref[2:, :]) < TOL[dtype]["w"] * 10


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_nan_bin_is_contained(Engine, dtype):
    """A NaN in one bin's slab (a dead sensor, an overflow upstream) must stay in that bin: the launch completes, the other
    bins come out as the oracle's, and the poisoned bin reports itself (status != 0 or non-finite filters) instead of
    returning finite numbers.  (The float factor's index permutation is built from comparisons of the diagonal: with NaN
    they are all false, and the indices must still stay inside the matrix.)"""
    L, M, K = 16, 32, 8
    rng = np.random.default_rng(91)
    XB, XD, d = cn(rng, K, M, L), cn(rng, K, M, L), cn(rng, K, M)
    XB[3, 5, 7] = np.nan
    XD[6, 0, :] = np.nan
    eng = Engine(K, L, M, ranks=(1, 8, 16), mu=1.0, compute_dtype=dtype)
    w, lam, status = eng.update(XB, XD, d, raise_on_status=False)
    eng.close()
    good = [k for k in range(K) if k not in (3, 6)]
    w_ref, lam_ref, _ = subband.update(XB[good], XD[good], d[good], 1.0, [1, 8, 16])
    assert not status[good].any()
    assert w_err(w[good], w_ref) < TOL[dtype]["w"] * 10
    assert np.abs(lam[good] / lam_ref - 1).max() < TOL[dtype]["lam"] * 10
    for k in (3, 6):
        assert status[k] != 0 or not np.isfinite(w[k]).all() or not np.isfinite(lam[k]).all(), k


@pytest.mark.parametrize("scale", [1e-8, 1e8])
def test_input_scale_robustness(Engine, scale):
    """The float32 pre-solve works on a copy of C brought to unit norm by a power of two: inputs far from unit scale
    (R of order 1e-16 or 1e+16) must give the oracle's answer all the same."""
    rng = np.random.default_rng(77)
    K, L, M = 32, 16, 32
    XB, XD, d = (cn(rng, K, M, L) * np.float32(scale)), (cn(rng, K, M, L) * np.float32(scale)), cn(rng, K, M) * np.float32(scale)
    reg = 1e-7 * scale * scale                      # keep the loading proportionate so that the problem stays the same
    eng = Engine(K, L, M, ranks=(1, 8, 16), mu=1.0, compute_dtype="f64", reg_dark=reg)
    w, lam, status = eng.update(XB, XD, d)
    eng.close()
    w_ref, lam_ref, _ = subband.update(XB, XD, d, 1.0, [1, 8, 16], reg=reg)
    assert not status.any()
    assert np.abs(lam / lam_ref - 1).max() < 1e-9
    assert w_err(w, w_ref) < 1e-7


def test_bench_distributed_rehearsal_without_torch():
    """The whole multi-rank code path of bench.py (TCP rendezvous, RCCL communicator, cfg4 shard, all-gather on the side
    stream, RCCL barrier) at world size 1, in a fresh interpreter that must never import torch."""
    import json
    import subprocess
    code = ("import sys, runpy; sys.argv = ['bench.py', '--steps', '4', '--warmup', '2', '--prespin', '0.05', '--no-cpu-baseline'];"
            "runpy.run_path(%r, run_name='__main__'); assert 'torch' not in sys.modules" % os.path.join(ROOT, "bench.py"))
    env = dict(os.environ, APV_BENCH_FORCE_DIST="1", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT="29655")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["config"]["workload"].startswith("cfg4") and line["collective_us"] > 0
    assert line["collective_bytes_per_rank"] == 32 * 4096 * 16 * 8 and line["value"] > 1e6          # 32 blocks of 4096 bins per rank and step


def test_bench_plain_run_is_the_headline_alone():
    """bench.py at one GPU: a plain run prints the headline without the sub-records, the CPU baseline or the one-stream roofline
    leg; --full adds that leg (here without the sub-records and the CPU baseline, which take tens of seconds)."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "APV_BENCH_FORCE_DIST")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "2", "--prespin", "0.05"]
    lines = []
    for extra in ([], ["--full", "--no-also", "--no-cpu-baseline"]):
        r = subprocess.run(cmd + extra, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    plain, full = lines
    for line in lines:
        assert line["unit"] == "updates/s" and line["value"] > 1e6 and line["steps"] == 4 and line["ms_per_step"] > 0
        assert line["config"]["update_streams"] == 2 and line["roofline"]["pipelined"]["ms_per_launch"] > 0
        assert "also" not in line and "cpu_baseline" not in line
    assert plain["roofline"]["kernel_ms"] is None and plain["roofline"]["alu"]["frac"] is None
    assert full["roofline"]["kernel_ms"] > 0 and full["roofline"]["alu"]["frac"] > 0
