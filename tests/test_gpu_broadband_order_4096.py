"""Broadband orders J L from 2049 up to 4096 (main.m's n = J L = 400 x 10 = 4000): the joint diagonalisations, the spectral
norm of the MATLAB dialect's relative loading, whole hops in both dialects, the static solver and the limits.  The CPU
oracle's generalised eigh at n = 4000 takes seconds per call, so every case is sized to finish within a minute or two."""
import os
import sys
import time
import warnings

import numpy as np
import pytest
import scipy.linalg as sla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import gevd  # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu

BUDGET_S = 240.0          # per case: the oracle's eigh at n = 4000 is the slow part


@pytest.fixture
def budget():
    t0 = time.perf_counter()
    yield
    assert time.perf_counter() - t0 < BUDGET_S, f"case took {time.perf_counter() - t0:.0f} s"


def synth_rirs(P, L, M, seed):
    rng = np.random.default_rng(seed)
    env = np.exp(-np.arange(P) / (P / 6.0))[:, None, None]
    return (rng.standard_normal((P, L, M)) * env * 1e-3, rng.standard_normal((P, L, M)) * env * 1e-3)


def spd_pair(n, seed):
    """A, B symmetric positive definite with eigenvalues spread over four decades (log-uniform spectra)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        G = rng.standard_normal((n, n + 64)) / np.sqrt(n)
        S = G @ G.T
        S += np.diag(10.0 ** rng.uniform(-2, 2, n))
        out.append(0.5 * (S + S.T))
    return out


def engine(**kw):
    from ap_vast_unofficial_amd import _capi
    return _capi.Engine(1, 4, 4, **kw)


def check_pairs(A, B, U, lam, reg):
    """lam against the oracle's eigenvalues; U^T (B + reg I) U = I and A U = (B + reg I) U diag(lam) column by column."""
    n = A.shape[0]
    Bl = B + reg * np.eye(n)
    lam_ref = sla.eigh(A, Bl, eigvals_only=True)[::-1]
    assert np.abs(lam / lam_ref - 1).max() <= 1e-9
    assert np.abs(U.T @ Bl @ U - np.eye(n)).max() <= 1e-9
    assert np.abs(A @ U - (Bl @ U) * lam[None, :]).max() <= 1e-9 * np.linalg.norm(A, 2)


# ---- 1. jdiag_large ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch", [(2049, 1), (2049, 2), (3001, 1), (3001, 2), (4000, 1), (4000, 2), (4096, 1), (4096, 2)])
def test_jdiag_large_beyond_2048(n, batch, budget):
    pairs = [spd_pair(n, 10 * n + z) for z in range(batch)]
    A = np.stack([p[0] for p in pairs])
    B = np.stack([p[1] for p in pairs])
    eng = engine(reg_dark=1e-7)
    U, lam = eng.jdiag_large(A, B)
    eng.close()
    for z in range(batch):
        check_pairs(A[z], B[z], U[z], lam[z], 1e-7)


def test_apvast_jdiag_4000_no_convergence_warning(budget):
    from ap_vast_unofficial_amd import apvast as mod
    A, B = spd_pair(4000, 7)
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # a ConvergenceWarning (or any other) fails the case
        U, D = mod.jdiag(A, B)
    lam = np.diag(D)
    reg = 1e-8 * np.linalg.norm(B, 2) if not mod.EXPERIMENTAL_REGULARIZATION else 1e-7
    lam_ref = sla.eigh(A, B + reg * np.eye(4000), eigvals_only=True)[::-1]
    assert np.abs(lam / lam_ref - 1).max() <= 1e-9


# ---- 2. jdiag_leading -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", [8, 40])
def test_jdiag_leading_4000(rank, budget):
    n = 4000
    A, B = spd_pair(n, 99 + rank)
    eng = engine(reg_dark=1e-7)
    U, lam, info = eng.jdiag_leading(A[None], B[None], rank)
    eng.close()
    U, lam = U[0], lam[0]
    Bl = B + 1e-7 * np.eye(n)
    lam_ref = sla.eigh(A, Bl, eigvals_only=True, subset_by_index=[n - rank, n - 1])[::-1]
    assert np.abs(lam / lam_ref - 1).max() <= 1e-9
    assert np.abs(U.T @ Bl @ U - np.eye(rank)).max() <= 1e-9
    assert np.abs(A @ U - (Bl @ U) * lam[None, :]).max() <= 1e-9 * np.linalg.norm(A, 2)


# ---- 3. main.m at full size, MATLAB dialect ---------------------------------------------------------------------------
@pytest.mark.parametrize("perceptual", [False, True])
def test_broadband_matlab_main_m_full_size(perceptual, budget):
    """main.m:34-42: N = 1020, J = 400, 10 loudspeakers (n = 4000), ranks 1, 2000, 4000, 8 kHz.  Synthetic responses: the
    bundled rirs.mat has 8 loudspeakers.  With M = 8 microphones the data matrix of apVast.m:410-425 has
    M (S - J + 1) = 8 x 621 = 4968 columns > n, so R is of full rank and rank 4000 is well defined."""
    from ap_vast_unofficial_amd.apvast import apvast
    from oracle.broadband_matlab import MatlabBroadbandOracle
    from oracle.perceptual import Model
    rA, rB = synth_rirs(500, 10, 8, 31)
    ranks = [1, 2000, 4000]
    kw = dict(fullscale_db_spl=94.0) if perceptual else {}
    ap = apvast(1020, rA, rB, 400, 50, 0, 0, ranks, 1.0, 1020, sampling_rate=8000, perceptual=perceptual,
                mode="broadband", dialect="matlab", **kw)
    orc = MatlabBroadbandOracle(1020, rA, rB, 400, 50, 0, 0, ranks, 1.0, 1020, sampling_rate=8000,
                                model=Model(1020, 8000, 94.0) if perceptual else None)
    rng = np.random.default_rng(21)                 # the small-noise start of test_broadband_matlab_main_m_construction
    orc.response[:] = 1e-3 * rng.standard_normal(orc.response.shape)
    orc.target_response[:] = 1e-3 * rng.standard_normal(orc.target_response.shape)
    ap.set_state({"response": orc.response.copy(), "target_response": orc.target_response.copy()})
    H = ap.hop_size
    x = np.random.default_rng(8).standard_normal((2, 2 * H))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for h in range(2):
            got = ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
            exp = orc.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
            # rank 2000 of 4000 is well posed only if lambda_2000 and lambda_2001 are apart
            for lam in (orc.lambda_A, orc.lambda_B):
                gap = (lam[1999] - lam[2000]) / abs(lam[1999])
                assert gap > 1e-6, gap
            for q in range(4):
                e = exp[q]
                assert np.abs(np.stack(got[q]) - e).max() <= 1e-6 * max(np.abs(e).max(), 1e-30), (h, q)
    for i in range(len(ranks)):
        assert np.linalg.norm(ap.w_A[i, :, 0] - orc.w_A[i]) <= 1e-6 * np.linalg.norm(orc.w_A[i]), i
        assert np.linalg.norm(ap.w_B[i, :, 0] - orc.w_B[i]) <= 1e-6 * np.linalg.norm(orc.w_B[i]), i
    ap.close()


# ---- 4. Python dialect at n = 4000 ------------------------------------------------------------------------------------
def test_broadband_python_dialect_4000(golden, budget):
    """The bundled 8-loudspeaker responses with J = 500 (n = 4000), three hops against the restatement of apvast.py at the
    bounds of test_g1_broadband_end_to_end_on_gpu.  M (S - J) = 8 x 524 = 4192 > n: full-rank statistics."""
    from ap_vast_unofficial_amd.apvast import apvast
    from oracle.broadband import BroadbandOracle
    rirs = golden("rirs_cfg1")
    rA, rB = rirs["rirA"], rirs["rirB"]
    N, J, S, V = 1024, 500, 1024, 8
    ap = apvast(N, rA, rB, J, 20, 1, 2, V, 1.0, S, perceptual=False, mode="broadband", seed=4)
    np.random.seed(4)
    orc = BroadbandOracle(N, rA, rB, J, 20, 1, 2, V, 1.0, S)
    H = ap.hop_size
    x = np.random.default_rng(8).standard_normal((2, 3 * H))
    worst = dict(out=0.0, lam=0.0, w=0.0)
    for h in range(3):
        got = ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        exp = orc.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        for q in range(4):
            e = exp[q]
            worst["out"] = max(worst["out"], np.abs(np.stack(got[q]) - e).max() / max(np.abs(e).max(), 1e-30))
        for lam, w, lr, wr in ((ap.lambda_A, ap.w_A, orc.lambda_A, orc.w_A), (ap.lambda_B, ap.w_B, orc.lambda_B, orc.w_B)):
            lam = np.diag(lam) if lam.ndim == 2 else lam
            worst["lam"] = max(worst["lam"], np.abs(lam[:V] / lr[:V] - 1).max())
            for i in range(V):
                worst["w"] = max(worst["w"], np.linalg.norm(w[i, :, 0] - wr[i]) / np.linalg.norm(wr[i]))
    print("worst relative errors vs the oracle:", worst)
    assert worst["lam"] < 1e-9
    assert worst["w"] < 1e-8
    assert worst["out"] < 1e-9
    ap.close()


# ---- 5. process_signal at n = 4000 ------------------------------------------------------------------------------------
def test_broadband_process_signal_order_4000(golden, budget):
    """At n = 4000 one hop's matrices take ~5 GB, so the group rule (stream_bb.hip, <= 8 GiB a group) forms groups of one
    hop: three hops are three groups.  Outputs and attributes as the hop loop leaves them."""
    from ap_vast_unofficial_amd.apvast import apvast
    rirs = golden("rirs_cfg1")
    N, J, S, V = 1024, 500, 1024, 8

    def mk():
        return apvast(N, rirs["rirA"], rirs["rirB"], J, 20, 1, 2, V, 1.0, S, perceptual=False, mode="broadband", seed=5)
    a, b = mk(), mk()
    H = a.hop_size
    hops = 3
    x = np.random.default_rng(77).standard_normal((2, hops * H))
    whole = a.process_signal(x[0], x[1])
    per_hop = [b.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H]) for h in range(hops)]
    worst = 0.0
    for q in range(4):
        for v in range(len(whole[q])):
            ref = np.concatenate([per_hop[h][q][v] for h in range(hops)])
            worst = max(worst, np.abs(whole[q][v] - ref).max() / max(np.abs(ref).max(), 1e-30))
    print("whole signal against the hop loop, worst relative difference:", worst)
    assert worst <= 1e-9
    for name in ("lambda_A", "lambda_B", "r_A", "R_A_to_A", "R_A_to_B"):
        va, vb = getattr(a, name), getattr(b, name)
        assert np.abs(va - vb).max() <= 1e-9 * np.abs(vb).max(), name
    a.close()
    b.close()


# ---- 6. the spectral norm ---------------------------------------------------------------------------------------------
def spiked_psd(n, seed):
    """A Wishart matrix plus a rank-one spike, so that the largest eigenvalue stands apart from the rest."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n + n // 4)) / np.sqrt(n)
    u = rng.standard_normal(n)
    R = G @ G.T + 8.0 * np.outer(u, u) / (u @ u)
    return 0.5 * (R + R.T)


def top_eig(R):
    n = R.shape[0]
    return sla.eigh(R, eigvals_only=True, subset_by_index=[n - 1, n - 1])[0]


@pytest.mark.parametrize("n", [2500, 4000])
def test_norm2_large_orders(n, budget):
    mats = np.stack([spiked_psd(n, n + q) for q in range(4)])
    ref = np.array([top_eig(m) for m in mats])
    eng = engine()
    auto = eng.norm2(mats)
    grid = eng.norm2(mats, "grid")
    one = eng.norm2(mats, "one_wg")
    eng.close()
    assert np.array_equal(auto, grid)                # above 2048 a hop runs the chip-wide steps
    assert np.abs(grid / ref - 1).max() <= 1e-10
    assert np.abs(one / ref - 1).max() <= 1e-10
    assert abs(np.linalg.norm(mats[0], 2) / grid[0] - 1) <= 1e-10


@pytest.mark.parametrize("n", [300, 2048])
def test_norm2_below_threshold_is_the_one_workgroup_kernel(n):
    mats = np.stack([spiked_psd(n, 3 * n + q) for q in range(3)])
    eng = engine()
    auto = eng.norm2(mats)
    one = eng.norm2(mats, "one_wg")
    grid = eng.norm2(mats, "grid")
    eng.close()
    assert np.array_equal(auto, one)                 # the kernel every accepted order ran before, bit for bit
    ref = np.array([np.linalg.norm(m, 2) for m in mats])
    assert np.abs(one / ref - 1).max() <= 1e-10
    assert np.abs(grid / ref - 1).max() <= 1e-10


# ---- 7. the static solver ---------------------------------------------------------------------------------------------
def test_static_vast_4000(budget):
    from ap_vast_unofficial_amd.evaluation import vast
    from oracle import static_vast
    rng = np.random.default_rng(13)
    P, L, J = 500, 10, 400
    env = np.exp(-np.arange(P) / 80.0)[None, :, None]
    gB = rng.standard_normal((8, P, L)) * env
    gD = rng.standard_normal((8, P, L)) * env
    w = vast(gB, gD, J, 20, 1, 100, 0.8)
    w_ref, _ = static_vast.vast(gB, gD, J, 20, 1, 100, 0.8)
    assert np.linalg.norm(w - w_ref) < 1e-8 * np.linalg.norm(w_ref)


# ---- 8. the limits ----------------------------------------------------------------------------------------------------
def test_order_limit_is_4096():
    from ap_vast_unofficial_amd.apvast import apvast
    from ap_vast_unofficial_amd import _capi
    from ap_vast_unofficial_amd import apvast as mod
    rA, rB = synth_rirs(300, 17, 2, 3)
    with pytest.raises(_capi.ApvError, match="4096"):
        apvast(512, rA, rB, 241, 8, 0, 0, 4, 1.0, 600, perceptual=False, mode="broadband", seed=0)       # 241 x 17 = 4097
    ap = apvast(512, rA[:, :16], rB[:, :16], 256, 8, 0, 0, 4, 1.0, 600, perceptual=False, mode="broadband", seed=0)   # 4096
    ap.close()
    eng = engine()
    z = np.zeros((1, 4097, 4097))
    for call in (lambda: eng.jdiag_large(z, z), lambda: eng.jdiag_leading(z, z, 4), lambda: eng.norm2(z)):
        with pytest.raises(_capi.ApvError, match="4096"):
            call()
    eng.close()
    with pytest.raises(NotImplementedError, match="4096"):
        mod.jdiag(np.eye(4097), np.eye(4097))
    with pytest.raises(_capi.ApvError, match="4096"):
        from ap_vast_unofficial_amd.evaluation import vast
        vast(np.zeros((2, 300, 17)), np.zeros((2, 300, 17)), 241, 5, 0, 1, 1.0)
