"""The trimmed float64 stages of the order-16 kernel (kernels_gevd16m.hip) where they can go wrong.

  failed pivots    Stage 1 no longer tests the pivot inside its loop: the sixteen steps run on whatever a bad pivot leaves and the
                   pivots are tested afterwards, each row its own.  Pairs R_D = L D L^H (L unit lower) with a pivot D_k <= 0 at
                   k = 0, 1, 3, 4, 7, 8, 15, one with D_0 = 0, one with a NaN and one with +inf on the diagonal, interleaved with
                   good bins: status 1 on exactly those bins with zero outputs, the good bins inside the parity bounds and bit for
                   bit what a launch without the bad bins gives.  The same through the fused entry (X_D of a bin zero, or one of its
                   columns, under a negative loading).
  eigenvalues      The refinement's second-order eigenvalue term is summed by columns.  Pairs 3e-3, 1e-3 and 1e-4 ||C|| apart at
                   the bottom, in the middle and at the top of the spectrum, and the bench's graded spectrum, to 1e-12 ||C||: the
                   corrected eigenvalue is exact to third order, and at |Z| <= 3e-5 the cubic term is below 3e-14 ||C||.
  rank lists       The output stage sums a filter on all 64 lanes, lane (i, q) the sorted columns q, q + 4, ...: every rank of
                   every list against the oracle, and a rank taken from a multi-rank launch bit for bit the single-rank launch's.

Bounds: those of tests/test_gpu_parity.py for the same quantities.  (The eigenvector output U is reached through jdiag_batched
alone, with the rank list (1,): test_gpu_parity.py::test_jdiag_batched_invariants covers it; its store did not change.)
Run on the MI355X box with `-m gpu`."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import subband  # noqa: E402  (checker only)
from presolve_cases import cn, rel_w, with_spectrum  # noqa: E402

L, M = 16, 32
REG = 1e-7                                    # the engine's and the oracle's loading of R_D
MU = 0.7
TOL = {"f64": dict(lam=1e-9, w=1e-7)}         # tests/test_gpu_parity.py; float32: the per-bin bound below
EPS32 = float(np.finfo(np.float32).eps)
BAD_AT = [0, 1, 3, 4, 7, 8, 15]               # pivot positions: first and last, and both sides of a column group's boundary


@pytest.fixture(scope="module")
def Engine():
    from ap_vast_unofficial_amd import Engine
    return Engine


# ---------------------------------------------------------------------------------------------------------------------
# failed pivots
# ---------------------------------------------------------------------------------------------------------------------
def ldl_pair(rng, D):
    """R_D with R_D + REG I = L D L^H, L unit lower triangular with entries of size 0.3 below the diagonal"""
    Lw = np.eye(L, dtype=np.complex128) + np.tril(0.3 * (rng.standard_normal((L, L)) + 1j * rng.standard_normal((L, L))), -1)
    A = (Lw * D) @ Lw.conj().T
    A = 0.5 * (A + A.conj().T)
    return A - REG * np.eye(L)


def pivots(A):
    """the pivots of the unpivoted elimination of A, as far as they are defined"""
    A = np.array(A, dtype=np.complex128)
    out = []
    for k in range(L):
        d = A[k, k].real
        out.append(d)
        if not np.isfinite(d) or d == 0:
            break
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:, k].conj()) / d
    return np.array(out)


def pivot_bins():
    """K = 21: good bins at the even indices, at the odd ones the ten bad bins.  Returns RB, RD, r, the bad mask and the D of
    every bin (None where the bin is not an L D L^H with finite D)."""
    rng = np.random.default_rng(4101)
    kinds = [("neg", k) for k in BAD_AT] + [("zero", 0), ("nan", 5), ("inf", 7)]
    K = 2 * len(kinds) + 1
    RB, RD, Ds, bad = [], [], [], np.zeros(K, bool)
    for k in range(K):
        Y = rng.standard_normal((M, L)) + 1j * rng.standard_normal((M, L))
        RB.append(Y.conj().T @ Y)
        D = rng.uniform(0.5, 2.0, L)
        if k & 1:
            bad[k] = True
            kind, pos = kinds[k // 2]
            if kind == "neg":
                D[pos] = -0.5
            elif kind == "zero":
                D[pos] = 0.0
        A = ldl_pair(rng, D)
        if k & 1 and kind == "nan":
            A[pos, pos] = np.nan
            D = None
        if k & 1 and kind == "inf":
            A[pos, pos] = np.inf
            D = None
        RD.append(A)
        Ds.append(D)
    r = rng.standard_normal((K, L)) + 1j * rng.standard_normal((K, L))
    return np.array(RB), np.array(RD), r, bad, Ds


def test_constructed_pivots():
    """The pairs have the pivots intended (runs without a GPU: it only inspects the inputs): D_k to 1e-10 at every position, the
    zero pivot exactly zero in float64 and in float32, NaN and +inf where they were put."""
    RB, RD, r, bad, Ds = pivot_bins()
    seen_bad = []
    for k in range(len(RD)):
        p = pivots(RD[k] + REG * np.eye(L))
        if Ds[k] is None:
            assert not np.isfinite(p[-1]) and np.isfinite(p[:-1]).all() and (p[:-1] > 0).all()
            seen_bad.append(len(p) - 1)
            continue
        if (Ds[k] == 0).any():
            assert p[0] == 0.0 and len(p) == 1
            assert np.float32(RD[k][0, 0].real) + np.float32(REG) == 0.0
            seen_bad.append(0)
            continue
        assert len(p) == L and np.allclose(p, Ds[k], rtol=1e-10, atol=0)
        neg = np.flatnonzero(p <= 0)
        assert (len(neg) > 0) == bool(bad[k])
        if len(neg):
            assert len(neg) == 1 and p[neg[0]] < -0.4
            seen_bad.append(int(neg[0]))
    assert seen_bad == BAD_AT + [0, 5, 7]


def f32_bounds(RD_loaded):
    """tests/test_gpu_parity.py: |d lam| / lam_max <= 4 eps32 cond(R_D + reg I), ||d w|| / ||w|| <= 16 eps32 cond, floor 1e-6"""
    bound = EPS32 * np.linalg.cond(RD_loaded)
    return np.maximum(4 * bound, 1e-6), np.maximum(16 * bound, 1e-6)


def check_good_bins(dtype, w, lam, w_ref, lam_ref, RD_loaded, label):
    if dtype == "f64":
        e_lam, e_w = np.abs(lam / lam_ref - 1).max(), rel_w(w, w_ref)
        print(f"{label}: lam {e_lam:.2e}  w {e_w:.2e}")
        assert e_lam < TOL["f64"]["lam"] and e_w < TOL["f64"]["w"]
    else:
        b_lam, b_w = f32_bounds(RD_loaded)
        e_lam = (np.abs(lam - lam_ref) / lam_ref[:, :1]).max(axis=1)
        e_w = (np.linalg.norm(w - w_ref, axis=-1) / np.linalg.norm(w_ref, axis=-1)).max(axis=1)
        print(f"{label}: lam / bound {(e_lam / b_lam).max():.2f}  w / bound {(e_w / b_w).max():.2f}")
        assert (e_lam <= b_lam).all() and (e_w <= b_w).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_failed_pivots_built_pairs(Engine, dtype):
    RB, RD, r, bad, _ = pivot_bins()
    K, ranks = len(RB), (1, 8, 16)
    eng = Engine(K, L, M, ranks=ranks, mu=MU, compute_dtype=dtype, reg_dark=REG)
    w, lam, status = eng.gevd_vast(RB, RD, r, raise_on_status=False)
    eng.close()
    print("status:", status)
    assert np.array_equal(status == 1, bad) and not status[~bad].any()
    assert not w[bad].any() and not lam[bad].any()
    good = ~bad
    eng = Engine(int(good.sum()), L, M, ranks=ranks, mu=MU, compute_dtype=dtype, reg_dark=REG)
    w0, lam0, status0 = eng.gevd_vast(RB[good], RD[good], r[good])
    eng.close()
    assert not status0.any()
    assert np.array_equal(w[good], w0) and np.array_equal(lam[good], lam0)
    w_ref, lam_ref, st_ref = subband.gevd_vast(RB[good], RD[good], r[good], MU, list(ranks), reg=REG)
    assert not st_ref.any()
    check_good_bins(dtype, w[good], lam[good], w_ref, lam_ref, RD[good] + REG * np.eye(L), f"built pairs, {dtype}")


def fused_pivot_bins():
    """K = 20 under the loading -1e-3: X_D of bin 3 zero (test_gpu_parity.py::test_not_positive_definite_raises), column c of X_D
    zero in bins 1, 5, 7, ... for c in BAD_AT (pivot c is the loading itself, the earlier ones are positive)"""
    rng = np.random.default_rng(4102)
    K = 20
    XB, XD, d = cn(rng, K, M, L), cn(rng, K, M, L), cn(rng, K, M)
    first_bad = {3: 0}
    XD[3] = 0
    for k, c in zip([1, 5, 7, 9, 11, 13, 15], BAD_AT):
        XD[k, :, c] = 0
        first_bad[k] = c
    bad = np.zeros(K, bool)
    bad[list(first_bad)] = True
    return XB, XD, d, bad, first_bad


FUSED_REG = -1e-3


def test_constructed_pivots_fused():
    XB, XD, d, bad, first_bad = fused_pivot_bins()
    _, RD, _ = subband.correlate(XB, XD, d)
    for k in range(len(RD)):
        p = pivots(RD[k] + FUSED_REG * np.eye(L))
        neg = np.flatnonzero(p <= 0)
        if bad[k]:
            assert neg[0] == first_bad[k] and abs(p[neg[0]] - FUSED_REG) < 1e-9
        else:
            assert len(neg) == 0 and p.min() > 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_failed_pivots_fused(Engine, dtype):
    XB, XD, d, bad, _ = fused_pivot_bins()
    K, ranks = len(XB), (1, 8, 16)
    eng = Engine(K, L, M, ranks=ranks, mu=MU, compute_dtype=dtype, reg_dark=FUSED_REG)
    with pytest.raises(np.linalg.LinAlgError):
        eng.update(XB, XD, d)
    w, lam, status = eng.update(XB, XD, d, raise_on_status=False)
    eng.close()
    print("status:", status)
    assert np.array_equal(status == 1, bad) and not status[~bad].any()
    assert not w[bad].any() and not lam[bad].any()
    good = ~bad
    eng = Engine(int(good.sum()), L, M, ranks=ranks, mu=MU, compute_dtype=dtype, reg_dark=FUSED_REG)
    w0, lam0, status0 = eng.update(XB[good], XD[good], d[good])
    eng.close()
    assert not status0.any()
    assert np.array_equal(w[good], w0) and np.array_equal(lam[good], lam0)
    w_ref, lam_ref, _ = subband.update(XB[good], XD[good], d[good], MU, list(ranks), reg=FUSED_REG)
    RD = subband.correlate(XB[good], XD[good], d[good])[1] + FUSED_REG * np.eye(L)
    check_good_bins(dtype, w[good], lam[good], w_ref, lam_ref, RD, f"fused, {dtype}")


# ---------------------------------------------------------------------------------------------------------------------
# eigenvalues
# ---------------------------------------------------------------------------------------------------------------------
PAIR_GAPS = [3e-3, 1e-3, 1e-4]                # x ||C||_F
PAIR_AT = {"bottom": 14, "middle": 7, "top": 0}
BINS_PER_CASE = 4
BENCH_BINS = 64


def pair_spectrum(gap, where):
    """a graded spectrum (1 ... 0.05) in which eigenvalue j + 1 is gap ||C||_F below eigenvalue j; descending, simple"""
    lam = np.geomspace(1.0, 0.05, L)
    j = PAIR_AT[where]
    for _ in range(3):                                                  # ||C||_F depends on the moved eigenvalue: settle it
        lam[j + 1] = lam[j] - gap * np.linalg.norm(lam)
    assert (np.diff(lam) < 0).all() and abs((lam[j] - lam[j + 1]) / np.linalg.norm(lam) - gap) < 1e-3 * gap
    return lam


def bench_C(n):
    """the bench workload's pencils whitened in float64 (as tools/probes/tridiag_presolve_model.py make_C does): its graded spectrum"""
    import bench
    XB, XD, _ = bench.synth(n, 1234)
    RB, RD, _ = subband.correlate(XB, XD, np.zeros(XB.shape[:2]))
    W = np.linalg.inv(np.linalg.cholesky(RD + REG * np.eye(L)))
    C = W @ RB @ W.conj().transpose(0, 2, 1)
    return 0.5 * (C + C.conj().transpose(0, 2, 1))


@pytest.fixture(scope="module")
def eigenvalues(Engine):
    """every case in ONE batch through the built-pair entry with R_D = I (the whitening is an exact scaling by 1 / (1 + REG)):
    lam in float64, and the eigenvalues of R_B by LAPACK"""
    rng = np.random.default_rng(4103)
    cases, RB = {}, []
    for gap in PAIR_GAPS:
        for where in PAIR_AT:
            cases[f"{gap:g}/{where}"] = slice(len(RB), len(RB) + BINS_PER_CASE)
            RB += [with_spectrum(rng, pair_spectrum(gap, where)) for _ in range(BINS_PER_CASE)]
    cases["bench"] = slice(len(RB), len(RB) + BENCH_BINS)
    RB += list(bench_C(BENCH_BINS))
    RB = np.array(RB)
    K = len(RB)
    assert 20 <= K <= 256
    r = rng.standard_normal((K, L)) + 1j * rng.standard_normal((K, L))
    RD = np.broadcast_to(np.eye(L, dtype=np.complex128), RB.shape).copy()
    eng = Engine(K, L, M, ranks=(1,), mu=MU, compute_dtype="f64", out_c128=True, reg_dark=REG)
    _, lam, status = eng.gevd_vast(RB, RD, r, raise_on_status=False)
    eng.close()
    lam_np = np.linalg.eigvalsh(RB)[:, ::-1] / (1 + REG)
    return cases, lam, status, lam_np


@pytest.mark.gpu
@pytest.mark.parametrize("name", [f"{gap:g}/{where}" for gap in PAIR_GAPS for where in PAIR_AT] + ["bench"])
def test_eigenvalues_to_third_order(eigenvalues, name):
    """Within 1e-12 ||C|| of LAPACK's (measured: 1.7e-15 at worst).  Checked once on a scratch build with the second-order term
    dropped (sLam2 = the Rayleigh quotients): it misses the bound at 0.003/top (4.1e-12) and at 0.001/middle (1.5e-12) and comes
    within a factor of three of it in five more cases."""
    cases, lam, status, lam_np = eigenvalues
    sel = cases[name]
    err = (np.abs(lam[sel] - lam_np[sel]) / lam_np[sel, :1]).max()
    print(f"{name}: status {np.unique(status[sel])}  lam error {err:.2e} ||C||")
    assert not status[sel].any()
    assert err < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# rank lists
# ---------------------------------------------------------------------------------------------------------------------
RANK_LISTS = [(1,), (3,), (4,), (5,), (8,), (16,), (1, 8, 16), (3, 5, 6, 7), (4, 16), tuple(range(1, 9))]
SINGLES = sorted({V for ranks in RANK_LISTS for V in ranks})
RK, RK_BAD = 24, 13                          # bins; the one whose X_D holds a NaN (status 1)


def rank_bins():
    rng = np.random.default_rng(4104)
    XB, XD, d = cn(rng, RK, M, L), cn(rng, RK, M, L), cn(rng, RK, M)
    XD[RK_BAD, 2, 9] = np.nan
    return XB, XD, d


def launch(Engine, XB, XD, d, ranks, dtype, out_c128, with_lam):
    """w, lam (None without), status of one launch; with_lam = False goes through the device entry with no lam buffer"""
    eng = Engine(RK, L, M, ranks=ranks, mu=MU, compute_dtype=dtype, out_c128=out_c128, reg_dark=REG)
    if with_lam:
        out = eng.update(XB, XD, d, raise_on_status=False)
    else:
        bufs = [eng.to_device(a) for a in (XB, XD, d)]
        dw = eng.alloc(RK * len(ranks) * L * np.dtype(eng.w_dtype).itemsize)
        ds = eng.alloc(RK * 4)
        eng.update_dev(bufs[0], bufs[1], bufs[2], dw, None, ds)
        eng.sync()
        out = (dw.download((RK, len(ranks), L), eng.w_dtype), None, ds.download((RK,), np.int32))
        for b in bufs + [dw, ds]:
            b.free()
    eng.close()
    return out


@pytest.fixture(scope="module")
def rank_reference():
    XB, XD, d = rank_bins()
    good = np.arange(RK) != RK_BAD
    w_ref, lam_ref, _ = subband.update(XB[good], XD[good], d[good], MU, SINGLES, reg=REG)
    RD = subband.correlate(XB[good], XD[good], d[good])[1] + REG * np.eye(L)
    return XB, XD, d, good, w_ref, lam_ref, f32_bounds(RD)


@pytest.mark.gpu
@pytest.mark.parametrize("with_lam", [True, False], ids=["lam", "no_lam"])
@pytest.mark.parametrize("out_c128", [False, True], ids=["c64", "c128"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rank_lists(Engine, rank_reference, dtype, out_c128, with_lam):
    XB, XD, d, good, w_ref, lam_ref, (b_lam, b_w) = rank_reference
    single = {V: launch(Engine, XB, XD, d, (V,), dtype, out_c128, with_lam) for V in SINGLES}
    # a c64 output adds the rounding of the float64 filter to float32: 2^-24 relative in every element, so in the norm
    w_tol = TOL["f64"]["w"] + (0.0 if out_c128 else 2.0 ** -24)
    for ranks in RANK_LISTS:
        w, lam, status = single[ranks[0]] if len(ranks) == 1 else launch(Engine, XB, XD, d, ranks, dtype, out_c128, with_lam)
        assert status[RK_BAD] == 1 and not status[good].any(), (ranks, status)
        assert not w[RK_BAD].any()
        if with_lam:
            assert lam.dtype == (np.float64 if out_c128 else np.float32) and not lam[RK_BAD].any()
            if dtype == "f32":
                assert ((np.abs(lam[good] - lam_ref) / lam_ref[:, :1]).max(axis=1) <= b_lam).all()
            else:
                assert np.abs(lam[good] / lam_ref - 1).max() < TOL["f64"]["lam"] + (0.0 if out_c128 else 2.0 ** -24)
        for t, V in enumerate(ranks):
            ref = w_ref[:, SINGLES.index(V)]
            e_w = np.linalg.norm(w[good, t] - ref, axis=-1) / np.linalg.norm(ref, axis=-1)
            assert (e_w <= (b_w if dtype == "f32" else w_tol)).all(), (ranks, V, e_w.max())
            assert np.array_equal(w[:, t], single[V][0][:, 0]), (ranks, V)
