"""The per-bin span at kernel level: Engine.update (fused slabs) and Engine.gevd_vast (explicit statistics) with a mu profile, a
rank cap and a contrast floor against tests/span_oracle.py, on every per-bin kernel.

K = 37 bins (odd: tails and grouped layouts), every rank 1..L, profiles whose 37 values are all distinct (m_k = 0.25 + 0.1 k,
cap_k = 1 + (7 k mod L)) and whose second rows differ from the first, so that a slip in the bin or the row shows.

Bounds: w and lambda at TOL[dtype] of tests/test_gpu_stream.py (orders up to 64, as tests/test_gpu_orders_17_to_64.py uses it) and at
lambda 1e-9, w 1e-7 (order 96, tests/test_gpu_order128.py); the contrast curve within TOL[dtype]["lam"] of the bin's lambda_1.  The
rank is an integer and is compared exactly."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::ap_vast_unofficial_amd._capi.ConvergenceWarning")]
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import subband  # noqa: E402  (checker only)
from span_oracle import span_gevd_vast  # noqa: E402
from test_gpu_stream import TOL  # noqa: E402

K, MU, REG = 37, 1.0, 1e-7
CASES = [(16, 32, "f64", True), (16, 32, "f64", False), (16, 32, "f32", True), (16, 32, "f32", False),   # order-16 kernel
         (24, 48, "f64", True), (24, 48, "f32", True),                                                   # LDS kernel
         (64, 128, "f64", True),                                                                         # order-64 kernel
         (96, 192, "f64", True)]                                                                         # kernels_gevd128.hip


def _tol(L, dtype):
    return dict(w_med=1e-7, w_max=1e-7, lam=1e-9) if L > 64 else TOL[dtype]


def _profiles(L):
    k = np.arange(K)
    m = 0.25 + 0.1 * k
    cap = 1 + (7 * k) % L
    return np.stack([m, m[::-1]]), np.stack([cap, cap[::-1]]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _inputs(L, M, dtype, fused):
    """Slabs (complex64, as Engine.update takes them) and the statistics the oracle solves: those of the slabs, or -- explicit launch --
    the matrices rounded to the engine's input type, which the device then reads bit for bit."""
    rng = np.random.default_rng(100 * L + M)

    def cn(*s):
        return ((rng.standard_normal(s) + 1j * rng.standard_normal(s)) * np.sqrt(0.5)).astype(np.complex64)
    XB, XD, d = cn(K, M, L), cn(K, M, L), cn(K, M)
    RB, RD, r = subband.correlate(XB, XD, d)
    if not fused and dtype == "f32":
        RB, RD, r = (a.astype(np.complex64).astype(np.complex128) for a in (RB, RD, r))
    for a in (XB, XD, d, RB, RD, r):
        a.flags.writeable = False
    return XB, XD, d, RB, RD, r


@functools.lru_cache(maxsize=None)
def _oracle(L, M, dtype, fused, floor):
    """(w, lam, rank, contrast, floor_db) of the oracle with the profiles, once per case; floor: the median of c_{L/2} over the bins"""
    RB, RD, r = _inputs(L, M, dtype, fused)[3:]
    m, cap = _profiles(L)
    ranks = list(range(1, L + 1))
    if not floor:
        return span_gevd_vast(RB, RD, r, MU, ranks, REG, m[0], cap[0], None) + (None,)
    con = _oracle(L, M, dtype, fused, False)[3]            # the curve does not depend on cap or floor
    floor_db = float(10.0 * np.log10(np.median(con[:, L // 2 - 1])))
    return span_gevd_vast(RB, RD, r, MU, ranks, REG, m[0], cap[0], floor_db) + (floor_db,)


def _engine(L, M, dtype, **span):
    from ap_vast_unofficial_amd import Engine
    return Engine(K, L, M, ranks=tuple(range(1, L + 1)), mu=MU, compute_dtype=dtype, reg_dark=REG, span=span or None)


def _launch(eng, L, M, dtype, fused):
    XB, XD, d, RB, RD, r = _inputs(L, M, dtype, fused)
    w, lam, status = eng.update(XB, XD, d) if fused else eng.gevd_vast(RB, RD, r)
    assert not status.any(), status
    return w.astype(np.complex128), lam.astype(np.float64)


def _check_w_lam(tag, w, lam, wr, lr, tol):
    err = np.linalg.norm(w - wr, axis=-1) / np.linalg.norm(wr, axis=-1)
    lerr = np.abs(lam - lr).max(axis=1) / lr[:, 0]
    print(f"{tag}: w median {np.median(err):.1e} max {err.max():.1e} lambda {lerr.max():.1e}")
    assert np.median(err) < tol["w_med"] and err.max() < tol["w_max"], (np.median(err), err.max())
    assert lerr.max() < tol["lam"], lerr.max()


@pytest.mark.parametrize("L,M,dtype,fused", CASES)
def test_profile_and_cap_vs_oracle(L, M, dtype, fused):
    m, cap = _profiles(L)
    wr, lr, rank_r, _, _ = _oracle(L, M, dtype, fused, False)
    eng = _engine(L, M, dtype, mu_profile=m, rank_cap=cap)
    w, lam = _launch(eng, L, M, dtype, fused)
    rank, con = eng.span(0)
    eng.close()
    assert con is None
    assert np.array_equal(rank, np.minimum(L, cap[0])) and np.array_equal(rank, rank_r)
    _check_w_lam(f"{L} x {M} {dtype} {'fused' if fused else 'explicit'}", w, lam, wr, lr, _tol(L, dtype))
    # slots past the cap repeat the bin's solution bit for bit
    for k in range(K):
        for t in range(cap[0, k], L):
            assert np.array_equal(w[k, t], w[k, cap[0, k] - 1]), (k, t)


@pytest.mark.parametrize("L,M,dtype,fused", CASES)
def test_contrast_floor_vs_oracle(L, M, dtype, fused):
    m, cap = _profiles(L)
    _, lr, rank_r, con_r, floor_db = _oracle(L, M, dtype, fused, True)
    eng = _engine(L, M, dtype, mu_profile=m, rank_cap=cap, contrast_floor_db=floor_db)
    w, lam = _launch(eng, L, M, dtype, fused)
    rank, con = eng.span(0)
    eng.close()
    tol = _tol(L, dtype)
    phi = 10.0 ** (floor_db / 10.0)
    # the rank is the prefix count of the device's own curve (at least 1) under the cap, exactly
    f = np.maximum(np.cumprod(con >= phi, axis=1).sum(axis=1), 1)
    assert np.array_equal(rank, np.minimum(cap[0], f))
    # the curve against the oracle's, relative to the bin's largest eigenvalue
    share = (np.abs(con - con_r).max(axis=1) / lr[:, 0]).max() / tol["lam"]
    print(f"{L} x {M} {dtype} {'fused' if fused else 'explicit'}: floor {floor_db:.2f} dB, ranks {rank.min()}..{rank.max()}, "
          f"{(rank != rank_r).sum()} of {K} bins differ from the oracle's rank, contrast at {share:.2e} of its bound")
    assert share <= 1.0, share
    # the filters against the oracle's at the device's rank
    RB, RD, r = _inputs(L, M, dtype, fused)[3:]
    wr = span_gevd_vast(RB, RD, r, MU, list(range(1, L + 1)), REG, m[0], rank, None)[0]
    _check_w_lam("  filters at the device's rank", w, lam, wr, lr, tol)


def test_second_row_is_program_b_and_absent_parts_change_nothing():
    """Engine.update reads row 0 of the tables; a span of ones, cap L and a floor far below every contrast is the plain launch bit for bit."""
    L, M, dtype = 16, 32, "f64"
    XB, XD, d = _inputs(L, M, dtype, True)[:3]
    plain = _engine(L, M, dtype)
    w0, lam0, _ = plain.update(XB, XD, d)
    from ap_vast_unofficial_amd._capi import ApvError
    with pytest.raises(ApvError):
        plain.span(0)
    plain.close()
    eng = _engine(L, M, dtype, mu_profile=np.ones((2, K)), rank_cap=np.full((2, K), L), contrast_floor_db=-300.0)
    w1, lam1, _ = eng.update(XB, XD, d)
    rank, con = eng.span(0)
    assert np.array_equal(w0, w1) and np.array_equal(lam0, lam1)
    assert (rank == L).all() and con.shape == (K, L) and (con[:, 0] <= lam1[:, 0] * (1 + 1e-12)).all()
    # later calls change the values of the parts that exist, and only those
    with pytest.raises(ApvError):
        eng.set_span(mu_profile=np.ones((2, K)), rank_cap=np.full((2, K), L))
    with pytest.raises(ApvError):
        eng.set_span(mu_profile=-np.ones((2, K)), rank_cap=np.full((2, K), L), contrast_floor_db=-300.0)
    with pytest.raises(ApvError):
        eng.set_span(mu_profile=np.ones((2, K)), rank_cap=np.full((2, K), L + 1), contrast_floor_db=-300.0)
    eng.set_span(mu_profile=np.full((2, K), 2.0), rank_cap=np.full((2, K), 3), contrast_floor_db=-300.0)
    w2, _, _ = eng.update(XB, XD, d)
    eng.set_mu(0.5)                       # mu_eff is re-formed from the profile the library keeps: 0.5 * 2 = the plain mu
    w3, _, _ = eng.update(XB, XD, d)
    assert (eng.span(0)[0] == 3).all()
    eng.close()
    assert not np.array_equal(w2[:, :3], w0[:, :3])
    assert np.array_equal(w3[:, :3], w0[:, :3]) and np.array_equal(w3[:, 3:], np.repeat(w0[:, 2:3], L - 3, axis=1))


def test_order_64_two_bins_per_workgroup():
    """K = 513 bins at 64 x 72: from 512 problems on the order-64 launch goes to the kernel that solves two bins per workgroup (here 256
    pairs and one odd bin).  Profiles, cap and floor against the oracle on the bins of the first pairs, a middle pair and the odd
    bin; ranks (2, 5, 64)."""
    from ap_vast_unofficial_amd import Engine
    L, M, Kx, ranks = 64, 72, 513, (2, 5, 64)
    rng = np.random.default_rng(6472)

    def cn(*s):
        return ((rng.standard_normal(s, dtype=np.float32) + 1j * rng.standard_normal(s, dtype=np.float32)) * np.float32(np.sqrt(0.5))).astype(np.complex64)
    XB, XD, d = cn(Kx, M, L), cn(Kx, M, L), cn(Kx, M)
    k = np.arange(Kx)
    m = np.stack([0.25 + 0.01 * k, np.ones(Kx)])
    cap = np.stack([1 + (7 * k) % L, np.full(Kx, L)]).astype(np.int32)
    pick = np.array([0, 1, 2, 3, 256, 257, 511, 512])
    RB, RD, r = subband.correlate(XB[pick], XD[pick], d[pick])
    con0 = span_gevd_vast(RB, RD, r, MU, list(ranks), REG, m[0, pick], cap[0, pick], None)[3]
    floor_db = float(10.0 * np.log10(np.median(con0[:, L // 2 - 1])))
    wr, lr, rank_r, con_r = span_gevd_vast(RB, RD, r, MU, list(ranks), REG, m[0, pick], cap[0, pick], floor_db)
    eng = Engine(Kx, L, M, ranks=ranks, mu=MU, compute_dtype="f64", reg_dark=REG,
                 span=dict(mu_profile=m, rank_cap=cap, contrast_floor_db=floor_db))
    w, lam, status = eng.update(XB, XD, d)
    rank, con = eng.span(0)
    eng.close()
    assert not status.any()
    phi = 10.0 ** (floor_db / 10.0)
    f = np.maximum(np.cumprod(con >= phi, axis=1).sum(axis=1), 1)
    assert np.array_equal(rank, np.minimum(cap[0], f))                                   # every bin, pairs and the odd one
    decided = ~(np.abs(con_r - phi) <= 1e-9 * lr[:, :1]).any(axis=1)
    assert np.array_equal(rank[pick][decided], rank_r[decided])
    assert (np.abs(con[pick] - con_r).max(axis=1) / lr[:, 0]).max() <= TOL["f64"]["lam"]
    wr = span_gevd_vast(RB, RD, r, MU, list(ranks), REG, m[0, pick], rank[pick], None)[0]
    _check_w_lam("64 x 72 f64, two bins per workgroup", w[pick].astype(np.complex128), lam[pick].astype(np.float64), wr, lr, TOL["f64"])
