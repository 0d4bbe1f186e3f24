"""The tail of the order-16 kernel (kernels_gevd16m.hip) forms the filter without the product X = W^H Q: g = W r, the coefficients
a_i = (q_i^H g) / (lam_i + mu), y_V = sum_{i < V} a_i q_i carried from rank to rank and w_V = W^H y_V, one matrix-vector product per
rank.  X itself is formed at the very end and only for a caller that asks for the eigenvectors U.

  parity       fused entry (Engine.update, c64 slabs) and built pairs (Engine.gevd_vast) against the complex128 oracle at the bounds
               of tests/test_gpu_parity.py as that file applies them (TOL; with M < L the loading is 1e-2, only ranks up to M are
               compared and float32 gets the factors 10 / 30 of test_update_vs_oracle), float64 and float32 arithmetic, M in
               {1, 8, 32, 33}, the rank lists (1,), (8,), (16,), (1 .. 16), (3, 9), with and without a lam buffer.
  bits         a rank taken from a list launch is its single-rank launch bit for bit.  A list with a repeated rank, (3, 3, 9), is
               refused when the handle is made ("ranks must be ascending", held here); the one way a launch takes the same rank
               twice is a rank cap, so (3, 5, 9) under a cap of 3 in every other bin stands in for it: the capped bins repeat the
               bits of rank 3 in all three slots, the others are the launch without a cap bit for bit.
  U            through jdiag_batched (the only kernel-level entry that returns U; it returns no filter, so "the filter's bits do
               not depend on U" is a property of the source: the filter is stored before the branch that forms X): U^H (B + reg) U = I,
               U^H A U = diag(lam), and every column's projector u u^H against the oracle's.
  stream       16 loudspeakers x 8 microphones, 257 bins: process_signal (the launch that covers the hops of a chunk, c128 slabs
               in float64, c64 slabs in "mixed" and float32) against the hop loop, bit for bit.
  span         contrast floor, rank cap and mu profile: span_rank and span_contrast against tests/span_oracle.py, the filters
               against the oracle at the ranks chosen, at the bounds of tests/test_gpu_span_kernels.py.
  status 1     bins whose X_D is zero under a zero loading (pivot 0): zero filters and eigenvalues, the neighbours bit for bit
               what a launch without those bins gives.
  sweeps       a bright matrix of rank 8 and an exact double eigenvalue (built pairs): bins the pre-solve does not vouch for, so the
               sweeps paths feed the same tail.

Checked once on a scratch build with g taken as W^H r in place of W r: all 24 parity cases, both span cases, both status-1 cases
(the neighbours' parity) and both rank-8 sweeps cases fail; the double-eigenvalue cases pass there because their R_D = I makes W a
real multiple of I (W^H = W), and the U, repeated-rank and stream cases pass because they compare two launches of the same build.
Run on the MI355X box with `-m gpu`."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

from oracle import gevd, subband  # noqa: E402  (checker only)
from presolve_cases import cn, rel_w, with_spectrum  # noqa: E402
from span_oracle import span_gevd_vast  # noqa: E402
from test_gpu_parity import TOL  # noqa: E402
from test_gpu_stream import TOL as SPAN_TOL  # noqa: E402  (the bounds tests/test_gpu_span_kernels.py holds the span launches to)

L, MU = 16, 0.7
K_BY_M = {1: 5, 8: 9, 32: 37, 33: 11}
RANK_LISTS = [(1,), (8,), (16,), tuple(range(1, 17)), (3, 9)]
ALL = list(range(1, 17))


def _engine(*a, **kw):
    from ap_vast_unofficial_amd import Engine
    return Engine(*a, **kw)


def _reg(M):
    return 1e-7 if M >= L else 1e-2          # test_gpu_parity.test_update_vs_oracle: a singular dark matrix is loaded visibly


@functools.lru_cache(maxsize=None)
def _case(M):
    """slabs, their statistics and the oracle's filters at every rank 1 .. 16 (shared, read-only)"""
    K = K_BY_M[M]
    rng = np.random.default_rng(5200 + M)
    XB, XD, d = cn(rng, K, M, L), cn(rng, K, M, L), cn(rng, K, M)
    RB, RD, r = subband.correlate(XB, XD, d)
    w_ref, lam_ref, st = subband.gevd_vast(RB, RD, r, MU, ALL, reg=_reg(M))
    assert not st.any()
    for a in (XB, XD, d, RB, RD, r, w_ref, lam_ref):
        a.setflags(write=False)
    return XB, XD, d, RB, RD, r, w_ref, lam_ref


def _launch(M, ranks, dtype, fused, with_lam=True):
    XB, XD, d, RB, RD, r = _case(M)[:6]
    K = K_BY_M[M]
    eng = _engine(K, L, M, ranks=ranks, mu=MU, compute_dtype=dtype, reg_dark=_reg(M))
    try:
        if not fused:
            if dtype == "f32":          # the device reads the matrices as complex64
                RB, RD, r = (a.astype(np.complex64) for a in (RB, RD, r))
            return eng.gevd_vast(RB, RD, r)
        if with_lam:
            return eng.update(XB, XD, d)
        bufs = [eng.to_device(a) for a in (XB, XD, d)]
        dw, ds = eng.alloc(K * len(ranks) * L * np.dtype(eng.w_dtype).itemsize), eng.alloc(K * 4)
        eng.update_dev(bufs[0], bufs[1], bufs[2], dw, None, ds)
        eng.sync()
        out = (dw.download((K, len(ranks), L), eng.w_dtype), None, ds.download((K,), np.int32))
        for b in bufs + [dw, ds]:
            b.free()
        return out
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _single(M, V, dtype, fused, with_lam):
    return _launch(M, (V,), dtype, fused, with_lam)


def _check_parity(tag, M, ranks, dtype, w, lam, status):
    w_ref, lam_ref = _case(M)[6:]
    assert not status.any(), status
    nz = min(L, M)                                   # beyond rank(R_B) the eigenvalues are rounding noise
    loose = dtype == "f32" and M < L
    tl, tw = TOL[dtype]["lam"] * (10 if loose else 1), TOL[dtype]["w"] * (30 if loose else 1)
    if lam is not None:
        e_lam = (np.abs(lam[:, :nz] - lam_ref[:, :nz]) / lam_ref[:, :1]).max()
        assert e_lam < tl, (tag, e_lam)
        if M >= L:
            assert np.abs(lam / lam_ref - 1).max() < TOL[dtype]["lam"], tag
    good = [t for t, V in enumerate(ranks) if V <= nz]
    if good:
        e_w = rel_w(w[:, good], w_ref[:, [ranks[t] - 1 for t in good]])
        print(f"{tag}: w {e_w:.2e} (bound {tw:.0e})")
        assert e_w < tw, (tag, e_w)


# (the built-pair entry always returns lam: it has no form without)
@pytest.mark.parametrize("fused,with_lam", [(True, True), (True, False), (False, True)], ids=["fused-lam", "fused-no_lam", "built-lam"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("M", [1, 8, 32, 33])
def test_parity_and_bits(M, dtype, fused, with_lam):
    for ranks in RANK_LISTS:
        w, lam, status = _launch(M, ranks, dtype, fused, with_lam)
        _check_parity(f"M={M} {dtype} {'fused' if fused else 'built'} {ranks}", M, ranks, dtype, w, lam, status)
        for t, V in enumerate(ranks):
            if V in (1, 3, 8, 9, 16):
                assert np.array_equal(w[:, t], _single(M, V, dtype, fused, with_lam)[0][:, 0]), (ranks, V)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_repeated_rank(dtype):
    from ap_vast_unofficial_amd._capi import ApvError
    M, K = 32, K_BY_M[32]
    XB, XD, d = _case(M)[:3]
    with pytest.raises(ApvError, match="ascending"):
        _engine(K, L, M, ranks=(3, 3, 9), mu=MU, compute_dtype=dtype, reg_dark=_reg(M))
    cap = np.where(np.arange(K) & 1, 3, L).astype(np.int32)
    eng = _engine(K, L, M, ranks=(3, 5, 9), mu=MU, compute_dtype=dtype, reg_dark=_reg(M), span=dict(rank_cap=cap))
    w, lam, status = eng.update(XB, XD, d)
    rank, _ = eng.span(0)
    eng.close()
    assert not status.any() and np.array_equal(rank, np.minimum(cap, 9))
    w0 = _launch(M, (3, 5, 9), dtype, True)[0]
    odd = (np.arange(K) & 1).astype(bool)
    assert np.array_equal(w[~odd], w0[~odd])
    for t in range(3):
        assert np.array_equal(w[odd, t], w0[odd, 0]), t
    assert np.array_equal(w0[:, 0], _single(M, 3, dtype, True, True)[0][:, 0])


# ---------------------------------------------------------------------------------------------------------------------------
# U
# ---------------------------------------------------------------------------------------------------------------------------
def test_U_is_the_product_in_descending_order():
    rng = np.random.default_rng(5301)
    batch, n = 7, L
    Y = rng.standard_normal((batch, 2 * n, n)) + 1j * rng.standard_normal((batch, 2 * n, n))
    Z = rng.standard_normal((batch, 2 * n, n)) + 1j * rng.standard_normal((batch, 2 * n, n))
    A = np.einsum("kmi,kmj->kij", Y.conj(), Y)
    B = np.einsum("kmi,kmj->kij", Z.conj(), Z)
    eng = _engine(1, 4, 4)
    U, lam = eng.jdiag_batched(A, B)
    eng.close()
    for k in range(batch):
        U0, lam0 = gevd.jdiag(A[k], B[k])
        Bl = B[k] + 1e-7 * np.eye(n)
        # the bounds of test_gpu_parity.test_jdiag_batched_invariants
        assert np.abs(U[k].conj().T @ Bl @ U[k] - np.eye(n)).max() < 1e-11
        assert np.abs(U[k].conj().T @ A[k] @ U[k] - np.diag(lam[k])).max() < 1e-10 * lam[k, 0]
        assert (np.diff(lam[k]) <= 0).all() and np.abs(lam[k] / lam0 - 1).max() < 1e-9
        # column by column, free of the column's phase: u u^H against the oracle's, relative, at the filters' bound
        for c in range(n):
            P, P0 = np.outer(U[k][:, c], U[k][:, c].conj()), np.outer(U0[:, c], U0[:, c].conj())
            assert np.linalg.norm(P - P0) < TOL["f64"]["w"] * np.linalg.norm(P0), (k, c)


# ---------------------------------------------------------------------------------------------------------------------------
# stream: the launch that covers the hops of a chunk
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "mixed", "f32"])
def test_stream_16x8_257_bins_equals_hop_loop(dtype):
    from ap_vast_unofficial_amd.apvast import apvast
    from test_gpu_stream import _hop_loop, synth_rirs
    N, H, n_hops, V = 512, 256, 17, 3                       # 257 bins; a chunk of 16 hops and one more
    rirA, rirB = synth_rirs(300, L, 8, 11)
    mk = lambda: apvast(N, rirA, rirB, 16, 5, 1, 2, V, 1.0, 4 * N, hop_size=H, seed=3, dtype=dtype, perceptual=False)
    a, b = mk(), mk()
    x = np.random.default_rng(8).standard_normal((2, n_hops * H))
    ref = _hop_loop(a, x, 0, n_hops)
    got = list(b.process_signal(x[0], x[1]))
    assert b.signal_schedule == (n_hops, 0)                 # every hop went through the chunked schedule
    for q in range(4):
        for v in range(len(ref[q])):
            assert np.array_equal(got[q][v], ref[q][v]), (q, v)
    for z in "AB":
        assert np.array_equal(getattr(a, "w_" + z), getattr(b, "w_" + z)), z
        assert np.array_equal(getattr(a, "lambda_" + z), getattr(b, "lambda_" + z)), z
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------
# span
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_span_launch(dtype):
    M, K = 32, K_BY_M[32]
    XB, XD, d, RB, RD, r = _case(M)[:6]
    k = np.arange(K)
    m, cap = 0.25 + 0.1 * k, (1 + (5 * k) % L).astype(np.int32)
    reg = _reg(M)
    con0 = span_gevd_vast(RB, RD, r, MU, ALL, reg, m, cap, None)[3]
    floor_db = float(10.0 * np.log10(np.median(con0[:, L // 2 - 1])))
    _, lam_r, rank_r, con_r = span_gevd_vast(RB, RD, r, MU, ALL, reg, m, cap, floor_db)
    eng = _engine(K, L, M, ranks=tuple(ALL), mu=MU, compute_dtype=dtype, reg_dark=reg,
                  span=dict(mu_profile=m, rank_cap=cap, contrast_floor_db=floor_db))
    w, lam, status = eng.update(XB, XD, d)
    rank, con = eng.span(0)
    eng.close()
    assert not status.any()
    phi = 10.0 ** (floor_db / 10.0)
    f = np.maximum(np.cumprod(con >= phi, axis=1).sum(axis=1), 1)
    assert np.array_equal(rank, np.minimum(cap, f))                       # the rank is the prefix count of the device's own curve
    tol = SPAN_TOL[dtype]
    decided = ~(np.abs(con_r - phi) <= tol["lam"] * lam_r[:, :1]).any(axis=1)
    assert decided.sum() >= K // 2 and np.array_equal(rank[decided], rank_r[decided])
    assert (np.abs(con - con_r).max(axis=1) / lam_r[:, 0]).max() <= tol["lam"]
    wr = span_gevd_vast(RB, RD, r, MU, ALL, reg, m, rank, None)[0]       # the oracle's filters at the device's rank
    err = np.linalg.norm(w - wr, axis=-1) / np.linalg.norm(wr, axis=-1)
    print(f"span {dtype}: ranks {rank.min()}..{rank.max()}, {int(decided.sum())} of {K} bins decided, w median {np.median(err):.1e} max {err.max():.1e}")
    assert np.median(err) < tol["w_med"] and err.max() < tol["w_max"]
    assert (np.abs(lam - lam_r).max(axis=1) / lam_r[:, 0]).max() < tol["lam"]


# ---------------------------------------------------------------------------------------------------------------------------
# status 1
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_zero_pivot_bins(dtype):
    M, K, ranks = 32, 12, (1, 8, 16)
    rng = np.random.default_rng(5401)
    XB, XD, d = cn(rng, K, M, L), cn(rng, K, M, L), cn(rng, K, M)
    bad = np.zeros(K, bool)
    bad[[0, 5, 6, 11]] = True
    XD[bad] = 0                                             # R_D = 0 and no loading: the first pivot is exactly zero
    eng = _engine(K, L, M, ranks=ranks, mu=MU, compute_dtype=dtype, reg_dark=0.0)
    w, lam, status = eng.update(XB, XD, d, raise_on_status=False)
    eng.close()
    assert np.array_equal(status == 1, bad) and not status[~bad].any(), status
    assert not w[bad].any() and not lam[bad].any()
    assert not (np.signbit(w[bad].real) | np.signbit(w[bad].imag)).any()        # +0, as a launch that skips the bin writes
    good = ~bad
    eng = _engine(int(good.sum()), L, M, ranks=ranks, mu=MU, compute_dtype=dtype, reg_dark=0.0)
    w0, lam0, st0 = eng.update(XB[good], XD[good], d[good])
    eng.close()
    assert not st0.any()
    assert np.array_equal(w[good], w0) and np.array_equal(lam[good], lam0)
    w_ref, lam_ref, _ = subband.update(XB[good], XD[good], d[good], MU, list(ranks), reg=0.0)
    assert np.abs(lam[good] / lam_ref - 1).max() < TOL[dtype]["lam"]
    assert rel_w(w[good], w_ref) < TOL[dtype]["w"]


# ---------------------------------------------------------------------------------------------------------------------------
# sweeps paths
# ---------------------------------------------------------------------------------------------------------------------------
def _sweeps_pairs():
    """built pairs the pre-solve does not vouch for: R_B of rank 8 (eight zero eigenvalues, spread beyond 1e3) and an exact double
    eigenvalue (R_D = I, so the pencil's eigenvalues are R_B's to the loading).  Rank lists that do not split a cluster."""
    rng = np.random.default_rng(5501)
    n = 6
    Y = rng.standard_normal((n, 8, L)) + 1j * rng.standard_normal((n, 8, L))
    Z = rng.standard_normal((n, 32, L)) + 1j * rng.standard_normal((n, 32, L))
    low = (np.einsum("kmi,kmj->kij", Y.conj(), Y), np.einsum("kmi,kmj->kij", Z.conj(), Z), (1, 8, 16))
    lam = np.geomspace(1.0, 0.05, L)
    lam[4] = lam[3]
    dbl = (np.array([with_spectrum(rng, lam) for _ in range(n)]), np.broadcast_to(np.eye(L, dtype=np.complex128), (n, L, L)).copy(),
           (3, 5, 16))
    r = rng.standard_normal((n, L)) + 1j * rng.standard_normal((n, L))
    return {"rank8": low + (r,), "double": dbl + (r,)}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["rank8", "double"])
def test_sweeps_paths_feed_the_tail(name, dtype):
    RB, RD, ranks, r = _sweeps_pairs()[name]
    if dtype == "f32":
        RB, RD, r = (a.astype(np.complex64).astype(np.complex128) for a in (RB, RD, r))      # what the device reads
    reg = 1e-7
    eng = _engine(len(RB), L, 32, ranks=ranks, mu=MU, compute_dtype=dtype, reg_dark=reg)
    w, lam, status = eng.gevd_vast(RB, RD, r)
    eng.close()
    assert not status.any(), status
    w_ref, lam_ref, _ = subband.gevd_vast(RB, RD, r, MU, list(ranks), reg=reg)
    e_lam, e_w = (np.abs(lam - lam_ref) / lam_ref[:, :1]).max(), rel_w(w, w_ref)
    print(f"{name} {dtype}: lam {e_lam:.2e}  w {e_w:.2e}")
    assert e_lam < TOL[dtype]["lam"] and e_w < TOL[dtype]["w"]
