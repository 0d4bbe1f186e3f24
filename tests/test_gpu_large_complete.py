"""apv_gevd_large's block-cyclic Jacobi (csrc/kernels_gevd_large.hip) as a COMPLETE solver: the spectrum families of
lead_cases.py, which the leading solver answers without ever reaching it, exact ties and trivial pencils, the relative loading
on a batch, a batch whose members need very different numbers of sweeps, sequences of calls on ONE engine (the driver keeps
last_sweeps, captured graph sets and buffers between calls), the per-member status at the sweep cap, the complex entry through
the real embedding, and the rank-list filter step of the stream when the complete solve runs.  Every decomposition is checked
whole by large_cases.check_full (every eigenvalue, orthonormality of all n columns, every residual) against the oracle's jdiag;
test_cpu_large_cases.py holds the oracle itself to a tenth of every bound on the same pencils."""
import functools
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import large_cases as lc  # noqa: E402
from lead_cases import check_pairs  # noqa: E402


@pytest.fixture(scope="module")
def Engine():
    from ap_vast_unofficial_amd import Engine
    return Engine


@functools.lru_cache(maxsize=None)
def _real(family, n, cond_b):
    """(A, B, oracle's lam) of a real case, computed once"""
    A, B, _ = lc.real_case(family, n, cond_b)
    for M in (A, B):
        M.setflags(write=False)
    return A, B, lc.reference(A, B)[1]


@functools.lru_cache(maxsize=None)
def _complex(family, n, cond_b):
    A, B, _ = lc.complex_case(family, n, cond_b)
    for M in (A, B):
        M.setflags(write=False)
    return A, B, lc.reference(A, B)[1]


@functools.lru_cache(maxsize=None)
def _tied(n):
    A, B, lam = lc.tied_diagonal(n)
    for M in (A, B):
        M.setflags(write=False)
    return A, B, lam


def _solve_and_check(eng, members, cond_b, what, complex_=False):
    """one call on `eng` with the batch of `members` [(A, B, lam_ref)]; every member through check_full"""
    A, B = np.stack([m[0] for m in members]), np.stack([m[1] for m in members])
    U, lam = (eng.jdiag_large_complex if complex_ else eng.jdiag_large)(A, B)
    assert U.shape == A.shape and lam.shape == A.shape[:2]
    for z, m in enumerate(members):
        lc.check_full(m[0], m[1], U[z], lam[z], m[2], cond_b, what=f"{what} member {z} of {len(members)}")
    return U, lam


# ---- A. the families on the complete solve ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,n,cond_b", lc.FAMILY_CASES, ids=[f"{lc.IDS[f]}-{n}-{c:g}" for f, n, c in lc.FAMILY_CASES])
def test_family_on_the_complete_solve(Engine, family, n, cond_b):
    """jdiag_large passes no leading rank: the Jacobi runs.  Twelve families at n = 33 (ne = 64, the smallest look-ahead), 96 (no
    ghost rows, three Cholesky panels, a ragged part in the halving), 129 (ne = 160) and 161 (ne = 192); graded at n = 193 with
    cond(B) = 1e6 (ne = 224, seven panels); close pairs and rank 1 at n = 17 and 32 (one pair of blocks)."""
    eng = Engine(1, 4, 4)
    try:
        _solve_and_check(eng, [_real(family, n, cond_b)], cond_b, family)
    finally:
        eng.close()


# ---- B. exact ties and trivial pencils --------------------------------------------------------------------------------------------
def test_exact_ties_on_a_diagonal_pencil(Engine):
    """A = diag with repeated entries in no order, loaded B = I to the bit, n = 40: nothing to rotate.  lam is the sorted diagonal
    exactly (rank_kernel must place tied entries in distinct slots) and U a signed permutation to 1e-15."""
    A, B, lam_ref = _tied(40)
    eng = Engine(1, 4, 4)
    try:
        U, lam = _solve_and_check(eng, [(A, B, lam_ref)], 1e2, "tied diagonal")
    finally:
        eng.close()
    U, lam = U[0], lam[0]
    print("lam - sorted diagonal", np.abs(lam - lam_ref).max())
    assert np.array_equal(lam, lam_ref)
    P = np.sort(np.abs(U), axis=0)
    print("signed permutation: |largest entry| - 1", np.abs(P[-1] - 1).max(), "others", P[:-1].max())
    assert np.abs(P[-1] - 1).max() <= 1e-15 and P[:-1].max() <= 1e-15
    assert sorted(np.abs(U).argmax(axis=0)) == list(range(40))                       # every row is some column's: a permutation
    assert np.array_equal(np.diag(A)[np.abs(U).argmax(axis=0)], lam)                  # and each column sits at its own eigenvalue


@pytest.mark.parametrize("n", lc.TRIVIAL_ORDERS)
def test_zero_and_equal_pencils(Engine, n):
    """A = 0: every eigenvalue exactly zero, U still B-orthonormal.  A = B_lambda: every eigenvalue 1 to 1e-12."""
    eng = Engine(1, 4, 4)
    try:
        _solve_and_check(eng, [lc.zero_pencil(n)], 1e2, "A = 0")
        _, lam = _solve_and_check(eng, [lc.equal_pencil(n)], 1e2, "A = B_lambda")
    finally:
        eng.close()
    print("A = B_lambda: |lam - 1|", np.abs(lam[0] - 1).max())
    assert np.abs(lam[0] - 1).max() <= 1e-12


# ---- C. loading --------------------------------------------------------------------------------------------------------------------
def test_relative_loading_on_a_batch_of_five(Engine):
    """B + 1e-8 ||B||_2 I (apvast.py:26-27) on five pencils of mixed families at n = 96 whose dark matrices carry the factors 1e-8,
    1, 1, 1e+8, 1: the norms arrive in a group of four and a group of one, and each member's loading is its own."""
    from ap_vast_unofficial_amd import _capi
    batch = lc.loading_batch()
    A, B = np.stack([p[0] for p in batch]), np.stack([p[1] for p in batch])
    eng = Engine(1, 4, 4, reg_mode=_capi.REG_REL, reg_dark=1e-8)
    try:
        U, lam = eng.jdiag_large(A, B)
    finally:
        eng.close()
    for z, (family, factor) in enumerate(lc.LOADING_CASES):
        lam_ref = lc.reference(A[z], B[z], rel=True)[1]
        lc.check_full(A[z], B[z], U[z], lam[z], lam_ref, 1e2, rel=True, what=f"relative loading, {family}, B x {factor:g}")


# ---- D. heterogeneous batch --------------------------------------------------------------------------------------------------------
def test_heterogeneous_batch(Engine):
    """Scales 1e-12 and 1e+9, rank 1, flat and noise-like in ONE batch at n = 129: the sweep loop runs until the slowest member
    meets the stop rule, and the members that were done long before must survive the surplus sweeps."""
    eng = Engine(1, 4, 4)
    try:
        _solve_and_check(eng, [_real(f, 129, 1e4) for f in lc.HETEROGENEOUS], 1e4, "heterogeneous")
    finally:
        eng.close()


# ---- E. call sequences on one engine -----------------------------------------------------------------------------------------------
def test_sequence_last_sweeps(Engine):
    """gs.last_sweeps of the call before decides how many sweeps run untested: many (rank 1), one (the diagonal pencil), many
    again, a geometric tail, none to speak of (A = 0), noise-like -- n = 96, batch 1, one engine."""
    seq = [_real("rank 1", 96, 1e2), _tied(96), _real("rank 1", 96, 1e2), _real("geometric 0.9^i", 96, 1e2), _real("zero", 96, 1e2),
           _real("random (noise-like)", 96, 1e2)]
    eng = Engine(1, 4, 4)
    try:
        for i, m in enumerate(seq):
            _solve_and_check(eng, [m], 1e2, f"last_sweeps call {i}")
    finally:
        eng.close()


def test_sequence_graph_set_cache(Engine):
    """GevdLargeWs::set_for keeps the captured sweeps of four batch sizes, and a batch beyond the buffers' capacity releases them
    all.  Sizes 1, 2, 3, 4, 5 at n = 65 (each outgrows the one before: released and captured again every time), 1 and 3 (new sets
    beside 5's), then 2 and 4 (the fifth set evicts the oldest, 5's), 5 (captured again, evicts 1's) and 1 (again, evicts 3's); the
    members are prefixes of one list of five pencils."""
    pencils = [_real(f, 65, 1e2) for f in lc.SEQUENCE_FAMILIES]
    eng = Engine(1, 4, 4)
    try:
        for batch in (1, 2, 3, 4, 5, 1, 3, 2, 4, 5, 1):
            _solve_and_check(eng, pencils[:batch], 1e2, f"graph sets, batch {batch}")
    finally:
        eng.close()


def test_sequence_capacity_and_order(Engine):
    """A smaller batch uses the head of buffers sized for a larger one; another order releases everything: (n, batch) = (96, 3),
    (96, 1), (129, 2), (96, 3)."""
    fam = lc.SEQUENCE_FAMILIES
    P = {96: [_real(f, 96, 1e2) for f in fam[:3]], 129: [_real(f, 129, 1e4) for f in fam[:2]]}
    eng = Engine(1, 4, 4)
    try:
        for n, batch in ((96, 3), (96, 1), (129, 2), (96, 3)):
            _solve_and_check(eng, P[n][:batch], 1e2 if n == 96 else 1e4, f"capacity, n {n} batch {batch}")
    finally:
        eng.close()


def test_sequence_after_an_error(Engine):
    """A dark matrix that is not positive definite at position 1 of 3 raises LinAlgError (apvast.py:21-24); the next call on the
    same engine, a good batch of 3, meets every bound."""
    good = [_real(f, 96, 1e2) for f in lc.SEQUENCE_FAMILIES[:3]]
    A, B = np.stack([m[0] for m in good]), np.stack([m[1] for m in good])
    B[1] = -B[1]
    eng = Engine(1, 4, 4)
    try:
        with pytest.raises(np.linalg.LinAlgError):
            eng.jdiag_large(A, B)
        _solve_and_check(eng, good, 1e2, "after an error")
    finally:
        eng.close()


def test_sequence_interleaved_entries(Engine):
    """jdiag_leading (rank 8), jdiag_large, jdiag_large_complex, jdiag_large on one engine: the leading rank and the caller's
    tolerance are one-shot requests (gl_lead_rank, gl_tol2), so the subspace iteration answers the first call alone (info == 0)
    and the complete solves that follow are complete."""
    g96, r96, c70 = _real("geometric 0.9^i", 96, 1e2), _real("rank 1", 96, 1e2), _complex("pairs (2 % apart)", 70, 1e2)
    eng = Engine(1, 4, 4)
    try:
        U, lam, info = eng.jdiag_leading(g96[0][None], g96[1][None], 8)
        print("jdiag_leading info", info)
        assert (info == 0).all()
        check_pairs(g96[0], g96[1], U[0], lam[0], g96[2], what="leading, rank 8")
        _solve_and_check(eng, [g96], 1e2, "complete after leading")
        _solve_and_check(eng, [c70], 1e2, "complex after complete", complex_=True)
        _solve_and_check(eng, [r96], 1e2, "complete after complex")
    finally:
        eng.close()


# ---- F. per-member status at the sweep cap -------------------------------------------------------------------------------------------
def test_status_per_member_at_the_sweep_cap(Engine):
    """max_sweeps = 1 (the driver runs two sweeps) on the diagonal pencil and a noise-like one at n = 96, through the C entry with a
    status array of the test's own: the call reports no convergence, the status is [0, 2] -- only the member still above the bound
    carries the sweep-cap status -- member 0's copied-back U and lam meet every bound and member 1 is finite.  The capped engine
    then finishes a batch it can finish, and an engine without the cap the batch that failed."""
    from ap_vast_unofficial_amd import _capi
    members = [_tied(96), _real("random (noise-like)", 96, 1e2)]
    A, B = np.ascontiguousarray(np.stack([m[0] for m in members])), np.ascontiguousarray(np.stack([m[1] for m in members]))
    eng = Engine(1, 4, 4, max_sweeps=1)
    try:
        U, lam = np.full_like(A, np.nan), np.full((2, 96), np.nan)
        status = np.full(2, -1, dtype=np.int32)
        rc = eng.lib.apv_jdiag_large(eng.h, 96, 2, _capi._ptr(A), _capi._ptr(B), _capi._ptr(U), _capi._ptr(lam), _capi._ptr(status))
        print("return code", rc, "status", status, eng.lib.apv_last_error(eng.h).decode())
        assert rc == _capi.ERR_NO_CONVERGE
        assert status.tolist() == [0, 2]
        lc.check_full(A[0], B[0], U[0], lam[0], members[0][2], 1e2, what="capped, member 0")
        assert np.isfinite(U[1]).all() and np.isfinite(lam[1]).all()
        with pytest.raises(np.linalg.LinAlgError, match="did not converge"):
            eng.jdiag_large(A, B)
        _solve_and_check(eng, [members[0], members[0]], 1e2, "capped engine, the diagonal pencil twice")
    finally:
        eng.close()
    eng = Engine(1, 4, 4)
    try:
        _solve_and_check(eng, members, 1e2, "without the cap")
    finally:
        eng.close()


# ---- G. complex path -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,n,cond_b", lc.COMPLEX_CASES, ids=[f"{lc.IDS[f]}-{n}-{c:g}" for f, n, c in lc.COMPLEX_CASES])
def test_complex_family(Engine, family, n, cond_b):
    """jdiag_large_complex on Hermitian pencils of order 70 and 97 (real embeddings of order 140 and 194: ne = 160 and 224): every
    eigenvalue of the embedding is double, so the selection of n columns independent over C is at work in every case."""
    eng = Engine(1, 4, 4)
    try:
        _solve_and_check(eng, [_complex(family, n, cond_b)], cond_b, "complex " + family, complex_=True)
    finally:
        eng.close()


def test_complex_batch_of_mixed_families(Engine):
    eng = Engine(1, 4, 4)
    try:
        _solve_and_check(eng, [_complex(f, 70, 1e2) for f in ("rank 1", "scale 1e+9", "cluster of 6 at the top")], 1e2,
                         "complex batch", complex_=True)
    finally:
        eng.close()


# ---- H. the rank-list filter step inside the complete solve ----------------------------------------------------------------------------
@pytest.mark.parametrize("dialect", ["python", "matlab"])
def test_stream_filters_from_the_complete_solve(golden, dialect):
    """A broadband stream on G1's configuration with max_sweeps = 30 (the default cap, but a caller's own: the hop goes to the
    complete solve, whose coef_kernel / vast_prefix_kernel form the filters from the stream's rank list) against the same
    stream without it (the leading route), three hops: every rank's w_A / w_B to 1e-8 of the filter's norm (test_gpu_leading.py's
    tolerance on filters), the leading eight eigenvalues to 1e-9, also against LAPACK.  The Python dialect's constructor takes a count, so its list
    is the default 1..8; the MATLAB dialect's takes a list, and gets the non-contiguous (1, 3, 8)."""
    from ap_vast_unofficial_amd.apvast import ConvergenceWarning, apvast
    g, rirs = golden("g1_broadband_cfg1"), golden("rirs_cfg1")
    H = 128
    ranks = 8 if dialect == "python" else [1, 3, 8]
    n_ranks = 8 if dialect == "python" else 3

    def mk(**kw):
        ap = apvast(256, rirs["rirA"], rirs["rirB"], 32, 16, 0, 0, ranks, 1.0, 512, hop_size=H, perceptual=False, mode="broadband",
                    seed=0, dialect=dialect, **kw)
        ap.set_state({"response": g["init_response"], "target_response": g["init_target_response"]})
        return ap
    full, lead = mk(max_sweeps=30), mk()
    x = g["x"]
    worst = dict(w=0.0, lam=0.0)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error", ConvergenceWarning)
            for h in range(3):
                for ap in (full, lead):
                    ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
                for name in ("w_A", "w_B"):
                    wf, wl = getattr(full, name), getattr(lead, name)
                    assert wf.shape == wl.shape and wf.shape[0] == n_ranks
                    for i in range(n_ranks):
                        worst["w"] = max(worst["w"], np.linalg.norm(wf[i] - wl[i]) / np.linalg.norm(wl[i]))
                for name in ("lambda_A", "lambda_B"):
                    lf, ll = np.asarray(getattr(full, name)), np.asarray(getattr(lead, name))
                    worst["lam"] = max(worst["lam"], np.abs(lf[:8] / ll[:8] - 1).max())
        # reading lambda_* in full makes the leading route complete its eigenpairs with this same solver: the two streams' eigenvalues
        # say little about each other, so the last hop's also face LAPACK on the matrices the object reports (the MATLAB dialect
        # loads both in place, apVast.m:552-569)
        import scipy.linalg
        load = 1e-7 if dialect == "python" else 0.0
        for ap in (full, lead):
            for lam, RX, RY in ((ap.lambda_A, ap.R_A_to_A, ap.R_A_to_B), (ap.lambda_B, ap.R_B_to_B, ap.R_B_to_A)):
                ref = scipy.linalg.eigh(RX, RY + load * np.eye(256), eigvals_only=True)[::-1]
                worst["lapack"] = max(worst.get("lapack", 0.0), np.abs(np.asarray(lam)[:8] / ref[:8] - 1).max())
        print(f"{dialect} dialect, complete solve against the leading route: worst", worst)
        assert full.not_converged == 0
        assert worst["w"] <= 1e-8
        assert worst["lam"] <= 1e-9
        assert worst["lapack"] <= 1e-9
    finally:
        full.close()
        lead.close()
