"""The leading-eigenpair solver (csrc/kernels_gevd_lead.hip) on batches: both product kernels, the per-matrix schedule inside a
batch (members that converge in different passes and ask for filters of different degrees), the batch-size limits, the fall-back of
a whole call, the error path, degenerate bright matrices, the relative loading and caller-set tolerances.  The iteration certifies
its own answer with its own product kernel and hands whatever does not converge to the complete solve, so every test here checks
against the oracle's jdiag, asserts `info`, or compares two routes to the same answer bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from lead_cases import (ROOT, block_width, check_against_oracle, loaded, parse_lead_log, pencil, reference, solve, stack,  # noqa: E402
                        workgroups)

# ---- A. both product kernels ------------------------------------------------------------------------------------------------
# name: n, rank, batch, families of the four distinct pencils
WIDE = {
    "b64": (288, 40, 30, ("graded 1/i", "geometric 0.9^i", "linear", "pairs (2 % apart)")),
    "b32": (544, 8, 31, ("graded 1/i", "geometric 0.9^i", "cluster of 6 at the top", "pairs (2 % apart)")),
}


@pytest.mark.parametrize("name", list(WIDE))
def test_wide_product_kernel_on_a_batch_past_2048_workgroups(name):
    """lead_mult_kernel<2> (16 x 32 outputs, four waves) runs when (ne / 16) (b / 16) batch > 2048 and b % 32 == 0:
      b64: n = 288 (ne = 288), rank 40 -> b = 64, batch 30: 18 * 4 * 30 = 2160 workgroups of 16 x 16
      b32: n = 544 (ne = 544), rank 8  -> b = 32, batch 31: 34 * 2 * 31 = 2108
    Four distinct pencils repeated through the batch: every member meets the oracle bounds (the first copy against the oracle, the
    others bit-identical to it), info == 0 everywhere, and each pencil agrees with its own batch-1 solve -- lead_mult_kernel<1, 8>,
    eight waves and another summation order, so to the oracle's bounds and not to the bit."""
    n, rank, batch, fams = WIDE[name]
    assert workgroups(n, rank, batch) > 2048 and block_width(n, rank) % 32 == 0
    P = [pencil(f, n, 100 + k, 1e3) for k, f in enumerate(fams)]
    order = [z % 4 for z in range(batch)]
    A, B = stack(P, order)
    U, lam, info = solve(A, B, rank)
    print("info", info)
    assert (info == 0).all()
    for k in range(4):
        ref = reference(P[k][0], P[k][1])
        check_against_oracle(P[k][0], P[k][1], U[k], lam[k], ref, what=f"{name} batch member {k}")
        for z in range(k + 4, batch, 4):
            assert np.array_equal(U[z], U[k]) and np.array_equal(lam[z], lam[k]), (z, k)
        U1, lam1, info1 = solve(P[k][0][None], P[k][1][None], rank)
        assert info1[0] == 0
        check_against_oracle(P[k][0], P[k][1], U1[0], lam1[0], ref, what=f"{name} alone {k}")
        assert np.abs(lam[k] / lam1[0] - 1).max() < 1e-9


# ---- B. the schedule within a batch (eight-wave product: <= 2048 workgroups) --------------------------------------------------
# name: n, rank, (family, seed) per member.  The slow families (linear, pairs) stay out of b32: their filters of degree 16 would
# lead every pass, and 15 product steps bring the three rotating buffers back to where they were.
HETERO = {
    "b32": (192, 8, (("geometric 0.9^i", 1), ("graded 1/i", 2), ("cluster of 6 at the top", 3), ("geometric 0.9^i", 11), ("graded 1/i", 12))),
    "b64": (256, 40, (("geometric 0.9^i", 6), ("graded 1/i", 7), ("cluster of 6 at the top", 8), ("linear", 9), ("rank 40 bright matrix", 10))),
}


def hetero_batch(name):
    n, rank, members = HETERO[name]
    P = [pencil(f, n, s) for f, s in members]
    A, B = stack(P, range(len(P)))
    return n, rank, P, A, B


@pytest.mark.parametrize("name", list(HETERO))
def test_heterogeneous_batch_equals_the_members_alone(name):
    """Members of one (n, rank) whose spectra converge in different passes and ask for filters of different degrees (that they do
    is asserted by test_heterogeneous_batch_is_heterogeneous): `active` drops the finished ones, final_buf[z] remembers which of the
    three rotating buffers holds a finished block, a member whose filter is shorter than the batch's longest takes identity steps.
    Every kernel handles matrix z by itself and the identity step is exact (ca == 0 skips the product, fma(1, Yc, 0) copies), so
    each member's U and lam are bit-identical to its batch-1 solve on a fresh engine; and within the oracle's bounds."""
    n, rank, P, A, B = hetero_batch(name)
    U, lam, info = solve(A, B, rank)
    print("info", info)
    assert (info == 0).all()
    for z, (Az, Bz, lz) in enumerate(P):
        check_against_oracle(Az, Bz, U[z], lam[z], reference(Az, Bz), rank_a=int((lz > 0).sum()), what=f"{name} member {z}")
        U1, lam1, info1 = solve(Az[None], Bz[None], rank)
        assert info1[0] == 0
        assert np.array_equal(lam1[0], lam[z]), z
        assert np.array_equal(U1[0], U[z]), (z, np.abs(U1[0] - U[z]).max())


_CHILD = """import sys
sys.path[:0] = [%r, %r]
import test_gpu_leading_batches as t
from lead_cases import solve
n, rank, P, A, B = t.hetero_batch(%r)
U, lam, info = solve(A, B, rank)
print("INFO", *info)
"""


@pytest.mark.parametrize("name", list(HETERO))
def test_heterogeneous_batch_is_heterogeneous(name):
    """Guard against a vacuous test above: the same batch in a fresh process with APV_LEAD_DEBUG=1 (the variable is read once per
    process).  From its log: the members converge in at least two different passes, and after at least one pass two members that
    are still active ask for filters of different degrees.  For final_buf[z] to matter, a filter whose product steps (its degree less
    one) are no multiple of three must run after a member has finished: else the three buffers are back in place and the finished
    block sits where the running one does.  b32 has such a pass.  b64 has not, and is not asked for one: at b >= 48 a pass does one
    Jacobi sweep, every member with a gap needs six passes, and the one that needs seven (rank 40) asks for degree 1."""
    env = dict(os.environ, APV_LEAD_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"), name)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stderr)
    calls = parse_lead_log(r.stderr)
    assert len(calls) == 1 and not calls[0]["full"]
    call = calls[0]
    assert call["batch"] == len(HETERO[name][2]) and sorted(call["converged"]) == list(range(call["batch"]))
    assert "INFO " + " ".join(["0"] * call["batch"]) in r.stdout
    assert len(set(call["converged"].values())) >= 2, call["converged"]
    assert any(len(d) >= 2 and len(set(d.values())) >= 2 for d in call["degrees"].values()), call["degrees"]
    first = min(call["converged"].values())
    rotating = [p for p, d in call["degrees"].items() if p >= first and (max(d.values()) - 1) % 3 != 0]
    print("passes whose filter moves the buffers after a member has finished:", rotating)
    if name == "b32":
        assert rotating


@pytest.fixture(scope="module")
def small_pencils():
    """four pencils of order 96 and their references, shared by the batch-size tests"""
    P = [pencil(f, 96, 40 + k) for k, f in enumerate(("geometric 0.9^i", "graded 1/i", "linear", "pairs (2 % apart)"))]
    return P, [reference(p[0], p[1]) for p in P]


def test_batch_of_32_is_the_full_mask(small_pencils):
    """batch == 32 takes the 0xFFFFFFFF branch of the `active` mask (1u << 32 is undefined): n = 96, rank 8, info == 0, every
    member within the oracle's bounds (copies of one pencil are bit-identical, the first copy is checked against the oracle)."""
    P, refs = small_pencils
    order = [z % 4 for z in range(32)]
    A, B = stack(P, order)
    U, lam, info = solve(A, B, 8)
    print("info", info)
    assert info.shape == (32,) and (info == 0).all()
    for z in range(32):
        k = order[z]
        if z == k:
            check_against_oracle(P[k][0], P[k][1], U[z], lam[z], refs[k], what=f"batch 32 member {z}")
        else:
            assert np.array_equal(U[z], U[k]) and np.array_equal(lam[z], lam[k]), z


def test_batch_of_33_goes_to_the_complete_solve(small_pencils):
    """batch > 32 (LEAD_MAXB) declines the call: info == 1 for all 33, every member within the same bounds."""
    P, refs = small_pencils
    order = [z % 4 for z in range(33)]
    A, B = stack(P, order)
    U, lam, info = solve(A, B, 8)
    print("info", info)
    assert info.shape == (33,) and (info == 1).all()
    for z in range(33):
        k = order[z]
        check_against_oracle(P[k][0], P[k][1], U[z], lam[z], refs[k], what=f"batch 33 member {z}")


def test_flat_member_sends_the_whole_batch_to_the_complete_solve():
    """One member the iteration cannot separate (eigenvalues within 0.1 % of one another) placed last among converging ones: the
    call runs out of passes for it and ALL members come from the complete solve (info == 1), each within the bounds."""
    n, V = 160, 8
    P = [pencil("geometric 0.9^i", n, 50), pencil("graded 1/i", n, 51), pencil("flat", n, 52)]
    A, B = stack(P, range(3))
    U, lam, info = solve(A, B, V)
    print("info", info)
    assert (info == 1).all()
    for z, (Az, Bz, lz) in enumerate(P):
        check_against_oracle(Az, Bz, U[z], lam[z], reference(Az, Bz), what=f"flat batch member {z}")
        assert np.abs(lam[z] / lz[:V] - 1).max() < 1e-9            # the prescribed eigenvalues themselves


def test_indefinite_dark_matrix_inside_a_batch_raises_and_leaves_the_engine_usable():
    """A dark matrix that is not positive definite at position 1 of 3 raises LinAlgError as the reference's cholesky does
    (apvast.py:21-24) -- the factorisation's flags come back with the iteration's first pass, for every member.  The same engine
    then solves a good batch bit-identically to a fresh engine."""
    from ap_vast_unofficial_amd import Engine
    n, V = 128, 8
    P = [pencil("geometric 0.9^i", n, 60), pencil("graded 1/i", n, 61), pencil("linear", n, 62)]
    A, B = stack(P, range(3))
    Bbad = B.copy()
    Bbad[1] = -np.eye(n)
    eng = Engine(1, 4, 4)
    with pytest.raises(np.linalg.LinAlgError):
        eng.jdiag_leading(A, Bbad, V)
    U, lam, info = eng.jdiag_leading(A, B, V)
    eng.close()
    U0, lam0, info0 = solve(A, B, V)
    assert (info == 0).all() and (info0 == 0).all()
    assert np.array_equal(U, U0) and np.array_equal(lam, lam0)
    for z, (Az, Bz, _) in enumerate(P):
        check_against_oracle(Az, Bz, U[z], lam[z], reference(Az, Bz), what=f"after the error, member {z}")


def test_zero_bright_matrix():
    """A = 0: every eigenvalue is zero and any B-orthonormal U is an answer.  The first Ritz value is not positive, so the
    iteration declines after its first pass and the complete solve answers (info == 1).  There is no lambda_1 to scale by: the
    bound on |lambda| is 1e-9 / ||B_lambda||_2, 1e-9 of the smallest leading eigenvalue that a bright matrix of unit norm can have
    with this dark matrix."""
    n, V = 96, 8
    A, B, _ = pencil("zero", n, 70)
    assert not A.any()
    U, lam, info = solve(A[None], B[None], V)
    Bl = loaded(B)
    print("info", info, "max |lam|", np.abs(lam).max(), "orth", np.abs(U[0].T @ Bl @ U[0] - np.eye(V)).max())
    assert np.isfinite(U).all()
    assert np.abs(lam).max() <= 1e-9 / np.linalg.norm(Bl, 2)
    assert np.abs(U[0].T @ Bl @ U[0] - np.eye(V)).max() < 1e-10


@pytest.mark.parametrize("family,n,rank_a", [("rank 1", 96, 1), ("rank 20", 128, 20)], ids=["rank1", "rank20"])
def test_rank_deficient_bright_matrix(family, n, rank_a):
    """A of rank 1 and of rank 20 at b = 32, V = 8: theta_b is zero to rounding, the damped interval's upper end is clamped to
    1e-12 theta_1 and the guard columns carry no direction the filter can amplify.  Correctness only: the non-zero eigenvalues to
    1e-9 relative, the zero ones to 1e-9 lambda_1 absolutely, B-orthonormality and residuals; the projector where V <= rank(A)
    leaves a gap.  Which solver answered is printed and recorded in profiles/r18/README.md (rank 1: the complete solve; rank 20:
    the subspace iteration)."""
    V = 8
    A, B, _ = pencil(family, n, 71)
    U, lam, info = solve(A[None], B[None], V)
    print(family, "info", info)
    check_against_oracle(A, B, U[0], lam[0], reference(A, B), rank_a=rank_a, what=family)


def test_relative_loading_on_a_batch_of_five():
    """reg_mode = REL loads the dark matrix with 1e-8 ||B||_2 (apvast.py:26-27); the norms come from apv_launch_norm2 in groups of
    four, so a batch of five has a ragged second group.  Against the oracle's jdiag with the same loading."""
    from ap_vast_unofficial_amd import _capi
    n, V = 128, 8
    fams = ("geometric 0.9^i", "graded 1/i", "linear", "pairs (2 % apart)", "cluster of 6 at the top")
    P = [pencil(f, n, 80 + k) for k, f in enumerate(fams)]
    for k in range(5):
        P[k] = (P[k][0], P[k][1] * (1.0 + k), P[k][2])           # five different norms
    A, B = stack(P, range(5))
    U, lam, info = solve(A, B, V, reg_mode=_capi.REG_REL, reg_dark=1e-8)
    print("info", info)
    assert (info == 0).all()
    for z, (Az, Bz, _) in enumerate(P):
        check_against_oracle(Az, Bz, U[z], lam[z], reference(Az, Bz, rel=True), rel=True, what=f"relative loading, member {z}")


@pytest.mark.parametrize("engine_args", [{"sweep_tol2": 1e-20}, {"max_sweeps": 30}], ids=["sweep_tol2", "max_sweeps"])
def test_caller_tolerances_ask_for_the_complete_solve(engine_args):
    """A caller who sets a sweep tolerance or a sweep cap is asking for the Jacobi iteration they belong to: info == 1, same
    bounds."""
    n, V = 96, 8
    A, B, _ = pencil("geometric 0.9^i", n, 90)
    U, lam, info = solve(A[None], B[None], V, **engine_args)
    print("info", info)
    assert info[0] == 1
    check_against_oracle(A, B, U[0], lam[0], reference(A, B), what=str(engine_args))
    U0, lam0, info0 = solve(A[None], B[None], V)
    assert info0[0] == 0
