"""The reference of test_gpu_large_complete.py measured against itself: the oracle's jdiag alone, through large_cases.check_full,
on every (family, n, cond(B), loading) that file hands to the kernels, real and complex, against the PRESCRIBED spectrum (under
the relative loading, where no spectrum is prescribed, against scipy.linalg.eigh).  Every bound is divided by ten here: a case
on which the reference itself keeps less than 10 x headroom has no place in the GPU file.  The worst figures stand in the
docstring of large_cases.py (run with -s to print them)."""
import numpy as np
import pytest

import large_cases as lc

MARGIN = 10.0
WORST = {}            # group -> bound -> (fraction of the bound, case)


def _note(group, what, f):
    w = WORST.setdefault(group, {})
    for k in ("lam", "orth", "res"):
        if f[k] >= w.get(k, (-1.0, ""))[0]:
            w[k] = (f[k], what)


def _oracle(group, A, B, lam_ref, cond_b, rel=False, what=""):
    U, lam = lc.reference(A, B, rel)
    _note(group, what, lc.check_full(A, B, U, lam, lam_ref, cond_b, rel=rel, what="oracle " + what, margin=MARGIN))


@pytest.mark.parametrize("family,n,cond_b", lc.FAMILY_CASES + lc.SEQUENCE_CASES,
                         ids=[f"{lc.IDS[f]}-{n}-{c:g}" for f, n, c in lc.FAMILY_CASES + lc.SEQUENCE_CASES])
def test_oracle_on_real_families(family, n, cond_b):
    A, B, lam = lc.real_case(family, n, cond_b)
    _oracle("real, cond(B) <= 1e4" if cond_b <= 1e4 else "real, cond(B) = 1e6", A, B, lam, cond_b, what=f"{family} n={n}")


@pytest.mark.parametrize("family,n,cond_b", lc.COMPLEX_CASES, ids=[f"{lc.IDS[f]}-{n}-{c:g}" for f, n, c in lc.COMPLEX_CASES])
def test_oracle_on_complex_families(family, n, cond_b):
    A, B, lam = lc.complex_case(family, n, cond_b)
    assert np.iscomplexobj(A) and np.array_equal(A, A.conj().T) and np.array_equal(B, B.conj().T)
    assert np.abs(A.imag).max() > 0 or family == "zero"
    _oracle("complex", A, B, lam, cond_b, what=f"complex {family} n={n}")


@pytest.mark.parametrize("n", lc.TRIVIAL_ORDERS)
def test_oracle_on_trivial_pencils(n):
    for name, make in (("tied diagonal", lc.tied_diagonal), ("A = 0", lc.zero_pencil), ("A = B_lambda", lc.equal_pencil)):
        A, B, lam = make(n)
        _oracle("trivial", A, B, lam, 1e2, what=f"{name} n={n}")
    A, B, lam = lc.tied_diagonal(n)
    U, got = lc.reference(A, B)
    assert np.array_equal(got, lam)
    P = np.abs(U)
    assert np.abs(np.sort(P, axis=0)[-1] - 1).max() <= 1e-15 and np.sort(P, axis=0)[:-1].max() <= 1e-15


def test_oracle_under_relative_loading():
    """B + 1e-8 ||B||_2 I with B scaled by 1e-8, 1, 1, 1e+8, 1: the oracle against LAPACK's generalised solver on the loaded pair."""
    for (family, factor), (A, B) in zip(lc.LOADING_CASES, lc.loading_batch()):
        lam_ref = lc.eigh_reference(A, B, rel=True)
        assert lam_ref[0] > 0 and abs(np.linalg.norm(B, 2) / factor) < 20          # the factor reached the dark matrix
        _oracle("relative loading", A, B, lam_ref, 1e2, rel=True, what=f"{family} B x {factor:g}")


def test_case_lists_are_what_the_gpu_file_needs():
    """twelve families at four shapes less the one that does not fit, the ill-conditioned case, the single-pair orders; seeds that
    depend on (family, n) alone; the complex pencils Hermitian with the prescribed spectrum"""
    assert len(lc.COMPLETE_FAMILIES) == 12 and set(lc.COMPLETE_FAMILIES) <= set(lc.FAMILIES)
    assert len(lc.FAMILY_CASES) == 12 * 4 - 1 + 1 + 4
    assert sum(c > 1e4 for _, _, c in lc.FAMILY_CASES) == 1
    assert lc.seed_of("flat", 96) == lc.seed_of("flat", 96) != lc.seed_of("flat", 97)
    a, b = lc.real_case("flat", 96), lc.real_case("flat", 96)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    A, B, lam = lc.complex_case("pairs (2 % apart)", 70)
    got = lc.eigh_reference(A, B)
    assert np.abs(got - lam).max() < 1e-12 * lam[0]
    for f in lc.HETEROGENEOUS + lc.SEQUENCE_FAMILIES + tuple(x for x, _ in lc.LOADING_CASES) + lc.COMPLEX_FAMILIES:
        assert f in lc.FAMILIES


def test_headroom_table():
    """Prints the worst fraction of each bound per group (the table of large_cases.py's docstring).  Runs last in this file."""
    for group, w in WORST.items():
        print(f"{group}: " + "; ".join(f"{k} {1 / v[0] if v[0] > 0 else float('inf'):.0f} x ({v[1]})" for k, v in w.items()))
        assert all(v[0] * MARGIN <= 1 for v in w.values())
