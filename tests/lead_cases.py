"""What the tests of the leading-eigenpair solver share (test_gpu_leading_batches.py, test_gpu_leading_edges.py): the pencil
construction and the nine spectrum families of tools/probes/lead_stress.py, the bounds of test_gpu_leading.py's _check_pairs, the
oracle's reference and a parser of the APV_LEAD_DEBUG=1 log.  Every pencil is a function of (family, n, seed, cond(B)) alone, so a
test and the child process that logs the same batch see the same matrices."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import gevd  # noqa: E402  (checker only)

LOAD = 1e-7             # jdiag's absolute loading of the dark matrix (apvast.py:24)


def _noise(n):
    return np.sort(np.random.default_rng(2025 + n).chisquare(8, n))[::-1]


# the nine families of tools/probes/lead_stress.py, by the names it prints
FAMILIES = {
    "graded 1/i": lambda n: 10.0 / (1 + np.arange(n)),
    "geometric 0.9^i": lambda n: 0.9 ** np.arange(n),
    "linear": lambda n: np.linspace(5.0, 0.01, n),
    "pairs (2 % apart)": lambda n: np.repeat(np.linspace(8.0, 0.1, (n + 1) // 2), 2)[:n] * np.tile([1.0, 0.98], (n + 1) // 2)[:n],
    "rank 40 bright matrix": lambda n: np.concatenate([np.linspace(3.0, 1.0, 40), np.zeros(n - 40)]),
    "cluster of 6 at the top": lambda n: np.concatenate([np.full(6, 4.0) * (1 + 1e-9 * np.arange(6)), np.linspace(2.0, 0.05, n - 6)]),
    "scale 1e-12": lambda n: 1e-12 * np.linspace(5.0, 0.01, n),
    "scale 1e+9": lambda n: 1e9 / (1 + np.arange(n)) ** 0.5,
    "random (noise-like)": _noise,
}
# spectra of the degenerate bright matrices and of the fall-back
FAMILIES.update({
    "zero": lambda n: np.zeros(n),
    "rank 1": lambda n: np.concatenate([[3.0], np.zeros(n - 1)]),
    "rank 20": lambda n: np.concatenate([np.linspace(3.0, 1.0, 20), np.zeros(n - 20)]),
    "flat": lambda n: 1.0 + 1e-3 * np.linspace(1.0, 0.0, n),            # test_leading_falls_back_on_a_flat_spectrum's
})


def block_width(n, rank):
    """apv_gevd_lead_block: the iteration's block width, 0 where the complete solve answers"""
    b = min(max((rank + 16 + 15) // 16 * 16, 32), 64)
    return 0 if rank <= 0 or b - rank < 8 or 3 * b > n else b


def workgroups(n, rank, batch):
    """16 x 16 output tiles of one block product: the wide product kernel runs beyond 2048 of them when b % 32 == 0"""
    return (n + 31) // 32 * 32 // 16 * (block_width(n, rank) // 16) * batch


def spectrum(family, n):
    return np.sort(np.asarray(FAMILIES[family](n), float))[::-1]


def pencil(family, n, seed, cond_b=1e2):
    """(A, B, lam) with A x_i = lam_i (B + 1e-7 I) x_i for the family's spectrum: B + 1e-7 I = X^-T X^-1 of condition cond_b,
    A = X^-T diag(lam) X^-1 (lead_stress.py's construction, the generator seeded per pencil)."""
    lam = spectrum(family, n)
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d = np.exp(rng.uniform(-0.5 * np.log(cond_b), 0.5 * np.log(cond_b), n) / 2)
    Xi = Q * d[None, :]
    Bl = Xi @ Xi.T
    A = Xi @ np.diag(lam) @ Xi.T
    return 0.5 * (A + A.T), 0.5 * (Bl + Bl.T) - LOAD * np.eye(n), lam


def stack(pencils, order):
    """the batch (A, B) that holds pencils[k] at every position z with order[z] == k"""
    return np.stack([pencils[k][0] for k in order]), np.stack([pencils[k][1] for k in order])


def loaded(B, rel=False):
    n = B.shape[0]
    return B + (gevd.REG_REL * np.linalg.norm(B, 2) if rel else LOAD) * np.eye(n)


def reference(A, B, rel=False):
    """(U, lam) of the oracle's jdiag"""
    return gevd.jdiag(A, B, reg_mode=gevd.REG_MODE_REL if rel else gevd.REG_MODE_ABS)


def check_pairs(A, B, U, lam, lam_ref, rank_a=None, rel=False, what=""):
    """The bounds of test_gpu_leading.py's _check_pairs: eigenvalues to 1e-9 relative, |U^T B_lambda U - I| < 1e-10, residuals
    below 1e-9 ||A||_2 max ||u||.  Eigenvalues from index rank_a on are exactly zero by construction (the reference's are rounding
    noise) and are compared absolutely, against 1e-9 lambda_1.  The figures are printed before they are asserted."""
    n, V = U.shape
    Bl = loaded(B, rel)
    lam_ref = np.asarray(lam_ref)[:V]
    nz = V if rank_a is None else min(V, rank_a)
    e_lam = np.abs(lam[:nz] / lam_ref[:nz] - 1).max() if nz else 0.0
    e_zero = np.abs(lam[nz:]).max() / lam_ref[0] if nz < V else 0.0
    e_orth = np.abs(U.T @ Bl @ U - np.eye(V)).max()
    res = np.linalg.norm(A @ U - (Bl @ U) * lam, axis=0).max()
    bound = 1e-9 * np.linalg.norm(A, 2) * np.linalg.norm(U, axis=0).max()
    print(f"{what} n={n} V={V}: lam {e_lam:.1e} zero {e_zero:.1e} orth {e_orth:.1e} res {res:.1e} (bound {bound:.1e})")
    assert np.isfinite(U).all() and np.isfinite(lam).all()
    assert e_lam < 1e-9
    assert e_zero < 1e-9
    assert e_orth < 1e-10
    assert res < bound


def has_gap(lam_ref, V):
    """the cut below the V-th eigenvalue is a gap: lambda_V - lambda_{V+1} >= 1e-2 lambda_V"""
    return V < len(lam_ref) and lam_ref[V - 1] - lam_ref[V] >= 1e-2 * lam_ref[V - 1]


def check_projector(B, U, Uo, lam_ref, rel=False, what=""):
    """The B-orthogonal projector on the leading subspace against the oracle's, to 1e-8, where the cut has a gap (without one the
    subspace is not defined).  Returns whether it was checked."""
    V = U.shape[1]
    if not has_gap(lam_ref, V):
        return False
    Bl = loaded(B, rel)
    P, Po = U @ U.T @ Bl, Uo[:, :V] @ Uo[:, :V].T @ Bl
    e = np.abs(P - Po).max() / np.abs(Po).max()
    print(f"{what} projector {e:.1e}")
    assert e < 1e-8
    return True


def check_against_oracle(A, B, U, lam, ref, rank_a=None, rel=False, what=""):
    Uo, lam_ref = ref
    check_pairs(A, B, U, lam, lam_ref, rank_a=rank_a, rel=rel, what=what)
    if rank_a is None or rank_a >= U.shape[1]:          # a cut inside the null space of A has no gap, whatever the rounding noise says
        check_projector(B, U, Uo, lam_ref, rel=rel, what=what)


def solve(A, B, rank, **engine_args):
    """jdiag_leading of the batch (A, B) on a fresh engine"""
    from ap_vast_unofficial_amd import Engine
    eng = Engine(1, 4, 4, **engine_args)
    try:
        return eng.jdiag_leading(A, B, rank)
    finally:
        eng.close()


_PASS = re.compile(r"\[apv lead\] pass (\d+) matrix (\d+): .*?( converged)?$")
_DEG = re.compile(r"\[apv lead\]\s+matrix (\d+): next filter of degree (\d+)")
_END = re.compile(r"\[apv lead\] n=(\d+) b=(\d+) rank=(\d+) batch=(\d+): (\d+) passes, (\d+) block products.*?( -> full solve)?$")


def parse_lead_log(text):
    """The calls of an APV_LEAD_DEBUG=1 log: per call a dict with n, b, rank, batch, passes, full (the call went to the complete
    solve), converged {matrix: pass} and degrees {pass: {matrix: degree of the filter that follows the pass}}."""
    calls, conv, deg, cur = [], {}, {}, None
    for line in text.splitlines():
        m = _PASS.search(line)
        if m:
            cur = int(m.group(1))
            if m.group(3):
                conv[int(m.group(2))] = cur
            continue
        m = _DEG.search(line)
        if m:
            deg.setdefault(cur, {})[int(m.group(1))] = int(m.group(2))
            continue
        m = _END.search(line)
        if m:
            n, b, rank, batch, passes = (int(m.group(i)) for i in range(1, 6))
            calls.append(dict(n=n, b=b, rank=rank, batch=batch, passes=passes, full=bool(m.group(7)), converged=conv, degrees=deg))
            conv, deg, cur = {}, {}, None
    return calls
