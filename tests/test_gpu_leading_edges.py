"""The leading-eigenpair solver (csrc/kernels_gevd_lead.hip) at the edges of apv_gevd_lead_block and of the padding, across
calls that reuse one engine's workspace, and on the spectrum families of tools/probes/lead_stress.py.  Every case is checked
against the oracle's jdiag with the bounds of test_gpu_leading.py, and `info` is asserted: a case that silently goes to the
complete solve passes every accuracy bound."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from lead_cases import block_width, check_against_oracle, pencil, reference, solve  # noqa: E402


# ---- C. widths and padding --------------------------------------------------------------------------------------------------
def _one(family, n, rank, seed, cond_b=1e2, rank_a=None):
    A, B, lam_true = pencil(family, n, seed, cond_b)
    U, lam, info = solve(A[None], B[None], rank)
    print(f"{family} n={n} rank={rank} cond(B)={cond_b:g}: info {info[0]}")
    check_against_oracle(A, B, U[0], lam[0], reference(A, B), rank_a=rank_a, what=family)
    return int(info[0]), lam[0], lam_true


@pytest.mark.parametrize("rank,b,info", [(16, 32, 0), (17, 48, 0), (32, 48, 0), (33, 64, 0), (56, 64, 0), (57, 0, 1)])
def test_block_width_switches(rank, b, info):
    """Ranks on both sides of the width switches 16|17 (b = 32|48) and 32|33 (48|64) and of the guard-vector limit 56|57 (eight
    guard vectors in a block of 64 | the complete solve), at n = 224: ne = 224, ne mod 128 = 96, a short last slab in
    lead_gram_kernel."""
    assert block_width(224, rank) == b
    got, _, _ = _one("geometric 0.9^i", 224, rank, 200 + rank)
    assert got == info


@pytest.mark.parametrize("n,rank,info", [(95, 8, 1), (96, 8, 0), (143, 20, 1), (144, 20, 0), (191, 40, 1), (192, 40, 0)])
def test_block_is_no_small_part_of_the_matrix(n, rank, info):
    """3 b > n hands the call to the complete solve: n = 95|96 at b = 32, 143|144 at b = 48, 191|192 at b = 64.  (95, 143 and 191
    also have ghost rows.)"""
    assert (block_width(n, rank) == 0) == bool(info)
    got, _, _ = _one("geometric 0.9^i", n, rank, 300 + n)
    assert got == info


@pytest.mark.parametrize("n", [97, 129, 161])
def test_ghost_rows_and_short_slabs(n):
    """n = 97: ne = 128, 31 ghost rows.  n = 129 and 161: ne = 160 and 192, last slabs of 32 and 64 rows in lead_gram_kernel
    (with test_block_width_switches' 96 every remainder of ne mod 128)."""
    got, _, _ = _one("geometric 0.9^i", n, 8, 400 + n)
    assert got == 0


# ---- D. workspace reuse ------------------------------------------------------------------------------------------------------
def test_workspace_reuse_across_calls_on_one_engine():
    """LeadWs is keyed on (ne, b, cap): a smaller batch reuses the buffers of a larger one (strides follow the call, not the
    capacity), another b or ne releases and allocates.  Each call of the sequence is bit-identical to the same call on a fresh
    engine, and the fifth to the first."""
    from ap_vast_unofficial_amd import Engine
    seq = [(192, 8, 3), (192, 8, 1), (192, 20, 2), (257, 20, 2), (192, 8, 3)]
    fams = ("geometric 0.9^i", "graded 1/i", "pairs (2 % apart)")
    P = {n: [pencil(f, n, 500 + n + k) for k, f in enumerate(fams)] for n in (192, 257)}
    refs = {}
    eng = Engine(1, 4, 4)
    got = []
    for n, rank, batch in seq:
        A, B = np.stack([p[0] for p in P[n][:batch]]), np.stack([p[1] for p in P[n][:batch]])
        got.append(eng.jdiag_leading(A, B, rank))
    eng.close()
    for (n, rank, batch), (U, lam, info) in zip(seq, got):
        A, B = np.stack([p[0] for p in P[n][:batch]]), np.stack([p[1] for p in P[n][:batch]])
        U0, lam0, info0 = solve(A, B, rank)
        print(n, rank, batch, "info", info, info0)
        assert (info == 0).all() and (info0 == 0).all()
        assert np.array_equal(U, U0) and np.array_equal(lam, lam0), (n, rank, batch)
        for z in range(batch):
            if (n, z) not in refs:
                refs[n, z] = reference(A[z], B[z])
            check_against_oracle(A[z], B[z], U[z], lam[z], refs[n, z], what=f"call {(n, rank, batch)} member {z}")
    assert np.array_equal(got[4][0], got[0][0]) and np.array_equal(got[4][1], got[0][1])


# ---- E. the stress families ----------------------------------------------------------------------------------------------------
STRESS_FAMILIES = ("graded 1/i", "geometric 0.9^i", "linear", "pairs (2 % apart)", "rank 40 bright matrix", "cluster of 6 at the top",
                   "scale 1e-12", "scale 1e+9", "random (noise-like)")
# n, rank, cond(B): b = 32 at 3 b = n, b = 32 with ghost rows and a short slab, b = 64
STRESS_SHAPES = ((96, 8, 1e2), (129, 16, 1e4), (192, 33, 1e3))
# cond(B) = 1e6, where the oracle itself keeps about 50 x headroom to the bounds: one case per group of families
STRESS_ILL = (("graded 1/i", 96, 8, 1e6), ("cluster of 6 at the top", 129, 16, 1e6), ("scale 1e+9", 192, 33, 1e6))


STRESS_CASES = [(f, *s) for f in STRESS_FAMILIES for s in STRESS_SHAPES] + list(STRESS_ILL)
STRESS_IDS = dict(zip(STRESS_FAMILIES, ("graded", "geometric", "linear", "pairs", "rank40", "cluster6", "scale1e-12", "scale1e+9", "noise")))


@pytest.mark.parametrize("family,n,rank,cond_b", STRESS_CASES, ids=[f"{STRESS_IDS[c[0]]}-{c[1]}-{c[2]}-{c[3]:g}" for c in STRESS_CASES])
def test_stress_family(family, n, rank, cond_b):
    """The nine spectrum families of tools/probes/lead_stress.py -- graded, geometric, linear, close pairs, a bright matrix of rank
    40, a cluster of six at the top, scales 1e-12 and 1e+9, noise-like -- against the oracle and, at cond(B) <= 1e4, the prescribed
    eigenvalues (the construction's rounding moves them by about 1e-16 cond(B) lambda_1).  The subspace iteration answers every
    one of them at these shapes (info == 0; profiles/r18/lead_debug_calls.log holds every call's closing APV_LEAD_DEBUG line): none falls back."""
    seed = 600 + 7 * STRESS_FAMILIES.index(family) + n
    got, lam, lam_true = _one(family, n, rank, seed, cond_b)
    if cond_b <= 1e4:
        e = np.abs(lam / lam_true[:rank] - 1).max()
        print("against the prescribed eigenvalues", e)
        assert e < 1e-9
    assert got == 0
