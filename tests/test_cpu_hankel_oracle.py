"""tests/hankel_oracle.py on its own, without a GPU: the plain reference of the Hankel statistics against the oracles restated
from the reference, one shape per dialect -- apvast.py's skipped sample (oracle.broadband), apVast.m's contiguous matrix
(oracle.broadband_matlab, before its scaling and loading) and vast.m's impulse drive (oracle.static_vast) with the packing
apv_vast_static uses.  Agreement to 1e-13 of the largest entry: both sides are float64 sums of the same products in
different orders."""
import numpy as np
import pytest

import hankel_oracle as ho
from oracle import static_vast
from oracle.broadband import AA, AB, BroadbandOracle, hankel_rows
from oracle.broadband_matlab import MatlabBroadbandOracle

TOL = 1e-13


def close(got, exp):
    return np.abs(got - exp).max() <= TOL * np.abs(exp).max()


def two_hops(orc, H, seed):
    x = np.random.default_rng(seed).standard_normal((2, 2 * H))
    for h in range(2):
        orc._update_response_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        orc._update_weighted()
    BroadbandOracle._update_statistics(orc)          # the class's own data matrix, no dialect scaling


@pytest.mark.parametrize("off", [0, 37])
def test_python_dialect(golden, off):
    rirs = golden("rirs_cfg1")
    L, M, N, H, J, S = 3, 2, 128, 64, 7, 150
    np.random.seed(2)
    orc = BroadbandOracle(N, rirs["rirA"][:96, :L, :M], rirs["rirB"][:96, :L, :M], J, 3, 0, 1, 2, 1.0, S, hop_size=H)
    two_hops(orc, H, 5)
    ncols, toff = S - J, J
    rings = np.stack([ho.pack_buffers(orc.stats[AA], off), ho.pack_buffers(orc.stats[AB], off)])
    trings = np.roll(orc.target_stats[0].T, off, axis=1)
    # the data matrix itself, channel by channel, is the reference's toeplitz(...) exactly
    for m in range(M):
        Y = ho.data_matrix(rings[0, m * L:(m + 1) * L], J, off, 1, ncols)
        assert Y.shape == (J * L, ncols)
        for s in range(L):
            assert np.array_equal(Y[s * J:(s + 1) * J], hankel_rows(orc.stats[AA][:, s, m], J))
    for dtype in (np.float64, ho.LD):
        R, r = ho.reference(rings, trings, J, L, M, off, 1, ncols, toff, dtype)
        assert R.dtype == dtype and r.dtype == dtype and R.shape == (2, J * L, J * L)
        assert close(R[0], orc.R_AA) and close(R[1], orc.R_AB) and close(r, orc.r_A)
    assert ho.reference(rings[1], None, J, L, M, off, 1, ncols, toff)[1] is None


def test_matlab_dialect(golden):
    rirs = golden("rirs_cfg1")
    L, M, N, H, J, S, off = 2, 3, 128, 64, 9, 140, 101
    orc = MatlabBroadbandOracle(N, rirs["rirA"][:96, :L, :M], rirs["rirB"][:96, :L, :M], J, 3, 0, 1, [1, 2], 1.0, S)
    rng = np.random.default_rng(21)
    orc.response[:] = 1e-3 * rng.standard_normal(orc.response.shape)
    orc.target_response[:] = 1e-3 * rng.standard_normal(orc.target_response.shape)
    two_hops(orc, H, 6)
    ncols, toff = S - J + 1, J - 1
    rings = np.stack([ho.pack_buffers(orc.stats[AA], off), ho.pack_buffers(orc.stats[AB], off)])
    trings = np.roll(orc.target_stats[0].T, off, axis=1)
    R, r = ho.reference(rings, trings, J, L, M, off, 0, ncols, toff)
    assert close(R[0], orc.R_AA) and close(R[1], orc.R_AB) and close(r, orc.r_A)


def test_static_solver_packing():
    rng = np.random.default_rng(4)
    Nb, Nd, P, L, J, delay, ref = 3, 2, 40, 2, 6, 4, 1
    env = np.exp(-np.arange(P) / 10.0)[None, :, None]
    gB, gD = rng.standard_normal((Nb, P, L)) * env, rng.standard_normal((Nd, P, L)) * env
    RB, RD, rB = static_vast.vast_statistics(gB, gD, J, delay, ref)
    f = 1.0 / (Nb * (P - J))
    ncols, S = 999, 999 + J
    Rb, r = ho.reference(ho.pack_static(gB, J, S), ho.pack_static_target(gB, J, S, delay, ref), J, L, Nb, 0, 0, ncols, J)
    Rd, _ = ho.reference(ho.pack_static(gD, J, S), None, J, L, Nd, 0, 0, ncols, J)
    assert close(Rb[0] * f, RB) and close(Rd[0] * f, RD) and close(r * f, rB)
    # responses longer than the 1000 steps vast.m drives are cut where the steps end
    g = rng.standard_normal((1, 1100, 1))
    RB2 = static_vast.vast_statistics(g, g, 4, 3, 0)
    S2 = 999 + 4
    R2, r2 = ho.reference(ho.pack_static(g, 4, S2), ho.pack_static_target(g, 4, S2, 3, 0), 4, 1, 1, 0, 0, 999, 4)
    f2 = 1.0 / (1100 - 4)
    assert close(R2[0] * f2, RB2[0]) and close(r2 * f2, RB2[2])


def test_the_reference_sees_a_single_misplaced_sample():
    """What the exact GPU cases rest on: with integer rings the float64 reference is exact, and moving one sample changes it."""
    rng = np.random.default_rng(0)
    J, L, M, S = 5, 2, 2, 23
    rings = rng.integers(-15, 16, (M * L, S)).astype(np.float64)
    for skip in (0, 1):
        ncols = S - J + (1 - skip)
        R64, _ = ho.reference(rings, None, J, L, M, 3, skip, ncols, 0)
        Rld, _ = ho.reference(rings, None, J, L, M, 3, skip, ncols, 0, ho.LD)
        assert np.array_equal(R64, Rld.astype(np.float64)) and np.array_equal(R64[0], R64[0].T)
        assert not np.array_equal(R64, ho.reference(rings, None, J, L, M, 4, skip, ncols, 0)[0])
