"""predictPressure / metrics / static VAST on the device against the NumPy restatement (unpinned) and KA-4."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import static_vast  # noqa: E402


def test_predict_pressure_vs_lfilter(golden):
    from ap_vast_unofficial_amd.evaluation import predict_pressure, nmse, acoustic_contrast_db
    g = golden("rirs_cfg1")
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1500, 8))
    pB = predict_pressure(x, g["rirA"])
    ref = static_vast.predict_pressure(x, g["rirA"])
    assert pB.shape == (1500, 8)
    assert np.abs(pB - ref).max() < 1e-12 * np.abs(ref).max()
    pD = predict_pressure(x, g["rirB"])
    assert abs(nmse(ref, pB)) < 1e-20
    ac = acoustic_contrast_db(pB, pD)
    assert abs(ac - 10 * np.log10((ref ** 2).sum() / (static_vast.predict_pressure(x, g["rirB"]) ** 2).sum())) < 1e-9


# (T, L, M, P): one sample; fewer samples than taps; 256 // 7 = 36 rows of a block with four idle threads; two rows with 56 idle
# threads; one row with one idle thread; one row, no idle thread
PRESSURE_SHAPES = [(1, 1, 1, 1), (5, 2, 3, 9), (1000, 4, 7, 50), (300, 3, 100, 7), (257, 2, 255, 4), (40, 1, 256, 3)]


@pytest.mark.parametrize("T,L,M,P", PRESSURE_SHAPES)
def test_predict_pressure_shapes_exact(T, L, M, P):
    """predict_pressure_kernel's row / microphone split of a block at its edges.  Integer signals and responses in -15..15: every
    partial sum is an integer below 225 P L < 2^53, so the kernel's fused multiply-adds and lfilter's sums are both exact."""
    from ap_vast_unofficial_amd.evaluation import predict_pressure
    rng = np.random.default_rng([T, L, M, P])
    x = rng.integers(-15, 16, (T, L)).astype(np.float64)
    rir = rng.integers(-15, 16, (P, L, M)).astype(np.float64)
    got = predict_pressure(x, rir)
    assert got.shape == (T, M) and np.array_equal(got, static_vast.predict_pressure(x, rir))


def test_predict_pressure_gaussian_and_microphone_limit():
    from ap_vast_unofficial_amd.evaluation import predict_pressure
    from ap_vast_unofficial_amd._capi import ApvError
    T, L, M, P = 300, 3, 100, 7
    rng = np.random.default_rng(12)
    x, rir = rng.standard_normal((T, L)), rng.standard_normal((P, L, M))
    ref = static_vast.predict_pressure(x, rir)
    assert np.abs(predict_pressure(x, rir) - ref).max() < 1e-12 * np.abs(ref).max()
    with pytest.raises(ApvError):
        predict_pressure(np.zeros((4, 1)), np.zeros((2, 1, 257)))


# (Nb, Nd, P, L, J, delay, ref, V): one microphone per zone and one loudspeaker; P = J + 1 and V = n; J = 1 with delay = P - 1 and the
# last reference; ten bright microphones (their 2 x 10 x 1013 doubles exceed the displacement form's LDS: the dense kernel at 999
# columns); twelve microphones per zone; responses longer than the 1000 steps vast.m drives
VAST_CASES = [(1, 1, 40, 1, 8, 0, 0, 3), (3, 2, 9, 2, 8, 0, 1, 16), (2, 5, 30, 3, 1, 29, 2, 2), (10, 4, 60, 4, 6, 5, 0, 7),
              (12, 12, 60, 3, 5, 59, 2, 15), (2, 3, 1100, 2, 4, 3, 0, 5)]


@pytest.mark.parametrize("case", VAST_CASES, ids=lambda c: "-".join(map(str, c)))
def test_static_vast_edges(case):
    """vast.m at the edges of its sizes against the oracle at the bound of test_static_vast_vs_oracle.  The inputs (seed sum(case),
    envelope exp(-q / max(P / 4, 2))) keep the comparison meaningful -- the oracle's cond(R_D) is at most 22 and the relative
    eigenvalue gap at V at least 0.025 where V < n -- and the condition number is asserted, so that a changed input cannot hollow
    out the bound."""
    from ap_vast_unofficial_amd.evaluation import vast
    Nb, Nd, P, L, J, delay, ref, V = case
    rng = np.random.default_rng(sum(case))
    env = np.exp(-np.arange(P) / max(P / 4, 2))[None, :, None]
    gB = rng.standard_normal((Nb, P, L)) * env
    gD = rng.standard_normal((Nd, P, L)) * env
    mu = 0.8
    w_ref, (RB, RD, rB) = static_vast.vast(gB, gD, J, delay, ref, V, mu)
    assert np.linalg.cond(RD) < 1e3
    w = vast(gB, gD, J, delay, ref, V, mu)
    assert w.shape == (J * L,)
    assert np.linalg.norm(w - w_ref) < 1e-8 * np.linalg.norm(w_ref)
    if V == J * L:
        # KA-4: the full-rank solution is pressure matching, w = (RB + mu RD)^-1 rB
        pm = np.linalg.solve(RB + mu * RD, rB)
        assert np.linalg.norm(w - pm) < 1e-8 * np.linalg.norm(pm)


@pytest.mark.parametrize("V", [1, 20, 48])
def test_static_vast_vs_oracle(V):
    """vast.m: 4 loudspeakers, 12-tap filters (n = 48), 6 + 5 microphones, 60-tap RIRs."""
    from ap_vast_unofficial_amd.evaluation import vast
    rng = np.random.default_rng(3)
    P, L, J = 60, 4, 12
    env = np.exp(-np.arange(P) / 15.0)[None, :, None]
    gB = rng.standard_normal((6, P, L)) * env
    gD = rng.standard_normal((5, P, L)) * env
    w = vast(gB, gD, J, 5, 1, V, 0.8)
    w_ref, (RB, RD, rB) = static_vast.vast(gB, gD, J, 5, 1, V, 0.8)
    assert np.linalg.norm(w - w_ref) < 1e-8 * np.linalg.norm(w_ref)
    if V == J * L:
        # KA-4: the full-rank solution is pressure matching, w = (RB + mu RD)^-1 rB
        pm = np.linalg.solve(RB + 0.8 * RD, rB)
        assert np.linalg.norm(w - pm) < 1e-8 * np.linalg.norm(pm)
