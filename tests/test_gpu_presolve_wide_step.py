"""The wave-wide first multisection step and the best-of-four shifts of the float32 pre-solve (kernels_gevd16m.hip,
tridiag_presolve16) where they can go wrong: eigenvalues on and between the 64 points of the wide step (the vote crosses 16-lane
rows and 32-lane halves), many eigenvalues inside one of its 65 brackets, close pairs on either side of a quad point and of the
boundary between two shifts, eigenvalues placed so that the first, the last or no single lane of the quad has the best shift, and
a NaN bin between healthy ones (the debug_stop = 9 marks against the NumPy model of this scheme: test_step_marks of
tests/test_gpu_multisection_steps.py).  L = 16, explicit R_B / R_D (R_D = I, so the
whitened C is R_B / (1 + reg)); spectra have ||lam||_2 = 1 = ||C||_F (1 + reg), so a value x is the point x ||C||_F of the kernel's
interval [-1e-3, 1.001] ||C||_F.  Bounds as tests/test_gpu_multisection_steps.py.  Every bin is solved twice: by the engine with
ranks (1,), and by one with ranks (1, 16), because only the full-rank filter sees every eigenvector."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import subband  # noqa: E402  (checker only)
from presolve_cases import check_nan_bin, presolve_model, rel_w, with_spectrum  # noqa: E402

model = presolve_model()

L, M = 16, 32
REG = 1e-7                                    # the engine's and the oracle's loading of R_D
MU = 0.1
BINS_PER_CASE = 4
LO, W = -1e-3, 1.002                          # the multisection's first interval, in units of ||C||_F
NW = model.NWIDE + 1                          # 65 brackets
WB = W / NW                                   # one bracket of the wide step
WF = WB * 5.0 ** -model.NQUAD_KERNEL          # the final interval
PAIR_GAPS = [3e-6, 1e-5, 3e-5, 1e-3]          # x ||C||_F; the `apart` threshold is 1.22e-5


def point(l):
    """the point lane l evaluates in the wide step"""
    return LO + (l + 1) * WB


Q0 = point(15) + 2 * WB / 5                   # a point of the first quad step inside bracket 16 (and an end of final intervals)


def filled(fixed, hi=0.15, lo=0.02, min_gap=1e-4):
    """`fixed` and a geometric fill scaled so that ||lam||_2 = 1, descending; the fill stays min_gap away from everything"""
    fixed = np.asarray(fixed, float)
    n = L - len(fixed)
    fill = np.geomspace(hi, lo, n) * (1 + 0.01 * np.arange(n))
    fill *= np.sqrt((1.0 - np.sum(fixed * fixed)) / np.sum(fill * fill))
    lam = np.sort(np.r_[fixed, fill])[::-1]
    assert abs(np.linalg.norm(lam) - 1) < 1e-12
    assert np.abs(fill[:, None] - fixed[None, :]).min() >= min_gap and np.diff(np.sort(fill)).min() >= min_gap
    return lam


def one_bracket():
    """all sixteen eigenvalues inside bracket 16 of the wide step, (point(15), point(16)) = (0.2457, 0.2611), gaps from 2e-5 up
    (1.3e-3 of the bracket)"""
    lam = 0.25 + np.r_[0.0, np.cumsum(np.geomspace(2e-5, 2.4e-3, L - 1))]
    lam = np.sort(lam / np.linalg.norm(lam))[::-1]
    assert point(15) < lam.min() and lam.max() < point(16) and -np.diff(lam).max() >= 1e-3 * WB
    return lam


def top_of_interval():
    """the largest eigenvalue 0.99996 ||C||_F, in the last bracket (point(63) = 0.9856, 1.001)"""
    rest = np.geomspace(6e-3, 1.1e-3, L - 1)
    lam = np.r_[np.sqrt(1 - np.sum(rest * rest)), rest]
    assert lam[0] > point(63) and lam[-1] > 1e-3 * lam[0]
    return lam


def spectra():
    s = {}
    # ---- on and between the points of the wide step
    s["grid/on_points_31_32_15_16_and_zero"] = filled([point(32), point(31), point(16), point(15), 0.0])
    s["grid/between_31_32_and_between_15_16"] = filled([0.5 * (point(31) + point(32)), 0.5 * (point(15) + point(16))])
    s["grid/on_points_48_0_and_zero"] = filled([point(48), point(0), 0.0])
    s["grid/on_point_63"] = filled([point(63)], hi=0.1)
    s["grid/top_of_interval"] = top_of_interval()
    s["grid/just_each_side_of_point_31"] = filled([point(31) + 2e-5, point(31) - 2e-5])
    # ---- eigenvalues sharing a bracket
    s["bracket/all_sixteen"] = one_bracket()
    s["bracket/two"] = filled([point(31) + 0.8 * WB, point(31) + 0.15 * WB])
    s["bracket/three"] = filled([point(31) + 0.9 * WB, point(31) + 0.5 * WB, point(31) + 0.1 * WB])
    s["bracket/eight"] = filled(point(15) + WB * np.array([0.95, 0.9, 0.7, 0.52, 0.5, 0.3, 0.12, 0.05]), hi=0.6, lo=0.03)
    # ---- pairs on either side of a quad point, and of the boundary between the shifts of lanes 1 and 0 three final intervals on
    for gap in PAIR_GAPS:
        s[f"pair/{gap:g}/quad_point"] = filled([Q0 + 0.5 * gap, Q0 - 0.5 * gap], min_gap=1e-3)
        s[f"pair/{gap:g}/shift_boundary"] = filled([Q0 + 3.25 * WF + 0.5 * gap, Q0 + 3.25 * WF - 0.5 * gap], min_gap=1e-3)
    # ---- which lane of the quad wins: every eigenvalue at 1/8 (lane 0's shift), at 7/8 (lane 3's) and at the middle of a final
    # interval (lanes 1 and 2 equally far).  The positions hold to the 1e-7 ||C|| of the float32 reduction, a tenth of WF.  The
    # smallest eigenvalue is not placed: it restores ||lam||_2 = 1.
    base = np.geomspace(0.6, 0.05, L)
    base /= np.linalg.norm(base)
    for name, f in (("winner/lane_0", 0.125), ("winner/lane_3", 0.875), ("winner/lanes_1_2_tie", 0.5)):
        lam = LO + (np.floor((base - LO) / WF) + f) * WF
        lam[-1] = np.sqrt(1 - np.sum(lam[:-1] ** 2))
        assert abs(lam[-1] - base[-1]) < 1e-4
        s[name] = lam
    # C = I / 4: the tridiagonal is diagonal, every quad ends in the same interval with the same four shifts and the same growth
    # lane by lane, all gaps read 0
    s["winner/multiple_of_identity"] = np.full(L, 0.25)
    return s


SPECTRA = spectra()


@pytest.fixture(scope="module")
def Engine():
    from ap_vast_unofficial_amd import Engine
    return Engine


@pytest.fixture(scope="module")
def solved(Engine):
    """every spectrum under BINS_PER_CASE random unitaries, in ONE batch: engine with ranks (1,), engine with ranks (1, 16), oracle"""
    rng = np.random.default_rng(61)
    cases, RB = {}, []
    for name, lam in SPECTRA.items():
        cases[name] = slice(len(RB), len(RB) + BINS_PER_CASE)
        RB += [with_spectrum(rng, lam) for _ in range(BINS_PER_CASE)]
    RB = np.array(RB)
    K = len(RB)
    assert 16 <= K <= 1024
    r = rng.standard_normal((K, L)) + 1j * rng.standard_normal((K, L))
    RD = np.broadcast_to(np.eye(L, dtype=np.complex128), RB.shape).copy()
    out = {}
    for ranks in ((1,), (1, 16)):
        eng = Engine(K, L, M, ranks=ranks, mu=MU, compute_dtype="f64", out_c128=True)
        out[ranks] = eng.gevd_vast(RB, RD, r, raise_on_status=False)
        eng.close()
    w_ref, lam_ref, _ = subband.gevd_vast(RB, RD, r, MU, [1, 16])
    lam_np = np.linalg.eigvalsh(RB)[:, ::-1] / (1 + REG)
    return cases, out, w_ref, lam_ref, lam_np


def check(solved, name, simple_top=True):
    cases, out, w_ref, lam_ref, lam_np = solved
    sel = cases[name]
    for ranks, (w, lam, status) in out.items():
        w, lam, status = w[sel], lam[sel], status[sel]
        e_or = (np.abs(lam - lam_ref[sel]) / lam_ref[sel, :1]).max()
        e_np = (np.abs(lam - lam_np[sel]) / lam_np[sel, :1]).max()
        e_w1 = rel_w(w[:, :1], w_ref[sel, :1])
        e_w16 = rel_w(w[:, 1:], w_ref[sel, 1:]) if len(ranks) > 1 else 0.0
        print(f"{name} ranks {ranks}: status {np.unique(status)}  lam vs oracle {e_or:.2e}  vs eigh {e_np:.2e}  "
              f"w(rank 1) {e_w1:.2e}  w(rank 16) {e_w16:.2e}")
        assert np.isfinite(w).all() and np.isfinite(lam).all()
        assert not status.any(), status
        assert e_or < 1e-12 and e_np < 1e-12
        # the full-rank filter is a function of the whole pencil, defined however a close pair's vectors are chosen; it is wrong
        # if the eigenvector matrix lacks a direction
        assert e_w16 < 1e-7
        if simple_top:
            assert e_w1 < 1e-7


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in SPECTRA if n.startswith("grid/")])
def test_eigenvalue_on_the_wide_grid(solved, name):
    """Eigenvalues on points of the 65-way grid (lanes 15 | 16 and 47 | 48 lie in different 16-lane rows, 31 | 32 in different
    32-lane halves too), between two such points, next to one on either side, at 0 (a singular C: the spread gate sends it to the
    double sweeps) and at the top of the interval."""
    check(solved, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in SPECTRA if n.startswith("bracket/")])
def test_eigenvalues_sharing_a_bracket(solved, name):
    """Two, three, eight and all sixteen eigenvalues inside one bracket of the wide step: their quads leave it with the same
    interval and the quad steps have to separate them."""
    check(solved, name)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["quad_point", "shift_boundary"])
@pytest.mark.parametrize("gap", PAIR_GAPS)
def test_close_pair(solved, gap, where):
    """A pair `gap` ||C|| apart centred on a quad point or on the boundary between two lanes' shifts.  3e-6 and 1e-5 are under the
    `apart` threshold and must reach the double sweeps (a pair that won with one and the same shift reads a gap of 0); a gate that
    is too lax would hand back a wrong eigenvector with status 0."""
    check(solved, f"pair/{gap:g}/{where}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in SPECTRA if n.startswith("winner/")])
def test_winning_lane(solved, name):
    """Every eigenvalue nearest the shift of lane 0, of lane 3, midway between those of lanes 1 and 2, and C = I / 4 (all gaps 0:
    only the full-rank filter is defined).  The winner's vector is what has to reach V32: with another lane's the result is still
    certified by the refinement, so this asserts the result, not the lane.  Which lane wins on these spectra is checked on the
    model, test_model_winning_lane: with gaps of 8e-3 ||C|| any of the four vectors stays far inside the one-step guard (model:
    |Z| <= 2.3e-5 with lane 0 forced where lane 3 should win, 4e-6 with the winner), so no mark of the kernel can tell them apart."""
    check(solved, name, simple_top=name != "winner/multiple_of_identity")


@pytest.mark.parametrize("name,lanes", [("winner/lane_0", (0,)), ("winner/lane_3", (3,)), ("winner/lanes_1_2_tie", (1, 2))])
def test_model_winning_lane(name, lanes):
    """The model's best_of_four (the kernel's key: the bits of the squared norm with 3 - jq in the two lowest) on the winner
    spectra, without noise: the placed eigenvalues (all but the smallest, ascending index 1..15) win with the lane whose shift
    they sit on.  The float32 reduction moves an eigenvalue by about 1e-7 ||C||, a tenth of the final interval, and one at 1/8 or
    7/8 of it leaves its interval (and wins with the lane at the other end of the neighbouring one) from 1/8 on: at least 90 % of
    the 8 x 15 eigenvalues must win with the expected lane.  Midway between lanes 1 and 2 the two are 1/8 away and lanes 0 and 3
    3/8: every winner must be 1 or 2, and both must occur."""
    rng = np.random.default_rng(67)
    C = np.array([with_spectrum(rng, SPECTRA[name]) for _ in range(8)]) / (1 + REG)
    nf2 = (np.abs(C) ** 2).sum((1, 2))
    sexp = -(np.frexp(nf2)[1] - 1) // 2
    A = (C * np.ldexp(1.0, sexp)[:, None, None]).astype(np.complex64)
    nrm = np.sqrt(np.ldexp(nf2, 2 * sexp)).astype(np.float32)
    a, e, e2, _, _ = model.tridiag(A)
    lo, hi = model.multisection(a, e2, nrm, model.NSTEP_KERNEL, 4, interval=True)
    _, lam, win = model.best_of_four(a, e, lo, hi, nrm)
    win = win[:, 1:]
    counts = np.bincount(win.ravel(), minlength=4)
    print(name, "winners by lane:", counts)
    assert (np.diff(lam, axis=1) > 0).all()
    if len(lanes) == 1:
        assert counts[lanes[0]] >= 0.9 * win.size, counts
    else:
        assert counts[list(lanes)].sum() == win.size and all(counts[j] > 0 for j in lanes), counts


@pytest.mark.gpu
def test_nan_bin_between_healthy_bins(Engine):
    """A NaN in one bin (every lane's Sturm count and every shift of that wave is NaN: a NaN key wins the quad and fails the gate)
    gives that bin a non-zero status and leaves its neighbours' results bit for bit as they are without it: bin 7 of 16, ranks (1,)."""
    check_nan_bin(Engine, K=16, k0=7, ranks=(1,))
