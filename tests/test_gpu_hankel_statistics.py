"""The broadband Hankel statistics at the kernel level (Engine.hankel_statistics -> apv_hankel_statistics): both forms of
csrc/kernels_bb.hip -- hankel_corr_kernel, the displacement form, and syrk_hankel_kernel, the dense products on the matrix
cores -- and xcorr_hankel_kernel at the edges of their lag blocks, column parts, walk segments, tiles, loudspeaker windows and
column chunks, against tests/hankel_oracle.py.

The exact cases use integer rings, every sample uniform in -15..15 and stored as float64.  Products are at most 225 and every
sum stays below 225 M ncols < 2^53, so every partial result of either kernel -- the walk's added and subtracted end products
included -- is an exactly representable integer, and so is the float64 reference: the comparison is np.array_equal, and one
wrong index, window, guard or mirror write fails it.  Every run asserts the form that was taken."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hankel_oracle as ho  # noqa: E402

FORMS = ("displacement", "dense", "auto")

# ---- the launcher's rules, restated (csrc/kernels_bb.hip) ------------------------------------------------------------------
HC_TPB, HC_MAXPARTS, HC_MAXSEG, HC_LDS = 1024, 10, 16, 158 * 1024
SY_BUF = 256 * 10


def hc_red_len(J):
    nbk, nqmax = (J + 3) // 4 + (J + 2) // 4, 2 * J - 1
    nseg = min(max(HC_TPB // nqmax, 1), HC_MAXSEG)
    return max(HC_MAXPARTS * nbk * 4, nqmax * nseg)


def displacement_lds(J, M, S):
    return 8 * (2 * M * (S + 8) + hc_red_len(J) + 2 * J)


def displacement_fits(J, M, S, ncols):
    return 2 * J - 1 <= HC_TPB and displacement_lds(J, M, S) <= HC_LDS and ncols + J + 2 <= S + 8


def walk_segments(J):
    """(segments, their odd length) of a diagonal of a pair of different loudspeakers, 2 J - 1 lags."""
    nseg = min(max(HC_TPB // (2 * J - 1), 1), HC_MAXSEG)
    return nseg, ((J + nseg - 1) // nseg) | 1


def syrk_tc(J):
    """Columns per LDS chunk of the dense kernel where the columns do not all fit one chunk (syrk_plan): a run of 32 rows touches
    at most nseg = 31 // J + 2 loudspeakers, both tile sides stage nseg windows of W = SY_BUF // (2 nseg) doubles, a window is
    a chunk and 32 more samples, chunks are multiples of four: J >= 32: nseg 2, W 640, TC 608; J in 16..31: nseg 3, W 426,
    TC = 4 (394 // 4) = 392."""
    nseg = 31 // J + 2
    return max((SY_BUF // (2 * nseg) - 32) // 4 * 4, 4)


@pytest.fixture(scope="module")
def eng():
    from ap_vast_unofficial_amd._capi import Engine
    e = Engine(1, 4, 4)
    yield e
    e.close()


def integers(rng, *shape):
    return rng.integers(-15, 16, shape).astype(np.float64)


def offsets(S, J):
    return sorted({0, 1, S - J, S - 1})          # a window straddles the wrap at every side


def exact(eng, J, L, M, S, *, njobs=1, ncols=None, skips=(1, 0), forms=FORMS, auto=None):
    """Every skip x ring offset x form of one shape, integer data: R, r equal to the float64 reference, R symmetric, the form taken
    the form asked for ("auto": the restated rule, and `auto` where the case names it); "displacement" raises where it does not
    fit.  Returns the forms that ran."""
    from ap_vast_unofficial_amd._capi import ApvError, ERR_ARG
    rng = np.random.default_rng([J, L, M, S, njobs])
    st, ts = integers(rng, njobs, M * L, S), integers(rng, M, S)
    ran = set()
    for skip in skips:
        nc = S - J + (1 - skip) if ncols is None else ncols
        toff = J if skip else J - 1
        assert 225 * M * nc < 2 ** 53
        fits = displacement_fits(J, M, S, nc)
        for off in offsets(S, J):
            Rref, rref = ho.reference(st, ts, J, L, M, off, skip, nc, toff, np.float64)
            for form in forms:
                what = (J, L, M, S, njobs, nc, skip, off, form)
                kw = dict(J=J, L=L, M=M, off=off, skip=skip, ncols=nc, toff=toff, form=form)
                if form == "displacement" and not fits:
                    with pytest.raises(ApvError) as ei:
                        eng.hankel_statistics(st, ts, **kw)
                    assert ei.value.code == ERR_ARG, what
                    continue
                R, r, taken = eng.hankel_statistics(st, ts, **kw)
                want = form if form != "auto" else ("displacement" if fits else "dense")
                assert taken == want, what
                if form == "auto" and auto is not None:
                    assert taken == auto, what
                ran.add(taken)
                assert R.shape == Rref.shape and r.shape == rref.shape
                assert np.array_equal(R, Rref), (what, np.argwhere(R != Rref)[:4])
                assert np.array_equal(R, R.transpose(0, 2, 1)), what
                assert np.array_equal(r, rref), (what, np.argwhere(r != rref)[:4])
    return ran


# ---- displacement form -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [1, 2, 3, 4, 5, 8, 9])
@pytest.mark.parametrize("S", ["smallest", 61])
def test_lag_blocks_of_four(eng, J, S):
    """The edges of the lag blocks: nb_pos = (J + 3) // 4 positive and nb_neg = (J + 2) // 4 negative blocks (none at J = 1), at the
    smallest legal ring, S = J + 2, where the 2 or 3 columns are fewer than the column parts, and at S = 61.  M ncols is below
    256 (the cross-correlation's one pass) at the former.  Both forms and "auto" return the same arrays."""
    S = J + 2 if S == "smallest" else S
    assert exact(eng, J, 3, 2, S, auto="displacement") == {"displacement", "dense"}


@pytest.mark.parametrize("J,nseg", [(17, 16), (32, 16), (33, 15), (64, 8), (65, 7)])
def test_walk_segments(eng, J, nseg):
    """The walk down each diagonal in 16, 16, 15, 8 and 7 segments of odd length, segments that start past the end of their
    diagonal included (J = 17: 16 segments of 3 cover 48 > 17)."""
    assert walk_segments(J)[0] == nseg
    if J == 17:
        assert walk_segments(J) == (16, 3)
    assert exact(eng, J, 2, 2, 2 * J + 37, auto="displacement") == {"displacement", "dense"}


def test_largest_lag_count(eng):
    """J = 512 is the largest the displacement form takes: 2 J - 1 = 1023 lag jobs for 1024 threads, one segment per diagonal, 256
    lag blocks in four column parts.  J = 513: the form is refused, "auto" reports the dense kernel, the result is exact."""
    assert walk_segments(512) == (1, 513) and HC_TPB // (128 + 128) == 4
    assert exact(eng, 512, 2, 1, 600, auto="displacement") == {"displacement", "dense"}
    assert not displacement_fits(513, 1, 600, 87)
    assert exact(eng, 513, 2, 1, 600, auto="dense") == {"dense"}


@pytest.mark.parametrize("L", [1, 5])
@pytest.mark.parametrize("M", [1, 7])
def test_pairs_and_microphones(eng, L, M):
    """One pair (s = s' only: no negative lags) and fifteen pairs; one and seven microphones."""
    assert exact(eng, 6, L, M, 90, auto="displacement") == {"displacement", "dense"}


@pytest.mark.parametrize("njobs", [1, 4])
def test_displacement_jobs(eng, njobs):
    """blockIdx.z: up to four rings sets with different data, one launch."""
    assert exact(eng, 12, 2, 3, 100, njobs=njobs, auto="displacement") == {"displacement", "dense"}


def test_lds_threshold(eng):
    """Where the choice flips.  J = 24: 12 lag blocks, 47 lags in 16 segments, so the work array is max(10 x 12 x 4, 47 x 16) = 752
    doubles; with M = 8 the launch needs 8 (2 x 8 (S + 8) + 752 + 48) = 128 (S + 8) + 6400 bytes against 158 KiB = 161 792:
    S + 8 <= 1214, S <= 1206."""
    J, L, M = 24, 2, 8
    assert hc_red_len(J) == 752 and displacement_lds(J, M, 1206) == 161792 == HC_LDS
    S = max(s for s in range(1100, 1300) if displacement_lds(J, M, s) <= HC_LDS)
    assert S == 1206
    assert exact(eng, J, L, M, S, auto="displacement") == {"displacement", "dense"}
    assert exact(eng, J, L, M, S + 1, auto="dense") == {"dense"}


# ---- dense form, at sizes "auto" gives to the other kernel -------------------------------------------------------------------
@pytest.mark.parametrize("J,L", [(1, 1), (1, 33), (31, 1), (16, 2), (11, 3), (7, 9), (13, 5), (31, 3), (32, 2), (33, 2), (100, 1)])
def test_tiles_and_windows(eng, J, L):
    """Orders 1, 33, 31, 32, 33, 63, 65, 93, 64, 66, 100 against the 32 x 32 tiles: J = 1 with 33 loudspeakers under one tile side
    (and the sp < L guard in the last tile), J = 31 with three loudspeakers per side, J >= 32 with two.  51 columns in both
    dialects: one chunk whose last step of four runs past the columns."""
    for skip in (1, 0):
        assert exact(eng, J, L, 2, J + 50 + skip, skips=(skip,), auto="displacement") == {"displacement", "dense"}


@pytest.mark.parametrize("J,TC", [(40, 608), (20, 392)])
def test_column_chunks(eng, J, TC):
    """ncols % 4 of every value in the first, a middle and the last chunk of TC columns."""
    assert syrk_tc(J) == TC
    for ncols in (1, 2, 3, 4, 5, TC - 1, TC, TC + 1, TC + 4, 2 * TC + 3):
        assert exact(eng, J, 2, 1, J + ncols + 1, ncols=ncols, auto="displacement") == {"displacement", "dense"}


def test_static_solver_launch(eng):
    """apv_vast_static's own launch for ten bright microphones: the contiguous matrix, 999 columns (six chunks of 148 and 111
    more: a tail step), off = 0, toff = J -- and 2 x 10 x 1013 doubles of sequences are more LDS than the displacement form has."""
    J, L, M = 6, 4, 10
    assert syrk_tc(J) == 148 and not displacement_fits(J, M, 999 + J, 999)
    assert exact(eng, J, L, M, 999 + J, ncols=999, skips=(0,), auto="dense") == {"dense"}


@pytest.mark.parametrize("njobs", [1, 2, 3, 4])
def test_dense_jobs(eng, njobs):
    """One to four ring sets, three microphones (M = 1: the column chunks above)."""
    assert exact(eng, 20, 2, 3, 100, njobs=njobs, forms=("dense", "auto"), auto="displacement") == {"displacement", "dense"}


# ---- the entry itself --------------------------------------------------------------------------------------------------------
def test_defaults_and_arguments(eng):
    """ncols and toff default to the python dialect's; a two-dimensional stats is one job; what apv_bb_init refuses is refused."""
    from ap_vast_unofficial_amd._capi import ApvError
    rng = np.random.default_rng(9)
    J, L, M, S = 5, 2, 2, 40
    st, ts = integers(rng, M * L, S), integers(rng, M, S)
    for skip in (1, 0):
        R, r, taken = eng.hankel_statistics(st, ts, J=J, L=L, M=M, off=7, skip=skip)
        Rref, rref = ho.reference(st, ts, J, L, M, 7, skip, S - J + (1 - skip), J if skip else J - 1)
        assert taken == "displacement" and np.array_equal(R, Rref) and np.array_equal(r, rref)
    R, r, _ = eng.hankel_statistics(st, J=J, L=L, M=M)
    assert r is None and np.array_equal(R, ho.reference(st, None, J, L, M, 0, 1, S - J, J)[0])
    ok = dict(J=J, L=L, M=M, off=0, skip=1, ncols=S - J, toff=J)
    for bad in (dict(off=S), dict(off=-1), dict(ncols=0), dict(ncols=S - J + 1), dict(toff=J + 1), dict(toff=-1), dict(J=0),
                dict(skip=0, ncols=S - J + 2)):
        with pytest.raises(ApvError):
            eng.hankel_statistics(st, ts, **{**ok, **bad})
    with pytest.raises(ApvError):
        eng.hankel_statistics(integers(rng, 1, 4097), J=4097, L=1, M=1, ncols=1, toff=0, skip=0, off=0)
    with pytest.raises(ApvError):
        eng.hankel_statistics(np.zeros((5, M * L, S)), J=J, L=L, M=M)
    with pytest.raises(ValueError):
        eng.hankel_statistics(st, ts, **ok, form="sparse")
    with pytest.raises(ValueError):
        eng.hankel_statistics(st, ts[:1], **ok)


# ---- float data --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,L,M,S", [(24, 3, 2, 700), (5, 4, 3, 700)])
def test_float_rings(eng, J, L, M, S):
    """Gaussian rings under an exponential envelope, as a stream's statistics buffers are, ring offset 300, both forms and both
    dialects against the long-double reference at the project's bound for these quantities, 1e-12 of the largest entry
    (test_broadband_statistics_shapes).  Measured on an MI355X, worst error / largest entry at (24, 3, 2, 700) and (5, 4, 3, 700):
    R in the displacement form 4.4e-16 and 3.6e-16, in the dense form 1.7e-15 and 2.0e-15; r 2.1e-16 and 9.1e-17."""
    rng = np.random.default_rng([J, L, M, S])
    env = np.exp(-np.arange(S)[::-1] / 150.0)               # the newest samples, at the ring's logical end, are the loudest
    off = 300
    st = np.roll(rng.standard_normal((M * L, S)) * env, off, axis=1)
    ts = np.roll(rng.standard_normal((M, S)) * env, off, axis=1)
    worst = {}
    for skip in (1, 0):
        nc, toff = S - J + (1 - skip), J if skip else J - 1
        Rref, rref = ho.reference(st, ts, J, L, M, off, skip, nc, toff, ho.LD)
        for form in ("displacement", "dense"):
            R, r, taken = eng.hankel_statistics(st, ts, J=J, L=L, M=M, off=off, skip=skip, ncols=nc, toff=toff, form=form)
            assert taken == form
            eR = float(np.abs(R[0] - Rref[0]).max() / np.abs(Rref[0]).max())
            er = float(np.abs(r - rref).max() / np.abs(rref).max())
            worst[form] = max(worst.get(form, 0.0), eR)
            worst["r"] = max(worst.get("r", 0.0), er)
            assert np.array_equal(R, R.transpose(0, 2, 1))
            assert eR <= 1e-12 and er <= 1e-12, (form, skip, eR, er)
    print(f"hankel statistics, float rings (J, L, M, S) = {(J, L, M, S)}: worst error / largest entry", worst)
