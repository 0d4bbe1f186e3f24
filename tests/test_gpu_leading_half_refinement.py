"""The float64 order-16 kernel's first refinement step runs in two halves of eight eigenvector columns (kernels_gevd16m.hip, stage
3; DESIGN 4.1, "The leading half alone"): half A, the eight leading columns, always; half B only for a launch that reads the
other eight (a rank above 8, a lam buffer, U, a contrast floor).  A half's two float32 products are packed ones on a real tile
[re | im] with the summation of the full complex product, so a column's bits do not depend on the form; and the leading columns
depend on half A alone, so a rank's filter has the same bits whether half B ran or not.

Launches that run half A only: ranks (8,), (1,) and (1, 4, 8) WITHOUT a lam buffer (Engine.update_dev for slabs, apv_gevd_vast_dev
with a null lam for built pairs).  Launches that run both: any list with 16, and any launch with a lam buffer.

  bit for bit    257 bins, M in {8, 32, 33}, c64 and c128 outputs, fused and built: every rank of the A-only launches equals the
                 same rank of the (1, 8, 16) launch (rank 4: of a (4,) launch with a lam buffer), and (8,) equals (8,) with a lam
                 buffer.  The A-only launches meet the oracle.
  close pairs    built pairs with two eigenvalues 1e-3 ||C|| and 1e-4 ||C|| apart, among the eight smallest, among the eight
                 largest, and as the 8th and 9th largest; an exact double eigenvalue in each half; 1.1e-5 ||C|| across the 8 | 9
                 boundary.  The A-only (8,) launch meets the oracle and equals rank 8 of the list launch; the debug_stop = 9 marks
                 are the parent commit's (MARKS).
  scale          the 2^+-160 pencils of test_gpu_mixed_refinement.py through the A-only launch: same status, same relative bounds.
  rare entries   a NaN bin and a zero pivot among good bins; a bright matrix of rank 8; the 16 x 8, 257-bin stream (V = 1) through
                 the launch that covers the hops of a chunk, bit for bit against the hop loop.

Bounds.  TOL["f64"] of tests/test_gpu_parity.py (a c64 output adds its rounding, 2^-24), and for w also max(2 x the parent's worst,
1e-10), PARENT below holding the parent commit's figures of this file (profiles/r16/new_tests_parent.log; on the parent every
launch takes the full step).  Why 2 and why the floor: as in test_gpu_mixed_refinement.py -- a bin that passes its guards has the
parent's bits; one in which only half B misses keeps the fast step's leading columns, whose error the model puts at the step's own
|Z|^2 truncation.

Checked on two scratch builds (profiles/r16/breakit_*.log): with the sign of -Rr in the second operand flipped, and with columns
0..7 taken as the leading half; both fail the file.
Run on the MI355X box with `-m gpu`."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, ROOT]

from oracle import subband  # noqa: E402  (checker only)
from presolve_cases import cn, rel_w, with_spectrum  # noqa: E402
from test_gpu_parity import TOL  # noqa: E402

L, MU, REG = 16, 0.7, 1e-7
C64 = 2.0 ** -24
LIST = (1, 8, 16)
A_ONLY = [(8,), (1,), (1, 4, 8)]
W_FLOOR = 1e-10
K_PLAIN = 257

# the parent commit's worst w error per case
PARENT = {
    "plain/M8/c64/fused": 3.932e-08, "plain/M8/c64/built": 3.932e-08, "plain/M8/c128/fused": 4.753e-12, "plain/M8/c128/built": 4.307e-12,
    "plain/M32/c64/fused": 3.867e-08, "plain/M32/c64/built": 3.867e-08, "plain/M32/c128/fused": 3.360e-11, "plain/M32/c128/built": 3.360e-11,
    "plain/M33/c64/fused": 3.815e-08, "plain/M33/c64/built": 3.815e-08, "plain/M33/c128/fused": 2.725e-11, "plain/M33/c128/built": 2.726e-11,
    "scale/0": 3.360e-11, "scale/+160": 3.360e-11, "scale/-160": 3.360e-11,
}
# debug_stop = 9 on the parent commit, four bins per placement (bottom, top, boundary): 8 = the bin missed the first step's guard
# only, 16 = the second step's too
MARKS = {
    "0.001": [0, 0, 0, 0, 0, 0, 0, 8, 0, 0, 0, 0], "0.0001": [8, 0, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8],
    "double": [0] * 6, "boundary1.1e-5": [0] * 6,
}


def _engine(*a, **kw):
    from ap_vast_unofficial_amd import Engine
    return Engine(*a, **kw)


def _tight(tag, e_w):
    bw = max(2 * PARENT[tag], W_FLOOR) if tag in PARENT else None
    print(f"FIGURES {tag}: w {e_w:.3e} (bound {bw})")
    assert bw is not None, f"no parent figure for {tag}"
    assert e_w <= bw, (tag, e_w, bw)


def _run(eng, K, args, fused, with_lam):
    """one launch from host arrays; without a lam buffer the launch gets a null pointer for it"""
    nV = eng.nV
    bufs = [eng.to_device(np.ascontiguousarray(a, dtype=np.complex64 if fused else eng.c_dtype)) for a in args]
    dw = eng.alloc(K * nV * L * np.dtype(eng.w_dtype).itemsize)
    dl = eng.alloc(K * L * np.dtype(eng.lam_dtype).itemsize) if with_lam else None
    ds = eng.alloc(K * 4)
    if fused:
        eng.update_dev(bufs[0], bufs[1], bufs[2], dw, dl, ds)
    else:
        eng._chk(eng.lib.apv_gevd_vast_dev(eng.h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, dw.ptr, dl.ptr if dl else None, ds.ptr))
    eng.sync()
    out = (dw.download((K, nV, L), eng.w_dtype), dl.download((K, L), eng.lam_dtype) if dl else None, ds.download((K,), np.int32))
    for b in bufs + [dw, ds] + ([dl] if dl else []):
        b.free()
    return out


def _launch(args, ranks, fused, with_lam, M=32, out_c128=True, reg=REG, mu=MU, **kw):
    K = len(args[0])
    eng = _engine(K, L, M, ranks=ranks, mu=mu, compute_dtype="f64", out_c128=out_c128, reg_dark=reg, **kw)
    try:
        return _run(eng, K, args, fused, with_lam)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------------
# bit for bit within the build, and against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
def _reg(M):
    return REG if M >= L else 1e-2          # a singular dark matrix is loaded visibly (test_gpu_parity.test_update_vs_oracle)


@functools.lru_cache(maxsize=None)
def _plain(M):
    rng = np.random.default_rng(6100 + M)   # the slabs of test_gpu_mixed_refinement.py
    XB, XD, d = cn(rng, K_PLAIN, M, L), cn(rng, K_PLAIN, M, L), cn(rng, K_PLAIN, M)
    RB, RD, r = subband.correlate(XB, XD, d)
    w_ref, _, st = subband.gevd_vast(RB, RD, r, MU, [1, 4, 8, 16], reg=_reg(M))
    assert not st.any()
    for a in (XB, XD, d, RB, RD, r, w_ref):
        a.setflags(write=False)
    return (XB, XD, d), (RB, RD, r), dict(zip((1, 4, 8, 16), np.moveaxis(w_ref, 1, 0)))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "built"])
@pytest.mark.parametrize("out_c128", [False, True], ids=["c64", "c128"])
@pytest.mark.parametrize("M", [8, 32, 33])
def test_bit_for_bit_and_oracle(M, out_c128, fused):
    slabs, pairs, w_ref = _plain(M)
    args = slabs if fused else pairs
    kw = dict(M=M, out_c128=out_c128, reg=_reg(M))
    both = {}
    w, _, st = _launch(args, LIST, fused, False, **kw)
    assert not st.any()
    both[1], both[8] = w[:, 0], w[:, 1]
    w, _, st = _launch(args, (4,), fused, True, **kw)
    assert not st.any()
    both[4] = w[:, 0]
    w8_lam = _launch(args, (8,), fused, True, **kw)[0][:, 0]
    extra = 0.0 if out_c128 else C64
    worst = 0.0
    for ranks in A_ONLY:
        w, lam, st = _launch(args, ranks, fused, False, **kw)
        assert lam is None and not st.any(), (ranks, st)
        for t, V in enumerate(ranks):
            assert np.array_equal(w[:, t], both[V]), (ranks, V)
            if V <= min(L, M):
                e_w = rel_w(w[:, t], w_ref[V])
                assert e_w < TOL["f64"]["w"] + extra, (ranks, V, e_w)
                worst = max(worst, e_w)
        if ranks == (8,):
            assert np.array_equal(w[:, 0], w8_lam)
    _tight(f"plain/M{M}/{'c128' if out_c128 else 'c64'}/{'fused' if fused else 'built'}", worst)


# ---------------------------------------------------------------------------------------------------------------------------
# where the close pair sits
# ---------------------------------------------------------------------------------------------------------------------------
PLACES = {"bottom": 11, "top": 3, "boundary": 7}       # descending index j of the pair (j, j + 1): 7 = the 8th and 9th largest


def _pair_spectrum(gap, j):
    """a graded spectrum (1 ... 0.05) in which eigenvalue j + 1 is gap ||C||_F below eigenvalue j; descending"""
    lam = np.geomspace(1.0, 0.05, L)
    for _ in range(3):
        lam[j + 1] = lam[j] - gap * np.linalg.norm(lam)
    assert (np.diff(lam) <= 0).all()
    return lam


@functools.lru_cache(maxsize=None)
def _close_pairs(name):
    rng = np.random.default_rng(6501)
    if name == "double":
        spectra = []
        for j in (11, 3):
            lam = np.geomspace(1.0, 0.05, L)
            lam[j + 1] = lam[j]
            spectra += [lam] * 3
        ranks = (3, 8, 16)                               # ranks that do not split a pair
    elif name == "boundary1.1e-5":
        spectra, ranks = [_pair_spectrum(1.1e-5, 7)] * 6, (1, 7, 16)
    else:
        spectra, ranks = [_pair_spectrum(float(name), j) for j in PLACES.values() for _ in range(4)], LIST
    RB = np.array([with_spectrum(rng, lam) for lam in spectra])
    RD = np.broadcast_to(np.eye(L, dtype=np.complex128), RB.shape).copy()
    r = rng.standard_normal((len(RB), L)) + 1j * rng.standard_normal((len(RB), L))
    w_ref, _, _ = subband.gevd_vast(RB, RD, r, MU, list(ranks), reg=REG)
    return (RB, RD, r), ranks, w_ref


@pytest.mark.parametrize("name", ["0.001", "0.0001", "double", "boundary1.1e-5"])
def test_close_pairs(name):
    pairs, ranks, w_ref = _close_pairs(name)
    marks = _launch(pairs, ranks, False, True, debug_stop=9)[2]
    print(f"MARKS {name}: {marks.tolist()}")
    w_list, _, st = _launch(pairs, ranks, False, True)
    assert not st.any(), st
    single = ranks[1]                                    # 8, or 7 where 8 would split the pair
    w, lam, st = _launch(pairs, (single,), False, False)
    assert lam is None and not st.any(), st
    e_w = rel_w(w[:, 0], w_ref[:, 1])
    print(f"FIGURES pairs/{name}: w {e_w:.3e}")
    assert e_w < TOL["f64"]["w"]
    assert rel_w(w_list, w_ref) < TOL["f64"]["w"]
    assert np.array_equal(w[:, 0], w_list[:, 1])
    assert name in MARKS, f"no parent marks for {name}"
    assert marks.tolist() == MARKS[name]


# ---------------------------------------------------------------------------------------------------------------------------
# scale
# ---------------------------------------------------------------------------------------------------------------------------
K_SCALE = 64


@functools.lru_cache(maxsize=None)
def _scale_runs():
    slabs, pairs, w_ref = _plain(32)
    XB, XD, d = (a[:K_SCALE] for a in slabs)
    RB, RD, r = (a[:K_SCALE] for a in pairs)
    runs = {}
    for e in (0, 40, -40):
        sb, sd = 2.0 ** e, 2.0 ** -e
        kw = dict(mu=MU * sb ** 2 / sd ** 2, reg=REG * sd ** 2)
        fused = _launch(((XB * np.float32(sb)).astype(np.complex64), (XD * np.float32(sd)).astype(np.complex64), d), (8,), True, False, **kw)
        built = _launch((RB * sb ** 2, RD * sd ** 2, r * sb), (8,), False, False, **kw)
        runs[4 * e] = (fused, built, w_ref[8][:K_SCALE] / sb)
    return runs


@pytest.mark.parametrize("e", [0, 160, -160], ids=["0", "+160", "-160"])
def test_scale(e):
    runs = _scale_runs()
    fused, built, w_ref = runs[e]
    worst = 0.0
    for name, (w, _, status), (_, _, status0) in (("fused", fused, runs[0][0]), ("built", built, runs[0][1])):
        assert np.array_equal(status, status0) and not status.any(), (name, status)
        e_w = rel_w(w[:, 0], w_ref)
        assert e_w < TOL["f64"]["w"], (name, e_w)
        worst = max(worst, e_w)
    _tight(f"scale/{e:+d}" if e else "scale/0", worst)


# ---------------------------------------------------------------------------------------------------------------------------
# rare entries
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "built"])
def test_nan_bin_and_zero_pivot(fused):
    """bin 3 holds a NaN, bin 8 has R_D = 0 under a zero loading: status 1 and zeros on exactly those, the others bit for bit the
    A-only launch without them"""
    K = 12
    XB, XD, d = (a[:K].copy() for a in _plain(32)[0])
    XD[3, 2, 9] = np.nan
    XD[8] = 0
    bad = np.zeros(K, bool)
    bad[[3, 8]] = True

    def run(sel):
        args = (XB[sel], XD[sel], d[sel]) if fused else subband.correlate(XB[sel], XD[sel], d[sel])
        return _launch(args, (8,), fused, False, reg=0.0)

    w, _, status = run(np.ones(K, bool))
    assert np.array_equal(status == 1, bad) and not status[~bad].any(), status
    assert not w[bad].any()
    w0, _, st0 = run(~bad)
    assert not st0.any()
    assert np.array_equal(w[~bad], w0)
    w_ref, _, _ = subband.update(XB[~bad], XD[~bad], d[~bad], MU, [8], reg=0.0)
    assert rel_w(w[~bad], w_ref) < TOL["f64"]["w"]


def test_rank8_bright_matrix():
    """R_B of rank 8: eight zero eigenvalues, a spread the pre-solve does not vouch for; the leading eight are all there is"""
    rng = np.random.default_rng(6401)
    n = 6
    Y = rng.standard_normal((n, 8, L)) + 1j * rng.standard_normal((n, 8, L))
    Z = rng.standard_normal((n, 32, L)) + 1j * rng.standard_normal((n, 32, L))
    RB, RD = np.einsum("kmi,kmj->kij", Y.conj(), Y), np.einsum("kmi,kmj->kij", Z.conj(), Z)
    r = rng.standard_normal((n, L)) + 1j * rng.standard_normal((n, L))
    w, _, status = _launch((RB, RD, r), (1, 8), False, False)
    assert not status.any(), status
    w_ref, _, _ = subband.gevd_vast(RB, RD, r, MU, [1, 8], reg=REG)
    e_w = rel_w(w, w_ref)
    print(f"FIGURES rank8: w {e_w:.3e}")
    assert e_w < TOL["f64"]["w"]
    assert np.array_equal(w, _launch((RB, RD, r), (1, 8), False, True)[0])


def test_stream_16x8_257_bins_rank_1_equals_hop_loop():
    from ap_vast_unofficial_amd.apvast import apvast
    from test_gpu_stream import _hop_loop, synth_rirs
    N, H, n_hops, V = 512, 256, 17, 1                       # 257 bins; a chunk of 16 hops and one more
    rirA, rirB = synth_rirs(300, L, 8, 12)
    mk = lambda: apvast(N, rirA, rirB, 16, 5, 1, 2, V, 1.0, 4 * N, hop_size=H, seed=4, dtype="f64", perceptual=False)
    a, b = mk(), mk()
    x = np.random.default_rng(9).standard_normal((2, n_hops * H))
    ref = _hop_loop(a, x, 0, n_hops)
    got = list(b.process_signal(x[0], x[1]))
    assert b.signal_schedule == (n_hops, 0)                 # every hop went through the chunked schedule
    for q in range(4):
        for v in range(len(ref[q])):
            assert np.array_equal(got[q][v], ref[q][v]), (q, v)
    for z in "AB":
        assert np.array_equal(getattr(a, "w_" + z), getattr(b, "w_" + z)), z
    a.close()
    b.close()
