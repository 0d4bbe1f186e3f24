"""The Householder reduction of the float32 pre-solve (kernels_gevd16m.hip, tridiag_presolve16 step 1) with its two row-to-column
fetches per reflector, u and w, going through LDS instead of the crossbar (one ds_write_b64 and one or two ds_read_b128 for up to
eight ds_bpermute; DESIGN 4.1, "The reduction's crossbar trips through LDS"), and the Lanczos scheme of the NumPy model
(tools/probes/tridiag_presolve_model.py, scheme token `lanczos`), which the kernel does not run.

  plain       257-bin slabs, M in {8, 32, 33}, c64 and c128 outputs, fused and built pairs; ranks (8,) without a lam buffer,
              (1, 8, 16) and (8,) with one, against the oracle
  built       pencils with R_D = I, so that the whitened C is R_B / (1 + reg) with its structure intact; the reflectors run
              through every number of column slots the fetch delivers (one read or two) and meet exactly zero columns:
                diagonal          C diagonal: every column below the diagonal is zero, every u and w a vector of zeros
                blocks            C block-diagonal of four 2 x 2 blocks [[a, b], [b, a]] and two 4 x 4 blocks [[A, B], [B, A]]
                orthogonal        one eigenvector exactly orthogonal to the model's Lanczos start vector
                double            an exact double eigenvalue
                pair1e-3, 1e-4    two eigenvalues 1e-3 and 1e-4 ||C|| apart
                rank8             a bright matrix of rank 8
              each against the oracle; no bin may miss the second step's guard
  scale       the 2^+-160 pencils of test_gpu_leading_half_refinement.py with ranks (1, 8, 16)
  rare        a NaN bin and a zero pivot between healthy bins, and a NaN that reaches the pre-solve: the neighbours keep their bits
  served      a wrong fetch cannot give a wrong filter: the pre-solve then fails its gate, the guarded path delivers a right
              (even closer) result, and a debug_stop = 9 run leaves a bin on that path unmarked.  That the pre-solve still
              SERVES shows where a working float32 pre-solve must leave marks: the pairs 1e-4 ||C|| apart (its error, 6e-8 ||C||
              at the least, over that gap is 6e-4, twenty times the one-step guard of 3e-5: at least half of the bins must take
              the second step), and 8 192 bench bins, whose share of second steps must lie at or below the Householder model's
              plus three binomial standard deviations and must not be zero (the model's share p = 0.3 % makes (1 - p)^8192 =
              1e-12 the chance of that with a working pre-solve)
  model       (no GPU) the Lanczos scheme at six Sturm evaluations keeps at least 99.6 % of 8 192 bench bins inside the one-step
              guard, and on the symmetric blocks it trusts every bin from its own start vector and none from ones / 4

Bounds.  TOL["f64"] of tests/test_gpu_parity.py (a c64 output adds its rounding, 2^-24), and for w also max(2 x the parent's worst,
1e-10), PARENT below holding the parent commit's figures of this file (profiles/r17/new_tests_parent.log); the fetch is a move, so
the change gives the parent's figures to the digit.  No mark is pinned to a bin: which bin near a guard misses it follows the
pre-solve's rounding.

Checked on a scratch build (profiles/r17/breakit_place.log) that writes element i to place i: it fails the two `served` cases and
passes the others.
Run on the MI355X box with `-m gpu`."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, ROOT]

from oracle import subband  # noqa: E402  (checker only)
from presolve_cases import binomial_bound, presolve_model, refinement_marks, rel_w, with_spectrum  # noqa: E402
from test_gpu_leading_half_refinement import _launch, _pair_spectrum, _plain, _reg  # noqa: E402
from test_gpu_parity import TOL  # noqa: E402

gpu = pytest.mark.gpu
L, MU, REG = 16, 0.7, 1e-7
C64 = 2.0 ** -24
LIST = (1, 8, 16)
W_FLOOR = 1e-10
LAM = np.geomspace(1.0, 0.05, L)

# the parent commit's worst w error per case (profiles/r17/new_tests_parent.log)
PARENT = {
    "plain/M8/c64/fused": 3.932e-08, "plain/M8/c64/built": 3.932e-08, "plain/M8/c128/fused": 4.753e-12, "plain/M8/c128/built": 4.307e-12,
    "plain/M32/c64/fused": 3.946e-08, "plain/M32/c64/built": 3.946e-08, "plain/M32/c128/fused": 1.451e-10, "plain/M32/c128/built": 1.451e-10,
    "plain/M33/c64/fused": 3.618e-08, "plain/M33/c64/built": 3.618e-08, "plain/M33/c128/fused": 1.233e-10, "plain/M33/c128/built": 1.230e-10,
    "scale/0": 4.030e-11, "scale/+160": 4.030e-11, "scale/-160": 4.030e-11,
}

def _tight(tag, e_w):
    bw = max(2 * PARENT[tag], W_FLOOR) if tag in PARENT else None
    print(f"FIGURES {tag}: w {e_w:.3e} (bound {bw})")
    assert bw is not None, f"no parent figure for {tag}"
    assert e_w <= bw, (tag, e_w, bw)


def _check_marks(name, marks):
    """debug_stop = 9: 8 = the bin missed the first step's guard only, 16 = the second step's too"""
    assert set(np.unique(marks)) <= {0, 8}, marks.tolist()
    if name == "pair1e-4":                       # `served` in the docstring
        assert np.count_nonzero(marks == 8) >= len(marks) // 2, marks.tolist()


# ---------------------------------------------------------------------------------------------------------------------------
# plain slabs
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "built"])
@pytest.mark.parametrize("out_c128", [False, True], ids=["c64", "c128"])
@pytest.mark.parametrize("M", [8, 32, 33])
def test_plain_against_oracle(M, out_c128, fused):
    slabs, pairs, w_ref = _plain(M)
    args = slabs if fused else pairs
    kw = dict(M=M, out_c128=out_c128, reg=_reg(M))
    extra = 0.0 if out_c128 else C64
    worst = 0.0
    for ranks, with_lam in (((8,), False), (LIST, False), ((8,), True)):
        w, lam, st = _launch(args, ranks, fused, with_lam, **kw)
        assert not st.any(), (ranks, st)
        for t, V in enumerate(ranks):
            if V <= min(L, M):
                e_w = rel_w(w[:, t], w_ref[V])
                assert e_w < TOL["f64"]["w"] + extra, (ranks, V, e_w)
                worst = max(worst, e_w)
        if with_lam:
            lam_ref = np.linalg.eigvalsh(np.linalg.solve(np.linalg.cholesky(pairs[1] + _reg(M) * np.eye(L)), pairs[0]) @
                                         np.linalg.inv(np.linalg.cholesky(pairs[1] + _reg(M) * np.eye(L))).conj().transpose(0, 2, 1))[:, ::-1]
            e_l = (np.abs(lam - lam_ref) / lam_ref[:, :1]).max()
            assert e_l < TOL["f64"]["lam"] + extra, e_l
    _tight(f"plain/M{M}/{'c128' if out_c128 else 'c64'}/{'fused' if fused else 'built'}", worst)


# ---------------------------------------------------------------------------------------------------------------------------
# built pencils
# ---------------------------------------------------------------------------------------------------------------------------
def _sym_blocks(rng):
    """blockdiag of four [[a, b], [b, a]] and two [[A, B], [B, A]] (A, B real symmetric 2 x 2) with the spectrum LAM dealt at
    random: the eigenvectors are (1, 1), (1, -1) and (x, x), (x, -x)"""
    lam = LAM[rng.permutation(L)]
    C = np.zeros((L, L))
    h = np.array([[1.0, 1.0], [1.0, -1.0]]) / np.sqrt(2)
    for b in range(4):
        C[2 * b:2 * b + 2, 2 * b:2 * b + 2] = (h * lam[2 * b:2 * b + 2]) @ h.T
    for b in range(2):
        th = rng.uniform(0.2, 1.3)
        x = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        U = np.block([[x, x], [x, -x]]) / np.sqrt(2)
        s = slice(8 + 4 * b, 12 + 4 * b)
        C[s, s] = (U * lam[8 + 4 * b:12 + 4 * b]) @ U.T
    return 0.5 * (C + C.T).astype(np.complex128)


def _orthogonal_to_start(rng):
    """the spectrum LAM with random eigenvectors of which the first is exactly orthogonal to the model's Lanczos start vector"""
    q0 = presolve_model().LANCZOS_START.astype(np.complex128)
    G = rng.standard_normal((L, L)) + 1j * rng.standard_normal((L, L))
    G[:, 0] -= q0 * (q0.conj() @ G[:, 0]) / (q0.conj() @ q0)
    U = np.linalg.qr(G)[0]
    assert abs(q0.conj() @ U[:, 0]) < 1e-15
    C = (U * LAM[rng.permutation(L)]) @ U.conj().T
    return 0.5 * (C + C.conj().T)


def _double(rng):
    lam = LAM.copy()
    lam[6] = lam[5]
    return with_spectrum(rng, lam)


BUILT = {
    "diagonal": (lambda rng: np.diag(LAM[rng.permutation(L)]).astype(np.complex128), LIST),
    "blocks": (_sym_blocks, LIST),
    "orthogonal": (_orthogonal_to_start, LIST),
    "double": (_double, (3, 8, 16)),                      # ranks that do not split the pair (5, 6)
    "pair1e-3": (lambda rng: with_spectrum(rng, _pair_spectrum(1e-3, 7)), (1, 7, 16)),
    "pair1e-4": (lambda rng: with_spectrum(rng, _pair_spectrum(1e-4, 3)), (1, 8, 16)),
}
BINS = 8
SEEDS = {"blocks": 1700, "diagonal": 1701, "double": 1702, "orthogonal": 1703, "pair1e-3": 1704, "pair1e-4": 1705}


@functools.lru_cache(maxsize=None)
def _built(name):
    make, ranks = BUILT[name]
    rng = np.random.default_rng(SEEDS[name])
    RB = np.array([make(rng) for _ in range(BINS)])
    RD = np.broadcast_to(np.eye(L, dtype=np.complex128), RB.shape).copy()
    r = rng.standard_normal((BINS, L)) + 1j * rng.standard_normal((BINS, L))
    w_ref, lam_ref, _ = subband.gevd_vast(RB, RD, r, MU, list(ranks), reg=REG)
    for a in (RB, RD, r, w_ref, lam_ref):
        a.setflags(write=False)
    return (RB, RD, r), ranks, w_ref, lam_ref


@gpu
@pytest.mark.parametrize("name", list(BUILT))
def test_built_pencils(name):
    pairs, ranks, w_ref, lam_ref = _built(name)
    marks = _launch(pairs, ranks, False, True, debug_stop=9)[2]
    print(f"MARKS {name}: {marks.tolist()}")
    w, lam, st = _launch(pairs, ranks, False, True)
    assert not st.any(), st
    e_w, e_l = rel_w(w, w_ref), (np.abs(lam - lam_ref) / lam_ref[:, :1]).max()
    print(f"FIGURES built/{name}: w {e_w:.3e} lam {e_l:.3e}")
    assert e_l < TOL["f64"]["lam"]
    assert e_w < TOL["f64"]["w"]
    w8 = _launch(pairs, ranks[1:2], False, False)[0]       # the launch that refines the leading half alone
    assert np.array_equal(w8[:, 0], w[:, 1])
    _check_marks(name, marks)


@gpu
def test_rank8_bright_matrix():
    rng = np.random.default_rng(1741)
    n = 6
    Y = rng.standard_normal((n, 8, L)) + 1j * rng.standard_normal((n, 8, L))
    Z = rng.standard_normal((n, 32, L)) + 1j * rng.standard_normal((n, 32, L))
    RB, RD = np.einsum("kmi,kmj->kij", Y.conj(), Y), np.einsum("kmi,kmj->kij", Z.conj(), Z)
    r = rng.standard_normal((n, L)) + 1j * rng.standard_normal((n, L))
    marks = _launch((RB, RD, r), (1, 8), False, True, debug_stop=9)[2]
    print(f"MARKS rank8: {marks.tolist()}")
    w, _, status = _launch((RB, RD, r), (1, 8), False, True)
    assert not status.any(), status
    w_ref, _, _ = subband.gevd_vast(RB, RD, r, MU, [1, 8], reg=REG)
    e_w = rel_w(w, w_ref)
    print(f"FIGURES built/rank8: w {e_w:.3e}")
    assert e_w < TOL["f64"]["w"]
    _check_marks("rank8", marks)


# ---------------------------------------------------------------------------------------------------------------------------
# scale, rare entries
# ---------------------------------------------------------------------------------------------------------------------------
K_SCALE = 64


@functools.lru_cache(maxsize=None)
def _scale_runs():
    slabs, pairs, w_ref = _plain(32)
    XB, XD, d = (a[:K_SCALE] for a in slabs)
    RB, RD, r = (a[:K_SCALE] for a in pairs)
    ref = np.stack([w_ref[V][:K_SCALE] for V in LIST], 1)
    runs = {}
    for e in (0, 40, -40):
        sb, sd = 2.0 ** e, 2.0 ** -e
        kw = dict(mu=MU * sb ** 2 / sd ** 2, reg=REG * sd ** 2)
        fused = _launch(((XB * np.float32(sb)).astype(np.complex64), (XD * np.float32(sd)).astype(np.complex64), d), LIST, True, True, **kw)
        built = _launch((RB * sb ** 2, RD * sd ** 2, r * sb), LIST, False, True, **kw)
        runs[4 * e] = (fused, built, ref / sb)
    return runs


@gpu
@pytest.mark.parametrize("e", [0, 160, -160], ids=["0", "+160", "-160"])
def test_scale(e):
    runs = _scale_runs()
    fused, built, w_ref = runs[e]
    worst = 0.0
    for name, (w, _, status), (_, _, status0) in (("fused", fused, runs[0][0]), ("built", built, runs[0][1])):
        assert np.array_equal(status, status0) and not status.any(), (name, status)
        e_w = rel_w(w, w_ref)
        assert e_w < TOL["f64"]["w"], (name, e_w)
        worst = max(worst, e_w)
    _tight(f"scale/{e:+d}" if e else "scale/0", worst)


@gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "built"])
def test_nan_bin_and_zero_pivot(fused):
    """bin 3 holds a NaN, bin 8 has R_D = 0 under a zero loading: status 1 and zeros on exactly those, the others bit for bit the
    launch without them"""
    K = 12
    XB, XD, d = (a[:K].copy() for a in _plain(32)[0])
    XD[3, 2, 9] = np.nan
    XD[8] = 0
    bad = np.zeros(K, bool)
    bad[[3, 8]] = True

    def run(sel):
        args = (XB[sel], XD[sel], d[sel]) if fused else subband.correlate(XB[sel], XD[sel], d[sel])
        return _launch(args, LIST, fused, True, reg=0.0)

    w, lam, status = run(np.ones(K, bool))
    assert np.array_equal(status == 1, bad) and not status[~bad].any(), status
    assert not w[bad].any()
    w0, lam0, st0 = run(~bad)
    assert not st0.any()
    assert np.array_equal(w[~bad], w0) and np.array_equal(lam[~bad], lam0)
    w_ref, _, _ = subband.update(XB[~bad], XD[~bad], d[~bad], MU, list(LIST), reg=0.0)
    assert rel_w(w[~bad], w_ref) < TOL["f64"]["w"]


@gpu
def test_nan_in_the_bright_matrix():
    """a NaN that reaches the pre-solve itself (through R_B: the Cholesky of R_D is healthy): every beta and alpha of that wave is
    NaN, the gate fails, the bin reports a non-zero status and its neighbours keep their bits"""
    K = 12
    XB, XD, d = (a[:K].copy() for a in _plain(32)[0])
    w0, lam0, st0 = _launch((XB, XD, d), LIST, True, True)
    XB[5, 1, 2] = np.nan
    w, lam, st = _launch((XB, XD, d), LIST, True, True)
    others = np.arange(K) != 5
    assert not st0.any() and st[5] != 0 and not st[others].any(), st
    assert np.array_equal(w[others], w0[others]) and np.array_equal(lam[others], lam0[others])


# ---------------------------------------------------------------------------------------------------------------------------
# the bench distribution: kernel against the Householder model; the Lanczos model against the guard
# ---------------------------------------------------------------------------------------------------------------------------
BENCH_BINS = 8192


@functools.lru_cache(maxsize=None)
def _bench_C():
    C = presolve_model().make_C(BENCH_BINS)              # bench.synth(BENCH_BINS, 1234), whitened in float64
    C.setflags(write=False)
    return C


@functools.lru_cache(maxsize=None)
def _model_share(scheme, nstep):
    """share of the bench bins outside the one-step guard |Z| <= 3e-5 in the NumPy model"""
    model = presolve_model()
    C = _bench_C()
    V, _, trust, _ = model.presolve(C, nstep, 4, np.random.default_rng(7), scheme)
    z = model.zmax(C, V)
    assert trust.all() and (z <= 1e-2).all()
    return float((z > 3e-5).mean())


@gpu
def test_bench_marks():
    """`served` in the docstring: the share of second steps over 8 192 bench bins against the model of the kernel's own scheme"""
    import bench
    from ap_vast_unofficial_amd import Engine
    model = presolve_model()
    XB, XD, d = bench.synth(BENCH_BINS, 1234)
    status = refinement_marks(Engine, XB, XD, d, mu=1.0)
    p = _model_share(model.SCHEME_KERNEL, model.NSTEP_KERNEL)
    second = np.count_nonzero(status == 8)
    bound = binomial_bound(p, BENCH_BINS)
    print(f"FIGURES bench marks: second step {second} of {BENCH_BINS} ({second / BENCH_BINS:.4f}), model {p:.4f}, bound {bound:.4f}")
    assert np.count_nonzero(status == 16) == 0
    assert second / BENCH_BINS <= bound, (second, p, bound)
    assert second > 0


def test_model_lanczos_share_inside_the_one_step_guard():
    """no GPU: the model's Lanczos scheme at six Sturm evaluations keeps at least 99.6 % of 8 192 bench bins inside the one-step
    guard (measured: 99.69 %)"""
    p = _model_share("wide+best4+lanczos", 6)
    print(f"Lanczos model, share outside the one-step guard: {p:.4%}")
    assert 1 - p >= 0.996


def test_model_lanczos_start_vector_on_symmetric_blocks():
    """no GPU: on the symmetric blocks the Lanczos model trusts every bin from its own start vector and meets the second-step
    limit; started from ones / 4 the recurrence breaks down (eight of sixteen directions) and the gate trusts none"""
    model = presolve_model()
    rng = np.random.default_rng(1701)
    C = np.array([_sym_blocks(rng) for _ in range(32)]) / (1 + REG)
    V, _, trust, _ = model.presolve(C, 6, 4, np.random.default_rng(7), "wide+best4+lanczos")
    assert trust.all() and (model.zmax(C, V) <= 1e-2).all()
    _, _, trust1, _ = model.presolve(C, 6, 4, np.random.default_rng(7), "wide+best4+lanczos+ones")
    assert not trust1.any()
