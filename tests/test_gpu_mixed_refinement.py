"""The float64 order-16 kernel's first refinement step (kernels_gevd16m.hip, stage 3) runs from the residual Rs = C V - V D: one
float64 product, the sixteen Rayleigh quotients as column dot products, and V^H Rs and V Z as float32 products behind the
pre-solve's 2^sexp.  A bin that misses the step's guard, or a caller that sets sweep_tol2, takes the float64 products
as before.  Every case goes through Engine.update (fused, c64 slabs) and Engine.gevd_vast (built pairs) in float64 against
oracle/subband.py.

  plain slabs    257 bins, M in {1, 8, 32, 33}, ranks (8,) and (1, 8, 16), with and without a lam buffer, c64 and c128 outputs;
                 every rank of the list bit for bit its single-rank launch; U (jdiag_batched) against the oracle.
  scale          the same 64 bins with X_B x 2^+-40 and X_D x 2^-+40, loading and mu scaled with them, so that the pencil is the
                 unscaled one times 2^+-160 exactly: the same bounds relative to the scaled oracle, the same status words.  This is
                 the 2^sexp in front of the float32 conversion: without it the residual overflows float32 one way (the bins fall
                 back to the float64 step, which passes) and flushes to zero the other way (Z = 0: V stays the pre-solve's).
  guard missed   built pairs with two eigenvalues 1e-3 ||C|| and 1e-4 ||C|| apart (tests/test_gpu_f64_stage_trim.py's spectra) and
                 with an exact double eigenvalue: under debug_stop = 9 the bins carry the marks recorded from the parent commit
                 (GUARD_MARKS), without it they meet the oracle.
  inside guard   built pairs with one gap of 4e-3 ||C||: tools/probes/mixed_refine_model.py (`gap 4e-3 64`, the same 64 matrices)
                 puts the pre-solve's max |Z| at 1.2e-6 / 5.7e-6 / 2.0e-5 (smallest / median / largest bin) against the guard's
                 3e-5.  All bins take the fast step: status 0 and no mark under debug_stop = 9.
  rare entries   a caller-set sweep_tol2 (jdiag_batched); a bright matrix of rank 8; a NaN bin and a zero pivot among good bins
                 (status and zeros as before, the neighbours bit for bit the launch without them); the 16 x 8, 257-bin stream
                 through the launch that covers the hops of a chunk, bit for bit against the hop loop.

Bounds.  TOL["f64"] of tests/test_gpu_parity.py everywhere (lam 1e-9, w 1e-7; a c64 output adds its rounding, 2^-24).  For plain
slabs, scale and inside guard also max(2 x the parent's worst, 1e-10) for w and U and max(2 x the parent's worst, 1e-13 ||C||) for
lam, PARENT below holding the parent commit's worst figures per case (profiles/r15/new_tests_parent.log).  Why 2: the model puts
the eigenvector error the float32 products add at 5e-6 to 2.5e-5 max |Z| (the worst element of 32 768 bins: 6.2e-10 at
max |Z| = 2.5e-5, profiles/r15/mixed_refine_model.txt), no more than the step's own |Z|^2 truncation there, 6.1e-10.  Why the floors:
the added error is proportionally larger only where both steps are below 1e-10; the eigenvalue formula differs by rounding only.

Checked on two scratch builds (profiles/r15/breakit_*.log): with P = V^H T in place of V^H Rs, and without the 2^sexp in front of
the float32 conversion; both fail the file.
Run on the MI355X box with `-m gpu`."""
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, ROOT]

from oracle import gevd, subband  # noqa: E402  (checker only)
from presolve_cases import cn, rel_w, with_spectrum  # noqa: E402
from test_gpu_parity import TOL  # noqa: E402

L, MU, REG = 16, 0.7, 1e-7
C64 = 2.0 ** -24                                    # the rounding of a float64 result to a c64 / float32 output
RANKS = (1, 8, 16)
W_FLOOR, LAM_FLOOR = 1e-10, 1e-13

# the parent commit's worst figures per case: (w or U, lam relative to the bin's largest eigenvalue)
PARENT = {
    "plain/M1/c64": (3.757e-08, 5.273e-08), "plain/M1/c128": (9.212e-14, 4.670e-14),
    "plain/M8/c64": (3.932e-08, 5.776e-08), "plain/M8/c128": (4.753e-12, 3.271e-13),
    "plain/M32/c64": (3.946e-08, 5.866e-08), "plain/M32/c128": (1.462e-10, 3.105e-15),
    "plain/M33/c64": (3.618e-08, 5.602e-08), "plain/M33/c128": (1.228e-10, 2.456e-15),
    "plain/U": (6.149e-13, 4.464e-15),
    "scale/0": (3.944e-11, 2.455e-15), "scale/+160": (3.944e-11, 2.455e-15), "scale/-160": (3.944e-11, 2.455e-15),
    "inside": (9.934e-11, 6.661e-16),
}
# debug_stop = 9 on the parent commit: 8 = the bin missed the first step's guard only, 16 = the second step's too
GUARD_MARKS = {"0.001": [0, 0, 0, 0, 0, 0, 0, 0, 8, 0, 0, 8], "0.0001": [8] * 12, "double": [0] * 6}


def _engine(*a, **kw):
    from ap_vast_unofficial_amd import Engine
    return Engine(*a, **kw)


def _tight(tag, e_w, e_lam):
    """print the figures, then hold them to max(2 x parent, floor)"""
    pw, pl = PARENT[tag]
    bw, bl = max(2 * pw, W_FLOOR), max(2 * pl, LAM_FLOOR)
    print(f"FIGURES {tag}: w {e_w:.3e} (bound {bw:.1e})  lam {e_lam:.3e} (bound {bl:.1e})")
    assert e_w <= bw, (tag, e_w, bw)
    assert e_lam <= bl, (tag, e_lam, bl)


def _lam_err(lam, lam_ref, nz=L):
    return float((np.abs(lam[:, :nz] - lam_ref[:, :nz]) / np.abs(lam_ref[:, :1])).max())


# ---------------------------------------------------------------------------------------------------------------------------
# plain slabs
# ---------------------------------------------------------------------------------------------------------------------------
K_PLAIN = 257


def _reg(M):
    return REG if M >= L else 1e-2          # test_gpu_parity.test_update_vs_oracle: a singular dark matrix is loaded visibly


@functools.lru_cache(maxsize=None)
def _plain(M):
    rng = np.random.default_rng(6100 + M)
    XB, XD, d = cn(rng, K_PLAIN, M, L), cn(rng, K_PLAIN, M, L), cn(rng, K_PLAIN, M)
    RB, RD, r = subband.correlate(XB, XD, d)
    w_ref, lam_ref, st = subband.gevd_vast(RB, RD, r, MU, list(RANKS), reg=_reg(M))
    assert not st.any()
    for a in (XB, XD, d, RB, RD, r, w_ref, lam_ref):
        a.setflags(write=False)
    return XB, XD, d, RB, RD, r, w_ref, lam_ref


def _launch(M, ranks, out_c128, fused, with_lam=True):
    XB, XD, d, RB, RD, r = _plain(M)[:6]
    K = K_PLAIN
    eng = _engine(K, L, M, ranks=ranks, mu=MU, compute_dtype="f64", out_c128=out_c128, reg_dark=_reg(M))
    try:
        if not fused:
            return eng.gevd_vast(RB, RD, r)
        if with_lam:
            return eng.update(XB, XD, d)
        bufs = [eng.to_device(a) for a in (XB, XD, d)]
        dw, ds = eng.alloc(K * len(ranks) * L * np.dtype(eng.w_dtype).itemsize), eng.alloc(K * 4)
        eng.update_dev(bufs[0], bufs[1], bufs[2], dw, None, ds)
        eng.sync()
        out = (dw.download((K, len(ranks), L), eng.w_dtype), None, ds.download((K,), np.int32))
        for b in bufs + [dw, ds]:
            b.free()
        return out
    finally:
        eng.close()


@pytest.mark.parametrize("out_c128", [False, True], ids=["c64", "c128"])
@pytest.mark.parametrize("M", [1, 8, 32, 33])
def test_plain_slabs(M, out_c128):
    w_ref, lam_ref = _plain(M)[6:]
    nz = min(L, M)                                   # beyond rank(R_B) the eigenvalues are rounding noise
    extra = 0.0 if out_c128 else C64
    worst_w = worst_lam = 0.0
    for fused, with_lam in [(True, True), (True, False), (False, True)]:
        single = {V: _launch(M, (V,), out_c128, fused, with_lam) for V in RANKS}
        for ranks in [(8,), RANKS]:
            w, lam, status = single[8] if ranks == (8,) else _launch(M, ranks, out_c128, fused, with_lam)
            tag = f"M={M} {'fused' if fused else 'built'} lam={with_lam} {ranks}"
            assert not status.any(), (tag, status)
            if lam is not None:
                assert lam.dtype == (np.float64 if out_c128 else np.float32)
                e_lam = _lam_err(lam, lam_ref, nz)
                assert e_lam < TOL["f64"]["lam"] + extra, (tag, e_lam)
                if M >= L:
                    assert np.abs(lam / lam_ref - 1).max() < TOL["f64"]["lam"] + extra, tag
                worst_lam = max(worst_lam, e_lam)
            for t, V in enumerate(ranks):
                assert np.array_equal(w[:, t], single[V][0][:, 0]), (tag, V)
                if V <= nz:
                    e_w = rel_w(w[:, t], w_ref[:, RANKS.index(V)])
                    assert e_w < TOL["f64"]["w"] + extra, (tag, V, e_w)
                    worst_w = max(worst_w, e_w)
    _tight(f"plain/M{M}/{'c128' if out_c128 else 'c64'}", worst_w, worst_lam)


def _U_errors(A, B, U, lam, reg=REG):
    """worst column projector u u^H against the oracle's, relative; worst eigenvalue error relative to the largest"""
    e_U = e_lam = 0.0
    n = A.shape[-1]
    for k in range(len(A)):
        U0, lam0 = gevd.jdiag(A[k], B[k])
        Bl = B[k] + reg * np.eye(n)
        # the bounds of test_gpu_parity.test_jdiag_batched_invariants
        assert np.abs(U[k].conj().T @ Bl @ U[k] - np.eye(n)).max() < 1e-11
        assert np.abs(U[k].conj().T @ A[k] @ U[k] - np.diag(lam[k])).max() < 1e-10 * lam[k, 0]
        assert (np.diff(lam[k]) <= 0).all() and np.abs(lam[k] / lam0 - 1).max() < TOL["f64"]["lam"]
        e_lam = max(e_lam, float(np.abs(lam[k] - lam0).max() / lam0[0]))
        for c in range(n):
            P, P0 = np.outer(U[k][:, c], U[k][:, c].conj()), np.outer(U0[:, c], U0[:, c].conj())
            e_U = max(e_U, float(np.linalg.norm(P - P0) / np.linalg.norm(P0)))
    return e_U, e_lam


def test_plain_slabs_U_and_caller_set_tolerance():
    """jdiag_batched sets sweep_tol2 = 1e-17: the one entry that returns U, and a caller-set tolerance, which asks for more than the
    refinement's 1e-9 and takes the float64 products and the sweeps as before"""
    RB, RD = (a[:32] for a in _plain(32)[3:5])
    eng = _engine(1, 4, 4)
    U, lam = eng.jdiag_batched(RB, RD)
    eng.close()
    e_U, e_lam = _U_errors(RB, RD, U, lam)
    assert e_U < TOL["f64"]["w"]
    _tight("plain/U", e_U, e_lam)


# ---------------------------------------------------------------------------------------------------------------------------
# scale
# ---------------------------------------------------------------------------------------------------------------------------
K_SCALE = 64


@functools.lru_cache(maxsize=None)
def _scale_runs():
    """exponent e of the pencil's scale -> results of the fused and the built-pair entry; the oracle once, unscaled"""
    XB, XD, d, RB, RD, r = (a[:K_SCALE] for a in _plain(32)[:6])
    w_ref, lam_ref = (a[:K_SCALE] for a in _plain(32)[6:])
    runs = {}
    for e in (0, 40, -40):
        sb, sd = 2.0 ** e, 2.0 ** -e
        kw = dict(ranks=RANKS, mu=MU * sb ** 2 / sd ** 2, compute_dtype="f64", out_c128=True, reg_dark=REG * sd ** 2)
        eng = _engine(K_SCALE, L, 32, **kw)
        fused = eng.update((XB * np.float32(sb)).astype(np.complex64), (XD * np.float32(sd)).astype(np.complex64), d, raise_on_status=False)
        built = eng.gevd_vast(RB * sb ** 2, RD * sd ** 2, r * sb, raise_on_status=False)
        eng.close()
        # U scales by 1 / sd, r by sb (d itself is not scaled), lam + mu by (sb / sd)^2: w by (sb / sd) (sd / sb)^2 / sd = 1 / sb
        runs[4 * e] = (fused, built, w_ref / sb, lam_ref * (sb / sd) ** 2)
    return runs


@pytest.mark.parametrize("e", [0, 160, -160], ids=["0", "+160", "-160"])
def test_scale(e):
    runs = _scale_runs()
    fused, built, w_ref, lam_ref = runs[e]
    worst_w = worst_lam = 0.0
    for name, (w, lam, status), (_, _, status0) in (("fused", fused, runs[0][0]), ("built", built, runs[0][1])):
        assert np.array_equal(status, status0) and not status.any(), (name, status)
        e_lam, e_w = _lam_err(lam, lam_ref), rel_w(w, w_ref)
        assert np.abs(lam / lam_ref - 1).max() < TOL["f64"]["lam"] and e_w < TOL["f64"]["w"], (name, e_lam, e_w)
        worst_w, worst_lam = max(worst_w, e_w), max(worst_lam, e_lam)
    _tight(f"scale/{e:+d}" if e else "scale/0", worst_w, worst_lam)


# ---------------------------------------------------------------------------------------------------------------------------
# built pairs around the guard
# ---------------------------------------------------------------------------------------------------------------------------
def _built(RB, ranks=RANKS, seed=6300, **kw):
    """built pairs with R_D = I (the whitening is an exact scaling by 1 / (1 + REG)): results and the oracle's"""
    K = len(RB)
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((K, L)) + 1j * rng.standard_normal((K, L))
    RD = np.broadcast_to(np.eye(L, dtype=np.complex128), RB.shape).copy()
    eng = _engine(K, L, 32, ranks=ranks, mu=MU, compute_dtype="f64", out_c128=True, reg_dark=REG, **kw)
    out = eng.gevd_vast(RB, RD, r, raise_on_status=False)
    eng.close()
    return out, RD, r


def _guard_pairs(name):
    from test_gpu_f64_stage_trim import pair_spectrum
    rng = np.random.default_rng(6301)
    if name == "double":
        lam = np.geomspace(1.0, 0.05, L)
        lam[4] = lam[3]
        return np.array([with_spectrum(rng, lam) for _ in range(6)]), (3, 5, 16)       # ranks that do not split the pair
    return np.array([with_spectrum(rng, pair_spectrum(float(name), where)) for where in ("bottom", "middle", "top") for _ in range(4)]), RANKS


@pytest.mark.parametrize("name", ["0.001", "0.0001", "double"])
def test_guard_missed(name):
    RB, ranks = _guard_pairs(name)
    (_, _, marks), _, _ = _built(RB, ranks, debug_stop=9)
    print(f"MARKS {name}: {marks.tolist()}")
    (w, lam, status), RD, r = _built(RB, ranks)
    assert not status.any(), status
    w_ref, lam_ref, _ = subband.gevd_vast(RB, RD, r, MU, list(ranks), reg=REG)
    e_lam, e_w = _lam_err(lam, lam_ref), rel_w(w, w_ref)
    print(f"FIGURES guard/{name}: w {e_w:.3e}  lam {e_lam:.3e}")
    assert e_lam < TOL["f64"]["lam"] and e_w < TOL["f64"]["w"]
    assert marks.tolist() == GUARD_MARKS[name]


@functools.lru_cache(maxsize=None)
def _refine_model():
    spec = importlib.util.spec_from_file_location("mixed_refine_model", os.path.join(ROOT, "tools", "probes", "mixed_refine_model.py"))
    model = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(model)
    return model


INSIDE_GAP, INSIDE_BINS = 4e-3, 64


def test_inside_guard():
    RB = _refine_model().gap_bins(INSIDE_GAP, INSIDE_BINS)           # the matrices the model was run on
    (_, _, marks), _, _ = _built(RB, debug_stop=9)
    assert not marks.any(), marks
    (w, lam, status), RD, r = _built(RB)
    assert not status.any(), status
    w_ref, lam_ref, _ = subband.gevd_vast(RB, RD, r, MU, list(RANKS), reg=REG)
    e_lam, e_w = _lam_err(lam, lam_ref), rel_w(w, w_ref)
    assert np.abs(lam / lam_ref - 1).max() < TOL["f64"]["lam"] and e_w < TOL["f64"]["w"]
    _tight("inside", e_w, e_lam)


# ---------------------------------------------------------------------------------------------------------------------------
# rare entries
# ---------------------------------------------------------------------------------------------------------------------------
def test_rank8_bright_matrix():
    """R_B of rank 8 (M = 8): eight zero eigenvalues, a spread the pre-solve does not vouch for"""
    rng = np.random.default_rng(6401)
    n = 6
    Y = rng.standard_normal((n, 8, L)) + 1j * rng.standard_normal((n, 8, L))
    Z = rng.standard_normal((n, 32, L)) + 1j * rng.standard_normal((n, 32, L))
    RB, RD = np.einsum("kmi,kmj->kij", Y.conj(), Y), np.einsum("kmi,kmj->kij", Z.conj(), Z)
    r = rng.standard_normal((n, L)) + 1j * rng.standard_normal((n, L))
    eng = _engine(n, L, 32, ranks=(1, 8), mu=MU, compute_dtype="f64", reg_dark=REG)
    w, lam, status = eng.gevd_vast(RB, RD, r)
    eng.close()
    assert not status.any(), status
    w_ref, lam_ref, _ = subband.gevd_vast(RB, RD, r, MU, [1, 8], reg=REG)
    e_lam, e_w = _lam_err(lam, lam_ref), rel_w(w, w_ref)
    print(f"FIGURES rank8: w {e_w:.3e}  lam {e_lam:.3e}")
    assert e_lam < TOL["f64"]["lam"] and e_w < TOL["f64"]["w"]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "built"])
def test_nan_bin_and_zero_pivot(fused):
    """bin 3 holds a NaN, bin 8 has R_D = 0 under a zero loading (pivot 0): status 1 and zero outputs on exactly those, the others
    bit for bit the launch without them and inside the bounds"""
    K = 12
    XB, XD, d = (a[:K].copy() for a in _plain(32)[:3])
    XD[3, 2, 9] = np.nan
    XD[8] = 0
    bad = np.zeros(K, bool)
    bad[[3, 8]] = True

    def run(sel):
        eng = _engine(int(sel.sum()), L, 32, ranks=RANKS, mu=MU, compute_dtype="f64", out_c128=True, reg_dark=0.0)
        try:
            if fused:
                return eng.update(XB[sel], XD[sel], d[sel], raise_on_status=False)
            RB, RD, r = subband.correlate(XB[sel], XD[sel], d[sel])
            return eng.gevd_vast(RB, RD, r, raise_on_status=False)
        finally:
            eng.close()

    w, lam, status = run(np.ones(K, bool))
    assert np.array_equal(status == 1, bad) and not status[~bad].any(), status
    assert not w[bad].any() and not lam[bad].any()
    w0, lam0, st0 = run(~bad)
    assert not st0.any()
    assert np.array_equal(w[~bad], w0) and np.array_equal(lam[~bad], lam0)
    w_ref, lam_ref, _ = subband.update(XB[~bad], XD[~bad], d[~bad], MU, list(RANKS), reg=0.0)
    assert np.abs(lam[~bad] / lam_ref - 1).max() < TOL["f64"]["lam"] and rel_w(w[~bad], w_ref) < TOL["f64"]["w"]


def test_stream_16x8_257_bins_equals_hop_loop():
    from ap_vast_unofficial_amd.apvast import apvast
    from test_gpu_stream import _hop_loop, synth_rirs
    N, H, n_hops, V = 512, 256, 17, 3                       # 257 bins; a chunk of 16 hops and one more
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
        assert np.array_equal(getattr(a, "lambda_" + z), getattr(b, "lambda_" + z)), z
    a.close()
    b.close()
