"""The rank choice by validation contrast as a kernel (Engine.validation_span_kernel, apv_validation_span,
csrc/kernels_valspan.hip) against tests/validation_span_oracle.py.

Bound, derived (not measured).  The arithmetic is float64 whatever the filters' type -- complex64 filters are widened exactly -- so
u = 2^-53.  A pressure p = sum_l G W is a dot product of L complex terms: summed in any order it errs by about L u s,
s = sum_l |G| |W|; its square |p|^2 then by about 2 L u s^2, and the sum of Mv squares adds Mv u of the sum, which is at most
S = sum_m s_m^2.  The float64 reference carries the same, so an energy is held to |got - ref| <= 4 (L + Mv + 4) u S.
The decisions are compared with the definition applied to the DEVICE's energies, exactly; the filters with the copies those
decisions prescribe, bit for bit."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from validation_span_oracle import choose, decide, energies, energy_scale  # noqa: E402

SHAPES = [(5, 4, 3, 2), (17, 16, 5, 16), (9, 24, 17, 24), (3, 70, 33, 70), (2, 128, 16, 128)]      # (K, L, Mv, nV)
CTYPES = [np.complex64, np.complex128]
U = 2.0 ** -53


@pytest.fixture(scope="module")
def eng():
    from ap_vast_unofficial_amd import Engine
    e = Engine(4, 4, 4, ranks=(1,), compute_dtype="f64")
    yield e
    e.close()


def build(K, L, Mv, nV, ctype, seed):
    """random banks and filters whose slots differ in scale, and the floor of every bin at the median of its own contrast curve:
    admissible slots, gaps and (in some bins) an inadmissible first slot all occur"""
    rng = np.random.default_rng(seed)
    cn = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    GB, GD = cn(K, Mv, L), cn(K, Mv, L) * rng.uniform(0.5, 2.0, (K, 1, 1))
    W = (cn(K, nV, L) * rng.uniform(0.25, 4.0, (K, nV, 1))).astype(ctype)
    b, d = energies(GB, GD, W)
    phi = np.median(b / d, axis=1)
    return W, GB, GD, phi


def check(got, W, GB, GD, phi, tag=""):
    w2, bright, dark, src, rank, guard = got
    K, nV, L = W.shape
    Mv = GB.shape[1]
    assert w2.dtype == W.dtype and w2.shape == W.shape and bright.shape == dark.shape == src.shape == (K, nV) and rank.shape == (K,)
    assert bright.dtype == dark.dtype == np.float64 and src.dtype == rank.dtype == np.int32
    assert guard == 0                                                  # the guard bands around every device buffer
    with np.errstate(all="ignore"):
        rb, rd = energies(GB, GD, W)
        sb, sd = energy_scale(GB, GD, W)
    bound = 4 * (L + Mv + 4) * U
    fin = np.isfinite(rb) & np.isfinite(rd)
    assert np.array_equal(np.isfinite(bright) & np.isfinite(dark), fin)
    share = 0.0
    for e, r, s in ((bright, rb, sb), (dark, rd, sd)):
        err, lim = np.abs(e[fin] - r[fin]), bound * s[fin]
        share = max(share, (err[lim > 0] / lim[lim > 0]).max(initial=0.0))
        assert (err <= lim).all()
    print(f"{tag} K={K} L={L} Mv={Mv} nV={nV} {W.dtype}: largest energy error {share:.3f} of its bound")
    # the decisions: the definition on the device's own energies, exactly
    src_d, top_d = decide(bright, dark, phi)
    assert np.array_equal(src, src_d) and np.array_equal(rank, top_d)
    assert np.array_equal(w2, choose(W, src), equal_nan=True)
    return src


@pytest.mark.parametrize("ctype", CTYPES)
@pytest.mark.parametrize("K,L,Mv,nV", SHAPES)
def test_kernel_vs_oracle(eng, K, L, Mv, nV, ctype):
    W, GB, GD, phi = build(K, L, Mv, nV, ctype, 1000 * K + 10 * L + Mv)
    keep = W.copy()
    got = eng.validation_span_kernel(W, GB, GD, phi)
    assert np.array_equal(W, keep)                                     # the caller's array is not the one replaced
    src = check(got, W, GB, GD, phi)
    own = src == np.arange(nV)
    assert own.any() and (~own).any()                                  # both branches run
    # two launches agree bit for bit
    again = eng.validation_span_kernel(W, GB, GD, phi)
    for a, b in zip(got, again):
        assert np.array_equal(a, b)
    # no floor: the energies are reported, the filters are bitwise unchanged
    free = eng.validation_span_kernel(W, GB, GD, np.zeros(K))
    assert np.array_equal(free[0], W) and np.array_equal(free[1], got[1]) and np.array_equal(free[2], got[2])
    assert (free[3] == np.arange(nV)).all() and (free[4] == nV).all() and free[5] == 0


@pytest.mark.parametrize("ctype", CTYPES)
@pytest.mark.parametrize("K,L,Mv,nV", [(5, 4, 3, 6), (5, 20, 17, 24)])
def test_none_admissible_zero_and_non_finite_slots(eng, K, L, Mv, nV, ctype):
    """a floor above every contrast (the running best), a zero slot (0/0: admissible under any floor), a dark bank that is zero
    in one bin (dark = 0 < bright: admissible), and slots whose energies are not finite -- on both arithmetic paths"""
    W, GB, GD, phi = build(K, L, Mv, nV, ctype, 77 + L)
    b, d = energies(GB, GD, W)
    phi = 4.0 * (b / d).max(axis=1)                                    # nothing admissible ...
    W[1, 2] = 0                                                        # ... but a zero slot
    GD[2] = 0                                                          # ... and a bin without dark energy
    W[0, 1, L // 2] = np.nan
    W[K - 1, 0, 0] = np.inf                                            # no finite slot at or below slot 0 of the last bin
    src = check(eng.validation_span_kernel(W, GB, GD, phi), W, GB, GD, phi, "edge")
    assert src[K - 1, 0] == -1 and src[0, 1] == 0 and (src[1, 2:] == 2).all() and (src[2] == np.arange(nV)).all()
    assert (src[3] <= np.arange(nV)).all() and (src[3, 1:] != np.arange(1, nV)).any()
    free = eng.validation_span_kernel(W, GB, GD, np.zeros(K))
    assert np.array_equal(free[0], W, equal_nan=True) and free[3][0, 1] == -1 and free[3][K - 1, 0] == -1


def test_entry_refusals(eng):
    from ap_vast_unofficial_amd._capi import ERR_ARG, ApvError
    K, L, Mv, nV = 2, 4, 3, 2
    W, GB, GD, phi = build(K, L, Mv, nV, np.complex128, 5)
    for bad in ([1.0, -1.0], [np.nan, 1.0], [np.inf, 1.0]):
        with pytest.raises(ApvError) as e:
            eng.validation_span_kernel(W, GB, GD, np.array(bad))
        assert e.value.code == ERR_ARG
    with pytest.raises(ValueError):
        eng.validation_span_kernel(W, GB, GD, np.ones(3))
    with pytest.raises(ValueError):
        eng.validation_span_kernel(W, GB, GD[:, :2], phi)
    with pytest.raises(ApvError) as e:                                 # L > 128
        eng.validation_span_kernel(np.ones((1, 2, 129), dtype=np.complex64), np.ones((1, 2, 129)), np.ones((1, 2, 129)), np.ones(1))
    assert e.value.code == ERR_ARG
    with pytest.raises(ApvError) as e:                                 # nV > 128
        eng.validation_span_kernel(np.ones((1, 129, 2), dtype=np.complex64), np.ones((1, 2, 2)), np.ones((1, 2, 2)), np.ones(1))
    assert e.value.code == ERR_ARG
    # null pointers and zero sizes, straight at the C entry
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    w = W.copy()
    args = [1, K, nV, L, Mv, p(w), p(GB), p(GD), p(phi), None, None, None, None, None, None]
    assert eng.lib.apv_validation_span(eng.h, *args) == 0
    assert np.array_equal(w, choose(W, decide(*energies(GB, GD, W), phi)[0]))
    for i in (5, 6, 7, 8):
        a = list(args)
        a[i] = None
        assert eng.lib.apv_validation_span(eng.h, *a) == ERR_ARG
    for i in (1, 2, 3, 4):
        a = list(args)
        a[i] = 0
        keep = w.copy()
        assert eng.lib.apv_validation_span(eng.h, *a) == ERR_ARG
        assert np.array_equal(w, keep)
    assert eng.lib.apv_validation_span(None, *args) == ERR_ARG
    # a handle without the stage has no outputs to fetch
    with pytest.raises(ApvError):
        eng.validation_span(0, 0)
