"""The array-effort limit as a kernel (Engine.limit_effort, apv_limit_effort, csrc/kernels_effort.hip) against
tests/effort_oracle.limit_effort.  Every slot is a random direction scaled to an effort of E f with f in {1/4, 1/2, 2, 4}: each
decision is a factor of two from its threshold, so the decisions are compared exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from effort_oracle import limit_effort  # noqa: E402

SHAPES = [(1, 1, 1), (3, 1, 5), (5, 3, 17), (7, 8, 16), (4, 16, 16), (3, 4, 24), (2, 64, 64), (2, 5, 100), (2, 128, 128)]
PATTERNS = ["all", "none", "late", "gap", "zero", "inf", "nan"]
CTYPES = [np.complex64, np.complex128]


@pytest.fixture(scope="module")
def eng():
    from ap_vast_unofficial_amd import Engine
    e = Engine(4, 4, 4, ranks=(1,), compute_dtype="f64")
    yield e
    e.close()


def factors(pattern, K, nV, rng):
    """f (K, nV): the effort of every slot as a multiple of the limit"""
    lo, hi = rng.choice([0.25, 0.5], (K, nV)), rng.choice([2.0, 4.0], (K, nV))
    t = np.arange(nV)[None, :]
    if pattern in ("all", "inf", "zero", "nan"):
        return lo
    if pattern == "none":
        return hi
    if pattern == "late":                              # the first slots inadmissible, the rest admissible
        return np.where(t < (nV + 1) // 2, hi, lo)
    # "gap": admissible / not / admissible in runs of a length that differs from bin to bin
    run = 1 + np.arange(K)[:, None] % 3
    return np.where((t // run) % 2 == 0, lo, hi)


def build(pattern, K, nV, L, ctype, seed):
    rng = np.random.default_rng(seed)
    E = rng.uniform(0.5, 2.0, K)
    f = factors(pattern, K, nV, rng)
    W = rng.standard_normal((K, nV, L)) + 1j * rng.standard_normal((K, nV, L))
    W *= np.sqrt(E[:, None] * f / (np.abs(W) ** 2).sum(-1))[:, :, None]
    W = W.astype(ctype)
    if pattern == "zero":
        W[:, nV // 2] = 0                              # effort 0: admissible
    if pattern == "nan":
        W[K // 2, nV // 2, L // 2] = np.nan            # one slot whose effort is not finite
        f = None
    if pattern == "inf":
        W *= 8                                         # every slot above E ... but there is no limit
        E = np.full(K, np.inf)
    return W, E


def check(got, W, E):
    w2, eff, src_top, gain = got
    K, nV, L = W.shape
    ref, e, _, g, src = limit_effort(W, E, list(range(1, nV + 1)))
    assert w2.dtype == W.dtype and w2.shape == W.shape and eff.shape == (K, nV) and src_top.shape == gain.shape == (K,)
    assert eff.dtype == gain.dtype == np.float64 and src_top.dtype == np.int32
    fin = np.isfinite(e)
    assert np.array_equal(np.isfinite(eff), fin)
    assert (np.abs(eff[fin] - e[fin]) <= 1e-13 * e[fin]).all()
    # src_top: the source slot, the slot's own index where it was scaled, -1 where its effort is not finite
    top = np.where(src[:, -1] >= 0, src[:, -1], np.where(fin[:, -1], nV - 1, -1))
    assert np.array_equal(src_top, top)
    assert (np.abs(gain - g) <= 1e-14 * g).all()
    for k in range(K):
        for t in range(nV):
            s = src[k, t]
            if s == t or not fin[k, t]:
                assert np.array_equal(w2[k, t], W[k, t], equal_nan=True), (k, t)          # untouched
            elif s >= 0:
                assert np.array_equal(w2[k, t], W[k, s]), (k, t, s)                       # a bit copy of its source
            else:
                # scaled: within 4 ulp of the filters' type per component
                d = w2[k, t] - ref[k, t]
                assert (np.abs(d.real) <= 4 * np.spacing(np.abs(ref[k, t].real))).all() and \
                       (np.abs(d.imag) <= 4 * np.spacing(np.abs(ref[k, t].imag))).all(), (k, t)


@pytest.mark.parametrize("ctype", CTYPES)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("K,nV,L", SHAPES)
def test_kernel_vs_oracle(eng, K, nV, L, pattern, ctype):
    W, E = build(pattern, K, nV, L, ctype, 1000 * K + 10 * nV + L)
    keep = W.copy()
    got = eng.limit_effort(W, E)
    assert np.array_equal(W, keep, equal_nan=True)                     # the caller's array is not the one limited
    check(got, W, E)
    if pattern in ("all", "inf", "zero"):
        assert np.array_equal(got[0], W) and (got[2] == nV - 1).all() and (got[3] == 1.0).all()
    if pattern == "none":
        assert (got[2] == nV - 1).all() and (got[3] < 1.0).all()


@pytest.mark.parametrize("ctype", CTYPES)
@pytest.mark.parametrize("K,nV,L", [(5, 3, 17), (4, 16, 16), (2, 5, 100), (2, 128, 128)])
def test_hops_in_one_launch_equal_the_per_hop_calls(eng, K, nV, L, ctype):
    hops = 3
    sets = [build(p, K, nV, L, ctype, 7 + i) for i, p in enumerate(["gap", "none", "late"])]
    E = sets[0][1]
    for i in range(hops):                              # one table for the call: rescale the later hops' filters to it
        sets[i] = ((sets[i][0] * np.sqrt(E / sets[i][1])[:, None, None]).astype(ctype), E)
    W = np.stack([s[0] for s in sets])
    got = eng.limit_effort(W, E)
    assert got[0].shape == W.shape and got[1].shape == (hops, K, nV) and got[2].shape == got[3].shape == (hops, K)
    changed = 0
    for i in range(hops):
        one = eng.limit_effort(W[i], E)
        for a, b in zip(got, one):
            assert np.array_equal(a[i], b)
        changed += int(not np.array_equal(one[0], W[i]))
    assert changed == hops


def test_errors(eng):
    from ap_vast_unofficial_amd._capi import ApvError
    W = np.ones((2, 3, 4), dtype=np.complex128)
    for bad in ([1.0, 0.0], [1.0, -1.0], [np.nan, 1.0]):
        with pytest.raises(ApvError):
            eng.limit_effort(W, np.array(bad))
    with pytest.raises(ValueError):
        eng.limit_effort(W, np.ones(3))
    with pytest.raises(ValueError):
        eng.limit_effort(W[0], np.ones(2))
    with pytest.raises(ApvError):
        eng.limit_effort(np.ones((1, 129, 2), dtype=np.complex64), np.ones(1))
    # a handle without a limit has no outputs to fetch
    with pytest.raises(ApvError):
        eng.effort(0)
