"""Per-bin evaluation spectra of the broadband stream, the three launches alone (apv_eval_spectra_hops,
csrc/kernels_bbevalspec.hip): lines, the stream's own transform over the frames of a launch, and the accumulation in hop order,
against the NumPy restatement of tests/eval_spectra_oracle.py fed the same pressures hop by hop.  The bound is that file's,

    |got - ref| <= 4 c(N) u N sum_t ||w f_t[:, m]||_2^2,   c(N) = 8 (log2 N + 2), three times that with log2 M for Bluestein sizes,

on the increment: the totals start from a random array in [0, 1) which the reference starts from too, and whose additions round
by n u (1 + N sum ||w f||^2) at the most on either side -- 10 / 224 of the bound at n = 5, c >= 56."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from eval_spectra_oracle import SpectraReference, bound_factor, check  # noqa: E402
from oracle.subband import sine_window  # noqa: E402

NH = [(36, 10), (36, 36), (64, 32), (64, 4), (68, 34)]      # H does not divide N; no tail; plain; tail longer than 3 hops; Bluestein


def split_totals(t, E):
    """(Z, 3 E + 1, K, Mv) as the device keeps them -> the dict of (Z, E, Mv, K) / (Z, Mv, K)"""
    t = t.transpose(0, 1, 3, 2)
    return {"bright": t[:, :E], "dark": t[:, E:2 * E], "error": t[:, 2 * E:3 * E], "target": t[:, 3 * E]}


def reference(N, H, Z, E, Mv, tail, start):
    """the helper with `tail` as the newest samples of its ring and `start` as its totals"""
    ref = SpectraReference(N, H, Z, E, Mv)
    if N > H:
        ref.ring[:, :, H:] = tail.transpose(0, 1, 3, 2)
    for k, v in split_totals(start, E).items():
        ref.totals[k] = v.copy()
    return ref


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H", NH)
def test_against_numpy(N, H):
    from ap_vast_unofficial_amd._capi import Engine
    assert bound_factor(N) < 1e-11
    eng = Engine(9, 4, 4)
    worst, K = [0.0], N // 2 + 1
    for Mv in (1, 5, 17):
        for E in (1, 2):
            for Z in (1, 2):
                for n in (1, 3, 5):
                    rng = np.random.default_rng(100000 * N + 1000 * H + 100 * Mv + 10 * E + 3 * Z + n)
                    p = rng.standard_normal((Z, 2 * E + 1, n * H, Mv))
                    tail = rng.standard_normal((Z, 2 * E + 1, Mv, N - H))
                    start = rng.random((Z, 3 * E + 1, K, Mv))
                    ref = reference(N, H, Z, E, Mv, tail, start)
                    for t in range(n):
                        ref.hop(p[:, :, t * H:(t + 1) * H])
                    tot, new_tail = eng.eval_spectra_hops(p, tail, N, H, totals=start)
                    check(split_totals(tot, E), ref, worst)
                    line = np.concatenate([tail, p.transpose(0, 1, 3, 2)], axis=3)       # N - H + n H samples per channel
                    assert new_tail.shape == tail.shape
                    assert np.array_equal(new_tail, line[..., n * H:]), (Mv, E, Z, n)
    print(f"N={N} H={H}: largest error / bound {worst[0]:.4f}")
    eng.close()


# 2 ---------------------------------------------------------------------------------------------------------------
def guarded(eng, a, pad=64):
    g = np.full(pad + a.size + pad, -777.0)
    g[pad:-pad] = a.ravel()
    d = eng.to_device(g)
    return d, ctypes.c_void_p(d.ptr.value + pad * 8)


def unguard(d, shape, pad=64):
    n = int(np.prod(shape))
    g = d.download((pad + n + pad,), np.float64)
    assert np.all(g[:pad] == -777.0) and np.all(g[-pad:] == -777.0)
    return g[pad:-pad].reshape(shape).copy()


@pytest.mark.parametrize("N,H,Mv", [(64, 4, 5), (36, 10, 17)])
def test_bits_do_not_depend_on_the_launch(N, H, Mv):
    """five hops as one call = as 2 + 3 = as 5 x 1 = as one call in sub-launches of 2; guard words around totals and tail"""
    from ap_vast_unofficial_amd._capi import Engine
    eng = Engine(9, 4, 4)
    Z, E, n, K = 2, 2, 5, N // 2 + 1
    sets = Z * (2 * E + 1)
    rng = np.random.default_rng(N + H + Mv)
    p = rng.standard_normal((Z, 2 * E + 1, n * H, Mv))
    tail0, start = rng.standard_normal((Z, 2 * E + 1, Mv, N - H)), rng.random((Z, 3 * E + 1, K, Mv))

    def run(parts, per_launch=0):
        dt, pt = guarded(eng, start)
        dl, pl = guarded(eng, tail0)
        t0 = 0
        for c in parts:
            dp, pp = guarded(eng, np.ascontiguousarray(p[:, :, t0 * H:(t0 + c) * H]))
            eng._chk(eng.lib.apv_eval_spectra_hops(eng.h, pp, pl, N, H, Z, E, Mv, c, per_launch, pt))
            assert np.array_equal(unguard(dp, (sets, c * H, Mv)).reshape(Z, 2 * E + 1, c * H, Mv), p[:, :, t0 * H:(t0 + c) * H])
            dp.free()
            t0 += c
        out = unguard(dt, start.shape), unguard(dl, tail0.shape)
        dt.free()
        dl.free()
        return out

    tot, tail = run([5])
    assert np.array_equal(tail, np.concatenate([tail0, p.transpose(0, 1, 3, 2)], axis=3)[..., n * H:])
    assert not np.array_equal(tot, start)
    for parts, per in (([2, 3], 0), ([1] * 5, 0), ([5], 2), ([5], 1), ([3, 2], 2)):
        t2, l2 = run(parts, per)
        assert np.array_equal(t2, tot), (parts, per)
        assert np.array_equal(l2, tail), (parts, per)
    # and the wrapper, on buffers of its own
    t3, l3 = eng.eval_spectra_hops(p, tail0, N, H, totals=start, hops_per_launch=2)
    assert np.array_equal(t3, tot) and np.array_equal(l3, tail)
    eng.close()


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,k0", [(32, 1), (32, 7), (32, 14), (60, 11), (68, 5)])
def test_known_answer_half_bin_cosine(N, k0):
    """p[n] = cos(2 pi (k0 + 1/2) n / N) on every bright channel, dark and target zero, H = N/2: under the sine window
    w f = [sin(2 pi (k0 + 1) i / N) - sin(2 pi k0 i / N)] / 2, so a full frame adds N^2 / 16 to bins k0 and k0 + 1 and nothing
    elsewhere; error equals bright, target is zero exactly.  The last hop's increment alone, behind five hops of one call."""
    from ap_vast_unofficial_amd._capi import Engine
    eng = Engine(9, 4, 4)
    Z, E, Mv, H, steps = 2, 2, 5, N // 2, 6
    K = N // 2 + 1
    x = np.cos(2 * np.pi * (k0 + 0.5) * np.arange(steps * H) / N)
    p = np.zeros((Z, 2 * E + 1, steps * H, Mv))
    p[:, :E] = x[:, None]
    _, tail = eng.eval_spectra_hops(p[:, :, :(steps - 1) * H], None, N, H)
    tot, _ = eng.eval_spectra_hops(p[:, :, (steps - 1) * H:], tail, N, H)
    got = split_totals(tot, E)
    frame = x[(steps - 2) * H:]
    bound = bound_factor(N) * np.sum((sine_window(N) * frame) ** 2)
    exp = np.zeros(K)
    exp[k0] = exp[k0 + 1] = N * N / 16.0
    share = np.abs(got["bright"] - exp).max() / bound
    print(f"N={N} k0={k0}: largest error / bound {share:.4f}")
    assert np.all(np.abs(got["bright"] - exp) <= bound)
    assert np.array_equal(got["error"], got["bright"])
    assert np.all(got["dark"] == 0.0) and np.all(got["target"] == 0.0)
    eng.close()


# 4 ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_totals_alone():
    from ap_vast_unofficial_amd import _capi
    eng = _capi.Engine(9, 4, 4)
    N, H, Z, E, Mv, n = 36, 10, 2, 1, 3, 2
    K, sets = N // 2 + 1, Z * (2 * E + 1)
    start = np.random.default_rng(4).random((Z, 3 * E + 1, K, Mv))
    dp, dl, dt = eng.to_device(np.ones((sets, n * H, Mv))), eng.to_device(np.ones((sets, Mv, N - H))), eng.to_device(start)
    f = eng.lib.apv_eval_spectra_hops
    good = dict(p=dp.ptr, tail=dl.ptr, N=N, H=H, Z=Z, E=E, Mv=Mv, n=n, per=0, tot=dt.ptr)
    bad = [dict(p=None), dict(tot=None), dict(tail=None), dict(N=0), dict(H=0), dict(Z=0), dict(E=0), dict(Mv=0), dict(n=0),
           dict(N=37), dict(N=4098, H=10), dict(H=N + 1), dict(H=N + 2), dict(Z=3), dict(per=-1), dict(n=2 ** 26, H=32, N=32),
           dict(n=2 ** 31 // 10 + 1)]
    for change in bad:
        a = dict(good, **change)
        rc = f(eng.h, a["p"], a["tail"], a["N"], a["H"], a["Z"], a["E"], a["Mv"], a["n"], a["per"], a["tot"])
        assert rc == _capi.ERR_ARG, change
        assert np.array_equal(dt.download(start.shape, np.float64), start), change
    # a null tail is fine where there is none
    dq = eng.to_device(np.ones((sets, n * N, Mv)))
    assert f(eng.h, dq.ptr, None, N, N, Z, E, Mv, n, 0, dt.ptr) == 0
    assert not np.array_equal(dt.download(start.shape, np.float64), start)
    with pytest.raises(ValueError):
        eng.eval_spectra_hops(np.zeros((1, 2, 8, 2)), None, 8, 4)            # an even number of pressure sets
    with pytest.raises(ValueError):
        eng.eval_spectra_hops(np.zeros((1, 3, 9, 2)), None, 8, 4)            # not a whole number of hops
    with pytest.raises(ValueError):
        eng.eval_spectra_hops(np.zeros((1, 3, 8, 2)), np.zeros((1, 3, 2, 5)), 8, 4)
    for b in (dp, dl, dt, dq):
        b.free()
    eng.close()
