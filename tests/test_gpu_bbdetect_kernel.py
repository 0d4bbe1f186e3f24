"""Detectability stage of the broadband stream, the three hop-batched launches alone (apv_eval_detect_hops,
Engine.eval_detect_hops, csrc/kernels_evaldetect.hip) on spectra [n][K][Z (2 E + 1) Mv] of n consecutive hops: against the NumPy
restatement of tests/detectability_oracle.py at its derived bound for given spectra, 2 (2 K + C + 16) u D; against themselves
under every split of the hops over calls and sub-launches, bit for bit; and against the per-hop launches of the subband stream
(apv_eval_detect_step), bit for bit.  Every comparison with the helper asserts bound < 1e-10 D, so the bound cannot hide a failure."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import detectability_oracle as do  # noqa: E402
from test_gpu_evaluation_detectability import fold, random_spectra, reference_hop, tables_of, within  # noqa: E402

# block, hop, sampling rate, channels of the model: a smooth transform; a Bluestein length with K - 1 = 68 no multiple of 16; K = 97
SIZES = [(96, 24, 48000, 44), (136, 40, 16000, 34), (192, 96, 3000, 19)]
MVS = [1, 5, 16, 17, 33]
ZE = [(1, 1), (2, 1), (2, 3), (1, 3)]
RATIOS = (1.0, 0.3, 0.1, 0.03, 0.01)                        # the target 0 to 40 dB above the disturbances
PAD = 64


@functools.lru_cache(maxsize=None)
def tables(n, fs):
    return tables_of(n, fs)


def hops_of(rng, K, Z, E, Mv, n):
    """(5, K, Z (2 E + 1), Mv): one hop per ratio"""
    return np.stack([random_spectra(rng, K, Z, E, Mv, n, r) for r in RATIOS])


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,fs,c", SIZES)
def test_against_numpy(n, h, fs, c):
    """five hops at every Mv and (Z, E): hop values within the bound; sum, max and audible count follow from the device's own
    hop values in the device's arithmetic, bit for bit, from a start that is not zero"""
    from ap_vast_unofficial_amd._capi import Engine
    tb = tables(n, fs)
    assert tb.n_channels == c
    eng = Engine(9, 4, 4)
    K, worst, sides = n // 2 + 1, [0.0], [False, False]
    for Mv in MVS:
        for Z, E in ZE:
            rng = np.random.default_rng(1000 * n + 10 * Mv + 3 * Z + E)
            spec = hops_of(rng, K, Z, E, Mv, n)
            start = np.zeros((Z, 6 * E, Mv))
            start.reshape(Z, 2, 3, E, Mv)[:, :, :2] = rng.random((Z, 2, 2, E, Mv))
            got, tot = eng.eval_detect_hops(spec, tb, Z, E, totals=start)
            assert got.shape == (len(RATIOS), Z, 2 * E, Mv)
            want = start
            for i in range(len(RATIOS)):
                ref = reference_hop(tb, spec[i], Z, E, n)
                within(got[i], ref, do.bound_given(K, c, ref), worst)
                want = fold(want, got[i], E)
            assert np.array_equal(tot, want), (Mv, Z, E)
            sides[0] |= bool((got > 1.0).any())
            sides[1] |= bool((got < 1.0).any())
    assert all(sides)
    print(f"N={n} Fs={fs}: largest error / bound {worst[0]:.4f}")
    eng.close()


# 2 ---------------------------------------------------------------------------------------------------------------
def guarded(eng, a):
    g = np.full(PAD + a.size + PAD, -777.0)
    g[PAD:-PAD] = a.ravel()
    d = eng.to_device(g)
    return d, d.ptr.value + PAD * 8


def unguard(d, shape):
    n = int(np.prod(shape))
    g = d.download((PAD + n + PAD,), np.float64)
    assert np.all(g[:PAD] == -777.0) and np.all(g[-PAD:] == -777.0)
    return g[PAD:-PAD].reshape(shape).copy()


@pytest.mark.parametrize("n,fs,Mv,Z,E", [(136, 16000, 17, 2, 3), (96, 48000, 5, 1, 1), (192, 3000, 33, 2, 1)])
def test_bits_do_not_depend_on_the_launch(n, fs, Mv, Z, E):
    """five hops as one call = as 2 + 3 = as 5 x 1 = as one call in sub-launches of 2 and of 1; guard words around both outputs"""
    from ap_vast_unofficial_amd._capi import Engine
    tb = tables(n, fs)
    eng = Engine(9, 4, 4)
    K, hops, items = n // 2 + 1, len(RATIOS), Z * 2 * E * Mv
    rng = np.random.default_rng(n + Mv)
    spec = hops_of(rng, K, Z, E, Mv, n)
    start = rng.random((Z, 6 * E, Mv))
    G2 = np.ascontiguousarray(tb.G2)

    def run(parts, per=None):
        dh, ph = guarded(eng, np.full(hops * items, -1.0))
        dt, pt = guarded(eng, start)
        t0 = 0
        for c in parts:
            ds = eng.to_device(np.ascontiguousarray(spec[t0:t0 + c]))
            eng._chk(eng.lib.apv_eval_detect_hops(eng.h, ds.ptr, c, per or c, n, Z, E, Mv, G2.shape[1],
                                                  G2.ctypes.data_as(ctypes.c_void_p), tb.Cs, tb.Ca, tb.Leff,
                                                  ctypes.c_void_p(ph + 8 * t0 * items), ctypes.c_void_p(pt)))
            ds.free()
            t0 += c
        out = unguard(dh, (hops, Z, 2 * E, Mv)), unguard(dt, start.shape)
        dh.free()
        dt.free()
        return out

    rec, tot = run([5])
    assert np.all(rec > 0.0) and not np.array_equal(tot, start)
    for parts, per in (([2, 3], None), ([1] * 5, None), ([5], 2), ([5], 1), ([3, 2], 2), ([5], 7)):
        r2, t2 = run(parts, per)
        assert np.array_equal(r2, rec), (parts, per)
        assert np.array_equal(t2, tot), (parts, per)
    # and the wrapper, on buffers of its own
    r3, t3 = eng.eval_detect_hops(spec, tb, Z, E, totals=start, hops_per_launch=2)
    assert np.array_equal(r3, rec) and np.array_equal(t3, tot)
    eng.close()


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,fs,c", SIZES)
def test_bits_of_the_per_hop_kernels(n, h, fs, c):
    """hop by hop, apv_eval_detect_step on the same spectra: the same hop values and the same running totals"""
    from ap_vast_unofficial_amd._capi import Engine
    tb = tables(n, fs)
    eng = Engine(9, 4, 4)
    K = n // 2 + 1
    for Mv, (Z, E) in zip(MVS, ZE + ZE[:1]):
        rng = np.random.default_rng(7 * n + Mv)
        spec = hops_of(rng, K, Z, E, Mv, n)
        start = rng.random((Z, 6 * E, Mv))
        rec, tot = eng.eval_detect_hops(spec, tb, Z, E, totals=start)
        step_tot, one_tot = start, start
        for i in range(len(RATIOS)):
            hopv, step_tot = eng.eval_detect_step(spec[i], tb, step_tot, Z, E)
            assert np.array_equal(rec[i], hopv), (Mv, Z, E, i)
            one, one_tot = eng.eval_detect_hops(spec[i:i + 1], tb, Z, E, totals=one_tot)
            assert np.array_equal(one[0], hopv) and np.array_equal(one_tot, step_tot), (Mv, Z, E, i)
        assert np.array_equal(tot, step_tot), (Mv, Z, E)
    eng.close()


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,fs,c", SIZES[:2])
def test_one_program_leaks_against_the_threshold_in_quiet(n, h, fs, c):
    from ap_vast_unofficial_amd._capi import Engine
    tb = tables(n, fs)
    eng = Engine(9, 4, 4)
    K, E, Mv, worst = n // 2 + 1, 3, 17, [0.0]
    spec = np.stack([random_spectra(np.random.default_rng(n + i), K, 1, E, Mv, n, 1e-4) for i in range(3)])
    got, _ = eng.eval_detect_hops(spec, tb, 1, E, hops_per_launch=2)
    quiet_curve = do.curve(tb, None, n)
    for i in range(3):
        _, Dk, _ = do.split(spec[i], 1, E)
        quiet = do.detectability(quiet_curve, Dk, n)          # (1, E, Mv)
        within(got[i][:, E:], quiet, do.bound_given(K, c, quiet), worst)
    print(f"N={n} Fs={fs}: one program, largest error / bound {worst[0]:.4f}")
    eng.close()


# 5 ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone():
    from ap_vast_unofficial_amd import _capi
    n, fs = 96, 48000
    tb = tables(n, fs)
    K, C = tb.G2.shape
    G2 = np.ascontiguousarray(tb.G2)
    g2 = G2.ctypes.data_as(ctypes.c_void_p)
    eng = _capi.Engine(9, 4, 4)
    Z, E, Mv, hops = 2, 1, 3, 2
    h0, t0 = np.full((hops, Z, 2, Mv), -3.0), np.full((Z, 6, Mv), 0.25)
    ds, dh, dt = eng.to_device(np.zeros((hops, K, Z * 3, Mv, 2))), eng.to_device(h0), eng.to_device(t0)
    f = eng.lib.apv_eval_detect_hops
    good = [ds.ptr, hops, hops, n, Z, E, Mv, C, g2, tb.Cs, tb.Ca, tb.Leff, dh.ptr, dt.ptr]
    for i, v in ((0, None), (8, None), (12, None), (13, None), (1, 0), (2, 0), (2, -1), (3, 0), (3, n + 1), (4, 0), (4, 3), (4, 4),
                 (5, 0), (6, 0), (7, 0), (7, 513), (10, 0.0), (10, -1.0), (9, np.nan), (11, np.inf), (3, 2 * 8192)):
        bad = list(good)
        bad[i] = v
        assert f(eng.h, *bad) == _capi.ERR_ARG, (i, v)
        assert np.array_equal(dh.download(h0.shape, np.float64), h0), (i, v)
        assert np.array_equal(dt.download(t0.shape, np.float64), t0), (i, v)
    # the good call: zero spectra give D = 0 in every slot, a sum that stays, a maximum that stays, no audible hop
    assert f(eng.h, *good) == _capi.OK
    assert not dh.download(h0.shape, np.float64).any()
    assert np.array_equal(dt.download(t0.shape, np.float64), t0)
    with pytest.raises(ValueError):
        eng.eval_detect_hops(np.zeros((K, Z * 3, Mv), dtype=complex), tb, Z, E)              # no hop axis
    with pytest.raises(ValueError):
        eng.eval_detect_hops(np.zeros((2, K, Z * 3 + 1, Mv), dtype=complex), tb, Z, E)
    with pytest.raises(ValueError):
        eng.eval_detect_hops(np.zeros((2, K, Z * 3, Mv), dtype=complex), tb, Z, E, totals=np.zeros((Z, 6, Mv + 1)))
    for d in (ds, dh, dt):
        d.free()
    eng.close()
