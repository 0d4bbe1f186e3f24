"""Detectability stage of the subband stream (apvast(..., evaluation_detectability=True), apv_stream_set_evaluation_detectability,
apv_eval_detect_step, csrc/kernels_evaldetect.hip) against the NumPy restatement of tests/detectability_oracle.py, which also
derives the two bounds: 2 (2 K + C + 16) u D on given spectra, and that plus the first-order propagation of the transform's
error on spectra the device formed from pressures.  Every test asserts that its bound is below 1e-10 of the reference value, so
the bound cannot hide a failure.  The stream tests feed the helper with the device's own per-hop predicted_pressure()."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import detectability_oracle as do  # noqa: E402
from eval_spectra_oracle import stack_sets  # noqa: E402
from test_gpu_stat_window import hop, same_outputs  # noqa: E402
from test_gpu_stream import synth_rirs  # noqa: E402
from test_gpu_stream_evaluation import validation_rirs  # noqa: E402

# block, hop, sampling rate, channels of the model: the smallest blocks the tables calibrate at.  (96, 24) a smooth transform;
# (136, 40) Bluestein, H does not divide N, the ring wraps; (96, 32, 14 kHz) C a full tile of 32; (192, 96) K = 97
SIZES = [(96, 24, 48000, 44), (136, 40, 16000, 34), (96, 32, 14000, 32), (192, 96, 3000, 19)]
MVS = [1, 5, 16, 17, 33]
ZE = [(1, 1), (2, 3), (2, 1), (1, 3), (2, 3)]
L, M, V = 4, 4, 3
DELAY, REF_A, REF_B = 3, 1, 2


def tables_of(n, fs):
    from ap_vast_unofficial_amd.perceptual import PerceptualTables
    return PerceptualTables(n, fs, 94.0)


def random_spectra(rng, K, Z, E, Mv, n, ratio):
    """bin-major spectra (K, Z (2 E + 1), Mv): targets of about unit pressure, bright = target - ratio x noise, dark = ratio x noise"""
    g = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)) * n
    spec = np.empty((K, Z, 2 * E + 1, Mv), dtype=np.complex128)
    spec[:, :, 2 * E] = g(K, Z, Mv)
    spec[:, :, :E] = spec[:, :, 2 * E][:, :, None] - ratio * g(K, Z, E, Mv)
    spec[:, :, E:2 * E] = ratio * g(K, Z, E, Mv)
    return spec.reshape(K, Z * (2 * E + 1), Mv)


def reference_hop(tb, spec, Z, E, n):
    B, Dk, T = do.split(spec, Z, E)
    err, leak, _, _ = do.reference(tb, B, Dk, T, n)
    return np.concatenate([err, leak], axis=1)                # (Z, 2 E, Mv), the device's slot


def fold(tot, hopv, E):
    """the totals (Z, 6 E, Mv) one hop later, in the device's arithmetic"""
    Z, _, Mv = hopv.shape
    t, h = tot.reshape(Z, 2, 3, E, Mv).copy(), hopv.reshape(Z, 2, E, Mv)
    t[:, :, 0] = t[:, :, 0] + h
    t[:, :, 1] = np.maximum(t[:, :, 1], h)
    t[:, :, 2] = t[:, :, 2] + (h > 1.0)
    return t.reshape(Z, 6 * E, Mv)


def within(got, ref, bound, worst):
    assert got.shape == ref.shape
    assert np.all(ref > 0) and np.all(bound < 1e-10 * ref)
    err = np.abs(got - ref)
    worst[0] = max(worst[0], float((err / bound).max()))
    assert np.all(err <= bound), worst


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,fs,c", SIZES)
def test_kernel_against_helper(n, h, fs, c):
    """three steps on random spectra at every Mv; the last case again on guard-padded buffers"""
    from ap_vast_unofficial_amd._capi import Engine
    tb = tables_of(n, fs)
    assert tb.n_channels == c
    eng = Engine(9, 4, 4)
    K, worst, sides = n // 2 + 1, [0.0], [False, False]
    for Mv, (Z, E) in zip(MVS, ZE):
        rng = np.random.default_rng(100 * n + Mv)
        tot = np.zeros((Z, 6 * E, Mv))
        for ratio in (0.3, 0.05, 0.01):
            spec = random_spectra(rng, K, Z, E, Mv, n, ratio)
            got, new = eng.eval_detect_step(spec, tb, tot, Z, E)
            ref = reference_hop(tb, spec, Z, E, n)
            within(got, ref, do.bound_given(K, c, ref), worst)
            # the totals follow from the entry's own per-hop values, bit for bit
            assert np.array_equal(new, fold(tot, got, E)), (Mv, ratio)
            sides[0] |= bool((got > 1.0).any())
            sides[1] |= bool((got < 1.0).any())
            tot = new
    assert all(sides)
    # canaries in front of and behind the hop's slot and the totals: the same bits, nothing outside touched
    pad = 64
    gh, gt = np.full(pad + got.size + pad, -777.0), np.full(pad + tot.size + pad, -777.0)
    gt[pad:-pad] = 0.0
    dh, dt, ds = eng.to_device(gh), eng.to_device(gt), eng.to_device(spec)
    G2 = np.ascontiguousarray(tb.G2)
    inner = lambda d: ctypes.c_void_p(d.ptr.value + pad * 8)
    eng._chk(eng.lib.apv_eval_detect_step(eng.h, ds.ptr, n, Z, E, Mv, c, G2.ctypes.data_as(ctypes.c_void_p), tb.Cs, tb.Ca, tb.Leff,
                                          inner(dh), inner(dt)))
    bh, bt = dh.download(gh.shape, np.float64), dt.download(gt.shape, np.float64)
    for b in (bh, bt):
        assert np.all(b[:pad] == -777.0) and np.all(b[-pad:] == -777.0)
    assert np.array_equal(bh[pad:-pad].reshape(got.shape), got)
    assert np.array_equal(bt[pad:-pad].reshape(tot.shape), fold(np.zeros_like(tot), got, E))
    for d in (dh, dt, ds):
        d.free()
    print(f"N={n} Fs={fs}: largest error / bound {worst[0]:.4f}")
    eng.close()


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,fs,c", SIZES)
def test_known_answer_calibration_identity(n, h, fs, c):
    """a 52 dB SPL probe on a 70 dB SPL masker at the calibration bin is just detectable: error = 1 to the 1e-4 the bisection of
    the tables leaves (test_perceptual_tables_calibration in tests/test_cpu_host.py holds the same identity to it); with a zero
    target, the threshold in quiet"""
    from ap_vast_unofficial_amd._capi import Engine
    from oracle.perceptual import Model
    tb, m = tables_of(n, fs), Model(n, fs)
    K, f, cal = n // 2 + 1, 2.0 / (n * n), m.cal_bin
    assert cal >= 1
    eng = Engine(9, 4, 4)
    Z, E, Mv = 1, 1, 3
    spec = np.zeros((K, 3, Mv), dtype=np.complex128)
    spec[cal, 2] = m.S70 / np.sqrt(f)
    spec[cal, 0] = spec[cal, 2] - m.S52 / np.sqrt(f) * np.exp(1j * np.array([0.0, 1.0, 2.5]))     # any phase
    got, _ = eng.eval_detect_step(spec, tb, np.zeros((Z, 6 * E, Mv)), Z, E)
    print(f"N={n} Fs={fs}: calibration identity, error - 1 = {np.abs(got[0, 0] - 1).max():.2e}")
    assert np.all(np.abs(got[0, 0] - 1.0) < 1e-4)
    assert np.all(got[0, 1] == 0.0)                           # no dark pressure: no leak
    spec[cal, 2] = 0.0
    spec[cal, 0] = -m.S52 / np.sqrt(f)
    got, _ = eng.eval_detect_step(spec, tb, np.zeros((Z, 6 * E, Mv)), Z, E)
    exp = float(np.asarray(do.curve(tb, None, n), dtype=np.float64)[cal] * m.S52 ** 2)
    assert do.bound_given(K, c, exp) < 1e-10 * exp
    print(f"N={n} Fs={fs}: threshold in quiet, largest error / bound {np.abs(got[0, 0] - exp).max() / do.bound_given(K, c, exp):.4f}")
    assert np.all(np.abs(got[0, 0] - exp) <= do.bound_given(K, c, exp))
    eng.close()


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,fs,c", SIZES[:2])
def test_one_program_leaks_against_the_threshold_in_quiet(n, h, fs, c):
    from ap_vast_unofficial_amd._capi import Engine
    tb = tables_of(n, fs)
    eng = Engine(9, 4, 4)
    K, E, Mv, worst = n // 2 + 1, 3, 17, [0.0]
    rng = np.random.default_rng(n)
    one = random_spectra(rng, K, 1, E, Mv, n, 1e-4)
    got1, _ = eng.eval_detect_step(one, tb, np.zeros((1, 6 * E, Mv)), 1, E)
    _, Dk, _ = do.split(one, 1, E)
    quiet = do.detectability(do.curve(tb, None, n), Dk, n)    # (1, E, Mv)
    within(got1[:, E:], quiet, do.bound_given(K, c, quiet), worst)
    # two programs, the second one's input silent: its target spectrum is zero, and program 0 leaks against the same curve
    two = np.zeros((K, 2, 2 * E + 1, Mv), dtype=np.complex128)
    two[:, 0] = one.reshape(K, 2 * E + 1, Mv)
    got2, _ = eng.eval_detect_step(two.reshape(K, 2 * (2 * E + 1), Mv), tb, np.zeros((2, 6 * E, Mv)), 2, E)
    within(got2[:1, E:], quiet, do.bound_given(K, c, quiet), worst)
    # (two device results, each within the bound of the exact value: the split of the bins over workgroups depends on Z)
    within(got2[:1, :E], got1[:, :E], 2 * do.bound_given(K, c, got1[:, :E]), worst)
    assert np.all(got2[1] == 0.0)
    print(f"N={n} Fs={fs}: one program, largest error / bound {worst[0]:.4f}")
    eng.close()


# 4 ---------------------------------------------------------------------------------------------------------------
def make(n, h, fs, dtype="f64", synth="wola", perceptual=False, run_A=True, run_B=True, Pv=9, Mv=5, ranks=None, P=12, detect=True,
         **kw):
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(P, L, M, 1)
    if synth != "wola":
        kw.update(constrain_filter_length=True, synthesis="fir" if synth == "fir" else "wola")
    rvA, rvB = validation_rirs(Pv, L, Mv)
    if detect is not None:
        kw.update(evaluation_detectability=detect)
    return apvast(n, rirA, rirB, 8, DELAY, REF_A, REF_B, V, 1.0, 4 * n, hop_size=h, sampling_rate=fs, run_A=run_A, run_B=run_B,
                  perceptual=perceptual, seed=0, dtype=dtype, validation_rir_A=rvA, validation_rir_B=rvB, evaluation_ranks=ranks,
                  evaluation_spectra=True, **kw)


def ramp_signal(hops, h, seed=99):
    """white noise rising from far below the threshold in quiet to full scale, so that inaudible and audible hops both occur"""
    x = np.random.default_rng(seed).standard_normal((2, hops * h))
    return x * np.repeat(10.0 ** np.linspace(-7.0, 0.0, hops), h)


CASES = [("f64", "wola", False, True, True, 5, None, 9), ("mixed", "constrained", True, True, False, 17, [2], 20),
         ("f32", "fir", True, True, True, 1, [1, 2, 3], 8), ("f64", "fir", False, False, True, 33, [2], 12),
         ("f32", "wola", True, True, True, 16, [1], 15)]


@pytest.mark.parametrize("dtype,synth,perceptual,run_A,run_B,Mv,ranks,Pv", CASES)
@pytest.mark.parametrize("n,h,fs,c", SIZES)
def test_stream_against_helper(n, h, fs, c, dtype, synth, perceptual, run_A, run_B, Mv, ranks, Pv):
    from ap_vast_unofficial_amd.evaluation import detectability_metrics
    from oracle.perceptual import Model
    Z, E, hops = int(run_A) + int(run_B), V if ranks is None else len(ranks), 8
    ap = make(n, h, fs, dtype, synth, perceptual, run_A, run_B, Pv, Mv, ranks)
    tb = ap.detectability_model
    assert tb.n_channels == c and (not perceptual or ap.model is tb)
    assert ap.evaluation_detectability() is None and ap.evaluation_detectability_hops() is None
    ref, other = do.StreamReference(tb, n, h, Z, E, Mv), do.StreamReference(do.from_model(Model(n, fs)), n, h, Z, E, Mv)
    x = ramp_signal(hops, h)
    worst, tot = [0.0], np.zeros((Z, 6 * E, Mv))
    sides = {"error": [False, False], "leak": [False, False]}
    for k in range(hops):
        hop(ap, x, k, h)
        p = stack_sets(ap.predicted_pressure())
        want, bound = ref.hop(p)
        cross, _ = other.hop(p)
        got = ap.evaluation_detectability_hops()
        for key in ("error", "leak"):
            assert got[key].shape == (1, Z, E, Mv)
            within(got[key][0], want[key], bound[key], worst)
            assert np.all(np.abs(got[key][0] - cross[key]) <= 4e-6 * cross[key]), key
            sides[key][0] |= bool((got[key] > 1.0).any())
            sides[key][1] |= bool((got[key] < 1.0).any())
        tot = fold(tot, np.concatenate([got["error"][0], got["leak"][0]], axis=1), E)
    assert all(sides["error"]) and all(sides["leak"]), sides
    t = ap.evaluation_detectability()
    assert t["hops"] == hops and t["error_audible"].dtype == np.int64
    dev = tot.reshape(Z, 2, 3, E, Mv)
    for i, key in enumerate(("error", "leak")):
        assert np.array_equal(t[key], dev[:, i, 0]) and np.array_equal(t[key + "_max"], dev[:, i, 1])
        assert np.array_equal(t[key + "_audible"], dev[:, i, 2].astype(np.int64))
    met = detectability_metrics(t)
    assert met["error_mean"].shape == (Z, E) and np.all(met["leak_audible_share"] <= 1.0)
    print(f"N={n} Fs={fs} {dtype} {synth} perceptual={perceptual}: largest error / bound {worst[0]:.4f}")
    ap.close()


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,fs,c", SIZES[:2])
@pytest.mark.parametrize("dtype,synth", [("f64", "wola"), ("f32", "fir")])
def test_call_forms_agree(n, h, fs, c, dtype, synth):
    hops = 8
    a, b = make(n, h, fs, dtype, synth), make(n, h, fs, dtype, synth)
    x = ramp_signal(hops, h)
    rec = {"error": [], "leak": []}
    for k in range(hops):
        hop(a, x, k, h)
        r = a.evaluation_detectability_hops()
        for key in rec:
            rec[key].append(r[key][0])
    b.process_signal(x[0], x[1])
    assert b.signal_schedule == (0, hops)
    rb, ta, tb = b.evaluation_detectability_hops(), a.evaluation_detectability(), b.evaluation_detectability()
    for key in rec:
        assert np.array_equal(rb[key], np.stack(rec[key])), key
    assert sorted(ta) == sorted(tb) == ["error", "error_audible", "error_max", "hops", "leak", "leak_audible", "leak_max"]
    for key in ta:
        assert np.array_equal(ta[key], tb[key]), key
    a.close()
    b.close()


# 6 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,fs,c", SIZES[:2])
def test_state_resume_and_reset(n, h, fs, c):
    Z, E, Mv = 2, 2, 5
    kw = dict(ranks=[1, 3], Mv=Mv)
    a, b, plain = make(n, h, fs, **kw), make(n, h, fs, **kw), make(n, h, fs, detect=None, **kw)
    x = ramp_signal(8, h)
    for k in range(8):
        hop(a, x, k, h)
        if k == 4:
            st = a.get_state()
            assert st["evaluation_detectability"].shape == (Z, 6 * E + 1, Mv) and np.all(st["evaluation_detectability"][:, -1] == 5)
            assert sorted(set(st) - set(plain.get_state())) == ["evaluation_detectability"]
            b.set_state(st)
    for k in range(5, 8):
        hop(b, x, k, h)
    ta, tb = a.evaluation_detectability(), b.evaluation_detectability()
    assert ta["hops"] == tb["hops"] == 8
    for key in ta:
        assert np.array_equal(ta[key], tb[key]), key
    ha, hb = a.evaluation_detectability_hops(), b.evaluation_detectability_hops()
    for key in ha:
        assert np.array_equal(ha[key], hb[key]), key
    assert np.array_equal(a.get_state()["evaluation_detectability"], b.get_state()["evaluation_detectability"])
    # reset: the next hop's totals are its own values
    a.reset_evaluation()
    assert not a.get_state()["evaluation_detectability"].any()
    hop(a, x, 7, h)
    t, r = a.evaluation_detectability(), a.evaluation_detectability_hops()
    assert t["hops"] == 1
    for key in ("error", "leak"):
        assert np.array_equal(t[key], r[key][0]) and np.array_equal(t[key + "_max"], r[key][0])
        assert np.array_equal(t[key + "_audible"], (r[key][0] > 1.0).astype(np.int64))
    for bad in (np.zeros((Z, 6 * E, Mv)), np.zeros((Z, 6 * E + 1, Mv + 1))):
        with pytest.raises(ValueError, match="evaluation_detectability"):
            b.set_state({"evaluation_detectability": bad})
    with pytest.raises(KeyError):
        plain.set_state({"evaluation_detectability": st["evaluation_detectability"]})
    for f in (plain.evaluation_detectability, plain.evaluation_detectability_hops):
        with pytest.raises(RuntimeError, match="evaluation_detectability=True"):
            f()
    for o in (a, b, plain):
        o.close()


# 7 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,perceptual", [("f64", True), ("f32", False)])
def test_nothing_else_moves(dtype, perceptual):
    """outputs, filters, eigenvalues, totals, record, spectra, pressures and signal_schedule of a stream with the keyword equal
    those of the same stream without it (keyword False, and keyword absent), six hops and a whole-signal call"""
    n, h, fs = 96, 24, 48000
    a, b, c = (make(n, h, fs, dtype, perceptual=perceptual, detect=d) for d in (True, False, None))
    x = ramp_signal(6, h)
    for k in range(6):
        oa, ob, oc = hop(a, x, k, h), hop(b, x, k, h), hop(c, x, k, h)
        same_outputs(oa, ob)
        same_outputs(oa, oc)
        for name in ("w_A", "w_B", "lambda_A", "lambda_B"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), (k, name)
        for f in ("evaluation_totals", "evaluation_hops", "predicted_pressure", "evaluation_spectra"):
            da, db = getattr(a, f)(), getattr(b, f)()
            for q in da:
                assert np.array_equal(da[q], db[q]), (k, f, q)
    sa, sb, sc = a.get_state(), b.get_state(), c.get_state()
    assert sorted(set(sa) - set(sb)) == ["evaluation_detectability"] and sorted(sb) == sorted(sc)
    for k in sb:
        assert np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])), k
    y = ramp_signal(4, h, seed=5)
    for q, r in zip(a.process_signal(y[0], y[1]), b.process_signal(y[0], y[1])):
        if q is not None:
            assert np.array_equal(np.stack(q), np.stack(r))
    assert a.signal_schedule == b.signal_schedule == (0, 4)
    for o in (a, b, c):
        o.close()


# 8 ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    from ap_vast_unofficial_amd import _capi
    n, fs = 96, 48000
    tb = tables_of(n, fs)
    K, C = tb.G2.shape
    G2 = np.ascontiguousarray(tb.G2)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rv = np.ones((5, L, 2))
    eng = _capi.Engine(K, L, M, ranks=[1, 2], block_size=n, hop_size=24, n_zones=3)
    setter = eng.lib.apv_stream_set_evaluation_detectability
    nan, inf = np.array(G2), np.array(G2)
    nan[3, 1], inf[K - 1, C - 1] = np.nan, np.inf
    for args in ((C, None, tb.Cs, tb.Ca, tb.Leff), (C, ptr(nan), tb.Cs, tb.Ca, tb.Leff), (C, ptr(inf), tb.Cs, tb.Ca, tb.Leff),
                 (C, ptr(G2), tb.Cs, 0.0, tb.Leff), (C, ptr(G2), tb.Cs, -1.0, tb.Leff), (C, ptr(G2), np.nan, tb.Ca, tb.Leff),
                 (C, ptr(G2), tb.Cs, tb.Ca, np.inf), (-1, ptr(G2), tb.Cs, tb.Ca, tb.Leff), (513, ptr(G2), tb.Cs, tb.Ca, tb.Leff)):
        assert setter(eng.h, *args) == _capi.ERR_ARG, args
    rirA, rirB = (np.ascontiguousarray(r, dtype=np.float64) for r in synth_rirs(12, L, M, 1))
    # on without the spectra stage: stream_init refuses; off again: it goes through
    eng.set_evaluation(rv, rv, [1, 2])
    eng.set_evaluation_detectability(tb)
    with pytest.raises(_capi.ApvError, match="needs the per-bin spectra"):
        eng.stream_init(rirA, rirB, REF_A, REF_B, DELAY)
    eng.set_evaluation_detectability(None)
    eng.stream_init(rirA, rirB, REF_A, REF_B, DELAY)
    assert setter(eng.h, C, ptr(G2), tb.Cs, tb.Ca, tb.Leff) == _capi.ERR_ARG           # after init
    with pytest.raises(_capi.ApvError):
        eng.state_bytes("eval_detect")
    # the entry: null pointers, sizes below 1, odd N, Z > 2
    step = eng.lib.apv_eval_detect_step
    Z, E, Mv = 2, 1, 3
    ds, dh, dt = (eng.to_device(np.zeros(s)) for s in ((K, Z * 3, Mv, 2), (Z, 2, Mv), (Z, 6, Mv)))
    good = [ds.ptr, n, Z, E, Mv, C, ptr(G2), tb.Cs, tb.Ca, tb.Leff, dh.ptr, dt.ptr]
    assert step(eng.h, *good) == _capi.OK
    for i, v in ((0, None), (6, None), (10, None), (11, None), (1, 0), (1, n + 1), (2, 0), (2, 3), (3, 0), (4, 0), (5, 0), (5, 513),
                 (8, 0.0), (7, np.nan)):
        bad = list(good)
        bad[i] = v
        assert step(eng.h, *bad) == _capi.ERR_ARG, (i, v)
    assert not dt.download((Z, 6, Mv), np.float64).any()     # zero spectra: D = 0, and the refused calls left it alone
    for d in (ds, dh, dt):
        d.free()
    eng.close()
